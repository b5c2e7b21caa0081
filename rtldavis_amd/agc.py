"""Gain control for ``wideband.WidebandReceiver``: the host policy on top of the device mechanism.

The receiver meters every chunk (``set_levels`` / ``levels()``) and switches per-channel gains at a chunk boundary
(``set_gain``); what to set is decided here, between chunks, as ``retune`` leaves the averaging of frequency errors to
the caller::

    rx.set_levels(True)
    agc = GainControl(rx.n_channels, rx.block_size)
    rx.set_gain(agc.gains())
    ...
    packets = rx.fetch()
    new = agc.update(rx.levels())
    if new is not None:
        rx.set_gain(new)

Pure Python on exact integers: the same level records give the same gains, on any machine; nothing here touches a device.
"""
from __future__ import annotations

from typing import Optional

import numpy as np


class GainControl:
    """One gain-table index and one quiet counter per channel.

    The table is fixed: ``G[i] = float32(min_gain * 10 ** (i * step_db / 20))`` for every i with ``G[i] <= max_gain``.
    ``update(levels)`` applies, per channel, to the chunk's record (``power`` = sum a^2 and ``clipped`` over the channel's
    ``2 * block_size`` bytes, a = 2 b - 255):

    - ``clipped > clip_max`` or ``power > high_power``: one step down, the quiet counter to 0;
    - else ``clipped == 0`` and ``power < low_power``: the quiet counter + 1; when it reaches ``hold``, one step up and
      the counter to 0;
    - else: the counter to 0, the index stays.

    At either end of the table the index stays.  All comparisons are between integers.

    It steers on POWER, i.e. on the noise floor, not on the bursts: a Davis transmitter visits a channel once in about
    130 s, for 4 ms, so a chunk almost always holds noise only, and a loop that waited for bursts would never settle.
    The gain has to sit where the noise occupies a few quantiser steps - below one step the demodulator sees a constant
    and a weak burst is lost - and a burst has headroom above it; a strong burst that clips is tolerated, FM carries its
    information in the zero crossings.

    Defaults, with N = 2 * block_size components per chunk and sigma the noise's standard deviation per component in
    byte steps (a = 2 (b - 127.5), so the mean of a^2 is 4 sigma^2 + 1 with the quantiser's own quarter step):

    - ``low_power = 9 N``: sigma below about 1.4 steps - step up;
    - ``high_power = 144 N``: sigma above about 6 steps, 26 dB under full scale - step down.  The window is 12 dB wide
      against ``step_db = 3`` (a step doubles the power): a step never carries a channel across it, the loop cannot hunt;
    - ``clip_max = N // 4``: a single burst that clips through its 4 ms inside a chunk of 8192 outputs (30 ms) clips a
      seventh of the bytes and moves nothing; a quarter means the channel is overdriven for most of the chunk;
    - ``hold = 4`` quiet chunks before a step up, one loud chunk for a step down: clipping loses information, a gain
      that is low for a few chunks longer does not;
    - ``min_gain = 0.25``, ``max_gain = 512``: 66 dB, the 96 dB of an int16 capture less the 48 dB of a byte, and room
      beyond the gain of 300 the weak default-plan capture needs; ``start_gain = 3``, the receivers' constructed default.
    """

    def __init__(self, n_channels: int, block_size: int, *, min_gain: float = 0.25, max_gain: float = 512.0,
                 step_db: float = 3.0, start_gain: float = 3.0, low_power: Optional[int] = None,
                 high_power: Optional[int] = None, clip_max: Optional[int] = None, hold: int = 4) -> None:
        n = 2 * int(block_size)
        if int(n_channels) < 1 or n < 2:
            raise ValueError("n_channels and block_size must be positive")
        if not (0.0 < float(min_gain) <= float(max_gain)) or not float(step_db) > 0.0 or int(hold) < 1:
            raise ValueError("0 < min_gain <= max_gain, step_db > 0 and hold >= 1")
        table, i = [], 0
        while True:
            g = np.float32(float(min_gain) * 10.0 ** (i * float(step_db) / 20.0))
            if not np.isfinite(g) or float(g) > float(max_gain):
                break
            table.append(g)
            i += 1
        if not table:
            raise ValueError("the gain table is empty")
        self.table = np.asarray(table, np.float32)
        self.low_power = 9 * n if low_power is None else int(low_power)
        self.high_power = 144 * n if high_power is None else int(high_power)
        self.clip_max = n // 4 if clip_max is None else int(clip_max)
        self.hold = int(hold)
        if self.low_power > self.high_power:
            raise ValueError("low_power above high_power")
        # the largest entry not above start_gain (the first one if there is none)
        start = max(0, int(np.searchsorted(self.table, np.float32(start_gain), side="right")) - 1)
        self.index = [start] * int(n_channels)
        self.quiet = [0] * int(n_channels)

    def gains(self) -> np.ndarray:
        """float32 per channel: the table entries of the indices in force."""
        return self.table[self.index]

    def update(self, levels) -> Optional[np.ndarray]:
        """One chunk's level records (``WidebandReceiver.levels()``, or its ``channels`` array, or any sequence of rows
        with ``power`` and ``clipped``) -> the gains to set (float32 per channel), or None when no index moved."""
        rows = getattr(levels, "channels", levels)
        if len(rows) != len(self.index):
            raise ValueError(f"{len(rows)} level records for {len(self.index)} channels")
        top, changed = len(self.table) - 1, False
        for c, row in enumerate(rows):
            power, clipped = int(row["power"]), int(row["clipped"])
            if clipped > self.clip_max or power > self.high_power:
                self.quiet[c] = 0
                if self.index[c] > 0:
                    self.index[c] -= 1
                    changed = True
            elif clipped == 0 and power < self.low_power:
                self.quiet[c] += 1
                if self.quiet[c] >= self.hold:
                    self.quiet[c] = 0
                    if self.index[c] < top:
                        self.index[c] += 1
                        changed = True
            else:
                self.quiet[c] = 0
        return self.gains() if changed else None
