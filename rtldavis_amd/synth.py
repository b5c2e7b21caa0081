"""Canonical synthetic Davis IQ streams.

Synthetic data only: the reference tree holds no recorded IQ.  The five
payloads are the CRC-valid on-air packets found in the reference's own tests
(tests/test_protocol.py:29, debug_tools/test_tx.py:37,
decoders/temperature_test.py:15, decoders/humidity_test.py:15,20), in the
on-air bit order ``Demodulator._slice`` emits (src/rtldavis/dsp.py:197-200).
"""
from __future__ import annotations

import numpy as np

BLOCK_SIZE = 8192
BLOCKS_PER_STREAM = 33
STREAM_SAMPLES = BLOCK_SIZE * BLOCKS_PER_STREAM  # 270336 complex samples = 1.0057 s
SAMPLE_RATE = 19200 * 14
SYMBOL_LENGTH = 14

OTA_PACKETS = (
    "cb8907c02b0b80408eff",
    "cb8981a0b1ccd3f08fbb",
    "cb8901a034349fd02679",
    "cb8905604ac11c005a13",
    "cb890520ac8bd4000e5c",
)


def packet_bits(ota_hex: str) -> np.ndarray:
    """MSB-first bits of a 10-byte on-air packet."""
    return np.unpackbits(np.frombuffer(bytes.fromhex(ota_hex), dtype=np.uint8))


def synth_stream(seed: int, n_samples: int = STREAM_SAMPLES,
                 amplitude: float = 0.5, noise: float = 0.05,
                 start: int | None = None, symbol_length: int = SYMBOL_LENGTH,
                 margin: int = BLOCK_SIZE) -> np.ndarray:
    """One stream of uint8 interleaved IQ (length 2*n_samples) holding one burst.

    The burst sits at -Fs/4 (+cfo) in the raw IQ because the reference's
    Fs/4 rotation (dsp.py:42-49) moves that frequency to DC.  Bit 1 is the
    +4800 Hz deviation (negative discriminator output, dsp.py:88-98).
    Draw order from the generator: payload, start, cfo, noise-real, noise-imag.
    ``start`` overrides the drawn burst position (the draw still happens, so
    the noise is unchanged); ``symbol_length`` changes samples per symbol (the
    sample rate follows, 19200 * symbol_length); ``margin`` is the burst-free
    guard at both ends.
    """
    sample_rate = 19200 * symbol_length
    rng = np.random.default_rng(seed)
    payload = OTA_PACKETS[int(rng.integers(0, len(OTA_PACKETS)))]
    sym = np.concatenate([
        np.tile(np.array([1, 0], dtype=np.uint8), 16),
        packet_bits(payload),
        np.zeros(8, dtype=np.uint8),
    ])
    chips = np.repeat(sym, symbol_length)
    drawn = int(rng.integers(margin, n_samples - chips.size - margin))
    start = drawn if start is None else int(start)
    cfo = float(rng.uniform(-2000.0, 2000.0))
    freq = np.full(n_samples, -sample_rate / 4.0 + cfo)
    on = np.zeros(n_samples)
    on[start:start + chips.size] = 1.0
    freq[start:start + chips.size] += np.where(chips == 1, 4800.0, -4800.0)
    phase = np.cumsum(freq) * (2.0 * np.pi / sample_rate)
    x = amplitude * on * np.exp(1j * phase)
    x = x + noise * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples))
    out = np.empty(2 * n_samples, dtype=np.uint8)
    out[0::2] = np.clip(np.rint(x.real * 127.6 + 127.4), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(x.imag * 127.6 + 127.4), 0, 255).astype(np.uint8)
    return out


def synth_two_bursts(seed: int, gap: int, n_samples: int = 4 * BLOCK_SIZE, amplitude: float = 0.5,
                      noise: float = 0.05) -> np.ndarray:
    """Two identical bursts `gap` samples apart (start to start) in one stream: both land in the
    same demodulate() window, so the per-call dedupe (dsp.py:203-205) has real work to do."""
    rng = np.random.default_rng(seed)
    payload = OTA_PACKETS[int(rng.integers(0, len(OTA_PACKETS)))]
    sym = np.concatenate([np.tile(np.array([1, 0], dtype=np.uint8), 16), packet_bits(payload),
                          np.zeros(8, dtype=np.uint8)])
    chips = np.repeat(sym, SYMBOL_LENGTH)
    start = BLOCK_SIZE + int(rng.integers(0, 2000))
    cfo = float(rng.uniform(-2000.0, 2000.0))
    freq = np.full(n_samples, -SAMPLE_RATE / 4.0 + cfo)
    on = np.zeros(n_samples)
    for s0 in (start, start + gap):
        on[s0:s0 + chips.size] = 1.0
        freq[s0:s0 + chips.size] += np.where(chips == 1, 4800.0, -4800.0)
    phase = np.cumsum(freq) * (2.0 * np.pi / SAMPLE_RATE)
    x = amplitude * on * np.exp(1j * phase)
    x = x + noise * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples))
    out = np.empty(2 * n_samples, dtype=np.uint8)
    out[0::2] = np.clip(np.rint(x.real * 127.6 + 127.4), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(x.imag * 127.6 + 127.4), 0, 255).astype(np.uint8)
    return out


def _swap_bits8(b: int) -> int:
    return int(f"{b:08b}"[::-1], 2)


def _crc16_ccitt(data: bytes) -> int:
    """CRC-16-CCITT, polynomial 0x1021, init 0, MSB first."""
    crc = 0
    for byte in data:
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def make_packet(ident: int, body, n_bytes: int = 10, flip_bit: int | None = None) -> bytes:
    """On-air bytes of a packet of ``n_bytes`` (>= 5): the sync word cb 89, then the message with every byte
    bit-reversed.  Message: byte 0 = (body[0] & 0xF8) | ident, then body[1:], then the CRC-16-CCITT of those bytes, high
    byte first, so that the check over the whole message is 0; ``body`` has n_bytes - 4 bytes.  ``flip_bit`` flips bit
    k of the message, counted the way the CRC takes them in (0 = bit 7 of message byte 0, 8 (n_bytes - 2) - 1 = bit 0
    of the CRC's low byte): still sync-valid, never CRC-valid (a CRC detects every single-bit error)."""
    body = bytes(body)
    if n_bytes < 5 or len(body) != n_bytes - 4 or not 0 <= ident <= 7:
        raise ValueError("make_packet: body must hold n_bytes - 4 bytes, ident 0..7")
    msg = bytearray([(body[0] & 0xF8) | ident]) + bytearray(body[1:])
    crc = _crc16_ccitt(bytes(msg))
    msg += bytes([crc >> 8, crc & 0xFF])
    if flip_bit is not None:
        if not 0 <= flip_bit < 8 * len(msg):
            raise ValueError("make_packet: flip_bit outside the message")
        msg[flip_bit // 8] ^= 0x80 >> (flip_bit % 8)
    return bytes([0xCB, 0x89]) + bytes(_swap_bits8(b) for b in msg)


def synth_bursts(bursts, n_samples: int, seed: int, symbol_length: int = SYMBOL_LENGTH, amplitude: float = 0.5,
                 noise: float = 0.05) -> np.ndarray:
    """One stream of uint8 interleaved IQ (length 2*n_samples) holding the given bursts: ``bursts`` is a list of
    (on-air bytes, start sample, cfo in Hz).  Each burst is what ``synth_stream`` plants - 32 alternating symbols, the
    packet's bits MSB first, 8 zero symbols, at -Fs/4 + cfo +- 4800 Hz with continuous phase - with the same noise and
    quantisation; the generator draws only the noise (real, then imaginary).  Where two bursts overlap, the one listed
    first keeps its samples: a burst may start inside its predecessor's trailing symbols and loses that much of its own
    lead-in."""
    sample_rate = 19200 * symbol_length
    rng = np.random.default_rng(seed)
    freq = np.full(n_samples, -sample_rate / 4.0)
    on = np.zeros(n_samples)
    for ota, start, cfo in reversed(list(bursts)):
        sym = np.concatenate([
            np.tile(np.array([1, 0], dtype=np.uint8), 16),
            np.unpackbits(np.frombuffer(bytes(ota), dtype=np.uint8)),
            np.zeros(8, dtype=np.uint8),
        ])
        chips = np.repeat(sym, symbol_length)
        start = int(start)
        if start < 0 or start + chips.size > n_samples:
            raise ValueError("synth_bursts: a burst does not fit the stream")
        on[start:start + chips.size] = 1.0
        freq[start:start + chips.size] = -sample_rate / 4.0 + float(cfo) + np.where(chips == 1, 4800.0, -4800.0)
    phase = np.cumsum(freq) * (2.0 * np.pi / sample_rate)
    x = amplitude * on * np.exp(1j * phase)
    x = x + noise * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples))
    out = np.empty(2 * n_samples, dtype=np.uint8)
    out[0::2] = np.clip(np.rint(x.real * 127.6 + 127.4), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(x.imag * 127.6 + 127.4), 0, 255).astype(np.uint8)
    return out


def synth_streams(seeds, n_samples: int = STREAM_SAMPLES) -> np.ndarray:
    """Stack of streams, shape [len(seeds), 2*n_samples] uint8."""
    seeds = list(seeds)
    out = np.empty((len(seeds), 2 * n_samples), dtype=np.uint8)
    for i, s in enumerate(seeds):
        out[i] = synth_stream(s, n_samples)
    return out


def synth_wideband(seeds, shifts_hz, n_out: int, decim: int = 100, out_rate: int = SYMBOL_LENGTH * 19200,
                   amplitude: float = 0.12, noise: float = 0.02, noise_seed: int = 1234, sample_format: str = "u8",
                   payloads=None):
    """One wideband capture (I,Q interleaved, decim*out_rate samples/s, n_out*decim samples; sample_format "u8":
    uint8 rint(x 127.6 + 127.4), "s8": int8 rint(x 128), "s16": int16 rint(x 32768), clipped, of the same complex x;
    "cf32": float32 x itself, unquantised and unclipped)
    holding one burst per entry: burst i is the packet synth_stream(seeds[i]) carries, at
    shifts_hz[i] Hz from the capture's centre (+ a random cfo of +-2 kHz), starting somewhere
    between the first and the last 8192 output samples.  ``payloads`` (one on-air hex string per burst) overrides the
    drawn packets; start and cfo are drawn as before.  Returns (raw, [(payload_hex, start_out)])."""
    fw = decim * out_rate
    n = n_out * decim
    rng = np.random.default_rng(noise_seed)
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    info = []
    for k, (seed, shift) in enumerate(zip(seeds, shifts_hz)):
        r = np.random.default_rng(seed)
        payload = OTA_PACKETS[int(r.integers(0, len(OTA_PACKETS)))]
        if payloads is not None:
            payload = payloads[k]
        sym = np.concatenate([np.tile(np.array([1, 0], dtype=np.uint8), 16), packet_bits(payload),
                              np.zeros(8, dtype=np.uint8)])
        chips = np.repeat(sym, SYMBOL_LENGTH * decim)
        start_out = int(r.integers(BLOCK_SIZE, n_out - chips.size // decim - BLOCK_SIZE))
        cfo = float(r.uniform(-2000.0, 2000.0))
        lo, hi = start_out * decim, start_out * decim + chips.size
        freq = float(shift) + cfo + np.where(chips == 1, 4800.0, -4800.0)
        # phase of the tone from sample 0 (continuous through the burst)
        phase = (float(shift) + cfo) * lo * (2.0 * np.pi / fw) + np.cumsum(freq) * (2.0 * np.pi / fw)
        x[lo:hi] += amplitude * np.exp(1j * phase)
        info.append((payload, start_out))
    if sample_format == "cf32":
        out = np.empty(2 * n, dtype=np.float32)
        out[0::2] = x.real
        out[1::2] = x.imag
        return out, info
    dtype, scale, offset = {"u8": (np.uint8, 127.6, 127.4), "s8": (np.int8, 128.0, 0.0),
                            "s16": (np.int16, 32768.0, 0.0)}[sample_format]
    lim = np.iinfo(dtype)
    out = np.empty(2 * n, dtype=dtype)
    out[0::2] = np.clip(np.rint(x.real * scale + offset), lim.min, lim.max).astype(dtype)
    out[1::2] = np.clip(np.rint(x.imag * scale + offset), lim.min, lim.max).astype(dtype)
    return out, info


def payload_of(seed: int) -> str:
    """The on-air packet hex synth_stream(seed) carries."""
    rng = np.random.default_rng(seed)
    return OTA_PACKETS[int(rng.integers(0, len(OTA_PACKETS)))]
