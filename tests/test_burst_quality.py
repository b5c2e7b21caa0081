"""k_chan_burst_quality on the device (include/rtldavis_hip.h, BURST QUALITY), through the hook rd_debug_burst_quality on
the crafted launches of tests/burst_quality_cases.py: the whole quality slot - every field of every record, and 0xA5
wherever the kernel must not write: the places past a channel's n_msgs and the expect part, which the hook never launches
over - equals the model's.  One launch per case.  tests/test_burst_quality_cpu.py asserts each case's edge on the model
without a device.  Equality throughout."""
import ctypes as C

import numpy as np
import pytest

import burst_quality_cases as QC
from rtldavis_amd.wideband import QUALITY_DTYPE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def _lib():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return _lib


def _run(_lib, X):
    cfg = _lib.make_config(X.cfg.bit_rate, X.cfg.symbol_length, X.cfg.preamble_symbols, X.cfg.packet_symbols, X.cfg.preamble, X.cfg.block_size)
    out = np.zeros(X.n_ch * X.cap + QC.BX_MAX, QUALITY_DTYPE)
    _lib.check(_lib.lib().rd_debug_burst_quality(C.byref(cfg), X.cur.ctypes.data, None if X.prev is None else X.prev.ctypes.data,
                                                 X.cur.shape[1], X.n_ch, X.gap, X.msgs.ctypes.data, X.n_msgs.ctypes.data, out.ctypes.data))
    return out


def _assert_slot(X, got):
    for i in range(got.size):
        if got[i].tobytes() != X.want[i].tobytes():
            where = f"expect place {i - X.n_ch * X.cap}" if i >= X.n_ch * X.cap else f"channel {i // X.cap} place {i % X.cap}"
            raise AssertionError(f"{X.name}: {where}: got {got[i]}, the model gives {X.want[i]}")


CASES = ("default_launch", "sl4_launch", "sl3_launch", "sl51_launch", "largest_launch", "residue_launch", "saturated_launch",
         "flat_launch", "record_launch", "occupancy_launch")


@pytest.mark.parametrize("case", CASES)
def test_slot_equals_model(_lib, case):
    X = getattr(QC, case)()
    _assert_slot(X, _run(_lib, X))


@pytest.mark.parametrize("which", (0, 1), ids=("alone", "prev"))
def test_window_placement(_lib, which):
    X = QC.placement_launches()[which]
    _assert_slot(X, _run(_lib, X))


def test_same_launch_twice_gives_the_same_bytes(_lib):
    X = QC.default_launch()
    assert _run(_lib, X).tobytes() == _run(_lib, X).tobytes()
