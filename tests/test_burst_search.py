"""k_chan_burst_search on the device (include/rtldavis_hip.h, BURST SEARCH), through the hook rd_debug_burst_search on the
crafted launches of tests/burst_search_cases.py: the whole slot - every field of every record, every header, and 0xA5
wherever the kernel must not write - equals the model's.  tests/test_burst_search_cpu.py asserts each case's edge on the
model without a device.  Equality throughout."""
import ctypes as C

import numpy as np
import pytest

import burst_decode_cases as DC
import burst_search_cases as SC
from rtldavis_amd.wideband import BURST_MSG_DTYPE, BURST_SEARCH_TILE, SEARCH_HDR_DTYPE

pytestmark = pytest.mark.gpu


def _lib_with_device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return _lib


def _config(_lib, cfg):
    return _lib.make_config(cfg.bit_rate, cfg.symbol_length, cfg.preamble_symbols, cfg.packet_symbols, cfg.preamble, cfg.block_size)


def _call(_lib, L, centres, msgs, hdr):
    cfg = _config(_lib, L.cfg)
    c = np.ascontiguousarray(centres, np.uint8)
    return _lib.lib().rd_debug_burst_search(C.byref(cfg), L.cur.ctypes.data, None if L.prev is None else L.prev.ctypes.data,
                                            L.cur.shape[1], L.n_ch, L.clock, L.seq, c.ctypes.data, c.size, msgs.ctypes.data, hdr.ctypes.data)


def _run(_lib, L):
    msgs = np.zeros((SC.MAX_CENTRES, L.n_ch, SC.PER), BURST_MSG_DTYPE)
    hdr = np.zeros((SC.MAX_CENTRES, L.n_ch), SEARCH_HDR_DTYPE)
    _lib.check(_call(_lib, L, L.centres, msgs, hdr))
    return msgs, hdr


def _assert_slot(L, got):
    msgs, hdr = got
    w_msgs, w_hdr = L.want()
    for f in SEARCH_HDR_DTYPE.names:
        assert np.array_equal(hdr[f], w_hdr[f]), (L.name, f, hdr[f][: len(L.centres)], w_hdr[f][: len(L.centres)])
    for idx in np.ndindex(msgs.shape):
        if msgs[idx].tobytes() != w_msgs[idx].tobytes():
            for f in BURST_MSG_DTYPE.names:
                assert np.array_equal(msgs[idx][f], w_msgs[idx][f]), (L.name, idx, f, msgs[idx][f], w_msgs[idx][f])
    assert msgs.tobytes() == w_msgs.tobytes() and hdr.tobytes() == w_hdr.tobytes(), L.name


def _check(launches):
    _lib = _lib_with_device()
    for L in launches:
        _assert_slot(L, _run(_lib, L))


@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: f"sl{s[0]}_n{s[1]}_b{s[2]}")
def test_packet_shapes(shape):
    """SL 4 .. 51 at three channels behind a chunk: a packet in mid-chunk, a packet that begins in the previous chunk,
    and a channel of quiet bytes."""
    _check((SC.shape_launch(*shape),))


def test_packet_ends_at_the_candidate_range_ends():
    """Packets whose last output is output 0, SL - 1 and B - 1."""
    _check((SC.ends_launch(),))


def test_first_chunk_has_no_candidates_below_sl():
    _check((SC.first_chunk_launch(),))


def test_six_packets_four_records_two_dropped():
    _check((SC.six_packets_launch(),))


def test_equal_margins_give_the_smaller_tau():
    _check((SC.tie_launch(),))


def test_packets_across_every_tile_boundary():
    assert BURST_SEARCH_TILE == SC.TILE
    _check((SC.tile_launch(),))


def test_the_largest_grid_and_slot():
    """8 centres x 70 channels."""
    _check((SC.largest_launch(),))


def test_seam_every_offset_reported_once():
    """The packet's last output at -SL .. SL around the boundary: chunk k and chunk k + 1 equal the model, and after step
    7s exactly one report survives per position, whichever side finds it."""
    _lib = _lib_with_device()
    first, back, data = SC.seam_launches()
    g0, g1 = _run(_lib, first), _run(_lib, back)
    _assert_slot(first, g0)
    _assert_slot(back, g1)
    a = np.asarray([g0[0][0, c, r] for c in range(first.n_ch) for r in range(int(g0[1][0, c]["n_msgs"]))], BURST_MSG_DTYPE).reshape(-1)
    b = np.asarray([g1[0][0, c, r] for c in range(back.n_ch) for r in range(int(g1[1][0, c]["n_msgs"]))], BURST_MSG_DTYPE).reshape(-1)
    b = SC.drop_repeats(b, a, DC.SEAM_SL)
    assert sorted([int(x["channel"]) for x in a] + [int(x["channel"]) for x in b]) == list(range(len(DC.SEAM_LAST)))
    assert all(bytes(x["data"][: DC.SEAM_N // 8]) == data for x in list(a) + list(b))


def test_bad_centres_are_refused_with_nothing_launched():
    """A duplicate, a centre of 64, no centre and nine: RD_ERR_ARG, and the caller's arrays stay as they were."""
    _lib = _lib_with_device()
    L = SC.first_chunk_launch()
    for centres in ([7, 7], [7, 64], [], list(range(9))):
        msgs = np.full((SC.MAX_CENTRES, L.n_ch, SC.PER), 0, BURST_MSG_DTYPE)
        hdr = np.zeros((SC.MAX_CENTRES, L.n_ch), SEARCH_HDR_DTYPE)
        hdr["chunk"] = 0x12345678
        with pytest.raises(ValueError):
            _lib.check(_call(_lib, L, centres, msgs, hdr))
        assert np.all(hdr["chunk"] == 0x12345678) and not msgs.tobytes().strip(b"\0")


def test_two_runs_give_identical_bytes():
    _lib = _lib_with_device()
    L = SC.largest_launch()
    a, b = _run(_lib, L), _run(_lib, L)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
