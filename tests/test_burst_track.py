"""k_chan_burst_expect on the device (include/rtldavis_hip.h, BURST EXPECT), through the hook rd_debug_burst_expect on the
crafted launches of tests/burst_track_cases.py: the whole slot - every field of every record, every header, and 0xA5
wherever the kernel must not write - equals the model's, at max_flips 0, 1, 2 without and with the narrow-band filter
(the wide forms alone where the symbol length is below 4).  tests/test_burst_track_cpu.py asserts each case's edge on the
model without a device.  Equality throughout."""
import ctypes as C

import numpy as np
import pytest

import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_track_cases as TK
from rtldavis_amd.wideband import BURST_MSG_DTYPE

pytestmark = pytest.mark.gpu


def _lib_with_device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return _lib


def _config(_lib, cfg):
    return _lib.make_config(cfg.bit_rate, cfg.symbol_length, cfg.preamble_symbols, cfg.packet_symbols, cfg.preamble, cfg.block_size)


def _run(_lib, X, max_flips, narrow):
    cfg = _config(_lib, X.cfg)
    msgs, hdr = np.zeros(TK.MAX, BURST_MSG_DTYPE), np.zeros(TK.MAX, TK.HDR_DTYPE)
    _lib.check(_lib.lib().rd_debug_burst_expect(C.byref(cfg), X.cur.ctypes.data, None if X.prev is None else X.prev.ctypes.data,
                                                X.cur.shape[1], X.n_ch, X.clock, X.seq, X.table.ctypes.data, X.table.size, max_flips,
                                                1 if narrow else 0, msgs.ctypes.data, hdr.ctypes.data))
    return msgs, hdr


def _assert_slot(X, r, narrow, got):
    msgs, hdr = got
    w_msgs, w_hdr = X.want(r, narrow)
    for f in TK.HDR_DTYPE.names:
        assert np.array_equal(hdr[f], w_hdr[f]), (X.name, r, narrow, f, hdr[f][: X.table.size], w_hdr[f][: X.table.size])
    for i in range(TK.MAX):
        if msgs[i].tobytes() != w_msgs[i].tobytes():
            for f in BURST_MSG_DTYPE.names:
                assert np.array_equal(msgs[i][f], w_msgs[i][f]), (X.name, r, narrow, i, f, msgs[i][f], w_msgs[i][f])
    assert msgs.tobytes() == w_msgs.tobytes() and hdr.tobytes() == w_hdr.tobytes(), (X.name, r, narrow)


def _check(launches, forms=None):
    _lib = _lib_with_device()
    for X in launches:
        for r, narrow in (X.forms() if forms is None else forms):
            _assert_slot(X, r, narrow, _run(_lib, X, r, narrow))


def _run_decode(_lib, L):
    """rd_debug_burst_decode on a burst_decode_cases.Launch: n_msgs per channel."""
    cfg = _config(_lib, L.cfg)
    msgs = np.zeros(L.msgs.shape, BURST_MSG_DTYPE)
    n_msgs, long_runs, chunk = (np.zeros(L.n_ch, np.uint32) for _ in range(3))
    _lib.check(_lib.lib().rd_debug_burst_decode(C.byref(cfg), L.cur.ctypes.data, None if L.prev is None else L.prev.ctypes.data,
                                                L.cur.shape[1], L.n_ch, L.clock, L.seq, L.runs.ctypes.data, L.n_runs.ctypes.data,
                                                msgs.ctypes.data, n_msgs.ctypes.data, long_runs.ctypes.data, chunk.ctypes.data))
    return n_msgs, long_runs


def test_window_edges():
    """The best tau at exactly t_lo, at t_hi, alone in its window; windows that end one output before the first valid tau
    and begin one after the last: candidates as the model says, no record, the place untouched."""
    _check((TK.edges_launch()[0],))


def test_seam_every_offset_reported_once():
    """The packet's last output at -SL .. SL around the boundary: chunk k and chunk k + 1 equal the model, and after step
    7' exactly one report survives per position, whichever side decodes it."""
    _lib = _lib_with_device()
    first, back, data = TK.seam_launches()
    for r, narrow in TK.FORMS:
        g0, g1 = _run(_lib, first, r, narrow), _run(_lib, back, r, narrow)
        _assert_slot(first, r, narrow, g0)
        _assert_slot(back, r, narrow, g1)
        a = g0[0][g0[1]["n_msgs"] == 1]
        b = TK.drop_repeats(g1[0][g1[1]["n_msgs"] == 1], a, DC.SEAM_SL)
        assert sorted([int(x["channel"]) for x in a] + [int(x["channel"]) for x in b]) == list(range(len(DC.SEAM_LAST))), (r, narrow)


def test_the_three_gaps_of_run_driven_decoding():
    """Window 0 OFF; a run of 33 windows; trailing symbols only: rd_debug_burst_decode gives no record - the gap is real -
    and the expectation gives the packet."""
    _lib = _lib_with_device()
    (r0, r1), X, _ = TK.gap_window0_off()
    for L in (r0, r1):
        assert not _run_decode(_lib, L)[0].any(), L.name
    R, Y = TK.gap_long_run()
    n_msgs, long_runs = _run_decode(_lib, R)
    assert list(n_msgs) == [1, 0] and list(long_runs) == [0, 1]
    (t0, t1), Z, _ = TK.gap_trailing_only()
    for L in (t0, t1):
        assert not _run_decode(_lib, L)[0].any(), L.name
    _check((X, Y, Z))
    for U in (X, Y, Z):
        assert len(U.recs()) == 1


def test_first_chunk_has_no_candidates_below_sl():
    _check(TK.first_chunk_launches())


def test_alignment_every_residue_of_t0():
    """t0 mod 8 = 0 .. 7, never a multiple of 128, loud bytes just outside the region: the rounded-down loads enter
    neither the candidates nor the filter."""
    _check((TK.alignment_launch()[0],))


def test_id_filter_also_behind_a_repair():
    _check(TK.id_launches())


def test_the_largest_region():
    """A window of 2048 at N 40, SL 51: 2049 candidates, 4089 outputs, 107 taps."""
    _check((TK.largest_launch(),))


def test_table_mechanics():
    """64 expectations in one launch, overlapping windows on a channel, idle ones between active ones; and a table with
    no active expectation: nothing is launched, the slot stays 0xA5."""
    _check((TK.full_table_launch(), TK.all_idle_launch()), forms=TK.FORMS)


def test_ties_and_corr_bounds():
    """Equal margins give the smaller tau; corr at the ends of its range on saturated bytes."""
    _check((TK.tie_launch(), TK.bounds_launch()))


def test_repair_composition():
    _check(TK.repair_launches())


@pytest.mark.parametrize("n", [40, 64, 80])
def test_packet_shapes(n):
    """N 40, 64, 80 x SL 4 .. 51: every packet shape the filter admits, an expectation per channel."""
    _check(tuple(TK.grid_launch(m, sl) for m, sl in NB.NGRID if m == n), forms=TK.FORMS)
