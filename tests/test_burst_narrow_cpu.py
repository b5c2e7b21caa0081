"""The narrow-band filter of the burst decoder (include/rtldavis_hip.h, BURST DECODE, step 4n), the part that needs no
GPU: the library's tables against the NumPy formula; every crafted case of tests/burst_narrow_cases.py built, which
asserts the edge it is made for on the model; the bounds of the header on a saturated region; the gain on noisy bursts
as a condition; the carrier estimates on the float64 channelizer model; the state rules of the setter and the argument
rules of the hook through the C ABI (host bookkeeping: no device is touched).  tests/test_burst_narrow.py holds the
kernel to the same model on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import burst_cases as BC
import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_repair_cases as RP
import retune_cases as RC
from rtldavis_amd import acquire
from rtldavis_amd.wideband import BURST_MSG_DTYPE, BURST_THRESHOLD_OFF

OUT_RATE, IF_HZ = 268800, -67200
SLS = (4, 8, 14, 25, 51)


# ------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("sl", SLS)
def test_library_table_equals_the_formula(sl):
    """rd_bd_narrow_table against the float64 formula in NumPy: every int16 equal (no last-bit difference between the
    C library's cos / sin and NumPy's has shown at these sizes: had one, the pair nearest a half would differ by 1 here),
    and the largest sum of |H.re| + |H.im| over g is the header's."""
    H, Cn = NB.table(sl)
    LH, LC = NB.library_table(sl)
    assert H.shape == (64, 2 * sl + 5, 2) and np.array_equal(LH, H) and np.array_equal(LC, Cn)
    assert int(np.abs(H).sum(axis=(1, 2)).max()) == NB.SUM_ABS[sl]
    assert 255 * NB.SUM_ABS[sl] < 2 ** 23 and (255 * NB.SUM_ABS[sl] + 1024) >> 11 <= NB.Y_MAX
    assert abs(int(H[0, :, 0].sum()) - 2 ** 14) <= sl + 3 and not H[0, :, 1].any()      # unit gain at the centre, to the rounding
    assert np.array_equal(H[:, sl + 2, 1], np.zeros(64)) and len(set(H[:, sl + 2, 0])) == 1   # k = 0 carries no phase
    assert tuple(Cn[0]) == (16384, 0) and tuple(Cn[16]) == (0, 16384) and tuple(Cn[1]) == (16305, 1606)


def test_table_arguments():
    from rtldavis_amd import _lib
    L = _lib.lib()
    taps, centres = np.zeros((64, 107, 2), np.int16), np.zeros((64, 2), np.int16)
    for sl in (3, 0, -1, 52):
        assert L.rd_bd_narrow_table(sl, taps.ctypes.data, centres.ctypes.data) == _lib.RD_ERR_ARG
    assert L.rd_bd_narrow_table(8, None, centres.ctypes.data) == _lib.RD_ERR_ARG
    assert L.rd_bd_narrow_table(8, taps.ctypes.data, None) == _lib.RD_ERR_ARG
    assert not taps.any() and not centres.any()
    assert L.rd_bd_narrow_table(51, taps.ctypes.data, centres.ctypes.data) == _lib.RD_OK and taps.any()


# ------------------------------------------------------------------------------------------ the crafted cases' edges
def test_grid_choice_and_its_ties():
    """(1606, 79) scores g = 0 and g = 1 alike and 0 wins; a correlation sum on each axis; corr_re = -1 with sh = 0; bit
    length 31 with sh = 16 and a floor of a negative part - each decodes its burst at that g (asserted in the builder)."""
    L = NB.choice_launch()
    assert [NB._pad(L.nrecs(0, c)[0])[3] for c in range(L.n_ch)] == [g for _, g in NB.CHOICE] == [0, 0, 16, 32, 48, 32, 59]
    assert NB.grid_choice(1606, 79)[3] == 0 and NB.grid_choice(1606, 80)[3] == 1 and NB.grid_choice(1606, -79)[3] == 0
    assert NB.grid_choice(1606, -80)[3] == 63
    assert NB.grid_choice(2 ** 15 - 1, 0)[0] == 0 and NB.grid_choice(2 ** 15, 0)[:2] == (1, 2 ** 14)
    assert NB.grid_choice(-(2 ** 15), 1)[:3] == (1, -(2 ** 14), 0)


def test_zero_extension_at_both_ends_of_the_region():
    """The run record is cut out of a longer stretch of carrier: the packet whose first symbol begins at t0 + 1 has
    tau = t0 + SL, the packet whose last output is t1 - 1 is decoded too, and y at the region's first and last output is
    not what the bytes beyond the region would have made it."""
    L, (t0, t1) = NB.edge_launch()
    sl, n = 4, 80
    assert NB.edge_taus(L) == [[t0 + sl], [t1 - 1 - sl * (n - 1)]]
    for c in (0, 1):
        assert all(L.ncounts(r)[c] == 1 for r in range(3)) and int(L.nrecs(0, c)[0]["flags"]) == NB.NARROW
        mine, theirs = NB.y_with_neighbours(L, c)
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) > 50 for a, b in zip(mine, theirs)), (mine, theirs)


@pytest.mark.parametrize("sl", SLS)
def test_saturated_region_reaches_the_bounds_and_no_further(sl):
    """Bytes 0 and 255 whose signs follow the taps at the filter's centre: acc there is 255 x the table's largest sum -
    below 2^23 - and |y| <= 3192; filter_region asserts both on every output."""
    H, _ = NB.table(sl)
    g = int(np.abs(H).sum(axis=(1, 2)).argmax())
    zi, zq, t = NB.worst_region(sl, g)
    assert set(np.abs(zi)) == {255} == set(np.abs(zq))
    (acc_re, acc_im), (y_re, y_im) = NB.filter_region(zi, zq, H[g])
    assert int(acc_re[t]) == 255 * NB.SUM_ABS[sl] == int(np.abs(acc_re).max()) < 2 ** 23
    assert int(y_re[t]) == (255 * NB.SUM_ABS[sl] + 1024) >> 11 <= NB.Y_MAX
    if sl == 4:
        assert int(y_re[t]) == NB.Y_MAX                      # the bound is met at the shortest filter


def test_saturated_launch_stays_inside_every_bound():
    """A hard-limited burst beside a correlation sum of bit length 30: decoded; symbol_sums asserts |p'| < 2^25, the
    SL-sums < 2^31 and |s| < 2^47, decode_run |f| < 2^36."""
    L = NB.saturated_launch()
    taus, s, _, p_re, p_im, _, g = L.nsums(0)
    assert int(np.abs(s).max()) > 2 ** 38 and max(int(np.abs(p_re).max()), int(np.abs(p_im).max())) > 2 ** 22
    m = L.nrecs(0, 0)[0]
    assert max(abs(int(m["f_re"])), abs(int(m["f_im"]))) > 2 ** 31   # (the kernel's int sums must have widened)


def test_the_other_crafted_launches_reach_their_edges():
    """Every launch the device test runs is built here: packet shapes with 26 different grid points, the seam with
    flags = 5, the longest regions at SL 25 and SL 51, one flipped symbol with pad = (1, k, 0, g)."""
    Ls = NB.crafted_launches()
    assert len({L.name for L in Ls}) == len(Ls) == len(NB.NGRID) + 8
    assert len(set(NB.grid_points())) == 2 * len(NB.NGRID)
    for L in Ls:                                             # narrow off is the repair module's model, whatever the bytes
        for r in range(3):
            got = RP.slot_model(L, r)
            assert got[0].tobytes() == L.want[r][0].tobytes()


def test_narrow_off_is_the_repair_modules_stream():
    _, _, (b0, b1), cfg, data = NB.seam_launches()
    blocks = [b0[None, :], b1[None, :]]
    for r in (0, 2):
        a = NB.decode_stream(blocks, DC.THR, cfg, r, narrow=False)
        b = RP.decode_stream(blocks, DC.THR, cfg, r)
        assert [m.records.tobytes() for _, m in a] == [m.records.tobytes() for _, m in b]
        on = NB.decode_stream(blocks, DC.THR, cfg, r)
        assert [m.records.size for _, m in on] == [0, 1] and bytes(on[1][1].records[0]["data"]) == data
        assert int(on[1][1].records[0]["flags"]) == 5
    rec = BC.model_bursts(b1[None, :], DC.THR, 1).records[0]
    assert NB.decode_run(b1, b0, rec, cfg, True, 1, narrow=False) == RP.decode_run(b1, b0, rec, cfg, True, 1)


# ------------------------------------------------------------------------------------------ the gain
def test_gain_on_noisy_bursts():
    """60 bursts of gain_blocks at noise 0.20 (amplitude 0.3, seed 7) under gain_threshold(0.20), R = 0: the wide model
    decodes none (measured: 0), the narrow model at least 45 with no payload that was not planted (measured: 53 and 0)."""
    out, datas = NB.gain_run(60, 0.20, 7, flips=(0,))
    wide, narrow = NB.tally(out[False, 0], datas), NB.tally(out[True, 0], datas)
    print(f"\n[narrow gain, noise 0.20, 60 bursts, R = 0] wide {wide[0]} decoded / {wide[1]} wrong, narrow {narrow[0]} / {narrow[1]}")
    assert wide == (0, 0)
    assert narrow[0] >= 45 and narrow[1] == 0
    assert all(int(r["flags"]) & NB.NARROW for r in out[True, 0])


# ------------------------------------------------------------------------------------------ carrier estimates
@functools.lru_cache(maxsize=None)
def _open_loop(planted):
    lc, want = DC.acq_plan(planted)
    blocks = RC.loop_model_blocks(lc, {})
    thr = BC.new_acquisition().thresholds(BC.burst_model(blocks[0], BURST_THRESHOLD_OFF)[1])
    return lc, want, blocks, thr


@pytest.mark.parametrize("planted", BC.PLANTED)
def test_carrier_estimates_on_the_channelizer_model(planted):
    """The acquisition capture's two bursts, 20, -20 and 38 kHz off, through the float64 channelizer model with narrow on:
    both decode, and burst_message_offset_hz of each narrow row lies within the 1500 Hz the closed loop allows."""
    lc, want, blocks, thr = _open_loop(planted)
    cfg = RC.packet_config(2048)
    est = {}
    for narrow in (False, True):
        out = NB.decode_stream(DC.rechunk(blocks, 2048), thr, cfg, 0, narrow)
        rows = [r for _, m in out for r in m.records]
        assert [bytes(r["data"]).hex() for r in rows] == [lc.payload, lc.payload]
        assert acquire.narrowband(np.asarray(rows, BURST_MSG_DTYPE)).tolist() == [narrow, narrow]
        est[narrow] = [acquire.burst_message_offset_hz(r, OUT_RATE, IF_HZ) for r in rows]
    print(f"\n[narrow estimates] planted {planted} Hz: " + ", ".join(
        f"wide {a - w:+.0f} Hz / narrow {b - w:+.0f} Hz" for a, b, w in zip(est[False], est[True], want)))
    for e, w in zip(est[True], want):
        assert abs(e - w) <= BC.ESTIMATE_TOL_HZ


# ------------------------------------------------------------------------------------------ C ABI without a device
def _receiver(bs=2048, decim=100, n_ch=2, sl=14):
    from rtldavis_amd import wideband
    chans = [RC.CENTRE - 100000 + 50000 * c for c in range(n_ch)]
    return wideband.WidebandReceiver(RC.packet_config(bs, sl), chans, RC.CENTRE, decim=decim, taps=np.ones(8) / 8)


def test_set_burst_narrow_state_rules():
    from rtldavis_amd import _lib
    L = _lib.lib()
    w = _receiver()
    assert w.burst_narrow() is False
    w.set_bursts(True)
    with pytest.raises(RuntimeError):
        w.set_burst_narrow(True)                             # decode is off
    assert "decode" in _lib.last_error() and not w.burst_narrow()
    assert L.rd_wb_set_burst_narrow(w._h, 0) == _lib.RD_ERR_STATE
    assert L.rd_wb_set_burst_narrow(None, 1) == _lib.RD_ERR_ARG and L.rd_wb_burst_narrow(w._h, None) == _lib.RD_ERR_ARG
    w.set_burst_decode(True)
    w.set_burst_narrow()
    assert w.burst_narrow() is True
    w.set_burst_repair(2)                                    # composes
    assert w.burst_narrow() and w.burst_repair() == 2
    w.reset()
    assert w.burst_narrow() and w.burst_repair() == 2        # reset() keeps both
    w.set_burst_narrow(False)
    assert not w.burst_narrow() and w.burst_repair() == 2
    w.set_burst_narrow(True)
    w.set_burst_decode(False)
    assert not w.burst_narrow()                              # decode off puts it back
    w.set_burst_decode(True)
    assert not w.burst_narrow()
    w.set_burst_narrow(True)
    w.set_bursts(False)
    assert not w.burst_narrow()
    small = _receiver(sl=3)                                  # SL 3: decode is legal, the filter is not
    small.set_bursts(True)
    small.set_burst_decode(True)
    with pytest.raises(ValueError):
        small.set_burst_narrow(True)
    assert "symbol_length" in _lib.last_error() and not small.burst_narrow()
    small.set_burst_narrow(False)
    four = _receiver(sl=4)
    four.set_bursts(True)
    four.set_burst_decode(True)
    four.set_burst_narrow(True)


def test_hook_arguments_are_refused_before_any_device_work():
    from rtldavis_amd import _lib
    L = _lib.lib()
    assert "rd_debug_burst_decode_narrow" in _lib.SIGNATURES and "rd_bd_narrow_table" in _lib.SIGNATURES
    G = NB.grid_launch(40, 8)
    msgs = np.zeros(G.narrow[0][0].shape, BURST_MSG_DTYPE)
    n_msgs, long_runs, chunk = (np.zeros(G.n_ch, np.uint32) for _ in range(3))

    def call(cfg, max_flips, narrow):
        c = _lib.make_config(cfg.bit_rate, cfg.symbol_length, cfg.preamble_symbols, cfg.packet_symbols, cfg.preamble, cfg.block_size)
        return L.rd_debug_burst_decode_narrow(C.byref(c), G.cur.ctypes.data, None, G.cur.shape[1], G.n_ch, 0, 0, G.runs.ctypes.data,
                                              G.n_runs.ctypes.data, max_flips, narrow, msgs.ctypes.data, n_msgs.ctypes.data,
                                              long_runs.ctypes.data, chunk.ctypes.data)

    assert call(G.cfg, 0, 2) == _lib.RD_ERR_ARG and "narrow" in _lib.last_error()
    assert call(G.cfg, 0, -1) == _lib.RD_ERR_ARG
    assert call(G.cfg, 3, 1) == _lib.RD_ERR_ARG
    assert call(DC.config(3, 40, 2048), 0, 1) == _lib.RD_ERR_ARG and "symbol_length" in _lib.last_error()
    assert not msgs.view(np.uint8).any()
