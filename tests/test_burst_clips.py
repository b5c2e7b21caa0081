"""k_chan_burst_clips on the device (include/rtldavis_hip.h, BURST CLIPS), through the hook rd_debug_burst_clips on the
crafted launches of tests/burst_clip_cases.py: the whole clip slot - every field of every record, every header, every byte
of every pool, and 0xA5 wherever the kernel must not write: the record places past a channel's n_clips, the padding in front
of the pools and each pool past 2 * used - equals the model's, byte for byte.  One launch per case.
tests/test_burst_clips_cpu.py asserts each case's edge on the model without a device.  Then the argument rules of the hook
and of rd_wb_set_burst_clips: RD_ERR_ARG before RD_ERR_STATE, and before any device work."""
import ctypes as C

import numpy as np
import pytest

import burst_clip_cases as CC
import burst_decode_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def _lib():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _call(_lib, X, **over):
    """The hook's return code and the slot it filled; ``over`` replaces settings (sources, pre, post, quota)."""
    cfg = _lib.make_config(X.cfg.bit_rate, X.cfg.symbol_length, X.cfg.preamble_symbols, X.cfg.packet_symbols, X.cfg.preamble, X.cfg.block_size)
    s = dict(sources=X.sources, pre=X.pre, post=X.post, quota=X.quota)
    s.update(over)
    out = np.zeros(CC.slot_bytes(X.n_ch, s["quota"] if 8 <= s["quota"] <= CC.MAX_QUOTA else 8), np.uint8)
    rc = _lib.lib().rd_debug_burst_clips(C.byref(cfg), X.cur.ctypes.data, _ptr(X.prev), X.cur.shape[1], X.n_ch, X.clock, X.seq,
                                        X.runs.ctypes.data, X.n_runs.ctypes.data, X.msgs.ctypes.data, X.n_msgs.ctypes.data,
                                        _ptr(X.x_msgs), _ptr(X.x_hdr), X.n_expect, _ptr(X.s_msgs), _ptr(X.s_hdr), X.n_search,
                                        _ptr(X.owed_prev), s["sources"], s["pre"], s["post"], s["quota"], out.ctypes.data)
    return rc, out


def _run(_lib, X):
    assert int(_lib.lib().rd_bc_slot_size(X.n_ch, X.quota)) == CC.slot_bytes(X.n_ch, X.quota)
    rc, out = _call(_lib, X)
    _lib.check(rc)
    return out


def _assert_slot(X, got):
    if got.tobytes() == X.want.tobytes():
        return
    g_recs, g_hdr, g_pool = CC.split_slot(got, X.n_ch, X.quota)
    w_recs, w_hdr, w_pool = CC.split_slot(X.want, X.n_ch, X.quota)
    for c in range(X.n_ch):
        assert g_hdr[c].tobytes() == w_hdr[c].tobytes(), f"{X.name}: header of channel {c}: got {g_hdr[c]}, the model gives {w_hdr[c]}"
        for i in range(CC.PER):
            assert g_recs[c, i].tobytes() == w_recs[c, i].tobytes(), f"{X.name}: channel {c} place {i}: got {g_recs[c, i]}, the model gives {w_recs[c, i]}"
        bad = np.flatnonzero(g_pool[c] != w_pool[c])
        assert bad.size == 0, f"{X.name}: pool of channel {c}: {bad.size} bytes differ, the first at {bad[0]}: got {g_pool[c, bad[0]]}, the model gives {w_pool[c, bad[0]]}"
    raise AssertionError(f"{X.name}: the padding between the headers and the pools was written")


def test_owed_chains_through_tails_that_are_cut_again(_lib):
    """B = 128, post = 1024: five consecutive launches, each fed the chunk before and the owed words the DEVICE wrote for it."""
    owed = None
    for X in CC.chain_launches():
        if owed is not None:
            assert np.array_equal(owed, X.owed_prev)
        got = _run(_lib, X)
        _assert_slot(X, got)
        owed = CC.split_slot(got, X.n_ch, X.quota)[1]["owed"].copy()
    assert list(owed) == [512, 0]


@pytest.mark.parametrize("which", range(4), ids=("256_prev", "256_alone", "2048_prev", "2048_alone"))
def test_a_run_at_window_0(_lib, which):
    X = CC.window0_launches()[which]
    _assert_slot(X, _run(_lib, X))


def test_a_run_at_the_last_window_and_the_tail_that_follows(_lib):
    a, b = CC.end_launches()
    got = _run(_lib, a)
    _assert_slot(a, got)
    assert np.array_equal(CC.split_slot(got, a.n_ch, a.quota)[1]["owed"], b.owed_prev)
    _assert_slot(b, _run(_lib, b))


CASES = ("no_roll_launch", "residue_launch", "per_launch", "quota_launch", "sources_launch", "skipped_launch")


@pytest.mark.parametrize("case", CASES)
def test_slot_equals_model(_lib, case):
    X = getattr(CC, case)()
    _assert_slot(X, _run(_lib, X))


@pytest.mark.parametrize("which", range(3), ids=("4_40", "14_80", "51_40"))
def test_packet_shapes(_lib, which):
    X = CC.shape_launches()[which]
    _assert_slot(X, _run(_lib, X))


@pytest.mark.parametrize("n_ch", (1, 3, 70))
def test_channel_counts(_lib, n_ch):
    X = CC.channels_launch(n_ch)
    _assert_slot(X, _run(_lib, X))


def test_same_launch_twice_gives_the_same_bytes(_lib):
    X = CC.sources_launch()
    assert _run(_lib, X).tobytes() == _run(_lib, X).tobytes()


BAD_SETTINGS = (dict(sources=4), dict(sources=7), dict(sources=-1), dict(sources=0), dict(pre=-8), dict(pre=4), dict(pre=1032),
                dict(post=-8), dict(post=12), dict(post=1032), dict(quota=0), dict(quota=4), dict(quota=12), dict(quota=65544))


@pytest.mark.parametrize("over", BAD_SETTINGS, ids=lambda o: "_".join(f"{k}{v}" for k, v in o.items()))
def test_the_hook_refuses_bad_settings(_lib, over):
    X = CC.no_roll_launch()
    rc, out = _call(_lib, X, **over)
    assert rc == _lib.RD_ERR_ARG, (over, rc, _lib.last_error())
    assert not out.any()                                         # (nothing was copied out)


def test_the_hook_refuses_a_pool_over_the_limit_and_a_configuration_decode_refuses(_lib):
    X = CC.channels_launch(70)
    assert 70 * 65536 * 2 <= CC.MAX_POOL
    big = CC.CLaunch("clips_pool", 4, 40, 128, 520, CC.RUNS, 0, 0, 8, seed=1)
    assert 520 * 65536 * 2 > CC.MAX_POOL >= 512 * 65536 * 2
    rc, _ = _call(_lib, big, quota=65536)
    assert rc == _lib.RD_ERR_ARG and "more than" in _lib.last_error()
    # B = 128 holds no packet: refused with RD_BC_MESSAGES, fine with runs alone (the chain launches)
    rc, _ = _call(_lib, CC.chain_launches()[0], sources=CC.RUNS | CC.MESSAGES)
    assert rc == _lib.RD_ERR_ARG
    assert X.n_ch == 70


def test_set_burst_clips_checks_arguments_before_state(_lib):
    """Without bursts every call is a state error - unless an argument is wrong, which is reported first.  No device work."""
    rx = DC.device_receiver(1152)
    assert rx.burst_clips_config() == (0, 256, 128, 4096)
    with pytest.raises(RuntimeError, match="bursts on"):
        rx.set_burst_clips()
    for bad in BAD_SETTINGS:
        if bad == dict(sources=0):
            continue
        with pytest.raises(ValueError):
            rx.set_burst_clips(**bad)
    with pytest.raises(ValueError, match="more than"):
        DC.device_receiver(1152, offsets_hz=tuple(range(-300000, 300000, 1000))).set_burst_clips(quota=65536)   # 600 channels
    rx.set_bursts(True)
    with pytest.raises(RuntimeError, match="burst decode on"):
        rx.set_burst_clips()
    rx.set_burst_clips(CC.RUNS, 8, 1024, 65536)
    assert rx.burst_clips_config() == (CC.RUNS, 8, 1024, 65536)
    with pytest.raises(ValueError):
        rx.set_burst_clips(CC.RUNS, 8, 1024, 65537)
    assert rx.burst_clips_config() == (CC.RUNS, 8, 1024, 65536)    # (a refused call changes nothing)
    rx.set_burst_decode(True)
    rx.set_burst_clips()
    assert rx.burst_clips_config() == (CC.RUNS | CC.MESSAGES, 256, 128, 4096)
    rx.set_burst_decode(False)
    assert rx.burst_clips_config()[0] == CC.RUNS                   # (clips of runs go on)
    rx.set_burst_decode(True)
    rx.set_burst_clips(CC.MESSAGES)
    rx.set_burst_decode(False)
    assert rx.burst_clips_config()[0] == 0                         # (nothing left: off)
    rx.set_burst_clips(CC.RUNS)
    rx.set_bursts(False)
    assert rx.burst_clips_config()[0] == 0
    with pytest.raises(RuntimeError):
        rx.burst_clips()                                           # no chunk fetched
    rx.set_bursts(True)
    rx.set_burst_clips(0)                                          # off is a setting like any other
    assert rx.burst_clips_config()[0] == 0
