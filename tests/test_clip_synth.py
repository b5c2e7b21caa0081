"""k_clip_synth / rd_clips_synth, rd_clips_download on the device (include/rtldavis_hip.h, CLIP SYNTH) against the NumPy model
of tests/clip_synth_cases.py: the downloaded pool byte for byte, for every case; the decoder on a synthesised pool against
the decoder on the model's pool uploaded; what an upload and a synthesis leave of each other; every refusal; and one
statistical check of the device's own noise.  The cases assert their own edges on the model when they are built."""
import ctypes as C

import numpy as np
import pytest

import burst_decode_cases as DC
import clip_replay_cases as RC
import clip_synth_cases as SC
from rtldavis_amd import _lib, replay
from rtldavis_amd.replay import SPEC_DTYPE, ClipDecoder

pytestmark = pytest.mark.gpu


def _decoder(cfg):
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return ClipDecoder(cfg)


def _first_difference(got, want):
    d = np.flatnonzero(got != want)
    return None if d.size == 0 else (int(d[0]), int(got[d[0]]), int(want[d[0]]), int(d.size))


def _assert_pool(dec, X):
    dec.synthesize(X.specs, X.pool_outputs)
    assert dec.pool_outputs == X.pool_outputs
    got = dec.download()
    assert got.dtype == np.uint8 and got.size == X.pool.size and _first_difference(got, X.pool) is None, (X.name, _first_difference(got, X.pool))
    return got


@pytest.mark.parametrize("X", SC.exact_cases(), ids=lambda X: X.name)
def test_pool_equals_the_model(X):
    dec = _decoder(X.config())
    first = _assert_pool(dec, X)
    again = _assert_pool(dec, X)                               # twice in a row: the same bytes
    assert first.tobytes() == again.tobytes() and dec.synth_ms() > 0.0


def test_random_specs_equal_the_model():
    X = SC.random_case()
    dec = _decoder(X.config())
    _assert_pool(dec, X)
    _assert_pool(dec, X)


def test_same_spec_same_bytes_wherever_it_lies():
    X = SC.seeds_case()
    dec = _decoder(X.config())
    got = _assert_pool(dec, X)
    assert X.clip(0, got).tobytes() == X.clip(4, got).tobytes() == X.clip(6, got).tobytes() != X.clip(5, got).tobytes()
    assert X.clip(2, got).tobytes() != X.clip(3, got).tobytes()           # seeds that differ in the high word alone


def test_gaps_read_zero_whatever_the_pool_held():
    X = SC.gaps_case()
    dec = _decoder(X.config())
    dec.upload(np.full(2 * X.pool_outputs + 4096, 0xA5, np.uint8))        # a larger pool of 0xA5 first
    assert np.all(dec.download() == 0xA5)
    got = _assert_pool(dec, X)
    used = np.zeros(X.pool_outputs, bool)
    for s in X.specs:
        used[int(s["offset"]): int(s["offset"]) + int(s["n"])] = True
    assert not got.reshape(-1, 2)[~used].any() and got.reshape(-1, 2)[used].all()


def test_pools_larger_smaller_larger():
    small, mid, big = SC.lengths_case(), SC.levels_case(), SC.random_case()
    assert small.pool_outputs < mid.pool_outputs < big.pool_outputs
    dec = _decoder(small.config())
    for X in (mid, small, big, small, mid):                    # shrinks (the allocation stays), grows, shrinks, grows within it
        _assert_pool(dec, X)


def _burst_case(sl):
    n_sym = 80 if sl * 80 + 1 <= 2048 else 40
    datas = [DC.packet(n_sym, ident=k % 8, seed=5600 + k) for k in range(6)]
    n = (32 + n_sym + 8) * sl + 301
    specs, tau = replay.burst_specs(datas, n=n, at=[60 + 7 * k for k in range(6)], seed=5600 + sl, amplitude=0.3,
                                    noise=[0.0, 0.02, 0.05, 0.1, 0.2, 0.3], offset_hz=[0.0, 900.0, -1500.0, 300.0, -200.0, 50.0], symbol_length=sl)
    return DC.config(sl, n_sym, 2048), specs, tau, datas


@pytest.mark.parametrize("sl", (3, 4, 14, 51))
def test_decode_on_a_synthesised_pool_equals_decode_on_the_models_pool(sl):
    cfg, specs, tau, datas = _burst_case(sl)
    n_sym = int(cfg.packet_symbols)
    model = SC.pool_of(specs, sl)
    syn, up = _decoder(cfg), _decoder(cfg)
    syn.synthesize(specs)
    up.upload(model)
    assert syn.pool_outputs == up.pool_outputs and _first_difference(syn.download(), model) is None
    jobs = np.concatenate([replay.centred_jobs(specs, tau, span=40), replay.centred_jobs(specs, tau, span=40, corr=syn.corr(0.0))])
    decoded = 0
    for r, nb in RC.forms_for(sl):
        a, b = syn.decode_jobs(jobs, r, nb, soft=True), up.decode_jobs(jobs, r, nb, soft=True)
        assert a.records.tobytes() == b.records.tobytes() and a.headers.tobytes() == b.headers.tobytes() and np.array_equal(a.soft, b.soft)
        for j in np.flatnonzero(a.headers["n_msgs"][:2] == 1):             # the clean clips give their planted packets where planted:
            dt = int(a.records[j]["tau"]) - int(tau[j])                    # the noise-free one exactly, the other within SL / 4
            assert bytes(a.records[j]["data"][: n_sym // 8]) == datas[j] and (dt == 0 if j == 0 else abs(dt) <= max(1, sl // 4)), (sl, r, nb, j, dt)
            decoded += 1
        assert int(a.headers["n_msgs"][0]) == 1, (sl, r, nb)
    assert decoded >= len(RC.forms_for(sl))


def test_upload_and_synthesis_leave_no_trace_of_each_other():
    X, Y = SC.gaps_case(), SC.seeds_case()
    dec = _decoder(X.config())
    noise = np.random.default_rng(5700).integers(0, 256, 2 * Y.pool_outputs + 64, dtype=np.uint8)
    _assert_pool(dec, X)
    dec.upload(noise)                                          # upload after synthesize
    assert dec.pool_outputs == noise.size // 2 and np.array_equal(dec.download(), noise)
    _assert_pool(dec, Y)                                       # synthesize after upload: smaller than what lay there
    dec.upload(noise[: 2 * 24])
    assert np.array_equal(dec.download(), noise[: 2 * 24])
    _assert_pool(dec, X)


def _synth_rc(dec, specs, pool_outputs, n=None):
    specs = np.ascontiguousarray(specs, SPEC_DTYPE).reshape(-1)
    return _lib.lib().rd_clips_synth(dec._h, specs.ctypes.data if specs.size else None, specs.size if n is None else n, int(pool_outputs))


def test_every_refusal_leaves_the_pool_and_a_decode_untouched():
    cfg, specs, tau, _ = _burst_case(14)
    dec = _decoder(cfg)
    L = _lib.lib()
    ms, out = C.c_float(), np.zeros(16, np.uint8)
    assert L.rd_clips_download(dec._h, out.ctypes.data, 16) == _lib.RD_ERR_STATE       # no pool yet
    assert L.rd_clips_synth_ms(dec._h, C.byref(ms)) == _lib.RD_ERR_STATE
    with pytest.raises(RuntimeError):
        dec.download()
    dec.synthesize(specs)
    pool = dec.download()
    jobs = replay.centred_jobs(specs, tau, span=40)
    before = dec.decode_jobs(jobs, 2, True, soft=True)
    took = dec.synth_ms()
    refused = SC.refused_lists()
    for what, bad_specs, bad_pool in refused:
        assert _synth_rc(dec, bad_specs, bad_pool) == _lib.RD_ERR_ARG, what
        with pytest.raises(ValueError):
            dec.synthesize(bad_specs, bad_pool)
    assert _synth_rc(dec, specs, SC.default_pool(specs), n=0) == _lib.RD_ERR_ARG
    assert _synth_rc(dec, specs, SC.default_pool(specs), n=2 ** 20 + 1) == _lib.RD_ERR_ARG
    assert _synth_rc(dec, specs[:0], 64, n=1) == _lib.RD_ERR_ARG                        # a null list
    assert _synth_rc(dec, specs, 2 ** 40 + 8) == _lib.RD_ERR_ARG                        # a pool no device holds
    assert L.rd_clips_synth(None, specs.ctypes.data, 1, 4096) == _lib.RD_ERR_ARG
    assert L.rd_clips_download(dec._h, out.ctypes.data, pool.size - 2) == _lib.RD_ERR_ARG
    assert L.rd_clips_download(dec._h, None, pool.size) == _lib.RD_ERR_ARG
    assert len(refused) >= 25 and dec.pool_outputs == pool.size // 2 and dec.synth_ms() == took
    assert np.array_equal(dec.download(), pool)
    after = dec.decode_jobs(jobs, 2, True, soft=True)
    assert after.records.tobytes() == before.records.tobytes() and after.headers.tobytes() == before.headers.tobytes()
    assert np.array_equal(after.soft, before.soft) and int(before.headers["n_msgs"].sum()) >= 2


@pytest.fixture(scope="module")
def stat_device_pool():
    specs = SC.stat_specs()
    dec = _decoder(DC.config(14, 80, 2048))
    dec.synthesize(specs)
    got = dec.download()
    assert np.array_equal(got, SC.stat_model_pool(specs))     # (and so the figures below are the model's)
    return got


def test_noise_variance_of_the_devices_bytes(stat_device_pool):
    mean, var, want = SC.stat_figures(stat_device_pool)
    print(f"device: mean {mean:.5f} variance {var:.4f} derived {want:.4f}")
    assert abs(var / want - 1.0) < 0.02, (var, want)


def test_noise_mean_of_the_devices_bytes(stat_device_pool):
    """Within 0.05 of 127.5 + 0.5: S is centred on 128 bytes and rounding half up is unbiased (clip_synth_cases.stat_figures)."""
    mean, _, _ = SC.stat_figures(stat_device_pool)
    assert abs(mean - SC.BYTE_MEAN) < 0.05, mean
