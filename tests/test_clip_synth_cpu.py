"""The host's share of the clip synthesiser (include/rtldavis_hip.h, CLIP SYNTH: rd_cs_check_specs and rd_cs_table in
rd_host.cpp, burst_specs in rtldavis_amd/replay.py) and the NumPy model of tests/clip_synth_cases.py itself: its Philox
against the known answers, its moments, its table, and for every mutant of the model a named case that tells it apart.
No device."""
import ctypes as C

import numpy as np
import pytest

import burst_decode_cases as DC
import clip_replay_cases as RC
import clip_synth_cases as SC
from rtldavis_amd import _lib, replay
from rtldavis_amd.replay import SPEC_DTYPE


def c_check(specs, pool_outputs, n=None):
    specs = np.ascontiguousarray(specs, SPEC_DTYPE).reshape(-1)
    bad, why = C.c_int(99), C.c_char_p()
    rc = _lib.lib().rd_cs_check_specs(specs.ctypes.data, specs.size if n is None else n, pool_outputs, C.byref(bad), C.byref(why))
    assert why.value is not None and bool(why.value) == (rc != 0)
    return rc, bad.value


def test_symbols_and_layout():
    L = _lib.lib()
    for name in ("rd_clips_synth", "rd_clips_download", "rd_clips_synth_ms", "rd_cs_check_specs", "rd_cs_table"):
        assert hasattr(L, name)
    assert SPEC_DTYPE.itemsize == 80 and SPEC_DTYPE.fields["bits"][1] == 56 and SPEC_DTYPE.fields["pad"][1] == 52


def test_philox_known_answers():
    got = SC.philox((0, 0, 0, 0), (0, 0))
    assert [int(w) for w in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = SC.philox((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    assert [int(w) for w in got] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    many = SC.philox((np.arange(5), 1, 0, 0), (7, 9))         # arrays give what single calls give
    for t in range(5):
        assert [int(w[t]) for w in many] == [int(w) for w in SC.philox((t, 1, 0, 0), (7, 9))]


def test_model_moments():
    """g over 2 x 10^5 outputs: mean 0 +- 4 sigma / sqrt(n), the derived deviation within 1 %, the kurtosis of a sum of 16
    uniform bytes (3 - 1.2 / 16 = 2.925) within 0.05, I / Q and lag-1 correlation below 0.01."""
    n = 100000
    g = SC.noise_g(np.arange(n)[:, None], np.arange(2)[None, :], 2024).astype(np.float64)
    assert g.min() >= -2040 and g.max() <= 2040
    assert abs(g.mean()) < 4 * SC.SIGMA_G / np.sqrt(2 * n) and abs(g.std() / SC.SIGMA_G - 1) < 0.01
    z = (g - g.mean()) / g.std()
    assert abs((z ** 4).mean() - 2.925) < 0.05
    assert abs((z[:, 0] * z[:, 1]).mean()) < 0.01 and abs((z[1:, 0] * z[:-1, 0]).mean()) < 0.01
    assert abs(SC.SIGMA_G - 295.601) < 1e-3 and abs(replay.NOISE_SIGMA * 2 ** 22 - SC.SIGMA_G) < 1e-9


def test_table_equals_the_librarys_and_its_symmetries():
    got = np.zeros(4096, np.int16)
    _lib.lib().rd_cs_table(got.ctypes.data)
    T = SC.TABLE
    assert np.array_equal(got.astype(np.int64), T)
    assert T[0] == 16384 and T[1024] == 0 and T[2048] == -16384 and T[3072] == 0
    j = np.arange(1, 4096)
    assert np.array_equal(T[j], T[4096 - j]) and np.array_equal(T[(j + 2048) % 4096], -T[j])
    assert np.abs(T - 16384 * np.cos(2 * np.pi * np.arange(4096) / 4096)).max() <= 0.5


@pytest.mark.parametrize("sl", (3, 4, 14, 51))
def test_burst_specs_round_trip(sl):
    """A noise-free clip of burst_specs decodes to its planted payload at the returned position, through the decoder's model."""
    n_sym = 80 if sl * 80 + 1 <= 2048 else 40
    datas = [DC.packet(n_sym, ident=k + 1, seed=5200 + k) for k in range(2)]
    n = (32 + n_sym + 8) * sl + 333
    specs, tau = replay.burst_specs(datas, n=n, at=[100, 131], seed=5, amplitude=0.3, noise=0.0, offset_hz=[900.0, -1500.0],
                                    symbol_length=sl)
    assert SC.check_specs(specs, SC.default_pool(specs)) == (0, -1) and c_check(specs, SC.default_pool(specs)) == (0, -1)
    assert specs["offset"].tolist() == [0, (n + 7) // 8 * 8] and tau.tolist() == [100 + 33 * sl - 1, 131 + 33 * sl - 1]
    dec = replay.ClipDecoder(DC.config(sl, n_sym, 2048))
    jobs = replay.centred_jobs(specs, tau, span=20, corr=[dec.corr(900.0), dec.corr(-1500.0)])
    for k in range(2):
        row, hdr, _ = RC.decode_job(SC.clip_bytes(specs[k], sl), jobs[k], k, sl, n_sym, 0, False)
        assert hdr[0] == 1 and hdr[1] == 21 and int(row[2]) == int(tau[k]), (sl, k, hdr, row)
        rec = np.zeros(1, replay.BURST_MSG_DTYPE)
        rec[0] = row
        assert bytes(rec[0]["data"][: n_sym // 8]) == datas[k]
    own = replay.centred_jobs(specs, tau, span=20)             # the clip's own direction finds it too
    assert RC.decode_job(SC.clip_bytes(specs[0], sl), own[0], 0, sl, n_sym, 0, False)[1][0] == 1


def test_burst_specs_units_and_refusals():
    data = DC.packet(80, seed=1)
    s, tau = replay.burst_specs([data], n=2048, at=300, seed=9, amplitude=0.3, noise=0.2)
    assert int(s["amp_q"][0]) == round(0.3 * 127.6 * 256) and int(s["noise_q"][0]) == round(0.2 * 127.6 * 2 ** 22 / SC.SIGMA_G)
    assert int(s["f_c"][0]) == -2 ** 30 and int(s["f_d"][0]) == round(2 ** 32 / 56) and int(s["n_sym"][0]) == 120
    assert SC.symbols_of(s[0])[:32].tolist() == [1, 0] * 16 and np.packbits(SC.symbols_of(s[0])[32:112]).tobytes() == data
    assert not SC.symbols_of(s[0])[112:].any() and int(tau[0]) == 300 + 33 * 14 - 1
    again, _ = replay.burst_specs([data], n=2048, at=300, seed=9, amplitude=0.3, noise=0.2)
    other, _ = replay.burst_specs([data], n=2048, at=300, seed=10, amplitude=0.3, noise=0.2)
    assert again.tobytes() == s.tobytes() and other["seed"][0] != s["seed"][0]
    q, _ = replay.burst_specs(None, count=5, n=100, at=0, seed=3, amplitude=0.7, noise=0.1)
    assert q.size == 5 and not q["amp_q"].any() and not q["n_sym"].any() and len(set(q["seed"].tolist())) == 5
    assert q["offset"].tolist() == [0, 104, 208, 312, 416] and c_check(q, 516) == (0, -1)
    for kw in (dict(n=0), dict(n=2 ** 24 + 1), dict(at=2 ** 30 + 1), dict(amplitude=2.1), dict(noise=0.8), dict(noise=-0.1),
               dict(pre=4097), dict(post=-1), dict(lead_symbols=105), dict(seed=[1, 2])):
        args = dict(n=2048, at=300, seed=9, amplitude=0.3, noise=0.2)
        args.update(kw)
        with pytest.raises(ValueError):
            replay.burst_specs([data], **args)
    with pytest.raises(ValueError):
        replay.burst_specs(None, n=100, at=0, seed=3, amplitude=0.0, noise=0.1)
    with pytest.raises(ValueError):
        replay.burst_specs([data, data[:5]], n=2048, at=300, seed=9, amplitude=0.3, noise=0.2)


def test_cases_hold_and_every_refusal_is_the_librarys():
    for X in SC.exact_cases() + [SC.random_case()]:
        assert c_check(X.specs, X.pool_outputs) == (0, -1), X.name
    for what, specs, pool in SC.refused_lists():
        want = SC.check_specs(specs, pool)
        assert c_check(specs, pool) == want and want[0] == -1, what
    one = SC.lay_out([SC.spec_row(8)])
    L = _lib.lib()
    for n in (0, -1, 2 ** 20 + 1):
        assert c_check(one, 8, n) == (-1, -1)
    assert L.rd_cs_check_specs(None, 1, 8, None, None) == _lib.RD_ERR_ARG
    assert L.rd_cs_check_specs(one.ctypes.data, 1, 8, None, None) == _lib.RD_OK
    assert c_check(one, 7) == (-1, 0)


def test_random_lists_equal_the_restatement():
    rng = np.random.default_rng(5300)
    edge = dict(SC.REFUSALS, offset=(4, 2 ** 64 - 8, 0), n=(0, 2 ** 24, 2 ** 24 + 1), at=(-2 ** 30, 2 ** 30, 2 ** 30 + 1), f_d=(2 ** 31 - 1, 2 ** 31),
                amp_q=(2 ** 16, 2 ** 16 + 1), noise_q=(2 ** 20, 2 ** 20 + 1), n_sym=(192, 193, 0), pre=(4096, 4097))
    n_ok = n_bad = 0
    for _ in range(400):
        k = int(rng.integers(1, 7))
        rows = [SC.spec_row(int(rng.integers(1, 200)), at=int(rng.integers(-50, 50)), sym=rng.integers(0, 2, int(rng.integers(0, 193))),
                            seed=int(rng.integers(0, 1000))) for _ in range(k)]
        specs = SC.lay_out(rows, gaps=rng.integers(0, 3, k))
        pool = SC.default_pool(specs) + int(rng.integers(-8, 9))
        kind = int(rng.integers(0, 4))
        i = int(rng.integers(0, k))
        if kind == 1:
            f = list(edge)[int(rng.integers(0, len(edge)))]
            specs[i][f] = edge[f][int(rng.integers(0, len(edge[f])))]
        elif kind == 2:
            specs[i]["bits"][int(rng.integers(0, 24))] |= 1 << int(rng.integers(0, 8))
        elif kind == 3 and k > 1:
            specs[i]["offset"] = max(0, int(specs[i - 1]["offset"]) + 8 * int(rng.integers(-2, 3))) if i else specs[1]["offset"]
        want = SC.check_specs(specs, max(pool, 0))
        assert c_check(specs, max(pool, 0)) == want, (specs, pool)
        n_ok += want[0] == 0
        n_bad += want[0] != 0
    assert n_ok >= 60 and n_bad >= 120, (n_ok, n_bad)


MUTANT_CASES = {"nine_rounds": ("levels", 0), "iq_noise_swapped": ("levels", 0), "sine_wrong_way": ("levels", 1),
                "symbol_off_by_one": ("levels", 1), "round_half_down": ("phase", 8), "no_clamp": ("levels", 3), "phase_at_u": ("levels", 1),
                "noise_by_pool_position": ("seeds", 4)}


@pytest.mark.parametrize("mutant", SC.MUTANTS)
def test_a_named_case_tells_each_mutant_apart(mutant):
    """Each wrong reading of the definition changes the bytes of a named clip - and the reading without a mutant does not."""
    assert set(MUTANT_CASES) == set(SC.MUTANTS) and len(SC.MUTANTS) >= 8
    cases = {X.name: X for X in SC.exact_cases()}
    name, k = MUTANT_CASES[mutant]
    X = cases[name]
    good = SC.clip_bytes(X.specs[k], X.sl)
    assert np.array_equal(good, X.clip(k))
    assert not np.array_equal(SC.clip_bytes(X.specs[k], X.sl, mutant), good), mutant


def test_round_half_up_is_exercised_exactly():
    """S exactly on a half goes up: 128 + 1/2 is 129; 128 + 1 and 128 itself are what they are under either rounding."""
    h = SC.spec_row(64, at=0, sym=[1] * 4, amp_q=128, phase0=0)          # S = 128 + 128 x 16384 / 2^22 = 128.5 bytes
    assert SC.clip_bytes(h, 14)[0] == 129 and SC.clip_bytes(h, 14, "round_half_down")[0] == 128
    s = SC.spec_row(64, at=0, sym=[1] * 4, amp_q=256, phase0=0)          # 129 exactly
    assert SC.clip_bytes(s, 14)[0] == 129 and SC.clip_bytes(s, 14, "round_half_down")[0] == 129
    assert SC.clip_bytes(SC.spec_row(8), 14).tolist() == [128] * 16 == SC.clip_bytes(SC.spec_row(8), 14, "round_half_down").tolist()


@pytest.fixture(scope="module")
def stat_pool():
    specs = SC.stat_specs()
    pool = SC.stat_model_pool(specs)
    for k in (0, 77, SC.STAT_CLIPS - 1):                       # the batched evaluation is the model's
        assert np.array_equal(pool[2 * SC.STAT_N * k: 2 * SC.STAT_N * (k + 1)], SC.clip_bytes(specs[k], 14))
    assert pool.min() > 128 - 8 * SC.STAT_SIGMA and pool.max() < 128 + 8 * SC.STAT_SIGMA      # no clamp takes part
    return pool


def test_statistical_variance_bound_holds_on_the_model(stat_pool):
    """The variance condition test_clip_synth.py puts to the device's bytes is one the model meets with margin, same seeds."""
    mean, var, want = SC.stat_figures(stat_pool)
    print(f"model: mean {mean:.5f} variance {var:.4f} derived {want:.4f}")
    assert abs(var / want - 1.0) < 0.02 and abs(var / want - 1.0) < 0.01, (var, want)


def test_statistical_mean_bound_holds_on_the_model(stat_pool):
    """The mean condition test_clip_synth.py puts to the device's bytes - within 0.05 of 127.5 + 0.5 - is one the model meets
    with margin (within half of it), same seeds."""
    mean, _, _ = SC.stat_figures(stat_pool)
    assert abs(mean - SC.BYTE_MEAN) < 0.05 and abs(mean - SC.BYTE_MEAN) < 0.025, mean
