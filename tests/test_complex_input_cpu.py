"""The complex-input cases (tests/complex_input_cases.py) on the CPU: the conditions under which comparing the device
with the oracle bit for bit is legitimate, that every case produces what it is for, which launch form each shape takes,
and a float64 restatement of the path with the faults it must be told apart from.  tests/test_complex_input.py runs the
same cases on the device."""
import os
import re

import numpy as np
import pytest

import complex_input_cases as CC
from oracle import dsp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(s.name, c) for s in CC.SHAPES if not s.legacy for c in CC.classes_of(s)]
DAVIS = [s.name for s in CC.SHAPES if s.davis and not s.legacy]
MODE_SHAPES = ("davis-2048", "davis-512")


def _packets(want):
    return [(c, p) for c, w in enumerate(want) if w.packets for p in w.packets]


def test_each_shape_takes_the_form_it_is_listed_under():
    """The form-selection rule restated (rd_stream.hip: one_ok, one_cplx; rd_stream_kernels.hip:
    rd_launch_stream_block_cplx), applied to the table; both forms and every reason for the multi-launch form occur."""
    for s in CC.SHAPES:
        assert CC.takes_one_launch(s.S, s.P, s.K, s.preamble, s.B, s.legacy) == (s.form == "one"), s.name
        oc = s.ocfg()
        assert oc.buffer_length == (s.K * s.S // s.B + 2) * s.B
    one = [s.B for s in CC.SHAPES if s.form == "one"]
    assert sorted(one) == [2048, 2144, 8192]
    assert [-(-b // CC.PIECE) for b in sorted(one)] == [1, 2, 4] and 2144 % CC.PIECE != 0
    multi = {s.name: s for s in CC.SHAPES if s.form == "multi"}
    assert multi["davis-512"].ocfg().buffer_length == 4 * 512 and multi["davis-1024"].ocfg().buffer_length == 3 * 1024
    assert multi["davis-16384"].ocfg().buffer_length == 2 * 16384      # declined for its size alone
    assert multi["davis-8192-legacy"].legacy and CC.takes_one_launch(14, 16, 80, CC.DAVIS_PRE, 8192, False)
    assert {(s.S, s.P, s.K, s.B) for s in CC.SHAPES if not s.davis} == {(8, 16, 80, 1024), (4, 4, 12, 64), (3, 6, 200, 96)}
    # the numbers the rule restates, where the sources spell them
    src = lambda f: open(os.path.join(ROOT, "rtldavis_amd", "csrc", f)).read()   # noqa: E731
    assert re.search(r"c\.B < 2048 \|\| c\.B > 8192", src("rd_stream_kernels.hip"))
    assert re.search(r"c\.B >= 2048 && c\.B <= 16384", src("rd_stream.hip")) and "h->dc.B <= 8192" in src("rd_stream.hip")
    assert re.search(r"define RD_SBC_THREADS 256\b", src("rd_internal.h")) and CC.PIECE == 8 * 256


@pytest.mark.parametrize("shape,cls", ALL, ids=[f"{s}-{c}" for s, c in ALL])
def test_the_oracle_sign_is_certain_at_every_position(shape, cls):
    """Exact comparison of ``quantized`` is legitimate: at every t the numerator is an exact signed zero, or it stands
    1024 summation bounds away from zero.  No position is excluded."""
    blocks, _ = CC.stream(shape, cls)
    ok, zero, margin = CC.certainty(CC.widened(blocks))
    assert ok.all(), (int((~ok).sum()), int(np.flatnonzero(~ok)[0]), float(margin[~ok].min()))
    f, d, bits = O.demod_stream_oneshot(CC.widened(blocks))
    assert np.array_equal(np.concatenate([w.quantized[-CC.SHAPE[shape].B:] for w in CC.expected(shape, cls)]), bits)


@pytest.mark.parametrize("shape", MODE_SHAPES)
def test_the_mode_change_stream_is_certain_too(shape):
    seq, x = CC.mode_change_blocks(shape)
    ok, _, margin = CC.certainty(x)
    assert ok.all(), float(margin[~ok].min())
    kinds = [c for _, c in seq]
    assert kinds[0] is False and kinds[1] is False and True in kinds and kinds[-1] is False and kinds[-2] is True
    want = CC.oracle_calls(CC.SHAPE[shape].ocfg(), [b for b, _ in seq])
    first_c = kinds.index(True)
    assert any(w.packets for w in want[first_c:]), "no packet after the change to complex input"


@pytest.mark.parametrize("shape", [s.name for s in CC.SHAPES if not s.legacy])
def test_plain_classes_report_their_bursts(shape):
    """``pyrtlsdr`` and ``float`` (and c64): both bursts' packets come out, in different calls.  At 3 and 4 samples per
    symbol the nine taps span two or three symbols and a planted packet need not survive: there, packets in several
    calls."""
    sh = CC.SHAPE[shape]
    for cls in CC.CLASSES_ANY + (("c64", "c64s") if sh.davis else ()):
        want = CC.expected(shape, cls)
        if sh.S < 8:
            assert len({c for c, _ in _packets(want)}) >= 2 and len(_packets(want)) >= 3, cls
            continue
        nbytes = (sh.K + 7) // 8
        calls = {}
        for k in range(2):
            ota = CC.packet_bytes(sh, k)[:nbytes]
            calls[k] = [c for c, p in _packets(want) if CC._same_packet(bytes.fromhex(p[1]), ota, sh.K)]
            assert calls[k], (cls, k)
        assert calls[0][0] < calls[1][0], (cls, calls)
    if sh.davis:
        raw = CC.stream(shape, "pyrtlsdr")[0]
        assert raw[0].dtype == np.complex128
        # pyrtlsdr's order of operations (a complex array divided in place, then the subtraction), not one of the
        # suite's tables
        k = np.arange(256.0)
        got = np.unique(np.concatenate(raw).real)
        table = k / 127.5 - 1.0
        assert got.size <= 256 and np.abs(got - table[np.searchsorted(table, got - 1e-9)]).max() < 1e-15
        assert not np.isin(got, (k - 127.5) / 127.5).all() and not np.isin(got, (k - 127.4) / 127.6).any()
        c64, c64s = CC.stream(shape, "c64")[0], CC.stream(shape, "c64s")[0]
        assert c64[0].dtype == np.complex64 and c64[0].flags["C_CONTIGUOUS"]
        assert c64s[0].dtype == np.complex64 and c64s[0].strides == (16,) and not c64s[1].flags["C_CONTIGUOUS"]
        assert np.array_equal(np.concatenate(c64), np.concatenate(c64s))
        fl = np.concatenate(CC.stream(shape, "float")[0])
        assert (np.concatenate(c64).astype(np.complex128) != fl).mean() > 0.99    # full mantissas: the rounding shows
        assert np.unique(fl.real).size == fl.size and (np.abs(fl) > 0).all()


@pytest.mark.parametrize("shape", DAVIS)
def test_twins_and_small_scales(shape):
    """Power-of-two twins give the oracle the same bits and packets as ``float``, RSSI shifted and SNR equal (but for an
    index-0 record, whose noise power is the constant 1e-9).  The scales near the discriminator's epsilon put the
    preamble's |f|^2 within a factor 100 of 1e-10 (x2^-17 and x1e-5; x2^-20 with amplitude 0.5 lies at 2.3e-13, under it by
    more: there epsilon IS the denominator)."""
    base = CC.expected(shape, "float")
    for cls, k in CC.TWINS.items():
        tw = CC.expected(shape, cls)
        for c, (a, b) in enumerate(zip(base, tw)):
            assert np.array_equal(a.quantized, b.quantized), (cls, c)
            assert [p[:2] for p in a.packets] == [p[:2] for p in b.packets], (cls, c)
            for p, q in zip(a.packets, b.packets):
                assert abs(q[2] - p[2] - 20 * np.log10(2.0 ** k)) < 1e-9 and (abs(q[3] - p[3]) < 1e-9 or p[0] == 0), (cls, c, p, q)
            assert np.array_equal(b.filtered, a.filtered * 2.0 ** k)
    sh = CC.SHAPE[shape]
    start = CC.stream(shape, "float")[1]["starts"][0] + CC.lead_in(sh)
    for cls in CC.SCALES:
        f, d, _ = O.demod_stream_oneshot(CC.widened(CC.stream(shape, cls)[0]))
        p = float(np.mean(np.abs(f[start + 20: start + 20 + 224]) ** 2))
        print(f"\n[complex-input] {shape} {cls}: preamble |f|^2 = {p:.3g}")
        if cls in CC.NEAR_EPSILON:
            assert 1e-12 <= p <= 1e-8, (cls, p)
        elif cls == "x2^-20":
            assert p < 1e-12       # (0.5 * 2^-20)^2: epsilon outweighs it 400 times
    # at those scales epsilon decides discriminated: without it the values differ by far more than the tolerance
    x = CC.widened(CC.stream(shape, "x1e-5")[0])
    f, d, _ = O.demod_stream_oneshot(x)
    fp = np.concatenate([[0j], f])
    with np.errstate(all="ignore"):
        bare = (fp.imag[:-1] * fp.real[1:] - fp.real[:-1] * fp.imag[1:]) / (np.abs(fp[:-1]) ** 2)
    assert np.nanmedian(np.abs(bare[start: start + 224] / d[start: start + 224])) > 2.0


@pytest.mark.parametrize("shape", DAVIS)
def test_silence_cases_produce_what_they_are_for(shape):
    sh = CC.SHAPE[shape]
    B = sh.B
    for cls in ("raise0", "raise1", "fall0", "fall1"):
        blocks, meta = CC.stream(shape, cls)
        want = CC.expected(shape, cls)
        rc = meta["report_call"]
        assert not np.concatenate(blocks)[rc * B:(rc + 1) * B].any() and rc + 1 < sh.nb
        assert np.concatenate(blocks)[(rc + 1) * B:].all()          # the stream goes on behind the silent block
        if cls.startswith("raise"):
            assert want[rc].packets is None and all(w.packets is not None for c, w in enumerate(want) if c != rc), cls
        else:
            assert want[rc].packets and all(p[2:] == (-120.0, 50.0) for p in want[rc].packets), (cls, want[rc].packets)
            assert all(w.packets is not None for w in want)
        # the call after the report is not trivially empty of state: its window still holds the burst's bits
        assert want[rc + 1].quantized.any()
    # edges: a record with index 0 (noise power = 1e-9), one whose signal window is clipped at B + 1
    pk = [p for _, p in _packets(CC.expected(shape, "edges"))]
    assert any(p[0] == 0 for p in pk) and any(B + 1 - 224 < p[0] <= B for p in pk)
    # zero runs: every length in burst and in noise; one over a block boundary, one over sample 2048 of a block
    for cls in ("runs", "runs-0"):
        blocks, meta = CC.stream(shape, cls)
        x = np.concatenate(blocks)
        runs = meta["runs"]
        b0, b1 = meta["starts"][0], meta["starts"][0] + CC.burst_len(sh)
        inside = sorted(n for s, n in runs if b0 <= s and s + n <= b1)
        outside = sorted(n for s, n in runs if s >= meta["starts"][-1] + CC.burst_len(sh))
        assert inside == sorted(CC.RUN_LENGTHS) and outside == sorted(CC.RUN_LENGTHS)
        for s, n in runs:
            assert not x[s:s + n].any() and x[s - 1] != 0 and x[s + n] != 0
            assert bool(np.signbit(x[s:s + n].real).all() and np.signbit(x[s:s + n].imag).all()) == (cls == "runs-0")
        assert any(s // B != (s + n - 1) // B for s, n in runs)
        if B > CC.PIECE:
            assert any(s % B < CC.PIECE <= (s + n - 1) % B and s // B == (s + n - 1) // B for s, n in runs)
        _, zero, _ = CC.certainty(x)
        # f is exactly zero where all nine samples under the taps are: n - 8 outputs of a run of n, n - 7 numerators
        assert zero.sum() == 2 + sum(n - 7 for _, n in runs if n >= 9)
        assert _packets(CC.expected(shape, cls))
    blocks, meta = CC.stream(shape, "zero-first")
    assert not blocks[0].any() and blocks[1].all() and _packets(CC.expected(shape, "zero-first"))
    blocks, meta = CC.stream(shape, "zero-gap")
    g = meta["zero_blocks"][0]
    assert not blocks[g].any() and meta["starts"][0] + CC.burst_len(sh) <= g * B < (g + 1) * B <= meta["starts"][1]
    assert any(c > g for c, _ in _packets(CC.expected(shape, "zero-gap")))
    # a zero numerator with the sign bit set occurs (what IEEE's sign rules decide, not rounding)
    n_neg = 0
    for cls in ("runs", "runs-0", "zero-gap", "raise0"):
        x = CC.widened(CC.stream(shape, cls)[0])
        _, d, bits = O.demod_stream_oneshot(x)
        n_neg += int(((d == 0) & (bits == 1)).sum())
    assert n_neg > 0


@pytest.mark.parametrize("shape", [s.name for s in CC.SHAPES if not s.legacy])
def test_the_restated_path_agrees_with_the_oracle(shape):
    """The float64 restatement (rotation on signs, taps in order from +0.0, the numerator's sign, windows clipped to
    B + 1, the three fallbacks and the raise) against OracleDemodulator on every case, at the device's tolerances."""
    sh = CC.SHAPE[shape]
    for cls in CC.classes_of(sh):
        bad = CC.compare(CC.model_calls(sh.ocfg(), CC.stream(shape, cls)[0]), list(CC.expected(shape, cls)))
        assert not bad, (cls, bad[:3])
    if shape in MODE_SHAPES:
        seq, _ = CC.mode_change_blocks(shape)
        blocks = [b for b, _ in seq]
        assert not CC.compare(CC.model_calls(sh.ocfg(), blocks), CC.oracle_calls(sh.ocfg(), blocks))


# mutant -> the named cases that must tell it apart (shape, class)
MUTANT_PLAN = {
    "no_epsilon": [("davis-2048", "x1e-5"), ("davis-512", "x2^-17"), ("davis-8192", "zero-gap")],
    "piece_phase": [("davis-2048", "float"), ("davis-8192", "pyrtlsdr")],
    "no_block_history": [("davis-2048", "float"), ("davis-512", "pyrtlsdr"), ("s4-64", "float")],
    "no_seam_history": [("davis-2144", "float"), ("davis-8192", "float"), ("davis-8192", "runs")],
    "zero_is_plus": [("davis-8192", "runs"), ("davis-2048", "runs-0")],
    "clip_at_B": [("davis-2048", "edges"), ("davis-8192", "edges"), ("davis-512", "edges")],
    "noise_fallback_0": [("davis-2048", "edges"), ("davis-1024", "edges")],
    "never_raise": [("davis-8192", "raise0"), ("davis-2144", "raise1"), ("davis-512", "raise0")],
    "c64_rounded_again": [("davis-2048", "c64"), ("davis-8192", "c64s")],
}


@pytest.mark.parametrize("mutant", sorted(CC.MUTANTS))
def test_every_mutant_is_told_apart(mutant):
    """Each fault, applied to the restatement, differs from the oracle on every case named for it - by the comparison the
    device test makes."""
    assert set(MUTANT_PLAN) == set(CC.MUTANTS)
    for shape, cls in MUTANT_PLAN[mutant]:
        sh = CC.SHAPE[shape]
        bad = CC.compare(CC.model_calls(sh.ocfg(), CC.stream(shape, cls)[0], mutant), list(CC.expected(shape, cls)))
        print(f"\n[complex-input-mutant] {mutant} ({CC.MUTANTS[mutant]}): told apart by {shape} {cls}: {bad[0] if bad else 'NOT'}")
        assert bad, (mutant, shape, cls)
