"""``Demodulator.demodulate(complex block)`` on the device against ``OracleDemodulator``: float samples, scaled samples,
complex64, silence and the reference's fallbacks, on the one-launch form (k_stream_block_cplx) and the multi-launch form
(roll_cplx, k_cplx_bits, k_window_update, k_search, k_slice_rssi<complex ring>, the k_disc / k_filt mirrors).  Inputs,
expected values and the comparison: tests/complex_input_cases.py; the conditions that make the exact comparison
legitimate: tests/test_complex_input_cpu.py.

After every call: ``quantized`` exactly, the packets' index, bytes, order and dedupe exactly, the raise, -120 / 50 with
==, RSSI / SNR within 1e-3 dB, ``filtered`` per component within 18 * 2^-53 * sum |c_m| |y_m|, ``discriminated`` within
1e-9 * max(1, |ref|).  ``python tests/test_complex_input.py`` prints the largest errors per form and class
(profiles/complex_input.txt)."""
import math

import numpy as np
import pytest

import complex_input_cases as CC

SUBMIT_CLASS = {   # the class each shape also runs through submit() / fetch() with two blocks in flight
    "davis-2048": "raise0", "davis-2144": "runs", "davis-8192": "raise1", "davis-512": "raise0", "davis-1024": "fall1",
    "davis-16384": "float", "s8-1024": "float", "s4-64": "pyrtlsdr", "s3-96": "float", "davis-8192-legacy": "raise0",
}
MODE_SHAPES = ("davis-2048", "davis-512")     # one shape of each form
CASES = [(s.name, c) for s in CC.SHAPES for c in CC.classes_of(s)]


@pytest.fixture(scope="module")
def dsp():
    from rtldavis_amd import dsp as mod
    return mod


def _handle(dsp, shape, monkeypatch=None):
    """A fresh handle; RD_STREAM_IMPL is read when its first block makes the device state."""
    if monkeypatch is not None:
        if shape.legacy:
            monkeypatch.setenv("RD_STREAM_IMPL", "legacy")
        else:
            monkeypatch.delenv("RD_STREAM_IMPL", raising=False)
    return dsp.Demodulator(dsp.PacketConfig(*shape.cfg_args()))


def _take(fn):
    try:
        return [(int(p.index), bytes(p.data).hex(), float(p.rssi), float(p.snr)) for p in fn()]
    except ValueError as e:
        assert str(e) == "math domain error", e
        return None


def _state(dem, mirrors=True):
    if not mirrors:
        return dict(quantized=None, filtered=None, discriminated=None, fbound=None)
    return dict(quantized=dem.quantized, filtered=dem.filtered, discriminated=dem.discriminated, fbound=None)


def run_demodulate(dem, blocks):
    return [CC.Call(packets=_take(lambda: dem.demodulate(blk)), **_state(dem)) for blk in blocks]


def run_pipelined(dem, blocks, submit=None):
    """submit() / fetch() with two blocks in flight; the state mirrors need a quiet handle: after the last fetch only."""
    submit = submit or (lambda b, blk: dem.submit(blk))
    out, sent = [], 0
    for b in range(len(blocks)):
        while sent < len(blocks) and dem.inflight < 2:
            submit(sent, blocks[sent])
            sent += 1
        assert dem.inflight == min(2, len(blocks) - b)
        pk = _take(dem.fetch)
        out.append(CC.Call(packets=pk, **_state(dem, mirrors=b == len(blocks) - 1)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cls", CASES, ids=[f"{s}-{c}" for s, c in CASES])
def test_demodulate_equals_the_oracle(dsp, monkeypatch, shape, cls):
    sh = CC.SHAPE[shape]
    blocks, _ = CC.stream(shape, cls)
    want = list(CC.expected(shape, cls))
    got = run_demodulate(_handle(dsp, sh, monkeypatch), blocks)
    bad = CC.compare(got, want)
    assert not bad, bad[:5]
    if SUBMIT_CLASS[shape] == cls:
        got = run_pipelined(_handle(dsp, sh, monkeypatch), blocks)
        bad = CC.compare(got, want)      # (the raise out of the right fetch: compare() holds it to its call)
        assert not bad, ("two in flight", bad[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s.name for s in CC.SHAPES if s.davis])
def test_power_of_two_twins_device_against_device(dsp, monkeypatch, shape):
    """Scaling by 2^k is exact in float64: the same bits and packets, rssi shifted by 20 log10(2^k) and snr equal within
    1e-9 dB (log10's rounding) - except a record with index 0, whose noise power is the constant 1e-9."""
    sh = CC.SHAPE[shape]
    for base_cls, twins in (("float", CC.TWINS),):
        base = run_demodulate(_handle(dsp, sh, monkeypatch), CC.stream(shape, base_cls)[0])
        for cls, k in twins.items():
            tw = run_demodulate(_handle(dsp, sh, monkeypatch), CC.stream(shape, cls)[0])
            shift = 20.0 * math.log10(2.0 ** k)
            for c, (a, b) in enumerate(zip(base, tw)):
                assert np.array_equal(a.quantized, b.quantized), (cls, c)
                assert [p[:2] for p in a.packets] == [p[:2] for p in b.packets], (cls, c)
                for p, q in zip(a.packets, b.packets):
                    assert abs(q[2] - p[2] - shift) <= 1e-9, (cls, c, p, q)
                    assert abs(q[3] - p[3]) <= 1e-9 or p[0] == 0, (cls, c, p, q)
                assert np.array_equal(b.filtered, a.filtered * 2.0 ** k), (cls, c)
    # the index-0 exception is exercised: the edges case, scaled here
    blocks = CC.stream(shape, "edges")[0]
    a = run_demodulate(_handle(dsp, sh, monkeypatch), blocks)
    b = run_demodulate(_handle(dsp, sh, monkeypatch), [blk * 2.0 ** -9 for blk in blocks])
    seen0 = False
    for ca, cb in zip(a, b):
        assert np.array_equal(ca.quantized, cb.quantized) and [p[:2] for p in ca.packets] == [p[:2] for p in cb.packets]
        for p, q in zip(ca.packets, cb.packets):
            shift = 20.0 * math.log10(2.0 ** -9)
            assert abs(q[2] - p[2] - shift) <= 1e-9
            if p[0] == 0:
                seen0 = True
                assert abs(q[3] - p[3] - shift) <= 1e-9      # signal over the constant 1e-9
            else:
                assert abs(q[3] - p[3]) <= 1e-9
    assert seen0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MODE_SHAPES)
def test_mode_changes_and_reset(dsp, monkeypatch, shape):
    """uint8 blocks, then complex blocks (the byte ring converted once: history carries over), then a uint8 block on the
    handle in complex mode (through the LUT), then reset() and the first blocks again."""
    sh = CC.SHAPE[shape]
    seq, _ = CC.mode_change_blocks(shape)
    blocks = [b for b, _ in seq]
    want = CC.oracle_calls(sh.ocfg(), blocks)
    dem = _handle(dsp, sh, monkeypatch)
    first_c = [c for _, c in seq].index(True)
    got = run_demodulate(dem, blocks)
    # before the first complex block the handle is on the uint8 path, whose mirrors have their own tests and tolerances
    for c in range(first_c):
        got[c] = got[c]._replace(filtered=None, discriminated=None)
    bad = CC.compare(got, want)
    assert not bad, bad[:5]
    dem.reset()
    assert not dem.quantized.any() and not dem.filtered.any() and not dem.discriminated.any()
    again = run_demodulate(dem, blocks[:first_c + 1])
    for c in range(first_c):
        again[c] = again[c]._replace(filtered=None, discriminated=None)
    bad = CC.compare(again, want[:first_c + 1])
    assert not bad, ("after reset", bad[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cls", [("davis-2048", "raise1"), ("davis-512", "runs"), ("davis-8192", "float")])
def test_submit_from_a_registered_buffer(dsp, monkeypatch, shape, cls):
    """register_input / submit_from(offset, B, is_complex=True) on the complex blocks viewed as bytes, two in flight: the
    lists demodulate() gives."""
    sh = CC.SHAPE[shape]
    B = sh.B
    blocks, _ = CC.stream(shape, cls)
    want = list(CC.expected(shape, cls))
    store = np.zeros(16 * B * len(blocks) + 4096, dtype=np.uint8)
    skip = (-store.ctypes.data) % 4096
    buf = store[skip: skip + 16 * B * len(blocks)]
    buf.view(np.complex128)[:] = np.concatenate(blocks)
    dem = _handle(dsp, sh, monkeypatch)
    dem.register_input(buf)
    try:
        with pytest.raises(ValueError):
            dem.submit_from(0, 2 * B, is_complex=True)
        got = run_pipelined(dem, blocks, submit=lambda b, blk: dem.submit_from(16 * B * b, B, is_complex=True))
    finally:
        dem.register_input(None)
    bad = CC.compare(got, want)
    assert not bad, bad[:5]


def measure():
    """The largest errors against the oracle per form and input class, over every shape of the form."""
    from rtldavis_amd import dsp as mod
    import os
    print("form   class        |dB err|   filtered / bound   discriminated / max(1,|ref|)")
    for form in ("one", "multi"):
        for cls in CC.CLASSES_DAVIS:
            err = CC.Errors()
            for sh in CC.SHAPES:
                if sh.form != form or cls not in CC.classes_of(sh):
                    continue
                if sh.legacy:
                    os.environ["RD_STREAM_IMPL"] = "legacy"
                else:
                    os.environ.pop("RD_STREAM_IMPL", None)
                got = run_demodulate(mod.Demodulator(mod.PacketConfig(*sh.cfg_args())), CC.stream(sh.name, cls)[0])
                bad = CC.compare(got, list(CC.expected(sh.name, cls)), err)
                assert not bad, (sh.name, cls, bad[:3])
            print(f"{form:6s} {cls:12s} {err.db:9.3e}  {err.filt * 18:9.3f} of 18 ulp  {err.disc:9.3e}")


if __name__ == "__main__":
    measure()
