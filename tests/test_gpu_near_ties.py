"""k_demod_mfma under stress: the planted near-ties of tests/near_tie_cases.py (what they are and what the model says about
them is checked on the CPU, tests/test_near_tie_cpu.py) through the kernel alone - both the instantiation that dumps g
and the one the product launches - and through every path that inherits its bits: the batch path with either tail, the
streaming Demodulator fed bytes and fed complex samples.

The list assertions need no tolerance: the generator keeps every group's guard value at least 1e-5 (relative) away from its
threshold, the kernel's g equals the integer model bit for bit, and every later operation is a single fp32 operation."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import near_tie_cases as NT  # noqa: E402
import test_gpu_mfma as TM  # noqa: E402  (run_kernel / check: shared, not copied)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 8192
PREAMBLE = "1100101110001001"


def _through_the_hook(c, want_g):
    """TM.check: g = the integer model bit for bit (want_g), no wrong sign outside the list against the oracle, zero bits
    past a ragged end, the forced entries.  Then the list itself against the fp32 model."""
    fix, _, words = TM.check(c.streams, c.hist, want_g=want_g, want_bits=True)
    ns, n = c.streams.shape[0], c.n
    nw = (n + 31) // 32
    assert (fix & 15 != 0).all(), "an entry with an empty group mask"
    listed, dup = NT.listed_groups(fix, ns, nw)
    # n_fix = the entries returned (run_kernel cuts the array at n_fix; its capacity is one entry per word, so a list
    # without duplicates fits): every one names a different word
    assert np.unique(fix >> 4).size == fix.size
    fast = np.unpackbits(words.view(np.uint8), bitorder="little").reshape(ns, -1)[:, :n]
    NT.check_list(c, listed, fast, dup)
    flagged_words = int(c.flagged_words().sum())
    print(f"{c.name}: {fix.size} entries, {flagged_words} words the model flags, "
          f"{int(((fast != c.bits) & np.repeat(c.valid, 8, axis=1)).sum())} wrong fast signs, all listed")


@pytest.mark.parametrize("name", NT.NAMES)
def test_list_and_signs_with_g(name):
    _through_the_hook(NT.case(name), True)


@pytest.mark.parametrize("name", NT.NAMES)
def test_list_and_signs_product_instantiation(name):
    _through_the_hook(NT.case(name), False)


# ---------------------------------------------------------------------------------------------------------------------
def _batch_input(c):
    """The case as whole blocks for the batch path: history in front (the batch path starts every stream from the zero
    state), the byte 127 behind.  Returns (raw [ns, 2 * BLOCK * nb], offset of the case's sample 0)."""
    st = c.streams if c.hist is None else np.concatenate([c.hist, c.streams], axis=1)
    off = 0 if c.hist is None else c.hist.shape[1] // 2
    ns, nbytes = st.shape
    nb = (nbytes // 2 + BLOCK - 1) // BLOCK
    raw = np.full((ns, 2 * BLOCK * nb), 127, dtype=np.uint8)
    raw[:, :nbytes] = st
    return raw, off


def _check_batch(c, bits_of, packets, overflowed):
    from oracle import c_oracle as CO
    raw, off = _batch_input(c)
    want, wbits = CO.demod_batch(raw, CO.make_cfg(), threads=4, want_bits=True)
    for i in range(raw.shape[0]):
        got = np.unpackbits(np.asarray(bits_of(i)).view(np.uint8), bitorder="little")
        assert np.array_equal(got[off: off + c.n], c.bits[i]), f"{c.name} stream {i}: bits differ from the exact integers"
        assert np.array_equal(np.asarray(bits_of(i)), wbits[i]), f"{c.name} stream {i}: bits differ from the C oracle"
        assert packets[i] == [(p.call, p.index, bytes(p.data).hex()) for p in want[i]], (c.name, i)
    print(f"{c.name}: batch path exact; second pass (a bucket overflowed into the fallback): {overflowed}")


@pytest.mark.parametrize("name", NT.NAMES)
def test_batch_path_one_launch_tail(name):
    from rtldavis_amd import batch, dsp
    c = NT.case(name)
    raw, _ = _batch_input(c)
    bd = batch.BatchDemodulator(dsp.PacketConfig(19200, 14, 16, 80, PREAMBLE, BLOCK), raw.shape[0], raw.shape[1] // (2 * BLOCK))
    res = bd.demodulate(raw)
    forms = bd.last_run_forms()
    pk = [[(cc, p.index, bytes(p.data).hex()) for cc, ps in enumerate(res[i]) for p in ps] for i in range(raw.shape[0])]
    _check_batch(c, bd.bits, pk, forms["second_pass"])


def test_batch_path_legacy_tail(tmp_path):
    """RD_TAIL_IMPL=legacy (separate kernels; the library reads the switch once per process): one child for all cases."""
    inp, out = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(inp, **{c.name: _batch_input(c)[0] for c in NT.cases()})
    child = (
        "import numpy as np\n"
        "from rtldavis_amd import batch, dsp\n"
        f"z = np.load(r'{inp}')\n"
        "o = {}\n"
        "for name in z.files:\n"
        "    raw = z[name]\n"
        f"    bd = batch.BatchDemodulator(dsp.PacketConfig(19200, 14, 16, 80, '{PREAMBLE}', {BLOCK}), raw.shape[0], raw.shape[1] // {2 * BLOCK})\n"
        "    res = bd.demodulate(raw)\n"
        "    f = bd.last_run_forms()\n"
        "    assert not f['one_launch_tail']\n"
        "    o[name + '/bits'] = np.stack([bd.bits(i) for i in range(raw.shape[0])])\n"
        "    o[name + '/pk'] = np.array([repr([(c, p.index, bytes(p.data).hex()) for c, ps in enumerate(res[i]) for p in ps])"
        " for i in range(raw.shape[0])])\n"
        "    o[name + '/second'] = np.array(bool(f['second_pass']))\n"
        f"np.savez(r'{out}', **o)\n")
    subprocess.run([sys.executable, "-c", child], check=True, env=dict(os.environ, RD_TAIL_IMPL="legacy"), cwd=ROOT, timeout=300)
    z = np.load(out)
    for c in NT.cases():
        bits = z[c.name + "/bits"]
        pk = [eval(s) for s in z[c.name + "/pk"]]   # (our own child's repr of tuples of ints and hex strings)
        _check_batch(c, lambda i: bits[i], pk, bool(z[c.name + "/second"]))


# ---------------------------------------------------------------------------------------------------------------------
def _stream_bits(dem, blocks):
    B = dem.cfg.block_size
    out = []
    for b in blocks:
        dem.demodulate(b)
        out.append(dem.quantized[dem.cfg.buffer_length - B:].copy())
    return np.concatenate(out)


@pytest.mark.parametrize("amp", list(NT.AMPS))
@pytest.mark.parametrize("form", ["u8/2048", "u8/8192", "c128/2048"])
def test_streaming_forms(amp, form):
    """Demodulator.demodulate block by block: bytes in blocks of 2048 and of 8192, and the same samples as complex128
    (k - 127.4) / 127.6, whose one-launch form decides from float64 sums - the planted numerators are >= 2e-10 of the products
    they are the difference of, seven orders above float64 rounding."""
    from rtldavis_amd import dsp
    c = NT.case(f"positions_{amp}")
    kind, B = form.split("/")
    B = int(B)
    n = c.n
    nb = (n + B - 1) // B
    bad = 0
    for s in range(c.streams.shape[0]):
        raw = np.full(2 * B * nb, 127, dtype=np.uint8)
        raw[: 2 * n] = c.streams[s]
        dem = dsp.Demodulator(dsp.PacketConfig(19200, 14, 16, 80, PREAMBLE, B))
        if kind == "u8":
            blocks = [raw[2 * B * b: 2 * B * (b + 1)] for b in range(nb)]
        else:
            z = ((raw[0::2].astype(np.float64) - 127.4) + 1j * (raw[1::2].astype(np.float64) - 127.4)) / 127.6
            blocks = [z[B * b: B * (b + 1)] for b in range(nb)]
        got = _stream_bits(dem, blocks)[:n]
        bad += int((got != c.bits[s]).sum())
    print(f"positions_{amp} {form}: {bad} bits differ from the exact integers")
    assert bad == 0
