"""Helpers shared by tests/test_clip_synth_cpu.py, tests/test_clip_synth.py and tools/burst_monte_carlo.py (no tests in
here): the NumPy model of k_clip_synth and its cases.  The model is written from the definition in
include/rtldavis_hip.h, CLIP SYNTH, in int64 / uint64 arithmetic with a Philox4x32-10 of its own and a cosine table of
NumPy's own (test_clip_synth_cpu.py holds ``rd_cs_table`` to it, not the other way round).  ``mutant`` names one wrong
reading of the definition; test_clip_synth_cpu.py shows for each a case that tells it apart.  Every case asserts, on the
model and when it is built, the edge it is built for.  Nothing here touches a device."""
import functools

import numpy as np

from rtldavis_amd.replay import MAX_AMP_Q, MAX_N, MAX_NOISE_Q, MAX_PRE, MAX_SPECS, MAX_SYM, SPEC_DTYPE

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TABLE = np.rint(16384.0 * np.cos(2.0 * np.pi * np.arange(4096) / 4096.0)).astype(np.int64)
SIGMA_G = (16 * 65535 / 12.0) ** 0.5                       # of g: 16 independent bytes
MUTANTS = ("nine_rounds", "iq_noise_swapped", "sine_wrong_way", "symbol_off_by_one", "round_half_down", "no_clamp",
           "phase_at_u", "noise_by_pool_position")


# ------------------------------------------------------------------------------------------ the definition
def philox(counter, key, rounds=10):
    """Philox4x32: ``counter`` four and ``key`` two arrays (or integers) of 32-bit values; four uint64 arrays < 2^32."""
    c = [np.asarray(x, np.uint64) & MASK for x in counter]
    k = [np.asarray(x, np.uint64) & MASK for x in key]
    for r in range(rounds):
        if r:
            k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
    return c


def noise_g(t, comp, seed, rounds=10):
    """g of output(s) ``t`` and component(s) ``comp`` under ``seed`` (arrays broadcast): int64."""
    seed = np.asarray(seed, np.uint64)
    words = philox((t, comp, 0, 0), (seed & MASK, seed >> np.uint64(32)), rounds)
    total = np.zeros(np.broadcast(*words).shape, np.int64)
    for w in words:
        for sh in (0, 8, 16, 24):
            total += ((w >> np.uint64(sh)) & np.uint64(0xFF)).astype(np.int64)
    return total - 2040


def to_byte(s, mutant=None):
    """S (int64) -> byte: round half up, clamp."""
    b = (s + (2 ** 21 - 1 if mutant == "round_half_down" else 2 ** 21)) >> 22
    return (b & 0xFF if mutant == "no_clamp" else np.clip(b, 0, 255)).astype(np.uint8)


def symbols_of(spec):
    return np.unpackbits(np.asarray(spec["bits"], np.uint8))[: int(spec["n_sym"])].astype(np.int64)


def clip_bytes(spec, sl, mutant=None):
    """The 2 n bytes of one spec's clip."""
    n, at, pre, post = int(spec["n"]), int(spec["at"]), int(spec["pre"]), int(spec["post"])
    amp_q, noise_q, seed = int(spec["amp_q"]), int(spec["noise_q"]), int(spec["seed"])
    t = np.arange(n, dtype=np.int64)
    step = np.repeat(2 * symbols_of(spec) - 1, sl)
    lead = pre + 1 if mutant == "symbol_off_by_one" else pre
    length = pre + step.size + post
    d = np.cumsum(np.concatenate([np.zeros(lead, np.int64), step, np.zeros(post, np.int64)])[:length])   # D(u), u < L
    u = t - (at - pre)
    on = (u >= 0) & (u < length)
    uo = u[on]
    phi = (int(spec["phase0"]) + (uo + (0 if mutant == "phase_at_u" else 1)) * int(spec["f_c"]) + int(spec["f_d"]) * d[uo]) % 2 ** 32
    quarter = 2 ** 30 if mutant != "sine_wrong_way" else -2 ** 30
    sig = np.zeros((2, n), np.int64)
    sig[0, on] = amp_q * TABLE[phi >> 20]
    sig[1, on] = amp_q * TABLE[((phi - quarter) % 2 ** 32) >> 20]
    tn = t + int(spec["offset"]) if mutant == "noise_by_pool_position" else t
    comp = np.array([[1], [0]] if mutant == "iq_noise_swapped" else [[0], [1]])
    g = noise_g(tn[None, :] % 2 ** 32, comp, seed, 9 if mutant == "nine_rounds" else 10)
    s = (256 << 21) + sig + noise_q * g
    return to_byte(s, mutant).T.reshape(-1).copy()


def pool_of(specs, sl, pool_outputs=None, mutant=None):
    """The pool a list of (legal) specs gives: zeros where no clip lies."""
    specs = np.asarray(specs, SPEC_DTYPE).reshape(-1)
    if pool_outputs is None:
        pool_outputs = default_pool(specs)
    pool = np.zeros(2 * int(pool_outputs), np.uint8)
    for s in specs:
        pool[2 * int(s["offset"]): 2 * (int(s["offset"]) + int(s["n"]))] = clip_bytes(s, sl, mutant)
    return pool


def default_pool(specs):
    return (int(specs["offset"][-1]) + int(specs["n"][-1]) + 7) // 8 * 8


def pack_bits(sym):
    out = np.zeros(MAX_SYM, np.uint8)
    out[: len(sym)] = sym
    return np.packbits(out)


def spec_row(n, at=0, sym=(), seed=1, amp_q=0, noise_q=0, f_c=0, f_d=0, phase0=0, pre=0, post=0, offset=0, pad=0, n_sym=None):
    row = np.zeros((), SPEC_DTYPE)
    row["offset"], row["seed"], row["n"], row["at"] = int(offset), int(seed) % 2 ** 64, int(n), int(at)
    row["phase0"], row["f_c"], row["f_d"] = int(phase0), int(f_c), int(f_d)
    row["amp_q"], row["noise_q"], row["pre"], row["post"], row["pad"] = int(amp_q), int(noise_q), int(pre), int(post), int(pad)
    row["n_sym"] = len(sym) if n_sym is None else int(n_sym)
    row["bits"] = pack_bits(np.asarray(sym, np.uint8))
    return row


def lay_out(rows, gaps=None):
    """The rows as a spec list at ascending offsets: each at the next multiple of 8 (+ 8 gaps[k] outputs in front of row k)."""
    specs = np.asarray(list(rows), SPEC_DTYPE).reshape(-1).copy()
    at = 0
    for k in range(specs.size):
        at += 8 * (int(gaps[k]) if gaps is not None else 0)
        specs[k]["offset"] = at
        at = (at + int(specs[k]["n"]) + 7) // 8 * 8
    return specs


def f_dev(sl):
    return int(round(2.0 ** 32 / (4 * sl)))


def f_car(cycles):
    return int(round(cycles * 2.0 ** 32) + 2 ** 31) % 2 ** 32 - 2 ** 31


class Case:
    """A spec list for one SL and the pool it gives (the model's, computed once)."""

    def __init__(self, name, sl, specs, pool_outputs=None):
        self.name, self.sl = name, int(sl)
        self.specs = np.asarray(specs, SPEC_DTYPE).reshape(-1)
        self.pool_outputs = default_pool(self.specs) if pool_outputs is None else int(pool_outputs)
        assert check_specs(self.specs, self.pool_outputs) == (0, -1), (name, check_specs(self.specs, self.pool_outputs))

    @functools.cached_property
    def pool(self):
        p = pool_of(self.specs, self.sl, self.pool_outputs)
        p.setflags(write=False)
        return p

    def clip(self, k, pool=None):
        s = self.specs[k]
        return (self.pool if pool is None else pool)[2 * int(s["offset"]): 2 * (int(s["offset"]) + int(s["n"]))]

    def config(self):
        import burst_decode_cases as DC
        return DC.config(self.sl, 80 if self.sl * 80 + 1 <= 2048 else 40, 2048)


def _sym(seed, k):
    return np.random.default_rng(seed).integers(0, 2, k).astype(np.uint8)


# ------------------------------------------------------------------------------------------ the cases
LENGTHS = (1, 7, 8, 9, 15, 16, 17, 1400)


@functools.lru_cache(maxsize=None)
def lengths_case():
    """SL 14: clips of 1, 7, 8, 9, 15, 16, 17 and 1400 outputs (n % 8 = 0, 1, 7 among them), each inside a burst with noise."""
    rows = [spec_row(n, at=-3, sym=_sym(4000 + n, 120), seed=4000 + n, amp_q=9000, noise_q=60000, f_c=f_car(-0.24), f_d=f_dev(14),
                     phase0=12345 * n, pre=5) for n in LENGTHS]
    X = Case("lengths", 14, lay_out(rows))
    assert {n % 8 for n in LENGTHS} >= {0, 1, 7}
    for k, n in enumerate(LENGTHS):                          # the slack behind a clip is zero in the model's pool
        end = int(X.specs[k]["offset"]) + n
        assert np.all(X.pool[2 * end: 2 * ((end + 7) // 8 * 8)] == 0) and len(set(X.clip(k).tolist())) > (1 if n > 1 else 0)
    return X


@functools.lru_cache(maxsize=None)
def placement_case():
    """SL 14, n = 1400, no noise so that OFF outputs read 128: the burst (L = 30 + 14 x 120 + 50 = 1760) cut at the front, wholly
    in front of the clip, ending at the clip's first output, cut at the back, beginning at the last output, wholly behind,
    covering the whole clip, beginning inside it, and at = -+2^30 (symbols_case holds bursts that lie wholly inside)."""
    L = 30 + 14 * 120 + 50
    ats = (-500, 30 - L, 30 - L + 1, 1000, 1399 + 30, 1400 + 30, -100, 200, -2 ** 30, 2 ** 30)
    rows = [spec_row(1400, at=a, sym=_sym(4100 + i, 120), amp_q=12000, f_c=f_car(0.013), f_d=f_dev(14), phase0=99 + i, pre=30, post=50)
            for i, a in enumerate(ats)]
    X = Case("placement", 14, lay_out(rows))
    on = [np.flatnonzero(np.any(X.clip(k).reshape(-1, 2) != 128, axis=1)) for k in range(len(ats))]
    assert on[0][0] == 0 and on[0][-1] == -500 - 30 + L - 1 and on[1].size == 0 and on[2].tolist() == [0]
    assert on[3][0] == 970 and on[3][-1] == 1399 and on[4].tolist() == [1399] and on[5].size == 0
    assert on[6].size == 1400 and on[7][0] == 170 and on[7][-1] == 1399 and on[8].size == 0 and on[9].size == 0
    return X


@functools.lru_cache(maxsize=None)
def symbols_case():
    """SL 14: n_sym 0 (pre / post alone: plain carrier), 1 and 192, with pre / post zero and non-zero."""
    rows = []
    for n_sym in (0, 1, 192):
        for pre, post in ((0, 0), (17, 0), (0, 23), (4096, 4096)):
            rows.append(spec_row(700 if n_sym < 192 else 3000, at=40 if pre < 100 else -3900, sym=_sym(4200 + n_sym, n_sym), seed=7,
                                 amp_q=20000, noise_q=3000, f_c=f_car(0.07), f_d=f_dev(14), pre=pre, post=post))
    X = Case("symbols", 14, lay_out(rows))
    quiet = spec_row(700, seed=7, noise_q=3000)
    assert np.array_equal(X.clip(0), clip_bytes(quiet, 14))                # no symbol, no pre, no post: nothing is ON
    assert not np.array_equal(X.clip(1), X.clip(0)) and not np.array_equal(X.clip(4), X.clip(5))
    return X


@functools.lru_cache(maxsize=None)
def levels_case():
    """SL 14: amp_q 0 with noise, noise 0 with signal, both 0 (every byte 128), and amp_q 65535 with noise_q 2^20: both clamps."""
    sym = _sym(4300, 120)
    kw = dict(at=10, sym=sym, f_c=f_car(-0.25), f_d=f_dev(14), seed=4300)
    rows = [spec_row(600, amp_q=0, noise_q=100000, **kw), spec_row(600, amp_q=9800, noise_q=0, **kw), spec_row(600, **kw),
            spec_row(2000, amp_q=65535, noise_q=MAX_NOISE_Q, **kw), spec_row(600, amp_q=MAX_AMP_Q, noise_q=0, **kw)]
    X = Case("levels", 14, lay_out(rows))
    assert np.all(X.clip(2) == 128) and X.clip(0).std() > 3 and set(X.clip(1)[: 2 * 10].tolist()) == {128}
    loud = X.clip(3)
    assert loud.min() == 0 and loud.max() == 255 and np.count_nonzero(loud == 0) > 50 and np.count_nonzero(loud == 255) > 50
    assert not np.array_equal(clip_bytes(X.specs[3], 14, "no_clamp"), loud)
    assert X.clip(4).max() == 255 and X.clip(4).min() <= 1                 # 256 bytes of amplitude clamp with no noise
    return X


@functools.lru_cache(maxsize=None)
def phase_case():
    """SL 14: phase0 = 0xFFFFFFFF; f_c = -(2^31 - 1), 0, 2^31 - 1; f_d = 0 and 2^31 - 1 (the phase wraps every output).  Clip 8:
    a flat carrier of amp_q 128 at phase 0 with no noise - S = 128 + 1/2 byte exactly at every ON output's I: the tie of the
    rounding (129 half up)."""
    sym = _sym(4400, 64)
    rows = [spec_row(500, at=5, sym=sym, amp_q=11000, noise_q=20000, seed=4400 + i, phase0=p, f_c=c, f_d=d, pre=3, post=3)
            for i, (p, c, d) in enumerate(((0xFFFFFFFF, f_car(0.01), f_dev(14)), (1, -(2 ** 31 - 1), f_dev(14)), (2, 0, f_dev(14)),
                                           (3, 2 ** 31 - 1, f_dev(14)), (4, f_car(0.2), 0), (5, f_car(0.2), 2 ** 31 - 1),
                                           (0xFFFFFFFF, -(2 ** 31 - 1), 2 ** 31 - 1), (0, 0, 0)))]
    rows.append(spec_row(500, at=5, sym=sym, amp_q=128, pre=3, post=3))
    X = Case("phase", 14, lay_out(rows))
    tie = X.clip(8).reshape(-1, 2)
    assert np.all(tie[2: 2 + 6 + 14 * 64, 0] == 129) and np.all(tie[:2, 0] == 128) and np.all(tie[:, 1] == 128)
    assert np.all(clip_bytes(X.specs[8], 14, "round_half_down") == 128)
    flat = spec_row(500, at=5, sym=sym, amp_q=11000, phase0=0, pre=3, post=3)
    on = clip_bytes(flat, 14).reshape(-1, 2)[2: 2 + 6 + 14 * 64]
    assert np.all(on[:, 0] == (256 * 2 ** 21 + 11000 * 16384 + 2 ** 21) >> 22) and np.all(on[:, 1] == 128)   # cos 0 and sin 0
    return X


SHAPE_SLS = (3, 4, 51)


@functools.lru_cache(maxsize=None)
def shape_case(sl):
    """SL 3, 4 and 51: 192 symbols and a short burst, both with noise, n % 8 = 5 and 3."""
    rows = [spec_row(192 * sl + 61, at=20, sym=_sym(4500 + sl, 192), seed=4500 + sl, amp_q=8000, noise_q=50000, f_c=f_car(-0.25 + 0.01),
                     f_d=f_dev(sl), pre=7, post=9),
            spec_row(16 * sl + 11, at=-sl - 1, sym=_sym(4600 + sl, 30), seed=4600 + sl, amp_q=30000, noise_q=0, f_c=f_car(0.3), f_d=f_dev(sl))]
    return Case(f"shape_sl{sl}", sl, lay_out(rows))


@functools.lru_cache(maxsize=None)
def seeds_case():
    """SL 14: seeds 0, 2^64 - 1, and two that differ in the high word alone; the same spec at two offsets and in two list
    positions (clips 4 and 6 are clip 0's spec again: equal bytes)."""
    seeds = (0, 2 ** 64 - 1, 0x0000000112345678, 0x0000000212345678)
    mk = lambda s: spec_row(333, at=20, sym=_sym(4700, 20), seed=s, amp_q=5000, noise_q=80000, f_c=f_car(0.1), f_d=f_dev(14))
    rows = [mk(s) for s in seeds] + [mk(seeds[0]), mk(12345), mk(seeds[0])]
    X = Case("seeds", 14, lay_out(rows, gaps=(0, 0, 1, 0, 3, 0, 0)))
    clips = [X.clip(k).tobytes() for k in range(7)]
    assert len(set(clips[:4])) == 4 and clips[4] == clips[0] == clips[6] and len(set(clips)) == 5
    return X


@functools.lru_cache(maxsize=None)
def gaps_case():
    """SL 14: gaps of whole vectors in front of, between and behind the clips, and a pool that is no multiple of 8 outputs."""
    rows = [spec_row(n, at=3, sym=_sym(4800 + n, 40), seed=n, amp_q=7000, noise_q=40000, f_c=f_car(-0.2), f_d=f_dev(14)) for n in (100, 9, 257, 1)]
    specs = lay_out(rows, gaps=(2, 1, 40, 5))
    X = Case("gaps", 14, specs, default_pool(specs) + 8 * 33 + 3)
    used = np.zeros(X.pool_outputs, bool)
    for s in X.specs:
        used[int(s["offset"]): int(s["offset"]) + int(s["n"])] = True
    assert np.all(X.pool.reshape(-1, 2)[~used] == 0) and np.count_nonzero(~used) > 8 * 80 and np.all(X.pool.reshape(-1, 2)[used] != 0)
    return X


@functools.lru_cache(maxsize=None)
def random_case(count=600, seed=4900):
    """SL 14: 600 seeded random specs of up to 300 outputs, every field drawn over its whole range - more workgroups than the
    chip has compute units."""
    rng = np.random.default_rng(seed)
    rows, gaps = [], []
    for _ in range(count):
        n_sym = int(rng.choice([0, 1, 20, 120, 192, int(rng.integers(0, 193))]))
        rows.append(spec_row(int(rng.integers(1, 301)), at=int(rng.integers(-3000, 400)), sym=rng.integers(0, 2, n_sym).astype(np.uint8),
                             seed=int(rng.integers(0, 2 ** 64, dtype=np.uint64)), amp_q=int(rng.choice([0, 1, 9800, MAX_AMP_Q, int(rng.integers(0, MAX_AMP_Q + 1))])),
                             noise_q=int(rng.choice([0, 1, 362105, MAX_NOISE_Q, int(rng.integers(0, MAX_NOISE_Q + 1))])),
                             f_c=int(rng.integers(-2 ** 31, 2 ** 31)), f_d=int(rng.integers(0, 2 ** 31)), phase0=int(rng.integers(0, 2 ** 32)),
                             pre=int(rng.choice([0, 1, 300, MAX_PRE])), post=int(rng.choice([0, 2, MAX_PRE]))))
        gaps.append(int(rng.choice([0, 0, 0, 1, 5])))
    X = Case("random", 14, lay_out(rows, gaps))
    lit = sum(bool(np.any(X.clip(k) != 128)) for k in range(count))
    assert lit > count // 2 and len({int(s["n"]) % 8 for s in X.specs}) == 8
    return X


def exact_cases():
    return [lengths_case(), placement_case(), symbols_case(), levels_case(), phase_case(), seeds_case(), gaps_case()] + \
        [shape_case(sl) for sl in SHAPE_SLS]


# ------------------------------------------------------------------------------------------ the statistical check
STAT_CLIPS, STAT_N, STAT_NOISE_Q = 4096, 256, 141900           # sigma = 141900 x 295.601 / 2^22 = 10.0 bytes: no byte clamps
STAT_SIGMA = STAT_NOISE_Q * SIGMA_G / 2 ** 22


def stat_specs():
    seeds = np.random.default_rng(5000).integers(0, 2 ** 64, STAT_CLIPS, dtype=np.uint64)
    specs = np.zeros(STAT_CLIPS, SPEC_DTYPE)
    specs["offset"] = np.arange(STAT_CLIPS, dtype=np.uint64) * np.uint64(STAT_N)
    specs["seed"], specs["n"], specs["noise_q"] = seeds, STAT_N, STAT_NOISE_Q
    return specs


def stat_model_pool(specs):
    """The model's pool for noise-only specs of one n at consecutive offsets, all clips in one call of the definition's parts."""
    n = int(specs["n"][0])
    g = noise_g(np.arange(n)[None, :, None], np.arange(2)[None, None, :], specs["seed"][:, None, None])
    return to_byte((256 << 21) + specs["noise_q"].astype(np.int64)[:, None, None] * g).reshape(-1)


BYTE_MEAN = 127.5 + 0.5                                       # of a noise-only clip: see stat_figures


def stat_figures(pool):
    """(mean, variance, derived variance) of the bytes of 4096 x 256 noise-only outputs.  Derived: S is centred on 128 bytes
    and a byte is floor(S + 1/2) - rounding half up -, with the noise symmetric around 0 and spread over many bytes: the
    rounding is unbiased, so the mean is 128 = 127.5 + 0.5, half a byte above the decoders' zero, and the variance
    sigma^2 + 1 / 12.  The sampling error of the mean is sigma / sqrt(2^21) = 0.007 and that of the variance
    sqrt(2 / 2^21) = 0.1 %."""
    b = np.asarray(pool, np.float64)
    assert b.size == 2 * STAT_CLIPS * STAT_N
    return b.mean(), b.var(), STAT_SIGMA ** 2 + 1.0 / 12.0


# ------------------------------------------------------------------------------------------ the argument rule, restated
def check_specs(specs, pool_outputs):
    """rd_cs_check_specs in Python: (0, -1), or (-1, the first offending spec; -1 for the count itself)."""
    specs = np.asarray(specs, SPEC_DTYPE).reshape(-1)
    if not 1 <= specs.size <= MAX_SPECS:
        return -1, -1
    nxt = 0
    for i, s in enumerate(specs):
        off, n, n_sym = int(s["offset"]), int(s["n"]), int(s["n_sym"])
        bits = np.unpackbits(s["bits"])
        bad = (off % 8 != 0 or not 1 <= n <= MAX_N or off < nxt or off + n > pool_outputs or n_sym > MAX_SYM or int(s["pre"]) > MAX_PRE
               or int(s["post"]) > MAX_PRE or int(s["amp_q"]) > MAX_AMP_Q or int(s["noise_q"]) > MAX_NOISE_Q or int(s["f_d"]) >= 2 ** 31
               or abs(int(s["at"])) > 2 ** 30 or int(s["pad"]) != 0 or (n_sym <= MAX_SYM and bool(np.any(bits[n_sym:]))))
        if bad:
            return -1, i
        nxt = (off + n + 7) // 8 * 8
    return 0, -1


REFUSALS = {"offset": (4, 2 ** 63 + 1), "n": (0, MAX_N + 1, 2 ** 32 - 1), "n_sym": (MAX_SYM + 1, 2 ** 32 - 1), "pre": (MAX_PRE + 1, 65535),
            "post": (MAX_PRE + 1,), "amp_q": (MAX_AMP_Q + 1, 2 ** 32 - 1), "noise_q": (MAX_NOISE_Q + 1,), "f_d": (2 ** 31, 2 ** 32 - 1),
            "at": (-2 ** 30 - 1, 2 ** 30 + 1, -2 ** 31), "pad": (1, 2 ** 32 - 1)}


def refused_lists():
    """[(what, specs, pool_outputs)]: spec lists that break one rule each - the second of three specs is the offender, but for
    the rules on the count and on the pool."""
    base = lay_out([spec_row(40, at=2, sym=_sym(5100 + k, 24), seed=k, amp_q=6000, noise_q=30000, f_d=f_dev(14)) for k in range(3)])
    pool = default_pool(base)
    out = []
    for f, values in REFUSALS.items():
        for v in values:
            s = base.copy()
            s[1][f] = v
            out.append((f"{f}={v}", s, pool))
    s = base.copy()
    s[1]["bits"][3] = 1                                       # bit 31 with n_sym = 24
    out.append(("bits past n_sym", s, pool))
    s = base.copy()
    s[1]["offset"] = 32                                       # overlaps clip 0 (outputs 0 .. 39)
    out.append(("overlap", s, pool))
    s = base.copy()
    s[[1, 2]] = s[[2, 1]]
    out.append(("descending", s, pool))
    out.append(("past the pool", base.copy(), pool - 1 - 7))
    out.append(("pool of 0", base.copy(), 0))
    for what, s, p in out:
        assert check_specs(s, p)[0] == -1, what
    return out
