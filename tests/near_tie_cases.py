"""Planted near-ties for k_demod_mfma (rtldavis_amd/csrc/rd_demod_mfma.hip).  TEST INFRASTRUCTURE ONLY.

The kernel decides bit[t] from an fp32 numerator n[t] = -(Re g[t-1] conj g[t]) and lists every 8-sample group whose guard
value  min |n| - 2^-21 max |t1|  does not clear c0(F) (rd_mfma.h).  Random inputs never come near that band at any
amplitude worth the name, so this module PLANTS samples there: n[t] depends on samples t-10 .. t-1, sample t-1 enters g[t]
only and sample t-10 enters g[t-1] only, so the numerator is affine in the bytes of either; a small lattice search over
those four bytes moves the exact numerator of a random window onto a target.

Three pieces, all NumPy and Python integers:
  exact reference   G[t] = sum_m C_m j^m U[t-9+m], U = 5 k - 637, C = fir9 taps * 1e12 (the integers of rd_math.h) in int64,
                    N[t] = -(Re G[t-1] conj G[t]); the bit is N < 0.  Float64 decides where it is certain, Python integers
                    everywhere else (all plants among them).
  fp32 model        what the kernel does with the g it returns, one IEEE fp32 operation at a time, bit exact (the fma
                    through float64 with round-to-odd; tests/test_near_tie_cpu.py re-derives the flagged groups with Fraction).
  cases             `cases()` - streams, plants and the model's verdicts, generated once per process.

Index convention (the kernel's): g[t] uses samples t-9 .. t-1; lane l of a stream decides samples 4 l .. 4 l + 3 from
g[4 l - 1 .. 4 l + 3]; group G = lanes 2 G, 2 G + 1; word W = groups 4 W .. 4 W + 3.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

import mfma_model as M

TILE = M.TILE
C12 = M.C12
# kernel units of g per unit of the exact integer G:  g = 2^-24 S (k - 127.4) c,  G = 1e12 c * 5 (k - 127.4)
K = M.UNIT * M.SCALE / 5.0e12
C0_MAX = np.float32(9.62e-4)   # RD_MF_C0_MAX
TWO_M21 = np.float32(4.76837158e-7)
assert float(TWO_M21) == 2.0 ** -21
MARGIN = 1.0e-5                # no group of any case has |nm - c0(F)| <= MARGIN * c0(F): rd_mf_c0 may be contracted
AMPS = {"full": (0, 255), "half": (64, 192), "low": (112, 144), "tiny": (124, 131)}
# deep+-: |N| <= 1e-6 F, either sign; in: |N| = 0.3 c0; t1: between c0 and c0 + 2^-21 max |t1| (listed only because of that
# term); out1.5 / out3: guard value 1.5 / 3 c0 (trusted at the tightest margin); far: well outside
KINDS = ("deep+", "deep-", "in", "t1", "out1.5", "out3", "far")


# ---------------------------------------------------------------------------------------------------------------------
# FIR in either integer model.  ur / ui: [..., nin]; output j uses inputs j .. j + 8 (oldest first).
def _fir(ur, ui, taps, nout):
    gr = np.zeros(ur.shape[:-1] + (nout,), dtype=ur.dtype)
    gi = np.zeros_like(gr)
    for m in range(9):
        c = taps[m if m <= 4 else 8 - m]
        a, b = ur[..., m:m + nout], ui[..., m:m + nout]
        ph = m & 3   # c j^m (I + jQ)
        if ph == 0:
            gr += c * a; gi += c * b
        elif ph == 1:
            gr -= c * b; gi += c * a
        elif ph == 2:
            gr -= c * a; gi -= c * b
        else:
            gr += c * b; gi -= c * a
    return gr, gi


def exact_G(raw: np.ndarray, hist: np.ndarray | None):
    """int64 G[t], t = -1 .. n-1 (index t + 1).  No history: the zero state (U = 0 before the stream)."""
    n = raw.size // 2
    u = np.zeros((2, n + 10), dtype=np.int64)
    u[0, 10:] = 5 * raw[0::2].astype(np.int64) - 637
    u[1, 10:] = 5 * raw[1::2].astype(np.int64) - 637
    if hist is not None:
        h = hist[-20:]
        u[0, :10] = 5 * h[0::2].astype(np.int64) - 637
        u[1, :10] = 5 * h[1::2].astype(np.int64) - 637
    return _fir(u[0], u[1], C12, n + 1)


def exact_N_int(Gr, Gi, t: int) -> int:
    """N[t] as a Python integer (G arrays indexed t + 1)."""
    return -(int(Gr[t]) * int(Gr[t + 1]) + int(Gi[t]) * int(Gi[t + 1]))


def exact_bits(Gr, Gi, zero_state=False):
    """bit[t] = N[t] < 0 for t = 0 .. n-1, and N in float64 (for reporting).  Float64 where its sign is certain
    (|N| above 2^-50 of the products), Python integers elsewhere.  Returns (bits, N64, number of zeros met).
    zero_state: G[-1] = G[0] = 0 (no sample of the stream has entered yet) make N[0] = N[1] = 0 by construction; the
    reference's float64 expression then gives -0.0 exactly when Re f[t] < 0 < Im f[t], f[t] = j^(t-9) g[t] (rd_math.h:
    rd_exact_bit).  Those two are not counted as zeros."""
    a, b, c, d = (x.astype(np.float64) for x in (Gr[:-1], Gi[:-1], Gr[1:], Gi[1:]))   # all exact: |G| < 2^53
    p1, p2 = a * c, b * d
    n64 = -(p1 + p2)
    unsure = ~(np.abs(n64) > 2.0 ** -50 * (np.abs(p1) + np.abs(p2)))
    bits = (n64 < 0).astype(np.uint8)
    zeros = 0
    for t in np.nonzero(unsure)[0]:
        v = exact_N_int(Gr, Gi, int(t))
        if v == 0 and t <= 1 and zero_state and Gr[t] == 0 and Gi[t] == 0:
            f = complex(int(Gr[t + 1]), int(Gi[t + 1])) * (-1j if t == 0 else 1)
            bits[t] = f.real < 0 and f.imag > 0
            continue
        zeros += v == 0
        bits[t] = v < 0
    return bits, n64, zeros


def kernel_g32(raw: np.ndarray, hist: np.ndarray | None) -> np.ndarray:
    """float32 g[t], t = -1 .. n-1 (index t + 1), [n + 1, 2]: the integer model of rd_mfma.h, one rounding.  Without
    history the outputs that see bytes before the stream (t < 9) are not the kernel's (it leaves them to the fix-up)."""
    n = raw.size // 2
    u = np.full((2, n + 10), 127.0)
    u[0, 10:] = raw[0::2]
    u[1, 10:] = raw[1::2]
    if hist is not None:
        h = hist[-20:]
        u[0, :10] = h[0::2]
        u[1, :10] = h[1::2]
    gr, gi = _fir(u[0], u[1], M.T, n + 1)
    off = 2048.0 * M.DHI
    return np.stack([(gr - off) * M.UNIT, (gi - off) * M.UNIT], axis=-1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# fp32, one operation at a time
def fma32(x, y, z):
    """fl32(x y + z) for float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd
    there (its error from TwoSum), and 53 >= 2 * 24 + 2 bits make the second rounding harmless."""
    p = x.astype(np.float64) * y.astype(np.float64)
    z = z.astype(np.float64)
    s = p + z
    bb = s - p
    e = (p - (s - bb)) + (z - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def c0(F):
    """rd_mf_c0 without contraction (tests/mfma_model.py)."""
    return M.c0(np.asarray(F, dtype=np.float32))


@dataclass
class LaneModel:
    n: np.ndarray        # [T] float32 numerators, sample order
    t1: np.ndarray       # [T]
    nm: np.ndarray       # [L] guard value of a lane (4 samples)
    F: np.ndarray        # [L]
    thr: np.ndarray      # [L] c0(F)
    lane_flag: np.ndarray
    fast_bits: np.ndarray  # [T] uint8


def lane_model(g32: np.ndarray, f_own_only=False, drop_t1=False) -> LaneModel:
    """g32: [..., T + 1, 2] with T a multiple of 4 (g[t-1] of the first sample first).  The two keyword arguments are the
    MUTANTS of tests/test_near_tie_cpu.py, not options."""
    a, b = g32[..., :-1, 0], g32[..., :-1, 1]
    c, d = g32[..., 1:, 0], g32[..., 1:, 1]
    t1 = b * d                                    # float32 * float32 -> float32: one rounding
    n = fma32(-a, c, -t1)
    sh = n.shape[:-1] + (n.shape[-1] // 4, 4)
    nmin = np.abs(n).reshape(sh).min(axis=-1)
    tmax = np.abs(t1).reshape(sh).max(axis=-1)
    nm = nmin if drop_t1 else fma32(np.broadcast_to(-TWO_M21, tmax.shape), tmax, nmin)
    mag = np.abs(g32).max(axis=-1)                # [.., T + 1]: |g[t]| over re, im; index t + 1
    L = sh[-2]
    # the predecessor's two outputs g[base-1], g[base] and the lane's outputs 0..2 = g[base+1 .. base+3]; index base + 1 + k
    idx = 4 * np.arange(L)[:, None] + np.arange(0 if not f_own_only else 2, 5)[None, :]
    F = mag[..., idx].max(axis=-1)
    thr = c0(F)
    return LaneModel(n, t1, nm, F, thr, ~(nm > thr), np.signbit(n).astype(np.uint8))


def round_f32(x: Fraction) -> float:
    """Fraction -> nearest float32 (ties to even), normal range."""
    if x == 0:
        return 0.0
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and e >= -126
    q = Fraction(2) ** (e - 23)
    m = a / q
    mi = m.numerator // m.denominator
    rem = m - mi
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and mi & 1):
        mi += 1
    return s * float(mi * q)


def lane_nm_fraction(g5: np.ndarray) -> float:
    """The guard value of ONE lane from its five g (float32 [5, 2]) in rational arithmetic, rounded where fp32 rounds."""
    ns, ts = [], []
    for k in range(4):
        a, b, c, d = (Fraction(float(v)) for v in (g5[k, 0], g5[k, 1], g5[k + 1, 0], g5[k + 1, 1]))
        t1 = Fraction(round_f32(b * d))
        ns.append(abs(Fraction(round_f32(-a * c - t1))))
        ts.append(abs(t1))
    return round_f32(min(ns) - Fraction(2) ** -21 * max(ts))


# ---------------------------------------------------------------------------------------------------------------------
# planting
def _windows(rng, lo, hi, r, kind, count):
    """`count` windows [13, 2] uint8 (samples base-10 .. base+2 of a lane) whose sample t = base + r is a near-tie of class
    `kind`, judged by the lane model and the exact integers.  Returns (windows, wrong) - wrong[i]: the modelled fast sign of
    the planted sample differs from the exact one."""
    out, wrong = [], []
    vals = np.arange(lo, hi + 1)
    nq = vals.size
    npair = max(1, min(32, 256 // nq))
    B = int(min(4096, max(1024, 128 * count)))
    c0t = int(C12[0])    # the tap both free samples enter with
    for _ in range(4000):
        if len(out) >= count:
            break
        w = rng.integers(lo, hi + 1, size=(B, 13, 2), dtype=np.int64)
        fr, fo = 9 + r, r                    # window index of sample t-1 (enters g[t] only) and of sample t-10
        # coarse step: the I byte of sample t-5 enters Re g[t] with the centre tap and Im g[t-1] with its neighbour, so N is
        # affine in it too, with a slope twelve times that of the free samples: it brings N within their reach
        u = (5 * w - 637).astype(np.float64)
        gr, gi = _fir(u[..., 0], u[..., 1], tuple(float(x) for x in C12), 5)
        slope = gr[:, r] * float(C12[4]) + float(C12[3]) * gi[:, r + 1]
        ncur = -(gr[:, r] * gr[:, r + 1] + gi[:, r] * gi[:, r + 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            du = np.nan_to_num(ncur / slope, posinf=0.0, neginf=0.0)
        w[:, 5 + r, 0] = np.clip(np.rint((u[:, 5 + r, 0] + du + 637) / 5.0), lo, hi).astype(np.int64)
        u = (5 * w - 637).astype(np.float64)
        u0 = u.copy()
        u0[:, fr] = 0
        u0[:, fo] = 0
        gr, gi = _fir(u0[..., 0], u0[..., 1], tuple(float(x) for x in C12), 5)   # G[base-1 .. base+3], exact in float64
        A0, B0, Cc0, D0 = gr[:, r], gi[:, r], gr[:, r + 1], gi[:, r + 1]
        pr = rng.integers(lo, hi + 1, size=(B, npair, 2))                   # (I', Q') of sample t-10
        A = A0[:, None] + c0t * (5.0 * pr[..., 0] - 637)                    # [B, P]
        Bq = B0[:, None] + c0t * (5.0 * pr[..., 1] - 637)
        D = D0[:, None] + c0t * (5.0 * vals[None, :] - 637)                 # [B, Q]
        Fk = K * np.maximum(np.maximum(np.abs(A), np.abs(Bq))[:, :, None], np.abs(D)[:, None, :])
        Fk = np.maximum(Fk, K * np.hypot(gr, gi).max(axis=1)[:, None, None])
        thr = 4.0 * M.E0 * Fk + 3.0e-10
        t1 = K * K * np.abs(Bq[:, :, None] * D[:, None, :]) * 2.0 ** -21
        # targets for |N| (kernel units).  The guard value is min |n| - 2^-21 max |t1|, so "just outside" is counted from
        # c0 + 2^-21 |t1| and not from c0: at full scale that term is several times c0.  Accepted below: the exact integer N
        # within 10 % of its target (tighter for the out classes: the guard value itself within (1, 2] c0 and (1, 4] c0).
        if kind in ("deep+", "deep-", "deep"):
            tgt = 0.5e-6 * Fk
            tol = 0.5e-6 * Fk
        elif kind == "in":
            tgt, tol = 0.3 * thr, 0.03 * thr
        elif kind == "band":     # anywhere inside (the dense tiles)
            tgt, tol = 0.3 * thr, 0.3 * thr
        elif kind == "t1":
            tgt, tol = thr + 0.5 * t1, 0.25 * t1
        elif kind == "out1.5":
            tgt, tol = t1 + 1.5 * thr, 0.15 * thr
        elif kind == "out3":
            tgt, tol = t1 + 3.0 * thr, 0.3 * thr
        else:
            tgt, tol = 100.0 * (t1 + thr), 10.0 * (t1 + thr)
        best, arg = None, None
        for sgn in ((1.0,) if kind == "deep+" else (-1.0,) if kind == "deep-" else (1.0, -1.0)):
            # N = -(A C + B D) = sgn tgt / K^2  ->  C, then the byte of I
            C = (-sgn * tgt / (K * K) - Bq[:, :, None] * D[:, None, :]) / A[:, :, None]
            kI = np.clip(np.rint(((C - Cc0[:, None, None]) / c0t + 637) / 5.0), lo, hi)
            C = Cc0[:, None, None] + c0t * (5.0 * kI - 637)
            N = -(A[:, :, None] * C + Bq[:, :, None] * D[:, None, :]) * (K * K)
            ok = (np.abs(np.abs(N) - tgt) <= tol) & (np.sign(N) == sgn)
            score = np.where(ok, np.abs(np.abs(N) - tgt) / tol, np.inf)
            flat = score.reshape(B, -1)
            a_ = flat.argmin(axis=1)
            s_ = flat[np.arange(B), a_]
            if best is None:
                best, arg, kIs = s_, a_, kI.reshape(B, -1)[np.arange(B), a_]
            else:
                better = s_ < best
                best = np.where(better, s_, best)
                arg = np.where(better, a_, arg)
                kIs = np.where(better, kI.reshape(B, -1)[np.arange(B), a_], kIs)
        hit = np.nonzero(np.isfinite(best))[0]
        if hit.size == 0:
            continue
        ip, iq = np.divmod(arg[hit], nq)
        wv = w[hit].copy()
        wv[:, fo, 0] = pr[hit, ip, 0]
        wv[:, fo, 1] = pr[hit, ip, 1]
        wv[:, fr, 0] = kIs[hit].astype(np.int64)
        wv[:, fr, 1] = vals[iq]
        wv = wv.astype(np.uint8)
        # judge by the lane model and the exact integers
        kr, ki = _fir(wv[..., 0].astype(np.float64), wv[..., 1].astype(np.float64), M.T, 5)
        off = 2048.0 * M.DHI
        g5 = np.stack([(kr - off) * M.UNIT, (ki - off) * M.UNIT], axis=-1).astype(np.float32)
        lm = lane_model(g5)
        uw = 5 * wv.astype(np.int64) - 637
        Gr, Gi = _fir(uw[..., 0], uw[..., 1], C12, 5)
        for i in range(hit.size):
            if len(out) >= count:
                break
            Nx = -(int(Gr[i, r]) * int(Gr[i, r + 1]) + int(Gi[i, r]) * int(Gi[i, r + 1]))
            if Nx == 0:
                continue
            Nk, F, th = abs(Nx) * K * K, float(lm.F[i, 0]), float(lm.thr[i, 0])
            nm, flag = float(lm.nm[i, 0]), bool(lm.lane_flag[i, 0])
            tm = 2.0 ** -21 * float(np.abs(lm.t1[i]).max())
            if abs(nm - th) <= 10 * MARGIN * th or np.abs(lm.n[i]).argmin() != r:
                continue
            if Nk < 2.0e-10 * F * F:     # the float64 forms (oracle, one-launch complex path) must still be certain of it
                continue
            if kind == "deep":
                good = flag and Nk <= 1.0e-6 * F
            elif kind == "band":
                good = flag and Nk <= 0.6 * th
            elif kind in ("deep+", "deep-"):
                good = flag and Nk <= 1.0e-6 * F and (Nx > 0) == (kind == "deep+")
            elif kind == "in":
                good = flag and abs(Nk - 0.3 * th) <= 0.03 * th
            elif kind == "t1":
                good = flag and float(np.abs(lm.n[i]).min()) > 1.001 * th
            elif kind == "out1.5":
                good = (not flag) and abs(Nk - (tm + 1.5 * th)) <= 0.1 * (tm + 1.5 * th) and nm <= 2.0 * th
            elif kind == "out3":
                good = (not flag) and abs(Nk - (tm + 3.0 * th)) <= 0.1 * (tm + 3.0 * th) and nm <= 4.0 * th
            else:
                good = (not flag) and nm >= 30.0 * th
            if good:
                out.append(wv[i])
                wrong.append(bool(lm.fast_bits[i, r]) != (Nx < 0))
    assert len(out) >= count, f"planting {kind} at r={r} in {lo}..{hi}: {len(out)} of {count}"
    return np.stack(out[:count]), np.array(wrong[:count])


@dataclass
class Plant:
    s: int
    t: int
    kind: str


@dataclass
class Case:
    name: str
    streams: np.ndarray                 # [ns, 2 n] uint8
    hist: np.ndarray | None             # [ns, 64] uint8 or None
    plants: list = field(default_factory=list)
    # filled by _evaluate
    g32: np.ndarray = None              # [ns, n + 1, 2] (index t + 1)
    bits: np.ndarray = None             # exact, [ns, n]
    n64: np.ndarray = None              # exact numerator, float64, units of G^2
    fast: np.ndarray = None             # modelled fast bits [ns, n]
    lane: LaneModel = None
    valid: np.ndarray = None            # [ns, n / 8] groups the model speaks about (not the first run without history)
    flagged: np.ndarray = None          # [ns, n / 8] model-flagged groups
    zeros: int = 0

    @property
    def n(self):
        return self.streams.shape[1] // 2

    def flagged_words(self):
        ns, ng = self.flagged.shape
        f = np.zeros((ns, (ng + 3) // 4 * 4), dtype=bool)   # the last word of a ragged stream may be partial
        f[:, :ng] = self.flagged
        return f.reshape(ns, -1, 4).any(axis=-1)


def _evaluate(c: Case, **mutant) -> Case:
    ns, n = c.streams.shape[0], c.n
    assert n % 8 == 0
    g32 = np.stack([kernel_g32(c.streams[s], None if c.hist is None else c.hist[s]) for s in range(ns)])
    lm = lane_model(g32, **mutant)
    flagged = lm.lane_flag.reshape(ns, n // 8, 2).any(axis=-1)
    valid = np.ones_like(flagged)
    if c.hist is None:
        valid[:, :4] = False
        flagged[:, :4] = False
    if mutant:
        return flagged
    c.g32, c.lane, c.flagged, c.valid, c.fast = g32, lm, flagged, valid, lm.fast_bits
    bits, n64, zeros = [], [], 0
    for s in range(ns):
        Gr, Gi = exact_G(c.streams[s], None if c.hist is None else c.hist[s])
        b, v, z = exact_bits(Gr, Gi, zero_state=c.hist is None)
        bits.append(b); n64.append(v); zeros += z
    c.bits, c.n64, c.zeros = np.stack(bits), np.stack(n64), zeros
    return c


evaluate = _evaluate   # (for other case modules)


def margin_ok(c: Case) -> bool:
    lm = c.lane
    bad = np.abs(lm.nm.astype(np.float64) - lm.thr) <= MARGIN * lm.thr
    if c.hist is None:
        bad[:, :8] = False
    return not bad.any()


def _put(streams, s, t, r, win):
    base = t - r
    streams[s, 2 * (base - 10): 2 * (base + 3)] = win.reshape(-1)


class _Pool:
    """windows by (r, kind), drawn in bulk"""
    def __init__(self, rng, lo, hi):
        self.rng, self.lo, self.hi, self.req = rng, lo, hi, {}

    def want(self, r, kind):
        self.req[(r, kind)] = self.req.get((r, kind), 0) + 1

    def draw(self, reuse=1):
        """reuse > 1: a window serves that many plants (the lane's verdict depends on the window alone; where it lies in the
        tile, and beside what, is what the dense tiles are about)"""
        self.win = {k: list(_windows(self.rng, self.lo, self.hi, k[0], k[1], (v + reuse - 1) // reuse)[0])
                    for k, v in sorted(self.req.items())}
        self.at = {k: 0 for k in self.win}

    def take(self, r, kind):
        k = (r, kind)
        self.at[k] += 1
        return self.win[k][self.at[k] % len(self.win[k])]


def plant(streams, slots, rng, lo, hi, reuse=1):
    """The planting routine (also for other case modules: tests/k1_schedule_cases.py).  slots: (s, t, kind) with t >= 10,
    t + 2 inside the stream and no two of a stream closer than 16 samples; sample t of stream s becomes a near-tie of class
    `kind` with bytes in lo .. hi - samples t - 10 .. t + 2 of `streams` are overwritten in place.  Returns the plants."""
    pool = _Pool(rng, lo, hi)
    for s, t, k in slots:
        pool.want(t % 4, k)
    pool.draw(reuse)
    plants = []
    for s, t, k in slots:
        _put(streams, s, t, t % 4, pool.take(t % 4, k))
        plants.append(Plant(s, t, k))
    return plants


def _positions(rng, amp, ns=8, n=7 * TILE + 1000, hist=False, kinds=KINDS):
    lo, hi = AMPS[amp]
    if amp in ("low", "tiny"):   # 2^-21 max |t1| is a few per cent of c0 there: no room to plant between the two
        kinds = tuple(k for k in kinds if k != "t1")
    streams = rng.integers(lo, hi + 1, size=(ns, 2 * n), dtype=np.uint8)
    h = rng.integers(lo, hi + 1, size=(ns, 64), dtype=np.uint8) if hist else None
    tiles = (n + TILE - 1) // TILE
    slots = []   # (s, t, kind)
    # the carry positions: a tile's first lane, t mod 2048 in 0..3, on tiles of either parity
    starts = [(s, ti) for ti in range(1, tiles) for s in range(ns)]
    todo = [(p, k) for k in kinds for p in range(4)]
    for par in (0, 1):
        mine = [x for x in starts if x[1] % 2 == par]
        for j, (p, k) in enumerate(todo):
            if j < len(mine):
                slots.append((mine[j][0], mine[j][1] * TILE + p, k))
    # every position mod 64, every class: position 17 i mod 64 for i = 0, 1, .. visits all 64, so consecutive plants of a
    # stream are 17 samples apart; even streams start on the ragged last tile
    todo = [(17 * i % 64, k) for k in kinds for i in range(64)]
    per = (len(todo) + ns - 1) // ns
    for s in range(ns):
        t = ((n // TILE) * TILE if (s % 2 == 0 and n % TILE) else 0) + (0 if hist else 64)
        for p, k in todo[s * per: (s + 1) * per]:
            t += 16
            t += (p - t) % 64
            while (t >= TILE and t % TILE < 24) or t % TILE > TILE - 16:
                t += 64
            if t + 8 > n:            # past the ragged end: go on at the stream's start
                t = 64 + (p - 64) % 64
            assert t + 8 <= n, (s, t, n)
            slots.append((s, t, k))
    if hist:   # the first word of a stream counts when history stands before it
        slots += [(s, 12 + s, ("deep+", "in")[s % 2]) for s in range(ns)]
    # no two plants closer than 16 samples in a stream
    for s in range(ns):
        ts = sorted(t for s_, t, _ in slots if s_ == s)
        assert all(b - a >= 16 for a, b in zip(ts, ts[1:])), (s, [b - a for a, b in zip(ts, ts[1:]) if b - a < 16])
    return streams, h, plant(streams, slots, rng, lo, hi)


def _dense(rng, amp, ns=8, tiles=4, counts=None):
    """a flagged plant in every 32-sample word (counts: per tile, how many words get one; the others stay plain)"""
    lo, hi = AMPS[amp]
    n = tiles * TILE
    streams = rng.integers(lo, hi + 1, size=(ns, 2 * n), dtype=np.uint8)
    slots = []
    for s in range(ns):
        for ti in range(tiles):
            words = np.arange(64)
            if counts is not None:
                words = np.sort(rng.permutation(64)[: counts[s][ti]])
            for wd in words:
                if ti == 0 and wd == 0:
                    continue     # the first run of a stream without history is re-evaluated whole
                t = ti * TILE + 32 * int(wd) + 12 + int(rng.integers(0, 20))
                kind = ("deep", "band")[int(rng.integers(0, 2))]   # half of them deep inside: many wrong fast signs
                slots.append((s, t, kind))
    return streams, None, plant(streams, slots, rng, lo, hi, reuse=1 if counts is not None else 4)


PARTIAL_COUNTS = [[0, 31, 32, 33, 64], [0, 33, 64, 32, 31]]   # model-flagged words per tile of dense_partial's two streams


def _build(name, seed):
    for attempt in range(8):
        rng = np.random.default_rng([seed, attempt])
        if name.startswith("positions_"):
            st, h, pl = _positions(rng, name.split("_")[1])
        elif name == "with_history":
            st, h, pl = _positions(rng, "full", ns=2, n=2 * TILE, hist=True, kinds=("deep+", "deep-", "in", "out1.5"))
        elif name == "dense_partial":
            st, h, pl = _dense(rng, "full", ns=2, tiles=5, counts=PARTIAL_COUNTS)
        else:
            st, h, pl = _dense(rng, name.split("_")[1])
        c = _evaluate(Case(name, st, h, pl))
        if not margin_ok(c) or c.zeros:
            continue
        if name == "dense_partial":
            got = c.flagged_words().reshape(2, 5, 64).sum(axis=-1)
            if not np.array_equal(got, np.array(PARTIAL_COUNTS)):
                continue
        return c
    raise AssertionError(f"case {name}: no draw met its conditions")


NAMES = tuple(f"positions_{a}" for a in AMPS) + ("dense_full", "dense_low", "dense_partial", "with_history")


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return _build(name, 9000 + NAMES.index(name))


def cases():
    return [case(nm) for nm in NAMES]


# ---------------------------------------------------------------------------------------------------------------------
# what a list of the kernel's must satisfy: shared by the GPU tests and by the mutation checks of the CPU module
def listed_groups(entries, ns: int, words: int):
    """entries ((word << 4) | mask) -> [ns, 4 words] bool, and the number of words that appear more than once"""
    e = np.asarray(entries, dtype=np.uint64)
    w, m = (e >> np.uint64(4)).astype(np.int64), (e & np.uint64(15)).astype(np.int64)
    assert ((w >= 0) & (w < ns * words)).all(), "an entry names a word outside the launch"
    out = np.zeros((ns * words, 4), dtype=bool)
    for gidx in range(4):
        out[w[(m >> gidx) & 1 == 1], gidx] = True
    dup = w.size - np.unique(w).size
    return out.reshape(ns, words * 4), dup


def check_list(c: Case, listed: np.ndarray, fast_bits: np.ndarray, dup: int = 0):
    """listed [ns, n / 8] bool: the groups on the kernel's list; fast_bits [ns, n]: its signs before the fix-up."""
    assert dup == 0, f"{c.name}: {dup} words listed twice"
    ng = c.flagged.shape[1]
    assert not listed[:, ng:].any(), f"{c.name}: a group past the end of a stream is listed"
    listed = listed[:, :ng]
    missing = c.flagged & ~listed
    assert not missing.any(), f"{c.name}: {missing.sum()} groups inside the guard band are not listed, first {np.argwhere(missing)[:4]}"
    extra = listed & ~c.flagged
    gi = np.arange(listed.shape[1])
    allowed = ((8 * gi) % TILE < 8)[None, :] | (~c.valid)
    assert not (extra & ~allowed).any(), f"{c.name}: listed without cause: {np.argwhere(extra & ~allowed)[:4]}"
    bad = (fast_bits != c.bits) & ~np.repeat(listed, 8, axis=1)
    assert not bad.any(), f"{c.name}: {bad.sum()} wrong signs outside the list, first {np.argwhere(bad)[:4]}"


def model_entries(c: Case, flagged=None):
    """the list an ideal kernel would write: per tile, the flagged words in lane order (and the first run of a stream
    without history, which the kernel always lists)"""
    fl = (c.flagged if flagged is None else flagged) | ~c.valid
    ns, words = fl.shape[0], (fl.shape[1] + 3) // 4
    pad = np.zeros((ns, 4 * words), dtype=bool)
    pad[:, : fl.shape[1]] = fl
    m = (pad.reshape(ns, words, 4) * (1 << np.arange(4))).sum(axis=-1)
    return [[(int(s * words + w) << 4) | int(m[s, w]) for w in range(ti * 64, min(words, ti * 64 + 64)) if m[s, w]]
            for s in range(ns) for ti in range((words + 63) // 64)]
