"""Inputs for the percentile-calibration kernels (csrc/mcaq_pct.h) and a
sort-based restatement of torch.quantile's rule (SURVEY App. A rule 10) that
returns the four order statistics and the interpolated value per channel.
Pure numpy / torch on the CPU; tests/test_percentile_cases_cpu.py proves that
every case reaches the branch its name claims, tests/test_percentile_gpu.py
runs mcaq_percentile on all of them.

The quantiles are the reference's (quantization.py:436-480): 0.01 % and
99.99 %, i.e. q = 0.01 / 100 and 99.99 / 100 as Python floats, rounded to
fp32 by torch.quantile."""
import collections
from fractions import Fraction

import numpy as np
import torch

f32 = np.float32
Q_LO, Q_HI = 0.01 / 100, 99.99 / 100

# x: CPU tensor (B, C, H, W) of the case's dtype; per_tensor: the whole tensor
# is one channel; offset: elements by which the device copy's base is moved off
# a 16-byte boundary (the copy stays contiguous)
Case = collections.namedtuple("Case", "name x per_tensor offset")


# ---- the key of csrc/mcaq_pct.h (unsigned order = value order, -0 -> +0)
def key_of(v):
    u = np.ascontiguousarray(v, dtype=f32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def bin0(v):
    """First-level bin (top 12 key bits)."""
    return key_of(v) >> 20


# ---- rule 10
def ranks(n, q):
    """(floor(rank), ceil(rank), w) with rank = fp32(q) * (n - 1) in fp32."""
    r = f32(q) * f32(n - 1)
    assert r.dtype == f32
    lo = np.floor(r)
    return int(lo), int(np.ceil(r)), f32(r - lo)


def _round_f32(exact):
    """The fp32 nearest to a Fraction, ties to even."""
    c = f32(float(exact))
    cands = {float(c), float(np.nextafter(c, f32(-np.inf))), float(np.nextafter(c, f32(np.inf)))}
    best = None
    for v in sorted(cands):
        if not np.isfinite(v):
            continue
        d = abs(Fraction(v) - exact)
        even = (int(f32(v).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, v, even)
    return f32(best[1])


def fma32(a, b, c):
    """fp32 fused multiply-add a * b + c, one rounding."""
    a, b, c = f32(a), f32(b), f32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return f32(a * b + c)          # inf / nan by the IEEE rules; no rounding involved
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        with np.errstate(all="ignore"):
            return f32(a * b + c)          # the sign of an exact zero
    r = _round_f32(exact)
    big = Fraction(float(np.finfo(f32).max)) + Fraction(2) ** 103       # halfway to 2^128
    if abs(exact) >= big:
        return f32(np.inf) if exact > 0 else f32(-np.inf)
    return r


def lerp32(a, b, w):
    """ATen's lerp: w < 0.5 -> fma(w, b - a, a), else fma(-(b - a), 1 - w, b)."""
    a, b, w = f32(a), f32(b), f32(w)
    with np.errstate(all="ignore"):
        d = f32(b - a)
        if w < f32(0.5):
            return fma32(w, d, a)
        return fma32(f32(-d), f32(f32(1) - w), b)


def restate(rows, q_lo=Q_LO, q_hi=Q_HI):
    """rows: (C, N) fp32 array.  Returns (stats (C, 4): the order statistics
    floor(r_lo), ceil(r_lo), floor(r_hi), ceil(r_hi); lo (C,), hi (C,)).  A
    NaN anywhere in a row makes its lo and hi NaN (torch.quantile)."""
    rows = np.ascontiguousarray(rows, dtype=f32)
    C, N = rows.shape
    stats = np.zeros((C, 4), f32)
    lo = np.zeros(C, f32)
    hi = np.zeros(C, f32)
    a0, a1, wa = ranks(N, q_lo)
    b0, b1, wb = ranks(N, q_hi)
    for c in range(C):
        s = np.sort(rows[c])           # NaN sorts last
        stats[c] = [s[a0], s[a1], s[b0], s[b1]]
        if np.isnan(rows[c]).any():
            lo[c] = hi[c] = np.nan
        else:
            lo[c] = lerp32(s[a0], s[a1], wa)
            hi[c] = lerp32(s[b0], s[b1], wb)
    return stats, lo, hi


def rows_of(case):
    """(C, N) fp32 rows of a case, as _calibrate_percentile forms them."""
    x = case.x.float()
    if case.per_tensor:
        return x.reshape(1, -1)
    return x.transpose(0, 1).flatten(1)


def expected(case):
    """torch.quantile over the full rows: (lo, hi) fp32 arrays."""
    r = rows_of(case)
    return (torch.quantile(r, Q_LO, dim=1).numpy(), torch.quantile(r, Q_HI, dim=1).numpy())


def same(a, b):
    """np.array_equal with NaN == NaN and -0 == +0."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def find_exact_rank_n(lo=4097, hi=1 << 20):
    """Smallest N in [lo, hi) for which both ranks are exact integers > 0."""
    for n in range(lo, hi):
        a0, a1, _ = ranks(n, Q_LO)
        b0, b1, _ = ranks(n, Q_HI)
        if a0 == a1 and b0 == b1 and a0 > 0:
            return n
    raise AssertionError("no exact-rank N")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


TIES_SHAPE = (2, 5, 48, 48)       # N = 4608 (two chunks a channel): the ranks are 0, 1, N-2, N-1
TIES = ("constant", "two_valued", "low_bits", "four_bins", "straddle")


def _ties():
    B, C, H, W = TIES_SHAPE
    N = B * H * W
    g = np.random.default_rng(77)
    rows = np.zeros((C, N), f32)
    rows[0] = 1.5
    rows[1] = np.where(g.random(N) < 0.5, f32(-1.0), f32(2.0))
    rows[2] = (np.uint32(0x3F800000) | g.integers(0, 256, N).astype(np.uint32)).view(f32)
    mid = (g.random(N) * 1.8 - 0.9).astype(f32)
    rows[3] = mid
    rows[3, :4] = [-8.0, -4.0, 4.0, 8.0]
    rows[4] = mid
    rows[4, :4] = [-2.0, np.nextafter(f32(-2.0), f32(0)), np.nextafter(f32(2.0), f32(0)), 2.0]
    for c in range(C):
        g.shuffle(rows[c])
    x = torch.from_numpy(rows.reshape(C, B, H, W)).transpose(0, 1).contiguous()
    return x


def _zeros():
    N = 1024
    g = np.random.default_rng(78)
    rows = np.zeros((2, N), f32)
    # channel 0: subnormals at the outer ranks, then zeros of both signs
    rows[0] = np.where(g.random(N) < 0.5, f32(-0.0), f32(0.0))
    rows[0, :4] = [-2e-40, -0.0, 0.0, 3e-40]
    # channel 1: nothing below zero - the low ranks are zeros of either sign,
    # the high ranks the two largest subnormals
    rows[1] = np.where(g.random(N) < 0.5, f32(-0.0), f32(0.0))
    rows[1, :6] = [1e-45, 4e-45, 1e-41, 2e-41, -0.0, 0.0]
    for c in range(2):
        g.shuffle(rows[c])
    return torch.from_numpy(rows.reshape(2, 1, 32, 32)).transpose(0, 1).contiguous()


def _nonfinite():
    N = 1024
    g = np.random.default_rng(79)
    rows = g.standard_normal((4, N)).astype(f32)
    rows[0, :4] = [-np.inf, -np.inf, np.inf, np.inf]     # both ranks of each end
    rows[1, 500] = np.nan                               # one NaN
    rows[2, :2] = [-np.inf, np.inf]                     # one rank of each end
    for c in range(4):
        g.shuffle(rows[c])
    return torch.from_numpy(rows.reshape(4, 1, 32, 32)).transpose(0, 1).contiguous()


def _build():
    out = []
    ref = torch.randn(2, 8, 32, 32, generator=_gen(1)) * 1.5
    # a slice of a wider map, made contiguous; its device copy starts one
    # element past a 16-byte boundary, so every run has a scalar head and tail
    odd = (torch.randn(3, 5, 20, 24, generator=_gen(2)) * 2.0)[..., 3:23].contiguous()
    out.append(Case("ref_shape", ref, False, 0))
    out.append(Case("odd", odd, False, 1))
    out.append(Case("odd_hw", torch.randn(2, 3, 13, 17, generator=_gen(3)), False, 0))   # runs of 221 elements
    out.append(Case("n6400", torch.randn(1, 4, 80, 80, generator=_gen(4)), False, 0))
    n = find_exact_rank_n()
    h = next(d for d in range(int(n ** 0.5), 0, -1) if n % d == 0)
    out.append(Case("exact_rank", torch.randn(1, 2, h, n // h, generator=_gen(5)), False, 0))
    out.append(Case("tiny_n1", torch.randn(1, 3, 1, 1, generator=_gen(6)), False, 0))
    out.append(Case("tiny_n2", torch.randn(2, 3, 1, 1, generator=_gen(7)), False, 0))
    out.append(Case("ties", _ties(), False, 0))
    out.append(Case("zeros", _zeros(), False, 0))
    out.append(Case("nonfinite", _nonfinite(), False, 0))
    s = torch.randn(4, 2, 160, 160, generator=_gen(8))
    s[:, 1] = torch.nn.functional.silu(s[:, 1] * 3.0)      # the SiLU plateau: over a tenth of the channel in one bin
    out.append(Case("sampled", s, False, 0))
    out.append(Case("per_tensor", ref, True, 0))
    for dt, tag in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        out.append(Case("half_ref_shape_" + tag, ref.to(dt), False, 0))
        out.append(Case("half_odd_" + tag, odd.to(dt), False, 1))
    return out


_CASES = None


def cases():
    """All cases, built once."""
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def case(name):
    return next(c for c in cases() if c.name == name)


def names():
    return [c.name for c in cases()]
