"""Seeded one-step cases for the optimizer kernels of csrc/mcaq_optim.h
(mcaq_clip_adamw: two launches; mcaq_clip_adamw_fused: one), each with a
float64 reference and a numpy restatement of the kernel's own arithmetic.

A case is ONE step from a given state (errors do not compound): segments
(size, hyper-parameter group, project_abs, step count before this step), 1-4
groups of (lr, weight_decay, beta1, beta2, eps), max_norm and seeded fp32
arrays param / grad / exp_avg / exp_avg_sq (exp_avg_sq >= 0).

The reference (`reference`) is plain numpy in float64 with the hyper-parameters
as Python doubles; nothing is imported from the package's kernels:

    n_k   = sqrt(sum g_k^2)                   per tensor
    tot   = sqrt(sum n_k^2)                   the norm of the per-tensor norms
    coef  = min(max_norm / (tot + 1e-6), 1)   NaN propagates; no clip at max_norm <= 0
    g     = g * coef
    p     = p - lr wd p                       decoupled decay first
    m     = b1 m + (1 - b1) g;   v = b2 v + (1 - b2) g^2      from the clipped gradient
    p     = p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps),   t = step + 1 of the segment
    p     = |p|                               where the segment is flagged
    step  = step + 1

The comparison rule is PER ELEMENT, not per tensor:

    |got - ref| <= M * eps32 * A + tiny          tiny: fp32's smallest normal

with A the sum of the magnitudes of the reference expression's terms: |g_ref|
for the clipped gradient, b1 |m| + (1 - b1) |g_ref| for exp_avg, v_ref for
exp_avg_sq, |p| + |update term| for the parameter and the total norm itself.
NaN positions must be equal; where the reference is +-inf or zero, got == ref.
Where the reference's coefficient is exactly 1 (or nothing clips) g * 1 is g in
any IEEE arithmetic: `Case.grads_exact`, the gradients stay bit-equal.

fp32 ATen is NOT the yardstick here: torch's own fp32 CPU step (clip_grad_norm_
+ AdamW, 8 threads) measures 14.0 by this rule at chunks_256 (its norm alone is
13.7 eps32 off, and with it every clipped gradient), where the restatement of
the kernel's arithmetic below is at 1.4 there (at most 1.62 over all cases).
The yardstick is float64.

Inputs stay where float64 and fp32 mean the same thing: nonzero |g| and |m|
are >= 1e-12, v is 0 or >= 1e-24 and no g^2 overflows - but for the named
cases nan_one, inf_one, nan_no_clip and sq_overflow.  sq_overflow states the
kernel's defined behaviour: the squares are fp32, so |g| = 1e20 makes the total
inf (float64's is finite) and every finite gradient +-0, as torch's fp32
clip_grad_norm_ does; its reference squares with fp32's overflow.

`kernel_arith` restates mcaq_optim.h in numpy: fp32 squares, each (chunk,
segment) part summed in the kernel's lane order, the chunks folded in chunk
order, sqrtf, the fp32 coefficient; decay and moments evaluated in double and
rounded once; fp32 bc1, sqrtf(bc2), step size and denominator as in the update
loop.  It runs on the CPU only: to show that the rule can be met (at M / 2) and
as the base the mutations of test_optim_cases_cpu.py are applied to.
"""
import functools
import math

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
TINY = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
# M = 8.  The longest chain is v = b2 v + (1 - b2) g^2 on the clipped gradient g = g_in * coef: its relative
# error is twice g's plus the half ulp of its one rounding.  g's error is the coefficient's plus the half ulp of
# the product; the coefficient's is the total norm's plus two roundings (tot + 1e-6f, the division), so g carries
# the norm's error e_n plus three roundings of eps32 / 2: 2 (e_n + 1.5 eps32) + 0.5 eps32 = 2 e_n + 3.5 eps32 on
# v.  The norm halves the relative error of the sum of squares; that sum's error is one rounding per level of the
# in-chunk tree (4 sequential adds, 2 + 6 tree levels: a few eps32 / 2 at worst, well under 1 eps32 in rms) plus
# the sequential fold over up to 257 chunks, a random walk of rms ~ 0.25 eps32 sqrt(nchunk / 3) = 2.3 eps32 at
# 256 chunks - e_n ~ 1.2 eps32 there, 2 e_n + 3.5 eps32 ~ 6 eps32 at a bad draw, under 4 eps32 at a typical one.
# 8 leaves that chain inside the rule and no room for a second error of its size.
M_DEFAULT = 8.0
# (case, tensor kind) -> an M above the default, each with a derivation from the float64 reference (none needed).
M_NAMED = {}
CH, TH, E = 1024, 256, 4          # OPT_CH, OPT_TH, OPT_E of mcaq_optim.h
MAXSEG, MAXGROUPS, FUSED_MAX_CHUNKS = 64, 4, 256
KINDS = ("grad", "exp_avg", "exp_avg_sq", "param")
DEFAULT_HP = (1e-3, 1e-2, 0.9, 0.999, 1e-8)     # lr, weight_decay, beta1, beta2, eps


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _pow(b, t):
    """b^t for an integer-valued t in double (the kernel's pow_int is within an ulp or two of it)."""
    return math.pow(b, float(t)) if b > 0.0 else (1.0 if t == 0 else 0.0)


def _expand(per_seg, sizes, dtype=np.float64):
    return np.repeat(np.asarray(per_seg, dtype=dtype), sizes)


# ---------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------
def reference(sizes, seg_group, seg_abs, seg_step, groups, max_norm, P, G, Mo, V, fp32_squares=False):
    sizes = np.asarray(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (P, G, Mo, V))
    clip = max_norm > 0.0
    out = {}
    with np.errstate(all="ignore"):
        if clip:
            sq = g * g
            if fp32_squares:
                sq = np.where(sq > FLT_MAX, np.inf, sq)
            nk = np.sqrt(np.array([sq[a:b].sum() for a, b in zip(starts[:-1], starts[1:])]))
            tot = float(np.sqrt((nk * nk).sum()))
            c = max_norm / (tot + 1e-6)
            coef = c if (c != c or c < 1.0) else 1.0
            g = g * coef
            out["total_norm"], out["coef"] = tot, coef
        else:
            out["total_norm"], out["coef"] = None, None
        hp = [np.array([groups[gi][j] for gi in seg_group]) for j in range(5)]
        lr, wd, b1, b2, eps = (_expand(h, sizes) for h in hp)
        t = np.asarray(seg_step, dtype=np.float64) + 1.0
        bc1 = _expand([1.0 - _pow(groups[gi][2], tk) for gi, tk in zip(seg_group, t)], sizes)
        bc2 = _expand([1.0 - _pow(groups[gi][3], tk) for gi, tk in zip(seg_group, t)], sizes)
        p1 = p - lr * wd * p
        m1 = b1 * m + (1.0 - b1) * g
        v1 = b2 * v + (1.0 - b2) * g * g
        upd = (lr / bc1) * m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps)
        p2 = p1 - upd
        p2 = np.where(_expand(seg_abs, sizes, bool), np.abs(p2), p2)
    out.update(grad=g, exp_avg=m1, exp_avg_sq=v1, param=p2, steps=t)
    A = dict(grad=np.abs(g), exp_avg=b1 * np.abs(m) + (1.0 - b1) * np.abs(g), exp_avg_sq=v1,
             param=np.abs(p) + np.abs(upd), total_norm=out["total_norm"])
    return out, A


# ---------------------------------------------------------------------------
# the kernel's arithmetic, restated
# ---------------------------------------------------------------------------
def _piece_sum(sq, lo, hi):
    """One wave's sum of sq[lo:hi] (a segment's part of a chunk) in the kernel's order: four partial sums per
    lane over 256-element rounds while i + 192 < hi, the 64-stride tail into the first, (a0 + a1) + (a2 + a3),
    then the xor butterfly from 32 down (every lane ends with the same bits; lane 0's are stored)."""
    lane = np.arange(64)
    a = np.zeros((4, 64), dtype=np.float32)
    i = lo + lane
    while True:
        go = i + 192 < hi
        if not go.any():
            break
        for r in range(4):
            a[r, go] = a[r, go] + sq[i[go] + 64 * r]
        i = np.where(go, i + 256, i)
    while True:
        go = i < hi
        if not go.any():
            break
        a[0, go] = a[0, go] + sq[i[go]]
        i = np.where(go, i + 64, i)
    acc = (a[0] + a[1]) + (a[2] + a[3])
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ o]
    return acc[0]


def kernel_norm(sizes, G):
    """(per-tensor squared norms, total norm) as launch 1 + the head of launch 2 compute them, fp32."""
    starts = np.concatenate([[0], np.cumsum(sizes)])
    total, nseg = int(starts[-1]), len(sizes)
    g = _f32(G)
    with np.errstate(all="ignore"):
        sq = g * g
        seg_acc = np.zeros(nseg, dtype=np.float32)
        for c in range((total + CH - 1) // CH):          # chunk order: the fold of launch 2
            for k in range(nseg):
                lo, hi = max(int(starts[k]), c * CH), min(int(starts[k + 1]), (c + 1) * CH)
                part = _piece_sum(sq, lo, hi) if lo < hi else np.float32(0.0)
                seg_acc[k] = seg_acc[k] + part
        nk = np.sqrt(seg_acc)
        t2 = np.zeros(64, dtype=np.float32)
        t2[:nseg] = nk * nk                              # fmaf(nk, nk, 0)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            t2 = t2 + t2[lane ^ o]
        return seg_acc, np.sqrt(t2[0])


MUTATIONS = ("eps_in_bc", "coupled_l2", "decay_after", "shared_step", "group_row0", "no_1e6", "no_clamp",
             "moments_unclipped", "fp32_one_minus_beta2", "bc_at_t", "abs_next_segment", "abs_before_update")


def kernel_arith(sizes, seg_group, seg_abs, seg_step, groups, max_norm, P, G, Mo, V, mut=None):
    """The step as mcaq_optim.h evaluates it -> dict of fp32 arrays (and total_norm, steps).  `mut`: one of
    MUTATIONS, a wrong kernel."""
    assert mut is None or mut in MUTATIONS
    sizes = np.asarray(sizes)
    p, g_in, m, v = (_f32(a).copy() for a in (P, G, Mo, V))
    mn = np.float32(max_norm)
    clip = bool(mn > 0.0)
    out = {"total_norm": None}
    one = np.float32(1.0)
    if mut == "group_row0":
        seg_group = [0] * len(sizes)
    if mut == "shared_step":
        seg_step = [seg_step[0]] * len(sizes)
    if mut == "abs_next_segment":
        seg_abs = [0] + list(seg_abs[:-1])
    with np.errstate(all="ignore"):
        g = g_in
        if clip:
            _, tot = kernel_norm(sizes, g_in)
            c = mn / (tot if mut == "no_1e6" else tot + np.float32(1e-6))
            coef = c if (c != c or c < one or mut == "no_clamp") else one
            g = g_in * np.float32(coef)
            out["total_norm"] = np.float32(tot)
        step = _f32(seg_step) + one
        tb = step - one if mut == "bc_at_t" else step
        ss, bc2s = [], []
        for gi, tk in zip(seg_group, tb):
            lr, _, b1, b2, _ = groups[gi]
            bc1 = np.float32(1.0 - _pow(b1, tk))
            bc2s.append(np.sqrt(np.float32(1.0 - _pow(b2, tk))))
            ss.append(np.float32(lr / float(bc1)) if bc1 != 0 else np.float32(np.inf))
        ss, bc2s = _expand(ss, sizes, np.float32), _expand(bc2s, sizes, np.float32)
        hp = [_expand([groups[gi][j] for gi in seg_group], sizes) for j in range(5)]
        lr, wd, b1, b2, eps = hp
        omb2 = _expand([float(np.float32(1.0) - np.float32(groups[gi][3])) for gi in seg_group], sizes) \
            if mut == "fp32_one_minus_beta2" else 1.0 - b2
        lrwd = lr * wd
        flag = _expand(seg_abs, sizes, bool)
        pd, gd = p.astype(np.float64), g.astype(np.float64)
        gm = g_in.astype(np.float64) if mut == "moments_unclipped" else gd
        if mut == "coupled_l2":
            gm = (gm + wd * pd).astype(np.float32).astype(np.float64)
        elif mut != "decay_after":
            p = (pd - lrwd * pd).astype(np.float32)
        if mut == "abs_before_update":
            p = np.where(flag, np.abs(p), p)
        m1 = (b1 * m.astype(np.float64) + (1.0 - b1) * gm).astype(np.float32)
        v1 = (b2 * v.astype(np.float64) + omb2 * gm * gm).astype(np.float32)
        if mut == "eps_in_bc":
            denom = ((np.sqrt(v1).astype(np.float64) + eps).astype(np.float32) / bc2s)
        else:
            denom = ((np.sqrt(v1) / bc2s).astype(np.float64) + eps).astype(np.float32)
        p = p - ss * m1 / denom
        if mut == "decay_after":
            p = (p.astype(np.float64) - lrwd * p.astype(np.float64)).astype(np.float32)
        if mut != "abs_before_update":
            p = np.where(flag, np.abs(p), p)
    out.update(grad=g, exp_avg=m1, exp_avg_sq=v1, param=p, steps=step)
    return out


# ---------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------
def compare(got, ref, A, M):
    """(number of elements that miss the rule, largest err / (eps32 A) among the finite nonzero ones)."""
    got = np.atleast_1d(np.asarray(got)).astype(np.float64).reshape(-1)
    ref = np.atleast_1d(np.asarray(ref, dtype=np.float64)).reshape(-1)
    A = np.atleast_1d(np.asarray(A, dtype=np.float64)).reshape(-1)
    assert got.shape == ref.shape == A.shape
    with np.errstate(all="ignore"):
        nr, ng = np.isnan(ref), np.isnan(got)
        exact = ~nr & (np.isinf(ref) | (ref == 0.0))
        ruled = ~nr & ~exact
        err = np.abs(got - ref)
        bad = (nr != ng) | (exact & ~(got == ref)) | (ruled & ~(err <= M * EPS32 * A + TINY))
        ratio = np.where(ruled & ~ng & (A > 0.0), err / (EPS32 * A), 0.0)
    return int(bad.sum()), float(ratio.max()) if ratio.size else 0.0


# ---------------------------------------------------------------------------
# layout predicates (which branches of the kernels a layout reaches)
# ---------------------------------------------------------------------------
def _lane_trips(L, lane):
    """(rounds of the `i + 192 < hi` loop, trips of the 64-stride tail) of one lane on a part of L elements."""
    i, u, t = lane, 0, 0
    while i + 192 < L:
        i, u = i + 256, u + 1
    while i < L:
        i, t = i + 64, t + 1
    return u, t


def layout(sizes):
    sizes = [int(n) for n in sizes]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    total, nseg = int(starts[-1]), len(sizes)
    nchunk = (total + CH - 1) // CH
    seg_of = np.repeat(np.arange(nseg), sizes)
    pieces = []                                   # lengths of every (chunk, segment) part
    segs_per_chunk = []
    for c in range(nchunk):
        ks = np.unique(seg_of[c * CH:(c + 1) * CH])
        segs_per_chunk.append(len(ks))
        for k in ks:
            pieces.append(min(int(starts[k + 1]), (c + 1) * CH) - max(int(starts[k]), c * CH))
    pad = np.concatenate([seg_of, np.full((-total) % E, seg_of[-1])]).reshape(-1, E)
    quad = int((np.diff(pad, axis=1) != 0).sum(axis=1).max()) + 1
    trips = [_lane_trips(L, l) for L in pieces for l in (0, 63)]
    return dict(total=total, nseg=nseg, nchunk=nchunk, max_segs_per_chunk=max(segs_per_chunk),
                wave_rounds=-(-nseg // 4),                 # trips of the `kk += 4` loop of a wave
                scan_full_wave=nseg == 64, bc_lanes_to=64 + nseg, quad_segments=quad,
                fold_rounds=-(-nchunk // 8),                # trips of the `w0 += 8` fold
                unrolled=any(u > 0 for u, _ in trips),      # some lane runs an `i + 192 < hi` round
                not_unrolled=any(u == 0 and t > 0 for u, t in trips),    # some lane goes straight to the tail
                tail_after_unrolled=any(u > 0 and t > 0 for u, t in trips),
                tail_trips=max(t for _, t in trips),        # most 64-stride tail trips of a lane
                chunk_aligned_start=any(int(s) % CH == 0 for s in starts[1:-1]),
                one_launch=nchunk <= FUSED_MAX_CHUNKS, pieces=pieces)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
class Case:
    def __init__(self, name, why, sizes, seed, max_norm=0.5, groups=(DEFAULT_HP,), seg_group=None, seg_abs=None,
                 seg_step=None, gscale=1.0, fresh=False, fp32_squares=False, edit=None):
        n = len(sizes)
        self.name, self.why, self.sizes, self.seed = name, why, tuple(int(s) for s in sizes), seed
        self.groups = [tuple(float(x) for x in g) for g in groups]
        self.seg_group = list(seg_group) if seg_group is not None else [0] * n
        self.seg_abs = list(seg_abs) if seg_abs is not None else [0] * n
        self.seg_step = list(seg_step) if seg_step is not None else [float(3 + k % 5) for k in range(n)]
        self.fp32_squares = fp32_squares
        rng = np.random.default_rng(seed)
        total = int(sum(sizes))
        self.starts = np.concatenate([[0], np.cumsum(self.sizes)])
        self.P = rng.standard_normal(total).astype(np.float32)
        self.G = (rng.standard_normal(total) * gscale).astype(np.float32)
        if fresh:
            self.M, self.V = np.zeros(total, np.float32), np.zeros(total, np.float32)
        else:
            self.M = (rng.standard_normal(total) * 0.1 * gscale).astype(np.float32)
            self.V = (rng.uniform(1e-4, 1e-2, total) * gscale * gscale).astype(np.float32)
        self.max_norm = max_norm
        if edit is not None:
            edit(self, rng)
        self.max_norm = float(np.float32(self.max_norm))          # as the entry receives it
        self.clip = self.max_norm > 0.0
        self.ref, self.A = reference(*self.args(), fp32_squares=fp32_squares)
        self.grads_exact = not self.clip or self.ref["coef"] == 1.0
        self.finite = bool(np.isfinite(self.G).all())

    def args(self):
        return (self.sizes, self.seg_group, self.seg_abs, self.seg_step, self.groups, self.max_norm, self.P, self.G,
                self.M, self.V)

    def seg(self, a, k):
        return a[self.starts[k]:self.starts[k + 1]]

    def kernel_arith(self, mut=None):
        return kernel_arith(*self.args(), mut=mut)

    def M_of(self, kind):
        return M_NAMED.get((self.name, kind), M_DEFAULT)

    def check(self, got, M=None):
        """got: dict like kernel_arith's -> ({kind: elements that miss}, {kind: largest ratio})."""
        miss, ratio = {}, {}
        kinds = KINDS + (("total_norm",) if self.clip else ())
        for k in kinds:
            miss[k], ratio[k] = compare(got[k], self.ref[k], self.A[k], self.M_of(k) if M is None else M)
        if self.grads_exact:
            miss["grad"] += int((_f32(got["grad"]).view(np.uint32) != self.G.view(np.uint32)).sum())
        miss["steps"] = int((np.asarray(got["steps"], dtype=np.float64) != self.ref["steps"]).sum())
        return {k: v for k, v in miss.items() if v}, ratio


def _hp(**kw):
    d = dict(zip(("lr", "weight_decay", "beta1", "beta2", "eps"), DEFAULT_HP))
    d.update(kw)
    return tuple(d[k] for k in ("lr", "weight_decay", "beta1", "beta2", "eps"))


def _ref_norm(c):
    g = c.G.astype(np.float64)
    return math.sqrt(sum(float((c.seg(g, k) ** 2).sum()) for k in range(len(c.sizes))))


def _edit_groups4(c, rng):
    # the two projected segments hold |p| < lr of both signs: the update decides the sign before |.|
    for k in (2, 5):
        lr = c.groups[c.seg_group[k]][0]
        s = c.seg(c.P, k)
        s[:16] = (rng.uniform(0.05, 0.9, 16) * lr * np.where(np.arange(16) % 2, 1.0, -1.0)).astype(np.float32)


def _edit_beta2_0(c, rng):
    c.G[np.abs(c.G) < 1e-3] = np.float32(1e-3)            # g != 0 everywhere: the denominator is |g|


def _edit_fresh_tiny(c, rng):
    n = c.G.size
    c.G[:] = (10.0 ** rng.uniform(-9.0, -7.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)


def _edit_clip_inactive(c, rng):
    c.max_norm = 2.0 * _ref_norm(c)                       # the coefficient would be ~2 without its clamp


def _edit_clip_edge(c, rng):
    c.max_norm = float(np.float32(_ref_norm(c)))          # coef = tot / (tot + 1e-6): just under 1


def _edit_tiny_norm(c, rng):
    c.G[:] = (c.G.astype(np.float64) * (2e-6 / _ref_norm(c))).astype(np.float32)


def _edit_zero_grads(c, rng):
    c.G[:] = 0.0


def _edit_nan_one(c, rng):
    k = int(np.argmin(c.sizes))
    c.seg(c.G, k)[0] = np.nan


def _edit_inf_one(c, rng):
    c.seg(c.G, 1)[5] = np.inf


def _edit_sq_overflow(c, rng):
    idx = rng.choice(c.G.size, 7, replace=False)
    c.G[idx] = (np.where(np.arange(7) % 2, -1.0, 1.0) * 1e20).astype(np.float32)


_G4 = (_hp(lr=1e-3, weight_decay=0.0),
       _hp(lr=1e-2, weight_decay=0.1, beta1=0.8, beta2=0.99, eps=1e-6),
       _hp(lr=3e-2, weight_decay=0.05, beta1=0.95, beta2=0.9999, eps=1e-10),
       _hp(lr=2e-4, weight_decay=0.3, beta1=0.5, beta2=0.9, eps=1e-3))
_SMALL = (97, 300, 41, 700)


def _cfgs():
    c = {}

    def add(name, why, sizes, **kw):
        c[name] = (why, sizes, kw)

    # ---- layout: one group, default hyper-parameters, max_norm 0.5 (the clip is active)
    for n, why in ((1, "one element: one thread of one chunk, every other lane clamped to it"),
                   (1023, "one short of a chunk: the last thread holds 3 elements"),
                   (1024, "exactly one chunk"), (1025, "a second chunk of one element")):
        add("one_%d" % n, why, (n,))
    add("aligned_1024x2", "a segment starts on a chunk boundary", (1024, 1024))
    add("quad_span", "one thread's four elements lie in three segments; the next segment starts a chunk",
        (1022, 1, 1, 1, 5))
    add("lanes", "both sides of `i + 192 < hi` and the 64-stride tail", (63, 65, 255, 257, 256, 64, 192, 193))
    add("seg64_one_chunk", "64 segments of 16: the full-wave scan, 16 segments per wave in one chunk", (16,) * 64)
    add("seg64_ragged", "64 segments of 1-200 elements over several chunks; lanes 64-127 compute the bias "
        "corrections", tuple(1 + (37 * k * k + 11 * k) % 200 for k in range(64)))
    add("chunks_8", "8 chunks: one round of the `w0 += 8` fold", (8192,))
    add("chunks_9", "9 chunks: a second round of one chunk", (8193,))
    add("chunks_256", "256 chunks: the one-launch maximum", (261144, 1000))
    add("chunks_257", "257 chunks: only the two-launch entry takes it", (262145, 1000))
    # ---- hyper-parameters and steps
    add("groups_4", "8 segments over 4 groups (lr, wd, betas, eps all differ; group order is not segment order); "
        "project_abs on two segments with |p| < lr of both signs", (97, 300, 41, 700, 5, 260, 33, 129),
        groups=_G4, seg_group=(2, 0, 3, 1, 1, 2, 0, 3), seg_abs=(0, 0, 1, 0, 0, 1, 0, 0),
        seg_step=(3, 0, 7, 1, 12, 2, 5, 40), edit=_edit_groups4)
    add("wd0", "weight_decay 0: no decay", _SMALL, groups=(_hp(weight_decay=0.0),))
    add("beta1_0", "beta1 0: exp_avg is the clipped gradient, bc1 = 1", _SMALL, groups=(_hp(beta1=0.0),))
    add("beta2_0_eps0", "beta2 0 and eps 0: v = g^2, bc2 = 1, the denominator is |g| (g != 0 everywhere)", _SMALL,
        groups=(_hp(beta2=0.0, eps=0.0),), edit=_edit_beta2_0)
    add("fresh_tiny_g", "first step from zero moments, |g| in 1e-9 .. 1e-7 around eps = 1e-8", _SMALL,
        seg_step=(0, 0, 0, 0), fresh=True, edit=_edit_fresh_tiny)
    add("steps_distinct", "steps 0, 1, 9, 999, 99999: every segment its own bias corrections, pow_int's large "
        "exponents", (97, 300, 41, 700, 64), seg_step=(0, 1, 9, 999, 99999))
    # ---- clip edges
    add("clip_inactive", "norm at half of max_norm: the clamp at 1 holds and the gradients stay bit-equal", _SMALL,
        edit=_edit_clip_inactive)
    add("clip_edge", "max_norm equal to the fp32 norm: coef = tot / (tot + 1e-6), just under 1", _SMALL,
        gscale=0.02, edit=_edit_clip_edge)
    add("tiny_norm", "tot ~ 2e-6 against max_norm 1e-6: the `+ 1e-6` decides the coefficient", _SMALL,
        max_norm=1e-6, edit=_edit_tiny_norm)
    add("zero_grads", "all gradients zero: coef = 1, the moments decay and the parameters still move", _SMALL,
        edit=_edit_zero_grads)
    add("no_clip_0", "max_norm 0 at the C entry: no clip, total_norm left as it was", _SMALL, max_norm=0.0)
    add("no_clip_neg", "max_norm -1 at the C entry: no clip, total_norm left as it was", _SMALL, max_norm=-1.0)
    # ---- values
    add("nan_one", "one NaN gradient in the smallest segment: the total and so everything of every segment is NaN",
        _SMALL, edit=_edit_nan_one)
    add("inf_one", "one +inf gradient: total inf, coef 0, finite gradients +-0 (their moments only decay), the inf "
        "element NaN", _SMALL, edit=_edit_inf_one)
    add("nan_no_clip", "one NaN gradient without clipping: only that element is NaN", _SMALL, max_norm=0.0,
        edit=_edit_nan_one)
    add("sq_overflow", "|g| = 1e20: the fp32 squares overflow, total inf, every gradient +-0 (float64's total is "
        "finite; defined as fp32 clip_grad_norm_ behaves)", _SMALL, fp32_squares=True, edit=_edit_sq_overflow)
    return c


CFGS = _cfgs()
NAMES = list(CFGS)
FINITE = [n for n in NAMES if n not in ("nan_one", "inf_one", "nan_no_clip", "sq_overflow")]


@functools.lru_cache(maxsize=None)
def case(name):
    """Built once, read only."""
    why, sizes, kw = CFGS[name]
    return Case(name, why, sizes, 100 * (NAMES.index(name) + 1), **kw)
