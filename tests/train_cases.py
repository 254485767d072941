"""Seeded cases for the train-step kernels of csrc/mcaq_train.h at their own
entries, each with a float64 reference and the same restatement in fp32:

  mapper  mcaq_mapper_train_forward / _backward
  head    mcaq_head_train_backward (bilateral adjoint + complexity-MLP backward)
  smask   mcaq_smask_train_backward (plain mode)
  fold    mcaq_qat_smask_backward_multi (the soft mask folding the quantizer's
          slice partials and the bit-budget gradient)

The references restate the modules here (nothing is imported from the package's
kernels, and nothing casts to fp32 inside): the golden parameters cast to the
run's dtype, plain torch ops on the CPU, autograd for every gradient.  Each
case names the branch of the kernel it is there for and is built once.

The comparison rule, for tensor k of a case (ref: float64, cpu32: the same
restatement in fp32, got: the kernel):

    e32_k = max |cpu32_k - ref_k|
    S_k   = max(max |ref_k|, largest |ref| among the gradient tensors of the same module in this case)
    pass iff max |got_k - ref_k| <= min(M * max(e32_k, eps32 * S_k), 1e-3 * S_k),   M = 8

The measure is what an fp32 evaluation of this very case loses against
float64; the floor covers tensors that cancel to zero in exact arithmetic
(the BN-fed Linear biases; the whole g_c at n = 1 and n = 2, where the batch
normalisation's output does not depend on its input); the cap keeps the rule
no looser than 1e-3 of the scale.  M = 8: e32_k is one draw of a maximum over
as few as one to eight elements, and the kernels sum sequentially or in fixed
trees where ATen cascades - both small integer factors at <= ~1500 terms.

Inputs stay off the kinks: a ReLU / clamp / round whose argument lies within
rounding of its kink has another gradient in fp32 than in float64, which is
no kernel error.  For every gate argument the builder takes d = the largest
|fp32 - float64| difference of that argument and requires every argument
that is not a deliberate tie to lie further than 64 d from its kink; if one
does not, the next seed is taken (at most 32 per case, then it raises).

What the kernels define and the references state:
  * BatchNorm at n = 1 (torch raises): variance 0, the running variance takes
    the variance itself (map_stats: `nf > 1 ? var * nf / (nf - 1) : var`).
  * The temperature and the momentum reach the kernels as fp32 numbers; the
    references use those fp32 values (0.1 is not 0.1f).
  * The bit-budget gradient of a tile is dA / (nscales * B ht wt): the budget
    is the mean over the scales of each scale's own mean, so the kernel divides
    by the bit budget's scale count times THIS scale's tile count (`(dA *
    (1 / nscales)) * rn`), not by the launch's total tile count.  The fold
    cases use nscales = 3 with one segment so that dropping either factor shows.
  * Fold mode takes ragged grids: a pixel belongs to the tile of its nearest
    source index (qat_fold_band's band_start over nearest_src; the fold kernel's
    hlo / hhi / wlo / whi are the same map), so (1,22,26,5,6) is a fold case.
  * The bilateral's `+ 1e-8` is invisible in fp32: the centre tap's weight is
    exactly 1, so the denominator is >= 1 and den + 1e-8f == den.  No fp32
    evaluation can tell the mutation that drops it; test_train_cases_cpu pins
    that fact instead of a failing case.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from conftest import load_weights

EPS32 = float(np.finfo(np.float32).eps)
M_DEFAULT = 8.0
# (case, tensor) -> an M above the default, each with its explanation.
M_NAMED = {
    # Measured ratio 14.2.  grad.net.2.bias is +-sum_t gl(t), gl(t) = g_m(t) m (1 - m), two elements of one
    # magnitude.  The net's last bias is (4, 0), so m(tile) is 0.990 .. 0.998 at this case and an fp32 `1 - m`
    # (the kernel's `mt * (1.0f - mt)`; ATen's softmax backward cancels the same way in g - g y) carries
    # (eps32 / 2) / (1 - m) = 6e-6 .. 3e-5 relative error per tile.  From the float64 reference alone, the
    # first-order rms of that error over this case's 80 tiles is sqrt(sum_t (gl(t) (eps32 / 2) / (1 - m(t)))^2) =
    # 1.5e-6, 59 times the rule's floor eps32 * S = 2.5e-8 - while the fp32 restatement's own draw of this
    # two-element maximum happens to be 1.8e-8 .. 4.8e-8 here (it is 4e-7 .. 2e-6 at the other soft-mask cases,
    # where the kernel's ratio is 0.5 .. 1.5).  So the measure understates fp32's loss at this tensor of this
    # case; M covers the reference-derived rms (59 -> 64).  The bound stays 7.6e-6 of the scale.
    ("smask_33x41_t8x10", "grad.net.2.bias"): 64.0,
}
CAP = 1e-3                     # never looser than 1e-3 of the scale
MAX_SEEDS = 32
KINK_MARGIN = 64.0
MIN_B, MAX_B = 2.0, 8.0
MOM = float(np.float32(0.1))   # the momentum as the kernel receives it
TR_TPB = 64                    # tiles per mapper / complexity-MLP workgroup
LDS_LIMIT = 160 * 1024 - 1024

MAPPER_PARAMS = ["%d.%s" % (i, s) for i in (0, 1, 3, 4, 6, 7) for s in ("weight", "bias")] + ["9.weight", "9.bias"]
CMLP_PARAMS = ["%d.%s" % (i, s) for i in (0, 1, 3, 4, 6) for s in ("weight", "bias")]
SMASK_PARAMS = ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias"]


@functools.lru_cache(maxsize=None)
def _golden():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in load_weights().items()}


def weights(prefix, dtype):
    return {k[len(prefix):]: v.to(dtype) if v.dtype.is_floating_point else v.clone()
            for k, v in _golden().items() if k.startswith(prefix)}


def _rand(seed, *shape, normal=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) if normal else torch.rand(*shape, generator=g)


def _gate_clamp(x, lo, hi, exclusive):
    """clamp with torch's inclusive backward gate, or (mutation) an exclusive one."""
    if not exclusive:
        return x.clamp(lo, hi)
    inside = (x > lo) & (x < hi)
    return torch.where(inside, x, x.detach().clamp(lo, hi))


class Gate:
    """A gate argument of one run: its values, its kinks ('half': the
    round's n + .5) and the mask of the deliberate ties."""

    def __init__(self, arg, kinks, ties=None):
        self.arg, self.kinks, self.ties = arg.detach().double().reshape(-1), kinks, ties

    def distance(self):
        a = self.arg
        if self.kinks == "half":
            d = ((a - torch.floor(a)) - 0.5).abs()
        else:
            d = torch.stack([(a - k).abs() for k in self.kinks]).amin(0)
        if self.ties is not None:
            d = d[~self.ties.reshape(-1)]
        return d


def off_kinks(g64, g32):
    """(ok, report): every non-tie gate argument further than 64 d from its kink."""
    ok, rep = True, {}
    for k in g64:
        d = float((g64[k].arg - g32[k].arg).abs().max())
        dist = g64[k].distance()
        near = float(dist.min()) if dist.numel() else float("inf")
        rep[k] = (near, d)
        if not near > KINK_MARGIN * d:
            ok = False
    return ok, rep


# ---------------------------------------------------------------------------
# mapper
# ---------------------------------------------------------------------------
def temperature_arg(T):
    """The temperature as the host hands it to the kernel: floored to 0.1,
    fp32; 0 for None (no temperature)."""
    return 0.0 if T is None else float(np.float32(max(float(T), 0.1)))


def mapper_inputs(cfg, seed):
    n = cfg["n"]
    c = _rand(seed, n) * 1.2 - 0.1                    # some tiles outside the [0, 1] clamp
    if n <= 2:
        c = _rand(seed, n) * 0.8 + 0.1                # inside it: two clamped tiles would be one tile twice
    ties = torch.zeros(n, dtype=torch.bool)
    if cfg.get("ties"):
        for i, v in enumerate((0.0, 1.0, -0.1, 1.1)):     # 0 and 1: gradient passes; -0.1 / 1.1: zero
            c[3 + 7 * i] = v
        ties[3], ties[10] = True, True
    return dict(c=c, gbits=_rand(seed + 1, n, normal=True), c_ties=ties)


def mapper_run(cfg, inp, dtype, mut=None):
    n, T, rnd = cfg["n"], temperature_arg(cfg["T"]), cfg["round"]
    W = weights("bit_mapper.mapping_network.", dtype)
    P = [W[k].clone().requires_grad_(True) for k in MAPPER_PARAMS]
    Pd = dict(zip(MAPPER_PARAMS, P))
    c = inp["c"].to(dtype).clone().requires_grad_(True)
    cc = _gate_clamp(c, 0.0, 1.0, mut == "gate_c_exclusive")
    h = torch.stack([cc, cc ** 2, torch.log1p(cc)], dim=1)
    gates = {"c": Gate(c, (0.0, 1.0), inp["c_ties"])}
    out, group = {}, {}
    for lin, bn in ((0, 1), (3, 4), (6, 7)):
        a = F.linear(h, Pd["%d.weight" % lin], Pd["%d.bias" % lin])
        mean = a.mean(0)
        var = ((a - mean) ** 2).mean(0)               # biased: the normalisation's
        y = (a - mean) / torch.sqrt(var + 1e-5) * Pd["%d.weight" % bn] + Pd["%d.bias" % bn]
        unb = var * (n / (n - 1.0)) if n > 1 and mut != "running_var_biased" else var
        mean, unb = mean.detach(), unb.detach()
        if cfg["update_stats"] == 1:
            out["running_mean.%d" % bn] = (1.0 - MOM) * W["%d.running_mean" % bn] + MOM * mean
            out["running_var.%d" % bn] = (1.0 - MOM) * W["%d.running_var" % bn] + MOM * unb
        else:                                         # deferred: (mean, unbiased var) left in the work buffer
            out["running_mean.%d" % bn] = W["%d.running_mean" % bn]
            out["running_var.%d" % bn] = W["%d.running_var" % bn]
            out["rstat.mean.%d" % bn], out["rstat.var.%d" % bn] = mean, unb
        gates["relu%d" % bn] = Gate(y, (0.0,))
        h = torch.relu(y)
    o = torch.sigmoid(F.linear(h, Pd["9.weight"], Pd["9.bias"])).reshape(n)
    b = MIN_B + (MAX_B - MIN_B) * o
    if T > 0.0:
        b = b * T
    b = b + (b.clamp(MIN_B, MAX_B) - b).detach()      # straight-through clamp
    if rnd:
        gates["round"] = Gate(b, "half")
        b = b + (torch.round(b) - b).detach()         # straight-through round-half-even
    grads = torch.autograd.grad(b, [c] + P, inp["gbits"].to(dtype))
    out["bits"] = b.detach()
    out["g_c"] = grads[0]
    group["g_c"] = "mapper"
    for k, g in zip(MAPPER_PARAMS, grads[1:]):
        out["grad." + k] = g
        group["grad." + k] = "mapper"
    exact = {"num_batches_tracked.%d" % bn: int(W["%d.num_batches_tracked" % bn]) + (cfg["update_stats"] == 1)
             for bn in (1, 4, 7)}
    return out, gates, group, exact


# ---------------------------------------------------------------------------
# analyzer head
# ---------------------------------------------------------------------------
def head_inputs(cfg, seed):
    B, ht, wt = cfg["shape"]
    n = B * ht * wt
    kind = cfg.get("craw", "rand")
    if kind == "zeros":
        craw = torch.zeros(B, ht, wt)                 # C exactly 0: on the bound, the gate open
    elif kind == "const3":
        craw = torch.full((B, ht, wt), 3.0)           # C > 1: the gate closed
    else:
        craw = _rand(seed + 1, B, ht, wt) * 1.4 - 0.2     # some bilateral outputs outside the [0, 1] clamp
    return dict(phi=_rand(seed, n, 8), craw=craw, gC=_rand(seed + 2, B, ht, wt, normal=True))


def bilateral(c, mut=None):
    """morphology.py:309-354 (sigma_s 2, sigma_r 0.1, 5x5, replicate pad), every operation in c's dtype."""
    B, H, W = c.shape
    patches = F.unfold(F.pad(c.unsqueeze(1), (2, 2, 2, 2), mode="replicate"), 5)
    center = c.reshape(B, 1, H * W)
    co = torch.arange(5, dtype=c.dtype) - 2
    yy, xx = torch.meshgrid(co, co, indexing="ij")
    spatial = torch.exp(-(yy ** 2 + xx ** 2) / (2 * 2.0 ** 2)).reshape(1, -1, 1)
    w = spatial * torch.exp(-((patches - center) ** 2) / (2 * 0.1 ** 2))
    den = w.sum(dim=1) if mut == "bilateral_no_eps" else w.sum(dim=1) + 1e-8
    return ((w * patches).sum(dim=1) / den).reshape(B, H, W)


def head_run(cfg, inp, dtype, mut=None):
    B, ht, wt = cfg["shape"]
    n = B * ht * wt
    W = weights("complexity_analyzer.complexity_mlp.", dtype)
    P = [W[k].clone().requires_grad_(True) for k in CMLP_PARAMS]
    craw = inp["craw"].to(dtype).clone().requires_grad_(True)
    Cb = bilateral(craw, mut)
    C = _gate_clamp(Cb, 0.0, 1.0, mut == "gate_C_exclusive")
    gcraw, = torch.autograd.grad(C, craw, inp["gC"].to(dtype))
    gates = {"C": Gate(Cb, (0.0, 1.0), torch.ones(n, dtype=torch.bool) if cfg.get("craw") == "zeros" else None)}
    h = inp["phi"].to(dtype)
    for lin, ln, width in ((0, 1, 64), (3, 4, 32)):
        y = F.layer_norm(F.linear(h, P[CMLP_PARAMS.index("%d.weight" % lin)], P[CMLP_PARAMS.index("%d.bias" % lin)]),
                         (width,), P[CMLP_PARAMS.index("%d.weight" % ln)], P[CMLP_PARAMS.index("%d.bias" % ln)])
        gates["relu%d" % ln] = Gate(y, (0.0,))
        h = torch.relu(y)
    o = torch.sigmoid(F.linear(h, P[8], P[9])).reshape(n)
    grads = torch.autograd.grad(o, P, gcraw.reshape(n))
    out, group = {"gcraw": gcraw.reshape(n)}, {"gcraw": "head"}
    for k, g in zip(CMLP_PARAMS, grads):
        out["grad." + k] = g
        group["grad." + k] = "cmlp"
    return out, gates, group, {}


def head_bwd_fits(ht, wt):
    """The launcher's bound (head_segs): 53 floats of LDS per tile of one image."""
    return 53 * ht * wt * 4 <= LDS_LIMIT


# ---------------------------------------------------------------------------
# soft mask
# ---------------------------------------------------------------------------
def smask_inputs(cfg, seed):
    B, H, W, ht, wt = cfg["shape"]
    bits = _rand(seed, B, ht, wt) * 7.0 + 1.5         # some tiles outside [2, 8]
    ties = torch.zeros(B, ht, wt, dtype=torch.bool)
    if cfg.get("ties"):
        flat, tf = bits.reshape(-1), ties.reshape(-1)
        for i, v in enumerate((2.0, 8.0, 1.5, 9.0)):      # 2 and 8: open; 1.5 / 9: closed
            flat[1 + 5 * i] = v
        tf[1], tf[6] = True, True
    inp = dict(bits=bits, bits_ties=ties, absmean=_rand(seed + 1, B, H, W))
    if cfg.get("C"):
        nsl = (cfg["C"] + 31) // 32
        inp["qwork"] = _rand(seed + 2, 2 * nsl, B, H, W, normal=True)     # [grad m partials | grad_bits partials]
        inp["avg"], inp["g_avg"], inp["g_loss"] = torch.tensor(4.625), torch.tensor(0.75), torch.tensor(-1.5)
    else:
        inp["gm"] = _rand(seed + 2, B, H, W, normal=True)
    return inp


def nearest_index(n_in, n_out):
    """F.interpolate(nearest)'s source index of every output, read off ATen itself."""
    src = torch.arange(n_in, dtype=torch.float64).reshape(1, 1, n_in, 1)
    return F.interpolate(src, size=(n_out, 1), mode="nearest").reshape(n_out).long()


def pool_windows(n_in, n_out):
    """adaptive_avg_pool2d's windows [floor(i n / o), ceil((i + 1) n / o))."""
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def smask_plane(bits, absmean, P, smooth, mut=None):
    """quantization.py:213-239 on (bits, |x| mean) -> m(p) (B, 1, H, W); the hidden pre-activations."""
    B, H, W = absmean.shape
    ht, wt = bits.shape[-2:]
    with torch.no_grad():
        if mut == "pool_floor":
            act = F.avg_pool2d(absmean.unsqueeze(1), (H // ht, W // wt))[:, :, :ht, :wt]
        else:
            act = F.adaptive_avg_pool2d(absmean.unsqueeze(1), (ht, wt))
        act = act / (act.amax(dim=(2, 3), keepdim=True) + 1e-8)
    f = (bits.unsqueeze(1) - 2.0) / 6.0
    pre = F.conv2d(torch.cat([_gate_clamp(f, 0.0, 1.0, mut == "gate_bits_exclusive"), act], dim=1), P[0], P[1],
                   padding=1)
    logits = F.conv2d(torch.relu(pre), P[2], P[3])
    m = torch.softmax(logits, dim=1)[:, :1]
    if mut == "nearest_block":
        ih = (torch.arange(H) // max(H // ht, 1)).clamp(max=ht - 1)
        iw = (torch.arange(W) // max(W // wt, 1)).clamp(max=wt - 1)
        up = m[:, :, ih][:, :, :, iw]
    else:
        up = F.interpolate(m, size=(H, W), mode="nearest")
    pad = F.pad(up, (2, 2, 2, 2)) if mut == "zero_pad" else F.pad(up, (2, 2, 2, 2), mode="replicate")
    return F.conv2d(pad, smooth), f, pre


def smask_run(cfg, inp, dtype, mut=None):
    B, H, W, ht, wt = cfg["shape"]
    Wt = weights("soft_mask.", dtype)
    P = [Wt[k].clone().requires_grad_(True) for k in SMASK_PARAMS]
    bits = inp["bits"].to(dtype).clone().requires_grad_(True)
    absmean = inp["absmean"].to(dtype)
    m, f, pre = smask_plane(bits, absmean, P, Wt["smooth_kernel"], mut)
    out, group = {}, {}
    if cfg.get("C"):
        # the fold: slice partials in slice order -> grad m(p) and the pixel
        # sums of the quantizer's grad_bits; a pixel belongs to the tile of its
        # nearest source index; every tile gets the bit-budget constant
        q = inp["qwork"].to(dtype)
        nsl = q.shape[0] // 2
        gm, fpix = q[0], q[nsl]
        for k in range(1, nsl):
            gm, fpix = gm + q[k], fpix + q[nsl + k]
        rh = F.one_hot(nearest_index(ht, H), ht).to(dtype)      # (H, ht)
        rw = F.one_hot(nearest_index(wt, W), wt).to(dtype)
        gbq = torch.einsum("hi,bhw,wj->bij", rh, fpix, rw)
        dA = inp["g_avg"].to(dtype) + inp["g_loss"].to(dtype) * (2.0 * (inp["avg"].to(dtype) - cfg["target"]))
        count = B * ht * wt if mut == "budget_scale_count" else cfg["nscales"] * B * ht * wt
        const = dA / count
    else:
        gm = inp["gm"].to(dtype)
    grads = torch.autograd.grad(m, [bits] + P, gm.unsqueeze(1))
    out["g_bits"] = (const + gbq) + grads[0] if cfg.get("C") else grads[0]
    group["g_bits"] = "smask"
    for k, g in zip(SMASK_PARAMS, grads[1:]):
        out["grad." + k] = g
        group["grad." + k] = "smask"
    gates = {"bits": Gate(f, (0.0, 1.0), inp["bits_ties"]), "hidden": Gate(pre, (0.0,))}
    return out, gates, group, {}


def smask_lds_bytes(H, W, ht, wt, stage, fold=False):
    """smask_lds_bytes of csrc/mcaq_train.h."""
    base = (22 * ht * wt + 64 + 1024 + 176 + H * wt + H * W) * 4 + 2 * (ht + wt) * 4
    st = ((base // 4 + 3) & ~3) * 4 + H * W * 4 if stage else base
    return st + (H * W + ht * W + ht * wt) * 4 if fold else st


def smask_predicates(cfg):
    """The host- and kernel-side branch predicates of a soft-mask case."""
    B, H, W, ht, wt = cfg["shape"]
    off = cfg.get("offset", 0)
    fold = bool(cfg.get("C"))
    if fold:
        staged = (H * W) % 4 == 0 and off == 0
        qoff = cfg.get("qoffset", 0)
        vec = (H * W) % 4 == 0 and (B * H * W) % 4 == 0 and qoff == 0
    else:
        staged = (H * W) % 4 == 0 and off == 0 and smask_lds_bytes(H, W, ht, wt, True) <= LDS_LIMIT
        vec = None
    wins = pool_windows(W, wt)
    hwins = pool_windows(H, ht)
    row4 = [staged and ((W | a | (b - a)) & 3) == 0 for a, b in wins]
    overlap = any(wins[i][1] > wins[i + 1][0] for i in range(wt - 1)) or \
        any(hwins[i][1] > hwins[i + 1][0] for i in range(ht - 1))
    iw = nearest_index(wt, W)
    blocks_w = torch.bincount(iw, minlength=wt)
    blocks_h = torch.bincount(nearest_index(ht, H), minlength=ht)
    starts_w = [int((iw == j).nonzero()[0]) for j in range(wt)]
    up4 = [staged and ((W | s | int(n)) & 3) == 0 for s, n in zip(starts_w, blocks_w)]
    return dict(staged=staged, fold_vec=vec, pool_row4_all=all(row4), pool_row4_any=any(row4),
                up_row4_all=all(up4), up_row4_any=any(up4), pixel_pass=staged and W >= 8,
                ragged=H % ht != 0 or W % wt != 0, overlap=overlap,
                uneven=len(set(blocks_w.tolist())) > 1 or len(set(blocks_h.tolist())) > 1,
                tiles=ht * wt, images=B, w_lt5=W < 5,
                fits=smask_lds_bytes(H, W, ht, wt, True, fold) <= LDS_LIMIT if fold else
                smask_lds_bytes(H, W, ht, wt, staged) <= LDS_LIMIT)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
RUN = {"mapper": (mapper_inputs, mapper_run), "head": (head_inputs, head_run), "smask": (smask_inputs, smask_run),
       "fold": (smask_inputs, smask_run)}


class Case:
    def __init__(self, name, kind, why, cfg, base_seed):
        self.name, self.kind, self.why, self.cfg = name, kind, why, cfg
        make, run = RUN[kind]
        for seed in range(base_seed, base_seed + MAX_SEEDS):
            inp = make(cfg, seed)
            ref, g64, group, exact = run(cfg, inp, torch.float64)
            c32, g32, _, _ = run(cfg, inp, torch.float32)
            ok, rep = off_kinks(g64, g32)
            if ok:
                break
        else:
            raise RuntimeError("case %s: no seed in %d keeps every gate argument off its kink" % (name, MAX_SEEDS))
        self.seed, self.tries, self.inp, self.kinks = seed, seed - base_seed + 1, inp, rep
        self.ref = {k: v.detach().double() for k, v in ref.items()}
        self.cpu32 = {k: v.detach() for k, v in c32.items()}
        self.group, self.exact = group, exact
        self.e32 = {k: float((self.cpu32[k].double() - self.ref[k]).abs().max()) for k in self.ref}
        gmax = {}
        for k, g in group.items():
            gmax[g] = max(gmax.get(g, 0.0), float(self.ref[k].abs().max()))
        self.S = {k: max(float(self.ref[k].abs().max()), gmax.get(group.get(k), 0.0)) for k in self.ref}

    def mutated32(self, mut):
        """The fp32 restatement with one mutation: stands in for a wrong kernel."""
        return {k: v.detach() for k, v in RUN[self.kind][1](self.cfg, self.inp, torch.float32, mut)[0].items()}

    def measure(self, k):
        return max(self.e32[k], EPS32 * self.S[k])

    def bound(self, k, M=None, extra=0.0):
        """extra: an absolute allowance the caller explains (the one fp32
        rounding of `start + g` when the entry accumulates)."""
        if M is None:
            M = M_NAMED.get((self.name, k), M_NAMED.get(k, M_DEFAULT))
        return min(M * self.measure(k), CAP * self.S[k]) + extra

    def error(self, k, got):
        return float((got.detach().double().cpu().reshape(self.ref[k].shape) - self.ref[k]).abs().max())

    def ratio(self, k, got):
        err, m = self.error(k, got), self.measure(k)
        return err / m if m > 0.0 else (0.0 if err == 0.0 else float("inf"))

    def failures(self, got, M=None, extra=None):
        """The tensors of `got` (name -> tensor) that miss the rule."""
        bad = []
        for k in self.ref:
            err = self.error(k, got[k])
            if not err <= self.bound(k, M, (extra or {}).get(k, 0.0)):     # a NaN fails
                bad.append((k, err, self.bound(k, M), self.ratio(k, got[k])))
        return bad


def _mapper_cfgs():
    c = {}
    why_n = {1: "one tile: BatchNorm at n = 1 as the kernel defines it", 2: "two tiles: xhat = +-1, g_c cancels to zero",
             15: "one short of a 16-tile MFMA block", 16: "exactly one 16-tile MFMA block", 17: "one past a 16-tile block",
             63: "one short of the 64-tile workgroup", 64: "exactly one workgroup", 65: "two workgroups, the second one tile",
             130: "three workgroups, the last two tiles"}
    for n, why in why_n.items():
        c["mapper_n%d" % n] = (why, dict(n=n, T=None, round=1, update_stats=1))
    for n in (2, 17, 130):
        for T, tn, tw in ((0.05, "t005", "temperature 0.05 floored to 0.1 by the host: every bit clamps to the minimum"),
                          (2.5, "t25", "temperature 2.5 saturates the upper clamp; the STE passes the gradient")):
            for rnd in (0, 1):
                c["mapper_n%d_%s_%s" % (n, tn, "round" if rnd else "cont")] = (
                    tw + ("" if rnd else "; continuous bits"), dict(n=n, T=T, round=rnd, update_stats=1))
    for n in (1, 16, 64, 65, 130):
        c["mapper_n%d_deferred" % n] = ("update_stats 2: (mean, unbiased var) left in the work buffer",
                                        dict(n=n, T=None, round=n % 2, update_stats=2))
    c["mapper_n65_ties"] = ("c exactly 0.0 and 1.0 (gradient passes) and -0.1 / 1.1 (gradient zero)",
                            dict(n=65, T=None, round=1, update_stats=1, ties=True))
    return c


def _head_cfgs():
    c = {}
    for shape, why in (((1, 1, 1), "1x1 grid: every tap range clamped on both sides"),
                       ((1, 1, 7), "one row: the vertical tap ranges clamped on both sides"),
                       ((2, 3, 2), "3x2 grids: no tile has an unclamped tap range"),
                       ((1, 5, 5), "the first grid with an unclamped centre"),
                       ((2, 5, 7), "two images, 70 tiles: a workgroup boundary inside the second image"),
                       ((1, 9, 8), "72 tiles: a workgroup boundary inside an image"),
                       ((3, 8, 8), "exactly 3 workgroups"),
                       ((1, 27, 28), "756 tiles: 12 workgroups, the last one partial"),
                       ((1, 24, 32), "768 tiles: exactly at the 53-float-per-tile LDS bound (inclusive)")):
        c["head_%dx%dx%d" % shape] = (why, dict(shape=shape))
    c["head_zeros"] = ("craw all zeros: C exactly 0, the gate open", dict(shape=(2, 5, 7), craw="zeros"))
    c["head_const3"] = ("craw constant 3.0: C > 1, the gradient zero", dict(shape=(2, 5, 7), craw="const3"))
    return c


def _smask_cfgs():
    c = {}
    for name, shape, why, kw in (
            ("4x4_t1", (1, 4, 4, 1, 1), "W < 5: every column an edge column, both-sided tap_range; one tile", {}),
            ("5x7_t1", (1, 5, 7, 1, 1), "H*W odd: unstaged; W < 8; one interior row", {}),
            ("8x8_t2", (2, 8, 8, 2, 2), "staged; W = 8, the smallest per-pixel horizontal pass; tiles 4 wide: row_sum4", {}),
            ("20x20_t4", (2, 20, 20, 4, 4), "staged; tiles 5 wide: scalar column sums beside a staged plane", {}),
            ("20x20_t4_off1", (2, 20, 20, 4, 4), "the same, base 1 float off 16 bytes: unstaged by alignment only",
             dict(offset=1)),
            ("21x23_t5", (2, 21, 23, 5, 5), "ragged and unstaged: overlapping pooling windows, uneven upsample blocks", {}),
            ("22x26_t5x6", (1, 22, 26, 5, 6), "ragged and staged (572 % 4 == 0)", {}),
            ("36x36_t8", (1, 36, 36, 8, 8), "ragged, staged, W % 4 == 0: aligned and unaligned blocks in one row", {}),
            ("33x41_t8x10", (1, 33, 41, 8, 10), "the hook's own ragged shape", {}),
            ("36x36_t33", (1, 36, 36, 33, 33), "1089 tiles: the tile loops' second round; blocks of 1-2 pixels", {}),
            ("20x20_t5_b3", (3, 20, 20, 5, 5), "three images: per-image partials and their reduction", {}),
            ("20x20_t5_ties", (1, 20, 20, 5, 5), "bits exactly 2.0 and 8.0 (open) and 1.5 / 9.0 (closed)",
             dict(ties=True))):
        c["smask_" + name] = (why, dict(shape=shape, **kw))
    return c


def _fold_cfgs():
    c = {}
    for name, shape, C, why, kw in (
            ("c40", (1, 20, 20, 5, 5), 40, "2 slices: a partial group of the 4-slice load rounds", {}),
            ("c160", (1, 20, 20, 5, 5), 160, "5 slices: two load rounds", {}),
            ("16x16_b2", (2, 16, 16, 4, 4), 64, "16-byte groups; two images", {}),
            ("18x18_qoff1", (1, 18, 18, 3, 3), 64, "the partials 1 float off 16 bytes: the scalar path by alignment",
             dict(qoffset=1)),
            ("15x15", (1, 15, 15, 3, 3), 64, "B*H*W = 225, no multiple of 4: the scalar path, |x| unstaged", {}),
            ("22x26_t5x6", (1, 22, 26, 5, 6), 40, "ragged grid: tiles by nearest source index", {}),
            ("20x20_ties", (1, 20, 20, 5, 5), 40, "bits on the clamp's bounds under the fold", dict(ties=True))):
        c["fold_" + name] = (why, dict(shape=shape, C=C, target=4.0, nscales=3, **kw))
    return c


KINDS = {"mapper": _mapper_cfgs(), "head": _head_cfgs(), "smask": _smask_cfgs(), "fold": _fold_cfgs()}
CFGS = {name: (kind, why, cfg) for kind, d in KINDS.items() for name, (why, cfg) in d.items()}
NAMES = list(CFGS)


def names(kind):
    return list(KINDS[kind])


@functools.lru_cache(maxsize=None)
def case(name):
    """Built once, read only."""
    kind, why, cfg = CFGS[name]
    return Case(name, kind, why, cfg, 1000 * (NAMES.index(name) + 1))
