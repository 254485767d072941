"""The smoothness term of the QAT loss (MCAQYOLOLoss.compute_smoothness_loss,
models/mcaq_yolo.py:86-107) fused into the multi-scale train step
(train_step.FUSED_SMOOTHNESS): the forward value from the bit-budget
workgroup, the gradient as the tile constant s kappa of the fused soft-mask
backward.  The oracle is the torch expression of the definition, written
here, with autograd for the gradient:

    S_k = (sum |b[:,1:,:] - b[:,:-1,:]| + sum |b[:,:,1:] - b[:,:,:-1]|) / max(1, n_edges_k)
    n_edges_k = B ((ht - 1) wt + ht (wt - 1)),   L_smooth = (sum_k S_k) / n_scales
"""
import ctypes

import pytest
import torch

from test_concurrent_scales_gpu import _close, _feats, _same
from test_train_fused_gpu import _hooks

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _expr(maps, dtype=torch.float64):
    tot = 0.0
    for b in maps:
        b = b.to(dtype)
        B, ht, wt = b.shape
        n_edges = B * ((ht - 1) * wt + ht * (wt - 1))
        tot = tot + ((b[:, 1:, :] - b[:, :-1, :]).abs().sum() + (b[:, :, 1:] - b[:, :, :-1]).abs().sum()) / max(1, n_edges)
    return tot / len(maps)


# ---------------------------------------------------------------------------
# 1. the forward kernels alone, through the C ABI
# ---------------------------------------------------------------------------
# (B, ht, wt) of every segment.  3 x 19 x 19 = 1,083 tiles: more than one
# 1024-thread stride of the stand-alone kernel and no multiple of it;
# 7 x 19 x 19 = 2,527 tiles: the same for the 2,048-tile round of the means in
# the quantizer launch's 256-thread budget workgroup
SEGMENTS = [
    [(1, 1, 1)],
    [(2, 1, 7)],
    [(2, 7, 1)],
    [(2, 5, 5), (2, 3, 5)],
    [(3, 19, 19)],
    [(3, 19, 19), (2, 5, 5), (1, 1, 1)],
    [(2, 3, 5), (1, 1, 7), (3, 19, 19)],
    [(7, 19, 19), (2, 3, 5)],
]


def _n_edges(B, ht, wt):
    return B * ((ht - 1) * wt + ht * (wt - 1))


@pytest.mark.parametrize("segs", SEGMENTS, ids=lambda s: "+".join("%dx%dx%d" % d for d in s))
def test_forward_value_through_the_c_abi(segs):
    """L_smooth of both forward entries (the stand-alone workgroup and the
    extra workgroup of the quantizer's forward launch) against the torch
    expression on the CPU in fp64, within n 2^-24 relative, n the number of
    addends (edges) of the largest segment: every addend |b' - b| carries one
    fp32 rounding and a sum of n non-negative fp32 addends in any order at
    most n - 1 more, relative to the sum; the kernels' strided sums and
    trees are far shallower than n.  avg and the budget loss of the same call
    equal those of the entries without the term, bit for bit."""
    from mcaq_yolo_amd import abi, core
    L = abi.lib()
    st = core._stream()
    g = torch.Generator().manual_seed(11)
    maps = [(2.0 + 6.0 * torch.rand(*d, generator=g)) for d in segs]
    dmaps = [m.to(DEV) for m in maps]
    ref = float(_expr(maps))
    n = len(segs)
    bound = max(_n_edges(*d) for d in segs) * 2.0 ** -24 * ref
    bp = (abi.P * n)(*[core._p(m) for m in dmaps])
    dims = (abi.I * (3 * n))(*[v for d in segs for v in d])
    cnt = (abi.I * n)(*[m.numel() for m in maps])
    out = torch.full((3, 3), float("nan"), device=DEV)      # rows: avg, loss, smooth; columns: old, alone, ride
    tl = abi.TileLosses(None, None, None, 4.5, n, core._p(out[2, 1:]), None)
    abi.check(L.mcaq_bit_budget_forward(bp, cnt, n, 4.5, core._p(out[0, 0:]), core._p(out[1, 0:]), st), "old")
    abi.check(L.mcaq_tile_losses_forward(bp, dims, n, core._p(out[0, 1:]), core._p(out[1, 1:]), ctypes.byref(tl), st),
              "mcaq_tile_losses_forward")
    # the quantizer launch: one tiny scale of its own, the synthetic maps as the loss segments
    x = torch.rand(1, 8, 16, 16, generator=g).to(DEV)
    qb = torch.full((1, 4, 4), 4.5, device=DEV)
    xmin, xmax = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    ys = torch.empty(2, *x.shape, device=DEV)
    res = torch.full((2, 2), float("nan"), device=DEV)      # old ride: avg, loss
    q = core._qat_struct(x, qb, None, xmin, xmax)
    q.y = core._p(ys[0])
    abi.check(L.mcaq_qat_forward_budget(ctypes.byref(q), 1, bp, cnt, n, 4.5, core._p(res[0, 0:]), core._p(res[0, 1:]),
                                        st), "old ride")
    q.y = core._p(ys[1])
    tl2 = abi.TileLosses(None, None, None, 4.5, n, core._p(out[2, 2:]), None)
    abi.check(L.mcaq_qat_forward_tile_losses(ctypes.byref(q), 1, bp, dims, n, core._p(out[0, 2:]), core._p(out[1, 2:]),
                                             ctypes.byref(tl2), st), "mcaq_qat_forward_tile_losses")
    torch.cuda.synchronize()
    out, res = out.cpu(), res.cpu()
    for col, what in ((1, "alone"), (2, "ride")):
        err = abs(float(out[2, col]) - ref)
        print("%s: L_smooth %.9g ref %.9g err %.3g bound %.3g" % (what, float(out[2, col]), ref, err, bound))
        assert err <= bound, what
    assert torch.equal(out[:2, 1], out[:2, 0])              # avg, loss: the stand-alone entries
    assert torch.equal(out[:2, 2], res[0])                  # ... and the riding ones
    assert torch.equal(ys[0], ys[1])
    # smooth = NULL: nothing but avg and loss is written
    chk = torch.full((3,), float("nan"), device=DEV)
    tl3 = abi.TileLosses(None, None, None, 4.5, n, None, None)
    abi.check(L.mcaq_tile_losses_forward(bp, dims, n, core._p(chk[0:]), core._p(chk[1:]), ctypes.byref(tl3), st), "null")
    torch.cuda.synchronize()
    assert torch.equal(chk[:2].cpu(), out[:2, 0]) and bool(torch.isnan(chk[2]))


# ---------------------------------------------------------------------------
# 2. the gradient alone, through the hooks
# ---------------------------------------------------------------------------
def test_isolated_gradient_through_the_hooks():
    """backward of smoothness_loss(aux) alone over 10x10, 5x5 and 3x5 tile
    grids (B = 2; the analyzer takes the non-square 12 x 20 map): every bit
    map's gradient equals autograd's of the expression on a CPU copy (rtol
    1e-5, the bar of tests/test_qat_gpu.py for the step's gradients), is
    exactly 0 wherever kappa = 0, and the feature maps' gradients are
    exactly 0 (zero upstream for the quantizer: its fold adds nothing)."""
    from mcaq_yolo_amd import hooks, train_step
    from mcaq_yolo_amd.hooks import MCAQHooks
    assert train_step.FUSED_SMOOTHNESS and train_step.FUSED_MASK_QAT and hooks.MULTI_SCALE_TRAIN
    h = _hooks()
    gen = torch.Generator().manual_seed(4)
    feats = [torch.nn.functional.silu(2.0 * torch.randn(2, c, H, W, generator=gen)).to(DEV).requires_grad_(True)
             for c, H, W in ((16, 40, 40), (32, 20, 20), (32, 12, 20))]
    outs, aux = h.forward_features(feats, temperature=1.0)
    assert [tuple(a["bit_map"].shape) for a in aux] == [(2, 10, 10), (2, 5, 5), (2, 3, 5)]
    for a in aux:
        a["bit_map"].retain_grad()
    loss = MCAQHooks.smoothness_loss(aux)
    assert loss is aux[0]["_bit_budget"]["loss_smooth"]         # the fused scalar, not torch ops
    loss.backward()
    torch.cuda.synchronize()
    cpu = [a["bit_map"].detach().cpu().requires_grad_(True) for a in aux]
    ref = _expr(cpu, torch.float32)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * float(ref.detach())
    for a, c in zip(aux, cpu):
        got = a["bit_map"].grad.cpu()
        b = c.detach()
        kap = torch.zeros_like(b)
        kap[:, 1:, :] += torch.sign(b[:, 1:, :] - b[:, :-1, :])
        kap[:, :-1, :] += torch.sign(b[:, :-1, :] - b[:, 1:, :])
        kap[:, :, 1:] += torch.sign(b[:, :, 1:] - b[:, :, :-1])
        kap[:, :, :-1] += torch.sign(b[:, :, :-1] - b[:, :, 1:])
        print("grid %s: max |grad| %.3g, kappa == 0 at %d tiles, max err %.3g" %
              (tuple(b.shape), float(got.abs().max()), int((kap == 0).sum()), float((got - c.grad).abs().max())))
        assert torch.allclose(got, c.grad, rtol=1e-5, atol=0.0)
        assert not got[kap == 0].any()
        assert bool((got[kap != 0] != 0).all())
    for f in feats:
        assert f.grad is not None and not f.grad.any()


# ---------------------------------------------------------------------------
# 3 - 5. the whole step
# ---------------------------------------------------------------------------
def _run(fused_smooth, steps=1, graph=False, smooth=True, spy=None):
    """test_concurrent_scales_gpu._run's multi-scale fused step (multi=True,
    fused_mq=True, budget=True) with loss = sum(y g) + 0.1 bit_budget_loss
    (+ 0.1 smoothness_loss if smooth), under train_step.FUSED_SMOOTHNESS =
    fused_smooth.  spy: called with the library before the steps; returns the
    function that undoes it."""
    from mcaq_yolo_amd import abi, hooks, train_step
    old = hooks.CONCURRENT_TRAIN_SCALES, hooks.MULTI_SCALE_TRAIN, train_step.FUSED_MASK_QAT, \
        train_step.FUSED_SMOOTHNESS
    hooks.CONCURRENT_TRAIN_SCALES, hooks.MULTI_SCALE_TRAIN = False, True
    train_step.FUSED_MASK_QAT, train_step.FUSED_SMOOTHNESS = True, fused_smooth
    undo = None
    try:
        h = _hooks("mlp")
        feats, gens = _feats()
        params = [p for p in h.parameters() if p.requires_grad]
        opt = torch.optim.SGD(params, lr=1e-2, momentum=0.9)
        rec = {}
        if spy is not None:
            undo = spy(abi.lib())

        def step():
            opt.zero_grad(set_to_none=True)
            for f in feats:
                f.grad = None
            outs, aux = h.forward_features(feats, temperature=1.0)
            loss = sum((o * g).sum() for o, g in zip(outs, gens)) + 0.1 * h.bit_budget_loss(aux, 4.0)
            if smooth:
                ls = h.smoothness_loss(aux)
                assert (ls is aux[0]["_bit_budget"]["loss_smooth"]) == fused_smooth
                loss = loss + 0.1 * ls
                rec["loss_smooth"] = [ls.detach()]
            loss.backward()
            rec["outs"] = [o.detach() for o in outs]
            rec["bits"] = [a["bit_map"].detach() for a in aux]
            rec["cplx"] = [a["complexity"].detach() for a in aux]
            opt.step()
            h.bit_mapper.enforce_weight_constraints()

        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()                         # warm-up: lazy buffers, grad sinks
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            opt.zero_grad(set_to_none=True)
            with torch.cuda.graph(g):
                step()
            for _ in range(steps):
                g.replay()
        else:
            for _ in range(steps):
                step()
        torch.cuda.synchronize()
        snap = {k: [t.clone() for t in v] for k, v in rec.items()}
        snap["fgrad"] = [f.grad.detach().clone() for f in feats]
        snap["grads"] = {k: p.grad.detach().clone() for k, p in h.named_parameters() if p.grad is not None}
        snap["params"] = {k: p.detach().clone() for k, p in h.named_parameters()}
        snap["bufs"] = {k: b.detach().clone() for k, b in h.named_buffers() if b is not None}
        return snap
    finally:
        if undo is not None:
            undo()
        hooks.CONCURRENT_TRAIN_SCALES, hooks.MULTI_SCALE_TRAIN, train_step.FUSED_MASK_QAT, \
            train_step.FUSED_SMOOTHNESS = old


def test_fused_step_close_to_torch_ops():
    """One full step with the smoothness term fused against the same step
    with the term as torch ops on the step's bit maps (FUSED_SMOOTHNESS off):
    the forward is bit-identical; the bit-map gradient sums its contributions
    in another association, so gradients agree within _close's bar.  (One
    step only, for the reason test_fused_mask_quant_budget_step_close_to_
    per_scale gives: SGD steps on rounding-noise gradients move the runs
    apart along directions the loss does not see.)"""
    a = _run(True)
    b = _run(False)
    for k in ("outs", "bits", "cplx"):
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k
    la, lb = float(a["loss_smooth"][0]), float(b["loss_smooth"][0])
    print("loss_smooth fused %.9g torch ops %.9g" % (la, lb))
    assert abs(la - lb) <= 1e-5 * abs(lb)
    _close(a, b)


NEW_FWD, NEW_BWD = "mcaq_qat_forward_tile_losses", "mcaq_qat_smask_backward_tile_losses"
OLD_FWD, OLD_BWD = "mcaq_qat_forward_budget", "mcaq_qat_smask_backward_multi"


def _spy(calls, null_smooth=False):
    """Record every native entry's name (and the tile-loss struct's pointers);
    null_smooth: the forward entry gets smooth = NULL."""
    from mcaq_yolo_amd import abi

    def install(L):
        orig = {n: getattr(L, n) for n in abi.EXPORTS}

        def wrap(n):
            def f(*a):
                info = None
                if n in (NEW_FWD, NEW_BWD):
                    tl = a[-2]._obj
                    if null_smooth and n == NEW_FWD:
                        tl.smooth = None
                    info = (tl.smooth is not None, tl.g_smooth is not None)
                calls.append((n, info))
                return orig[n](*a)
            return f
        for n in abi.EXPORTS:
            setattr(L, n, wrap(n))

        def undo():
            for n, f in orig.items():
                setattr(L, n, f)
        return undo
    return install


def test_unused_term_changes_nothing():
    """The native call sequence of forward + backward has the same length with
    and without smoothness_loss in the loss; without it the backward entry
    receives g_smooth = NULL.  The step without the term through the old
    entries (FUSED_SMOOTHNESS off: mcaq_qat_forward_budget,
    mcaq_qat_smask_backward_multi) and through the new entries with null
    smoothness pointers leaves every gradient bit-identical."""
    c_with, c_without, c_old, c_null = [], [], [], []
    _run(True, smooth=True, spy=_spy(c_with))
    a = _run(True, smooth=False, spy=_spy(c_without))
    b = _run(False, smooth=False, spy=_spy(c_old))
    c = _run(True, smooth=False, spy=_spy(c_null, null_smooth=True))
    names = lambda cs: [n for n, _ in cs]
    assert len(c_with) == len(c_without) == len(c_old) and names(c_with) == names(c_without)
    assert dict(c_with)[NEW_FWD] == (True, False) and dict(c_with)[NEW_BWD] == (False, True)
    assert dict(c_without)[NEW_FWD] == (True, False) and dict(c_without)[NEW_BWD] == (False, False)
    assert dict(c_null)[NEW_FWD] == (False, False) and dict(c_null)[NEW_BWD] == (False, False)
    swap = {NEW_FWD: OLD_FWD, NEW_BWD: OLD_BWD}
    assert [swap.get(n, n) for n in names(c_without)] == names(c_old)
    assert names(c_with).count(NEW_FWD) == 1 and names(c_with).count(NEW_BWD) == 1
    _same(a, b)
    _same(c, b)


def test_fused_smoothness_graph():
    """The step of test_fused_step_close_to_torch_ops captured in a HIP graph
    (warm-up step + 3 replays) == 4 eager steps, bit for bit, loss_smooth
    included: the forward reduction has a fixed order."""
    a = _run(True, steps=3, graph=True)
    b = _run(True, steps=4)
    assert torch.equal(a["loss_smooth"][0], b["loss_smooth"][0])
    _same(a, b)
