"""The optimizer kernels of csrc/mcaq_optim.h at their C ABI entries against
the float64 references of tests/optim_cases.py, by its per-element rule

    |got - ref| <= 8 * eps32 * A + tiny

(A: the sum of the magnitudes of the reference expression's terms; NaN
positions equal; +-inf and zero by ==; gradients bit-equal where the
reference's coefficient is exactly 1).  Step counters, refusal codes and the
exchange status word are compared exactly.  Device buffers, the mcaq_adamw_seg
array and the group table are built here: every tensor kind is one flat buffer
with 3 sentinel floats before, between and after the segments (so no segment
starts on a 16-byte boundary and a write outside a segment shows), the step
array has a spare entry around every used one, and total_norm starts as a
sentinel.  Every case runs through mcaq_clip_adamw; every clipping case of at
most 256 chunks also through mcaq_clip_adamw_fused, bit-identical.

MCAQ_OPTIM_VALUES_OUT=<file>: the largest err / (eps32 A) of every (case,
tensor kind) is written there as JSON (profiles/optim_values.json is one
such run)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import optim_cases as oc
from mcaq_yolo_amd import abi
from test_optim_cases_cpu import clip_adamw_from_case, collect

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID = 1                     # hipErrorInvalidValue: an entry's refusal
GUARD, SENT = 3, -7.0           # sentinel floats around every segment
NORM_SENT = 123.5               # total_norm before the launch
RATIOS = {}
ONE_LAUNCH = [n for n in oc.NAMES if oc.CFGS[n][2].get("max_norm", 0.5) > 0 and
              -(-sum(oc.CFGS[n][1]) // oc.CH) <= oc.FUSED_MAX_CHUNKS]
REFUSED = [n for n in oc.NAMES if n not in ONE_LAUNCH]


@pytest.fixture(scope="module", autouse=True)
def _ratio_file():
    yield
    out = os.environ.get("MCAQ_OPTIM_VALUES_OUT")
    if out and RATIOS:
        worst = max((r, c, k) for c, d in RATIOS.items() for k, r in d.items())
        with open(out, "w") as f:
            json.dump({"rule": "per element |got-ref| <= M eps32 A + tiny, M = 8; ratios are max err / (eps32 A) "
                               "through mcaq_clip_adamw (mcaq_clip_adamw_fused is bit-identical)",
                       "largest": {"ratio": worst[0], "case": worst[1], "tensor": worst[2]}, "ratios": RATIOS},
                      f, indent=1, sort_keys=True)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same_bits(a, b):
    """Bit-identical, NaNs equal to NaNs."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


class Launch:
    """The device side of one case: buffers, descriptors, and what a launch left in them."""

    def __init__(self, c):
        self.c = c
        nseg = len(c.sizes)
        self.off = [int(c.starts[k]) + (k + 1) * GUARD for k in range(nseg)]
        self.host, self.dev = {}, {}
        for kind, src in zip(oc.KINDS, (c.G, c.M, c.V, c.P)):
            h = np.full(int(c.starts[-1]) + (nseg + 1) * GUARD, SENT, dtype=np.float32)
            for k in range(nseg):
                h[self.off[k]:self.off[k] + c.sizes[k]] = c.seg(src, k)
            self.host[kind], self.dev[kind] = h, torch.from_numpy(h.copy()).to(DEV)
        self.step_idx = [2 * (nseg - 1 - k) + 1 for k in range(nseg)]       # not in segment order; spares between
        hs = np.full(2 * nseg + 1, SENT, dtype=np.float32)
        hs[self.step_idx] = c.seg_step
        self.host["steps"], self.dev["steps"] = hs, torch.from_numpy(hs.copy()).to(DEV)
        self.dev["total_norm"] = torch.full((1,), NORM_SENT, device=DEV)
        self.groups = torch.tensor([v for g in c.groups for v in g], dtype=torch.float64, device=DEV)
        self.segs = (abi.AdamwSeg * nseg)()
        for k, s in enumerate(self.segs):
            for kind in oc.KINDS:          # the struct's fields carry the same names
                assert 0 < self.off[k] and self.off[k] + c.sizes[k] + GUARD <= self.dev[kind].numel()
                setattr(s, kind, self.dev[kind].data_ptr() + 4 * self.off[k])
            assert 0 <= self.step_idx[k] < hs.size
            s.n, s.project_abs, s.group, s.step_idx = c.sizes[k], c.seg_abs[k], c.seg_group[k], self.step_idx[k]
        self.status = None

    def two(self):
        L, c = abi.lib(), self.c
        self.work = torch.empty(L.mcaq_clip_adamw_work_floats(int(c.starts[-1])), device=DEV)
        err = L.mcaq_clip_adamw(self.segs, len(c.sizes), _p(self.groups), len(c.groups), _p(self.dev["steps"]),
                                c.max_norm, _p(self.dev["total_norm"]), _p(self.work), _stream())
        torch.cuda.synchronize()
        return err

    def fused(self):
        L, c = abi.lib(), self.c
        total, nseg = int(c.starts[-1]), len(c.sizes)
        nb = L.mcaq_clip_adamw_sync_bytes(total, nseg)
        assert nb == 256 + (-(-total // oc.CH)) * nseg * 8
        self.sync = torch.zeros((nb + 7) // 8, dtype=torch.int64, device=DEV)
        err = L.mcaq_clip_adamw_fused(self.segs, nseg, _p(self.groups), len(c.groups), _p(self.dev["steps"]),
                                      c.max_norm, _p(self.dev["total_norm"]), _p(self.sync), self.sync.numel() * 8,
                                      _stream())
        torch.cuda.synchronize()
        self.status = int(self.sync.view(torch.int32)[abi.ADAMW_SYNC_STATUS_WORD].item())
        return err

    def read(self):
        """What the launch left: the segments in case order, the step array, total_norm; asserts the guards."""
        c = self.c
        got = {}
        for kind in oc.KINDS:
            d = self.dev[kind].cpu().numpy()
            mask = np.ones(d.size, dtype=bool)
            for k in range(len(c.sizes)):
                mask[self.off[k]:self.off[k] + c.sizes[k]] = False
            assert bool((d[mask] == SENT).all()), "%s: a write outside the segments" % kind
            got[kind] = d[~mask]
        s = self.dev["steps"].cpu().numpy()
        got["all_steps"] = s
        got["steps"] = s[self.step_idx]
        got["total_norm"] = self.dev["total_norm"].cpu().numpy()[0]
        return got

    def untouched(self):
        return all(_same_bits(self.dev[k].cpu().numpy(), self.host[k]) for k in oc.KINDS + ("steps",)) and \
            float(self.dev["total_norm"][0]) == NORM_SENT


@functools.lru_cache(maxsize=None)
def two_launch(name):
    """The case through mcaq_clip_adamw: run once, shared, read only."""
    run = Launch(oc.case(name))
    err = run.two()
    return err, run.read()


def _check(c, got, record=None):
    miss, ratio = c.check(got)
    print("%-16s %s" % (c.name, {k: "%.3g" % v for k, v in ratio.items()}))
    if record is not None:
        RATIOS[record] = ratio
    assert not miss, (miss, ratio)
    spare = np.ones(got["all_steps"].size, dtype=bool)
    spare[[2 * k + 1 for k in range(len(c.sizes))]] = False
    assert bool((got["all_steps"][spare] == SENT).all()), "a step counter outside the launch moved"
    if not c.clip:
        assert float(got["total_norm"]) == NORM_SENT      # no clip: total_norm is left as it was


@pytest.mark.parametrize("name", oc.NAMES)
def test_two_launch_values(name):
    c = oc.case(name)
    err, got = two_launch(name)
    assert err == 0
    _check(c, got, record=name)


@pytest.mark.parametrize("name", ONE_LAUNCH)
def test_one_launch_values_equal_two_launches(name):
    c = oc.case(name)
    run = Launch(c)
    assert run.fused() == 0
    assert run.status == 0
    got = run.read()
    _check(c, got)
    err, ref = two_launch(name)
    assert err == 0
    for k in oc.KINDS + ("all_steps", "total_norm"):
        assert _same_bits(got[k], ref[k]), k


@pytest.mark.parametrize("name", REFUSED)
def test_one_launch_entry_refuses(name):
    """More than 256 chunks, or max_norm <= 0: hipErrorInvalidValue before any launch, nothing written."""
    assert name in ("chunks_257", "no_clip_0", "no_clip_neg", "nan_no_clip")
    run = Launch(oc.case(name))
    assert run.fused() == INVALID
    assert run.status == 0 and not bool(run.sync.any())
    assert run.untouched()


def test_sq_overflow_is_what_torch_clip_grad_norm_does_on_the_device():
    """|g| = 1e20: torch's fp32 clip_grad_norm_ on the same device gradients
    also gives an inf total and +-0 gradients."""
    c = oc.case("sq_overflow")
    err, got = two_launch("sq_overflow")
    assert err == 0
    ps = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in c.sizes]
    for k, p in enumerate(ps):
        p.grad = torch.from_numpy(c.seg(c.G, k).copy()).to(DEV)
    tn = torch.nn.utils.clip_grad_norm_(ps, c.max_norm)
    tg = np.concatenate([p.grad.cpu().numpy() for p in ps])
    assert float(tn) == float("inf") == float(got["total_norm"])
    assert not tg.any() and not got["grad"].any()
    assert np.array_equal(np.signbit(tg), np.signbit(got["grad"]))


# ---- through optim.ClipAdamW -------------------------------------------------
def test_clip_adamw_groups_4_from_param_group_dicts():
    """groups_4 as four param-group dicts (the segments in group order, the
    state through load_state_dict): the table's reference by the rule."""
    c = oc.case("groups_4")
    o, ps, order = clip_adamw_from_case(c, torch.device(DEV))
    o.step()
    torch.cuda.synchronize()
    assert o._sync is not None and int(o._sync.view(torch.int32)[abi.ADAMW_SYNC_STATUS_WORD].item()) == 0
    miss, ratio = c.check(collect(c, o, ps, order))
    print(ratio)
    assert not miss, (miss, ratio)


def test_clip_adamw_257_chunks_takes_the_two_launches():
    c = oc.case("chunks_257")
    o, ps, order = clip_adamw_from_case(c, torch.device(DEV))
    o.step()
    torch.cuda.synchronize()
    assert o._sync is None
    miss, ratio = c.check(collect(c, o, ps, order))
    assert not miss, (miss, ratio)


def test_clip_adamw_fifth_group_is_refused():
    from mcaq_yolo_amd.optim import ClipAdamW
    ps = [torch.nn.Parameter(torch.randn(8, device=DEV)) for _ in range(5)]
    o = ClipAdamW([dict(params=[p], lr=1e-3 * (k + 1)) for k, p in enumerate(ps)], max_norm=1.0)
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(ValueError, match="parameter groups"):
        o.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, p) for a, p in zip(before, ps))


def test_clip_adamw_add_param_group_after_a_step_matches_torch():
    """Two steps, a group with its own lr added, two more (clipping on, so the
    one-launch form and its exchange buffer are rebuilt for the new layout):
    the new parameter starts from zero moments at step 0, the old ones keep
    theirs - torch's clip_grad_norm_ + fused AdamW doing the same.  Per step
    the clipped gradients of both sides are within ~4 eps32, so the update
    within 5e-7 lr and the parameter within eps32 / 2 |p| + 5e-9: four steps
    stay inside rtol 1e-6, atol 1e-7."""
    from mcaq_yolo_amd.optim import ClipAdamW
    torch.manual_seed(13)
    ps = [torch.randn(n, device=DEV, requires_grad=True) for n in (97, 2048, 5, 700)]
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    o0 = torch.optim.AdamW(ps[:3], lr=1e-2, weight_decay=0.05, fused=True)
    o1 = ClipAdamW(qs[:3], lr=1e-2, weight_decay=0.05, max_norm=0.5, project_abs=[qs[1]])
    for it in range(4):
        if it == 2:
            o0.add_param_group(dict(params=[ps[3]], lr=3e-3))
            o1.add_param_group(dict(params=[qs[3]], lr=3e-3))
        live = 3 if it < 2 else 4
        for p, q in zip(ps[:live], qs[:live]):
            g = torch.randn_like(p)
            p.grad, q.grad = g.clone(), g.clone()
        torch.nn.utils.clip_grad_norm_(ps[:live], 0.5)
        o0.step()
        with torch.no_grad():
            ps[1].abs_()
        o1.step()
    torch.cuda.synchronize()
    assert int(o1._sync.view(torch.int32)[abi.ADAMW_SYNC_STATUS_WORD].item()) == 0
    for p, q in zip(ps, qs):
        assert torch.allclose(q, p, rtol=1e-6, atol=1e-7)
        assert torch.allclose(o1.state[q]["exp_avg"], o0.state[p]["exp_avg"], rtol=1e-5, atol=1e-9)
    assert [float(o1.state[q]["step"]) for q in qs] == [4.0, 4.0, 4.0, 2.0]


def test_clip_adamw_leaves_an_empty_parameter_out():
    """A CUDA parameter with numel() == 0 and a gradient is no segment of the
    launch (the entry refuses n < 1): the step equals the one without it, bit
    for bit."""
    from mcaq_yolo_amd.optim import ClipAdamW
    torch.manual_seed(14)
    ps = [torch.randn(n, device=DEV, requires_grad=True) for n in (97, 2048)]
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    e = torch.zeros(0, 4, device=DEV, requires_grad=True)
    o0 = ClipAdamW(ps, lr=1e-2, weight_decay=0.05, max_norm=0.5)
    o1 = ClipAdamW([qs[0], e, qs[1]], lr=1e-2, weight_decay=0.05, max_norm=0.5)
    for it in range(2):
        for p, q in zip(ps, qs):
            g = torch.randn_like(p)
            p.grad, q.grad = g.clone(), g.clone()
        e.grad = torch.zeros_like(e)
        o0.step()
        o1.step()
    torch.cuda.synchronize()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q) and torch.equal(o0.state[p]["exp_avg_sq"], o1.state[q]["exp_avg_sq"])
    assert torch.equal(o0.last_total_norm, o1.last_total_norm)
    assert [float(o1.state[q]["step"]) for q in qs] == [2.0, 2.0]
