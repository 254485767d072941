"""The single-scale train entries of the C ABI against their one-segment
multi-segment twins (csrc/mcaq_train.h), called directly on the same seeded
inputs and the golden parameters: every output bit-identical - the bit map, the
whole work buffer (activations, statistics, the deferred running-statistics
region), gradients, per-workgroup partials, reduced parameter gradients and the
BatchNorm running statistics.  A single-scale entry is a multi launch with
nseg = 1; this pins that."""
import copy
import ctypes

import pytest
import torch

from mcaq_yolo_amd import abi, core
from mcaq_yolo_amd.core import _p, _stream
from test_train_fused_gpu import DEV, _hooks

pytestmark = pytest.mark.gpu

MG_SIZE, CG_SIZE, SG_SIZE = 4609, 2881, 170      # parameter-gradient floats: mapper, complexity MLP, soft mask
MIN_B, MAX_B, TEMP, MOM = 2.0, 8.0, 1.0, 0.1
MAPPER_N = [1, 63, 64, 65, 130]      # one partial workgroup, the 64-tile boundary on both sides, 3 workgroups + tail


@pytest.fixture(scope="module")
def hooks():
    return _hooks()


def _rand(seed, *shape, normal=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randn(*shape, generator=g) if normal else torch.rand(*shape, generator=g)
    return t.to(DEV)


def _ok(err, what):
    abi.check(err, what)


def _reduce1(L, part, out, nparts, count, acc):
    seg = (abi.ReduceSeg * 1)()
    seg[0].part, seg[0].out = _p(part), _p(out)
    seg[0].nparts, seg[0].stride, seg[0].count, seg[0].accumulate, seg[0].scale = nparts, count, count, acc, 0.0
    _ok(L.mcaq_train_reduce_multi(seg, 1, 0, _stream()), "mcaq_train_reduce_multi")


def _mapper_pair(hooks):
    """Two private copies of the golden mapping network (running statistics
    are outputs) with their parameter structs."""
    nets = [copy.deepcopy(hooks.bit_mapper.mapping_network).train() for _ in range(2)]
    return nets, [core._mapper_params(n) for n in nets]


def _mseg(c, bits, work, gbits=None, gc=None, gpart=None):
    seg = (abi.MapperSeg * 1)()
    seg[0].c, seg[0].bits, seg[0].work, seg[0].n = _p(c), _p(bits), _p(work), c.numel()
    seg[0].gbits, seg[0].gc, seg[0].gpart = _p(gbits), _p(gc), _p(gpart)
    return seg


def _same_running(nets):
    for i in (1, 4, 7):
        a, b = nets[0][i], nets[1][i]
        assert torch.equal(a.running_mean, b.running_mean), "running_mean %d" % i
        assert torch.equal(a.running_var, b.running_var), "running_var %d" % i
        assert torch.equal(a.num_batches_tracked, b.num_batches_tracked)


@pytest.mark.parametrize("update_stats", [1, 2])
@pytest.mark.parametrize("n", MAPPER_N)
def test_mapper_train_forward_backward_equal_one_segment(hooks, n, update_stats):
    L = abi.lib()
    nets, qs = _mapper_pair(hooks)
    c = _rand(10 + n, n) * 1.2 - 0.1                 # some tiles outside the [0, 1] clamp
    gbits = _rand(20 + n, n, normal=True)
    nw = L.mcaq_mapper_work_floats(n)
    work = [torch.zeros(nw, device=DEV) for _ in range(2)]
    bits = [torch.zeros(n, device=DEV) for _ in range(2)]
    _ok(L.mcaq_mapper_train_forward(ctypes.byref(qs[0]), _p(c), n, MIN_B, MAX_B, TEMP, MOM, 1, update_stats,
                                    _p(bits[0]), _p(work[0]), _stream()), "mcaq_mapper_train_forward")
    _ok(L.mcaq_mapper_train_forward_multi(ctypes.byref(qs[1]), _mseg(c, bits[1], work[1]), 1, MIN_B, MAX_B, TEMP, MOM,
                                          1, update_stats, _stream()), "mcaq_mapper_train_forward_multi")
    assert torch.equal(bits[0], bits[1])
    assert torch.equal(work[0], work[1])             # with the rstat region (update_stats 2)
    assert bool((bits[0] >= MIN_B).all()) and bool((bits[0] <= MAX_B).all())
    _same_running(nets)
    if update_stats == 1:
        assert int(nets[0][1].num_batches_tracked) == int(hooks.bit_mapper.mapping_network[1].num_batches_tracked) + 1
    ng = L.mcaq_mapper_gpart_floats(n)
    for acc in (0, 1):
        gc = [torch.zeros(n, device=DEV) for _ in range(2)]
        gpart = [torch.zeros(ng, device=DEV) for _ in range(2)]
        gpar = [_rand(30 + n, MG_SIZE, normal=True) for _ in range(2)]
        _ok(L.mcaq_mapper_train_backward(ctypes.byref(qs[0]), _p(c), n, _p(gbits), MIN_B, MAX_B, TEMP, _p(work[0]),
                                         _p(gc[0]), _p(gpar[0]), _p(gpart[0]), acc, _stream()),
            "mcaq_mapper_train_backward")
        _ok(L.mcaq_mapper_train_backward_multi(ctypes.byref(qs[1]), _mseg(c, bits[1], work[1], gbits, gc[1], gpart[1]),
                                               1, MIN_B, MAX_B, TEMP, _stream()), "mcaq_mapper_train_backward_multi")
        _reduce1(L, gpart[1], gpar[1], ng // MG_SIZE, MG_SIZE, acc)
        assert torch.equal(gc[0], gc[1])
        assert torch.equal(gpart[0], gpart[1])
        assert torch.equal(gpar[0], gpar[1])
        assert torch.equal(work[0], work[1])
        assert bool(gpar[0].isfinite().all()) and bool(gc[0].isfinite().all())


@pytest.mark.parametrize("n", MAPPER_N)
def test_mapper_train_stage_entries_equal_one_segment(hooks, n):
    """The sharded-batch stage entries, as two ranks holding the same tiles:
    every rank's (mean, M2, n) entry and the all-reduced BN sums are this
    process's own, twice."""
    L = abi.lib()
    world = 2
    nets, qs = _mapper_pair(hooks)
    c = _rand(40 + n, n) * 1.2 - 0.1
    gbits = _rand(50 + n, n, normal=True)
    nw, ng = L.mcaq_mapper_work_floats(n), L.mcaq_mapper_gpart_floats(n)
    work = [torch.zeros(nw, device=DEV) for _ in range(2)]
    bits = [torch.zeros(n, device=DEV) for _ in range(2)]
    PP = ctypes.c_void_p * 1

    def share(k, kind, layer, count):
        out = torch.zeros(count, device=DEV)
        _ok(L.mcaq_mapper_train_reduce(_p(work[k]), n, kind, layer, _p(out), _stream()), "mcaq_mapper_train_reduce")
        return out

    gath = [[None] * 4 for _ in range(2)]
    for st in (1, 2, 3, 4):
        _ok(L.mcaq_mapper_train_forward_stage(ctypes.byref(qs[0]), _p(c), n, MIN_B, MAX_B, TEMP, MOM, 1, 1, _p(bits[0]),
                                              _p(work[0]), st, _p(gath[0][st - 1]), world, _stream()),
            "mcaq_mapper_train_forward_stage")
        g1 = gath[1][st - 1]
        _ok(L.mcaq_mapper_train_forward_stage_multi(ctypes.byref(qs[1]), _mseg(c, bits[1], work[1]), 1, MIN_B, MAX_B,
                                                    TEMP, MOM, 1, 1, st, PP(g1.data_ptr()) if g1 is not None else None,
                                                    world, _stream()), "mcaq_mapper_train_forward_stage_multi")
        if st <= 3:
            for k in range(2):
                gath[k][st] = share(k, 0, st, 129).repeat(world)
    assert torch.equal(bits[0], bits[1])
    assert torch.equal(work[0], work[1])
    _same_running(nets)
    gc = [torch.zeros(n, device=DEV) for _ in range(2)]
    gpart = [torch.zeros(ng, device=DEV) for _ in range(2)]
    gs = [[None] * 5 for _ in range(2)]
    for st in (4, 3, 2, 1):
        _ok(L.mcaq_mapper_train_backward_stage(ctypes.byref(qs[0]), _p(c), n, _p(gbits), MIN_B, MAX_B, TEMP, _p(work[0]),
                                               _p(gc[0]), _p(gpart[0]), st, _p(gs[0][st]), _p(gath[0][1]), world,
                                               _stream()), "mcaq_mapper_train_backward_stage")
        s1 = gs[1][st]
        _ok(L.mcaq_mapper_train_backward_stage_multi(
            ctypes.byref(qs[1]), _mseg(c, bits[1], work[1], gbits, gc[1], gpart[1]), 1, MIN_B, MAX_B, TEMP, st,
            PP(s1.data_ptr()) if s1 is not None else PP(None), PP(gath[1][1].data_ptr()), world, _stream()),
            "mcaq_mapper_train_backward_stage_multi")
        if st >= 2:
            for k in range(2):
                gs[k][st - 1] = share(k, 1, st - 1, 128) * float(world)
    assert torch.equal(gc[0], gc[1])
    assert torch.equal(gpart[0], gpart[1])
    assert torch.equal(work[0], work[1])
    assert bool(gc[0].isfinite().all()) and bool(gpart[0].isfinite().all())


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("B,ht,wt", [(1, 1, 1), (2, 5, 7), (3, 8, 8)])      # (3, 8, 8): exactly 3 workgroups
def test_head_train_backward_equals_one_segment(hooks, B, ht, wt, acc):
    L = abi.lib()
    n = B * ht * wt
    params = list(hooks.complexity_analyzer.complexity_mlp.parameters())
    q = core._ptr_struct(abi.CmlpParams, params)
    phi = _rand(60 + n, n, 8)
    craw = _rand(61 + n, B, ht, wt) * 1.4 - 0.2      # some bilateral outputs outside the [0, 1] clamp
    gC = _rand(62 + n, B, ht, wt, normal=True)
    ng = L.mcaq_head_gpart_floats(n)
    gcraw = [torch.zeros(n, device=DEV) for _ in range(2)]
    gpart = [torch.zeros(ng, device=DEV) for _ in range(2)]
    gpar = [_rand(63 + n, CG_SIZE, normal=True) for _ in range(2)]
    _ok(L.mcaq_head_train_backward(ctypes.byref(q), _p(phi), _p(craw), _p(gC), B, ht, wt, _p(gcraw[0]), _p(gpar[0]),
                                   _p(gpart[0]), acc, _stream()), "mcaq_head_train_backward")
    seg = (abi.HeadSeg * 1)()
    seg[0].phi, seg[0].craw, seg[0].gC, seg[0].gcraw, seg[0].gpart = _p(phi), _p(craw), _p(gC), _p(gcraw[1]), _p(gpart[1])
    seg[0].B, seg[0].ht, seg[0].wt = B, ht, wt
    _ok(L.mcaq_head_train_backward_multi(ctypes.byref(q), seg, 1, _stream()), "mcaq_head_train_backward_multi")
    _reduce1(L, gpart[1], gpar[1], ng // CG_SIZE, CG_SIZE, acc)
    assert torch.equal(gcraw[0], gcraw[1])
    assert torch.equal(gpart[0], gpart[1])
    assert torch.equal(gpar[0], gpar[1])
    assert bool(gcraw[0].isfinite().all()) and bool(gpar[0].isfinite().all())


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("B,H,W,ht,wt", [(1, 20, 20, 5, 5), (2, 44, 52, 11, 13)])
def test_smask_train_backward_equals_one_segment(hooks, B, H, W, ht, wt, acc):
    L = abi.lib()
    params = list(hooks.quantizers["4"].soft_mask.net.parameters())
    q = core._ptr_struct(abi.SmaskParams, params)
    bits = torch.round(_rand(70 + H, B, ht, wt) * 6.0 + 2.0)
    absmean = _rand(71 + H, B, H, W)
    gm = _rand(72 + H, B, H, W, normal=True)
    gbits = [_rand(73 + H, B, ht, wt, normal=True) for _ in range(2)]       # added to when acc
    gpart = [torch.zeros(L.mcaq_smask_gpart_floats(B), device=DEV) for _ in range(2)]
    gpar = [torch.zeros(SG_SIZE, device=DEV) for _ in range(2)]
    _ok(L.mcaq_smask_train_backward(ctypes.byref(q), _p(bits), _p(absmean), _p(gm), B, H, W, ht, wt, _p(gbits[0]), acc,
                                    _p(gpar[0]), _p(gpart[0]), _stream()), "mcaq_smask_train_backward")
    seg = (abi.SmaskSeg * 1)()
    seg[0].P = q
    seg[0].bits, seg[0].absmean, seg[0].gm, seg[0].gbits, seg[0].gpart = (_p(bits), _p(absmean), _p(gm), _p(gbits[1]),
                                                                           _p(gpart[1]))
    seg[0].B, seg[0].H, seg[0].W, seg[0].ht, seg[0].wt, seg[0].accumulate = B, H, W, ht, wt, acc
    _ok(L.mcaq_smask_train_backward_multi(seg, 1, _stream()), "mcaq_smask_train_backward_multi")
    _reduce1(L, gpart[1], gpar[1], B, SG_SIZE, 0)
    assert torch.equal(gbits[0], gbits[1])
    assert torch.equal(gpart[0], gpart[1])
    assert torch.equal(gpar[0], gpar[1])
    assert bool(gbits[0].isfinite().all()) and bool(gpar[0].isfinite().all()) and bool(gpar[0].any())


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("nparts", [1, 16, 17])      # the 16-deep load groups of the ordered sum: one, full, full + 1
@pytest.mark.parametrize("entry,count", [("mcaq_mapper_train_grad_reduce", MG_SIZE),
                                         ("mcaq_head_train_grad_reduce", CG_SIZE)])
def test_grad_reduce_equals_one_segment_and_ordered_sum(entry, count, nparts, acc):
    L = abi.lib()
    n = nparts * 64 - 5                              # tiles of `nparts` workgroups, the last one partial
    part = _rand(80 + nparts, nparts * count, normal=True)
    start = _rand(81 + nparts, count, normal=True)
    out = [start.clone() for _ in range(2)]
    _ok(getattr(L, entry)(n, _p(part), _p(out[0]), acc, _stream()), entry)
    _reduce1(L, part, out[1], nparts, count, acc)
    assert torch.equal(out[0], out[1])
    s = torch.zeros(count, device=DEV)
    for w in range(nparts):                          # fp32 adds in workgroup order
        s = s + part[w * count:(w + 1) * count]
    assert torch.equal(out[0], start + s if acc else s)
