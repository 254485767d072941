"""The train-step kernels of csrc/mcaq_train.h at their C ABI entries against
the float64 references of tests/train_cases.py, by its rule: for tensor k

    max |got_k - ref_k| <= min(8 * max(e32_k, eps32 * S_k), 1e-3 * S_k)

(e32_k: what the fp32 restatement of the same case loses against float64; S_k:
the tensor's or its module's largest reference magnitude).  Counters and
refusal codes are compared exactly.  Where an entry accumulates into a buffer
that held `start`, got - start is compared and the bound grows by the one fp32
rounding of start + g: |start| <= max |ref_k|, so by eps32 * max |ref_k|.

MCAQ_TRAIN_VALUES_OUT=<file>: the measured ratio max |got - ref| / max(e32,
eps32 * S) of every (case, tensor) is written there as JSON
(profiles/train_values.json is one such run)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import train_cases as tc
from conftest import load_weights
from mcaq_yolo_amd import abi, core
from mcaq_yolo_amd.core import _p, _stream
from test_train_entries_gpu import CG_SIZE, MG_SIZE, SG_SIZE, _mseg, _ok, _reduce1
from test_train_fused_gpu import DEV, _check_step_vs_torch

pytestmark = pytest.mark.gpu
INVALID = 1      # hipErrorInvalidValue: an entry's refusal
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_file():
    yield
    out = os.environ.get("MCAQ_TRAIN_VALUES_OUT")
    if out and RATIOS:
        worst = max(((r, c, k) for c, d in RATIOS.items() for k, r in d.items()), default=None)
        with open(out, "w") as f:
            json.dump({"rule": "max|got-ref| / max(e32, eps32*S); pass at <= 8 (and <= 1e-3 S)",
                       "largest": {"ratio": worst[0], "case": worst[1], "tensor": worst[2]}, "ratios": RATIOS},
                      f, indent=1, sort_keys=True)


def _check(case, got, exact=None, extra=None, record=True):
    ratios = {k: case.ratio(k, got[k]) for k in case.ref}
    for k in sorted(ratios, key=ratios.get, reverse=True)[:6]:
        print("%-26s %-24s err %.3g e32 %.3g S %.3g ratio %.3g" % (case.name, k, case.error(k, got[k]), case.e32[k],
                                                                 case.S[k], ratios[k]))
    if record:
        RATIOS[case.name] = ratios
    bad = case.failures(got, extra=extra)
    assert not bad, bad
    for k, v in case.exact.items():
        assert exact[k] == v, (k, exact[k], v)


def _split(flat, case, names):
    out, o = {}, 0
    for k in names:
        n = case.ref["grad." + k].numel()
        out["grad." + k] = flat[o:o + n]
        o += n
    assert o == flat.numel()
    return out


def _start(case, names, seed):
    """A buffer the entry accumulates into: per tensor uniform in +-max |ref_k|; the matching allowance."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    parts, extra = [], {}
    for k in names:
        r = case.ref["grad." + k]
        parts.append(((torch.rand(r.numel(), generator=g) * 2.0 - 1.0) * float(r.abs().max())).float())
        extra["grad." + k] = tc.EPS32 * float(r.abs().max())
    return torch.cat(parts).to(DEV), extra


def _golden(prefix, names):
    W = load_weights()
    return [torch.from_numpy(np.asarray(W[prefix + k])).to(DEV).contiguous() for k in names]


def _offset(t, off):
    """A copy of t whose base lies `off` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, device=DEV)
    lead = (-(buf.data_ptr() // 4)) % 4 + off
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


# ---- mapper -----------------------------------------------------------------
MAPPER_ACC = ("mapper_n1", "mapper_n65")              # the accumulating reduction: one workgroup's partials, two


@pytest.mark.parametrize("name,acc", [(n, 0) for n in tc.names("mapper")] + [(n, 1) for n in MAPPER_ACC])
def test_mapper_train_values(name, acc):
    case = tc.case(name)
    cfg = case.cfg
    L = abi.lib()
    W = load_weights()
    m = core.ComplexityToBitMappingNetwork().to(DEV)
    m.load_state_dict({k[len("bit_mapper."):]: torch.from_numpy(np.asarray(v))
                       for k, v in W.items() if k.startswith("bit_mapper.")})
    net = m.mapping_network.train()
    q = core._mapper_params(net)
    n = cfg["n"]
    T = 0.0 if cfg["T"] is None else max(float(cfg["T"]), 0.1)       # the host's floor (core._MapperTrainFn)
    c, gbits = case.inp["c"].to(DEV), case.inp["gbits"].to(DEV)
    work = torch.zeros(L.mcaq_mapper_work_floats(n), device=DEV)
    bits = torch.zeros(n, device=DEV)
    _ok(L.mcaq_mapper_train_forward(ctypes.byref(q), _p(c), n, tc.MIN_B, tc.MAX_B, T, 0.1, cfg["round"],
                                    cfg["update_stats"], _p(bits), _p(work), _stream()),
        "mcaq_mapper_train_forward")
    ng = L.mcaq_mapper_gpart_floats(n)
    assert ng // MG_SIZE == (n + tc.TR_TPB - 1) // tc.TR_TPB
    gc = torch.zeros(n, device=DEV)
    gpart = torch.zeros(ng, device=DEV)
    start, extra = _start(case, tc.MAPPER_PARAMS, 7) if acc else (torch.randn(MG_SIZE).to(DEV), None)
    gpar = start.clone()
    _ok(L.mcaq_mapper_train_backward_multi(ctypes.byref(q), _mseg(c, bits, work, gbits, gc, gpart), 1, tc.MIN_B,
                                           tc.MAX_B, T, _stream()), "mcaq_mapper_train_backward_multi")
    _reduce1(L, gpart, gpar, ng // MG_SIZE, MG_SIZE, acc)
    torch.cuda.synchronize()
    got = {"bits": bits, "g_c": gc}
    got.update(_split(gpar.double() - start.double() if acc else gpar, case, tc.MAPPER_PARAMS))
    rstat = work[-3 * 128:]                              # MapperWork.rstat: the buffer's last region
    for layer, bn in enumerate((1, 4, 7)):
        width = net[bn].running_mean.numel()
        got["running_mean.%d" % bn], got["running_var.%d" % bn] = net[bn].running_mean, net[bn].running_var
        if cfg["update_stats"] == 2:
            got["rstat.mean.%d" % bn] = rstat[layer * 128:layer * 128 + width]
            got["rstat.var.%d" % bn] = rstat[layer * 128 + 64:layer * 128 + 64 + width]
    exact = {"num_batches_tracked.%d" % bn: int(net[bn].num_batches_tracked) for bn in (1, 4, 7)}
    _check(case, got, exact, extra, record=not acc)


# ---- analyzer head ----------------------------------------------------------
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("name", tc.names("head"))
def test_head_train_values(name, acc):
    case = tc.case(name)
    B, ht, wt = case.cfg["shape"]
    n = B * ht * wt
    L = abi.lib()
    params = _golden("complexity_analyzer.complexity_mlp.", tc.CMLP_PARAMS)
    q = core._ptr_struct(abi.CmlpParams, params)
    phi, craw, gC = (case.inp[k].to(DEV).contiguous() for k in ("phi", "craw", "gC"))
    gcraw = torch.zeros(n, device=DEV)
    gpart = torch.zeros(L.mcaq_head_gpart_floats(n), device=DEV)
    start, extra = _start(case, tc.CMLP_PARAMS, 8) if acc else (torch.randn(CG_SIZE).to(DEV), None)
    gpar = start.clone()
    _ok(L.mcaq_head_train_backward(ctypes.byref(q), _p(phi), _p(craw), _p(gC), B, ht, wt, _p(gcraw), _p(gpar),
                                   _p(gpart), acc, _stream()), "mcaq_head_train_backward")
    torch.cuda.synchronize()
    got = {"gcraw": gcraw}
    got.update(_split(gpar.double() - start.double() if acc else gpar, case, tc.CMLP_PARAMS))
    _check(case, got, extra=extra, record=not acc)


def test_head_entry_refuses_past_the_lds_bound():
    """25 x 31 = 775 tiles: the first grid past 53 floats x 768 tiles of LDS.
    The entry returns hipErrorInvalidValue before any launch and writes
    nothing; core._head_bwd_fits routes the shape to the torch path."""
    B, ht, wt = 1, 25, 31
    assert not core._head_bwd_fits(ht, wt) and core._head_bwd_fits(24, 32)
    n = B * ht * wt
    L = abi.lib()
    params = _golden("complexity_analyzer.complexity_mlp.", tc.CMLP_PARAMS)
    q = core._ptr_struct(abi.CmlpParams, params)
    phi, craw, gC = torch.rand(n, 8, device=DEV), torch.rand(B, ht, wt, device=DEV), torch.randn(B, ht, wt, device=DEV)
    gcraw = torch.full((n,), 7.0, device=DEV)
    gpar = torch.full((CG_SIZE,), 7.0, device=DEV)
    gpart = torch.zeros(L.mcaq_head_gpart_floats(n), device=DEV)
    err = L.mcaq_head_train_backward(ctypes.byref(q), _p(phi), _p(craw), _p(gC), B, ht, wt, _p(gcraw), _p(gpar),
                                     _p(gpart), 0, _stream())
    torch.cuda.synchronize()
    assert err == INVALID
    assert bool((gcraw == 7.0).all()) and bool((gpar == 7.0).all())


# ---- soft mask, plain mode --------------------------------------------------
SMASK_ACC = ("smask_8x8_t2", "smask_21x23_t5")       # the accumulating store: a staged and an unstaged case


@pytest.mark.parametrize("name,acc", [(n, 0) for n in tc.names("smask")] + [(n, 1) for n in SMASK_ACC])
def test_smask_train_values(name, acc):
    case = tc.case(name)
    B, H, W, ht, wt = case.cfg["shape"]
    L = abi.lib()
    params = _golden("soft_mask.", tc.SMASK_PARAMS)
    q = core._ptr_struct(abi.SmaskParams, params)
    off = case.cfg.get("offset", 0)
    bits = case.inp["bits"].to(DEV).contiguous()
    absmean, gm = _offset(case.inp["absmean"].to(DEV), off), _offset(case.inp["gm"].to(DEV), off)
    extra = None
    if acc:
        r = case.ref["g_bits"]
        start = ((torch.rand(r.shape, generator=torch.Generator().manual_seed(9)) * 2.0 - 1.0) *
                 float(r.abs().max())).float().to(DEV)
        extra = {"g_bits": tc.EPS32 * float(r.abs().max())}
    else:
        start = torch.randn(B, ht, wt).to(DEV)
    gbits = start.clone()
    gpart = torch.zeros(L.mcaq_smask_gpart_floats(B), device=DEV)
    gpar = torch.randn(SG_SIZE).to(DEV)                  # overwritten
    _ok(L.mcaq_smask_train_backward(ctypes.byref(q), _p(bits), _p(absmean), _p(gm), B, H, W, ht, wt, _p(gbits), acc,
                                    _p(gpar), _p(gpart), _stream()), "mcaq_smask_train_backward")
    torch.cuda.synchronize()
    got = {"g_bits": gbits.double() - start.double() if acc else gbits}
    got.update(_split(gpar, case, tc.SMASK_PARAMS))
    _check(case, got, extra=extra, record=not acc)


# ---- soft mask, fold mode ---------------------------------------------------
@pytest.mark.parametrize("name", tc.names("fold"))
def test_qat_smask_fold_values(name):
    case = tc.case(name)
    cfg = case.cfg
    B, H, W, ht, wt = cfg["shape"]
    L = abi.lib()
    params = _golden("soft_mask.", tc.SMASK_PARAMS)
    bits = case.inp["bits"].to(DEV).contiguous()
    absmean = _offset(case.inp["absmean"].to(DEV), 0)
    qwork = _offset(case.inp["qwork"].to(DEV), cfg.get("qoffset", 0))
    avg, g_avg, g_loss = (case.inp[k].to(DEV) for k in ("avg", "g_avg", "g_loss"))
    gbits = torch.randn(B, ht, wt).to(DEV)               # overwritten
    gpart = torch.zeros(L.mcaq_smask_gpart_floats(B), device=DEV)
    gpar = torch.randn(SG_SIZE).to(DEV)
    seg = (abi.QatSmaskSeg * 1)()
    seg[0].P = core._ptr_struct(abi.SmaskParams, params)
    seg[0].bits, seg[0].absmean, seg[0].qat_work, seg[0].gbits, seg[0].gpart = (_p(bits), _p(absmean), _p(qwork),
                                                                                 _p(gbits), _p(gpart))
    seg[0].B, seg[0].C, seg[0].H, seg[0].W, seg[0].ht, seg[0].wt = B, cfg["C"], H, W, ht, wt
    bb = abi.BitBudget(_p(avg), _p(g_avg), _p(g_loss), cfg["target"], cfg["nscales"])
    _ok(L.mcaq_qat_smask_backward_multi(seg, 1, ctypes.byref(bb), _stream()), "mcaq_qat_smask_backward_multi")
    _reduce1(L, gpart, gpar, B, SG_SIZE, 0)
    torch.cuda.synchronize()
    got = {"g_bits": gbits}
    got.update(_split(gpar, case, tc.SMASK_PARAMS))
    _check(case, got)


# ---- the hook step at ragged maps -------------------------------------------
def test_fused_train_step_ragged_maps_matches_torch_path():
    """The three hooks at 33x41 / 20x20 / 12x12 maps (tile grids 8x10, 5x5,
    3x3) of 12 / 8 / 16 channels, B = 2: the fused step against the torch path
    at test_train_fused_gpu's tolerances.  Where a fused launcher cannot take
    a shape the hook takes the torch path; the comparison is the same."""
    _check_step_vs_torch(1.0, B=2, shapes=((12, (33, 41)), (8, (20, 20)), (16, (12, 12))))
