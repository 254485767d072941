"""The smoothness term of the QAT loss (MCAQYOLOLoss.compute_smoothness_loss,
models/mcaq_yolo.py:86-107) without a GPU: MCAQHooks.smoothness_loss /
tile_losses on CPU aux records against the torch expression of the
definition, written here,

    S_k = (sum |b[:,1:,:] - b[:,:-1,:]| + sum |b[:,:,1:] - b[:,:,:-1]|) / max(1, n_edges_k)
    n_edges_k = B ((ht - 1) wt + ht (wt - 1)),   L_smooth = (sum_k S_k) / n_scales

its gradient through autograd (sign(0) = 0 at ties), and the additive C ABI:
the new exports, the unchanged version, and the new entries' argument checks
(refused before any launch, so no GPU is touched)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from mcaq_yolo_amd import abi
from mcaq_yolo_amd.hooks import MCAQHooks, smoothness_of

HDR = os.path.join(ROOT, "include", "mcaq_hip.h")
NEW = ("mcaq_qat_forward_tile_losses", "mcaq_tile_losses_forward", "mcaq_qat_smask_backward_tile_losses")
GRIDS = ((1, 1), (1, 4), (4, 1), (5, 5), (3, 5))


def _expr(maps):
    """The definition, in fp64 on the maps' values."""
    tot = 0.0
    for b in maps:
        b = b.double()
        B, ht, wt = b.shape
        n_edges = B * ((ht - 1) * wt + ht * (wt - 1))
        tot = tot + ((b[:, 1:, :] - b[:, :-1, :]).abs().sum() + (b[:, :, 1:] - b[:, :, :-1]).abs().sum()) / max(1, n_edges)
    return tot / len(maps)


def _maps(grids, B=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(2.0 + 6.0 * torch.rand(B, ht, wt, generator=g)) for ht, wt in grids]


def _aux(maps):
    return [{"layer": i, "complexity": torch.zeros_like(m), "bit_map": m, "features_q": None}
            for i, m in enumerate(maps)]


@pytest.mark.parametrize("grid", GRIDS)
def test_smoothness_loss_one_scale(grid):
    (m,) = _maps([grid])
    aux = _aux([m])
    got = MCAQHooks.smoothness_loss(aux)
    ref = _expr([m])
    # fp32 sums of at most 80 positive addends against fp64
    assert abs(float(got) - float(ref)) <= 80 * 2.0 ** -24 * float(ref)
    if grid == (1, 1):
        assert float(got) == 0.0            # no edge: 0 / max(1, 0)
    # what the reference accepts: one 3-D map, one 2-D map, a list of maps
    assert torch.equal(MCAQHooks.smoothness_loss(m), got)
    assert torch.equal(MCAQHooks.smoothness_loss([m]), got)
    assert torch.equal(MCAQHooks.smoothness_loss(m[0]), smoothness_of(m[:1]))


def test_smoothness_loss_scales_and_tile_losses():
    maps = _maps(GRIDS)
    aux = _aux(maps)
    ref = float(_expr(maps))
    got = MCAQHooks.smoothness_loss(aux)
    assert abs(float(got) - ref) <= 80 * 2.0 ** -24 * ref
    h = MCAQHooks(device="cpu")
    t = h.tile_losses(aux, 5.0)
    assert set(t) == {"avg_bits", "loss_bit", "loss_smooth"}
    assert torch.equal(t["loss_smooth"], got)
    avg = torch.stack([m.mean() for m in maps]).mean()
    assert torch.equal(t["avg_bits"], avg) and torch.equal(t["loss_bit"], (avg - 5.0) ** 2)
    assert torch.equal(h.tile_losses(aux)["loss_bit"], (avg - h.target_bits) ** 2)


def test_smoothness_constant_map_is_exactly_zero():
    m = torch.full((2, 5, 5), 4.25, requires_grad=True)
    loss = MCAQHooks.smoothness_loss(_aux([m]))
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert torch.equal(m.grad, torch.zeros_like(m))


def test_smoothness_integer_maps_of_eval_mode():
    m = torch.randint(2, 9, (2, 3, 5), generator=torch.Generator().manual_seed(1))
    got = MCAQHooks.smoothness_loss(_aux([m]))
    assert got.dtype == torch.float32
    assert abs(float(got) - float(_expr([m]))) <= 1e-6


def test_smoothness_gradient_with_ties():
    """The gradient through autograd is s kappa, kappa the sum of
    sign(b - b(neighbour)): 0 across a tie, as abs differentiates."""
    b = torch.tensor([[[3.0, 3.0, 5.0],
                       [3.0, 3.0, 2.0],
                       [4.0, 6.0, 2.0]]], requires_grad=True)
    loss = MCAQHooks.smoothness_loss(_aux([b]))
    loss.backward()
    n_edges = 12
    kappa = torch.tensor([[[0, -1, 2],
                           [-1, 0, -2],
                           [0, 3, -1]]], dtype=torch.float32)
    # (autograd adds a tile's up to four +-1/12 one by one: fp32 rounding apart)
    assert torch.allclose(b.grad, kappa / n_edges, rtol=1e-6, atol=0.0)
    assert torch.equal(b.grad == 0, kappa == 0)
    assert float(b.grad[0, 0, 0]) == 0.0     # the corner tied with both neighbours
    # and over two scales: each map's gradient carries 1 / n_scales
    b2 = b.detach().clone().requires_grad_(True)
    c = torch.full((1, 1, 1), 5.0, requires_grad=True)
    MCAQHooks.smoothness_loss(_aux([b2, c])).backward()
    assert torch.allclose(b2.grad, kappa / 2 / n_edges, rtol=1e-6, atol=0.0)
    assert torch.equal(c.grad, torch.zeros_like(c))


def test_smoothness_loss_of_a_cpu_hook_forward():
    """The aux records of a real forward on CPU tensors (the pure-PyTorch
    path): train mode (continuous bit maps with a graph) and eval mode."""
    torch.manual_seed(0)
    h = MCAQHooks(device="cpu", indices=(4,))
    x = torch.rand(2, 8, 40, 24, generator=torch.Generator().manual_seed(2))
    h.train()
    _, aux = h.forward_features([x])
    got = MCAQHooks.smoothness_loss(aux)
    assert aux[0]["bit_map"].shape == (2, 10, 6) and "_bit_budget" not in aux[0]
    assert abs(float(got.detach()) - float(_expr([aux[0]["bit_map"].detach()]))) <= 1e-6
    assert got.requires_grad
    h.eval()
    with torch.no_grad():
        _, aux = h.forward_features([x])
    assert abs(float(MCAQHooks.smoothness_loss(aux)) - float(_expr([aux[0]["bit_map"]]))) <= 1e-6


def test_new_exports_and_version():
    assert abi.ABI_VERSION == 31
    hdr = open(HDR).read()
    assert re.search(r"^#define MCAQ_ABI_VERSION (\d+)", hdr, re.M).group(1) == "31"
    lib = abi.load_library()
    assert lib.mcaq_abi_version() == 31
    for n in NEW:
        assert n in abi.EXPORTS and hasattr(lib, n)
        assert re.search(r"^int %s\(" % n, hdr, re.M), n
    # additive: the budget struct and the old entries are still declared
    for n in ("mcaq_qat_forward_budget", "mcaq_bit_budget_forward", "mcaq_qat_smask_backward_multi"):
        assert n in abi.EXPORTS and hasattr(lib, n)
    assert abi.TileLosses._fields_[:len(abi.BitBudget._fields_)] == abi.BitBudget._fields_
    assert [f[0] for f in abi.TileLosses._fields_[-2:]] == ["smooth", "g_smooth"]


def test_library_without_the_new_symbols_asks_for_a_rebuild(monkeypatch, tmp_path):
    """An older build of ABI 30 lacks the additive entries: NativeLibraryMissing, no AttributeError."""
    class Old:
        def __getattr__(self, n):
            if n in NEW:
                raise AttributeError("undefined symbol: " + n)
            return ctypes.CFUNCTYPE(ctypes.c_int)(lambda: 30)
    monkeypatch.setattr(ctypes, "CDLL", lambda p: Old())
    with pytest.raises(abi.NativeLibraryMissing, match="rebuild"):
        abi.load_library()


F = 0x1000      # a pointer that is never dereferenced: every call below is refused first
INVAL = 1       # hipErrorInvalidValue


def _scale():
    q = abi.QatScale()
    for k in ("x", "g", "y", "gx", "work", "bits", "xmin", "xmax"):
        setattr(q, k, F)
    q.B, q.C, q.H, q.W, q.ht, q.wt = 1, 8, 16, 16, 4, 4
    return q


def _bad_forward_args():
    """(bits, dims, nseg, avg, tl) of every refused forward call."""
    tl = abi.TileLosses(None, None, None, 4.0, 1, F, None)
    ok_bits = (abi.P * 4)(F, F, F, F)
    ok_dims = (abi.I * 12)(*([1, 4, 4] * 4))
    yield "null avg", ok_bits, ok_dims, 1, None, ctypes.byref(tl)
    yield "nseg 0", ok_bits, ok_dims, 0, F, ctypes.byref(tl)
    yield "nseg 4", ok_bits, ok_dims, 4, F, ctypes.byref(tl)
    yield "null tl", ok_bits, ok_dims, 1, F, None
    yield "null dims", ok_bits, None, 1, F, ctypes.byref(tl)
    yield "null bit map", (abi.P * 1)(None), ok_dims, 1, F, ctypes.byref(tl)
    for k in range(3):
        for v in (0, -1):
            d = [2, 4, 4, 2, 4, 4]
            d[3 + k] = v
            yield "dims[%d] = %d" % (3 + k, v), ok_bits, (abi.I * 6)(*d), 2, F, ctypes.byref(tl)


def test_forward_entries_refuse_bad_arguments():
    lib = abi.load_library()
    q = _scale()
    for what, bits, dims, nseg, avg, tl in _bad_forward_args():
        assert lib.mcaq_tile_losses_forward(bits, dims, nseg, avg, F, tl, None) == INVAL, what
        assert lib.mcaq_qat_forward_tile_losses(ctypes.byref(q), 1, bits, dims, nseg, avg, F, tl, None) == INVAL, what
    tl = abi.TileLosses(None, None, None, 4.0, 1, F, None)
    bits, dims = (abi.P * 1)(F), (abi.I * 3)(1, 4, 4)
    for bad_nscales in (0, 4):
        assert lib.mcaq_qat_forward_tile_losses(ctypes.byref(q), bad_nscales, bits, dims, 1, F, F, ctypes.byref(tl),
                                                None) == INVAL


def _seg(**kw):
    s = abi.QatSmaskSeg()
    s.P = abi.SmaskParams(F, F, F, F)
    s.bits = s.absmean = s.qat_work = s.gbits = s.gpart = F
    s.B, s.C, s.H, s.W, s.ht, s.wt = 1, 8, 16, 16, 4, 4
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_backward_entry_refuses_bad_arguments():
    lib = abi.load_library()
    tl = abi.TileLosses(F, None, None, 4.0, 1, None, F)
    f = lib.mcaq_qat_smask_backward_tile_losses
    one = (abi.QatSmaskSeg * 4)(_seg(), _seg(), _seg(), _seg())
    assert f(one, 0, ctypes.byref(tl), None) == INVAL
    assert f(one, 4, ctypes.byref(tl), None) == INVAL
    assert f(one, 1, None, None) == INVAL
    assert f(None, 1, ctypes.byref(tl), None) == INVAL
    assert f((abi.QatSmaskSeg * 1)(_seg(gbits=None)), 1, ctypes.byref(tl), None) == INVAL     # null output
    for k in ("B", "C", "ht", "wt", "H", "W"):
        for v in (0, -1):
            assert f((abi.QatSmaskSeg * 1)(_seg(**{k: v})), 1, ctypes.byref(tl), None) == INVAL, (k, v)
    bad = abi.TileLosses(F, None, None, 4.0, 0, None, F)          # nscales < 1
    assert f(one, 1, ctypes.byref(bad), None) == INVAL
    bad = abi.TileLosses(None, F, None, 4.0, 1, None, F)          # a budget gradient without the forward's avg
    assert f(one, 1, ctypes.byref(bad), None) == INVAL
