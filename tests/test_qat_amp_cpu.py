"""mcaq_qat_scale.dtype (the element type of x and grad_x in the QAT kernels)
without a GPU: the struct's layout and ABI version, the launchers' refusals
before any launch, and half maps in train mode on CPU tensors (the
pure-PyTorch path, unchanged by the native GPU route)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from mcaq_yolo_amd import abi

HDR = os.path.join(ROOT, "include", "mcaq_hip.h")


def test_qat_scale_ends_with_dtype():
    assert abi.QatScale._fields_[-1] == ("dtype", abi.I)
    assert abi.QatScale._fields_[-2][0] == "arrive"        # appended: every earlier offset as before
    body = re.search(r"typedef struct \{([^{}]*)\} mcaq_qat_scale;", open(HDR).read()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert body.split(";")[-2].strip() == "int dtype"
    assert abi.QatScale().dtype == abi.DTYPE_F32 == 0       # a zeroed struct is an fp32 call


def test_abi_version_30():
    """Named for the ABI that added the dtype field; pins the current number."""
    assert abi.ABI_VERSION == 31
    assert re.search(r"^#define MCAQ_ABI_VERSION (\d+)", open(HDR).read(), re.M).group(1) == "31"
    if os.path.exists(abi.LIB_PATH):
        assert ctypes.CDLL(abi.LIB_PATH).mcaq_abi_version() == 31


def _scale(dtype):
    q = abi.QatScale()
    for k in ("x", "g", "y", "gx", "work", "bits", "xmin", "xmax"):
        setattr(q, k, 0x1000)            # never dereferenced: every call below is refused first
    q.B, q.C, q.H, q.W, q.ht, q.wt = 1, 8, 16, 16, 4, 4
    q.dtype = dtype
    return q


def test_qat_dtype_refusals_without_gpu():
    """A dtype outside MCAQ_DTYPE_F32 / _F16 / _BF16, and scales of different
    dtype in one launch, are refused before any launch."""
    if not os.path.exists(abi.LIB_PATH):
        pytest.skip("library not built")
    lib = abi._declare(ctypes.CDLL(abi.LIB_PATH))
    inval = 1                            # hipErrorInvalidValue
    for bad in (7, -1, 3):
        q = _scale(bad)
        assert lib.mcaq_qat_forward(ctypes.byref(q), 1, None) == inval
        assert lib.mcaq_qat_backward(ctypes.byref(q), 1, None) == inval
    for a, b in ((abi.DTYPE_F16, abi.DTYPE_BF16), (abi.DTYPE_F32, abi.DTYPE_F16), (abi.DTYPE_BF16, abi.DTYPE_F32)):
        arr = (abi.QatScale * 2)(_scale(a), _scale(b))
        assert lib.mcaq_qat_forward(arr, 2, None) == inval
        assert lib.mcaq_qat_backward(arr, 2, None) == inval
        bits = (abi.P * 2)(0x1000, 0x1000)
        n = (abi.I * 2)(16, 16)
        assert lib.mcaq_qat_forward_budget(arr, 2, bits, n, 2, 4.0, ctypes.c_void_p(0x1000), None, None) == inval


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_cpu_train_half_maps_equal_float_run(dtype):
    """CPU tensors keep the pure-PyTorch path: train-mode hooks on half maps
    give the outputs, aux and parameter gradients of the run on .float(), and
    the map's gradient is that run's rounded to the map's dtype."""
    from mcaq_yolo_amd import train_step
    from mcaq_yolo_amd.hooks import MCAQHooks
    assert train_step.HALF_NATIVE is True
    gen = torch.Generator().manual_seed(5)
    base = [torch.nn.functional.silu(1.5 * torch.randn(2, c, s, s, generator=gen)).to(dtype)
            for c, s in ((8, 16), (16, 8))]
    runs = []
    for widen in (False, True):
        torch.manual_seed(0)
        h = MCAQHooks(device="cpu", grid_size=4).train()
        feats = [(b.float() if widen else b.clone()).requires_grad_(True) for b in base]
        outs, aux = h.forward_features(feats, temperature=1.0)
        loss = sum((o * o).mean() for o in outs) + 0.01 * torch.stack([a["bit_map"].mean() for a in aux]).mean()
        loss.backward()
        runs.append((feats, outs, aux, {k: p.grad for k, p in h.named_parameters()}))
    (fh, oh, ah, gh), (ff, of, af, gf) = runs
    for a, b in zip(oh, of):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    for a, b in zip(ah, af):
        assert torch.equal(a["bit_map"], b["bit_map"]) and torch.equal(a["complexity"], b["complexity"])
    assert any(g is not None for g in gf.values())
    for k in gf:
        assert (gh[k] is None) == (gf[k] is None), k
        if gf[k] is not None:
            assert torch.equal(gh[k], gf[k]), k
    for a, b in zip(fh, ff):
        assert a.grad.dtype == dtype and torch.equal(a.grad, b.grad.to(dtype))
