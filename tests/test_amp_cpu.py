"""fp16 / bf16 feature maps, the parts that need no GPU: the result type of
the reference on half maps (tests/golden/amp_types.npz) on the package's CPU
path, the Python gate engine.half_native_ok against the conditions of
mcaq_quant's tile-aligned path, and the measured gap between the fp32
arithmetic this package keeps on half maps and the reference's per-op half
arithmetic (reference data only: DESIGN s.11 quotes these numbers)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_weights
from oracle import mcaq_oracle as O

f32 = np.float32
DTS = {"f16": torch.float16, "bf16": torch.bfloat16}
AMP_KEYS = ["%s_s%d_c%d" % (dt, s, c) for dt in ("f16", "bf16") for s in (1, 0) for c in (1, 0)]


def test_amp_types_fixture_is_fp32_everywhere():
    """What the reference does (quantization.py:732-738: the fp32 tile mask
    promotes the sum): fp32 for fp16 and bf16 maps, with and without the soft
    mask, per channel or per tensor."""
    d = np.load(os.path.join(GOLDEN, "amp_types.npz"))
    assert sorted(k[6:] for k in d.files if k.startswith("dtype_")) == sorted(AMP_KEYS)
    assert {str(d["dtype_" + k]) for k in AMP_KEYS} == {"torch.float32"}


@pytest.mark.parametrize("key", AMP_KEYS)
def test_cpu_path_result_type_vs_reference(key):
    """The hooks on CPU tensors (the pure-PyTorch path) return the reference's
    result type and bits on a half map, and the oracle's y."""
    from mcaq_yolo_amd.hooks import MCAQHooks
    d = np.load(os.path.join(GOLDEN, "amp_types.npz"))
    dt, smooth, per_channel = key.split("_")[0], key.split("_")[1] == "s1", key.split("_")[2] == "c1"
    want = getattr(torch, str(d["dtype_" + key]).split(".")[1])
    xw = d["x"].astype(f32) if dt == "f16" else d["x_bf16"]
    W = load_weights()
    torch.manual_seed(0)
    h = MCAQHooks(grid_size=int(d["grid"]), bit_mapping="mlp", device="cpu", indices=(4,))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in W.items() if not k.startswith("soft_mask.")}
    sd.update({"quantizers.4." + k: torch.from_numpy(np.asarray(v)) for k, v in W.items() if k.startswith("soft_mask.")})
    h.load_state_dict(sd, strict=False)
    h.eval()
    q = h.quantizers["4"]
    q.smooth_transitions, q.per_channel = smooth, per_channel
    with torch.no_grad():
        outs, aux = h.forward_features([torch.from_numpy(xw).to(DTS[dt])])
    assert outs[0].dtype == want
    assert np.array_equal(aux[0]["bit_map"].numpy(), d["bits_" + key])
    if per_channel:
        mn, mx = xw.min(axis=(0, 2, 3)), xw.max(axis=(0, 2, 3))
    else:
        mn, mx = np.full(xw.shape[1], xw.min(), f32), np.full(xw.shape[1], xw.max(), f32)
    ref = O.hook_forward(xw, W, int(d["grid"]), smooth=smooth, xmin=mn, xmax=mx)
    assert np.array_equal(outs[0].numpy(), ref["y"])


def _qmaxnt():
    src = open(os.path.join(ROOT, "mcaq_yolo_amd", "csrc", "mcaq_quant.h")).read()
    return int(re.search(r"constexpr int QMAXNT = (\d+);", src).group(1))


def _tile_ok(H, W, ht, wt, nbits, qmaxnt):
    """mcaq_quant's tile-aligned family (csrc/mcaq_quant.h, quant_plan: `vec` geometry +
    `tile`), restated: the only pass-2 kernels that read a half map."""
    sh = sw = 0
    while (ht << sh) < H:
        sh += 1
    while (wt << sw) < W:
        sw += 1
    return (ht << sh) == H and (wt << sw) == W and sw >= 2 and nbits <= 8 and ht * wt <= qmaxnt and (H * W) % 4 == 0


def test_half_native_gate_equals_tile_kernel_conditions():
    """engine.half_native_ok (Python) and tile_ok in mcaq_quant (host C++)
    must agree: a map the gate lets through that the launcher turns away
    makes the hook raise.  Every H, W in 4..160 x grid x bit range."""
    from mcaq_yolo_amd.engine import ScaleGeom, half_native_ok
    qmaxnt = _qmaxnt()
    n = accepted = 0
    for grid in (2, 4, 8, 16):
        for H in range(4, 161):
            for W in range(4, 161):
                try:
                    g = ScaleGeom(1, 1, H, W, grid)
                except ValueError:
                    continue          # smaller than one tile: no plan exists
                for lo, hi in ((2, 8), (4, 8), (1, 9)):
                    want = _tile_ok(H, W, g.ht, g.wt, hi - lo + 1, qmaxnt)
                    assert half_native_ok(g, float(lo), float(hi)) == want, (H, W, grid, lo, hi)
                    n += 1
                    accepted += want
    assert n > 250000 and 0 < accepted < n
    # every shape of the GPU edge tests is native
    from test_amp_edges_gpu import SHAPES
    for shape, grid in SHAPES + [((2, 40, 16, 16), 8), ((2, 12, 16, 16), 8), ((2, 16, 20, 20), 8)]:
        assert half_native_ok(ScaleGeom(*shape, grid)), shape
    assert not half_native_ok(ScaleGeom(2, 16, 10, 10, 8))


@pytest.mark.parametrize("name", ["p3", "p4", "p5"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gap_to_reference_half_arithmetic(name, dt):
    """The reference's quantizer rounds every elementwise op to fp16 / bf16 on
    a half map; this package keeps fp32 arithmetic on the widened map (the
    oracle's y, to which the kernels are pinned bit for bit).  The distance
    between the two is a property of reference data alone: measured and
    printed here (DESIGN s.11), asserted finite."""
    d = np.load(os.path.join(GOLDEN, "amp_%s.npz" % name))
    x = d["x"].astype(f32) if dt == "f16" else d["x_bf16"]
    y32 = O.hook_forward(x, load_weights(), int(d["grid"]))["y"]
    yh = d["y_" + dt]
    assert np.isfinite(y32).all() and np.isfinite(yh).all()
    gap = float(np.abs(y32 - yh).max())
    frac = float((np.abs(y32 - yh) > 1e-4 * np.abs(yh)).mean())
    print("amp %s %s: max |y_fp32_arith - y_ref_half_arith| = %.4g, %.1f %% of elements differ by > 1e-4 relative"
          % (name, dt, gap, 100.0 * frac))
    assert np.isfinite(gap) and np.isfinite(frac)
