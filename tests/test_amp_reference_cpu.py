"""half_arithmetic="reference" without a GPU: an fp16 / bf16 map quantized in
the reference's own arithmetic under autocast, every elementwise result
rounded to the map's dtype.

* the hooks on CPU tensors against the reference's outputs on half maps
  (tests/golden/amp_{p3,p4,p5}.npz, keys y_f16 / y_bf16): bit for bit;
* the rounded-fp32 formula the HIP kernel implements, written once here
  (spec_quantize / spec_act: fp32 ops, each followed by one rounding to the
  map's dtype, IEEE fp32 division) against fallback.py's literal half ops on
  small adversarial inputs (equal_nan);
* the answer to "does ATen round the channel sum / tile sum before dividing
  by the count": no - one rounding after the division (C = 3; a 4 x 4 tile
  cannot tell, dividing by 16 is exact, so 3 x 3 windows settle the pool);
* the default mode on the same inputs is the fp32 path."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_weights
from oracle import mcaq_oracle as O

DTS = {"f16": torch.float16, "bf16": torch.bfloat16}


def _r(t, dt):
    return t.to(dt).float()


def spec_quantize(x, bit_map, per_channel=True):
    """The kernel's arithmetic: fp32 operations, each rounded once to x.dtype."""
    dt = x.dtype
    xf = x.float()
    B, C, H, W = xf.shape
    if per_channel:
        mn, mx = xf.amin(dim=(0, 2, 3), keepdim=True), xf.amax(dim=(0, 2, 3), keepdim=True)
    else:
        mn, mx = xf.min(), xf.max()
    eps = _r(torch.tensor(1e-8), dt)
    y = torch.zeros_like(xf)
    for v in torch.unique(bit_map):
        b = int(round(float(v)))
        qmin, qmax = float(-(2 ** (b - 1))), float(2 ** (b - 1) - 1)
        rng = torch.clamp(_r(mx - mn, dt), min=float(eps))
        s = _r(rng / (qmax - qmin), dt)
        zp = torch.clamp(_r(qmin - _r(mn / s, dt), dt), qmin, qmax)
        t = _r(_r(xf / s, dt) + zp, dt)
        xq = _r(_r(torch.clamp(torch.round(t), qmin, qmax) - zp, dt) * s, dt)
        mask = F.interpolate((bit_map == v).float().unsqueeze(1), size=(H, W), mode="nearest")
        y = y + xq * mask
    return y


def spec_act(x, Ht, Wt):
    """The soft mask's side information: am = r(sum_c |x| / C),
    act_tile = r(mean_tile(am)), act = r(act_tile / r(amax + r(1e-8)))."""
    dt = x.dtype
    am = _r(x.float().abs().mean(1, keepdim=True), dt)
    at = _r(F.adaptive_avg_pool2d(am, (Ht, Wt)), dt)
    den = _r(at.amax(dim=(2, 3), keepdim=True) + _r(torch.tensor(1e-8), dt), dt)
    return _r(at / den, dt)


def _bits(B, ht, wt, seed, widths=(2, 3, 4, 5, 6, 7, 8)):
    g = torch.Generator().manual_seed(seed)
    w = torch.tensor(widths, dtype=torch.float32)
    return w[torch.randint(0, len(widths), (B, ht, wt), generator=g)]


def adversarial_cases():
    """(name, x fp32 values exactly representable after the cast, bit map):
    16 x 16 maps with 4 x 4 tiles unless the name says otherwise."""
    g = torch.Generator().manual_seed(7)
    cases = []
    x = torch.randn(1, 3, 16, 16, generator=g) * 3
    cases.append(("c3", x, _bits(1, 4, 4, 1)))
    x = torch.randn(1, 4, 16, 16, generator=g)
    x[:, 1] = 0.75                      # constant channel: fp16 range 0 -> scale 0
    x[:, 2] = 0.0                       # constant zero: min / scale = 0 / 0
    cases.append(("constant", x, _bits(1, 4, 4, 2)))
    x = torch.randn(1, 3, 16, 16, generator=g) * 100
    x[0, 0, 0, 0], x[0, 0, 5, 7] = 65504.0, -65504.0        # fp16: max - min overflows to inf
    x[0, 1] = x[0, 1].abs() * 300 + 20000                   # finite range, (q - zp) * s near the fp16 limit
    x[0, 1, 3, 3] = 65504.0
    x[0, 1, 9, 9] = 200.0
    cases.append(("overflow", x, _bits(1, 4, 4, 3)))
    x = torch.randn(1, 3, 16, 16, generator=g) * 3e-6        # fp16 subnormals (< 6.1e-5)
    x[0, 2] = torch.randn(16, 16, generator=g) * 2e-7
    cases.append(("subnormal", x, _bits(1, 4, 4, 4)))
    x = torch.randn(1, 3, 16, 16, generator=g)
    x[:, 0] = 1.5                       # bf16: range 0 -> r(1e-8) = 1.0012e-8, a finite non-zero scale
    x[:, 1] = torch.randn(16, 16, generator=g) * 1e-8
    cases.append(("tiny_range", x, _bits(1, 4, 4, 5)))
    x = torch.randn(1, 3, 16, 16, generator=g)
    x[0, 1, 2, 2] = float("inf")
    x[0, 2, 4, 4] = float("nan")
    cases.append(("nonfinite", x, _bits(1, 4, 4, 6, widths=(2, 8))))
    x = torch.randn(1, 5, 16, 16, generator=g) * 2
    cases.append(("one_width", x, torch.full((1, 4, 4), 4.0)))
    return cases


CASES = adversarial_cases()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fallback_literal_half_ops_equal_rounded_fp32_spec(case, per_channel, dt):
    from mcaq_yolo_amd import fallback
    _, x, bits = case
    xh = x.to(DTS[dt])
    got = fallback.quantize_reference_half(xh, bits, per_channel)
    want = spec_quantize(xh, bits, per_channel)
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy(), want.numpy(), equal_nan=True)
    a = fallback.soft_mask_act_reference_half(xh, 4, 4)
    assert a.dtype == DTS[dt]
    assert np.array_equal(a.float().numpy(), spec_act(xh, 4, 4).numpy(), equal_nan=True)


def test_adversarial_cases_reach_the_edges():
    """The inputs do what their names say (else the spec test shows nothing)."""
    from mcaq_yolo_amd import fallback
    by = {c[0]: c for c in CASES}
    y = fallback.quantize_reference_half(by["constant"][1].half(), by["constant"][2])
    # scale 0: x / 0 = inf clamps to qmax and (qmax - zp) * 0 = 0; 0 / 0 = NaN stays
    assert bool((y[:, 1] == 0).all()) and torch.isnan(y[:, 2]).all() and torch.isfinite(y[:, 0]).all()
    y = fallback.quantize_reference_half(by["overflow"][1].half(), by["overflow"][2])
    assert torch.isnan(y[:, 0]).all() and torch.isfinite(y[:, 2]).all()
    xs = by["subnormal"][1].half()
    assert bool(((xs != 0) & (xs.abs().float() < 6.1e-5)).any())
    y = fallback.quantize_reference_half(xs, by["subnormal"][2])
    # channels 0 / 1: subnormal results survive; channel 2: the scale itself rounds to 0
    assert torch.isfinite(y[:, :2]).all() and bool(((y[:, :2] != 0) & (y[:, :2].abs() < 6.1e-5)).any())
    assert float(torch.tensor(1e-8).half()) == 0.0 and float(torch.tensor(1e-8).bfloat16()) > 0.0
    y = fallback.quantize_reference_half(by["tiny_range"][1].bfloat16(), by["tiny_range"][2])
    assert torch.isfinite(y).all()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_aten_rounds_once_after_the_division(dt):
    """x.abs().mean(1) and adaptive_avg_pool2d on a half tensor: the fp32 sum
    is divided by the count and rounded once; it is not rounded to half first.
    C = 3 and 3 x 3 windows, where the two variants differ."""
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(2, 3, 16, 16, generator=g) * 3).to(DTS[dt])
    s32 = x.float().abs().sum(1, keepdim=True)
    once, twice = _r(s32 / 3, DTS[dt]), _r(_r(s32, DTS[dt]) / 3, DTS[dt])
    assert int((once != twice).sum()) > 0
    am = x.abs().mean(1, keepdim=True)
    assert torch.equal(am.float(), once)
    # the tile mean: a 4 x 4 window cannot tell (dividing by 16 is exact), so a
    # 12 x 12 plane pooled to 4 x 4 (3 x 3 windows) settles it
    am = am[:, :, :12, :12].contiguous()
    p = F.adaptive_avg_pool2d(am, (4, 4)).float()
    w32 = am.float().reshape(2, 1, 4, 3, 4, 3).permute(0, 1, 2, 4, 3, 5).reshape(2, 1, 4, 4, 9)
    s = torch.zeros(2, 1, 4, 4)
    for i in range(9):                        # row-major, sequential, fp32
        s = s + w32[..., i]
    p_once, p_twice = _r(s / 3 / 3, DTS[dt]), _r(_r(s, DTS[dt]) / 9, DTS[dt])
    assert int((p_once != p_twice).sum()) > 0
    assert torch.equal(p, p_once)
    assert torch.equal(p, _r(F.adaptive_avg_pool2d(am.float(), (4, 4)), DTS[dt]))


def _hooks(d, half_arithmetic=None):
    from mcaq_yolo_amd.hooks import MCAQHooks
    torch.manual_seed(0)
    kw = {} if half_arithmetic is None else {"half_arithmetic": half_arithmetic}
    h = MCAQHooks(grid_size=int(d["grid"]), bit_mapping="mlp", device="cpu", indices=(4,), **kw)
    W = load_weights()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in W.items() if not k.startswith("soft_mask.")}
    sd.update({"quantizers.4." + k: torch.from_numpy(np.asarray(v)) for k, v in W.items() if k.startswith("soft_mask.")})
    h.load_state_dict(sd, strict=False)
    return h.eval()


def _run(h, xt):
    old = torch.get_num_threads()
    torch.set_num_threads(O.REF_THREADS)      # the fixtures' soft-mask softmax thread partition
    try:
        with torch.no_grad():
            return h.forward_features([xt])
    finally:
        torch.set_num_threads(old)


@pytest.mark.parametrize("name", ["p3", "p4", "p5"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_cpu_hooks_reference_mode_vs_reference_fixture(name, dt):
    """The feature: y of a half map is the reference's y, bit for bit."""
    d = np.load(os.path.join(GOLDEN, "amp_%s.npz" % name))
    x = d["x"].astype(np.float32) if dt == "f16" else d["x_bf16"]
    h = _hooks(d, "reference")
    assert "half_arithmetic" not in "".join(h.state_dict().keys())
    outs, aux = _run(h, torch.from_numpy(x).to(DTS[dt]))
    assert np.array_equal(aux[0]["bit_map"].numpy(), d["bits_" + dt])
    assert str(outs[0].dtype) == str(d["y_%s_dtype" % dt])
    assert np.array_equal(outs[0].numpy(), d["y_" + dt])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_default_mode_is_the_fp32_path(dt):
    """half_arithmetic defaults to "fp32": the hooks on a fixture and the
    quantizer on the adversarial inputs give what they give on x.float()."""
    from mcaq_yolo_amd.core import SpatialAdaptiveQuantization
    d = np.load(os.path.join(GOLDEN, "amp_p5.npz"))
    x = d["x"].astype(np.float32) if dt == "f16" else d["x_bf16"]
    h = _hooks(d)
    assert h.half_arithmetic == "fp32" and h.quantizers["4"].half_arithmetic == "fp32"
    outs, _ = _run(h, torch.from_numpy(x).to(DTS[dt]))
    assert np.array_equal(outs[0].numpy(), O.hook_forward(x, load_weights(), int(d["grid"]))["y"])
    assert not np.array_equal(outs[0].numpy(), d["y_" + dt])
    q = SpatialAdaptiveQuantization(smooth_transitions=False).eval()
    for _, xc, bits in CASES:
        xh = xc.to(DTS[dt])
        with torch.no_grad():
            assert np.array_equal(q(xh, bits).numpy(), q(xh.float(), bits).numpy(), equal_nan=True)


def test_mode_is_validated_and_frozen_statistics_keep_fp32():
    from mcaq_yolo_amd.core import SpatialAdaptiveQuantization
    from mcaq_yolo_amd.hooks import MCAQHooks
    with pytest.raises(ValueError):
        SpatialAdaptiveQuantization(half_arithmetic="fp16")
    with pytest.raises(ValueError):
        MCAQHooks(device="cpu", half_arithmetic="half")
    _, x, bits = CASES[0]
    q = SpatialAdaptiveQuantization(smooth_transitions=False, half_arithmetic="reference").eval()
    p = SpatialAdaptiveQuantization(smooth_transitions=False).eval()
    assert q.reference_half(x.half()) and not q.reference_half(x) and not q.reference_half(x.half(), training=True)
    for m in (q, p):
        m.update_running_stats(x)
        m.freeze_calibration()
    assert not q.reference_half(x.half())
    with torch.no_grad():
        assert torch.equal(q(x.half(), bits), p(x.half(), bits))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_soft_mask_stage_source_on_host_vs_cpu_statement(dt):
    """The soft-mask stage of mcaq_morph.h with smask_arith set, compiled for
    the host (tests/emu), against LearnedSoftMask's CPU path in reference
    mode: the m plane bit for bit, NaN activations included.  One-image cases
    are evaluated by torch as two copies (a single image's 3 x 3
    convolution takes an MKL path the kernels do not follow in either mode)."""
    import ctypes
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    from mcaq_yolo_amd import abi, params
    lib = ctypes.CDLL(build_emu.build())
    lib.emu_morph.argtypes = [ctypes.POINTER(abi.MorphScale)]
    sm = params.pack_soft_mask(params.sub(load_weights(), "soft_mask."))
    d = np.load(os.path.join(GOLDEN, "amp_p5.npz"))
    mask = _hooks(d, "reference").quantizers["4"].soft_mask

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)
    g = torch.Generator().manual_seed(3)
    cases = [(x, b) for _, x, b in CASES] + [(torch.randn(2, 16, 20, 20, generator=g) * 2, _bits(2, 5, 5, 8)),
                                             (torch.randn(1, 3, 20, 20, generator=g), _bits(1, 5, 5, 9))]
    old = torch.get_num_threads()
    torch.set_num_threads(O.REF_THREADS)
    try:
        for x, bits in cases:
            xh = x.to(DTS[dt])
            B, _, H, W = xh.shape
            ht, wt = bits.shape[1:]
            x2, b2 = (torch.cat([xh, xh]), torch.cat([bits, bits])) if B == 1 else (xh, bits)
            with torch.no_grad():
                want = mask(b2, x2, half_arithmetic="reference").numpy()[:B, 0]
            am = xh.float().abs().mean(1).numpy().copy()          # pass 1's fp32 plane
            m = np.zeros((B, H, W), np.float32)
            b_in = bits.numpy().astype(np.float32).copy()
            s = abi.MorphScale()
            s.absmean, s.smask, s.bits_in, s.m_out = ptr(am), ptr(sm), ptr(b_in), ptr(m)
            s.B, s.H, s.W, s.Hc, s.Wc, s.tile, s.ht, s.wt = B, H, W, ht * 4, wt * 4, 4, ht, wt
            s.batch_offset, s.batch_total, s.flags, s.hyst_iters = 0, B, abi.F_SOFTMASK, 8
            s.softmax_threads = O.REF_THREADS
            s.temperature, s.min_bits, s.max_bits = 1.0, 2.0, 8.0
            s.smask_arith = abi.DTYPE_F16 if dt == "f16" else abi.DTYPE_BF16
            lib.emu_morph(ctypes.byref(s))
            assert np.array_equal(m, want, equal_nan=True), tuple(xh.shape)
    finally:
        torch.set_num_threads(old)
