"""half_arithmetic="reference" on the GPU: mcaq_quant_tile_ref_kernel and the
soft-mask stage's rounded side information against the reference's outputs on
half maps (tests/golden/amp_*.npz) and against the CPU statement of the mode
(fallback.quantize_reference_half / soft_mask_act_reference_half through the
modules on CPU tensors), bit for bit with equal_nan."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_weights
from oracle import mcaq_oracle as O
from test_amp_edges_gpu import SHAPES, leaky_gaussian
from test_amp_reference_cpu import CASES, _bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTS = {"f16": torch.float16, "bf16": torch.bfloat16}


def _hooks(dev, grid=8, smooth=True, per_channel=True, half_arithmetic="reference"):
    from mcaq_yolo_amd.hooks import MCAQHooks
    torch.manual_seed(0)
    h = MCAQHooks(grid_size=grid, bit_mapping="mlp", device=dev, half_arithmetic=half_arithmetic)
    sd = {}
    for k, v in load_weights().items():
        t = torch.from_numpy(np.asarray(v))
        if k.startswith("soft_mask."):
            for idx in (4, 6, 9):
                sd["quantizers.%d.%s" % (idx, k)] = t
        else:
            sd[k] = t
    h.load_state_dict(sd, strict=False)
    for q in h.quantizers.values():
        q.smooth_transitions = smooth
        q.per_channel = per_channel
    h.softmax_threads = O.REF_THREADS
    return h.eval()


class _threads:
    """The soft mask's softmax follows ATen's thread partition: the CPU run and
    the kernels that reproduce it see the same thread count."""

    def __enter__(self):
        self.old = torch.get_num_threads()
        torch.set_num_threads(O.REF_THREADS)

    def __exit__(self, *exc):
        torch.set_num_threads(self.old)
        return False


@pytest.fixture(scope="module")
def quantizers():
    """(GPU, CPU) quantizer modules with the fixture soft-mask weights."""
    return _hooks(DEV).quantizers["4"], _hooks("cpu").quantizers["4"]


def _cpu_statement(qc, xh, bits):
    """The CPU statement's y.  A single image with the soft mask on is
    evaluated as a batch of two copies (image 0 taken): ATen runs a one-image
    3 x 3 convolution through an MKL matrix product whose summation order the
    kernels' unchanged fp32 soft-mask network does not follow in either
    arithmetic mode (they follow oneDNN's, used from batch 2 on);
    the copy changes neither the batch statistics nor the widths present.  At
    the tile counts used here (<= 25 per image, 8 threads) every softmax
    position takes the scalar exp in both batch partitions."""
    if xh.shape[0] == 1 and qc.smooth_transitions:
        return qc(torch.cat([xh, xh]), torch.cat([bits, bits]), training=False)[:1]
    return qc(xh, bits, training=False)


def _both(quantizers, xh, bits, smooth, per_channel):
    """y of the GPU module and of the CPU statement for one half map."""
    qg, qc = quantizers
    for q in (qg, qc):
        q.smooth_transitions, q.per_channel = smooth, per_channel
    with _threads(), torch.no_grad():
        yg = qg(xh.to(DEV), bits.to(DEV), training=False)
        torch.cuda.synchronize()
        yc = _cpu_statement(qc, xh, bits)
    assert yg.dtype == torch.float32 and yc.dtype == torch.float32 and yg.shape == yc.shape
    return yg.cpu().numpy(), yc.numpy()


def _eq(a, b, what=""):
    assert np.array_equal(a, b, equal_nan=True), "%s: %d of %d elements differ" % (
        what, int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum()), a.size)


@pytest.mark.parametrize("name", ["p3", "p4", "p5"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gpu_hooks_reference_mode_vs_reference_fixture(name, dt):
    d = np.load("%s/amp_%s.npz" % (GOLDEN, name))
    x = d["x"].astype(np.float32) if dt == "f16" else d["x_bf16"]
    h = _hooks(DEV, int(d["grid"]))
    with torch.no_grad():
        outs, aux = h.forward_features([torch.from_numpy(x).to(DEV).to(DTS[dt])])
    torch.cuda.synchronize()
    assert np.array_equal(aux[0]["bit_map"].cpu().numpy(), d["bits_" + dt])
    assert outs[0].dtype == torch.float32 and str(outs[0].dtype) == str(d["y_%s_dtype" % dt])
    assert np.array_equal(outs[0].cpu().numpy(), d["y_" + dt])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("hw", [16, 20])
@pytest.mark.parametrize("C", [1, 3, 12, 40])
def test_kernel_vs_cpu_statement_small(quantizers, C, hw, per_channel, smooth, dt):
    """B = 1, slice tails (C = 1, 3, 12, and 40 = a second slice of 8), a
    whole 256-pixel unit (16 x 16) and a partial second one (20 x 20)."""
    xh = leaky_gaussian((1, C, hw, hw), 100 * C + hw).to(DTS[dt])
    bits = _bits(1, hw // 4, hw // 4, C + hw)
    yg, yc = _both(quantizers, xh, bits, smooth, per_channel)
    _eq(yg, yc, "C=%d %dx%d" % (C, hw, hw))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape,grid", SHAPES)
def test_kernel_vs_cpu_statement_edge_shapes(quantizers, shape, grid, dt):
    """The shapes of the fp32-arithmetic edge tests: several slices, 400 tiles,
    64-pixel tiles, images smaller than a unit."""
    from mcaq_yolo_amd.engine import ScaleGeom
    g = ScaleGeom(*shape, grid)
    xh = leaky_gaussian(shape, sum(shape) + 1).to(DTS[dt])
    bits = _bits(shape[0], g.ht, g.wt, sum(shape))
    yg, yc = _both(quantizers, xh, bits, True, True)
    _eq(yg, yc, str(shape))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_vs_cpu_statement_adversarial(quantizers, case, per_channel, dt):
    """Constant channels (fp16 scale 0), a range that overflows fp16, fp16
    subnormals, bf16's non-zero r(1e-8), inf / NaN in x: the literal chain and
    the NaN a non-finite x_q of another present width leaves through x_q * 0."""
    _, x, bits = case
    xh = x.to(DTS[dt])
    for smooth in (False, True):
        yg, yc = _both(quantizers, xh, bits, smooth, per_channel)
        _eq(yg, yc, "%s smooth=%s" % (case[0], smooth))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_views_offset_and_non_contiguous(quantizers, dt):
    """A 16-byte aligned offset view runs the kernel, a 2-byte aligned one the
    torch restatement on the device, a strided view is made contiguous: all
    give the CPU statement's y of the same values."""
    shape = (1, 12, 16, 16)
    n = int(np.prod(shape))
    base = leaky_gaussian(shape, 5).to(DTS[dt])
    bits = _bits(1, 4, 4, 9)
    qg, qc = quantizers
    for q in (qg, qc):
        q.smooth_transitions, q.per_channel = True, True
    with _threads(), torch.no_grad():
        want = _cpu_statement(qc, base, bits).numpy()
        for off in (8, 1):
            buf = torch.zeros(n + 8, dtype=DTS[dt], device=DEV)
            buf[off:off + n] = base.reshape(-1).to(DEV)
            xv = buf[off:off + n].view(shape)
            assert xv.data_ptr() % 16 == (2 * off) % 16
            _eq(qg(xv, bits.to(DEV), training=False).cpu().numpy(), want, "offset %d" % off)
        wide = torch.zeros(1, 12, 16, 32, dtype=DTS[dt], device=DEV)
        wide[..., ::2] = base.to(DEV)
        xs = wide[..., ::2]
        assert not xs.is_contiguous()
        _eq(qg(xs, bits.to(DEV), training=False).cpu().numpy(), want, "strided")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("per_channel", [True, False])
def test_hook_plan_equals_module_path(dt, per_channel):
    """HookPlan.run (the planned / captured path) and the quantizer module on
    the hook's bit map agree, and differ from the default mode."""
    from mcaq_yolo_amd.engine import HookPlan, ScaleGeom
    shape = (2, 40, 16, 16)
    xh = leaky_gaussian(shape, 21).to(DTS[dt]).to(DEV)
    h = _hooks(DEV, 8, True, per_channel)
    with _threads(), torch.no_grad():
        outs, aux = h.forward_features([xh])
        ym = h.quantizers["4"](xh, aux[0]["bit_map"], training=False)
        an, q = h.complexity_analyzer, h.quantizers["4"]
        plan = HookPlan([ScaleGeom(*shape, 8)], DEV)
        b = plan.run([xh], an.cmlp_blob(), h.bit_mapper.mapper_blob(), [q.soft_mask.blob()], per_tensor=not per_channel,
                     softmax_threads=O.REF_THREADS, half_arithmetic="reference")[0]
        torch.cuda.synchronize()
        h32 = _hooks(DEV, 8, True, per_channel, half_arithmetic="fp32")
        o32, a32 = h32.forward_features([xh])
    assert torch.equal(b["bits"], aux[0]["bit_map"]) and torch.equal(a32[0]["bit_map"], aux[0]["bit_map"])
    assert torch.equal(b["y"], outs[0]) and torch.equal(ym, outs[0])
    assert not torch.equal(o32[0], outs[0])
    with pytest.raises(ValueError, match="reference"):
        plan.run([xh.float()], an.cmlp_blob(), h.bit_mapper.mapper_blob(), [q.soft_mask.blob()],
                 softmax_threads=O.REF_THREADS, half_arithmetic="reference")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_non_native_geometry_equals_cpu_statement(dt):
    """(2, 16, 10, 10) at grid 8 crops to 8 x 8: pass 2 does not take the half
    map, and the hook runs the torch restatement on the device tensor - not the
    fp32 arithmetic."""
    from mcaq_yolo_amd.engine import ScaleGeom, half_native_ok
    shape = (2, 16, 10, 10)
    assert not half_native_ok(ScaleGeom(*shape, 8))
    xh = leaky_gaussian(shape, 33).to(DTS[dt])
    with _threads(), torch.no_grad():
        og, ag = _hooks(DEV).forward_features([xh.to(DEV)])
        oc, ac = _hooks("cpu").forward_features([xh])
        o32, _ = _hooks(DEV, half_arithmetic="fp32").forward_features([xh.to(DEV)])
    assert np.array_equal(ag[0]["bit_map"].cpu().numpy(), ac[0]["bit_map"].numpy())
    assert og[0].dtype == torch.float32
    _eq(og[0].cpu().numpy(), oc[0].numpy(), "10x10")
    assert not torch.equal(o32[0], og[0])


def test_abi_refuses_reference_arithmetic_where_it_does_not_apply():
    from mcaq_yolo_amd import abi
    lib = abi.lib()
    ENOTSUP = 801      # hipErrorNotSupported
    B, C, H, W, ht, wt = 1, 4, 16, 16, 4, 4
    y = torch.empty(B, C, H, W, device=DEV)
    bits = torch.full((B, ht, wt), 4.0, device=DEV)
    lo, hi = torch.full((C,), -1.0, device=DEV), torch.full((C,), 1.0, device=DEV)

    def scale(x, dtype, **kw):
        q = abi.QuantScale()
        q.x, q.y, q.bits, q.xmin, q.xmax = (ctypes.c_void_p(t.data_ptr()) for t in (x, y, bits, lo, hi))
        q.B, q.C, q.H, q.W, q.ht, q.wt = B, C, H, W, ht, wt
        q.bits_lo, q.nbits, q.stats_cover_x, q.dtype, q.arith = 2, 7, 1, dtype, abi.ARITH_REFERENCE
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x32 = torch.zeros(B, C, H, W, device=DEV)
    x16 = x32.half()
    assert lib.mcaq_quant(ctypes.byref(scale(x32, abi.DTYPE_F32)), 1, stream) == ENOTSUP
    assert lib.mcaq_quant(ctypes.byref(scale(x16, abi.DTYPE_F16, stats_cover_x=0)), 1, stream) == ENOTSUP   # frozen stats
    assert lib.mcaq_quant(ctypes.byref(scale(x16, abi.DTYPE_F16, nbits=8)), 1, stream) == ENOTSUP          # 9-bit widths
    assert lib.mcaq_quant(ctypes.byref(scale(x16, abi.DTYPE_F16, ht=3, wt=3)), 1, stream) == ENOTSUP       # not tile aligned
    assert lib.mcaq_quant(ctypes.byref(scale(x16, abi.DTYPE_F16, arith=2)), 1, stream) != 0
    assert lib.mcaq_quant(ctypes.byref(scale(x16, abi.DTYPE_F16)), 1, stream) == 0
    torch.cuda.synchronize()
    # x = 0 in [-1, 1] at 4 bits, in fp16: s = r(2 / 15), zp = -0.5, rint(-0.5) = -0, y = r(0.5 * s)
    s = torch.tensor(2.0).half() / 15
    assert bool((y == float((torch.tensor(0.5).half() * s).float())).all())
    m = abi.MorphScale()
    m.B, m.H, m.W, m.Hc, m.Wc, m.tile, m.ht, m.wt = 1, 16, 16, 16, 16, 4, 4, 4
    m.smask_arith = 3
    assert lib.mcaq_morph(ctypes.byref(m), 1, stream) != 0


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_spatial_quantize_half_input_keeps_fp32_arithmetic(dt):
    """The drop-in op has no mode: fp32 arithmetic on the widened input."""
    from mcaq_yolo_amd import mcaq_cuda_ops
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 8, 16, 16, generator=g).to(DEV)
    bits = torch.randint(2, 9, (2, 4, 4), generator=g).float().to(DEV)
    xh = x.to(DTS[dt])
    mn, mx = xh.float().amin(dim=(0, 2, 3)), xh.float().amax(dim=(0, 2, 3))
    yh = mcaq_cuda_ops.spatial_quantize(xh, bits, mn, mx, 4, 4, None)
    y32 = mcaq_cuda_ops.spatial_quantize(xh.float(), bits, mn, mx, 4, 4, None)
    assert yh.dtype == DTS[dt] and torch.equal(yh, y32.to(DTS[dt]))
