"""Percentile calibration on the GPU: mcaq_percentile (csrc/mcaq_pct.h) on every
case of tests/percentile_cases.py against torch.quantile on the CPU, the
module and the hooks against the reference's own runs (tests/golden/
pct_*.npz) and the pure-PyTorch CPU path, HIP-graph capture and run-to-run
identity.  lo / hi compare with NaN == NaN and -0 == +0 (percentile_cases.
same); everything else bit for bit unless a tolerance is named."""
import numpy as np
import pytest
import torch

from conftest import load_case, load_weights
from mcaq_yolo_amd import fallback

import percentile_cases as PC
from test_percentile_cpu import INFER, TRAIN, load, quantizer, train_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
HOOK_CASES = ["p3_c16", "odd_c20", "g16_c16"]


def N(t):
    return t.detach().cpu().numpy()


def upload(case):
    """The case's map on the device, contiguous, its base `offset` elements
    past a 16-byte boundary."""
    x = case.x
    buf = torch.empty(x.numel() + case.offset, dtype=x.dtype, device=DEV)
    v = buf[case.offset:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == (case.offset * x.element_size()) % 16
    return v


def native(case):
    from mcaq_yolo_amd import core
    lo, hi = core.channel_percentiles(upload(case), PC.Q_LO, PC.Q_HI, per_channel=not case.per_tensor)
    torch.cuda.synchronize()
    return N(lo), N(hi)


@pytest.mark.parametrize("name", PC.names())
def test_native_percentiles_equal_torch_quantile(name):
    """Every channel of every case."""
    c = PC.case(name)
    lo, hi = native(c)
    elo, ehi = PC.expected(c)
    print(name, "lo", lo, "expected", elo, "hi", hi, "expected", ehi)
    assert PC.same(lo, elo) and PC.same(hi, ehi)


def test_nan_channel_gives_nan_for_both():
    lo, hi = native(PC.case("nonfinite"))
    assert np.isnan(lo[1]) and np.isnan(hi[1])
    assert np.isfinite(lo[3]) and np.isfinite(hi[3])


def test_two_scales_in_one_call_equal_two_calls():
    from mcaq_yolo_amd import abi, core
    L = abi.lib()
    cs = [PC.case("odd"), PC.case("half_ref_shape_bf16")]
    xs = [upload(c) for c in cs]
    single = [core.channel_percentiles(x, PC.Q_LO, PC.Q_HI) for x in xs]
    s = (abi.PercentileScale * 2)()
    outs = []
    for i, x in enumerate(xs):
        B, C, H, W = x.shape
        lo, hi = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        outs.append((lo, hi))
        s[i].x, s[i].lo, s[i].hi = core._p(x), core._p(lo), core._p(hi)
        s[i].B, s[i].C, s[i].H, s[i].W = B, C, H, W
        s[i].dtype = core._ABI_DTYPES[x.dtype]
        s[i].q_lo, s[i].q_hi = PC.Q_LO, PC.Q_HI
    nb = L.mcaq_percentile_workspace_bytes(sum(x.shape[1] for x in xs))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    assert L.mcaq_percentile(s, 2, core._p(ws), nb - 1, core._stream()) != 0      # short for two scales
    abi.check(L.mcaq_percentile(s, 2, core._p(ws), nb, core._stream()), "mcaq_percentile")
    torch.cuda.synchronize()
    for (lo, hi), (slo, shi) in zip(outs, single):
        assert torch.equal(lo, slo) and torch.equal(hi, shi)


def test_run_twice_bit_identical():
    for name in ("sampled", "ties", "half_odd_f16"):
        a, b = native(PC.case(name)), native(PC.case(name))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("name", INFER)
def test_module_inference_equals_reference(name):
    d = load(name)
    q = quantizer(d, DEV).eval()
    x = torch.from_numpy(d["x"]).to(DEV)
    lo, hi = q.batch_percentiles(x)
    C = x.shape[1]
    assert np.array_equal(N(lo), np.broadcast_to(d["lo"], (C,))) and np.array_equal(N(hi), np.broadcast_to(d["hi"], (C,)))
    with torch.no_grad():
        y = q(x, torch.from_numpy(d["bits"]).to(DEV))
    assert y.dtype == torch.float32 and np.array_equal(N(y), d["y"])
    # frozen statistics are not read in this mode
    n = d["lo"].size
    shape = (1, -1, 1, 1) if bool(d["per_channel"]) else ()
    q.running_min = torch.full((n,), -0.5, device=DEV).reshape(shape)
    q.running_max = torch.full((n,), 0.25, device=DEV).reshape(shape)
    q.freeze_calibration()
    with torch.no_grad():
        assert np.array_equal(N(q(x, torch.from_numpy(d["bits"]).to(DEV))), d["y"])


@pytest.mark.parametrize("name", TRAIN)
def test_module_train_equals_reference(name):
    """y, grad x and the running buffers bit for bit; the gradient to the bit
    map within 1e-4 of its largest magnitude, the bound of the minmax-mode QAT
    tests (tests/test_qat_gpu.py) - and bit for bit in the test below."""
    d = load(name)
    q, x, b, y = train_step(d, DEV)
    assert np.array_equal(N(y), d["y"])
    assert np.array_equal(N(x.grad), d["gx"])
    assert np.array_equal(N(q.running_min).reshape(-1), d["rmin"])
    assert np.array_equal(N(q.running_max).reshape(-1), d["rmax"])
    assert int(q.num_batches_tracked) == int(d["nbt"])
    ref = d["gbits"].astype(np.float64)
    assert np.abs(N(b.grad).astype(np.float64) - ref).max() <= 1e-4 * np.abs(ref).max()


@pytest.mark.parametrize("name", TRAIN)
def test_module_train_bit_gradient_equals_reference(name):
    """The gradient to the bit map, bit for bit: in this mode the module's
    backward sums it in the reference's order (mcaq_qat_bits_gradient)."""
    d = load(name)
    _, _, b, _ = train_step(d, DEV)
    got, ref = N(b.grad), d["gbits"]
    print("gbits max |diff| %g of max |ref| %g, %d of %d entries differ"
          % (np.abs(got - ref).max(), np.abs(ref).max(), int((got != ref).sum()), ref.size))
    assert np.array_equal(got, ref)


# (B, C, H, W, ht, wt, with m): C above one and above several 16-row cascade
# blocks, C not a multiple of 4 (leftover rows of the tail columns), H W not
# a multiple of 32 (tail columns), tiles that do not divide the map, one tile
@pytest.mark.parametrize("shape", [(2, 40, 19, 17, 3, 4, True), (1, 33, 20, 20, 5, 5, False),
                                   (2, 70, 13, 17, 2, 3, True), (1, 3, 8, 8, 1, 1, False),
                                   (1, 300, 6, 7, 2, 2, False), (2, 16, 40, 40, 10, 10, True)])
def test_bit_gradient_in_reference_order_equals_the_cpu_autograd_graph(shape):
    """mcaq_qat_bits_gradient against the reference's autograd graph restated
    on the CPU (fallback.fractional_quant_graph, which the fixtures pin to the
    reference bit for bit): the same gradient to the bit map, bit for bit,
    with and without a mask plane."""
    from mcaq_yolo_amd import core
    B, C, H, W, ht, wt, with_m = shape
    gen = torch.Generator().manual_seed(sum(shape[:6]))
    x = torch.randn(B, C, H, W, generator=gen) * 1.5
    g = torch.randn(B, C, H, W, generator=gen)
    bits = 2.0 + 6.0 * torch.rand(B, ht, wt, generator=gen)
    if bits.numel() > 3:             # exact integers among the tiles, both ends (a lone tile stays fractional)
        bits.view(-1)[0], bits.view(-1)[1], bits.view(-1)[2] = 8.0, 2.0, 5.0
    m = (0.5 + 0.5 * torch.rand(B, 1, H, W, generator=gen)) if with_m else None
    lo, hi = PC.expected(PC.Case("s", x, False, 0))
    lo, hi = torch.from_numpy(lo), torch.from_numpy(hi)
    bt = bits.clone().requires_grad_(True)
    y = fallback.fractional_quant_graph(x, bt, lo, hi)
    if with_m:
        y = y * m
    y.backward(g)
    got = core.qat_bits_gradient_reference_order(g.to(DEV), x.to(DEV), bits.to(DEV),
                                                 None if m is None else m[:, 0].contiguous().to(DEV),
                                                 lo.to(DEV), hi.to(DEV))
    assert float(bt.grad.abs().max()) > 0
    assert np.array_equal(N(got), bt.grad.numpy())


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", ["pct_p4_smooth", "pct_rect_tensor"])
def test_half_map_equals_fp32_path_on_widened_values(name, dt):
    d = load(name)
    bits = torch.from_numpy(d["bits"]).to(DEV)
    xh = torch.from_numpy(d["x"]).to(dt).to(DEV)
    q = quantizer(d, DEV).eval()
    with torch.no_grad():
        yh = q(xh, bits)
        yf = q(xh.float(), bits)
    assert yh.dtype == torch.float32 and torch.equal(yh, yf)
    lo_h, hi_h = q.batch_percentiles(xh)
    lo_f, hi_f = q.batch_percentiles(xh.float())
    assert torch.equal(lo_h, lo_f) and torch.equal(hi_h, hi_f)
    q.train()
    xt = xh.clone().requires_grad_(True)
    xf = xh.float().requires_grad_(True)
    cont = bits + 0.25
    g = torch.randn(xh.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    yt = q(xt, cont.clamp(max=8.0), training=True)
    yt.backward(g)
    yr = q(xf, cont.clamp(max=8.0), training=True)
    yr.backward(g)
    assert yt.dtype == torch.float32 and torch.equal(yt, yr)
    assert xt.grad.dtype == dt and torch.equal(xt.grad, xf.grad.to(dt))


def _hooks(mode, grid, dev, **kw):
    from mcaq_yolo_amd.hooks import MCAQHooks
    W = load_weights()
    h = MCAQHooks(grid_size=grid, device=dev, indices=(4,), calibration_mode=mode, **kw)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in W.items()
          if k.startswith(("complexity_analyzer.", "bit_mapper."))}
    sd.update({"quantizers.4." + k: torch.from_numpy(np.asarray(v)) for k, v in W.items()
               if k.startswith("soft_mask.")})
    h.load_state_dict(sd, strict=False)
    return h.to(dev)


@pytest.mark.parametrize("name", HOOK_CASES)
def test_hooks_eval(name):
    """bits and complexity equal the minmax hooks' (the analysis does not
    depend on the mode); y equals fallback.quantize with the CPU quantiles
    times the soft mask of the CPU path, bit for bit."""
    d = load_case(name)
    grid = int(d["grid"])
    x = torch.from_numpy(d["x"].astype(f32))
    hp, hm = _hooks("percentile", grid, DEV).eval(), _hooks("minmax", grid, DEV).eval()
    with torch.no_grad():
        outs, aux = hp.forward_features([x.to(DEV)])
        outs_m, aux_m = hm.forward_features([x.to(DEV)])
    assert torch.equal(aux[0]["bit_map"], aux_m[0]["bit_map"])
    assert torch.equal(aux[0]["complexity"], aux_m[0]["complexity"])
    assert not torch.equal(outs[0], outs_m[0])
    lo, hi = PC.expected(PC.Case(name, x, False, 0))
    bits = aux[0]["bit_map"].cpu()
    hc = _hooks("percentile", grid, "cpu").eval()
    with torch.no_grad():
        ref = fallback.quantize(x, bits, torch.from_numpy(lo), torch.from_numpy(hi)).contiguous()
        ref = ref * hc.quantizers["4"].soft_mask(bits, x)
    assert outs[0].dtype == torch.float32 and torch.equal(outs[0].cpu(), ref)
    # calibrating: the running statistics are still the batch min / max EMA
    with torch.no_grad():
        hp.begin(calibrating=True)
        y = hp.run_scale(4, x.to(DEV), hp._mcaq_state)
        hp.end()
    q = hp.quantizers["4"]
    assert torch.equal(y, outs[0]) and int(q.num_batches_tracked) == 1
    assert np.array_equal(N(q.running_min).reshape(-1), x.amin(dim=(0, 2, 3)).numpy())
    assert np.array_equal(N(q.running_max).reshape(-1), x.amax(dim=(0, 2, 3)).numpy())


@pytest.mark.parametrize("name", HOOK_CASES)
def test_hooks_train_takes_the_per_scale_path_and_matches_cpu(name, monkeypatch):
    """Train mode through forward_features: never the fused multi-scale step
    and not the concurrent streams; the continuous bit map is the minmax
    hooks' bit for bit (the analysis does not depend on the mode).

    Against the pure-PyTorch CPU path.  Gradients: the tolerances of
    tests/test_train_fused_gpu.py (1e-3 of the largest magnitude; fp32 sums
    in other orders than ATen's).  y: the CPU and GPU analyzers / mappers give
    bit maps db apart (train-mode BatchNorm over as few as 50 tiles; the same
    code and the same db in minmax mode), and y is continuous and piecewise
    linear in the bits with slope |Q_hi - Q_lo| m <= one 2-bit step
    (hi - lo) / 3 times m, so |dy| <= db max_c(hi - lo) / 3 max m, plus 1e-5
    of max |y| for the fp32 arithmetic itself."""
    from mcaq_yolo_amd import train_step as ts
    from test_train_fused_gpu import _cmp_grads, _rel
    d = load_case(name)
    grid = int(d["grid"])
    x = torch.from_numpy(d["x"].astype(f32))
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(4)) * 1e-3

    def boom(*a, **k):
        raise AssertionError("the fused multi-scale step ran in percentile mode")
    two = _hooks("percentile", grid, DEV).train()
    two.backbone_out_indices = [4, 4]
    assert not ts.multi_ok(two, [x.to(DEV), x.to(DEV)]) and not two._concurrent_ok([x.to(DEV), x.to(DEV)])
    monkeypatch.setattr(ts, "forward_features", boom)
    res = {}
    for key, mode, dev in (("cpu", "percentile", "cpu"), ("gpu", "percentile", DEV), ("minmax", "minmax", DEV)):
        h = _hooks(mode, grid, dev).train()
        xt = x.clone().to(dev).requires_grad_(True)
        outs, aux = h.forward_features([xt])
        loss = (outs[0] * g.to(dev)).sum() + 0.1 * (aux[0]["bit_map"].mean() - 4.0) ** 2
        loss.backward()
        res[key] = (outs[0].detach().cpu(), aux[0]["bit_map"].detach().cpu(), xt.grad.detach().cpu(),
                    {k: p.grad.detach().cpu() for k, p in h.named_parameters() if p.grad is not None},
                    h.quantizers["4"])
    yc, bc, gxc, gc, qc = res["cpu"]
    yg, bg, gxg, gg, qg = res["gpu"]
    assert torch.equal(bg, res["minmax"][1]) and not torch.equal(yg, res["minmax"][0])
    lo, hi = PC.expected(PC.Case(name, x, False, 0))
    with torch.no_grad():
        m = qc.soft_mask(bc, x)
    db = float((bg - bc).abs().max())
    bound = db * float((hi - lo).max()) / 3.0 * float(m.abs().max()) + 1e-5 * float(yc.abs().max())
    err = float((yg - yc).abs().max())
    print("db %g  |dy| %g  bound %g" % (db, err, bound))
    assert err <= bound
    _rel(gxg, gxc, 1e-3)
    _cmp_grads(gg, gc)
    assert torch.equal(qg.running_min.cpu(), qc.running_min) and torch.equal(qg.running_max.cpu(), qc.running_max)
    assert int(qg.num_batches_tracked) == int(qc.num_batches_tracked) == 1


def test_hooks_eval_graph_replay_equals_eager():
    """The eval hook step captured into one HIP graph (the process keeps its
    default queue settings) and replayed on two other inputs copied into the
    static buffer equals the eager step."""
    d = load_case("odd_c20")
    h = _hooks("percentile", int(d["grid"]), DEV).eval()
    gen = torch.Generator().manual_seed(9)
    x0 = torch.from_numpy(d["x"].astype(f32))
    inputs = [x0, torch.nn.functional.silu(2 * torch.randn(x0.shape, generator=gen)), x0.flip(0) * 1.5 - 0.25]
    static = x0.to(DEV).clone()

    def step():
        outs, aux = h.forward_features([static])
        return outs[0], aux[0]["bit_map"]
    with torch.no_grad():
        eager = []
        for x in inputs:
            static.copy_(x.to(DEV))
            eager.append([t.clone() for t in step()])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        static.copy_(inputs[0].to(DEV))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step()
        for x, ref in zip(inputs[1:] + inputs[:1], eager[1:] + eager[:1]):
            static.copy_(x.to(DEV))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(outs[0], ref[0]) and torch.equal(outs[1], ref[1])
    assert len({o[0].sum().item() for o in eager}) == 3
