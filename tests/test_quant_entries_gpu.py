"""Pass 2 at its own entry: every case of tests/quant_cases.py through
abi.lib().mcaq_quant directly, y equal to the expectation bit for bit (NaNs
equal NaNs), and the > 256 MB launch (nontemporal loads of x) against the same
data run as two half-batch launches."""
import ctypes

import numpy as np
import pytest
import torch

import quant_cases as Q
from mcaq_yolo_amd import abi

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def launch(scales):
    """One mcaq_quant launch of the scales' host data -> (error code, [y of each scale])."""
    qs = (abi.QuantScale * len(scales))()
    keep, ys = [], []
    for q, s in zip(qs, scales):
        src = s["xh"] if s["dtype"] != "f32" else torch.from_numpy(s["x"])
        n, off = src.numel(), s["offset"]
        buf = torch.zeros(n + 4, dtype=src.dtype, device=DEV)     # offset: a contiguous view that starts off a 16-byte boundary
        buf[off:off + n] = src.reshape(-1).to(DEV)
        x = buf[off:off + n]
        assert x.data_ptr() % 16 == (off * src.element_size()) % 16
        y = torch.full(src.shape, float("nan"), device=DEV)
        t = dict(x=x, y=y, bits=_dev(s["bits"]), xmin=_dev(-s["xmin"] if s["neg_min"] else s["xmin"]), xmax=_dev(s["xmax"]))
        for k in ("mt", "m"):
            if s[k] is not None:
                t[k] = _dev(s[k])
        for k, v in t.items():
            setattr(q, k, _ptr(v))
        for k in ("B", "C", "H", "W", "ht", "wt", "bits_lo", "nbits", "neg_min", "stats_cover_x", "arith"):
            setattr(q, k, s[k])
        q.dtype, q.ydtype = (Q.HALF[s["dtype"]][1] if s["dtype"] != "f32" else abi.DTYPE_F32), abi.DTYPE_F32
        keep.append(t)
        ys.append(y)
    err = abi.lib().mcaq_quant(qs, len(scales), _stream())
    torch.cuda.synchronize()
    return err, [y.cpu().numpy() for y in ys]


def _eq(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True), "%s: %d of %d elements differ" % (
        what, int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()), got.size)


@pytest.mark.parametrize("name", Q.NAMES)
def test_quant_entry_case(name):
    scales, want = Q.case(name)
    err, got = launch(scales)
    assert err == 0
    for i, (g, w) in enumerate(zip(got, want)):
        _eq(g, w, "%s scale %d" % (name, i))


def test_cases_reach_their_branches():
    """The inputs do what their names say: the poisoned channels make their
    rows NaN and leave the others finite, narrow statistics clamp, and the
    soft-mask cases differ from their unmasked y."""
    for fam in Q.FLAG_SHAPES:
        y = Q.case(fam + "_nan_inf")[1][0]
        bad = np.isnan(y).all(axis=(0, 2, 3))
        assert bad[1] and bad[9] and not bad[[0, 2, 8, 10, 16, 31]].any()
        s, (y,) = Q.case(fam + "_frozen_narrow")
        assert float(y.max()) < float(s[0]["x"].max()) * 0.75
    s, (y,) = Q.case("tile_20x20_mt")
    assert not np.array_equal(y, Q.case("tile_20x20_none")[1][0])


def test_mixed_kinds_equal_single_launches():
    """A launch whose scales differ in their m(p) source runs one launch per
    scale: the same y as launching each scale alone."""
    scales, _ = Q.case("multi_mixed")
    err, got = launch(scales)
    assert err == 0
    for i, s in enumerate(scales):
        e1, (y1,) = launch([s])
        assert e1 == 0
        _eq(got[i], y1, "scale %d" % i)


def test_mixed_kinds_stop_at_the_first_failing_scale():
    """Mixed kinds with a half map the tile family does not take in second
    place: the first scale has launched (its y is written), the second is
    refused with hipErrorNotSupported, the third never runs."""
    a = Q.scale((1, 8, 16, 16), (4, 4), 61, "mt", dtype="f16")
    b = Q.scale((1, 8, 12, 12), (4, 4), 62, dtype="f16")      # 12 is no power-of-two multiple of 4
    c = Q.scale((1, 8, 16, 16), (4, 4), 63, dtype="f16")
    err, (ya, yb, yc) = launch([a, b, c])
    assert err == 801
    _eq(ya, Q.expected(a), "scale 0")
    assert np.isnan(yb).all() and np.isnan(yc).all()


def test_above_256mb_equals_two_half_batch_launches():
    """B 66, C 64, 128 x 128 fp32 is 264 MiB of x: the launch loads x
    nontemporally; each half batch stays under the threshold.  Same data, same
    statistics: the same y, bit for bit."""
    B, C, H, W, ht, wt = 66, 64, 128, 128, 16, 16
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(B, C, H, W, device=DEV, generator=g)
    assert x.numel() * 4 > 256 << 20 > x.numel() * 2
    bits = torch.randint(2, 9, (B, ht, wt), device=DEV, generator=g).float()
    mt = torch.rand(B, ht, wt, device=DEV, generator=g)
    xmin, xmax = x.amin(dim=(0, 2, 3)), x.amax(dim=(0, 2, 3))
    y1, y2 = torch.empty_like(x), torch.empty_like(x)

    def run(y, b0, nb):
        q = abi.QuantScale()
        q.x, q.y, q.bits, q.mt = _ptr(x[b0:]), _ptr(y[b0:]), _ptr(bits[b0:]), _ptr(mt[b0:])
        q.xmin, q.xmax = _ptr(xmin), _ptr(xmax)
        q.B, q.C, q.H, q.W, q.ht, q.wt = nb, C, H, W, ht, wt
        q.bits_lo, q.nbits, q.stats_cover_x, q.dtype, q.ydtype = 2, 7, 1, abi.DTYPE_F32, abi.DTYPE_F32
        assert abi.lib().mcaq_quant(ctypes.byref(q), 1, _stream()) == 0

    run(y1, 0, B)
    run(y2, 0, B // 2)
    run(y2, B // 2, B // 2)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
    assert bool(torch.isfinite(y1).all()) and float(y1.abs().max()) > 0
