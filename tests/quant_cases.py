"""Seeded cases for pass 2 at its own entry (mcaq_quant): each case is a list
of scales (the host data of one mcaq_quant_scale each) and, per scale, the
expected y.  With fp32 arithmetic the expectation is the oracle's quantize
(bit for bit), m(p) being the 5x5 Gaussian of the nearest-upsampled m(tile)
values or the given plane; with ARITH_REFERENCE it is the CPU statement
fallback.quantize_reference_half times the same fp32 plane.

The shapes are the smallest at which each branch of csrc/mcaq_quant.h can go
wrong; each case names the branch it is there for."""
import functools

import numpy as np
import torch

from mcaq_yolo_amd import abi
from oracle import mcaq_oracle as O

f32 = np.float32
HALF = {"f16": (torch.float16, abi.DTYPE_F16), "bf16": (torch.bfloat16, abi.DTYPE_BF16)}


def _x(shape, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 1.5).astype(f32)
    return np.where(x > 0, x, x * f32(0.1)).astype(f32)


def _bits(B, ht, wt, seed, lo=2, hi=8):
    return np.random.default_rng(seed).integers(lo, hi + 1, (B, ht, wt)).astype(f32)


def _mt(B, ht, wt, seed):
    return np.random.default_rng(seed).uniform(0.2, 1.0, (B, ht, wt)).astype(f32)


def m_plane(mt, H, W):
    """m(p) of LearnedSoftMask from its tile values: nearest upsample, 5x5 Gaussian, replicate pad."""
    up = mt[:, O.nearest_index(H, mt.shape[1])][:, :, O.nearest_index(W, mt.shape[2])]
    return O.conv2d(up, O.K["smooth5_softmask"], pad="replicate")


def scale(shape, tiles, seed, kind="none", widths=(2, 8), dtype="f32", arith=abi.ARITH_FP32, offset=0, neg_min=0,
          stats="own", poison=False):
    """One scale.  kind: none / mt (m(tile) values) / plane (a given m plane).
    stats: own (min / max of x, stats_cover_x = 1) or narrow (external, inside
    x's range, stats_cover_x = 0).  poison: a NaN in channel 1 and an infinity
    in channel 9.  offset: x starts this many elements into its buffer."""
    B, C, H, W = shape
    ht, wt = tiles
    x = _x(shape, seed)
    if poison:
        x[0, 1, 3, 3] = np.nan
        x[0, 9, 5, 5] = np.inf
    s = dict(B=B, C=C, H=H, W=W, ht=ht, wt=wt, bits_lo=widths[0], nbits=widths[1] - widths[0] + 1, dtype=dtype,
             arith=arith, offset=offset, neg_min=neg_min, stats_cover_x=1)
    if dtype != "f32":
        s["xh"] = torch.from_numpy(x).to(HALF[dtype][0])
        x = s["xh"].float().numpy()
    s["x"] = x
    s["bits"] = _bits(B, ht, wt, seed + 1, *widths)
    s["mt"] = _mt(B, ht, wt, seed + 2) if kind == "mt" else None
    s["m"] = m_plane(_mt(B, ht, wt, seed + 3), H, W) if kind == "plane" else None
    s["xmin"], s["xmax"] = x.min(axis=(0, 2, 3)), x.max(axis=(0, 2, 3))      # NaN-propagating, as amin / amax
    if stats == "narrow":
        s["xmin"], s["xmax"] = (s["xmin"] * f32(0.5)).astype(f32), (s["xmax"] * f32(0.5)).astype(f32)
        s["stats_cover_x"] = 0
    return s


def expected(s):
    m = s["m"] if s["m"] is not None else (m_plane(s["mt"], s["H"], s["W"]) if s["mt"] is not None else None)
    if s["arith"] == abi.ARITH_REFERENCE:
        from mcaq_yolo_amd import fallback
        y = fallback.quantize_reference_half(s["xh"], torch.from_numpy(s["bits"])).numpy()
        return y if m is None else (y * m[:, None]).astype(f32)
    return O.quantize(s["x"], s["bits"], m, s["xmin"], s["xmax"])


TILE_SHAPES = {
    "c40_16x16": ((2, 40, 16, 16), (2, 2)),   # two slices, the second of 8 channels: three waves return after the barriers
    "20x20": ((1, 8, 20, 20), (5, 5)),        # tiles 4 wide (the minimum); two chunks, the second partial
    "289tiles": ((1, 8, 68, 68), (17, 17)),   # m(tile) staging past the first 256 threads
}
FLAG_SHAPES = {"tile": ((1, 32, 16, 16), (4, 4)), "general": ((1, 32, 12, 12), (4, 4))}


def _builders():
    c = {}
    for name, (shape, tiles) in TILE_SHAPES.items():
        for kind in ("none", "mt"):
            c["tile_%s_%s" % (name, kind)] = lambda shape=shape, tiles=tiles, kind=kind: [scale(shape, tiles, 11, kind)]
    # the general kernel
    c["gen_12x12_vec"] = lambda: [scale((2, 8, 12, 12), (4, 4), 21)]                       # 16-byte rows, not tile-aligned
    c["gen_9x9_elem"] = lambda: [scale((2, 8, 9, 9), (2, 2), 22)]                          # HW % 4 != 0: element-wise
    c["gen_12x12_offset"] = lambda: [scale((2, 8, 12, 12), (4, 4), 23, offset=1)]          # unaligned base: element-wise
    c["gen_big_table"] = lambda: [scale((1, 32, 16, 16), (2, 2), 24, widths=(2, 10))]      # 288 table entries: kBig
    c["gen_big_tiles"] = lambda: [scale((1, 4, 50, 50), (17, 17), 25, "mt")]               # 289 staged tiles: kBig
    c["gen_mt_l2"] = lambda: [scale((1, 4, 132, 132), (33, 33), 26, "mt")]                 # 1089 tiles: read from L2
    c["gen_plane"] = lambda: [scale((2, 8, 12, 12), (4, 4), 27, "plane")]
    c["gen_plane_big"] = lambda: [scale((1, 32, 16, 16), (2, 2), 28, "plane", widths=(2, 10))]
    # several scales in one launch
    c["multi_tile"] = lambda: [scale((2, 40, 16, 16), (2, 2), 31, "mt"), scale((1, 8, 20, 20), (5, 5), 32, "mt"),
                               scale((1, 16, 32, 16), (4, 4), 33, "mt")]
    c["multi_general"] = lambda: [scale((2, 8, 12, 12), (4, 4), 34, "mt"), scale((1, 40, 20, 12), (3, 5), 35, "mt"),
                                  scale((1, 8, 16, 16), (2, 2), 36, "mt", widths=(2, 10))]
    c["multi_mixed"] = lambda: [scale((2, 8, 16, 16), (4, 4), 37, "mt"), scale((1, 40, 16, 16), (2, 2), 38)]
    # statistics flags
    for fam, (shape, tiles) in FLAG_SHAPES.items():
        c["%s_neg_min" % fam] = lambda shape=shape, tiles=tiles: [scale(shape, tiles, 41, "mt", neg_min=1)]
        c["%s_frozen_narrow" % fam] = lambda shape=shape, tiles=tiles: [scale(shape, tiles, 42, "mt", stats="narrow")]
        c["%s_nan_inf" % fam] = lambda shape=shape, tiles=tiles: [scale(shape, tiles, 43, "mt", poison=True)]
    # half maps: the fp32-arithmetic tile kernel and the reference-arithmetic one
    for dt in HALF:
        for name in ("c40_16x16", "20x20"):
            shape, tiles = TILE_SHAPES[name]
            for an, arith in (("fp32", abi.ARITH_FP32), ("ref", abi.ARITH_REFERENCE)):
                for kind in ("none", "mt"):
                    c["%s_%s_%s_%s" % (dt, an, name, kind)] = lambda shape=shape, tiles=tiles, kind=kind, dt=dt, arith=arith: [
                        scale(shape, tiles, 51, kind, dtype=dt, arith=arith)]
    return c


BUILDERS = _builders()
NAMES = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(scales, expected y of each scale); built once, read only."""
    scales = BUILDERS[name]()
    return scales, [expected(s) for s in scales]
