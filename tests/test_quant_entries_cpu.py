"""Argument refusals of mcaq_quant (csrc/mcaq_quant.h: quant_args, then the
plan's "not supported").  Every refusal happens before any launch, so no GPU
is needed and no pointer is dereferenced (0x1000 stands for every device
pointer; no call here has valid arguments).  Each case starts from a
descriptor the entry would accept, breaks one field, at scale 0 and at the
last of three scales, and checks the exact code."""
import ctypes
import os

import pytest

from mcaq_yolo_amd import abi

INVALID = 1          # hipErrorInvalidValue
NOTSUP = 801         # hipErrorNotSupported
FAKE = 0x1000        # 16-byte aligned; never dereferenced: every call below is refused first
F32, F16, BF16, REF = abi.DTYPE_F32, abi.DTYPE_F16, abi.DTYPE_BF16, abi.ARITH_REFERENCE


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(abi.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return abi._declare(ctypes.CDLL(abi.LIB_PATH))


def _scales(n, base, broken=None, at=0):
    """n acceptable scales (fields `base` over the fp32 default), `broken` applied to scale `at`."""
    qs = (abi.QuantScale * n)()
    for i, q in enumerate(qs):
        for f in ("x", "y", "bits", "xmin", "xmax"):
            setattr(q, f, FAKE)
        q.B, q.C, q.H, q.W, q.ht, q.wt = 1, 4, 16, 16, 4, 4
        q.bits_lo, q.nbits, q.stats_cover_x, q.dtype, q.ydtype, q.arith = 2, 7, 1, F32, F32, abi.ARITH_FP32
        for f, v in dict(base, **(broken if i == at and broken else {})).items():
            setattr(q, f, v)
    return qs


def _refused(lib, code, broken, base=None):
    """`broken` at scale 0 of one, at scale 0 of three and at the last of three."""
    base = base or {}
    for n, at in ((1, 0), (3, 0), (3, 2)):
        assert lib.mcaq_quant(_scales(n, base, broken, at), n, None) == code, (broken, n, at)


def test_scale_count_refusals(lib):
    assert lib.mcaq_quant(_scales(1, {}), 0, None) == INVALID
    assert lib.mcaq_quant(_scales(1, {}), -1, None) == INVALID
    n = abi.MAX_SEGMENTS + 1
    assert lib.mcaq_quant(_scales(n, {}), n, None) == INVALID


@pytest.mark.parametrize("broken", [
    {"nbits": 0}, {"nbits": 16}, {"bits_lo": 0}, {"bits_lo": 3, "nbits": 15},      # top width 17
    {"H": 0}, {"C": 0}, {"ht": 0}, {"wt": 0},
    {"x": None}, {"y": None}, {"bits": None}, {"xmin": None}, {"xmax": None},
    {"dtype": -1}, {"dtype": 3}, {"dtype": F16},                                     # the last: differs between scales
    {"ydtype": F16}, {"arith": -1}, {"arith": 2}], ids=str)
def test_invalid_value_refusals(lib, broken):
    if broken == {"dtype": F16}:      # alone it is a valid half map: only among fp32 scales
        for at in (0, 2):
            assert lib.mcaq_quant(_scales(3, {}, broken, at), 3, None) == INVALID
        return
    _refused(lib, INVALID, broken)


def test_not_supported_refusals(lib):
    half = {"dtype": F16}
    ref = {"dtype": BF16, "arith": REF}
    # one arithmetic per launch
    for at in (0, 2):
        assert lib.mcaq_quant(_scales(3, half, {"arith": REF}, at), 3, None) == NOTSUP
    # reference arithmetic: a half map with its own batch statistics, no plane, widths <= 8
    for n in (1, 3):
        assert lib.mcaq_quant(_scales(n, {"arith": REF}), n, None) == NOTSUP             # fp32 map
    _refused(lib, NOTSUP, {"stats_cover_x": 0}, ref)
    _refused(lib, NOTSUP, {"m": FAKE}, ref)
    _refused(lib, NOTSUP, {"nbits": 8}, ref)                                             # 9-bit widths
    # a half map outside the tile-aligned family, in either arithmetic
    for base in (half, ref):
        _refused(lib, NOTSUP, {"ht": 3, "wt": 3}, base)            # 16 is no power-of-two multiple of 3
        _refused(lib, NOTSUP, {"W": 8, "wt": 4}, base)             # tiles 2 pixels wide
        _refused(lib, NOTSUP, {"x": FAKE + 2}, base)               # base not 16-byte aligned
    _refused(lib, NOTSUP, {"nbits": 9, "bits_lo": 1}, half)        # 9 widths
    for n in (1, 3):                                               # a plane (on every scale: one m(p) source,
        assert lib.mcaq_quant(_scales(n, dict(half, m=FAKE)), n, None) == NOTSUP   # so nothing launches per scale)
    # a scale's invalid value comes before its unsupported arithmetic
    assert lib.mcaq_quant(_scales(3, half, {"arith": REF, "nbits": 0}, 2), 3, None) == INVALID
