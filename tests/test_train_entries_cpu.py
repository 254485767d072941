"""Argument refusals of the train-mode C entries (csrc/mcaq_train.h): the
eight single-scale entries and the multi-segment entries they share their
launcher layer with.  Every refusal happens before any launch, so no GPU is
needed and no pointer is dereferenced (0x1000 stands for every device pointer;
no call here has valid arguments).  Each case starts from an argument set the
entry would accept and breaks one thing; the entry must answer
hipErrorInvalidValue."""
import ctypes
import os

import pytest

from mcaq_yolo_amd import abi

INVALID = 1          # hipErrorInvalidValue
FAKE = 0x1000        # never dereferenced: every call below is refused first


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(abi.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return abi._declare(ctypes.CDLL(abi.LIB_PATH))


def _refusals(call, base, cases):
    """call(**args) with `base` changed by each case in turn -> all refused."""
    for case in cases:
        args = dict(base)
        args.update(case)
        assert call(**args) == INVALID, case


def _nulls(*names):
    return [{n: None} for n in names]


def _segs(cls, ptrs, ints, nseg, over, kw):
    """max(nseg, 1) acceptable segments; over / kw = {field: value} (segment 0) or {(k, field): value}."""
    segs = (cls * max(nseg, 1))()
    for s in segs:
        for f in ptrs:
            setattr(s, f, FAKE)
        for f, v in ints.items():
            setattr(s, f, v)
    for key, v in dict(over or {}, **kw).items():
        k, f = key if isinstance(key, tuple) else (0, key)
        setattr(segs[k], f, v)
    return segs


def _mseg(nseg=1, over=None, **kw):
    return _segs(abi.MapperSeg, ("c", "bits", "work", "gbits", "gc", "gpart"), {"n": 130}, nseg, over, kw)


def _hseg(nseg=1, over=None, **kw):
    return _segs(abi.HeadSeg, ("phi", "craw", "gC", "gcraw", "gpart"), {"B": 2, "ht": 5, "wt": 7}, nseg, over, kw)


def _sseg(nseg=1, over=None, **kw):
    return _segs(abi.SmaskSeg, ("bits", "absmean", "gm", "gbits", "gpart"),
                 {"B": 2, "H": 44, "W": 52, "ht": 11, "wt": 13}, nseg, over, kw)


def _rseg(nseg=1, over=None, **kw):
    return _segs(abi.ReduceSeg, ("part", "out"), {"nparts": 3, "stride": 170, "count": 170}, nseg, over, kw)


def _seg_cases(make, fields, nseg_arg="nseg", segs_arg="segs"):
    """One broken field of segment 0 and of the last of three segments."""
    out = []
    for f, v in fields:
        out.append({segs_arg: make(1, **{f: v})})
        out.append({segs_arg: make(3, {(2, f): v}), nseg_arg: 3})
    return out


MP = ctypes.byref(abi.MapperParams())
CP = ctypes.byref(abi.CmlpParams())
SP = ctypes.byref(abi.SmaskParams())
MAPPER_FWD_SEG = [("c", None), ("bits", None), ("work", None), ("n", 0)]
MAPPER_BWD_SEG = [("c", None), ("gbits", None), ("gc", None), ("gpart", None), ("work", None), ("n", 0)]
HEAD_SEG = [("phi", None), ("craw", None), ("gC", None), ("gcraw", None), ("gpart", None), ("B", 0), ("ht", 0),
            ("wt", 0)]
SMASK_SEG = [("bits", None), ("absmean", None), ("gm", None), ("gbits", None), ("gpart", None), ("B", 0), ("ht", 0),
             ("wt", 0), ("H", 10), ("W", 12)]
REDUCE_SEG = [("part", None), ("nparts", 0), ("stride", 169), ("count", 0)]


# ---- the single-scale entries ----------------------------------------------
def test_mapper_train_forward_refusals(lib):
    def call(P, c, n, bits, work):
        return lib.mcaq_mapper_train_forward(P, c, n, 2.0, 8.0, 1.0, 0.1, 1, 1, bits, work, None)
    base = dict(P=MP, c=FAKE, n=130, bits=FAKE, work=FAKE)
    _refusals(call, base, _nulls("P", "c", "bits", "work") + [{"n": 0}, {"n": -3}])


def test_mapper_train_backward_refusals(lib):
    def call(P, c, n, gbits, work, gc, gparams, gpart):
        return lib.mcaq_mapper_train_backward(P, c, n, gbits, 2.0, 8.0, 1.0, work, gc, gparams, gpart, 0, None)
    base = dict(P=MP, c=FAKE, n=130, gbits=FAKE, work=FAKE, gc=FAKE, gparams=FAKE, gpart=FAKE)
    _refusals(call, base, _nulls("P", "c", "gbits", "work", "gc", "gpart") + [{"n": 0}])


def test_mapper_train_forward_stage_refusals(lib):
    def call(P, c, n, bits, work, stage, gathered, world):
        return lib.mcaq_mapper_train_forward_stage(P, c, n, 2.0, 8.0, 1.0, 0.1, 1, 1, bits, work, stage, gathered,
                                                   world, None)
    base = dict(P=MP, c=FAKE, n=130, bits=FAKE, work=FAKE, stage=2, gathered=FAKE, world=2)
    _refusals(call, base, _nulls("P", "c", "bits", "work", "gathered") + [
        {"n": 0}, {"stage": 0}, {"stage": 5}, {"world": 0}, {"stage": 1, "world": 0},
        {"stage": 3, "gathered": None}, {"stage": 4, "gathered": None}])


def test_mapper_train_backward_stage_refusals(lib):
    def call(P, c, n, gbits, work, gc, gpart, stage, gsums, gathered1, world):
        return lib.mcaq_mapper_train_backward_stage(P, c, n, gbits, 2.0, 8.0, 1.0, work, gc, gpart, stage, gsums,
                                                    gathered1, world, None)
    base = dict(P=MP, c=FAKE, n=130, gbits=FAKE, work=FAKE, gc=FAKE, gpart=FAKE, stage=3, gsums=FAKE, gathered1=FAKE,
                world=2)
    _refusals(call, base, _nulls("P", "c", "gbits", "work", "gc", "gpart", "gsums", "gathered1") + [
        {"n": 0}, {"stage": 0}, {"stage": 5}, {"world": 0}, {"stage": 4, "world": 0},
        {"stage": 1, "gsums": None}, {"stage": 2, "gathered1": None}])


@pytest.mark.parametrize("entry", ["mcaq_mapper_train_grad_reduce", "mcaq_head_train_grad_reduce"])
def test_grad_reduce_refusals(lib, entry):
    def call(n, gpart, gparams):
        return getattr(lib, entry)(n, gpart, gparams, 0, None)
    _refusals(call, dict(n=130, gpart=FAKE, gparams=FAKE), _nulls("gpart", "gparams") + [{"n": 0}, {"n": -1}])


def test_head_train_backward_refusals(lib):
    def call(P, phi, craw, gC, B, ht, wt, gcraw, gparams, gpart):
        return lib.mcaq_head_train_backward(P, phi, craw, gC, B, ht, wt, gcraw, gparams, gpart, 0, None)
    base = dict(P=CP, phi=FAKE, craw=FAKE, gC=FAKE, B=2, ht=5, wt=7, gcraw=FAKE, gparams=FAKE, gpart=FAKE)
    _refusals(call, base, _nulls("P", "phi", "craw", "gC", "gcraw", "gpart") + [
        {"B": 0}, {"ht": 0}, {"wt": 0},
        {"ht": 28, "wt": 28}])           # 53 x 784 floats of LDS per image > 160 KiB - 1 KiB


def test_smask_train_backward_refusals(lib):
    def call(P, bits, absmean, gm, B, H, W, ht, wt, gbits, gparams, gpart):
        return lib.mcaq_smask_train_backward(P, bits, absmean, gm, B, H, W, ht, wt, gbits, 0, gparams, gpart, None)
    base = dict(P=SP, bits=FAKE, absmean=FAKE, gm=FAKE, B=2, H=44, W=52, ht=11, wt=13, gbits=FAKE, gparams=FAKE,
                gpart=FAKE)
    _refusals(call, base, _nulls("P", "bits", "absmean", "gm", "gbits", "gparams", "gpart") + [
        {"B": 0}, {"ht": 0}, {"wt": 0}, {"H": 10}, {"W": 12},
        {"H": 400, "W": 400}])           # one image's planes above the LDS bound


# ---- the multi-segment entries ---------------------------------------------
def test_mapper_train_forward_multi_refusals(lib):
    def call(P, segs, nseg, upd):
        return lib.mcaq_mapper_train_forward_multi(P, segs, nseg, 2.0, 8.0, 1.0, 0.1, 1, upd, None)
    base = dict(P=MP, segs=_mseg(1), nseg=1, upd=2)
    _refusals(call, base, _nulls("P", "segs") + [
        {"nseg": 0}, {"segs": _mseg(4), "nseg": 4},
        {"segs": _mseg(2), "nseg": 2, "upd": 1}] +            # two segments would race on the running statistics
        _seg_cases(_mseg, MAPPER_FWD_SEG))


def test_mapper_train_backward_multi_ride_refusals(lib):
    def call(P, segs, nseg, rsegs, nr):
        return lib.mcaq_mapper_train_backward_multi_ride(P, segs, nseg, 2.0, 8.0, 1.0, rsegs, nr, None)
    base = dict(P=MP, segs=_mseg(1), nseg=1, rsegs=_rseg(1), nr=1)
    _refusals(call, base, _nulls("P", "segs", "rsegs") + [
        {"nseg": 0}, {"segs": _mseg(4), "nseg": 4}, {"nr": -1}, {"rsegs": _rseg(4), "nr": 4}] +
        _seg_cases(_mseg, MAPPER_BWD_SEG) +
        _seg_cases(_rseg, REDUCE_SEG + [("out", None)], "nr", "rsegs") +     # per-segment: every out required
        [{"rsegs": _rseg(2, {(1, "count"): 144, (1, "stride"): 144}), "nr": 2}])
    assert lib.mcaq_mapper_train_backward_multi(None, _mseg(1), 1, 2.0, 8.0, 1.0, None) == INVALID
    assert lib.mcaq_mapper_train_backward_multi(MP, _mseg(1, gc=None), 1, 2.0, 8.0, 1.0, None) == INVALID


def test_mapper_train_forward_stage_multi_refusals(lib):
    def call(P, segs, nseg, upd, stage, gathered, world):
        return lib.mcaq_mapper_train_forward_stage_multi(P, segs, nseg, 2.0, 8.0, 1.0, 0.1, 1, upd, stage, gathered,
                                                         world, None)
    PP = ctypes.c_void_p * 3
    base = dict(P=MP, segs=_mseg(1), nseg=1, upd=2, stage=2, gathered=PP(FAKE, FAKE, FAKE), world=2)
    _refusals(call, base, _nulls("P", "segs", "gathered") + [
        {"nseg": 0}, {"segs": _mseg(4), "nseg": 4}, {"segs": _mseg(2), "nseg": 2, "upd": 1},
        {"stage": 0}, {"stage": 5}, {"world": 0}, {"stage": 1, "world": 0},
        {"gathered": PP(None, FAKE, FAKE)}, {"segs": _mseg(3), "nseg": 3, "gathered": PP(FAKE, FAKE, None)},
        {"stage": 4, "gathered": PP(None, FAKE, FAKE)}] +
        _seg_cases(_mseg, MAPPER_FWD_SEG))


def test_mapper_train_backward_stage_multi_refusals(lib):
    def call(P, segs, nseg, stage, gsums, gathered1, world):
        return lib.mcaq_mapper_train_backward_stage_multi(P, segs, nseg, 2.0, 8.0, 1.0, stage, gsums, gathered1, world,
                                                          None)
    PP = ctypes.c_void_p * 3
    ok = PP(FAKE, FAKE, FAKE)
    base = dict(P=MP, segs=_mseg(1), nseg=1, stage=3, gsums=ok, gathered1=ok, world=2)
    _refusals(call, base, _nulls("P", "segs", "gsums", "gathered1") + [
        {"nseg": 0}, {"segs": _mseg(4), "nseg": 4}, {"stage": 0}, {"stage": 5}, {"world": 0},
        {"stage": 4, "world": 0}, {"gsums": PP(None, FAKE, FAKE)}, {"stage": 1, "gathered1": PP(None, FAKE, FAKE)},
        {"segs": _mseg(3), "nseg": 3, "stage": 2, "gsums": PP(FAKE, FAKE, None)}] +
        _seg_cases(_mseg, MAPPER_BWD_SEG))


def test_head_train_backward_multi_ride_refusals(lib):
    def call(P, segs, nseg, rsegs, nr):
        return lib.mcaq_head_train_backward_multi_ride(P, segs, nseg, rsegs, nr, None)
    base = dict(P=CP, segs=_hseg(1), nseg=1, rsegs=_rseg(1), nr=1)
    _refusals(call, base, _nulls("P", "segs", "rsegs") + [
        {"nseg": 0}, {"segs": _hseg(4), "nseg": 4}, {"nr": -1}, {"rsegs": _rseg(4), "nr": 4},
        {"segs": _hseg(1, ht=28, wt=28)}, {"segs": _hseg(3, {(2, "ht"): 28, (2, "wt"): 28}), "nseg": 3},
        {"rsegs": _rseg(1, out=None)},                        # a chain: segment 0's out is the output
        {"rsegs": _rseg(2, {(1, "count"): 144, (1, "stride"): 144}), "nr": 2}] +
        _seg_cases(_hseg, HEAD_SEG) + _seg_cases(_rseg, REDUCE_SEG, "nr", "rsegs"))
    assert lib.mcaq_head_train_backward_multi(None, _hseg(1), 1, None) == INVALID
    assert lib.mcaq_head_train_backward_multi(CP, _hseg(1, gcraw=None), 1, None) == INVALID


def test_smask_train_backward_multi_refusals(lib):
    def call(segs, nseg):
        return lib.mcaq_smask_train_backward_multi(segs, nseg, None)
    base = dict(segs=_sseg(1), nseg=1)
    _refusals(call, base, _nulls("segs") + [
        {"nseg": 0}, {"segs": _sseg(4), "nseg": 4}, {"segs": _sseg(1, H=400, W=400)}] +
        _seg_cases(_sseg, SMASK_SEG))


@pytest.mark.parametrize("chain", [0, 1])
def test_train_reduce_multi_refusals(lib, chain):
    def call(segs, nseg):
        return lib.mcaq_train_reduce_multi(segs, nseg, chain, None)
    cases = _nulls("segs") + [{"nseg": 0}, {"segs": _rseg(4), "nseg": 4}, {"segs": _rseg(1, out=None)}]
    cases += _seg_cases(_rseg, REDUCE_SEG)
    if chain:      # every segment sums into segment 0's output: equal counts
        cases.append({"segs": _rseg(2, {(1, "count"): 144, (1, "stride"): 144}), "nseg": 2})
    else:          # each segment into its own output
        cases.append({"segs": _rseg(3, {(2, "out"): None}), "nseg": 3})
    _refusals(call, dict(segs=_rseg(1), nseg=1), cases)
