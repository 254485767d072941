"""The batched NMS kernels (mcaq_nms.h) at their branch edges: every input of
tests/nms_cases.py - each shown by tests/test_nms_cases_cpu.py to reach the
branch it was built for - through `nms_padded`, bit-exact against the NMS
restatement (oracle/nms_oracle.py): counts equal, rows equal, zero rows past
the count."""
import numpy as np
import pytest
import torch

import nms_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _compare(out, cnt, ref, equal_nan=False):
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    assert len(ref) == out.shape[0] == cnt.shape[0]
    for b, r in enumerate(ref):
        assert cnt[b] == r.shape[0], (b, cnt[b], r.shape)
        assert np.array_equal(out[b, :cnt[b]], r, equal_nan=equal_nan), b
        assert not out[b, cnt[b]:].any()
    return cnt


def _check(case, equal_nan=False):
    from mcaq_yolo_amd.postprocess import nms_padded
    pred, kw = case
    out, cnt = nms_padded(torch.from_numpy(pred).to(DEV), **kw)
    return _compare(out, cnt, C.oracle(pred, kw), equal_nan)


def _twice(case):
    """The scan's slot order depends on its atomics; the sort must erase it."""
    from mcaq_yolo_amd.postprocess import nms_padded
    pred, kw = case
    p = torch.from_numpy(pred).to(DEV)
    first = [t.clone() for t in nms_padded(p, **kw)]
    second = nms_padded(p, **kw)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def test_kept_beyond_lds():
    case = C.kept_beyond_lds()
    cnt = _check(case)
    assert cnt[0] >= C.LDS_KEPT + C.CHUNK and cnt[1] == case[1]["max_det"]
    _twice(case)


def test_keys_8192_and_8193():
    case = C.keys_boundary()
    _check(case)
    _twice(case)


def test_chunk_words():
    assert _check(C.chunk_words_counts()).tolist() == list(C.CHUNK_WORD_COUNTS)
    cnt = _check(C.chunk_words_dups())
    assert cnt.tolist() == [513 - len(p) for p in C.CHUNK_WORD_DUPS]


@pytest.mark.parametrize("name", ["chain_in_chunk", "chain_cross_chunk"])
def test_chains(name):
    _check(getattr(C, name)())


@pytest.mark.parametrize("thr,suppressed", [(0.6, True), (0.5, False), (0.7, False)])
def test_iou_at_threshold(thr, suppressed):
    assert _check(C.iou_at_threshold(thr)).tolist() == [1 if suppressed else 2]
    assert _check(C.iou_at_threshold(thr, classes=(1, 1), nc=2)).tolist() == [1 if suppressed else 2]
    for agnostic in (True, False):
        cnt = _check(C.iou_at_threshold(thr, classes=(0, 1), nc=2, agnostic=agnostic))
        assert cnt.tolist() == [1 if suppressed and agnostic else 2]


@pytest.mark.parametrize("max_nms", C.MAX_NMS_EDGES + (C.MAX_NMS_TIE_CUT,))
def test_max_nms_edges(max_nms):
    cnt = _check(C.max_nms_edges(max_nms))
    assert 0 < cnt[0] <= max_nms


@pytest.mark.parametrize("max_det", [1, 256, 257])
def test_max_det_edges(max_det):
    assert _check(C.max_det_edges(max_det)).tolist() == [max_det]


@pytest.mark.parametrize("nc", C.SCAN_NCS)
def test_scan_class_loop(nc):
    assert _check(C.scan_class_loop(nc))[0] > len(C.argmax_tie_pairs(nc))


@pytest.mark.parametrize("N", C.SCAN_WAVE_NS)
def test_scan_waves(N):
    cnt = _check(C.scan_waves(N))
    assert cnt[0] == N and cnt[1:4].tolist() == [1, 1, 1]


def test_batch_mix():
    cnt = _check(C.batch_mix())
    assert (cnt[0::4] == 0).all() and (cnt[1::4] == 1).all() and (cnt[3::4] == 100).all() and (cnt[2::4] > 1).all()


def test_plan_reuse():
    """One plan, four inputs in a row: nothing of an earlier call (keys, their
    ~0 padding, classes, kept boxes, counts) may show in a later one."""
    from mcaq_yolo_amd.postprocess import NmsPlan
    preds, kw = C.reuse_sequence()
    plan = NmsPlan(*preds[0].shape, kw["max_det"], torch.device(DEV))
    refs = [C.oracle(pred, kw) for pred in preds]
    for i in (0, 1, 2, 3, 0):
        out, cnt = plan.run(torch.from_numpy(preds[i]).to(DEV), kw["conf_thres"], kw["iou_thres"], kw["agnostic"],
                            kw["max_nms"])
        _compare(out, cnt, refs[i])


def test_graph_replay():
    """The memset and the two launches captured once serve any later input:
    nothing of the capture-time candidate count is baked in."""
    from mcaq_yolo_amd.postprocess import NmsPlan
    preds, kw = C.graph_sequence()
    plan = NmsPlan(*preds[0].shape, kw["max_det"], torch.device(DEV))
    static = torch.from_numpy(preds[1]).to(DEV)
    run = lambda: plan.run(static, kw["conf_thres"], kw["iou_thres"], kw["agnostic"], kw["max_nms"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, cnt = run()
    refs = [C.oracle(pred, kw) for pred in preds]
    for i in (0, 1, 2, 0, 1):
        static.copy_(torch.from_numpy(preds[i]))
        graph.replay()
        torch.cuda.synchronize()
        _compare(out, cnt, refs[i])


def test_nonfinite_nan_scores():
    """An anchor with a NaN in any class score is no candidate, whichever class
    carries it (`amax` propagates NaN)."""
    from mcaq_yolo_amd.postprocess import nms_padded
    pred, kw = C.nan_scores()
    out, cnt = nms_padded(torch.from_numpy(pred).to(DEV), **kw)
    ref = C.oracle(pred, kw)
    # say which anchors came through before the rows are compared
    got = {tuple(r) for r in out[0, :int(cnt[0])].cpu().numpy()[:, :4].tolist()}
    boxes = C.NO.xywh2xyxy(pred[0, :4].T).tolist()
    kinds = sorted({int(C.nan_kind(a)) for a, b in enumerate(boxes) if tuple(b) in got and C.nan_kind(a) < 8})
    assert not kinds, "NaN-scored anchors kept as candidates: kinds %s (0-2: NaN at class 0, 3-7: NaN at a later class)" % kinds
    _compare(out, cnt, ref)


def test_nonfinite_inf_and_boxes():
    cnt = _check(C.inf_score())
    assert cnt[0] == 68
    assert _check(C.nonfinite_boxes(), equal_nan=True).tolist() == [40]


def test_nonfinite_signed_zeros():
    """+0 and -0 scores tie and fall back to the anchor order."""
    _check(C.signed_zeros())


def test_inputs():
    from mcaq_yolo_amd.postprocess import NmsPlan, nms_padded
    pred, kw = C.scan_class_loop(9)
    pred = np.concatenate([pred, C.scan_class_loop(9, N=257)[0][:, :, ::-1]])
    # fp16: the kernel sees the fp16 values widened to fp32
    h = pred.astype(np.float16)
    out, cnt = nms_padded(torch.from_numpy(h).to(DEV), **kw)
    assert _compare(out, cnt, C.oracle(h.astype(np.float32), kw)).min() > 0
    # a transposed, non-contiguous view
    t = torch.from_numpy(np.ascontiguousarray(pred.transpose(0, 2, 1))).to(DEV).transpose(1, 2)
    assert not t.is_contiguous() and tuple(t.shape) == pred.shape
    out, cnt = nms_padded(t, **kw)
    _compare(out, cnt, C.oracle(pred, kw))
    # no anchors at all
    empty = np.zeros((2, 13, 0), np.float32)
    out, cnt = nms_padded(torch.from_numpy(empty).to(DEV), **kw)
    assert _compare(out, cnt, C.oracle(empty, kw)).tolist() == [0, 0] and tuple(out.shape) == (2, 300, 6)
    # a plan refuses another shape, dtype or layout
    plan = NmsPlan(2, 13, 257, 300, torch.device(DEV))
    good = torch.from_numpy(pred).to(DEV)
    _compare(*plan.run(good), C.oracle(pred, kw))
    for bad in (good[:1], good[:, :, :256], good.half(), t):
        with pytest.raises(ValueError):
            plan.run(bad)
