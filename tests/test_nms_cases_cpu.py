"""Reach checks for the NMS edge inputs (tests/nms_cases.py), on the CPU with
the oracle alone: every input is shown to arrive at the kernel branch it was
built for, so the bit-exact GPU comparison in tests/test_nms_edges_gpu.py can
never pass vacuously.  Also pins the oracle's greedy NMS against a second,
scalar restatement."""
import numpy as np
import pytest

import nms_cases as C
from oracle import nms_oracle as NO

F32 = np.float32


def _greedy_inputs(img, kw):
    """Sorted offset boxes and scores of one image, as NO.nms receives them."""
    order, score, cls, box = C.sorted_candidates(img, kw["conf_thres"])
    off = box + (cls.astype(F32) * F32(0 if kw["agnostic"] else 7680))[:, None]
    return off, score


def test_kept_beyond_lds_reaches_the_workspace():
    pred, kw = C.kept_beyond_lds()
    assert pred.shape == (2, 5, 4096) and kw["max_det"] == 2000
    ref = C.oracle(pred, kw)
    assert ref[0].shape[0] >= C.LDS_KEPT + C.CHUNK and ref[0].shape[0] < kw["max_det"]
    assert ref[1].shape[0] == kw["max_det"]                       # image 1: max_det reached
    for b in range(2):
        kept, sup, iou = C.kept_vs_suppressed(pred[b], kw["conf_thres"], kw["iou_thres"])
        hit = iou.astype(np.float64) > kw["iou_thres"]            # (kept rank, suppressed candidate)
        assert hit.any(0).all()
        first = hit.argmax(0)                                     # lowest kept rank that suppresses
        beyond = first >= C.LDS_KEPT                              # every suppressor is past the LDS cache
        assert beyond.sum() >= 64
        # ... and at least 64 of them meet their suppressor as a kept box of an
        # EARLIER chunk (the float4 reads of the workspace), the others inside
        # their own chunk (the workspace writes alone)
        earlier_chunk = kept[first] // C.CHUNK < sup // C.CHUNK
        assert (beyond & earlier_chunk).sum() >= 64 and (beyond & ~earlier_chunk).sum() >= 64
        assert (beyond & earlier_chunk & (kept[first] < kw["max_det"])).sum() >= 64
        # the kept count passes NMS_LDS_KEPT inside a chunk, not at its edge
        assert kept[C.LDS_KEPT] % C.CHUNK not in (0, C.CHUNK - 1)
        # and boxes inside the LDS cache suppress across chunks too
        assert (~beyond & earlier_chunk).sum() >= 32


def test_keys_boundary_counts():
    pred, kw = C.keys_boundary()
    assert pred.shape == (2, 5, C.LDS_KEYS + 1)
    assert C.candidate_counts(pred, kw["conf_thres"]).tolist() == [C.LDS_KEYS, C.LDS_KEYS + 1]
    ref = C.oracle(pred, kw)
    for b, r in enumerate(ref):
        # every survivor is in the result, and the last kept one comes from the
        # tail of the sorted order: the whole sort matters
        assert 2000 < r.shape[0] < kw["max_det"]
        kept, _, _ = C.kept_vs_suppressed(pred[b], kw["conf_thres"], kw["iou_thres"])
        assert kept[-1] == C.LDS_KEYS - 1 + b
    # the anchors do not arrive sorted
    order = C.sorted_candidates(pred[1], kw["conf_thres"])[0]
    assert (np.diff(order) < 0).sum() > 3000


def test_chunk_words_reach():
    pred, kw = C.chunk_words_counts()
    assert C.candidate_counts(pred, kw["conf_thres"]).tolist() == list(C.CHUNK_WORD_COUNTS)
    assert [r.shape[0] for r in C.oracle(pred, kw)] == list(C.CHUNK_WORD_COUNTS)      # disjoint: all kept
    pred, kw = C.chunk_words_dups()
    for b, pairs in enumerate(C.CHUNK_WORD_DUPS):
        kept, sup, iou = C.kept_vs_suppressed(pred[b], kw["conf_thres"], kw["iou_thres"])
        assert sup.tolist() == [q for _, q in pairs]
        hit = iou.astype(np.float64) > kw["iou_thres"]
        assert [kept[hit[:, k]].tolist() for k in range(len(pairs))] == [[p] for p, _ in pairs]


@pytest.mark.parametrize("name", ["chain_in_chunk", "chain_cross_chunk"])
def test_chains_need_greedy_liveness(name):
    pred, kw = getattr(C, name)()
    assert pred.shape[2] <= 600
    triples = C.CHAIN_IN_CHUNK if name == "chain_in_chunk" else C.CHAIN_CROSS_CHUNK
    off, score = _greedy_inputs(pred[0], kw)
    greedy = NO.nms(off, score, kw["iou_thres"])
    loose = C.nms_non_greedy(off, score, kw["iou_thres"])
    assert not np.array_equal(greedy, loose)
    iou = C.iou_matrix(off, off).astype(np.float64)
    for k, (a, b, c) in enumerate(triples):
        assert iou[a, b] > kw["iou_thres"] and iou[b, c] > kw["iou_thres"] and iou[a, c] <= kw["iou_thres"]
        assert a in greedy and b not in greedy and c in greedy and c not in loose
        if name == "chain_in_chunk":
            assert a // C.CHUNK == b // C.CHUNK == c // C.CHUNK == 0
        elif k < 2:
            assert b // C.CHUNK == c // C.CHUNK == a // C.CHUNK + 1
        else:
            assert a // C.CHUNK < b // C.CHUNK < c // C.CHUNK
    if name == "chain_in_chunk":
        assert any(b % 64 == 63 and c % 64 == 0 for _, b, c in triples)      # one chain straddles a word edge
    # the independent scalar restatement agrees with the oracle's greedy NMS
    n = 320 if name == "chain_cross_chunk" else 80
    assert np.array_equal(C.nms_scalar(off[:n], score[:n], kw["iou_thres"]), NO.nms(off[:n], score[:n], kw["iou_thres"]))
    assert len(NO.nms(off[:n], score[:n], kw["iou_thres"])) < n


@pytest.mark.parametrize("thr,suppressed", [(0.6, True), (0.5, False), (0.7, False)])
def test_iou_at_threshold_reach(thr, suppressed):
    pred, kw = C.iou_at_threshold(thr)
    assert pred.shape == (1, 5, 2) and kw["iou_thres"] == thr
    off, score = _greedy_inputs(pred[0], kw)
    ovr = C.iou_matrix(off[:1], off[1:])[0, 0]
    assert ovr.dtype == F32 and ovr.tobytes() == F32(thr).tobytes()
    if thr == 0.6:
        assert float(F32(thr)) > thr
    elif thr == 0.5:
        assert float(ovr) == 0.5
    else:
        assert float(F32(thr)) < thr
    ref = C.oracle(pred, kw)[0]
    assert ref.shape[0] == (1 if suppressed else 2)
    assert np.array_equal(C.nms_scalar(off, score, thr), NO.nms(off, score, thr))
    # classes 0 and 1: the same two boxes meet only when the NMS is class-agnostic
    for agnostic in (True, False):
        p2, kw2 = C.iou_at_threshold(thr, classes=(0, 1), nc=2, agnostic=agnostic)
        r = C.oracle(p2, kw2)[0]
        assert r.shape[0] == (1 if suppressed and agnostic else 2)
        assert r[:, 5].tolist() == [0.0, 1.0][:r.shape[0]]
    p3, kw3 = C.iou_at_threshold(thr, classes=(1, 1), nc=2)      # both offset by max_wh: same exact ratio
    assert C.oracle(p3, kw3)[0].shape[0] == (1 if suppressed else 2)


def test_max_nms_tie_cut_reach():
    m = C.MAX_NMS_TIE_CUT
    pred, kw = C.max_nms_edges(m)
    assert pred.shape == (1, 6, 1000) and kw["max_nms"] == m
    assert C.candidate_counts(pred, kw["conf_thres"])[0] > m
    order, score, cls, box = C.sorted_candidates(pred[0], kw["conf_thres"])
    assert score[m - 1] == score[m] and order[m - 1] < order[m]
    # the first box past the cut overlaps nothing: it is absent from the
    # result only because of the cut
    iou = C.iou_matrix(box[m:m + 1], box)[0]
    iou[m] = 0
    assert not iou.any()
    cut = C.oracle(pred, kw)[0]
    full = C.oracle(pred, dict(kw, max_nms=30000))[0]
    has = lambda r: (r[:, :4] == box[m]).all(1).any()
    assert has(full) and not has(cut)
    for mn in C.MAX_NMS_EDGES:                       # every cut falls inside a run of tied scores
        assert mn == 1 or score[mn - 1] == score[mn]
        assert score[mn] == score[mn + 1] or score[mn - 1] == score[mn]
    assert 0 < full.shape[0] < 1000                  # some suppression, both classes
    assert set(full[:, 5].tolist()) == {0.0, 1.0}


def test_max_det_chunk_end_reach():
    pred, kw = C.max_det_edges(256)
    assert C.candidate_counts(pred, kw["conf_thres"])[0] > C.CHUNK and kw["max_det"] == C.CHUNK
    assert C.oracle(pred, dict(kw, max_det=1000))[0].shape[0] == 300       # disjoint
    assert C.oracle(pred, kw)[0].shape[0] == C.CHUNK


@pytest.mark.parametrize("nc", C.SCAN_NCS)
def test_argmax_ties_reach(nc):
    pred, kw = C.scan_class_loop(nc)
    assert pred.shape == (1, 4 + nc, 257)
    pairs = C.argmax_tie_pairs(nc)
    assert all(p in pairs for p in C.ARGMAX_TIE_PAIRS if p[1] < nc)
    ref = C.oracle(pred, kw)[0]
    cls = pred[0, 4:]
    for t, (lo, hi) in enumerate(pairs):
        assert lo < hi and cls[lo, t] == cls[hi, t] == cls[:, t].max() > kw["conf_thres"]
        assert (cls[:, t] == cls[:, t].max()).sum() == 2
        row = ref[(ref[:, :4] == NO.xywh2xyxy(C.tie_box(t)[None])[0]).all(1)]
        assert row.shape[0] == 1 and row[0, 5] == lo
    # every class is the argmax of some kept detection, and something is suppressed
    assert set(ref[:, 5].astype(int).tolist()) == set(range(nc))
    n = C.candidate_counts(pred, kw["conf_thres"])[0]
    assert ref.shape[0] < n < 257


def test_listed_tie_pairs_are_all_used():
    used = {p for nc in C.SCAN_NCS for p in C.argmax_tie_pairs(nc)}
    assert set(C.ARGMAX_TIE_PAIRS) <= used


@pytest.mark.parametrize("N", C.SCAN_WAVE_NS)
def test_scan_waves_reach(N):
    pred, kw = C.scan_waves(N)
    assert pred.shape == (6, 7, N)
    cand = pred[:, 4:].max(1) > F32(kw["conf_thres"])
    assert cand[0].all()
    assert cand[1].nonzero()[0].tolist() == [0]
    assert cand[2].nonzero()[0].tolist() == [min(63, N - 1)]
    assert cand[3].nonzero()[0].tolist() == [N - 1]
    waves = set((cand[4].nonzero()[0] // 64).tolist())
    assert waves <= {0, 3} and (N <= 192 or waves == {0, 3})
    assert [r.shape[0] for r in C.oracle(pred, kw)] == cand.sum(1).tolist()


def test_batch_mix_reach():
    pred, kw = C.batch_mix()
    assert pred.shape == (33, 8, 700)
    n = C.candidate_counts(pred, kw["conf_thres"])
    cnt = np.asarray([r.shape[0] for r in C.oracle(pred, kw)])
    assert (n[0::4] == 0).all() and (n[1::4] == 1).all() and (n[2::4] == 700).all() and (n[3::4] > kw["max_det"]).all()
    assert (cnt[0::4] == 0).all() and (cnt[1::4] == 1).all() and (cnt[3::4] == kw["max_det"]).all()
    assert ((cnt[2::4] > 1) & (cnt[2::4] < kw["max_det"])).all()


def test_reuse_and_graph_sequences_reach():
    preds, kw = C.reuse_sequence()
    counts = [C.candidate_counts(p, kw["conf_thres"]).tolist() for p in preds]
    assert counts[0] == [C.LDS_KEYS, C.LDS_KEYS + 1] and counts[1] == [10, 10] and counts[3] == [0, 0]
    assert min(counts[2]) > 2000 and all(p.shape == preds[0].shape for p in preds)
    preds, kw = C.graph_sequence()
    counts = [int(C.candidate_counts(p, kw["conf_thres"])[0]) for p in preds]
    assert counts == [0, 300, C.LDS_KEYS + 1]


def test_nan_scores_reach():
    pred, kw = C.nan_scores()
    cls = pred[0, 4:]
    kind = C.nan_kind(np.arange(pred.shape[2]))
    first = kind < len(C.NAN_FIRST)
    later = ~first & (kind < len(C.NAN_FIRST) + len(C.NAN_LATER))
    assert first.sum() >= 8 and later.sum() >= 8
    assert np.isnan(cls[0, first]).all() and np.isnan(cls[:, first | later]).any(0).all()
    assert not np.isnan(cls[0, later]).any() and not np.isnan(cls[:, ~(first | later)]).any()
    # otherwise above conf: the finite maximum clears the threshold (but for the all-NaN kind)
    with np.errstate(all="ignore"), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        finite_max = np.nanmax(cls, 0)
    all_nan = np.isnan(cls).all(0)
    assert (finite_max[later] > kw["conf_thres"]).all() and (finite_max[first & ~all_nan] > kw["conf_thres"]).all()
    assert all_nan.sum() >= 4 and (first & ~all_nan).sum() >= 8
    # NaN in the unrolled group (classes 1..8) and in the remainder (class 9)
    assert np.isnan(cls[1:9, later]).any() and np.isnan(cls[9, later]).any()
    # the oracle drops both kinds and keeps every plain anchor (disjoint boxes)
    ref = C.oracle(pred, kw)[0]
    plain = ~(first | later)
    assert ref.shape[0] == plain.sum() == C.candidate_counts(pred, kw["conf_thres"])[0]
    boxes = NO.xywh2xyxy(pred[0, :4].T)
    assert sorted(map(tuple, ref[:, :4].tolist())) == sorted(map(tuple, boxes[plain].tolist()))


def test_other_nonfinite_inputs_reach():
    pred, kw = C.inf_score()
    ref = C.oracle(pred, kw)[0]
    assert np.isinf(ref[:2, 4]).all() and np.isfinite(ref[2:, 4]).all() and ref.shape[0] == 70 - 2
    pred, kw = C.nonfinite_boxes()
    ref = C.oracle(pred, kw)[0]
    assert ref.shape[0] == 40                                    # nothing suppressed ...
    finite = np.where(np.isfinite(pred[0, :4]), pred[0, :4], 10.0).astype(F32)
    assert C.oracle(np.concatenate([finite, pred[0, 4:]])[None], kw)[0].shape[0] < 40 - 3   # ... though finite boxes there would
    assert np.isnan(ref[:, :4]).any(1).sum() >= 2 and np.isinf(ref[:, :4]).any(1).sum() >= 3
    pred, kw = C.signed_zeros()
    s = pred[0, 4]
    zeros = s == 0
    neg = np.signbit(s)
    assert kw["conf_thres"] < 0 and (zeros & neg).sum() >= 16 and (zeros & ~neg).sum() >= 16
    assert (np.diff(neg[zeros].astype(int)) != 0).sum() >= 16           # interleaved over the anchors
    ref = C.oracle(pred, kw)[0]
    # ordering every +0 before every -0 (the unfixed key) gives another result
    t = pred.copy()
    t[0, 4] = np.where(zeros & np.signbit(s), F32(-2.0 ** -20), s)
    alt = C.oracle(t, kw)[0]
    assert ref.shape == alt.shape and not np.array_equal(ref[:, :4], alt[:, :4])
    assert (ref[:, 4] == 0).sum() >= 3
