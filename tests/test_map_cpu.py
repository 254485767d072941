"""mcaq_yolo_amd.evaluation without a GPU: compute_map against the reference
fixture (tests/golden/map_cases.npz: the reference's compute_map with a
restated box_iou), the result keys and the target helpers.

Tolerance: AP and mAP are float64 sums of non-negative terms totalling <= 1;
another summation order than numpy's pairwise sum moves them by at most
n * 2^-53, for the few thousand terms here < 1e-12: the bound is 1e-12
absolute.  The TP flags are integers: exact."""
import os

import numpy as np
import pytest
import torch

import map_cases as MC
from conftest import GOLDEN
from mcaq_yolo_amd import evaluation as E

TOL = 1e-12
SCENARIOS = ["mixed", "ties", "sparse", "empty"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "map_cases.npz"))


def _lists(g, name):
    det, counts, tgt, tcounts = (g["%s_%s" % (name, k)] for k in ("det", "counts", "tgt", "tcounts"))
    return ([torch.from_numpy(det[i, :counts[i]].copy()) for i in range(len(counts))],
            [torch.from_numpy(tgt[i, :tcounts[i]].copy()) for i in range(len(tcounts))])


@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("interp", ["voc", "coco"])
@pytest.mark.parametrize("tset", ["default", "t50"])
def test_cpu_compute_map_equals_reference(golden, name, interp, tset):
    dets, tgts = _lists(golden, name)
    m = E.compute_map(dets, tgts, iou_thresholds=None if tset == "default" else [0.5], interp=interp)
    keys = [str(k) for k in golden["%s_%s_%s_keys" % (name, interp, tset)]]
    vals = golden["%s_%s_%s_vals" % (name, interp, tset)]
    assert list(m.keys()) == keys
    for k, v in zip(keys, vals):
        assert isinstance(m[k], float) and abs(m[k] - v) <= TOL, (k, m[k], v)


def test_key_names_and_empty_result():
    dets, tgts = [torch.from_numpy(a) for a in MC.all_tp_all_fp()[0]], [torch.from_numpy(a) for a in MC.all_tp_all_fp()[1]]
    m = E.compute_map(dets, tgts)
    assert list(m) == ["mAP@0.5", "mAP@0.5:0.95"] + ["mAP@%.2f" % t for t in np.linspace(0.5, 0.95, 10)]
    assert list(m)[2] == "mAP@0.50" and list(m)[-1] == "mAP@0.95"
    assert list(E.compute_map(dets, tgts, iou_thresholds=[0.75, 0.5])) == ["mAP@0.5", "mAP@0.5:0.95", "mAP@0.75",
                                                                          "mAP@0.50"]
    empty = E.compute_map([torch.zeros(0, 6)] * 2, [torch.zeros(0, 5)] * 2)
    assert empty == {"mAP@0.5": 0.0, "mAP@0.5:0.95": 0.0}
    assert E.compute_map([], []) == {"mAP@0.5": 0.0, "mAP@0.5:0.95": 0.0}
    with pytest.raises(ValueError):
        E.compute_map(dets, tgts, interp="pascal")


@pytest.mark.parametrize("case", ["iou_half_large", "iou_half_small", "iou_055_above", "iou_055_below",
                                  "equal_iou_first_row", "best_taken_other_passes", "low_iou_does_not_consume",
                                  "tie_inside_image", "tie_across_images", "count_edges", "all_tp_all_fp"])
def test_cpu_flags_and_metrics_on_edges(case):
    dets, tgts = getattr(MC, case)()
    for interp in ("voc", "coco"):
        ref, flags = MC.greedy_map(dets, tgts, interp=interp)
        m = E.compute_map([torch.from_numpy(d) for d in dets], [torch.from_numpy(t) for t in tgts], interp=interp)
        assert list(m) == list(ref)
        assert all(abs(m[k] - ref[k]) <= TOL for k in ref), (m, ref)
    _, _, tp, _ = E.match_cpu(dets, tgts, MC.DEFAULT_THR)
    assert np.array_equal(tp, np.concatenate(flags))


def test_extract_targets_both_formats():
    boxes = torch.tensor([[0.5, 0.5, 0.5, 0.25], [0.25, 0.75, 0.125, 0.5], [0.5, 0.5, 1.0, 1.0]])
    px = E.cxcywh_norm_to_xyxy_pixels(boxes, 64, 32)
    assert px.dtype == torch.float32
    assert px.tolist() == [[16, 12, 48, 20], [12, 16, 20, 32], [0, 0, 64, 32]]
    batch = {"cls": torch.tensor([[3.0], [1.0], [7.0]]), "bboxes": boxes, "batch_idx": torch.tensor([0.0, 2.0, 0.0])}
    per = E.extract_targets_per_image(batch, 3, 64, 32)
    assert per[0].tolist() == [[3, 16, 12, 48, 20], [7, 0, 0, 64, 32]]
    assert tuple(per[1].shape) == (0, 5)                     # an image without targets
    assert per[2].tolist() == [[1, 12, 16, 20, 32]]
    labels = [torch.tensor([[3.0, 0.5, 0.5, 0.5, 0.25]]), torch.zeros(0, 5), torch.tensor([[1.0, 0.25, 0.75, 0.125, 0.5]])]
    per = E.extract_targets_per_image({"labels": labels}, 3, 64, 32)
    assert per[0].tolist() == [[3, 16, 12, 48, 20]] and tuple(per[1].shape) == (0, 5)
    assert per[2].tolist() == [[1, 12, 16, 20, 32]]
    one = E.extract_targets_per_image({"labels": labels[0]}, 2, 64, 32)     # a single (m, 5) tensor: image 0
    assert one[0].tolist() == [[3, 16, 12, 48, 20]] and tuple(one[1].shape) == (0, 5)
    assert all(tuple(t.shape) == (0, 5) for t in E.extract_targets_per_image({}, 2, 64, 32))
    tgt, cnt = E.pad_targets(per, "cpu")
    assert tuple(tgt.shape) == (3, 1, 5) and tgt.dtype == torch.float32 and cnt.dtype == torch.int32
    assert cnt.tolist() == [1, 0, 1] and not tgt[1].any()
