"""tests/map_cases.py is a yardstick of the mAP tests: its restatement of
the matching rule must reproduce the reference's compute_map (the fixture
tests/golden/map_cases.npz), and every edge input must reach the edge it is
named for."""
import os

import numpy as np
import pytest

import map_cases as MC
from conftest import GOLDEN

F32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "map_cases.npz"))


def _unpad(g, name):
    det, counts, tgt, tcounts = (g["%s_%s" % (name, k)] for k in ("det", "counts", "tgt", "tcounts"))
    return [det[i, :counts[i]] for i in range(len(counts))], [tgt[i, :tcounts[i]] for i in range(len(tcounts))]


@pytest.mark.parametrize("name", ["mixed", "ties", "sparse", "empty"])
def test_fixture_inputs_are_the_builders(golden, name):
    dets, tgts = MC.fixture_scenarios()[name]
    fd, ft = _unpad(golden, name)
    assert all(np.array_equal(a, b) for a, b in zip(dets, fd)) and len(dets) == len(fd)
    assert all(np.array_equal(a, b) for a, b in zip(tgts, ft))


@pytest.mark.parametrize("name", ["mixed", "ties", "sparse", "empty"])
@pytest.mark.parametrize("interp", ["voc", "coco"])
@pytest.mark.parametrize("tset", ["default", "t50"])
def test_restatement_equals_reference(golden, name, interp, tset):
    dets, tgts = _unpad(golden, name)
    m, _ = MC.greedy_map(dets, tgts, None if tset == "default" else [0.5], interp)
    keys = [str(k) for k in golden["%s_%s_%s_keys" % (name, interp, tset)]]
    vals = golden["%s_%s_%s_vals" % (name, interp, tset)]
    assert list(m.keys()) == keys
    for k, v in zip(keys, vals):
        assert abs(m[k] - v) <= 1e-12, (k, m[k], v)


def test_fixture_scenarios_are_not_trivial(golden):
    for name in ("mixed", "ties", "sparse"):
        v = golden["%s_voc_default_vals" % name]
        assert 0.02 < v[1] < 0.98 and len(set(np.round(v[2:], 9))) > 3, name
        assert not np.array_equal(v, golden["%s_coco_default_vals" % name])
    assert list(golden["empty_voc_default_keys"]) == ["mAP@0.5", "mAP@0.5:0.95"]
    d = golden["ties_det"]
    conf = d[..., 4][d[..., 4] > 0]
    assert len(np.unique(conf)) <= 8 < conf.size              # real confidence ties


# ---------------------------------------------------------------- IoU edges
def _iou(case):
    dets, tgts = case
    return MC.box_iou1(dets[0][0, :4], tgts[0][0, 1:5])


def test_iou_half_edges():
    big, small = _iou(MC.iou_half_large()), _iou(MC.iou_half_small())
    assert big == F32(0.5) and F32(256) + F32(1e-7) == F32(256)          # the eps vanishes
    assert small < F32(0.5) and F32(0.0625) + F32(1e-7) > F32(0.0625)    # the eps lowers it
    _, f = MC.greedy_map(*MC.iou_half_large())
    assert f[0][0].tolist() == [True] + [False] * 9
    _, f = MC.greedy_map(*MC.iou_half_small())
    assert not f[0].any()


def test_iou_055_edges():
    thr = MC.DEFAULT_THR[1]
    assert abs(thr - 0.55) < 1e-15
    up, dn = _iou(MC.iou_055_above()), _iou(MC.iou_055_below())
    assert up == F32(0.55) and float(up) >= thr and float(up) > 0.55
    assert dn == np.nextafter(F32(0.55), F32(0)) and float(dn) < thr
    _, f = MC.greedy_map(*MC.iou_055_above())
    assert f[0][0].tolist() == [True, True] + [False] * 8
    _, f = MC.greedy_map(*MC.iou_055_below())
    assert f[0][0].tolist() == [True] + [False] * 9


# ---------------------------------------------------------------- matching-rule edges
def test_equal_iou_first_row():
    dets, tgts = MC.equal_iou_first_row()
    assert MC.best_gt(dets[0][0], tgts[0])[0] == 0 and MC.best_gt(dets[0][1], tgts[0])[0] == 0
    assert MC.box_iou1(dets[0][1, :4], tgts[0][1, 1:5]) == MC.box_iou1(dets[0][1, :4], tgts[0][0, 1:5])
    _, f = MC.greedy_map(dets, tgts)
    assert f[0][0].all() and not f[0][1].any()


def test_best_taken_other_passes():
    dets, tgts = MC.best_taken_other_passes()
    g, iou = MC.best_gt(dets[0][1], tgts[0])
    other = MC.box_iou1(dets[0][1, :4], tgts[0][1, 1:5])
    assert g == 0 and iou > other and float(other) >= 0.65
    _, f = MC.greedy_map(dets, tgts)
    assert f[0][0].all() and not f[0][1].any()


def test_low_iou_does_not_consume():
    dets, tgts = MC.low_iou_does_not_consume()
    assert MC.best_gt(dets[0][0], tgts[0]) == (0, F32(0.6)) and MC.best_gt(dets[0][1], tgts[0]) == (0, F32(0.9))
    assert float(F32(0.6)) >= MC.DEFAULT_THR[2] and MC.DEFAULT_THR[7] <= float(F32(0.9)) < MC.DEFAULT_THR[8]
    _, f = MC.greedy_map(dets, tgts)
    assert f[0][0].tolist() == [True] * 3 + [False] * 7
    assert f[0][1].tolist() == [False] * 3 + [True] * 5 + [False] * 2


# ---------------------------------------------------------------- order edges
def test_tie_edges():
    dets, tgts = MC.tie_inside_image()
    assert len(set(dets[0][:, 4])) == 1
    m, f = MC.greedy_map(dets, tgts)
    assert f[0][1].all() and not f[0][2].any() and not f[0][0].any()
    assert abs(m["mAP@0.5"] - 0.5) < 1e-9                     # FP first, then the TP
    dets, tgts = MC.tie_across_images()
    assert dets[0][0, 4] == dets[1][0, 4]
    m, _ = MC.greedy_map(dets, tgts)
    assert abs(m["mAP@0.5:0.95"] - 0.5) < 1e-9
    m, _ = MC.greedy_map(dets[::-1], tgts[::-1])
    assert abs(m["mAP@0.5:0.95"] - 1.0) < 1e-9                # the image order decides


# ---------------------------------------------------------------- count edges
def test_count_edges():
    dets, tgts = MC.count_edges(6)
    assert [(len(d), len(t)) for d, t in zip(dets, tgts)] == [(0, 2), (2, 0), (0, 0), (6, 3)]
    dc = {int(c) for d in dets for c in d[:, 5]}
    gc = {int(c) for t in tgts for c in t[:, 0]}
    assert 3 in dc - gc and 4 in gc - dc
    m, f = MC.greedy_map(dets, tgts)
    assert 0 < m["mAP@0.5"] < 1 and f[3].any()


def test_all_tp_all_fp():
    dets, tgts = MC.all_tp_all_fp()
    m, f = MC.greedy_map(dets, tgts)
    for d, fl in zip(dets, f):
        assert fl[d[:, 5] == 0].all() and not fl[d[:, 5] == 1].any()
    assert abs(m["mAP@0.5:0.95"] - 0.5) < 1e-9                # (1 + 0) / 2
