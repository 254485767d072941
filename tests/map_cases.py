"""A plain restatement of the reference's mAP matching rule
(mcaq_yolo/utils/evaluation.py:102-190) that also returns the true-positive
flags - the reference does not expose them - and the builders of the inputs
that drive mcaq_yolo_amd.evaluation to the edges of the rule.
tests/test_map_cases_cpu.py proves that the restatement's metrics equal the
reference fixture (tests/golden/map_cases.npz) and that every edge input
reaches the edge it is named for, before tests/test_map_cpu.py relies on
either.

Every builder returns `(dets, tgts)`: per-image lists of (n, 6) fp32
[x1, y1, x2, y2, conf, cls] and (m, 5) fp32 [cls, x1, y1, x2, y2] arrays.

Imports numpy only."""
import numpy as np

F32 = np.float32
DEFAULT_THR = np.linspace(0.5, 0.95, 10).tolist()


# ---------------------------------------------------------------- restatement
def box_iou1(a, b):
    """ultralytics box_iou of one box against one box, on np.float32 scalars:
    inter / (area_a + area_b - inter + 1e-7), operands added in that order."""
    a, b = [F32(v) for v in a], [F32(v) for v in b]
    w = max(F32(min(a[2], b[2]) - max(a[0], b[0])), F32(0))
    h = max(F32(min(a[3], b[3]) - max(a[1], b[1])), F32(0))
    inter = F32(w * h)
    aa = F32(F32(a[2] - a[0]) * F32(a[3] - a[1]))
    ab = F32(F32(b[2] - b[0]) * F32(b[3] - b[1]))
    return F32(inter / F32(F32(F32(aa + ab) - inter) + F32(1e-7)))


def best_gt(det_row, tgt):
    """(row, iou) of the first maximum over the same-class GT rows; (-1, None)
    without one."""
    best, biou = -1, None
    for g, row in enumerate(tgt):
        if row[0] != det_row[5]:
            continue
        iou = box_iou1(det_row[:4], row[1:5])
        if biou is None or iou > biou:
            best, biou = g, iou
    return best, biou


def ap_from_flags(tp, n_gt, interp):
    tp = np.asarray(tp, np.float64)
    tp_cum, fp_cum = np.cumsum(tp), np.cumsum(1.0 - tp)
    recall = tp_cum / (n_gt + 1e-10)
    precision = tp_cum / (tp_cum + fp_cum + 1e-10)
    r = np.concatenate(([0.0], recall, [1.0]))
    p = np.concatenate(([1.0], precision, [0.0]))
    for i in range(len(p) - 2, -1, -1):
        p[i] = max(p[i], p[i + 1])
    if interp == "coco":
        return float(np.interp(np.linspace(0.0, 1.0, 101), r, p).mean())
    idx = np.where(r[1:] != r[:-1])[0]
    return float(np.sum((r[idx + 1] - r[idx]) * p[idx + 1]))


def greedy_map(dets, tgts, thresholds=None, interp="voc"):
    """Per-detection greedy matching.  Returns (metrics, flags): the
    reference's result dict and, per image, an (n, T) bool array of TP flags."""
    thresholds = DEFAULT_THR if thresholds is None else list(thresholds)
    T = len(thresholds)
    flags = [np.zeros((len(d), T), bool) for d in dets]
    classes = sorted({int(c) for t in tgts for c in t[:, 0]} | {int(c) for d in dets for c in d[:, 5]})
    if not classes:
        return {"mAP@0.5": 0.0, "mAP@0.5:0.95": 0.0}, flags
    recs = []            # (image, row, conf, cls, best row, iou)
    for i, (d, t) in enumerate(zip(dets, tgts)):
        for r, row in enumerate(d):
            g, iou = best_gt(row, t)
            recs.append((i, r, float(row[4]), float(row[5]), g, iou))
    maps = []
    for ti, thr in enumerate(thresholds):
        aps = []
        for c in classes:
            n_gt = sum(int((t[:, 0] == c).sum()) for t in tgts)
            mine = sorted((x for x in recs if x[3] == c), key=lambda x: -x[2])      # stable
            if n_gt == 0 or not mine:
                aps.append(0.0)
                continue
            matched = set()
            tp = []
            for i, r, _, _, g, iou in mine:
                hit = g >= 0 and float(iou) >= thr and (i, g) not in matched
                if hit:
                    matched.add((i, g))
                    flags[i][r, ti] = True
                tp.append(hit)
            aps.append(ap_from_flags(tp, n_gt, interp))
        maps.append(float(np.mean(aps)))
    out = {"mAP@0.5": maps[0], "mAP@0.5:0.95": float(np.mean(maps))}
    for t, m in zip(thresholds, maps):
        out["mAP@%.2f" % t] = m
    return out, flags


# ---------------------------------------------------------------- helpers
def D(*rows):
    return np.asarray(rows, F32).reshape(-1, 6)


def G(*rows):
    return np.asarray(rows, F32).reshape(-1, 5)


def pad(dets, tgts, max_det=None, gwidth=None):
    """Padded (B, max_det, 6), counts, (B, G, 5), tcounts as numpy arrays."""
    B = len(dets)
    max_det = max_det or max([1] + [len(d) for d in dets])
    gwidth = gwidth or max([1] + [len(t) for t in tgts])
    out, tgt = np.zeros((B, max_det, 6), F32), np.zeros((B, gwidth, 5), F32)
    for i, (d, t) in enumerate(zip(dets, tgts)):
        out[i, :len(d)] = d
        tgt[i, :len(t)] = t
    return out, np.asarray([len(d) for d in dets], np.int32), tgt, np.asarray([len(t) for t in tgts], np.int32)


def scene(seed, n_img, max_n, max_m, nc, empty_every=0, conf_steps=64, grid=0):
    """Random images: GT boxes, detections that are jittered copies of GT rows
    (some with the wrong class) plus stray boxes; confidences are multiples of
    1 / conf_steps, so ties are common; grid > 0 snaps the coordinates (equal
    IoUs, identical boxes)."""
    rng = np.random.default_rng(seed)
    dets, tgts = [], []
    for i in range(n_img):
        m = int(rng.integers(0, max_m + 1))
        n = int(rng.integers(0, max_n + 1))
        if empty_every and i % empty_every == 0:
            m = 0
        if empty_every and i % empty_every == 1:
            n = 0
        xy = rng.uniform(0, 500, (m, 2))
        wh = rng.uniform(20, 120, (m, 2))
        gcls = rng.integers(0, nc, m)
        t = np.concatenate([gcls[:, None], xy, xy + wh], 1).astype(F32)
        rows = []
        for _ in range(n):
            if m and rng.random() < 0.75:
                g = int(rng.integers(0, m))
                box = t[g, 1:5] + rng.normal(0, 6, 4)
                c = t[g, 0] if rng.random() < 0.85 else rng.integers(0, nc + 1)
            else:
                p = rng.uniform(0, 500, 2)
                box = np.concatenate([p, p + rng.uniform(20, 120, 2)])
                c = rng.integers(0, nc + 1)
            rows.append(list(box) + [rng.integers(1, conf_steps) / conf_steps, c])
        d = np.asarray(rows, F32).reshape(-1, 6)
        if grid:
            d[:, :4] = np.round(d[:, :4] / grid) * grid
            t[:, 1:5] = np.round(t[:, 1:5] / grid) * grid
        dets.append(d)
        tgts.append(t)
    return dets, tgts


# ---------------------------------------------------------------- fixture scenarios
def fixture_scenarios():
    """name -> (dets, tgts): what tests/golden/make_golden_map.py feeds the
    reference's compute_map."""
    s = {
        "mixed": scene(1, 24, 30, 8, 4),
        "ties": scene(2, 16, 24, 6, 3, conf_steps=8, grid=16),
        "sparse": scene(3, 20, 12, 4, 6, empty_every=3),
        "empty": ([np.zeros((0, 6), F32)] * 3, [np.zeros((0, 5), F32)] * 3),
    }
    return s


# ---------------------------------------------------------------- IoU edges
def _pair(w, s, h):
    """GT [0, 0, w, h] and a detection shifted by s: IoU (w - s) / (w + s)."""
    return [0.0, 0.0, w, h], [s, 0.0, w + s, h]


def iou_half_large():
    """IoU 128 / 256: + 1e-7 vanishes in fp32, the IoU is exactly 0.5: TP at 0.5."""
    g, d = _pair(24.0, 8.0, 8.0)
    return [D(d + [0.9, 0])], [G([0] + g)]


def iou_half_small():
    """The same ratio at 1/64 of the size: union 0.0625, + 1e-7 lowers the
    IoU below 0.5: FP at 0.5."""
    g, d = _pair(0.375, 0.125, 0.125)
    return [D(d + [0.9, 0])], [G([0] + g)]


def iou_055_above():
    """176 / 320: the fp32 quotient is fp32(0.55) = 0.55000001 >= the double 0.55."""
    g, d = _pair(31.0, 9.0, 8.0)
    return [D(d + [0.9, 0])], [G([0] + g)]


def iou_055_below():
    """0.6875 / (1.25 + 1e-7): the fp32 quotient is the neighbour below
    fp32(0.55), 0.54999995 < the double 0.55."""
    g, d = _pair(7.75, 2.25, 0.125)
    return [D(d + [0.9, 0])], [G([0] + g)]


# ---------------------------------------------------------------- matching-rule edges
def equal_iou_first_row():
    """Two identical GT rows: both detections' best GT is row 0; the second
    detection is a FP and row 1 is never matched."""
    box = [10.0, 10.0, 50.0, 50.0]
    return [D(box + [0.9, 2], box + [0.8, 2])], [G([2] + box, [2] + box)]


def best_taken_other_passes():
    """Detection 1's best GT (row 0, IoU 15/17) is taken by detection 0; its
    IoU with row 1 (13/19) would pass 0.5: still a FP."""
    return ([D([0, 0, 16, 16, 0.9, 0], [1, 0, 17, 16, 0.8, 0])],
            [G([0, 0, 0, 16, 16], [0, 4, 0, 20, 16])])


def low_iou_does_not_consume():
    """Detection 0 (conf 0.9) has IoU 0.6 with the GT, detection 1 (0.8) IoU
    0.9: at thresholds <= 0.6 detection 0 takes the row, above it does not
    and detection 1 is the TP up to 0.85 (fp32(0.9) lies below the double 0.9)."""
    return ([D([10, 0, 50, 8, 0.9, 1], [0, 0, 36, 8, 0.8, 1])],
            [G([1, 0, 0, 40, 8], [1, 500, 500, 510, 510])])


# ---------------------------------------------------------------- order edges
def tie_inside_image():
    """Equal confidences in one image, same best GT: the lower row is the TP."""
    box = [0.0, 0.0, 20.0, 20.0]
    return [D([500, 500, 520, 520, 0.5, 0], box + [0.5, 0], box + [0.5, 0])], [G([0] + box)]


def tie_across_images():
    """Equal confidences over two images: image 0's FP precedes image 1's TP
    (AP 0.5 at every threshold; the other order would give 1.0)."""
    box = [0.0, 0.0, 20.0, 20.0]
    return ([D([300, 300, 320, 320, 0.5, 0]), D(box + [0.5, 0])],
            [np.zeros((0, 5), F32), G([0] + box)])


# ---------------------------------------------------------------- count edges
def count_edges(max_det=6):
    """Images with no detection, no GT, neither; one with counts == max_det;
    class 3 only in the detections, class 4 only in GT."""
    box = [0.0, 0.0, 20.0, 20.0]
    full = D(*[[20.0 * k, 0, 20.0 * k + 20, 20, 0.9 - 0.1 * k, k % 2] for k in range(max_det)])
    dets = [np.zeros((0, 6), F32), D(box + [0.7, 0], box + [0.6, 3]), np.zeros((0, 6), F32), full]
    tgts = [G([0] + box, [4] + box), np.zeros((0, 5), F32), np.zeros((0, 5), F32),
            G([0, 0, 0, 20, 20], [1, 20, 0, 40, 20], [0, 41, 0, 59, 20])]
    return dets, tgts


# ---------------------------------------------------------------- AP edges
def all_tp_all_fp():
    """Class 0: every detection an exact GT copy (AP ~ 1); class 1: every
    detection far from its GT (AP 0)."""
    dets, tgts = [], []
    for i in range(5):
        g = G([0, 0, 0, 30, 30], [0, 50, 0, 80, 30], [1, 0, 100, 30, 130])
        d = D([0, 0, 30, 30, 0.9 - 0.1 * i, 0], [50, 0, 80, 30, 0.85 - 0.1 * i, 0], [300, 300, 330, 330, 0.8, 1])
        dets.append(d)
        tgts.append(g)
    return dets, tgts
