"""mAP evaluation: the reference's `utils/evaluation.py` driver on this package.

`compute_map`, `extract_targets_per_image`, `cxcywh_norm_to_xyxy_pixels` and
`evaluate_mcaq_yolo` keep the reference's names, argument names, defaults and
result keys (mcaq_yolo/utils/evaluation.py:36-307); the algorithm is restated,
not copied.

The matching rule (evaluation.py:156-174), per IoU threshold and class, walks
the class's detections in confidence order; each takes its best ground truth
(GT: the first argmax of `box_iou` over the image's same-class rows) and is a
true positive (TP) iff that IoU reaches the threshold and the row is still
unmatched.  A detection's best GT depends neither on the threshold nor on
what is matched, so the TP of a (GT row, threshold) pair is the FIRST
detection in order whose best GT is that row with IoU >= threshold; every
other detection pointing at the row is a false positive - also when another
row would pass.  Nothing is sequential: compute_map here is vectorised
numpy with no per-detection Python loop.

  * IoU: ultralytics `box_iou` in fp32, inter / (area_a + area_b - inter +
    1e-7), compared with the threshold in double.
  * order: confidence descending, ties by (image, row) ascending (the
    reference's stable sort over records appended image by image).
  * classes: GT classes | detected classes; a class without GT or without
    detections has AP 0.0 and counts in the mean.  Class ids are integer
    values.
  * NaN / inf confidences or coordinates are outside the contract: the NMS
    never emits them and the reference's sort is undefined on them.

compute_map has no device path yet: it takes CPU tensors and raises on CUDA
tensors (no silent copy).  evaluate_mcaq_yolo decodes on
the device with the HIP NMS and moves each batch's detections to the host, as
the reference does.

Batch-sharded evaluation needs no new collective: a rank evaluates the output
of `postprocess.gather_detections` (and its targets, gathered the same way).
"""
import json
import os

import numpy as np
import torch

F32 = np.float32


def _default_thresholds():
    return np.linspace(0.5, 0.95, 10).tolist()


# ---------------------------------------------------------------- targets
def cxcywh_norm_to_xyxy_pixels(boxes, img_w, img_h):
    """Normalised (cx, cy, w, h) -> pixel (x1, y1, x2, y2), fp32."""
    b = boxes.clone().float()
    cx, cy, w, h = b[:, 0] * img_w, b[:, 1] * img_h, b[:, 2] * img_w, b[:, 3] * img_h
    return torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dim=1)


def extract_targets_per_image(batch, batch_size, img_w, img_h):
    """Per-image (m, 5) [cls, x1, y1, x2, y2] pixel tensors (CPU) from either
    collate format: ultralytics' ('cls', 'bboxes', 'batch_idx') or the custom
    'labels' ((m, 5) [cls, cx, cy, w, h], one tensor or one per image)."""
    per_image = [torch.zeros(0, 5) for _ in range(batch_size)]
    if isinstance(batch, dict) and "bboxes" in batch and "batch_idx" in batch:
        cls = batch["cls"].reshape(-1).float().cpu()
        boxes = cxcywh_norm_to_xyxy_pixels(batch["bboxes"].cpu().reshape(-1, 4), img_w, img_h)
        bidx = batch["batch_idx"].reshape(-1).long().cpu()
        for i in range(batch_size):
            sel = bidx == i
            if bool(sel.any()):
                per_image[i] = torch.cat([cls[sel].unsqueeze(1), boxes[sel]], dim=1)
    elif isinstance(batch, dict) and "labels" in batch:
        labels = batch["labels"]
        items = labels if isinstance(labels, (list, tuple)) else [labels]
        for i, lab in enumerate(items[:batch_size]):
            lab = lab.cpu().float()
            if lab.numel():
                per_image[i] = torch.cat([lab[:, :1], cxcywh_norm_to_xyxy_pixels(lab[:, 1:5], img_w, img_h)], dim=1)
    return per_image


def pad_targets(per_image, device):
    """Per-image (m, 5) targets -> (B, G, 5) fp32 (zero rows past the count,
    G = the largest m, at least 1) and (B,) int32 counts on `device`."""
    B = len(per_image)
    G = max([1] + [int(t.shape[0]) for t in per_image])
    tgt = torch.zeros(B, G, 5)
    cnt = torch.zeros(B, dtype=torch.int32)
    for i, t in enumerate(per_image):
        m = int(t.shape[0])
        if m:
            tgt[i, :m] = t.detach().float().cpu()
        cnt[i] = m
    return tgt.to(device), cnt.to(device)


# ---------------------------------------------------------------- AP from TP flags (CPU)
def _ap(tp, n_gt, interp):
    """evaluation.py:81-99, 176-180 on one class's TP flags in order."""
    tp_cum = np.cumsum(tp.astype(np.float64))
    fp_cum = np.cumsum(1.0 - tp.astype(np.float64))
    recall = tp_cum / (n_gt + 1e-10)
    precision = tp_cum / (tp_cum + fp_cum + 1e-10)
    r = np.concatenate(([0.0], recall, [1.0]))
    p = np.concatenate(([1.0], precision, [0.0]))
    p = np.maximum.accumulate(p[::-1])[::-1]
    if interp == "coco":
        return float(np.interp(np.linspace(0.0, 1.0, 101), r, p).mean())
    idx = np.where(r[1:] != r[:-1])[0]
    return float(np.sum((r[idx + 1] - r[idx]) * p[idx + 1]))


def _box_iou(a, b):
    """ultralytics box_iou restated in fp32 numpy: a (n, 4) against b (m, 4)."""
    a, b = a.astype(F32)[:, None, :], b.astype(F32)[None, :, :]
    wh = np.maximum(np.minimum(a[..., 2:], b[..., 2:]) - np.maximum(a[..., :2], b[..., :2]), F32(0))
    inter = wh[..., 0] * wh[..., 1]
    aa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    ab = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    return inter / (aa + ab - inter + F32(1e-7))


def match_cpu(detections, targets, iou_thresholds):
    """The matching rule, vectorised: returns (cls, conf, tp, gt_cls) with one
    entry per detection in (image, row) order - tp is (n, T) bool - and the
    class of every GT row."""
    cls_l, conf_l, gid_l, iou_l, gtc_l = [], [], [], [], []
    gbase = 0
    for det, tgt in zip(detections, targets):
        d = np.asarray(det.detach().cpu().numpy() if torch.is_tensor(det) else det, F32).reshape(-1, 6)
        g = np.asarray(tgt.detach().cpu().numpy() if torch.is_tensor(tgt) else tgt, F32).reshape(-1, 5)
        gtc_l.append(g[:, 0])
        n, m = d.shape[0], g.shape[0]
        gid = np.full(n, -1, np.int64)
        biou = np.full(n, -1.0, F32)
        if n and m:
            iou = np.where(g[None, :, 0] == d[:, None, 5], _box_iou(d[:, :4], g[:, 1:5]), F32(-1))
            best = iou.argmax(1)                                   # the first maximum
            biou = iou[np.arange(n), best]
            gid = np.where(biou >= 0, gbase + best, -1)
        cls_l.append(d[:, 5])
        conf_l.append(d[:, 4])
        gid_l.append(gid)
        iou_l.append(biou)
        gbase += m
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    cls, conf = cat(cls_l, F32), cat(conf_l, F32)
    gid, biou, gt_cls = cat(gid_l, np.int64), cat(iou_l, np.float64), cat(gtc_l, F32)
    n = cls.shape[0]
    order = np.lexsort((np.arange(n), -conf.astype(np.float64)))    # confidence desc, record asc
    tp = np.zeros((n, len(iou_thresholds)), bool)
    for t, thr in enumerate(iou_thresholds):
        cand = order[(gid[order] >= 0) & (biou[order] >= float(thr))]
        _, first = np.unique(gid[cand], return_index=True)          # first passing detection of every GT row
        tp[cand[first], t] = True
    return cls, conf, tp, gt_cls


def _metrics(maps, iou_thresholds):
    out = {"mAP@0.5": float(maps[0]), "mAP@0.5:0.95": float(np.mean(maps))}
    for t, m in zip(iou_thresholds, maps):
        out["mAP@%.2f" % t] = float(m)
    return out


def _compute_map_cpu(detections, targets, iou_thresholds, interp):
    cls, conf, tp, gt_cls = match_cpu(detections, targets, iou_thresholds)
    classes = sorted({int(c) for c in gt_cls.tolist()} | {int(c) for c in cls.tolist()})
    if not classes:
        return {"mAP@0.5": 0.0, "mAP@0.5:0.95": 0.0}
    n = cls.shape[0]
    order = np.lexsort((np.arange(n), -conf.astype(np.float64)))
    ap = np.zeros((len(classes), len(iou_thresholds)))
    for i, c in enumerate(classes):
        n_gt = int((gt_cls == c).sum())
        sel = order[cls[order] == c]
        if n_gt == 0 or sel.size == 0:
            continue
        for t in range(len(iou_thresholds)):
            ap[i, t] = _ap(tp[sel, t], n_gt, interp)
    return _metrics([float(np.mean(ap[:, t])) for t in range(len(iou_thresholds))], iou_thresholds)


def compute_map(detections, targets, iou_thresholds=None, interp="voc"):
    """mAP over a dataset (evaluation.py:102-190).

    detections: per-image (n, 6) tensors [x1, y1, x2, y2, conf, cls] (pixels);
    targets: per-image (m, 5) tensors [cls, x1, y1, x2, y2] (pixels);
    iou_thresholds: default 0.50:0.05:0.95; interp: 'voc' (all-point) or
    'coco' (101-point).  Returns {'mAP@0.5', 'mAP@0.5:0.95', 'mAP@<t:.2f>'
    per threshold}; with no class on either side exactly the two zeros.
    CPU tensors only: CUDA tensors raise (move them with .cpu() first)."""
    if iou_thresholds is None:
        iou_thresholds = _default_thresholds()
    iou_thresholds = [float(t) for t in iou_thresholds]
    if interp not in ("voc", "coco"):
        raise ValueError("interp must be 'voc' or 'coco'")
    if any(torch.is_tensor(t) and t.is_cuda for t in list(detections) + list(targets)):
        raise RuntimeError("compute_map has no device path: pass CPU tensors")
    return _compute_map_cpu(detections, targets, iou_thresholds, interp)


# ---------------------------------------------------------------- model evaluation
def evaluate_mcaq_yolo(model, dataloader, device="cuda", compute_complexity=True, save_results=None, quantize=True):
    """evaluation.py:206-307: mAP, latency, bit statistics, complexity
    statistics and compression ratio of an MCAQYOLO over a dataloader.

    Detections are decoded on the device with postprocess.nms_padded(
    conf_thres=0.001, iou_thres=0.65, max_det=300) (the reference's
    _decode_outputs defaults) and moved to the host batch by batch, as the
    reference moves them; the timing events and the bit / complexity means
    stay on the device and are read once at the end.  The decode is the HIP
    NMS, so `device` must be a CUDA device.

    Batch-sharded use: every rank runs its shard and evaluates
    postprocess.gather_detections(out, counts) (and the targets gathered the
    same way); no further collective is needed."""
    from .postprocess import nms_padded
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("evaluate_mcaq_yolo decodes with the HIP NMS: device must be CUDA")
    model.eval()
    model = model.to(dev)
    dets, tgts, events, bits, cplx = [], [], [], [], []
    print("Running evaluation...")
    with torch.no_grad():
        for batch in dataloader:
            images = batch["img"] if isinstance(batch, dict) else batch[0]
            images = images.to(dev)
            if images.dtype == torch.uint8:
                images = images.float() / 255.0
            B, _, img_h, img_w = images.shape
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            outputs, aux = model(images, temperature=1.0, return_aux=True, quantize=quantize)
            end.record()
            events.append((start, end))
            if "avg_bits" in aux:
                bits.append(aux["avg_bits"].detach().reshape(()).to(torch.float64))
            if compute_complexity and aux.get("complexity_map"):
                cmap = aux["complexity_map"]
                maps = cmap if isinstance(cmap, (list, tuple)) else [cmap]
                cplx.append(torch.stack([m.float().mean() for m in maps]).mean().to(torch.float64))
            out, counts = nms_padded(outputs, conf_thres=0.001, iou_thres=0.65, max_det=300)
            out, counts = out.cpu(), counts.tolist()         # one device->host copy per batch
            dets += [out[b, :counts[b]].clone() for b in range(B)]
            tgts += extract_targets_per_image(batch, B, img_w, img_h)
    torch.cuda.synchronize(dev)
    metrics = compute_map(dets, tgts)
    times = [s.elapsed_time(e) for s, e in events]
    results = {
        "mAP@0.5": metrics["mAP@0.5"],
        "mAP@0.5:0.95": metrics["mAP@0.5:0.95"],
        "avg_inference_time_ms": float(np.mean(times)) if times else 0.0,
        "std_inference_time_ms": float(np.std(times)) if times else 0.0,
    }
    if bits:
        b = torch.stack(bits).cpu().numpy()
        results.update({"avg_bits": float(np.mean(b)), "std_bits": float(np.std(b)),
                        "min_bits": float(np.min(b)), "max_bits": float(np.max(b))})
        results["compression_ratio"] = 32.0 / results["avg_bits"]
    if cplx:
        c = torch.stack(cplx).cpu().numpy()
        results.update({"avg_complexity": float(np.mean(c)), "std_complexity": float(np.std(c))})
    if save_results:
        os.makedirs(os.path.dirname(os.path.abspath(save_results)), exist_ok=True)
        with open(save_results, "w") as f:
            json.dump(results, f, indent=4)
        print("Saved evaluation results to %s" % save_results)
    print("\n" + "=" * 50 + "\nEvaluation Results:\n" + "=" * 50)
    for k, v in results.items():
        print("%-25s: %.4f" % (k, v))
    print("=" * 50 + "\n")
    return results
