"""evaluate_mcaq_yolo end to end on the GPU: a random-weight MCAQYOLO, the HIP
NMS decode with the reference's _decode_outputs defaults, the CPU compute_map
on the detections moved to the host.  compute_map itself has no device path:
CUDA tensors raise."""
import math
import os

import pytest
import torch

from mcaq_yolo_amd import evaluation as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-12
REFERENCE_KEYS = ["mAP@0.5", "mAP@0.5:0.95", "avg_inference_time_ms", "std_inference_time_ms", "avg_bits", "std_bits",
                  "min_bits", "max_bits", "compression_ratio", "avg_complexity", "std_complexity"]


def _shift_class_bias(model, x, target, conf):
    """Random weights put every class score below any threshold
    (Detect.bias_init): shift all class biases by one constant so that about
    `target` anchors per image clear `conf`."""
    (y, _), _ = model(x)
    p = y[:, 4:].amax(1).clamp(1e-12, 1 - 1e-7)
    kth = torch.log(p / (1 - p)).topk(target, dim=1).values[:, -1]
    delta = float(math.log(conf / (1 - conf)) - kth.median()) + 1e-3
    for seq in model.model.model[-1].cv3:
        seq[-1].bias.add_(delta)


def test_compute_map_refuses_cuda_tensors():
    with pytest.raises(RuntimeError, match="no device path"):
        E.compute_map([torch.zeros(1, 6, device=DEV)], [torch.zeros(1, 5)])
    with pytest.raises(RuntimeError):
        E.evaluate_mcaq_yolo(torch.nn.Identity(), [], device="cpu")


def test_evaluate_mcaq_yolo_end_to_end(monkeypatch, tmp_path):
    from mcaq_yolo_amd import postprocess
    from mcaq_yolo_amd.yolo import MCAQYOLO
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(0)
        model = MCAQYOLO("yolov8n", grid_size=8, bit_mapping="linear", device=DEV).eval()
        g = torch.Generator().manual_seed(7)
        imgs = [torch.rand(2, 3, 256, 256, generator=g) for _ in range(2)]
        batches = []
        with torch.no_grad():
            _shift_class_bias(model, imgs[0].to(DEV), 400, 0.001)
            for x in imgs:                                     # synthetic targets: some of the model's own boxes
                (y, _), _ = model(x.to(DEV))
                out, cnt = postprocess.nms_padded(y, 0.001, 0.65, 300)
                out, cnt = out.cpu(), cnt.cpu()
                cls, box, bidx = [], [], []
                for b in range(2):
                    for r in range(0, int(cnt[b]), 37):
                        x1, y1, x2, y2 = out[b, r, :4].tolist()
                        box.append([(x1 + x2) / 512, (y1 + y2) / 512, (x2 - x1) / 256, (y2 - y1) / 256])
                        cls.append([float(out[b, r, 5])])
                        bidx.append(float(b))
                batches.append({"img": x, "cls": torch.tensor(cls).reshape(-1, 1),
                                "bboxes": torch.tensor(box).reshape(-1, 4), "batch_idx": torch.tensor(bidx)})
        seen = []
        real = postprocess.nms_padded

        def spy(*a, **k):
            out, cnt = real(*a, **k)
            seen.append((out.clone(), cnt.clone(), k))
            return out, cnt

        monkeypatch.setattr(postprocess, "nms_padded", spy)
        path = str(tmp_path / "eval" / "results.json")
        res = E.evaluate_mcaq_yolo(model, batches, device=DEV, save_results=path)
    finally:
        torch.backends.cudnn.deterministic = det
    assert list(res) == REFERENCE_KEYS and os.path.exists(path)
    assert all(k == {"conf_thres": 0.001, "iou_thres": 0.65, "max_det": 300} for _, _, k in seen) and len(seen) == 2
    dets, tgts = [], []
    for (out, cnt, _), batch in zip(seen, batches):
        dets += [out[b, :int(cnt[b])].cpu() for b in range(2)]
        tgts += E.extract_targets_per_image(batch, 2, 256, 256)
    assert sum(len(d) for d in dets) > 100 and sum(len(t) for t in tgts) > 4
    ref = E.compute_map(dets, tgts)
    assert abs(res["mAP@0.5"] - ref["mAP@0.5"]) <= TOL and abs(res["mAP@0.5:0.95"] - ref["mAP@0.5:0.95"]) <= TOL
    assert ref["mAP@0.5"] > 0
    assert res["avg_inference_time_ms"] > 0 and 2 <= res["min_bits"] <= res["avg_bits"] <= res["max_bits"] <= 8
    assert abs(res["compression_ratio"] - 32.0 / res["avg_bits"]) < 1e-12
