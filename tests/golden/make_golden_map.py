"""Generate tests/golden/map_cases.npz from the reference's own compute_map.

Runs only where the reference tree exists (/root/reference); the tests read
the committed .npz.  `mcaq_yolo/utils/evaluation.py` is loaded by FILE PATH
(the _refload.py pattern: the package __init__ imports ultralytics eagerly).

Ultralytics is not installed here, so `ultralytics.utils.metrics.box_iou` is
REPLACED by a torch fp32 restatement of its published formula,
    inter = prod(clamp(min(a2, b2) - max(a1, b1), 0))
    iou   = inter / (area_a + area_b - inter + 1e-7)
and the NMS import by a stub that raises if called (compute_map never calls
it); `tqdm` is stubbed only if it is absent.  Parity of this package's mAP is
therefore pinned to the reference's compute_map WITH A RESTATED box_iou; it
is unpinned against ultralytics itself.

Per scenario of tests/map_cases.fixture_scenarios() the file holds the padded
inputs (`<name>_det`, `_counts`, `_tgt`, `_tcounts`) and, for interp in
(voc, coco) and the threshold sets `default` (0.50:0.05:0.95) and `t50`
([0.5]), `<name>_<interp>_<set>_keys` / `_vals`: the reference's result dict
in its own key order.

    python tests/golden/make_golden_map.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference/mcaq_yolo/utils/evaluation.py"


def box_iou(box1, box2, eps=1e-7):
    (a1, a2), (b1, b2) = box1.float().unsqueeze(1).chunk(2, 2), box2.float().unsqueeze(0).chunk(2, 2)
    inter = (torch.min(a2, b2) - torch.max(a1, b1)).clamp_(0).prod(2)
    return inter / ((a2 - a1).prod(2) + (b2 - b1).prod(2) - inter + eps)


def load_reference():
    def forbidden(*a, **k):  # pragma: no cover - must never fire
        raise RuntimeError("NMS stub called: compute_map must not need it")

    ul = types.ModuleType("ultralytics")
    utils = types.ModuleType("ultralytics.utils")
    metrics = types.ModuleType("ultralytics.utils.metrics")
    nms = types.ModuleType("ultralytics.utils.nms")
    metrics.box_iou = box_iou
    nms.non_max_suppression = forbidden
    ul.utils, utils.metrics, utils.nms = utils, metrics, nms
    for name, mod in (("ultralytics", ul), ("ultralytics.utils", utils), ("ultralytics.utils.metrics", metrics),
                      ("ultralytics.utils.nms", nms)):
        assert name not in sys.modules
        sys.modules[name] = mod
    try:
        import tqdm  # noqa: F401
    except ImportError:
        t = types.ModuleType("tqdm")
        t.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = t
    spec = importlib.util.spec_from_file_location("ref_evaluation", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import map_cases as MC
    ref = load_reference()
    out = {}
    for name, (dets, tgts) in MC.fixture_scenarios().items():
        det, counts, tgt, tcounts = MC.pad(dets, tgts)
        out[name + "_det"], out[name + "_counts"] = det, counts
        out[name + "_tgt"], out[name + "_tcounts"] = tgt, tcounts
        td = [torch.from_numpy(d) for d in dets]
        tt = [torch.from_numpy(t) for t in tgts]
        for interp in ("voc", "coco"):
            for sname, thr in (("default", None), ("t50", [0.5])):
                m = ref.compute_map(td, tt, iou_thresholds=thr, interp=interp)
                out["%s_%s_%s_keys" % (name, interp, sname)] = np.asarray(list(m.keys()))
                out["%s_%s_%s_vals" % (name, interp, sname)] = np.asarray(list(m.values()), np.float64)
                print(name, interp, sname, m["mAP@0.5"], m["mAP@0.5:0.95"], flush=True)
    path = os.path.join(HERE, "map_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
