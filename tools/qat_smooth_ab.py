"""A/B of the QAT hook train step with the loss's smoothness term
(MCAQHooks.smoothness_loss; train_step.FUSED_SMOOTHNESS) at the BASELINE
config-5 shapes: the hook step bench.py --config 5 builds (bs16, the three
yolov8n scales, forward_features + loss + backward as one HIP graph).

    python tools/qat_smooth_ab.py --parent-tree DIR [--rounds 5] [--reps 60]
                                  [--out profiles/qat_smooth_ab_config5.json]

Legs:
  a    loss = sum(y g) + 0.1 bit budget, this tree
  a'   the same on the build of the parent commit: DIR holds that commit's
       mcaq_yolo_amd package with its own built library (--parent-tree)
  b    a + 0.1 smoothness_loss, fused (FUSED_SMOOTHNESS = True)
  c    a + 0.1 smoothness_loss as torch ops on the step's bit maps
       (FUSED_SMOOTHNESS = False: what a user of the parent writes)

Interleaved rounds on one box: every round starts three child processes, each
under its own `timeout`: this tree with a alone, the parent tree with a'
alone (the same process shape on both sides of that comparison), and this
tree with a, b and c as three graphs replayed alternately (a_joint, b, c:
b - a_joint and c - b are differences inside one process), `--reps` timed
replays a leg.  A child that fails or runs out of time ends the run, nothing
more is started on the GPU.  Per timed replay: a 640 MiB read first (the maps
leave the 256 MiB Infinity Cache), then device events around the replay.  A
leg's figure is the median of its per-round medians; a leg's spread is the
(max - min) of its per-round medians, and the spread the acceptance uses is
the largest of the five.  Last, one more child counts the
device kernels of one eager step of b and of c with torch.profiler (a run of
its own: tracing slows the host)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {5: {"chans": (64, 128, 256), "sizes": ((80, 80), (40, 40), (20, 20)), "grid": 8, "mapper": "mlp"}}
EVICT_BYTES = 640 << 20
LEG_TIMEOUT_S = 240
TAG = "QAT_SMOOTH_AB_RESULT "
LEGS = {"a": (False, True), "b": (True, True), "c": (True, False)}     # smoothness in the loss, FUSED_SMOOTHNESS


def mark(what):
    sys.stderr.write("qat_smooth_ab: %s\n" % what)
    sys.stderr.flush()


def synth(B, C, H, W, seed, dev):
    """bench.py's synthetic feature maps (silu(1.5 randn + 2 up(randn)))."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device="cpu").manual_seed(seed)
    lo = torch.randn(B, C, max(1, H // 8), max(1, W // 8), generator=g)
    hi = torch.randn(B, C, H, W, generator=g)
    up = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
    return F.silu(1.5 * hi + 2.0 * up).contiguous().to(dev)


def make_sides(args, legs):
    """One hooks object, maps and step function per leg, seeded alike."""
    import torch
    from mcaq_yolo_amd import train_step
    from mcaq_yolo_amd.hooks import MCAQHooks
    cfg = CONFIGS[args.config]
    dev = torch.device("cuda:0")
    base = [synth(args.batch, c, h, w, 5000 + i, dev) for i, (c, (h, w)) in enumerate(zip(cfg["chans"], cfg["sizes"]))]
    gen = torch.Generator(device="cpu").manual_seed(77)
    G = [(1e-3 * torch.randn(b.shape, generator=gen)).to(dev) for b in base]
    w_bit = torch.full((), 0.1, device=dev)
    sides = {}
    for leg in legs:
        smooth, fused = LEGS[leg]
        torch.manual_seed(0)
        h = MCAQHooks(grid_size=cfg["grid"], bit_mapping=cfg["mapper"], device=dev).train()
        h.target_bits = 4.0
        feats = [b.clone().requires_grad_(True) for b in base]

        def step(h=h, feats=feats, smooth=smooth, fused=fused):
            if hasattr(train_step, "FUSED_SMOOTHNESS"):      # the parent's package has no such switch
                train_step.FUSED_SMOOTHNESS = fused
            for p in h.parameters():
                p.grad = None
            for f in feats:
                f.grad = None
            outs, aux = h.forward_features(feats, temperature=1.0)
            heads, grads = list(outs) + [h.bit_budget_loss(aux, 4.0)], list(G) + [w_bit]
            if smooth:
                heads.append(h.smoothness_loss(aux))
                grads.append(w_bit)
            torch.autograd.backward(heads, grads)
        sides[leg] = {"h": h, "feats": feats, "step": step}
    return sides


def leg_time(args, legs):
    import torch
    sides = make_sides(args, legs)
    dev = torch.device("cuda:0")
    evict = torch.ones(EVICT_BYTES // 4, device=dev)
    # every eager step on ONE side stream, as in bench.py (the capture below
    # must not touch the default stream)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mark("eager steps")
        for leg in legs:
            for _ in range(args.warmup):
                sides[leg]["step"]()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for leg in legs:
        mark("capture " + leg)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            sides[leg]["step"]()
        sides[leg]["graph"] = graph
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
    mark("timed replays")
    st = torch.cuda.current_stream()
    ev = [(leg, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.reps) for leg in legs]
    for leg, a, b in ev:
        torch.sum(evict)
        a.record(st)
        sides[leg]["graph"].replay()
        b.record(st)
    torch.cuda.synchronize()
    res = {}
    for leg in legs:
        us = sorted(a.elapsed_time(b) * 1e3 for k, a, b in ev if k == leg)
        res[leg] = {"median_us": round(statistics.median(us), 3), "min_us": round(us[0], 3),
                    "p10_us": round(us[len(us) // 10], 3), "p90_us": round(us[(9 * len(us)) // 10], 3)}
    return res


def leg_count(args, legs):
    """Device kernels of one eager step per leg (torch.profiler)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    sides = make_sides(args, legs)
    res = {}
    for leg in legs:
        step = sides[leg]["step"]
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and
                 not e.name.lower().startswith(("memcpy", "memset", "copybuffer", "fillbuffer"))]
        native = sum(1 for n in names if "mcaq" in n)
        res[leg] = {"kernels": len(names), "native_kernels": native, "other_kernels": len(names) - native}
    return res


def child(script_args, tree, leg, legs):
    """One leg in a child process that imports mcaq_yolo_amd from `tree`."""
    cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S), sys.executable, os.path.abspath(__file__),
           "--leg", leg, "--legs", ",".join(legs), "--tree", tree] + script_args
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("qat_smooth_ab: leg %s of %s ended with status %d; nothing more started" %
                         (leg, tree, p.returncode))
    return json.loads(line[-1][len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=5, choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="directory holding the parent commit's built mcaq_yolo_amd")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(internal) run in this process: time|count")
    ap.add_argument("--legs", default=None, help="(internal) the legs of this process")
    ap.add_argument("--tree", default=None, help="(internal) import mcaq_yolo_amd from here")
    args = ap.parse_args()
    if args.leg:
        sys.path.insert(0, os.path.abspath(args.tree))
        import torch
        import mcaq_yolo_amd
        assert os.path.dirname(os.path.dirname(os.path.abspath(mcaq_yolo_amd.__file__))) == os.path.abspath(args.tree)
        if not torch.cuda.is_available():
            raise SystemExit("qat_smooth_ab: no GPU (a measurement does not fall back)")
        r = (leg_time if args.leg == "time" else leg_count)(args, args.legs.split(","))
        print(TAG + json.dumps(r), flush=True)
        return
    if not args.parent_tree or not os.path.isdir(os.path.join(args.parent_tree, "mcaq_yolo_amd")):
        ap.error("--parent-tree must hold the parent commit's mcaq_yolo_amd package (built)")
    parent = os.path.abspath(args.parent_tree)
    out = args.out or os.path.join(ROOT, "profiles", "qat_smooth_ab_config%d.json" % args.config)
    passthrough = []
    for k in ("config", "batch", "reps", "warmup"):
        passthrough += ["--" + k, str(getattr(args, k))]
    rounds = {"a": [], "a_parent": [], "a_joint": [], "b": [], "c": []}
    detail = []
    for r in range(args.rounds):
        alone = child(passthrough, ROOT, "time", ["a"])
        there = child(passthrough, parent, "time", ["a"])
        here = child(passthrough, ROOT, "time", ["a", "b", "c"])
        detail.append({"this_tree_a": alone, "parent_a": there, "this_tree_abc": here})
        rounds["a"].append(alone["a"]["median_us"])
        rounds["a_parent"].append(there["a"]["median_us"])
        rounds["a_joint"].append(here["a"]["median_us"])
        for k in ("b", "c"):
            rounds[k].append(here[k]["median_us"])
        print("round", r, {k: v[-1] for k, v in rounds.items()}, flush=True)
    med = {k: round(statistics.median(v), 3) for k, v in rounds.items()}
    leg_spread = {k: round(max(v) - min(v), 3) for k, v in rounds.items()}
    spread = max(leg_spread.values())
    cfg = CONFIGS[args.config]
    doc = {"config": args.config, "B": args.batch, "chans": list(cfg["chans"]), "sizes": [list(s) for s in cfg["sizes"]],
           "rounds": args.rounds, "reps": args.reps,
           "what": "QAT hook train step (forward_features + loss + backward, the three scales, one HIP graph per leg); "
                   "a: bit budget only, this tree, a process of its own; a_parent: the same on the parent commit's "
                   "build, a process of its own; a_joint / b / c: bit budget only / + smoothness fused / + smoothness "
                   "as torch ops (FUSED_SMOOTHNESS = False), this tree, three graphs replayed alternately in one "
                   "process.  Per round the three processes in turn, %d timed replays a leg, a %d MiB read before "
                   "every timed replay, device events around the replay; median_us: the median of the per-round "
                   "medians; spread_us: the largest (max - min) of the per-round medians over the five legs"
                   % (args.reps, EVICT_BYTES >> 20),
           "median_us": med, "per_round_median_us": rounds, "per_leg_spread_us": leg_spread,
           "spread_us": spread,
           "a_minus_a_parent_us": round(med["a"] - med["a_parent"], 3),
           "b_minus_a_us": round(med["b"] - med["a_joint"], 3),
           "c_minus_b_us": round(med["c"] - med["b"], 3),
           "a_no_slower_than_parent_beyond_spread": bool(med["a"] - med["a_parent"] <= spread),
           "b_faster_than_c_beyond_spread": bool(med["c"] - med["b"] > spread),
           "rounds_detail": detail}
    try:
        doc["launches_per_eager_step"] = child(passthrough, ROOT, "count", ["b", "c"])
    except SystemExit as e:           # the timing stands; the count is reported as missing
        doc["launches_per_eager_step"] = {"error": str(e)}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("median_us", "per_leg_spread_us", "spread_us", "a_minus_a_parent_us", "b_minus_a_us",
                                          "c_minus_b_us", "launches_per_eager_step")}))
    print("wrote", out)


if __name__ == "__main__":
    main()
