"""A/B of the eval hook step with percentile calibration
(MCAQHooks(calibration_mode="percentile"), csrc/mcaq_pct.h) at the BASELINE
config-2 shapes: bs32, the three yolov8n scales, forward_features in eval mode
as one HIP graph per leg.

    python tools/percentile_ab.py --parent-tree DIR [--rounds 5] [--reps 60]
                                  [--out profiles/percentile_ab_config2.json]
    python tools/percentile_ab.py --trace-summary STATS.csv
                                  [--out profiles/percentile_kernel_trace_config2.json]

Legs:
  a    minmax mode, this tree
  a'   minmax mode on the build of the parent commit: DIR holds that commit's
       mcaq_yolo_amd package with its own built library (--parent-tree)
  b    percentile mode, native (the mcaq_percentile launches inside the step)
  c    percentile mode as a user of the parent writes it: torch.quantile on
       the device over x.transpose(0, 1).flatten(1), copied into the
       quantizer's running statistics, which are frozen (the frozen-statistics
       route of the minmax hooks).  The six torch.quantile calls run eagerly
       in front of the graph replay, inside the timed region: a HIP graph
       holding torch's sort (rocprim onesweep) faulted on replay here, so it is
       never captured

Interleaved rounds on one box: every round starts three child processes, each
under its own `timeout`: this tree with a alone, the parent tree with a'
alone (the same process shape on both sides of that comparison), and this
tree with a, b and c as three graphs replayed alternately.  A child that
fails or runs out of time ends the run, nothing more is started on the GPU.
Per timed replay: a 640 MiB read first (the maps leave the 256 MiB Infinity
Cache), then device events around the replay.  A leg's figure is the median
of its per-round medians; a leg's spread is the (max - min) of its per-round
medians, and the spread the acceptance uses is the largest of them.

Kernel times: run `--leg trace` (eager percentile launches on the three maps)
under `rocprofv3 --kernel-trace --stats`, a run of its own, and hand the
kernel stats CSV to --trace-summary: per new kernel the mean time a launch
and, for the level kernels (which read x once each), 4 B C H W / t."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {2: {"batch": 32, "chans": (64, 128, 256), "sizes": ((80, 80), (40, 40), (20, 20)), "grid": 8,
               "mapper": "mlp"}}
EVICT_BYTES = 640 << 20
LEG_TIMEOUT_S = 240
TAG = "PERCENTILE_AB_RESULT "
PEAK_TBS = 8.0


def mark(what):
    sys.stderr.write("percentile_ab: %s\n" % what)
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


def maps(args, dev):
    cfg = CONFIGS[args.config]
    return [synth(args.batch, c, h, w, 5000 + i, dev) for i, (c, (h, w)) in enumerate(zip(cfg["chans"], cfg["sizes"]))]


def make_sides(args, legs):
    import torch
    from mcaq_yolo_amd.hooks import MCAQHooks
    cfg = CONFIGS[args.config]
    dev = torch.device("cuda:0")
    feats = maps(args, dev)
    sides = {}
    for leg in legs:
        torch.manual_seed(0)
        kw = {"calibration_mode": "percentile"} if leg == "b" else {}     # the parent's hooks have no such keyword
        h = MCAQHooks(grid_size=cfg["grid"], bit_mapping=cfg["mapper"], device=dev, **kw).eval()
        if leg == "c":
            for idx, f in zip(h.backbone_out_indices, feats):
                q = h.quantizers[str(idx)]
                q.running_min = torch.zeros(1, f.shape[1], 1, 1, device=dev)
                q.running_max = torch.ones(1, f.shape[1], 1, 1, device=dev)
                q.freeze_calibration()
                q._frozen()

        def pre(h=h):
            # eager, never captured: torch.quantile sorts with rocprim's onesweep radix sort, and a HIP
            # graph that holds that sort faulted on replay (illegal memory access in its iteration kernel)
            with torch.no_grad():
                for idx, f in zip(h.backbone_out_indices, feats):
                    q = h.quantizers[str(idx)]
                    rows = f.transpose(0, 1).flatten(1)
                    q.running_min.view(-1).copy_(torch.quantile(rows, 0.01 / 100, dim=1))
                    q.running_max.view(-1).copy_(torch.quantile(rows, 99.99 / 100, dim=1))

        def step(h=h):
            with torch.no_grad():
                return h.forward_features(feats, temperature=1.0)[0]
        sides[leg] = {"h": h, "step": step, "pre": pre if leg == "c" else None}
    return sides


def leg_time(args, legs):
    import torch
    sides = make_sides(args, legs)
    dev = torch.device("cuda:0")
    evict = torch.ones(EVICT_BYTES // 4, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mark("eager steps")
        for leg in legs:
            for _ in range(args.warmup):
                if sides[leg]["pre"]:
                    sides[leg]["pre"]()
                sides[leg]["step"]()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for leg in legs:
        mark("capture " + leg)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            sides[leg]["out"] = sides[leg]["step"]()
        sides[leg]["graph"] = graph
        for _ in range(3):
            if sides[leg]["pre"]:
                sides[leg]["pre"]()
            graph.replay()
        torch.cuda.synchronize()
    same = None
    if "b" in legs and "c" in legs:
        # do the two percentile legs quantize with the same ranges?  (recorded, not required: the device
        # torch.quantile may round its interpolation differently from the CPU's)
        same = all(bool(torch.equal(yb, yc)) for yb, yc in zip(sides["b"]["out"], sides["c"]["out"]))
    mark("timed replays")
    st = torch.cuda.current_stream()
    ev = [(leg, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.reps) for leg in legs]
    for leg, a, b in ev:
        torch.sum(evict)
        a.record(st)
        if sides[leg]["pre"]:
            sides[leg]["pre"]()
        sides[leg]["graph"].replay()
        b.record(st)
    torch.cuda.synchronize()
    res = {}
    for leg in legs:
        us = sorted(a.elapsed_time(b) * 1e3 for k, a, b in ev if k == leg)
        res[leg] = {"median_us": round(statistics.median(us), 3), "min_us": round(us[0], 3),
                    "p10_us": round(us[len(us) // 10], 3), "p90_us": round(us[(9 * len(us)) // 10], 3)}
    if same is not None:
        res["b_equals_c"] = same
    return res


def leg_trace(args, legs):
    """Eager percentile launches on the three maps, for a kernel trace."""
    import torch
    from mcaq_yolo_amd import core
    dev = torch.device("cuda:0")
    feats = maps(args, dev)
    evict = torch.ones(EVICT_BYTES // 4, device=dev)
    for _ in range(args.reps):
        for f in feats:
            torch.sum(evict)
            core.channel_percentiles(f, 0.01 / 100, 99.99 / 100)
    torch.cuda.synchronize()
    return {"launch_sets": args.reps, "shapes": [list(f.shape) for f in feats]}


def trace_summary(args):
    """Kernel stats CSV of a `--leg trace` run -> per-kernel times and the
    level kernels' achieved read bandwidth.  The stats rows are per kernel
    name over all three maps, so the bandwidth is total bytes / total time."""
    cfg = CONFIGS[args.config]
    total_bytes = sum(4 * args.batch * c * h * w for c, (h, w) in zip(cfg["chans"], cfg["sizes"]))
    rows = []
    with open(args.trace_summary) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "mcaq_pct" not in name:
                continue
            calls = int(r["Calls"])
            total_ns = float(r["TotalDurationNs"])
            sets = calls / 3.0
            row = {"kernel": name.split("(")[0], "calls": calls, "mean_us_per_launch": round(total_ns / calls / 1e3, 3),
                   "us_per_step_three_maps": round(total_ns / sets / 1e3, 3)}
            if "level_kernel" in name:
                tbs = total_bytes / (total_ns / sets * 1e-9) / 1e12
                row["read_TBps"] = round(tbs, 3)
                row["of_peak"] = round(tbs / PEAK_TBS, 3)
            rows.append(row)
    doc = {"config": args.config, "B": args.batch, "bytes_read_per_level_three_maps": total_bytes,
           "peak_TBps": PEAK_TBS,
           "what": "rocprofv3 --kernel-trace --stats of eager mcaq_percentile launches on the three config-2 maps "
                   "(a 640 MiB read before each); read_TBps = 4 B C H W summed over the maps / the kernel's time "
                   "summed over the maps",
           "kernels": rows,
           "us_per_step_all_new_kernels": round(sum(r["us_per_step_three_maps"] for r in rows), 3)}
    out = args.out or os.path.join(ROOT, "profiles", "percentile_kernel_trace_config%d.json" % args.config)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    print("wrote", out)


def child(script_args, tree, leg, legs):
    """One leg in a child process that imports mcaq_yolo_amd from `tree`."""
    cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S), sys.executable, os.path.abspath(__file__),
           "--leg", leg, "--legs", ",".join(legs), "--tree", tree] + script_args
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(TAG)]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("percentile_ab: leg %s of %s ended with status %d; nothing more started" %
                         (leg, tree, p.returncode))
    return json.loads(line[-1][len(TAG):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="directory holding the parent commit's built mcaq_yolo_amd")
    ap.add_argument("--trace-summary", default=None, help="kernel stats CSV of a --leg trace run under rocprofv3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(internal) run in this process: time|trace")
    ap.add_argument("--legs", default="b", help="(internal) the legs of this process")
    ap.add_argument("--tree", default=ROOT, help="(internal) import mcaq_yolo_amd from here")
    args = ap.parse_args()
    if args.batch is None:
        args.batch = CONFIGS[args.config]["batch"]
    if args.trace_summary:
        return trace_summary(args)
    if args.leg:
        sys.path.insert(0, os.path.abspath(args.tree))
        import torch
        import mcaq_yolo_amd
        assert os.path.dirname(os.path.dirname(os.path.abspath(mcaq_yolo_amd.__file__))) == os.path.abspath(args.tree)
        if not torch.cuda.is_available():
            raise SystemExit("percentile_ab: no GPU (a measurement does not fall back)")
        r = (leg_time if args.leg == "time" else leg_trace)(args, args.legs.split(","))
        print(TAG + json.dumps(r), flush=True)
        return
    if not args.parent_tree or not os.path.isdir(os.path.join(args.parent_tree, "mcaq_yolo_amd")):
        ap.error("--parent-tree must hold the parent commit's mcaq_yolo_amd package (built)")
    parent = os.path.abspath(args.parent_tree)
    out = args.out or os.path.join(ROOT, "profiles", "percentile_ab_config%d.json" % args.config)
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
           "what": "eval hook step (forward_features, the three scales, one HIP graph per leg); a: minmax mode, this "
                   "tree, a process of its own; a_parent: the same on the parent commit's build, a process of its "
                   "own; a_joint / b / c: minmax / percentile native / percentile by eager torch.quantile into "
                   "frozen statistics + the graph, this tree, three graphs replayed alternately in one process.  Per round the three "
                   "processes in turn, %d timed replays a leg, a %d MiB read before every timed replay, device "
                   "events around the replay; median_us: the median of the per-round medians; spread_us: the "
                   "largest (max - min) of the per-round medians over the five legs" % (args.reps, EVICT_BYTES >> 20),
           "median_us": med, "per_round_median_us": rounds, "per_leg_spread_us": leg_spread,
           "spread_us": spread,
           "a_minus_a_parent_us": round(med["a"] - med["a_parent"], 3),
           "a_parent_spread_us": leg_spread["a_parent"],
           "b_minus_a_us": round(med["b"] - med["a_joint"], 3),
           "c_minus_b_us": round(med["c"] - med["b"], 3),
           "a_within_a_parent_spread": bool(med["a"] - med["a_parent"] <= leg_spread["a_parent"]),
           "b_faster_than_c_beyond_spread": bool(med["c"] - med["b"] > spread),
           "rounds_detail": detail}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("median_us", "per_leg_spread_us", "spread_us", "a_minus_a_parent_us",
                                          "b_minus_a_us", "c_minus_b_us", "a_within_a_parent_spread",
                                          "b_faster_than_c_beyond_spread")}))
    print("wrote", out)


if __name__ == "__main__":
    main()
