"""A/B of the QAT hook train step on fp16 / bf16 feature maps: the native route
(train_step.HALF_NATIVE = True: pass 1 and the QAT quantizer read the half
maps as they are, grad_x comes back in the map's dtype) against the upcast
route (False: x.float() copies), at the BASELINE config-5 shapes.

    python tools/qat_amp_ab.py [--config 5] [--batch 16] [--reps 48] [--block 12]
                               [--dtypes f16,bf16] [--out profiles/qat_amp_ab_config5.json]

Two legs per dtype, each a child process under its own `timeout` (a leg that
fails or runs out of time ends the run: nothing more is started on the GPU):

  step     forward_features + loss + backward of the three hook scales as one
           HIP graph per setting (its own hooks, maps and graph, seeded alike),
           the two graphs replayed alternately in one process.  Per timed
           replay: a 640 MiB read first (the maps leave the 256 MiB Infinity
           Cache), then device events around the replay.  Block medians over
           `--block` replays; the margin is the spread (max - min) of the
           upcast route's block medians.  Also: the peak
           torch.cuda.max_memory_allocated of three eager steps of each
           setting, and a bit-for-bit comparison of the two settings' outputs
           and map gradients.
  kernels  the QAT forward and backward dispatches alone (the three scales in
           one launch, gm = gb = NULL as in the fused step), fp32 x against
           half x, alternating, timed by mcaq_time_launch (the dispatch's own
           start and end), the same eviction before every timed dispatch.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {5: {"chans": (64, 128, 256), "sizes": ((80, 80), (40, 40), (20, 20)), "grid": 8, "mapper": "mlp"}}
EVICT_BYTES = 640 << 20
LEG_TIMEOUT_S = 240


def summary(us, block):
    us = list(us)
    blocks = [statistics.median(us[i:i + block]) for i in range(0, len(us) - block + 1, block)]
    s = sorted(us)
    return {"median_us": round(statistics.median(us), 3), "min_us": round(s[0], 3),
            "p10_us": round(s[len(s) // 10], 3), "p90_us": round(s[(9 * len(s)) // 10], 3),
            "block_medians_us": [round(b, 3) for b in blocks],
            "block_spread_us": round(max(blocks) - min(blocks), 3)}


def mark(what):
    """Progress of a leg on stderr (the driver shows its tail when a leg fails)."""
    sys.stderr.write("qat_amp_ab: %s\n" % what)
    sys.stderr.flush()


def synth(B, C, H, W, seed, dtype, dev):
    """bench.py's synthetic feature maps (silu(1.5 randn + 2 up(randn)))."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device="cpu").manual_seed(seed)
    lo = torch.randn(B, C, max(1, H // 8), max(1, W // 8), generator=g)
    hi = torch.randn(B, C, H, W, generator=g)
    up = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
    return F.silu(1.5 * hi + 2.0 * up).to(dtype).contiguous().to(dev)


def leg_step(args, dtype):
    import torch
    from mcaq_yolo_amd import train_step
    from mcaq_yolo_amd.hooks import MCAQHooks
    cfg = CONFIGS[args.config]
    dev = torch.device("cuda:0")
    B = args.batch
    base = [synth(B, c, h, w, 5000 + i, dtype, dev) for i, (c, (h, w)) in enumerate(zip(cfg["chans"], cfg["sizes"]))]
    gen = torch.Generator(device="cpu").manual_seed(77)
    G = [(1e-3 * torch.randn(b.shape, generator=gen)).to(dev) for b in base]
    w_bit = torch.full((), 0.1, device=dev)
    evict = torch.ones(EVICT_BYTES // 4, device=dev)
    sides = {}
    for native in (False, True):
        torch.manual_seed(0)
        h = MCAQHooks(grid_size=cfg["grid"], bit_mapping=cfg["mapper"], device=dev).train()
        h.target_bits = 4.0
        feats = [b.clone().requires_grad_(True) for b in base]
        last = {}

        def step(h=h, feats=feats, native=native, last=last):
            train_step.HALF_NATIVE = native
            for p in h.parameters():
                p.grad = None
            for f in feats:
                f.grad = None
            outs, aux = h.forward_features(feats, temperature=1.0)
            if last.get("keep"):         # values only: no autograd graph outlives its step
                last["outs"] = [o.detach().clone() for o in outs]
            lbit = h.bit_budget_loss(aux, 4.0)
            torch.autograd.backward(list(outs) + [lbit], list(G) + [w_bit])
        sides[native] = {"h": h, "feats": feats, "step": step, "last": last}
    res = {"equal_outputs_and_map_grads": True}
    # Every eager step runs on ONE side stream, as in bench.py: a step on the
    # default stream would leave AccumulateGrad nodes tied to it, and the
    # capture below must not touch the default stream.
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mark("eager steps")
        # one step each from the same state: the values must not differ
        for native in (False, True):
            sides[native]["last"]["keep"] = True
            sides[native]["step"]()
            sides[native]["last"]["keep"] = False
        torch.cuda.synchronize()
        for a, b in zip(sides[False]["last"]["outs"], sides[True]["last"]["outs"]):
            res["equal_outputs_and_map_grads"] &= bool(torch.equal(a, b))
        for a, b in zip(sides[False]["feats"], sides[True]["feats"]):
            res["equal_outputs_and_map_grads"] &= bool(a.grad.dtype == b.grad.dtype == dtype and
                                                       torch.equal(a.grad, b.grad))
        # peak memory of eager steps, per setting
        for native in (False, True):
            s = sides[native]
            s["last"].pop("outs", None)
            for f in s["feats"]:
                f.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            for _ in range(3):
                s["step"]()
            torch.cuda.synchronize()
            s["peak"] = {"max_memory_allocated_bytes": torch.cuda.max_memory_allocated(),
                         "allocated_before_bytes": before,
                         "step_peak_above_before_bytes": torch.cuda.max_memory_allocated() - before}
        for native in (False, True):
            for _ in range(args.warmup):
                sides[native]["step"]()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # one graph per setting
    for native in (False, True):
        s = sides[native]
        run = s["step"]
        if not args.eager:
            mark("capture, HALF_NATIVE = %s" % native)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                s["step"]()
            s["graph"] = graph
            run = graph.replay
        s["run"] = run
        mark("first replays, HALF_NATIVE = %s" % native)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
    mark("timed replays")
    st = torch.cuda.current_stream()
    times = {False: [], True: []}
    ev = [(native, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.reps) for native in (False, True)]
    for native, a, b in ev:
        torch.sum(evict)
        a.record(st)
        sides[native]["run"]()
        b.record(st)
        if args.eager:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    for native, a, b in ev:
        times[native].append(a.elapsed_time(b) * 1e3)
    for native, key in ((False, "upcast"), (True, "native")):
        res[key] = summary(times[native], args.block)
        res[key].update(sides[native]["peak"])
    res["native_over_upcast"] = round(res["native"]["median_us"] / res["upcast"]["median_us"], 4)
    res["margin_us"] = res["upcast"]["block_spread_us"]
    res["faster_beyond_margin"] = bool(res["upcast"]["median_us"] - res["native"]["median_us"] > res["margin_us"])
    res["hip_graph"] = not args.eager
    return res


def leg_kernels(args, dtype):
    import torch
    from mcaq_yolo_amd import abi, core
    cfg = CONFIGS[args.config]
    dev = torch.device("cuda:0")
    B = args.batch
    L = abi.lib()
    st = torch.cuda.current_stream()
    sh = ctypes.c_void_p(st.cuda_stream)
    xh = [synth(B, c, h, w, 5000 + i, dtype, dev) for i, (c, (h, w)) in enumerate(zip(cfg["chans"], cfg["sizes"]))]
    gen = torch.Generator(device="cpu").manual_seed(77)
    G = [(1e-3 * torch.randn(x.shape, generator=gen)).to(dev) for x in xh]
    grids = [core._tile_grid(h, w, cfg["grid"]) for (h, w) in cfg["sizes"]]
    bits = [torch.rand(B, ht, wt, device=dev) * 6 + 2 for (ht, wt) in grids]
    ms = [torch.rand(B, h, w, device=dev) * 0.1 + 0.9 for (h, w) in cfg["sizes"]]
    mm = [core._channel_minmax(x.float()) for x in xh]
    evict = torch.ones(EVICT_BYTES // 4, device=dev)
    arrs, keep = {}, []
    for key, xs in (("fp32_x", [x.float() for x in xh]), ("half_x", xh)):
        arr = (abi.QatScale * 3)()
        for i, x in enumerate(xs):
            y = torch.empty(x.shape, device=dev)
            gx = torch.empty_like(x)
            work = torch.empty(L.mcaq_qat_work_floats(*x.shape), device=dev)
            q = core._qat_struct(x, bits[i], ms[i], mm[i][0], mm[i][1])
            q.g, q.y, q.gx, q.work = core._p(G[i]), core._p(y), core._p(gx), core._p(work)
            arr[i] = q
            keep += [x, y, gx, work]
        arrs[key] = arr
    res = {}
    for name, fn in (("qat_forward", L.mcaq_qat_forward), ("qat_backward_kernel", L.mcaq_qat_backward)):
        for key in arrs:                 # warm up: code objects loaded
            for _ in range(3):
                abi.check(fn(arrs[key], 3, sh), name)
        ev = [(key, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(args.reps) for key in arrs]
        for _, a, b in ev:               # create the HIP events
            a.record(st)
            b.record(st)
        torch.cuda.synchronize()
        for key, a, b in ev:
            torch.sum(evict)
            L.mcaq_time_launch(0, ctypes.c_void_p(a.cuda_event), ctypes.c_void_p(b.cuda_event))
            abi.check(fn(arrs[key], 3, sh), name)
        torch.cuda.synchronize()
        res[name] = {key: summary([a.elapsed_time(b) * 1e3 for k, a, b in ev if k == key], args.block)
                     for key in arrs}
        res[name]["half_over_fp32"] = round(res[name]["half_x"]["median_us"] / res[name]["fp32_x"]["median_us"], 4)
    n = sum(x.numel() for x in xh)
    res["elements"] = n
    res["bytes_per_element"] = {"qat_forward": {"fp32_x": 8, "half_x": 6}, "qat_backward_kernel": {"fp32_x": 12, "half_x": 8}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=5, choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=48)
    ap.add_argument("--block", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtypes", default="f16,bf16")
    ap.add_argument("--eager", action="store_true", help="no HIP graphs: events around the eager step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(internal) run one leg in this process: step|kernels")
    ap.add_argument("--dtype", default=None, help="(internal) the leg's dtype")
    args = ap.parse_args()
    if args.reps < args.block or args.block < 1:
        ap.error("--reps must be at least --block")
    if args.leg:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("qat_amp_ab: no GPU (a measurement does not fall back)")
        dtype = {"f16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
        r = (leg_step if args.leg == "step" else leg_kernels)(args, dtype)
        print("QAT_AMP_AB_RESULT " + json.dumps(r), flush=True)
        return
    out = args.out or os.path.join(ROOT, "profiles", "qat_amp_ab_config%d.json" % args.config)
    cfg = CONFIGS[args.config]
    doc = {"config": args.config, "B": args.batch, "chans": list(cfg["chans"]), "sizes": [list(s) for s in cfg["sizes"]],
           "reps": args.reps, "block": args.block,
           "what": "QAT hook train step (forward_features + loss + backward, the three scales) on half maps, "
                   "train_step.HALF_NATIVE False (upcast: the baseline) against True (native), one HIP graph per "
                   "setting replayed alternately in one process, %d replays each, a %d MiB read before every "
                   "timed replay, device events around the replay, block medians over %d replays, margin = spread of "
                   "the upcast route's block medians; kernels: the QAT forward / backward dispatch alone (three "
                   "scales in one launch) by mcaq_time_launch, fp32 x against half x, alternating"
                   % (args.reps, EVICT_BYTES >> 20, args.block)}
    passthrough = []
    for k in ("config", "batch", "reps", "block", "warmup"):
        passthrough += ["--" + k, str(getattr(args, k))]
    if args.eager:
        passthrough.append("--eager")
    for dt in args.dtypes.split(","):
        for leg in ("step", "kernels"):
            cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S), sys.executable, os.path.abspath(__file__),
                   "--leg", leg, "--dtype", dt] + passthrough
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("QAT_AMP_AB_RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit("qat_amp_ab: leg %s %s ended with status %d; nothing more started" %
                                 (leg, dt, p.returncode))
            doc.setdefault(dt, {})[leg] = json.loads(line[-1][len("QAT_AMP_AB_RESULT "):])
            print(dt, leg, json.dumps(doc[dt][leg])[:400], flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
