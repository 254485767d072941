"""tests/optim_cases.py on the CPU: every case builds from its seed with the
expectations its name claims, the numpy restatement of the kernel's
arithmetic meets the per-element rule at M / 2 on every case (so the rule can
be met, with half of it to spare), every case reaches the branch of
csrc/mcaq_optim.h it is there for (predicates computed from the layout), and
the cases discriminate: each mutation of the restatement - a wrong kernel -
misses the rule at the case named for it."""
import numpy as np
import pytest

import optim_cases as oc


@pytest.mark.parametrize("name", oc.NAMES)
def test_case_builds_and_kernel_arith_meets_half_the_rule(name):
    c = oc.case(name)
    print("%s: %s" % (name, c.why))
    assert len(c.sizes) <= oc.MAXSEG and 1 <= len(c.groups) <= oc.MAXGROUPS and min(c.sizes) >= 1
    assert all(0 <= g < len(c.groups) for g in c.seg_group)
    for a in (c.P, c.G, c.M, c.V):
        assert a.dtype == np.float32 and a.size == sum(c.sizes)
    assert bool((c.V >= 0).all())
    if name in oc.FINITE:
        # where float64 and fp32 mean the same thing
        g, m = np.abs(c.G[c.G != 0]), np.abs(c.M[c.M != 0])
        assert (g.size == 0 or g.min() >= 1e-12) and (m.size == 0 or m.min() >= 1e-12)
        assert bool(((c.V == 0) | (c.V >= 1e-24)).all()) and float(np.abs(c.G).max(initial=0.0)) < 1e18
        for k in oc.KINDS:
            assert bool(np.isfinite(c.ref[k]).all()), k
        assert c.ref["total_norm"] is None or np.isfinite(c.ref["total_norm"])
    ka = c.kernel_arith()
    miss, ratio = c.check(ka, M=oc.M_DEFAULT / 2)
    print("  kernel_arith ratios:", {k: round(v, 2) for k, v in ratio.items()})
    assert not miss, miss
    assert not oc.M_NAMED or all(n in oc.NAMES and k in oc.KINDS + ("total_norm",) for n, k in oc.M_NAMED)
    # the rule is not vacuous: the unchanged state misses it
    same = dict(ka, param=c.P, exp_avg=c.M, exp_avg_sq=c.V)
    assert {"param", "exp_avg"} <= set(c.check(same)[0])


# ---- the cases reach their branches ----------------------------------------
EXPECT = {  # name -> the layout predicates the case is there for
    "one_1": dict(nchunk=1, total=1, quad_segments=1),
    "one_1023": dict(nchunk=1, total=1023),
    "one_1024": dict(nchunk=1, total=1024),
    "one_1025": dict(nchunk=2, total=1025),
    "aligned_1024x2": dict(nchunk=2, chunk_aligned_start=True, max_segs_per_chunk=1),
    "quad_span": dict(quad_segments=3, chunk_aligned_start=True, nchunk=2),
    "lanes": dict(unrolled=True, not_unrolled=True, tail_after_unrolled=True, tail_trips=3, nchunk=2),
    "seg64_one_chunk": dict(nseg=64, scan_full_wave=True, nchunk=1, max_segs_per_chunk=64, wave_rounds=16,
                            bc_lanes_to=128),
    "seg64_ragged": dict(nseg=64, scan_full_wave=True, bc_lanes_to=128, wave_rounds=16),
    "chunks_8": dict(nchunk=8, fold_rounds=1),
    "chunks_9": dict(nchunk=9, fold_rounds=2),
    "chunks_256": dict(nchunk=256, one_launch=True, fold_rounds=32),
    "chunks_257": dict(nchunk=257, one_launch=False, fold_rounds=33),
    "groups_4": dict(nseg=8, wave_rounds=2),
}


@pytest.mark.parametrize("name", oc.NAMES)
def test_case_reaches_its_branch(name):
    c = oc.case(name)
    L = oc.layout(c.sizes)
    pieces = L.pop("pieces")
    print("%s: %s; parts %s" % (name, L, pieces[:12]))
    for k, v in EXPECT.get(name, {}).items():
        assert L[k] == v, (k, L[k], v)
    ref = c.ref
    if name == "quad_span":
        # elements 1020 .. 1023 of the last thread of chunk 0 lie in segments 0, 0, 1, 2; segment 4 starts chunk 1
        assert c.starts[1] == 1022 and c.starts[4] == 1025 and c.starts[3] == 1024
    if name == "lanes":
        assert {63, 65, 255, 257, 256, 64, 193} <= set(pieces)
    if name == "seg64_ragged":
        assert L["nchunk"] >= 3 and L["max_segs_per_chunk"] > 4 and min(c.sizes) == 1 and max(c.sizes) <= 200
        assert any(c.starts[k] // oc.CH != (c.starts[k + 1] - 1) // oc.CH for k in range(64))     # straddles
    if name == "groups_4":
        assert len(c.groups) == 4 and sorted(set(c.seg_group)) == [0, 1, 2, 3]
        assert c.seg_group != sorted(c.seg_group) and sum(c.seg_abs) == 2
        assert all(len(set(g[j] for g in c.groups)) == 4 for j in range(5))       # lr, wd, betas, eps all differ
        for k in (2, 5):
            p, lr = c.seg(c.P, k)[:16], c.groups[c.seg_group[k]][0]
            assert bool((np.abs(p) < lr).all()) and bool((p > 0).any()) and bool((p < 0).any())
            assert bool((c.seg(ref["param"], k) >= 0).all())
        assert bool((c.seg(ref["param"], 3) < 0).any()) and bool((c.seg(ref["param"], 6) < 0).any())
    if name == "wd0":
        assert c.groups[0][1] == 0.0
    if name == "beta1_0":
        assert np.array_equal(ref["exp_avg"], ref["grad"])
    if name == "beta2_0_eps0":
        assert np.array_equal(ref["exp_avg_sq"], ref["grad"] ** 2) and bool((c.G != 0).all())
    if name == "fresh_tiny_g":
        a = np.abs(c.G)
        assert c.seg_step == [0, 0, 0, 0] and not c.M.any() and not c.V.any()
        assert 1e-9 <= a.min() < 1e-8 < a.max() <= 1e-7 and c.groups[0][4] == 1e-8 and ref["coef"] == 1.0
    if name == "steps_distinct":
        assert c.seg_step == [0, 1, 9, 999, 99999] and list(ref["steps"]) == [1, 2, 10, 1000, 100000]
    if name == "clip_inactive":
        assert ref["coef"] == 1.0 and ref["total_norm"] < 0.51 * c.max_norm and c.grads_exact
        assert np.array_equal(ref["grad"], c.G.astype(np.float64))
    if name == "clip_edge":
        assert c.max_norm == float(np.float32(ref["total_norm"]))
        assert 1.0 - 1e-5 < ref["coef"] < 1.0 - 4 * oc.EPS32 and not c.grads_exact
    if name == "tiny_norm":
        assert abs(ref["total_norm"] - 2e-6) < 1e-9 and c.max_norm == float(np.float32(1e-6))
        assert abs(ref["coef"] - 1.0 / 3.0) < 1e-3            # 0.5 without the + 1e-6
    if name == "zero_grads":
        assert ref["total_norm"] == 0.0 and ref["coef"] == 1.0 and not ref["grad"].any()
        assert bool((ref["exp_avg"] != c.M).all()) and bool((ref["param"] != c.P).all())
    if name in ("no_clip_0", "no_clip_neg", "nan_no_clip"):
        assert not c.clip and ref["total_norm"] is None and c.grads_exact
    if name == "nan_one":
        k = int(np.argmin(c.sizes))
        assert np.isnan(c.seg(c.G, k)[0]) and int(np.isnan(c.G).sum()) == 1 and np.isnan(ref["total_norm"])
        assert all(bool(np.isnan(ref[kind]).all()) for kind in oc.KINDS)
    if name == "inf_one":
        j = int(np.flatnonzero(np.isinf(c.G))[0])
        assert ref["total_norm"] == np.inf and ref["coef"] == 0.0
        fin = np.arange(c.G.size) != j
        assert not ref["grad"][fin].any() and bool(np.signbit(ref["grad"][fin]).any())        # +-0
        assert np.array_equal(ref["exp_avg_sq"][fin], 0.999 * c.V.astype(np.float64)[fin])     # only decays
        assert all(np.isnan(ref[kind][j]) and not np.isnan(ref[kind][fin]).any() for kind in oc.KINDS)
    if name == "nan_no_clip":
        j = int(np.flatnonzero(np.isnan(c.G))[0])
        assert all(int(np.isnan(ref[kind]).sum()) == 1 and np.isnan(ref[kind][j]) for kind in oc.KINDS)
    if name == "sq_overflow":
        assert int((np.abs(c.G) == np.float32(1e20)).sum()) == 7 and ref["total_norm"] == np.inf
        assert not ref["grad"].any() and not np.isnan(ref["param"]).any()
        with np.errstate(over="ignore"):
            assert np.isinf(np.float32(1e20) * np.float32(1e20))
        assert np.isfinite(oc.reference(*c.args())[0]["total_norm"])          # float64's own total is finite


# ---- the cases discriminate -------------------------------------------------
MUTATIONS = {  # mutation of kernel_arith -> (what it is, the case that must catch it, the tensor kind it shows in)
    "eps_in_bc": ("eps divided by the bias correction: (sqrt(v) + eps) / sqrt(bc2)", "fresh_tiny_g", "param"),
    "coupled_l2": ("coupled L2 decay: g += wd p, no decoupled decay", "groups_4", "exp_avg"),
    "decay_after": ("the decay applied after the update", "groups_4", "param"),
    "shared_step": ("one shared step (segment 0's) for all segments", "steps_distinct", "param"),
    "group_row0": ("row 0 of the group table for every segment", "groups_4", "param"),
    "no_1e6": ("max_norm / tot without the + 1e-6", "tiny_norm", "grad"),
    "no_clamp": ("the coefficient not clamped at 1", "clip_inactive", "grad"),
    "moments_unclipped": ("the moments from the unclipped gradient", "one_1023", "exp_avg"),
    "fp32_one_minus_beta2": ("1 - beta2 evaluated in fp32 (1.3e-5 off)", "fresh_tiny_g", "exp_avg_sq"),
    "bc_at_t": ("bias corrections at t instead of t + 1", "fresh_tiny_g", "param"),
    "abs_next_segment": ("|p| applied to the following segment", "groups_4", "param"),
    "abs_before_update": ("|p| taken before the update", "groups_4", "param"),
}


def test_every_mutation_is_listed():
    assert sorted(MUTATIONS) == sorted(oc.MUTATIONS)


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_mutation_is_caught(mut):
    what, name, kind = MUTATIONS[mut]
    c = oc.case(name)
    miss, ratio = c.check(c.kernel_arith(mut))
    print("%s (%s) at %s: misses %s, ratios %s" % (mut, what, name, miss, {k: "%.3g" % v for k, v in ratio.items()}))
    assert miss.get(kind, 0) > 0, "%s does not catch %s" % (name, mut)


def test_moments_from_the_unclipped_gradient_show_at_every_clipped_case():
    for name in oc.FINITE:
        c = oc.case(name)
        if c.clip and c.ref["coef"] < 0.9:
            assert "exp_avg" in c.check(c.kernel_arith("moments_unclipped"))[0], name


def test_per_tensor_max_rule_would_pass_the_fp32_one_minus_beta2():
    """What the per-element rule is for: the fp32 `1 - beta2` moves every
    element of a fresh second moment by 1.3e-5 relative - under `rtol 1e-5 *
    max |tensor|` every element below 3/4 of the tensor's largest passes (over
    90 % of them here), and under this rule none does."""
    c = oc.case("fresh_tiny_g")
    mut = c.kernel_arith("fp32_one_minus_beta2")["exp_avg_sq"].astype(np.float64)
    ref = c.ref["exp_avg_sq"]
    rel = np.abs(mut - ref) / ref
    assert 1.2e-5 < rel.min() and rel.max() < 1.4e-5
    per_tensor = [float(np.mean(np.abs(c.seg(mut, k) - c.seg(ref, k)) <= 1e-5 * c.seg(ref, k).max()))
                  for k in range(len(c.sizes))]
    print("share of elements a per-tensor-max rule accepts:", per_tensor)
    assert min(per_tensor) > 0.9
    assert oc.compare(mut, ref, c.A["exp_avg_sq"], oc.M_DEFAULT)[0] == mut.size


def test_rule_compares_special_values_exactly():
    ref = np.array([np.nan, np.inf, 0.0, 1.0, -0.0])
    A = np.abs(ref)
    assert oc.compare(ref.astype(np.float32), ref, A, 8.0)[0] == 0
    assert oc.compare(np.float32([np.nan, np.inf, -0.0, 1.0, 0.0]), ref, A, 8.0)[0] == 0     # zeros by ==
    assert oc.compare(np.float32([0.0, np.inf, 0.0, 1.0, 0.0]), ref, A, 8.0)[0] == 1         # a lost NaN
    assert oc.compare(np.float32([np.nan, 3e38, 0.0, 1.0, 0.0]), ref, A, 8.0)[0] == 1        # inf by ==
    assert oc.compare(np.float32([np.nan, np.inf, 1e-30, 1.0, 0.0]), ref, A, 8.0)[0] == 1    # zero by ==
    assert oc.compare(np.float32([np.nan, np.inf, 0.0, np.nan, 0.0]), ref, A, 8.0)[0] == 1   # a new NaN
    assert oc.compare(np.float32([np.nan, np.inf, 0.0, 1.0 + 9 * oc.EPS32, 0.0]), ref, A, 8.0)[0] == 1
    assert oc.compare(np.float32([np.nan, np.inf, 0.0, 1.0 + 7 * oc.EPS32, 0.0]), ref, A, 8.0)[0] == 0


# ---- the Python class on CPU parameters ------------------------------------
def test_clip_adamw_cpu_path_meets_the_rule_at_groups_4():
    """optim.ClipAdamW's torch-op path (CPU parameters) on the groups_4 table,
    from four param-group dicts: fp32 ATen sums the norm in another order, so
    the clipped gradients are compared at the rule's M and not at half of it."""
    import torch
    from mcaq_yolo_amd.optim import ClipAdamW
    c = oc.case("groups_4")
    o, ps, order = clip_adamw_from_case(c, torch.device("cpu"))
    o.step()
    miss, ratio = c.check(collect(c, o, ps, order))
    print(ratio)
    assert not miss, miss


def clip_adamw_from_case(c, dev):
    """A ClipAdamW holding the case's state: one param-group dict per group (its segments in segment order),
    moments and steps through load_state_dict -> (optimizer, parameters in optimizer order, their segments)."""
    import torch
    from mcaq_yolo_amd.optim import ClipAdamW
    order = [k for gi in range(len(c.groups)) for k in range(len(c.sizes)) if c.seg_group[k] == gi]
    ps = {k: torch.nn.Parameter(torch.from_numpy(c.seg(c.P, k).copy()).to(dev)) for k in order}
    gd = [dict(params=[ps[k] for k in order if c.seg_group[k] == gi], lr=g[0], weight_decay=g[1], betas=(g[2], g[3]),
               eps=g[4]) for gi, g in enumerate(c.groups)]
    o = ClipAdamW(gd, max_norm=c.max_norm if c.clip else None, project_abs=[ps[k] for k in order if c.seg_abs[k]])
    sd = o.state_dict()
    sd["state"] = {i: dict(step=torch.tensor(float(c.seg_step[k])), exp_avg=torch.from_numpy(c.seg(c.M, k).copy()),
                           exp_avg_sq=torch.from_numpy(c.seg(c.V, k).copy())) for i, k in enumerate(order)}
    o.load_state_dict(sd)
    for k in order:
        ps[k].grad = torch.from_numpy(c.seg(c.G, k).copy()).to(dev)
    return o, [ps[k] for k in order], order


def collect(c, o, ps, order):
    """The optimizer's tensors back in the case's segment order."""
    inv = {k: i for i, k in enumerate(order)}
    cat = lambda f: np.concatenate([f(ps[inv[k]]).detach().cpu().numpy().reshape(-1) for k in range(len(c.sizes))])
    return dict(grad=cat(lambda p: p.grad), param=cat(lambda p: p), exp_avg=cat(lambda p: o.state[p]["exp_avg"]),
                exp_avg_sq=cat(lambda p: o.state[p]["exp_avg_sq"]),
                steps=np.array([float(o.state[ps[inv[k]]]["step"]) for k in range(len(c.sizes))]),
                total_norm=None if o.last_total_norm is None else float(o.last_total_norm))
