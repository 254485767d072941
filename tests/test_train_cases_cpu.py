"""tests/train_cases.py on the CPU: every case builds off the kinks within the
seed cap, the rule's inputs are sane (the fp32 restatement loses at most 1e-3
of the scale against float64, so the rule is never looser than the earlier
1e-3), every case reaches the branch its name says (the host-side predicates
restated here), and the cases discriminate: for each mutation of the
reference at least one named case fails the rule at M = 8 with the mutated
fp32 restatement in the kernel's place."""
import numpy as np
import pytest
import torch

import train_cases as tc


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_builds_and_rule_inputs_are_sane(name):
    c = tc.case(name)
    print("%s [%s]: seed %d (try %d of %d) - %s" % (name, c.kind, c.seed, c.tries, tc.MAX_SEEDS, c.why))
    for g, (near, d) in c.kinks.items():
        print("  gate %-7s nearest non-tie argument %.3g from its kink, fp32 difference %.3g" % (g, near, d))
        assert near > tc.KINK_MARGIN * d
    assert c.tries <= tc.MAX_SEEDS
    for k in c.ref:
        assert bool(torch.isfinite(c.ref[k]).all()) and bool(torch.isfinite(c.cpu32[k]).all()), k
        assert c.e32[k] <= tc.CAP * c.S[k], "%s: e32 %g vs scale %g" % (k, c.e32[k], c.S[k])
        assert c.cpu32[k].dtype == torch.float32 and c.ref[k].dtype == torch.float64
    assert not c.failures(c.cpu32, M=1.0)            # by construction
    zero = {k: torch.zeros_like(v) for k, v in c.ref.items()}
    if any(c.S[k] > 0.0 for k in c.ref):
        assert c.failures(zero)                      # the rule is not vacuous


# ---- the cases reach their branches ----------------------------------------
MAPPER_WG = {1: 1, 2: 1, 15: 1, 16: 1, 17: 1, 63: 1, 64: 1, 65: 2, 130: 3}


@pytest.mark.parametrize("name", tc.names("mapper"))
def test_mapper_case_reaches_its_branch(name):
    c = tc.case(name)
    cfg = c.cfg
    n = cfg["n"]
    nwg = (n + tc.TR_TPB - 1) // tc.TR_TPB
    print("%s: n %d, %d workgroup(s), last one %d tile(s), %d full 16-tile block(s) + %d" %
          (name, n, nwg, n - (nwg - 1) * tc.TR_TPB, n // 16, n % 16))
    assert nwg == MAPPER_WG[n]
    T = tc.temperature_arg(cfg["T"])
    raw = tc.MIN_B + (tc.MAX_B - tc.MIN_B) * 0.5
    if cfg["T"] == 0.05:
        assert T == float(np.float32(0.1))           # floored by the host
        assert bool((c.ref["bits"] == tc.MIN_B).all())
    if cfg["T"] == 2.5:
        assert raw * T > tc.MAX_B and bool((c.ref["bits"] == tc.MAX_B).any())     # the upper clamp saturates
        assert float(c.ref["g_c"].abs().max()) > 0.0 or n <= 2                 # and the STE passes the gradient
    if cfg["round"]:
        assert bool((c.ref["bits"] == torch.round(c.ref["bits"])).all())
    else:
        assert n <= 2 or cfg["T"] is not None or bool((c.ref["bits"] != torch.round(c.ref["bits"])).any())
    assert ("rstat.mean.1" in c.ref) == (cfg["update_stats"] == 2)
    if n <= 2:
        # the batch normalisation's output does not depend on its input: g_c is zero in exact arithmetic
        assert float(c.ref["g_c"].abs().max()) <= 1e-9 * c.S["g_c"]
    if n == 1:
        assert all(float(c.ref["rstat.var.%d" % k].abs().max()) == 0.0 for k in (1, 4, 7) if "rstat.var.1" in c.ref)
    if cfg.get("ties"):
        cin, g = c.inp["c"], c.ref["g_c"]
        assert [float(cin[i]) for i in (3, 10)] == [0.0, 1.0]                  # exactly on the bounds
        assert float(cin[17]) == float(np.float32(-0.1)) and float(cin[24]) == float(np.float32(1.1))
        assert float(g[3]) != 0.0 and float(g[10]) != 0.0                      # inclusive gate: the gradient passes
        assert float(g[17]) == 0.0 and float(g[24]) == 0.0


HEAD_EXPECT = {  # name -> (MLP workgroups, images, tiles with an unclamped 5x5 window)
    "head_1x1x1": (1, 1, 0), "head_1x1x7": (1, 1, 0), "head_2x3x2": (1, 2, 0), "head_1x5x5": (1, 1, 1),
    "head_2x5x7": (2, 2, 3), "head_1x9x8": (2, 1, 20), "head_3x8x8": (3, 3, 16), "head_1x27x28": (12, 1, 552),
    "head_1x24x32": (12, 1, 560), "head_zeros": (2, 2, 3), "head_const3": (2, 2, 3)}


@pytest.mark.parametrize("name", tc.names("head"))
def test_head_case_reaches_its_branch(name):
    c = tc.case(name)
    B, ht, wt = c.cfg["shape"]
    n = B * ht * wt
    nwg = (n + tc.TR_TPB - 1) // tc.TR_TPB
    inner = max(ht - 4, 0) * max(wt - 4, 0)
    print("%s: %d tiles, %d MLP workgroup(s), %d bilateral workgroup(s), %d unclamped tile(s) per image, LDS %d B" %
          (name, n, nwg, B, inner, 53 * ht * wt * 4))
    assert (nwg, B, inner) == HEAD_EXPECT[name]
    assert tc.head_bwd_fits(ht, wt)
    if name == "head_3x8x8":
        assert n % tc.TR_TPB == 0
    if name in ("head_1x9x8", "head_2x5x7"):
        assert n % tc.TR_TPB != 0 and ht * wt % tc.TR_TPB != 0
    if c.cfg.get("craw") == "zeros":
        assert float(c.inp["craw"].abs().max()) == 0.0
        assert float(c.ref["gcraw"].abs().max()) > 0.0          # C = 0 sits on the bound and the gate is open
    if c.cfg.get("craw") == "const3":
        assert all(float(v.abs().max()) == 0.0 for v in c.ref.values())


def test_head_lds_bound_is_inclusive_at_768_tiles():
    """53 floats per tile against 160 KiB - 1 KiB: 24 x 32 = 768 tiles take
    exactly the bound and fit (`<=` in core._head_bwd_fits, `l > TR_LDS_MAX`
    refused in head_segs); 25 x 31 = 775 tiles are the first refused."""
    from mcaq_yolo_amd import core
    assert 53 * 24 * 32 * 4 == tc.LDS_LIMIT == core._TRAIN_LDS_LIMIT
    for ht, wt in ((27, 28), (24, 32), (25, 31), (32, 32), (1, 1)):
        assert core._head_bwd_fits(ht, wt) == tc.head_bwd_fits(ht, wt) == (ht * wt <= 768)


SMASK_EXPECT = {  # name -> the predicates the case is there for
    "smask_4x4_t1": dict(w_lt5=True, tiles=1, staged=True, pixel_pass=False),
    "smask_5x7_t1": dict(staged=False, pixel_pass=False, w_lt5=False, tiles=1),
    "smask_8x8_t2": dict(staged=True, pixel_pass=True, pool_row4_all=True, up_row4_all=True, ragged=False),
    "smask_20x20_t4": dict(staged=True, pixel_pass=True, pool_row4_any=False, up_row4_any=False, ragged=False),
    "smask_20x20_t4_off1": dict(staged=False, pixel_pass=False, ragged=False),
    "smask_21x23_t5": dict(staged=False, ragged=True, overlap=True, uneven=True, images=2),
    "smask_22x26_t5x6": dict(staged=True, ragged=True, overlap=True, uneven=True, pixel_pass=True),
    "smask_36x36_t8": dict(staged=True, ragged=True, overlap=True, uneven=True, pool_row4_any=False,
                           up_row4_any=True, up_row4_all=False),
    "smask_33x41_t8x10": dict(staged=False, ragged=True, overlap=True, uneven=True),
    "smask_36x36_t33": dict(staged=True, ragged=True, tiles=1089, uneven=True),
    "smask_20x20_t5_b3": dict(staged=True, images=3, ragged=False),
    "smask_20x20_t5_ties": dict(staged=True, ragged=False),
    "fold_c40": dict(staged=True, fold_vec=True), "fold_c160": dict(staged=True, fold_vec=True),
    "fold_16x16_b2": dict(staged=True, fold_vec=True, images=2),
    "fold_18x18_qoff1": dict(staged=True, fold_vec=False),
    "fold_15x15": dict(staged=False, fold_vec=False),
    "fold_22x26_t5x6": dict(staged=True, fold_vec=True, ragged=True, uneven=True),
    "fold_20x20_ties": dict(staged=True, fold_vec=True)}


@pytest.mark.parametrize("name", tc.names("smask") + tc.names("fold"))
def test_smask_case_reaches_its_branch(name):
    c = tc.case(name)
    p = tc.smask_predicates(c.cfg)
    print("%s: %s" % (name, p))
    assert p["fits"]
    for k, v in SMASK_EXPECT[name].items():
        assert p[k] == v, (k, p[k])
    if name == "smask_36x36_t33":
        assert p["tiles"] > 1024                      # the 1024-thread tile loops take a second round
        assert set(torch.bincount(tc.nearest_index(33, 36)).tolist()) == {1, 2}
    if c.kind == "fold":
        nsl = (c.cfg["C"] + 31) // 32
        assert c.inp["qwork"].shape[0] == 2 * nsl
        assert {"fold_c40": 2, "fold_c160": 5}.get(name, nsl) == nsl
    if c.cfg.get("ties"):
        b, g = c.inp["bits"].reshape(-1), c.ref["g_bits"].reshape(-1)
        assert [float(b[i]) for i in (1, 6, 11, 16)] == [2.0, 8.0, 1.5, 9.0]
        f = (c.inp["bits"].reshape(-1) - 2.0) / 6.0                            # fp32, as the kernel forms it
        assert float(f[1]) == 0.0 and float(f[6]) == 1.0                       # exactly on the bounds
        if c.kind == "smask":
            assert float(g[1]) != 0.0 and float(g[6]) != 0.0                   # open
            assert float(g[11]) == 0.0 and float(g[16]) == 0.0                 # closed


def test_nearest_index_is_atens_fp32_formula():
    """The fold's tile membership and the upsample's blocks: floor(o * fp32(in / out)), clamped."""
    for n_in, n_out in ((5, 21), (5, 23), (8, 33), (10, 41), (33, 36), (6, 26), (3, 18)):
        sc = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
        idx = torch.floor(torch.arange(n_out, dtype=torch.float32) * sc).long().clamp(max=n_in - 1)
        assert torch.equal(idx, tc.nearest_index(n_in, n_out))


# ---- the cases discriminate -------------------------------------------------
MUTATIONS = {  # mutation -> (what it is, the cases that must catch it)
    "gate_c_exclusive": ("mapper: c's clamp gate exclusive", ["mapper_n65_ties"]),
    "gate_C_exclusive": ("head: C's clamp gate exclusive", ["head_zeros"]),
    "gate_bits_exclusive": ("soft mask: the bits clamp gate exclusive", ["smask_20x20_t5_ties", "fold_20x20_ties"]),
    "zero_pad": ("soft mask: zero pad for replicate pad in the 5x5 smoothing", ["smask_4x4_t1", "smask_8x8_t2"]),
    "pool_floor": ("soft mask: floor-division pooling windows", ["smask_21x23_t5", "smask_33x41_t8x10"]),
    "nearest_block": ("soft mask: o // (H // ht) for the nearest index", ["smask_21x23_t5", "smask_36x36_t33"]),
    "running_var_biased": ("mapper: the running var fed the biased variance", ["mapper_n2", "mapper_n130_deferred"]),
    "budget_scale_count": ("fold: the bit-budget term divided by the scale's tile count alone", ["fold_c40"]),
}


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_mutation_is_caught(mut):
    what, must = MUTATIONS[mut]
    kind = tc.CFGS[must[0]][0]
    caught = {}
    for name in tc.names(kind) + (tc.names("fold") if kind == "smask" else []):
        bad = tc.case(name).failures(tc.case(name).mutated32(mut))
        if bad:
            caught[name] = max(bad, key=lambda b: b[3])
    print("%s (%s): caught by %d case(s)" % (mut, what, len(caught)))
    for name, (k, err, bound, ratio) in caught.items():
        print("  %-26s %-22s err %.3g bound %.3g ratio %.3g" % (name, k, err, bound, ratio))
    for name in must:
        assert name in caught, "%s does not catch %s" % (name, mut)


def test_bilateral_eps_cannot_be_told_in_fp32():
    """The `+ 1e-8` of the bilateral's denominator: the centre tap's weight
    is exactly 1, so the denominator is >= 1, where fp32's spacing is 1.2e-7:
    den + 1e-8f == den.  The mutation that drops it gives the fp32
    restatement's own bits at every head case, the all-zero one included (its
    C is 0 / den either way), so no fp32 evaluation - the kernel's or ATen's -
    can be told from its mutant; in float64 the term moves C by ~1e-9."""
    assert np.float32(1.0) + np.float32(1e-8) == np.float32(1.0)
    for name in tc.names("head"):
        c = tc.case(name)
        mut = c.mutated32("bilateral_no_eps")
        assert all(torch.equal(mut[k], c.cpu32[k]) for k in c.ref), name
    c = tc.case("head_zeros")
    with_eps = tc.bilateral(c.inp["craw"].double() + 0.5)
    without = tc.bilateral(c.inp["craw"].double() + 0.5, "bilateral_no_eps")
    assert 0.0 < float((with_eps - without).abs().max()) < 1e-8
