"""tests/percentile_cases.py: every case reaches the branch its name claims,
and the sort-based restatement of torch.quantile's rule (SURVEY App. A rule
10) equals torch.quantile on all of them."""
import numpy as np
import pytest
import torch

import percentile_cases as PC

f32 = np.float32


def _chan(name, c):
    return PC.rows_of(PC.case(name)).numpy()[c]


def test_rank_rule_branches():
    """N = 2048 and N = 6400 take the two lerp branches the other way round;
    exact_rank has w = 0 for both quantiles; below N = 10,001 the four ranks
    are 0, 1, N - 2, N - 1."""
    a0, a1, wa = PC.ranks(2048, PC.Q_LO)
    b0, b1, wb = PC.ranks(2048, PC.Q_HI)
    assert (a0, a1, b0, b1) == (0, 1, 2046, 2047) and wa < 0.5 <= wb
    a0, a1, wa = PC.ranks(6400, PC.Q_LO)
    b0, b1, wb = PC.ranks(6400, PC.Q_HI)
    assert (a0, a1, b0, b1) == (0, 1, 6398, 6399) and wb < 0.5 <= wa
    x = PC.case("exact_rank").x
    n = x.shape[0] * x.shape[2] * x.shape[3]
    a0, a1, wa = PC.ranks(n, PC.Q_LO)
    b0, b1, wb = PC.ranks(n, PC.Q_HI)
    assert a0 == a1 >= 1 and b0 == b1 and wa == 0 and wb == 0
    assert PC.ranks(1, PC.Q_LO) == (0, 0, 0) and PC.ranks(1, PC.Q_HI) == (0, 0, 0)
    assert PC.ranks(2, PC.Q_HI)[:2] == (0, 1)
    assert PC.rows_of(PC.case("ref_shape")).shape[1] == 2048
    assert PC.rows_of(PC.case("n6400")).shape[1] == 6400
    assert PC.rows_of(PC.case("per_tensor")).shape == (1, 16384)
    assert PC.rows_of(PC.case("sampled")).shape[1] == 102400 > 100000
    # interior ranks: the low ranks of `sampled` are 10 and 11
    assert PC.ranks(102400, PC.Q_LO)[:2] == (10, 11)


def test_key_is_order_preserving():
    v = np.array([-np.inf, -3.0, -1e-40, -0.0, 0.0, 1e-45, 1.0, np.nextafter(f32(2), f32(0)), 2.0, np.inf], f32)
    k = PC.key_of(v).astype(np.int64)
    assert np.all(np.diff(k) >= 0) and k[3] == k[4]
    assert np.all(np.diff(np.delete(k, 3)) > 0)


def test_ties_channels_have_their_structure():
    t = PC.TIES
    x = PC.case("ties").x
    N = x.shape[0] * x.shape[2] * x.shape[3]
    assert PC.ranks(N, PC.Q_LO)[:2] == (0, 1) and PC.ranks(N, PC.Q_HI)[:2] == (N - 2, N - 1)
    assert x.shape[2] * x.shape[3] < 4096 and x.shape[0] > 1        # more than one workgroup per channel
    c = _chan("ties", t.index("constant"))
    assert np.unique(c).size == 1
    c = _chan("ties", t.index("two_valued"))
    assert np.unique(c).size == 2 and min((c == -1).sum(), (c == 2).sum()) > 2
    c = _chan("ties", t.index("low_bits"))
    k = PC.key_of(c)
    assert np.unique(k >> 8).size == 1 and np.unique(k & 0xff).size > 100
    stats, _, _ = PC.restate(PC.rows_of(PC.case("ties")).numpy())
    assert np.unique(PC.bin0(stats[t.index("four_bins")])).size == 4
    b = PC.bin0(stats[t.index("straddle")])
    assert b[0] != b[1] and b[2] != b[3]
    # ... and the two values are neighbours: nothing lies between them
    s = stats[t.index("straddle")]
    assert np.nextafter(s[0], f32(0)) == s[1] and np.nextafter(s[2], f32(4)) == s[3]


def test_zero_and_nonfinite_cases():
    z = PC.rows_of(PC.case("zeros")).numpy()
    stats, lo, hi = PC.restate(z)
    tiny = np.finfo(f32).tiny
    assert 0 < -stats[0, 0] < tiny and stats[0, 1] == 0 and stats[0, 2] == 0 and 0 < stats[0, 3] < tiny
    assert np.signbit(z[0]).any() and (~np.signbit(z[0][z[0] == 0])).any()       # zeros of both signs
    assert stats[1, 0] == 0 and stats[1, 1] == 0 and 0 < stats[1, 2] < stats[1, 3] < tiny
    assert lo[0] < 0 < hi[0] and lo[1] == 0
    n = PC.rows_of(PC.case("nonfinite")).numpy()
    stats, lo, hi = PC.restate(n)
    assert np.all(np.isneginf(stats[0, :2])) and np.all(np.isposinf(stats[0, 2:]))
    assert np.isnan(n[1]).sum() == 1 and np.isnan(lo[1]) and np.isnan(hi[1])
    assert np.isneginf(stats[2, 0]) and np.isfinite(stats[2, 1]) and np.isposinf(stats[2, 3])
    assert np.isfinite(n[3]).all()


def test_odd_and_half_cases():
    o = PC.case("odd")
    assert o.offset == 1 and o.x.is_contiguous() and tuple(o.x.shape) == (3, 5, 20, 20)
    assert (13 * 17) % 4 != 0 and tuple(PC.case("odd_hw").x.shape) == (2, 3, 13, 17)
    for tag, dt in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        assert PC.case("half_ref_shape_" + tag).x.dtype == dt and PC.case("half_odd_" + tag).x.dtype == dt
        assert PC.case("half_odd_" + tag).offset == 1
    s = PC.rows_of(PC.case("sampled")).numpy()[1]
    b = PC.bin0(s)
    assert np.bincount(b).max() > 0.1 * s.size         # the SiLU plateau: over a tenth in one first-level bin


def test_fma32_single_rounding():
    # a product whose low bits decide the rounding of the sum
    a, b, c = f32(1 + 2 ** -12), f32(1 + 2 ** -12), f32(-1)
    assert PC.fma32(a, b, c) == f32(2 ** -11 + 2 ** -24)
    assert f32(f32(a * b) + c) != PC.fma32(a, b, c)
    assert np.isnan(PC.fma32(0.3, np.inf, -np.inf)) and PC.fma32(0.0, 5.0, 2.0) == 2.0


@pytest.mark.parametrize("name", PC.names())
def test_restatement_equals_torch_quantile(name):
    c = PC.case(name)
    rows = PC.rows_of(c)
    lo, hi = PC.expected(c)
    _, rlo, rhi = PC.restate(rows.numpy())
    assert PC.same(rlo, lo), (rlo, lo)
    assert PC.same(rhi, hi), (rhi, hi)
