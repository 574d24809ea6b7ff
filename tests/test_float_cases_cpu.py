"""The exactness conditions of tests/float_cases.py, on the very operands the
GPU tests upload.  The GPU tests of the float paths assert equality with the
fp64 oracle; that is only a fair demand while these hold, so a changed
generator cannot silently turn an exact test into a tolerance test.

For every class, variant and size used by test_gpu_float_exact.py:
  * a numpy model of k_split6 (h = rne(x), m = rne(x - h), l = rne(x - h - m),
    the six plane pairs of its two patterns) sums to the exact product sum;
  * max over (pod, node) of sum_m sum_planes |b| |a| < 2^24 q, q the class's
    quantum: every partial sum, in any order, is a multiple of q below 2^24 q
    and so exactly representable in fp32;
  * every operand and plane is a multiple of the quantum's factors;
  * the planes the class is meant to populate are populated.
And the bf16 CSR reference of float_cases.py: order-independent sums, planted
rounding cases."""
import numpy as np
import pytest

import float_cases as fc
import oracle
from util import bf16_bits_to_f64, f32_to_bf16_bits


def check_exact(cls, WA, L):
    q = fc.QUANTUM[cls]
    total, mag = fc.six_term(WA, L)
    exact = WA.astype(np.float64) @ L.astype(np.float64)
    assert np.array_equal(total, exact)
    assert mag.max() < 2.0 ** 24 * q, (cls, mag.max())
    # every plane product is a multiple of q: the planes are multiples of
    # q_l and q_w with q_l * q_w = q
    ql, qw = {"dyadic": (2.0 ** -3, 2.0 ** -6)}.get(cls, (1.0, 1.0))
    for plane in fc.split6(L):
        assert np.array_equal(np.round(plane / ql) * ql, plane)
    for plane in fc.split6(WA):
        assert np.array_equal(np.round(plane / qw) * qw, plane)
    # the dropped terms are zero: x = h + m + l, and no (m, l), (l, m), (l, l) pair
    for x in (WA, L):
        h, m, lo = fc.split6(x)
        assert np.array_equal(h + m + lo, x.astype(np.float64))
    (_, lm, ll), (_, wm, wl) = fc.split6(L), fc.split6(WA)
    assert not (ll.any() and (wm.any() or wl.any()))
    assert not (wl.any() and lm.any())
    # the oracle's own fp64 sum is this exact sum
    rows = slice(0, min(len(WA), 64))
    assert np.array_equal(oracle.cost(WA[rows], L, "f32"), exact[rows])
    return exact


def plane_shares(x):
    """Share of the non-zero entries of x with a non-zero m / l plane."""
    _, m, lo = fc.split6(x)
    nz = x != 0
    return (m != 0)[nz].mean(), (lo != 0)[nz].mean()


def check_population(cls, WA, L):
    if WA.any() and cls == "L20xW1":
        m, lo = plane_shares(L)
        assert m >= 0.9 and lo >= 0.5, (m, lo)
        assert plane_shares(WA) == (0, 0)
    elif WA.any() and cls == "L1xW20":
        if (WA != 0).sum() >= 100:
            m, lo = plane_shares(WA)
            assert m >= 0.9 and lo >= 0.5, (m, lo)
        assert plane_shares(L) == (0, 0)
    elif WA.any():
        if L.size >= 100:
            assert plane_shares(L)[0] >= 0.6, plane_shares(L)
        if (WA != 0).sum() >= 100:
            assert plane_shares(WA)[0] >= 0.6, plane_shares(WA)
        assert plane_shares(L)[1] == 0 and plane_shares(WA)[1] == 0


def test_plane_population_shares():
    """The table of float_cases.py: l in ~88% of the 20-bit operands, m in ~75%
    of the 10-bit ones."""
    rng = np.random.default_rng(0)
    m, lo = plane_shares(fc._odd20(rng, 100000))
    assert m > 0.98 and 0.85 <= lo <= 0.91, (m, lo)
    m, lo = plane_shares(fc._int10(rng, 100000))
    assert 0.72 <= m <= 0.78 and lo == 0, (m, lo)
    m, lo = plane_shares(fc._int10(rng, 100000) / 64)
    assert 0.72 <= m <= 0.78 and lo == 0, (m, lo)


@pytest.mark.parametrize("N", fc.SMALL_N)
@pytest.mark.parametrize("cls,signed", fc.VARIANTS)
def test_small_cases_are_exact(cls, signed, N):
    for P in fc.SMALL_P:
        for dup in (0, 5):
            WA, L, pairs, free, req = fc.small_case(cls, signed, P, N, dup)
            cost = check_exact(cls, WA, L)
            if P > 1:
                # tight: lists that are dry from the start next to full ones,
                # pods that are placed next to pods that find no node
                nfit = (req[:, None, :] <= free[None, :, :]).all(2).sum(1)
                assert (nfit < 8).any() and (N < 63 or (nfit >= 8).any()), (nfit.min(), nfit.max())
                want, wcost, _ = oracle.place(WA, L, req, free, "f32")
                assert (want < 0).any() and (want >= 0).any()
                assert not signed or N < 63 or (wcost < 0).any()
            if P > 1:
                check_population(cls, WA, L)
            for a, b in pairs:
                assert a < b and np.array_equal(cost[:, a], cost[:, b])
            assert bool(pairs) == (dup > 0 and N >= 2)
            nnz = (WA != 0).sum(1)
            assert nnz.max() <= 8 and (P == 1 or nnz.min() == 0)
            if not signed:
                assert (WA >= 0).all() and (L > 0).all() and (cost >= 0).all()
            elif P > 1 and N >= 63:
                # costs of both signs in (nearly) every row with traffic
                live = (WA != 0).sum(1) >= 2
                both = (cost.min(1) < 0) & (cost.max(1) > 0)
                assert both[live].mean() >= 0.95, (cls, both[live].mean())


@pytest.mark.parametrize("cls", fc.WIDE_CLASSES)
def test_wide_cases_are_exact(cls):
    WA, L, _, _ = fc.wide_case(cls)
    assert WA.shape == fc.WIDE_SHAPE
    check_exact(cls, WA, L)
    check_population(cls, WA, L)


@pytest.mark.parametrize("cls,signed", fc.COMP_VARIANTS)
def test_composition_cases_are_exact(cls, signed):
    for tag in ("group2", "group3", "shard", "loop", "constraints", "batch0", "batch1", "batch2"):
        WA, L, _, _ = fc.comp_case(cls, signed, tag)
        cost = check_exact(cls, WA, L)
        check_population(cls, WA, L)
        # the hot nodes: cheaper than every other node for (nearly) every pod
        # with three peers or more (a single latency entry elsewhere can
        # undercut them for a pod with one peer)
        live = (WA != 0).sum(1) >= 3
        assert (cost[live, :6].max(1) < cost[live, 6:].min(1)).mean() >= 0.95
    WA, L, _, _ = fc.cache_case(cls, signed)
    assert WA.shape == fc.CACHE_SHAPE
    cost = check_exact(cls, WA, L)
    live = (WA != 0).sum(1) >= 3
    h = fc.CACHE_HOT
    assert (cost[live, :h].max(1) < cost[live, h:].min(1)).mean() >= 0.95


def test_int_bf16_operands_are_exact():
    WA, L, pairs = fc.int_bf16_operands(np.random.default_rng(1), 300, 130, dup=6)
    wa, la = bf16_bits_to_f64(WA), bf16_bits_to_f64(L)
    assert np.array_equal(wa, np.round(wa)) and np.array_equal(la, np.round(la))
    assert (np.abs(wa) @ np.abs(la)).max() < 2 ** 24
    assert len(pairs) == 6 and all(np.array_equal(la[:, a], la[:, b]) and a < b for a, b in pairs)
    assert (WA[0] == 0x8000).all() and (WA[3] == 0).all()


def test_csr_bf16_reference():
    P, N = 777, 130
    row_ptr, peer, w, planted = fc.csr_bf16_case(np.random.default_rng(2), P, N)
    ref = fc.csr_bf16_reference(row_ptr, peer, w, N)
    assert ref.shape == (P, N)
    for (p, m), v in planted.items():
        assert bf16_bits_to_f64(ref[p, m]) == v, (p, m)
    assert not ref[2].any()  # the cancelled row is +0 everywhere (no -0 bits)
    deg = np.diff(row_ptr)
    assert deg.min() == 0 and deg[1] == 300 and np.delete(deg, [0, 1, 2]).max() == 12
    assert 8 <= np.count_nonzero(ref[1]) <= 10
    for bad in (-1, N, N + 5, 2 ** 30):
        assert (peer == bad).any()
    # every fp32 sum is exact, so the order of summation does not matter: an
    # fp64 sum per (pod, node), rounded once, gives the same bits
    wf = bf16_bits_to_f64(w)
    dense = np.zeros((P, N))
    cnt = np.zeros((P, N), np.int64)
    nonadjacent = cancelled = 0
    for p in range(P):
        seg = peer[row_ptr[p]:row_ptr[p + 1]]
        for i, m in enumerate(seg):
            if 0 <= m < N:
                dense[p, m] += wf[row_ptr[p] + i]
                cnt[p, m] += 1
                nonadjacent += i >= 2 and m in seg[:i - 1] and seg[i - 1] != m
    cancelled = int(((cnt >= 2) & (dense == 0)).sum())
    assert np.array_equal(dense.astype(np.float32).astype(np.float64), dense)
    assert np.array_equal(f32_to_bf16_bits(dense.astype(np.float32)), ref)
    assert np.delete(cnt, 1, axis=0).max() <= 12
    assert nonadjacent >= 50 and cancelled >= 20, (nonadjacent, cancelled)
    # ties in the final rounding occur beyond the planted ones
    u = dense.astype(np.float32).view(np.uint32)
    assert ((u & 0xFFFF) == 0x8000).sum() >= 3
