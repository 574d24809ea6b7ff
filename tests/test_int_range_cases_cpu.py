"""The claims of tests/int_range_cases.py, on the very operands the GPU tests
upload (numpy and the oracle only).  test_gpu_int_range.py means to drive the
cost epilogue through a chosen key coding at a chosen distance from the int32
limits; that only holds while each case's guard product, per-tile class and
planted costs are what its name says, and while the sequential oracle really
places pods on the planted extremes."""
import numpy as np
import pytest

import int_range_cases as ic
import oracle

INT32_MAX = 2 ** 31 - 1


def test_limit_is_the_documented_bound():
    """include/nas.h: accepted up to INT32_MAX - 1 (all-ones key word reserved)."""
    assert ic.LIMIT == INT32_MAX - 1


def check_case(c, want_guard=None):
    WA, L = c["WA"], c["L"]
    P, N = WA.shape
    cost = oracle.cost(WA, L, "i8")
    assert np.array_equal(cost[:64], WA[:64].astype(np.int64) @ L.astype(np.int64))
    assert np.abs(cost).max() <= ic.guard_product(WA, L) <= c["limit"]
    if want_guard is not None:
        assert ic.guard_product(WA, L) == want_guard
    cls = ic.tile_classes(cost, N)
    full = N // ic.TILE if N >= ic.TILE else 1  # (a lone partial tile counts: it holds the case)
    assert (cls[:, :full] == c["intended"]).all(), (c["name"], np.unique(cls[:, :full]))
    # a select row's extremes lie within one aligned group of four nodes of
    # some tile: one lane sees the whole span
    if c["intended"] == "select":
        g = np.zeros((P, -(-N // 4) * 4), np.int64)
        g[:, :N] = cost
        g = g.reshape(P, -1, 4)
        assert ((g.max(2) - g.min(2)).max(1) >= ic.E26 - 1).all()
    for p, n, v in c["planted"]:
        assert cost[p, n] == v, (c["name"], p, n, v, cost[p, n])
    return cost


@pytest.mark.parametrize("name", list(ic.CASES))
def test_small_cases(name):
    c = ic.case(name)
    cls = name.split("-")[0]
    at_limit = cls in ("ceiling_select", "ceiling_packed", "floor_packed")
    want = ic.LIMIT if at_limit else ic.LIMIT // 128 * 128 if cls == "lmax128" else None
    cost = check_case(c, want)
    P, N = c["WA"].shape
    if at_limit:  # every row is at the limit, not only the largest
        assert (np.abs(c["WA"].astype(np.int64)).sum(1) == ic.LIMIT).all()
    if cls == "lmax128":
        assert c["L"].min() == -128 and c["L"].max() == 127
        assert (cost > 0).any(1).all() and (cost < 0).any(1).all()
    # the planted extremes: the largest planted magnitude, in the signs the class names
    vals = {v for _, _, v in c["planted"]}
    ext = max(abs(v) for v in vals)
    want_vals = {"ceiling_select": {ic.LIMIT, ic.LIMIT - 1, -ic.LIMIT, -(ic.LIMIT - 1)},
                 "ceiling_packed": {ic.LIMIT, ic.LIMIT - (ic.E26 - 2)},
                 "floor_packed": {-ic.LIMIT, -ic.LIMIT + ic.E26 - 2},
                 "lmax128": {ic.LIMIT // 128 * 128, -(ic.LIMIT // 128 * 128)}}.get(cls)
    if want_vals:
        assert vals == want_vals
    # ties at the extreme between two nodes of one pod
    by_pod = {}
    for p, n, v in c["planted"]:
        if abs(v) == ext:
            by_pod.setdefault((p, v), []).append(n)
    assert any(len(ns) >= 2 for ns in by_pod.values())
    # the oracle places pods on planted extremes, and for some pods only the
    # exclusive group's nodes fit
    node, score, _ = oracle.place(c["WA"], c["L"], c["req"], c["free"], "i8")
    on_ext = [p for (p, v), ns in by_pod.items() if node[p] in ns]
    assert on_ext, name
    assert all(score[p] == cost[p, node[p]] for p in on_ext)
    assert (node < 0).sum() <= P // 10
    fit = oracle.fit_mask(c["req"], c["free"])
    nfit = np.array([sum(bin(int(w)).count("1") for w in row) for row in fit[:24]])
    assert (nfit == len(c["excl"][0])).sum() >= 8
    # a tie at the extreme goes to the lower node
    tied = [(p, ns) for (p, v), ns in by_pod.items() if len(ns) >= 2 and node[p] in ns]
    wn, wc, wcnt = oracle.topk(cost, fit, 8)
    for p, ns in tied:
        got = [n for n in wn[p, :wcnt[p]].tolist() if n in ns]
        assert got == sorted(got)


@pytest.mark.parametrize("name", ["ceiling_select-130", "floor_packed-256"])
def test_crowded_cases(name):
    c = ic.crowded(ic.case(name))
    check_case(c, ic.LIMIT)
    # lists run dry: far more pods share a best node than it has pod slots
    cost = oracle.cost(c["WA"], c["L"], "i8")
    best = np.bincount(cost.argmin(1), minlength=cost.shape[1])
    assert best.max() > 4 * c["free"][:, 2].min()


@pytest.mark.parametrize("name", ["ceiling_select-257", "ceiling_packed-256"])
def test_wide_cases(name):
    c = ic.case(name, ic.WIDE_P)
    assert c["WA"].shape[0] >= 32768  # the wide tile's threshold (nas_api.hip)
    check_case(c, ic.LIMIT)


def test_csr_sums_to_the_dense_traffic():
    from kubernetesnetawarescheduler_amd import workloads
    c = ic.case("ceiling_select-130")
    rng = np.random.default_rng(5)
    row_ptr, peer, w = ic.csr_of(c["WA"], rng)
    N = c["WA"].shape[1]
    ok = peer >= 0
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    dense = np.zeros(c["WA"].shape, np.int64)
    np.add.at(dense, (rows[ok], peer[ok]), w[ok].astype(np.int64))
    assert np.array_equal(dense, c["WA"])
    assert np.array_equal(workloads.csr_to_dense(row_ptr, peer, w, N), c["WA"])
    # colliding peers: aggregates at the limit are made of several weights
    coll = np.bincount(rows[ok] * N + peer[ok], minlength=dense.size).reshape(dense.shape)
    assert ((coll >= 2) & (np.abs(dense) == ic.LIMIT)).any()
    assert (~ok).any()
