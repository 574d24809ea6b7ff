"""int8-path costs at the int32 limits and at the seams of the key packing.

The operands come from tests/int_range_cases.py (held to their claims on the
CPU by test_int_range_cases_cpu.py): costs planted at +-LIMIT, rows whose
costs lie 2^26 - 2 under the ceiling or above the floor, and rows on either
side of the thresholds at which the cost epilogue (k_cost.hip) changes its key
coding.  Everything is compared with the sequential oracle for equality:
candidate lists with exact integer costs, placements, scores, the capacity
left and the unschedulable count -- through the narrow and the wide tile, a
batch, node shards, CSR traffic, the cost-row cache under the herd plan, and
with constraints uploaded.

The guard (include/nas.h): a problem is refused when some pod's sum_m |WA[p,
m]| * max|L| exceeds LIMIT = INT32_MAX - 1.  INT32_MAX itself is not
accepted: its key word is all-ones, the word that means "does not fit".
Measured while the guard still accepted INT32_MAX (ceiling_select, N = 130,
pod 0: traffic INT32_MAX to node 5, only nodes 5 and 77 fit, both at cost
INT32_MAX): the oracle places pod 0 on node 5, the engine returned -1 -- an
empty list reported complete, from the select path; and on cached rescores
(crowded ceiling_packed, N = 256, pod 12: expected node 126, returned -1).
The packed codings ranked the same cost correctly."""
import numpy as np
import pytest

import constraint_ref as cref
import int_range_cases as ic
import oracle
from kubernetesnetawarescheduler_amd import Engine, LocalGroup, NasError, _lib, local_ranks

pytestmark = pytest.mark.gpu

_WANT = {}


def expect(c):
    """The oracle's answers for a case, computed once: cost, fit words, the
    8-lists and the sequential placement."""
    key = (c["name"], len(c["WA"]))
    if key not in _WANT:
        cost = oracle.cost(c["WA"], c["L"], "i8")
        mask = oracle.fit_mask(c["req"], c["free"])
        _WANT[key] = dict(cost=cost, mask=mask, topk=oracle.topk(cost, mask, 8),
                          place=oracle.place(c["WA"], c["L"], c["req"], c["free"], "i8"))
    return _WANT[key]


def upload(e, c, csr=None):
    e.upload_latency(c["L"], "i8")
    e.upload_capacity(c["free"])
    e.upload_pods(c["req"])
    if csr is None:
        e.upload_traffic(c["WA"], "i8")
    else:
        e.upload_traffic_csr(*csr, "i8", c["WA"].shape[1])


def check_lists(got, want_topk, tag=""):
    """test_candidates_i8_exact's form: the usable prefix is the oracle's
    ranking (nodes and exact integer costs), count >= min(4, #fitting), a
    complete list holds every fitting node."""
    node, ci, _, cnt, complete = got
    wn, wc, wcnt = want_topk
    assert (cnt >= np.minimum(4, wcnt)).all(), tag
    use = np.arange(8)[None, :] < cnt[:, None]
    bad = np.flatnonzero(((node != wn) & use).any(1) | ((ci != wc) & use).any(1))
    assert len(bad) == 0, (tag, bad[:4], node[bad[:4]], wn[bad[:4]], ci[bad[:4]], wc[bad[:4]])
    assert (node[~use] == -1).all(), tag
    assert (cnt[complete] == wcnt[complete]).all() and (wcnt[complete] < 8).all(), tag


def check_place(got, cap, want, tag=""):
    node, cf, ci = got
    wnode, wcost, wfree = want
    bad = np.flatnonzero(node != wnode)
    assert len(bad) == 0, (tag, bad[:6], node[bad[:6]], wnode[bad[:6]])
    assert np.array_equal(ci, wcost), tag
    if cf is not None:
        assert np.array_equal(cf, wcost.astype(np.float32)), tag
    assert (cap == wfree).all(), tag


def score_and_place(e, c, tag=""):
    w = expect(c)
    e.reset_capacity()
    e.score()
    check_lists(e.candidates(), w["topk"], tag)
    e.reset_capacity()
    got = e.place()
    check_place(got, e.get_capacity(), w["place"], tag)
    t = e.timings()
    assert t["unschedulable"] == int((w["place"][0] < 0).sum()), tag
    return t


# ------------------------------------------------- 1. every class, narrow tile
@pytest.mark.parametrize("name", list(ic.CASES))
def test_class_lists_and_placement(engine, name):
    c = ic.case(name)
    upload(engine, c)
    score_and_place(engine, c, name)


# ------------------------------------------------------------ 2. the wide tile
@pytest.mark.parametrize("name", ["ceiling_select-257", "ceiling_packed-256"])
def test_wide_tile(engine, name):
    c = ic.case(name, ic.WIDE_P)
    upload(engine, c)
    score_and_place(engine, c, name)


# ------------------------------------------------------------------- 3. batch
@pytest.mark.parametrize("names", [("ceiling_select", "floor_packed", "span_edge"),
                                   ("direct_edge", "offset_edge", "ceiling_packed")])
def test_batch_of_three_classes(names):
    """P = 900: Pp = 1,024 pods split into 768 on the wide tile and 256 on the
    narrow one (score_batch); every cluster another class."""
    P, N = 900, 256
    make = {"ceiling_select": lambda: ic.ceiling_select(P, N), "floor_packed": lambda: ic.packed(P, N, -1),
            "ceiling_packed": lambda: ic.packed(P, N, +1), "span_edge": lambda: ic.span_edge(P, ic.E26 - 1),
            "direct_edge": lambda: ic.direct_edge(P, ic.E26 - 2),
            "offset_edge": lambda: ic.offset_edge(P, ic.E26)}
    cs = [make[n]() for n in names]
    with Engine(0) as e:
        e.set_batch(3)
        e.upload_latency(np.stack([c["L"] for c in cs]), "i8")
        e.upload_capacity(np.stack([c["free"] for c in cs]))
        e.upload_pods(np.stack([c["req"] for c in cs]))
        e.upload_traffic(np.stack([c["WA"] for c in cs]), "i8")
        e.score()
        lists = e.candidates()
        e.reset_capacity()
        node, cf, ci = e.place()
        cap = e.get_capacity()
        t = e.timings()
    unsched = 0
    for b, c in enumerate(cs):
        w = expect(c)
        rows = slice(b * P, (b + 1) * P)
        check_lists([a[rows] for a in lists], w["topk"], (b, c["name"]))
        check_place((node[b], cf[b], ci[b]), cap[b], w["place"], (b, c["name"]))
        unsched += int((w["place"][0] < 0).sum())
    assert t["unschedulable"] == unsched


# -------------------------------------------------------------- 4. node shards
@pytest.mark.parametrize("G,name", [(2, "ceiling_select-257"), (3, "ceiling_select-257"),
                                    (3, "lmax128-257")])
def test_node_shards(G, name):
    """N = 257 over G ranks of an in-process group: uneven shards, the last
    one ending on the copied column."""
    c = ic.case(name)
    w = expect(c)
    group = LocalGroup(G)
    engines = [Engine(0) for _ in range(G)]
    try:
        def run(r, e):
            e.set_option("COMM_TIMEOUT_MS", 60000)
            e.comm_init_local(group, r)
            upload(e, c)
            e.reset_capacity()
            got = e.place()
            return got, e.get_capacity(), e.timings()
        res = local_ranks(engines, run)
    finally:
        for e in engines:
            e.close()
        group.close()
    for r, (got, cap, t) in enumerate(res):
        check_place(got, cap, w["place"], (G, r))
        assert t["unschedulable"] == int((w["place"][0] < 0).sum())


# ------------------------------------------------------------------- 5. CSR
@pytest.mark.parametrize("name", ["ceiling_select-130", "floor_packed-256", "lmax128-257"])
def test_csr_int32_aggregates_at_the_limit(engine, name):
    """The same traffic as colliding int32 peer weights of both signs whose
    aggregates land exactly on the planted values (+-LIMIT among them)."""
    c = ic.case(name)
    csr = ic.csr_of(c["WA"], np.random.default_rng(11))
    upload(engine, c, csr)
    rows, _, _, _ = engine.read_inputs(0, len(c["WA"]), want_L=False)
    assert np.array_equal(rows, c["WA"])
    score_and_place(engine, c, name)


# ------------------------------------------- 6. cost-row cache under herd plan
@pytest.mark.parametrize("name", ["ceiling_select-130", "floor_packed-256"])
def test_cached_keys_at_the_limits(engine, name):
    """Crowded variants: lists run dry, and the rescores read the cached key
    words (k_rescore_cached) of costs at +-LIMIT."""
    c = ic.crowded(ic.case(name))
    engine.set_option("COST_CACHE", 1)
    engine.set_option("HERD_PLAN", 1)
    try:
        upload(engine, c)
        t = score_and_place(engine, c, name)
        assert t["rescore_rounds"] > 0, t
    finally:
        engine.set_option("COST_CACHE", 2)
        engine.set_option("HERD_PLAN", 2)


# ------------------------------------------------------------- 7. constraints
@pytest.mark.parametrize("name", ["ceiling_select-257", "ceiling_packed-256"])
def test_with_constraints(name):
    """Node and pod constraints uploaded: k_fit_c and the masked narrow tile."""
    c = ic.case(name)
    P, N = c["WA"].shape
    lab, tnt, rq, tl = cref.pattern("mix", np.random.default_rng(3), P, N)
    # (the exclusive pods keep their nodes: no requirement, every taint tolerated)
    rq[:24], tl[:24] = 0, ~np.uint64(0)
    elig = cref.eligible(lab, tnt, rq, tl)
    want = cref.place(c["WA"], c["L"], c["req"], c["free"], elig)
    with Engine(0) as e:
        upload(e, c)
        e.upload_node_constraints(lab, tnt)
        e.upload_pod_constraints(rq, tl)
        e.score()
        check_lists(e.candidates(),
                    oracle.topk(expect(c)["cost"], cref.fits32(c["req"], c["free"], elig), 8), name)
        e.reset_capacity()
        got = e.place()
        check_place(got, e.get_capacity(), want, name)
        assert e.timings()["unschedulable"] == int((want[0] < 0).sum())
        ext = {(p, n) for p, n, v in c["planted"] if abs(v) == ic.LIMIT}
        assert any((p, int(n)) in ext for p, n in enumerate(want[0]))


# ---------------------------------------------------------- 8. guard boundary
GP, GN = 77, 96  # pods (no multiple of a tile), nodes (more than 64)


def guard_base(rng, lmax=1):
    """Small in-plane traffic (row sums far below the limit), latency within
    +-lmax with the extreme present, roomy capacity."""
    WA = rng.integers(-100, 101, (GP, GN)).astype(np.int64)
    if lmax == 1:
        L = rng.integers(-1, 2, (GN, GN))
        L[0, 0] = -1
    else:
        L = rng.integers(-128, 128, (GN, GN))
        L[0, 0] = -128
    free = np.stack([rng.integers(2000, 8000, GN), rng.integers(2_000_000, 8_000_000, GN),
                     np.full(GN, 3)], 1).astype(np.int32)
    req = np.stack([rng.integers(1, 540, GP), rng.integers(7_464, 303_749, GP),
                    np.ones(GP, np.int64)], 1).astype(np.int32)
    return WA, L.astype(np.int8), free, req


def _row(kind, rng, total):
    """A traffic row (GN,) int64 with sum_m |row[m]| == total, the sum carried
    the way `kind` says."""
    row = np.zeros(GN, np.int64)
    if kind == "plane":
        # every column holds an in-plane value, -128 and 127 and the last
        # column among them; one entry past int8 makes up the rest
        row[:] = rng.integers(-128, 128, GN)
        row[0], row[1], row[GN - 1], row[5], row[7] = -128, 127, -128, 5, 0
        row[7] = total - np.abs(row).sum()
    elif kind == "positive":
        row[[3, 64, GN - 1]] = ic._split(rng, total - 3 * 128, 3) + 128
    elif kind == "negative":
        row[[0, 65, GN - 2]] = -(ic._split(rng, total - 3 * 129, 3) + 129)
    elif kind == "many":  # 70 entries past int8, of both signs
        cols = rng.choice(GN, 70, replace=False)
        row[cols] = (ic._split(rng, total - 70 * 129, 70) + 129) * rng.choice([-1, 1], 70)
    else:
        raise ValueError(kind)
    assert np.abs(row).sum() == total
    return row


def _bump(row, kind):
    """The same row with sum |.| one larger, the 1 added where `kind` carries it."""
    row = row.copy()
    if kind == "plane":
        assert 0 <= row[5] < 127
        row[5] += 1  # an in-plane entry: the plane's own sum decides
    else:
        m = np.flatnonzero(np.abs(row) > 128)[-1]
        row[m] += 1 if row[m] > 0 else -1
    return row


def refused_then_exact(e, over, upload_over, fine, upload_fine, lists=True):
    """`over` (guard product LIMIT + 1) is refused by score and place alike;
    then `fine` (LIMIT) is accepted on the same context with exact results."""
    WA1, L, free, req = over
    WA0 = fine[0]
    lmax = int(np.abs(L.astype(np.int64)).max())
    assert ic.guard_product(WA0, L) == ic.LIMIT // lmax * lmax
    assert ic.guard_product(WA1, L) == ic.LIMIT // lmax * lmax + lmax > ic.LIMIT
    upload_over(e)
    for call in (e.score, e.place):
        with pytest.raises(NasError) as ei:
            call()
        assert ei.value.code == _lib.NAS_ERR_UNSUPPORTED
    upload_fine(e)
    cost = oracle.cost(WA0, L, "i8")
    if lists:
        e.score()
        check_lists(e.candidates(), oracle.topk(cost, oracle.fit_mask(req, free), 8))
        e.reset_capacity()
    got = e.place()
    check_place(got, e.get_capacity(), oracle.place(WA0, L, req, free, "i8"))


def _dense(c):
    def up(e):
        WA, L, free, req = c
        e.upload_latency(L, "i8")
        e.upload_capacity(free)
        e.upload_pods(req)
        e.upload_traffic(WA, "i8")
    return up


@pytest.mark.parametrize("kind,pod", [("plane", 9), ("positive", 9), ("negative", 9), ("many", 9),
                                      ("positive", GP - 1)])
def test_guard_boundary_dense(engine, kind, pod):
    """The deciding row sum carried by the int8 plane (an exact LIMIT from
    plane entries alone would take 131,072 nodes: here one entry past int8
    holds the bulk and an in-plane entry decides), by positive entries past
    int8, by -128 plane entries with negative excess, by more than 64 entries
    past int8 -- on an inner pod and on the last."""
    rng = np.random.default_rng(len(kind) * 100 + pod)
    WA, L, free, req = guard_base(rng)
    WA[pod] = _row(kind, rng, ic.LIMIT)
    over = WA.copy()
    over[pod] = _bump(WA[pod], kind)
    refused_then_exact(engine, (over, L, free, req), _dense((over, L, free, req)),
                       (WA, L, free, req), _dense((WA, L, free, req)))


def test_guard_boundary_lmax128(engine):
    """max|L| = 128 through L = -128: row sum LIMIT // 128 accepted, one more refused."""
    rng = np.random.default_rng(128)
    WA, L, free, req = guard_base(rng, lmax=128)
    assert L.min() == -128 and L.max() < 128
    WA[9] = _row("many", rng, ic.LIMIT // 128)
    over = WA.copy()
    over[9] = _bump(WA[9], "many")
    refused_then_exact(engine, (over, L, free, req), _dense((over, L, free, req)),
                       (WA, L, free, req), _dense((WA, L, free, req)))


def test_guard_boundary_csr(engine):
    """The deciding aggregate made of colliding int32 peer weights."""
    rng = np.random.default_rng(77)
    WA, L, free, req = guard_base(rng)
    WA[9] = _row("many", rng, ic.LIMIT)
    over = WA.copy()
    over[9] = _bump(WA[9], "many")

    def csr(W):
        parts = ic.csr_of(W, np.random.default_rng(5))

        def up(e):
            e.upload_latency(L, "i8")
            e.upload_capacity(free)
            e.upload_pods(req)
            e.upload_traffic_csr(*parts, "i8", GN)
        return up
    refused_then_exact(engine, (over, L, free, req), csr(over), (WA, L, free, req), csr(WA))


def test_guard_boundary_batch_cluster_2():
    """The deciding row in cluster b = 2 of a batch of three."""
    rng = np.random.default_rng(2)
    cs = [guard_base(rng) for _ in range(3)]
    cs[2][0][GP - 2] = _row("positive", rng, ic.LIMIT)
    over = cs[2][0].copy()
    over[GP - 2] = _bump(over[GP - 2], "positive")

    def up(e, last):
        e.upload_latency(np.stack([c[1] for c in cs]), "i8")
        e.upload_capacity(np.stack([c[2] for c in cs]))
        e.upload_pods(np.stack([c[3] for c in cs]))
        e.upload_traffic(np.stack([cs[0][0], cs[1][0], last]), "i8")

    with Engine(0) as e:
        e.set_batch(3)
        up(e, over)
        for call in (e.score, e.place):
            with pytest.raises(NasError) as ei:
                call()
            assert ei.value.code == _lib.NAS_ERR_UNSUPPORTED
        up(e, cs[2][0])
        node, cf, ci = e.place()
        cap = e.get_capacity()
        for b, (WA, L, free, req) in enumerate(cs):
            check_place((node[b], cf[b], ci[b]), cap[b], oracle.place(WA, L, req, free, "i8"), b)
