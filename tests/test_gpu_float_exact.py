"""The fp32 cost path (NAS_DT_F32: three bf16 planes per operand, six plane
products on the bf16 MFMA) and the bf16 path on operands for which every
product and partial sum is exact in fp32 (tests/float_cases.py; the conditions
are held by tests/test_float_cases_cpu.py).  Nothing here has a tolerance:
costs equal float32(oracle cost) bit for bit; candidate lists, placements and
remaining capacity equal the fp64 sequential oracle's.

The classes populate the m and l planes (a transposed entry of a plane
pattern shows at 2^-9 relative), the signed variants give negative costs and
the epilogue's exact select network, the positive ones its packed keys;
duplicated latency columns give bit-identical costs, where the lower node
index must win.  Shapes: N below one tile and below 64 (Kp all padding in each
of the six segments), odd sizes, the wide tile; then fp32 through node shards,
a cluster batch, node selectors and taints, the host-driven loop, the cost-row
cache and the herd plan."""
import numpy as np
import pytest

import constraint_ref as cref
import float_cases as fc
import oracle
from kubernetesnetawarescheduler_amd import Engine, LocalGroup, local_ranks
from kubernetesnetawarescheduler_amd.sharded import place_local_shards
from util import KEY_INVALID, merge_lists, usable

pytestmark = pytest.mark.gpu


def upload(e, WA, L, free, req, dtype="f32"):
    e.upload_latency(L, dtype)
    e.upload_capacity(free)
    e.upload_pods(req)
    e.upload_traffic(WA, dtype)


def fitting(req, free):
    return (req[:, None, :].astype(np.int64) <= free[None, :, :].astype(np.int64)).all(2)


def check_lists(e, WA, L, free, req, dtype="f32", pairs=()):
    """score() + candidates() against oracle.topk, as
    test_gpu_edge.py::test_wide_cost_range_exact_select_path: the nodes and
    cost_f of the first `count` entries, count >= min(4, fitting)."""
    e.score()
    node, _, cf, cnt, complete = e.candidates()
    cost = oracle.cost(WA, L, dtype)
    wn, wc, wcnt = oracle.topk(cost, oracle.fit_mask(req, free), 8)
    assert (cnt >= np.minimum(4, wcnt)).all()
    assert (wcnt == np.minimum(8, fitting(req, free).sum(1))).all()
    for p in range(len(req)):
        c = cnt[p]
        assert node[p, :c].tolist() == wn[p, :c].tolist(), p
        assert np.array_equal(cf[p, :c].astype(np.float64), wc[p, :c]), p
        assert (node[p, c:] == -1).all(), p
        if complete[p]:
            assert c == wcnt[p] < 8, p
        for a, b in pairs:  # bit-identical costs: the lower index first
            row = node[p, :c].tolist()
            if b in row:
                assert a in row[:row.index(b)] or not fitting(req[p:p + 1], free[a:a + 1])[0, 0], (p, a, b)
    return cost, cnt, wcnt


def check_place(e, WA, L, free, req, dtype="f32"):
    node, cf, _ = e.place()
    want, wcost, wfree = oracle.place(WA, L, req, free, dtype)
    bad = np.nonzero(node != want)[0]
    assert len(bad) == 0, (bad[:8], node[bad[:8]], want[bad[:8]])
    assert np.array_equal(cf.astype(np.float64), wcost)
    assert (e.get_capacity() == wfree).all()
    return want, wcost, wfree


# ------------------------------------------------------ small and odd shapes
@pytest.mark.parametrize("N", fc.SMALL_N)
@pytest.mark.parametrize("P", fc.SMALL_P)
@pytest.mark.parametrize("cls,signed", fc.VARIANTS)
def test_small_shapes_exact(engine, cls, signed, P, N):
    WA, L, _, free, req = fc.small_case(cls, signed, P, N)
    upload(engine, WA, L, free, req)
    cost, cnt, wcnt = check_lists(engine, WA, L, free, req)
    want, wcost, _ = check_place(engine, WA, L, free, req)
    if P > 1:
        assert (want < 0).any() and (want >= 0).any()  # tight: some pods find no node
        assert (wcnt < 8).any()                        # some lists run dry
        if N >= 63:
            assert (wcnt == 8).any()
            if signed:
                assert (wcost < 0).any() and (cost > 0).any()


# ----------------------------------------------------------------------- ties
@pytest.mark.parametrize("N", [2, 65, 257])
@pytest.mark.parametrize("cls,signed", [("L20xW1", True), ("M10x10", True), ("dyadic", False)])
def test_ties_lower_index_first_f32(engine, cls, signed, N):
    """Duplicated latency columns: both nodes of a pair cost every pod the
    same bits.  Rows of -0.0 traffic cost +0 on every node: all ties."""
    P = 300
    WA, L, pairs, free, req = fc.small_case(cls, signed, P, N, dup=5)
    WA = WA.copy()
    WA[::9] = -0.0
    assert pairs
    upload(engine, WA, L, free, req)
    check_lists(engine, WA, L, free, req, pairs=pairs)
    want, wcost, _ = check_place(engine, WA, L, free, req)
    copies = [b for _, b in pairs]
    assert np.isin(want, copies).any(), "no pod was left to a duplicate's higher index"
    assert (wcost[::9] == 0).all()


@pytest.mark.parametrize("N", [2, 65, 257])
def test_ties_lower_index_first_bf16(engine, N):
    P = 300
    rng = np.random.default_rng(N)
    WA, L, pairs = fc.int_bf16_operands(rng, P, N, dup=5)
    free, req = fc.tight_capacity(rng, P, N, slots=1 if N > 130 else 2)
    upload(engine, WA, L, free, req, "bf16")
    check_lists(engine, WA, L, free, req, "bf16", pairs=pairs)
    want, _, _ = check_place(engine, WA, L, free, req, "bf16")
    assert np.isin(want, [b for _, b in pairs]).any()


# ------------------------------------------------- wide tile with live planes
@pytest.mark.parametrize("cls", fc.WIDE_CLASSES)
def test_wide_tile_live_planes(engine, cls):
    """33,000 pods on one cluster at world 1: the 256 x 384 tile, here with
    non-zero m (and, in L20xW1, l) planes and costs of both signs."""
    WA, L, free, req = fc.wide_case(cls)
    upload(engine, WA, L, free, req)
    node, _, _ = engine.place()
    want, _, wfree = oracle.place(WA, L, req, free, "f32")
    bad = np.nonzero(node != want)[0]
    assert len(bad) == 0, (bad[:8], node[bad[:8]], want[bad[:8]])
    assert (engine.get_capacity() == wfree).all()
    assert (want < 0).any() and (want >= 0).any()


# ---------------------------------------------------------------- node shards
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("cls,signed", fc.COMP_VARIANTS)
def test_f32_local_group(cls, signed, G):
    """G ranks of an in-process group (nas_comm_init_local): 301 nodes do not
    divide by 3.  Every rank equals the oracle."""
    WA, L, free, req = fc.comp_case(cls, signed, f"group{G}")
    want, wcost, wfree = oracle.place(WA, L, req, free, "f32")
    group = LocalGroup(G)
    engines = [Engine(0) for _ in range(G)]
    try:
        def run(r, e):
            e.set_option("COMM_TIMEOUT_MS", 60000)
            e.comm_init_local(group, r)
            upload(e, WA, L, free, req)
            node, cf, _ = e.place()
            return node, cf, e.get_capacity(), e.timings()
        res = local_ranks(engines, run)
    finally:
        for e in engines:
            e.close()
        group.close()
    for r, (node, cf, cap, t) in enumerate(res):
        assert node.tolist() == want.tolist(), (G, r)
        assert np.array_equal(cf.astype(np.float64), wcost), (G, r)
        assert (cap == wfree).all(), (G, r)
        assert t["rescore_rounds"] > 0, (G, r, t)


def key_costs(keys):
    """The float cost in the high word of candidate keys (k_cost.hip okey:
    negative floats complemented, the others with the sign bit set)."""
    u = (keys >> np.uint64(32)).astype(np.uint32)
    bits = np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u)
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("cls,signed", fc.COMP_VARIANTS)
def test_f32_set_shard_host_merge(cls, signed, G):
    """nas_set_shard: every shard's lists stay inside its node columns; merged
    on the host (util.merge_lists) they are the oracle's ranking with its
    costs, and the host-exchange placement equals the oracle on every shard."""
    P, N = fc.COMP_SHAPE
    WA, L, free, req = fc.comp_case(cls, signed, "shard")
    cost = oracle.cost(WA, L, "f32")
    wn, wc, wcnt = oracle.topk(cost, oracle.fit_mask(req, free), 8)
    want, _, wfree = oracle.place(WA, L, req, free, "f32")
    engines, parts = [], []
    try:
        for r in range(G):
            e = Engine(0)
            engines.append(e)
            e.set_shard(r, G)
            upload(e, WA, L, free, req)
            e.score()
            keys, bounds = e.candidate_keys()
            parts.append((keys, bounds))
            nodes = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
            valid = keys != KEY_INVALID
            assert ((nodes[valid] >= r * N // G) & (nodes[valid] < (r + 1) * N // G)).all()
        mk, mb = merge_lists(parts)
        node, cnt = usable(mk, mb)
        assert (cnt >= np.minimum(4, wcnt)).all()
        kc = key_costs(mk)
        for p in range(P):
            assert node[p, :cnt[p]].tolist() == wn[p, :cnt[p]].tolist(), p
            assert np.array_equal(kc[p, :cnt[p]], wc[p, :cnt[p]]), p
        got, _, rounds = place_local_shards(engines, P)
        caps = [e.get_capacity() for e in engines]
    finally:
        for e in engines:
            e.close()
    assert rounds > 0
    assert got.tolist() == want.tolist()
    for c in caps:
        assert (c == wfree).all()


# ---------------------------------------------------------------------- batch
@pytest.mark.parametrize("dtype,cls,signed", [("f32",) + v for v in fc.COMP_VARIANTS] +
                         [("bf16", None, True)])
def test_batch_of_three_clusters(dtype, cls, signed):
    P, N = fc.COMP_SHAPE
    cs = []
    for b in range(3):
        if dtype == "f32":
            cs.append(fc.comp_case(cls, signed, f"batch{b}"))
        else:
            rng = np.random.default_rng(40 + b)
            WA, L, _ = fc.int_bf16_operands(rng, P, N)
            cs.append((WA, L) + fc.tight_capacity(rng, P, N))
    assert not np.array_equal(cs[0][0], cs[1][0]) and not np.array_equal(cs[1][1], cs[2][1])
    with Engine(0) as e:
        e.set_batch(3)
        e.upload_latency(np.stack([c[1] for c in cs]), dtype)
        e.upload_capacity(np.stack([c[2] for c in cs]))
        e.upload_pods(np.stack([c[3] for c in cs]))
        e.upload_traffic(np.stack([c[0] for c in cs]), dtype)
        node, cf, _ = e.place()
        cap = e.get_capacity()
    for b, (WA, L, free, req) in enumerate(cs):
        want, wcost, wfree = oracle.place(WA, L, req, free, dtype)
        assert node[b].tolist() == want.tolist(), b
        assert np.array_equal(cf[b].astype(np.float64), wcost), b
        assert (cap[b] == wfree).all(), b


# ---------------------------------------------------------------- constraints
@pytest.mark.parametrize("cls,signed", fc.COMP_VARIANTS)
def test_f32_constraints(cls, signed):
    """Mixed selector / taint words (constraint_ref.pattern "mix") in fp32,
    as test_gpu_constraints.py::test_place_bf16_integer_valued in bf16."""
    P, N = fc.COMP_SHAPE
    WA, L, free, req = fc.comp_case(cls, signed, "constraints")
    words = cref.pattern("mix", np.random.default_rng(P + N), P, N)
    elig = cref.eligible(*words)
    want, wcost, wfree = cref.place(WA, L, req, free, elig, "f32")
    plain, _, _ = oracle.place(WA, L, req, free, "f32")
    assert want.tolist() != plain.tolist()
    with Engine(0) as e:
        upload(e, WA, L, free, req)
        e.upload_node_constraints(words[0], words[1])
        e.upload_pod_constraints(words[2], words[3])
        node, cf, _ = e.place()
        cap = e.get_capacity()
        t = e.timings()
    placed = np.flatnonzero(node >= 0)
    assert elig[placed, node[placed]].all(), "a pod sits on an ineligible node"
    assert node.tolist() == want.tolist()
    assert np.array_equal(cf.astype(np.float64), wcost)
    assert (cap == wfree).all()
    assert t["unschedulable"] == int((want < 0).sum())


# ----------------------------------------------------------- host-driven loop
@pytest.mark.parametrize("cls,signed", fc.COMP_VARIANTS)
def test_f32_host_driven_loop(engine, cls, signed):
    """The loop of include/nas.h: score_range, get and set keys, commit, and
    score_range again at each stop -- equal to place() and to the oracle."""
    P, N = fc.COMP_SHAPE
    WA, L, free, req = fc.comp_case(cls, signed, "loop")
    upload(engine, WA, L, free, req)
    placed, wcost, wfree = check_place(engine, WA, L, free, req)
    engine.reset_capacity()

    def sync(lo, hi):
        engine.score_range(lo, hi)
        keys, bounds = engine.candidate_keys_range(lo, hi - lo)
        engine.set_candidate_keys(lo, keys, bounds)
        return keys

    keys = sync(0, P)
    node = np.full(P, -9, np.int32)
    stop, stops = 0, []
    while True:
        stop = engine.commit(stop, node)
        if stop >= P:
            break
        stops.append(stop)
        assert (node[:stop] != -9).all()
        hi = min(P, stop + 1024)
        keys[stop:hi] = sync(stop, hi)
    assert stops and stops == sorted(stops)
    assert node.tolist() == placed.tolist()
    assert (engine.get_capacity() == wfree).all()
    # the key each pod was placed from carries its cost (a pod without
    # traffic may sit past its list: the commit's zero-traffic scan)
    at = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64) == node[:, None]
    at &= keys != KEY_INVALID
    ok = (node >= 0) & (WA != 0).any(1)
    assert at[ok].any(1).all()
    first = at.argmax(1)
    assert np.array_equal(key_costs(keys[np.arange(P), first])[ok], wcost[ok])


# ------------------------------------------------------- cache and herd plan
@pytest.mark.parametrize("cache,herd", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("cls,signed", fc.COMP_VARIANTS)
def test_f32_cost_cache_and_herd_plan(engine, cls, signed, cache, herd):
    """Hot nodes with 3 pod slots each: every list runs dry on them, the walk
    halts and rescores -- from the cost-row cache (k_rescore_cached reads the
    float keys stored by the cost launches) when it is on."""
    WA, L, free, req = fc.cache_case(cls, signed)
    want, wcost, wfree = oracle.place(WA, L, req, free, "f32")
    engine.set_option("COST_CACHE", cache)
    engine.set_option("HERD_PLAN", herd)
    try:
        upload(engine, WA, L, free, req)
        for _ in range(2):
            engine.reset_capacity()
            node, cf, _ = engine.place()
            bad = np.nonzero(node != want)[0]
            assert len(bad) == 0, (bad[:8], node[bad[:8]], want[bad[:8]])
            assert np.array_equal(cf.astype(np.float64), wcost)
            assert (engine.get_capacity() == wfree).all()
            t = engine.timings()
            assert t["rescore_rounds"] > 0, t
            if cache:
                assert t["rescored_pods"] > 0, t
    finally:
        engine.set_option("COST_CACHE", 2)
        engine.set_option("HERD_PLAN", 2)
