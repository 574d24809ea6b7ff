"""Node selectors and taints on the GPU (include/nas.h nas_upload_*_constraints):
while constraints are uploaded, "fits" means eligible AND the three resources
fit -- in nas_filter's words, the candidate lists, nas_place, the host-driven
score_range / commit loop and timings.unschedulable.

The reference is constraint_ref.place, a sequential Python loop over
oracle.cost (pinned to oracle.place by tests/test_constraints_cpu.py).  int8
unless stated, so every comparison is exact equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import constraint_ref as cref
import oracle
from kubernetesnetawarescheduler_amd import Engine, NasError, _lib
from kubernetesnetawarescheduler_amd.sharded import place_local_shards
from util import cluster

pytestmark = pytest.mark.gpu
U64 = np.uint64


@pytest.fixture(scope="module")
def own_engine():
    """An Engine of this module's own: constraints are context state, and the
    session's shared Engine must reach the other modules as they expect it."""
    with Engine(0) as e:
        yield e


@pytest.fixture
def eng(own_engine):
    """Every test starts and ends without constraints and with default options."""
    own_engine.clear_constraints()
    yield own_engine
    own_engine.clear_constraints()
    own_engine.set_option("COST_CACHE", 2)
    own_engine.set_option("HERD_PLAN", 2)


def upload(e, WA, L, free, req, dtype="i8"):
    e.upload_latency(L, dtype)
    e.upload_capacity(free)
    e.upload_pods(req)
    e.upload_traffic(WA, dtype)


def constrain(e, words):
    lab, tnt, rq, tl = words
    e.upload_node_constraints(lab, tnt)
    e.upload_pod_constraints(rq, tl)
    return cref.eligible(lab, tnt, rq, tl)


def check_place(e, WA, L, req, free, elig, dtype="i8"):
    """One pass against the reference; the eligibility rule first and on its
    own, so a failure names the rule broken."""
    node, cf, ci = e.place()
    placed = np.flatnonzero(node >= 0)
    assert elig[placed, node[placed]].all(), "a pod sits on an ineligible node"
    want, wcost, wfree = cref.place(WA, L, req, free, elig, dtype)
    assert node.tolist() == want.tolist()
    if dtype == "i8":
        assert ci.tolist() == wcost.tolist()
    else:
        assert np.array_equal(cf.astype(np.float64), wcost)
    assert (e.get_capacity() == wfree).all()
    t = e.timings()
    assert t["unschedulable"] == int((want < 0).sum())
    return want, t


# ------------------------------------------------------------ 1. filter words
@pytest.mark.parametrize("pat,cap", [("allfit", 20.0), ("nolabel", 0.07), ("mix", 0.07),
                                     ("mix", 20.0)])
@pytest.mark.parametrize("P,N", [(3, 5), (257, 129), (1000, 300), (513, 1000)])
def test_filter_words(eng, P, N, pat, cap):
    """Engine.filter() (k_fit2: pod 0 is even) = oracle.fit_mask's resource
    words AND the eligibility words; the same bits through k_fit (score_range
    from the odd pod 1): complete candidate lists hold exactly the fitting
    nodes and every usable prefix is the reference ranking."""
    rng = np.random.default_rng(P * 7 + N)
    # cap 20: every request fits every node, so the chunk's AND / OR of the
    # words alone decide between the all-fit word, the zero word and the
    # per-pod ballots; cap 0.07: about half the (pod, node) pairs fit by
    # resources, so resource and eligibility bits mix in every chunk
    WA, L, free, req = cluster(rng, P, N, cap_scale=cap)
    upload(eng, WA, L, free, req)
    elig = constrain(eng, cref.pattern(pat, rng, P, N))
    want32 = cref.fits32(req, free, elig)
    got = eng.filter()
    assert got.shape == (-(-N // 64), P)
    assert (got == cref.words64(want32)).all()
    if pat == "nolabel":
        assert not got.any()
    if pat == "allfit":  # every valid node of every chunk, padding bits clear
        assert (want32 == oracle.fit_mask(req, free)).all()
        assert int(np.unpackbits(want32.view(np.uint8)).sum()) == P * N
    if P < 2:
        return
    eng.score_range(1, P)
    node, ci, _, cnt, complete = eng.candidates()
    wn, wc, wcnt = oracle.topk(oracle.cost(WA, L, "i8"), want32, 8)
    for p in range(1, P):
        c = cnt[p]
        assert c >= min(4, wcnt[p]), p
        assert node[p, :c].tolist() == wn[p, :c].tolist(), p
        assert ci[p, :c].tolist() == wc[p, :c].tolist(), p
        if complete[p]:
            assert c == wcnt[p] < 8, p


# -------------------------------------------------------------- 2. candidates
@pytest.mark.parametrize("P,N,lo,hi", [(700, 1500, -128, 127), (256, 256, 0, 20)])
def test_candidates(eng, P, N, lo, hi):
    rng = np.random.default_rng(P + N)
    WA, L, free, req = cluster(rng, P, N, lo=lo, hi=hi, cap_scale=0.1)
    upload(eng, WA, L, free, req)
    elig = constrain(eng, cref.pattern("mix", rng, P, N))
    eng.score()
    node, ci, _, cnt, complete = eng.candidates()
    wn, wc, wcnt = oracle.topk(oracle.cost(WA, L, "i8"), cref.fits32(req, free, elig), 8)
    assert (cnt >= np.minimum(4, wcnt)).all()
    for p in range(P):
        c = cnt[p]
        assert node[p, :c].tolist() == wn[p, :c].tolist(), p
        assert ci[p, :c].tolist() == wc[p, :c].tolist(), p
        assert (node[p, c:] == -1).all()
        if complete[p]:
            assert c == wcnt[p] < 8
    keys, bounds = eng.candidate_keys()
    k2, b2 = eng.candidate_keys_range(3, P - 3)
    assert (k2 == keys[3:]).all() and (b2 == bounds[3:]).all()
    first = (keys[:, 0] & U64(0xFFFFFFFF)).astype(np.int64)
    has = cnt > 0
    assert (first[has] == wn[has, 0]).all()


# --------------------------------------------------------------- 3. placement
def boosted(rng, P, N, cap):
    WA, L, free, req = cluster(rng, P, N, lo=0, hi=60, cap_scale=cap)
    # test_place_i8_exact's locality boost: many pods want the same few nodes
    WA[:, : N // 10] = np.minimum(WA[:, : N // 10].astype(np.int32) + 60, 127).astype(np.int8)
    return WA, L, free, req


@pytest.mark.parametrize("P,N,cap", [(1200, 333, 0.05), (3000, 1000, 0.02)])
def test_place(eng, P, N, cap):
    rng = np.random.default_rng(P ^ N)
    WA, L, free, req = boosted(rng, P, N, cap)
    upload(eng, WA, L, free, req)
    elig = constrain(eng, cref.pattern("mix", rng, P, N))
    want, _ = check_place(eng, WA, L, req, free, elig)
    assert (want < 0).any() and (want >= 0).any()
    # the words persist across uploads of the same shape
    eng.upload_capacity(free)
    eng.upload_pods(req)
    check_place(eng, WA, L, req, free, elig)


# ------------------------------------------------- 4. cordon == zero capacity
def test_cordon_equals_zero_capacity(eng):
    P, N = 1200, 333
    rng = np.random.default_rng(41)
    WA, L, free, req = boosted(rng, P, N, 0.05)
    cordoned = rng.random(N) < 1 / 3
    tnt = np.where(cordoned, U64(1), U64(0))
    upload(eng, WA, L, free, req)
    eng.upload_node_constraints(None, tnt)  # node words alone: nobody tolerates
    node, _, ci = eng.place()
    zeroed = free.copy()
    zeroed[cordoned] = 0
    want, wcost, wfree = oracle.place(WA, L, req, zeroed, "i8")
    assert not cordoned[node[node >= 0]].any(), "a pod sits on a cordoned node"
    assert node.tolist() == want.tolist()
    assert ci.tolist() == wcost.tolist()
    left = eng.get_capacity()
    assert (left[~cordoned] == wfree[~cordoned]).all()
    assert (left[cordoned] == free[cordoned]).all()  # untouched
    assert eng.timings()["unschedulable"] == int((want < 0).sum())


# ------------------------------------------------- 5. herd, cache forced on
def test_herd_with_forced_cache(eng):
    """test_rescore_path_runs's herd; half the pods barred from nodes 0..3 by a
    label.  The cost-row cache cannot be used under constraints: placements
    must be right with NAS_OPT_COST_CACHE forced to 1 (and the herd plan on),
    and with both off."""
    rng = np.random.default_rng(77)
    P, N = 2000, 256
    WA, L, free, req = cluster(rng, P, N, lo=0, hi=30, cap_scale=0.02)
    WA[:, :8] = 127  # everyone wants nodes 0..7
    lab = np.where(np.arange(N) >= 4, U64(1), U64(0))
    rq = np.where(rng.random(P) < 0.5, U64(1), U64(0))
    words = (lab, np.zeros(N, U64), rq, np.zeros(P, U64))
    upload(eng, WA, L, free, req)
    elig = constrain(eng, words)
    for opt in (1, 0):
        eng.set_option("COST_CACHE", opt)
        eng.set_option("HERD_PLAN", opt)
        for _ in range(2):  # (the second pass runs with the first one's slot hints)
            eng.reset_capacity()
            _, t = check_place(eng, WA, L, req, free, elig)
            assert t["rescore_rounds"] > 0, (opt, t)


# --------------------------------------------------------- 6. zero-traffic pods
def test_zero_traffic_pods_skip_tainted_nodes(eng):
    """The smallest exhausting shape of test_gpu_zero_traffic.py; half the
    traffic rows empty.  A zero-traffic pod takes the lowest-numbered node
    that fits, and the lowest-numbered roomy nodes are tainted: a
    capacity-only scan past an exhausted list would choose them."""
    rng = np.random.default_rng(5)
    P, N = 700, 100
    WA, L, free, req = cluster(rng, P, N, cap_scale=0.02)
    WA[rng.random(P) < 0.5] = 0
    free[:30] *= 4  # roomy
    tnt = np.where(np.arange(N) < 30, U64(2), U64(0))
    tl = np.where(rng.random(P) < 0.1, U64(2), U64(0))
    words = (np.zeros(N, U64), tnt, np.zeros(P, U64), tl)
    upload(eng, WA, L, free, req)
    elig = constrain(eng, words)
    want, _ = check_place(eng, WA, L, req, free, elig)
    assert (want < 0).any()
    # the host-driven loop on the same context
    eng.reset_capacity()
    node, score, _ = place_local_shards([eng], P)
    wnode, wcost, wfree = cref.place(WA, L, req, free, elig)
    assert node.tolist() == wnode.tolist()
    assert score.tolist() == wcost.tolist()
    assert (eng.get_capacity() == wfree).all()


# -------------------------------------------- 7. past the wide-tile threshold
def test_switching_at_the_wide_tile_threshold(eng):
    """33,000 pods: an unconstrained pass takes the wide tile with the fused
    fit, a constrained one k_fit + the 256 x 256 tile -- and back, and again."""
    P, N = 33000, 256
    rng = np.random.default_rng(33)
    WA, L, free, req = cluster(rng, P, N, lo=0, hi=30, cap_scale=0.3)
    words = cref.pattern("mix", rng, P, N)
    upload(eng, WA, L, free, req)
    elig = constrain(eng, words)
    ref = cref.place(WA, L, req, free, elig)
    plain = oracle.place(WA, L, req, free, "i8")
    assert ref[0].tolist() != plain[0].tolist()

    def run(want):
        eng.reset_capacity()
        node, _, ci = eng.place()
        assert node.tolist() == want[0].tolist()
        assert ci.tolist() == want[1].tolist()
        assert (eng.get_capacity() == want[2]).all()

    run(ref)
    eng.clear_constraints()
    run(plain)
    constrain(eng, words)
    run(ref)


# -------------------------------------------------------------------- 8. bf16
def test_place_bf16_integer_valued(eng):
    P, N = 500, 200
    rng = np.random.default_rng(P + 3 * N)
    WA, L, free, req = cluster(rng, P, N, dtype="bf16", lo=0, hi=16, cap_scale=0.05)
    upload(eng, WA, L, free, req, "bf16")
    elig = constrain(eng, cref.pattern("mix", rng, P, N))
    check_place(eng, WA, L, req, free, elig, "bf16")


# ------------------------------------------------------------- 9. node shards
@pytest.mark.parametrize("G", [2, 3])
def test_local_group_node_shards(G):
    """A local group of G ranks equals the world-1 pass and the reference
    (constraints_shard_worker.py).  In a child process: an in-process group
    runs on CU-masked streams, each a hardware queue of its own that stays in
    the process-wide pool until the process exits, and the suite's
    timing-sensitive herd tests must not find more queues alive than the
    modules before this one left them."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "constraints_shard_worker.py")
    r = subprocess.run([sys.executable, worker, str(G)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert f"G={G} ok" in r.stdout


# ------------------------------------------------------------------ 10. errors
def test_size_mismatch_and_batch_errors(eng):
    P, N = 300, 70
    rng = np.random.default_rng(10)
    WA, L, free, req = cluster(rng, P, N, cap_scale=0.05)
    plain = oracle.place(WA, L, req, free, "i8")

    def check_plain(e):
        e.clear_constraints()
        e.reset_capacity()
        node, _, ci = e.place()
        assert node.tolist() == plain[0].tolist() and ci.tolist() == plain[1].tolist()

    upload(eng, WA, L, free, req)
    eng.upload_node_constraints(np.zeros(N + 1, U64), None)
    with pytest.raises(NasError) as ex:
        eng.place()
    assert ex.value.code == _lib.NAS_ERR_ARG
    assert str(N + 1) in str(ex.value) and str(N) in str(ex.value)
    with pytest.raises(NasError) as ex:
        eng.filter()
    assert ex.value.code == _lib.NAS_ERR_ARG
    check_plain(eng)
    eng.upload_pod_constraints(None, np.zeros(P - 1, U64))
    with pytest.raises(NasError) as ex:
        eng.place()
    assert ex.value.code == _lib.NAS_ERR_ARG
    assert str(P - 1) in str(ex.value) and str(P) in str(ex.value)
    check_plain(eng)
    with Engine(0) as e:  # a batch refuses constraints, constraints refuse a batch
        e.upload_node_constraints(np.zeros(N, U64), None)
        with pytest.raises(NasError) as ex:
            e.set_batch(2)
        assert ex.value.code == _lib.NAS_ERR_UNSUPPORTED
        upload(e, WA, L, free, req)
        check_plain(e)
    with Engine(0) as e:
        e.set_batch(2)
        for call in (lambda: e.upload_node_constraints(np.zeros(N, U64), None),
                     lambda: e.upload_pod_constraints(np.zeros(P, U64), None)):
            with pytest.raises(NasError) as ex:
                call()
            assert ex.value.code == _lib.NAS_ERR_UNSUPPORTED
        upload(e, np.stack([WA, WA]), np.stack([L, L]), np.stack([free, free]),
               np.stack([req, req]))
        node, _, ci = e.place()
        for b in range(2):
            assert node[b].tolist() == plain[0].tolist() and ci[b].tolist() == plain[1].tolist()
