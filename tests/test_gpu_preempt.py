"""nas_preempt on the GPU (include/nas.h, k_preempt.hip): per listed pod the
node to take and the lower-priority bound pods to evict there, against the
working capacity and the bound table at the time of the call.  All integer, so
every comparison with the plain-Python reference (preempt_ref.py) is exact
equality."""
import functools

import numpy as np
import pytest

import preempt_ref as pref
from kubernetesnetawarescheduler_amd import Engine, NasError, _lib
from kubernetesnetawarescheduler_amd._lib import ptr
from util import cluster

pytestmark = pytest.mark.gpu
U64 = np.uint64
I32_MAX, I32_MIN, BIAS = 2**31 - 1, -2**31, 2**31
EMPTY = (-1, 0, 0, 0, 0)
# N below / at / above one 64-node chunk, beyond one node slab (512 nodes) and
# beyond four of them (the pick reduces five slabs' partials), P below / at /
# above one 64-entry group and no multiple of it
SHAPES = [(1, 1), (5, 3), (63, 65), (64, 64), (65, 130), (129, 257), (70, 1100), (33, 2100)]


@pytest.fixture(scope="module")
def own_engine():
    """An Engine of this module's own: constraints and bound pods are context state."""
    with Engine(0) as e:
        yield e


@pytest.fixture
def eng(own_engine):
    own_engine.clear_constraints()
    yield own_engine
    own_engine.clear_constraints()


def upload(e, c, bound=True):
    e.upload_latency(c["L"], "i8")
    e.upload_capacity(c["free"])
    e.upload_pods(c["req"])
    e.upload_traffic(c["WA"], "i8")
    if c["words"] is None:
        e.clear_constraints()
    else:
        e.upload_node_constraints(*c["words"][:2])
        e.upload_pod_constraints(*c["words"][2:])
    if bound:
        e.upload_bound(*c["bound"])


@functools.lru_cache(maxsize=None)
def solved(P, N, profile, pat=None):
    """The shared instance and its reference answer with 80 victim slots
    (computed once; tests only read them)."""
    c = pref.case(P, N, profile, pat)
    want = pref.preempt(c["req"], c["prio"], c["free"], c["bound"], pref.elig_of(c["words"]), 80)
    return c, want


def small(e, free, req, bound=None, words=None):
    """A hand-made cluster (zero latency and traffic); bound = (node, priority,
    req) or None for an empty table."""
    free = np.asarray(free, np.int32).reshape(-1, 3)
    req = np.asarray(req, np.int32).reshape(-1, 3)
    c = dict(L=np.zeros((len(free), len(free)), np.int8), WA=np.zeros((len(req), len(free)), np.int8),
             free=free, req=req, words=words, bound=bound)
    upload(e, c, bound=False)
    if bound is None:
        e.upload_bound([], [], np.zeros((0, 3), np.int32))
    else:
        e.upload_bound(*bound)


def ask(e, prio, free, req, bound=None, words=None, mv=4):
    """Every pod of `req` with its priority -> (records, victims) as lists,
    checked against the reference."""
    got, vict = e.preempt(prio, max_victims=mv)
    elig = pref.elig_of(None if words is None else [np.asarray(w, U64) for w in words])
    want, wvict = pref.preempt(req, prio, free, bound, elig, mv)
    assert got.tolist() == want.tolist() and vict.tolist() == wvict.tolist()
    return got.tolist(), vict.tolist()


def one(e, r, pi, free, bound=None, words=None, mv=4):
    """One pod on a hand-made cluster -> (record, victims)."""
    small(e, free, [r], bound, words)
    got, vict = ask(e, [pi], free, [r], bound, words, mv)
    return got[0], vict[0]


# ------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("pat", [None, "mix"])
@pytest.mark.parametrize("profile", pref.PROFILES)
@pytest.mark.parametrize("P,N", SHAPES)
def test_equals_reference(eng, P, N, profile, pat):
    c, (want, wvict) = solved(P, N, profile, pat)
    upload(eng, c)
    for mv in (80, 2, 0):
        got, vict = eng.preempt(c["prio"], max_victims=mv)
        assert got.dtype == _lib.PREEMPTION_DTYPE and got.shape == (P,)
        assert vict.dtype == np.int32 and vict.shape == (P, mv)
        bad = np.flatnonzero(got != want.astype(got.dtype))
        assert len(bad) == 0, (bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
        assert (vict == wvict[:, :mv]).all(), np.argwhere(vict != wvict[:, :mv])[:8].tolist()
    assert (wvict[:, -1] == -1).all()  # 80 slots held every victim list whole


# ------------------------------------------------------------------ 2. pod lists
def test_pod_lists(eng):
    P, N = 129, 257
    c, (want, wvict) = solved(P, N, "tight")
    upload(eng, c)
    rng = np.random.default_rng(5)
    # a shuffled subset with duplicates, longer than one 64-entry group
    pods = rng.permutation(P)[:90].astype(np.int32)
    pods = np.concatenate([pods, pods[:17], [pods[3]] * 5, [0, P - 1]]).astype(np.int32)
    rng.shuffle(pods)
    got, vict = eng.preempt(c["prio"][pods], pods, max_victims=3)
    assert got.shape == (len(pods),) and vict.shape == (len(pods), 3)
    assert (got == want[pods]).all() and (vict == wvict[pods, :3]).all()
    # the priority belongs to the list entry, not to the pod
    other = np.where(c["prio"][pods] == 50, -3, 50).astype(np.int32)
    w2, v2 = pref.preempt(c["req"][pods], other, c["free"], c["bound"], None, 3)
    got, vict = eng.preempt(other, pods, max_victims=3)
    assert (got == w2).all() and (vict == v2).all()
    got, _ = eng.preempt(c["prio"][::-1], np.arange(P)[::-1])
    assert (got == want[::-1]).all()
    # pods = NULL with n_pods < P: pods 0 .. n_pods-1; past n_pods nothing is written
    for n in (1, 64, 100):
        out = np.full(n + 1, -7, _lib.PREEMPTION_DTYPE)
        v = np.full((n + 1, 2), -7, np.int32)
        assert eng._L.nas_preempt(eng._h, None, ptr(c["prio"]), n, ptr(out), ptr(v), 2) == _lib.NAS_OK
        assert (out[:n] == want[:n]).all() and out[n].tolist() == (-7,) * 5
        assert (v[:n] == wvict[:n, :2]).all() and (v[n] == -7).all()
    # n_pods == 0 is NAS_OK and writes nothing
    out = np.full(1, -7, _lib.PREEMPTION_DTYPE)
    v = np.full((1, 2), -7, np.int32)
    assert eng._L.nas_preempt(eng._h, None, ptr(c["prio"]), 0, ptr(out), ptr(v), 2) == _lib.NAS_OK
    assert eng._L.nas_preempt(eng._h, None, None, 0, None, None, 0) == _lib.NAS_OK
    assert out[0].tolist() == (-7,) * 5 and (v == -7).all()
    got, vict = eng.preempt(np.zeros(0, np.int32), np.zeros(0, np.int32), max_victims=2)
    assert got.shape == (0,) and vict.shape == (0, 2)


# ---------------------------------------------------------- 3. decisive operands
@pytest.mark.parametrize("r", [0, 1, 2])
def test_one_resource_decides(eng, r):
    """One node with one bound pod of priority 0, a pod of priority 1; resource
    r alone decides, the other two fit with room.  free + bound == request
    evicts and fits, one more unit fits nowhere."""
    M = I32_MAX

    def run(f, q, want_r):
        free, breq, req = [5000] * 3, [10] * 3, [20] * 3
        free[r], breq[r], req[r] = f, q, want_r
        return one(eng, req, 1, [free], ([0], [0], [breq]))[0]

    stays, goes = (0, 0, 0, 1, 0), (0, 1, 0, 1, BIAS)
    assert run(0, 0, 0) == stays and run(0, 0, 1) == EMPTY
    assert run(0, 1, 1) == goes and run(0, 1, 2) == EMPTY and run(0, 1, 0) == stays
    assert run(1, 0, 1) == stays and run(1, 0, 2) == EMPTY
    assert run(1, 1, 2) == goes and run(1, 1, 3) == EMPTY and run(1, 1, 1) == stays
    assert run(0, M, M) == goes and run(0, M - 1, M) == EMPTY
    assert run(1, M - 1, M) == goes and run(1, M - 2, M) == EMPTY
    assert run(M, 0, M) == stays and run(M - 1, 0, M) == EMPTY
    # free + bound passes int32: the sum is taken in 64 bits
    assert run(M, M, M) == stays and run(M - 1, M, M) == goes
    assert run(M, M, 0) == stays and run(M - 1, 1, M) == goes


def test_priority_decides(eng):
    """Priority pi - 1 is a victim, pi is not, at the int32 limits too."""
    for pi in (0, 7, I32_MAX, I32_MIN + 1):
        bound = lambda p: ([0], [p], [(100, 0, 0)])  # noqa: E731
        assert one(eng, (100, 0, 0), pi, [(0, 0, 0)], bound(pi - 1)) == \
            ((0, 1, pi - 1, 1, pi - 1 + BIAS), [0, -1, -1, -1])
        assert one(eng, (100, 0, 0), pi, [(0, 0, 0)], bound(pi))[0] == EMPTY
    # nothing is below INT32_MIN
    assert one(eng, (100, 0, 0), I32_MIN, [(0, 0, 0)], ([0], [I32_MIN], [(100, 0, 0)]))[0] == EMPTY


def test_ineligible_node_is_never_chosen(eng):
    """Node 0 is empty but tainted / lacks the label; node 1 needs a victim."""
    free, bound = [(9000, 9000, 9), (0, 0, 0)], ([1], [0], [(100, 0, 0)])
    hi = 1 << 63
    for lab, tnt, rq, tl in (([0, 0], [hi, 0], [0], [0]), ([0, hi], [0, 0], [hi], [0])):
        words = (lab, tnt, rq, tl)
        words = [np.array(w, U64) for w in words]
        assert one(eng, (100, 0, 0), 1, free, bound, words) == ((1, 1, 0, 1, BIAS), [0, -1, -1, -1])
        # and when the other node cannot help, no node is chosen
        assert one(eng, (200, 0, 0), 1, free, bound, words)[0] == EMPTY
    assert one(eng, (100, 0, 0), 1, free, bound)[0] == (0, 0, 0, 2, 0)


# --------------------------------------------------------------- 4. reprieve order
def test_reprieve_order(eng):
    # three lower pods: the first would leave too little, the middle one can
    # stay, the last cannot any more
    bound = ([0, 0, 0], [3, 2, 1], [(300, 0, 0), (100, 0, 0), (100, 0, 0)])
    assert one(eng, (400, 0, 0), 9, [(0, 0, 0)], bound) == \
        ((0, 2, 3, 1, 4 + 2 * BIAS), [0, 2, -1, -1])
    # the walk is by priority, not by bound index
    bound = ([0, 0, 0], [1, 2, 3], [(100, 0, 0), (100, 0, 0), (300, 0, 0)])
    assert one(eng, (400, 0, 0), 9, [(0, 0, 0)], bound) == \
        ((0, 2, 3, 1, 4 + 2 * BIAS), [2, 0, -1, -1])
    # equal priorities walk by bound index: swapping the two swaps the victim
    a = ([0, 0], [2, 2], [(100, 0, 0), (200, 0, 0)])
    b = ([0, 0], [2, 2], [(200, 0, 0), (100, 0, 0)])
    assert one(eng, (200, 0, 0), 9, [(0, 0, 0)], a) == ((0, 1, 2, 1, 2 + BIAS), [1, -1, -1, -1])
    assert one(eng, (200, 0, 0), 9, [(0, 0, 0)], b) == ((0, 1, 2, 1, 2 + BIAS), [0, -1, -1, -1])


# ------------------------------------------------------------------- 5. the ladder
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("level", ["top", "sum", "count", "index"])
def test_ladder(eng, level, swap):
    """Two nodes that differ at exactly one level of the key, in both orders."""
    A, B, (nv, top, psum) = pref.ladder_cases()[level]
    need = sum(q[0] for q in A[1])
    got, _ = one(eng, (need, 0, 0), 9, [(0, 0, 0)] * 2, pref.ladder_bound(A, B, swap))
    assert got == (0 if level == "index" else int(swap), nv, top, 2, psum)


def test_victimless_beats_any_victims(eng):
    bound = ([0], [I32_MIN], [(100, 0, 0)])
    assert one(eng, (100, 0, 0), 0, [(0, 0, 0), (100, 0, 0)], bound)[0] == (1, 0, 0, 2, 0)
    assert one(eng, (100, 0, 0), 0, [(0, 0, 0), (99, 0, 0)], bound) == \
        ((0, 1, I32_MIN, 1, 0), [0, -1, -1, -1])


# -------------------------------------------------------------- 6. the bound table
def test_no_table_is_the_lowest_fitting_node():
    free = [(100, 0, 0), (300, 0, 0), (300, 0, 0)]
    req = [(200, 0, 0), (100, 0, 0), (400, 0, 0)]
    want = [(1, 0, 0, 2, 0), (0, 0, 0, 3, 0), EMPTY]
    with Engine(0) as e:  # never uploaded
        e.upload_capacity(np.array(free, np.int32))
        e.upload_pods(np.array(req, np.int32))
        assert ask(e, [5, 5, 5], free, req)[0] == want
        # uploaded, then cleared with B == 0 (NULL arrays)
        bound = ([0, 2], [1, 1], [(100, 0, 0), (100, 0, 0)])
        e.upload_bound(*bound)
        assert ask(e, [5, 5, 5], free, req, bound)[0] == \
            [(1, 0, 0, 3, 0), (0, 0, 0, 3, 0), (2, 1, 1, 1, 1 + BIAS)]
        assert e._L.nas_upload_bound(e._h, None, None, None, None, None, 0) == _lib.NAS_OK
        assert ask(e, [5, 5, 5], free, req)[0] == want


def test_reupload_replaces_the_table(eng):
    free, req = [(0, 0, 0)] * 2, [(100, 0, 0)]
    small(eng, free, req, ([0], [1], [(100, 0, 0)]))
    assert ask(eng, [5], free, req, ([0], [1], [(100, 0, 0)]))[0] == [(0, 1, 1, 1, 1 + BIAS)]
    bound = ([1, 1], [2, 3], [(50, 0, 0), (50, 0, 0)])
    eng.upload_bound(*bound)
    assert ask(eng, [5], free, req, bound) == ([(1, 2, 3, 1, 5 + 2 * BIAS)], [[1, 0, -1, -1]])


def test_long_rows(eng):
    """A node with 70 bound pods (longer than a wave), and every bound pod of
    the cluster on one node."""
    rng = np.random.default_rng(70)
    for N, at in ((1, 0), (3, 1), (130, 129)):
        B = 70 if N == 1 else 300
        bound = (np.full(B, at, np.int32), rng.integers(-5, 30, B).astype(np.int32),
                 np.stack([rng.integers(0, 4, B) * 100, rng.integers(0, 3, B) * 1000,
                           rng.integers(0, 2, B)], 1).astype(np.int32))
        free = np.zeros((N, 3), np.int32)
        req = np.stack([rng.integers(0, 60, 40) * 100, rng.integers(0, 40, 40) * 1000,
                        rng.integers(0, 20, 40)], 1).astype(np.int32)
        prio = rng.choice([-6, 0, 10, 29, 30], 40).astype(np.int32)
        small(eng, free, req, bound)
        got, vict = ask(eng, prio, free, req, bound, mv=80)
        assert max(g[1] for g in got) > 20 and min(g[0] for g in got) == -1
        assert all(g[0] in (at, -1) for g in got)


# ----------------------------------------------------------------- 7. after a pass
def test_after_a_pass(eng):
    P, N = 129, 257
    c, _ = solved(P, N, "roomy", "mix")
    upload(eng, c)
    node, _, _ = eng.place()
    t = eng.timings()
    left = eng.get_capacity()
    assert (left != c["free"]).any()
    none = np.flatnonzero(node < 0).astype(np.int32)
    assert len(none) and len(none) < P
    got, vict = eng.preempt(c["prio"][none], none, max_victims=8)
    want, wvict = pref.preempt(c["req"][none], c["prio"][none], left, c["bound"],
                               pref.elig_of(c["words"])[none], 8)
    assert (got == want).all() and (vict == wvict).all()
    # a pod the pass could not place fits no node as it is
    assert ((got["n_victims"] > 0) | (got["node"] == pref.EMPTY)).all()
    assert (got["n_victims"] > 0).any() and (got["node"] == pref.EMPTY).any()
    # blocking, and nas_timings is not touched
    assert eng.timings() == t


# ------------------------------------------------------------------ 8. node shard
def test_node_shard_answers_for_the_whole_cluster():
    P, N = 65, 130
    c, (want, wvict) = solved(P, N, "tight", "mix")
    with Engine(0) as s:
        s.set_shard(1, 2)
        upload(s, c)
        got, vict = s.preempt(c["prio"], max_victims=80)
        assert (got == want).all() and (vict == wvict).all()
        assert (got["node"][got["node"] >= 0] < N // 2).any()  # winners outside the shard
        s.clear_constraints()
        w2, v2 = solved(P, N, "tight")[1]
        got, vict = s.preempt(c["prio"], max_victims=80)
        assert (got == w2).all() and (vict == v2).all()


# ----------------------------------------------------------------------- 9. errors
def code_of(fn, *a, **k):
    with pytest.raises(NasError) as ex:
        fn(*a, **k)
    return ex.value


def test_errors_leave_the_context_usable(eng):
    P, N = 63, 65
    c, (want, wvict) = solved(P, N, "tight", "mix")
    upload(eng, c)
    prio = c["prio"]

    def still_right():
        got, vict = eng.preempt(prio, max_victims=80)
        assert (got == want).all() and (vict == wvict).all()

    for bad in ([P], [-1], [0, 1, P, 2], [3, -1]):
        assert code_of(eng.preempt, prio[:len(bad)], bad).code == _lib.NAS_ERR_ARG
        still_right()
    out = np.zeros(P + 1, _lib.PREEMPTION_DTYPE)
    v = np.zeros((P + 1, 2), np.int32)
    pp = np.zeros(P + 1, np.int32)
    call = eng._L.nas_preempt
    assert call(eng._h, None, ptr(pp), -1, ptr(out), None, 0) == _lib.NAS_ERR_ARG
    assert call(eng._h, None, ptr(pp), P + 1, ptr(out), None, 0) == _lib.NAS_ERR_ARG
    assert call(eng._h, None, ptr(pp), P, None, None, 0) == _lib.NAS_ERR_ARG
    assert call(eng._h, None, None, P, ptr(out), None, 0) == _lib.NAS_ERR_ARG
    assert call(eng._h, None, ptr(pp), P, ptr(out), None, 2) == _lib.NAS_ERR_ARG
    assert call(eng._h, None, ptr(pp), P, ptr(out), ptr(v), -1) == _lib.NAS_ERR_ARG
    still_right()
    # words of another shape
    eng.upload_pod_constraints(c["words"][2][:P - 1], c["words"][3][:P - 1])
    assert code_of(eng.preempt, prio).code == _lib.NAS_ERR_ARG
    eng.upload_pod_constraints(*c["words"][2:])
    still_right()
    # a bad bound entry: the message names the first one, the table in place stays
    node, bp, br = c["bound"]
    B = len(node)
    for b, val in ((5, N), (7, -1)):
        bad = node.copy()
        bad[b], bad[B - 1] = val, N
        err = code_of(eng.upload_bound, bad, bp, br)
        assert err.code == _lib.NAS_ERR_ARG and f"node[{b}]" in str(err)
        still_right()
    bad = br.copy()
    bad[11, 1], bad[40, 0] = -1, -5
    err = code_of(eng.upload_bound, node, bp, bad)
    assert err.code == _lib.NAS_ERR_ARG and "bound pod 11" in str(err)
    cols = [np.ascontiguousarray(br[:, k]) for k in range(3)]
    assert eng._L.nas_upload_bound(eng._h, ptr(node), ptr(bp), *[ptr(x) for x in cols], -1) == \
        _lib.NAS_ERR_ARG
    assert eng._L.nas_upload_bound(eng._h, None, ptr(bp), *[ptr(x) for x in cols], B) == \
        _lib.NAS_ERR_ARG
    still_right()
    # a node whose bound requests sum above INT32_MAX
    big = br.copy()
    big[node == N - 1, 2] = 0
    on = np.flatnonzero(node == N - 1)[:2]
    big[on, 2] = I32_MAX // 2 + 1
    err = code_of(eng.upload_bound, node, bp, big)
    assert err.code == _lib.NAS_ERR_UNSUPPORTED and f"node {N - 1}" in str(err)
    still_right()
    big[on[1], 2] = I32_MAX // 2  # exactly INT32_MAX is held
    eng.upload_bound(node, bp, big)
    got, vict = eng.preempt(prio, max_victims=80)
    w2, v2 = pref.preempt(c["req"], prio, c["free"], (node, bp, big), pref.elig_of(c["words"]), 80)
    assert (got == w2).all() and (vict == v2).all()
    eng.upload_bound(node, bp, br)
    still_right()
    # capacity uploaded with another n: the table no longer matches the cluster
    c2, (want2, wvict2) = solved(5, 3, "tight")
    upload(eng, c2, bound=False)
    assert code_of(eng.preempt, c2["prio"]).code == _lib.NAS_ERR_ARG
    eng.upload_bound(*c2["bound"])
    got, vict = eng.preempt(c2["prio"], max_victims=80)
    assert (got == want2).all() and (vict == wvict2).all()


def test_state_and_batch_errors():
    c, (want, _) = solved(5, 3, "tight")
    with Engine(0) as e:
        assert code_of(e.preempt, [0], [0]).code == _lib.NAS_ERR_STATE  # before uploads
        assert code_of(e.upload_bound, *c["bound"]).code == _lib.NAS_ERR_STATE  # no capacity
        e.upload_capacity(c["free"])
        assert code_of(e.preempt, [0], [0]).code == _lib.NAS_ERR_STATE  # capacity alone
        e.upload_bound(*c["bound"])
        e.upload_pods(c["req"])
        assert (e.preempt(c["prio"])[0] == want).all()  # capacity, bound pods and pods suffice
    with Engine(0) as e:
        e.set_batch(2)
        WA, L, free, req = cluster(np.random.default_rng(1), 4, 6)
        rep = lambda a: np.stack([a, a])  # noqa: E731
        e.upload_latency(rep(L), "i8")
        e.upload_capacity(rep(free))
        e.upload_pods(rep(req))
        e.upload_traffic(rep(WA), "i8")
        assert code_of(e.preempt, [0], [0]).code == _lib.NAS_ERR_UNSUPPORTED
        assert code_of(e.upload_bound, [0], [0], [(1, 1, 1)]).code == _lib.NAS_ERR_UNSUPPORTED
        node = e.place()[0].reshape(-1)  # still usable
        assert node.shape[0] == 8 and (node[:4] == node[4:]).all() and (node >= 0).all()
