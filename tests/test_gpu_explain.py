"""nas_explain on the GPU (include/nas.h NAS_WHY_*, k_explain.hip): per-reason
node counts of the listed pods over all nodes, against the working capacity at
the time of the call.  Integer counts, so every comparison with the numpy
reference (explain_ref.py) is exact equality."""
import ctypes

import numpy as np
import pytest

import constraint_ref as cref
import explain_ref as xref
from kubernetesnetawarescheduler_amd import Engine, NasError, _lib
from kubernetesnetawarescheduler_amd._lib import ptr
from util import cluster

pytestmark = pytest.mark.gpu
U64 = np.uint64
I32_MAX = 2**31 - 1
# N below / at / above one 64-node chunk, beyond one node slab (1,024 nodes),
# P below / at / above one 64-pod group and no multiple of it
SHAPES = [(1, 1), (3, 5), (65, 63), (64, 64), (130, 65), (257, 129), (700, 1100)]


@pytest.fixture(scope="module")
def own_engine():
    """An Engine of this module's own: constraints are context state."""
    with Engine(0) as e:
        yield e


@pytest.fixture
def eng(own_engine):
    own_engine.clear_constraints()
    yield own_engine
    own_engine.clear_constraints()


def upload(e, WA, L, free, req, words=None):
    e.upload_latency(L, "i8")
    e.upload_capacity(free)
    e.upload_pods(req)
    e.upload_traffic(WA, "i8")
    if words is None:
        e.clear_constraints()
    else:
        e.upload_node_constraints(words[0], words[1])
        e.upload_pod_constraints(words[2], words[3])


def one_node(e, free, req, label=0, taint=0, require=0, tolerate=0, words=True):
    """One node, one pod -> the pod's record."""
    z = np.zeros((1, 1), np.int8)
    w = [np.array([v], U64) for v in (label, taint, require, tolerate)] if words else None
    upload(e, z, z, np.array([free], np.int32), np.array([req], np.int32), w)
    got = e.explain()
    assert got.shape == (1, 8) and got.dtype == np.int32
    if words:
        assert got.tolist() == xref.explain([req], [free], *w).tolist()
    else:
        assert got.tolist() == xref.explain([req], [free]).tolist()
    return got[0].tolist()


# ------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("P,N", SHAPES)
def test_equals_reference(eng, P, N):
    """The shared generator's instance with its words, then with the
    constraints cleared (TAINT = SELECTOR = 0)."""
    WA, L, free, req, words = xref.case(P, N)
    upload(eng, WA, L, free, req, words)
    want = xref.explain(req, free, *words)
    got = eng.explain()
    assert got.shape == (P, 8) and got.dtype == np.int32
    assert (got == want).all(), np.argwhere(got != want)[:8].tolist()
    c = got
    assert (c[:, [xref.TAINT, xref.SELECTOR, xref.RESOURCES, xref.FIT]].sum(1) == N).all()
    if P >= 65:  # (the CPU test pins that the generator gets there)
        assert (c[:, :xref.NODES] > 0).any(0).all()
    eng.clear_constraints()
    got = eng.explain()
    want = xref.explain(req, free)
    assert (got == want).all(), np.argwhere(got != want)[:8].tolist()
    assert not got[:, [xref.TAINT, xref.SELECTOR]].any()


def test_one_side_of_the_words_only(eng):
    """A side never uploaded is all zero: node words alone close a tainted node
    to every pod, pod words alone make every non-zero require unsatisfiable."""
    P, N = 130, 65
    WA, L, free, req, (lab, tnt, rq, tl) = xref.case(P, N)
    upload(eng, WA, L, free, req)
    eng.upload_node_constraints(lab, tnt)
    assert (eng.explain() == xref.explain(req, free, lab, tnt)).all()
    eng.clear_constraints()
    eng.upload_pod_constraints(rq, tl)
    got = eng.explain()
    assert (got == xref.explain(req, free, None, None, rq, tl)).all()
    assert (got[rq != 0, xref.SELECTOR] == N).all()


# ------------------------------------------------------------------ 2. pod lists
def test_pod_lists(eng):
    P, N = 257, 129
    WA, L, free, req, words = xref.case(P, N)
    upload(eng, WA, L, free, req, words)
    want = xref.explain(req, free, *words)
    rng = np.random.default_rng(5)
    # a shuffled subset with duplicates, longer than one 64-pod group
    pods = rng.permutation(P)[:90].astype(np.int32)
    pods = np.concatenate([pods, pods[:17], [pods[3]] * 5, [0, P - 1]]).astype(np.int32)
    rng.shuffle(pods)
    got = eng.explain(pods)
    assert got.shape == (len(pods), 8)
    assert (got == want[pods]).all()
    assert (eng.explain([P - 1]) == want[P - 1:]).all()
    assert (eng.explain(np.arange(P)[::-1]) == want[::-1]).all()
    # pods = NULL with n_pods < P: pods 0 .. n_pods-1
    for n in (1, 64, 100):
        out = np.full((n + 1, 8), -7, np.int32)
        assert eng._L.nas_explain(eng._h, None, n, ptr(out)) == _lib.NAS_OK
        assert (out[:n] == want[:n]).all() and (out[n] == -7).all()
    # n_pods == 0 is NAS_OK and writes nothing
    out = np.full((1, 8), -7, np.int32)
    assert eng._L.nas_explain(eng._h, None, 0, ptr(out)) == _lib.NAS_OK
    assert eng._L.nas_explain(eng._h, None, 0, None) == _lib.NAS_OK
    assert (out == -7).all()
    assert eng.explain(np.zeros(0, np.int32)).shape == (0, 8)


# ---------------------------------------------------------- 3. decisive operands
@pytest.mark.parametrize("words", [False, True])
@pytest.mark.parametrize("r", [0, 1, 2])
def test_one_resource_decides(eng, r, words):
    """One node; resource r alone decides, the other two fit with room."""
    slot = (xref.CPU, xref.MEM, xref.PODS)[r]
    for f in (0, 1, 1000, I32_MAX - 1, I32_MAX):
        free = [5000, 5000, 5000]
        free[r] = f
        req = [10, 10, 10]
        req[r] = f  # req == free: equality fits
        assert one_node(eng, free, req, words=words) == [0, 0, 0, 0, 0, 0, 1, 1]
        if f < I32_MAX:
            req[r] = f + 1  # one more: short in r alone
            want = [0, 0, 1, 0, 0, 0, 0, 1]
            want[slot] = 1
            assert one_node(eng, free, req, words=words) == want
        if f > 0:
            req[r] = f - 1
            assert one_node(eng, free, req, words=words) == [0, 0, 0, 0, 0, 0, 1, 1]
    # free 0 takes only a zero request; an all-zero request fits an empty node
    assert one_node(eng, [0, 0, 0], [0, 0, 0], words=words) == [0, 0, 0, 0, 0, 0, 1, 1]
    assert one_node(eng, [I32_MAX] * 3, [I32_MAX] * 3, words=words) == [0, 0, 0, 0, 0, 0, 1, 1]
    assert one_node(eng, [0, 0, 0], [1, 1, 1], words=words) == [0, 0, 1, 1, 1, 1, 0, 1]


def test_word_bits_decide(eng):
    """One node; label bit 63 and taint bit 63, and the ownership order."""
    hi = 1 << 63
    fit, sel, tnt = [0, 0, 0, 0, 0, 0, 1, 1], [0, 1, 0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 0, 0, 1]
    free, req, big = [100, 100, 1], [100, 100, 1], [101, 101, 2]
    assert one_node(eng, free, req, label=hi, require=hi) == fit
    assert one_node(eng, free, req, label=hi - 1, require=hi) == sel
    assert one_node(eng, free, req, label=hi, require=hi | 1) == sel
    assert one_node(eng, free, req, taint=hi, tolerate=hi) == fit
    assert one_node(eng, free, req, taint=hi, tolerate=hi - 1) == tnt
    assert one_node(eng, free, req, taint=hi | 1, tolerate=hi) == tnt
    # the first failing filter owns the node: taint before selector before resources
    assert one_node(eng, free, big, taint=hi, require=hi) == tnt
    assert one_node(eng, free, big, require=hi) == sel
    assert one_node(eng, free, big, label=hi, require=hi, taint=1, tolerate=1) == \
        [0, 0, 1, 1, 1, 1, 0, 1]


# -------------------------------------------------------- 4. constraint patterns
@pytest.mark.parametrize("P,N", [(130, 65), (257, 1100)])
def test_allfit_and_nolabel_patterns(eng, P, N):
    """One class takes every node: every pod fits every node / no node carries
    the required label."""
    rng = np.random.default_rng(P * 7 + N)
    WA, L, free, req = cluster(rng, P, N, cap_scale=20)
    words = cref.pattern("allfit", rng, P, N)
    upload(eng, WA, L, free, req, words)
    got = eng.explain()
    assert (got == xref.explain(req, free, *words)).all()
    assert (got[:, xref.FIT] == N).all() and not got[:, :xref.FIT].any()
    words = cref.pattern("nolabel", rng, P, N)
    upload(eng, WA, L, free, req, words)
    got = eng.explain()
    assert (got == xref.explain(req, free, *words)).all()
    assert (got[:, xref.SELECTOR] == N).all() and not got[:, xref.FIT].any()


def test_taint_on_every_node(eng):
    """A taint every node carries: the pods that do not tolerate it count all N
    nodes under TAINT whatever else is short, the others only the nodes with
    the second taint."""
    P, N = 70, 200
    WA, L, free, req, (lab, tnt, rq, tl) = xref.case(P, N)
    tnt = tnt | (U64(1) << U64(7))
    tl[::2] |= U64(1) << U64(7)
    upload(eng, WA, L, free, req, (lab, tnt, rq, tl))
    got = eng.explain()
    assert (got == xref.explain(req, free, lab, tnt, rq, tl)).all()
    assert (got[1::2, xref.TAINT] == N).all() and (got[::2, xref.TAINT] < N).all()


# ------------------------------------------------------------- 5. after a pass
def test_after_a_pass(eng):
    P, N = 600, 300
    rng = np.random.default_rng(P * 7 + N)
    WA, L, free, req = cluster(rng, P, N, cap_scale=0.07)
    words = cref.pattern("mix", rng, P, N)
    upload(eng, WA, L, free, req, words)
    node, _, _ = eng.place()
    t = eng.timings()
    left = eng.get_capacity()
    assert (left != free).any()
    got = eng.explain()
    assert (got == xref.explain(req, left, *words)).all()
    none = node < 0
    assert none.any() and (~none).any()
    assert (got[none, xref.FIT] == 0).all()
    assert int(none.sum()) == t["unschedulable"]
    # blocking, and nas_timings is not touched
    assert eng.timings() == t
    assert (eng.explain(np.flatnonzero(none)) == got[none]).all()


# --------------------------------------------------------------- 6. node shard
def test_node_shard_counts_the_whole_cluster(eng):
    P, N = 130, 300
    WA, L, free, req, words = xref.case(P, N)
    upload(eng, WA, L, free, req, words)
    want = eng.explain()
    assert (want == xref.explain(req, free, *words)).all()
    with Engine(0) as s:
        s.set_shard(1, 2)
        upload(s, WA, L, free, req, words)
        assert (s.explain() == want).all()
        s.clear_constraints()
        assert (s.explain() == xref.explain(req, free)).all()


# ------------------------------------------------------------------- 7. errors
def test_errors_leave_the_context_usable(eng):
    P, N = 65, 63
    WA, L, free, req, words = xref.case(P, N)
    upload(eng, WA, L, free, req, words)
    want = xref.explain(req, free, *words)
    for bad in ([P], [-1], [0, 1, P, 2], [3, -1]):
        with pytest.raises(NasError) as ex:
            eng.explain(bad)
        assert ex.value.code == _lib.NAS_ERR_ARG
        assert (eng.explain([0, P - 1]) == want[[0, P - 1]]).all()
    out = np.zeros((P + 1, 8), np.int32)
    assert eng._L.nas_explain(eng._h, None, -1, ptr(out)) == _lib.NAS_ERR_ARG
    assert eng._L.nas_explain(eng._h, None, P + 1, ptr(out)) == _lib.NAS_ERR_ARG
    assert eng._L.nas_explain(eng._h, None, P, None) == _lib.NAS_ERR_ARG
    assert (eng.explain() == want).all()
    # words of another shape
    eng.upload_pod_constraints(words[2][:P - 1], words[3][:P - 1])
    with pytest.raises(NasError) as ex:
        eng.explain()
    assert ex.value.code == _lib.NAS_ERR_ARG
    eng.upload_pod_constraints(words[2], words[3])
    assert (eng.explain() == want).all()


def test_state_and_batch_errors():
    with Engine(0) as e:
        with pytest.raises(NasError) as ex:  # before uploads
            e.explain([0])
        assert ex.value.code == _lib.NAS_ERR_STATE
        WA, L, free, req, _ = xref.case(3, 5)
        e.upload_capacity(free)
        with pytest.raises(NasError) as ex:  # capacity alone
            e.explain([0])
        assert ex.value.code == _lib.NAS_ERR_STATE
        e.upload_pods(req)
        assert (e.explain() == xref.explain(req, free)).all()  # capacity and pods suffice
    with Engine(0) as e:
        e.set_batch(2)
        WA, L, free, req = cluster(np.random.default_rng(1), 4, 6)
        rep = lambda a: np.stack([a, a])  # noqa: E731
        e.upload_latency(rep(L), "i8")
        e.upload_capacity(rep(free))
        e.upload_pods(rep(req))
        e.upload_traffic(rep(WA), "i8")
        with pytest.raises(NasError) as ex:
            e.explain([0])
        assert ex.value.code == _lib.NAS_ERR_UNSUPPORTED
        node = e.place()[0].reshape(-1)  # still usable
        assert node.shape[0] == 8 and (node[:4] == node[4:]).all() and (node >= 0).all()
