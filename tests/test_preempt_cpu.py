"""CPU side of nas_preempt: the plain-Python reference of the GPU tests on hand
cases, what the shared generator reaches per profile and shape, and header /
binding agreement on the new names."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import preempt_ref as pref
from kubernetesnetawarescheduler_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN = -2**31
BIAS = 2**31
SLAB = 512  # nodes per block of k_preempt_scan (PR_SLAB)


def one(r, pi, free, bound=None, elig=None, mv=4):
    got, vict = pref.preempt([r], [pi], free, bound, elig, mv)
    return got[0].tolist(), vict[0].tolist()


# ------------------------------------------------------------------ hand cases
def test_reference_fits_as_is_or_nowhere():
    free = [(100, 1000, 1), (300, 3000, 1)]
    assert one((200, 2000, 1), 0, free) == ((1, 0, 0, 1, 0), [-1] * 4)
    assert one((100, 1000, 1), 0, free) == ((0, 0, 0, 2, 0), [-1] * 4)  # equality fits
    assert one((400, 0, 0), 0, free) == ((-1, 0, 0, 0, 0), [-1] * 4)
    assert one((0, 0, 0), 0, [(0, 0, 0)]) == ((0, 0, 0, 1, 0), [-1] * 4)


def test_reference_victims_and_priorities():
    free = [(0, 0, 0)]
    bound = ([0, 0], [4, 5], [(100, 0, 0), (100, 0, 0)])
    # priority 5: only the pod of priority 4 is lower
    assert one((100, 0, 0), 5, free, bound) == ((0, 1, 4, 1, 4 + BIAS), [0, -1, -1, -1])
    assert one((200, 0, 0), 5, free, bound) == ((-1, 0, 0, 0, 0), [-1] * 4)
    # priority 6: both are lower; the walk starts at priority 5 (bound pod 1)
    assert one((200, 0, 0), 6, free, bound) == ((0, 2, 5, 1, 9 + 2 * BIAS), [1, 0, -1, -1])
    # one of the two can stay: the first walked (priority 5) is reprieved
    assert one((100, 0, 0), 6, free, bound) == ((0, 1, 4, 1, 4 + BIAS), [0, -1, -1, -1])
    # an equal priority is no victim
    assert one((100, 0, 0), 4, free, bound) == ((-1, 0, 0, 0, 0), [-1] * 4)
    # max_victims cuts the list, not the count
    assert one((200, 0, 0), 6, free, bound, mv=1) == ((0, 2, 5, 1, 9 + 2 * BIAS), [1])
    assert one((200, 0, 0), 6, free, bound, mv=0) == ((0, 2, 5, 1, 9 + 2 * BIAS), [])


def test_reference_reprieve_order():
    # three lower pods, walked by priority: the first would leave too little,
    # the middle one can stay, the last cannot any more
    bound = ([0, 0, 0], [3, 2, 1], [(300, 0, 0), (100, 0, 0), (100, 0, 0)])
    assert one((400, 0, 0), 9, [(0, 0, 0)], bound) == ((0, 2, 3, 1, 4 + 2 * BIAS), [0, 2, -1, -1])
    # equal priorities walk by bound index: swapping the two swaps the victim
    a = ([0, 0], [2, 2], [(100, 0, 0), (200, 0, 0)])
    b = ([0, 0], [2, 2], [(200, 0, 0), (100, 0, 0)])
    assert one((200, 0, 0), 9, [(0, 0, 0)], a) == ((0, 1, 2, 1, 2 + BIAS), [1, -1, -1, -1])
    assert one((200, 0, 0), 9, [(0, 0, 0)], b) == ((0, 1, 2, 1, 2 + BIAS), [0, -1, -1, -1])


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("level", ["top", "sum", "count", "index"])
def test_reference_ladder(level, swap):
    A, B, (nv, top, psum) = pref.ladder_cases()[level]
    need = sum(r[0] for r in A[1])
    got, _ = one((need, 0, 0), 9, [(0, 0, 0)] * 2, pref.ladder_bound(A, B, swap))
    win = 0 if level == "index" else int(swap)
    assert got == (win, nv, top, 2, psum)


def test_reference_victimless_beats_any_victims_and_ineligible_never_wins():
    bound = ([0], [I32_MIN], [(100, 0, 0)])
    free = [(0, 0, 0), (100, 0, 0)]
    assert one((100, 0, 0), 0, free, bound)[0] == (1, 0, 0, 2, 0)
    elig = np.array([[True, False]])
    assert one((100, 0, 0), 0, free, bound, elig) == ((0, 1, I32_MIN, 1, 0), [0, -1, -1, -1])
    assert one((100, 0, 0), 0, free, None, np.array([[False, False]]))[0] == (-1, 0, 0, 0, 0)


def test_reference_sums_in_64_bits():
    big = 2**31 - 1
    bound = ([0], [0], [(big, big, big)])
    assert one((big, 0, 0), 1, [(big, big, big)], bound)[0] == (0, 0, 0, 1, 0)
    assert one((2 * big, 0, 0), 1, [(big, big, big)], bound)[0][:2] == (0, 1)


# ---------------------------------------------------------- generator coverage
@functools.lru_cache(maxsize=None)
def solved(P, N, profile):
    c = pref.case(P, N, profile)
    return c, pref.preempt(c["req"], c["prio"], c["free"], c["bound"], None, 80, detail=True)


def first_difference(a, b):
    """The level at which two sorted candidates (key, node, victims) differ."""
    for lvl, name in enumerate(("top", "sum", "count")):
        if a[0][lvl] != b[0][lvl]:
            return name
    return "index"


TIGHT = [(63, 65), (64, 64), (65, 130), (129, 257), (70, 1100), (33, 2100)]


@pytest.mark.parametrize("P,N", TIGHT)
def test_tight_profile_reaches_every_feature(P, N):
    c, (rec, vict, det) = solved(P, N, "tight")
    node, prio, _ = c["bound"]
    assert np.bincount(node, minlength=N).max() == pref.LONG_ROW
    assert (np.diff(node) < 0).any()  # shuffled
    # winners with victims, decided against the runner-up at each of these
    # levels (the count level needs INT32_MIN victims: a hand case)
    levels = {first_difference(d[0], d[1]) for d in det if len(d) > 1 and d[0][0][2] > 0}
    assert levels >= {"top", "sum", "index"}, levels
    assert (rec["node"] == pref.EMPTY).any() and (rec["candidates"][rec["node"] < 0] == 0).all()
    assert rec["n_victims"].max() >= 3
    assert (vict[rec["n_victims"] > 0, 0] >= 0).all()
    # a reprieved pod on the winner: more lower-priority pods there than victims
    lower = np.array([((node == r["node"]) & (prio < p)).sum() if r["node"] >= 0 else 0
                      for r, p in zip(rec, c["prio"])])
    assert ((lower > rec["n_victims"]) & (rec["n_victims"] > 0)).any()
    if N > 2 * SLAB:  # winners in three or more node slabs
        assert len(set((rec["node"][rec["node"] >= 0] // SLAB).tolist())) >= 3


@pytest.mark.parametrize("P,N", [(5, 3)] + TIGHT)
def test_roomy_profile_reaches_victimless_winners(P, N):
    _, (rec, _, _) = solved(P, N, "roomy")
    fit = (rec["node"] >= 0) & (rec["n_victims"] == 0)
    assert fit.any()
    assert (rec["priority_sum"][fit] == 0).all() and (rec["top_priority"][fit] == 0).all()
    if N >= 64:
        assert (rec["n_victims"] > 0).any()


def test_generator_with_words_keeps_every_outcome():
    c = pref.case(65, 130, "tight", "mix")
    rec, _ = pref.preempt(c["req"], c["prio"], c["free"], c["bound"], pref.elig_of(c["words"]))
    plain = solved(65, 130, "tight")[1][0]
    assert (rec["candidates"] <= plain["candidates"]).all()
    assert (rec["candidates"] < plain["candidates"]).any()
    assert (rec["node"] >= 0).any() and (rec["n_victims"] > 0).any()


# ------------------------------------------------------------------ the binding
def _declared():
    with open(os.path.join(ROOT, "include", "nas.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(nas_[a-z0-9_]+)\s*\(", src)), src


def test_header_and_bindings_agree_on_the_new_names():
    names, hdr = _declared()
    L = _lib.lib()
    for n in ("nas_upload_bound", "nas_preempt"):
        assert n in names and n in _lib.SIGNATURES and hasattr(L, n), n
    with open(os.path.join(ROOT, "scheduler", "nas.go")) as f:
        go = f.read()
    assert {"nas_upload_bound", "nas_preempt"} <= set(re.findall(r"\bC\.(nas_[a-z0-9_]+)\(", go))
    assert re.search(r"func \(e \*nasEngine\) UploadBound\(", go)
    assert re.search(r"func \(e \*nasEngine\) Preempt\(", go)
    # the record: header, ctypes, numpy and the reference agree on the fields
    body = re.search(r"typedef struct nas_preemption \{(.*?)\} nas_preemption;", hdr, re.S).group(1)
    fields = re.findall(r"(int32_t|int64_t)\s+([a-z_]+)\s*;", body)
    assert [f for _, f in fields] == [f for f, _ in _lib.NasPreemption._fields_]
    assert [f for _, f in fields] == list(pref.DTYPE.names) == list(_lib.PREEMPTION_DTYPE.names)
    for (t, f) in fields:
        assert _lib.PREEMPTION_DTYPE[f].itemsize == pref.DTYPE[f].itemsize == int(t[3:5]) // 8
    assert L.nas_version() == 2  # additive: no layout change


def test_record_is_24_bytes():
    assert ctypes.sizeof(_lib.NasPreemption) == 24
    assert _lib.PREEMPTION_DTYPE.itemsize == 24 == pref.DTYPE.itemsize
    assert _lib.PREEMPTION_DTYPE.fields["priority_sum"][1] == 16


def test_null_context_is_rejected():
    L = _lib.lib()
    assert L.nas_upload_bound(None, None, None, None, None, None, 0) == _lib.NAS_ERR_ARG
    assert L.nas_preempt(None, None, None, 0, None, None, 0) == _lib.NAS_ERR_ARG
