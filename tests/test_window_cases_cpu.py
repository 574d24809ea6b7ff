"""CPU checks behind test_gpu_windows.py: window_cases.ref_lists agrees with
the project's oracle before any GPU list is judged against it; every context's
capacity, from reference values alone, differs after the pass and shows every
class of list inside the scored windows; the constants of the sources still
put the shapes on the boundaries they were chosen for; and
window_cases.check_window catches each fault a window could commit, injected
into correct lists on the host."""
import os
import re

import numpy as np
import pytest

import constraint_ref as cref
import oracle
import window_cases as wc
from util import KEY_INVALID, merge_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kubernetesnetawarescheduler_amd", "csrc")
U64 = np.uint64


def spans(c, windows=None):
    """The windows of a context (or `windows`) as disjoint pod spans (their union)."""
    m = np.zeros(c["P"] + 2, bool)
    for lo, hi in c["windows"] if windows is None else windows:
        m[lo + 1:hi + 1] = True
    d = np.diff(m.astype(np.int8))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def nfit_over(c, n0=0, n1=None, windows=None):
    left = wc.remaining(c)
    ws = spans(c, windows)
    return np.concatenate([wc.window_ref(c, lo, hi, left, n0, n1)["nfit"] for lo, hi in ws])


# ------------------------------------------------ the reference vs the oracle
@pytest.mark.parametrize("name", wc.NAMES)
def test_reference_agrees_with_oracle(name):
    """Cost words decode to oracle.cost, the fitting set is oracle.fit_mask
    (AND constraint_ref.eligible), and each full list starts with oracle.topk's
    ranking -- on the capacity the pass leaves, for every window pod."""
    c = wc.make(name)
    left = wc.remaining(c)
    dtype = c["dtype"]
    seen = 0
    for lo, hi in spans(c):
        ref = wc.window_ref(c, lo, hi)
        cost = oracle.cost(c["WA"][lo:hi], c["L"], dtype)
        word = (ref["true"] >> U64(32)).astype(np.uint32)
        fits = ref["true"] != KEY_INVALID
        if dtype == "i8":
            got = (word ^ np.uint32(0x80000000)).view(np.int32).astype(np.int64)
        else:
            bits = np.where(word & np.uint32(0x80000000), word ^ np.uint32(0x80000000), ~word)
            got = bits.astype(np.uint32).view(np.float32).astype(np.float64)
        assert np.array_equal(got[fits], (cost + 0)[fits])
        assert ((ref["true"][fits] & U64(0xFFFFFFFF)) == np.nonzero(fits)[1].astype(U64)).all()
        mask = oracle.fit_mask(c["req"][lo:hi], left)
        if c["elig"] is not None:
            mask = mask & cref.words32(cref.eligible(*c["words"])[lo:hi])
        assert np.array_equal(cref.words32(fits), mask)
        wn, _, wcnt = oracle.topk(cost, mask, wc.KC)
        assert np.array_equal(np.minimum(ref["nfit"], wc.KC), wcnt)
        head = ref["full"][:, :wc.KC]
        nodes = np.where(head != KEY_INVALID, (head & U64(0xFFFFFFFF)).astype(np.int64), -1)
        use = np.arange(wc.KC)[None, :] < wcnt[:, None]
        assert np.array_equal(nodes[use], wn[use]) and (nodes[~use] == -1).all()
        assert (ref["full"][:, 1:] >= ref["full"][:, :-1]).all()
        seen += hi - lo
    assert seen == len(wc.window_pods(c["windows"], c["P"]))


@pytest.mark.parametrize("name", wc.C_NAMES + wc.D_NAMES)
@pytest.mark.parametrize("G", wc.SHARD_WORLDS)
def test_shard_references_merge_to_the_whole(name, G):
    """The per-shard references (local columns only), cut to lists and merged
    with util.merge_lists, give the unsharded reference's usable prefix."""
    c = wc.make(name)
    for lo, hi in spans(c):
        whole = wc.window_ref(c, lo, hi)
        for keep in (4, 8):
            parts = []
            for r in range(G):
                ref = wc.window_ref(c, lo, hi, None, *wc.shard_cols(c["N"], r, G))
                assert (ref["nfit"] <= whole["nfit"]).all()
                parts.append(wc.ideal_lists(ref, keep))
            mk, mb = merge_lists(parts)
            sk, sb = wc.sentinels(c["P"], c["N"])
            keys, bounds = sk.copy(), sb.copy()
            keys[lo:hi], bounds[lo:hi] = mk, mb
            wc.check_window(keys, bounds, sk, sb, lo, hi, whole)
        assert sum(wc.window_ref(c, lo, hi, None, *wc.shard_cols(c["N"], r, G))["nfit"]
                   for r in range(G)).tolist() == whole["nfit"].tolist()


# ------------------------------------------------------- the capacity state
@pytest.mark.parametrize("name", wc.NAMES)
def test_every_class_of_list_and_a_changed_capacity(name):
    c = wc.make(name)
    left = wc.remaining(c)
    assert (left != c["free"]).any(1).sum() > c["N"] // 2, "the pass must change the capacity"
    assert (left >= 0).all()
    views = [(0, None, None)]
    if c["ctx"] == "C":
        views += [wc.shard_cols(c["N"], r, G) + (None,) for G in wc.SHARD_WORLDS for r in range(G)]
        views.append((0, None, wc.E_WINDOWS))  # E: 258 pods on the whole cluster
    if c["ctx"] == "D":  # the constrained shard run, over the windows it scores
        views += [wc.shard_cols(c["N"], r, wc.D_SHARD_WORLD) + (wc.D_SHARD_WINDOWS,)
                  for r in range(wc.D_SHARD_WORLD)]
    for n0, n1, windows in views:
        k = wc.classes(nfit_over(c, n0, n1, windows))
        assert wc.classes_ok(k), (name, n0, n1, windows, k)
    if c["dtype"] != "i8":
        assert wc.zero_rows(c).sum() > 0  # (zero-traffic pods: every key has the cost-0 word)
    # the working capacity is not the uploaded one for the window pods either:
    # their references differ
    lo, hi = max(c["windows"], key=lambda w: w[1] - w[0])
    a = wc.window_ref(c, lo, hi)["nfit"]
    b = wc.ref_lists(c["WA"], c["L"], c["req"], c["free"], c["dtype"], lo, hi, c["elig"])["nfit"]
    assert (a <= b).all() and (a < b).sum() > (hi - lo) // 2


def test_exact_traffic_cases_hold_their_entries():
    """int32 traffic: entries outside int8 on window pods and on the rows just
    outside each window (A), on the rows a wide window's last tile reads past
    its rounded end (B), and the two B variants on either side of the LDS
    stage's size."""
    for name in wc.NAMES:
        c = wc.make(name)
        if c["kind"] not in ("i32", "i32g"):
            assert c["WA"].dtype != np.int32
            continue
        has = ((c["WA"] > 127) | (c["WA"] < -128)).any(1)
        if c["ctx"] == "A":
            for lo, hi in c["windows"]:
                assert has[lo] and has[hi - 1]
                assert lo == 0 or has[lo - 1]
                assert hi == c["P"] or has[hi]
        else:
            planted = 0
            for lo, hi in c["windows"]:
                wide, pr0, tiles, over = wc.launch_form(c["P"], lo, hi)
                end = wc.round_up(hi, wc.TILE)
                rows = np.arange(end, min(end + over, c["P"]))
                planted += int(has[rows].sum())
                assert len(rows) == 0 or has[rows].sum() >= len(rows) // 2
                assert has[lo:hi].any()
            assert planted >= 256
    staged = wc.tile_entries_max(wc.make("B-i32")["WA"])
    walked = wc.tile_entries_max(wc.make("B-i32g")["WA"])
    assert 0 < staged <= wc.OVF_STAGE_ENTRIES < walked, \
        (f"B-i32 must stay at or below OVF_STAGE_ENTRIES = {wc.OVF_STAGE_ENTRIES} entries per "
         f"384-row tile (has {staged}) and B-i32g above it (has {walked}): move the planted rows "
         "of window_cases.make")


# ----------------------------------------------------------------- constants
def _const(path, name):
    with open(os.path.join(CSRC, path)) as f:
        text = re.sub(r"//[^\n]*", "", f.read())
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert m, f"{name} not found in {path}"
    return int(m.group(1))


def test_source_constants_give_the_tested_boundaries():
    """A retuned constant moves a boundary: then the shapes of window_cases.py
    must move with it, or the GPU test stops reaching the launch form it names."""
    wide_min = _const("pass_plan.h", "WIDE_MIN_PODS")
    pad = _const("nas_internal.h", "WA_PAD_ROWS")
    stage = _const("nas_internal.h", "OVF_STAGE_ENTRIES")
    tile = _const("nas_internal.h", "COST_BN")
    wide_tile = _const("k_cost.hip", "WIDE_PODS")
    assert (tile, wide_tile) == (wc.TILE, wc.WIDE_TILE) == (256, 384), \
        "tile pod counts changed: every window of window_cases.py was chosen for 256 / 384"
    assert wide_min == wc.WIDE_MIN_PODS and pad == wc.WA_PAD_ROWS and stage == wc.OVF_STAGE_ENTRIES
    # B's padded pods sit exactly on the threshold; A's and D's stay below it
    PB = wc.make("B-i8")["P"]
    assert wc.round_up(PB, tile) == wide_min and wc.round_up(PB - tile, tile) < wide_min, \
        f"move B's P = {PB} so that its padded pod count is WIDE_MIN_PODS = {wide_min}"
    for name in wc.A_NAMES + wc.D_NAMES:
        assert wc.round_up(wc.make(name)["P"], tile) < wide_min, f"move {name}'s P below {wide_min}"
    # B's windows: every start class modulo the wide tile, every overshoot, and
    # the two that read the padding behind the traffic, up to its last row
    forms = {w: wc.launch_form(PB, *w) for w in wc.B_WINDOWS}
    assert forms == {(32513, 32600): (True, 32512, 1, 128), (32300, 32600): (True, 32256, 2, 256),
                     (32200, 32600): (True, 32000, 2, 0), (257, 511): (True, 256, 1, 128),
                     (0, 1): (True, 0, 1, 128), (16000, 17025): (True, 15872, 4, 256)}, forms
    assert {f[1] % wide_tile for f in forms.values()} == {0, 128, 256}
    Pp = wc.round_up(PB, tile)
    past = sorted(pr0 + t * wide_tile - Pp for _, pr0, t, _ in forms.values()
                  if pr0 + t * wide_tile > Pp)
    assert past == [128, 256] and past[-1] == pad, \
        (f"B's windows (32513, 32600) and (32300, 32600) must read 128 and WA_PAD_ROWS = {pad} "
         f"rows of padding (read {past})")
    # A: the fused 256 x 256 tile, launches rounded to it, one to six tiles
    PA = wc.make("A-i8-300")["P"]
    fa = [wc.launch_form(PA, *w) for w in wc.A_WINDOWS]
    assert not any(f[0] for f in fa) and all(f[3] == 0 for f in fa)
    assert {f[2] for f in fa} == {1, 2, 4, 5, 6}
    # C: the wide tile at a small size, with and without overshoot; D: either parity
    PC = wc.make("C-i8")["P"]
    fcs = [wc.launch_form(PC, *w, shard=True) for w in wc.C_WINDOWS]
    assert all(f[0] for f in fcs) and {f[3] for f in fcs} >= {0, 128}
    assert not any(wc.launch_form(1300, *w, shard=True, constrained=True)[0] for w in wc.D_WINDOWS)
    assert {lo % 2 for lo, _ in wc.D_WINDOWS} == {0, 1} and wc.C_ODD_WINDOW[0] % 2 == 1


# --------------------------------------------- the checks catch their faults
def emulate(c, lo, hi, keep=4):
    """What a correct window leaves: sentinels outside, lists of the reference
    inside (bound at the keep-th key: keys past the bound stay in the list)."""
    sk, sb = wc.sentinels(c["P"], c["N"])
    keys, bounds = sk.copy(), sb.copy()
    ref = wc.window_ref(c, lo, hi)
    keys[lo:hi], bounds[lo:hi] = wc.ideal_lists(ref, keep)
    return keys, bounds, sk, sb, ref


@pytest.mark.parametrize("name", ["A-i8-300", "A-ties-70", "A-f32-300", "A-bf16-70", "D-i8", "B-i32"])
@pytest.mark.parametrize("keep", [4, 8])
def test_correct_lists_pass(name, keep):
    c = wc.make(name)
    for lo, hi in c["windows"]:
        keys, bounds, sk, sb, ref = emulate(c, lo, hi, keep)
        cnt = wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
        assert np.array_equal(cnt, np.minimum(ref["nfit"], np.where(ref["nfit"] < 8, 8, keep)))


def test_sentinels_are_valid_and_foreign():
    for name in ("A-i8-70", "B-i8"):
        c = wc.make(name)
        sk, sb = wc.sentinels(c["P"], c["N"])
        assert (sk[:, 1:] > sk[:, :-1]).all() and ((sk & U64(0xFFFFFFFF)) < c["N"]).all()
        assert len(np.unique(sk)) == sk.size and len(np.unique(sb)) == len(sb)
        assert (sb != KEY_INVALID).all() and (sb[:, None] == sk).any(1).all()
        lo, hi = c["windows"][-1]
        true = wc.window_ref(c, lo, hi)["true"]
        assert (sk >> U64(32)).max() < (true >> U64(32)).min()  # below every real cost word


FAULT_WINDOW = (255, 257)


def test_fault_neighbour_overwrite():
    c = wc.make("A-i8-300")
    lo, hi = FAULT_WINDOW
    for victim, src in ((lo - 1, lo), (hi, hi - 1)):
        keys, bounds, sk, sb, ref = emulate(c, lo, hi)
        keys[victim], bounds[victim] = keys[src], bounds[src]
        with pytest.raises(AssertionError, match="outside the window"):
            wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
    keys, bounds, sk, sb, ref = emulate(c, lo, hi)
    bounds[hi] = KEY_INVALID  # (a bound alone)
    with pytest.raises(AssertionError, match="outside the window"):
        wc.check_window(keys, bounds, sk, sb, lo, hi, ref)


def test_fault_bound_too_generous():
    c = wc.make("A-i8-300")
    lo, hi = 256, 512
    ref = wc.window_ref(c, lo, hi)
    p = int(np.flatnonzero(ref["nfit"] > 9)[0])
    keys, bounds, sk, sb, _ = emulate(c, lo, hi)
    # the list dropped the 5th key; with the bound on the 4th that is allowed
    keys[lo + p] = ref["full"][p, [0, 1, 2, 3, 5, 6, 7, 8]]
    bounds[lo + p] = ref["full"][p, 3]
    wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
    bounds[lo + p] = keys[lo + p, 7]  # raised past the dropped key
    with pytest.raises(AssertionError, match="usable prefix differs"):
        wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
    # keys dropped from the tail: all 8 kept, the bound raised past the 9th (a
    # merge that lost min(bound, kept[7])) ...
    keys, bounds, sk, sb, _ = emulate(c, lo, hi, 8)
    bounds[lo + p] = ref["full"][p, 9]
    with pytest.raises(AssertionError, match="at or below the bound is missing"):
        wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
    # ... and 4 kept, the bound left on the 7th (a tile's bound not carried
    # through the merge)
    keys, bounds, sk, sb, _ = emulate(c, lo, hi, 8)
    keys[lo + p, 4:] = KEY_INVALID
    bounds[lo + p] = ref["full"][p, 6]
    with pytest.raises(AssertionError, match="at or below the bound is missing"):
        wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
    bounds[lo + p] = ref["full"][p, 3]  # (the same list with its true bound is right,
    wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
    bounds[lo + p] = ref["full"][p, 4] - U64(1)  # and with a bound just below the 5th key)
    wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
    keys, bounds, sk, sb, _ = emulate(c, lo, hi, 8)
    bounds[lo + p] = KEY_INVALID  # "nothing was dropped" with more than 8 fitting
    with pytest.raises(AssertionError, match="bound of all ones"):
        wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
    q = int(np.flatnonzero(ref["nfit"] == 0)[0])
    keys, bounds, sk, sb, _ = emulate(c, lo, hi)
    bounds[lo + q] = U64(5)  # no node fits: the bound must still say "complete"
    with pytest.raises(AssertionError, match="no node fits"):
        wc.check_window(keys, bounds, sk, sb, lo, hi, ref)


def test_fault_short_prefix():
    c = wc.make("A-i8-300")
    lo, hi = 256, 512
    ref = wc.window_ref(c, lo, hi)
    for p in (int(np.flatnonzero(ref["nfit"] > 8)[0]), int(np.flatnonzero(ref["nfit"] == 4)[0])):
        keys, bounds, sk, sb, _ = emulate(c, lo, hi)
        bounds[lo + p] = keys[lo + p, 2]  # below the fourth key
        with pytest.raises(AssertionError, match="short prefix"):
            wc.check_window(keys, bounds, sk, sb, lo, hi, ref)


def test_fault_tie_order():
    c = wc.make("A-ties-300")
    lo, hi = 256, 512
    ref = wc.window_ref(c, lo, hi)
    head = ref["full"][:, :4]
    tie = (head[:, 1:] >> U64(32) == head[:, :-1] >> U64(32)) & (head[:, 1:] != KEY_INVALID)
    assert tie.any(1).sum() > (hi - lo) // 4, "the tie-heavy case must tie inside the first four keys"
    p = int(np.flatnonzero(tie.any(1))[0])
    j = int(np.flatnonzero(tie[p])[0])
    keys, bounds, sk, sb, _ = emulate(c, lo, hi)
    keys[lo + p, [j, j + 1]] = keys[lo + p, [j + 1, j]]  # the higher node first
    with pytest.raises(AssertionError, match="keys do not ascend"):
        wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
    # the same mistake in a list that still ascends: of two equal costs the higher
    # node kept, the lower one dropped
    keys, bounds, sk, sb, _ = emulate(c, lo, hi)
    keys[lo + p, j:-1] = keys[lo + p, j + 1:].copy()
    keys[lo + p, -1] = KEY_INVALID if ref["nfit"][p] <= 8 else ref["full"][p, 8]
    bounds[lo + p] = keys[lo + p, max(3, j)]
    with pytest.raises(AssertionError, match="usable prefix differs"):
        wc.check_window(keys, bounds, sk, sb, lo, hi, ref)


@pytest.mark.parametrize("name", ["A-i8-300", "C-i8", "D-i8", "B-i8"])
def test_fault_wrong_capacity(name):
    """Lists scored against the uploaded capacity instead of the working one
    (the same as a reference built from the wrong capacity): caught in every
    window of the context."""
    c = wc.make(name)
    sk, sb = wc.sentinels(c["P"], c["N"])
    for lo, hi in c["windows"]:
        stale = wc.ref_lists(c["WA"], c["L"], c["req"], c["free"], c["dtype"], lo, hi, c["elig"])
        keys, bounds = sk.copy(), sb.copy()
        keys[lo:hi], bounds[lo:hi] = wc.ideal_lists(stale)
        if hi - lo < 50:  # (a few pods may rank the same nodes first before and after)
            continue
        with pytest.raises(AssertionError):
            wc.check_window(keys, bounds, sk, sb, lo, hi, wc.window_ref(c, lo, hi))
        keys, bounds, _, _, ref = emulate(c, lo, hi)
        with pytest.raises(AssertionError):
            wc.check_window(keys, bounds, sk, sb, lo, hi, stale)
