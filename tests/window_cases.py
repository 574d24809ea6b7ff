"""Cases and the list-by-list reference for host-driven scoring windows
(nas_score_range), shared by test_window_cases_cpu.py and test_gpu_windows.py.
No GPU is used here.

`ref_lists` is the reference: a plain numpy restatement of what a window must
produce for a pod range -- per pod the full ascending list of packed keys over
the fitting nodes of the context's node columns, against a given capacity.
`check_window` holds the rules of csrc/klist.h and include/nas.h that every
window's lists are judged by (the GPU test calls it on the lists it read back,
the CPU test on emulated lists with a fault injected).  The contexts (A: fused
256 x 256 tile, B: wide tile past WIDE_MIN_PODS, C: node shards, D:
constraints, E: an exchanging in-process group) and their windows are the
smallest shapes that reach each launch form of score_range / launch_cost."""
import zlib

import numpy as np

import constraint_ref as cref
import float_cases as fc
import oracle
from util import KEY_INVALID, bf16_bits_to_f64, cluster

KC = 8
U64 = np.uint64
# restated from the sources; test_window_cases_cpu.py pins them
TILE = 256             # COST_BN: a window's cost launch is rounded to it
WIDE_TILE = 384        # WIDE_PODS of k_cost.hip
WIDE_MIN_PODS = 32768  # csrc/pass_plan.h: padded pods from which world 1 runs the wide tile
WA_PAD_ROWS = 256      # rows allocated behind the traffic
OVF_STAGE_ENTRIES = 308

A_WINDOWS = [(0, 1), (64, 65), (1299, 1300), (0, 256), (1, 256), (255, 257), (256, 512),
             (511, 1025), (300, 1299), (0, 1300)]
B_WINDOWS = [(32513, 32600), (32300, 32600), (32200, 32600), (257, 511), (0, 1), (16000, 17025)]
C_WINDOWS = [(0, 700), (1, 2), (255, 513), (640, 700)]
C_ODD_WINDOW = (255, 513)  # the constrained shard run: an odd p_lo (k_fit_c)
D_WINDOWS = [(2, 700), (3, 700), (255, 257), (1299, 1300)]
E_WINDOWS = [(255, 513), (300, 513)]  # launch starts 0 and 256: the send buffer's offset
D_SHARD_WORLD = 2  # the constrained shard run
D_SHARD_WINDOWS = [C_ODD_WINDOW, (2, 700)]
B_PREFIX = 1024  # pods of B that the initial pass places


def round_down(x, m):
    return x // m * m


def round_up(x, m):
    return -(-x // m) * m


def launch_form(P, lo, hi, shard=False, constrained=False):
    """What score_range launches for window [lo, hi) of P pods (its conditions,
    restated): (wide, launch start, tiles, rows read past the rounded end).
    Only the constants are pinned to the sources (test_window_cases_cpu.py);
    the conditions themselves -- wide_ok and score_range of nas_api.hip: the
    wide tile on shards and from WIDE_MIN_PODS padded pods, the mask-reading
    256 x 256 tile under constraints -- are restated by hand, so when those
    change this function and the shapes chosen with it must be revisited: the
    GPU tests cannot tell which tile ran."""
    wide = not constrained and (shard or round_up(P, TILE) >= WIDE_MIN_PODS)
    pr0, pr1 = round_down(lo, TILE), round_up(hi, TILE)
    t = WIDE_TILE if wide else TILE
    tiles = -(-(pr1 - pr0) // t)
    return wide, pr0, tiles, pr0 + tiles * t - pr1


# ------------------------------------------------------------- the reference
def cost_words(WA_rows, L_cols, dtype):
    """The 32-bit orderable cost word of every (pod, node):
    int8 scoring: the int64 cost ^ 2^31; float: the sign-flip word of the fp32
    cost, -0 as +0.  The fp64 cost must be an fp32 value (exact operands)."""
    if dtype == "i8":
        c = WA_rows.astype(np.int64) @ L_cols.astype(np.int64)
        assert np.abs(c).max(initial=0) < 2**31 - 1
        return ((c ^ np.int64(-2**31)) & 0xFFFFFFFF).astype(U64)
    if dtype == "bf16":
        c = bf16_bits_to_f64(WA_rows) @ bf16_bits_to_f64(L_cols)
    else:
        c = WA_rows.astype(np.float64) @ L_cols.astype(np.float64)
    c32 = (c + 0.0).astype(np.float32)
    assert np.array_equal(c32.astype(np.float64), c + 0.0), "costs are not exact in fp32"
    b = np.where(c32 == 0, np.float32(0), c32).view(np.uint32)
    neg = (b >> np.uint32(31)).astype(bool)
    return np.where(neg, ~b, b ^ np.uint32(0x80000000)).astype(U64)


def ref_lists(WA, L, req, cap, dtype, lo, hi, elig=None, n0=0, n1=None):
    """Pods [lo, hi) against capacity `cap` on node columns [n0, n1).
    -> dict: true (n, Nloc) the key of (pod, node) or KEY_INVALID where the pod
    does not fit the node; full (n, >= 8) each pod's ascending list of all its
    fitting keys, KEY_INVALID behind them; nfit (n,); n0."""
    n1 = L.shape[1] if n1 is None else n1
    word = cost_words(WA[lo:hi], L[:, n0:n1], dtype)
    fits = (np.asarray(req, np.int64)[lo:hi, None, :]
            <= np.asarray(cap, np.int64)[None, n0:n1, :]).all(2)
    if elig is not None:
        fits &= elig[lo:hi, n0:n1]
    true = np.where(fits, (word << U64(32)) | np.arange(n0, n1, dtype=U64)[None, :], KEY_INVALID)
    full = np.sort(true, axis=1)
    if full.shape[1] < KC:
        full = np.concatenate([full, np.full((hi - lo, KC - full.shape[1]), KEY_INVALID)], 1)
    return dict(true=true, full=full, nfit=fits.sum(1), n0=n0)


def ideal_lists(ref, keep=KC):
    """Lists a correct window may write for `ref`: the first 8 keys; the bound
    is all ones when nothing was dropped, else the `keep`-th key (4 <= keep <=
    8: a bound below the last key leaves keys past the bound)."""
    keys = ref["full"][:, :KC].copy()
    bounds = np.where(ref["nfit"] < KC, KEY_INVALID, keys[:, keep - 1])
    return keys, bounds


def sentinels(P, N):
    """A distinct valid list per pod that scoring cannot write: ascending keys
    on nodes below N whose cost words 8p + 1 .. 8p + 8 stand for no cost (an
    int cost below -2^31 + 2^20, a negative NaN as float)."""
    assert 8 * P + 8 < 2**20
    p = np.arange(P, dtype=np.int64)[:, None]
    j = np.arange(KC, dtype=np.int64)[None, :]
    keys = ((8 * p + j + 1).astype(U64) << U64(32)) | ((3 * p + 5 * j) % N).astype(U64)
    bounds = keys[np.arange(P), np.arange(P) % KC].copy()
    return np.ascontiguousarray(keys), bounds


def check_window(keys, bounds, skeys, sbounds, lo, hi, ref):
    """Lists of all P pods read back after score_range(lo, hi) over the
    sentinels; ref = ref_lists(..., lo, hi, ...) on the working capacity.
    Raises AssertionError naming the rule broken."""
    out = np.ones(len(bounds), bool)
    out[lo:hi] = False
    assert np.array_equal(keys[out], skeys[out]) and np.array_equal(bounds[out], sbounds[out]), \
        f"outside the window: lists of pods {np.flatnonzero(out & ((keys != skeys).any(1) | (bounds != sbounds)))[:8]} changed"
    k, b = keys[lo:hi], bounds[lo:hi]
    true, full, nfit, n0 = ref["true"], ref["full"], ref["nfit"], ref["n0"]
    n, nloc = true.shape
    pod = lambda m: (lo + np.flatnonzero(m)[:8]).tolist()  # noqa: E731
    asc = (k[:, 1:] >= k[:, :-1]).all(1)
    assert asc.all(), f"keys do not ascend: pods {pod(~asc)}"
    valid = k != KEY_INVALID
    col = (k & U64(0xFFFFFFFF)).astype(np.int64) - n0
    inside = valid & (col >= 0) & (col < nloc)
    at = true[np.arange(n)[:, None], np.clip(col, 0, nloc - 1)]
    real = ~valid | (inside & (at == k))
    assert real.all(), f"a key is not the key of a fitting local node: pods {pod(~real.all(1))}"
    use = valid & (k <= b[:, None])
    cnt = use.sum(1)
    same = (~use | (k == full[:, :KC])).all(1)
    assert same.all(), f"usable prefix differs from the reference ranking: pods {pod(~same)}"
    # every fitting key at or below a finite bound is in the list: the reference
    # holds as many of them as the usable prefix does
    comp = b == KEY_INVALID
    below = ((full != KEY_INVALID) & (full <= b[:, None])).sum(1)
    gen = ~comp & (below != cnt)
    assert not gen.any(), f"a fitting key at or below the bound is missing: pods {pod(gen)}"
    short = cnt < np.minimum(4, nfit)
    assert not short.any(), f"short prefix (fewer than min(4, fitting) usable keys): pods {pod(short)}"
    bad = comp & ~((cnt == nfit) & (nfit < KC))
    assert not bad.any(), f"bound of all ones on a list that dropped keys: pods {pod(bad)}"
    none = nfit == 0
    bad = none & ~(~valid.any(1) & comp)
    assert not bad.any(), f"no node fits, yet the list is not empty and complete: pods {pod(bad)}"
    return cnt


def classes(nfit):
    """How many pods fit 0, 1..3, 4..7, exactly 8 and more than 8 nodes."""
    return dict(zero=int((nfit == 0).sum()), few=int(((nfit >= 1) & (nfit <= 3)).sum()),
                some=int(((nfit >= 4) & (nfit <= 7)).sum()), eight=int((nfit == 8).sum()),
                many=int((nfit > 8).sum()))


def classes_ok(c):
    return c["zero"] >= 20 and c["few"] >= 20 and c["some"] >= 20 and c["many"] >= 20 \
        and c["eight"] >= 1


def tile_entries_max(WA):
    """nas::ovf_window_max: the most entries outside int8 in any 384 rows that
    start at a multiple of 128."""
    cnt = ((WA > 127) | (WA < -128)).sum(1)
    cs = np.concatenate([[0], np.cumsum(cnt)])
    P = len(cnt)
    return max(int(cs[min(s + WIDE_TILE, P)] - cs[s]) for s in range(0, P, 128))


# ------------------------------------------------------------------- contexts
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _excess(rng, n):
    v = rng.integers(128, 100000, n)
    return np.where(rng.random(n) < 0.5, v, -v - 1).astype(np.int32)


def _plant(rng, WA, rows, k=1):
    P, N = WA.shape
    for p in rows:
        if 0 <= p < P:
            WA[p, rng.choice(N, k, replace=False)] = _excess(rng, k)


def _edge_rows(windows, P):
    """Rows just inside and just outside each window."""
    return sorted({p for lo, hi in windows for p in (lo - 2, lo - 1, lo, hi - 1, hi, hi + 1)
                   if 0 <= p < P})


def _operands(rng, kind, P, N):
    """-> WA, L, dtype of one operand kind (capacity and requests come from
    util.cluster, overridden per context)."""
    if kind in ("i8", "i32", "i32g"):
        WA, L, _, _ = cluster(rng, P, N, lo=0, hi=40)
        return (WA if kind == "i8" else WA.astype(np.int32)), L, "i8"
    if kind == "ties":  # the node index decides most ranks
        return rng.integers(0, 2, (P, N)).astype(np.int8), rng.integers(0, 3, (N, N)).astype(np.int8), "i8"
    if kind == "bf16":
        WA, L, _ = fc.int_bf16_operands(rng, P, N, dup=4)
        return WA, L, "bf16"
    if kind == "f32":
        WA, L, _ = fc.exact_operands(rng, "M10x10", P, N, signed=True, dup=4)
        return WA, L, "f32"
    raise ValueError(kind)


MEM_LO, MEM_HI = 7_464, 303_749  # util.cluster's memory requests


def _greedy(WA, L, req, free, elig, dtype, K):
    """Capacity left by the sequential greedy over the first K pods."""
    if elig is None:
        return oracle.place(WA[:K], L, req[:K], free, dtype)[2]
    return cref.place(WA[:K], L, req[:K], free, elig[:K], dtype)[2]


def open_nodes(N):
    """The nodes that stay open through the pass: m of them, evenly spread
    over the columns (36 at N = 300: 12 in each third, 18 in each half)."""
    m = 36 if N >= 300 else 30 if N >= 200 else 12
    return np.arange(m) * N // m + N // (2 * m)


def _capacity(rng, WA, L, dtype, elig, P, N, K):
    """Capacity whose remainder after the pass over the first K pods shows
    every class of list, and the requests of util.cluster.

    Ordinary nodes close during the pass: two in three hold one pod, the third
    has cpu for one or two, so lists run dry and the commit halts on the way.
    The open nodes have cpu and slots for everybody and a memory of (what the
    pass consumes on them) + T.  The remainders T lie at quantiles of the
    memory requests: the 8 largest from 57% to 87% (a pod's request between two
    of them fits 1..7 open nodes, above them none), the others from 14% to
    55%.  They are interleaved over the columns -- each third of the columns
    holds every third rank, each half every second of the middle third's -- so
    the whole cluster and each half or third of it show every class.  The
    consumption comes from the pass itself, repeated a few times (a pod that an
    open node's memory turns away late in the pass shifts it)."""
    _, _, free, req = cluster(rng, P, N, lo=0, hi=2)
    open_ = open_nodes(N)
    m = len(open_)
    i = np.arange(m)
    t, k, n3 = i // (m // 3), i % (m // 3), m // 3
    k = np.where(t == 1, np.where(k < n3 // 2, 2 * k, 2 * (k - n3 // 2) + 1), k)
    rank = 3 * k + t
    q = np.where(rank < m - 8, 0.14 + 0.41 * rank / (m - 9), 0.57 + 0.30 * (rank - (m - 8)) / 7)
    T = (MEM_LO + q * (MEM_HI - MEM_LO)).astype(np.int64)
    n = np.arange(N)
    free[:, 0] = np.where(n % 3 == 1, rng.integers(100, 700, N), 2**30)
    free[:, 1] = 2**30
    free[:, 2] = np.where(n % 3 == 1, 2**20, 1)
    free[open_] = (2**30, 2**30, 2**20)
    for _ in range(4):
        left = _greedy(WA, L, req, free, elig, dtype, K)
        used = free[open_, 1].astype(np.int64) - left[open_, 1]
        free[open_, 1] = used + T
    return free, req


_CONTEXTS = {
    # name: (context, kind, P, N, windows)
}
for _kind in ("i8", "bf16", "f32", "i32", "ties"):
    for _N in (300, 70):
        _CONTEXTS[f"A-{_kind}-{_N}"] = ("A", _kind, 1300, _N, A_WINDOWS)
for _kind in ("i8", "i32", "i32g", "ties"):
    _CONTEXTS[f"B-{_kind}"] = ("B", _kind, 32600, 257, B_WINDOWS)
for _kind in ("i8", "ties"):
    _CONTEXTS[f"C-{_kind}"] = ("C", _kind, 700, 300, C_WINDOWS)
    _CONTEXTS[f"D-{_kind}"] = ("D", _kind, 1300, 300, D_WINDOWS)
NAMES = sorted(_CONTEXTS)
A_NAMES = [n for n in NAMES if n[0] == "A"]
B_NAMES = [n for n in NAMES if n[0] == "B"]
C_NAMES = [n for n in NAMES if n[0] == "C"]  # (E runs C's inputs as one exchanging group)
D_NAMES = [n for n in NAMES if n[0] == "D"]
SHARD_WORLDS = (2, 3)

_made = {}


def make(name):
    """The (seeded, cached, read-only) inputs of one context: dict with WA, L,
    free, req, dtype, P, N, windows, prefix (pods the initial pass places),
    words (constraint words or None) and elig."""
    if name in _made:
        return _made[name]
    ctx, kind, P, N, windows = _CONTEXTS[name]
    rng = _rng("window", name)
    WA, L, dtype = _operands(rng, kind, P, N)
    prefix = B_PREFIX if ctx == "B" else P
    if dtype == "i8":
        # positive integer costs rank the nodes alike for every pod; an open node
        # (_capacity) early in that order would take the whole pass.  Their
        # latency columns are the dearest, so pods reach them as the others close
        op = open_nodes(N)
        L[:, op] = rng.integers(3, 5, (N, len(op))) if kind == "ties" else \
            rng.integers(50, 100, (N, len(op)))
    words = elig = None
    if ctx == "D":
        words = cref.pattern("mix", rng, P, N)
        elig = cref.eligible(*words)
    if kind in ("i32", "i32g"):
        if ctx == "A":  # sparse entries, and on the rows around every window's ends
            _plant(rng, WA, np.flatnonzero(rng.random(P) < 0.1), 2)
            _plant(rng, WA, _edge_rows(windows, P), 3)
        else:  # B: 5% of the pods, and the 256 rows behind each window's rounded end, which
            # its last tile may read: all of them behind (16000, 17025), every second
            # one behind (0, 1) and (257, 511) (512 adjacent rows: a tile stays staged)
            _plant(rng, WA, np.flatnonzero(rng.random(P) < 0.05))
            _plant(rng, WA, [p for lo, hi in windows for p in (lo, hi - 1)], 2)
            for lo, hi in windows:
                end = round_up(hi, TILE)
                _plant(rng, WA, range(end, end + WA_PAD_ROWS, 1 if lo == 16000 else 2))
            if kind == "i32g":  # fuller tiles: the whole upload seeds from global memory
                _plant(rng, WA, [16100], 250)
                _plant(rng, WA, [16101, 17200], 120)
    free, req = _capacity(_rng("capacity", name), WA, L, dtype, elig, P, N, prefix)
    c = dict(name=name, ctx=ctx, kind=kind, WA=WA, L=L, free=free, req=req, dtype=dtype, P=P, N=N,
             windows=windows, prefix=prefix, words=words, elig=elig)
    _made[name] = c
    return c


def zero_rows(c):
    """Pods the engine treats as zero-traffic (k_zero_rows: every bit of the
    row clear, so a bf16 -0.0 is traffic)."""
    WA = c["WA"]
    return ~(WA.view(np.uint32 if WA.dtype == np.float32 else WA.dtype) != 0).any(1)


def remaining(c):
    """Capacity the initial pass leaves, from the oracle alone: the sequential
    greedy over the first `prefix` pods."""
    key = ("left", c["name"])
    if key not in _made:
        _made[key] = _greedy(c["WA"], c["L"], c["req"], c["free"], c["elig"], c["dtype"],
                             c["prefix"])
    return _made[key]


def shard_cols(N, r, G):
    return r * N // G, (r + 1) * N // G


def window_ref(c, lo, hi, cap=None, n0=0, n1=None):
    """ref_lists of one window of a context on the remaining capacity (cached
    when cap is None)."""
    if cap is not None:
        return ref_lists(c["WA"], c["L"], c["req"], cap, c["dtype"], lo, hi, c["elig"], n0, n1)
    key = ("ref", c["name"], lo, hi, n0, n1)
    if key not in _made:
        _made[key] = ref_lists(c["WA"], c["L"], c["req"], remaining(c), c["dtype"], lo, hi,
                               c["elig"], n0, n1)
    return _made[key]


def window_pods(windows, P):
    m = np.zeros(P, bool)
    for lo, hi in windows:
        m[lo:hi] = True
    return np.flatnonzero(m)
