"""Operands for the int8 path at the int32 limits and at the seams of the
cost epilogue's key packing, with a CPU model of the path the epilogue takes.
No GPU is used here.

The int8 path returns exact integer costs while the guard holds: for every
pod sum_m |WA[p, m]| * max|L| <= LIMIT (include/nas.h).  Every case below
keeps max|L| = 1 (`lmax128`: 128), so that costs can be planted exactly under
the guard:

  * L = identity (with a few copied columns): cost[p, n] = WA[p, n];
  * L = ones - Z, Z sparse 0/1: cost[p, n] = S_p - (WA Z)[p, n], S_p the row
    sum -- every node within a small distance of S_p.

The cost epilogue (k_cost.hip) ranks a cost as its 32-bit key cost ^ 2^31 and
chooses per wave between three codings, which `tile_classes` models per
(pod, 256-node tile) from the tile's smallest and largest cost (padding nodes
past N count as cost 0: Lt is zero-padded):

  direct    min >= 0 and max < 2^26 - 1:   x = cost << 6 | slot
  relative  max - min < 2^26 - 1:          x = (cost - min) << 6 | slot
  select    otherwise:                     full keys through the Top4 network

A lane holds 64 (or 32) of a tile's nodes, among them whole aligned groups of
four, and the wave votes: a class of the whole tile that is `direct` or
`relative` holds for every lane, and the cases plant the two extremes of a
`select` row within one aligned group of four nodes, so that one lane sees
the whole span.  Every case is homogeneous: all its pods are of one class on
every full tile (the last tile of N = 257 holds node 256 alone and is not
constrained).

Classes (`CASES` lists the seeded cases the GPU tests use):

  ceiling_select  identity L, a few int32 entries of both signs per row, every
                  row's |sum| exactly LIMIT; planted costs +LIMIT, LIMIT - 1,
                  -LIMIT, -(LIMIT - 1); two copied latency columns, so that
                  the extreme is tied between two nodes
  ceiling_packed  L = ones - Z, traffic >= 0, row sum LIMIT, costs within
                  [LIMIT - (2^26 - 2), LIMIT]: relative keys, base near the top
  floor_packed    the same negated: costs within [-LIMIT, -LIMIT + 2^26 - 2]
  direct_edge     identity L, costs >= 0 with row minimum 0 and row maximum
                  2^26 - 3, 2^26 - 2 (direct), 2^26 - 1, 2^26 (select)
  offset_edge     L = ones - Z with a node every pod talks to: all costs > 0,
                  span < 2^17, row maximum 2^26 - 2 (direct with a non-zero
                  minimum), 2^26 - 1, 2^26 (relative with a positive base)
  span_edge       identity L, row minimum -2^25, span 2^26 - 2 (relative) and
                  2^26 - 1 (select)
  lmax128         L over the whole int8 range with -128, int32 traffic, the
                  largest row sum LIMIT // 128, costs of both signs

Capacity: every node takes most pods; two groups of four nodes (`excl`) are
the only ones that `exclusive` pods fit (by cpu, by memory), and those pods'
planted costs sit on them -- for them only the extreme-cost nodes fit, they
move up the group as it fills, and the last of them stay unschedulable.
"""
import zlib

import numpy as np

# the largest accepted sum_m |WA[p, m]| * max|L| (include/nas.h: the key word
# of cost INT32_MAX, all-ones, is reserved for "does not fit")
LIMIT = 2 ** 31 - 2
E26 = 2 ** 26
TILE = 256
BIG_CPU, BIG_MEM = 100_000, 100_000_000


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def tile_classes(cost, N):
    """-> (P, ceil(N / 256)) array of 'direct' / 'relative' / 'select'."""
    cost = np.asarray(cost, np.int64)
    P = cost.shape[0]
    T = -(-N // TILE)
    pad = np.zeros((P, T * TILE), np.int64)
    pad[:, :N] = cost
    t = pad.reshape(P, T, TILE)
    lo, hi = t.min(2), t.max(2)
    out = np.full((P, T), "select", dtype=object)
    packed = hi - lo < E26 - 1
    out[packed] = "relative"
    out[packed & (lo >= 0) & (hi < E26 - 1)] = "direct"
    return out


def guard_product(WA, L):
    """max_p sum_m |WA[p, m]| * max|L|, in Python integers."""
    rows = np.abs(np.asarray(WA, np.int64)).sum(1)
    return int(rows.max()) * int(np.abs(np.asarray(L, np.int64)).max())


def _capacity(rng, P, N, excl, n_excl):
    """free (N, 3), req (P, 3): roomy ordinary nodes (a pod fits about 3 of 4)
    and the two exclusive groups: excl[0]'s nodes alone fit the cpu of pods
    [0, n_excl) with even index, excl[1]'s alone the memory of the odd ones;
    each group has room for about two thirds of its pods."""
    free = np.stack([rng.integers(400, 2400, N), rng.integers(2_000_000, 8_000_000, N),
                     np.full(N, max(4, 2 * P // N))], 1).astype(np.int64)
    req = np.stack([rng.integers(1, 540, P), rng.integers(7_464, 303_749, P),
                    np.ones(P, np.int64)], 1)
    ex = np.arange(n_excl)
    req[ex[ex % 2 == 0], 0] = BIG_CPU
    req[ex[ex % 2 == 1], 1] = BIG_MEM
    room = max(1, n_excl // 3)  # pods of a group: n_excl / 2; room for 2/3 of them
    for g, (res, big) in enumerate(((0, BIG_CPU), (1, BIG_MEM))):
        nodes = excl[g]
        share = [room - room // 2, room // 2] + [0] * (len(nodes) - 2)
        for n, k in zip(nodes, share):
            free[n, res] = big * k + free[n, res]
        for n in nodes[2:]:
            free[n, res] = big + free[n, res]  # (one pod each further up the group)
        free[nodes, 2] = P
    return free.astype(np.int32), req.astype(np.int32)


def _finish(name, WA, L, free, req, planted, intended, excl, limit):
    WA = np.asarray(WA, np.int64)
    assert np.abs(WA).max() < 2 ** 31
    return dict(name=name, WA=WA.astype(np.int32), L=np.asarray(L, np.int8), free=free, req=req,
                planted=planted, intended=intended, excl=excl, limit=limit)


def _n_excl(P):
    return min(P // 8, 24) // 2 * 2


def _neighbour(x, plain):
    """A second node for a row's +-1 entry: in x's aligned group of four when
    the group has another plain node."""
    return next((y for y in (x ^ 1, x ^ 2, x ^ 3) if y in plain), x - 4)


def _split(rng, total, k):
    """k non-negative integers that sum to total."""
    cuts = np.sort(rng.integers(1, total, k - 1))
    return np.diff(np.concatenate([[0], cuts, [total]]))


def ceiling_select(P, N, limit=LIMIT, seed=0):
    rng = _rng("ceiling_select", P, N, seed)
    L = np.eye(N, dtype=np.int64)
    # two copied columns: node b costs every pod what node a costs it
    pairs = [(5, N // 2 + 12), (N // 4 + 9, N - 1)]
    for a, b in pairs:
        L[:, b] = L[:, a]
    excl = [[a, b] for a, b in pairs]
    copies = [b for _, b in pairs]
    plain = np.setdiff1d(np.arange(N), copies)
    n_excl = _n_excl(P)
    WA = np.zeros((P, N), np.int64)
    planted = []
    for p in range(P):
        kind = p % 6
        if p < n_excl:
            x, kind = pairs[p % 2][0], (p // 2) % 4
        else:
            x = int(rng.choice(plain))
        y = _neighbour(x, plain)
        if kind == 0:
            WA[p, x] = limit
            planted.append((p, x, limit))
        elif kind == 1:
            WA[p, x], WA[p, y] = limit - 1, rng.choice([-1, 1])
            planted.append((p, x, limit - 1))
        elif kind == 2:
            WA[p, x] = -limit
            planted.append((p, x, -limit))
        elif kind == 3:
            WA[p, x], WA[p, y] = -(limit - 1), rng.choice([-1, 1])
            planted.append((p, x, -(limit - 1)))
        else:  # 2 .. 5 entries of both signs, the magnitudes a random split of limit
            k = int(rng.integers(2, 6))
            cols = rng.choice(plain, k, replace=False)
            sg = rng.choice([-1, 1], k)
            sg[0], sg[1] = 1, -1
            WA[p, cols] = sg * _split(rng, limit, k)
    for a, b in pairs:  # the tie: the copy carries the planted value too
        planted += [(p, b, v) for p, n, v in planted if n == a]
    free, req = _capacity(rng, P, N, excl, n_excl)
    assert (np.abs(WA).sum(1) == limit).all()
    return _finish(f"ceiling_select-{N}", WA, L, free, req, planted, "select", excl, limit)


def _ones_minus_z(rng, N, clean, pairs):
    """Z = identity plus, for about a third of the other columns, one more 1
    from another ordinary node; the `clean` nodes keep a diagonal-only row and
    column; pairs (a, b): column b becomes a copy of column a."""
    Z = np.eye(N, dtype=np.int64)
    other = np.setdiff1d(np.arange(N), clean)
    for n in other:
        if rng.random() < 0.3:
            Z[rng.choice(other[other != n]), n] = 1
    for a, b in pairs:
        Z[:, b] = Z[:, a]
    return Z


def packed(P, N, sign, limit=LIMIT, seed=0):
    """ceiling_packed (sign = +1) / floor_packed (sign = -1)."""
    assert N % TILE == 0
    name = "ceiling_packed" if sign > 0 else "floor_packed"
    rng = _rng(name, P, N, seed)
    # per tile one aligned group of four clean nodes; the first two groups are
    # the exclusive ones, and their last node is a copy of their first
    groups = [[t * TILE + 124 + i for i in range(4)] for t in range(N // TILE)]
    groups.append([128 + 56 + i for i in range(4)])
    excl = groups[:2] if N > TILE else [groups[0], groups[-1]]
    pairs = [(g[0], g[3]) for g in excl]
    clean = np.array(sorted(n for g in groups for n in g))
    Z = _ones_minus_z(rng, N, clean, pairs)
    L = 1 - Z
    unit = limit // N
    span = E26 - 2
    assert 2 * 2 * unit < span
    n_excl = _n_excl(P)
    copies = [b for _, b in pairs]
    WA = rng.integers(unit // 4, 2 * unit - unit // 4, (P, N))
    # per pod a group: the row's largest cost (no traffic to the node) and,
    # `span` below it, its smallest lie within that aligned group of four; an
    # exclusive group's copy shares its first node's cost, and an exclusive
    # pod's third node is at the ceiling too
    rows = np.arange(P)
    gi = rng.integers(len(groups), size=P)
    gi[:n_excl] = [groups.index(excl[p % 2]) for p in range(n_excl)]
    G = np.array(groups)[gi]
    swap = ((rows // 2) % 2 == 1) & np.isin(gi, [groups.index(g) for g in excl])
    top, low = np.where(swap, G[:, 1], G[:, 0]), np.where(swap, G[:, 0], G[:, 1])
    WA[rows, top], WA[rows, low] = 0, span
    WA[rows[:n_excl], G[:n_excl, 2]] = 0
    fixed = np.zeros((P, N), bool)
    fixed[rows, top] = fixed[rows, low] = fixed[rows, G[:, 2]] = True
    fixed[:, copies] = True
    # the other entries share what the row still lacks to sum to the limit
    q, r = np.divmod(limit - WA.sum(1), (~fixed).sum(1))
    WA += ~fixed * (q[:, None] + (np.cumsum(~fixed, 1) <= r[:, None]))
    assert (WA.sum(1) == limit).all() and WA.min() >= 0 and WA[~fixed].max() < 2 * unit
    planted = [(p, int(top[p]), sign * limit) for p in range(P)]
    planted += [(p, int(low[p]), sign * (limit - span)) for p in range(P)]
    planted += [(p, int(G[p, 2]), sign * limit) for p in range(n_excl)]
    for a, b in pairs:
        planted += [(p, b, v) for p, n, v in planted if n == a]
    free, req = _capacity(rng, P, N, excl, n_excl)
    return _finish(f"{name}-{N}", sign * WA, L, free, req, planted, "relative", excl, limit)


def _edge_groups():
    """N = 256: the exclusive groups end on the last slot of a lane (nodes 127
    and 255 of the 256-node tile)."""
    return [[124, 125, 126, 127], [252, 253, 254, 255]]


def direct_edge(P, top, seed=0):
    """Identity L: costs = traffic in [0, top]; every row holds 0 and top
    within one aligned group of four."""
    N = TILE
    rng = _rng("direct_edge", P, top, seed)
    excl = _edge_groups()
    n_excl = _n_excl(P)
    WA = rng.integers(1, 2 ** 22, (P, N))
    planted = []
    for p in range(P):
        g = excl[p % 2] if p < n_excl else excl[int(rng.integers(2))]
        WA[p, g] = [0, top - 2, top - 1, top] if p % 3 else [top - 1, 0, top, top]
        planted += [(p, n, int(WA[p, n])) for n in g]
    free, req = _capacity(rng, P, N, excl, n_excl)
    want = "direct" if top < E26 - 1 else "select"
    return _finish(f"direct_edge-{top - E26:+d}", WA, np.eye(N, dtype=np.int64), free, req,
                   planted, want, excl, LIMIT)


def offset_edge(P, top, seed=0):
    """L = ones - Z, Z the identity without node 60's row: cost[p, n] = top -
    WA[p, n] (n != 60), cost[p, 60] = top.  Every cost is positive and the
    span below 2^17."""
    N = TILE
    rng = _rng("offset_edge", P, top, seed)
    excl = _edge_groups()
    n_excl = _n_excl(P)
    heavy = 60
    Z = np.eye(N, dtype=np.int64)
    Z[heavy, heavy] = 0
    WA = rng.integers(1, 2 ** 16, (P, N))
    planted = []
    for p in range(P):
        g = excl[p % 2] if p < n_excl else excl[int(rng.integers(2))]
        WA[p, g] = [2 ** 17 - 1, 1, 0, 0] if p % 3 else [1, 2 ** 17 - 1, 0, 0]
        planted.append((p, g[3], top))
        planted.append((p, g[2], top))
    WA[:, heavy] = 0
    WA[:, heavy] = top - WA.sum(1)
    free, req = _capacity(rng, P, N, excl, n_excl)
    want = "direct" if top < E26 - 1 else "relative"
    return _finish(f"offset_edge-{top - E26:+d}", WA, 1 - Z, free, req, planted, want, excl, LIMIT)


def span_edge(P, span, seed=0):
    """Identity L, dense small traffic of both signs; every row holds its
    minimum -2^25 and its maximum span - 2^25 within one aligned group."""
    N = TILE
    rng = _rng("span_edge", P, span, seed)
    excl = _edge_groups()
    n_excl = _n_excl(P)
    lo = -(2 ** 25)
    WA = rng.integers(-(2 ** 21), 2 ** 21, (P, N))
    planted = []
    for p in range(P):
        g = excl[p % 2] if p < n_excl else excl[int(rng.integers(2))]
        WA[p, g] = [lo, lo + span - 1, lo + 1, lo + span] if p % 3 else [lo + span, lo, lo, lo + span]
        planted += [(p, n, int(WA[p, n])) for n in g]
    free, req = _capacity(rng, P, N, excl, n_excl)
    want = "relative" if span < E26 - 1 else "select"
    return _finish(f"span_edge-{span - E26:+d}", WA, np.eye(N, dtype=np.int64), free, req,
                   planted, want, excl, LIMIT)


def lmax128(P, N=257, limit=LIMIT, seed=0):
    """Latency over the whole int8 range; rows of 1 .. 5 int32 entries of both
    signs with |sum| <= limit // 128.  The exclusive groups' latency from node
    3 is -128, -128, 127, 126: a pod whose only traffic is -+(limit // 128) to
    node 3 costs +-128 * (limit // 128) on a group's first two nodes."""
    rng = _rng("lmax128", P, N, seed)
    R = limit // 128
    L = rng.integers(-128, 128, (N, N))
    excl = [[124, 125, 126, 127], [N - 5, N - 4, N - 3, N - 2]]
    src = 3
    for g in excl:
        L[src, g] = [-128, -128, 127, 126]
    n_excl = _n_excl(P)
    WA = np.zeros((P, N), np.int64)
    planted = []
    for p in range(P):
        if p < n_excl or p % 5 == 0:
            s = -1 if (p // 2) % 2 == 0 else 1
            WA[p, src] = s * R
            for g in excl:
                planted += [(p, g[0], -s * 128 * R), (p, g[1], -s * 128 * R)]
            continue
        k = int(rng.integers(2, 6))
        cols = rng.choice(N, k, replace=False)
        sg = rng.choice([-1, 1], k)
        sg[0], sg[1] = 1, -1
        WA[p, cols] = sg * _split(rng, R, k)
    free, req = _capacity(rng, P, N, excl, n_excl)
    return _finish(f"lmax128-{N}", WA, L, free, req, planted, "select", excl, limit)


def crowded(case, hot=6, slots=1):
    """A crowded variant: the case's rows with capacity so tight that lists
    run dry -- few pod slots on every node, so that the pods' common
    preferences (ties broken towards node 0; the planted floors) fill up and
    commits stop for a rescore."""
    c = dict(case)
    free = case["free"].copy()
    free[:, 2] = slots
    free[:hot, :2] = 10 * BIG_CPU, 2_000_000_000  # every pod fits them: slots alone close them
    c["free"] = free
    c["name"] = case["name"] + "-crowded"
    return c


def csr_of(WA, rng, split=3):
    """The dense int32 traffic as CSR with colliding peers: every non-zero
    aggregate is cut into up to `split` int32 weights of both signs that sum
    to it, in shuffled order, with unbound peers (-1) between them.
    -> row_ptr, peer, weight (int32)."""
    WA = np.asarray(WA, np.int64)
    P, N = WA.shape
    rows_p, rows_w = [], []
    for p in range(P):
        cols = np.flatnonzero(WA[p])
        pe, we = [], []
        for n in cols:
            v = int(WA[p, n])
            k = int(rng.integers(1, split + 1))
            parts = []
            for _ in range(k - 1):  # each part keeps the running rest within int32
                lo, hi = max(-2 ** 31, v - (2 ** 31 - 1)), min(2 ** 31 - 1, v + 2 ** 31)
                w = int(rng.integers(max(lo, -abs(v) - 7), min(hi, abs(v) + 7) + 1))
                parts.append(w)
                v -= w
            parts.append(v)
            pe += [n] * k
            we += parts
        if len(cols) and p % 4 == 0:
            pe.append(-1)
            we.append(int(rng.integers(-2 ** 31, 2 ** 31)))
        order = rng.permutation(len(pe))
        rows_p.append(np.asarray(pe, np.int64)[order])
        rows_w.append(np.asarray(we, np.int64)[order])
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows_p])]).astype(np.int32)
    peer = np.concatenate(rows_p).astype(np.int32)
    weight = np.concatenate(rows_w)
    assert np.abs(weight).max() < 2 ** 31
    return row_ptr, peer, weight.astype(np.int32)


# ------------------------------------------- the cases of the GPU tests, seeded
SMALL_P = 300
WIDE_P = 33000
CASES = {
    "ceiling_select-130": lambda P=SMALL_P: ceiling_select(P, 130),
    "ceiling_select-257": lambda P=SMALL_P: ceiling_select(P, 257),
    "ceiling_packed-256": lambda P=SMALL_P: packed(P, 256, +1),
    "ceiling_packed-512": lambda P=SMALL_P: packed(P, 512, +1),
    "floor_packed-256": lambda P=SMALL_P: packed(P, 256, -1),
    "floor_packed-512": lambda P=SMALL_P: packed(P, 512, -1),
    "direct_edge--3": lambda P=SMALL_P: direct_edge(P, E26 - 3),
    "direct_edge--2": lambda P=SMALL_P: direct_edge(P, E26 - 2),
    "direct_edge--1": lambda P=SMALL_P: direct_edge(P, E26 - 1),
    "direct_edge-+0": lambda P=SMALL_P: direct_edge(P, E26),
    "offset_edge--2": lambda P=SMALL_P: offset_edge(P, E26 - 2),
    "offset_edge--1": lambda P=SMALL_P: offset_edge(P, E26 - 1),
    "offset_edge-+0": lambda P=SMALL_P: offset_edge(P, E26),
    "span_edge--2": lambda P=SMALL_P: span_edge(P, E26 - 2),
    "span_edge--1": lambda P=SMALL_P: span_edge(P, E26 - 1),
    "lmax128-257": lambda P=SMALL_P: lmax128(P),
}
_CACHE = {}


def case(name, P=SMALL_P):
    """The seeded case (built once; treat it as read-only)."""
    if (name, P) not in _CACHE:
        _CACHE[name, P] = CASES[name](P)
        assert _CACHE[name, P]["name"] == name
    return _CACHE[name, P]
