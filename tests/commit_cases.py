"""Crafted candidate lists for the commit kernels (k_commit.hip), shared by
test_commit_ref_cpu.py and test_gpu_commit_direct.py.

A case is a dict: keys (P, 8) / bounds (P,) uint64, req (P, 3) and free (N, 3)
int32, zero (P,) bool (zero-traffic pods), and fixups {pod: (keys row, bound)}:
the fresh list a test writes for a pod the walk is meant to halt at, before it
resumes from that pod.  A halt at any other pod is a failure.  Nothing here is
scored: the lists are written as the commit's input directly."""
import numpy as np

from util import KEY_INVALID, ZERO_COST_HI, commit_ref, commit_walk, keys_from_costs

KC = 8
# boundaries of launch_commit (test_commit_ref_cpu.py pins them to k_commit.hip)
AOS_MAX_NODES = 8656
LDS_CAP_MAX_NODES = 11541
ONE_WAVE_MAX_PODS = 16384
ZSCAN_LDS = 1024
ZSCAN_L2 = 16
FETCH_SUB_MAX = 1 << 21
POD_PAD = 256  # pods are padded to the cost tile before launch_commit sees them

# (N, P): the smallest shapes that select each launch variant and sit on each
# boundary of N and P
SHAPES = [(300, 1500), (8656, 700), (8657, 700), (11541, 700), (11542, 700),
          (300, 16384), (300, 16385), (11542, 16385)]
# the zero-traffic scan: every variant, both scan limits
ZSCAN_SHAPES = [(300, 1500), (8657, 700), (11542, 700), (300, 16385), (11542, 16385)]


def window(P):
    """Pods per round of the kernel launch_commit picks for P pods."""
    return 64 if -(-P // POD_PAD) * POD_PAD <= ONE_WAVE_MAX_PODS else 1024


def variant(N, P):
    """The kernel launch_commit picks (its conditions, restated)."""
    lds = N <= LDS_CAP_MAX_NODES
    if window(P) == 64:
        return "k_commit_w<true,true>" if N <= AOS_MAX_NODES else \
            "k_commit_w<true,false>" if lds else "k_commit_w<false>"
    return "k_commit<true>" if lds else "k_commit<false>"


def default_free(N):
    """Capacities that differ per node and per resource, so a mis-indexed
    capacity image changes a placement instead of reading an equal value."""
    n = np.arange(N, dtype=np.int64)
    return np.stack([1000 + 7 * n, 10**6 + 13 * n, 3 + n % 5], 1)


def row(nodes, costs, n_usable=None):
    """One list: keys of (cost, node) ascending, padded with KEY_INVALID, and
    the key of its n_usable-th entry as bound (None: complete list)."""
    k = np.sort(keys_from_costs(np.asarray(nodes, np.int64), np.asarray(costs, np.int64)))
    out = np.full(KC, KEY_INVALID, np.uint64)
    out[:len(k)] = k
    return out, (KEY_INVALID if n_usable is None else out[n_usable - 1])


def _case(keys, bounds, req, free, zero, fixups):
    assert (keys[:, 1:] >= keys[:, :-1]).all()  # ascending (as the API demands)
    assert free.min() >= 0 and free.max() <= 2**31 - 1 and req.min() >= 0
    return dict(keys=keys, bounds=bounds, req=req.astype(np.int32), free=free.astype(np.int32),
                zero=zero, fixups=fixups)


def herd(N, P, rng):
    """(a) Every pod lists the same 8 nodes; node j holds k_j pods, k below and
    above the window width, each limited by another resource.  Pods past the
    total either have complete lists (-1) or halt the walk."""
    W = window(P)
    nodes = [N - 1, 7, N - 33, N // 2, N - 2, 3, N - 64, N // 3]
    room = [40, 64, 65, 100, 17, 130, 1, 63] if P < 8000 else \
        [700, 1024, 1025, 1500, 300, 2100, 1, 1023]
    assert min(room) < W < max(room) and sum(room) + 200 < P
    r = (10, 1000, 1)
    free = default_free(N)
    for j, (n, k) in enumerate(zip(nodes, room)):
        free[n] = (10**6 + 7 * n, 10**9 + 13 * n, 10**5 + n % 5)
        free[n, j % 3] = k * r[j % 3] + r[j % 3] - 1  # room for exactly k pods
    lst, last = row(nodes, 10 + 3 * np.arange(KC), KC)
    T = sum(room)
    keys = np.tile(lst, (P, 1))
    bounds = np.where(np.arange(P) % 3 > 0, last, KEY_INVALID).astype(np.uint64)
    bounds[T:] = KEY_INVALID  # nothing fits any more: -1 ...
    halts = [T + d for d in (5, 70, 71, 200)]
    fixups = {}
    for i, p in enumerate(halts):  # ... or a halt; the fresh list names a node with room
        bounds[p] = last
        fixups[p] = row([nodes[0], N - 5 - i], [1, 2])
    req = np.tile(np.array(r, np.int64), (P, 1))
    return _case(keys, bounds, req, free, np.zeros(P, bool), fixups)


def mixed(N, P, rng):
    """(b) Zero, small, around-FETCH_SUB_MAX and huge requests mixed on shared
    nodes with capacities up to 2^31 - 1; nodes tight in one resource only
    (partial grants that must be released), nodes of capacity 0 offered to
    zero-request pods, and roomy nodes in keys past the bound."""
    free = default_free(N)
    ordinary = [11, 12, N // 4, N // 4 + 1, N // 2 + 3, N - 3, N - 10, N - 40, N - 63, 20]
    big = [N - 1, 5, N // 3, N - 20]
    for i, n in enumerate(big):
        free[n] = (2**31 - 1 - 7 * i, 2**31 - 1 - 13 * i, 2**31 - 1 - i)
    tight = [N - 2, N // 5, 6]
    free[N - 2] = (2**31 - 1, 1500, 10**6)  # cpu granted, memory refused
    free[N // 5] = (700, 2**31 - 1, 10**6)  # cpu refused, memory granted
    free[6] = (2**30, 2**30, 2)             # the pod slot refused
    empty = [N - 4, N - 12]
    free[empty] = 0
    decoy = [N - 6, N - 7, 30, 31]
    for i, n in enumerate(decoy):
        free[n] = (2**31 - 1 - n, 2**31 - 2 - n, 2**30 + i)
    pool = np.array(ordinary + big + tight)
    tail = pool[pool >= N - 64]  # every list reaches into the last 64 nodes

    def draw(size):
        cls = rng.choice(4, size, p=[0.2, 0.55, 0.15, 0.1])
        v = [np.zeros(size, np.int64), rng.integers(1, 501, size),
             FETCH_SUB_MAX + rng.integers(-1, 2, size), rng.integers(2**29, 2**30 + 1, size)]
        return np.choose(cls, v)

    req = np.stack([draw(P), draw(P), draw(P)], 1)
    nothing = rng.random(P) < 0.1
    req[nothing] = 0
    keys = np.full((P, KC), KEY_INVALID, np.uint64)
    bounds = np.full(P, KEY_INVALID, np.uint64)
    n_use = np.zeros(P, np.int64)
    for p in range(P):
        complete = rng.random() < 0.4
        m = int(rng.integers(1, 9)) if complete else int(rng.choice([1, 2, 3, 4, 4, 4]))
        t = int(rng.choice(tail))
        nodes = [t] + rng.choice(pool[pool != t], m - 1, replace=False).tolist()
        costs = rng.choice(np.arange(-50, 200), m, replace=False).tolist()
        if nothing[p]:  # a zero request fits a node of capacity 0: its best candidate
            i = int(np.argmin(costs))
            nodes[i], costs[i] = empty[p % 2], -60
        if not complete:
            nodes += decoy
            costs += [300, 301, 302, 303]
        keys[p], bounds[p] = row(nodes, costs, None if complete else m)
        if not complete and p % 2:  # a bound between two keys: same cost, highest node
            bounds[p] |= np.uint64(0xFFFFFFFF)
        n_use[p] = m
    # keep three halts (their fresh list: the same keys, complete, so the roomy
    # nodes become usable); any further pod that would halt gets a complete list
    fixups, p, inv = {}, 0, int(KEY_INVALID)
    K, B, R, cap = keys.tolist(), bounds.tolist(), req.tolist(), free.tolist()
    out = np.zeros(P, np.int64)
    while True:
        p = commit_walk(K, B, R, [False] * P, cap, p, out, out, out)
        if p == P:
            break
        if len(fixups) < 3:
            fixups[p] = (keys[p].copy(), KEY_INVALID)
        else:
            keys[p, n_use[p]:] = KEY_INVALID
            bounds[p] = KEY_INVALID
            K[p] = keys[p].tolist()
        B[p] = inv
    return _case(keys, bounds, req, free, np.zeros(P, bool), fixups)


def halting_pods(P):
    h = {0, 128, 193, 322, 387, 447, 1023, 1024, 2047, 2048, 5121, P - 1}
    return sorted(p for p in h if p < P)


def stops(N, P, rng):
    """(c) Halts at p % 64 in {0, 1, 2, 3, 63}, p % 1024 in {0, 1023} and
    p = P - 1 (incomplete lists on full nodes); each is resumed with a fresh
    list, so walks begin at odd pods and at pods that are no multiple of 4."""
    free = default_free(N)
    pool = np.array([N - 1, N - 2, N - 17, N - 31, N - 64, 4, 17, N // 2, N // 3, N // 7, 40, N - 5])
    for n in pool:
        free[n] = (10**7 + 7 * n, 10**9 + 13 * n, 10**5 + n % 5)
    last64 = pool[pool >= N - 64]  # every list reaches into the last 64 nodes
    full = [N - 9, 9, N // 2 + 1, N - 50]
    free[full, 2] = 0
    roomy = N - 8
    free[roomy] = (2**31 - 1, 2**31 - 1, 2**31 - 1)
    req = np.stack([rng.integers(1, 41, P), rng.integers(100, 2001, P), np.ones(P, np.int64)], 1)
    keys = np.full((P, KC), KEY_INVALID, np.uint64)
    bounds = np.full(P, KEY_INVALID, np.uint64)
    halts = halting_pods(P)
    assert {p % 64 for p in halts} >= {0, 1, 2, 3, 63} and P - 1 in halts
    fixups = {}
    for p in range(P):
        if p in halts:
            keys[p], bounds[p] = row(full + [roomy], [3, 5, 8, 13, 21], 4)
            fixups[p] = row([full[p % 4], int(last64[p % len(last64)])], [2, 6])
            continue
        t = int(rng.choice(last64))
        nodes = [t] + rng.choice(pool[pool != t], 2, replace=False).tolist()
        costs = rng.choice(200, 3, replace=False).tolist()
        if rng.random() < 0.3:
            keys[p], bounds[p] = row(nodes, costs)
        else:
            keys[p], bounds[p] = row(nodes + [roomy], costs + [250], 3)
    return _case(keys, bounds, req, free, np.zeros(P, bool), fixups)


def zkey(node):
    return np.uint64((ZERO_COST_HI << 32) | int(node))


def zscan(N, P, rng):
    """Zero-traffic pods whose lists (low-index nodes, all full) are exhausted:
    the first fitting node above the bound's node lies 1..16 nodes above, is
    missing up to N - 1 from a bound within 16 of it, the bound is N - 1
    itself, (capacity in LDS) 17..1,024 above, or (N >= 8,657) further than
    1,024 above; ordinary pods carry the same lists and must halt; five pods
    of one window contend for the same first-fit nodes."""
    lds = N <= LDS_CAP_MAX_NODES
    n = np.arange(N, dtype=np.int64)
    # every node full for any request of cpu >= 10, memory >= 500, 1 pod slot:
    # by cpu, by memory or by pod slots in turn
    free = default_free(N)
    free[n % 3 == 0, 0] = 5 + n[n % 3 == 0] % 4
    free[n % 3 == 1, 1] = 100 + n[n % 3 == 1] % 200
    free[n % 3 == 2, 2] = 0
    BIG, TINY = (100, 5000, 1), (10, 500, 1)
    filler_nodes = [12, 13, 14, 15]
    for m in filler_nodes:
        free[m] = (2**30 + 7 * m, 2**31 - 1 - 13 * m, 2**20 + m)

    def open_(m, room):
        free[m] = (1000 + 7 * m, 10**6 + 13 * m, room)

    specs = []  # (zero-traffic, request, bound's node, fresh list's node or None)
    for i, d in enumerate((1, 2, 8, 9, 16)):
        open_(20 + 20 * i + d, 1)
        specs.append((True, TINY if i % 2 else BIG, 20 + 20 * i, None))
    open_(153, 4)
    specs.append((False, BIG, 150, 153))  # an ordinary pod: halts, is not scanned
    first_contender = len(specs)
    for m, room in ((132, 1), (135, 2), (139, 1), (146, 1)):
        open_(m, room)
    specs += [(True, BIG, 130, None)] * 5  # the window that starts at the halted pod
    if lds:
        open_(177, 1)
        specs.append((True, BIG, 160, None))  # 17 above
        if N >= 8657:
            open_(200 + ZSCAN_LDS, 1)
            specs.append((True, BIG, 200, None))  # exactly at the limit
        else:
            open_(280, 1)
            specs.append((True, BIG, 180, None))
    specs.append((False, TINY, 150, 153))
    free[N - 1] = (50, 10**6 + 13 * (N - 1), 1)  # fits one TINY pod, never a BIG one
    specs.append((True, TINY, N - 9, None))      # takes the last node
    specs += [(True, BIG, N - 1 - d, None) for d in (1, 7, 16)]  # nothing fits up to N - 1
    specs.append((False, BIG, 150, 153))
    specs += [(True, BIG, N - 1, None), (True, TINY, N - 1, None), (True, TINY, N - 2, None)]
    specs.append((True, BIG, 150, None))
    if N >= 8657:
        open_(1300 + ZSCAN_LDS + 1, 1)
        open_(3900, 1)
        specs += [(True, BIG, 1300, None), (True, TINY, 2400, None)]  # beyond every scan limit
    where, p = [], 5
    for i in range(len(specs)):
        where.append(p)
        p += 1 if first_contender - 1 <= i < first_contender + 4 else 19
    assert p < P and {q % 4 for q, s in zip(where, specs) if not s[0]} - {0}

    req = np.stack([rng.integers(1, 51, P), rng.integers(100, 3001, P), np.ones(P, np.int64)], 1)
    zero = rng.random(P) < 0.5
    keys = np.full((P, KC), KEY_INVALID, np.uint64)
    bounds = np.full(P, KEY_INVALID, np.uint64)
    for q in range(P):  # fillers: their first candidate fits
        if zero[q]:
            m = np.sort(rng.choice(filler_nodes, int(rng.integers(1, 5)), replace=False))
            keys[q, :len(m)] = [zkey(x) for x in m]
            bounds[q] = keys[q, len(m) - 1]
        else:
            m = rng.choice(filler_nodes, 2, replace=False)
            keys[q], bounds[q] = row(m, [3, 9], 2 if q % 2 else None)
    fixups = {}
    for q, (z, r, bn, fix) in zip(where, specs):
        zero[q], req[q] = z, r
        keys[q] = [zkey(x) for x in np.sort(rng.choice(12, KC, replace=False))]
        bounds[q] = zkey(bn)
        if fix is not None:
            fixups[q] = row([fix], [7])
    return _case(keys, bounds, req, free, zero, fixups)


GENERATORS = {"herd": herd, "mixed": mixed, "stops": stops, "zscan": zscan}
_made = {}


def make(name, N, P):
    """The (seeded, cached) case of one generator at one shape; read-only."""
    if (name, N, P) not in _made:
        rng = np.random.default_rng([sorted(GENERATORS).index(name), N, P])
        _made[name, N, P] = GENERATORS[name](N, P, rng)
    return _made[name, N, P]


def ref_walk(case):
    """The whole walk by commit_ref: halt, write the pod's fresh list, resume.
    Returns (node, score, free_after, halts, dist) over all pods."""
    keys, bounds = case["keys"].copy(), case["bounds"].copy()
    P = len(bounds)
    node, score = np.full(P, -3, np.int32), np.zeros(P, np.int64)
    dist = np.full(P, -1, np.int64)
    p, cur, halts = 0, case["free"], []
    while True:
        nd, sc, cur, stop, ds = commit_ref(keys, bounds, case["req"], cur, case["zero"], p, True)
        node[p:stop], score[p:stop], dist[p:stop] = nd[p:stop], sc[p:stop], ds[p:stop]
        if stop == P:
            return node, score, cur, halts, dist
        halts.append(stop)
        keys[stop], bounds[stop] = case["fixups"][stop]
        p = stop


def zscan_rows(case):
    """How often each row of the scan's contract occurs in a zscan case."""
    N = len(case["free"])
    node, _, _, halts, dist = ref_walk(case)
    bn = (case["bounds"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    scanned, found = dist >= 0, node >= 0
    contended = {}
    for p in np.flatnonzero(scanned & found):
        contended.setdefault(int(bn[p]), set()).add(int(node[p]))
    return dict(near=int((scanned & found & (dist >= 1) & (dist <= ZSCAN_L2)).sum()),
                none_near_end=int((scanned & ~found & (dist >= 1) & (dist <= ZSCAN_L2)).sum()),
                bound_is_last=int((scanned & ~found & (bn == N - 1)).sum()),
                mid=int((scanned & found & (dist > ZSCAN_L2) & (dist <= ZSCAN_LDS)).sum()),
                at_lds_limit=int((scanned & found & (dist == ZSCAN_LDS)).sum()),
                far=int((scanned & found & (dist > ZSCAN_LDS)).sum()),
                last_node=int((scanned & (node == N - 1)).sum()),
                ordinary_halts=len(halts),
                contended=max(len(v) for v in contended.values()))
