"""Operands and references for the float cost paths (NAS_DT_F32, NAS_DT_BF16).
No GPU is used here.

Exact operand classes for fp32.  NAS_DT_F32 splits each operand into three
bf16 planes (k_misc.hip k_split6: h = bf16(x), m = bf16(x - h), l = bf16(x - h
- m)) and sums six plane products in fp32.  In every class below each operand
is h + m + l exactly, the three dropped plane products are zero, and every
product and every partial sum in any order is a multiple of the class's
quantum q below 2^24 q -- exactly representable in fp32.  The GPU must
therefore reproduce the fp64 oracle bit for bit: costs, candidate lists,
placements and remaining capacity.  tests/test_float_cases_cpu.py holds the
classes to these conditions at the sizes the GPU tests use.

  class    latency L                       traffic WA (non-zeros)         planes
  L20xW1   +-odd integers in [2^19, 2^20)  +-1                            L: h m l, WA: h
  L1xW20   +-1, +-2                        +-odd integers in [2^19, 2^20) WA: h m l, L: h
  M10x10   +-integers in [513, 1024)       +-integers in [513, 1024)      both: h m
  dyadic   integers in [513, 1024) / 8     +-integers in [513, 1024) / 64 both: h m

Every traffic row has at most 8 non-zeros (7 in L1xW20, so that 7 * 2 * 2^20
stays below 2^24), and some rows none.  signed=False gives the all-positive
variant: a row's costs then lie within a few binades, so the cost epilogue
keeps its packed keys.  With signed=True every row has costs of both signs
(the float keys of a lane span far more than 2^26: the exact select
network); in `dyadic`, whose latency is positive, the signed traffic comes
in +w / -w pairs on different nodes for that.
"""
import numpy as np

from util import bf16_bits_to_f64, f32_to_bf16_bits

CLASSES = ("L20xW1", "L1xW20", "M10x10", "dyadic")
QUANTUM = {"L20xW1": 1.0, "L1xW20": 1.0, "M10x10": 1.0, "dyadic": 2.0 ** -9}
MAX_NNZ = {"L20xW1": 8, "L1xW20": 7, "M10x10": 8, "dyadic": 8}


def _odd20(rng, shape):
    return (2 * rng.integers(2 ** 18, 2 ** 19, shape) + 1).astype(np.float64)


def _int10(rng, shape):
    return rng.integers(513, 1024, shape).astype(np.float64)


def _signs(rng, shape, signed):
    return rng.choice([-1.0, 1.0], shape) if signed else np.ones(shape)


def exact_operands(rng, cls, P, N, signed=True, dup=0, hot=0):
    """-> WA (P, N) float32, L (N, N) float32, pairs.

    dup: that many latency columns are overwritten with a copy of a
    lower-numbered column; pairs lists (source, copy), source < copy -- the
    two nodes then cost every pod bit-identically.
    hot: nodes [0, hot) become the cheapest for every pod: small-magnitude
    latency columns in the positive variants; in the signed ones the traffic's
    sign becomes a function of the peer node alone, and the hot columns carry
    the opposite sign at near-largest magnitude (every value stays inside its
    class)."""
    if cls == "L20xW1":
        L = _signs(rng, (N, N), signed) * _odd20(rng, (N, N))
        val = lambda k: _signs(rng, k, signed)  # noqa: E731
    elif cls == "L1xW20":
        L = _signs(rng, (N, N), signed) * rng.integers(1, 3, (N, N))
        val = lambda k: _signs(rng, k, signed) * _odd20(rng, k)  # noqa: E731
    elif cls == "M10x10":
        L = _signs(rng, (N, N), signed) * _int10(rng, (N, N))
        val = lambda k: _signs(rng, k, signed) * _int10(rng, k)  # noqa: E731
    elif cls == "dyadic":
        L = _int10(rng, (N, N)) / 8
        val = lambda k: _int10(rng, k) / 64  # noqa: E731
    else:
        raise ValueError(cls)
    WA = np.zeros((P, N))
    for p in range(P):
        k = int(rng.integers(0, min(MAX_NNZ[cls], N) + 1))
        if cls == "dyadic" and signed and N >= 2:
            k -= k % 2
        cols = rng.choice(N, k, replace=False)
        v = val(k)
        if cls == "dyadic" and signed:  # +w / -w pairs on two nodes
            v[1::2] = -v[0:2 * (k // 2):2]
        WA[p, cols] = v
    if hot:
        if signed:
            s = _signs(rng, N, True)
            WA = np.abs(WA) * s[None, :]
            top = {"L20xW1": lambda k: 2.0 ** 20 - 1 - 2 * rng.integers(0, 64, k),
                   "L1xW20": lambda k: np.full(k, 2.0),
                   "M10x10": lambda k: 1023.0 - rng.integers(0, 8, k),
                   "dyadic": None}[cls]
            if top is None:
                raise ValueError("dyadic latency is positive: no signed hot nodes")
            L[:, :hot] = -s[:, None] * top((N, hot))
        else:
            low = {"L20xW1": lambda k: 2.0 ** 19 + 1 + 2 * rng.integers(0, 64, k),
                   "L1xW20": lambda k: np.ones(k),
                   "M10x10": lambda k: 513.0 + rng.integers(0, 8, k),
                   "dyadic": lambda k: (513.0 + rng.integers(0, 8, k)) / 8}[cls]
            L[:, :hot] = low((N, hot))
    pairs = []
    if dup and N >= 2:
        copies = rng.choice(np.arange(max(1, hot), N), min(dup, N - max(1, hot)), replace=False)
        for b in sorted(copies.tolist()):
            if any(b == a for a, _ in pairs):
                continue  # a source stays a source
            lower = [a for a in range(b) if all(a != c for _, c in pairs)]
            a = int(rng.choice(lower))
            L[:, b] = L[:, a]
            pairs.append((a, b))
    WA32, L32 = WA.astype(np.float32), L.astype(np.float32)
    assert np.array_equal(WA32, WA) and np.array_equal(L32, L)
    return WA32, L32, pairs


def tight_capacity(rng, P, N, slots=2, skew=False):
    """free (N, 3), req (P, 3) int32: about half the (pod, node) pairs fit by
    cpu, and `slots` pods per node at the most, so lists run dry during the
    commit and -- with P > slots * N -- pods stay unschedulable.  skew: most
    nodes are small in cpu and memory, so that already at the first scoring
    pods range from no fitting node at all to far more than 8."""
    if skew:
        cpu = 1 + (700 * rng.random(N) ** 4).astype(np.int64)
        mem = 1000 + (1_200_000 * rng.random(N) ** 2).astype(np.int64)
    else:
        cpu, mem = rng.integers(100, 700, N), rng.integers(300_000, 2_000_000, N)
    free = np.stack([cpu, mem, np.full(N, slots)], 1).astype(np.int32)
    req = np.stack([rng.integers(1, 540, P), rng.integers(7_464, 303_749, P),
                    np.ones(P, np.int64)], 1).astype(np.int32)
    return free, req


def int_bf16_operands(rng, P, N, dup=0):
    """Signed integer-valued bf16 operands (at most 8 significant bits, dense
    traffic with some -0.0 and empty rows): exact on the bf16 path.
    -> WA bits (P, N) uint16, L bits (N, N) uint16, pairs."""
    WA = rng.integers(-50, 51, (P, N)).astype(np.float32)
    L = rng.integers(-20, 21, (N, N)).astype(np.float32)
    WA[::7] = -0.0
    WA[3::7] = 0.0
    pairs = []
    for b in sorted(rng.choice(np.arange(1, N), min(dup, N - 1), replace=False).tolist()):
        a = int(rng.integers(0, b))
        L[:, b] = L[:, a]
        pairs.append((a, b))
    return f32_to_bf16_bits(WA), f32_to_bf16_bits(L), pairs


# ------------------------------------------------------------- k_split6 model
def _rne_bf16(x):
    """float64 values exactly representable in fp32 -> nearest-even bf16, as float64."""
    x32 = np.asarray(x, np.float64).astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    return bf16_bits_to_f64(f32_to_bf16_bits(x32))


def split6(x):
    """The three bf16 planes of k_split6, as float64: h = rne(x), m = rne(x -
    h), l = rne(x - h - m)."""
    x = np.asarray(x, np.float64)
    h = _rne_bf16(x)
    m = _rne_bf16(x - h)
    lo = _rne_bf16(x - h - m)
    return h, m, lo


# plane of each of the six K-segments (k_misc.hip k_split6): A = latency, B = traffic
A_PAT = "hhmhlm"
B_PAT = "hmhlhm"


def six_term(WA, L):
    """-> (sum, abs_sum), both (P, N) float64: the six-segment contraction of
    the plane patterns, and the same with every plane product's magnitude."""
    a = dict(zip("hml", split6(L)))
    b = dict(zip("hml", split6(WA)))
    total = np.zeros((WA.shape[0], L.shape[1]))
    mag = np.zeros_like(total)
    for pa, pb in zip(A_PAT, B_PAT):
        total += b[pb] @ a[pa]
        mag += np.abs(b[pb]) @ np.abs(a[pa])
    return total, mag


# ------------------------------------------------------- bf16 CSR aggregation
def csr_bf16_reference(row_ptr, peer, w_bits, N):
    """k_csr_bf16's contract: per (pod, node) the weights summed as float32
    from +0 in CSR order, rounded once to bf16 (nearest even); peers < 0 or
    >= N skipped.  -> dense bf16 bits (P, N) uint16."""
    P = len(row_ptr) - 1
    w = (np.asarray(w_bits, np.uint16).astype(np.uint32) << 16).view(np.float32)
    acc = np.zeros((P, N), np.float32)
    for p in range(P):
        for x in range(row_ptr[p], row_ptr[p + 1]):
            m = int(peer[x])
            if 0 <= m < N:
                acc[p, m] = np.float32(acc[p, m] + w[x])
    return f32_to_bf16_bits(acc)


def csr_bf16_case(rng, P, N):
    """CSR traffic for k_csr_bf16 with every fp32 sum exact (bf16 weights of 8
    significant bits within [0.5, 512), at most 12 per (pod, node) outside
    pod 1's whole-number weights: the reference does not depend on the
    summation order).  Degrees 0..12 with empty rows; skipped peers -1, N,
    N + 5, 2^30; non-adjacent duplicates; +w / -w pairs; and planted rows:
      pod 0   256+1 -> 256 (tie, down), 258+1 -> 260 (tie, up),
              255+0.5 -> 256 (carry), each split by another node's entry
      pod 1   ~300 peers over ~10 nodes (the O(nnz^2) dedupe walk)
      pod 2   every weight cancelled by its negative: the row is +0
    -> row_ptr int32 (P + 1), peer int32, weight bits uint16, planted dict."""
    rows_p, rows_w = [], []

    def bf(v):
        b = f32_to_bf16_bits(np.asarray(v, np.float32))
        assert np.array_equal(bf16_bits_to_f64(b), np.asarray(v, np.float64))
        return b

    for p in range(P):
        deg = int(rng.integers(0, 13))
        if p % 11 == 5:
            deg = 0
        pe = rng.integers(0, N, deg)
        if deg >= 3 and p % 2:
            pe[-1] = pe[0]  # a duplicate that is not adjacent
        bad = rng.random(deg) < 0.2
        pe[bad] = rng.choice([-1, N, N + 5, 2 ** 30], int(bad.sum()))
        # 8-bit mantissas over four binades: any sum of <= 12 is exact in fp32
        wv = rng.integers(128, 256, deg) * 2.0 ** rng.integers(-8, -4, deg) * rng.choice([-1, 1], deg)
        if deg >= 4 and p % 3 == 0:
            pe[2], wv[2] = pe[1], -wv[1]  # +w, -w to one node: +0
        rows_p.append(pe.astype(np.int64))
        rows_w.append(wv)
    a, b, c, d = 3, N - 1, 64, 77
    rows_p[0] = np.array([a, d, a, b, -1, b, c, N, c, 2 ** 30])
    rows_w[0] = np.array([256.0, 3.0, 1.0, 258.0, 9.0, 1.0, 255.0, 7.0, 0.5, 5.0])
    nodes = rng.choice(N, 10, replace=False)
    rows_p[1] = nodes[rng.integers(0, 10, 300)]
    rows_w[1] = rng.integers(1, 4, 300).astype(np.float64)  # sums <= 900: exact
    pe = rng.integers(0, N, 6)
    wv = rng.integers(128, 256, 6) / 16.0
    rows_p[2] = np.concatenate([pe, [N + 5], pe[::-1]])
    rows_w[2] = np.concatenate([wv, [2.0], -wv[::-1]])
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows_p])]).astype(np.int32)
    peer = np.concatenate(rows_p).astype(np.int32)
    weight = bf(np.concatenate(rows_w))
    planted = {(0, a): 256.0, (0, b): 260.0, (0, c): 256.0, (0, d): 3.0}
    return row_ptr, peer, weight, planted


# ------------------------------------ signed, wide-range operands (tolerance)
def measured_operands(rng, P, N):
    """Measured-style operands that are not exact: latency log-uniform over
    1e-2 .. 1e6, traffic log-uniform over 1e-6 .. 1e5, about half the entries
    of each negated.  -> WA (P, N), L (N, N) float32."""
    L = 10.0 ** rng.uniform(-2, 6, (N, N)) * rng.choice([-1.0, 1.0], (N, N))
    WA = 10.0 ** rng.uniform(-6, 5, (P, N)) * rng.choice([-1.0, 1.0], (P, N))
    return WA.astype(np.float32), L.astype(np.float32)


def check_within_abs_sum(node, cf, cnt, exact, want_cost, want_cnt, S, rel_tol):
    """The float paths' accuracy contract (include/nas.h) on returned candidate
    lists: every candidate's cost_f within rel_tol * S[p, n] of the exact cost,
    S[p, n] = sum_m |WA[p, m] * L[m, n]| in fp64 -- the cost's own magnitude
    when nothing cancels --, and the j-th candidate's exact cost within rel_tol
    * max_n S[p, n] of the oracle's j-th best.  -> the measured max |err| / S."""
    assert (cnt >= np.minimum(4, want_cnt)).all()
    rows = np.arange(len(node))[:, None]
    use = np.arange(node.shape[1])[None, :] < cnt[:, None]
    assert (node[use] >= 0).all()
    at = np.maximum(node, 0)
    err = np.abs(cf.astype(np.float64) - exact[rows, at])
    ratio = (err / S[rows, at])[use].max()
    print(f"max |cost_f - exact| / sum_m |WA L| = {ratio:.3e} (bound {rel_tol:.0e})")
    assert (err <= rel_tol * S[rows, at])[use].all(), ratio
    rank = np.abs(exact[rows, at] - want_cost)
    print(f"max rank gap / max_n sum_m |WA L| = {(rank / S.max(1)[:, None])[use].max():.3e}")
    assert (rank <= rel_tol * S.max(1)[:, None])[use].all()
    return ratio


# ------------------------------------------- the cases of the GPU tests, seeded
SMALL_N = (1, 2, 63, 65, 130, 257)
SMALL_P = (1, 300)
VARIANTS = [(c, s) for c in CLASSES for s in (True, False)]
WIDE_SHAPE = (33000, 256)
WIDE_CLASSES = ("L20xW1", "M10x10")
COMP_SHAPE = (600, 301)
COMP_VARIANTS = [("L20xW1", True), ("M10x10", False)]  # select network / packed keys
# the cost-row cache case.  Tried on the GPU at P = 50 .. 2,000 (DESIGN.md, fp32
# path): rescore_rounds and rescored_pods are non-zero from P = 50 on, under
# all four option pairs; P = 1,000 is the smallest tried at which the herd
# plan's counters differ from the pipelined plan's (below it both plans are
# one chunk), so that each pair runs a plan of its own
CACHE_SHAPE = (1000, 700)
CACHE_HOT = 12


def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def small_case(cls, signed, P, N, dup=0):
    """-> WA, L, pairs, free, req at a small / odd shape."""
    rng = _rng("small", cls, signed, P, N, dup)
    WA, L, pairs = exact_operands(rng, cls, P, N, signed, dup=dup)
    free, req = tight_capacity(rng, P, N, slots=1 if N > 130 else 2, skew=True)
    if N <= 2:
        free[0, :2] = 600, 1_000_000  # (a node that most pods fit)
    # every 17th pod asks for the cpu of the 4th-roomiest node: its list is
    # short from the start
    req[::17, 0] = np.sort(free[:, 0])[::-1][min(3, N - 1)]
    return WA, L, pairs, free, req


def wide_case(cls):
    """Signed operands past the wide tile's threshold; 40 pod slots per node."""
    P, N = WIDE_SHAPE
    rng = _rng("wide", cls)
    WA, L, _ = exact_operands(rng, cls, P, N, True)
    free, req = tight_capacity(rng, P, N, slots=40)
    free[:, 0] *= 30
    free[:, 1] *= 30
    return WA, L, free, req


def comp_case(cls, signed, tag, hot=6):
    """A composition's cluster (tag seeds it): a few hot nodes so that commits
    stop and rescore."""
    P, N = COMP_SHAPE
    rng = _rng("comp", cls, signed, tag)
    WA, L, _ = exact_operands(rng, cls, P, N, signed, hot=hot)
    free, req = tight_capacity(rng, P, N, slots=2)
    free[:hot, :2] = 100_000, 100_000_000  # every pod fits the hot nodes: slots alone close them
    return WA, L, free, req


def cache_case(cls, signed):
    """CACHE_HOT hot nodes cheapest for every pod, 3 pod slots each."""
    P, N = CACHE_SHAPE
    rng = _rng("cache", cls, signed)
    WA, L, _ = exact_operands(rng, cls, P, N, signed, hot=CACHE_HOT)
    free, req = tight_capacity(rng, P, N, slots=3)
    free[:, 0] *= 4
    free[:CACHE_HOT, :2] = 100_000, 100_000_000
    return WA, L, free, req
