// k_cost_diag.hip -- DIAGNOSTIC ONLY (included by tools/mb_cost.hip and
// tools/mb_aux.hip, never built into libnas.so): the round-3 cost kernel
// with every measured-and-rejected variant of DESIGN.md §4 still selectable
// -- PIPE 1-7 (triple-buffered B, register staging, phased / staggered loops,
// L2 touches), SCHED 1-5 (pinned MFMA / ds_read interleaves, setprio,
// iglp_opt), NWN = 2 (one wave per SIMD), EPI 1-6 (main loop alone, top-1,
// exact select network, all-L2-hit and LDS-only ceilings), COST_AUX cache
// policies and the early overflow seeding.  The product kernel
// (../k_cost.hip) keeps only the shipped configuration.
// k_cost.hip -- network cost contraction on gfx950 MFMA with a fused
// fit-mask + per-pod top-k epilogue.
//
//   cost[p, n] = sum_m WA[p, m] * L[m, n]          (north star kernel (2))
//
// computed transposed, C^T[n, p] = sum_m Lt[n, m] * WA[p, m], so that the
// MFMA accumulator puts the NODE on the register axis and the POD on the
// lane axis: each lane then reduces its own pod's candidates in registers,
// with no cross-lane traffic until one lane^32 exchange (north star (3)).
// The cost matrix is never written to HBM.
//
//  * int8 path: v_mfma_i32_32x32x32_i8, int32 accumulation -- exact, so the
//    integer scores and the chosen nodes are bit-identical to the oracle.
//  * bf16 path: v_mfma_f32_32x32x16_bf16, fp32 accumulation; also the fp32
//    path, whose operands are split into three bf16 planes each and laid out
//    along a six-fold K (k_misc.hip k_split6: products to 2^-24 relative).
//
// Tile: 256 nodes x 256 pods per 512-thread workgroup (8 wave64 as 2 x 4),
// each wave 128 nodes x 64 pods = 4 x 2 MFMA 32x32 tiles.  K is staged 128
// bytes per row per step into a double-buffered LDS image (2 x 64 KiB) with
// global_load_lds_dwordx4 (LDS-DMA); rows are 128 B with a 16-byte-chunk XOR
// swizzle (chunk ^= (row >> 1) & 7) applied to the SOURCE address, so the
// ds_read_b128 fragment reads are bank-conflict free.  Workgroup ids are
// remapped so the blocks sharing an XCD's L2 cover a 4 (node tiles) x 8
// (pod tiles) super-tile.
//
// Epilogue: per lane, 64 (node, cost) values per pod -> mask from the fit
// kernel (bit per node) -> sorted top-4 of (orderable cost, node) in
// registers -> merged with lane^32 into an 8-list with an exactness bound
// (klist.h) -> merged across the two node-half waves through LDS ->
// partial[node_tile][pod][8] + pbound[node_tile][pod] (72 B per pod per tile).
#include "../klist.h"

#include <type_traits>

namespace nas {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

[[maybe_unused]] constexpr int THREADS = 512;  // the default (NWN = 4) workgroup, for tools/
constexpr int BM = COST_BM;   // nodes per tile
constexpr int BN = COST_BN;   // pods per tile
constexpr int BKB = COST_BKB; // bytes of K per LDS stage (full 128-byte lines)
constexpr int STAGE_BYTES = (BM + BN) * BKB;  // 64 KiB
constexpr int TILE_BYTES = BM * BKB;          // 32 KiB: one operand, one stage
#ifndef COST_PIPE
#define COST_PIPE 0
#endif
// XCD tile order: GM > 0 = node-group major (GM node tiles x every pod tile);
// GM = -PG = pod-group major (PG pod tiles x every node tile).  Pod groups of
// 4 (32 concurrent workgroups per XCD = 8 node tiles x 4 pod tiles) fetch
// fewer traffic rows from HBM per window and more latency rows from the
// Infinity Cache (Lt, 105 MB, fits it): 2.0-2.5% faster than GM = 4 in 4 of 4
// interleaved repetitions (profiles/r02_mb_cost_order.log)
#ifndef COST_GM
#define COST_GM (-4)
#endif
// the wide tile's order: pod groups of 2 (2 x 384 pods x every node tile):
// C3 pass 8.04-8.09 vs 8.09-8.12 ms for groups of 4 (launch equal), groups
// of 1 / 3 / 8 and node-group-major 2 / 8 slower (profiles/r02_s4_ab_gm.txt)
#ifndef COST_GM_WIDE
#define COST_GM_WIDE (-2)
#endif
// PIPE 0: A and B double-buffered (128 KiB).  PIPE 1: A (latency rows, mostly
// L2/MALL-resident) double-buffered, B (the 1 GB traffic stream, mostly HBM)
// triple-buffered so its loads get two K-steps of cover (160 KiB, all of LDS).
// PIPE 2: as 0, but B is staged through registers (global_load_dwordx4 ->
// ds_write_b128) instead of LDS-DMA; PIPE 3: both operands register-staged.
// PIPE 5 / 6: as 0, plus an L2 "touch" of the stage 2 / 3 K-steps ahead (one
// 4-byte LDS-DMA per 128-byte line of A and B into a junk LDS word, left in
// flight across the step's barrier), so the stage's own LDS-DMA one step
// later hits L2 instead of waiting on HBM / MALL; PIPE 7: as 5, B lines only.
template <int PIPE>
constexpr int lds_bytes() {
    return PIPE == 1 ? 5 * TILE_BYTES : PIPE >= 5 ? 2 * STAGE_BYTES + 256 : 2 * STAGE_BYTES;
}
#ifndef COST_SCHED
#define COST_SCHED 0
#endif
// wave layout of the 256 x 256 tile: NWN = 4 -> 8 waves (2 node halves x 4 pod
// quarters), each 128 nodes x 64 pods (4 x 2 MFMA tiles, 128 accumulator
// registers, two waves per SIMD); NWN = 2 -> 4 waves (2 x 2), each 128 nodes x
// 128 pods (4 x 4 tiles, 256 accumulator registers, one wave per SIMD): half
// the LDS fragment reads per MFMA (the layout hipBLASLt picks for this shape,
// MT256x256, 4 waves; profiles/r02_s3_vendor_gemm_kernels.txt)
#ifndef COST_NWN_I8
#define COST_NWN_I8 4
#endif
#ifndef COST_NWN_BF16
#define COST_NWN_BF16 4
#endif
template <int DT>
constexpr int cost_nwn() {
    return DT == NAS_DT_I8 ? COST_NWN_I8 : COST_NWN_BF16;
}
// the main scoring pass (no rescore window) on the wide tile: 256 nodes x
// 384 pods per 12-wave workgroup (3 waves per SIMD, each 128 x 64 as in the
// 8-wave layout, 160 KiB of LDS double buffer), 17% fewer staged bytes per
// MAC than 256 x 256
#ifndef COST_WIDE_I8
#define COST_WIDE_I8 1
#endif
#ifndef COST_WIDE_BF16
#define COST_WIDE_BF16 1
#endif
template <int DT>
constexpr bool cost_wide() {
    return DT == NAS_DT_I8 ? COST_WIDE_I8 : COST_WIDE_BF16;
}

#ifndef COST_OVF_EARLY
#define COST_OVF_EARLY 0
#endif

template <int DT>
struct Mma;

template <>
struct Mma<NAS_DT_I8> {
    using acc_t = v16i;
    static __device__ __forceinline__ acc_t mma(v4i a, v4i b, acc_t c) {
        return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ unsigned okey(int x) { return (unsigned)x ^ 0x80000000u; }
};

template <>
struct Mma<NAS_DT_BF16> {
    using acc_t = v16f;
    static __device__ __forceinline__ acc_t mma(v4i a, v4i b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                        __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ unsigned okey(float x) {
        x = x + 0.0f;  // -0 -> +0: the oracle compares costs, not sign bits
        const unsigned u = __float_as_uint(x);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
};

// cache policy of the LDS-DMA loads per operand (build-time knob for
// tools/mb_aux.hip; gfx950 CPol bits: 1 sc0, 2 nt, 16 sc1).  Measured round 2
// (same box, alternating): sc1 / sc0 sc1 equal to the default within 1%, nt
// on the traffic rows +5%, on both operands +15-30% -- default kept.
#ifndef COST_AUX_A
#define COST_AUX_A 0
#endif
#ifndef COST_AUX_B
#define COST_AUX_B 0
#endif
template <int AUX = 0>
__device__ __forceinline__ void glds16(const void *g, void *l) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)g,
                                     (void __attribute__((address_space(3))) *)l, 16, 0, AUX);
}

__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) {
    unsigned d;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// Per-lane running top-4 as separate (orderable cost, node) u32 words.
// A lane visits its nodes in ascending node order, so a new (x, n) sorts
// before entry j iff x < cost[j] strictly (an equal cost has the larger node):
// four independent 32-bit compares and a select network, no 64-bit compares.
struct Top4 {
    unsigned c[4], n[4];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = n[j] = 0xffffffffu;
    }
    __device__ __forceinline__ void insert(unsigned x, unsigned node) {
        const bool b0 = x < c[0], b1 = x < c[1], b2 = x < c[2], b3 = x < c[3];
        const unsigned c3 = b2 ? c[2] : (b3 ? x : c[3]), n3 = b2 ? n[2] : (b3 ? node : n[3]);
        const unsigned c2 = b1 ? c[1] : (b2 ? x : c[2]), n2 = b1 ? n[1] : (b2 ? node : n[2]);
        const unsigned c1 = b0 ? c[0] : (b1 ? x : c[1]), n1 = b0 ? n[0] : (b1 ? node : n[1]);
        c[0] = b0 ? x : c[0];
        n[0] = b0 ? node : n[0];
        c[1] = c1; n[1] = n1; c[2] = c2; n[2] = n2; c[3] = c3; n[3] = n3;
    }
    __device__ __forceinline__ u64 key(int j) const { return ((u64)c[j] << 32) | n[j]; }
};

// EPI != 0 are diagnostic variants for tools/mb_cost.hip: 1 = accumulators
// kept alive with an empty asm and no epilogue (times the main loop alone),
// 2 = per-lane top-1 instead of top-4, 6 = the exact Top4 select network
// only (the default takes the packed med3 path whenever every lane's keys
// span < 2^26 - 1).  SCHED selects the k-substep schedule
// (A/B'd in tools/mb_cost.hip and on the C3 bench): 0 hipcc's own (the
// default: ~1% ahead of 1 on the bench, 3 of 3 pairs), 1 pinned MFMA/ds_read
// interleave, 2 s_setprio(1) around each MFMA cluster, 3 iglp_opt(0),
// 4 iglp_opt(1).
// RMAP: a gathered rescore view -- view row q's traffic is WA row rowmap[q]
// (read in place by the LDS-DMA source addresses; rows past the view's count
// read its last row and are never merged)
template <int DT, int EPI = 0, int SCHED = COST_SCHED, int PIPE = COST_PIPE, int GM = COST_GM,
          bool RMAP = false, int NWN = 4, bool FUSE = (NWN == 6)>
__global__ void __launch_bounds__(128 * NWN, 1)
k_cost_topk(const unsigned char *__restrict__ Lt, const unsigned char *__restrict__ WA, int Kb,
            int n_mt, int n_nt, int p0, int Pp, const u64 *__restrict__ mask,
            u64 *__restrict__ partial, u64 *__restrict__ pbound, int node_base,
            const int *__restrict__ dyn_start, int dyn_hi, const int *__restrict__ dyn_hi_ptr,
            Ovf ov, const int *__restrict__ rowmap, FitSrc fs) {
    static_assert(!RMAP || PIPE == 0, "the row map is wired into the LDS-DMA staging only");
    static_assert(NWN == 4 || ((NWN == 2 || NWN == 6) && PIPE == 0 && (SCHED == 0 || SCHED == 2)),
                  "the 4- and 12-wave layouts have the two-stage LDS-DMA pipeline only");
    static_assert(NWN != 6 || (!RMAP && EPI == 0 && FUSE), "the wide tile serves the main pass only");
    static_assert(!FUSE || (!RMAP && EPI == 0 && PIPE == 0), "the fused fit: main-range launches");
    constexpr int NW = 2 * NWN;              // waves
    constexpr int NI = NWN == 2 ? 4 : 2;     // 32-pod MFMA tiles per wave
    constexpr int WPODS = 32 * NI;           // pods per wave
    constexpr int BNK = NWN * WPODS;         // pods per tile (256; the wide tile 384)
    constexpr int STG = (BM + BNK) * BKB;    // bytes per LDS stage (PIPE 0)
    constexpr int PPWA = (BM / 8 + NW - 1) / NW;   // 1 KiB LDS-DMA pieces of A per wave per stage
    constexpr int PPWB = (BNK / 8 + NW - 1) / NW;  // ... of B
    constexpr int PPW = PPWB;
    using M = Mma<DT>;
    using acc_t = typename M::acc_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // the fused fit's words after the main loop: behind the cross-wave merge's
    // lists ([NWN][NI][32][9] u64), inside the smallest staging image
    constexpr int FIT_LDS_OFF = 32768;
    static_assert(FIT_LDS_OFF >= NWN * NI * 32 * 9 * 8 &&
                  FIT_LDS_OFF + NW * NI * 2 * 64 * 8 <= 2 * STG, "fused-fit LDS words");

    // ---- XCD-aware tile order: blocks b, b+8, ... share an XCD (speed only)
    const int nwg = n_mt * n_nt;
    const int b = blockIdx.x;
    const int xcd = b & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b >> 3);
    int mt, nt;
    if constexpr (GM > 0) {
        // node-group major: GM node tiles x every pod tile, pod-minor
        const int gsize = GM * n_nt;
        const int g = v / gsize;
        const int first_mt = g * GM;
        const int gm = min(n_mt - first_mt, GM);
        mt = first_mt + (v % gsize) % gm;
        nt = (v % gsize) / gm;
    } else {
        // pod-group major (GM = -PG): PG pod tiles x every node tile, so an
        // XCD keeps one pod group's traffic rows (PG x 2.5 MB at C3) hot in
        // the memory-side cache while it sweeps the node tiles
        constexpr int PG = GM < 0 ? -GM : 1;
        const int gsize = PG * n_mt;
        const int g = v / gsize, r = v % gsize;
        const int first_nt = g * PG;
        const int pg = min(n_nt - first_nt, PG);
        mt = r / pg;
        nt = first_nt + r % pg;
    }
    const int cb = blockIdx.y;  // cluster of a batched launch
    if constexpr (FUSE) {
        fs.cap += (size_t)cb * 3 * fs.N;
        fs.req += (size_t)cb * 3 * Pp;
    }
    Lt += (size_t)cb * n_mt * BM * Kb;  // (tile order above: speed only)
    WA += (size_t)cb * Pp * Kb;
    mask += (size_t)cb * (n_mt * BM / 64) * Pp;
    partial += (size_t)cb * n_mt * Pp * KC;
    pbound += (size_t)cb * n_mt * Pp;
    if (dyn_start) {  // rescore slot: pod tiles from the window start in device memory
        const int s = dyn_start[cb * STATUS_INTS];
        if (s < 0) return;
        if (dyn_hi_ptr) dyn_hi = dyn_hi_ptr[cb * STATUS_INTS];
        p0 = s / BN * BN;
        if (p0 + nt * BNK >= dyn_hi) return;  // whole block: before any barrier
    }
    // the wide tile (BNK = 384 over a launch of 256-pod units): pods at and
    // past p_end (= dyn_hi, the launch's end) read rows past it (the next
    // launch's, or the WA_PAD_ROWS padding) and are never written
    const int p_end = (BNK != BN && !dyn_start) ? dyn_hi : 0x7fffffff;

    // (the wide tile: the wave index wave-uniform in SGPRs, and the lane index
    // re-derived after the main loop -- see below -- so that nothing per-lane
    // outlives the loop beside the 128 accumulators: at three waves per SIMD
    // the loop fills the 168 registers, and values held across it spilled)
    const int tid = threadIdx.x;
    int lane = tid & 63;
    const int w = NWN == 6 ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    const int wm = w / NWN, wn = w % NWN;

    const unsigned char *Ag = Lt + (size_t)mt * BM * Kb;
    const unsigned char *Bg = WA + (size_t)(p0 + nt * BNK) * Kb;
    if constexpr (EPI == 3) {  // diagnostic: every block streams tile (0, 0): all L2 hits
        Ag = Lt;
        Bg = WA;
    }

    // LDS-DMA staging: piece j of wave w fills rows (NW*j + w)*8 .. +8 of A
    // and of B (1 KiB each, lane-linear: lane l -> row + l/8, 16-byte chunk
    // l%8; whole 128-byte lines per row -- 64-byte row pieces measured 12%
    // slower); the chunk swizzle chunk ^= (row >> 1) & 7 is applied on the
    // SOURCE address so fragment reads are bank-conflict free.
    const int srow_in = lane >> 3;
    const int sq = lane & 7;
    // buffer b of operand A / B (PIPE 0: A|B interleaved per stage; PIPE 1:
    // A0 A1 B0 B1 B2)
    auto abuf = [&](int b) -> unsigned char * {
        return PIPE != 1 ? lds + b * STG : lds + b * TILE_BYTES;
    };
    auto bbuf = [&](int b) -> unsigned char * {
        return PIPE != 1 ? lds + b * STG + TILE_BYTES : lds + (2 + b) * TILE_BYTES;
    };
    // one 1 KiB LDS-DMA piece (8 rows x 128 B) of operand A / B: piece j of
    // wave w fills rows (NW*j + w)*8 .. +8
    auto pieceA = [&](int buf, int k0, int j) {
        if (BM / 8 % NW && j * NW + w >= BM / 8) return;
        const int r0 = (j * NW + w) * 8;
        const int row = r0 + srow_in;
        const int c = sq ^ ((row >> 1) & 7);
        glds16<COST_AUX_A>(Ag + (size_t)row * Kb + k0 + c * 16, abuf(buf) + r0 * BKB);
    };
    int bpod[PPW];  // RMAP: the WA rows of this lane's B pieces
    if constexpr (RMAP) {
#pragma unroll
        for (int j = 0; j < PPW; ++j)
            bpod[j] = rowmap[min(p0 + nt * BNK + (j * NW + w) * 8 + srow_in, dyn_hi - 1)];
    }
    auto pieceB = [&](int buf, int k0, int j) {
        if (BNK / 8 % NW && j * NW + w >= BNK / 8) return;
        const int r0 = (j * NW + w) * 8;
        const int row = r0 + srow_in;
        const int c = sq ^ ((row >> 1) & 7);
        const unsigned char *src = RMAP ? WA + (size_t)bpod[j] * Kb : Bg + (size_t)row * Kb;
        glds16<COST_AUX_B>(src + k0 + c * 16, bbuf(buf) + r0 * BKB);
    };
    // the wide tile stages A rows then B rows as one run of 80 pieces (the
    // B image follows the A image in LDS); piece pj of wave wu is 8 rows at
    // pj * 8, and since pj = 12 j + wu has the parity of wu, every piece of a
    // wave has the same swizzled lane offset: one VGPR, the row base uniform
    // (3 waves per SIMD leave 168 registers, 128 of them accumulators)
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const unsigned loff = (unsigned)(srow_in * Kb) +
                          ((unsigned)(sq ^ ((4 * (wu & 1) + (srow_in >> 1)) & 7)) << 4);
    auto piece6 = [&](int buf, int k0, int j) {
        const int pj = j * NW + wu;
        if (pj >= (BM + BNK) / 8) return;
        const unsigned char *base = pj < BM / 8 ? Ag + (size_t)pj * 8 * Kb
                                                : Bg + (size_t)(pj - BM / 8) * 8 * Kb;
        glds16<0>(base + k0 + loff, lds + buf * STG + pj * 8 * BKB);
    };
    auto stageA = [&](int buf, int k0) {
        if constexpr (NWN == 6) {
#pragma unroll
            for (int j = 0; j < ((BM + BNK) / 8 + NW - 1) / NW; ++j) piece6(buf, k0, j);
        } else {
#pragma unroll
            for (int j = 0; j < PPWA; ++j) pieceA(buf, k0, j);
        }
    };
    auto stageB = [&](int buf, int k0) {
        if constexpr (NWN != 6) {  // (the wide tile's stageA stages both)
#pragma unroll
            for (int j = 0; j < PPW; ++j) pieceB(buf, k0, j);
        }
    };

    // Fused fit (main-range launches: the pass's chunks launch back to back
    // with no k_fit between them -- a fit launch in front of every cost
    // launch could not start until a wide workgroup drained its CU, and the
    // cost launch behind it then waited too).  The workgroup decides the fit
    // words itself, exactly as k_fit does, after its main loop: per 64-node
    // chunk the minima / maxima of the free capacity (read then -- after the
    // previous chunks' commits and possibly during this chunk's predecessor's;
    // capacity only shrinks, so a "does not fit" read at any earlier time
    // still holds at the pod's turn) decide every pod that fits all valid
    // nodes or none; the rest compare against the lanes' capacities (three
    // ballots).  The words land where the k_fit mask words would (mwp).
    int rq[FUSE ? NI : 1][3];
    int fcap[2][3];
    auto fit_issue = [&]() {  // the requests of the lane's pods, its nodes' capacities
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int pod = min(p0 + nt * BNK + wn * WPODS + ni * 32 + (lane & 31), p_end - 1);
#pragma unroll
            for (int r = 0; r < 3; ++r) rq[ni][r] = fs.req[(size_t)r * Pp + pod];
        }
#pragma unroll
        for (int mi2 = 0; mi2 < 2; ++mi2) {
            const int nl = mt * BM + wm * 128 + mi2 * 64 + lane;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                fcap[mi2][r] = nl < fs.nloc ? __hip_atomic_load(const_cast<int *>(fs.cap) + (size_t)r * fs.N + fs.n0 + nl,
                                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                            : -1;
        }
    };
    // fit words: bit j of word (ni, mi2) = the lane's pod of group ni fits
    // node wm*128 + mi2*64 + j of the tile; each lane stores its own words in
    // LDS (fit_slot, past the cross-wave merge's region) and reads them back
    // per pod group in the epilogue (held in registers beside the 128
    // accumulators they spilled: 24 B of scratch per lane)
    auto fit_slot = [&](int ni, int mi2) -> u64 * {
        return reinterpret_cast<u64 *>(lds + FIT_LDS_OFF) + ((w * NI + ni) * 2 + mi2) * 64 + lane;
    };
    auto fit_words = [&]() {
#pragma unroll
        for (int mi2 = 0; mi2 < 2; ++mi2) {
            const bool real = mt * BM + wm * 128 + mi2 * 64 + lane < fs.nloc;
            const u64 valid = __builtin_amdgcn_ballot_w64(real);
            int mn[3], mx[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                int a = real ? fcap[mi2][r] : 0x7fffffff, x = real ? fcap[mi2][r] : (int)0x80000000;
#pragma unroll
                for (int o = 32; o; o >>= 1) {
                    a = min(a, __shfl_xor(a, o));
                    x = max(x, __shfl_xor(x, o));
                }
                mn[r] = __builtin_amdgcn_readfirstlane(a);
                mx[r] = __builtin_amdgcn_readfirstlane(x);
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int a = rq[ni][0], bq = rq[ni][1], d = rq[ni][2];
                const bool all = a <= mn[0] && bq <= mn[1] && d <= mn[2];
                const bool none = a > mx[0] || bq > mx[1] || d > mx[2];
                u64 word = all ? valid : 0ull;
                // lanes l and l + 32 hold the same pod: decide lanes 0..31
                u64 rest = __builtin_amdgcn_ballot_w64(!all && !none) & 0xffffffffull;
                while (rest) {
                    const int i = (int)__builtin_ctzll(rest);
                    rest &= rest - 1;
                    const int ra = __builtin_amdgcn_readlane(a, i), rb = __builtin_amdgcn_readlane(bq, i);
                    const int rd = __builtin_amdgcn_readlane(d, i);
                    const u64 m = __builtin_amdgcn_ballot_w64(ra <= fcap[mi2][0]) &
                                  __builtin_amdgcn_ballot_w64(rb <= fcap[mi2][1]) &
                                  __builtin_amdgcn_ballot_w64(rd <= fcap[mi2][2]);
                    if ((lane & 31) == i) word = m;
                }
                *fit_slot(ni, mi2) = word;
            }
        }
    };

    // the epilogue's fit-mask words, loaded now so their latency hides
    // under the main loop (k_fit wrote them before this launch)
    // (issued after the overflow seeding, whose loop they would otherwise
    // stay live across)
    u64 mwp[NI][2];
    auto load_mask = [&]() __attribute__((always_inline)) {
        if constexpr (!FUSE && (EPI == 0 || EPI == 2 || EPI == 6)) {
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int mi2 = 0; mi2 < 2; ++mi2) {
                    const int pod = min(p0 + nt * BNK + wn * WPODS + ni * 32 + (lane & 31), p_end - 1);
                    const int chunk = (mt * BM + wm * 128 + mi2 * 64) >> 6;
                    mwp[ni][mi2] = mask[(size_t)chunk * Pp + pod];
                }
        }
    };
    acc_t acc[4][NI];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = acc_t{};
    int fr = lane & 31, fh = lane >> 5;
    // ---- exact int32 traffic: the entries outside the int8 plane (nas::Ovf):
    // e * L[m][n] for the lane's 64 nodes per pod are the accumulators'
    // initial value (4 dwords of Lr per 32-node tile: rows (reg & 3) +
    // 8 * (reg >> 2) + 4 * fh are 4 groups of 4 consecutive nodes).  Both pod
    // groups' list bounds load together, and an entry's 16 row dwords (all
    // four 32-node tiles) in one round, so an entry costs two dependent
    // loads, not eight; the two-stage pipeline runs this behind its first
    // stage's LDS-DMA (the prologue waits once for both)
    // (the layout of rounds 1-2, inline: the wide tile, whose registers allow
    // one tile's row dwords at a time, and the 256 x 256 launches without the
    // fused fit -- node shards, rescore windows -- which must stay at <= 192
    // VGPRs: a node shard's merge / all-gather / commit kernels run beside a
    // cost workgroup only while its two waves per SIMD leave registers free
    // (at 256 VGPRs the G = 8 rehearsal pass rose from 1.39 to 1.50 ms:
    // profiles/r03_bisect_g8.txt))
    constexpr bool OVF_ROUND2 = NWN == 6 || !FUSE;
    if constexpr (OVF_ROUND2 && DT == NAS_DT_I8 && (EPI == 0 || EPI == 2 || EPI == 6)) {
        if (ov.ptr) {
            const int cnt_lim = ov.row_count ? *ov.row_count : 0x7fffffff;
            const signed char *lr = ov.Lr + (size_t)cb * ov.N * (n_mt * BM) + mt * BM + wm * 128 + 4 * fh;
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int r = p0 + nt * BNK + wn * WPODS + ni * 32 + (lane & 31);
                int beg = 0, end = 0;
                if (r < cnt_lim && r < p_end) {
                    const int pod = (ov.row_pod ? ov.row_pod[r] : r) + cb * Pp;
                    beg = ov.ptr[pod];
                    end = ov.ptr[pod + 1];
                }
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    for (int j = beg; j < end; ++j) {
                        const int e = ov.e[j];
                        const signed char *row = lr + (size_t)ov.m[j] * (n_mt * BM) + mi * 32;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int v = *reinterpret_cast<const int *>(row + 8 * g);
#pragma unroll
                            for (int c = 0; c < 4; ++c)
                                acc[mi][ni][4 * g + c] += e * (int)(signed char)(v >> (8 * c));
                        }
                    }
            }
        }
    }
    constexpr bool OVF_EARLY = COST_OVF_EARLY;
    auto seed_ovf = [&]() __attribute__((always_inline)) {
        if constexpr (!OVF_ROUND2 && DT == NAS_DT_I8 && (EPI == 0 || EPI == 2 || EPI == 6)) {
            if (ov.ptr) {
                const int cnt_lim = ov.row_count ? *ov.row_count : 0x7fffffff;
                const signed char *lr = ov.Lr + (size_t)cb * ov.N * (n_mt * BM) + mt * BM + wm * 128 + 4 * fh;
                // pod group ni's entries [beg, end)
                auto bounds = [&](int ni, int &beg, int &end) {
                    const int r = p0 + nt * BNK + wn * WPODS + ni * 32 + (lane & 31);
                    beg = end = 0;
                    if (r < cnt_lim && r < p_end) {
                        const int pod = (ov.row_pod ? ov.row_pod[r] : r) + cb * Pp;
                        beg = ov.ptr[pod];
                        end = ov.ptr[pod + 1];
                    }
                };
                {
                    int beg[NI], end[NI];
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) bounds(ni, beg[ni], end[ni]);
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        for (int j = beg[ni]; j < end[ni]; ++j) {
                            const int e = ov.e[j];
                            const signed char *row = lr + (size_t)ov.m[j] * (n_mt * BM);
                            int v[4][4];
#pragma unroll
                            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                                for (int g = 0; g < 4; ++g)
                                    v[mi][g] = *reinterpret_cast<const int *>(row + mi * 32 + 8 * g);
#pragma unroll
                            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                                for (int g = 0; g < 4; ++g)
#pragma unroll
                                    for (int c = 0; c < 4; ++c)
                                        acc[mi][ni][4 * g + c] += e * (int)(signed char)(v[mi][g] >> (8 * c));
                        }
                }
            }
        }
    };
    if constexpr (PIPE != 0 || OVF_EARLY) seed_ovf();
    if constexpr (PIPE != 0 || OVF_EARLY || NWN == 6) load_mask();

    // fragments of k-substep kk+1 are read from LDS while the 8 MFMAs of kk
    // run (register double buffer; the just-in-time schedule hipcc picks on
    // its own exposes the LDS latency every 4 MFMAs)
    // compute one K-step from LDS; `piece(kk)` issues the next stage's LDS-DMA
    // pieces that SCHED 5 spreads across the MFMA stream (their issue cost,
    // 60-185 cycles each, otherwise stalls the wave at the top of the step)
    auto compute = [&](int ab, int bbi, auto &&piece) {
        const unsigned char *As = abuf(ab);
        const unsigned char *Bs = bbuf(bbi);
        v4i a[2][4], bb[2][NI];
        auto read = [&](int kk, v4i (&ra)[4], v4i (&rb)[NI]) {
            const int c = kk * 2 + fh;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int r = wm * 128 + mi * 32 + fr;
                ra[mi] = *reinterpret_cast<const v4i *>(As + r * BKB + ((c ^ ((r >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int r = wn * WPODS + ni * 32 + fr;
                rb[ni] = *reinterpret_cast<const v4i *>(Bs + r * BKB + ((c ^ ((r >> 1) & 7)) << 4));
            }
        };
        read(0, a[0], bb[0]);
#pragma unroll
        for (int kk = 0; kk < BKB / 32; ++kk) {
            if constexpr (SCHED == 5) piece(kk);
            if (kk + 1 < BKB / 32) read(kk + 1, a[(kk + 1) & 1], bb[(kk + 1) & 1]);
            if constexpr (SCHED == 2) __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    acc[mi][ni] = M::mma(a[kk & 1][mi], bb[kk & 1][ni], acc[mi][ni]);
            if constexpr (SCHED == 2) __builtin_amdgcn_s_setprio(0);
            if constexpr (SCHED == 1) {
                // pin the interleave: MFMA, LDS read, MFMA, ... (6 reads of
                // the next k-substep hidden under the 8 MFMAs of this one)
                if (kk + 1 < BKB / 32) {
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                }
            }
            if constexpr (SCHED == 5) {
                // MFMA, DMA piece, MFMA, LDS read, ... : 2 pieces + 6 reads in 8 MFMAs
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (kk + 1 < BKB / 32) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (kk + 1 < BKB / 32) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    }
                } else {
                    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                }
            }
            if constexpr (SCHED == 3) __builtin_amdgcn_iglp_opt(0);
            if constexpr (SCHED == 4) __builtin_amdgcn_iglp_opt(1);
        }
    };
    auto nopiece = [](int) {};

    const int nk = Kb / BKB;
    if constexpr (EPI == 4 || EPI == 5) {
        // diagnostic: stage once, then run the K loop on LDS only (4: with
        // the per-step barrier, 5: without) -- the in-core ceiling
        stageA(0, 0);
        stageB(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int t = 0; t < nk; ++t) {
            compute(0, 0, nopiece);
            if constexpr (EPI == 4) {
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
        }
    } else if constexpr (PIPE == 4) {
        // Phased, staggered pipeline.  Each K-step is 4 phases (one 32-byte
        // k-substep each); a phase is a LOAD segment (the next phase's 6
        // fragment ds_reads + this wave's share of the next stage's LDS-DMA)
        // and an MFMA segment (8 MFMAs at s_setprio 1), each closed by a raw
        // s_barrier.  Waves 4-7 run one barrier behind waves 0-3, so on every
        // SIMD one wave's MFMA segment overlaps its partner's load segment.
        // Stage t+1 is issued in phases 0-1 of step t (4 pieces each), retired
        // by a vmcnt(0) in phase 2's load segment and first read in phase 3's
        // (a barrier apart, for both wave groups); its buffer's previous
        // reads ended in phase 2 of step t-1.  No __syncthreads in the loop:
        // its fence would drain the DMA.
        v4i fa[2][4], fb[2][2];
        auto readf = [&](int buf, int kk, v4i (&ra)[4], v4i (&rb)[2]) {
            const unsigned char *As = abuf(buf);
            const unsigned char *Bs = bbuf(buf);
            const int c = kk * 2 + fh;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int r = wm * 128 + mi * 32 + fr;
                ra[mi] = *reinterpret_cast<const v4i *>(As + r * BKB + ((c ^ ((r >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int r = wn * 64 + ni * 32 + fr;
                rb[ni] = *reinterpret_cast<const v4i *>(Bs + r * BKB + ((c ^ ((r >> 1) & 7)) << 4));
            }
        };
        auto mma8 = [&](const v4i (&ra)[4], const v4i (&rb)[2]) {
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = M::mma(ra[mi], rb[ni], acc[mi][ni]);
            __builtin_amdgcn_s_setprio(0);
        };
        auto bar = [] {
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        };
        // prologue: stage 0, fragments of (0, 0), then the stagger
        stageA(0, 0);
        stageB(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        readf(0, 0, fa[0], fb[0]);
        if (wm == 1) bar();
        // one K-step; MORE = a next stage exists (the last step is peeled, so
        // the steady-state body is one basic block: hipcc's waitcnt pass then
        // keeps the next phase's ds_reads in flight over the MFMA segment)
        auto step = [&](int t, auto more_c) {
            constexpr bool MORE = decltype(more_c)::value;
            const int cur = t & 1;
            const int kn = (t + 1) * BKB;
            // phase 0 (fragment reads first, then the DMA pieces)
            readf(cur, 1, fa[1], fb[1]);
            if constexpr (MORE) {
                pieceA(cur ^ 1, kn, 0); pieceA(cur ^ 1, kn, 1);
                pieceB(cur ^ 1, kn, 0); pieceB(cur ^ 1, kn, 1);
            }
            bar();
            mma8(fa[0], fb[0]);
            bar();
            // phase 1
            readf(cur, 2, fa[0], fb[0]);
            if constexpr (MORE) {
                pieceA(cur ^ 1, kn, 2); pieceA(cur ^ 1, kn, 3);
                pieceB(cur ^ 1, kn, 2); pieceB(cur ^ 1, kn, 3);
            }
            bar();
            mma8(fa[1], fb[1]);
            bar();
            // phase 2: retire this wave's pieces of stage t+1 (vmcnt(0) only)
            if constexpr (MORE) __builtin_amdgcn_s_waitcnt(0x0F70);
            readf(cur, 3, fa[1], fb[1]);
            bar();
            mma8(fa[0], fb[0]);
            bar();
            // phase 3
            if constexpr (MORE) readf(cur ^ 1, 0, fa[0], fb[0]);
            bar();
            mma8(fa[1], fb[1]);
            bar();
        };
        for (int t = 0; t + 1 < nk; ++t) step(t, std::true_type{});
        step(nk - 1, std::false_type{});
        if (wm == 0) bar();  // re-align the barrier count of the two groups
        __syncthreads();
    } else if constexpr (PIPE >= 5) {
        // two-stage pipeline + L2 touch of stage t + D: per step each wave
        // issues its 8 pieces of stage t+1, then (if any) one touch, and
        // waits vmcnt(1) -- the pieces and the previous step's touch have
        // landed, this step's touch stays in flight across the raw barrier
        constexpr int D = PIPE == 6 ? 3 : 2;
        unsigned char *junk = lds + 2 * STAGE_BYTES;
        // PIPE 5/6: threads 0..255 touch A row tid, 256..511 B row tid-256;
        // PIPE 7: threads 0..255 touch B row tid, the other waves nothing
        const bool toucher = PIPE != 7 || tid < 256;
        const unsigned char *trow = (PIPE == 7 || tid >= 256) ? Bg + (size_t)(tid & 255) * Kb
                                                              : Ag + (size_t)tid * Kb;
        auto touch = [&](int k0) {
            __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)(trow + k0),
                                             (void __attribute__((address_space(3))) *)junk, 4, 0, 0);
        };
        stageA(0, 0);
        stageB(0, 0);
        if (toucher && 1 < nk) touch(BKB);  // stage 1 (its own DMA comes at step 0)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int t = 0; t < nk; ++t) {
            const int cur = t & 1;
            if (t + 1 < nk) {
                stageA(cur ^ 1, (t + 1) * BKB);
                stageB(cur ^ 1, (t + 1) * BKB);
            }
            const bool tch = toucher && t + D < nk;
            if (tch) touch((t + D) * BKB);
            compute(cur, cur, nopiece);
            if (tch) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        __syncthreads();
    } else if constexpr (PIPE >= 2) {
        // register-staged operands: step t+1's rows are loaded into VGPRs at
        // the top of step t (latency hidden by its MFMAs) and written to the
        // other LDS buffer (same swizzled image as the DMA path) at its end
        v4i rb[4], ra[4];
        auto gload = [&](const unsigned char *G, int k0, v4i (&r)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = (j * 8 + w) * 8 + srow_in;
                r[j] = *reinterpret_cast<const v4i *>(G + (size_t)row * Kb + k0 + sq * 16);
            }
        };
        auto lwrite = [&](unsigned char *L, const v4i (&r)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = (j * 8 + w) * 8 + srow_in;
                const int c = sq ^ ((row >> 1) & 7);
                *reinterpret_cast<v4i *>(L + row * BKB + c * 16) = r[j];
            }
        };
        if constexpr (PIPE == 2) stageA(0, 0);
        else gload(Ag, 0, ra);
        gload(Bg, 0, rb);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (PIPE == 3) lwrite(abuf(0), ra);
        lwrite(bbuf(0), rb);
        __syncthreads();
        for (int t = 0; t < nk; ++t) {
            const int cur = t & 1;
            const bool more = t + 1 < nk;
            if (more) {
                if constexpr (PIPE == 2) stageA(cur ^ 1, (t + 1) * BKB);
                else gload(Ag, (t + 1) * BKB, ra);
                gload(Bg, (t + 1) * BKB, rb);
            }
            compute(cur, cur, nopiece);
            if (more) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if constexpr (PIPE == 3) lwrite(abuf(cur ^ 1), ra);
                lwrite(bbuf(cur ^ 1), rb);
            }
            __syncthreads();
        }
    } else if constexpr (PIPE == 0) {
        // two-stage pipeline: stage t+1 streams in (LDS-DMA) while t is read
        stageA(0, 0);
        stageB(0, 0);
        if constexpr (!OVF_EARLY) seed_ovf();
        if constexpr (!OVF_EARLY && NWN != 6) load_mask();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        for (int t = 0; t < nk; ++t) {
            const int cur = t & 1;
            const bool more = t + 1 < nk;
            if constexpr (SCHED == 5) {
                compute(cur, cur, [&](int kk) {
                    if (more) {
                        pieceA(cur ^ 1, (t + 1) * BKB, kk);
                        pieceB(cur ^ 1, (t + 1) * BKB, kk);
                    }
                });
            } else {
                if (more) {
                    stageA(cur ^ 1, (t + 1) * BKB);
                    stageB(cur ^ 1, (t + 1) * BKB);
                }
                compute(cur, cur, nopiece);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    } else {
        // A one stage ahead, B two stages ahead.  Issue order per step is
        // A(t+1) then B(t+2), so vmcnt(4) (= B's 4 pieces per wave) leaves
        // exactly B(t+2) in flight across the barrier; a raw s_barrier (no
        // __syncthreads, whose fence would drain it) ends the step.
        stageA(0, 0);
        stageB(0, 0);
        if (nk > 1) stageB(1, BKB);
        if (nk > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        int b3 = 0;  // t % 3
        for (int t = 0; t < nk; ++t) {
            if (t + 1 < nk) stageA((t + 1) & 1, (t + 1) * BKB);
            if (t + 2 < nk) stageB(b3 == 0 ? 2 : b3 - 1, (t + 2) * BKB);  // (t+2) % 3
            compute(t & 1, b3, nopiece);
            if (t + 2 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            b3 = b3 == 2 ? 0 : b3 + 1;
        }
        __syncthreads();
    }

    if constexpr (EPI == 1 || (EPI >= 3 && EPI <= 5)) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
#if defined(__HIP_DEVICE_COMPILE__)
                asm volatile("" ::"v"(acc[mi][ni]));
#endif
            }
        return;
    }
    if constexpr (NWN == 6) {
        // the lane index afresh (volatile: not CSE'd with the prologue's), so
        // the old one dies in the loop
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        lane = l;
        fr = l & 31;
        fh = l >> 5;
    }
    if constexpr (FUSE) {
        // the fused fit, after the main loop: nothing of it is live across
        // the loop (held there, its registers pushed the loop's LDS-DMA
        // addresses into scratch: the launch ran 12-24% slower); the loads'
        // latency (~1 us of L2) is exposed once per workgroup
        fit_issue();
        fit_words();
    }
    // ---- epilogue: fit mask + per-pod candidate list
    // per lane: top-4 of its 64 (node, cost) values per pod; lanes l and l^32
    // (same pod, complementary rows) merge into a sorted 8-list whose bound is
    // the smaller of the two 4th keys (every key <= bound is in the list)
    u64 key[NI][8], bnd[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        u64 mwf[2];
        if constexpr (FUSE) {
#pragma unroll
            for (int mi2 = 0; mi2 < 2; ++mi2) mwf[mi2] = *fit_slot(ni, mi2);
        }
        const u64 *mw = FUSE ? mwf : mwp[ni];
        // orderable keys of the lane's 64 (node, cost) values and their range
        // (int8: the range of the raw int32 costs -- the key is x ^ 2^31, so
        // key differences are cost differences)
        unsigned u[4][16];
        unsigned kmin = 0xffffffffu, kmax = 0u;
        int smin = 0x7fffffff, smax = -0x7fffffff - 1;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                if constexpr (DT == NAS_DT_I8) {
                    smin = min(smin, (int)acc[mi][ni][reg]);
                    smax = max(smax, (int)acc[mi][ni][reg]);
                } else {
                    u[mi][reg] = M::okey(acc[mi][ni][reg]);
                    kmin = min(kmin, u[mi][reg]);
                    kmax = max(kmax, u[mi][reg]);
                }
            }
        if constexpr (DT == NAS_DT_I8) {
            kmin = M::okey(smin);
            kmax = M::okey(smax);
        }
        u64 k4[4];
        if (EPI == 0 && __all(kmax - kmin < (1u << 26) - 1u)) {
            // packed path (every lane's keys span < 2^26 - 1): one u32 per
            // value, (key - kmin) << 6 | i with i = mi*16 + reg increasing in
            // node order, so u32 order = (cost, node) order; a non-fitting
            // value is all-ones (never < a fitting one, < 2^32 - 1).  Sorted
            // insert of x into c0 <= .. <= c3: c3 = med3(c2, c3, x), c2 =
            // med3(c1, c2, x), c1 = med3(c0, c1, x), c0 = min(c0, x).
            unsigned c0 = 0xffffffffu, c1 = c0, c2 = c0, c3 = c0;
            // int8 with every lane's costs in [0, 2^26 - 1) (the common case:
            // non-negative traffic and latency): x = cost << 6 | i directly
            // (key base = okey(0)); otherwise relative to the lane's base
            // (int8: raw = cost bits, base = min cost; bf16: raw = key, base =
            // kmin).  Epilogue VALU per value 8 -> 5 (direct, every node of the
            // 32-node half fitting every lane's pod: one v_lshl_or_b32) / 7
            // (PMC: the epilogue is VALU-issue-bound, 1,377 instructions per
            // wave = ~10% of a C5 launch, profiles/r03_pmc_epilogue.txt)
            const bool direct = DT == NAS_DT_I8 && __all(smin >= 0 && smax < (1 << 26) - 1);
            const unsigned kbase = direct ? 0x80000000u : kmin;
            const unsigned nk6 = 0u - ((DT == NAS_DT_I8 ? (unsigned)smin : kmin) << 6);
            auto insert = [&](unsigned x) {
                c3 = umed3(c2, c3, x);
                c2 = umed3(c1, c2, x);
                c1 = umed3(c0, c1, x);
                c0 = min(c0, x);
            };
#pragma unroll
            for (int mi2 = 0; mi2 < 2; ++mi2)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int mi = mi2 * 2 + h;
                    const unsigned bitsw = (unsigned)(mw[mi2] >> (32 * h));
                    const unsigned nbits = ~bitsw;
                    if (direct && __all(bitsw == 0xffffffffu)) {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg)
                            insert(((unsigned)(int)acc[mi][ni][reg] << 6) | (unsigned)(mi * 16 + reg));
                    } else {
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) {
                            const int row = (reg & 3) + 8 * (reg >> 2) + 4 * fh;
                            const unsigned raw = DT == NAS_DT_I8 ? (unsigned)(int)acc[mi][ni][reg]
                                                                 : u[mi][reg];
                            // (raw << 6) - (base << 6) in one v_lshl_add (hipcc
                            // otherwise emits a subtract and a shift); slot and
                            // the sign-extended not-fit bit (v_bfe_i32) OR'ed in
                            unsigned y;
                            if (direct) {
                                y = raw << 6;
                            } else {
                                asm("v_lshl_add_u32 %0, %1, 6, %2" : "=v"(y) : "v"(raw), "v"(nk6));
                            }
                            insert(y | (unsigned)(mi * 16 + reg) |
                                   (unsigned)__builtin_amdgcn_sbfe((int)nbits, row, 1));
                        }
                    }
                }
            const unsigned cc[4] = {c0, c1, c2, c3};
            const unsigned nb = (unsigned)(node_base + mt * BM + wm * 128 + 4 * fh);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned i = cc[j] & 63u, r = i & 15u;
                const unsigned node = nb + (i >> 4) * 32u + (r & 3u) + 8u * (r >> 2);
                k4[j] = cc[j] == 0xffffffffu ? KEY_INVALID
                                             : ((u64)((cc[j] >> 6) + kbase) << 32) | node;
            }
        } else {
            Top4 t4;
            t4.init();
            unsigned best1 = 0xffffffffu, bnode1 = 0xffffffffu;
#pragma unroll
            for (int mi2 = 0; mi2 < 2; ++mi2) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int mi = mi2 * 2 + h;
                    const unsigned bits = (unsigned)(mw[mi2] >> (32 * h));
                    const unsigned node0 = (unsigned)(node_base + mt * BM + wm * 128 + mi * 32);
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * fh;
                        // not fitting -> cost all-ones, never inserted (branch-free)
                        const unsigned key = DT == NAS_DT_I8 ? M::okey(acc[mi][ni][reg]) : u[mi][reg];
                        const unsigned x = key | ((((bits >> row) & 1u) ^ 1u) * 0xffffffffu);
                        if constexpr (EPI == 2) {
                            const bool b = x < best1;
                            best1 = b ? x : best1;
                            bnode1 = b ? node0 + row : bnode1;
                        } else {
                            t4.insert(x, node0 + row);
                        }
                    }
                }
            }
            if constexpr (EPI == 2) t4.c[0] = best1, t4.n[0] = bnode1;
#pragma unroll
            for (int j = 0; j < 4; ++j) k4[j] = t4.c[j] == 0xffffffffu ? KEY_INVALID : t4.key(j);
        }
        u64 o4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o4[j] = shfl_xor64(k4[j], 32);
        merge44(k4, o4, key[ni]);
        bnd[ni] = umin64(k4[3], o4[3]);
    }

    // merge the two node-half waves (wm = 0, 1) through LDS
    u64 *xk = reinterpret_cast<u64 *>(lds);  // [wn][ni][32][9], staging is dead
    if (wm == 1 && fh == 0) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            u64 *d = xk + ((wn * NI + ni) * 32 + fr) * 9;
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = key[ni][j];
            d[8] = bnd[ni];
        }
    }
    __syncthreads();
    if (wm == 0) {
        // round rr: lane < 32 -> pods wn*WPODS + 64rr + 0..31 (ni = 2rr), lane >=
        // 32 -> +32..63 (ni = 2rr + 1); constant-index branches, not key[fh][j]
        // (a runtime index puts the lists in scratch)
        auto finish = [&](u64 (&mine)[8], u64 b, int ni, int rr) {
            u64 other[8];
            const u64 *s = xk + ((wn * NI + ni) * 32 + fr) * 9;
#pragma unroll
            for (int j = 0; j < 8; ++j) other[j] = s[j];
            merge88(mine, other);
            b = umin64(umin64(b, s[8]), mine[7]);
            const int pod = p0 + nt * BNK + wn * WPODS + rr * 64 + lane;
            if (pod >= p_end) return;
            store8(partial + ((size_t)mt * Pp + pod) * KC, mine);
            pbound[(size_t)mt * Pp + pod] = b;
        };
#pragma unroll
        for (int rr = 0; rr < NI / 2; ++rr) {
            if (fh == 0) finish(key[2 * rr], bnd[2 * rr], 2 * rr, rr);
            else finish(key[2 * rr + 1], bnd[2 * rr + 1], 2 * rr + 1, rr);
        }
    }
}

// merge n_lists candidate lists per pod (list l of pod p at
// keys[l * stride + (p - src_p0) * KC], bound[l * bstride + p - src_p0]).
// MERGE_LANES lanes per pod: lane s folds lists s, s + MERGE_LANES, ... in
// registers, then three xor-shuffle rounds merge the lanes' lists.  The 8
// smallest keys of the union do not depend on the merge tree, and neither
// does the bound: every intermediate kept[7] is >= the final kept[7], so the
// result is min(all list bounds, final kept[7]) -- identical to a serial fold.
constexpr int MERGE_LANES = 8;
constexpr int MERGE_SRC_WINDOW = 1, MERGE_DST_WINDOW = 2;  // dyn_flags (k_cost.hip)
// 64 pods per workgroup (2 waves per SIMD at 56 VGPRs): still co-resides
// with a 256 x 256 cost workgroup (2 waves per SIMD at 192 VGPRs) on a node
// shard; 1,024-thread blocks do not, and measured 7% slower at G = 8 (the
// wide tile admits nothing beside it either way: C3 within noise for 256 /
// 512 / 1,024, profiles/r03_ab_merge_block.txt)
#ifndef MERGE_BLOCK
#define MERGE_BLOCK 512
#endif

__global__ void __launch_bounds__(MERGE_BLOCK)
k_merge(const u64 *__restrict__ keys, const u64 *__restrict__ bounds, int n_lists,
        long long stride, long long bstride, int src_p0, int p0, int np,
        u64 *__restrict__ dst, u64 *__restrict__ dst_bound, int dst_p0,
        const int *__restrict__ dyn_start, int dyn_hi, int dyn_flags, long long dst_cs,
        const int *__restrict__ dyn_hi_ptr, const int *__restrict__ dst_idx) {
    const int cb = blockIdx.y;  // cluster of a batched launch (dst_cs pods apart)
    keys += (size_t)cb * n_lists * stride;
    bounds += (size_t)cb * n_lists * bstride;
    dst += (size_t)cb * dst_cs * KC;
    dst_bound += (size_t)cb * dst_cs;
    if (dyn_start) {  // rescore slot: pods [s, min(s + np, hi)); source / destination
        const int s = dyn_start[cb * STATUS_INTS];  // indexed from s when flagged (staging)
        if (s < 0) return;
        if (dyn_hi_ptr) dyn_hi = dyn_hi_ptr[cb * STATUS_INTS];
        p0 = s;
        np = min(np, dyn_hi - s);
        if (dyn_flags & MERGE_SRC_WINDOW) src_p0 = s;
        if (dyn_flags & MERGE_DST_WINDOW) dst_p0 = s;
    }
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = t / MERGE_LANES, s = t % MERGE_LANES;
    const bool live = i < np;  // the whole 8-lane group shares i: shuffles stay in-group
    const size_t ps = (size_t)(p0 + (live ? i : 0) - src_p0);
    u64 a[8], bb[8];
    u64 bound = KEY_INVALID;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = KEY_INVALID;
    if (live) {
        for (int l = s; l < n_lists; l += MERGE_LANES) {
            load8(keys + l * stride + ps * KC, bb);
            merge88(a, bb);
            bound = umin64(bound, bounds[l * bstride + ps]);
        }
    }
#pragma unroll
    for (int m = 1; m < MERGE_LANES; m <<= 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bb[j] = shfl_xor64(a[j], m);
        bound = umin64(bound, shfl_xor64(bound, m));
        merge88(a, bb);
    }
    if (!live || s != 0) return;
    // dst_idx (gathered rescore view, one cluster): row r's lists go straight
    // back to pod dst_idx[r]'s slots -- the scatter fused into the store
    const int r = p0 + i - dst_p0;
    const int p = dst_idx ? dst_idx[r] : r;
    store8(dst + (size_t)p * KC, a);
    dst_bound[p] = umin64(bound, a[7]);
}

#ifdef NAS_DIAG_VARIANTS
#define NAS_INST(E, S, PP, G)                                                                      \
    template __global__ void k_cost_topk<NAS_DT_I8, E, S, PP, G>(                                  \
        const unsigned char *, const unsigned char *, int, int, int, int, int, const u64 *, u64 *,  \
        u64 *, int, const int *, int, const int *, Ovf, const int *, FitSrc);
NAS_INST(0, 0, 0, 4) NAS_INST(1, 0, 0, 4) NAS_INST(0, 5, 0, 4) NAS_INST(1, 5, 0, 4)
NAS_INST(3, 5, 0, 4) NAS_INST(0, 1, 0, 4) NAS_INST(0, 5, 0, 8) NAS_INST(4, 0, 0, 4)
NAS_INST(0, 1, 2, 4) NAS_INST(0, 1, 3, 4) NAS_INST(0, 0, 2, 4) NAS_INST(0, 0, 3, 4)
NAS_INST(1, 1, 2, 4) NAS_INST(1, 1, 3, 4)
NAS_INST(0, 0, 4, 4) NAS_INST(1, 0, 4, 4) NAS_INST(0, 0, 4, 8) NAS_INST(0, 0, 4, 2)
NAS_INST(0, 0, 0, -2) NAS_INST(0, 0, 0, -4) NAS_INST(0, 0, 0, -8) NAS_INST(0, 0, 0, 8)
NAS_INST(0, 0, 0, 2) NAS_INST(0, 0, 0, 16)
#undef NAS_INST

#endif

template <int DT, bool RMAP, int NWN = cost_nwn<DT>(), bool FUSE = (NWN == 6)>
hipError_t launch_cost_t(hipStream_t st, const void *Lt, const void *WA, int Mp, int Kb, int Pp,
                         int p0, int np, const uint64_t *mask, uint64_t *partial,
                         uint64_t *pbound, int node_base, const Dyn *dyn, int batch,
                         const Ovf &ov, const int32_t *rowmap, const FitSrc &fs = FitSrc{}) {
    constexpr int BNK = NWN * (NWN == 2 ? 128 : 64);
    const void *fn = reinterpret_cast<const void *>(
        &k_cost_topk<DT, 0, COST_SCHED, COST_PIPE, NWN == 6 ? COST_GM_WIDE : COST_GM, RMAP, NWN, FUSE>);
    const int lds = NWN == 6 ? 2 * (BM + BNK) * BKB : lds_bytes<COST_PIPE>();
    static std::atomic<unsigned long long> attr_set{0};
    hipError_t e = set_lds_once(fn, lds, attr_set);
    if (e != hipSuccess) return e;
    const int n_mt = Mp / BM, n_nt = (np + BNK - 1) / BNK;
    // the wide tile's last pod tile reads up to WA_PAD_ROWS rows past the
    // launch; past the last cluster's Pp rows only the padding is allocated
    if (NWN == 6 && (int64_t)p0 + (int64_t)n_nt * BNK > (int64_t)Pp + WA_PAD_ROWS)
        return hipErrorInvalidValue;
    // the fused fit (the wide tile always): capacity and requests
    if (FUSE && (!fs.cap || !fs.req || fs.nloc > Mp || fs.n0 + fs.nloc > fs.N || dyn))
        return hipErrorInvalidValue;
    auto *lt = static_cast<const unsigned char *>(Lt);
    auto *wa = static_cast<const unsigned char *>(WA);
    auto *mk = reinterpret_cast<const u64 *>(mask);
    auto *pa = reinterpret_cast<u64 *>(partial);
    auto *pb = reinterpret_cast<u64 *>(pbound);
    const int *ds = dyn ? dyn->start : nullptr;
    const int dh = dyn ? dyn->hi : 0;
    const int *dhp = dyn ? dyn->hi_ptr : nullptr;
    // the wide tile's launch end rides in dyn_hi (unused without a window)
    const int dhi = NWN == 6 ? p0 + np : dh;
    k_cost_topk<DT, 0, COST_SCHED, COST_PIPE, NWN == 6 ? COST_GM_WIDE : COST_GM, RMAP, NWN, FUSE><<<dim3(n_mt * n_nt, batch), 128 * NWN, lds, st>>>(
        lt, wa, Kb, n_mt, n_nt, p0, Pp, mk, pa, pb, node_base, ds, dhi, dhp, ov, rowmap, fs);
    return hipGetLastError();
}

}  // namespace

int cost_tile_pods(int dtype) {
    const bool wide = dtype == NAS_DT_I8 ? cost_wide<NAS_DT_I8>() : cost_wide<NAS_DT_BF16>();
    return wide ? 384 : BN;
}

// Kp: padded contraction length in ELEMENTS; np: pods, multiple of BN,
// p0 + np <= Pp; Mp multiple of BM.
hipError_t launch_cost_topk(hipStream_t st, int dtype, const void *Lt, const void *WA, int Mp,
                            int Kp, int Pp, int p0, int np, const uint64_t *mask,
                            uint64_t *partial, uint64_t *pbound, int node_base, const Dyn *dyn,
                            int batch, const Ovf *ovf, const int32_t *rowmap, bool wide,
                            const FitSrc *fit) {
    if (fit && (dyn || rowmap)) return hipErrorInvalidValue;  // windows keep the k_fit mask
    if (!fit && wide && !dyn && !rowmap) return hipErrorInvalidValue;  // the wide tile fuses
    const Ovf ov = ovf ? *ovf : Ovf{};
    if (rowmap && (!dyn || batch != 1)) return hipErrorInvalidValue;
#define NAS_COST_DISPATCH(DTV, KB, OVV)                                                            \
    (rowmap ? launch_cost_t<DTV, true>(st, Lt, WA, Mp, KB, Pp, p0, np, mask, partial, pbound,     \
                                       node_base, dyn, batch, OVV, rowmap)                        \
     : (!dyn && wide && cost_wide<DTV>())                                                                 \
            ? launch_cost_t<DTV, false, 6>(st, Lt, WA, Mp, KB, Pp, p0, np, mask, partial, pbound, \
                                           node_base, dyn, batch, OVV, nullptr, *fit)             \
     : fit ? launch_cost_t<DTV, false, cost_nwn<DTV>(), true>(st, Lt, WA, Mp, KB, Pp, p0, np,     \
                                                             mask, partial, pbound, node_base,    \
                                                             dyn, batch, OVV, nullptr, *fit)      \
            : launch_cost_t<DTV, false>(st, Lt, WA, Mp, KB, Pp, p0, np, mask, partial, pbound,    \
                                        node_base, dyn, batch, OVV, nullptr))
    if (dyn) {  // tiles covering any window [s, s + win) clipped to hi: one extra for the offset
        p0 = 0;
        np = (int)round_up(dyn->win, BN) + BN;
        if (!dyn->hi_ptr && dyn->hi > Pp) return hipErrorInvalidValue;
    }
    if (np <= 0) return hipSuccess;
    if (Mp % BM || np % BN || (!dyn && p0 + np > Pp)) return hipErrorInvalidValue;
    if (dtype == NAS_DT_I8) {
        if (Kp % BKB) return hipErrorInvalidValue;
        return NAS_COST_DISPATCH(NAS_DT_I8, Kp, ov);
    }
    // (NAS_DT_F32 operands arrive here as their bf16 six-segment splits,
    // dtype NAS_DT_BF16: nas_api.hip launch_cost)
    if (dtype != NAS_DT_BF16) return hipErrorInvalidValue;
    if ((2 * Kp) % BKB) return hipErrorInvalidValue;
    return NAS_COST_DISPATCH(NAS_DT_BF16, 2 * Kp, Ovf{});
#undef NAS_COST_DISPATCH
}

hipError_t launch_merge(hipStream_t st, const uint64_t *keys, const uint64_t *bounds, int n_lists,
                        int64_t stride, int64_t bstride, int src_p0, int p0, int np,
                        uint64_t *cand_key, uint64_t *cand_bound, int dst_p0, const Dyn *dyn,
                        int dyn_flags, int batch, int64_t dst_cluster_pods,
                        const int32_t *dst_idx) {
    if (dyn) np = dyn->win;
    if (np <= 0) return hipSuccess;
    if (dst_idx && batch != 1) return hipErrorInvalidValue;
    k_merge<<<dim3((int)(((int64_t)np * MERGE_LANES + MERGE_BLOCK - 1) / MERGE_BLOCK), batch),
              MERGE_BLOCK, 0, st>>>(
        reinterpret_cast<const u64 *>(keys), reinterpret_cast<const u64 *>(bounds), n_lists, stride,
        bstride, src_p0, p0, np, reinterpret_cast<u64 *>(cand_key),
        reinterpret_cast<u64 *>(cand_bound), dst_p0, dyn ? dyn->start : nullptr, dyn ? dyn->hi : 0,
        dyn_flags, (long long)dst_cluster_pods, dyn ? dyn->hi_ptr : nullptr, dst_idx);
    return hipGetLastError();
}

}  // namespace nas
