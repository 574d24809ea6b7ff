// pass_plan.h -- how a placement pass (nas_place, nas_api.hip) is laid out,
// as plain host arithmetic: the scoring chunks, the slot / cache / herd
// constants and the mode flags that decide which streams carry what and how
// many collectives every rank of a node-sharded pass issues.  No HIP runtime
// call and no context: everything here is a function of a PassShape and
// explicit inputs, so it runs (and is tested: tests/sanitize/pass_plan_driver.cpp)
// without a GPU.  DESIGN.md, "Pass planning".
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <utility>
#include <vector>

#include "nas_internal.h"

namespace nas {

constexpr int RESCORE_PODS = 1024;  // pods per device-side rescore slot (multiple of COST_BN)
// dry pods rescored per gathered slot (gathered_slot).  1024, not 4096: a
// bf16 C3 halt (the last chunk's lists, scored against capacity two chunks
// stale, run dry in a herd) flags > 4096 pods with STALE_MIN_FIT 2, but the
// first 1024 of them always let the walk finish -- the slot's cost launch
// 690 -> 235 us, the halting pass's slots 0.9 -> 0.37 ms (traced); 256 / 512
// need more slots (profiles/r04_ab_gather_pods.txt)
// (round 6: 6 tiles = 1,536 pods for C3 -- still one wave of cost workgroups
// over 40 node tiles -- took 65 instead of 89 slots through the full-range
// herd but 31.6 instead of 29.4 ms, same box: profiles/r06b_ab_slots.txt)
constexpr int GATHER_PODS = 1024;
// a pass with the cost-row cache rescores from cached rows (k_rescore_cached:
// no cost launch), so its slots take more pods
constexpr int GATHER_PODS_CACHED = 2048;
// NAS_OPT_COST_CACHE auto: the previous pass's rescore rounds that turn the
// cache on, and its largest size (C4 at world 1 would need 100 GB)
constexpr int CACHE_MIN_ROUNDS = 4;
constexpr size_t CACHE_MAX_BYTES = (size_t)16 << 30;
// NAS_OPT_HERD_PLAN auto: rescore rounds of one pass that make its shape a herd
constexpr int HERD_MIN_ROUNDS = 8;
// gathered slots behind each chunk's commit in the herd plan
constexpr int HERD_SLOTS = 1;
// ... of at most this many pods (they run on the CUs a chunk's wave leaves
// free, C3: 16, where a 2,048-pod rescore takes ~190 us; 512-pod slots
// measured no faster and less stable: profiles/r06e_ab_herd.txt)
constexpr int HERD_SLOT_PODS = 2048;
constexpr int GATHER_SLOTS_PER_SYNC = 4;  // gathered slots enqueued per host check of the halt word
constexpr int MAX_SPEC_SLOTS = 8;         // speculative slots at most (nas_place, slot_hint)
// ... except the second check: a walk still halted after a full batch is
// usually nearly done (C2: 5 slots), and an idle slot's ~8 launches cost about
// what one more host round trip does, so the second batch is one slot (C2
// median 1.17 / 1.07 / 1.04 ms with a second batch of 4 / 2 / 1, same
// placements).  With the cost-row cache (a herd; an idle slot is 3 launches)
// 8 slots per check from the fourth on
inline int gather_batch(int check, bool cached) {
    return check == 2 ? 1 : (cached && check > 3) ? 8 : GATHER_SLOTS_PER_SYNC;
}
// (a one-slot FIRST batch for walks halting near their end helped a 12-pod
// rescore, 0.39 -> 0.26 ms, but cost bench C1's 3-slot case two extra round
// trips, 0.39 -> 0.52 ms: with a round trip ~2 idle slots, 4 then 1 is the
// robust order)
// pinned staging of nas_place results in host_status: behind the status words
// of every cluster of a batch (B * STATUS_INTS ints; nas_set_batch allows up to
// 65535 clusters), page-aligned
inline size_t host_out_offset(int B) {
    const size_t status_bytes = (size_t)std::max(B, 1) * (STATUS_INTS + 4) * 4;
    return std::max<size_t>(4096, (status_bytes + 4095) & ~(size_t)4095);
}
// Rescore slots run only for a walk known to have halted (after the
// pipeline): an idle gathered slot still costs ~0.1 ms of launches (C3,
// measured), more than the host round trip a stop costs once the pipeline is
// done -- the results fetch brings the halt word back with the placements --
// and scoring against the live capacity makes stops rare.

// What the planning may read of a pass.  No rank-local field (Nloc, Nloc0,
// Mp, rank): ranks of a communicator hold the same values of all of these, so
// whatever is computed from a PassShape alone is the same on every rank --
// every rank must plan the same chunks, or their per-chunk all-gathers
// mismatch.
struct PassShape {
    int P, Pp;      // pods of one cluster, padded
    int N;          // nodes of the whole cluster
    int B;          // clusters of a batch
    int world;      // ranks sharing the nodes
    int rehearse;   // NAS_OPT_REHEARSE_WORLD
    int n_cu;       // compute units of the device
    int wide_pods;  // pods of the wide cost tile (nas::cost_tile_pods)
};

// The wide cost tile (256 nodes x 384 pods, 12 waves) for the main scoring
// pass of one whole cluster with many pods (full launch 3.5% (int8) / 6%
// (bf16) faster than 256 x 256: profiles/r02_s4_ab_wide*.txt), for batches of
// clusters (C5: launch frac 0.42 -> 0.45 although a 5,000-pod cluster is
// 13.02 wide tiles, profiles/r04_ab_narrow_fit_wide.txt) and for node shards,
// there together with CU-masked streams (nas_api.hip, RESERVE_SHARD_CUS; the
// wide tile alone lost on shards in round 2: longer workgroups, coarser
// tails).  Small clusters, rescore windows and row-mapped views keep 256 x 256.
constexpr int WIDE_MIN_PODS = 32768;
inline bool wide_ok(const PassShape &sh) {
    const bool shard = sh.world > 1 || sh.rehearse > 1;
    if (sh.B > 1) return !shard;
    return sh.Pp >= WIDE_MIN_PODS || shard;
}
inline int tile_pods(const PassShape &sh) { return wide_ok(sh) ? sh.wide_pods : COST_BN; }

// pods per pipelined scoring chunk starting at pod lo: at least 32 pod
// tiles, and enough tiles that one chunk's cost launch has ~512 workgroups on
// this rank's node tiles (node shards have few node tiles).  The first chunk
// is 32 tiles, so the commit stream starts early, and the last is at most
// about 32, so the commit left after the scoring ends (the serial tail, which
// matters most on a node shard's short scoring) is short.
constexpr int CHUNK_WORKGROUPS = 512;  // cost workgroups per big chunk (measured best)
// a node shard's chunks after the first, on shards of up to
// SHARD_CHUNKS_MAX_MT node tiles (C3 from G = 4 on)
constexpr int SHARD_CHUNKS = 6;
constexpr int SHARD_CHUNKS_MAX_MT = 10;
// 256-pod units per chunk on the wide tile: 32 tiles of 384 (1,280 workgroups
// at 40 node tiles, as the 256-pod form's 32-unit chunks); 24 / 33 units
// measured 0.5-2% slower (profiles/r02_s4_ab_chunk.txt)
constexpr int CHUNK_TILES_WIDE = 48;
// node tiles per rank for chunk planning: the LARGEST shard's, the same on
// every rank (rank shards differ by up to one node, so their own Mp can
// differ by a tile, e.g. 2,049 nodes over 8 ranks: 256 vs 257 nodes); every
// rank must plan the same chunks, or their per-chunk all-gathers mismatch
inline int plan_n_mt(const PassShape &sh) {
    const int64_t widest = ((int64_t)sh.N + sh.world - 1) / sh.world;
    return (int)(round_up(std::max<int64_t>(widest, 1), COST_BM) / COST_BM);
}

inline int chunk_pods(const PassShape &sh, int c, int lo) {
    const int wgs = CHUNK_WORKGROUPS;
    const int n_mt = plan_n_mt(sh);
    const int big = std::max(32, (wgs + n_mt - 1) / n_mt);
    // 32-tile chunks (whole waves of workgroups at 8+ node tiles) with a
    // short last one; when the workgroup target sets the size (a node shard
    // with few node tiles), equal chunks: on rank 0 of a G = 8 rehearsal
    // 1.45 ms vs 1.56 ms per C3 pass, while at G = 1 the 32-tile form is
    // 2.5% ahead (8.15 vs 8.37 ms)
    const int mode = big > 32 ? 2 : 0;
    const int left = (sh.P - lo + COST_BN - 1) / COST_BN;  // pod tiles left
    int tiles = c == 0 ? 32 : big;
    // (one cluster, G = 1) the wide tile's chunks: the first chunk of the
    // second scoring stream is half as long, so the two streams' chunk
    // boundaries stay half a chunk apart -- a stream's next chunk waits for
    // its previous one to complete, and while that drains its last round the
    // other stream still has undispatched workgroups to fill the CUs (with
    // equal chunks both streams drained together: ~20 us of idle CUs per
    // chunk pair in the C3 pass timeline)
    if (tile_pods(sh) != COST_BN && sh.world == 1)
        tiles = c == 1 ? CHUNK_TILES_WIDE / 2 : CHUNK_TILES_WIDE;
    // a pass whose pods fit one big chunk (C2: 40 pod tiles on 4 node tiles)
    // is one chunk: pipelining its short tail would save less than the
    // cross-stream hops and launches it adds (device time 0.96 -> 0.92 ms, C2)
    if (c == 0 && left <= big) tiles = left;
    if (mode == 0) {
        // a big last chunk is split in two so that the last is 32 tiles (unless
        // the first part would be a sliver of under 16)
        if (c > 0 && left > 32 && left <= big && left - 32 >= 16) tiles = left - 32;
    } else if (mode == 2 && c > 0) {
        // the rest in equal chunks: SHARD_CHUNKS of them (counting from
        // chunk 1; fewer when a chunk would drop below 32 units) on shards of
        // up to SHARD_CHUNKS_MAX_MT node tiles, else of at most `big` tiles
        // (~512 workgroups).  Six measured best on the C3 rehearsal: G = 8
        // 1.213 vs 1.227 ms, G = 4 2.105 vs 2.174 ms, but G = 3 (14 node
        // tiles, 560-workgroup chunks) 2.850 vs 2.812 ms; three to seven
        // swept (profiles/r05ab_ab_shard_chunks.txt).  (A short last chunk of
        // 16 / 32 tiles, to shorten the commit left after the scoring,
        // measured 7-13% slower at G = 8 and 2-3% at G = 4: one more chunk
        // costs more cross-stream hops than its shorter commit saves)
        //  the six-way split is capped at 2 x `big` tiles per chunk
        // (~1,024 workgroups), so a much larger P keeps chunks -- and the
        // serial merge / exchange / commit of the tail chunk after the
        // scoring -- bounded instead of growing linearly with P; C3's plans
        // are unchanged (G = 4: 60-tile chunks under a 104-tile cap, G = 8:
        // 60 under 206)
        const int n = n_mt <= SHARD_CHUNKS_MAX_MT
                          ? std::max({1, std::min(SHARD_CHUNKS - c + 1, left / 32),
                                      (left + 2 * big - 1) / (2 * big)})
                          : (left + big - 1) / big;
        tiles = (left + n - 1) / n;
    }  // (decreasing chunk sizes n, n-1, ..., 1 measured 7-10% slower at G = 4 / 8)
    // whole cost tiles per chunk: the wide tile (384 pods) needs multiples of
    // 3 units, or a chunk's last tile would score pods of the next chunk
    const int unit = tile_pods(sh) / std::gcd(tile_pods(sh), COST_BN);
    tiles = std::min(left, (tiles + unit - 1) / unit * unit);
    return tiles * COST_BN;
}

// The pass's scoring chunks [lo, hi) in pod order; chunk c runs on scoring
// stream c & 1.  On the wide tile (one cluster, G = 1) the two streams'
// totals are balanced at the end: the remainder after the 48-unit chunks is
// split over one last chunk per stream, sized so that both streams carry the
// same number of units and finish together (with the last chunks alternating
// as before, the stream that drew the first full chunk carried ~37 more wide
// tiles of 261 at C3, and ran alone -- one partial wave of idle CUs per
// chunk -- for the last ~1.4 ms of the scoring: profiles/r03_pass_timeline_c3_*.txt,
// r03_ab_balance_ksweep.txt)
// Node shards keep equal chunks (chunk_pods mode 2): the balanced plan put
// two chunk chains in the pass's tail and measured 4-8% slower at G = 8 and
// 1% at G = 4 (profiles/r03_ab_chunk_plan_shard.txt).  Putting the half-length
// chunk first (chunks then finish in pod order) measured the same or 0.5%
// slower, and so did moving units from a stream's short last chunk to its
// previous one (r03_ab_chunk_order.txt).
inline std::vector<std::pair<int, int>> plan_chunks(const PassShape &sh, bool herd = false) {
    std::vector<std::pair<int, int>> chunks;
    const int P = sh.P;
    const bool wide = tile_pods(sh) != COST_BN && sh.world == 1;
    if (herd) {
        // the herd plan's chunks (nas_place): ONE wave of cost workgroups
        // each -- as many pod tiles as the CUs hold beside this rank's node
        // tiles (C3: 6 wide tiles = 2,304 pods over 40 node tiles = 240
        // workgroups), so the commit stream keeps the CUs left over -- and at
        // most ~1.25 pods per node (a chunk's own pods compete for the nodes
        // its fit saw free; tools/herd_model.py: 0 slots at 3,072 pods per
        // chunk, 5 at 6,144, 18 at 12,288 for 36,864 pods over 10k nodes)
        const int tp = tile_pods(sh);
        int tiles = std::min(sh.n_cu / std::max(plan_n_mt(sh), 1),
                             std::max(1, (int)((5LL * sh.N / 4) / tp)));
        if (tp != COST_BN) tiles = std::max(2, tiles / 2 * 2);  // whole 256-pod units
        tiles = std::max(tiles, 1);
        const int step = tiles * tp;
        for (int lo = 0; lo < P; lo += step) chunks.push_back({lo, std::min(P, lo + step)});
        return chunks;
    }
    if (!wide) {
        for (int c = 0, lo = 0; lo < P; ++c) {
            const int hi = std::min(P, lo + chunk_pods(sh, c, lo));
            chunks.push_back({lo, hi});
            lo = hi;
        }
        return chunks;
    }
    const int unit = tile_pods(sh) / std::gcd(tile_pods(sh), COST_BN);  // wide: 3 (256-pod units)
    const int total = (P + COST_BN - 1) / COST_BN;                    // 256-pod units
    std::vector<int> sizes;
    int load[2] = {0, 0}, left = total;
    auto take = [&](int u) {
        u = std::min(left, (u + unit - 1) / unit * unit);
        sizes.push_back(u);
        load[(sizes.size() - 1) & 1] += u;
        left -= u;
    };
    // 48-unit chunks, the second stream's first one half as long
    const int big = CHUNK_TILES_WIDE;
    if (left <= big) {
        take(left);
    } else {
        take(big);
        take(big / 2);
        while (left > 0) {
            // can the rest end as one chunk on the next stream s and one on
            // the other, both at most `big`, with equal stream totals?
            const int s = sizes.size() & 1;
            const int x = std::max(0, (left + load[s ^ 1] - load[s]) / 2) / unit * unit;
            if (x >= unit && x <= big && left - x <= big) {
                take(x);
                if (left > 0) take(left);
                break;
            }
            if (x < unit && left <= big) {  // stream s is ahead: one last chunk
                take(left);
                break;
            }
            take(big);
        }
    }
    for (int lo = 0, i = 0; i < (int)sizes.size(); ++i) {
        const int hi = std::min(P, lo + sizes[i] * COST_BN);
        chunks.push_back({lo, hi});
        lo = hi;
    }
    return chunks;
}

// ---- the pass's mode: what nas_place decides before its first enqueue

// everything the mode reads besides the shape
struct PassInputs {
    // options (nas_set_option)
    int32_t opt_herd_plan, opt_cost_cache;
    int64_t opt_inject_stall_ms, opt_commit_wait_ms, opt_comm_timeout_ms;
    PassHistory hist;  // what earlier passes left (note_pass)
    // the call issues collectives other ranks must join / exchanges lists with
    // them (exchanging implies has_coll)
    bool has_coll, exchanging;
    bool constrained;  // node selectors / taints are uploaded
    bool live_cap;     // commit_in_lds(N): scoring reads the working capacity
    // the cost-row cache's size, Pp * Mp * 4: the ONE rank-local input (Mp is
    // this rank's node tiles, and shards can differ by one); it only gates
    // want_cache against CACHE_MAX_BYTES (DESIGN.md §10 on what follows when
    // ranks end up with different caches)
    size_t cache_bytes;
};

struct PassPlan {
    bool herd;        // the herd plan (below), not the pipelined one
    bool want_cache;  // the pass runs with the cost-row cache if it can be allocated
    // chunk bounds; every scoring launch is enqueued before any commit-stream
    // work, so the host's enqueue time of merges / commits / copies never
    // delays the next chunk's cost launch
    std::vector<std::pair<int, int>> chunks;
    bool one_stream;
    int spec;
    bool late_slots, status_in_commit, xs_mode, init_in_merge;
    int64_t commit_wait_ms;
};

inline PassPlan plan_pass(const PassShape &sh, const PassInputs &in) {
    PassPlan p;
    const PassHistory &h = in.hist;
    const bool hinted = h.slot_hint_P == sh.P && h.slot_hint_N == sh.N;
    // (the herd plan, auto: sticky for a shape once one of its passes
    // needed HERD_MIN_ROUNDS rescore rounds; it turns the cache on too)
    p.herd = !in.has_coll && (in.opt_herd_plan == 1 ||
                              (in.opt_herd_plan == 2 && h.herd_P == sh.P && h.herd_N == sh.N));
    // The cost-row cache (NAS_OPT_COST_CACHE, k_rescore_cached): in auto mode
    // when the previous pass of this shape needed CACHE_MIN_ROUNDS rescore
    // rounds or more (a herd: consecutive passes over similar clusters stop
    // alike, as the speculative slots below assume too).  It costs the main
    // cost launches a 4-byte store per (pod, node) and saves every gathered
    // slot its fit / cost / merge launches.  Same placements either way.
    // (not with node selectors / taints: k_rescore_cached rebuilds lists from
    // cached rows against capacity alone.  The constraints are replicated, so
    // every rank of a communicator decides alike; the slots recompute through
    // the constrained k_fit, whatever NAS_OPT_COST_CACHE says)
    p.want_cache = false;
    if (in.opt_cost_cache != 0 && !in.constrained) {
        const bool herd = hinted && h.last_rescore_rounds >= CACHE_MIN_ROUNDS;
        p.want_cache = (in.opt_cost_cache == 1 || herd || p.herd) && in.cache_bytes <= CACHE_MAX_BYTES;
    }
    p.chunks = plan_chunks(sh, p.herd);
    // a one-chunk pass without a communicator has nothing to pipeline: its
    // merge / commit / copies stay on the scoring stream, which saves the
    // cross-stream event hops (~15-20 us each) that dominate a small pass
    // (C1 extended 0.41 -> 0.385 ms per nas_place)
    p.one_stream = p.chunks.size() == 1 && !in.has_coll;
    // speculative slots: as many as the previous pass of this shape needed
    // (consecutive passes over similar clusters stop alike), enqueued before
    // the first status round trip; a slot whose walk is not halted exits at
    // once.  Not with a communicator: every rank must issue the same slots.
    p.spec = (!p.herd && !in.has_coll && hinted) ? h.slot_hint : 0;
    // (the herd plan's slots run inside its chunk loop, behind each commit;
    // pods they place after their chunk's rows were staged are unpacked again
    // at the end, like the speculative slots' -- `late_slots`)
    p.late_slots = p.spec > 0 || p.herd;
    // (an injected stall, NAS_OPT_INJECT_STALL_MS, sits on st behind the
    // pass: the host must wait on st then)
    // (the pass's last commit writes the status words to the pinned host area)
    p.status_in_commit = !p.late_slots && in.opt_inject_stall_ms == 0;
    // its bound: with collectives the communicator deadline -- the
    // commit stream's last commit may wait on an all-gather whose peer died --
    // so the pass fails as a communicator failure, never with a shorter fixed
    // budget that makes the tail "complete" while RCCL is stuck
    p.commit_wait_ms =
        in.opt_commit_wait_ms > 0 ? in.opt_commit_wait_ms
        : in.has_coll             ? (in.opt_comm_timeout_ms > 0 ? in.opt_comm_timeout_ms : 600000)
                                  : 2000;
    // (one stream: the chunk's merge starts the status words itself)
    p.init_in_merge = p.one_stream && in.live_cap;
    // A node-shard pass's chunks merge and exchange on their own stream (the
    // exchange stream; nas_place's pipelined loop).  one_stream implies
    // !has_coll and exchanging implies has_coll, so `exchanging && !one_stream`
    // is just `exchanging`.
    p.xs_mode = in.exchanging && !p.one_stream;
    return p;
}

// the end of a pass of shape (P, N) that needed rescore_rounds gathered slots
inline void note_pass(PassHistory &h, int P, int N, int rescore_rounds) {
    h.slot_hint = std::min(rescore_rounds, MAX_SPEC_SLOTS);
    h.last_rescore_rounds = rescore_rounds;
    if (rescore_rounds >= HERD_MIN_ROUNDS) {
        h.herd_P = P;
        h.herd_N = N;
    }
    h.slot_hint_P = P;
    h.slot_hint_N = N;
}

}  // namespace nas
