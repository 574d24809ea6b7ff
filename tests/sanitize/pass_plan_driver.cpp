// Pass planning (csrc/pass_plan.h) and result decoding (csrc/result_decode.h)
// under ASan + UBSan, without a GPU or the HIP runtime:
//  a. the chunk plans DESIGN.md quotes, pinned end offset by end offset;
//  b. over a sweep of shapes: chunks are non-empty, contiguous, cover [0, P),
//     end on whole cost tiles, and the planner terminates;
//  c. plan_pass()'s mode flags against a literal restatement of the
//     expressions nas_place computed in line, over every combination of their
//     inputs, the implications between them by name, and note_pass();
//  d. decode_cost / decode_int_score / unpack_range against per-element
//     restatements.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "pass_plan.h"
#include "result_decode.h"

using namespace nas;

static long n_checked = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
        ++n_checked;                                                         \
    } while (0)

constexpr int WIDE_PODS = 384;  // nas::cost_tile_pods() on gfx950

static PassShape shape(int P, int N, int world, int n_cu = 256) {
    return {P, (int)round_up(P, COST_BN), N, 1, world, 0, n_cu, WIDE_PODS};
}

typedef std::vector<std::pair<int, int>> Chunks;

// contiguous from 0, non-empty, ending at P
static void check_cover(const Chunks &c, int P) {
    CHECK(!c.empty() && c.front().first == 0 && c.back().second == P);
    for (size_t i = 0; i < c.size(); ++i) {
        CHECK(c[i].first < c[i].second);
        if (i) CHECK(c[i].first == c[i - 1].second);
    }
}

static void check_ends(const PassShape &s, bool herd, std::initializer_list<int> want) {
    const Chunks c = plan_chunks(s, herd);
    check_cover(c, s.P);
    CHECK(c.size() == want.size());
    size_t i = 0;
    for (int e : want) CHECK(c[i++].second == e);
}

// `n` chunks whose sizes are runs {count, pods}, in order
static void check_runs(const PassShape &s, bool herd, size_t n,
                       std::initializer_list<std::pair<int, int>> runs) {
    const Chunks c = plan_chunks(s, herd);
    check_cover(c, s.P);
    CHECK(c.size() == n);
    size_t i = 0;
    for (const auto &r : runs)
        for (int k = 0; k < r.first; ++k, ++i) {
            CHECK(i < c.size());
            CHECK(c[i].second - c[i].first == r.second);
        }
    CHECK(i == n);
}

static void pinned_plans() {
    check_ends(shape(8193, 4097, 1), false, {8192, 8193});
    check_ends(shape(8192, 4097, 1), false, {8192});
    check_ends(shape(20000, 4097, 1), false, {8192, 16384, 20000});
    CHECK(tile_pods(shape(33000, 300, 1)) == WIDE_PODS);
    check_ends(shape(33000, 300, 1), false, {12288, 18432, 22272, 33000});
    check_ends(shape(50000, 600, 1), false, {12288, 18432, 30720, 43008, 50000});
    check_ends(shape(10000, 1000, 1), false, {10000});  // C2
    for (int n_cu : {256, 304})
        check_ends(shape(3000, 600, 1, n_cu), true, {512, 1024, 1536, 2048, 2560, 3000});
    check_ends(shape(2000, 300, 1), true, {256, 512, 768, 1024, 1280, 1536, 1792, 2000});
    // C3
    check_ends(shape(100000, 10000, 1), false,
               {12288, 18432, 30720, 43008, 55296, 67584, 79872, 92160, 92928, 100000});
    check_runs(shape(100000, 10000, 1, 256), true, 44, {{43, 2304}, {1, 928}});
    check_runs(shape(100000, 10000, 2), false, 12, {{11, 8448}, {1, 7072}});
    check_runs(shape(100000, 10000, 3), false, 11, {{1, 8448}, {9, 9216}, {1, 8608}});
    for (int world : {4, 8})
        check_ends(shape(100000, 10000, world), false,
                   {8448, 23808, 39168, 54528, 69888, 85248, 100000});
    // C4
    check_runs(shape(500000, 50000, 1), false, 42,
               {{1, 12288}, {1, 6144}, {38, 12288}, {1, 3840}, {1, 10784}});
    check_runs(shape(500000, 50000, 8), false, 60, {{59, 8448}, {1, 1568}});
    check_ends(shape(32767, 2049, 8), false, {32767});
    check_ends(shape(40000, 300, 4), false, {40000});
    check_ends(shape(1, 1, 1), false, {1});
    check_ends(shape(1, 1, 1), true, {1});
}

static long sweep_properties() {
    std::vector<int> pods;
    for (int P = 1; P <= 70000; P += 257 + P % 223) pods.push_back(P);
    for (int P : {32767, 32768, 32769, 65536, 131072, 262144, 999999, 2000000}) pods.push_back(P);
    long shapes = 0;
    size_t longest = 0;
    for (int P : pods)
        for (int N : {1, 255, 256, 257, 600, 2049, 4097, 10000, 50000, 200000})
            for (int world : {1, 2, 3, 4, 8, 16, 64})
                for (int n_cu : {64, 256, 304})
                    for (int herd = 0; herd < (world == 1 ? 2 : 1); ++herd) {
                        const PassShape s = shape(P, N, world, n_cu);
                        const Chunks c = plan_chunks(s, herd != 0);
                        check_cover(c, P);
                        // terminated with chunks of at least one 256-pod unit
                        CHECK(c.size() <= (size_t)s.Pp / COST_BN);
                        const int unit = tile_pods(s) == COST_BN ? COST_BN : 768;  // lcm(384, 256)
                        for (const auto &ch : c) CHECK(ch.second == P || ch.second % unit == 0);
                        longest = std::max(longest, c.size());
                        ++shapes;
                    }
    CHECK(longest > 1000);  // the sweep reaches long plans
    return shapes;
}

// ---- c. the mode flags as nas_place computed them in line, on a context
struct OldCtx {
    int P, N;
    int32_t opt_herd_plan, opt_cost_cache;
    int64_t opt_inject_stall_ms, opt_commit_wait_ms, opt_comm_timeout_ms;
    int32_t herd_P, herd_N, slot_hint, slot_hint_P, slot_hint_N, last_rescore_rounds;
    bool coll, exch, con;
};
static bool has_coll(const OldCtx *ctx) { return ctx->coll; }
static bool exchanging(const OldCtx *ctx) { return ctx->exch; }
static bool constrained(const OldCtx *ctx) { return ctx->con; }

struct OldMode {
    bool herd, cache_wanted, one_stream;
    int spec;
    bool late_slots, status_in_commit, xs_mode, init_in_merge;
    int64_t commit_wait_ms;
};
static bool old_herd_shape(const OldCtx *ctx) {
    const int P = ctx->P, N = ctx->N;
    const bool herd_shape = !has_coll(ctx) &&
                            (ctx->opt_herd_plan == 1 ||
                             (ctx->opt_herd_plan == 2 && ctx->herd_P == P && ctx->herd_N == N));
    return herd_shape;
}
static OldMode old_mode(const OldCtx *ctx, size_t bytes, size_t n_chunks, bool live_cap) {
    const int P = ctx->P, N = ctx->N;
    OldMode m;
    const bool herd_shape = old_herd_shape(ctx);
    m.cache_wanted = false;
    if (ctx->opt_cost_cache != 0 && !constrained(ctx)) {
        const bool herd = ctx->slot_hint_P == P && ctx->slot_hint_N == N &&
                          ctx->last_rescore_rounds >= CACHE_MIN_ROUNDS;
        if ((ctx->opt_cost_cache == 1 || herd || herd_shape) && bytes <= CACHE_MAX_BYTES)
            m.cache_wanted = true;
    }
    const bool herd = herd_shape;
    const bool one_stream = n_chunks == 1 && !has_coll(ctx);
    const int spec = (!herd && !has_coll(ctx) && ctx->slot_hint_P == P && ctx->slot_hint_N == N)
                         ? ctx->slot_hint : 0;
    const bool late_slots = spec > 0 || herd;
    const bool status_in_commit = !late_slots && ctx->opt_inject_stall_ms == 0;
    const int64_t commit_wait_ms =
        ctx->opt_commit_wait_ms > 0 ? ctx->opt_commit_wait_ms
        : has_coll(ctx)             ? (ctx->opt_comm_timeout_ms > 0 ? ctx->opt_comm_timeout_ms : 600000)
                                    : 2000;
    const bool init_in_merge = one_stream && live_cap;
    const bool xs_mode = exchanging(ctx) && !one_stream;
    m.herd = herd;
    m.one_stream = one_stream;
    m.spec = spec;
    m.late_slots = late_slots;
    m.status_in_commit = status_in_commit;
    m.commit_wait_ms = commit_wait_ms;
    m.init_in_merge = init_in_merge;
    m.xs_mode = xs_mode;
    return m;
}
// the end of nas_place: its seven assignments
static void old_note(OldCtx *ctx, int P, int N, const int32_t *hs) {
    ctx->slot_hint = std::min(hs[1], MAX_SPEC_SLOTS);
    ctx->last_rescore_rounds = hs[1];
    if (hs[1] >= HERD_MIN_ROUNDS) {
        ctx->herd_P = P;
        ctx->herd_N = N;
    }
    ctx->slot_hint_P = P;
    ctx->slot_hint_N = N;
}

// the smallest pod count (in 256-pod steps) of a 4,097-node, world-1 pass with
// n chunks
constexpr int MODE_NODES = 4097;  // 17 node tiles: 32-tile chunks, so few pods make many chunks
static int pods_with_chunks(size_t n, bool herd) {
    for (int P = 256; P < 200000; P += 256)
        if (plan_chunks(shape(P, MODE_NODES, 1), herd).size() == n) return P;
    CHECK(!"no shape with that many chunks");
    return 0;
}

static void mode_flags() {
    const int N = MODE_NODES;
    const size_t counts[3] = {1, 2, 7};
    int pods[2][3];
    for (int h = 0; h < 2; ++h)
        for (int k = 0; k < 3; ++k) pods[h][k] = pods_with_chunks(counts[k], h != 0);
    for (int herd_plan = 0; herd_plan <= 2; ++herd_plan)
    for (int cost_cache = 0; cost_cache <= 2; ++cost_cache)
    for (int ce = 0; ce < 3; ++ce)  // (has_coll, exchanging): (0,0) (1,0) (1,1)
    for (int con = 0; con < 2; ++con)
    for (int herd_eq = 0; herd_eq < 2; ++herd_eq)
    for (int hint_eq = 0; hint_eq < 2; ++hint_eq)
    for (int rounds : {0, 3, 4, 8})
    for (int hint : {0, 3, 8})
    for (int k = 0; k < 3; ++k)
    for (int live_cap = 0; live_cap < 2; ++live_cap)
    for (int64_t stall : {0, 5})
    for (int64_t wait : {0, 50})
    for (int64_t timeout : {0, 120000})
    for (size_t bytes : {(size_t)1 << 20, ((size_t)16 << 30) + 4}) {
        OldCtx o{};
        o.N = N;
        o.opt_herd_plan = herd_plan;
        o.opt_cost_cache = cost_cache;
        o.opt_inject_stall_ms = stall;
        o.opt_commit_wait_ms = wait;
        o.opt_comm_timeout_ms = timeout;
        o.coll = ce >= 1;
        o.exch = ce == 2;
        o.con = con != 0;
        o.slot_hint = hint;
        o.last_rescore_rounds = rounds;
        // whether the pass is a herd does not depend on P beyond herd_eq:
        // decide it first, then take the pod count with the wanted chunks
        o.P = 1;
        o.herd_P = herd_eq ? 1 : 2;
        o.herd_N = N;
        const bool herd = old_herd_shape(&o);
        const int P = pods[herd][k];
        o.P = P;
        o.herd_P = herd_eq ? P : P + 1;
        o.slot_hint_P = P;
        o.slot_hint_N = hint_eq ? N : N + 1;
        CHECK(old_herd_shape(&o) == herd);

        PassInputs in{};
        in.opt_herd_plan = herd_plan;
        in.opt_cost_cache = cost_cache;
        in.opt_inject_stall_ms = stall;
        in.opt_commit_wait_ms = wait;
        in.opt_comm_timeout_ms = timeout;
        in.hist.herd_P = o.herd_P;
        in.hist.herd_N = o.herd_N;
        in.hist.slot_hint = o.slot_hint;
        in.hist.slot_hint_P = o.slot_hint_P;
        in.hist.slot_hint_N = o.slot_hint_N;
        in.hist.last_rescore_rounds = o.last_rescore_rounds;
        in.has_coll = o.coll;
        in.exchanging = o.exch;
        in.constrained = o.con;
        in.live_cap = live_cap != 0;
        in.cache_bytes = bytes;
        const PassShape s = shape(P, N, 1);
        const PassPlan p = plan_pass(s, in);
        CHECK(p.chunks == plan_chunks(s, herd));
        CHECK(p.chunks.size() == counts[k]);
        const OldMode m = old_mode(&o, bytes, p.chunks.size(), live_cap != 0);
        CHECK(p.herd == m.herd);
        CHECK(p.want_cache == m.cache_wanted);
        CHECK(p.one_stream == m.one_stream);
        CHECK(p.spec == m.spec);
        CHECK(p.late_slots == m.late_slots);
        CHECK(p.status_in_commit == m.status_in_commit);
        CHECK(p.xs_mode == m.xs_mode);
        CHECK(p.init_in_merge == m.init_in_merge);
        CHECK(p.commit_wait_ms == m.commit_wait_ms);
        // the implications, by name
        if (in.has_coll) CHECK(!p.herd && p.spec == 0 && !p.one_stream);
        if (p.herd) CHECK(p.spec == 0 && p.late_slots);
        if (p.status_in_commit) CHECK(!p.late_slots && stall == 0);
        if (in.constrained) CHECK(!p.want_cache);
        CHECK(p.xs_mode == in.exchanging);
        CHECK(p.commit_wait_ms == (wait > 0 ? wait : in.has_coll ? (timeout > 0 ? timeout : 600000) : 2000));
    }
    // note_pass against the seven assignments, chained so that a herd shape sticks
    OldCtx o{};
    o.herd_P = o.herd_N = o.slot_hint_P = o.slot_hint_N = -1;
    PassHistory h;
    CHECK(h.herd_P == -1 && h.herd_N == -1 && h.slot_hint == 0 && h.slot_hint_P == -1 &&
          h.slot_hint_N == -1 && h.last_rescore_rounds == 0);
    const int passes[][3] = {{100, 10, 0}, {100, 10, 3}, {100, 10, 7}, {100, 10, 8}, {200, 10, 2},
                             {100, 20, 90}, {100, 10, 0}, {1, 1, 9}};
    for (const auto &ps : passes) {
        const int32_t hs[2] = {-1, ps[2]};
        old_note(&o, ps[0], ps[1], hs);
        note_pass(h, ps[0], ps[1], ps[2]);
        CHECK(h.herd_P == o.herd_P && h.herd_N == o.herd_N && h.slot_hint == o.slot_hint &&
              h.slot_hint_P == o.slot_hint_P && h.slot_hint_N == o.slot_hint_N &&
              h.last_rescore_rounds == o.last_rescore_rounds);
    }
    // the other host constants' functions
    CHECK(gather_batch(1, false) == 4 && gather_batch(2, false) == 1 && gather_batch(2, true) == 1 &&
          gather_batch(3, true) == 4 && gather_batch(4, false) == 4 && gather_batch(4, true) == 8);
    CHECK(host_out_offset(0) == 4096 && host_out_offset(1) == 4096 && host_out_offset(128) == 4096 &&
          host_out_offset(129) == 8192 && host_out_offset(65535) == (size_t)65535 * 32 + 32);
}

// ---- d. decoding
static uint32_t int_key(int32_t v) { return (uint32_t)v ^ 0x80000000u; }  // k_cost.hip okey
static uint32_t float_key(float f) {                                      // k_cost.hip fkey
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// what nas_place's results hold for pod i, element by element
static float ref_cost(int32_t node, uint32_t raw, int dtype) {
    if (node < 0) return 0.f;
    if (dtype == NAS_DT_I8) return (float)(int32_t)(raw ^ 0x80000000u);
    const uint32_t u = (raw & 0x80000000u) ? (raw & 0x7fffffffu) : ~raw;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static int64_t ref_score(int32_t node, uint32_t raw, int dtype) {
    return (node < 0 || dtype != NAS_DT_I8) ? 0 : (int64_t)(int32_t)(raw ^ 0x80000000u);
}

static void decoding() {
    const int32_t ints[] = {INT32_MIN, -1, 0, 1, INT32_MAX - 1};
    for (int32_t v : ints) {
        CHECK(decode_int_score(int_key(v)) == v);
        CHECK(decode_cost(int_key(v), NAS_DT_I8) == (float)v);
    }
    const float inf = std::numeric_limits<float>::infinity();
    const float floats[] = {0.f, -0.f, 1.5f, -1.5f, FLT_MAX, -FLT_MAX, inf, -inf};
    for (float f : floats)
        for (int dt : {NAS_DT_BF16, NAS_DT_F32}) CHECK(same_bits(decode_cost(float_key(f), dt), f));
    // keys ascend with their values
    for (size_t i = 1; i < sizeof(ints) / sizeof(ints[0]); ++i) CHECK(int_key(ints[i - 1]) < int_key(ints[i]));
    CHECK(float_key(-inf) < float_key(-1.5f) && float_key(-1.5f) < float_key(-0.f) &&
          float_key(-0.f) < float_key(0.f) && float_key(0.f) < float_key(1.5f) &&
          float_key(1.5f) < float_key(inf));

    // unpack_range: a stage of n pods, some unplaced, exactly sized on the heap
    const int n = 13;
    for (int dt : {NAS_DT_I8, NAS_DT_BF16, NAS_DT_F32}) {
        auto node = std::make_unique<int32_t[]>(n);
        auto raw = std::make_unique<int32_t[]>(n);
        for (int i = 0; i < n; ++i) {
            node[i] = (i % 4 == 2) ? -1 : 7 * i;
            const uint32_t k = dt == NAS_DT_I8 ? int_key(ints[i % 5])
                                               : float_key(floats[i % 8] * (i < 8 ? 1.f : 0.5f));
            std::memcpy(&raw[i], &k, 4);
        }
        const int ranges[][2] = {{0, n}, {3, n}, {3, 7}, {5, 5}, {2, 3}};
        for (const auto &r : ranges)
            for (int wc = 0; wc < 2; ++wc)
                for (int wi = 0; wi < 2; ++wi) {
                    const int lo = r[0], hi = r[1];
                    auto out_n = std::make_unique<int32_t[]>(n);
                    auto out_c = std::make_unique<float[]>(n);
                    auto out_i = std::make_unique<int64_t[]>(n);
                    for (int i = 0; i < n; ++i) {
                        out_n[i] = -777;
                        out_c[i] = -777.f;
                        out_i[i] = -777;
                    }
                    int unsched = 5, want_unsched = 5;
                    unpack_range(out_n.get(), wc ? out_c.get() : nullptr, wi ? out_i.get() : nullptr,
                                 node.get(), raw.get(), lo, hi, dt, unsched);
                    for (int i = 0; i < n; ++i) {
                        const bool in = i >= lo && i < hi;
                        uint32_t k;
                        std::memcpy(&k, &raw[i], 4);
                        want_unsched += in && node[i] < 0;
                        CHECK(out_n[i] == (in ? node[i] : -777));
                        CHECK(same_bits(out_c[i], in && wc ? ref_cost(node[i], k, dt) : -777.f));
                        CHECK(out_i[i] == (in && wi ? ref_score(node[i], k, dt) : -777));
                    }
                    CHECK(unsched == want_unsched);
                }
    }
}

int main() {
    pinned_plans();
    const long shapes = sweep_properties();
    mode_flags();
    decoding();
    std::printf("PASS PLAN OK %ld checks (%ld swept shapes)\n", n_checked, shapes);
    return 0;
}
