// Host side of the launch boundary (csrc/nas_internal.h) under ASan + UBSan:
// the argument structs' defaults against the launchers' former default
// arguments, and precheck() -- what launch_fit / launch_merge / launch_commit
// decide before they launch anything -- against a literal restatement of the
// launchers' former validation, over every combination of the inputs those
// rules read.  No GPU and no HIP runtime: precheck() is host-only code.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "nas_internal.h"

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

// ---- the rules as the launchers stated them on their positional parameters
static hipError_t old_fit(int *launched, const int32_t *rowmap, int batch, const Elig *el, int np) {
    *launched = 0;
    if (rowmap && batch != 1) return hipErrorInvalidValue;
    if (el && (batch != 1 || !el->labels || !el->taints || !el->require || !el->tolerate))
        return hipErrorInvalidValue;
    if (np <= 0) return hipSuccess;
    *launched = 1;
    return hipSuccess;
}
static hipError_t old_merge(int *launched, const Dyn *dyn, int np, const int32_t *dst_idx,
                            int batch, int32_t *init_status) {
    *launched = 0;
    if (dyn) np = dyn->win;
    if (np <= 0) return hipSuccess;
    if (dst_idx && batch != 1) return hipErrorInvalidValue;
    if (init_status && (dyn || batch != 1)) return hipErrorInvalidValue;
    *launched = 1;
    return hipSuccess;
}
static hipError_t old_commit(int *launched, int p_begin, int p_end, int32_t *stage_node, int batch,
                             int32_t *stage_status) {
    *launched = 0;
    if (p_begin >= 0 && p_end <= p_begin) return hipSuccess;
    if (stage_node && (p_begin < 0 || (batch != 1 && p_begin != 0))) return hipErrorInvalidValue;
    if (stage_status && batch != 1) return hipErrorInvalidValue;
    *launched = 1;
    return hipSuccess;
}

template <typename A>
static void same(const A &a, hipError_t want, int launched) {
    const Pre p = precheck(a);
    CHECK(pre_error(p) == want);
    CHECK((p == Pre::Launch) == (launched == 1));
}

int main() {
    // ---- defaults == the former default arguments
    {
        const FitArgs f;
        CHECK(!f.dyn && f.batch == 1 && !f.rowmap && f.req_stride == 0 && !f.el);
        CHECK(!f.cap && !f.req && !f.mask && f.np == 0);
        const MergeArgs m;
        CHECK(m.dst_p0 == 0 && !m.dyn && m.batch == 1 && m.dst_cluster_pods == 0 && !m.dst_idx &&
              !m.init_status);
        CHECK(!m.keys && !m.bounds && !m.cand_key && !m.cand_bound && m.np == 0);
        const CommitArgs c;
        CHECK(c.batch == 1 && !c.pub && !c.zrow && !c.stage_node && !c.stage_cost &&
              !c.stage_status);
        CHECK(!c.cand_key && !c.cap && !c.halt && c.p_begin == 0 && c.p_end == 0);
        const CostArgs k;
        CHECK(!k.dyn && k.batch == 1 && !k.ovf && !k.rowmap && !k.fit && !k.force_narrow &&
              !k.cache);
        // all three are empty ranges: hipSuccess without a launch
        CHECK(precheck(f) == Pre::Empty && precheck(m) == Pre::Empty && precheck(c) == Pre::Empty);
        CHECK(pre_error(Pre::Empty) == hipSuccess && pre_error(Pre::Launch) == hipSuccess &&
              pre_error(Pre::Invalid) == hipErrorInvalidValue);
    }
    // heap dummies (never dereferenced by the rules; ASan guards their bounds)
    auto words = std::make_unique<uint64_t[]>(4);
    auto ints = std::make_unique<int32_t[]>(4);
    const int batches[] = {0, 1, 2, 64}, counts[] = {-1, 0, 1, 300};
    int launched = 0;
    // ---- launch_fit: rowmap x batch x el (absent, complete, each word missing) x np
    for (int rm = 0; rm < 2; ++rm)
        for (int batch : batches)
            for (int e = -1; e <= 4; ++e)  // -1: no el; 0..3: that word null; 4: complete
                for (int np : counts) {
                    Elig el;
                    el.labels = e == 0 ? nullptr : words.get();
                    el.taints = e == 1 ? nullptr : words.get() + 1;
                    el.require = e == 2 ? nullptr : words.get() + 2;
                    el.tolerate = e == 3 ? nullptr : words.get() + 3;
                    FitArgs a;
                    a.rowmap = rm ? ints.get() : nullptr;
                    a.batch = batch;
                    a.el = e < 0 ? nullptr : &el;
                    a.np = np;
                    const hipError_t want = old_fit(&launched, a.rowmap, batch, a.el, np);
                    same(a, want, launched);
                }
    // ---- launch_merge: dyn (absent, win 0, win 5) x np x dst_idx x batch x init_status
    for (int d = 0; d < 3; ++d)
        for (int np : counts)
            for (int di = 0; di < 2; ++di)
                for (int batch : batches)
                    for (int is = 0; is < 2; ++is) {
                        const Dyn dyn{ints.get(), d == 1 ? 0 : 5, 7};
                        MergeArgs a;
                        a.dyn = d ? &dyn : nullptr;
                        a.np = np;
                        a.dst_idx = di ? ints.get() : nullptr;
                        a.batch = batch;
                        a.init_status = is ? ints.get() + 1 : nullptr;
                        const hipError_t want =
                            old_merge(&launched, a.dyn, np, a.dst_idx, batch, a.init_status);
                        same(a, want, launched);
                    }
    // ---- launch_commit: p_begin x p_end x stage_node x batch x stage_status
    for (int pb : {-1, 0, 3, 7})
        for (int pe : {0, 3, 7})
            for (int sn = 0; sn < 2; ++sn)
                for (int batch : batches)
                    for (int ss = 0; ss < 2; ++ss) {
                        CommitArgs a;
                        a.p_begin = pb;
                        a.p_end = pe;
                        a.stage_node = sn ? ints.get() : nullptr;
                        a.batch = batch;
                        a.stage_status = ss ? ints.get() + 2 : nullptr;
                        const hipError_t want =
                            old_commit(&launched, pb, pe, a.stage_node, batch, a.stage_status);
                        same(a, want, launched);
                    }
    std::printf("LAUNCH ARGS OK %ld checks\n", n_checked);
    return 0;
}
