// k_fit.hip -- batched resource-fit filter over all pod x node pairs.
//
// The reference's filter stage is findNodesThatFit (scheduler/scheduler.go:239-246),
// which lists the nodes and filters nothing; the north star's filter is the
// Kubernetes NodeResourcesFit rule: pod p fits node n iff
// req[r][p] <= free[r][n] for r in {cpu millicores, memory KiB, pod slots}.
//
// Layout: lane-per-NODE.  Each wave owns one 64-node chunk c (lane j = node
// 64c + j) and walks its pods 64 at a time, lane i holding pod i's requests;
// the decision itself -- the chunk's minima and maxima first, the remaining
// pods broadcast one by one -- is fit_wave.h's (FitChunk, fit_decide), shared
// with the cost kernel's fused fit.  The 64 words leave in one coalesced
// 8-byte-per-lane store:
//   mask[c * Pp + p]  bit j  <=>  pod p fits local node 64c + j.
// Requests are small against node capacity until nodes fill up, so most
// (pod, chunk) pairs cost 1/64 of a compare; the kernel runs near the rate of
// its mask write (P*N/8 bytes, HBM) -- see DESIGN.md.
//
// Constrained form (C = true, nas::Elig: node selectors and taints): a pod's
// require / tolerate words travel with its requests.  The unconstrained
// kernels are the C = false instantiations of the same bodies.
#include "fit_wave.h"

namespace nas {
namespace {

constexpr int FIT_THREADS = 256;  // 4 waves = 4 node chunks per block
constexpr int FIT_WAVES = FIT_THREADS / 64;
constexpr int FIT_PF = 2;  // groups of requests in flight ahead of the one decided

// G = 64-pod groups per wave (compile time: the group loop is unrolled and the
// request ring stays in registers).  Measured at the C3 shape (10k nodes x 100k
// pods, tools/mb_fit.hip): 29.0 us for the round-2 kernel (runtime group loop,
// one group prefetched), 25.5 us unrolled with the uniform bounds in SGPRs,
// 24.5 us with non-temporal mask stores (the mask is written once).
template <int G, bool C>
__device__ __forceinline__ void
fit_body(const int *cap, int N, int n0, int nloc, int n_chunks,
         const int *__restrict__ req, int Pp, int p0, int p_end, unsigned long long *__restrict__ mask,
         const int *__restrict__ dyn_start, int dyn_win, const int *__restrict__ dyn_hi_ptr,
         const int *__restrict__ rowmap, int rs, const Elig &el) {
    // rowmap (gathered rescore view): row q's requests are pod rowmap[q]'s,
    // in the main request array (row stride rs); the mask keeps view rows
    if (dyn_start) {  // window [*dyn_start, +dyn_win) read from device memory (rescore slots)
        const int s = dyn_start[blockIdx.z * STATUS_INTS];
        if (s < 0) return;
        p0 = s;
        if (dyn_hi_ptr) p_end = dyn_hi_ptr[blockIdx.z * STATUS_INTS];
        p_end = min(p_end, s + dyn_win);
    }
    const int pb0 = p0 + (int)blockIdx.x * 64 * G;
    if (pb0 >= p_end) return;  // whole block (no barriers below)
    const int cb = blockIdx.z;  // cluster of a batched launch
    cap += (size_t)cb * 3 * N;
    req += (size_t)cb * 3 * rs;
    mask += (size_t)cb * n_chunks * Pp;
    const int lane = threadIdx.x & 63;
    const int c = (int)blockIdx.y * FIT_WAVES + (int)(threadIdx.x >> 6);
    if (c >= n_chunks) return;
    const int nl = c * 64 + lane;
    const int pend = min(p_end, pb0 + 64 * G);
    // lane i holds pod pb + i's requests (one coalesced load per resource),
    // FIT_PF groups ahead of the one being decided; rows past the range are
    // clamped to its last row (loaded, never stored)
    auto row = [&](int r) { const int q = min(r, p_end - 1); return rowmap ? rowmap[q] : q; };
    constexpr int RING = FIT_PF + 1 < G ? FIT_PF + 1 : G;
    int ra[RING], rb[RING], rd[RING];
    u64 rq[C ? RING : 1], rt[C ? RING : 1];  // (constrained) the pod's require / tolerate words
#pragma unroll
    for (int g = 0; g < RING; ++g) {
        const int q = row(pb0 + 64 * g + lane);
        ra[g] = req[q];
        rb[g] = req[rs + q];
        rd[g] = req[2 * (size_t)rs + q];
        if constexpr (C) {
            rq[g] = el.require[q];
            rt[g] = el.tolerate[q];
        }
    }
    FitChunk<C> ch;
    ch.load(cap, N, n0 + nl, nl < nloc);
    ch.reduce(nl < nloc);
    if constexpr (C) ch.constrain(el, n0 + nl, nl < nloc);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int pb = pb0 + 64 * g;
        if (pb >= pend) break;
        const int sl = g % RING;
        const int a0 = ra[sl], b0 = rb[sl], d0 = rd[sl];
        const u64 q0 = C ? rq[C ? sl : 0] : 0, t0 = C ? rt[C ? sl : 0] : 0;
        if (g + RING < G) {  // refill the slot just consumed
            const int q = row(pb + 64 * RING + lane);
            ra[sl] = req[q];
            rb[sl] = req[rs + q];
            rd[sl] = req[2 * (size_t)rs + q];
            if constexpr (C) {
                rq[sl] = el.require[q];
                rt[sl] = el.tolerate[q];
            }
        }
        const bool in = pb + lane < pend;
        const u64 word = fit_decide<64>(ch, lane, a0, b0, d0, in, q0, t0);
        if (in) __builtin_nontemporal_store(word, mask + (size_t)c * Pp + pb + lane);
    }
}

template <int G>
__global__ void __launch_bounds__(FIT_THREADS)
k_fit(const int *cap, int N, int n0, int nloc, int n_chunks,
      const int *__restrict__ req, int Pp, int p0, int p_end, unsigned long long *__restrict__ mask,
      const int *__restrict__ dyn_start, int dyn_win, const int *__restrict__ dyn_hi_ptr,
      const int *__restrict__ rowmap, int rs) {
    fit_body<G, false>(cap, N, n0, nloc, n_chunks, req, Pp, p0, p_end, mask, dyn_start, dyn_win,
                       dyn_hi_ptr, rowmap, rs, Elig{});
}

// the constrained form: fits <=> eligible and the three resources fit
template <int G>
__global__ void __launch_bounds__(FIT_THREADS)
k_fit_c(const int *cap, int N, int n0, int nloc, int n_chunks,
        const int *__restrict__ req, int Pp, int p0, int p_end, unsigned long long *__restrict__ mask,
        const int *__restrict__ dyn_start, int dyn_win, const int *__restrict__ dyn_hi_ptr,
        const int *__restrict__ rowmap, int rs, const Elig el) {
    fit_body<G, true>(cap, N, n0, nloc, n_chunks, req, Pp, p0, p_end, mask, dyn_start, dyn_win,
                      dyn_hi_ptr, rowmap, rs, el);
}

// Two pods per lane (pods pb + 2i and pb + 2i + 1 of a 128-pod group): the
// requests arrive as one 8-byte load per resource and the two fit words leave
// as ONE 16-byte store per lane -- half the memory instructions of k_fit per
// pod for the same bytes.  Same decisions as k_fit (the chunk's extremes
// first, then the remaining pods one by one); main pod ranges only (no row
// map: a gathered view's rows are not adjacent).
template <int G, bool C>
__device__ __forceinline__ void
fit2_body(const int *cap, int N, int n0, int nloc, int n_chunks,
          const int *__restrict__ req, int Pp, int p0, int p_end, unsigned long long *__restrict__ mask,
          const int *__restrict__ dyn_start, int dyn_win, const int *__restrict__ dyn_hi_ptr,
          const Elig &el) {
    if (dyn_start) {
        const int s = dyn_start[blockIdx.z * STATUS_INTS];
        if (s < 0) return;
        p0 = s & ~1;  // pairs start on an even pod (the store is 16-byte aligned)
        if (dyn_hi_ptr) p_end = dyn_hi_ptr[blockIdx.z * STATUS_INTS];
        p_end = min(p_end, s + dyn_win);
    }
    const int pb0 = p0 + (int)blockIdx.x * 128 * G;
    if (pb0 >= p_end) return;
    const int cb = blockIdx.z;
    cap += (size_t)cb * 3 * N;
    req += (size_t)cb * 3 * Pp;
    mask += (size_t)cb * n_chunks * Pp;
    const int lane = threadIdx.x & 63;
    const int c = (int)blockIdx.y * FIT_WAVES + (int)(threadIdx.x >> 6);
    if (c >= n_chunks) return;
    const int nl = c * 64 + lane;
    const int pend = min(p_end, pb0 + 128 * G);
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    // requests of the lane's two pods (8-byte loads; rows past the range read
    // the last even pair, loaded, never stored); constrained: their require /
    // tolerate words too (16-byte loads)
    u64x2 rq = {0, 0}, rt = {0, 0};
    auto load2 = [&](int pb, int2 &a, int2 &b, int2 &d) {
        const int q = min(pb + 2 * lane, (p_end - 1) & ~1);
        a = *reinterpret_cast<const int2 *>(req + q);
        b = *reinterpret_cast<const int2 *>(req + Pp + q);
        d = *reinterpret_cast<const int2 *>(req + 2 * (size_t)Pp + q);
        if constexpr (C) {
            rq = *reinterpret_cast<const u64x2 *>(el.require + q);
            rt = *reinterpret_cast<const u64x2 *>(el.tolerate + q);
        }
    };
    int2 ra, rb, rd;
    load2(pb0, ra, rb, rd);  // (ahead of the chunk, as in fit_body: behind it, one VGPR more at G = 1)
    FitChunk<C> ch;
    ch.load(cap, N, n0 + nl, nl < nloc);
    ch.reduce(nl < nloc);
    if constexpr (C) ch.constrain(el, n0 + nl, nl < nloc);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int pb = pb0 + 128 * g;
        if (pb >= pend) break;
        const int2 a0 = ra, b0 = rb, d0 = rd;
        const u64x2 q0 = rq, t0 = rt;
        if (g + 1 < G) load2(pb + 128, ra, rb, rd);  // next group in flight
        const bool in0 = pb + 2 * lane < pend, in1 = pb + 2 * lane + 1 < pend;
        const u64 w0 = fit_decide<64>(ch, lane, a0.x, b0.x, d0.x, in0, q0.x, t0.x);
        const u64 w1 = fit_decide<64>(ch, lane, a0.y, b0.y, d0.y, in1, q0.y, t0.y);
        unsigned long long *dst = mask + (size_t)c * Pp + pb + 2 * lane;
        // plain stores: 24.7-24.9 vs 25.1-25.8 us for non-temporal ones at the
        // C3 shape (profiles/r04_ab_fold.txt, fitpl)
        if (in1) {
            *reinterpret_cast<u64x2 *>(dst) = u64x2{w0, w1};
        } else if (in0) {
            *dst = w0;
        }
    }
}

template <int G>
__global__ void __launch_bounds__(FIT_THREADS)
k_fit2(const int *cap, int N, int n0, int nloc, int n_chunks,
       const int *__restrict__ req, int Pp, int p0, int p_end, unsigned long long *__restrict__ mask,
       const int *__restrict__ dyn_start, int dyn_win, const int *__restrict__ dyn_hi_ptr) {
    fit2_body<G, false>(cap, N, n0, nloc, n_chunks, req, Pp, p0, p_end, mask, dyn_start, dyn_win,
                        dyn_hi_ptr, Elig{});
}

template <int G>
__global__ void __launch_bounds__(FIT_THREADS)
k_fit2_c(const int *cap, int N, int n0, int nloc, int n_chunks,
         const int *__restrict__ req, int Pp, int p0, int p_end, unsigned long long *__restrict__ mask,
         const int *__restrict__ dyn_start, int dyn_win, const int *__restrict__ dyn_hi_ptr,
         const Elig el) {
    fit2_body<G, true>(cap, N, n0, nloc, n_chunks, req, Pp, p0, p_end, mask, dyn_start, dyn_win,
                       dyn_hi_ptr, el);
}

}  // namespace

hipError_t launch_fit(hipStream_t st, const FitArgs &a) {
    if (const Pre pre = precheck(a); pre != Pre::Launch) return pre_error(pre);
    const int32_t *cap = a.cap, *req = a.req, *rowmap = a.rowmap;
    const int N = a.N, n0 = a.n0, nloc = a.nloc, Pp = a.Pp, p0 = a.p0, np = a.np, batch = a.batch;
    const Dyn *dyn = a.dyn;
    const Elig *el = a.el;
    const int n_chunks = a.Mp / 64;
    // one pod per lane (k_fit, groups of 64 pods), or two (k_fit2, groups of
    // 128) over a main range from an even pod
    const bool pair = !rowmap && p0 % 2 == 0;
    const int gp = pair ? 128 : 64;
    // pods per block: up to 512, fewer when the launch is small, so a rescore
    // slot's few thousand pods still spread over ~2k blocks (each wave's pod
    // groups run back to back: latency, not work, sets a small launch's time)
    const int yb = (n_chunks + FIT_WAVES - 1) / FIT_WAVES;
    const long long groups = ((long long)np + gp - 1) / gp * yb;
    const int k = (int)std::max(1LL, std::min<long long>(512 / gp, groups / 2048));
    const int G = k >= 8 ? 8 : k >= 4 ? 4 : k >= 2 ? 2 : 1;  // instantiated group counts
    // (pairs: a window from an odd pod starts one pod early, so one more block)
    dim3 grid((np + gp * G - 1) / (gp * G) + (pair && dyn ? 1 : 0), yb, batch);
    auto *m = reinterpret_cast<unsigned long long *>(a.mask);
    const int pe = dyn ? dyn->hi : p0 + np;
    const int *ds = dyn ? dyn->start : nullptr, *dh = dyn ? dyn->hi_ptr : nullptr;
    const int dw = dyn ? dyn->win : 0, rs = rowmap ? a.req_stride : Pp;
#define NAS_FIT(K, GV, ...)                                                                         \
    if (el)                                                                                         \
        K##_c<GV><<<grid, FIT_THREADS, 0, st>>>(cap, N, n0, nloc, n_chunks, req, Pp, p0, pe, m, ds, \
                                                dw, dh, ##__VA_ARGS__, *el);                        \
    else                                                                                            \
        K<GV><<<grid, FIT_THREADS, 0, st>>>(cap, N, n0, nloc, n_chunks, req, Pp, p0, pe, m, ds, dw, \
                                            dh, ##__VA_ARGS__)
    if (pair) {
        switch (G) {
        case 4: NAS_FIT(k_fit2, 4); break;
        case 2: NAS_FIT(k_fit2, 2); break;
        default: NAS_FIT(k_fit2, 1); break;
        }
    } else {
        switch (G) {
        case 8: NAS_FIT(k_fit, 8, rowmap, rs); break;
        case 4: NAS_FIT(k_fit, 4, rowmap, rs); break;
        case 2: NAS_FIT(k_fit, 2, rowmap, rs); break;
        default: NAS_FIT(k_fit, 1, rowmap, rs); break;
        }
    }
#undef NAS_FIT
    return hipGetLastError();
}

}  // namespace nas
