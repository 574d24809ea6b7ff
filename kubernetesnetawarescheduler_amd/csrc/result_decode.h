// result_decode.h -- the host's decoding of what a pass leaves: the orderable
// 32-bit cost words of candidate keys and commit results (k_cost.hip: int8
// path, the exact int32 score with its sign bit flipped; bf16 / fp32 paths, the
// float's bits made orderable) into the C ABI's float cost and integer score.
// Host-only, no HIP runtime (tests/sanitize/pass_plan_driver.cpp).
#pragma once

#include <stdint.h>

#include <cstring>

#include "../../include/nas.h"

namespace nas {

// the int8 path's exact score from its orderable word
inline int32_t decode_int_score(uint32_t raw) { return (int32_t)(raw ^ 0x80000000u); }

inline float decode_cost(uint32_t raw, int dtype) {
    if (dtype == NAS_DT_I8) return (float)decode_int_score(raw);
    const uint32_t u = (raw & 0x80000000u) ? (raw & 0x7fffffffu) : ~raw;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// decode pods [lo, hi) of a staging area (placements `from`, raw cost words
// `raw_in`) into the caller's arrays; an unplaced pod (node < 0) scores 0 and
// counts in `unsched`
inline void unpack_range(int32_t *__restrict__ node_out, float *__restrict__ cost_out,
                         int64_t *__restrict__ int_score_out, const int32_t *__restrict__ from,
                         const int32_t *__restrict__ raw_in, int lo, int hi, int dtype,
                         int &unsched) {
    const uint32_t *__restrict__ raw = reinterpret_cast<const uint32_t *>(raw_in);
    int none = 0;
    if (dtype == NAS_DT_I8 && cost_out && int_score_out) {
        // the common case in one pass over the stage (host-memory bound:
        // 24 B per pod; 0.24 vs 0.49 ms per 100k pods for the per-pod loop
        // with the dtype test and a possibly aliased counter inside)
        for (int i = lo; i < hi; ++i) {
            const int32_t n = from[i];
            const int32_t v = decode_int_score(raw[i]);
            const bool z = n < 0;
            node_out[i] = n;
            none += z;
            cost_out[i] = z ? 0.f : (float)v;
            int_score_out[i] = z ? 0 : (int64_t)v;
        }
        unsched += none;
        return;
    }
    std::memcpy(node_out + lo, from + lo, (size_t)(hi - lo) * 4);
    for (int i = lo; i < hi; ++i) none += from[i] < 0;
    unsched += none;
    if (cost_out)
        for (int i = lo; i < hi; ++i) cost_out[i] = from[i] < 0 ? 0.f : decode_cost(raw[i], dtype);
    if (int_score_out) {
        if (dtype == NAS_DT_I8) {
            for (int i = lo; i < hi; ++i)
                int_score_out[i] = from[i] < 0 ? 0 : (int64_t)decode_int_score(raw[i]);
        } else {
            std::memset(int_score_out + lo, 0, (size_t)(hi - lo) * 8);
        }
    }
}

}  // namespace nas
