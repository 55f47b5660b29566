// tn_tet_stats_core.h -- the three scalar rules of the per-tetrahedron training statistics (tn_tet_stats_accumulate), written
// once for the kernel (tn_tet_stats.hip) and the CPU emulation (tests/host/tet_stats_emul.cpp), the way tn_split_core.h states
// the split.  The same statement in numpy: render.tet_stats_statement.
//
// The rule.  stats i64 [T, 3], accumulated in place; a row q < count of S samples belongs to ray
// r = ray_index ? ray_index[q] : q; w = the composite's own weight of the sample (rayops::ray_composite, nan_to_num included),
// v = ray_value ? ray_value[r] : 1.
//   ACCEPT.   a sample counts iff its cell id is < T (unmatched samples carry 0xFFFFFFFF).
//   CLAMPS.   w^ = w >= 0 ? min(w, 1) : 0;   v^ = v >= 0 ? min(v, 256) : 0     (NaN and negative values -> 0, -0 -> 0)
//   SUMS.     stats[t, 0] += 1
//             stats[t, 1] += rint(w^ * 2^32)                  (the fp32 product by a power of two is exact; half to even)
//             stats[t, 2] += rint(fl32(w^ * v^) * 2^32)       (ONE fp32 multiply, fused with nothing)
// Largest terms: 2^32 (weight) and 2^40 (error), so a tetrahedron holds 2^31 accepted samples in the weight channel and
// MAX_SAMPLES_PER_CELL = 2^23 in the error channel before a sum could reach 2^63.  Nothing saturates: the caller resets first.
// Integer sums are associative and commutative: any order of the samples, any folding, any order of the atomics -- same bytes.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef TN_HD
#if defined(__HIPCC__)
#define TN_HD __host__ __device__ __forceinline__
#else
#define TN_HD inline
#endif
#endif

namespace tn {
namespace tetstats {

constexpr float WEIGHT_CAP = 1.0f, VALUE_CAP = 256.0f;
constexpr float SCALE = 4294967296.0f;                      // 2^32
constexpr int64_t MAX_WEIGHT_TERM = (int64_t)1 << 32, MAX_ERROR_TERM = (int64_t)1 << 40;
constexpr int64_t MAX_SAMPLES_PER_CELL = (int64_t)1 << 23;  // 2^23 * 2^40 = 2^63: one fewer always fits

TN_HD bool accept(uint32_t cell, uint32_t T) { return cell < T; }

TN_HD float clamp_weight(float w) { return w >= 0.0f ? (w < WEIGHT_CAP ? w : WEIGHT_CAP) : 0.0f; }
TN_HD float clamp_value(float v) { return v >= 0.0f ? (v < VALUE_CAP ? v : VALUE_CAP) : 0.0f; }

// rint(x * 2^32) for 0 <= x <= 256: the product is exact, rintf rounds half to even (the default rounding mode on the host,
// v_rndne_f32 on the device), the result is an integer <= 2^40 and converts exactly
TN_HD int64_t quantise(float x) { return (int64_t)rintf(x * SCALE); }

TN_HD int64_t weight_term(float w) { return quantise(clamp_weight(w)); }

// (one fp32 multiply: the library and the emulation are both built with -ffp-contract=off)
TN_HD int64_t error_term(float w, float v) {
    const float p = clamp_weight(w) * clamp_value(v);
    return quantise(p);
}

}  // namespace tetstats
}  // namespace tn
