// tn_ray_key.h -- the sort key of a binned trace_rays call (TN_TRACE_BIN_RAYS), as the device computes it.  Plain C++ without a
// HIP include: k_ray_keys (tn_ray_order.hip) calls ray_key() per lane, and tests/host/ray_key_check.cpp compiles the same
// function with g++ to compare it, without a GPU, with the statement of the key in tetra-nerf_amd/ray_order.py.  Every
// operation is a single IEEE float32 rounding (the build uses -ffp-contract=off and correctly rounded division); sums are
// associated as ((x + y) + z).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TN_RAY_KEY_HD __host__ __device__ __forceinline__
#else
#define TN_RAY_KEY_HD inline
#endif

namespace tn {

constexpr int RAY_KEY_ORIGIN_BITS = 4, RAY_KEY_POINT_BITS = 6, RAY_KEY_BITS = 3 * (RAY_KEY_ORIGIN_BITS + RAY_KEY_POINT_BITS);

// what the key needs of the mesh box [lo, hi]: centre, three times the half extents, half diagonal (ray_order.box_constants)
struct RayKeyBox { float c[3], e[3], r; };
inline RayKeyBox ray_key_box(const float lo[3], const float hi[3]) {
    RayKeyBox b{};
    float h[3];
    for (int k = 0; k < 3; ++k) {
        b.c[k] = (lo[k] + hi[k]) * 0.5f;
        h[k] = (hi[k] - lo[k]) * 0.5f;
        b.e[k] = h[k] * 3.0f;
    }
    b.r = std::sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]);
    return b;
}

// float -> cell 0 .. top: NaN and everything below 0 -> 0, everything above (+inf too) -> top.  Clamped BEFORE the conversion,
// so the conversion is always defined.
TN_RAY_KEY_HD uint32_t ray_key_cell(float x, float top) {
    x = x > 0.0f ? x : 0.0f;
    x = x < top ? x : top;
    return (uint32_t)x;
}
template <int BITS>
TN_RAY_KEY_HD uint32_t ray_key_morton(uint32_t cx, uint32_t cy, uint32_t cz) {
    uint32_t key = 0;
    for (int i = 0; i < BITS; ++i)
        key |= (((cx >> i) & 1u) << (3 * i)) | (((cy >> i) & 1u) << (3 * i + 1)) | (((cz >> i) & 1u) << (3 * i + 2));
    return key;
}

// bits 18..29: Morton cell of the origin in [c - 3h, c + 3h]; bits 0..17: Morton cell of the point of the ray's line closest to c in [c - r, c + r]
TN_RAY_KEY_HD uint32_t ray_key(float ox, float oy, float oz, float dx, float dy, float dz, const RayKeyBox &b) {
    const float wx = b.c[0] - ox, wy = b.c[1] - oy, wz = b.c[2] - oz;
    const float dd = (dx * dx + dy * dy) + dz * dz;
    const float t = ((wx * dx + wy * dy) + wz * dz) / dd;
    const float px = ox + dx * t, py = oy + dy * t, pz = oz + dz * t;
    constexpr float NO = (float)(1 << (RAY_KEY_ORIGIN_BITS - 1)), NP = (float)(1 << (RAY_KEY_POINT_BITS - 1));
    constexpr float TO = (float)((1 << RAY_KEY_ORIGIN_BITS) - 1), TP = (float)((1 << RAY_KEY_POINT_BITS) - 1);
    const uint32_t ko = ray_key_morton<RAY_KEY_ORIGIN_BITS>(ray_key_cell(((ox - b.c[0]) / b.e[0]) * NO + NO, TO),
                                                            ray_key_cell(((oy - b.c[1]) / b.e[1]) * NO + NO, TO),
                                                            ray_key_cell(((oz - b.c[2]) / b.e[2]) * NO + NO, TO));
    const uint32_t kp = ray_key_morton<RAY_KEY_POINT_BITS>(ray_key_cell(((px - b.c[0]) / b.r) * NP + NP, TP),
                                                           ray_key_cell(((py - b.c[1]) / b.r) * NP + NP, TP),
                                                           ray_key_cell(((pz - b.c[2]) / b.r) * NP + NP, TP));
    return (ko << (3 * RAY_KEY_POINT_BITS)) | kp;
}

}  // namespace tn
