// tn_vertex_guard_core.h -- the per-element arithmetic of the vertex step limiter (tn_tet_quality, tn_limit_vertex_step), written
// once for the kernels (tn_vertex_guard.hip) and the CPU emulation (tests/host/vertex_guard_emul.cpp), the way tn_build_core.h
// states the build.  The same statements in torch: geometry.py (tet_width_orient, star_width, limit_vertex_step_statement).
//
// The rule.  The WIDTH w of a tetrahedron -- its smallest extent over all directions -- is attained
// on one of seven slabs: the four heights and the three distances between opposite edges.  If every vertex of a tetrahedron
// moves by less than w / 2, the four points are coplanar at no fraction of the straight move, so the signed volume keeps its
// sign.  star_w[v] = the smallest fl32(w) over the tetrahedra around v; a vertex may move by fraction * star_w[v], fraction
// <= 0.45; a vertex whose star_w is below 2^-17 of its largest |coordinate| does not move at all (the rounding of the new
// coordinates would no longer be a small part of the budget).
#pragma once
#include <cstdint>
#include <cstring>
#include <cmath>

#if !defined(TN_HD)
#if defined(__HIPCC__)
#define TN_HD __host__ __device__ __forceinline__
#else
#define TN_HD inline
#endif
#endif

namespace tn {
namespace guard {

constexpr float MAX_FRACTION = 0.45f;            // the proof needs 0.45 (1 + 2^-20) + 1/32 < 1/2
constexpr float FREEZE_RATIO = 1.0f / 131072.f;  // 2^-17: star_w below this part of max |coordinate| freezes the vertex
constexpr uint32_t INF_BITS = 0x7F800000u;       // star_w of a vertex no tetrahedron names

enum Kind : int {
    KEPT = 0,           // within the limit: the new position stays, bit for bit
    CLAMPED = 1,        // moved too far, or to a non-finite place: shortened to the limit (or back to the old position)
    FROZEN_MOVED = 2,   // frozen and asked to move: back to the old position
    FROZEN_STILL = 3,   // frozen and not asked to move
};

struct WidthOrient { uint32_t width_bits; int orient; };

TN_HD uint32_t f32_bits(float x) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(x);
#else
    std::memcpy(&u, &x, 4);
#endif
    return u;
}

// sign of ((p1-p0) x (p2-p0)) . (p3-p0) in double on the fp32 coordinates: -1, 0 (also for NaN), 1; *vol6_out = the volume
TN_HD int tet_orient(const float p[4][3], double *vol6_out = nullptr) {
    // every product rounds once on every build (tn_build_core.h: tet_min_height_bits says why)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double e1[3], e2[3], e3[3];
    for (int a = 0; a < 3; ++a) {
        e1[a] = (double)p[1][a] - (double)p[0][a]; e2[a] = (double)p[2][a] - (double)p[0][a]; e3[a] = (double)p[3][a] - (double)p[0][a];
    }
    const double n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2], n2 = e1[0] * e2[1] - e1[1] * e2[0];
    const double vol6 = (n0 * e3[0] + n1 * e3[1]) + n2 * e3[2];
    if (vol6_out) *vol6_out = vol6;
    return vol6 > 0.0 ? 1 : (vol6 < 0.0 ? -1 : 0);
}

// width (as fp32 bits; 0 for anything that is not 0 <= w < inf) and orientation of one tetrahedron
TN_HD WidthOrient tet_width_orient(const float p[4][3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double vol6;
    const int orient = tet_orient(p, &vol6);
    double q[4][3];
    for (int i = 0; i < 4; ++i) for (int a = 0; a < 3; ++a) q[i][a] = (double)p[i][a];
    // |(q[b]-q[a]) x (q[d]-q[c])|: faces (a = c: two edges from one corner) and pairs of opposite edges
    const int s[7][4] = {{1, 2, 1, 3}, {0, 2, 0, 3}, {0, 1, 0, 3}, {0, 1, 0, 2}, {0, 1, 2, 3}, {0, 2, 1, 3}, {0, 3, 1, 2}};
    double den = 0.0;
    for (int k = 0; k < 7; ++k) {
        double u[3], v[3];
        for (int a = 0; a < 3; ++a) { u[a] = q[s[k][1]][a] - q[s[k][0]][a]; v[a] = q[s[k][3]][a] - q[s[k][2]][a]; }
        const double w0 = u[1] * v[2] - u[2] * v[1], w1 = u[2] * v[0] - u[0] * v[2], w2 = u[0] * v[1] - u[1] * v[0];
        const double n = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
        den = n > den ? n : den;
    }
    const double w = den > 0.0 ? fabs(vol6) / den : 0.0;
    float wf = (float)w;
    if (!(wf >= 0.f && wf < INFINITY)) wf = 0.f;
    return WidthOrient{f32_bits(wf), orient};
}

TN_HD bool vertex_frozen(float star_w, const float old_[3]) {
    float m = fabsf(old_[0]);
    const float ay = fabsf(old_[1]), az = fabsf(old_[2]);
    m = ay > m ? ay : m;
    m = az > m ? az : m;
    return !(star_w >= FREEZE_RATIO * m);
}

// One vertex of the clamp, fp32, every operation rounded once and in this order (geometry.limit_vertex_step_statement).
// `check_range` = false lifts the freeze rule (the tests' power case: the same step clamped to a whole width).
TN_HD void clamp_vertex(const float old_[3], const float new_[3], float star_w, float fraction, float out[3], int *kind,
                        bool check_range = true) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (check_range && vertex_frozen(star_w, old_)) {
        const bool asked = new_[0] != old_[0] || new_[1] != old_[1] || new_[2] != old_[2];
        for (int a = 0; a < 3; ++a) out[a] = old_[a];
        *kind = asked ? FROZEN_MOVED : FROZEN_STILL;
        return;
    }
    const float dx = new_[0] - old_[0], dy = new_[1] - old_[1], dz = new_[2] - old_[2];
    const float n = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float lim = fraction * star_w;
    const bool finite = n < INFINITY;   // false for NaN
    if (finite && n <= lim) {
        for (int a = 0; a < 3; ++a) out[a] = new_[a];
        *kind = KEPT;
        return;
    }
    const float s = lim / n;
    out[0] = finite ? old_[0] + dx * s : old_[0];
    out[1] = finite ? old_[1] + dy * s : old_[1];
    out[2] = finite ? old_[2] + dz * s : old_[2];
    *kind = CLAMPED;
}

}  // namespace guard
}  // namespace tn
