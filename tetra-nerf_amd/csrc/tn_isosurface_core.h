// tn_isosurface_core.h -- the per-tetrahedron and per-edge rule of the isosurface extraction (tn_isosurface_count /
// tn_isosurface_emit), written once for the kernels (tn_isosurface.hip) and the CPU emulation (tests/host/isosurface_emul.cpp),
// the way tn_delaunay_core.h states the monitor.  The same statement in numpy: geometry.py (isosurface_statement).
//
// The rule.  The surface is the level set of the piecewise-linear interpolant of a per-vertex scalar
// over a tetrahedron soup: marching tetrahedra.
//   inside(v) = values[v] >= level.
//   A tetrahedron is SKIPPED (emits nothing) if its mask byte is 0, an id is >= V, or one of its four values is not finite or is
//   at least 2^126 in magnitude (with |level| < 2^126 no difference below overflows).
//   The six tet edges are 0..5 = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3) in stored corner order; an edge CROSSES if its ends
//   differ in `inside`.  Three crossing edges give one triangle, four give two, anything else nothing: TRI_TABLE, indexed by the
//   inside code (bit k = corner k is inside), names the tet edges of each triangle.  The table is written for a tetrahedron of
//   non-negative orientation (guard::tet_orient, 0 counts as positive) so that (q1-q0) x (q2-q0) points towards values < level;
//   for a negative orientation corners 1 and 2 of every triangle are swapped.
//   A surface vertex belongs to a MESH edge (a, b), a < b as global ids, key = a << 32 | b, and is computed from the SORTED pair
//   whichever way a tetrahedron stores it, so every tetrahedron around the edge sees the same bits:
//       t = (level - values[a]) / (values[b] - values[a]),      p_k = xyz[a][k] + t (xyz[b][k] - xyz[a][k])
//   in fp32, one rounding per operation, no fused multiply-add.  The ends differ in `inside`, so the denominator is not 0 and,
//   rounding being monotone, t is in [0, 1].  A value equal to `level` is inside: t = 0 (or 1) and the endpoint itself.
#pragma once
#include <cstdint>
#include <cmath>

#include "tn_vertex_guard_core.h"

namespace tn {
namespace iso {

constexpr float VALUE_LIMIT = 8.507059173023462e37f;   // 2^126: values and level must be below it in magnitude
constexpr uint64_t MAX_TETS = 1ull << 30;              // T must be below it: 4 T edge references fit 32 bits

// the two corners of tet edge e
constexpr int EDGE_CORNERS[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};

// TRI_TABLE[code][row][k]: tet edge k of triangle `row` for the inside code (bit c = corner c inside); -1 = no triangle
constexpr int8_t TRI_TABLE[16][2][3] = {
    {{-1, -1, -1}, {-1, -1, -1}},   // 0000
    {{ 0,  1,  2}, {-1, -1, -1}},   // 0001
    {{ 0,  4,  3}, {-1, -1, -1}},   // 0010
    {{ 1,  2,  4}, { 1,  4,  3}},   // 0011
    {{ 1,  3,  5}, {-1, -1, -1}},   // 0100
    {{ 0,  3,  5}, { 0,  5,  2}},   // 0101
    {{ 0,  4,  5}, { 0,  5,  1}},   // 0110
    {{ 2,  4,  5}, {-1, -1, -1}},   // 0111
    {{ 2,  5,  4}, {-1, -1, -1}},   // 1000
    {{ 0,  1,  5}, { 0,  5,  4}},   // 1001
    {{ 0,  2,  5}, { 0,  5,  3}},   // 1010
    {{ 1,  5,  3}, {-1, -1, -1}},   // 1011
    {{ 1,  3,  4}, { 1,  4,  2}},   // 1100
    {{ 0,  3,  4}, {-1, -1, -1}},   // 1101
    {{ 0,  2,  1}, {-1, -1, -1}},   // 1110
    {{-1, -1, -1}, {-1, -1, -1}},   // 1111
};

// finite and below 2^126 in magnitude (false for NaN): what `level` and every value of an emitting tetrahedron must be
TN_HD bool in_range(float v) { return fabsf(v) < VALUE_LIMIT; }

// what both passes need to know of one tetrahedron
struct TetCase {
    uint32_t code;     // inside code, 0 for a skipped tetrahedron
    uint32_t cross;    // bit e = tet edge e crosses
    uint32_t ntri;     // 0, 1, 2
    uint32_t nref;     // 0, 3, 4 = popcount(cross)
};

// the classification of a tetrahedron that is not skipped for its mask or ids: v = its four values in stored corner order
TN_HD TetCase classify(const float v[4], float level) {
    TetCase c{0u, 0u, 0u, 0u};
    if (!(in_range(v[0]) && in_range(v[1]) && in_range(v[2]) && in_range(v[3]))) return c;
    for (int k = 0; k < 4; ++k) c.code |= (uint32_t)(v[k] >= level) << k;
    for (int e = 0; e < 6; ++e)
        c.cross |= (((c.code >> EDGE_CORNERS[e][0]) ^ (c.code >> EDGE_CORNERS[e][1])) & 1u) << e;
    c.ntri = (TRI_TABLE[c.code][0][0] >= 0) + (TRI_TABLE[c.code][1][0] >= 0);
    c.nref = c.ntri ? c.ntri + 2 : 0;
    return c;
}

// skipped for its ids (the mask is the caller's test: it is read before anything else)
TN_HD bool ids_ok(const uint32_t c[4], uint32_t V) { return c[0] < V && c[1] < V && c[2] < V && c[3] < V; }

// position of tet edge e among the crossing edges of its tetrahedron, in tet-edge order
TN_HD uint32_t edge_rank(uint32_t cross, int e) {
    uint32_t below = cross & ((1u << e) - 1u), n = 0;
    for (int k = 0; k < 5; ++k) n += (below >> k) & 1u;
    return n;
}

// the welding key of the mesh edge between global ids u and w
TN_HD uint64_t edge_key(uint32_t u, uint32_t w) {
    const uint32_t a = u < w ? u : w, b = u < w ? w : u;
    return (uint64_t)a << 32 | b;
}

// one rounding per operation on both sides (the device intrinsics are these operations; contraction is off either way)
TN_HD float fsub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
TN_HD float fadd(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}
TN_HD float fmul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}
TN_HD float fdiv(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

// the surface vertex of the mesh edge (a, b), a < b: va / vb their values, xa / xb their positions
TN_HD float edge_vertex(float va, float vb, float level, const float xa[3], const float xb[3], float p[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t = fdiv(fsub(level, va), fsub(vb, va));
    for (int k = 0; k < 3; ++k) p[k] = fadd(xa[k], fmul(t, fsub(xb[k], xa[k])));
    return t;
}

// the corner order of triangle `row`: corners 1 and 2 change places in a tetrahedron of negative orientation
TN_HD int tri_corner(int k, bool negative) { return negative && k ? 3 - k : k; }

}  // namespace iso
}  // namespace tn
