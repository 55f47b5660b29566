// tn_isosurface_core.h -- the per-tetrahedron and per-edge rule of the isosurface extraction (tn_isosurface_count /
// tn_isosurface_emit), written once for the kernels (tn_isosurface.hip) and the CPU emulation (tests/host/isosurface_emul.cpp),
// the way tn_delaunay_core.h states the monitor.  The same statement in numpy: geometry.py (isosurface_statement).  Below it, the
// per-vertex rule of the refinement (tn_isosurface_refine_*), in the same three places.
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

// ---------------------------------------------------------------------------------------------------------------------------
// The REFINEMENT of the surface vertices (tn_isosurface_refine_*, tn_isosurface_refine.hip; the emulation:
// tests/host/isosurface_refine_emul.cpp; in numpy: geometry.isosurface_refine_statement).  The topology
// stays what the extraction emitted; every welded vertex moves along its own mesh edge (a, b), a < b, to a crossing of a density
// the CALLER evaluates on that edge at the parameters asked for -- the network, where the extraction assumed a straight line.
//   STATE per vertex: a bracket (t_lo, t_hi, s_lo, s_hi), 16 bytes, and a flag byte.  It starts as (0, 1, values[a], values[b]),
//   flag 0.  The two ends differ in inside(s) = s >= level, and every round keeps that.
//   A ROUND: w = t_hi - t_lo and C = 7 candidates t_j = t_lo + (float(j) * 0.125f) * w, j = 1..7.  The caller evaluates s_j at
//   t_j.  With (t_0, s_0) = (t_lo, s_lo) and (t_8, s_8) = (t_hi, s_hi) the new bracket is (t_j, t_j+1, s_j, s_j+1) for the FIRST j
//   in 0..7 whose ends differ in `inside`: the crossing nearest a.  One exists, because the old ends differ.  If one of the
//   seven s_j is not in_range (not finite, or >= 2^126 in magnitude) the edge is FROZEN: flag REFINE_FROZEN, the bracket stays as
//   it is in this and every later round.
//   ORDER: t_lo <= t_1 <= ... <= t_7 <= t_hi for every 0 <= t_lo <= t_hi <= 1.  Proof.  j / 8 is exact and rounding is monotone,
//   so m_j = fl(j/8 * w) is non-negative and does not decrease with j, and neither does t_j = fl(t_lo + m_j) >= fl(t_lo) = t_lo.
//   For the upper end let d = t_hi - t_lo exactly.  If d is a float then w = d and m_7 = fl(7/8 w) <= fl(w) = d.  If it is not,
//   then d >= 2^-125 (a difference of floats below that is a multiple of 2^-149 with at most 24 bits, hence a float), w <= d (1 + u)
//   with u = 2^-24, the product is normal and m_7 <= 7/8 d (1 + u)^2 < d.  Either way t_lo + m_7 <= t_hi exactly, and rounding it
//   cannot pass the float t_hi.
//   THE VERTEX: q = (level - s_lo) / (s_hi - s_lo), t = t_lo + q (t_hi - t_lo), put back into [t_lo, t_hi] (it leaves it only
//   where the ends do not differ in `inside` -- an edge that started frozen -- and then stays on the edge; a NaN goes to t_lo),
//   p = xyz[a] + t (xyz[b] - xyz[a]): edge_vertex on the last bracket.  Where t_lo is 0 the
//   sum is not formed, t = q (t_hi - t_lo): 0 + m = m but for the sign of a zero m, which edge_vertex keeps (s_lo == level with a
//   inside gives q = -0).  After no round the bracket is (0, 1, values[a], values[b]), q * 1 = q, and t and p ARE edge_vertex's.
//   An edge whose ids are not both < V gets flag REFINE_BAD_IDS, the bracket (0, 1, 0, 0), candidates on edge (0, 0), and
//   t = 0, p = 0, as the extraction writes it.  An edge whose two values are not in range, or lie on one side of the level (the
//   caller changed `values` since the extraction), starts FROZEN.
constexpr int REFINE_CANDIDATES = 7;        // C: candidates per vertex and round, at j/8 of the bracket
constexpr uint32_t REFINE_MAX_ROUNDS = 8;   // 8^-8 = 2^-24: the bracket is an ulp of t = 1 wide
constexpr uint8_t REFINE_FROZEN = 1, REFINE_BAD_IDS = 2;

struct Bracket { float t_lo, t_hi, s_lo, s_hi; };

TN_HD bool inside(float s, float level) { return s >= level; }

// the state of the vertex on mesh edge (a, b) before the first round; values is read only where both ids are < V
TN_HD uint8_t refine_begin(uint32_t a, uint32_t b, uint32_t V, const float *values, float level, Bracket &br) {
    br = Bracket{0.f, 1.f, 0.f, 0.f};
    if (!(a < V && b < V)) return REFINE_BAD_IDS;
    br.s_lo = values[a];
    br.s_hi = values[b];
    const bool ok = in_range(br.s_lo) && in_range(br.s_hi) && inside(br.s_lo, level) != inside(br.s_hi, level);
    return ok ? (uint8_t)0 : REFINE_FROZEN;
}

// candidate j = 1 .. REFINE_CANDIDATES of the bracket [t_lo, t_hi]
TN_HD float refine_candidate(float t_lo, float t_hi, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return fadd(t_lo, fmul((float)j * 0.125f, fsub(t_hi, t_lo)));
}

// one round: s[j - 1] = the density at refine_candidate(j).  Returns the new flag; br changes only where it returns 0.
TN_HD uint8_t refine_select(Bracket &br, const float s[REFINE_CANDIDATES], float level, uint8_t flag) {
    if (flag) return flag;
    for (int j = 0; j < REFINE_CANDIDATES; ++j)
        if (!in_range(s[j])) return REFINE_FROZEN;
    const Bracket old = br;
    float t_prev = old.t_lo, s_prev = old.s_lo;
    for (int j = 1; j <= REFINE_CANDIDATES + 1; ++j) {
        const float t_next = j <= REFINE_CANDIDATES ? refine_candidate(old.t_lo, old.t_hi, j) : old.t_hi;
        const float s_next = j <= REFINE_CANDIDATES ? s[j - 1] : old.s_hi;
        if (inside(s_prev, level) != inside(s_next, level)) {
            br = Bracket{t_prev, t_next, s_prev, s_next};
            return 0;
        }
        t_prev = t_next;
        s_prev = s_next;
    }
    return REFINE_FROZEN;   // both ends on one side: not reached from refine_begin's flag 0
}

// the vertex of a bracket: edge_vertex on (t_lo, t_hi, s_lo, s_hi) in the place of (0, 1, va, vb)
TN_HD float refine_vertex(const Bracket &br, float level, const float xa[3], const float xb[3], float p[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float q = fdiv(fsub(level, br.s_lo), fsub(br.s_hi, br.s_lo));
    const float m = fmul(q, fsub(br.t_hi, br.t_lo));
    float t = br.t_lo == 0.f ? m : fadd(br.t_lo, m);
    t = !(t >= br.t_lo) ? br.t_lo : (t > br.t_hi ? br.t_hi : t);
    for (int k = 0; k < 3; ++k) p[k] = fadd(xa[k], fmul(t, fsub(xb[k], xa[k])));
    return t;
}

}  // namespace iso
}  // namespace tn
