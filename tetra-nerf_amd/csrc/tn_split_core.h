// tn_split_core.h -- the per-tetrahedron and per-vertex rule of the 1 -> 4 tetrahedron split at the centroid (tn_split_count /
// tn_split_emit / tn_split_vertex_rows), written once for the kernels (tn_split.hip) and the CPU emulation
// (tests/host/split_emul.cpp), the way tn_isosurface_core.h states the extraction.  The same statement in numpy: geometry.py
// (split_tetrahedra_statement, split_vertex_rows_statement).
//
// The rule.  xyz f32 [V, 3], cells u32 [T, 4], select u8 [T] (non-zero = asked).
//   ACCEPTANCE.  Tetrahedron t is accepted iff it is asked, its four ids are < V (decided before any read of xyz), the
//   orientation s = guard::tet_orient(p) of its stored row is not 0 (0 also for NaN), and every one of its four children has
//   that same orientation s.  Child i is the stored row with slot i replaced by the centroid, so where the arithmetic were exact
//   a child has its parent's orientation as stored; it does not where the fp32 centroid rounds onto or across a face.  About
//   half of all stored rows are negative: the children are compared with the PARENT'S sign, not with "positive".
//   CENTROID.  Per coordinate c = ((p0 + p1) + (p2 + p3)) * 0.25f in fp32, one rounding per operation in this order, no fused
//   multiply-add.
//   NUMBERING.  k = the accepted tetrahedra with an id below t (an exclusive sum), K = their total.  The new vertex is V + k;
//   child 0 overwrites row t; children 1, 2, 3 are rows T + 3 k, T + 3 k + 1, T + 3 k + 2.  cell_parent[row] = row for a row < T
//   and the parent's id for an appended row; vertex_parents[k] = the parent's row as stored.
//   COUNTERS u32 [4]: asked, accepted, refused for a flat or inverted parent or child, refused for an id >= V.
//   A NEW PER-VERTEX VALUE is the centroid's expression on the four parents' values: ((x[a] + x[b]) + (x[c] + x[d])) * 0.25f with
//   (a, b, c, d) = vertex_parents[k].
#pragma once
#include <cstdint>

#include "tn_isosurface_core.h"   // iso::fadd / iso::fmul: one rounding per operation on both sides; guard::tet_orient

namespace tn {
namespace split {

constexpr uint64_t MAX_CELLS = 1ull << 30;   // T + 3 K must be below it (the limit of every per-tetrahedron table)
constexpr uint32_t MODE_MEAN = 0, MODE_ZERO = 1;

enum Verdict : uint32_t {
    NOT_ASKED = 0,
    ACCEPTED = 1,
    REFUSED_FLAT = 2,   // the parent or a child is flat, inverted against the parent, or has a NaN coordinate
    REFUSED_ID = 3,     // an id >= V
};

// ((a + b) + (c + d)) * 0.25f: the centroid's coordinate and the new per-vertex value
TN_HD float mean4(float a, float b, float c, float d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return iso::fmul(iso::fadd(iso::fadd(a, b), iso::fadd(c, d)), 0.25f);
}

TN_HD void centroid(const float p[4][3], float c[3]) {
    for (int a = 0; a < 3; ++a) c[a] = mean4(p[0][a], p[1][a], p[2][a], p[3][a]);
}

// the verdict on an ASKED tetrahedron whose ids are < V: p = its four positions in stored order; cen receives the centroid
TN_HD Verdict judge_positions(const float p[4][3], float cen[3]) {
    const int s = guard::tet_orient(p);
    centroid(p, cen);
    if (s == 0) return REFUSED_FLAT;
    for (int i = 0; i < 4; ++i) {
        float q[4][3];
        for (int j = 0; j < 4; ++j)
            for (int a = 0; a < 3; ++a) q[j][a] = j == i ? cen[a] : p[j][a];
        if (guard::tet_orient(q) != s) return REFUSED_FLAT;
    }
    return ACCEPTED;
}

// the verdict on tetrahedron row c; xyz is read only where the row is asked and its ids are < V
TN_HD Verdict judge(bool asked, const uint32_t c[4], uint32_t V, const float *xyz, float cen[3]) {
    if (!asked) return NOT_ASKED;
    if (!iso::ids_ok(c, V)) return REFUSED_ID;
    float p[4][3];
    for (int j = 0; j < 4; ++j)
        for (int a = 0; a < 3; ++a) p[j][a] = xyz[3 * (size_t)c[j] + a];
    return judge_positions(p, cen);
}

// child i of row c with the new vertex id v: slot i replaced, the other three in their stored order
TN_HD void child_row(const uint32_t c[4], int i, uint32_t v, uint32_t out[4]) {
    for (int j = 0; j < 4; ++j) out[j] = j == i ? v : c[j];
}

// the row of child i of the k-th accepted tetrahedron t
TN_HD size_t child_slot(size_t T, size_t t, size_t k, int i) { return i == 0 ? t : T + 3 * k + (size_t)(i - 1); }

}  // namespace split
}  // namespace tn
