// tn_flip_core.h -- the per-face rule of the Delaunay REPAIR by bistellar flips (tn_flip_count / tn_flip_count_tables /
// tn_flip_emit): a certainly violated interior face is removed by a 2-3 flip (its two tetrahedra become three around the new edge)
// or by a 3-2 flip (three tetrahedra around a reflex edge become two).  Written once for the kernels (tn_flip.hip) and the CPU
// emulation (tests/host/flip_emul.cpp), the way tn_edge_split_core.h states the edge split.  The same statement in numpy:
// geometry.py (flip_faces_statement).  No vertex is added or moved.
//
// The rule.  xyz f32 [V, 3], cells u32 [T, 4], the face table faces u32 [F, 3] and face_tets u32 [F, 2] of
// the cells (a hull face has face_tets[f, 1] == 0xFFFFFFFF).  Every sign is the sign of delaunay::orient_det or insphere_det, and
// it is CERTAIN iff |det| > bound * permanent (tn_delaunay_core.h): no new arithmetic.
//   TET_FACES u32 [T, 4].  tet_faces[t, j] = the face that names every id of row t but the one in slot j: face f writes its own id
//   into slot(t0) and slot(t1), slot(t) = the first slot of row t whose id is not one of faces[f] (none: nothing is written).
//   FACE f, interior (t1 != EMPTY): (a, b, c) = faces[f] as stored, t0, t1 = face_tets[f], d = the id in slot(t0) of row t0, e =
//   the id in slot(t1) of row t1.
//   REFUSALS, the first that holds, in this order:
//     ID           t0 or t1 >= T, or a, b, c or an id of row t0 or t1 is >= V, or row t0 or t1 has no slot.  Decided before any
//                  read of xyz; such a face has no verdict.
//     (verdict)    delaunay::face_verdict(row t0 in stored order, opposite_vertex(row t0, row t1)) -- tn_delaunay_check's own call.
//                  REGULAR and UNCERTAIN faces are no candidates; VIOLATED ones are.
//     INVALID      O(a,b,c,d) or O(a,b,c,e) is uncertain, or they have the same sign: d and e are not on opposite sides.
//     UNCERTAIN    one of o_k = O(x_k, y_k, d, e) is uncertain, (x_k, y_k) = (a,b), (b,c), (c,a) for k = 0, 1, 2 (the 4-4
//                  configuration, d, e and an edge of the face in one plane, lands here).
//     UNFLIPPABLE  o_k is GOOD iff it has the sign of O(a,b,c,e) -- the sign all three have when the segment de crosses the inside
//                  of abc.  Three good: a 2-3 flip with the rows {t0, t1}.  Two good, one bad k: a 3-2 flip, flippable iff one row
//                  t2 is the neighbour of t0 across the face opposite z and the neighbour of t1 across the face opposite z (z = the
//                  id of (a, b, c) that is not x_k, y_k; the neighbours through tet_faces and face_tets) and holds x_k, y_k, d, e.
//                  Otherwise, and with fewer than two good, unflippable.
//     LOST         every flippable candidate claims its 2 or 3 rows; the winner of a row is the smallest claiming face id; a
//                  candidate that does not win every one of its rows is lost.
//   Otherwise the candidate is ACCEPTED.  Accepted flips share no row.
//   CHILDREN.  For every good k in ascending order the row (x_k, y_k, d, e) in that slot order: all have the sign of O(a,b,c,e).
//   NUMBERING.  Child 0 takes the place of t0, child 1 that of t1.  The place of t2 (3-2) is deleted: the new position of an old
//   row is tet_offsets[t], the exclusive sums of "row t is not a deleted t2".  Child 2 (2-3) is appended at (T - K32) + its rank
//   among the accepted 2-3 flips in ascending face id.  T' = T + K23 - K32.
//   CELL_SOURCES u32 [T', 3]: (t, EMPTY, EMPTY) for a copied row, (t0, t1, EMPTY) for the children of a 2-3 flip, (t0, t1, t2)
//   for those of a 3-2 flip: the old rows whose union holds the new one.
//   FACE_FLIP u32 [F, 3] = (code, t2, rank): (NONE, EMPTY, EMPTY) for a face that is not accepted, (FLIP23, EMPTY, rank among the
//   accepted 2-3 flips) or (FLIP32 + bad k, t2, EMPTY) for one that is.  TET_FLIP u32 [T] = the accepted face that claimed the row,
//   EMPTY for an untouched row; FLIPPED u8 [T] = tet_flip != EMPTY.
//   COUNTERS u32 [10]: interior faces, violated, verdict uncertain, refused id / invalid / uncertain / unflippable / lost, accepted
//   2-3 flips K23, accepted 3-2 flips K32.  violated = the sum of the last seven but refused id.
#pragma once
#include <cstddef>
#include <cstdint>

#include "tn_delaunay_core.h"

namespace tn {
namespace flip {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint64_t MAX_CELLS = 1ull << 30;   // T + K23 must be below it
constexpr int NUM_COUNTERS = 10;
enum Counter : int {
    INTERIOR = 0, VIOLATED = 1, VERDICT_UNCERTAIN = 2, REFUSED_ID = 3, REFUSED_INVALID = 4, REFUSED_UNCERTAIN = 5,
    REFUSED_UNFLIPPABLE = 6, REFUSED_LOST = 7, ACCEPTED_23 = 8, ACCEPTED_32 = 9,
};
// what a face is, before the precedence among candidates is decided
enum Kind : uint32_t {
    NONE = 0,        // hull, regular or verdict-uncertain (face_flip's code of every face that is not accepted, too)
    FLIP23 = 1,      // flippable 2-3
    FLIP32 = 2,      // flippable 3-2: FLIP32 + the bad k (2, 3, 4)
    K_HULL = 8, K_REGULAR = 9, K_VERDICT_UNCERTAIN = 10, K_ID = 11, K_INVALID = 12, K_UNCERTAIN = 13, K_UNFLIPPABLE = 14,
};

// the first slot of row c whose id is not one of the face's three; -1 where every slot is
TN_HD int apex_slot(const uint32_t c[4], const uint32_t f[3]) {
    for (int j = 0; j < 4; ++j)
        if (c[j] != f[0] && c[j] != f[1] && c[j] != f[2]) return j;
    return -1;
}

// +1 / -1 where the sign of the orientation determinant of (q0, q1, q2, q3) is certain, 0 where it is not (NaN too)
TN_HD int orient_sign(const float *q0, const float *q1, const float *q2, const float *q3) {
    float p[4][3];
    for (int a = 0; a < 3; ++a) { p[0][a] = q0[a]; p[1][a] = q1[a]; p[2][a] = q2[a]; p[3][a] = q3[a]; }
    const delaunay::Det o = delaunay::orient_det(p);
    if (!(fabs(o.det) > delaunay::ORIENT_BOUND * o.perm)) return 0;
    return o.det > 0.0 ? 1 : -1;
}

struct Face {
    uint32_t kind;     // K_* or FLIP23, or FLIP32 + bad k BEFORE t2 is looked up (find_t2 turns it into K_UNFLIPPABLE)
    uint32_t d, e;     // the two apices (valid unless kind is K_HULL or K_ID)
};

// Everything of the rule that reads positions: the kind of interior face (a, b, c) = f between the rows c0 = cells[t0] and c1 =
// cells[t1].  The caller has checked t0, t1 < T.  xyz is read only after every id is known to be < V.
TN_HD Face judge_face(const uint32_t f[3], const uint32_t c0[4], const uint32_t c1[4], uint32_t V, const float *xyz) {
    Face r{K_ID, EMPTY, EMPTY};
    const int s0 = apex_slot(c0, f), s1 = apex_slot(c1, f);
    bool ok = s0 >= 0 && s1 >= 0 && f[0] < V && f[1] < V && f[2] < V;
    for (int j = 0; j < 4; ++j) ok = ok && c0[j] < V && c1[j] < V;
    if (!ok) return r;
    r.d = c0[s0];
    r.e = c1[s1];
    float p[4][3];
    for (int j = 0; j < 4; ++j)
        for (int a = 0; a < 3; ++a) p[j][a] = xyz[3 * (size_t)c0[j] + a];
    const uint32_t ev = delaunay::opposite_vertex(c0, c1);
    const delaunay::Verdict v = delaunay::face_verdict(p, xyz + 3 * (size_t)ev);
    if (v.state != delaunay::VIOLATED) {
        r.kind = v.state == delaunay::REGULAR ? K_REGULAR : K_VERDICT_UNCERTAIN;
        return r;
    }
    const float *pa = xyz + 3 * (size_t)f[0], *pb = xyz + 3 * (size_t)f[1], *pc = xyz + 3 * (size_t)f[2];
    const float *pd = xyz + 3 * (size_t)r.d, *pe = xyz + 3 * (size_t)r.e;
    const int sd = orient_sign(pa, pb, pc, pd), se = orient_sign(pa, pb, pc, pe);
    if (sd == 0 || se == 0 || sd == se) { r.kind = K_INVALID; return r; }
    const int o0 = orient_sign(pa, pb, pd, pe), o1 = orient_sign(pb, pc, pd, pe), o2 = orient_sign(pc, pa, pd, pe);
    if (o0 == 0 || o1 == 0 || o2 == 0) { r.kind = K_UNCERTAIN; return r; }
    const int good = (o0 == se) + (o1 == se) + (o2 == se);
    if (good == 3) r.kind = FLIP23;
    else if (good == 2) r.kind = FLIP32 + (o0 != se ? 0u : o1 != se ? 1u : 2u);
    else r.kind = K_UNFLIPPABLE;
    return r;
}

// The third row of a 3-2 candidate with the bad edge k: the neighbour of t0 and of t1 across their faces opposite z = f[(k + 2) % 3],
// where both are the same row and that row holds x_k, y_k, d, e; EMPTY otherwise.  Every index is checked before it is an address.
TN_HD uint32_t find_t2(const uint32_t f[3], int k, uint32_t d, uint32_t e, uint32_t t0, uint32_t t1, const uint32_t c0[4],
                       const uint32_t c1[4], size_t T, size_t F, const uint32_t *cells, const uint32_t *face_tets,
                       const uint32_t *tet_faces) {
    const uint32_t z = f[(k + 2) % 3], x = f[k], y = f[(k + 1) % 3];
    uint32_t n[2];
    for (int side = 0; side < 2; ++side) {
        const uint32_t *c = side ? c1 : c0;
        const uint32_t t = side ? t1 : t0;
        int slot = -1;
        for (int j = 3; j >= 0; --j)
            if (c[j] == z) slot = j;
        if (slot < 0) return EMPTY;
        const uint32_t g = tet_faces[4 * (size_t)t + slot];
        if (g >= F) return EMPTY;
        const uint32_t u = face_tets[2 * (size_t)g], w = face_tets[2 * (size_t)g + 1];
        n[side] = u == t ? w : (w == t ? u : EMPTY);
    }
    if (n[0] != n[1] || n[0] >= T || n[0] == t0 || n[0] == t1) return EMPTY;
    const uint32_t *c2 = cells + 4 * (size_t)n[0];
    int have = 0;
    for (int j = 0; j < 4; ++j) have |= (c2[j] == x ? 1 : 0) | (c2[j] == y ? 2 : 0) | (c2[j] == d ? 4 : 0) | (c2[j] == e ? 8 : 0);
    return have == 15 ? n[0] : EMPTY;
}

// the good k of an accepted code, ascending; returns their number (3 for FLIP23, 2 for FLIP32 + bad k, 0 otherwise)
TN_HD int good_edges(uint32_t code, int ks[3]) {
    if (code == FLIP23) { ks[0] = 0; ks[1] = 1; ks[2] = 2; return 3; }
    if (code >= FLIP32 && code < FLIP32 + 3) {
        const int bad = (int)(code - FLIP32);
        int n = 0;
        for (int k = 0; k < 3; ++k)
            if (k != bad) ks[n++] = k;
        ks[2] = -1;
        return 2;
    }
    return 0;
}

// the child of good edge k: (x_k, y_k, d, e)
TN_HD void child_row(const uint32_t f[3], int k, uint32_t d, uint32_t e, uint32_t out[4]) {
    out[0] = f[k];
    out[1] = f[(k + 1) % 3];
    out[2] = d;
    out[3] = e;
}

}  // namespace flip
}  // namespace tn
