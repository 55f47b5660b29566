// tn_edge_split_core.h -- the per-tetrahedron, per-face and per-edge rule of the EDGE split (tn_edge_split_count /
// tn_edge_split_count_tables / tn_edge_split_emit): selected edges are bisected at their midpoints together with every
// tetrahedron around them.  Written once for the kernels (tn_edge_split.hip) and the CPU emulation
// (tests/host/edge_split_emul.cpp), the way tn_split_core.h states the centroid split.  The same statement in numpy: geometry.py
// (split_edges_statement).
//
// The rule.  xyz f32 [V, 3], cells u32 [T, 4] (any soup), select u8 [T] (non-zero = asked), the face table
// faces u32 [F, 3] and face_tets u32 [F, 2] of the cells (a hull face has face_tets[f, 1] == 0xFFFFFFFF).
//   EDGE.  The sorted id pair (lo, hi), lo < hi, key = lo << 32 | hi.  Its squared length is taken from the SORTED pair,
//   d = p[hi] - p[lo] per coordinate, (dx dx + dy dy) + dz dz in fp32, one rounding per operation, no fused multiply-add: every
//   tetrahedron around an edge sees the same bits.  Edge e BEATS f iff len2(e) > len2(f), or they are equal and key(e) < key(f).
//   The BEST of a list of edges is a fold in the list's order: the first edge, replaced by each later one that beats it (where no
//   length is NaN this is the maximum of a total order and the order of the list does not matter).
//   CANDIDATES.  An asked tetrahedron whose four ids are < V (decided before any read of xyz) and whose stored orientation
//   s = guard::tet_orient is not 0 nominates the best of its six edges, in tet-edge order (iso::EDGE_CORNERS).  The candidates are
//   the distinct nominated keys, in ascending order.
//   RING.  The ring of a candidate is every row of cells that holds both its ids.  The WINNER of a row is the best of the
//   candidates among its six edges, in tet-edge order, or none.
//   REFUSALS.  A candidate is refused for the first of these that holds:  ID a ring row has an id >= V;  HULL the edge is an edge of
//   a hull face;  LOST the winner of some ring row is another edge;  FLAT some ring row has orientation 0, or one of its two
//   children has not the row's own orientation s.  Otherwise it is ACCEPTED.  Two accepted edges share no row: a row has one winner.
//   MIDPOINT.  Per coordinate split::mean4(p_lo, p_hi, p_lo, p_hi) = ((a + b) + (a + b)) * 0.25f, and vertex_parents =
//   (lo, hi, lo, hi): tn_split_vertex_rows carries the per-vertex arrays with the same expression.
//   NUMBERING.  Accepted edges are ranked j = 0 .. K_v - 1 in ascending key order; the new vertex is V + j.  A bisected row t -- one
//   whose winner is accepted -- with k = the bisected rows below it and K_t their total: child 0 = the row with the slot holding hi
//   replaced by V + j, in row t; child 1 = the row with the slot holding lo replaced, in row T + k.  The other slots keep their
//   stored order, and with it the stored orientation.  cell_parent[row] = row below T, the parent for an appended row.
//   COUNTERS u32 [10]: asked, asked refused for an id, asked refused flat, candidates, candidates refused id / hull / lost / flat,
//   accepted edges, bisected tetrahedra.
#pragma once
#include <cstddef>
#include <cstdint>

#include "tn_split_core.h"   // split::mean4, split::child_row, split::MAX_CELLS; iso::fadd / fsub / fmul, iso::edge_key; guard::tet_orient

namespace tn {
namespace esplit {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint64_t MAX_CELLS = split::MAX_CELLS;   // T + K_t must be below it
constexpr int NUM_COUNTERS = 10;
enum Counter : int {
    ASKED = 0, ASKED_ID = 1, ASKED_FLAT = 2, CANDIDATES = 3, REFUSED_ID = 4, REFUSED_HULL = 5, REFUSED_LOST = 6, REFUSED_FLAT = 7,
    ACCEPTED = 8, BISECTED = 9,
};
// what the rows and hull faces around a candidate say of it (or-ed together: no order matters)
constexpr uint32_t FLAG_ID = 1u, FLAG_HULL = 2u, FLAG_LOST = 4u, FLAG_FLAT = 8u;

enum Nomination : uint32_t { NOT_ASKED = 0, NOMINATES = 1, ASKED_REFUSED_FLAT = 2, ASKED_REFUSED_ID = 3 };

// the key a tetrahedron that nominates nothing puts into the sort: above every key of two ids < V, and within the
// 32 + bit_width(V) bits the sort looks at
TN_HD uint64_t sentinel(uint32_t V) { return (uint64_t)V << 32; }

// squared length of the edge from the position of its lower id to that of its higher id
TN_HD float len2(const float lo[3], const float hi[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float dx = iso::fsub(hi[0], lo[0]), dy = iso::fsub(hi[1], lo[1]), dz = iso::fsub(hi[2], lo[2]);
    return iso::fadd(iso::fadd(iso::fmul(dx, dx), iso::fmul(dy, dy)), iso::fmul(dz, dz));
}

TN_HD bool beats(float len_e, uint64_t key_e, float len_f, uint64_t key_f) {
    return len_e > len_f || (len_e == len_f && key_e < key_f);
}

// the slots of tet edge e that hold its lower and its higher id
TN_HD void edge_slots(const uint32_t c[4], int e, int &slot_lo, int &slot_hi) {
    const int a = iso::EDGE_CORNERS[e][0], b = iso::EDGE_CORNERS[e][1];
    const bool a_low = c[a] < c[b];
    slot_lo = a_low ? a : b;
    slot_hi = a_low ? b : a;
}

// keys and squared lengths of the six edges of a row whose ids are < V; p = its four positions in stored order
TN_HD void row_edges(const uint32_t c[4], const float p[4][3], uint64_t key[6], float len[6]) {
    for (int e = 0; e < 6; ++e) {
        int lo, hi;
        edge_slots(c, e, lo, hi);
        key[e] = iso::edge_key(c[lo], c[hi]);
        len[e] = len2(p[lo], p[hi]);
    }
}

TN_HD void gather_row(const uint32_t c[4], const float *xyz, float p[4][3]) {
    for (int j = 0; j < 4; ++j)
        for (int a = 0; a < 3; ++a) p[j][a] = xyz[3 * (size_t)c[j] + a];
}

// what tetrahedron row c nominates: *key receives the key of its best edge (the sentinel where it nominates nothing).  xyz is read
// only where the row is asked and its ids are < V.
TN_HD Nomination nominate(bool asked, const uint32_t c[4], uint32_t V, const float *xyz, uint64_t *key) {
    *key = sentinel(V);
    if (!asked) return NOT_ASKED;
    if (!iso::ids_ok(c, V)) return ASKED_REFUSED_ID;
    float p[4][3];
    gather_row(c, xyz, p);
    if (guard::tet_orient(p) == 0) return ASKED_REFUSED_FLAT;
    uint64_t k[6];
    float len[6];
    row_edges(c, p, k, len);
    int best = 0;
    for (int e = 1; e < 6; ++e)
        if (beats(len[e], k[e], len[best], k[best])) best = e;
    *key = k[best];
    return NOMINATES;
}

// the index of `key` in the ascending list cand[0 .. C), EMPTY where it is not there
TN_HD uint32_t find(const uint64_t *cand, uint32_t C, uint64_t key) {
    uint32_t lo = 0, hi = C;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cand[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < C && cand[lo] == key ? lo : EMPTY;
}

// the midpoint of the edge between the positions of its lower and higher id
TN_HD void midpoint(const float lo[3], const float hi[3], float m[3]) {
    for (int a = 0; a < 3; ++a) m[a] = split::mean4(lo[a], hi[a], lo[a], hi[a]);
}

// What row c says of the candidates among its six edges: found[e] = the candidate index of tet edge e (EMPTY: not a candidate),
// flag[e] = what to or into that candidate's flags (0: nothing).  Returns the row's winner (a candidate index), EMPTY where it has
// none or has an id >= V.  xyz is read only where the ids are < V.
TN_HD uint32_t judge_row(const uint32_t c[4], uint32_t V, const float *xyz, const uint64_t *cand, uint32_t C, uint32_t found[6],
                         uint32_t flag[6]) {
    for (int e = 0; e < 6; ++e) { found[e] = EMPTY; flag[e] = 0u; }
    if (C == 0) return EMPTY;
    if (!iso::ids_ok(c, V)) {
        for (int e = 0; e < 6; ++e) {
            int lo, hi;
            edge_slots(c, e, lo, hi);
            if (c[lo] >= c[hi]) continue;
            found[e] = find(cand, C, iso::edge_key(c[lo], c[hi]));
            flag[e] = FLAG_ID;
        }
        return EMPTY;
    }
    uint64_t key[6];
    float len[6], p[4][3];
    gather_row(c, xyz, p);
    row_edges(c, p, key, len);
    int best = -1;
    for (int e = 0; e < 6; ++e) {
        found[e] = find(cand, C, key[e]);
        if (found[e] != EMPTY && (best < 0 || beats(len[e], key[e], len[best], key[best]))) best = e;
    }
    if (best < 0) return EMPTY;
    const int s = guard::tet_orient(p);
    bool flat = s == 0;
    if (!flat) {
        int slot_lo, slot_hi;
        edge_slots(c, best, slot_lo, slot_hi);
        float m[3];
        midpoint(p[slot_lo], p[slot_hi], m);
        for (int child = 0; child < 2; ++child) {
            const int replaced = child == 0 ? slot_hi : slot_lo;
            float q[4][3];
            for (int j = 0; j < 4; ++j)
                for (int a = 0; a < 3; ++a) q[j][a] = j == replaced ? m[a] : p[j][a];
            if (guard::tet_orient(q) != s) flat = true;
        }
    }
    for (int e = 0; e < 6; ++e)
        if (found[e] != EMPTY) flag[e] = found[e] == found[best] ? (flat ? FLAG_FLAT : 0u) : FLAG_LOST;
    return found[best];
}

// the counter a candidate with these flags adds to: the first refusal that holds, or ACCEPTED
TN_HD Counter classify(uint32_t flags) {
    if (flags & FLAG_ID) return REFUSED_ID;
    if (flags & FLAG_HULL) return REFUSED_HULL;
    if (flags & FLAG_LOST) return REFUSED_LOST;
    if (flags & FLAG_FLAT) return REFUSED_FLAT;
    return ACCEPTED;
}

// the first slots of row c that hold lo and hi; false where one is missing
TN_HD bool slots_of(const uint32_t c[4], uint32_t lo, uint32_t hi, int &slot_lo, int &slot_hi) {
    slot_lo = slot_hi = -1;
    for (int j = 3; j >= 0; --j) {
        if (c[j] == lo) slot_lo = j;
        if (c[j] == hi) slot_hi = j;
    }
    return slot_lo >= 0 && slot_hi >= 0;
}

}  // namespace esplit
}  // namespace tn
