// tn_prune_core.h -- the per-tetrahedron, per-face and per-vertex rule of vertex pruning (tn_prune_count / tn_prune_count_tables /
// tn_prune_emit / tn_prune_vertex_rows), written once for the kernels (tn_prune.hip) and the CPU emulation
// (tests/host/prune_emul.cpp), the way tn_split_core.h states the split.  The same statement in numpy: geometry.py
// (prune_vertices_statement, prune_vertex_rows_statement).
//
// The rule.  cells u32 [T, 4], dead u8 [T] (non-zero = dead), the face table faces u32 [F, 3] and
// face_tets u32 [F, 2], vertex_select u8 [V] or null (where given, only these vertices are asked).
//   MARKS.  A vertex is NAMED if some row of cells contains it; LIVE if a tetrahedron that is not dead names it -- a row with an
//   id >= V counts as live for its in-range ids, so nothing is removed next to a malformed row; HULL if it is a vertex of a face
//   with face_tets[f, 1] == 0xFFFFFFFF.  Ids >= V in either table are skipped.
//   DECISION, for an asked vertex, in this order: kept because live; kept because hull; kept because no tetrahedron names it;
//   otherwise removed.  A vertex that is not asked is kept.
//   COUNTERS u32 [5]: asked, removed, kept live, kept hull, kept unreferenced (the last four add up to the first).
//   NUMBERING.  offsets u32 [V + 1] = exclusive sums of the keep flags, V' = offsets[V]; new_id[v] = offsets[v] for a kept vertex
//   and 0xFFFFFFFF for a removed one; kept_ids[j] = the old id of new vertex j (ascending); xyz_out[j] = xyz[kept_ids[j]].
//   ROWS.  out[r, j] = values[r, kept_ids[j]] (0 where kept_ids[j] >= V), out_vm[j, r] the same value.
#pragma once
#include <cstdint>

#ifndef TN_HD
#if defined(__HIPCC__)
#define TN_HD __host__ __device__ __forceinline__
#else
#define TN_HD inline
#endif
#endif

namespace tn {
namespace prune {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr int NUM_COUNTERS = 5;

enum Outcome : uint32_t {
    NOT_ASKED = 0,
    REMOVED = 1,
    KEPT_LIVE = 2,
    KEPT_HULL = 3,
    KEPT_UNREFERENCED = 4,
};

// the marks one tetrahedron row sets: named[c[k]] = 1 for every id < V, and live[c[k]] = 1 too where the row is not dead or has
// an id >= V.  Plain stores of 1: any order of the lanes gives the same bytes.
TN_HD void mark_tet(const uint32_t c[4], bool is_dead, uint32_t V, uint8_t *named, uint8_t *live) {
    const bool bad = !(c[0] < V && c[1] < V && c[2] < V && c[3] < V);
    const bool lives = !is_dead || bad;
    for (int k = 0; k < 4; ++k) {
        if (c[k] >= V) continue;
        named[c[k]] = 1;
        if (lives) live[c[k]] = 1;
    }
}

// the marks one face sets: hull[f[k]] = 1 for every id < V where the face has no second tetrahedron
TN_HD void mark_face(const uint32_t f[3], uint32_t second_tet, uint32_t V, uint8_t *hull) {
    if (second_tet != EMPTY) return;
    for (int k = 0; k < 3; ++k)
        if (f[k] < V) hull[f[k]] = 1;
}

TN_HD Outcome classify(bool asked, bool named, bool live, bool hull) {
    if (!asked) return NOT_ASKED;
    if (live) return KEPT_LIVE;
    if (hull) return KEPT_HULL;
    if (!named) return KEPT_UNREFERENCED;
    return REMOVED;
}

// (asked, removed, kept live, kept hull, kept unreferenced) += the one-hot of outcome o
TN_HD void count(Outcome o, uint32_t n[NUM_COUNTERS]) {
    n[0] += o != NOT_ASKED;
    n[1] += o == REMOVED;
    n[2] += o == KEPT_LIVE;
    n[3] += o == KEPT_HULL;
    n[4] += o == KEPT_UNREFERENCED;
}

}  // namespace prune
}  // namespace tn
