// tn_build.h -- the device-side structure build of load_tetrahedra (tn_build.hip).
#pragma once
#include "tn_build_core.h"
#include "tn_devbuf.h"

namespace tn {

// shape of the median-split binary tree over n faces (tn_mesh.cpp)
void build_bin_topology(size_t n, std::vector<core::BinNode> &bn, std::vector<std::vector<uint32_t>> &frontier,
                        std::vector<uint32_t> &level_start, std::vector<uint32_t> &leaf_nodes, uint32_t leaf_w = WIDE);

struct BuildTargets {
    DevBuf<uint32_t> &faces, &face_tets;   // [F,3], [F,2]
    DevBuf<WalkVar> &vars;                 // [4T]
    DevBuf<float> &hull_nodes, &hull_tris;
    DevWideBvh &bvh;
};
struct BuildInfo {
    uint32_t F = 0, n_hull = 0, n_hull_nodes = 0, max_stack = 1;
    float scene_max = 0.f;
};
// What a load with the tracer option "refit_tables" keeps for tn_update_vertices (tn_refit.hip): the part of the build that is
// a function of `cells` alone and that the tables the kernels read do not already hold, and the refit's two work arrays (so a
// refit allocates nothing on the device).  Empty after a load without the option.
constexpr size_t REFIT_STAT_WORDS = 7 * 32;   // seven reduced numbers, one 128-byte line each (tn_refit.hip)
struct RefitTables {
    DevBuf<uint32_t> order;        // [T]  tet of walk record r (inverse of rec_of_tet)
    DevBuf<uint32_t> hull_info;    // [n_hull][12]  core::hull_face_info: words 3 / 7 / 11 = face id, tet record, local face
    DevBuf<core::BinNode> bn;      // binary tree over the faces (shape: build_bin_topology) ...
    DevBuf<uint32_t> face_order;   // [F]  ... the face order its (first, count) ranges index ...
    DevBuf<uint32_t> leaf_nodes;   // [n_leaves]  ... its leaves by leaf index ...
    DevBuf<uint32_t> wide_sub;     // [n_wide]  ... and the root of the binary subtree each 64-wide node was collapsed from
    std::vector<uint32_t> level_start;   // binary nodes of level l: [level_start[l], level_start[l + 1])
    DevBuf<float> node_lo, node_hi;      // work: [nodes][3] boxes of the binary nodes
    DevBuf<uint32_t> vmin;               // work: [V + REFIT_STAT_WORDS] star minima of the thin pass, then max |coordinate| and the mesh box
    bool valid = false;
    size_t bytes() const {
        return 4 * (order.n + hull_info.n + face_order.n + leaf_nodes.n + wide_sub.n + node_lo.n + node_hi.n + vmin.n) +
               sizeof(core::BinNode) * bn.n;
    }
    void release() {
        order.release(); hull_info.release(); bn.release(); face_order.release(); leaf_nodes.release(); wide_sub.release();
        node_lo.release(); node_hi.release(); vmin.release(); level_start.clear();
        valid = false;
    }
};

// Everything load_tetrahedra owns, built on the device from the caller's (device) xyz / cells on `stream`:
// face table in first-seen order, face -> tets, Morton-ordered walk records, hull tree, 64-wide face BVH.
// Blocking (a handful of small D2H reads: counts, the hull faces, the child rows for the stack bound).
// Throws the reference's errors ("A triangle is shared by more than two tetrahedra!", out-of-bounds vertex ids).
// `keep` (may be null): filled for a later device_refit; with null the build launches and keeps exactly what it did without it.
void device_build(size_t V, size_t T, const float *xyz, const uint32_t *cells, hipStream_t stream, BuildTargets out,
                  BuildInfo &info, uint32_t leaf_w = WIDE, RefitTables *keep = nullptr);

// The tables of a device build whose `cells` stay and whose vertices moved (tn_refit.hip): everything that holds positions is
// recomputed in place from `xyz` -- pn and the thin exponent of the 4T walk records, the face BVH's boxes and leaf triangles
// over the kept tree, the hull tree -- with the build's expressions, so every table equals a fresh build's up to the order the
// fresh build would give records, faces and hull slots.  Blocking (two small D2H reads: the hull faces; max |coordinate| and the box of the
// referenced vertices, which come back in scene_max / box_lo / box_hi = what tn::mesh_box computes).
struct RefitTargets {
    WalkHot *hot;                              // [4T]
    const uint32_t *faces;                     // [F,3]
    DevBuf<float> &hull_nodes, &hull_tris;     // sizes stay (n_hull is topological)
    DevWideBvh &bvh;                           // boxes and leaf_tri rewritten; child, leaf_id, n_nodes stay
};
void device_refit(size_t V, size_t T, const float *xyz, const uint32_t *cells, hipStream_t stream, RefitTargets out,
                  RefitTables &kept, float &scene_max, float box_lo[3], float box_hi[3]);

// The vertex step limiter (tn_vertex_guard.hip; the rule: tn_vertex_guard_core.h).  Both enqueue on `s` and return: no read-back,
// no device allocation.  launch_tet_quality: width f32 [T] / orient i8 [T] / star_width f32 [V], each may be null; star_width is
// preset to +inf by a fill.  launch_limit_vertex_step: star widths of xyz_old into star_width, xyz_new clamped in place,
// counters u32 [4] zeroed and then = clamped, frozen but asked to move, flipped, collapsed (the last two only with `verify`).
void launch_tet_quality(size_t V, size_t T, const uint32_t *cells, const float *xyz, float *width, int8_t *orient, float *star_width,
                        hipStream_t s);
void launch_limit_vertex_step(size_t V, size_t T, const uint32_t *cells, const float *xyz_old, float *xyz_new, float fraction,
                              float *star_width, uint32_t *counters, bool verify, hipStream_t s);

// The Delaunay monitor and the per-tetrahedron state transfer (tn_delaunay.hip; the predicate and the rule: tn_delaunay_core.h).
// Both enqueue on `s` and return: no read-back, no device allocation.  launch_delaunay_check: counters u32 [4] zeroed and then =
// interior faces, violated, uncertain, violated with an inverted first tetrahedron; face_state i8 [F] and tet_violations u8 [T]
// (zeroed here; 4-byte aligned storage of 4 ceil(T / 4) bytes) may be null.  launch_remap_tet_values: star_max f32 [V] is the
// call's scratch (zeroed here); vertex ids >= V are passed over.
void launch_delaunay_check(size_t T, size_t F, const uint32_t *cells, const uint32_t *face_tets, const float *xyz, uint32_t *counters,
                           int8_t *face_state, uint8_t *tet_violations, hipStream_t s);
void launch_remap_tet_values(size_t V, size_t T_old, const uint32_t *old_cells, const float *old_values, size_t T_new,
                             const uint32_t *new_cells, float *new_values, float *star_max, hipStream_t s);

// The isosurface extraction (tn_isosurface.hip; the rule: tn_isosurface_core.h).  Both enqueue on `s` and return: no read-back; one
// stream-ordered allocation each.  launch_isosurface_count: tri_offsets / ref_offsets u32 [T + 1] = exclusive sums of the triangles
// and crossing edges per tetrahedron, the totals last.  launch_isosurface_emit: the caller read those totals back and passes
// them as num_triangles / num_refs, which bound every store; the vertex outputs have capacity num_refs, *num_out_vertices
// receives the welded count.  tet_mask u8 [T] may be null.  The entries (tn_api_tracer.hip) have checked the arguments.
void launch_isosurface_count(size_t V, size_t T, const uint32_t *cells, const float *values, float level, const uint8_t *tet_mask,
                             uint32_t *tri_offsets, uint32_t *ref_offsets, hipStream_t s);
void launch_isosurface_emit(size_t V, size_t T, const float *xyz, const uint32_t *cells, const float *values, float level,
                            const uint8_t *tet_mask, const uint32_t *tri_offsets, const uint32_t *ref_offsets, size_t num_triangles,
                            size_t num_refs, uint32_t *triangles, uint32_t *triangle_tets, uint32_t *edge_vertices, float *edge_t,
                            float *positions, uint32_t *num_out_vertices, hipStream_t s);

// The refinement of the extracted vertices (tn_isosurface_refine.hip; the rule: tn_isosurface_core.h).  N welded vertices;
// edge_vertices u32 [N, 2] (8-byte aligned), brackets f32 [N, 4] (16-byte aligned), flags u8 [N], vertex_indices u32 [7 N, 4]
// (16-byte aligned), barycentric f32 [7 N, 3], densities f32 [7 N].  Each enqueues one kernel on `s` (none for N == 0), allocates
// nothing and reads nothing back.  The entries (tn_api_tracer.hip) have checked the arguments.
void launch_isosurface_refine_begin(size_t V, size_t N, const uint32_t *edge_vertices, const float *values, float level,
                                    float *brackets, uint8_t *flags, hipStream_t s);
void launch_isosurface_refine_points(size_t N, const uint32_t *edge_vertices, const float *brackets, const uint8_t *flags,
                                     uint32_t *vertex_indices, float *barycentric, hipStream_t s);
void launch_isosurface_refine_select(size_t N, float level, const float *densities, float *brackets, uint8_t *flags,
                                     hipStream_t s);
void launch_isosurface_refine_vertices(size_t V, size_t N, const float *xyz, const uint32_t *edge_vertices, const float *brackets,
                                       float level, float *edge_t, float *positions, hipStream_t s);

// The tetrahedron split (tn_split.hip; the rule: tn_split_core.h; no reference counterpart: the reference never changes its
// mesh).  A selected tetrahedron is split 1 -> 4 at its centroid c = ((p0 + p1) + (p2 + p3)) * 0.25f iff its ids are < V, its
// orientation s (guard::tet_orient) is not 0 and each of its four children has orientation s.  All three enqueue on `s` and
// return: no read-back.  launch_split_count: offsets u32 [T + 1] = exclusive sums of the accepted flags, the total K last;
// counters u32 [4] zeroed and then = asked, accepted, refused flat or inverted, refused for an id >= V; one stream-ordered
// allocation.  launch_split_emit: the caller read K back and passes it as num_new, which bounds every store; xyz_out f32
// [V + num_new, 3], cells_out u32 [T + 3 num_new, 4], cell_parent u32 [T + 3 num_new], vertex_parents u32 [num_new, 4].
// launch_split_vertex_rows: out f32 [rows, V + K] = values f32 [rows, V] with K new columns (new_mode 0: the mean4 of the four
// parent columns, 1: zeros; a parent id >= V gives 0), out_vm f32 [V + K, rows] (nullable) its transposition; values_vm f32
// [V, rows] (nullable) = the transposition of values, then read in the place of the parent columns.  The entries
// (tn_api_tracer.hip) have checked the arguments.
void launch_split_count(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint8_t *select, uint32_t *offsets,
                        uint32_t *counters, hipStream_t s);
void launch_split_emit(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint32_t *offsets, size_t num_new,
                       float *xyz_out, uint32_t *cells_out, uint32_t *cell_parent, uint32_t *vertex_parents, hipStream_t s);
void launch_split_vertex_rows(size_t rows, size_t V, size_t K, const float *values, const float *values_vm,
                              const uint32_t *vertex_parents, uint32_t new_mode, float *out, float *out_vm, hipStream_t s);

// Vertex pruning (tn_prune.hip; the rule: tn_prune_core.h; no reference counterpart).  An asked vertex is removed iff some
// tetrahedron names it, every tetrahedron that names it is dead, and it is on no hull face.  All three enqueue on `s` and return:
// no read-back.  launch_prune_count: offsets u32 [V + 1] = exclusive sums of the keep flags, V' last; counters u32 [5] zeroed and
// then = asked, removed, kept live, kept hull, kept unreferenced; one stream-ordered allocation.  launch_prune_emit: the caller
// read V' back and passes it as num_kept, which bounds every store; new_id u32 [V], kept_ids u32 [num_kept], xyz_out f32
// [num_kept, 3].  launch_prune_vertex_rows: out f32 [rows, V'] = values[:, kept_ids] (an id >= V gives 0), out_vm f32 [V', rows]
// (nullable) its transposition; values_vm f32 [V, rows] (nullable) = the transposition of values, then read in its place.  The
// entries (tn_api_tracer.hip) have checked the arguments.
void launch_prune_count(size_t V, size_t T, const uint32_t *cells, size_t F, const uint32_t *faces, const uint32_t *face_tets,
                        const uint8_t *dead, const uint8_t *select, uint32_t *offsets, uint32_t *counters, hipStream_t s);
void launch_prune_emit(size_t V, const float *xyz, const uint32_t *offsets, size_t num_kept, uint32_t *new_id, uint32_t *kept_ids,
                       float *xyz_out, hipStream_t s);
void launch_prune_vertex_rows(size_t rows, size_t V, size_t num_kept, const float *values, const float *values_vm,
                              const uint32_t *kept_ids, float *out, float *out_vm, hipStream_t s);

// The edge split (tn_edge_split.hip; the rule: tn_edge_split_core.h; no reference counterpart).  The best edge of every asked
// tetrahedron is a candidate; a candidate is bisected at its midpoint with every row around it unless a ring row has an id >= V,
// it lies on a hull face, a ring row prefers another candidate, or a ring row or child is flat.  Both enqueue on `s` and return: no
// read-back.  launch_edge_split_count: tet_offsets u32 [T + 1] = exclusive sums of the bisected flags; tet_edge u32 [T] = the rank
// of the row's accepted edge (0xFFFFFFFF: not bisected); bisected u8 [T]; edge_vertices u32 [T, 2] of which the first K_v rows are
// written; counters u32 [10] zeroed and then filled (K_v = counters[8], K_t = counters[9]); one stream-ordered allocation.
// launch_edge_split_emit: the caller read the two totals back and passes them as num_new and num_rows, which bound every store;
// xyz_out f32 [V + num_new, 3], cells_out u32 [T + num_rows, 4], cell_parent u32 [T + num_rows], vertex_parents u32 [num_new, 4].
// The entries (tn_api_tracer.hip) have checked the arguments.
void launch_edge_split_count(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint8_t *select, size_t F,
                             const uint32_t *faces, const uint32_t *face_tets, uint32_t *tet_offsets, uint32_t *tet_edge,
                             uint8_t *bisected, uint32_t *edge_vertices, uint32_t *counters, hipStream_t s);
void launch_edge_split_emit(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint32_t *tet_offsets,
                            const uint32_t *tet_edge, const uint32_t *edge_vertices, size_t num_new, size_t num_rows, float *xyz_out,
                            uint32_t *cells_out, uint32_t *cell_parent, uint32_t *vertex_parents, hipStream_t s);

// The Delaunay repair by flips (tn_flip.hip; the rule: tn_flip_core.h; no reference counterpart).  A certainly violated interior
// face is a candidate; it is flipped 2-3 or 3-2 unless a row it reads has a bad id, its two apices are not certainly on opposite
// sides, an orientation around the new edge is uncertain, the configuration is unflippable, or a row it needs goes to a candidate
// with a smaller face id.  Both enqueue on `s` and return: no read-back.  launch_flip_count: tet_offsets u32 [T + 1] = exclusive sums
// of "row t is kept" (all rows but the deleted third rows of 3-2 flips); tet_flip u32 [T] = the accepted face that takes the row
// (0xFFFFFFFF: untouched); flipped u8 [T]; face_flip u32 [F, 3] = (code, t2, rank); counters u32 [10] zeroed and then filled (K23 =
// counters[8], K32 = counters[9]); one stream-ordered allocation.  launch_flip_emit: the caller read the two totals back and passes
// them as num_23 and num_32, which bound every store; cells_out u32 [T + num_23 - num_32, 4], cell_sources u32 [same, 3].  The
// entries (tn_api_tracer.hip) have checked the arguments.
void launch_flip_count(size_t V, size_t T, const float *xyz, const uint32_t *cells, size_t F, const uint32_t *faces,
                       const uint32_t *face_tets, uint32_t *tet_offsets, uint32_t *tet_flip, uint8_t *flipped, uint32_t *face_flip,
                       uint32_t *counters, hipStream_t s);
void launch_flip_emit(size_t T, const uint32_t *cells, size_t F, const uint32_t *faces, const uint32_t *face_tets,
                      const uint32_t *tet_offsets, const uint32_t *tet_flip, const uint32_t *face_flip, size_t num_23, size_t num_32,
                      uint32_t *cells_out, uint32_t *cell_sources, hipStream_t s);

// The face table of any cell rows, without a tracer (tn_build.hip: the face-table stage of device_build on its own; the rule:
// face_hash_insert / face_is_first / face_emit of tn_build_core.h, in words DESIGN.md section 4.24).  Both enqueue on `s` and
// return: no read-back.  launch_face_table_count: partner u32 [4T] = the other sighting of sighting i's face or 0xFFFFFFFF;
// face_index u32 [4T + 1] = exclusive sums of "sighting i is the first of its face", the total F last; counters u32 [4] zeroed and
// then = F, hull faces, FLAG_CELL_OOB | FLAG_TRIPLE_FACE, 0; one stream-ordered allocation (hash slots: the smallest power of two
// >= 8T + 16).  launch_face_table_emit: the caller read F back and passes it as num_faces, which bounds every store to faces u32
// [num_faces, 3] and face_tets u32 [num_faces, 2]; tet_faces u32 [T, 4] may be null (then one stream-ordered allocation).  The
// entries (tn_api_tracer.hip) have checked the arguments.
void launch_face_table_count(size_t V, size_t T, const uint32_t *cells, uint32_t *partner, uint32_t *face_index, uint32_t *counters,
                             hipStream_t s);
void launch_face_table_emit(size_t T, const uint32_t *cells, const uint32_t *partner, const uint32_t *face_index, size_t num_faces,
                            uint32_t *faces, uint32_t *face_tets, uint32_t *tet_faces, hipStream_t s);

}  // namespace tn
