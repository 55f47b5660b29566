/*
 * tetranerf_hip.h -- C-ABI of libtetranerf_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the ray -> tetrahedra hot path of jkulhanek/tetra-nerf.
 * Every entry point replaces one native function the reference's pybind11 module
 * (`tetranerf_cpp_extension`, /root/reference/src/py_binding.cpp:433-449) binds; the
 * reference interface each one stands in for is cited at the declaration.
 *
 * Conventions
 *   - plain C, raw DEVICE pointers and sizes, no torch / HIP types in signatures;
 *     `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - every function returns 0 on success, non-zero on error; the message is available
 *     from tn_last_error() (thread-local) and mirrors the reference's exception text where
 *     callers can observe it (src/utils/exception.h:164-181 -> Python RuntimeError);
 *   - all work is enqueued on `stream`; no call synchronises the device except
 *     tn_load_tetrahedra (one-off build, like TetrahedraStructure::build's blocking copies,
 *     src/tetrahedra_tracer.cpp:255-259);
 *   - the caller owns every input/output buffer.  The tracer owns only what it derives
 *     from the mesh (face tables, acceleration structures, scratch); the vertex and cell
 *     buffers are borrowed for the tracer's lifetime (src/tetrahedra_tracer.h:300-303);
 *   - output buffers need NOT be initialised: each kernel writes every byte of its outputs
 *     exactly once (the reference memsets them first, py_binding.cpp:53-57,188-191).
 *   - indices are uint32 with 0xFFFFFFFF = "empty" (int32 -1 on the torch side).
 */
#ifndef TETRANERF_HIP_H
#define TETRANERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tn_tracer *tn_tracer_t;

/* thread-local text of the last error raised on this thread ("" if none) */
const char *tn_last_error(void);

/* library / build identification: "tetranerf_hip <version> abi <TN_ABI_VERSION> gfx950" */
const char *tn_version(void);

/* Number of this header's binary interface: raised whenever an exported signature changes (round 5 added count / ray_index
 * pointers to tn_find_matched_cells_indexed, tn_mlp_forward_gather, tn_composite, tn_sample_coarse, tn_sample_pdf and removed
 * tn_render_pass).  A binding compares tn_abi_version() of the library it loaded with the TN_ABI_VERSION it was written
 * against and refuses a mismatch (tetra-nerf_amd/_lib.py does) instead of calling through shifted arguments. */
#define TN_ABI_VERSION 6
int tn_abi_version(void);

/* TetrahedraTracer::TetrahedraTracer(int8_t device)   src/tetrahedra_tracer.h:284-378,
 *                                                       src/tetrahedra_tracer.cpp:90-135
 * PyTetrahedraTracer ctor                               src/py_binding.cpp:30-36 */
int tn_tracer_create(int device, tn_tracer_t *out);

/* TetrahedraTracer::~TetrahedraTracer                  src/tetrahedra_tracer.cpp:178-189 */
int tn_tracer_destroy(tn_tracer_t tracer);

/* TetrahedraTracer::load_tetrahedra -> TetrahedraStructure::build
 *   src/tetrahedra_tracer.h:304-309, src/tetrahedra_tracer.cpp:244-340;
 *   face table = convert_tetrahedra_to_triangles, src/tetrahedra_tracer.cpp:45-71
 * xyz   f32 [V,3] device, cells u32 [T,4] device (borrowed).
 * The structures are built ON THE DEVICE from these buffers (csrc/tn_build.hip; option "gpu_build" = 0 selects the
 * single-threaded host build of csrc/tn_mesh.cpp, which produces identical face tables, walk records and hull tree).
 * Blocking, like the reference's.
 * Errors: "A triangle is shared by more than two tetrahedra!", "cells contains a vertex index that is out of bounds",
 * "load_tetrahedra needs at least one tetrahedron" (num_cells = 0, either build; refused before anything is touched: a mesh
 * loaded earlier stays loaded) */
int tn_load_tetrahedra(tn_tracer_t tracer, size_t num_vertices, size_t num_cells,
                       const float *xyz, const uint32_t *cells, void *stream);

/* Refit (no reference counterpart: the reference reloads).  The vertices of the loaded mesh moved and `cells` did not: everything
 * tn_load_tetrahedra built that holds positions is recomputed in place from xyz (csrc/tn_refit.hip) -- the position and the
 * thin-neighbourhood exponent of the 4T walk records, the face BVH's boxes and leaf triangles over the kept tree, the hull tree,
 * max |coordinate| and the mesh box of binned calls -- and everything that depends on `cells` alone is kept (face table, Morton
 * order of the records, adjacency codes, shape and face order of the BVH).  Afterwards every query answers as a tracer freshly
 * loaded on xyz does, row for row; only the ORDER of records and BVH leaves stays that of the vertices of the load, so locality
 * degrades with large deformation: reload every so often.
 * xyz  f32 [V,3] device: the buffer given to tn_load_tetrahedra, modified in place, or another one; borrowed from now on.
 * Needs a tracer loaded with option "refit_tables" = 1 by the device build.  Blocking, like the load (two small read-backs);
 * launches on `stream`; allocates nothing on the device.  The call makes no promise the load does not make: a move after which
 * tetrahedra overlap gives a mesh the walk's certification does not cover, refitted or freshly loaded.  tn_limit_vertex_step
 * (below) shortens a move so that no tetrahedron inverts; call it on the new vertices before this.
 * Errors (nothing is touched): tracer not loaded; num_vertices != the loaded V; xyz null; loaded without "refit_tables";
 * loaded by the host build ("gpu_build" = 0). */
int tn_update_vertices(tn_tracer_t tracer, size_t num_vertices, const float *xyz, void *stream);

/* device bytes the loaded mesh keeps for tn_update_vertices beyond its tables (0: loaded without "refit_tables", or not loaded) */
size_t tn_refit_table_bytes(tn_tracer_t tracer);

/* Vertex step limiter (no reference counterpart: the reference never moves vertices).  An optimiser's step can turn a tetrahedron
 * inside out; these two entries bound it on the device, with no host synchronisation (csrc/tn_vertex_guard.hip, DESIGN.md
 * section 4.11).  The WIDTH w of a tetrahedron is its smallest extent over all directions = the smallest of its four heights and
 * its three distances between opposite edges, evaluated in double on the fp32 coordinates.  If every vertex of a tetrahedron moves
 * by less than w / 2, its signed volume keeps its sign along the whole straight move.  star_width[v] = the smallest fl32(w) over
 * the tetrahedra around v (+inf, bits 0x7F800000, where no tetrahedron names v).
 *
 * tn_tet_quality: of the loaded cells on `xyz` f32 [V,3] (any positions: the loaded ones, or candidates), each output optional:
 *   width f32 [T], orient i8 [T] (sign of ((p1-p0) x (p2-p0)) . (p3-p0): -1, 0, 1), star_width f32 [V].
 * tn_limit_vertex_step: xyz_new f32 [V,3] (in, out) is the move an optimiser wants from xyz_old f32 [V,3].  Per vertex, in fp32:
 *   limit = fraction * star_width[v] (star widths of xyz_old; written to star_width, which is required: it is the call's scratch);
 *   star_width[v] < 2^-17 max(|x|,|y|,|z|) of the old position: FROZEN, new = old bit for bit (the rounding of new coordinates
 *   must stay a small part of the budget; the vertices of zero-volume tetrahedra are frozen by this rule);
 *   |new - old| <= limit: untouched;  otherwise new = old + (new - old) (limit / |new - old|), or old where |new - old| is not finite.
 *   counters u32 [4] (zeroed by the call): vertices clamped, frozen vertices that were asked to move, and -- the call's own
 *   cross-check, unless TN_LIMIT_STEP_NO_VERIFY is set -- tetrahedra whose orientation changed sign from xyz_old to the clamped
 *   xyz_new (flipped) and those that went from non-zero to zero (collapsed).  Both are 0 whenever the bound applies.
 *   fraction must be in (0, 0.45].
 * The bound is per tetrahedron: parts of the hull that are far apart in the mesh and move INTO each other are not covered.
 * Both work on any loaded tracer (they read the borrowed `cells` only; neither "refit_tables" nor the device build is needed),
 * leave the tracer's tables alone (tn_update_vertices makes it follow), launch on `stream`, read nothing back and allocate nothing.
 * Errors (nothing is touched): tracer not loaded; num_vertices != the loaded V; xyz / xyz_old / xyz_new / star_width / counters
 * null; fraction not in (0, 0.45] (NaN included); unknown flags. */
#define TN_LIMIT_STEP_NO_VERIFY 1u
int tn_tet_quality(tn_tracer_t tracer, size_t num_vertices, const float *xyz, float *width, int8_t *orient, float *star_width,
                   void *stream);
int tn_limit_vertex_step(tn_tracer_t tracer, size_t num_vertices, const float *xyz_old, float *xyz_new, float fraction,
                         float *star_width, uint32_t *counters, uint32_t flags, void *stream);

/* Delaunay monitor (no reference counterpart: the reference never moves vertices).  A limited vertex step keeps every tetrahedron
 * valid, not the mesh Delaunay; this entry counts the interior faces of the loaded mesh that are not locally Delaunay on `xyz`
 * (csrc/tn_delaunay.hip, csrc/tn_delaunay_core.h).  One lane per face of the loaded face table: with
 * face_tets[f] = (t0, t1), p0..p3 = xyz[cells[t0]] in stored order and e = xyz[the vertex of cells[t1] that cells[t0] does not
 * name], the face is VIOLATED iff e lies strictly inside the circumsphere of t0, i.e. iff the 4 x 4 in-sphere determinant
 * (translated by e) and the 3 x 3 orientation determinant (translated by p3) have the same sign.  Both are Shewchuk's stage-A
 * expressions in double on the fp32 coordinates, each with its permanent; a determinant is CERTAIN iff its magnitude exceeds
 * (16 + 224 eps) eps permanent (in-sphere) or (7 + 56 eps) eps permanent (orientation), eps = 2^-53 -- a-priori bounds that cover
 * the rounding of the differences, so a certain sign is the exact sign.  There is no exact fallback on the device.
 *   face_state     i8 [F], optional: 0 hull face (t1 empty), 1 regular (both certain, e not inside), 2 violated (both certain,
 *                  e inside), 3 uncertain (either filter fails: cospherical points, zero-volume tetrahedra, NaN).
 *   tet_violations u8 [T], optional: the violated faces of every tetrahedron, 0..4.  Counted through 32-bit atomics: the storage
 *                  must be 4-byte aligned and 4 ceil(T / 4) bytes long; all of it is zeroed by the call.
 *   counters       u32 [4], zeroed by the call: interior faces, violated, uncertain, and violated faces whose t0 is certainly of
 *                  negative orientation AS STORED (((p1-p0) x (p2-p0)) . (p3-p0) < 0).  In a table stored with positive
 *                  orientations the last one counts inverted cells: the caller moved vertices without tn_limit_vertex_step.
 * Works on any loaded tracer, host or device build (it reads the borrowed `cells` and the face table), leaves the tracer alone,
 * launches on `stream`, reads nothing back and allocates nothing.
 * Errors (nothing is touched): tracer not loaded; num_vertices != the loaded V; xyz / counters null; tet_violations misaligned. */
int tn_delaunay_check(tn_tracer_t tracer, size_t num_vertices, const float *xyz, uint32_t *counters, int8_t *face_state,
                      uint8_t *tet_violations, void *stream);

/* Per-tetrahedron state across a change of cells, without point location (csrc/tn_delaunay.hip).  For values >= 0 (the occupancy
 * field):   star_max[v] = max{ old_values[t] : old_cells[t] names v }  (0 where no old cell names v),
 *           new_values[t'] = max of star_max over the four vertices of new_cells[t'].
 * Conservative: a new tetrahedron gets at least the value of every old tetrahedron around each of its vertices, so nothing that was
 * live is culled by the transfer; the price is a dilation by one ring of tetrahedra.  The rule the kernels follow is the maximum
 * of the values' BIT PATTERNS as unsigned integers, which is the maximum of non-negative floats; NaN and negative values are not
 * checked and follow that rule (a set sign bit beats everything).  Vertex ids >= num_vertices are passed over.
 * old_cells u32 [num_old_cells, 4], old_values f32 [num_old_cells], new_cells u32 [num_new_cells, 4], new_values f32
 * [num_new_cells] (out), star_max f32 [num_vertices] (out: the call's scratch), all on the current device.  Needs no tracer;
 * launches on `stream`, reads nothing back and allocates nothing.  Errors (nothing is touched): a null pointer beside a non-zero
 * count. */
int tn_remap_tet_values(size_t num_vertices, size_t num_old_cells, const uint32_t *old_cells, const float *old_values,
                        size_t num_new_cells, const uint32_t *new_cells, float *new_values, float *star_max, void *stream);

/* Isosurface extraction (no reference counterpart: the reference renders its field and never meshes it).  Marching tetrahedra on
 * the mesh the field lives on: the level set { values = level } of the piecewise-linear interpolant of a per-vertex scalar over
 * any tetrahedron soup, as a WELDED, consistently ORIENTED triangle mesh in a DETERMINISTIC order (csrc/tn_isosurface.hip, the
 * rule once in csrc/tn_isosurface_core.h; every output is bit-equal to geometry.isosurface_statement).
 *   xyz f32 [V,3], cells u32 [T,4], values f32 [V], tet_mask u8 [T] (nullable; 0 = skip), all on the current device.
 *   inside(v) = values[v] >= level.  A tetrahedron is skipped if its mask byte is 0, an id is >= V, or one of its four values is
 *   not finite or is >= 2^126 in magnitude.  Tet edges 0..5 = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) in stored corner order; an edge
 *   crosses if its ends differ in `inside`; three crossing edges give one triangle, four give two.  Each triangle is oriented so
 *   that (q1-q0) x (q2-q0) points towards values < level in a tetrahedron whose ((p1-p0) x (p2-p0)) . (p3-p0) is >= 0 as
 *   evaluated by tn_tet_quality's orientation, and the other way round in one where it is negative.
 *   A surface vertex belongs to a mesh edge (a, b), a < b, and is computed once from the sorted pair, in fp32 with one rounding
 *   per operation and no fused multiply-add:  t = (level - values[a]) / (values[b] - values[a]) in [0, 1],
 *   p = xyz[a] + t (xyz[b] - xyz[a]).  A value equal to level is inside and yields the endpoint itself; the zero-area triangles
 *   this makes are kept.  Vertices ascend by (a << 32 | b); triangles ascend by tetrahedron, then by table row.
 * Two entries with one small read-back between them, which is the caller's:
 * tn_isosurface_count: tri_offsets / ref_offsets u32 [T+1] = exclusive sums over the tetrahedra of their triangles (0, 1, 2) and
 *   crossing edges (0, 3, 4); the totals num_triangles / num_refs are the last elements.
 * tn_isosurface_emit:  given those arrays and totals (host values), triangles u32 [num_triangles,3] (welded vertex ids),
 *   triangle_tets u32 [num_triangles] (the source tetrahedron), and -- capacity num_refs each, the first *num_out_vertices rows
 *   written -- edge_vertices u32 [.,2] = (a, b), edge_t f32 [.], positions f32 [.,3]; num_out_vertices u32 [1] on the device.
 *   Every store is bounded by the totals passed: a caller who changed `values` between the two entries gets a wrong mesh, never
 *   a write outside its buffers.
 * Neither needs a tracer.  Both launch on `stream`, read nothing back, use no atomics and take their scratch as one
 * stream-ordered allocation.  T == 0, or no crossing edge, gives empties (offsets of zeros, *num_out_vertices = 0) without a
 * launch.  Errors (nothing is touched): a null pointer beside a non-zero count; level not finite or >= 2^126 in magnitude;
 * num_cells >= 2^30; num_vertices >= 2^32 - 1; num_triangles > 2 num_cells or num_refs > 4 num_cells. */
int tn_isosurface_count(size_t num_vertices, size_t num_cells, const uint32_t *cells, const float *values, float level,
                        const uint8_t *tet_mask, uint32_t *tri_offsets, uint32_t *ref_offsets, void *stream);
int tn_isosurface_emit(size_t num_vertices, size_t num_cells, const float *xyz, const uint32_t *cells, const float *values,
                       float level, const uint8_t *tet_mask, const uint32_t *tri_offsets, const uint32_t *ref_offsets,
                       size_t num_triangles, size_t num_refs, uint32_t *triangles, uint32_t *triangle_tets,
                       uint32_t *edge_vertices, float *edge_t, float *positions, uint32_t *num_out_vertices, void *stream);

/* Isosurface refinement (no reference counterpart: the reference never meshes its field).  The mesh of tn_isosurface_emit is the
 * level set of the LINEAR interpolant of the vertex values; where the values are a network's density, which is not linear along a
 * mesh edge, these four steps move every welded vertex along its own edge (a, b) onto a crossing of the density the CALLER
 * evaluates between them.  The topology is not touched: same triangles, same welding, same order (csrc/tn_isosurface_refine.hip,
 * the rule once in csrc/tn_isosurface_core.h; every output is bit-equal to
 * geometry.isosurface_refine_statement on the same densities).
 *   N = num_surface_vertices; edge_vertices u32 [N,2] = tn_isosurface_emit's (8-byte aligned); brackets f32 [N,4] =
 *   (t_lo, t_hi, s_lo, s_hi) (16-byte aligned); frozen u8 [N]: 0, 1 = frozen, 2 = an id >= num_vertices.
 * tn_isosurface_refine_begin:    brackets = (0, 1, values[a], values[b]), frozen = 0; an edge whose values are not finite, are
 *   >= 2^126 in magnitude or lie on one side of `level` starts frozen; an id >= num_vertices gives (0, 1, 0, 0) and frozen = 2.
 * tn_isosurface_refine_points:   for round `round` (0..7) the 7 N candidates as the inputs of tn_mlp_forward_gather:
 *   vertex_indices u32 [N,7,4] = (a, b, a, a) (16-byte aligned), barycentric f32 [N,7,3] = (t_j, 0, 0),
 *   t_j = t_lo + (j / 8) (t_hi - t_lo), j = 1..7, in fp32 with one rounding per operation: t_lo <= t_1 <= ... <= t_7 <= t_hi.
 *   An edge with frozen = 2 asks for vertex 0.  The caller then evaluates densities f32 [N,7] there, e.g. by
 *   tn_mlp_forward_gather(n = 7 N, samples_per_ray = 1, dirs = NULL, rgb = NULL) in any of its modes.
 * tn_isosurface_refine_select:   in place; with (t_0, s_0) = (t_lo, s_lo) and (t_8, s_8) = (t_hi, s_hi) the new bracket is
 *   (t_j, t_j+1, s_j, s_j+1) for the FIRST j in 0..7 whose ends differ in inside(s) = s >= level: of several crossings the one
 *   nearest a.  If one of the seven densities is not finite or is >= 2^126 in magnitude the edge is frozen: frozen = 1, and its
 *   bracket stays as it is in this and every later round.
 * tn_isosurface_refine_vertices: edge_t f32 [N], positions f32 [N,3] of the brackets as they stand:
 *   q = (level - s_lo) / (s_hi - s_lo), t = t_lo + q (t_hi - t_lo) put back into [t_lo, t_hi] (t = q (t_hi - t_lo) where
 *   t_lo == 0), p = xyz[a] + t (xyz[b] - xyz[a]).  Straight after _begin these are tn_isosurface_emit's edge_t and positions, bit
 *   for bit.  An id >= num_vertices gives t = 0, p = 0, as tn_isosurface_emit writes it.
 * A refinement of R <= 8 rounds is begin, R x (points, the caller's densities, select), vertices.  None needs a tracer; each is
 * one kernel on `stream`, a lane per element, one writer per element, no atomics, no allocation, nothing read back.
 * num_surface_vertices == 0 is a valid call without a launch.  Errors (nothing is touched): a null or misaligned pointer beside
 * a non-zero count; level not finite or >= 2^126 in magnitude; round >= 8; num_vertices >= 2^32 - 1; num_surface_vertices above
 * what 2^30 tetrahedra emit; tn_isosurface_refine_points with num_vertices == 0. */
int tn_isosurface_refine_begin(size_t num_vertices, size_t num_surface_vertices, const uint32_t *edge_vertices,
                               const float *values, float level, float *brackets, uint8_t *frozen, void *stream);
int tn_isosurface_refine_points(size_t num_vertices, size_t num_surface_vertices, uint32_t round, const uint32_t *edge_vertices,
                                const float *brackets, const uint8_t *frozen, uint32_t *vertex_indices, float *barycentric,
                                void *stream);
int tn_isosurface_refine_select(size_t num_surface_vertices, uint32_t round, float level, const float *densities,
                                float *brackets, uint8_t *frozen, void *stream);
int tn_isosurface_refine_vertices(size_t num_vertices, size_t num_surface_vertices, const float *xyz,
                                  const uint32_t *edge_vertices, const float *brackets, float level, float *edge_t,
                                  float *positions, void *stream);

/* Tetrahedron split (no reference counterpart: the reference's mesh is its input point cloud for the whole run).  Selected
 * tetrahedra are split 1 -> 4 at their centroids, which changes the RESOLUTION of the mesh and nothing else: the four outer faces
 * of a split tetrahedron stay, so the mesh stays conforming without touching a neighbour (csrc/tn_split.hip, the rule once in
 * csrc/tn_split_core.h; every output is bit-equal to geometry.split_tetrahedra_statement /
 * geometry.split_vertex_rows_statement).
 *   xyz f32 [V,3], cells u32 [T,4], select u8 [T] (non-zero = asked), all on the current device.
 *   Tetrahedron t is ACCEPTED iff it is asked, its four ids are < V, the orientation s of its stored row -- the sign of
 *   ((p1-p0) x (p2-p0)) . (p3-p0) as tn_tet_quality evaluates it, 0 also for NaN -- is not 0, and each of its four children has
 *   that orientation s.  Child i is the stored row with slot i replaced by the centroid c = ((p0 + p1) + (p2 + p3)) * 0.25f per
 *   coordinate, in fp32 with one rounding per operation and no fused multiply-add.  (A child fails where the rounded centroid
 *   lies on or across a face; the children are compared with the parent's own sign, stored rows being of either sign.)
 *   With k = the accepted tetrahedra below t and K their total: the new vertex is V + k; child 0 overwrites row t; children 1,
 *   2, 3 are rows T + 3k, T + 3k + 1, T + 3k + 2; cell_parent[row] = row for a row < T and the parent for an appended row;
 *   vertex_parents[k] = the parent's row as stored.
 * tn_split_count: offsets u32 [T+1] = exclusive sums of the accepted flags, K last (reading it back is the caller's one
 *   synchronisation); counters u32 [4], zeroed by the call: asked, accepted, refused for a flat or inverted parent or child,
 *   refused for an id >= V.
 * tn_split_emit: given offsets and num_new = K (a host value): xyz_out f32 [V+num_new,3], cells_out u32 [T+3 num_new,4],
 *   cell_parent u32 [T+3 num_new], vertex_parents u32 [num_new,4].  Accepted means offsets[t+1] > offsets[t]; select is not read
 *   again.  Every store is bounded by the num_new passed: a caller who changed the inputs between the two entries gets a wrong
 *   mesh, never a write outside its buffers.
 * tn_split_vertex_rows: a per-vertex array grown by the new vertices: out f32 [rows,V+K] = values f32 [rows,V] followed by K
 *   new columns, new_mode 0: ((x[a] + x[b]) + (x[c] + x[d])) * 0.25f with (a,b,c,d) = vertex_parents[k], the centroid's form;
 *   new_mode 1: zeros.  A parent id >= V gives 0.  out_vm f32 [V+K,rows] (nullable) is the transposition of out, bit-equal to
 *   tn_transpose_f32 of it, written in the same pass.  values_vm f32 [V,rows] (nullable) is the caller's transposition of values
 *   (the vertex-major shadow of the field): where given, the parent columns are read from it as rows and the old part of out_vm
 *   is a copy of it.  Carries the [64,V] field and both moments of its optimiser.
 * None needs a tracer.  All launch on `stream` and read nothing back; the only atomics are the four counters (one add per block);
 * tn_split_count takes its scratch as one stream-ordered allocation.  T == 0 or num_new == 0 gives empties or plain copies.
 * Errors (nothing is touched): a null pointer beside a non-zero count; num_new > num_cells; num_vertices + num_new >= 2^32 - 1;
 * num_cells + 3 num_new >= 2^30; rows == 0; an unknown new_mode. */
int tn_split_count(size_t num_vertices, size_t num_cells, const float *xyz, const uint32_t *cells, const uint8_t *select,
                   uint32_t *offsets, uint32_t *counters, void *stream);
int tn_split_emit(size_t num_vertices, size_t num_cells, const float *xyz, const uint32_t *cells, const uint32_t *offsets,
                  size_t num_new, float *xyz_out, uint32_t *cells_out, uint32_t *cell_parent, uint32_t *vertex_parents,
                  void *stream);
int tn_split_vertex_rows(size_t rows, size_t num_vertices, size_t num_new, const float *values, const float *values_vm,
                         const uint32_t *vertex_parents, uint32_t new_mode, float *out, float *out_vm, void *stream);

/* Vertex pruning (no reference counterpart: the reference's mesh is its input point cloud for the whole run).  Vertices whose
 * every tetrahedron is dead, and which lie on no hull face, are removed; the per-vertex arrays are compacted; the kept points get
 * their cells from the caller's triangulation (csrc/tn_prune.hip, the rule once in csrc/tn_prune_core.h, DESIGN.md section 4.21;
 * every output is bit-equal to geometry.prune_vertices_statement / geometry.prune_vertex_rows_statement).
 *   cells u32 [T,4], dead u8 [T] (non-zero = dead), faces u32 [F,3] and face_tets u32 [F,2] (the face table of those cells),
 *   vertex_select u8 [V] (nullable: every vertex is asked), all on the current device.
 *   A vertex is NAMED if a row of cells contains it, LIVE if a tetrahedron that is not dead names it (a row with an id >= V counts
 *   as live for its in-range ids), HULL if it is a vertex of a face with face_tets[f,1] == 0xFFFFFFFF; ids >= V in either table
 *   are skipped.  An asked vertex is kept because live, else kept because hull, else kept because no tetrahedron names it, else
 *   removed; a vertex that is not asked is kept.
 * tn_prune_count / tn_prune_count_tables: offsets u32 [V+1] = exclusive sums of the keep flags, V' last (reading it back is the
 *   caller's one synchronisation); counters u32 [5], zeroed by the call: asked, removed, kept live, kept hull, kept unreferenced.
 *   tn_prune_count reads the loaded mesh's own device cells and face tables (num_vertices must be the loaded V);
 *   tn_prune_count_tables reads the arrays given, on `device`.
 * tn_prune_emit: given offsets and num_kept = V' (a host value): new_id u32 [V] (offsets[v] for a kept vertex, 0xFFFFFFFF for a
 *   removed one), kept_ids u32 [num_kept] (the old id of each new vertex, ascending), xyz_out f32 [num_kept,3] = xyz[kept_ids].
 *   Every store is bounded by the num_kept passed.
 * tn_prune_vertex_rows: a per-vertex array compacted: out f32 [rows,num_kept] with out[r,j] = values[r,kept_ids[j]] (0 where
 *   kept_ids[j] >= V).  out_vm f32 [num_kept,rows] (nullable) is the transposition of out, bit-equal to tn_transpose_f32 of it,
 *   written in the same pass.  values_vm f32 [V,rows] (nullable) is the caller's transposition of values (the vertex-major shadow
 *   of the field): where given, the kept columns are read from it as rows.  Carries the [64,V] field and both moments of its
 *   optimiser.
 * None but tn_prune_count needs a tracer.  All launch on `stream` and read nothing back; the only atomics are the five counters
 * (one add per block); the count entries take their scratch as one stream-ordered allocation.  V == 0 or num_kept == 0 gives
 * empties.  Errors (nothing is touched): a null pointer beside a non-zero count; num_vertices >= 2^32 - 1; num_cells >= 2^30;
 * num_kept > num_vertices; rows == 0; tn_prune_count without a loaded mesh or with another num_vertices. */
int tn_prune_count(tn_tracer_t tracer, size_t num_vertices, const uint8_t *dead, const uint8_t *vertex_select, uint32_t *offsets,
                   uint32_t *counters, void *stream);
int tn_prune_count_tables(int device, size_t num_vertices, size_t num_cells, const uint32_t *cells, size_t num_faces,
                          const uint32_t *faces, const uint32_t *face_tets, const uint8_t *dead, const uint8_t *vertex_select,
                          uint32_t *offsets, uint32_t *counters, void *stream);
int tn_prune_emit(size_t num_vertices, const float *xyz, const uint32_t *offsets, size_t num_kept, uint32_t *new_id,
                  uint32_t *kept_ids, float *xyz_out, void *stream);
int tn_prune_vertex_rows(size_t rows, size_t num_vertices, size_t num_kept, const float *values, const float *values_vm,
                         const uint32_t *kept_ids, float *out, float *out_vm, void *stream);

/* Edge split (no reference counterpart: the reference's mesh is its input point cloud for the whole run).  Selected edges are
 * bisected at their midpoints together with every tetrahedron around them: the standard refinement, which halves the edge and the
 * volumes, needs no hanging node and keeps the hull and every other face of the ring (csrc/tn_edge_split.hip, the rule once in
 * csrc/tn_edge_split_core.h; every output is bit-equal to geometry.split_edges_statement).
 *   xyz f32 [V,3], cells u32 [T,4], select u8 [T] (non-zero = asked), faces u32 [F,3] and face_tets u32 [F,2] (the face table of
 *   those cells; a hull face has face_tets[f,1] == 0xFFFFFFFF), all on the current device.
 *   An EDGE is the sorted id pair (lo, hi), key = lo << 32 | hi; its squared length is (dx dx + dy dy) + dz dz of d = p[hi] - p[lo]
 *   in fp32, one rounding per operation, no fused multiply-add.  Edge e beats f iff it is longer, or as long with the smaller key.
 *   An asked tetrahedron whose ids are < V and whose stored orientation s (as tn_tet_quality evaluates it, 0 also for NaN) is not 0
 *   nominates its best edge; the CANDIDATES are the distinct nominated edges.  The ring of a candidate is every row that holds
 *   both its ids; the winner of a row is the best candidate among its six edges.  A candidate is refused, in this precedence, for
 *   an id >= V in a ring row; for lying on a hull face; because some ring row's winner is another edge; because a ring row has
 *   orientation 0 or one of its two children has not the row's orientation.  Otherwise it is ACCEPTED: accepted edges share no row.
 *   Accepted edges are ranked j in ascending key order; the new vertex V + j is ((p_lo + p_hi) + (p_lo + p_hi)) * 0.25f per
 *   coordinate and vertex_parents[j] = (lo, hi, lo, hi), so tn_split_vertex_rows carries the per-vertex arrays.  A bisected row t,
 *   with k = the bisected rows below it: child 0 (the slot holding hi replaced) overwrites row t, child 1 (the slot holding lo
 *   replaced) is row T + k; the other slots keep their stored order.
 * tn_edge_split_count / tn_edge_split_count_tables: tet_offsets u32 [T+1] = exclusive sums of the bisected flags; tet_edge u32 [T]
 *   = the rank j of the row's accepted edge, 0xFFFFFFFF for a row that is not bisected; bisected u8 [T]; edge_vertices u32 [T,2],
 *   of which the first K_v rows are written; counters u32 [10], zeroed by the call: asked, asked refused for an id, asked refused
 *   flat, candidates, candidates refused id / hull / lost / flat, accepted edges K_v, bisected tetrahedra K_t (reading them back is
 *   the caller's one synchronisation).  tn_edge_split_count reads the loaded mesh's own device cells and face tables (num_vertices
 *   must be the loaded V; xyz may be any positions of those vertices); tn_edge_split_count_tables reads the arrays given, on
 *   `device`.
 * tn_edge_split_emit: given those arrays and num_new = K_v, num_rows = K_t (host values): xyz_out f32 [V+num_new,3], cells_out u32
 *   [T+num_rows,4], cell_parent u32 [T+num_rows] (the row itself below T, the parent for an appended row), vertex_parents u32
 *   [num_new,4].  Every store is bounded by the two counts passed: a caller who changed the inputs between the two entries gets a
 *   wrong mesh, never a write outside its buffers.
 * Only tn_edge_split_count needs a tracer.  All launch on `stream` and read nothing back; the atomics are the ten counters (one add
 *   per block) and or-ed flag words, so no result depends on an order; the count entries take their scratch as one stream-ordered
 *   allocation.  T == 0 gives empties.  Errors (nothing is touched): a null pointer beside a non-zero count; num_new or num_rows >
 *   num_cells; num_vertices + num_new >= 2^32 - 1; num_cells + num_rows >= 2^30; num_faces >= 2^32 - 1; tn_edge_split_count without
 *   a loaded mesh or with another num_vertices. */
int tn_edge_split_count_tables(int device, size_t num_vertices, size_t num_cells, const float *xyz, const uint32_t *cells,
                               const uint8_t *select, size_t num_faces, const uint32_t *faces, const uint32_t *face_tets,
                               uint32_t *tet_offsets, uint32_t *tet_edge, uint8_t *bisected, uint32_t *edge_vertices,
                               uint32_t *counters, void *stream);
int tn_edge_split_count(tn_tracer_t tracer, size_t num_vertices, const float *xyz, const uint8_t *select, uint32_t *tet_offsets,
                        uint32_t *tet_edge, uint8_t *bisected, uint32_t *edge_vertices, uint32_t *counters, void *stream);
int tn_edge_split_emit(size_t num_vertices, size_t num_cells, const float *xyz, const uint32_t *cells, const uint32_t *tet_offsets,
                       const uint32_t *tet_edge, const uint32_t *edge_vertices, size_t num_new, size_t num_rows, float *xyz_out,
                       uint32_t *cells_out, uint32_t *cell_parent, uint32_t *vertex_parents, void *stream);

/* Delaunay repair by bistellar flips (no reference counterpart).  A CERTAINLY violated interior face -- tn_delaunay_check's own
 * verdict -- is removed by a 2-3 flip (its two tetrahedra become three around the new edge de) or by a 3-2 flip (three tetrahedra
 * around a reflex edge become two).  No vertex is added or moved, so every per-vertex array stays as it is (csrc/tn_flip.hip, the
 * rule once in csrc/tn_flip_core.h; every output is bit-equal to geometry.flip_faces_statement).
 *   xyz f32 [V,3], cells u32 [T,4], faces u32 [F,3] and face_tets u32 [F,2] (the face table of those cells; a hull face has
 *   face_tets[f,1] == 0xFFFFFFFF), all on the current device.
 *   For an interior face f: (a, b, c) = faces[f], t0, t1 = face_tets[f], d / e = the id of row t0 / t1 that the face does not name.
 *   A violated face is refused, in this precedence: ID (a row index >= T or an id >= V, decided before any read of xyz: such a face
 *   has no verdict); INVALID (the orientation of (a,b,c,d) or (a,b,c,e) is uncertain, or both have one sign); UNCERTAIN (one of
 *   o_k = orientation of (x_k, y_k, d, e), (x_k, y_k) = (a,b), (b,c), (c,a), is uncertain); UNFLIPPABLE (o_k is good iff it has the
 *   sign of (a,b,c,e); three good: 2-3; two good: 3-2, if one row t2 is the neighbour of t0 and of t1 across their faces opposite
 *   the third id and holds x_k, y_k, d, e of the bad k; anything else); LOST (a row it needs is claimed by a candidate with a smaller
 *   face id).  Otherwise it is accepted; accepted flips share no row: an independent set, not a maximal one -- call again for more.
 *   Children: (x_k, y_k, d, e) for every good k ascending.  Child 0 takes the place of t0, child 1 that of t1, the place of t2 is
 *   deleted (the new position of old row t is tet_offsets[t]), child 2 of a 2-3 flip is row (T - K32) + its rank among the accepted
 *   2-3 flips in ascending face id.
 * tn_flip_count / tn_flip_count_tables: tet_offsets u32 [T+1] = exclusive sums of "row t is not a deleted t2"; tet_flip u32 [T] =
 *   the accepted face that takes the row, 0xFFFFFFFF for an untouched one; flipped u8 [T]; face_flip u32 [F,3] = (code, t2, rank):
 *   (0, 0xFFFFFFFF, 0xFFFFFFFF) for a face that is not accepted, (1, 0xFFFFFFFF, rank) for a 2-3 flip, (2 + bad k, t2, 0xFFFFFFFF)
 *   for a 3-2 flip; counters u32 [10], zeroed by the call: interior faces, violated, verdict uncertain, refused id / invalid /
 *   uncertain / unflippable / lost, accepted 2-3 flips K23, accepted 3-2 flips K32 (reading them back is the caller's one
 *   synchronisation).  tn_flip_count reads the loaded mesh's own device cells and face tables (num_vertices must be the loaded V;
 *   xyz may be any positions of those vertices, NULL = the loaded ones); tn_flip_count_tables reads the arrays given, on `device`.
 * tn_flip_emit: given those arrays and num_23 = K23, num_32 = K32 (host values): cells_out u32 [T+num_23-num_32,4], cell_sources
 *   u32 [T+num_23-num_32,3] = the old rows whose union holds the new row, (t, 0xFFFFFFFF, 0xFFFFFFFF) for a copied one.  Every store
 *   is bounded by the two counts passed: a caller who changed the inputs between the two entries gets a wrong mesh, never a write
 *   outside its buffers.
 * Only tn_flip_count needs a tracer.  All launch on `stream` and read nothing back; the atomics are the ten counters (one add per
 *   block) and the claims (atomicMin), so no result depends on an order; the count entries take their scratch as one stream-ordered
 *   allocation.  T == 0 gives empties.  Errors (nothing is touched): a null pointer beside a non-zero count; num_cells or num_cells
 *   + num_23 >= 2^30; num_faces >= 2^32 - 1; num_23 or num_32 > num_faces; 2 num_23 + 3 num_32 > num_cells; tn_flip_count without
 *   a loaded mesh or with another num_vertices. */
int tn_flip_count_tables(int device, size_t num_vertices, size_t num_cells, const float *xyz, const uint32_t *cells, size_t num_faces,
                         const uint32_t *faces, const uint32_t *face_tets, uint32_t *tet_offsets, uint32_t *tet_flip,
                         uint8_t *flipped, uint32_t *face_flip, uint32_t *counters, void *stream);
int tn_flip_count(tn_tracer_t tracer, size_t num_vertices, const float *xyz, uint32_t *tet_offsets, uint32_t *tet_flip,
                  uint8_t *flipped, uint32_t *face_flip, uint32_t *counters, void *stream);
int tn_flip_emit(size_t num_cells, const uint32_t *cells, size_t num_faces, const uint32_t *faces, const uint32_t *face_tets,
                 const uint32_t *tet_offsets, const uint32_t *tet_flip, const uint32_t *face_flip, size_t num_23, size_t num_32,
                 uint32_t *cells_out, uint32_t *cell_sources, void *stream);
/* tn_flip_emit on the loaded mesh's own device cells and face tables: the second half of tn_flip_count (the tracer is not
 * touched; load the new cells to make it follow).  Error: no loaded mesh, and those of tn_flip_emit. */
int tn_flip_emit_loaded(tn_tracer_t tracer, const uint32_t *tet_offsets, const uint32_t *tet_flip, const uint32_t *face_flip,
                        size_t num_23, size_t num_32, uint32_t *cells_out, uint32_t *cell_sources, void *stream);

/* The face table of any cell rows, on the device and without a tracer: the face-table stage of load_tetrahedra's device build as
 * an entry of its own (csrc/tn_build.hip; the rule: face_hash_insert / face_is_first / face_emit of csrc/tn_build_core.h, in words
 * DESIGN.md section 4.24; every output is byte-equal to geometry.face_table_statement and to the table a load of the same cells
 * builds).  Sighting i = 4 t + j is local face j of row t: the ids cells[t][(j+1)&3], [(j+2)&3], [(j+3)&3].  Sightings are keyed by
 * their sorted id triple; one sighting is a hull face, two pair up, a third sets FLAG_TRIPLE_FACE.  A face's id is the rank of its
 * first sighting among the first sightings; its stored ids are its first sighting's, in that order.
 * tn_face_table_count: partner u32 [4T] = the other sighting of sighting i's face, 0xFFFFFFFF for none; face_index u32 [4T+1] =
 *   exclusive sums of "sighting i is the first of its face", the total F last; counters u32 [4], zeroed by the call: F, the number
 *   of hull faces, flag bits (1: an id >= num_vertices -- the table is still defined, only ids are compared; 2: a face with more
 *   than two sightings -- the table is then unspecified, and still nothing is written outside the buffers), a reserved 0.  The
 *   hash has the smallest power of two >= 8T + 16 slots; scratch is one stream-ordered allocation.
 * tn_face_table_emit: given those arrays and num_faces = F (a host value): faces u32 [num_faces,3], face_tets u32 [num_faces,2]
 *   (first sighting's row, the partner's row or 0xFFFFFFFF), tet_faces u32 [T,4] (may be NULL) = the face id of every sighting.
 *   A face whose id is >= num_faces is skipped whole (its tet_faces entries too): no store goes to a row >= num_faces.
 * Both launch on `stream` and read nothing back; the only atomics are the hash's claims and three counter adds per block, so no
 *   result depends on an order.  T == 0 gives empties and zero counters.  Errors (nothing is touched): a null pointer beside a
 *   non-zero count; num_cells >= 2^30; num_faces > 4 num_cells. */
int tn_face_table_count(int device, size_t num_vertices, size_t num_cells, const uint32_t *cells, uint32_t *partner,
                        uint32_t *face_index, uint32_t *counters, void *stream);
int tn_face_table_emit(size_t num_cells, const uint32_t *cells, const uint32_t *partner, const uint32_t *face_index, size_t num_faces,
                       uint32_t *faces, uint32_t *face_tets, uint32_t *tet_faces, void *stream);

/* number of unique faces of the loaded mesh (0 before load) */
size_t tn_num_faces(tn_tracer_t tracer);

/* copies the face tables to HOST buffers (test/debug aid; faces u32 [F,3] in first-seen
 * order with the unsorted first-seen triple, face_tets u32 [F,2]) */
int tn_get_faces(tn_tracer_t tracer, uint32_t *faces_host, uint32_t *face_tets_host);

/* test aid: copies one structure load_tetrahedra built to a HOST buffer.  which: 0 faces, 1 face_tets, 2 walk records
 * (64 B each), 3 hull nodes, 4 hull triangles, 5 BVH child rows, 6 BVH boxes, 7 BVH leaf ids, 8 BVH leaf triangles.
 * *bytes receives the size in bytes; dst may be NULL (size query). */
int tn_get_build_table(tn_tracer_t tracer, int which, void *dst, size_t *bytes);

/* TetrahedraTracer::trace_rays                         src/tetrahedra_tracer.h:311-331,
 *   TraceRaysPipeline::trace_rays                       src/tetrahedra_tracer.cpp:137-176,
 *   device programs                                      src/optix/optix_trace_rays.cu:268-331
 *   launch-parameter block `Params`                     src/optix_types.h:1-14
 * origins, directions f32 [R,3]; max_ray_triangles = M must be a power of two
 *   ("max_ray_triangles must be a power of 2.", py_binding.cpp:44-47).
 * num_visited u32 [R]; visited u32 [R,M]; bary f32 [R,M,2,3]; dist f32 [R,M,2];
 * verts u32 [R,M,4] (nullable, cf. optix_trace_rays.cu:220).
 * Slots >= num_visited[r]: visited/verts = 0xFFFFFFFF, bary/dist = 0. */
int tn_trace_rays(tn_tracer_t tracer, size_t num_rays, uint32_t max_ray_triangles,
                  const float *origins, const float *directions, uint32_t *num_visited,
                  uint32_t *visited, float *bary, float *dist, uint32_t *verts, void *stream);

/* tn_trace_rays with per-call flags (no reference counterpart: the reference always materialises the dense rows).
 * TN_TRACE_COMPACT_ROWS: slots >= num_visited[r] are left UNWRITTEN (and rows of rays that miss the mesh untouched but
 * for num_visited[r] = 0) -- for consumers that read the rows only through num_visited (tn_sample_*, tn_render_rays,
 * tn_find_matched_cells_indexed): 52 B per segment instead of 52*M B per ray.  A per-call argument rather than a tracer
 * option, so that threads sharing a tracer (nerfstudio's viewer and trainer share the model) cannot see each other's
 * choice.  Calls on ONE tracer handle are serialised inside the library (a per-tracer mutex around the host section: the
 * tracer's scratch buffers, counters, side streams and events are shared state); their kernels queue on the streams.
 *
 * TN_TRACE_BIN_RAYS (combines with TN_TRACE_COMPACT_ROWS): for batches of INCOHERENT rays (random pixels over many cameras).  The
 * library walks the rays in a locality order of its own -- a stable radix sort on a 30-bit key of (origin, direction, mesh
 * box): Morton cell of the origin, then Morton cell of the point of the ray's line closest to the centre of the mesh;
 * stated in tetra-nerf_amd/ray_order.py, computed by csrc/tn_ray_order.hip -- and still writes every output row at the
 * caller's ray index: the five arrays are bit for bit those of an unbinned call, and tn_trace_stats / tn_trace_flag_reasons /
 * tn_trace_cross_check report the same numbers.  Eligible is a call that takes the walk path as ONE chunk; a small batch on
 * the BVH path (below "walk_min_rays") and a call processed in ray chunks ("log_cap_mb") ignore the flag and produce the
 * same rows.  Costs 20 bytes of scratch per ray + the sort's temporary storage, allocated at the first binned call.
 * Option "bin_rays" = 1 / TETRANERF_HIP_BIN_RAYS=1 bins every eligible call without the flag. */
#define TN_TRACE_COMPACT_ROWS 1u
#define TN_TRACE_BIN_RAYS 2u
int tn_trace_rays_ex(tn_tracer_t tracer, size_t num_rays, uint32_t max_ray_triangles,
                     const float *origins, const float *directions, uint32_t *num_visited,
                     uint32_t *visited, float *bary, float *dist, uint32_t *verts, uint32_t flags, void *stream);

/* TetrahedraTracer::trace_rays_triangles                src/tetrahedra_tracer.h:333-352,
 *   device programs                                      src/optix/optix_trace_rays_triangles.cu:50-115
 * the sorted all-hits list of each ray, without the pairing stage (not called by the model).
 * visited u32 [R,M] face ids; bary f32 [R,M,2] = (u,v); dist f32 [R,M] = t; verts u32 [R,M,3] = the face's
 * stored vertex triple.  Slots >= num_visited[r]: 0 in every array (the reference's torch::zeros defaults). */
int tn_trace_rays_triangles(tn_tracer_t tracer, size_t num_rays, uint32_t max_ray_triangles,
                            const float *origins, const float *directions, uint32_t *num_visited,
                            uint32_t *visited, float *bary, float *dist, uint32_t *verts, void *stream);

/* TetrahedraTracer::find_tetrahedra                      src/tetrahedra_tracer.h:354-366,
 *   device programs                                      src/optix/optix_find_tetrahedra.cu:84-212
 * point location by two closest-hit rays (+x, -x): tetrahedra u32 [N] (0xFFFFFFFF = outside),
 * bary f32 [N,3] (weights of verts[1..3]; verts[0] has 1 - sum), verts u32 [N,4]; not found: bary/verts = 0. */
int tn_find_tetrahedra(tn_tracer_t tracer, size_t num_points, const float *positions, uint32_t *tetrahedra,
                       float *bary, uint32_t *verts, void *stream);

/* find_matched_cells                                   src/tetrahedra_tracer.h:380-393,
 *                                                       src/tetrahedra_tracer.cu:115-193
 * (PyTetrahedraTracer::find_visited_cells, src/py_binding.cpp:163-216; `cells` of the
 *  reference signature is unused there and omitted here)
 * distances f32 [R,S] ascending per ray.  Outputs: cells_out u32 [R,S] (default
 * 0xFFFFFFFF), verts_out u32 [R,S,4] (0xFFFFFFFF), mask_out u8 [R,S] (0), bary_out
 * f32 [R,S,3] (0). */
int tn_find_matched_cells(size_t num_rays, size_t num_samples, size_t max_visited_cells,
                          const uint32_t *num_visited, const uint32_t *visited,
                          const float *dist, const float *bary, const float *distances,
                          const uint32_t *verts, uint32_t *cells_out, uint32_t *verts_out,
                          uint8_t *mask_out, float *bary_out, void *stream);

/* The same for a SUBSET of the traced rays without compacting their rows first (addition): sample row r of
 * distances / outputs ([R,S...]) is matched against trace row ray_index[r] of the [*,M] arrays.  The model
 * compacts the 26 KB rows of the hitting rays with boolean indexing (model.py:560-567); this reads them in place. */
int tn_find_matched_cells_indexed(size_t num_rays, size_t num_samples, size_t max_visited_cells,
                                  const uint32_t *ray_index, const uint32_t *num_visited, const uint32_t *visited,
                                  const float *dist, const float *bary, const float *distances,
                                  const uint32_t *verts, uint32_t *cells_out, uint32_t *verts_out,
                                  uint8_t *mask_out, float *bary_out, const uint32_t *count /* see tn_compact_hits */,
                                  void *stream);

/* Compaction of the hitting rays ON THE DEVICE (addition; the reference compacts with boolean indexing, model.py:540-567 --
 * a device -> host synchronisation per call).  A stable partition of the rays of a trace call by num_visited > 0:
 * order u32 [R]: order[0 .. *count) = the rays that hit the mesh, in ray order, order[*count .. R) = the others, in ray order;
 * count u32 [1] stays in DEVICE memory; padded u32 [R] (nullable) = order with the entries from *count on replaced by
 * order[0] (a full-size index whose tail names a valid ray: what a padded, sync-free batch is gathered with).
 * scratch: 2 * ceil(R / 2048) uint32 of device memory (scratch_len = its length).
 * `count` ARGUMENTS of the entry points below (tn_sample_coarse, tn_sample_pdf, tn_find_matched_cells_indexed,
 * tn_mlp_forward_gather, tn_composite, tn_render_rays): a nullable device pointer to the number of rays to process; when it is
 * given, the size argument (num_hit_rays / num_rays / n) is only the UPPER BOUND the launch is sized for and the outputs are
 * allocated for -- rows from *count on are left unwritten -- so that nothing on the host ever waits for the ray count. */
int tn_compact_hits(size_t num_rays, const uint32_t *num_visited, uint32_t *order, uint32_t *count, uint32_t *padded,
                    uint32_t *scratch, size_t scratch_len, void *stream);

/* interpolate_values<D>                                src/tetrahedra_tracer.h:395-402,
 *                                                       src/tetrahedra_tracer.cu:195-221,250-266
 * vertex_indices u32 [n,D], barycentric f32 [n,D-1], field f32 [F,V] feature-major,
 * result f32 [F,n].  D in {2,3,4,6}, else
 * "Unsupported interpolation dimension with value <D>" (py_binding.cpp:258-276). */
int tn_interpolate_values(uint32_t interpolation_dim, uint32_t num_vertices,
                          uint32_t num_values, uint32_t field_dim,
                          const uint32_t *vertex_indices, const float *barycentric,
                          const float *field, float *result, void *stream);

/* interpolate_values_backward<D>                       src/tetrahedra_tracer.h:404-411,
 *                                                       src/tetrahedra_tracer.cu:223-248,268-290
 * grad_in f32 [F,n] (the transposed contiguous copy py_binding.cpp:369 makes),
 * field_grad_out f32 [F,V]: fully written (zero + scatter-add). */
int tn_interpolate_values_backward(uint32_t interpolation_dim, uint32_t num_vertices,
                                   uint32_t num_values, uint32_t field_dim,
                                   const uint32_t *vertex_indices, const float *barycentric,
                                   const float *grad_in, float *field_grad_out, void *stream);

/* The same with the gradient in the layout autograd hands over, grad_rows f32 [n,F] (sample-major):
 * saves the transposed copy of py_binding.cpp:369 (addition to the reference surface). */
int tn_interpolate_values_backward_rows(uint32_t interpolation_dim, uint32_t num_vertices,
                                        uint32_t num_values, uint32_t field_dim,
                                        const uint32_t *vertex_indices, const float *barycentric,
                                        const float *grad_rows, float *field_grad_out, void *stream);

/* Vertex-major variants (additions): the reference keeps its field feature-major [F,V] (checkpoint layout,
 * model.py:269-271), which makes every vertex row a 4-byte gather; these take a [V,F] shadow copy that the caller
 * refreshes once per field version with tn_transpose_f32 -- no per-call O(V) transposition and no temporaries.
 *   tn_transpose_f32: in [rows, cols] -> out [cols, rows]
 *   tn_interpolate_values_vm: field_vm f32 [V,F]; result f32 [F,n] as tn_interpolate_values
 *   tn_interpolate_values_backward_vm: grad_rows f32 [n,F]; field_grad_vm f32 [V,F] is ACCUMULATED into
 *     (zero it first; the adjoint of tn_transpose_f32 brings it back to [F,V])
 * ALIGNMENT: `result`, `field_vm` and `grad_rows` must be 16-byte aligned, here and in tn_interpolate_values[_backward*] and
 * tn_interpolate_values_backward_bary_vm: whenever a row is a multiple of 16 bytes (F % 4 == 0 for the [V,F] and [n,F] rows,
 * num_values % 4 == 0 for the [F,n] result rows) the kernels read and write it as 16-byte vectors. */
int tn_transpose_f32(uint32_t rows, uint32_t cols, const float *in, float *out, void *stream);
int tn_interpolate_values_vm(uint32_t interpolation_dim, uint32_t num_values, uint32_t field_dim,
                             const uint32_t *vertex_indices, const float *barycentric, const float *field_vm,
                             float *result, void *stream);
int tn_interpolate_values_backward_vm(uint32_t interpolation_dim, uint32_t num_values, uint32_t field_dim,
                                      const uint32_t *vertex_indices, const float *barycentric,
                                      const float *grad_rows, float *field_grad_vm, void *stream);
/* The same WITHOUT float atomics (addition; the reference's kernel, tetrahedra_tracer.cu:223-247, adds with atomicAdd and so
 * does tn_interpolate_values_backward_vm): the (sample, vertex) pairs are sorted by vertex and every gradient element is
 * summed by one writer in a fixed order -- bit-identical from run to run, 3-5x the time.  Needs num_vertices. */
int tn_interpolate_values_backward_vm_det(uint32_t interpolation_dim, uint32_t num_vertices, uint32_t num_values,
                                          uint32_t field_dim, const uint32_t *vertex_indices, const float *barycentric,
                                          const float *grad_rows, float *field_grad_vm, void *stream);

/* ---- position gradients (additions) -----------------------------------------------------------
 * What the reference leaves open: "TODO: implement grad computation wrt barycentric coords for pose optimisation"
 * (src/py_binding.cpp:354), and the one link it does ship as a batched PyTorch solve, add_barycentrics_grad
 * (tetranerf/utils/extension/__init__.py:45-68).  These two entry points complete both.  Tet membership, the sample
 * distances t, near / far and the sampler draws are constants of these gradients.
 *
 * (A) tn_interpolate_values_backward_bary_vm: the gather's adjoint w.r.t. the barycentrics.  With
 *       phi = b0 F[v1] + b1 F[v2] + ... + (1 - (b0 + b1 + ...)) F[v0]      (D - 1 barycentrics, D in {2,3,4,6})
 *     and grad_rows f32 [n,F] = dL/dphi as sample-major rows, field_vm f32 [V,F] the vertex-major field:
 *       grad_bary[s,k] = sum_c grad_rows[s,c] (F[v_{k+1},c] - F[v_0,c]),  k = 0 .. D-2;  f32 [n,D-1], every element written.
 *     The row of an EMPTY id (0xFFFFFFFF) is a zero row. */
int tn_interpolate_values_backward_bary_vm(uint32_t interpolation_dim, uint32_t num_values, uint32_t field_dim,
                                           const uint32_t *vertex_indices, const float *grad_rows, const float *field_vm,
                                           float *grad_bary, void *stream);
/* (B) tn_sample_positions_backward: the adjoint of the sample position (D = 4).  Sample s of ray r (row r * S + s of
 *     vertex_indices u32 [R*S,4], barycentric / grad_bary f32 [R*S,3]) lies in the tetrahedron with vertex positions x_0..x_3
 *     (rows of vertices f32 [V,3]).  With e_k = x_k - x_0, T = rows (e_1, e_2, e_3) and g = the sample's grad_bary row,
 *     p - x_0 = T^T b, so dL/dp = m where T m = g, in closed form
 *       m = (g_0 (e_2 x e_3) + g_1 (e_3 x e_1) + g_2 (e_1 x e_2)) / (e_1 . (e_2 x e_3)).
 *       grad_points     f32 [R*S,3]  m per sample                                              (written)
 *       grad_vertices   f32 [V,3]    vertex v_k receives -w_k m, w = (1 - (b0+b1+b2), b0, b1, b2)   (ACCUMULATED into, atomics)
 *       grad_origins    f32 [R,3]    sum_s m            (p = o + t d with t held constant)      (written, one writer per ray)
 *       grad_directions f32 [R,3]    sum_s t_s m,  t = distances f32 [R,S] (the sample distances handed to the matcher)
 *     A sample with an EMPTY or out-of-range id, a zero determinant or a non-finite m contributes exact zeros everywhere.
 *     Each of the four outputs may be null; distances may be null unless grad_directions is asked for. */
int tn_sample_positions_backward(size_t num_rays, uint32_t samples_per_ray, uint32_t num_vertices,
                                 const uint32_t *vertex_indices, const float *barycentric, const float *grad_bary,
                                 const float *distances, const float *vertices,
                                 float *grad_points, float *grad_origins, float *grad_directions,
                                 float *grad_vertices, void *stream);

/* Test aid: run only the dedupe / pairing / tail-fill stage
 * (post_process_tetrahedra, src/optix/optix_trace_rays.cu:110-266) on caller-supplied
 * sorted hit rows: hit_count u32 [R], hit_ids u32 [R,M], hit_t f32 [R,M], hit_uv f32 [R,M,2]. */
int tn_postprocess_hits(tn_tracer_t tracer, size_t num_rays, uint32_t max_ray_triangles,
                        const uint32_t *hit_count, const uint32_t *hit_ids, const float *hit_t,
                        const float *hit_uv, uint32_t *num_visited, uint32_t *visited,
                        float *bary, float *dist, uint32_t *verts, void *stream);

/* the same on caller-supplied face tables (faces u32 [F,3], face_tets u32 [F,2]) instead of a loaded mesh's:
 * lets hit lists that do not come from a mesh at hand -- the reference's tests/test_sort.py vectors -- be paired */
int tn_postprocess_hits_tables(int device, size_t num_rays, uint32_t max_ray_triangles, const uint32_t *faces,
                               const uint32_t *face_tets, const uint32_t *hit_count, const uint32_t *hit_ids,
                               const float *hit_t, const float *hit_uv, uint32_t *num_visited, uint32_t *visited,
                               float *bary, float *dist, uint32_t *verts, void *stream);

/* per-call statistics of the last tn_trace_rays on this tracer (host values; forces a
 * stream sync).  stats[0] = rays certified by the adjacency walk, stats[1] = all other rays (literal pairing of
 * their logged hits, or re-traced by the general all-hits path), stats[2] = rays whose post-process ran the serial
 * literal branch, stats[3] = rays that overflowed M-1 hits. */
int tn_trace_stats(tn_tracer_t tracer, uint64_t stats[4]);

/* diagnostic: why the adjacency walk did not certify rays of the last tn_trace_rays.
 * reasons[k], k = 1..12: 1 zero edge function / zero determinant on a hull face, 2 not exactly two
 * hull crossings, 3 equal hull distances, 4 a vertex of a visited tet within rounding distance of the ray,
 * 5 zero edge function, 6 not exactly two crossed faces in a tet, 7 a gap below eps / a tie / an inversion in t
 * (the chain is sound, its order is not certified), 9 more than M-1 faces, 10 invalid t after a valid one,
 * 11 exit face mismatch, 12 step limit, 8 fold guard: a tet whose neighbourhood holds a tet thinner than 32 rounding
 * distances AND one of whose edges passes within 8 rounding distances of the ray (csrc/tn_trace_walk.hip header).
 * Reason 7 rays keep their logged hits, which go through the literal sort + pairing (reasons[13] counts them);
 * all others are re-traced through the BVH all-hits path.  With option "verify_stride": reasons[15] = certified rays
 * cross-checked against a count-only BVH traversal, reasons[14] = those whose face count differed from the walk's
 * (re-traced through the BVH path; never observed). */
int tn_trace_flag_reasons(tn_tracer_t tracer, uint64_t reasons[16]);

/* The cross-check of the walk's certification in the last tn_trace_rays (host values; forces a stream sync).  Two populations of
 * CERTIFIED rays are re-counted by a count-only BVH all-hits traversal (a differing count re-traces the ray through the BVH path):
 *   the blind sample   every verify_stride-th ray:                      out[0] = stride, out[1] = checked, out[2] = mismatches
 *   the risk classes   EVERY ray inside the wide band (16 rounding distances by default; the guards that hand a ray over act at 8) of
 *                      a hull edge (out[3] = rays of that class) or of an edge of a thin-neighbourhood tet (out[4]):
 *                      out[5] = checked (those not already in the blind sample), out[6] = mismatches
 * See csrc/tn_trace_walk.hip (edge_band) and DESIGN.md section 2.  Option "verify_risk" = 0 switches the risk classes off. */
int tn_trace_cross_check(tn_tracer_t tracer, uint64_t out[8]);

/* Per-kernel breakdown of the last one-chunk walk call traced with option "timing" = 1 (measurement aid; bench.py prints it):
 * with that option the kernels of a call are enqueued on the CALLER's stream in program order with a timing event after each
 * (a normal call overlaps them on four streams, so its parts do not add up to its duration).  ms[0..7] = speculative tail fill,
 * adjacency walk, BVH re-trace of the fallback rays, count cross-check, segment writer, literal pairing of the logged hits,
 * tail fill, re-trace of cross-check mismatches.  A binned call (TN_TRACE_BIN_RAYS) counts its key kernel and its sort in
 * ms[1], with the hull entry search and the walk.  Waits for the call to finish. */
int tn_trace_timings(tn_tracer_t tracer, float ms[8]);

/* test / diagnostic aid: the order in which the LAST tn_trace_rays* call on this tracer walked its rays, copied to the host:
 * order_host[i] = caller index of the i-th walked ray.  *n receives the ray count when that call was binned
 * (TN_TRACE_BIN_RAYS or option "bin_rays", and eligible) and 0 when it was not; order_host may be NULL (size query).
 * Waits for the call's stream, like tn_trace_stats. */
int tn_trace_ray_order(tn_tracer_t tracer, uint32_t *order_host, size_t *n);

/* The constant tails of the dense reference rows (py_binding.cpp:53-57: torch::zeros / full(-1) of the five outputs) for slots
 * [first_slot, M) of EVERY row: visited / verts = 0xFFFFFFFF, bary / dist = 0.  first_slot must be a multiple of 32 (a 128-byte
 * line boundary in all four arrays); any other value fails rather than being rounded down over written segments.  The kernel is
 * k_fill_linear (csrc/tn_fill.hip: one linear stream per array, no per-row lookups; the tracer's own tail fill with option
 * "fill_blocks" = -2): what a caller that traced with TN_TRACE_COMPACT_ROWS runs if it later needs dense rows, and what bench.py
 * times to learn the write rate THIS box sustains (the ceiling of a trace_rays call, whose bytes are 88 % constant tails). */
int tn_fill_rows(size_t num_rays, uint32_t max_ray_triangles, uint32_t first_slot, uint32_t *visited, float *bary, float *dist,
                 uint32_t *verts, void *stream);

/* knobs ("walk", "gpu_build" and "bin_rays" also through the environment, read at tn_tracer_create: TETRANERF_HIP_WALK,
 * TETRANERF_HIP_GPU_BUILD, TETRANERF_HIP_BIN_RAYS):
 *   "walk"    1 = adjacency-walk fast path with general-path fallback (default),
 *             0 = general all-hits path for every ray, 2 = walk for any batch size
 *   "walk_min_rays"  smallest batch the walk is used for (default 12288; 8192 from 2M tets, 6144 from 4M tets on until
 *             the option is set; below it one wavefront per
 *             ray through the wide BVH has the lower latency).  Whatever the options say, the walk path needs
 *             max_ray_triangles >= 4 (16-byte stores into the rows); 1 and 2 take the BVH path
 *   "dense_tails"  1 (default) = every slot of the [R,M] rows is written, as the reference does;
 *             0 = slots >= num_visited[r] of walked rows are left UNWRITTEN (non-reference: for callers
 *             that only read rows through num_visited, e.g. tn_find_matched_cells; saves ~88 % of the bytes).
 *             Tracer-wide; prefer the per-call flag TN_TRACE_COMPACT_ROWS of tn_trace_rays_ex
 *   "literal" 1 (default) = rays whose order the walk cannot certify have their logged hits sorted and paired
 *             literally; 0 = they are re-traced through the BVH all-hits path (cross-check of the two paths)
 *   "spec_fill"  1 = the last quarter / half of every row (slots no ray, or hardly any ray, of this mesh reaches) is filled
 *             beside the walk on a stream of its own (the schedule of rounds 2-5); 0 (default since round 6) = the whole
 *             tail fill after the segment writer.  "spec_k0" = first speculatively filled slot (multiple of 32; 0 = the
 *             rule of csrc/tn_api_tracer.hip: spec_fill_first_slot) -- tests force it low so that rays of every class overwrite speculatively filled slots;
 *             "spec_blocks" (512) = grid of that fill, "walk_lds_kb" (26) = dynamic LDS reserved per walk block beside it
 *   "fill_blocks"  grid of the tail fill: -1 (default) = one block per row (k_fill_rows_fine), -2 = one linear stream per
 *             array with one store per thread (k_fill_linear: what tn_fill_rows uses), n > 0 = n blocks of persistent waves
 *   "writer_blocks"  grid of the segment writer (0 = default: 2 blocks per CU, what is resident at once)
 *   "hull_flat"  1 (default) = the walk's entry search (k_hull_entry) goes through the flat box table staged in LDS when the
 *             hull has at most 1024 faces; 0 = the threaded hull tree for every hull size (tests, A/B)
 *   "cert_ends"  statement of the walk's order test: 0 round 5's pairwise test, 3 the same + the end-of-chain rules A-C,
 *             1 the cluster test with rules A-D, 2 (default) = by mesh size.  Moves rays between the segment writer and the
 *             literal pairing kernel, never a byte of a row
 *   "log_cap_mb"  cap of the hit log in MiB (0 = default: a quarter of the free device memory, at most 24 GiB);
 *             larger calls are processed in ray chunks
 *   "gpu_build"  1 (default) = load_tetrahedra builds its structures on the device; 0 = single-threaded host build
 *   "leaf_width" 16 (default) / 32 / 64: faces per leaf of the face BVH (applies at the next tn_load_tetrahedra); the BVH
 *             path tests 64 / leaf_width crossed leaves per wave instruction
 *   "small_lds"  1 (default) = batches below walk_min_rays use LDS hit arrays sized for the mesh (every ray resident at
 *             once) and re-trace the rays with more hits in a second launch; "lds_cap" forces their size (tests)
 *   "verify_stride"  k > 0 (default 256): every k-th ray
 *             the walk certified is cross-checked: a count-only BVH all-hits
 *             traversal must find exactly the faces the walk logged, otherwise the ray is re-traced through the BVH path and
 *             counted in tn_trace_flag_reasons()[14].  A one-chunk call runs the check beside the row writers (< 1 % of the
 *             call; linear in the rays checked: tests and the fuzzer run it at 1); 0 = off.
 *             "verify_inject" 1 = every checked ray counts as a mismatch (tests of the hand-over)
 *   "literal_sort_passes"  (default 8) odd-even transposition passes over the nearly sorted hits the walk logged for a ray
 *             whose order it does not certify, before the bitonic network takes over (same result: distinct keys; tests run 0 and 1)
 *   "verify_risk"  1 (default) = every certified ray of the RISK classes is cross-checked as well (tn_trace_cross_check); 0 = only
 *             the blind sample.  "risk_band" (default 2) = width of the classes' band in units of the guards' own 8 rounding
 *             distances (2: rays between 8 and 16; measured cost in DESIGN.md section 2)
 *   "bin_rays"  0 (default) / 1 = every eligible tn_trace_rays* call is binned, as if it carried TN_TRACE_BIN_RAYS (see there)
 *   "timing"  1 = serialise the kernels of a one-chunk walk call on the caller's stream with timing events (tn_trace_timings);
 *             0 (default) = the overlapped four-stream schedule
 *   "writer_table"  0 (default) = the segment writer's record table by mesh size (one record per (tet, entry face) below
 *             500k tets, one per tet above), 1 / 2 force either (applies at the next tn_load_tetrahedra; tests, A/B)
 *   "refit_tables"  0 (default) / 1 = the next tn_load_tetrahedra (device build) keeps what tn_update_vertices needs
 *             (tn_refit_table_bytes; 26 .. 35 B per tet); 0 = a load launches and keeps exactly what it does without the option
 * Unknown names are an error. */
int tn_set_option(tn_tracer_t tracer, const char *name, int value);

/* gather_uint32<T> / scatter_ema_uint32<T>              src/tetrahedra_tracer.cu:30-113,
 *                                                       src/py_binding.cpp:374-431
 * (exported by the reference, not called by its model).  elem_size 4 = float32, 8 = float64.
 * gather: result[i] = values[indices[i]];  scatter: result[k] = result[k]*decay + (1-decay)*values[i], k = indices[i],
 * applied atomically per element (compare-and-swap).  Out-of-range indices are skipped. */
int tn_gather_uint32(int elem_size, uint32_t num_values, uint32_t num_indices, const uint32_t *indices,
                     const void *values, void *result, void *stream);
int tn_scatter_ema_uint32(int elem_size, uint32_t num_result, uint32_t num_indices, const uint32_t *indices,
                          double decay, const void *values, void *result, void *stream);

/* ---- shallow MLP + volume render (inference forward) ------------------------------------------
 * The arithmetic of these two lives in nerfstudio, not in /root/reference; the call sites are
 * tetranerf/nerfstudio/model.py:414-455 (modules), :602-621 (MLP + heads), :632-638 (weights and
 * renderers).  Weights use the nn.Linear layout [out, in], row-major fp32, i.e. what a reference
 * checkpoint holds (mlp_base.layers.{0,1,2}, field_output_density.net, mlp_head.layers.0,
 * field_output_color.net). */
typedef struct tn_mlp_weights {
    const float *w1, *b1; /* [128,64],  [128] */
    const float *w2, *b2; /* [128,128], [128] */
    const float *w3, *b3; /* [128,128], [128] */
    const float *wd, *bd; /* [1,128],   [1]    density head  */
    const float *wh, *bh; /* [128,155], [128]  mlp_head: columns [direction encoding 27 | base 128] */
    const float *wr, *br; /* [3,128],   [3]    rgb head      */
} tn_mlp_weights;

/* A handle owns the packed forms of ONE set of weights (per kernel family: fp32-MFMA forward with / without the fused
 * gather, bf16x3 pieces, transposed for the backward pass) and the small per-call scratch (direction encodings): the
 * entry points below neither pack nor allocate.  tn_mlp_set_weights packs; call it once per parameter VERSION (after
 * an optimiser step, after loading a checkpoint).  One handle serves one stream at a time. */
typedef struct tn_mlp *tn_mlp_t;
int tn_mlp_create(int device, tn_mlp_t *out);
int tn_mlp_destroy(tn_mlp_t mlp);
int tn_mlp_set_weights(tn_mlp_t mlp, const tn_mlp_weights *weights, void *stream);

/* Arithmetic `mode` of the two forward entry points (per call):
 *   0  v_mfma_f32_32x32x2_f32: an exact fp32 fma chain (157 TFLOP/s peak) -- what every parity claim refers to;
 *   1  "bf16x3": v_mfma_f32_32x32x16_bf16 on operands split into three bf16 pieces, six partial products per
 *      multiply, fp32 accumulation: dropped terms < 2^-24 of a product at 2.67x fewer matrix-core cycles (opt-in).
 *   2  "bf16": ONE v_mfma_f32_32x32x16_bf16 per product (opt-in, evaluation only, NOT at the parity bar of modes 0 and 1).  In
 *      the four wide layers (mlp_base layers 0, 1, 2; mlp_head layer 0 on [direction encoding 27 | base 128]) both operands
 *      of every product are rounded to bf16, round to nearest even -- the weight once by tn_mlp_set_weights, the input (the
 *      fp32 activation; the fp32 direction encoding) as it enters the matrix core; products are accumulated in fp32, bias and
 *      ray_head_bias added in fp32, ReLU taken in fp32; the narrow heads (density, rgb) read the fp32 activations and run in
 *      fp32.  Only these two entry points take it: tn_mlp_forward_gather_train[_ex] and tn_render_rays_ex reject mode 2.
 * feats f32 [64, n] feature-major (the buffer tn_interpolate_values writes), dirs f32 [n/samples_per_ray, 3]
 * (one direction per ray; samples of a ray are consecutive) -> sigma f32 [n] (softplus), rgb f32 [n,3] (sigmoid).
 * rgb == NULL: density only (mlp_base + density head: the coarse pass of the model, model.py:577-581); dirs unused. */
int tn_mlp_forward(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const float *feats, const float *dirs, int mode,
                   float *sigma, float *rgb, void *stream);

/* the same with the barycentric gather fused in (tn_interpolate_values<4> + tn_mlp_forward without the
 * [64,n] intermediate): vertex_indices u32 [n,4], barycentric f32 [n,3], field_vm f32 [V,64] VERTEX-major
 * (tn_transpose_f32 of the [64,V] parameter, refreshed by the caller once per field version) */
/* ray_head_bias f32 [n / samples_per_ray, 128] or NULL (here and in tn_mlp_forward_gather_train; tn_render_rays takes rows over ALL rays): a
 * per-RAY vector added to the pre-activation of mlp_head -- the reference's appearance embedding (model.py:437-447,
 * 608-620: head input = cat[encoded_dir, base, embedded_appearance], the embedding constant along a ray), whose E columns
 * of the head GEMM collapse to c_ray = Wh[:, 155:] emb(camera of the ray), an [rays, E] x [E, 128] product the caller
 * makes (and differentiates: tn_mlp_ray_head_grad returns dL/dc_ray).  wh of tn_mlp_weights stays [128, 155]. */
int tn_mlp_forward_gather(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const uint32_t *vertex_indices,
                          const float *barycentric, const float *field_vm, const float *dirs, int mode, float *sigma,
                          float *rgb, const float *ray_head_bias, const uint32_t *count /* device-side number of RAYS, nullable */,
                          void *stream);

/* ---- per-tetrahedron occupancy field (addition) ------------------------------------------------
 * The reference declares the field and leaves it unused: TetrahedraNerfConfig.use_occupancy_field registers a
 * `tetrahedra_occupancy` buffer, f32 [num_cells] (tetranerf/nerfstudio/model.py:98-99,256-265), exports gather_uint32 /
 * scatter_ema_uint32 for it, and get_outputs never reads or writes it.  The three entry points below finish it; all are
 * opt-in, on the caller's stream, without a host synchronisation.
 *
 * tn_occupancy_update: occupancy f32 [num_cells], in place:
 *     occupancy[t] = max(decay * occupancy[t], max{ sigma[i] : cells[i] == t })
 * cells u32 [n] = the matched tetrahedron of every sample (tn_find_matched_cells' cells_out; 0xFFFFFFFF = unmatched), sigma
 * f32 [n] their densities.  Samples whose cell is unmatched or >= num_cells, or whose sigma is not >= 0 (NaN, negative),
 * contribute nothing; every tetrahedron decays on every update (one rounding: fl32(decay * occupancy[t])); a NaN occupancy
 * stays NaN.  One linear pass, then one integer atomic maximum per run of equal cells on the float's bit pattern (accepted
 * sigmas are >= 0): independent of the order of the samples, identical from run to run.  count (nullable): device-side
 * number of RAYS of samples_per_ray samples each (see tn_compact_hits); samples from *count * samples_per_ray on are not read. */
int tn_occupancy_update(uint32_t num_cells, size_t n, const uint32_t *cells, const float *sigma, float decay, float *occupancy,
                        uint32_t samples_per_ray, const uint32_t *count, void *stream);

/* tn_cull_samples (the reference has no counterpart: model.py:98-99,256-265 declares the field and leaves it unused): a sample
 * is CULLED iff its cell is a valid id < num_cells and occupancy[cell] < threshold.  Unmatched samples stay live (they are
 * evaluated on zero features, as without a field), a NaN occupancy is live, threshold <= 0 culls nothing.
 * live u32 [n]: live[0 .. *live_count) = the indices of the live samples in ASCENDING order (a stable compaction: neighbours
 * on a ray stay neighbours in the list and share their vertices' field rows; the list equals torch.nonzero of the live mask);
 * live_count u32 [1] stays in DEVICE memory.  sigma f32 [n] and rgb f32 [n,3] (nullable) are set to 0 at every culled sample
 * and not touched at live ones; nothing is touched from sample *count * samples_per_ray on (count nullable, as above).
 * scratch: ceil(n / 1024) + 1 uint32 of device memory (scratch_len = its length): live samples per 1024-sample tile, scanned
 * by one block (tn_compact_hits' two levels plus that scan). */
int tn_cull_samples(size_t n, uint32_t samples_per_ray, const uint32_t *cells, const float *occupancy, uint32_t num_cells,
                    float threshold, uint32_t *live, uint32_t *live_count, float *sigma, float *rgb, uint32_t *scratch,
                    size_t scratch_len, const uint32_t *count, void *stream);

/* tn_mlp_forward_gather over the listed samples only (the consumer of tn_cull_samples; model.py:98-99,256-265 declares the
 * occupancy field and leaves it unused): slot i < *live_count of the launch computes sample s = live[i] -- it gathers at s, takes
 * the per-ray head term (and ray_head_bias row) of ray s / samples_per_ray and stores sigma[s] / rgb[s]; positions not listed
 * are NOT written.  All arrays keep the shapes of tn_mlp_forward_gather over n_max samples, which is also what the launch is
 * sized for; rgb == NULL: density only.  For every listed sample the result is bit for bit what tn_mlp_forward_gather gives
 * it in the same mode.  mode: 0 (fp32 MFMA) or 1 (bf16x3 MFMA); 2 (plain bf16) is refused.  List entries >= n_max (or, with
 * count, >= *count * samples_per_ray) are skipped. */
int tn_mlp_forward_gather_indexed(tn_mlp_t mlp, size_t n_max, uint32_t samples_per_ray, const uint32_t *live,
                                  const uint32_t *live_count, const uint32_t *vertex_indices, const float *barycentric,
                                  const float *field_vm, const float *dirs, int mode, float *sigma, float *rgb,
                                  const float *ray_head_bias, const uint32_t *count, void *stream);

/* ---- per-tetrahedron training statistics (addition; no reference counterpart: the reference never changes its mesh) ---------
 * tn_tet_stats_accumulate: stats i64 [num_cells, 3], ACCUMULATED in place (the caller zeroes it): per tetrahedron the number of
 * samples matched to it, the sum of their composite weights and the sum of weight x per-ray value (the caller's error of the
 * rendered pixel), the last two in fixed point with 32 fractional bits.  What a densification policy selects by.
 * Row q < min(num_rows, *count) (count nullable: all rows) holds samples_per_ray = S samples: cells u32 [num_rows, S] (the matched
 * tetrahedron, 0xFFFFFFFF = unmatched), sigma f32 [num_rows, S], edges f32 [num_rows, S + 1], and belongs to ray
 * r = ray_index ? ray_index[q] : q of ray_value f32 [rays] (nullable: every value 1; ray_index[q] must be a valid index of it).
 *   w   = the weight tn_composite(..., rgb = NULL, out_weights) writes for the same sigma and edges, bit for bit (the kernel calls
 *         the same device function; NaN -> 0 included)
 *   w^  = w >= 0 ? min(w, 1) : 0;     v^ = v >= 0 ? min(v, 256) : 0 with v = ray_value[r]   (NaN, negative, -0 -> 0)
 *   for every sample with cell t < num_cells (others contribute nothing):
 *     stats[t, 0] += 1;   stats[t, 1] += rint(w^ * 2^32);   stats[t, 2] += rint(fl32(w^ * v^) * 2^32)     (rint: half to even)
 * Rows from *count on are NOT read: they are the padded duplicates of the sync-free training form (tn_compact_hits) and would
 * be counted twice.  Integer sums: the result does not depend on the order of the samples or of the atomics, is identical from
 * run to run and equals the numpy statement (render.tet_stats_statement) byte for byte.  A term is at most 2^32 (weight) or 2^40
 * (error): a tetrahedron holds 2^31 resp. 2^23 = 8,388,608 accepted samples before a sum could pass 2^63; nothing saturates --
 * reset before that.  One wavefront per row, the row's weights in LDS, three 64-bit integer atomic adds per run of equal cells.
 * samples_per_ray: 1 .. 8192, more is refused (not truncated).  Caller's stream, no host synchronisation. */
int tn_tet_stats_accumulate(uint32_t num_cells, size_t num_rows, uint32_t samples_per_ray, const uint32_t *cells, const float *sigma,
                            const float *edges, const float *ray_value, const uint32_t *ray_index, const uint32_t *count,
                            int64_t *stats, void *stream);

/* ---- occupancy-guided coarse sampler (addition; model.py:98-99,256-265 declares the occupancy field and leaves it unused) -----
 * One wavefront per HITTING ray; the trace rows (num_visited u32 [R], visited u32 [R,M], hit_distances f32 [R,M,2]) are read in
 * place through ray_index u32 [r]; count as for tn_sample_coarse (rows from *count on are left unwritten).
 * A segment k of a ray is LIVE unless tn_cull_samples would cull its cell (visited < num_cells and occupancy[visited] <
 * threshold; invalid ids and a NaN occupancy are live, threshold <= 0 makes every segment live); w_k = max(t_out_k - t_in_k, 0)
 * for a live segment, else 0; cum = the prefix sums of w, L = their total.  A ray with L == 0 counts every segment live; a row
 * without a segment has near = 0, L = 1.  The LIVE-LENGTH coordinate s in [near, near + L] closes culled space up.
 * tn_sample_live (model.py:98-99,256-265): near_far_live f32 [r,2] = (first t_in, first t_in + L) and s_edges f32 [r, S+1] =
 *   tn_sample_coarse's uniform edges over that span (linspace f32 [S+1], t_rand f32 [r, S+1] or NULL, as there).
 * tn_live_to_distance (model.py:98-99,256-265): values f32 [r,n] in the live-length coordinate (bin centres, edges, a depth) ->
 *   t f32 [r,n] distances and slot u32 [r,n] segment indices: s' = clamp(s - near, 0, L), k = the first segment with cum[k+1] >
 *   s' (none: the last with w > 0), t = min(t_in_k + clamp((s' - cum[k]) / w_k, 0, 1) len_k, t_out_k): always inside a live
 *   segment of positive length when the ray has one.  A row without a segment: t = s, slot = 0.
 * Both need (max_ray_triangles + 1) * 16 B <= 64 KB of LDS per block and fail with a message beyond (as the biased sampler). */
int tn_sample_live(size_t num_hit_rays, uint32_t num_samples, uint32_t max_ray_triangles, const uint32_t *ray_index,
                   const uint32_t *num_visited, const uint32_t *visited, const float *hit_distances, const float *occupancy,
                   uint32_t num_cells, float threshold, const float *linspace, const float *t_rand, float *s_edges,
                   float *near_far_live, const uint32_t *count, void *stream);
int tn_live_to_distance(size_t num_hit_rays, uint32_t num_values, uint32_t max_ray_triangles, const uint32_t *ray_index,
                        const uint32_t *num_visited, const uint32_t *visited, const float *hit_distances, const float *occupancy,
                        uint32_t num_cells, float threshold, const float *values, float *t, uint32_t *slot, const uint32_t *count,
                        void *stream);

/* background colour of nerfstudio's RGBRenderer as the reference model configures / overrides it (model.py:466,504-518;
 * `renderers.BACKGROUND_COLOR_OVERRIDE`): comp_rgb + background (1 - accumulation).  clamp != 0 = the renderer's
 * evaluation mode (RGBRenderer.forward when not training): nan_to_num of the sample colours, result clamped to [0, 1].
 * A NULL pointer means white without clamp (the shipped configurations in training mode). */
typedef struct tn_rgb_background { float r, g, b; int clamp; } tn_rgb_background;
/* EVERYTHING between tn_trace_rays and the frame as ONE persistent launch (reference span
 * tetranerf/nerfstudio/model.py:531-662 in evaluation mode): coarse sampler (uniform or biased) -> find_visited_cells ->
 * interpolate_values + mlp_base + density head -> get_weights -> PDFSampler (include_original) -> find_visited_cells ->
 * interpolate_values + mlp_base + heads -> get_weights + RGB / accumulation / median-depth renderers, written into the frame.
 * The ray set is ray_index u32 [num_hit_rays_max] = tn_compact_hits' `order` and its SIZE lives on the device (count u32 [1];
 * NULL: all num_hit_rays_max entries) -- nothing on the host waits for the trace.  The trace rows are read in place; dirs f32
 * [R,3] and ray_head_bias f32 [R,128] (nullable) are arrays over ALL rays, indexed by ray; out_rgb f32 [R,3], out_acc f32 [R],
 * out_depth f32 [R] are written at the hitting rays' own rows (pre-fill them with the background values).
 * num_fine = 0: one pass over the coarse samples.  linspace f32 [S+1], u_table f32 [num_fine+1] (bin-centred quantiles),
 * histogram_padding / eps as in tn_sample_coarse / tn_sample_pdf.  fp32 MFMA arithmetic; every stage runs the same device
 * function as the stand-alone entry points, so the frame is bit-identical to tn_sample_coarse -> tn_find_matched_cells_indexed
 * -> tn_mlp_forward_gather -> tn_composite -> tn_sample_pdf -> ... (csrc/tn_render_rays.hip).
 * Needs max(2 M, 3 S + num_fine + 3) * 32 B <= 160 KB of LDS (M <= 2048 at the shipped sample counts). */
int tn_render_rays(tn_mlp_t mlp, uint32_t max_ray_triangles, const uint32_t *num_visited, const float *hit_distances,
                   const float *barycentric, const uint32_t *vertex_indices, const uint32_t *ray_index, const uint32_t *count,
                   size_t num_hit_rays_max, uint32_t num_samples, uint32_t num_fine, int biased, const float *linspace,
                   const float *u_table, float histogram_padding, float eps, const float *field_vm, const float *dirs,
                   const tn_rgb_background *background, float *out_rgb, float *out_acc, float *out_depth,
                   const float *ray_head_bias, void *stream);
/* ... with the arithmetic of the MLP phases as a per-call argument like tn_mlp_forward's `mode` (round 6): 0 = fp32 MFMA (what
 * tn_render_rays runs), 1 = bf16x3 (split-operand bf16 MFMA, csrc/tn_mlp_x3.hip; opt-in): then the frame is bit-identical to the
 * kernel chain run with mode 1.  Mode 2 is rejected (the kernel chain renders it).  Same reference span (model.py:531-662). */
int tn_render_rays_ex(tn_mlp_t mlp, uint32_t max_ray_triangles, const uint32_t *num_visited, const float *hit_distances,
                   const float *barycentric, const uint32_t *vertex_indices, const uint32_t *ray_index, const uint32_t *count,
                   size_t num_hit_rays_max, uint32_t num_samples, uint32_t num_fine, int biased, const float *linspace,
                   const float *u_table, float histogram_padding, float eps, const float *field_vm, const float *dirs,
                   const tn_rgb_background *background, float *out_rgb, float *out_acc, float *out_depth,
                   const float *ray_head_bias, int mode, void *stream);

/* ---- ray samplers between tn_trace_rays and the render passes (model.py:111-192, 549-557, 582-586; nerfstudio's
 * UniformSampler / PDFSampler for the parts the reference imports).  One wavefront per HITTING ray; the trace rows are
 * read in place through ray_index u32 [r] (as in tn_render_rays).
 * tn_sample_coarse: near / far of every hitting ray (near_far f32 [r,2]: first t_in, last t_out, model.py:531-544) and
 *   its num_samples + 1 coarse bin edges (edges f32 [r, S+1], euclidean): linspace f32 [S+1] = the spacing bins
 *   (torch.linspace(0, 1, S+1): the caller's table, so that both sides use the same values); t_rand f32 [r, S+1] uniform
 *   draws = training-mode stratified bins (model.py:166-175), NULL = evaluation; biased != 0: the edges are re-mapped so
 *   that every visited tetrahedron receives the same share of the samples (map_from_real_distances_to_biased_with_bounds,
 *   model.py:111-122).
 * tn_sample_pdf: PDFSampler with include_original (model.py:463,584): inverse-CDF samples of the coarse weights f32 [r,S]
 *   (+ histogram_padding, eps as in nerfstudio: 0.01, 1e-5) at the num_fine + 1 quantiles u_table f32 [num_fine+1]
 *   (evaluation: bin centres; training: bin starts + u_rand f32 [r, num_fine+1] / (num_fine+1), u_rand NULL otherwise),
 *   merged with the coarse edges: edges_out f32 [r, S + num_fine + 2], sorted, euclidean. */
int tn_sample_coarse(size_t num_hit_rays, uint32_t num_samples, uint32_t max_ray_triangles, const uint32_t *ray_index,
                     const uint32_t *num_visited, const float *hit_distances, const float *linspace, const float *t_rand,
                     int biased, float *edges, float *near_far, const uint32_t *count, void *stream);
int tn_sample_pdf(size_t num_hit_rays, uint32_t num_samples, uint32_t num_fine, const float *edges, const float *weights,
                  const float *near_far, const float *u_table, const float *u_rand, float histogram_padding, float eps,
                  float *edges_out, const uint32_t *count, void *stream);

/* RaySamples.get_weights + RGB (background blend) / accumulation / median-depth renderers.
 * sigma f32 [R,S], rgb f32 [R,S,3], edges f32 [R,S+1] (bin edges: starts = edges[:, :-1], ends = edges[:, 1:]);
 * out_rgb f32 [R,3], out_acc f32 [R], out_depth f32 [R], out_weights f32 [R,S] (nullable).
 * rgb == NULL and out_rgb == NULL: only out_weights is written (get_weights of the coarse pass, model.py:582).
 * ray_index u32 [R] (nullable): out_rgb / out_acc / out_depth are then arrays over ALL rays of the trace call and row q is
 * written at ray_index[q] (the scatter of model.py:640-662 into the frame, without an index_put pass). */
int tn_composite(size_t num_rays, uint32_t num_samples, const float *sigma, const float *rgb, const float *edges,
                 const tn_rgb_background *background, float *out_rgb, float *out_acc, float *out_depth,
                 float *out_weights, const uint32_t *ray_index, const uint32_t *count, void *stream);

/* ---- training: the MLP node and the composite node (PyTorch autograd in the reference: the trainer
 * back-propagates through nerfstudio's MLP / renderers, model.py:602-638).  Three calls per batch of n samples, all on
 * the handle's weights, fp32 MFMA:
 *   tn_mlp_forward_gather_train  = tn_mlp_forward_gather (mode 0) that also SAVES what the backward pass needs:
 *       x0 [64,n] gathered features, h1..h4 [128,n] layer outputs after ReLU (the operands of the weight-gradient
 *       GEMMs) and masks [4,n,2] u64 = the ReLU masks of h1..h4 (all the dX chain needs);
 *   tn_mlp_backward  runs the reverse network from the masks and the forward's OUTPUTS sigma [n] / rgb [n,3]
 *       (softplus' = 1 - exp(-sigma), sigmoid' = rgb (1 - rgb)) -- nothing is recomputed -- given d_sigma f32 [n],
 *       d_rgb f32 [n,3]; fills d1..d4 [128,n] (gradients w.r.t. the pre-activations of mlp_base layers 0..2 and of
 *       mlp_head), dhead [4,n] = d sigma_raw, d rgb_raw[0..2] (four plain rows), and dx0 [n,64] = the gradient of the
 *       gathered features as SAMPLE-major rows (feed it to tn_interpolate_values_backward_vm / _rows);
 *   The [F,n] tensors x0, h1..h4, d1..d4 are opaque to the caller and QUAD-major: [F/4][n][4] floats, element (feature
 *   f, sample s) at ((f / 4) n + s) 4 + f % 4 -- 16-byte stores for the kernels that produce them, 16-byte tile loads for
 *   the GEMMs that consume them.
 *   tn_mlp_param_grads  ACCUMULATES the gradients of the twelve parameter tensors (tn_mlp_grads: fp32 gradient buffers
 *       in nn.Linear layout, zeroed by the caller before the first batch) from those buffers: dW_l = d_l (input of
 *       layer l)^T as sample-streaming fp32-MFMA GEMMs (the 27 direction-encoding columns of mlp_head and the density
 *       head's vector ride along the mlp_head GEMM), the rgb head / bias sums as one bandwidth-bound pass; per-block
 *       partial sums are added in a fixed order (no atomics): bit-reproducible.  dirs f32 [n / samples_per_ray, 3].
 * All buffers are device memory owned by the caller (4.4 KB per sample in total). */
typedef struct tn_mlp_backward_buffers {
    float *x0, *h1, *h2, *h3, *h4;   /* forward -> param_grads */
    void *masks;                     /* forward -> backward: u64 [4, n, 2] */
    float *d1, *d2, *d3, *d4, *dhead, *dx0;   /* backward -> param_grads / gather adjoint */
} tn_mlp_backward_buffers;
int tn_mlp_forward_gather_train(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const uint32_t *vertex_indices,
                                const float *barycentric, const float *field_vm, const float *dirs, float *sigma, float *rgb,
                                const tn_mlp_backward_buffers *buffers, const float *ray_head_bias, void *stream);
/* The same with the arithmetic of the forward chosen per call: mode as in tn_mlp_forward_gather (0 fp32 MFMA =
 * tn_mlp_forward_gather_train, 1 bf16x3 MFMA).  Mode 1: sigma / rgb are bit for bit those of tn_mlp_forward_gather(mode 1), and
 * x0, h1..h4 and masks are saved in the same layouts, so tn_mlp_backward / tn_mlp_ray_head_grad / tn_mlp_param_grads run
 * unchanged (fp32) on them: the gradient is the exact fp32 adjoint at the bf16x3 forward's activations and ReLU decisions.
 * (The dX chain has an arithmetic of its own, chosen independently: tn_mlp_backward_ex below, and so do the weight-gradient
 * GEMMs: tn_mlp_param_grads_ex.)  Mode 2 is rejected: plain bf16 is an evaluation arithmetic. */
int tn_mlp_forward_gather_train_ex(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const uint32_t *vertex_indices,
                                   const float *barycentric, const float *field_vm, const float *dirs, int mode, float *sigma,
                                   float *rgb, const tn_mlp_backward_buffers *buffers, const float *ray_head_bias, void *stream);
int tn_mlp_backward(tn_mlp_t mlp, size_t n, const float *sigma, const float *rgb, const float *d_sigma, const float *d_rgb,
                    const tn_mlp_backward_buffers *buffers, void *stream);
/* The same with the arithmetic of the dX chain chosen per call, independently of the forward's: mode 0 (fp32 MFMA) IS
 * tn_mlp_backward -- the same launcher, the same bits; mode 1 (bf16x3 MFMA) evaluates the four matrix products of the chain
 * (Wh[:, 27:]^T d4, W3^T d3, W2^T d2, W1^T d1) on the bf16 matrix cores with three bf16 pieces per operand, six products per
 * multiply and fp32 accumulation, as the forward's mode 1 does.  Everything else stays fp32, operation for operation as in
 * mode 0: softplus' / sigmoid' from the forward's outputs, d4 = ReLU'(h4) Wr^T d rgb_raw, the density term wd d sigma_raw, the
 * ReLU masks and the transposition of dx0 -- so dhead and d4 are bit for bit those of mode 0, and d3, d2, d1, dx0 each follow
 * from the stored gradient before them within 2^-21 of the sum of the products' magnitudes.  Buffers and layouts are those of
 * tn_mlp_backward: tn_mlp_ray_head_grad, tn_mlp_param_grads (fp32 in either mode) and the gather adjoint run on them
 * unchanged.  Any other mode fails with a message (tn_last_error); mode 2, plain bf16, is an evaluation arithmetic.
 * Measured on an MI355X (profiles/train_x3_adjoint_bench.txt): 2.34 -> 1.62 ms at 4096 x 513 samples (1.45x), 1.21 -> 0.81 ms at
 * 4096 x 257 (1.49x); a training iteration -6.4 % / -6.3 % (tetra-nerf-original / tetra-nerf).  k_mlp_backward_x3: 256 VGPRs,
 * 172 bytes of scratch per lane, 2 waves per SIMD, 146 KB of LDS (one 8-wave block per CU). */
int tn_mlp_backward_ex(tn_mlp_t mlp, size_t n, const float *sigma, const float *rgb, const float *d_sigma, const float *d_rgb,
                       const tn_mlp_backward_buffers *buffers, int mode, void *stream);
/* gradient of the per-ray head bias after tn_mlp_backward: d_ray_head_bias f32 [n / samples_per_ray, 128] = the sum over
 * each ray's samples of d4 (bit-reproducible) */
int tn_mlp_ray_head_grad(size_t n, uint32_t samples_per_ray, const tn_mlp_backward_buffers *buffers, float *d_ray_head_bias,
                         void *stream);
typedef struct tn_mlp_grads { /* same shapes as tn_mlp_weights */
    float *w1, *b1, *w2, *b2, *w3, *b3, *wd, *bd, *wh, *bh, *wr, *br;
} tn_mlp_grads;
int tn_mlp_param_grads(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const float *dirs,
                       const tn_mlp_backward_buffers *buffers, const tn_mlp_grads *grads, void *stream);
/* The same with the arithmetic of the four weight-gradient GEMMs chosen per call, independently of the forward's and of the dX
 * chain's: mode 0 (fp32 MFMA) IS tn_mlp_param_grads -- the same launcher, the same bits; mode 1 (bf16x3 MFMA) evaluates d4 [h3 |
 * enc]^T, d3 h2^T, d2 h1^T and d1 x0^T on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, K = the sample axis): BOTH streamed
 * operands are split into three bf16 pieces (round to nearest even, residuals formed in fp32) once per element per block, as
 * they are staged into LDS, six products per multiply (hh, hm, mh, hl, lh, mm), fp32 accumulation -- each product within 2^-21
 * of |a| |b|.  Everything else stays fp32: the bias gradients (row sums of d1..d4) and d wd = sum d sigma_raw h3 are VALU
 * statements over the unsplit values, the rgb head / d bd / d br kernels are those of mode 0 (the same bits).  Buffers, layouts,
 * accumulation INTO grads, the scratch and the fixed-order reductions are those of tn_mlp_param_grads: no atomics,
 * bit-reproducible.  Any other mode fails with a message (tn_last_error); mode 2, plain bf16, is an evaluation arithmetic.
 * Measured on an MI355X: profiles/train_x3_dw_bench.txt. */
int tn_mlp_param_grads_ex(tn_mlp_t mlp, size_t n, uint32_t samples_per_ray, const float *dirs,
                          const tn_mlp_backward_buffers *buffers, const tn_mlp_grads *grads, int mode, void *stream);

/* Occupancy-culled TRAINING (the reference has no counterpart: model.py:98-99,256-265 declares the occupancy field and leaves it
 * unused).  The four entries below run a training batch on the n_live listed samples only; n_live is a HOST value (the caller
 * reads tn_cull_samples' *live_count back: one synchronisation per culled batch), live u32 [n_live] is ascending, n_samples is
 * the size of the uncompacted arrays.  Every tn_mlp_backward_buffers tensor holds n_live COMPACT columns in the usual quad-major
 * layout with stride n_live: column i belongs to sample live[i].  tn_mlp_backward[_ex] runs unchanged on such buffers with n =
 * n_live and compacted sigma / rgb / d_sigma / d_rgb (tn_compact_rows).  n_live == 0 is a valid call of each: no launch.
 *
 * tn_mlp_forward_gather_train_ex over the list (model.py:98-99,256-265): slot i gathers at s = live[i], takes the head term (and
 * ray_head_bias row) of ray s / samples_per_ray, stores sigma[s] / rgb[s] -- the bits tn_mlp_forward_gather_train_ex gives that
 * sample in the same mode -- and saves at column i.  Positions not listed are NOT written; a list entry >= n_samples stores no
 * output.  vertex_indices, barycentric, sigma, rgb cover n_samples samples, dirs and ray_head_bias n_samples / samples_per_ray
 * rays.  mode 0 (fp32 MFMA) or 1 (bf16x3 MFMA); 2 (plain bf16) is refused. */
int tn_mlp_forward_gather_train_indexed(tn_mlp_t mlp, size_t n_live, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live,
                                        const uint32_t *vertex_indices, const float *barycentric, const float *field_vm,
                                        const float *dirs, int mode, float *sigma, float *rgb, const tn_mlp_backward_buffers *buffers,
                                        const float *ray_head_bias, void *stream);
/* tn_mlp_param_grads_ex on compact buffers (model.py:98-99,256-265): the twelve gradients, ACCUMULATED, summed over the listed
 * samples; only the head layer's GEMM reads the list (the direction encoding of ray live[i] / samples_per_ray).  dirs f32
 * [n_samples / samples_per_ray, 3].  n_live == 0: grads untouched. */
int tn_mlp_param_grads_indexed(tn_mlp_t mlp, size_t n_live, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live,
                               const float *dirs, const tn_mlp_backward_buffers *buffers, const tn_mlp_grads *grads, int mode,
                               void *stream);
/* tn_mlp_ray_head_grad on compact buffers (model.py:98-99,256-265): d_ray_head_bias f32 [n_samples / samples_per_ray, 128], row r =
 * the sum of d4's columns whose sample belongs to ray r, in a fixed order; zeros for a ray without a live sample (all rows
 * when n_live == 0). */
int tn_mlp_ray_head_grad_indexed(size_t n_live, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live,
                                 const tn_mlp_backward_buffers *buffers, float *d_ray_head_bias, void *stream);
/* dst row i = src row live[i], i < n_live; rows of words_per_row = 1, 3 or 4 32-bit words (model.py:98-99,256-265: the vertex ids,
 * barycentrics, outputs and output gradients of the listed samples, for the per-sample kernels that read them by position).
 * Every list entry must be a row of src. */
int tn_compact_rows(uint32_t words_per_row, size_t n_live, const uint32_t *live, const void *src, void *dst, void *stream);

/* adjoint of tn_composite w.r.t. sigma [R,S] and rgb [R,S,3], given the gradients of the rendered rgb [R,3] and
 * accumulation [R] (either nullable); the median depth carries no gradient. */
int tn_composite_backward(size_t num_rays, uint32_t num_samples, const float *sigma, const float *rgb, const float *edges,
                          const tn_rgb_background *background, const float *d_out_rgb, const float *d_out_acc,
                          float *d_sigma, float *d_rgb, void *stream);

/* Expected-depth moment and distortion loss of a ray (addition, same ABI version: nothing existing changes).  Replaces, on the
 * training path, nerfstudio's DepthRenderer(method="expected") (model_components/renderers.py) and
 * losses.lossfun_distortion (model_components/losses.py; mip-NeRF 360 eq. 15), which run in PyTorch on the materialised
 * [R,S] weights, the distortion's pairwise term in O(S^2) per ray.  sigma f32 [R,S], edges f32 [R,S+1] non-decreasing per ray;
 * with w = tn_composite's weights (the same bits), delta_i = e_{i+1} - e_i, u'_i = ((e_i - e_0) + (e_{i+1} - e_0)) / 2:
 *   out_depth_moment f32 [R] = e_0 sum w_i + sum w_i u'_i                       (the caller divides by accumulation + eps)
 *   out_distortion   f32 [R] = sum_ij w_i w_j |u'_i - u'_j| + 1/3 sum_i w_i^2 delta_i   (the caller divides by e_S - e_0)
 *   out_weights      f32 [R,S]
 * each nullable.  Linear time per ray (prefix sums of w and w u'). */
int tn_composite_aux(size_t num_rays, uint32_t num_samples, const float *sigma, const float *edges, float *out_depth_moment,
                     float *out_distortion, float *out_weights, void *stream);

/* tn_composite_backward with the gradients of tn_composite_aux's two per-ray outputs, d_out_depth_moment f32 [R] and
 * d_out_distortion f32 [R] (either nullable), as further terms of dL/dw: the adjoint of DepthRenderer(method="expected")'s
 * numerator and of losses.lossfun_distortion, which PyTorch autograd forms through the materialised weights.  Edges are
 * constants of the gradient.  Everything else as tn_composite_backward. */
int tn_composite_backward_aux(size_t num_rays, uint32_t num_samples, const float *sigma, const float *rgb, const float *edges,
                              const tn_rgb_background *background, const float *d_out_rgb, const float *d_out_acc,
                              const float *d_out_depth_moment, const float *d_out_distortion, float *d_sigma, float *d_rgb,
                              void *stream);

/* The RAdam step of a training iteration (addition, same ABI version: nothing existing changes).  Replaces torch.optim.RAdam
 * (torch/optim/radam.py, the single-tensor form), the optimiser of the reference's one parameter group "fields" -- the vertex
 * field and the MLP (tetranerf/nerfstudio/registration.py:37-45) -- which PyTorch runs as a chain of element-wise launches over
 * whole tensors, and the transposition that its in-place step causes before the next gather.  Per element, every line one fp32
 * operation and one rounding, every scalar rounded to fp32 once by the caller:
 *   decay_mode 1 (coupled, decay = wd):            g = g + decay * p
 *   decay_mode 2 (decoupled, decay = 1 - lr wd):   p = p * decay
 *   m = m + one_minus_beta1 * (g - m)
 *   v = beta2 * v + (one_minus_beta2 * g) * g
 *   adaptive != 0:  p = p - (step_size * m) / (sqrt(v) + eps)        adaptive == 0:  p = p - step_size * m
 * with, for step count t >= 1 in double precision on the host: bc1 = 1 - b1^t, bc2 = 1 - b2^t, rho_inf = 2 / (1 - b2) - 1,
 * rho_t = rho_inf - 2 t b2^t / bc2; rho_t > 5: step_size = lr sqrt((rho_t-4)(rho_t-2) rho_inf / ((rho_inf-4)(rho_inf-2) rho_t))
 * sqrt(bc2) / bc1, adaptive = 1; otherwise step_size = lr / bc1, adaptive = 0.  m = exp_avg and v = exp_avg_sq keep torch's
 * layout (the parameter's), so optimiser state interchanges with torch.optim.RAdam.  fp32 denormals are kept and non-finite
 * gradients propagate as in torch; neither is part of the contract.  The caller's stream; no synchronisation, no allocation. */
typedef struct tn_radam_hyper {
    float one_minus_beta1, beta2, one_minus_beta2, eps, decay;
    int decay_mode;              /* 0: no weight decay, 1: coupled, 2: decoupled */
} tn_radam_hyper;
typedef struct tn_radam_tensor {
    float *param;                /* count contiguous f32; 4-byte alignment suffices */
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    size_t count;
    float step_size;             /* of THIS tensor's step count: parameters of a group can sit at different counts */
    int adaptive;
} tn_radam_tensor;
/* field, grad, exp_avg, exp_avg_sq f32 [64, num_vertices] feature-major, updated in place in one pass; shadow_vm f32
 * [num_vertices, 64] (nullable) receives the new field vertex-major in the same pass, bit-equal to tn_transpose_f32 of it. */
int tn_radam_step_field(uint32_t num_vertices, float *field, const float *grad, float *exp_avg, float *exp_avg_sq, float *shadow_vm,
                        float step_size, int adaptive, const tn_radam_hyper *hyper, void *stream);
/* num_tensors contiguous tensors of one parameter group, one launch per 32 of them; a tensor of count 0 is skipped. */
int tn_radam_step(size_t num_tensors, const tn_radam_tensor *tensors, const tn_radam_hyper *hyper, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TETRANERF_HIP_H */
