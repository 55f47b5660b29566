// tn_isosurface.hip -- tn_isosurface_count and tn_isosurface_emit: the level set of the piecewise-linear interpolant of a
// per-vertex scalar over a tetrahedron soup, as a welded, consistently oriented triangle mesh in a deterministic order (the rule:
// tn_isosurface_core.h).
//
//   k_iso_count      lane per tetrahedron: mask byte, cell row (16 B), four value gathers; writes the triangle count (0, 1, 2)
//                    and the crossing-edge count (0, 3, 4).  Two rocprim::exclusive_scan calls turn them into tri_offsets[T + 1]
//                    and ref_offsets[T + 1]; the totals are the last elements.
//   k_iso_fill       lane per edge reference: key = all ones, payload = its own index (a slot k_iso_keys does not reach -- the
//                    caller changed `values` between the two entries -- then names no vertex and reads nothing).
//   k_iso_keys       lane per tetrahedron: the key (a << 32 | b, a < b) of each crossing edge at ref_offsets[t] + its rank among
//                    the tetrahedron's crossing edges in tet-edge order.
//   rocprim::radix_sort_pairs on bits [0, 32 + bit_width(V - 1)) of the keys, payload = the slot.
//   k_iso_heads      lane per sorted position: 1 where a run of equal keys starts; an exclusive scan over num_refs + 1 flags gives
//                    the welded id of every position (its inclusive count - 1) and the vertex count (the last element).
//   k_iso_vertices   lane per sorted position: slot_id[payload] = id; the head of a run writes edge_vertices, edge_t and
//                    positions of its vertex from the key alone; the last position writes the vertex count.
//   k_iso_triangles  lane per tetrahedron: the table rows, the orientation swap and the slot_id lookups give `triangles` and
//                    `triangle_tets` at tri_offsets[t] + row.
//
// Every kernel is a grid-stride loop on at most ISO_BLOCKS blocks (tn_mesh_ops.h).  No float atomics, no atomics at all: every
// output element has one writer, and the sort is stable, so nothing depends on scheduling.  Scratch is ONE stream-ordered
// allocation per entry (AsyncBytes, tn_mesh_ops.h; tn_interp.hip does the same for its sort).  Every store is bounded by the
// counts the caller passed; ids read from a key are checked against V.  Nothing is read back here: the caller reads the totals
// between the two entries.
#include <algorithm>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "tn_build.h"
#include "tn_mesh_ops.h"
#include "tn_isosurface_core.h"

namespace tn {

namespace {

constexpr int BT = 256;
constexpr unsigned ISO_BLOCKS = 1024;   // grid cap of every kernel here (TetrahedraTracer.ISOSURFACE_GRID_LANES = ISO_BLOCKS * BT)

// the case of tetrahedron t; c = its cell row (read only when the mask lets it through)
__device__ __forceinline__ iso::TetCase tet_case(size_t t, uint32_t V, const uint32_t *__restrict__ cells,
                                                 const float *__restrict__ values, float level,
                                                 const uint8_t *__restrict__ tet_mask, uint32_t c[4]) {
    const iso::TetCase none{0u, 0u, 0u, 0u};
    if (tet_mask && tet_mask[t] == 0) return none;
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = cells[4 * t + k];
    if (!iso::ids_ok(c, V)) return none;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = values[c[k]];
    return iso::classify(v, level);
}

// lanes T .. T (one past the tetrahedra) write the 0 the exclusive scans turn into the totals
__global__ __launch_bounds__(BT) void k_iso_count(size_t T, uint32_t V, const uint32_t *__restrict__ cells,
                                                  const float *__restrict__ values, float level,
                                                  const uint8_t *__restrict__ tet_mask, uint32_t *__restrict__ tri_count,
                                                  uint32_t *__restrict__ ref_count) {
    for (size_t t = gid(); t <= T; t += stride<BT>()) {
        uint32_t c[4];
        const iso::TetCase k = t < T ? tet_case(t, V, cells, values, level, tet_mask, c) : iso::TetCase{0u, 0u, 0u, 0u};
        tri_count[t] = k.ntri;
        ref_count[t] = k.nref;
    }
}

__global__ __launch_bounds__(BT) void k_iso_fill(size_t num_refs, uint64_t *__restrict__ keys, uint32_t *__restrict__ slots) {
    for (size_t i = gid(); i < num_refs; i += stride<BT>()) {
        keys[i] = ~0ull;
        slots[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(BT) void k_iso_keys(size_t T, uint32_t V, const uint32_t *__restrict__ cells,
                                                 const float *__restrict__ values, float level,
                                                 const uint8_t *__restrict__ tet_mask, const uint32_t *__restrict__ ref_offsets,
                                                 size_t num_refs, uint64_t *__restrict__ keys) {
    for (size_t t = gid(); t < T; t += stride<BT>()) {
        uint32_t c[4];
        const iso::TetCase k = tet_case(t, V, cells, values, level, tet_mask, c);
        if (k.nref == 0) continue;
        size_t slot = ref_offsets[t];
#pragma unroll
        for (int e = 0; e < 6; ++e)
            if ((k.cross >> e) & 1u) {
                if (slot < num_refs) keys[slot] = iso::edge_key(c[iso::EDGE_CORNERS[e][0]], c[iso::EDGE_CORNERS[e][1]]);
                ++slot;
            }
    }
}

// flags[i], i in [0, num_refs]: 1 where sorted position i starts a run of equal keys; flags[num_refs] = 0
__global__ __launch_bounds__(BT) void k_iso_heads(size_t num_refs, const uint64_t *__restrict__ sorted_keys,
                                                  uint32_t *__restrict__ flags) {
    for (size_t i = gid(); i <= num_refs; i += stride<BT>())
        flags[i] = i < num_refs && (i == 0 || sorted_keys[i] != sorted_keys[i - 1]);
}

// below[i] = heads in front of sorted position i (the exclusive scan of the flags): below[i + 1] - 1 is the welded id of i
__global__ __launch_bounds__(BT) void k_iso_vertices(size_t num_refs, uint32_t V, const uint64_t *__restrict__ sorted_keys,
                                                     const uint32_t *__restrict__ sorted_slots, const uint32_t *__restrict__ below,
                                                     const float *__restrict__ xyz, const float *__restrict__ values, float level,
                                                     uint32_t *__restrict__ slot_id, uint32_t *__restrict__ edge_vertices,
                                                     float *__restrict__ edge_t, float *__restrict__ positions,
                                                     uint32_t *__restrict__ num_out_vertices) {
    for (size_t i = gid(); i < num_refs; i += stride<BT>()) {
        const uint32_t before = below[i], upto = below[i + 1];
        const uint32_t id = upto - 1u;                     // upto >= 1: position 0 is a head
        const uint32_t slot = sorted_slots[i];
        if (slot < num_refs) slot_id[slot] = id;
        if (upto != before) {                              // a head: id < num_refs, the capacity of the vertex outputs
            const uint64_t key = sorted_keys[i];
            const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
            float t = 0.f, p[3] = {0.f, 0.f, 0.f};
            if (a < V && b < V) {
                float xa[3], xb[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) { xa[k] = xyz[3 * (size_t)a + k]; xb[k] = xyz[3 * (size_t)b + k]; }
                t = iso::edge_vertex(values[a], values[b], level, xa, xb, p);
            }
            edge_vertices[2 * (size_t)id] = a;
            edge_vertices[2 * (size_t)id + 1] = b;
            edge_t[id] = t;
#pragma unroll
            for (int k = 0; k < 3; ++k) positions[3 * (size_t)id + k] = p[k];
        }
        if (i + 1 == num_refs) *num_out_vertices = upto;
    }
}

__global__ __launch_bounds__(BT) void k_iso_triangles(size_t T, uint32_t V, const float *__restrict__ xyz,
                                                      const uint32_t *__restrict__ cells, const float *__restrict__ values,
                                                      float level, const uint8_t *__restrict__ tet_mask,
                                                      const uint32_t *__restrict__ tri_offsets,
                                                      const uint32_t *__restrict__ ref_offsets, size_t num_triangles, size_t num_refs,
                                                      const uint32_t *__restrict__ slot_id, uint32_t *__restrict__ triangles,
                                                      uint32_t *__restrict__ triangle_tets) {
    for (size_t t = gid(); t < T; t += stride<BT>()) {
        uint32_t c[4];
        const iso::TetCase k = tet_case(t, V, cells, values, level, tet_mask, c);
        if (k.ntri == 0) continue;
        float p[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int a = 0; a < 3; ++a) p[j][a] = xyz[3 * (size_t)c[j] + a];
        const bool negative = guard::tet_orient(p) < 0;
        const size_t tri0 = tri_offsets[t], ref0 = ref_offsets[t];
        for (uint32_t row = 0; row < k.ntri; ++row) {
            const size_t tri = tri0 + row;
            if (tri >= num_triangles) break;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const size_t slot = ref0 + iso::edge_rank(k.cross, iso::TRI_TABLE[k.code][row][iso::tri_corner(j, negative)]);
                triangles[3 * tri + j] = slot < num_refs ? slot_id[slot] : 0u;
            }
            triangle_tets[tri] = (uint32_t)t;
        }
    }
}

unsigned bit_width(uint64_t v) { unsigned b = 0; while (v) { ++b; v >>= 1; } return b; }

}  // namespace

void launch_isosurface_count(size_t V, size_t T, const uint32_t *cells, const float *values, float level, const uint8_t *tet_mask,
                             uint32_t *tri_offsets, uint32_t *ref_offsets, hipStream_t s) {
    if (T == 0) {
        TN_HIP(hipMemsetAsync(tri_offsets, 0, sizeof(uint32_t), s));
        TN_HIP(hipMemsetAsync(ref_offsets, 0, sizeof(uint32_t), s));
        return;
    }
    const size_t n = T + 1, tmp_bytes = scan_bytes(n, s), count_bytes = align256(n * sizeof(uint32_t));
    AsyncBytes all(2 * count_bytes + tmp_bytes, s);   // triangle counts | crossing-edge counts | rocprim's scratch
    uint32_t *tri_count = all.at<uint32_t>(), *ref_count = all.at<uint32_t>(count_bytes);
    void *tmp = all.p + 2 * count_bytes;
    hipLaunchKernelGGL(k_iso_count, dim3(grid_for<BT, ISO_BLOCKS>(n)), dim3(BT), 0, s, T, (uint32_t)V, cells, values, level, tet_mask,
                       tri_count, ref_count);
    TN_HIP(hipGetLastError());
    scan(tmp, tmp_bytes, tri_count, tri_offsets, n, s);
    scan(tmp, tmp_bytes, ref_count, ref_offsets, n, s);
}

void launch_isosurface_emit(size_t V, size_t T, const float *xyz, const uint32_t *cells, const float *values, float level,
                            const uint8_t *tet_mask, const uint32_t *tri_offsets, const uint32_t *ref_offsets, size_t num_triangles,
                            size_t num_refs, uint32_t *triangles, uint32_t *triangle_tets, uint32_t *edge_vertices, float *edge_t,
                            float *positions, uint32_t *num_out_vertices, hipStream_t s) {
    if (T == 0 || num_refs == 0) {
        TN_HIP(hipMemsetAsync(num_out_vertices, 0, sizeof(uint32_t), s));
        return;
    }
    const size_t nr = num_refs;
    const unsigned end_bit = 32u + (V > 1 ? bit_width(V - 1) : 0u);   // V < 2^32 - 1: at most 64
    size_t sort_bytes = 0;
    // (the iterator types of the size query are those of the call below: one instantiation of the sort, and not tn_build.hip's)
    TN_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                     (uint32_t *)nullptr, nr, 0u, end_bit, s));
    const size_t tmp_bytes = std::max(sort_bytes, scan_bytes(nr + 1, s));
    const size_t key_bytes = align256(nr * sizeof(uint64_t)), word_bytes = align256((nr + 1) * sizeof(uint32_t));
    // keys | sorted keys | slots | sorted slots | head flags | their scan | slot -> welded id | rocprim's scratch
    AsyncBytes all(2 * key_bytes + 5 * word_bytes + tmp_bytes, s);
    uint64_t *keys = all.at<uint64_t>(), *sorted_keys = all.at<uint64_t>(key_bytes);
    uint32_t *words[5];
    for (int k = 0; k < 5; ++k) words[k] = all.at<uint32_t>(2 * key_bytes + k * word_bytes);
    uint32_t *slots = words[0], *sorted_slots = words[1], *flags = words[2], *below = words[3], *slot_id = words[4];
    void *tmp = all.p + 2 * key_bytes + 5 * word_bytes;

    hipLaunchKernelGGL(k_iso_fill, dim3(grid_for<BT, ISO_BLOCKS>(nr)), dim3(BT), 0, s, nr, keys, slots);
    hipLaunchKernelGGL(k_iso_keys, dim3(grid_for<BT, ISO_BLOCKS>(T)), dim3(BT), 0, s, T, (uint32_t)V, cells, values, level, tet_mask,
                       ref_offsets, nr, keys);
    TN_HIP(hipGetLastError());
    TN_HIP(rocprim::radix_sort_pairs(tmp, sort_bytes, keys, sorted_keys, slots, sorted_slots, nr, 0u, end_bit, s));
    hipLaunchKernelGGL(k_iso_heads, dim3(grid_for<BT, ISO_BLOCKS>(nr + 1)), dim3(BT), 0, s, nr, sorted_keys, flags);
    TN_HIP(hipGetLastError());
    scan(tmp, tmp_bytes, flags, below, nr + 1, s);
    hipLaunchKernelGGL(k_iso_vertices, dim3(grid_for<BT, ISO_BLOCKS>(nr)), dim3(BT), 0, s, nr, (uint32_t)V, sorted_keys, sorted_slots,
                       below, xyz, values, level, slot_id, edge_vertices, edge_t, positions, num_out_vertices);
    if (num_triangles)
        hipLaunchKernelGGL(k_iso_triangles, dim3(grid_for<BT, ISO_BLOCKS>(T)), dim3(BT), 0, s, T, (uint32_t)V, xyz, cells, values,
                           level, tet_mask, tri_offsets, ref_offsets, num_triangles, nr, slot_id, triangles, triangle_tets);
    TN_HIP(hipGetLastError());
}

}  // namespace tn
