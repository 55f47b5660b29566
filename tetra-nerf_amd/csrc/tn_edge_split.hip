// tn_edge_split.hip -- tn_edge_split_count(_tables) and tn_edge_split_emit: selected edges bisected at their midpoints together
// with every tetrahedron around them (the rule: tn_edge_split_core.h).  The per-vertex arrays grow through
// the unchanged tn_split_vertex_rows (tn_split.hip): vertex_parents = (lo, hi, lo, hi).
//
//   k_esplit_nominate  lane per tetrahedron: select byte, cell row (16 B), four position gathers, one orientation in double; writes
//                      the key of its best edge, or the sentinel V << 32 that sorts behind every key; counts asked / refused id /
//                      refused flat.  rocprim::radix_sort_keys on bits [0, 32 + bit_width(V)).
//   k_esplit_heads     lane per sorted position: 1 where a run of equal keys that is not the sentinel starts; an exclusive scan over
//                      T + 1 flags numbers the candidates; their count C stays on the device (the last element).
//   k_esplit_compact   lane per sorted position: a head writes its key into the candidate list and zeroes its flag word.
//   k_esplit_rows      lane per tetrahedron, ALL rows: binary search of its six keys in the list, the winner, atomicOr of LOST / FLAT
//                      / ID into the flag words of the candidates it holds, the winner's index.
//   k_esplit_hull      lane per face: a hull face ors HULL into the flag words of its three edges.
//   k_esplit_classify  lane per candidate slot: the verdict by precedence, the accepted flag (slot T writes the 0 the scan turns into
//                      the total), five counters.  An exclusive scan gives the rank j of every accepted edge.
//   k_esplit_edges     lane per candidate: an accepted one writes edge_vertices[j].
//   k_esplit_tets      lane per tetrahedron: bisected byte, the rank of its accepted winner (tet_edge) and the flag the last scan
//                      turns into tet_offsets[T + 1]; counts the bisected rows.
//   k_esplit_vertices  (emit) lane per accepted edge: the midpoint and vertex_parents.
//   k_esplit_cells     (emit) lane per tetrahedron: copies the row or writes its two children and their parents.
//
// Every kernel is a grid-stride loop on at most ESPLIT_BLOCKS blocks (tn_mesh_ops.h).  The atomics are the ten counters (one add
// per block and counter) and the flag words (atomicOr of constants: no result depends on an order).  Scratch is ONE stream-ordered
// allocation (AsyncBytes; the count entries alone need any).  Every store is bounded by the counts the caller passed, every id is
// checked against V before it is used as an address.  Nothing is read back here.
#include <algorithm>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "tn_build.h"
#include "tn_mesh_ops.h"
#include "tn_edge_split_core.h"

namespace tn {

namespace {

constexpr int BT = 256;
constexpr unsigned ESPLIT_BLOCKS = 1024;   // grid cap of every kernel here (TetrahedraTracer.EDGE_SPLIT_GRID_LANES = ESPLIT_BLOCKS * BT)

// the length of the candidate list, as the scan left it on the device; never above the capacity T of the per-candidate arrays
__device__ __forceinline__ uint32_t cand_count(const uint32_t *__restrict__ num_cand, size_t T) {
    const uint32_t c = *num_cand;
    return c < T ? c : (uint32_t)T;
}

__device__ __forceinline__ void load_row(const uint32_t *__restrict__ cells, size_t t, uint32_t c[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = cells[4 * t + k];
}

__global__ __launch_bounds__(BT) void k_esplit_nominate(size_t T, uint32_t V, const float *__restrict__ xyz,
                                                        const uint32_t *__restrict__ cells, const uint8_t *__restrict__ select,
                                                        uint64_t *__restrict__ keys, uint32_t *__restrict__ counters) {
    uint32_t n[3] = {0u, 0u, 0u};   // asked, asked refused id, asked refused flat
    for (size_t t = gid(); t < T; t += stride<BT>()) {
        uint64_t key = esplit::sentinel(V);
        esplit::Nomination v = esplit::NOT_ASKED;
        if (select[t] != 0) {
            uint32_t c[4];
            load_row(cells, t, c);
            v = esplit::nominate(true, c, V, xyz, &key);
        }
        keys[t] = key;
        n[0] += v != esplit::NOT_ASKED;
        n[1] += v == esplit::ASKED_REFUSED_ID;
        n[2] += v == esplit::ASKED_REFUSED_FLAT;
    }
    block_count<BT>(n, counters + esplit::ASKED);
}

// flags[i], i in [0, T]: 1 where sorted position i starts a run of equal keys below the sentinel; flags[T] = 0
__global__ __launch_bounds__(BT) void k_esplit_heads(size_t T, uint32_t V, const uint64_t *__restrict__ sorted,
                                                     uint32_t *__restrict__ flags) {
    for (size_t i = gid(); i <= T; i += stride<BT>())
        flags[i] = i < T && sorted[i] < esplit::sentinel(V) && (i == 0 || sorted[i] != sorted[i - 1]);
}

// below = the exclusive scan of the head flags: a head's place in the candidate list (below[i] < T: the capacity of cand and eflags)
__global__ __launch_bounds__(BT) void k_esplit_compact(size_t T, const uint64_t *__restrict__ sorted, const uint32_t *__restrict__ below,
                                                       uint64_t *__restrict__ cand, uint32_t *__restrict__ eflags) {
    for (size_t i = gid(); i < T; i += stride<BT>()) {
        const uint32_t at = below[i];
        if (below[i + 1] == at || at >= T) continue;
        cand[at] = sorted[i];
        eflags[at] = 0u;
    }
}

__global__ __launch_bounds__(BT) void k_esplit_rows(size_t T, uint32_t V, const float *__restrict__ xyz,
                                                    const uint32_t *__restrict__ cells, const uint64_t *__restrict__ cand,
                                                    const uint32_t *__restrict__ num_cand, uint32_t *__restrict__ eflags,
                                                    uint32_t *__restrict__ winner) {
    const uint32_t C = cand_count(num_cand, T);
    for (size_t t = gid(); t < T; t += stride<BT>()) {
        uint32_t c[4], found[6], flag[6];
        load_row(cells, t, c);
        winner[t] = esplit::judge_row(c, V, xyz, cand, C, found, flag);
#pragma unroll
        for (int e = 0; e < 6; ++e)
            if (found[e] != esplit::EMPTY && flag[e]) atomicOr(eflags + found[e], flag[e]);   // found[e] < C <= T
    }
}

__global__ __launch_bounds__(BT) void k_esplit_hull(size_t F, size_t T, const uint32_t *__restrict__ faces,
                                                    const uint32_t *__restrict__ face_tets, const uint64_t *__restrict__ cand,
                                                    const uint32_t *__restrict__ num_cand, uint32_t *__restrict__ eflags) {
    const uint32_t C = cand_count(num_cand, T);
    if (C == 0) return;
    for (size_t f = gid(); f < F; f += stride<BT>()) {
        if (face_tets[2 * f + 1] != esplit::EMPTY) continue;
        uint32_t ids[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) ids[k] = faces[3 * f + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // (a key with an id >= V is above every candidate: it is never found, and never an address)
            const uint32_t at = esplit::find(cand, C, iso::edge_key(ids[k], ids[(k + 1) % 3]));
            if (at != esplit::EMPTY) atomicOr(eflags + at, esplit::FLAG_HULL);
        }
    }
}

__global__ __launch_bounds__(BT) void k_esplit_classify(size_t T, const uint32_t *__restrict__ num_cand,
                                                        const uint32_t *__restrict__ eflags, uint32_t *__restrict__ accepted,
                                                        uint32_t *__restrict__ counters) {
    const uint32_t C = cand_count(num_cand, T);
    uint32_t n[6] = {0u, 0u, 0u, 0u, 0u, 0u};   // candidates, refused id / hull / lost / flat, accepted
    for (size_t i = gid(); i <= T; i += stride<BT>()) {
        bool ok = false;
        if (i < C) {
            const esplit::Counter v = esplit::classify(eflags[i]);
            ok = v == esplit::ACCEPTED;
            n[0] += 1u;
            n[v - esplit::CANDIDATES] += 1u;
        }
        accepted[i] = ok;
    }
    block_count<BT>(n, counters + esplit::CANDIDATES);
}

// rank = the exclusive scan of the accepted flags; edge_vertices has room for T pairs and rank[i] < C <= T
__global__ __launch_bounds__(BT) void k_esplit_edges(size_t T, const uint32_t *__restrict__ num_cand, const uint64_t *__restrict__ cand,
                                                     const uint32_t *__restrict__ rank, uint32_t *__restrict__ edge_vertices) {
    const uint32_t C = cand_count(num_cand, T);
    for (size_t i = gid(); i < C; i += stride<BT>()) {
        const uint32_t j = rank[i];
        if (rank[i + 1] == j || j >= T) continue;
        edge_vertices[2 * (size_t)j] = (uint32_t)(cand[i] >> 32);
        edge_vertices[2 * (size_t)j + 1] = (uint32_t)cand[i];
    }
}

__global__ __launch_bounds__(BT) void k_esplit_tets(size_t T, const uint32_t *__restrict__ num_cand, const uint32_t *__restrict__ winner,
                                                    const uint32_t *__restrict__ rank, uint8_t *__restrict__ bisected,
                                                    uint32_t *__restrict__ tet_edge, uint32_t *__restrict__ flags,
                                                    uint32_t *__restrict__ counters) {
    const uint32_t C = cand_count(num_cand, T);
    uint32_t n[1] = {0u};
    for (size_t t = gid(); t <= T; t += stride<BT>()) {
        bool b = false;
        uint32_t j = esplit::EMPTY;
        if (t < T) {
            const uint32_t w = winner[t];
            if (w < C && rank[w + 1] != rank[w]) { b = true; j = rank[w]; }
            bisected[t] = b;
            tet_edge[t] = j;
        }
        flags[t] = b;
        n[0] += b;
    }
    block_count<BT>(n, counters + esplit::BISECTED);
}

__global__ __launch_bounds__(BT) void k_esplit_vertices(size_t num_new, uint32_t V, const float *__restrict__ xyz,
                                                        const uint32_t *__restrict__ edge_vertices, float *__restrict__ xyz_out,
                                                        uint32_t *__restrict__ vertex_parents) {
    for (size_t j = gid(); j < num_new; j += stride<BT>()) {
        const uint32_t lo = edge_vertices[2 * j], hi = edge_vertices[2 * j + 1];
        float m[3] = {0.f, 0.f, 0.f};
        if (lo < V && hi < V) {   // (false only where the caller changed the arrays between the two entries)
            float a[3], b[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { a[k] = xyz[3 * (size_t)lo + k]; b[k] = xyz[3 * (size_t)hi + k]; }
            esplit::midpoint(a, b, m);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) xyz_out[3 * ((size_t)V + j) + k] = m[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) vertex_parents[4 * j + k] = k & 1 ? hi : lo;
    }
}

__global__ __launch_bounds__(BT) void k_esplit_cells(size_t T, uint32_t V, const uint32_t *__restrict__ cells,
                                                     const uint32_t *__restrict__ tet_offsets, const uint32_t *__restrict__ tet_edge,
                                                     const uint32_t *__restrict__ edge_vertices, size_t num_new, size_t num_rows,
                                                     uint32_t *__restrict__ cells_out, uint32_t *__restrict__ cell_parent) {
    for (size_t t = gid(); t < T; t += stride<BT>()) {
        uint32_t c[4], child0[4], child1[4];
        load_row(cells, t, c);
        const size_t k = tet_offsets[t];
        const bool bisected = tet_offsets[t + 1] > tet_offsets[t] && k < num_rows;   // k < num_rows bounds the appended row
#pragma unroll
        for (int j = 0; j < 4; ++j) child0[j] = child1[j] = c[j];
        if (bisected) {
            const uint32_t j = tet_edge[t];
            int slot_lo, slot_hi;
            // (one of the two is false only where the caller changed the arrays between the two entries: the row is then copied)
            if (j < num_new && esplit::slots_of(c, edge_vertices[2 * (size_t)j], edge_vertices[2 * (size_t)j + 1], slot_lo, slot_hi)) {
                split::child_row(c, slot_hi, V + j, child0);
                split::child_row(c, slot_lo, V + j, child1);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) cells_out[4 * (T + k) + i] = child1[i];
            cell_parent[T + k] = (uint32_t)t;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) cells_out[4 * t + i] = child0[i];
        cell_parent[t] = (uint32_t)t;
    }
}

unsigned bit_width(uint64_t v) { unsigned b = 0; while (v) { ++b; v >>= 1; } return b; }

}  // namespace

void launch_edge_split_count(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint8_t *select, size_t F,
                             const uint32_t *faces, const uint32_t *face_tets, uint32_t *tet_offsets, uint32_t *tet_edge,
                             uint8_t *bisected, uint32_t *edge_vertices, uint32_t *counters, hipStream_t s) {
    TN_HIP(hipMemsetAsync(counters, 0, esplit::NUM_COUNTERS * sizeof(uint32_t), s));
    if (T == 0) {
        TN_HIP(hipMemsetAsync(tet_offsets, 0, sizeof(uint32_t), s));
        return;
    }
    const size_t n = T + 1;
    const unsigned end_bit = 32u + bit_width(V);   // the sentinel V << 32 has bit_width(V) bits above bit 32; V < 2^32 - 1
    size_t sort_bytes = 0;
    TN_HIP(rocprim::radix_sort_keys(nullptr, sort_bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, T, 0u, end_bit, s));
    const size_t tmp_bytes = std::max(sort_bytes, scan_bytes(n, s));
    const size_t key_bytes = align256(T * sizeof(uint64_t)), word_bytes = align256(n * sizeof(uint32_t));
    // keys | sorted keys | candidates | flags to scan | their scan (candidate numbers, then tet flags) | candidate flag words |
    // winners | accepted ranks | rocprim's scratch
    AsyncBytes all(3 * key_bytes + 5 * word_bytes + tmp_bytes, s);
    uint64_t *keys = all.at<uint64_t>(), *sorted = all.at<uint64_t>(key_bytes), *cand = all.at<uint64_t>(2 * key_bytes);
    uint32_t *words[5];
    for (int k = 0; k < 5; ++k) words[k] = all.at<uint32_t>(3 * key_bytes + k * word_bytes);
    uint32_t *flags = words[0], *below = words[1], *eflags = words[2], *winner = words[3], *rank = words[4];
    void *tmp = all.p + 3 * key_bytes + 5 * word_bytes;
    const uint32_t *num_cand = below + T;
    const dim3 grid_t(grid_for<BT, ESPLIT_BLOCKS>(T)), grid_n(grid_for<BT, ESPLIT_BLOCKS>(n)), block(BT);

    hipLaunchKernelGGL(k_esplit_nominate, grid_t, block, 0, s, T, (uint32_t)V, xyz, cells, select, keys, counters);
    TN_HIP(hipGetLastError());
    TN_HIP(rocprim::radix_sort_keys(tmp, sort_bytes, keys, sorted, T, 0u, end_bit, s));
    hipLaunchKernelGGL(k_esplit_heads, grid_n, block, 0, s, T, (uint32_t)V, sorted, flags);
    TN_HIP(hipGetLastError());
    scan(tmp, tmp_bytes, flags, below, n, s);
    hipLaunchKernelGGL(k_esplit_compact, grid_t, block, 0, s, T, sorted, below, cand, eflags);
    hipLaunchKernelGGL(k_esplit_rows, grid_t, block, 0, s, T, (uint32_t)V, xyz, cells, cand, num_cand, eflags, winner);
    if (F) hipLaunchKernelGGL(k_esplit_hull, dim3(grid_for<BT, ESPLIT_BLOCKS>(F)), block, 0, s, F, T, faces, face_tets, cand, num_cand, eflags);
    hipLaunchKernelGGL(k_esplit_classify, grid_n, block, 0, s, T, num_cand, eflags, flags, counters);
    TN_HIP(hipGetLastError());
    scan(tmp, tmp_bytes, flags, rank, n, s);
    hipLaunchKernelGGL(k_esplit_edges, grid_t, block, 0, s, T, num_cand, cand, rank, edge_vertices);
    hipLaunchKernelGGL(k_esplit_tets, grid_n, block, 0, s, T, num_cand, winner, rank, bisected, tet_edge, flags, counters);
    TN_HIP(hipGetLastError());
    scan(tmp, tmp_bytes, flags, tet_offsets, n, s);
}

void launch_edge_split_emit(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint32_t *tet_offsets,
                            const uint32_t *tet_edge, const uint32_t *edge_vertices, size_t num_new, size_t num_rows, float *xyz_out,
                            uint32_t *cells_out, uint32_t *cell_parent, uint32_t *vertex_parents, hipStream_t s) {
    if (V) TN_HIP(hipMemcpyAsync(xyz_out, xyz, 3 * V * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (num_new)
        hipLaunchKernelGGL(k_esplit_vertices, dim3(grid_for<BT, ESPLIT_BLOCKS>(num_new)), dim3(BT), 0, s, num_new, (uint32_t)V, xyz,
                           edge_vertices, xyz_out, vertex_parents);
    if (T)
        hipLaunchKernelGGL(k_esplit_cells, dim3(grid_for<BT, ESPLIT_BLOCKS>(T)), dim3(BT), 0, s, T, (uint32_t)V, cells, tet_offsets,
                           tet_edge, edge_vertices, num_new, num_rows, cells_out, cell_parent);
    TN_HIP(hipGetLastError());
}

}  // namespace tn
