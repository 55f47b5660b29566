// tn_prune.hip -- tn_prune_count(_tables), tn_prune_emit and tn_prune_vertex_rows: the removal of dead vertices, and the compaction
// of the per-vertex arrays that goes with it (the rule: tn_prune_core.h).  The kept points get their cells
// from triangulate() on the host; the per-tetrahedron values go through tn_remap_tet_values.  Nothing here touches cells.
//
//   k_prune_mark_tets   lane per tetrahedron: cell row (16 B) and dead byte; plain byte stores of 1 into `named` and `live`.
//   k_prune_mark_faces  lane per face: face_tets[f, 1], then the three ids; plain byte stores of 1 into `hull`.
//   k_prune_classify    lane per vertex: select byte and three marks -> the keep flag (lane V writes the 0 the scan turns into
//                       the total) and the five counts per lane; a block adds its sums to `counters` once (block_count,
//                       tn_mesh_ops.h).  rocprim::exclusive_scan gives offsets[V + 1].
//   k_prune_emit        lane per vertex: new_id, and where kept kept_ids and the 12-byte row of xyz at its new place.
//   k_prune_rows<from the shadow?>  block per 64 kept vertices x 64 rows through an LDS tile: the kept columns are read as rows of
//                       the vertex-major shadow (256 B each at 64 rows) or as single elements of the feature-major array;
//                       out[r, j] is stored along j and out_vm[j, r] along r, both whole lines.
//
// Every kernel is a grid-stride loop on at most PRUNE_BLOCKS blocks (tn_mesh_ops.h).  The only atomics are the five counters (one
// add per block and counter).  Scratch is ONE stream-ordered allocation (AsyncBytes; tn_prune_count alone needs any).  Every
// store is bounded by the counts the caller passed, every id is checked against V before it is used as an address.  Nothing is
// read back here.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "tn_build.h"
#include "tn_mesh_ops.h"
#include "tn_prune_core.h"

namespace tn {

namespace {

constexpr int BT = 256;
constexpr unsigned PRUNE_BLOCKS = 1024;   // grid cap of every kernel here (TetrahedraTracer.PRUNE_GRID_LANES = PRUNE_BLOCKS * BT)
constexpr int TILE = 64;                  // kept vertices and rows per block of k_prune_rows

__global__ __launch_bounds__(BT) void k_prune_mark_tets(size_t T, uint32_t V, const uint32_t *__restrict__ cells,
                                                        const uint8_t *__restrict__ dead, uint8_t *__restrict__ named,
                                                        uint8_t *__restrict__ live) {
    for (size_t t = gid(); t < T; t += stride<BT>()) {
        uint32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = cells[4 * t + k];
        prune::mark_tet(c, dead[t] != 0, V, named, live);
    }
}

__global__ __launch_bounds__(BT) void k_prune_mark_faces(size_t F, uint32_t V, const uint32_t *__restrict__ faces,
                                                         const uint32_t *__restrict__ face_tets, uint8_t *__restrict__ hull) {
    for (size_t f = gid(); f < F; f += stride<BT>()) {
        const uint32_t second = face_tets[2 * f + 1];
        if (second != prune::EMPTY) continue;
        uint32_t ids[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) ids[k] = faces[3 * f + k];
        prune::mark_face(ids, second, V, hull);
    }
}

__global__ __launch_bounds__(BT) void k_prune_classify(size_t V, const uint8_t *__restrict__ select, const uint8_t *__restrict__ named,
                                                       const uint8_t *__restrict__ live, const uint8_t *__restrict__ hull,
                                                       uint32_t *__restrict__ flags, uint32_t *__restrict__ counters) {
    uint32_t n[prune::NUM_COUNTERS] = {0u, 0u, 0u, 0u, 0u};
    for (size_t v = gid(); v <= V; v += stride<BT>()) {
        prune::Outcome o = prune::NOT_ASKED;
        if (v < V) o = prune::classify(!select || select[v] != 0, named[v] != 0, live[v] != 0, hull[v] != 0);
        flags[v] = v < V && o != prune::REMOVED;
        prune::count(o, n);
    }
    block_count<BT>(n, counters);
}

__global__ __launch_bounds__(BT) void k_prune_emit(size_t V, const float *__restrict__ xyz, const uint32_t *__restrict__ offsets,
                                                   size_t num_kept, uint32_t *__restrict__ new_id, uint32_t *__restrict__ kept_ids,
                                                   float *__restrict__ xyz_out) {
    for (size_t v = gid(); v < V; v += stride<BT>()) {
        const uint32_t j = offsets[v];
        const bool kept = offsets[v + 1] > j && j < num_kept;   // j < num_kept bounds every store below
        new_id[v] = kept ? j : prune::EMPTY;
        if (!kept) continue;
        kept_ids[j] = (uint32_t)v;
#pragma unroll
        for (int a = 0; a < 3; ++a) xyz_out[3 * (size_t)j + a] = xyz[3 * v + a];
    }
}

template <bool FROM_VM>
__global__ __launch_bounds__(BT) void k_prune_rows(size_t rows, size_t V, size_t Vp, const float *__restrict__ values,
                                                   const float *__restrict__ values_vm, const uint32_t *__restrict__ kept_ids,
                                                   float *__restrict__ out, float *__restrict__ out_vm) {
    __shared__ float tile[TILE][TILE + 1];   // [kept vertex][row]
    __shared__ uint32_t ids[TILE];
    const size_t rtiles = (rows + TILE - 1) / TILE, tiles = ((Vp + TILE - 1) / TILE) * rtiles;
    const int lane = threadIdx.x & (TILE - 1), quarter = threadIdx.x >> 6;   // BT / TILE = 4 quarters
    for (size_t tile_id = blockIdx.x; tile_id < tiles; tile_id += gridDim.x) {
        const size_t j0 = (tile_id / rtiles) * TILE, r0 = (tile_id % rtiles) * TILE;
        __syncthreads();   // the last trip's reads of the tile and the ids are done
        if (threadIdx.x < TILE) {
            const size_t j = j0 + threadIdx.x;
            ids[threadIdx.x] = j < Vp ? kept_ids[j] : prune::EMPTY;
        }
        __syncthreads();
        if (FROM_VM) {
            // phase 1, lanes along the rows: one 4 * rows-byte row of the shadow per kept vertex, out_vm along the rows
            for (int jj = quarter; jj < TILE; jj += BT / TILE) {
                const size_t j = j0 + jj, r = r0 + lane;
                if (j >= Vp || r >= rows) continue;
                const uint32_t id = ids[jj];
                const float v = id < V ? values_vm[(size_t)id * rows + r] : 0.f;
                tile[jj][lane] = v;
                if (out_vm) out_vm[j * rows + r] = v;
            }
            __syncthreads();
            // phase 2, lanes along the kept vertices: out[r, j]
            for (int rr = quarter; rr < TILE; rr += BT / TILE) {
                const size_t j = j0 + lane, r = r0 + rr;
                if (j < Vp && r < rows) out[r * Vp + j] = tile[lane][rr];
            }
        } else {
            // phase 1, lanes along the kept vertices: one element of row r per kept vertex, out[r, j] along j
            for (int rr = quarter; rr < TILE; rr += BT / TILE) {
                const size_t j = j0 + lane, r = r0 + rr;
                if (j >= Vp || r >= rows) continue;
                const uint32_t id = ids[lane];
                const float v = id < V ? values[r * V + id] : 0.f;
                tile[lane][rr] = v;
                out[r * Vp + j] = v;
            }
            if (out_vm) {   // (uniform over the block)
                __syncthreads();
                for (int jj = quarter; jj < TILE; jj += BT / TILE) {
                    const size_t j = j0 + jj, r = r0 + lane;
                    if (j < Vp && r < rows) out_vm[j * rows + r] = tile[jj][lane];
                }
            }
        }
    }
}

}  // namespace

void launch_prune_count(size_t V, size_t T, const uint32_t *cells, size_t F, const uint32_t *faces, const uint32_t *face_tets,
                        const uint8_t *dead, const uint8_t *select, uint32_t *offsets, uint32_t *counters, hipStream_t s) {
    TN_HIP(hipMemsetAsync(counters, 0, prune::NUM_COUNTERS * sizeof(uint32_t), s));
    if (V == 0) {
        TN_HIP(hipMemsetAsync(offsets, 0, sizeof(uint32_t), s));
        return;
    }
    const size_t n = V + 1, tmp_bytes = scan_bytes(n, s), mark_bytes = align256(V), flag_bytes = align256(n * sizeof(uint32_t));
    AsyncBytes all(3 * mark_bytes + flag_bytes + tmp_bytes, s);   // named | live | hull | keep flags | rocprim's scratch
    uint8_t *named = all.at<uint8_t>(), *live = all.at<uint8_t>(mark_bytes), *hull = all.at<uint8_t>(2 * mark_bytes);
    uint32_t *flags = all.at<uint32_t>(3 * mark_bytes);
    TN_HIP(hipMemsetAsync(named, 0, 3 * mark_bytes, s));
    if (T) {
        hipLaunchKernelGGL(k_prune_mark_tets, dim3(grid_for<BT, PRUNE_BLOCKS>(T)), dim3(BT), 0, s, T, (uint32_t)V, cells, dead, named,
                           live);
        TN_HIP(hipGetLastError());
    }
    if (F) {
        hipLaunchKernelGGL(k_prune_mark_faces, dim3(grid_for<BT, PRUNE_BLOCKS>(F)), dim3(BT), 0, s, F, (uint32_t)V, faces, face_tets,
                           hull);
        TN_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_prune_classify, dim3(grid_for<BT, PRUNE_BLOCKS>(n)), dim3(BT), 0, s, V, select, named, live, hull, flags,
                       counters);
    TN_HIP(hipGetLastError());
    scan(all.p + 3 * mark_bytes + flag_bytes, tmp_bytes, flags, offsets, n, s);
}

void launch_prune_emit(size_t V, const float *xyz, const uint32_t *offsets, size_t num_kept, uint32_t *new_id, uint32_t *kept_ids,
                       float *xyz_out, hipStream_t s) {
    if (V == 0) return;
    hipLaunchKernelGGL(k_prune_emit, dim3(grid_for<BT, PRUNE_BLOCKS>(V)), dim3(BT), 0, s, V, xyz, offsets, num_kept, new_id, kept_ids,
                       xyz_out);
    TN_HIP(hipGetLastError());
}

void launch_prune_vertex_rows(size_t rows, size_t V, size_t num_kept, const float *values, const float *values_vm,
                              const uint32_t *kept_ids, float *out, float *out_vm, hipStream_t s) {
    if (num_kept == 0) return;
    const size_t tiles = ((num_kept + TILE - 1) / TILE) * ((rows + TILE - 1) / TILE);
    const unsigned grid = (unsigned)std::min<size_t>(tiles, PRUNE_BLOCKS);
    if (values_vm)
        hipLaunchKernelGGL(k_prune_rows<true>, dim3(grid), dim3(BT), 0, s, rows, V, num_kept, values, values_vm, kept_ids, out, out_vm);
    else
        hipLaunchKernelGGL(k_prune_rows<false>, dim3(grid), dim3(BT), 0, s, rows, V, num_kept, values, values_vm, kept_ids, out, out_vm);
    TN_HIP(hipGetLastError());
}

}  // namespace tn
