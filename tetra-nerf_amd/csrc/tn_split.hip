// tn_split.hip -- tn_split_count, tn_split_emit and tn_split_vertex_rows: the 1 -> 4 split of selected tetrahedra at their
// centroids, and the growth of the per-vertex arrays that go with it (the rule: tn_split_core.h).
//
//   k_split_flags     lane per tetrahedron: select byte, cell row (16 B), four position gathers, five orientations in double;
//                     writes the accepted flag (lane T writes the 0 the scan turns into the total) and counts the four verdicts
//                     per lane; a block adds its four sums to `counters` once (block_count, tn_mesh_ops.h).
//                     rocprim::exclusive_scan gives offsets[T + 1].
//   k_split_cells     lane per tetrahedron: copies the row or, where offsets say accepted, writes the centroid, the four children,
//                     their parents and the new vertex's parents.  The old vertices are one device-to-device copy.
//   k_split_copy_rows lane per 16-byte chunk of the OUTPUT: out[r, 0 .. V) = values[r, 0 .. V).  The two strides differ (V and
//                     V + K need not agree mod 4), so the stores are the aligned ones and the loads take what alignment is left;
//                     the chunks at the two ends of a row are written element by element.
//   k_split_new_columns<from the shadow?>  block per 64 new vertices x 64 rows through an LDS tile: the four parent columns are
//                     read as rows of the vertex-major shadow (256 B each at 64 rows) or as single elements of the feature-major
//                     array; out[r, V + k] is stored along k and out_vm[V + k, r] along r, both whole lines.
//   The old part of out_vm is a copy of values_vm where the caller has it and launch_transpose(values) where it has not.
//
// Every kernel is a grid-stride loop on at most SPLIT_BLOCKS blocks (tn_mesh_ops.h).  The only atomics are the four counters (one
// add per block and counter).  Scratch is ONE stream-ordered allocation (AsyncBytes; tn_split_count alone needs any).  Every store
// is bounded by the counts the caller passed, every id is checked against V before it is used as an address.  Nothing is read back
// here.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "tn_build.h"
#include "tn_kernels.h"
#include "tn_mesh_ops.h"
#include "tn_split_core.h"

namespace tn {

namespace {

constexpr int BT = 256;
constexpr unsigned SPLIT_BLOCKS = 1024;   // grid cap of every kernel here (TetrahedraTracer.SPLIT_GRID_LANES = SPLIT_BLOCKS * BT)
constexpr int TILE = 64;                  // new vertices and rows per block of k_split_new_columns

__global__ __launch_bounds__(BT) void k_split_flags(size_t T, uint32_t V, const float *__restrict__ xyz,
                                                    const uint32_t *__restrict__ cells, const uint8_t *__restrict__ select,
                                                    uint32_t *__restrict__ flags, uint32_t *__restrict__ counters) {
    uint32_t n[4] = {0u, 0u, 0u, 0u};   // asked, accepted, refused flat, refused id
    for (size_t t = gid(); t <= T; t += stride<BT>()) {
        split::Verdict v = split::NOT_ASKED;
        if (t < T && select[t] != 0) {
            uint32_t c[4];
            float cen[3];
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = cells[4 * t + k];
            v = split::judge(true, c, V, xyz, cen);
        }
        flags[t] = v == split::ACCEPTED;
        n[0] += v != split::NOT_ASKED;
        n[1] += v == split::ACCEPTED;
        n[2] += v == split::REFUSED_FLAT;
        n[3] += v == split::REFUSED_ID;
    }
    block_count<BT>(n, counters);
}

__global__ __launch_bounds__(BT) void k_split_cells(size_t T, uint32_t V, const float *__restrict__ xyz,
                                                    const uint32_t *__restrict__ cells, const uint32_t *__restrict__ offsets,
                                                    size_t num_new, float *__restrict__ xyz_out, uint32_t *__restrict__ cells_out,
                                                    uint32_t *__restrict__ cell_parent, uint32_t *__restrict__ vertex_parents) {
    for (size_t t = gid(); t < T; t += stride<BT>()) {
        uint32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = cells[4 * t + k];
        const size_t k = offsets[t];
        const bool accepted = offsets[t + 1] > offsets[t] && k < num_new;   // k < num_new bounds every store below
        cell_parent[t] = (uint32_t)t;
        if (!accepted) {
#pragma unroll
            for (int j = 0; j < 4; ++j) cells_out[4 * t + j] = c[j];
            continue;
        }
        float cen[3] = {0.f, 0.f, 0.f};
        if (iso::ids_ok(c, V)) {   // (false only where the caller changed `cells` between the two entries)
            float p[4][3];
            gather_tet(c, xyz, p);
            split::centroid(p, cen);
        }
        const uint32_t v = V + (uint32_t)k;
#pragma unroll
        for (int a = 0; a < 3; ++a) xyz_out[3 * (size_t)v + a] = cen[a];
#pragma unroll
        for (int j = 0; j < 4; ++j) vertex_parents[4 * k + j] = c[j];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const size_t row = split::child_slot(T, t, k, i);
            uint32_t child[4];
            split::child_row(c, i, v, child);
#pragma unroll
            for (int j = 0; j < 4; ++j) cells_out[4 * row + j] = child[j];
            cell_parent[row] = (uint32_t)t;
        }
    }
}

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at the alignment of a float
typedef float float4a __attribute__((ext_vector_type(4), aligned(16)));

// chunks = an upper bound of the aligned 16-byte chunks one row of V floats touches in `out`; vec = `out` is 16-byte aligned
__global__ __launch_bounds__(BT) void k_split_copy_rows(size_t rows, size_t V, size_t K, size_t chunks,
                                                        const float *__restrict__ values, float *__restrict__ out, bool vec) {
    const size_t total = rows * chunks;
    for (size_t idx = gid(); idx < total; idx += stride<BT>()) {
        const size_t r = idx / chunks, j = idx - r * chunks;
        const size_t d0 = r * (V + K), d1 = d0 + V, s0 = r * V;
        const size_t a = (d0 & ~(size_t)3) + 4 * j;
        const size_t lo = a > d0 ? a : d0, hi = a + 4 < d1 ? a + 4 : d1;
        if (lo >= hi) continue;
        const float *src = values + s0 + (lo - d0);
        if (vec && hi - lo == 4) {
            *reinterpret_cast<float4a *>(out + a) = *reinterpret_cast<const float4u *>(src);
        } else {
            for (size_t e = lo; e < hi; ++e) out[e] = src[e - lo];
        }
    }
}

template <bool FROM_VM>
__global__ __launch_bounds__(BT) void k_split_new_columns(size_t rows, size_t V, size_t K, const float *__restrict__ values,
                                                          const float *__restrict__ values_vm,
                                                          const uint32_t *__restrict__ vertex_parents, uint32_t new_mode,
                                                          float *__restrict__ out, float *__restrict__ out_vm) {
    __shared__ float tile[TILE][TILE + 1];   // [new vertex][row]
    __shared__ uint32_t par[TILE][4];
    __shared__ uint32_t par_ok[TILE];
    const size_t rtiles = (rows + TILE - 1) / TILE, tiles = ((K + TILE - 1) / TILE) * rtiles;
    const int lane = threadIdx.x & (TILE - 1), quarter = threadIdx.x >> 6;   // BT / TILE = 4 quarters
    for (size_t tile_id = blockIdx.x; tile_id < tiles; tile_id += gridDim.x) {
        const size_t k0 = (tile_id / rtiles) * TILE, r0 = (tile_id % rtiles) * TILE;
        __syncthreads();   // the last trip's reads of the tile and the parents are done
        {
            const size_t k = k0 + (threadIdx.x >> 2);
            par[threadIdx.x >> 2][threadIdx.x & 3] = k < K ? vertex_parents[4 * k + (threadIdx.x & 3)] : 0u;
        }
        __syncthreads();
        if (threadIdx.x < TILE) {
            const uint32_t *p = par[threadIdx.x];
            par_ok[threadIdx.x] = p[0] < V && p[1] < V && p[2] < V && p[3] < V;   // a parent id >= V: the new value is 0
        }
        __syncthreads();
        if (FROM_VM) {
            // phase 1, lanes along the rows: four 4 * rows-byte rows of the shadow per new vertex, out_vm along the rows
            for (int kk = quarter; kk < TILE; kk += BT / TILE) {
                const size_t k = k0 + kk, r = r0 + lane;
                if (k >= K || r >= rows) continue;
                float v = 0.f;
                if (new_mode == split::MODE_MEAN && par_ok[kk])
                    v = split::mean4(values_vm[(size_t)par[kk][0] * rows + r], values_vm[(size_t)par[kk][1] * rows + r],
                                     values_vm[(size_t)par[kk][2] * rows + r], values_vm[(size_t)par[kk][3] * rows + r]);
                tile[kk][lane] = v;
                if (out_vm) out_vm[(V + k) * rows + r] = v;
            }
            __syncthreads();
            // phase 2, lanes along the new vertices: out[r, V + k]
            for (int rr = quarter; rr < TILE; rr += BT / TILE) {
                const size_t k = k0 + lane, r = r0 + rr;
                if (k < K && r < rows) out[r * (V + K) + V + k] = tile[lane][rr];
            }
        } else {
            // phase 1, lanes along the new vertices: four single elements of row r per new vertex, out[r, V + k] along k
            for (int rr = quarter; rr < TILE; rr += BT / TILE) {
                const size_t k = k0 + lane, r = r0 + rr;
                if (k >= K || r >= rows) continue;
                float v = 0.f;
                if (new_mode == split::MODE_MEAN && par_ok[lane])
                    v = split::mean4(values[r * V + par[lane][0]], values[r * V + par[lane][1]], values[r * V + par[lane][2]],
                                     values[r * V + par[lane][3]]);
                tile[lane][rr] = v;
                out[r * (V + K) + V + k] = v;
            }
            if (out_vm) {   // (uniform over the block)
                __syncthreads();
                for (int kk = quarter; kk < TILE; kk += BT / TILE) {
                    const size_t k = k0 + kk, r = r0 + lane;
                    if (k < K && r < rows) out_vm[(V + k) * rows + r] = tile[kk][lane];
                }
            }
        }
    }
}

}  // namespace

void launch_split_count(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint8_t *select, uint32_t *offsets,
                        uint32_t *counters, hipStream_t s) {
    TN_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(uint32_t), s));
    if (T == 0) {
        TN_HIP(hipMemsetAsync(offsets, 0, sizeof(uint32_t), s));
        return;
    }
    const size_t n = T + 1, tmp_bytes = scan_bytes(n, s), flag_bytes = align256(n * sizeof(uint32_t));
    AsyncBytes all(flag_bytes + tmp_bytes, s);   // accepted flags | rocprim's scratch
    uint32_t *flags = all.at<uint32_t>();
    hipLaunchKernelGGL(k_split_flags, dim3(grid_for<BT, SPLIT_BLOCKS>(n)), dim3(BT), 0, s, T, (uint32_t)V, xyz, cells, select, flags,
                       counters);
    TN_HIP(hipGetLastError());
    scan(all.p + flag_bytes, tmp_bytes, flags, offsets, n, s);
}

void launch_split_emit(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint32_t *offsets, size_t num_new,
                       float *xyz_out, uint32_t *cells_out, uint32_t *cell_parent, uint32_t *vertex_parents, hipStream_t s) {
    if (V) TN_HIP(hipMemcpyAsync(xyz_out, xyz, 3 * V * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (T == 0) return;
    hipLaunchKernelGGL(k_split_cells, dim3(grid_for<BT, SPLIT_BLOCKS>(T)), dim3(BT), 0, s, T, (uint32_t)V, xyz, cells, offsets,
                       num_new, xyz_out, cells_out, cell_parent, vertex_parents);
    TN_HIP(hipGetLastError());
}

void launch_split_vertex_rows(size_t rows, size_t V, size_t K, const float *values, const float *values_vm,
                              const uint32_t *vertex_parents, uint32_t new_mode, float *out, float *out_vm, hipStream_t s) {
    if (V) {
        if (K == 0) {   // equal strides: the whole array is one copy
            TN_HIP(hipMemcpyAsync(out, values, rows * V * sizeof(float), hipMemcpyDeviceToDevice, s));
        } else {
            const size_t chunks = V / 4 + 2;
            hipLaunchKernelGGL(k_split_copy_rows, dim3(grid_for<BT, SPLIT_BLOCKS>(rows * chunks)), dim3(BT), 0, s, rows, V, K, chunks,
                               values, out, ((uintptr_t)out & 15u) == 0);
        }
        if (out_vm) {   // rows [0, V) of the shadow are contiguous
            if (values_vm) TN_HIP(hipMemcpyAsync(out_vm, values_vm, rows * V * sizeof(float), hipMemcpyDeviceToDevice, s));
            else launch_transpose(values, out_vm, (uint32_t)rows, (uint32_t)V, s);
        }
    }
    if (K) {
        const size_t tiles = ((K + TILE - 1) / TILE) * ((rows + TILE - 1) / TILE);
        const unsigned grid = (unsigned)std::min<size_t>(tiles, SPLIT_BLOCKS);
        if (values_vm)
            hipLaunchKernelGGL(k_split_new_columns<true>, dim3(grid), dim3(BT), 0, s, rows, V, K, values, values_vm, vertex_parents,
                               new_mode, out, out_vm);
        else
            hipLaunchKernelGGL(k_split_new_columns<false>, dim3(grid), dim3(BT), 0, s, rows, V, K, values, values_vm, vertex_parents,
                               new_mode, out, out_vm);
    }
    TN_HIP(hipGetLastError());
}

}  // namespace tn
