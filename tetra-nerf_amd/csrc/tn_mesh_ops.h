// tn_mesh_ops.h -- what the kernels of the mesh operations share: the vertex guard, the Delaunay monitor, isosurface extraction
// and refinement, the split (tn_vertex_guard.hip, tn_delaunay.hip, tn_isosurface.hip, tn_isosurface_refine.hip, tn_split.hip);
// AsyncBytes also serves tn_interp.hip, the scan tn_build.hip.  Device and launcher helpers only: the host emulations under
// tests/host take the *_core.h files, never this one.  Every kernel stays in its own file and anonymous namespace.
//
//   gid, stride<BT>, grid_for<BT, BLOCKS>   a grid-stride loop: lane gid() takes i, i + stride<BT>(), ... on grid_for(n) blocks
//                     of BT lanes -- one lane per element up to BLOCKS blocks, BLOCKS persistent blocks beyond.  stride is the
//                     compile-time gridDim.x * BT, not blockDim.x.
//   gather_tet        the positions of the four corners a cell row names.
//   block_count<BT>   N per-lane counts summed over the block (wave shuffle, then LDS) -> one atomicAdd per counter and block, none
//                     where the sum is 0 (k_refit_records: one same-address atomic per wave serialises).
//   AsyncBytes        a stream-ordered temporary, released when the scope is left (also when a launch check throws); at<T>(offset)
//                     is the array at that byte offset, align256 the offset of the next one.
//   scan_bytes, scan  rocprim's uint32_t exclusive scan: the scratch it needs, then the call.  `In` is the input pointer type
//                     (uint32_t * or const uint32_t *: two instantiations of rocprim's kernels, as before these helpers).
//
// Three open-coded forms stay where the helper would change the kernel's instructions (profiles/mesh_ops_device_code.txt): the
// guard's two-counter reduction, and the corner gathers of k_delaunay_faces and k_iso_triangles.
#pragma once
#include <algorithm>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "tn_common.h"

namespace tn {

__device__ __forceinline__ size_t gid() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }
template <int BT>
__device__ __forceinline__ size_t stride() { return (size_t)gridDim.x * BT; }
template <int BT, unsigned BLOCKS>
inline unsigned grid_for(size_t n) { return (unsigned)std::min<size_t>((n + BT - 1) / BT, BLOCKS); }

__device__ __forceinline__ void gather_tet(const uint32_t *c, const float *__restrict__ xyz, float p[4][3]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) p[k][a] = xyz[3 * (size_t)c[k] + a];
}

// sums of n[0 .. N) over the block -> one atomicAdd on out[c] per non-zero sum
template <int BT, int N>
__device__ __forceinline__ void block_count(uint32_t (&n)[N], uint32_t *out) {
    __shared__ uint32_t part[BT / 64][N];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int c = 0; c < N; ++c) n[c] += (uint32_t)__shfl_xor((int)n[c], off);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int c = 0; c < N; ++c) part[threadIdx.x >> 6][c] = n[c];
    __syncthreads();
    if (threadIdx.x < N) {
        uint32_t r = 0;
        for (int w = 0; w < BT / 64; ++w) r += part[w][threadIdx.x];
        if (r) atomicAdd(out + threadIdx.x, r);
    }
}

struct AsyncBytes {
    char *p = nullptr;
    hipStream_t s;
    AsyncBytes(size_t bytes, hipStream_t stream) : s(stream) {
        if (bytes) TN_HIP(hipMallocAsync((void **)&p, bytes, stream));
    }
    ~AsyncBytes() { if (p) (void)hipFreeAsync(p, s); }
    AsyncBytes(const AsyncBytes &) = delete;
    AsyncBytes &operator=(const AsyncBytes &) = delete;
    template <typename T>
    T *at(size_t offset = 0) const { return reinterpret_cast<T *>(p + offset); }   // the array at byte `offset`
};

inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

template <typename In = uint32_t *>
size_t scan_bytes(size_t n, hipStream_t s) {
    size_t bytes = 0;
    TN_HIP(rocprim::exclusive_scan(nullptr, bytes, (In)nullptr, (uint32_t *)nullptr, 0u, n, rocprim::plus<uint32_t>(), s));
    return bytes;
}
template <typename In>
void scan(void *tmp, size_t bytes, In in, uint32_t *out, size_t n, hipStream_t s) {
    TN_HIP(rocprim::exclusive_scan(tmp, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), s));
}

}  // namespace tn
