// tn_vertex_guard.hip -- tn_tet_quality and tn_limit_vertex_step: an optimiser's vertex move, shortened per vertex so that no
// tetrahedron of the loaded mesh turns inside out (the rule and its proof: tn_vertex_guard_core.h).
//
// Three passes over the borrowed `cells`, each value through the element function that states it:
//
//   k_star_width      lane per tetrahedron: four vertex gathers, guard::tet_width_orient in double, four atomicMin of the
//                     width's fp32 bits on star_w (non-negative floats order like their bits: k_tet_thin's trick); optionally
//                     the width and the orientation per tetrahedron.
//   k_clamp_vertices  lane per vertex: guard::clamp_vertex on the 12-byte rows, xyz_new written in place and only where it
//                     changes; counts clamped vertices and frozen vertices that were asked to move.
//   k_verify_orient   lane per tetrahedron: orientation on xyz_old and on the clamped xyz_new; counts flipped and collapsed
//                     tetrahedra.  The guard's own cross-check: both read 0 wherever the bound applies.
//
// All three are grid-stride loops on at most GUARD_BLOCKS blocks (tn_mesh_ops.h).  Counters are reduced per block (shuffle, then
// LDS) to one atomic per block and counter, and none where the block's sum is 0 (k_refit_records: one same-address atomic per
// wave serialises).  No read-back, no allocation; everything is enqueued on the caller's stream.
#include <hip/hip_runtime.h>

#include "tn_build.h"
#include "tn_mesh_ops.h"
#include "tn_vertex_guard_core.h"

namespace tn {

namespace {

constexpr int BT = 256;
constexpr unsigned GUARD_BLOCKS = 1024;   // grid cap of the three kernels (TetrahedraTracer.VERTEX_GUARD_GRID_LANES = GUARD_BLOCKS * BT)

// sum of (a, b) over the block -> one atomicAdd per non-zero sum.  Not tn_mesh_ops.h's block_count<BT>: on two counters its
// array form compiles to other instructions (LDS stores and the atomic's address), and these kernels keep theirs.
__device__ __forceinline__ void block_count2(uint32_t a, uint32_t b, uint32_t *out_a, uint32_t *out_b) {
    __shared__ uint32_t part[BT / 64][2];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += (uint32_t)__shfl_xor((int)a, off);
        b += (uint32_t)__shfl_xor((int)b, off);
    }
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = a; part[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t r = 0;
        for (int w = 0; w < BT / 64; ++w) r += part[w][threadIdx.x];
        if (r) atomicAdd(threadIdx.x ? out_b : out_a, r);
    }
}

__global__ __launch_bounds__(BT) void k_star_width(size_t T, const uint32_t *__restrict__ cells, const float *__restrict__ xyz,
                                                   float *__restrict__ width, int8_t *__restrict__ orient, uint32_t *star_w) {
    for (size_t i = gid(); i < T; i += stride<BT>()) {
        const uint32_t *c = cells + 4 * i;
        float p[4][3];
        gather_tet(c, xyz, p);
        const guard::WidthOrient r = guard::tet_width_orient(p);
        if (width) width[i] = __uint_as_float(r.width_bits);
        if (orient) orient[i] = (int8_t)r.orient;
        if (star_w)
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicMin(star_w + c[k], r.width_bits);
    }
}

__global__ __launch_bounds__(BT) void k_clamp_vertices(size_t V, const float *__restrict__ xyz_old, float *xyz_new,
                                                       const uint32_t *__restrict__ star_w, float fraction, uint32_t *counters) {
    uint32_t n_clamped = 0, n_frozen = 0;
    for (size_t v = gid(); v < V; v += stride<BT>()) {
        float o[3], n[3], out[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { o[a] = xyz_old[3 * v + a]; n[a] = xyz_new[3 * v + a]; }
        int kind;
        guard::clamp_vertex(o, n, __uint_as_float(star_w[v]), fraction, out, &kind);
        if (kind == guard::CLAMPED || kind == guard::FROZEN_MOVED) {
#pragma unroll
            for (int a = 0; a < 3; ++a) xyz_new[3 * v + a] = out[a];
        }
        n_clamped += kind == guard::CLAMPED;
        n_frozen += kind == guard::FROZEN_MOVED;
    }
    block_count2(n_clamped, n_frozen, counters + 0, counters + 1);
}

__global__ __launch_bounds__(BT) void k_verify_orient(size_t T, const uint32_t *__restrict__ cells, const float *__restrict__ xyz_old,
                                                      const float *__restrict__ xyz_new, uint32_t *counters) {
    uint32_t n_flipped = 0, n_collapsed = 0;
    for (size_t i = gid(); i < T; i += stride<BT>()) {
        const uint32_t *c = cells + 4 * i;
        float p[4][3];
        gather_tet(c, xyz_old, p);
        const int before = guard::tet_orient(p);
        gather_tet(c, xyz_new, p);
        const int after = guard::tet_orient(p);
        n_flipped += before * after < 0;
        n_collapsed += before != 0 && after == 0;
    }
    block_count2(n_flipped, n_collapsed, counters + 2, counters + 3);
}

}  // namespace

void launch_tet_quality(size_t V, size_t T, const uint32_t *cells, const float *xyz, float *width, int8_t *orient, float *star_width,
                        hipStream_t s) {
    if (star_width && V) TN_HIP(hipMemsetD32Async((hipDeviceptr_t)star_width, (int)guard::INF_BITS, V, s));
    if (T)
        hipLaunchKernelGGL(k_star_width, dim3(grid_for<BT, GUARD_BLOCKS>(T)), dim3(BT), 0, s, T, cells, xyz, width, orient,
                           reinterpret_cast<uint32_t *>(star_width));
    TN_HIP(hipGetLastError());
}

void launch_limit_vertex_step(size_t V, size_t T, const uint32_t *cells, const float *xyz_old, float *xyz_new, float fraction,
                              float *star_width, uint32_t *counters, bool verify, hipStream_t s) {
    TN_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(uint32_t), s));
    launch_tet_quality(V, T, cells, xyz_old, nullptr, nullptr, star_width, s);
    if (V)
        hipLaunchKernelGGL(k_clamp_vertices, dim3(grid_for<BT, GUARD_BLOCKS>(V)), dim3(BT), 0, s, V, xyz_old, xyz_new,
                           reinterpret_cast<const uint32_t *>(star_width), fraction, counters);
    if (verify && T)
        hipLaunchKernelGGL(k_verify_orient, dim3(grid_for<BT, GUARD_BLOCKS>(T)), dim3(BT), 0, s, T, cells, xyz_old, xyz_new, counters);
    TN_HIP(hipGetLastError());
}

}  // namespace tn
