// tn_isosurface_refine.hip -- the four steps of tn_isosurface_refine_*: the welded vertices of an extracted isosurface move along
// their own mesh edges onto a crossing of a density the caller evaluates between the steps (the rule: tn_isosurface_core.h,
// DESIGN.md section 4.17).  The topology is not touched.
//
//   k_iso_refine_begin     lane per vertex: the bracket (0, 1, values[a], values[b]) and the flag byte; ids checked against V.
//   k_iso_refine_points    lane per (vertex, j), j = 0..6: the inputs of the gathering forward for candidate j + 1 --
//                          vertex_indices (a, b, a, a) as one 16-byte store, barycentrics (t_j, 0, 0).  The gather weights
//                          corner 0 by 1 - (t + 0 + 0), so the sample is the point at t on the edge.  An edge with bad ids asks for
//                          vertex 0.
//   k_iso_refine_select    lane per vertex: seven densities (28 contiguous bytes), the bracket and the flag in, both out, in
//                          place -- the lane that reads an element is the one that writes it.
//   k_iso_refine_vertices  lane per vertex: edge_t and positions of the bracket as it stands.
//
// Every kernel is a grid-stride loop on at most ISO_BLOCKS blocks of BT (tn_mesh_ops.h), a lane per element, one writer per
// element, no atomics, no scratch, nothing read back.  Every index is bounded by the count the caller passed; ids are checked
// against V before `values` or `xyz` is read.
#include <hip/hip_runtime.h>

#include "tn_build.h"
#include "tn_mesh_ops.h"
#include "tn_isosurface_core.h"

namespace tn {

namespace {

constexpr int BT = 256;
constexpr unsigned ISO_BLOCKS = 1024;   // the grid cap of tn_isosurface.hip
constexpr int C = iso::REFINE_CANDIDATES;

__device__ __forceinline__ iso::Bracket load_bracket(const float4 *__restrict__ brackets, size_t i) {
    const float4 b = brackets[i];
    return iso::Bracket{b.x, b.y, b.z, b.w};
}
__device__ __forceinline__ void store_bracket(float4 *__restrict__ brackets, size_t i, const iso::Bracket &b) {
    brackets[i] = make_float4(b.t_lo, b.t_hi, b.s_lo, b.s_hi);
}

__global__ __launch_bounds__(BT) void k_iso_refine_begin(size_t N, uint32_t V, const uint2 *__restrict__ edge_vertices,
                                                         const float *__restrict__ values, float level,
                                                         float4 *__restrict__ brackets, uint8_t *__restrict__ flags) {
    for (size_t i = gid(); i < N; i += stride<BT>()) {
        const uint2 e = edge_vertices[i];
        iso::Bracket br;
        flags[i] = iso::refine_begin(e.x, e.y, V, values, level, br);
        store_bracket(brackets, i, br);
    }
}

__global__ __launch_bounds__(BT) void k_iso_refine_points(size_t N, const uint2 *__restrict__ edge_vertices,
                                                          const float4 *__restrict__ brackets, const uint8_t *__restrict__ flags,
                                                          uint4 *__restrict__ vertex_indices, float *__restrict__ barycentric) {
    const size_t n = N * C;
    for (size_t i = gid(); i < n; i += stride<BT>()) {
        const size_t v = i / C;
        const int j = (int)(i - v * C) + 1;
        uint2 e = edge_vertices[v];
        if (flags[v] & iso::REFINE_BAD_IDS) e = make_uint2(0u, 0u);
        const iso::Bracket br = load_bracket(brackets, v);
        vertex_indices[i] = make_uint4(e.x, e.y, e.x, e.x);
        barycentric[3 * i] = iso::refine_candidate(br.t_lo, br.t_hi, j);
        barycentric[3 * i + 1] = 0.f;
        barycentric[3 * i + 2] = 0.f;
    }
}

__global__ __launch_bounds__(BT) void k_iso_refine_select(size_t N, float level, const float *__restrict__ densities,
                                                          float4 *__restrict__ brackets, uint8_t *__restrict__ flags) {
    for (size_t i = gid(); i < N; i += stride<BT>()) {
        const uint8_t flag = flags[i];
        if (flag) continue;                 // frozen: the bracket and the flag stay
        float s[C];
#pragma unroll
        for (int j = 0; j < C; ++j) s[j] = densities[C * i + j];
        iso::Bracket br = load_bracket(brackets, i);
        const uint8_t now = iso::refine_select(br, s, level, flag);
        if (now) flags[i] = now;
        else store_bracket(brackets, i, br);
    }
}

__global__ __launch_bounds__(BT) void k_iso_refine_vertices(size_t N, uint32_t V, const float *__restrict__ xyz,
                                                            const uint2 *__restrict__ edge_vertices,
                                                            const float4 *__restrict__ brackets, float level,
                                                            float *__restrict__ edge_t, float *__restrict__ positions) {
    for (size_t i = gid(); i < N; i += stride<BT>()) {
        const uint2 e = edge_vertices[i];
        float t = 0.f, p[3] = {0.f, 0.f, 0.f};
        if (e.x < V && e.y < V) {
            float xa[3], xb[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { xa[k] = xyz[3 * (size_t)e.x + k]; xb[k] = xyz[3 * (size_t)e.y + k]; }
            t = iso::refine_vertex(load_bracket(brackets, i), level, xa, xb, p);
        }
        edge_t[i] = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) positions[3 * i + k] = p[k];
    }
}

}  // namespace

void launch_isosurface_refine_begin(size_t V, size_t N, const uint32_t *edge_vertices, const float *values, float level,
                                    float *brackets, uint8_t *flags, hipStream_t s) {
    if (N == 0) return;
    hipLaunchKernelGGL(k_iso_refine_begin, dim3(grid_for<BT, ISO_BLOCKS>(N)), dim3(BT), 0, s, N, (uint32_t)V,
                       reinterpret_cast<const uint2 *>(edge_vertices), values, level, reinterpret_cast<float4 *>(brackets), flags);
    TN_HIP(hipGetLastError());
}

void launch_isosurface_refine_points(size_t N, const uint32_t *edge_vertices, const float *brackets, const uint8_t *flags,
                                     uint32_t *vertex_indices, float *barycentric, hipStream_t s) {
    if (N == 0) return;
    hipLaunchKernelGGL(k_iso_refine_points, dim3(grid_for<BT, ISO_BLOCKS>(N * C)), dim3(BT), 0, s, N,
                       reinterpret_cast<const uint2 *>(edge_vertices), reinterpret_cast<const float4 *>(brackets), flags,
                       reinterpret_cast<uint4 *>(vertex_indices), barycentric);
    TN_HIP(hipGetLastError());
}

void launch_isosurface_refine_select(size_t N, float level, const float *densities, float *brackets, uint8_t *flags,
                                     hipStream_t s) {
    if (N == 0) return;
    hipLaunchKernelGGL(k_iso_refine_select, dim3(grid_for<BT, ISO_BLOCKS>(N)), dim3(BT), 0, s, N, level, densities,
                       reinterpret_cast<float4 *>(brackets), flags);
    TN_HIP(hipGetLastError());
}

void launch_isosurface_refine_vertices(size_t V, size_t N, const float *xyz, const uint32_t *edge_vertices, const float *brackets,
                                       float level, float *edge_t, float *positions, hipStream_t s) {
    if (N == 0) return;
    hipLaunchKernelGGL(k_iso_refine_vertices, dim3(grid_for<BT, ISO_BLOCKS>(N)), dim3(BT), 0, s, N, (uint32_t)V, xyz,
                       reinterpret_cast<const uint2 *>(edge_vertices), reinterpret_cast<const float4 *>(brackets), level, edge_t,
                       positions);
    TN_HIP(hipGetLastError());
}

}  // namespace tn
