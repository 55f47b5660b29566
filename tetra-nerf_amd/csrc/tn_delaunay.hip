// tn_delaunay.hip -- tn_delaunay_check and tn_remap_tet_values: is the loaded mesh still Delaunay on these vertices, and the
// per-tetrahedron state carried to another set of cells (the predicate, its bound and the transfer's rule: tn_delaunay_core.h,
// DESIGN.md section 4.16).
//
//   k_delaunay_faces  lane per face of the loaded face table: face_tets (8 B), the two cell rows (32 B), five vertex gathers
//                     (60 B), delaunay::face_verdict in double; optionally the state per face and +1 on the byte of both
//                     tetrahedra of a violated face (an atomicAdd on the 32-bit word that holds the byte: a tetrahedron has
//                     four faces, so no byte carries).  Counts interior, violated, uncertain and inverted-violated faces.
//   k_star_max        lane per old tetrahedron: atomicMax of its value's bits on the four vertices it names (non-negative
//                     floats order like their bits: k_star_width's trick with the other sign); a value of +0 launches nothing.
//   k_remap           lane per new tetrahedron: the largest star_max of its four vertices.
//
// All three are grid-stride loops on at most DELAUNAY_BLOCKS blocks (tn_mesh_ops.h).  Counters are reduced per block to one
// atomic per block and counter, and none where the block's sum is 0 (block_count, tn_mesh_ops.h).  No read-back, no
// allocation; everything is enqueued on the caller's stream.  The transfer's cells come from the caller, not from a loaded
// tracer: a vertex id that is not below num_vertices is passed over by both of its kernels.
#include <hip/hip_runtime.h>

#include "tn_build.h"
#include "tn_mesh_ops.h"
#include "tn_delaunay_core.h"

namespace tn {

namespace {

constexpr int BT = 256;
constexpr unsigned DELAUNAY_BLOCKS = 1024;   // grid cap of the three kernels (TetrahedraTracer.DELAUNAY_GRID_LANES = DELAUNAY_BLOCKS * BT)

__global__ __launch_bounds__(BT) void k_delaunay_faces(size_t F, const uint32_t *__restrict__ face_tets,
                                                       const uint32_t *__restrict__ cells, const float *__restrict__ xyz,
                                                       int8_t *__restrict__ face_state, uint32_t *tet_violations, uint32_t *counters) {
    uint32_t n[4] = {0, 0, 0, 0};
    for (size_t f = gid(); f < F; f += stride<BT>()) {
        const uint32_t t0 = face_tets[2 * f], t1 = face_tets[2 * f + 1];
        int state = delaunay::HULL;
        if (t1 != TN_EMPTY) {
            uint32_t c0[4], c1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { c0[k] = cells[4 * (size_t)t0 + k]; c1[k] = cells[4 * (size_t)t1 + k]; }
            const uint32_t ev = delaunay::opposite_vertex(c0, c1);
            float p[4][3], e[3];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int a = 0; a < 3; ++a) p[k][a] = xyz[3 * (size_t)c0[k] + a];
#pragma unroll
            for (int a = 0; a < 3; ++a) e[a] = xyz[3 * (size_t)ev + a];
            const delaunay::Verdict v = delaunay::face_verdict(p, e);
            state = v.state;
            n[0] += 1;
            n[1] += state == delaunay::VIOLATED;
            n[2] += state == delaunay::UNCERTAIN;
            n[3] += v.inverted;
            if (tet_violations && state == delaunay::VIOLATED) {
                atomicAdd(tet_violations + (t0 >> 2), 1u << (8 * (t0 & 3)));
                atomicAdd(tet_violations + (t1 >> 2), 1u << (8 * (t1 & 3)));
            }
        }
        if (face_state) face_state[f] = (int8_t)state;
    }
    block_count<BT>(n, counters);
}

__global__ __launch_bounds__(BT) void k_star_max(size_t T, uint32_t V, const uint32_t *__restrict__ cells,
                                                 const uint32_t *__restrict__ values, uint32_t *star_max) {
    for (size_t i = gid(); i < T; i += stride<BT>()) {
        const uint32_t bits = values[i];
        if (bits == 0) continue;                       // the preset already holds +0
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t v = cells[4 * i + k];
            if (v < V) atomicMax(star_max + v, bits);
        }
    }
}

__global__ __launch_bounds__(BT) void k_remap(size_t T, uint32_t V, const uint32_t *__restrict__ cells,
                                              const uint32_t *__restrict__ star_max, uint32_t *__restrict__ values) {
    for (size_t i = gid(); i < T; i += stride<BT>()) {
        uint32_t m = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t v = cells[4 * i + k];
            m = delaunay::max_bits(m, v < V ? star_max[v] : 0u);
        }
        values[i] = m;
    }
}

}  // namespace

void launch_delaunay_check(size_t T, size_t F, const uint32_t *cells, const uint32_t *face_tets, const float *xyz, uint32_t *counters,
                           int8_t *face_state, uint8_t *tet_violations, hipStream_t s) {
    TN_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(uint32_t), s));
    if (tet_violations && T) TN_HIP(hipMemsetAsync(tet_violations, 0, 4 * ((T + 3) / 4), s));
    if (F)
        hipLaunchKernelGGL(k_delaunay_faces, dim3(grid_for<BT, DELAUNAY_BLOCKS>(F)), dim3(BT), 0, s, F, face_tets, cells, xyz,
                           face_state, reinterpret_cast<uint32_t *>(tet_violations), counters);
    TN_HIP(hipGetLastError());
}

void launch_remap_tet_values(size_t V, size_t T_old, const uint32_t *old_cells, const float *old_values, size_t T_new,
                             const uint32_t *new_cells, float *new_values, float *star_max, hipStream_t s) {
    if (V) TN_HIP(hipMemsetAsync(star_max, 0, V * sizeof(float), s));
    if (T_old)
        hipLaunchKernelGGL(k_star_max, dim3(grid_for<BT, DELAUNAY_BLOCKS>(T_old)), dim3(BT), 0, s, T_old, (uint32_t)V, old_cells,
                           reinterpret_cast<const uint32_t *>(old_values), reinterpret_cast<uint32_t *>(star_max));
    if (T_new)
        hipLaunchKernelGGL(k_remap, dim3(grid_for<BT, DELAUNAY_BLOCKS>(T_new)), dim3(BT), 0, s, T_new, (uint32_t)V, new_cells,
                           reinterpret_cast<const uint32_t *>(star_max), reinterpret_cast<uint32_t *>(new_values));
    TN_HIP(hipGetLastError());
}

}  // namespace tn
