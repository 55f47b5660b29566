// tn_position_grad.hip -- gradients w.r.t. WHERE a sample sits: the gather's adjoint w.r.t. the barycentrics and the
// adjoint of the sample position (ray origin / direction, mesh vertices).
//
// The reference leaves both open ("TODO: implement grad computation wrt barycentric coords for pose optimisation",
// src/py_binding.cpp:354) and ships only the last link as a PyTorch function (add_barycentrics_grad,
// tetranerf/utils/extension/__init__.py:45-68: a batched solve over gathered [n,4,3] copies).  Statement (also in plain torch:
// tetra-nerf_amd/geometry.py):
//
//  (A) phi = b0 F[v1] + b1 F[v2] + b2 F[v3] + (1 - (b0+b1+b2)) F[v0]   (D = 4; D - 1 barycentrics in general)
//      g_k = dL/db_k = sum_c G[c] (F[v_{k+1}, c] - F[v_0, c]),  G = dL/dphi;  a row of an EMPTY id is a zero row.
//
//  (B) x_k = position of v_k, e_k = x_k - x_0, T = rows (e_1, e_2, e_3):  p - x_0 = T^T b, so dL/dp = m with T m = g,
//      m = (g_0 (e_2 x e_3) + g_1 (e_3 x e_1) + g_2 (e_1 x e_2)) / (e_1 . (e_2 x e_3));
//      vertex v_k receives -w_k m, w = (1 - (b0+b1+b2), b0, b1, b2) -- the weights as the forward gather forms them;
//      with p = o + t d (t held constant) the ray receives dL/do = sum_s m, dL/dd = sum_s t_s m.
//      A sample with an EMPTY (or out-of-range) id, a zero determinant or a non-finite m contributes exact zeros.
//
// Tet membership, t, near / far and the sampler draws are constants of these gradients.
// Every fp32 operation is a single rounding (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "tn_device.h"
#include "tn_kernels.h"
#include "tn_ray_ops.h"

namespace tn {

namespace {

// (A).  The forward gather's shape (k_interp_fwd): one wavefront = 32 samples, lane (h = lane >> 5, s = lane & 31) holds
// the 32 features 32h .. 32h+31 of each 64-feature block of sample s; G and the D vertex rows are read as eight 16-byte
// loads per row and lane.
// SUMMATION ORDER of one output g_k: each half-wave lane adds its products G[c] * (F[v_{k+1}, c] - F[v_0, c]) in
// increasing c (its 32 features of block 0, then of block 1, ...) starting from 0; the result is (lower half) + (upper half).
template <int D>
__global__ __launch_bounds__(256) void k_interp_bwd_bary(uint32_t n, uint32_t Fd, const uint32_t *__restrict__ vi,
                                                         const float *__restrict__ grad_rows, const float *__restrict__ fieldT,
                                                         float *__restrict__ grad_bary) {
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const uint32_t ntiles = (n + 31) / 32;
    const uint32_t wave0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    const bool wide = (Fd & 3) == 0;     // 16-byte aligned rows
    for (uint32_t tix = wave0; tix < ntiles; tix += nwaves) {
        const uint32_t s = tix * 32 + (lane & 31);
        const bool ok = s < n;
        uint32_t v[D];
#pragma unroll
        for (int k = 0; k < D; ++k) v[k] = ok ? vi[(size_t)s * D + k] : TN_EMPTY;
        float acc[D - 1];
#pragma unroll
        for (int k = 0; k < D - 1; ++k) acc[k] = 0.f;
        for (uint32_t f0 = 32 * h; f0 < Fd; f0 += 64) {
            if (!ok) continue;
            const float *grow = grad_rows + (size_t)s * Fd + f0;
            if (wide && f0 + 32 <= Fd) {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float4 g = reinterpret_cast<const float4 *>(grow)[q];
                    float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (v[0] != TN_EMPTY) x0 = reinterpret_cast<const float4 *>(fieldT + (size_t)v[0] * Fd + f0)[q];
#pragma unroll
                    for (int k = 0; k < D - 1; ++k) {
                        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (v[k + 1] != TN_EMPTY) x = reinterpret_cast<const float4 *>(fieldT + (size_t)v[k + 1] * Fd + f0)[q];
                        acc[k] += g.x * (x.x - x0.x);
                        acc[k] += g.y * (x.y - x0.y);
                        acc[k] += g.z * (x.z - x0.z);
                        acc[k] += g.w * (x.w - x0.w);
                    }
                }
            } else {
                for (uint32_t j = 0; j < 32 && f0 + j < Fd; ++j) {
                    const float g = grow[j];
                    const float x0 = v[0] != TN_EMPTY ? fieldT[(size_t)v[0] * Fd + f0 + j] : 0.f;
#pragma unroll
                    for (int k = 0; k < D - 1; ++k) {
                        const float x = v[k + 1] != TN_EMPTY ? fieldT[(size_t)v[k + 1] * Fd + f0 + j] : 0.f;
                        acc[k] += g * (x - x0);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < D - 1; ++k) {
            const float other = __shfl_xor(acc[k], 32);
            // (h == 0 stores: its own sum is the lower half, the partner's the upper half)
            if (ok && h == 0) grad_bary[(size_t)s * (D - 1) + k] = acc[k] + other;
        }
    }
}

template <int D>
void run_bwd_bary(uint32_t n, uint32_t Fd, const uint32_t *vi, const float *rows, const float *fieldT, float *grad_bary,
                  hipStream_t stream) {
    const uint32_t nblocks = ((n + 31) / 32 + 3) / 4;  // 4 waves (128 samples) per block
    // (tests/test_gather_edges_gpu.py: SECOND_TRIP["bary"] quotes 128 samples per block and this cap of 4096 blocks)
    const unsigned grid = nblocks < 256u * 16u ? nblocks : 256u * 16u;
    hipLaunchKernelGGL(k_interp_bwd_bary<D>, dim3(grid), dim3(256), 0, stream, n, Fd, vi, rows, fieldT, grad_bary);
}

// (B).  One wavefront per ray, lane = sample, chunks of 64 samples.  Each lane keeps the sums of m and t m of ITS samples
// (sample lane, lane + 64, ... in that order); after the last chunk the 64 lane sums are combined by a butterfly
// (xor 32, 16, ..., 1) and lane 0 writes the ray's two rows: one writer per ray, the same bits on every run.  The twelve vertex
// terms of a sample are added with atomicAdd (hardware global_atomic_add_f32 under -munsafe-fp-atomics).
__global__ __launch_bounds__(256) void k_sample_positions_bwd(size_t R, uint32_t S, uint32_t V, const uint32_t *__restrict__ vi,
                                                              const float *__restrict__ bc, const float *__restrict__ gb,
                                                              const float *__restrict__ dist, const float *__restrict__ verts,
                                                              float *__restrict__ grad_points, float *__restrict__ grad_o,
                                                              float *__restrict__ grad_d, float *__restrict__ grad_v) {
    const int lane = threadIdx.x & 63;
    const size_t wave0 = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const size_t nwaves = (size_t)gridDim.x * (blockDim.x >> 6);
    for (size_t r = wave0; r < R; r += nwaves) {
        float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f};
        for (uint32_t s0 = 0; s0 < S; s0 += 64) {
            const uint32_t s = s0 + lane;
            if (s >= S) continue;
            const size_t i = r * S + s;
            const uint4 v = reinterpret_cast<const uint4 *>(vi)[i];
            float m[3] = {0.f, 0.f, 0.f};
            bool live = v.x < V && v.y < V && v.z < V && v.w < V;      // (TN_EMPTY is >= every V)
            float b[3] = {0.f, 0.f, 0.f};
            if (live) {
                float g[3], x[4][3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { b[c] = bc[i * 3 + c]; g[c] = gb[i * 3 + c]; }
                const uint32_t id[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) x[k][c] = verts[(size_t)id[k] * 3 + c];
                float e[3][3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) e[k][c] = x[k + 1][c] - x[0][c];
                // c23 = e2 x e3, c31 = e3 x e1, c12 = e1 x e2
                const float c23[3] = {e[1][1] * e[2][2] - e[1][2] * e[2][1], e[1][2] * e[2][0] - e[1][0] * e[2][2],
                                      e[1][0] * e[2][1] - e[1][1] * e[2][0]};
                const float c31[3] = {e[2][1] * e[0][2] - e[2][2] * e[0][1], e[2][2] * e[0][0] - e[2][0] * e[0][2],
                                      e[2][0] * e[0][1] - e[2][1] * e[0][0]};
                const float c12[3] = {e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2],
                                      e[0][0] * e[1][1] - e[0][1] * e[1][0]};
                const float det = (e[0][0] * c23[0] + e[0][1] * c23[1]) + e[0][2] * c23[2];
#pragma unroll
                for (int c = 0; c < 3; ++c) m[c] = ((g[0] * c23[c] + g[1] * c31[c]) + g[2] * c12[c]) / det;
                // a zero determinant gives inf or nan here; (x - x != 0) is true exactly for inf and nan
                live = det != 0.f && !(m[0] - m[0] != 0.f) && !(m[1] - m[1] != 0.f) && !(m[2] - m[2] != 0.f);
                if (!live) { m[0] = 0.f; m[1] = 0.f; m[2] = 0.f; }
                if (live && grad_v) {
                    const float w[4] = {1.0f - ((b[0] + b[1]) + b[2]), b[0], b[1], b[2]};
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int c = 0; c < 3; ++c) atomicAdd(&grad_v[(size_t)id[k] * 3 + c], -(w[k] * m[c]));
                }
            }
            if (grad_points) {
#pragma unroll
                for (int c = 0; c < 3; ++c) grad_points[i * 3 + c] = m[c];
            }
            if (live) {
                const float t = dist ? dist[i] : 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) { so[c] += m[c]; sd[c] += t * m[c]; }
            }
        }
        if (grad_o || grad_d) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { so[c] = rayops::wave_sum(so[c]); sd[c] = rayops::wave_sum(sd[c]); }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (grad_o) grad_o[r * 3 + c] = so[c];
                    if (grad_d) grad_d[r * 3 + c] = sd[c];
                }
            }
        }
    }
}

}  // namespace

void launch_interpolate_values_backward_bary_vm(uint32_t D, uint32_t n, uint32_t Fd, const uint32_t *vi, const float *grad_rows,
                                                const float *fieldT, float *grad_bary, hipStream_t stream) {
    if (n == 0) return;
    switch (D) {
        case 2: run_bwd_bary<2>(n, Fd, vi, grad_rows, fieldT, grad_bary, stream); break;
        case 3: run_bwd_bary<3>(n, Fd, vi, grad_rows, fieldT, grad_bary, stream); break;
        case 4: run_bwd_bary<4>(n, Fd, vi, grad_rows, fieldT, grad_bary, stream); break;
        case 6: run_bwd_bary<6>(n, Fd, vi, grad_rows, fieldT, grad_bary, stream); break;
        default: throw Error("Unsupported interpolation dimension with value " + std::to_string(D));
    }
}

void launch_sample_positions_backward(size_t R, uint32_t S, uint32_t V, const uint32_t *vi, const float *bc, const float *grad_bary,
                                      const float *dist, const float *verts, float *grad_points, float *grad_o, float *grad_d,
                                      float *grad_v, hipStream_t stream) {
    if (R == 0 || S == 0) return;
    const size_t nblocks = (R + 3) / 4;     // 4 waves = 4 rays per block
    const unsigned grid = (unsigned)(nblocks < 256u * 32u ? nblocks : 256u * 32u);
    hipLaunchKernelGGL(k_sample_positions_bwd, dim3(grid), dim3(256), 0, stream, R, S, V, vi, bc, grad_bary, dist, verts, grad_points,
                       grad_o, grad_d, grad_v);
}

}  // namespace tn
