// tn_optim.hip -- the RAdam step of a training iteration (tn_radam_step_field, tn_radam_step).
//
// Replaces torch.optim.RAdam (torch/optim/radam.py, single-tensor form), the optimiser of the reference's one parameter
// group "fields" (tetranerf/nerfstudio/registration.py:37-45), which runs the update as a chain of element-wise launches
// over whole tensors, and -- for the vertex field -- the tn_transpose_f32 launch that the in-place step causes before the
// next gather (the [V, 64] shadow is per tensor version).
//
// The statement, per element, every line one fp32 operation and one rounding (-ffp-contract=off), every scalar rounded to
// fp32 once by the caller (optim.radam_statement is the same text on the CPU; the kernels are bit-equal to it):
//     coupled decay:    g = g + wd * p                 decoupled decay:  p = p * (1 - lr wd)
//     m = m + (1 - b1) * (g - m)
//     v = b2 * v + ((1 - b2) * g) * g
//     adaptive:  p = p - (a * m) / (sqrt(v) + eps)     else:  p = p - a * m
// `a` and `adaptive` come from the step count on the host (optim.radam_scalars): bias corrections and the variance
// rectification folded into one factor.  sqrtf and / are the correctly rounded sequences here.  Denormals are kept (gfx950
// fp32 mode of the build), a non-finite gradient propagates into m, v and p as in torch: neither is part of the contract.
//
// Both kernels are pure streams.  k_radam_field: 4 reads + 4 writes of 64 x 64 tiles of a feature-major [64, V] field, the
// new p passing through a padded LDS tile so that the block also stores the 64 vertex rows (256 B each) of the vertex-major
// shadow.  k_radam_flat: up to 32 contiguous tensors per launch, each with its own (a, adaptive).
#include <hip/hip_runtime.h>

#include "tn_common.h"
#include "tn_kernels.h"

namespace tn {

namespace {

__device__ __forceinline__ void radam_element(float &p, float g, float &m, float &v, const RadamHyper &h, float a, bool adaptive) {
    if (h.decay_mode == 1) g = g + h.decay * p;
    else if (h.decay_mode == 2) p = p * h.decay;
    m = m + h.one_minus_beta1 * (g - m);
    v = h.beta2 * v + (h.one_minus_beta2 * g) * g;
    if (adaptive) p = p - (a * m) / (sqrtf(v) + h.eps);
    else p = p - a * m;
}

__device__ __forceinline__ void radam_element4(float4 &p, const float4 &g, float4 &m, float4 &v, const RadamHyper &h, float a,
                                               bool adaptive) {
    radam_element(p.x, g.x, m.x, v.x, h, a, adaptive);
    radam_element(p.y, g.y, m.y, v.y, h, a, adaptive);
    radam_element(p.z, g.z, m.z, v.z, h, a, adaptive);
    radam_element(p.w, g.w, m.w, v.w, h, a, adaptive);
}

constexpr int FT = 64;    // tile edge: all 64 features x 64 vertices
constexpr int FTP = 65;   // padded LDS row (floats): 64 banks of 4 B, both the row-wise writes and the column-wise reads of a
                          // wave touch every bank once

// One block = one tile of 64 vertices (all 64 features).  VEC: 16-byte accesses along V (V % 4 == 0, all bases 16-byte
// aligned): a wave instruction covers 4 feature rows x 256 B of p / g / m / v, and 4 vertex rows x 256 B of the shadow.
// Otherwise 4-byte accesses, 256 B of one row per wave instruction, as k_transpose.
template <bool VEC>
__global__ __launch_bounds__(256) void k_radam_field(uint32_t V, float *__restrict__ p, const float *__restrict__ g,
                                                     float *__restrict__ m, float *__restrict__ v, float *__restrict__ shadow,
                                                     RadamHyper h, float a, int adaptive_) {
    __shared__ float tile[FT][FTP];
    const bool adaptive = adaptive_ != 0;
    const uint32_t c0 = blockIdx.x * FT;
    if (VEC) {
        const uint32_t q = threadIdx.x & 15u, r0 = threadIdx.x >> 4;
        const uint32_t c = c0 + 4 * q;
        if (c < V) {
            float4 P[4], G[4], M[4], W[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t at = (size_t)(r0 + 16 * i) * V + c;
                P[i] = *reinterpret_cast<const float4 *>(p + at);
                G[i] = *reinterpret_cast<const float4 *>(g + at);
                M[i] = *reinterpret_cast<const float4 *>(m + at);
                W[i] = *reinterpret_cast<const float4 *>(v + at);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t r = r0 + 16 * i;
                const size_t at = (size_t)r * V + c;
                radam_element4(P[i], G[i], M[i], W[i], h, a, adaptive);
                *reinterpret_cast<float4 *>(p + at) = P[i];
                *reinterpret_cast<float4 *>(m + at) = M[i];
                *reinterpret_cast<float4 *>(v + at) = W[i];
                if (shadow) {
                    tile[r][4 * q] = P[i].x; tile[r][4 * q + 1] = P[i].y;
                    tile[r][4 * q + 2] = P[i].z; tile[r][4 * q + 3] = P[i].w;
                }
            }
        }
        if (!shadow) return;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t col = r0 + 16 * i;          // vertex of the tile; this lane's features 4q .. 4q+3
            if (c0 + col < V) {
                const float4 o = make_float4(tile[4 * q][col], tile[4 * q + 1][col], tile[4 * q + 2][col], tile[4 * q + 3][col]);
                *reinterpret_cast<float4 *>(shadow + (size_t)(c0 + col) * FT + 4 * q) = o;
            }
        }
    } else {
        const uint32_t tx = threadIdx.x & 63u, ty = threadIdx.x >> 6;
        if (c0 + tx < V) {
            for (uint32_t r = ty; r < FT; r += 4) {
                const size_t at = (size_t)r * V + c0 + tx;
                float P = p[at], M = m[at], W = v[at];
                radam_element(P, g[at], M, W, h, a, adaptive);
                p[at] = P; m[at] = M; v[at] = W;
                if (shadow) tile[r][tx] = P;
            }
        }
        if (!shadow) return;
        __syncthreads();
        for (uint32_t col = ty; col < FT; col += 4)
            if (c0 + col < V) shadow[(size_t)(c0 + col) * FT + tx] = tile[tx][col];
    }
}

constexpr uint32_t FLAT_CHUNK = 4096;   // elements of one block: 256 threads x 4 trips x 4 floats

// Block b serves chunk (b - first_block) of the tensor whose block range holds b.  16-byte accesses where all four bases of the
// tensor are 16-byte aligned (a chunk starts at a multiple of 4096 elements), 4-byte accesses otherwise and for the last
// n % 4 elements: either way a wave instruction covers whole consecutive 128-byte lines.
__global__ __launch_bounds__(256) void k_radam_flat(RadamTable tab, RadamHyper h) {
    uint32_t t = 0;
    while (t + 1 < tab.count && blockIdx.x >= tab.t[t + 1].first_block) ++t;
    const RadamTensor T = tab.t[t];
    const bool adaptive = T.adaptive != 0;
    const uint64_t e0 = (uint64_t)(blockIdx.x - T.first_block) * FLAT_CHUNK;
    const bool vec = ((reinterpret_cast<uintptr_t>(T.p) | reinterpret_cast<uintptr_t>(T.g) | reinterpret_cast<uintptr_t>(T.m) |
                       reinterpret_cast<uintptr_t>(T.v)) & 15u) == 0;
    if (vec && e0 + FLAT_CHUNK <= T.n) {
        // a whole chunk: all 16 loads of the thread are issued before the first store (the pointers may alias for all the
        // compiler knows, so it does not move a load above a store itself)
        float4 P[4], G[4], M[4], W[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t e = e0 + (uint64_t)(i * 256 + threadIdx.x) * 4;
            P[i] = *reinterpret_cast<const float4 *>(T.p + e);
            G[i] = *reinterpret_cast<const float4 *>(T.g + e);
            M[i] = *reinterpret_cast<const float4 *>(T.m + e);
            W[i] = *reinterpret_cast<const float4 *>(T.v + e);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t e = e0 + (uint64_t)(i * 256 + threadIdx.x) * 4;
            radam_element4(P[i], G[i], M[i], W[i], h, T.a, adaptive);
            *reinterpret_cast<float4 *>(T.p + e) = P[i];
            *reinterpret_cast<float4 *>(T.m + e) = M[i];
            *reinterpret_cast<float4 *>(T.v + e) = W[i];
        }
    } else if (vec) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t e = e0 + (uint64_t)(i * 256 + threadIdx.x) * 4;
            if (e + 4 <= T.n) {
                float4 P = *reinterpret_cast<const float4 *>(T.p + e), M = *reinterpret_cast<const float4 *>(T.m + e);
                float4 W = *reinterpret_cast<const float4 *>(T.v + e);
                const float4 G = *reinterpret_cast<const float4 *>(T.g + e);
                radam_element4(P, G, M, W, h, T.a, adaptive);
                *reinterpret_cast<float4 *>(T.p + e) = P;
                *reinterpret_cast<float4 *>(T.m + e) = M;
                *reinterpret_cast<float4 *>(T.v + e) = W;
            } else {
                for (uint64_t k = e; k < T.n && k < e + 4; ++k) {
                    float P = T.p[k], M = T.m[k], W = T.v[k];
                    radam_element(P, T.g[k], M, W, h, T.a, adaptive);
                    T.p[k] = P; T.m[k] = M; T.v[k] = W;
                }
            }
        }
    } else {
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const uint64_t k = e0 + (uint64_t)(i * 256 + threadIdx.x);
            if (k < T.n) {
                float P = T.p[k], M = T.m[k], W = T.v[k];
                radam_element(P, T.g[k], M, W, h, T.a, adaptive);
                T.p[k] = P; T.m[k] = M; T.v[k] = W;
            }
        }
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

// The grid is NOT capped: one block per 64-vertex tile (V < 2^32 gives at most 2^26 blocks), no block strides.
void launch_radam_field(uint32_t V, float *p, const float *g, float *m, float *v, float *shadow, const RadamHyper &h, float a,
                        bool adaptive, hipStream_t stream) {
    if (V == 0) return;
    const unsigned tiles = (unsigned)(((uint64_t)V + FT - 1) / FT);
    const bool vec = V % 4 == 0 && aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(shadow);
    if (vec)
        hipLaunchKernelGGL(k_radam_field<true>, dim3(tiles), dim3(256), 0, stream, V, p, g, m, v, shadow, h, a, adaptive ? 1 : 0);
    else
        hipLaunchKernelGGL(k_radam_field<false>, dim3(tiles), dim3(256), 0, stream, V, p, g, m, v, shadow, h, a, adaptive ? 1 : 0);
}

// One launch per TN_RADAM_TABLE (32) tensors; tensors of 0 elements take no slot.
void launch_radam_flat(size_t count, const RadamTensor *tensors, const RadamHyper &h, hipStream_t stream) {
    RadamTable tab;
    tab.count = 0;
    uint64_t blocks = 0;
    auto flush = [&] {
        if (tab.count) hipLaunchKernelGGL(k_radam_flat, dim3((unsigned)blocks), dim3(256), 0, stream, tab, h);
        tab.count = 0;
        blocks = 0;
    };
    for (size_t i = 0; i < count; ++i) {
        if (tensors[i].n == 0) continue;
        const uint64_t nb = (tensors[i].n + FLAT_CHUNK - 1) / FLAT_CHUNK;
        if (nb > 0x7FFFFFFFull) throw Error("radam step: a tensor of more than 2^43 elements is not supported");
        if (tab.count == RADAM_TABLE || blocks + nb > 0x7FFFFFFFull) flush();
        RadamTensor &T = tab.t[tab.count++];
        T = tensors[i];
        T.first_block = (uint32_t)blocks;
        blocks += nb;
    }
    flush();
}

}  // namespace tn
