// tn_occupancy_train.hip -- occupancy-culled TRAINING (the field itself: tn_occupancy.hip; tetranerf/nerfstudio/model.py:98-99,
// 256-265 registers the buffer and never uses it).  A culled training batch runs the saving forward, the dX chain and the
// weight-gradient GEMMs on the listed samples only.  The kernels of this file:
//   saving forward, indexed   mlp_forward_group / x3::forward_group with TRAIN and INDEXED: slot i of the list gathers, takes its
//                             ray's head term and stores sigma / rgb at sample live[i], and SAVES at column i of buffers that
//                             hold n_live columns -- the dX kernel, three of the four weight-gradient GEMMs, the bias sums and the
//                             rgb head are per-column code and run unchanged on those buffers with n = n_live
//   per-ray head-bias sums    out[ray] = sum of d4[:, slot] over the slots whose sample belongs to the ray
//   row compaction            dst[i] = src[live[i]] for rows of 1, 3 or 4 words: what the unchanged per-sample kernels read by
//                             position (vertex ids, barycentrics, the forward's outputs and their gradients)
// (the fourth GEMM, the head layer's, maps a sample to its ray: tn_occupancy_dw.hip).  n_live is a HOST value here: it sizes
// the buffers and every launch.  A translation unit of its own, as tn_mlp_x3_train.hip is: every existing kernel keeps its code.
#include "tn_mlp_fwd.h"
#include "tn_mlp_x3_fwd.h"

namespace tn {

namespace {

// k_mlp_forward<true, false, MLP_BLOCK, true> (tn_mlp.hip) over the list
__global__ __launch_bounds__(mlp::MLP_BLOCK, 2) void k_mlp_forward_train_indexed(
    size_t n_live, size_t n_samples, uint32_t samples_per_ray, const uint32_t *__restrict__ live, const uint32_t *__restrict__ vi,
    const float *__restrict__ bc, const float *__restrict__ fieldT, const float *__restrict__ hterm, const float *__restrict__ pk,
    float *__restrict__ sigma, float *__restrict__ rgb, mlp::FwdSave sv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *lds = reinterpret_cast<float *>(smem);
    constexpr size_t GROUP = (mlp::MLP_BLOCK / 64) * 32;
    const size_t ngroups = (n_live + GROUP - 1) / GROUP;
    mlp::FwdCarry cy;
#pragma unroll
    for (int j = 0; j < mlp::KSH; ++j) cy.h4[j] = 0.f;
    cy.p = nullptr; cy.m = nullptr;
    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        mlp::mlp_forward_group<true, false, mlp::MLP_BLOCK, true, true>(lds, g, n_live, samples_per_ray, nullptr, vi, bc, fieldT, hterm, pk,
                                                                        sigma, rgb, sv, &cy, live, n_samples);
    mlp::flush_carry(cy, n_live);
}

// k_mlp_forward_x3_train (tn_mlp_x3_train.hip) over the list
__global__ __launch_bounds__(x3::X3_BLOCK) void k_mlp_forward_x3_train_indexed(
    size_t n_live, size_t n_samples, uint32_t samples_per_ray, const uint32_t *__restrict__ live, const uint32_t *__restrict__ vi,
    const float *__restrict__ bc, const float *__restrict__ fieldT, const float *__restrict__ enc, const uint4 *__restrict__ blob,
    float *__restrict__ sigma, float *__restrict__ rgb, const float *__restrict__ ray_bias, mlp::FwdSave sv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem);
    constexpr size_t GROUP = (x3::X3_BLOCK / 64) * 32;
    const size_t ngroups = (n_live + GROUP - 1) / GROUP;
    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        x3::forward_group<true, false, true, true>(lds, g, n_live, samples_per_ray, nullptr, vi, bc, fieldT, enc, blob, sigma, rgb, ray_bias,
                                                   &sv, live, n_samples);
}

// first slot of live[0 .. n) whose sample is >= key (n when there is none); the list is ascending
__device__ __forceinline__ size_t lower_bound(const uint32_t *__restrict__ live, size_t n, size_t key) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if ((size_t)live[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// k_ray_head_grad (tn_mlp_bwd.hip) on compact columns: the slots of a ray are the contiguous range of the list between two
// lower bounds; thread = (quad, one of 8 consecutive slots of the range), sub = (slot - start of the range) & 7 as there, the 8
// partial sums combined by the same shuffles -- a fixed order, and with the identity list k_ray_head_grad's.  A ray without a
// live sample gets zeros; out covers all n_samples / S rays.
__global__ __launch_bounds__(256) void k_ray_head_grad_indexed(size_t n_live, size_t n_samples, uint32_t S, const uint32_t *__restrict__ live,
                                                               const float *__restrict__ d4, float *__restrict__ out) {
    const uint32_t quad = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const size_t rays = n_samples / S;
    const float4 *src = reinterpret_cast<const float4 *>(d4) + (size_t)quad * n_live;
    for (size_t ray = blockIdx.x; ray < rays; ray += gridDim.x) {
        const size_t first = lower_bound(live, n_live, ray * S), last = lower_bound(live, n_live, (ray + 1) * S);   // (block-uniform)
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (size_t j = first + sub; j < last; j += 8) {
            const float4 v = src[j];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            a.x += __shfl_xor(a.x, off); a.y += __shfl_xor(a.y, off); a.z += __shfl_xor(a.z, off); a.w += __shfl_xor(a.w, off);
        }
        if (sub == 0) *reinterpret_cast<float4 *>(out + ray * mlp::HID + 4 * quad) = a;
    }
}

// dst row i = src row live[i], rows of W 32-bit words
template <int W>
__global__ __launch_bounds__(256) void k_compact_rows(size_t n_live, const uint32_t *__restrict__ live, const uint32_t *__restrict__ src,
                                                      uint32_t *__restrict__ dst) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_live; i += (size_t)gridDim.x * 256) {
        const size_t s = live[i];
        if constexpr (W == 4) {
            reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[s];
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) dst[W * i + k] = src[W * s + k];
        }
    }
}

}  // namespace

void launch_mlp_forward_train_indexed(size_t n_live, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live, const uint32_t *vi,
                                      const float *bc, const float *fieldT, const float *dirs, const MlpPacks &w, int mode, float *sigma,
                                      float *rgb, const MlpBackwardBuffers &save, hipStream_t stream) {
    if (n_live == 0 || n_samples == 0) return;
    const size_t num_rays = n_samples / samples_per_ray;
    if (mode == 0) {
        launch_head_ray_term(num_rays, dirs, w, stream);
        mlp::launch_group_kernel<k_mlp_forward_train_indexed, mlp::MLP_BLOCK>(
            n_live, mlp::MAX_STAGE_FLOATS * sizeof(float), stream, n_live, n_samples, samples_per_ray, live, vi, bc, fieldT,
            (const float *)w.hterm, w.pk_gather, sigma, rgb, mlp::FwdSave(save));
    } else {
        launch_dir_encoding(num_rays, dirs, w.enc, mlp::ENC32, stream);
        mlp::launch_group_kernel<k_mlp_forward_x3_train_indexed, x3::X3_BLOCK>(
            n_live, x3::MAX_STAGE_U4 * sizeof(uint4), stream, n_live, n_samples, samples_per_ray, live, vi, bc, fieldT, (const float *)w.enc,
            w.blob, sigma, rgb, w.ray_bias, mlp::FwdSave(save));
    }
}

void launch_ray_head_grad_indexed(size_t n_live, size_t n_samples, uint32_t samples_per_ray, const uint32_t *live, const float *d4,
                                  float *out, hipStream_t stream) {
    if (n_samples == 0 || samples_per_ray == 0) return;
    const size_t rays = n_samples / samples_per_ray;
    if (n_live == 0) {   // no slot: every ray's sum is empty
        TN_HIP(hipMemsetAsync(out, 0, rays * mlp::HID * sizeof(float), stream));
        return;
    }
    hipLaunchKernelGGL(k_ray_head_grad_indexed, dim3((unsigned)(rays < 256 * 8 ? rays : 256 * 8)), dim3(256), 0, stream, n_live, n_samples,
                       samples_per_ray, live, d4, out);
}

void launch_compact_rows(int words_per_row, size_t n_live, const uint32_t *live, const void *src, void *dst, hipStream_t stream) {
    if (n_live == 0) return;
    const size_t blocks = (n_live + 255) / 256;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048));
    const uint32_t *s = static_cast<const uint32_t *>(src);
    uint32_t *d = static_cast<uint32_t *>(dst);
    if (words_per_row == 1) hipLaunchKernelGGL(k_compact_rows<1>, grid, dim3(256), 0, stream, n_live, live, s, d);
    else if (words_per_row == 3) hipLaunchKernelGGL(k_compact_rows<3>, grid, dim3(256), 0, stream, n_live, live, s, d);
    else if (words_per_row == 4) hipLaunchKernelGGL(k_compact_rows<4>, grid, dim3(256), 0, stream, n_live, live, s, d);
    else throw Error("compact_rows: rows of 1, 3 or 4 32-bit words");
}

}  // namespace tn
