// tn_mlp_x3_train.hip -- the bf16x3 TRAINING forward (tn_mlp_forward_gather_train_ex, mode 1; the arithmetic is described in
// tn_mlp_x3.hip).  A translation unit of its own: with this kernel beside them the compiler allocates the registers of the
// k_mlp_forward_x3 instantiations differently (more scratch, other VGPR counts), and those must keep their code.
#include "tn_mlp_x3_fwd.h"

namespace tn {

using namespace x3;

// The gathering full network of k_mlp_forward_x3 -- the same arithmetic, so the same sigma / rgb bits -- which also saves x0,
// h1..h4 and the ReLU masks for the (fp32) adjoint kernels of tn_mlp_bwd.hip / tn_mlp_grad.hip in the layouts of the fp32
// training forward (tn_mlp_x3_fwd.h: TRAIN).  256 VGPRs, 28 bytes of scratch per lane (6 spilled registers), 2 waves per SIMD
// -- the occupancy of k_mlp_forward_x3<true, false> (256 VGPRs, no scratch), which its 120 KB of staged weights set anyway.
__global__ __launch_bounds__(X3_BLOCK) void k_mlp_forward_x3_train(size_t n, uint32_t samples_per_ray, const uint32_t *__restrict__ vi,
                                                                   const float *__restrict__ bc, const float *__restrict__ fieldT,
                                                                   const float *__restrict__ enc, const uint4 *__restrict__ blob,
                                                                   float *__restrict__ sigma, float *__restrict__ rgb,
                                                                   const float *__restrict__ ray_bias, mlp::FwdSave sv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem);
    constexpr size_t GROUP = (X3_BLOCK / 64) * 32;
    const size_t ngroups = (n + GROUP - 1) / GROUP;
    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        forward_group<true, false, true>(lds, g, n, samples_per_ray, nullptr, vi, bc, fieldT, enc, blob, sigma, rgb, ray_bias, &sv);
}

void launch_mlp_forward_x3_train(size_t n, uint32_t samples_per_ray, size_t num_rays, const uint32_t *vi, const float *bc,
                                 const float *fieldT, const float *dirs, const MlpPacks &w, float *sigma, float *rgb,
                                 const MlpBackwardBuffers &save, hipStream_t stream) {
    if (n == 0) return;
    launch_dir_encoding(num_rays, dirs, w.enc, ENC32, stream);
    mlp::launch_group_kernel<k_mlp_forward_x3_train, X3_BLOCK>(n, MAX_STAGE_U4 * sizeof(uint4), stream, n, samples_per_ray, vi, bc,
                                                                 fieldT, (const float *)w.enc, w.blob, sigma, rgb, w.ray_bias,
                                                                 mlp::FwdSave(save));
}

}  // namespace tn
