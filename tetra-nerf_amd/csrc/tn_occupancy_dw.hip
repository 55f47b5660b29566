// tn_occupancy_dw.hip -- the head layer's weight-gradient GEMM of occupancy-culled training (tn_occupancy_train.hip), fp32 and
// bf16x3: k_dw_gemm<4, true> / k_dw_gemm_x3<4, true> on compact columns.  Of the four GEMMs only this one maps a sample to its
// ray -- its B operand has a tile of the ray's direction encoding -- so only this one has an indexed form: the row of the
// encoding is that of ray live[slot] / spr.  Grid, slices, slots and the reduction are tn_mlp_grad.hip's.  A translation unit of
// its own: every existing kernel keeps its code.  The kernel bodies are tn_mlp_grad.hip's and tn_mlp_x3_dw.hip's, included as text.
#include "tn_mlp_x3_fwd.h"

namespace tn {

namespace {

__global__ __launch_bounds__(256, 2) void k_dw_gemm_head_indexed(DwGemmArgs g, size_t n, uint32_t slice, const uint32_t *__restrict__ live,
                                                                 uint32_t num_rays) {
    using namespace mlp;
    constexpr int NBM = 4;
    constexpr bool EXTRA = true, INDEXED = true;
#include "tn_mlp_dw_body.inc"
}

__global__ __launch_bounds__(256, 2) void k_dw_gemm_x3_head_indexed(DwGemmArgs g, size_t n, uint32_t slice, const uint32_t *__restrict__ live,
                                                                    uint32_t num_rays) {
    using namespace x3;
    constexpr int NBM = 4;
    constexpr bool EXTRA = true, INDEXED = true;
#include "tn_mlp_x3_dw_body.inc"
}

}  // namespace

void launch_dw_gemm_head_indexed(bool x3, unsigned grid, const DwGemmArgs &g, size_t n, uint32_t slice, const uint32_t *live,
                                 uint32_t num_rays, hipStream_t stream) {
    if (x3) hipLaunchKernelGGL(k_dw_gemm_x3_head_indexed, dim3(grid), dim3(256), 0, stream, g, n, slice, live, num_rays);
    else hipLaunchKernelGGL(k_dw_gemm_head_indexed, dim3(grid), dim3(256), 0, stream, g, n, slice, live, num_rays);
}

}  // namespace tn
