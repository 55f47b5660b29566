// tn_mlp_x3_dw.hip -- the weight-gradient GEMMs of the training adjoint on the bf16 matrix cores at fp32 accuracy ("bf16x3";
// tn_mlp_param_grads_ex, mode 1).  The arithmetic is described in tn_mlp_x3.hip, the statement of the products and the slots of
// the partial sums in tn_mlp_grad.hip, whose host chain (slicing, k_reduce_partials, the rgb head) runs in either mode.
// A translation unit of its own, as tn_mlp_x3_train.hip and tn_mlp_x3_bwd.hip are: next to other kernels the compiler allocates
// their registers differently, and every existing device symbol must keep its code.
//
// k_dw_gemm_x3<NBM, EXTRA>: k_dw_gemm's arguments, grid, slices and slot layout; dW[128, 32 NB] = A[128, n] B[32 NB, n]^T with K =
// the sample axis, v_mfma_f32_32x32x16_bf16.  BOTH operands are streamed, so both are split -- once per element per block, on the
// way from the fetch registers into LDS, not once per consuming wave (four waves read every B tile):
//
//   fetch    a thread owns TWO consecutive samples of a step of 32 (tid & 15) and one quad of four feature rows per pass of 16
//            quads (tid >> 4): two 16-byte loads per pass, a quarter-wave 512 contiguous bytes.  Unconditional and clamped to the
//            slice's last sample; A of the lanes beyond s_end is zeroed, so they contribute exact zeros.  Issued one step ahead.
//   split    the eight values of a pass (4 features x 2 samples) are one x3::split8: each 32-bit result is the bf16 pair (sample
//            2 c, sample 2 c + 1) of one feature row and one piece -- twelve 4-byte LDS stores per pass, no cross-lane traffic.
//   LDS      row r of an operand: [hi: 32 bf16 | mid: 32 bf16 | lo: 32 bf16 | 16 bytes unused] = 208 bytes, sample i of the step
//            at element i of each piece.  A lane's eight K values of one piece (samples 16 q + 8 (lane >> 5) + 0..7 of K-step q)
//            are one aligned 16-byte read.  The row stride is 13 sixteen-byte slots, an odd number: the 16 lanes that a
//            ds_read_b128 serves together hold 16 rows that are distinct mod 16 and so 16 distinct slots of the 256-byte bank row
//            -- conflict-free; the stores of a half-wave (16 sample pairs x 2 quads, rows 4 apart = 208 dwords = 16 mod 32) cover
//            the 32 store banks once.  A: 128 rows = 26 KB, B: up to 160 rows = 32.5 KB; two blocks per CU as in k_dw_gemm.
//   MFMA     wave w owns output rows 32 w .. 32 w + 31 against every B tile: per K-step three 16-byte reads for A, three per B
//            tile, six MFMAs per tile (hh, hm, mh, hl, lh, mm, small terms first; two tiles interleaved so that consecutive
//            MFMAs do not share an accumulator).
//   VALU     the bias gradients (row sums of A) and d wd = sum_s d sigma_raw[s] h3[f][s] are fp32 statements over the unsplit
//            fetch registers, per thread over its two samples, reduced over the 16 sample pairs once at the end.
//
// The encoding tile of EXTRA (27 columns padded to 32) is fetched per ray as in k_dw_gemm (re-read only when a sample's ray
// changes) and goes through the same split.  Partial sums go to the block's slot; k_reduce_partials adds the slots in a fixed
// order: no atomics, bit-reproducible.
#include "tn_mlp_x3_fwd.h"

namespace tn {

using namespace x3;

namespace {

// (the body is tn_mlp_x3_dw_body.inc, text shared with the indexed head-layer GEMM of occupancy-culled training)
template <int NBM, bool EXTRA>
__global__ __launch_bounds__(256, 2) void k_dw_gemm_x3(DwGemmArgs g, size_t n, uint32_t slice) {
    constexpr bool INDEXED = false;        // (the indexed form: tn_occupancy_dw.hip)
    const uint32_t *const live = nullptr;
    constexpr uint32_t num_rays = 0;
#include "tn_mlp_x3_dw_body.inc"
}

}  // namespace

void launch_dw_gemm_x3(int nbm, bool extra, unsigned grid, const DwGemmArgs &g, size_t n, uint32_t slice, hipStream_t stream) {
    if (nbm == 4 && extra) hipLaunchKernelGGL((k_dw_gemm_x3<4, true>), dim3(grid), dim3(256), 0, stream, g, n, slice);
    else if (nbm == 4 && !extra) hipLaunchKernelGGL((k_dw_gemm_x3<4, false>), dim3(grid), dim3(256), 0, stream, g, n, slice);
    else if (nbm == 2 && !extra) hipLaunchKernelGGL((k_dw_gemm_x3<2, false>), dim3(grid), dim3(256), 0, stream, g, n, slice);
    else throw Error("launch_dw_gemm_x3: no such tile shape");
}

}  // namespace tn
