// tn_mlp_bf16.hip -- the shallow MLP + heads in PLAIN bf16 on the matrix cores: the evaluation-only arithmetic
// TN_MLP_MODE_BF16 (mode 2 of tn_mlp_forward / tn_mlp_forward_gather).
//
// The arithmetic (render.py: mlp_forward_bf16_statement is its one definition): in the four wide layers both operands of every
// product are rounded to bf16, round to nearest even -- the weight once at pack time, the fp32 activation (for the head layer's
// first two K-steps: the fp32 direction encoding) right before it enters the matrix core -- the products, exact in fp32, are
// accumulated in fp32 on top of the fp32 bias, the per-ray head bias is added in fp32 and the ReLU taken in fp32.  The narrow
// heads read the fp32 activations and run in fp32 on the VALU (mlp::density_head / rgb_head), like in the other two modes.
// ONE v_mfma_f32_32x32x16_bf16 per (K-step, tile) where bf16x3 spends six, one conversion per operand register pair where it
// spends three and four subtractions: this mode does not hold the 1e-5 parity bar and is never a default.
//
// Dataflow as in tn_mlp_x3.hip: a wave owns 32 samples, computes Y^T = W X^T and feeds the accumulators of a layer back as the B
// operand of the next in the x3::acc_k K order, the gather is fused in, the direction encoding of the sample's ray supplies the
// head layer's first two K-steps.  What differs is where the weights live: one piece of all four layers is 120 KB
// ([30 K-steps][4 tiles][64 lanes] x 16 B), so a block stages the WHOLE network into LDS once and then runs group after
// group without a single barrier -- its 8 waves drift apart, and the VALU stretches of one (gather, ReLU, heads) run under the
// MFMAs of the other wave of its SIMD.  The per-layer staging of the bf16x3 kernel (<= 40 KB at a time, two barriers per layer
// and group) measured 1.5-1.6x slower (profiles/mlp_bf16_bench.txt); it stays behind -DTN_BF16_STAGED=1 as a
// variant library for that A/B (make BUILD=build_staged OUT=../variants/libtetranerf_hip_staged.so EXTRA=-DTN_BF16_STAGED=1)
// and is not part of the product.
//
// The blob is the "hi" piece of the bf16x3 blob (x3::pk_bf16 is round to nearest even, and x_hi = bf16(x) is this mode's
// rounding) re-laid without the other two pieces, followed by the fp32 biases and head vectors in the layouts of
// tn_mlp_common.h; k_mlp_pack_bf16 makes it from the bf16x3 blob of the same tn_mlp_set_weights call.
#include "tn_mlp_x3_fwd.h"

namespace tn {

namespace {

using namespace x3;

#if defined(TN_BF16_STAGED) && TN_BF16_STAGED
constexpr bool RESIDENT_WEIGHTS = false;
#else
constexpr bool RESIDENT_WEIGHTS = true;
#endif
constexpr int BF16_BLOCK = mlp::MLP_BLOCK;
constexpr size_t GROUP = (BF16_BLOCK / 64) * 32;

// blob / resident LDS image, in 16-byte units: weights of L1 (4 K-steps), L2 (8), L3 (8), head (2 encoding + 8 base steps),
// then the four bias blocks ([tile][half][16] floats), the density vector and the rgb vectors
constexpr size_t su4(int steps) { return (size_t)steps * 4 * 64; }
constexpr size_t W_L1 = 0, W_L2 = W_L1 + su4(4), W_L3 = W_L2 + su4(8), W_HEAD = W_L3 + su4(8), N_W = W_HEAD + su4(10);
constexpr size_t O_BIAS = N_W, O_DV = O_BIAS + 4 * bu4(4), O_CV = O_DV + DVEC_U4, N_BF16_BLOB = O_CV + CVEC_U4;
// staged form: [the layer's weights, <= 10 K-steps][its bias][its head vector]
constexpr size_t S_BIAS = su4(10), S_VEC = S_BIAS + bu4(4), N_STAGED = S_VEC + CVEC_U4;
static_assert(N_BF16_BLOB * sizeof(uint4) <= 160 * 1024, "the resident image must fit the LDS of a CU");

__global__ void k_mlp_pack_bf16(const uint4 *__restrict__ x3blob, uint4 *__restrict__ blob) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N_W) {   // (K-step, tile) st of the network, lane: the hi piece of the bf16x3 blob's [st][piece][lane]
        const size_t st = i >> 6, lane = i & 63;
        const size_t src = st < 16 ? x3::O_L1 + st * 192 : st < 48 ? x3::O_L2 + (st - 16) * 192
                         : st < 80 ? x3::O_L3 + (st - 48) * 192 : x3::O_HEAD + (st - 80) * 192;
        blob[i] = x3blob[src + lane];
        return;
    }
    i -= N_W;
    const size_t boff[4] = {x3::O_L1 + wu4(4, 4), x3::O_L2 + wu4(8, 4), x3::O_L3 + wu4(8, 4), x3::O_HEAD + wu4(2, 4) + wu4(8, 4)};
    if (i < 4 * bu4(4)) {
        blob[O_BIAS + i] = x3blob[boff[i / bu4(4)] + i % bu4(4)];
        return;
    }
    i -= 4 * bu4(4);
    if (i < DVEC_U4) {
        blob[O_DV + i] = x3blob[x3::O_L3 + x3::N_L2 + i];
        return;
    }
    i -= DVEC_U4;
    if (i < CVEC_U4) blob[O_CV + i] = x3blob[boff[3] + bu4(4) + i];
}

static __device__ __forceinline__ uint4 pack8(const float *v) {   // 8 fp32 -> one bf16 operand register quadruple, RNE
    return make_uint4(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7]));
}

// STEPS consecutive K = 16 steps over bin[0 .. 8 STEPS): acc[t] += W[q][t] x bf16(bin[8 q .. 8 q + 7]).  The A operands and the
// conversion of step q + 1 are issued before the MFMAs of step q (one LDS latency per step otherwise: mlp::gemm_steps)
template <int STEPS>
static __device__ __forceinline__ void bf16_steps(f32x16 (&acc)[4], const uint4 *wl, const float *bin, int lane) {
    const uint4 *w = wl + lane;
    uint4 a[4], an[4], b = pack8(bin), bn;
#pragma unroll
    for (int t = 0; t < 4; ++t) a[t] = w[64 * t];
#pragma unroll
    for (int q = 0; q < STEPS; ++q) {
        if (q + 1 < STEPS) {
#pragma unroll
            for (int t = 0; t < 4; ++t) an[t] = w[(q + 1) * 256 + 64 * t];
            bn = pack8(bin + 8 * (q + 1));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = mma(a[t], b, acc[t]);
        __builtin_amdgcn_sched_barrier(0);
        if (q + 1 < STEPS) {
#pragma unroll
            for (int t = 0; t < 4; ++t) a[t] = an[t];
            b = bn;
        }
    }
}

// One group of 256 samples (8 waves x 32).  RESIDENT: lds holds the whole blob image and nothing here synchronises; otherwise
// all 512 threads call it together and every layer is staged behind a block barrier (lds: N_STAGED uint4).
template <bool GATHER, bool DENSITY_ONLY, bool RESIDENT>
static __device__ __forceinline__ void bf16_group(uint4 *lds, size_t g, size_t n, uint32_t samples_per_ray, const float *__restrict__ feats,
                                                  const uint32_t *__restrict__ vi, const float *__restrict__ bc,
                                                  const float *__restrict__ fieldT, const float *__restrict__ enc,
                                                  const uint4 *__restrict__ blob, float *__restrict__ sigma, float *__restrict__ rgb,
                                                  const float *__restrict__ ray_bias) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    const size_t s = g * GROUP + (size_t)wave * 32 + (lane & 31);
    if constexpr (RESIDENT) {
        if (g * GROUP + (size_t)wave * 32 >= n) return;   // (wave-uniform: a wave without a sample has nothing to wait for)
    }
    const size_t sc = s < n ? s : n - 1;
    float bin[KSH];

    // weights / bias of layer l (3: head) and the head vectors, resident or as staged by begin()
    auto wl = [&](size_t off) { return RESIDENT ? lds + off : lds; };
    auto bias = [&](int l) { return RESIDENT ? lds + O_BIAS + l * bu4(4) : lds + S_BIAS; };
    const uint4 *dvec = RESIDENT ? lds + O_DV : lds + S_VEC, *cvec = RESIDENT ? lds + O_CV : lds + S_VEC;
    auto begin = [&](size_t off, int steps, int l) {   // staged form: issue the loads of a layer (stage_wait() completes them)
        if constexpr (!RESIDENT) {
            __syncthreads();
            mlp::stage<BF16_BLOCK>(lds, blob + off, (uint32_t)su4(steps));
            mlp::stage<BF16_BLOCK>(lds + S_BIAS, blob + O_BIAS + l * bu4(4), (uint32_t)bu4(4));
            if (l == 2) mlp::stage<BF16_BLOCK>(lds + S_VEC, blob + O_DV, (uint32_t)DVEC_U4);
            if (l == 3) mlp::stage<BF16_BLOCK>(lds + S_VEC, blob + O_CV, (uint32_t)CVEC_U4);
        }
    };
    auto ready = [&] { if constexpr (!RESIDENT) stage_wait(); };

    // ---- layer 1: this lane supplies features 32h .. 32h+31 of its sample
    begin(W_L1, 4, 0);
    if constexpr (!GATHER) {   // B operands straight from the feature-major input [64, n]; row offsets i * n are wave-uniform
        const float *col = feats + (size_t)(32 * h) * n + sc;
#pragma unroll
        for (int i = 0; i < 32; ++i) bin[i] = col[(size_t)i * n];
    } else mlp::gather_features(bin, vi, bc, fieldT, sc, h);
    ready();
    {
        f32x16 acc[4];
        init_bias(acc, bias(0), h);
        bf16_steps<4>(acc, wl(W_L1), bin, lane);
        relu_to_bin(acc, bin);
    }
    // ---- layers 2, 3
#pragma unroll
    for (int l = 1; l < 3; ++l) {
        begin(l == 1 ? W_L2 : W_L3, 8, l);
        ready();
        f32x16 acc[4];
        init_bias(acc, bias(l), h);
        bf16_steps<8>(acc, wl(l == 1 ? W_L2 : W_L3), bin, lane);
        relu_to_bin(acc, bin);
    }
    mlp::density_head(reinterpret_cast<const float *>(dvec), bin, h, s, n, sigma);
    if constexpr (DENSITY_ONLY) return;
    // ---- head [enc(27) | base(128)] -> 128 ReLU
    begin(W_HEAD, 10, 3);
    ready();
    {
        f32x16 acc[4];
        init_bias(acc, bias(3), h);
        const float *e = enc + (sc / samples_per_ray) * ENC32;
        float ev[16];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 e0 = *reinterpret_cast<const float4 *>(e + 16 * q + 8 * h);
            const float4 e1 = *reinterpret_cast<const float4 *>(e + 16 * q + 8 * h + 4);
            ev[8 * q] = e0.x; ev[8 * q + 1] = e0.y; ev[8 * q + 2] = e0.z; ev[8 * q + 3] = e0.w;
            ev[8 * q + 4] = e1.x; ev[8 * q + 5] = e1.y; ev[8 * q + 6] = e1.z; ev[8 * q + 7] = e1.w;
        }
        bf16_steps<2>(acc, wl(W_HEAD), ev, lane);
        bf16_steps<8>(acc, wl(W_HEAD) + su4(2), bin, lane);
        if (ray_bias) mlp::add_ray_bias(acc, ray_bias + (sc / samples_per_ray) * HID, h);   // wave-uniform test
        relu_to_bin(acc, bin);
    }
    mlp::rgb_head(reinterpret_cast<const float *>(cvec), bin, h, s, n, rgb);
}

template <bool GATHER, bool DENSITY_ONLY, bool RESIDENT>
__global__ __launch_bounds__(BF16_BLOCK) void k_mlp_forward_bf16(size_t n, uint32_t samples_per_ray, const float *__restrict__ feats,
                                                                 const uint32_t *__restrict__ vi, const float *__restrict__ bc,
                                                                 const float *__restrict__ fieldT, const float *__restrict__ enc,
                                                                 const uint4 *__restrict__ blob, float *__restrict__ sigma,
                                                                 float *__restrict__ rgb, const float *__restrict__ ray_bias,
                                                                 const uint32_t *__restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem);
    if (count) n = (size_t)*count * samples_per_ray;   // device-side ray count (sync-free callers: n = the upper bound)
    const size_t ngroups = (n + GROUP - 1) / GROUP;
    if (blockIdx.x >= ngroups) return;                  // (block-uniform)
    if constexpr (RESIDENT) {
        // the network, once per block: the layers the form runs, the biases and head vectors behind them
        mlp::stage<BF16_BLOCK>(lds, blob, (uint32_t)(DENSITY_ONLY ? W_HEAD : N_W));
        mlp::stage<BF16_BLOCK>(lds + O_BIAS, blob + O_BIAS, (uint32_t)((DENSITY_ONLY ? O_CV : N_BF16_BLOB) - O_BIAS));
        stage_wait();
    }
    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        bf16_group<GATHER, DENSITY_ONLY, RESIDENT>(lds, g, n, samples_per_ray, feats, vi, bc, fieldT, enc, blob, sigma, rgb, ray_bias);
}

}  // namespace

size_t mlp_bf16_blob_u4() { return N_BF16_BLOB; }

void launch_mlp_pack_bf16(const uint4 *x3blob, uint4 *blob, hipStream_t stream) {
    hipLaunchKernelGGL(k_mlp_pack_bf16, dim3((unsigned)((N_BF16_BLOB + 255) / 256)), dim3(256), 0, stream, x3blob, blob);
}

void launch_mlp_forward_bf16(size_t n, uint32_t samples_per_ray, size_t num_rays, const float *feats, const uint32_t *vi,
                             const float *bc, const float *fieldT, const float *dirs, const MlpPacks &w, float *sigma, float *rgb,
                             hipStream_t stream, const uint32_t *count) {
    if (n == 0) return;
    const bool gather = feats == nullptr;
    const bool density_only = rgb == nullptr;
    if (density_only) num_rays = 0;
    launch_dir_encoding(num_rays, dirs, w.enc, ENC32, stream);
    constexpr size_t smem = (RESIDENT_WEIGHTS ? N_BF16_BLOB : N_STAGED) * sizeof(uint4);
    mlp::dispatch_gather_density(gather, density_only, [&](auto G, auto D) {
        mlp::launch_group_kernel<k_mlp_forward_bf16<decltype(G)::value, decltype(D)::value, RESIDENT_WEIGHTS>, BF16_BLOCK>(
            n, smem, stream, n, samples_per_ray, feats, vi, bc, fieldT, (const float *)w.enc, w.blob_bf16, sigma, rgb, w.ray_bias, count);
    });
}

}  // namespace tn
