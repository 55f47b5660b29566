// tn_mlp_x3_fwd.h -- the bf16x3 forward of ONE group of 256 samples (8 waves x 32) as a device function: the loop body of
// k_mlp_forward_x3 (tn_mlp_x3.hip, where the arithmetic is described) and of the MLP phases of the persistent render kernel in
// its bf16x3 mode (tn_render_rays.hip, round 6) -- the same code, so the two produce identical bits.  Whatever does not depend on
// the arithmetic (gather, staging, the VALU heads, the per-ray bias, the save layouts) is tn_mlp_common.h's.
#pragma once
#include "tn_mlp_common.h"

namespace tn {
namespace x3 {

using mlp::f32x16;
using mlp::HID; using mlp::FD; using mlp::ENC; using mlp::ENC32; using mlp::KSH;
using mlp::acc_feature; using mlp::relu_to_bin; using mlp::stage_wait;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int X3_BLOCK = mlp::MLP_BLOCK;

// sizes in 16-byte units
constexpr size_t wu4(int steps, int tiles) { return (size_t)steps * tiles * 3 * 64; }
constexpr size_t bu4(int tiles) { return (size_t)tiles * 8; }  // bias: [tile][half][16] floats
// The narrow heads (density 128 -> 1, rgb 128 -> 3) run on the VALU as in tn_mlp.hip: their fp32 vectors
// ([half][64] floats in the lane's K order + bias) ride behind the layer that produces their input.
constexpr size_t DVEC_U4 = mlp::DVEC / 4, CVEC_U4 = mlp::CVEC / 4;
constexpr size_t N_L1 = wu4(4, 4) + bu4(4);
constexpr size_t N_L2 = wu4(8, 4) + bu4(4);
constexpr size_t N_L3 = N_L2 + DVEC_U4;
constexpr size_t N_HEAD = wu4(2, 4) + wu4(8, 4) + bu4(4) + CVEC_U4;
constexpr size_t O_L1 = 0, O_L2 = O_L1 + N_L1, O_L3 = O_L2 + N_L2, O_HEAD = O_L3 + N_L3, N_BLOB = O_HEAD + N_HEAD;
constexpr size_t MAX_STAGE_U4 = N_HEAD > N_L3 ? N_HEAD : N_L3;

// input feature consumed by K slot (step q, half h, element j) of a layer fed from accumulators
__host__ __device__ constexpr int acc_k(int q, int h, int j) { return 32 * (q >> 1) + acc_feature(8 * (q & 1) + j, h); }

static __device__ __forceinline__ uint32_t pk_bf16(float a, float b) {  // a -> low half, round to nearest even
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// 8 fp32 values -> three packed-bf16 operand registers quadruples (hi, mid, lo)
static __device__ __forceinline__ void split8(const float *v, uint4 &hi, uint4 &mid, uint4 &lo) {
    uint32_t H[4], Mi[4], L[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const float a = v[2 * p], b = v[2 * p + 1];
        const uint32_t ph = pk_bf16(a, b);
        const float ra = a - __uint_as_float(ph << 16), rb = b - __uint_as_float(ph & 0xFFFF0000u);
        const uint32_t pm = pk_bf16(ra, rb);
        const float sa = ra - __uint_as_float(pm << 16), sb = rb - __uint_as_float(pm & 0xFFFF0000u);
        H[p] = ph; Mi[p] = pm; L[p] = pk_bf16(sa, sb);
    }
    hi = make_uint4(H[0], H[1], H[2], H[3]);
    mid = make_uint4(Mi[0], Mi[1], Mi[2], Mi[3]);
    lo = make_uint4(L[0], L[1], L[2], L[3]);
}

static __device__ __forceinline__ f32x16 mma(const uint4 &a, const uint4 &b, const f32x16 &c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

struct B3 { uint4 h, m, l; };  // the three bf16 pieces of 8 K-values of a lane

// one K = 16 step of NT output tiles: acc[t] += W[t](hi,mid,lo) x B(hi,mid,lo), six partial products,
// small terms first; two tiles are interleaved so that consecutive MFMAs never share an accumulator
// (the six-product sequence stays written out for the pair and for the odd tile: behind a helper taking the tiles as an array it
//  changed the instruction stream of every bf16x3 kernel, and the bf16x3 render measured 0.7 % slower;
//  profiles/mlp_forward_dedupe.txt)
template <int NT, int TILES>
static __device__ __forceinline__ void x3_mma(f32x16 (&acc)[TILES], const uint4 *wl, const B3 &b, int lane) {
#pragma unroll
    for (int t = 0; t + 1 < NT; t += 2) {
        const uint4 *w0 = wl + (size_t)t * 192 + lane, *w1 = w0 + 192;
        const uint4 ah0 = w0[0], am0 = w0[64], al0 = w0[128];
        const uint4 ah1 = w1[0], am1 = w1[64], al1 = w1[128];
        acc[t] = mma(al0, b.h, acc[t]);     acc[t + 1] = mma(al1, b.h, acc[t + 1]);
        acc[t] = mma(ah0, b.l, acc[t]);     acc[t + 1] = mma(ah1, b.l, acc[t + 1]);
        acc[t] = mma(am0, b.m, acc[t]);     acc[t + 1] = mma(am1, b.m, acc[t + 1]);
        acc[t] = mma(am0, b.h, acc[t]);     acc[t + 1] = mma(am1, b.h, acc[t + 1]);
        acc[t] = mma(ah0, b.m, acc[t]);     acc[t + 1] = mma(ah1, b.m, acc[t + 1]);
        acc[t] = mma(ah0, b.h, acc[t]);     acc[t + 1] = mma(ah1, b.h, acc[t + 1]);
    }
    if constexpr (NT & 1) {
        constexpr int t = NT - 1;
        const uint4 *w0 = wl + (size_t)t * 192 + lane;
        const uint4 ah0 = w0[0], am0 = w0[64], al0 = w0[128];
        acc[t] = mma(al0, b.h, acc[t]);
        acc[t] = mma(ah0, b.l, acc[t]);
        acc[t] = mma(am0, b.m, acc[t]);
        acc[t] = mma(am0, b.h, acc[t]);
        acc[t] = mma(ah0, b.m, acc[t]);
        acc[t] = mma(ah0, b.h, acc[t]);
    }
}

// STEPS consecutive K = 16 steps over bin[0 .. 8*STEPS): the operand split of step q+1 (VALU) is issued
// in the same scheduling region as the MFMAs of step q, so it runs in their shadow; the sched_barrier
// between regions keeps the A-operand reads of later steps from being hoisted (registers).
// shadow(q): issued behind the MFMAs of step q, inside their scheduling region (x3_steps_store)
template <int STEPS, int NT, int TILES, typename Shadow>
static __device__ __forceinline__ void x3_steps(f32x16 (&acc)[TILES], const uint4 *wl, const float *bin, int lane, Shadow &&shadow) {
    B3 cur, nxt;
    split8(bin, cur.h, cur.m, cur.l);
#pragma unroll
    for (int q = 0; q < STEPS; ++q) {
        if (q + 1 < STEPS) split8(bin + 8 * (q + 1), nxt.h, nxt.m, nxt.l);
        x3_mma<NT>(acc, wl + (size_t)q * NT * 192, cur, lane);
        shadow(q);
        __builtin_amdgcn_sched_barrier(0);
        cur = nxt;
    }
}
template <int STEPS, int NT, int TILES>
static __device__ __forceinline__ void x3_steps(f32x16 (&acc)[TILES], const uint4 *wl, const float *bin, int lane) {
    x3_steps<STEPS, NT>(acc, wl, bin, lane, [](int) {});
}

// TRAIN (k_mlp_forward_x3_train): x3_steps that also SAVES its B operand in the layout of the fp32 training forward
// (tn_mlp_common.h: quad-major [F / 4][n][4]; gemm_steps_store) -- step q consumes bin[8 q .. 8 q + 7] = two quads, which
// leave in the scheduling region of that step's MFMAs, and (MASK: the operand is a ReLU output) eight bits of its mask
// word ride along.  p: this lane's first quad; qstride: distance of consecutive quads in float4 units (2 n in accumulator
// order, n for x0).  The stored values are the fp32 activations themselves, not their bf16 pieces: the fp32 adjoint
// kernels read them unchanged.
template <int STEPS, int NT, int TILES, bool MASK>
static __device__ __forceinline__ void x3_steps_store(f32x16 (&acc)[TILES], const uint4 *wl, const float (&bin)[KSH], int lane,
                                                      float4 *__restrict__ p, size_t qstride,
                                                      unsigned long long *__restrict__ mask_out = nullptr) {
    uint32_t lo = 0, hi = 0;
    x3_steps<STEPS, NT>(acc, wl, bin, lane, [&](int q) {
        p[0] = mlp::quad_of(bin, 2 * q);
        p[qstride] = mlp::quad_of(bin, 2 * q + 1);
        p += 2 * qstride;
        if constexpr (MASK) {
#pragma unroll
            for (int j = 8 * q; j < 8 * q + 8; ++j) {
                if (j < 32) lo |= mlp::relu_bit(bin[j], j);
                else hi |= mlp::relu_bit(bin[j], j);
            }
        }
    });
    if constexpr (MASK) *mask_out = ((unsigned long long)hi << 32) | lo;
}

template <int TILES>
static __device__ __forceinline__ void init_bias(f32x16 (&acc)[TILES], const uint4 *bias, int h) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const float4 *b = reinterpret_cast<const float4 *>(bias) + (t * 2 + h) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 x = b[q];
            acc[t][4 * q] = x.x; acc[t][4 * q + 1] = x.y; acc[t][4 * q + 2] = x.z; acc[t][4 * q + 3] = x.w;
        }
    }
}

// One group: samples g * 256 + wave * 32 + (lane & 31) of n; lds: MAX_STAGE_U4 uint4.  enc f32 [rays][32]: the direction encoding
// of the sample's ray (ray = sample / samples_per_ray), ray_bias f32 [rays][128] or null; blob: k_mlp_pack_x3's.  All 512 threads
// of the block call it together (block barriers inside).
// TRAIN (with GATHER, not DENSITY_ONLY): x0, h1..h4 and the four ReLU mask words of every sample go to `sv`, byte-compatible with
// what mlp::mlp_forward_group<.., TRAIN> saves -- in gather mode both kernels hold x0 in bin[0..31] = features 32 h + i, and
// every hidden layer in bin[16 t + r] = feature 32 t + acc_feature(r, h), the slot order of mlp::acc_k.  Lanes beyond n store
// their duplicate of sample n - 1 where its owner stores it.  h4 and its mask, which have no GEMM of their own group to leave
// under, are stored right behind the head layer: carried in registers into the next group's layer-1 GEMM, as the fp32 kernel
// does (mlp::FwdCarry), they cost this kernel -- which has no register to spare: 256 VGPRs at 2 waves per SIMD -- 30 spilled
// registers and measured 3 % SLOWER (1.83 against 1.78 ms at 2.1 M samples, alternating processes).  The arithmetic, and so sigma / rgb, are those of
// TRAIN = false.
// INDEXED: as in mlp::mlp_forward_group -- n counts the slots of the list `live`, slot i stands for sample live[i] < n_samples;
// with TRAIN the saves go to the slot (n slots: the quad-major stride).
template <bool GATHER, bool DENSITY_ONLY, bool TRAIN = false, bool INDEXED = false>
static __device__ __forceinline__ void forward_group(uint4 *lds, size_t g, size_t n, uint32_t samples_per_ray, const float *__restrict__ feats,
                                                     const uint32_t *__restrict__ vi, const float *__restrict__ bc,
                                                     const float *__restrict__ fieldT, const float *__restrict__ enc,
                                                     const uint4 *__restrict__ blob, float *__restrict__ sigma, float *__restrict__ rgb,
                                                     const float *__restrict__ ray_bias, const mlp::FwdSave *sv = nullptr,
                                                     const uint32_t *__restrict__ live = nullptr, size_t n_samples = 0) {
    static_assert(!TRAIN || (GATHER && !DENSITY_ONLY), "the training forward is the gathering, full network");
    static_assert(!INDEXED || GATHER, "the indexed forward gathers its samples itself");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    constexpr size_t GROUP = (X3_BLOCK / 64) * 32;
    const size_t slot = g * GROUP + (size_t)wave * 32 + (lane & 31);
    const size_t slotc = slot < n ? slot : n - 1;
    const mlp::IndexedSample ix = mlp::indexed_sample<INDEXED>(slot, slotc, n, live, n_samples);
    const size_t s = ix.s, sc = ix.sc, ns = ix.ns;
    const size_t col = INDEXED ? slotc : sc;   // TRAIN: the column of the save buffers (INDEXED: the slot, n slots in all)
    float bin[KSH];

    // ---- layer 1: this lane supplies features 32h .. 32h+31 of its sample
    __syncthreads();
    mlp::stage<X3_BLOCK>(lds, blob + O_L1, N_L1);
    if constexpr (!GATHER) {  // B operands straight from the feature-major input [64, n]
#pragma unroll
        for (int i = 0; i < 32; ++i) bin[i] = feats[(size_t)(32 * h + i) * n + sc];
    } else mlp::gather_features(bin, vi, bc, fieldT, sc, h);
    stage_wait();
    {
        f32x16 acc[4];
        init_bias(acc, lds + wu4(4, 4), h);
        if constexpr (TRAIN) x3_steps_store<4, 4, 4, false>(acc, lds, bin, lane, mlp::quad_ptr_x0(sv->x0, n, col, h), n);
        else x3_steps<4, 4>(acc, lds, bin, lane);
        relu_to_bin(acc, bin);
    }
    auto mask_ptr = [&](int layer) { return sv->masks + ((size_t)layer * n + col) * 2 + h; };   // TRAIN only
    // ---- layers 2, 3
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        __syncthreads();
        mlp::stage<X3_BLOCK>(lds, blob + (l == 0 ? O_L2 : O_L3), l == 0 ? N_L2 : N_L3);
        stage_wait();
        f32x16 acc[4];
        init_bias(acc, lds + wu4(8, 4), h);
        if constexpr (TRAIN) x3_steps_store<8, 4, 4, true>(acc, lds, bin, lane, mlp::quad_ptr(l == 0 ? sv->h1 : sv->h2, n, col, h), 2 * n, mask_ptr(l));
        else x3_steps<8, 4>(acc, lds, bin, lane);
        relu_to_bin(acc, bin);
    }
    mlp::density_head(reinterpret_cast<const float *>(lds + N_L2), bin, h, s, ns, sigma);   // (vector behind layer 3's blob)
    if constexpr (DENSITY_ONLY) return;
    // ---- head [enc(27) | base(128)] -> 128 ReLU
    __syncthreads();
    mlp::stage<X3_BLOCK>(lds, blob + O_HEAD, N_HEAD);
    stage_wait();
    {
        f32x16 acc[4];
        init_bias(acc, lds + wu4(2, 4) + wu4(8, 4), h);
        const float *e = enc + (sc / samples_per_ray) * ENC32;
        float ev[16];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 e0 = *reinterpret_cast<const float4 *>(e + 16 * q + 8 * h);
            const float4 e1 = *reinterpret_cast<const float4 *>(e + 16 * q + 8 * h + 4);
            ev[8 * q] = e0.x; ev[8 * q + 1] = e0.y; ev[8 * q + 2] = e0.z; ev[8 * q + 3] = e0.w;
            ev[8 * q + 4] = e1.x; ev[8 * q + 5] = e1.y; ev[8 * q + 6] = e1.z; ev[8 * q + 7] = e1.w;
        }
        x3_steps<2, 4>(acc, lds, ev, lane);
        if constexpr (TRAIN) x3_steps_store<8, 4, 4, true>(acc, lds + wu4(2, 4), bin, lane, mlp::quad_ptr(sv->h3, n, col, h), 2 * n, mask_ptr(2));
        else x3_steps<8, 4>(acc, lds + wu4(2, 4), bin, lane);
        if (ray_bias) mlp::add_ray_bias(acc, ray_bias + (sc / samples_per_ray) * HID, h);   // (appearance embedding) wave-uniform test
        relu_to_bin(acc, bin);
    }
    if constexpr (TRAIN) {
        mlp::store_bin(sv->h4, n, col, bin, h);
        *mask_ptr(3) = mlp::mask_of(bin);
    }
    mlp::rgb_head(reinterpret_cast<const float *>(lds + wu4(2, 4) + wu4(8, 4) + bu4(4)), bin, h, s, ns, rgb);
}

}  // namespace x3
}  // namespace tn
