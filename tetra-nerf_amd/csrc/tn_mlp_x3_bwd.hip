// tn_mlp_x3_bwd.hip -- the dX chain of the training adjoint on the bf16 matrix cores at fp32 accuracy ("bf16x3";
// tn_mlp_backward_ex, mode 1).  The arithmetic is described in tn_mlp_x3.hip, the statement of the chain in tn_mlp_bwd.hip.
// A translation unit of its own, as tn_mlp_x3_train.hip is: next to other kernels the compiler allocates their registers
// differently, and every existing device symbol must keep its code.
//
//   k_mlp_pack_x3_t.   Wh[:, 27:]^T, W3^T, W2^T, W1^T as bf16 hi / mid / lo pieces (x3::split8, as k_mlp_pack_x3 splits) in the
//       [K-step of 16][tile of INPUT features][piece][lane] order x3_mma reads; K runs over the layer's OUTPUT features in
//       accumulator order (x3::acc_k), as in k_mlp_pack_t.  The fp32 vectors the VALU parts need ride behind the first stage:
//       the density vector in accumulator order and the rgb-head rows in K order (k_mlp_pack_t's, float for float).
//   k_mlp_backward_x3. k_mlp_backward's inputs, outputs and layouts; the dataflow of x3::forward_group: 8 waves x 32 samples
//       share ONE staged layer (96 KB of pieces), two block barriers per layer.  Only the four matrix products are bf16x3:
//       softplus' / sigmoid', d_pre4, the density term, the masks and the transposition of d x0 are k_mlp_backward's fp32
//       statements, operation for operation, so dhead and d4 are its bits.
#include "tn_mlp_x3_fwd.h"

namespace tn {

using namespace x3;

namespace {

// ---- the transposed blob, in 16-byte units
constexpr int OTI1 = FD / 32;                                      // input tiles of layer 1
constexpr int QS = HID / 16;                                       // K = 16 steps over a layer's 128 output features
constexpr size_t T_H = wu4(QS, 4);                                 // one 128 x 128 layer: 96 KB
constexpr size_t T_1 = wu4(QS, OTI1);                              // W1^T: 48 KB
constexpr size_t N_TH = T_H + DVEC_U4 + CVEC_U4;                   // first stage: Wh^T, the density vector, the rgb rows
constexpr size_t O_TH = 0, O_T3 = O_TH + N_TH, O_T2 = O_T3 + T_H, O_T1 = O_T2 + T_H, N_BLOB_T = O_T1 + T_1;

__global__ void k_mlp_pack_x3_t(MlpWeights w, uint4 *__restrict__ blob) {
    struct Seg { const float *m; int ld, col0, tiles; size_t off; };
    const Seg segs[4] = {{w.wh, ENC + HID, ENC, 4, O_TH}, {w.w3, HID, 0, 4, O_T3}, {w.w2, HID, 0, 4, O_T2}, {w.w1, FD, 0, OTI1, O_T1}};
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int s = 0; s < 4; ++s) {
        const size_t cnt = (size_t)QS * segs[s].tiles * 64;
        if (i < cnt) {
            const int lane = (int)(i & 63), st = (int)(i >> 6), tile = st % segs[s].tiles, q = st / segs[s].tiles;
            const int row = lane & 31, h = lane >> 5;
            float v[8];
            // A[input feature 32 tile + row][K slot (q, h, j)] = W[output feature acc_k(q, h, j)][input feature]
            for (int j = 0; j < 8; ++j) v[j] = segs[s].m[(size_t)acc_k(q, h, j) * segs[s].ld + segs[s].col0 + 32 * tile + row];
            uint4 hi, mid, lo;
            split8(v, hi, mid, lo);
            uint4 *dst = blob + segs[s].off + (size_t)st * 192 + lane;
            dst[0] = hi; dst[64] = mid; dst[128] = lo;
            return;
        }
        i -= cnt;
    }
    // fp32 vectors behind the first stage, as in k_mlp_pack_t
    float *dv = reinterpret_cast<float *>(blob + O_TH + T_H);
    float *cv = dv + mlp::DVEC;
    if (i < mlp::DVEC) {
        const int jj = (int)i;
        dv[jj] = jj < 128 ? w.wd[mlp::acc_k(jj & 63, jj >> 6)] : 0.f;
        return;
    }
    i -= mlp::DVEC;
    if (i < mlp::CVEC) {
        const int jj = (int)i;
        cv[jj] = jj < 384 ? w.wr[(size_t)(jj >> 7) * HID + mlp::acc_k(jj & 63, (jj >> 6) & 1)] : 0.f;
    }
}
constexpr size_t PACK_T_THREADS = (size_t)QS * (3 * 4 + OTI1) * 64 + mlp::DVEC + mlp::CVEC;

struct BwdIn {
    const unsigned long long *masks;   // [4, n, 2] ReLU masks of h1..h4
    const float *sigma, *rgb;          // the forward's outputs [n], [n, 3]
    const float *d_sigma, *d_rgb;      // [n], [n, 3]
};
struct BwdOut {
    float *d1, *d2, *d3, *d4;  // [128, n] quad-major
    float *dhead;              // [4, n]
    float *dx0;                // [n, 64] sample-major rows
};

// LDS: region A = one 128 x 128 stage (+ the vectors of the first); region B = W1^T, requested when the W2^T GEMM starts and
// landing under it.  d x0 is transposed through region A, which is free once every wave has left the W2^T GEMM.
constexpr int BWD_X3_BLOCK = X3_BLOCK;
constexpr size_t TR_FLOATS = (size_t)(BWD_X3_BLOCK / 64) * 32 * 65;
constexpr size_t LDS_A = N_TH, LDS_B = T_1;
static_assert(TR_FLOATS * sizeof(float) <= LDS_A * sizeof(uint4), "the transposition of d x0 fits the layer stage");
static_assert((LDS_A + LDS_B) * sizeof(uint4) <= 160 * 1024, "a layer stage and W1^T must fit the CU's LDS");

}  // namespace

__global__ __launch_bounds__(BWD_X3_BLOCK) void k_mlp_backward_x3(size_t n, BwdIn in, const uint4 *__restrict__ blob, BwdOut o) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint4 *ldsA = reinterpret_cast<uint4 *>(smem), *ldsB = ldsA + LDS_A;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    constexpr size_t GROUP = (BWD_X3_BLOCK / 64) * 32;
    const size_t ngroups = (n + GROUP - 1) / GROUP;
    // the sample of this lane in group gg, clamped: lanes beyond the end recompute sample n - 1 and store the same values
    // to the same places as its owner
    auto sample_of = [&](size_t gg) {
        const size_t s = gg * GROUP + (size_t)wave * 32 + (lane & 31);
        return s < n ? s : n - 1;
    };
    // what a group needs of its samples before the first GEMM: four mask words and the head gradients (k_mlp_backward's)
    struct Head { unsigned long long m1, m2, m3, m4; float dsr, dr0, dr1, dr2; };
    auto load_head = [&](size_t gg) {
        const size_t sc = sample_of(gg);
        Head q;
        q.m1 = in.masks[(0 * n + sc) * 2 + h]; q.m2 = in.masks[(1 * n + sc) * 2 + h];
        q.m3 = in.masks[(2 * n + sc) * 2 + h]; q.m4 = in.masks[(3 * n + sc) * 2 + h];
        q.dsr = in.d_sigma[sc] * -expm1f(-in.sigma[sc]);
        const float y0 = in.rgb[3 * sc], y1 = in.rgb[3 * sc + 1], y2 = in.rgb[3 * sc + 2];
        q.dr0 = in.d_rgb[3 * sc] * (y0 * (1.0f - y0));
        q.dr1 = in.d_rgb[3 * sc + 1] * (y1 * (1.0f - y1));
        q.dr2 = in.d_rgb[3 * sc + 2] * (y2 * (1.0f - y2));
        return q;
    };

    Head hd = load_head(blockIdx.x);

    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const size_t s = g * GROUP + (size_t)wave * 32 + (lane & 31);
        const size_t sc = s < n ? s : n - 1;     // columns of the lanes beyond the end: their owner's, same values
        float bin[KSH];
        f32x16 acc[4];
        const unsigned long long m1 = hd.m1, m2 = hd.m2, m3 = hd.m3;
        const float dsr = hd.dsr;
        // ---- d h3 = Wh[:, 27:]^T d_pre4 + wd * d sigma_raw, masked; d_pre4 = ReLU'(h4) Wr^T d c
        __syncthreads();                          // the previous group's transposition has left region A
        mlp::stage<BWD_X3_BLOCK>(ldsA, blob + O_TH, N_TH);
        if (h == 0 && s < n) {
            o.dhead[s] = dsr;
            o.dhead[n + s] = hd.dr0; o.dhead[2 * n + s] = hd.dr1; o.dhead[3 * n + s] = hd.dr2;
        }
        stage_wait();
        {
            const float *cv = reinterpret_cast<const float *>(ldsA + T_H) + mlp::DVEC;
            const float *w0 = cv + 64 * h, *w1 = cv + 128 + 64 * h, *w2 = cv + 256 + 64 * h;
#pragma unroll
            for (int j = 0; j < KSH; ++j) {
                const float v = (w0[j] * hd.dr0 + w1[j] * hd.dr1) + w2[j] * hd.dr2;
                bin[j] = ((hd.m4 >> j) & 1ull) ? v : 0.f;
            }
        }
        mlp::zero_acc(acc);
        x3_steps_store<QS, 4, 4, false>(acc, ldsA, bin, lane, mlp::quad_ptr(o.d4, n, sc, h), 2 * n);
        {
            const float *dv = reinterpret_cast<const float *>(ldsA + T_H) + 64 * h;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] += dv[t * 16 + r] * dsr;
            mlp::masked_to_bin(acc, m3, bin);
        }
        // ---- d h2 = W3^T d_pre3
        __syncthreads();
        mlp::stage<BWD_X3_BLOCK>(ldsA, blob + O_T3, T_H);
        stage_wait();
        mlp::zero_acc(acc);
        x3_steps_store<QS, 4, 4, false>(acc, ldsA, bin, lane, mlp::quad_ptr(o.d3, n, sc, h), 2 * n);
        mlp::masked_to_bin(acc, m2, bin);
        // ---- d h1 = W2^T d_pre2; W1^T goes to region B meanwhile (its readers of the previous group are two barriers back)
        __syncthreads();
        mlp::stage<BWD_X3_BLOCK>(ldsA, blob + O_T2, T_H);
        stage_wait();
        mlp::stage<BWD_X3_BLOCK>(ldsB, blob + O_T1, T_1);
        mlp::zero_acc(acc);
        x3_steps_store<QS, 4, 4, false>(acc, ldsA, bin, lane, mlp::quad_ptr(o.d2, n, sc, h), 2 * n);
        mlp::masked_to_bin(acc, m1, bin);
        // ---- d x0 = W1^T d_pre1  (64 input features = 2 tiles)
        stage_wait();                             // W1^T has landed; every wave has left region A
        // the next group's masks and head gradients: requested under the one GEMM that holds two accumulator tiles, not four
        const Head hn = load_head(g + gridDim.x < ngroups ? g + gridDim.x : g);
        {
            f32x16 acc2[OTI1];
            mlp::zero_acc(acc2);
            x3_steps_store<QS, OTI1, OTI1, false>(acc2, ldsB, bin, lane, mlp::quad_ptr(o.d1, n, sc, h), 2 * n);
            // d x0 leaves as SAMPLE-major rows [n, 64]: through this wave's slice of region A ([32 samples][65]: conflict-free
            // both ways), each sample's 64 values then go out as one coalesced store
            float *tr = reinterpret_cast<float *>(ldsA) + (size_t)wave * (32 * 65);
            {
                float *col = tr + (lane & 31) * 65 + 4 * h;
#pragma unroll
                for (int j = 0; j < OTI1 * 16; ++j) col[32 * (j >> 4) + (j & 3) + 8 * ((j >> 2) & 3)] = acc2[j >> 4][j & 15];
            }
            const size_t s0 = g * GROUP + (size_t)wave * 32;
#pragma unroll 8
            for (int i = 0; i < 32; ++i)
                if (s0 + i < n) o.dx0[(s0 + i) * FD + lane] = tr[i * 65 + lane];
        }
        hd = hn;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no async copy outlives the block's LDS
}

size_t mlp_x3_t_blob_u4() { return N_BLOB_T; }

void launch_mlp_pack_x3_t(const MlpWeights &w, uint4 *blob_t, hipStream_t stream) {
    hipLaunchKernelGGL(k_mlp_pack_x3_t, dim3((unsigned)((PACK_T_THREADS + 255) / 256)), dim3(256), 0, stream, w, blob_t);
}

void launch_mlp_backward_x3(size_t n, const float *sigma, const float *rgb, const MlpPacks &w, const float *d_sigma, const float *d_rgb,
                            const MlpBackwardBuffers &b, hipStream_t stream) {
    if (n == 0) return;
    mlp::launch_group_kernel<k_mlp_backward_x3, BWD_X3_BLOCK>(n, (LDS_A + LDS_B) * sizeof(uint4), stream, n,
                                                               BwdIn{b.masks, sigma, rgb, d_sigma, d_rgb}, w.blob_t,
                                                               BwdOut{b.d1, b.d2, b.d3, b.d4, b.dhead, b.dx0});
}

}  // namespace tn
