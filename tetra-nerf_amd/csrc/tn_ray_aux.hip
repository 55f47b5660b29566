// tn_ray_aux.hip -- two more per-ray sums over the composite's weights, and the composite adjoint that takes their cotangents.
//
// Replaces what a nerfstudio trainer runs in PyTorch on the materialised [R, S] weights: DepthRenderer(method="expected")
// (renderers.py: sum w steps / (sum w + eps)) and losses.lossfun_distortion (mip-NeRF 360 eq. 15: an O(S^2) pairwise term per
// ray); the reference model has neither (tetranerf/nerfstudio/model.py:632-662 renders rgb, accumulation and the median depth).
// The PyTorch statement render.composite_aux_statement is the parity definition.
//
// One ray: edges e_0 <= .. <= e_S, delta_i = e_{i+1} - e_i, weights w_i EXACTLY those of ray_composite_chunks (tn_ray_ops.h: the
// same expressions in the same order, so the same bits), midpoints relative to the first edge, u'_i = ((e_i - e_0) + (e_{i+1} -
// e_0)) / 2, so that fp32 keeps its digits on a ray that starts far from the camera:
//     depth_moment   = e_0 sum w_i + sum w_i u'_i                                            (= sum w_i (e_i + e_{i+1}) / 2)
//     distortion_raw = sum_i sum_j w_i w_j |u'_i - u'_j| + (1/3) sum_i w_i^2 delta_i
// Linear time: with the exclusive prefixes W_i = sum_{j<i} w_j, WU_i = sum_{j<i} w_j u'_j (u' ascends with i)
//     sum_i sum_j w_i w_j |u'_i - u'_j| = 2 sum_i w_i (u'_i W_i - WU_i)
//     d distortion_raw / d w_k = 2 (u'_k W_k - WU_k + WU>_k - u'_k W>_k) + (2/3) w_k delta_k,    W>_k, WU>_k: the sums over j > k
//     d depth_moment / d w_k   = (e_k + e_{k+1}) / 2.
//
// k_composite_aux            forward, one wavefront per ray, no LDS: the dd scan and carry of ray_composite_chunks, then two more
//                            inclusive wave scans per chunk (w and w u') with their carries in registers; groups of CH chunks are
//                            processed together (wave_incl_scan_multi<CH>), dispatched on S like ray_composite: 2 / 5 / 9 chunks.
// k_composite_backward_aux   k_composite_backward (tn_mlp_bwd.hip; that kernel is not touched) with a_i = dL/dw_i carrying g_depth
//                            d depth_moment / dw_i + g_dist d distortion_raw / dw_i.  The near-to-far sweep leaves three floats of
//                            LDS per chunk: the carries of dd, W and WU.  The far-to-near sweep forms the prefixes from carry +
//                            in-chunk scan and the SUFFIXES AS TOTAL MINUS INCLUSIVE PREFIX: W and WU are sums of non-negative
//                            terms bounded by 1 and by the ray's span, so ulp(total) is an error of 2^-24 of the scale every
//                            term of d distortion_raw / dw has (span x 1) -- unlike sum delta sigma, whose total can be hundreds
//                            while the prefix that matters is a fraction of 1 -- and it saves two of the four extra wave scans per
//                            chunk that carried far-side sums would need.  dd's prefix stays carry + scan: w_i has the forward's bits.
// Edges are constants of the gradient.  Plain C++ HIP: no inline assembly.
#include "tn_ray_ops.h"

namespace tn {

using namespace rayops;

namespace {

template <int CH>
__device__ __forceinline__ void ray_composite_aux_chunks(uint32_t S, const float *__restrict__ sigma, const float *__restrict__ e,
                                                         float *__restrict__ out_moment, float *__restrict__ out_dist,
                                                         float *__restrict__ out_w, int lane) {
    const float e0 = e[0];
    float carry = 0.f;                 // sum of sigma * delta of all previous samples (ray_composite_chunks' carry)
    float cW = 0.f, cWU = 0.f;         // sums of w and of w u' over all previous chunks
    float accw = 0.f, swu = 0.f, pair = 0.f, self = 0.f;      // per-lane partial sums
    for (uint32_t base0 = 0; base0 < S; base0 += 64 * CH) {
        float stv[CH], env[CH], dd[CH], inc[CH];
        bool ok[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint32_t j = base0 + 64u * c + lane;
            ok[c] = j < S;
            const size_t q = ok[c] ? j : S - 1;
            stv[c] = e[q]; env[c] = e[q + 1];
            const float sg = sigma[q];
            dd[c] = ok[c] ? (env[c] - stv[c]) * sg : 0.f;
            inc[c] = dd[c];
        }
        wave_incl_scan_multi<CH>(inc, lane);
        float w[CH], u[CH], wu[CH], winc[CH], wuinc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float excl = carry + (inc[c] - dd[c]);
            float wi = (1.0f - expf(-dd[c])) * expf(-excl);
            if (!(wi == wi) || !ok[c]) wi = 0.f;  // nan_to_num
            w[c] = wi;
            carry += __shfl(inc[c], 63);
            u[c] = ((stv[c] - e0) + (env[c] - e0)) / 2.0f;
            wu[c] = wi * u[c];
            winc[c] = wi; wuinc[c] = wu[c];
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint32_t j = base0 + 64u * c + lane;
            if (out_w && ok[c]) out_w[j] = w[c];
        }
        wave_incl_scan_multi<CH>(winc, lane);
        wave_incl_scan_multi<CH>(wuinc, lane);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float Wex = cW + (winc[c] - w[c]), WUex = cWU + (wuinc[c] - wu[c]);
            pair += w[c] * (u[c] * Wex - WUex);
            self += (w[c] * w[c]) * (env[c] - stv[c]);
            accw += w[c];
            swu += wu[c];
            cW += __shfl(winc[c], 63);
            cWU += __shfl(wuinc[c], 63);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        accw += __shfl_xor(accw, off); swu += __shfl_xor(swu, off); pair += __shfl_xor(pair, off); self += __shfl_xor(self, off);
    }
    if (lane == 0) {
        if (out_moment) out_moment[0] = e0 * accw + swu;
        if (out_dist) out_dist[0] = 2.0f * pair + self / 3.0f;
    }
}

}  // namespace

__global__ __launch_bounds__(64) void k_composite_aux(size_t R, uint32_t S, const float *__restrict__ sigma,
                                                      const float *__restrict__ edges, float *__restrict__ out_moment,
                                                      float *__restrict__ out_dist, float *__restrict__ out_weights) {
    const int lane = threadIdx.x;
    for (size_t ray = blockIdx.x; ray < R; ray += gridDim.x) {
        const float *sg = sigma + ray * S, *e = edges + ray * (S + 1);
        float *om = out_moment ? out_moment + ray : nullptr, *od = out_dist ? out_dist + ray : nullptr;
        float *ow = out_weights ? out_weights + ray * S : nullptr;
        // wave-uniform dispatch on the ray's chunk count, the groups of ray_composite (same bits for any grouping)
        if (S <= 64 * 2) ray_composite_aux_chunks<2>(S, sg, e, om, od, ow, lane);
        else if (S <= 64 * 5) ray_composite_aux_chunks<5>(S, sg, e, om, od, ow, lane);
        else ray_composite_aux_chunks<9>(S, sg, e, om, od, ow, lane);
    }
}

__global__ __launch_bounds__(64) void k_composite_backward_aux(size_t R, uint32_t S, const float *__restrict__ sigma,
                                                               const float *__restrict__ rgb, const float *__restrict__ edges,
                                                               Background background, const float *__restrict__ g_rgb,
                                                               const float *__restrict__ g_acc, const float *__restrict__ g_moment,
                                                               const float *__restrict__ g_dist, float *__restrict__ d_sigma,
                                                               float *__restrict__ d_rgb) {
    extern __shared__ float carries[];                   // [3][chunks of the ray]: what dd, w and w u' sum to in front of a chunk
    const int lane = threadIdx.x;
    const uint32_t nchunks = (S + 63) / 64;
    float *c_dd = carries, *c_w = carries + nchunks, *c_wu = carries + 2 * (size_t)nchunks;
    for (size_t ray = blockIdx.x; ray < R; ray += gridDim.x) {
        const float *e = edges + ray * (S + 1);
        const float e0 = e[0];
        const float gr = g_rgb ? g_rgb[3 * ray] : 0.f, gg = g_rgb ? g_rgb[3 * ray + 1] : 0.f, gb = g_rgb ? g_rgb[3 * ray + 2] : 0.f;
        const float ga = g_acc ? g_acc[ray] : 0.f;
        const float gm = g_moment ? g_moment[ray] : 0.f, gd = g_dist ? g_dist[ray] : 0.f;
        const float a_const = ga - ((background.r * gr + background.g * gg) + background.b * gb);
        // near to far: the carries every chunk starts from
        float carry = 0.f, carry_w = 0.f, carry_wu = 0.f;
        for (uint32_t c = 0; c < nchunks; ++c) {
            const uint32_t j = c * 64 + lane;
            const bool ok = j < S;
            const float stv = ok ? e[j] : 0.f, env = ok ? e[j + 1] : 0.f;
            const float dd = ok ? (env - stv) * sigma[ray * S + j] : 0.f;
            const float inc = wave_incl_scan(dd, lane);
            const float excl = carry + (inc - dd);
            float w = (1.0f - expf(-dd)) * expf(-excl);
            if (!(ok && (w == w) && fabsf(w) <= 3.0e38f)) w = 0.f;
            float v[2] = {w, w * (((stv - e0) + (env - e0)) / 2.0f)};
            wave_incl_scan_multi<2>(v, lane);
            if (lane == 0) { c_dd[c] = carry; c_w[c] = carry_w; c_wu[c] = carry_wu; }
            carry += __shfl(inc, 63);
            carry_w += __shfl(v[0], 63);
            carry_wu += __shfl(v[1], 63);
        }
        lds_sync();
        const float w_total = carry_w, wu_total = carry_wu;
        float carry_aw = 0.f;                            // sum of a w over the chunks already processed (farther samples)
        for (uint32_t c = nchunks; c-- > 0;) {
            const uint32_t j = c * 64 + lane;
            const bool ok = j < S;
            const size_t q = ray * S + (ok ? j : S - 1);
            const float stv = ok ? e[j] : 0.f, env = ok ? e[j + 1] : 0.f;
            const float delta = env - stv;
            const float dd = ok ? delta * sigma[q] : 0.f;
            const float inc = wave_incl_scan(dd, lane);
            const float excl = c_dd[c] + (inc - dd);            // sum_{k<j} dd_k, as ray_composite_chunks forms it
            const float Ti = expf(-excl), Tn = expf(-(excl + dd));
            float w = (1.0f - expf(-dd)) * Ti;
            const bool fin = ok && (w == w) && fabsf(w) <= 3.0e38f;
            if (!fin) w = 0.f;
            const float u = ((stv - e0) + (env - e0)) / 2.0f, wu = w * u;
            float v[2] = {w, wu};
            wave_incl_scan_multi<2>(v, lane);
            const float w_incl = c_w[c] + v[0], wu_incl = c_wu[c] + v[1];
            const float w_ex = c_w[c] + (v[0] - w), wu_ex = c_wu[c] + (v[1] - wu);
            const float near_side = u * w_ex - wu_ex;                                   // sum_{k<j} w_k (u'_j - u'_k)
            const float far_side = (wu_total - wu_incl) - u * (w_total - w_incl);       // sum_{k>j} w_k (u'_k - u'_j)
            const float ddist = 2.0f * (near_side + far_side) + (2.0f / 3.0f) * (w * delta);
            const float c0 = rgb[3 * q], c1 = rgb[3 * q + 1], c2 = rgb[3 * q + 2];
            const float ai = ((((gr * c0 + gg * c1) + gb * c2) + a_const) + gm * (0.5f * (stv + env))) + gd * ddist;
            const float aw = fin ? ai * w : 0.f;
            // exclusive suffix sum of a w within the chunk: the inclusive one of the values one lane farther
            const float nxt = __shfl_down(aw, 1);
            float suf = lane < 63 ? nxt : 0.f;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const float o2 = __shfl_down(suf, off);
                if (lane + off < 64) suf += o2;
            }
            const float later = suf + carry_aw;                 // sum_{k>j} a_k w_k
            if (ok) {
                float ds = delta * (ai * Tn - later);
                if (!fin || !(ds == ds)) ds = 0.f;
                d_sigma[q] = ds;
                d_rgb[3 * q] = w * gr; d_rgb[3 * q + 1] = w * gg; d_rgb[3 * q + 2] = w * gb;
            }
            carry_aw += __shfl(suf, 0) + __shfl(aw, 0);
        }
        lds_sync();                                      // the next ray overwrites the carries
    }
}

void launch_composite_aux(size_t R, uint32_t S, const float *sigma, const float *edges, float *out_moment, float *out_dist,
                          float *out_weights, hipStream_t stream) {
    if (R == 0 || S == 0) return;
    const unsigned grid = (unsigned)(R < 256u * 32u ? R : 256u * 32u);
    hipLaunchKernelGGL(k_composite_aux, dim3(grid), dim3(64), 0, stream, R, S, sigma, edges, out_moment, out_dist, out_weights);
}

void launch_composite_backward_aux(size_t R, uint32_t S, const float *sigma, const float *rgb, const float *edges, Background background,
                                   const float *d_out_rgb, const float *d_out_acc, const float *d_out_moment, const float *d_out_dist,
                                   float *d_sigma, float *d_rgb, hipStream_t stream) {
    if (R == 0 || S == 0) return;
    const size_t smem = 3 * (((size_t)S + 63) / 64) * sizeof(float);
    if (smem > 64 * 1024) throw Error("composite_backward: too many samples per ray");
    const unsigned grid = (unsigned)(R < 256u * 32u ? R : 256u * 32u);
    hipLaunchKernelGGL(k_composite_backward_aux, dim3(grid), dim3(64), smem, stream, R, S, sigma, rgb, edges, background, d_out_rgb,
                       d_out_acc, d_out_moment, d_out_dist, d_sigma, d_rgb);
}

}  // namespace tn
