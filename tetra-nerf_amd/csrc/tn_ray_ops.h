// tn_ray_ops.h -- the per-RAY stages between trace_rays and the frame (coarse sampler, PDF sampler, matcher, composite) as
// wave-level device functions: ONE wavefront works on one ray.  The stand-alone kernels (k_sample_coarse / k_sample_pdf in
// tn_samplers.hip, k_find_matched in tn_match.hip, k_composite in tn_mlp.hip) and the persistent render kernel
// (tn_render_rays.hip) call the SAME functions, so a ray's values do not depend on which launch shape produced them.
// Reference: tetranerf/nerfstudio/model.py:111-192, 531-557, 560-567, 582-586, 632-662, src/tetrahedra_tracer.cu:115-160 (+
// nerfstudio's UniformSampler / PDFSampler / RaySamples.get_weights / renderers, restated in tetra-nerf_amd/render.py -- those
// PyTorch statements are the parity definition).
#pragma once
#include "tn_device.h"
#include "tn_kernels.h"

namespace tn {
namespace rayops {

__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}
// running maximum over an LDS array of n floats (wave-cooperative): makes a list that is sorted up to rounding
// (an inversion of an ulp between neighbours) non-decreasing, so that the merge by rank below is a permutation
__device__ __forceinline__ void lds_running_max(float *a, uint32_t n, int lane) {
    float carry = -INFINITY;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t k = base + lane;
        float v = k < n ? a[k] : -INFINITY;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float o = __shfl_up(v, off);
            if (lane >= off) v = fmaxf(v, o);
        }
        v = fmaxf(v, carry);
        if (k < n) a[k] = v;
        carry = __shfl(v, 63);
    }
}
// CH independent inclusive wave scans (sum / running maximum), step by step TOGETHER: a scan is a chain of six dependent
// cross-lane moves (ds_bpermute: an LDS-crossbar round trip each), and a wave that owns its ray alone -- the persistent render
// kernel runs 8 waves per CU -- has nothing to fill the gaps with but the other chunks' chains.  Per chunk the operations and
// their order are exactly those of wave_incl_scan: same bits.
template <int CH>
__device__ __forceinline__ void wave_incl_scan_multi(float (&v)[CH], int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        float o[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) o[c] = __shfl_up(v[c], off);
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if (lane >= off) v[c] += o[c];
    }
}
template <int CH>
__device__ __forceinline__ void wave_incl_max_multi(float (&v)[CH], int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        float o[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) o[c] = __shfl_up(v[c], off);
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if (lane >= off) v[c] = fmaxf(v[c], o[c]);
    }
}
// running maximum over an LDS array of n <= 64 CH floats, the chunks' scans interleaved (same values as lds_running_max)
template <int CH>
__device__ __forceinline__ void lds_running_max_multi(float *a, uint32_t n, int lane) {
    float v[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) { const uint32_t k = 64u * c + lane; v[c] = k < n ? a[k] : -INFINITY; }
    wave_incl_max_multi<CH>(v, lane);
    float carry = -INFINITY;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint32_t k = 64u * c + lane;
        const float m = fmaxf(v[c], carry);
        if (k < n) a[k] = m;
        carry = __shfl(m, 63);
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ void lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Coarse sampler of one hitting ray (model.py:531-557, 111-122, 166-177): near / far + the S + 1 bin edges.
// `ray` = its row in the trace outputs; lin [S+1] = linspace(0, 1, S+1); t_row [S+1] uniform draws of THIS ray or null
// (evaluation); cum: M + 1 floats of LDS owned by the wave (biased only); edges [S+1], near_far [2] of THIS ray.
// ray_sample_coarse_nf: nb = num_visited[ray] and the ray's near / far are the CALLER's (the persistent kernel loads them for a
// whole tile at once); edges2 (nullable): a second copy of the edges, e.g. in the wave's LDS for the matcher that follows.
__device__ __forceinline__ void ray_sample_coarse_nf(uint32_t S, uint32_t M, size_t ray, uint32_t nb, float near, float far,
                                                     const float *__restrict__ hit_dist, const float *__restrict__ lin,
                                                     const float *__restrict__ t_row, int biased, float *__restrict__ edges,
                                                     float *edges2, float *cum, int lane) {
    const float2 *row = reinterpret_cast<const float2 *>(hit_dist + ray * (size_t)M * 2);
    if (biased) {
        // lengths (clamped at 0: the cell -1 closing segments) and their running sum from the first entry point
        float carry = near;   // bounds_start = hit_distances[..., 0, 0]
        if (lane == 0) cum[0] = carry;
        for (uint32_t base = 0; base < nb; base += 64) {
            const uint32_t k = base + lane;
            float len = 0.f;
            if (k < nb) { const float2 s = row[k]; len = fmaxf(s.y - s.x, 0.f); }
            const float inc = wave_incl_scan(len, lane);
            if (k < nb) cum[k + 1] = carry + inc;
            carry += __shfl(inc, 63);
        }
        lds_sync();
    }
    const float fnb = (float)nb;
    for (uint32_t j = lane; j <= S; j += 64) {
        float b = lin[j];
        if (t_row) {   // stratified: every edge jittered between the centres of its two neighbouring bins
            const float lower = j == 0 ? lin[0] : (lin[j] + lin[j - 1]) / 2.0f;
            const float upper = j == S ? lin[S] : (lin[j + 1] + lin[j]) / 2.0f;
            b = lower + (upper - lower) * t_row[j];
        }
        float e = b * far + (1.0f - b) * near;
        if (biased && nb) {
            float rest = (e - near) / (far - near) * fnb;
            float iv = floorf(rest);
            iv = fminf(iv, fnb - 1.0f);
            iv = fmaxf(iv, 0.0f);
            rest = rest - iv;
            const uint32_t i = (uint32_t)iv;
            const float2 s = row[i];
            e = cum[i] + fmaxf(s.y - s.x, 0.f) * rest;
        }
        edges[j] = e;
        if (edges2) edges2[j] = e;
    }
    if (biased || edges2) lds_sync();
}

// the same with near / far read from the ray's row (the stand-alone kernel); near_far [2] of THIS ray
__device__ __forceinline__ void ray_sample_coarse(uint32_t S, uint32_t M, size_t ray, uint32_t nb,
                                                  const float *__restrict__ hit_dist, const float *__restrict__ lin,
                                                  const float *__restrict__ t_row, int biased, float *__restrict__ edges,
                                                  float *__restrict__ near_far, float *cum, int lane) {
    const float2 *row = reinterpret_cast<const float2 *>(hit_dist + ray * (size_t)M * 2);
    // (a ray that misses the mesh has no row -- with compact rows not even a written one: the sync-free training path
    // names such rays only when a whole batch misses; their samples are discarded, they just have to be finite)
    const float near = nb ? row[0].x : 0.0f;
    const float far = nb ? row[nb - 1].y : 1.0f;
    if (lane == 0) { near_far[0] = near; near_far[1] = far; }
    ray_sample_coarse_nf(S, M, ray, nb, near, far, hit_dist, lin, t_row, biased, edges, nullptr, cum, lane);
}

// Live lengths of one ray for the occupancy-guided sampler (render.live_lengths_statement; the reference declares the occupancy
// field and never uses it, model.py:98-99,256-265): w_k = max(t_out_k - t_in_k, 0) for a LIVE segment -- one that
// cull_mask_statement would not cull: cell_k >= T, or not occupancy[cell_k] < threshold -- else 0.  cum [nb + 1] (M + 1 floats
// of LDS owned by the wave): cum[0] = 0, cum[k + 1] = the running MAXIMUM over the segments j <= k with w_j > 0 of the prefix
// sum w_0 + .. + w_j -- the prefix sums themselves, made non-decreasing and exactly flat over every segment of weight 0
// whatever the summation tree of the wave scan rounds to, so that "first k with cum[k + 1] > s" always names a segment with
// w_k > 0.  A ray whose live length is 0 (everything culled) is redone with every segment live.  Returns near = the first t_in,
// L = cum[nb], last = the last segment with w > 0 (0 without one); a row without a segment: (0, 1, 0), cum[0] = 0.
struct LiveCum { float near, L; uint32_t last; };
constexpr int LIVE_CH = 4;    // chunks of 64 segments (ray_live_cum) / of 64 values (ray_live_to_distance) in flight per wave

__device__ __forceinline__ LiveCum ray_live_cum(uint32_t M, size_t ray, uint32_t nb, const uint32_t *__restrict__ visited,
                                                const float *__restrict__ hit_dist, const float *__restrict__ occupancy, uint32_t T,
                                                float threshold, float *cum, int lane) {
    if (nb > M) nb = M;
    const float2 *row = reinterpret_cast<const float2 *>(hit_dist + ray * (size_t)M * 2);
    const uint32_t *vis = visited + ray * (size_t)M;
    LiveCum res;
    res.near = 0.f; res.L = 1.f; res.last = 0;
    if (lane == 0) cum[0] = 0.f;
    if (nb == 0) { lds_sync(); return res; }
    res.near = row[0].x;
    const bool culls = T > 0 && threshold > 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        float carry = 0.f, top = 0.f;
        uint32_t last = 0;
        for (uint32_t base0 = 0; base0 < nb; base0 += 64 * LIVE_CH) {
            float w[LIVE_CH], inc[LIVE_CH], mx[LIVE_CH];
#pragma unroll
            for (int c = 0; c < LIVE_CH; ++c) {
                const uint32_t k = base0 + 64u * c + lane;
                w[c] = 0.f;
                if (k < nb) {
                    const float2 s = row[k];
                    bool live = true;
                    if (culls && pass == 0) {
                        const uint32_t cell = vis[k];
                        if (cell < T) live = !(occupancy[cell] < threshold);
                    }
                    w[c] = live ? fmaxf(s.y - s.x, 0.f) : 0.f;
                }
                inc[c] = w[c];
            }
            wave_incl_scan_multi<LIVE_CH>(inc, lane);
#pragma unroll
            for (int c = 0; c < LIVE_CH; ++c) {
                mx[c] = w[c] > 0.f ? carry + inc[c] : 0.f;
                carry += __shfl(inc[c], 63);
            }
            wave_incl_max_multi<LIVE_CH>(mx, lane);
#pragma unroll
            for (int c = 0; c < LIVE_CH; ++c) {
                const uint32_t k = base0 + 64u * c + lane;
                const float m = fmaxf(mx[c], top);
                if (k < nb) cum[k + 1] = m;
                top = __shfl(m, 63);
                const uint64_t pos = __ballot(w[c] > 0.f);
                if (pos) last = base0 + 64u * c + (63u - (uint32_t)__clzll((long long)pos));
            }
        }
        res.L = top; res.last = last;
        if (top > 0.f || !culls) break;
    }
    lds_sync();
    return res;
}

// The binary searches of searchsorted / the merge by rank, for the CH items a lane owns AT ONCE: the classic lo / hi / mid loop
// with a fixed trip count (K >= the longest search; a finished item idles), so every item visits exactly the mids the plain
// loop visits -- same result on any array, sorted or not -- while the LDS reads of the CH items overlap instead of forming one
// chain of K dependent round trips per item (a wave that owns its ray alone has nothing else to hide them behind).
// LE: count of entries <= v (searchsorted side = "right"); otherwise: entries < v.
template <int CH, bool LE>
__device__ __forceinline__ void multi_search(const float *arr, uint32_t N, const float (&v)[CH], const bool (&on)[CH], uint32_t (&res)[CH]) {
    uint32_t lo[CH], hi[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) { lo[c] = 0; hi[c] = N; }
    const int K = N ? 32 - __clz((int)N) : 0;     // a range of N halves to nothing in at most floor(log2 N) + 1 steps
    const uint32_t last = N ? N - 1 : 0;
    for (int it = 0; it < K; ++it) {
        // straight-line (selects, no exec-masked branches): the CH reads of a step are issued together
        uint32_t mid[CH];
        float a[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) { mid[c] = (lo[c] + hi[c]) >> 1; a[c] = arr[mid[c] < last ? mid[c] : last]; }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const bool act = on[c] && lo[c] < hi[c];
            const bool take = LE ? (a[c] <= v[c]) : (a[c] < v[c]);
            lo[c] = (act && take) ? mid[c] + 1 : lo[c];
            hi[c] = (act && !take) ? mid[c] : hi[c];
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) res[c] = lo[c];
}

// render.live_to_distance_statement for n values of one ray, after ray_live_cum (cum, lc): s' = clamp(s - near, 0, L); k = the
// first segment with cum[k + 1] > s' (multi_search: LIVE_CH values per lane, their reads issued together), or the last segment
// with w > 0 when there is none; the segment's row is gathered after the search; t = min(t_in + frac len, t_out) with frac =
// clamp((s' - cum[k]) / len, 0, 1) -- w_k = len_k at every segment the search can name -- so t lies inside segment k bit-wise.
// A row without a segment: t = s, slot 0.  s [n]; out: t [n], slot [n] of THIS ray.
__device__ __forceinline__ void ray_live_to_distance(uint32_t n, uint32_t M, size_t ray, uint32_t nb, const float *__restrict__ hit_dist,
                                                     const float *__restrict__ s, const LiveCum &lc, const float *cum,
                                                     float *__restrict__ t, uint32_t *__restrict__ slot, int lane) {
    if (nb > M) nb = M;
    const float2 *row = reinterpret_cast<const float2 *>(hit_dist + ray * (size_t)M * 2);
    for (uint32_t base0 = 0; base0 < n; base0 += 64 * LIVE_CH) {
        float v[LIVE_CH], sv[LIVE_CH];
        bool on[LIVE_CH];
        uint32_t k[LIVE_CH];
#pragma unroll
        for (int c = 0; c < LIVE_CH; ++c) {
            const uint32_t j = base0 + 64u * c + lane;
            on[c] = j < n;
            sv[c] = on[c] ? s[j] : 0.f;
            v[c] = fminf(fmaxf(sv[c] - lc.near, 0.f), lc.L);
        }
        multi_search<LIVE_CH, true>(cum + 1, nb, v, on, k);      // entries of cum[1 .. nb] that are <= s'
        float2 seg[LIVE_CH];
        float c0[LIVE_CH];
#pragma unroll
        for (int c = 0; c < LIVE_CH; ++c) {
            if (k[c] >= nb) k[c] = lc.last;
            seg[c] = make_float2(0.f, 0.f);
            c0[c] = 0.f;
            if (on[c] && nb) { seg[c] = row[k[c]]; c0[c] = cum[k[c]]; }
        }
#pragma unroll
        for (int c = 0; c < LIVE_CH; ++c) {
            const uint32_t j = base0 + 64u * c + lane;
            if (!on[c]) continue;
            const float len = fmaxf(seg[c].y - seg[c].x, 0.f);
            const float frac = len > 0.f ? fminf(fmaxf((v[c] - c0[c]) / len, 0.f), 1.f) : 0.f;
            t[j] = nb ? fminf(seg[c].x + frac * len, seg[c].y) : sv[c];
            slot[j] = k[c];
        }
    }
}

// floats of LDS ray_sample_pdf needs per wave
__host__ __device__ constexpr size_t pdf_lds_floats(uint32_t S, uint32_t nb) { return 2 * (size_t)(S + 1) + nb; }

// nerfstudio's PDFSampler (include_original) for one ray (model.py:582-586): e [S+1] euclidean coarse edges, w [S] coarse
// weights -> out [S + 1 + nb] merged, sorted euclidean edges (nb = num_fine + 1).  u_table [nb]: evaluation = the bin-centred
// quantiles, training = the bin starts, to which u_row [nb] / nb is added (u_row null otherwise).  lds: pdf_lds_floats(S, nb).
// ray_sample_pdf_chunks<CH>: S + 1 <= 64 CH and nb <= 64 CH -- every load of the ray requested before its first use, the
// chunks' scans and the lane's binary searches interleaved (see wave_incl_scan_multi / multi_search); ray_sample_pdf_loops:
// any size, plain loops.  Same expressions in the same order: same bits.
template <int CH>
__device__ __forceinline__ void ray_sample_pdf_chunks(uint32_t S, uint32_t nb, const float *__restrict__ e, const float *__restrict__ w,
                                                      float near, float far, const float *__restrict__ u_table,
                                                      const float *__restrict__ u_row, float histogram_padding, float eps,
                                                      float *__restrict__ o, float *lds, int lane, float *o2 = nullptr) {
    float *cdf = lds;                // [S+1]
    float *sp = cdf + (S + 1);       // [S+1] spacing edges
    float *nw = sp + (S + 1);        // [nb]  new bins
    float ev[CH], wv[CH], uv[CH];
    bool on[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint32_t j = 64u * c + lane;
        ev[c] = j <= S ? e[j] : 0.f;
        wv[c] = j < S ? w[j] : 0.f;
        on[c] = j < nb;
        uv[c] = 0.f;
        if (on[c]) {
            float u = u_table[j];
            if (u_row) u = u + u_row[j] / (float)nb;
            uv[c] = u;
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint32_t j = 64u * c + lane;
        if (j <= S) sp[j] = (ev[c] - near) / (far - near);
    }
    // padded weights -> pdf -> cdf
    float part = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint32_t j = 64u * c + lane;
        if (j < S) part += wv[c] + histogram_padding;
    }
    float wsum = wave_sum(part);
    const float padding = fmaxf(eps - wsum, 0.f);
    const float add = padding / (float)S;
    wsum = wsum + padding;
    float inc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint32_t j = 64u * c + lane;
        inc[c] = j < S ? ((wv[c] + histogram_padding) + add) / wsum : 0.f;
    }
    wave_incl_scan_multi<CH>(inc, lane);
    float carry = 0.f;
    if (lane == 0) cdf[0] = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint32_t j = 64u * c + lane;
        if (j < S) cdf[j + 1] = fminf(1.0f, carry + inc[c]);
        carry += __shfl(inc[c], 63);
    }
    lds_sync();
    // inverse CDF at the quantiles
    uint32_t pos[CH];
    multi_search<CH, true>(cdf, S + 1, uv, on, pos);         // searchsorted(cdf, u, side = "right"): number of entries <= u
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint32_t k = 64u * c + lane, lo = pos[c];
        const float u = uv[c];
        const uint32_t below = lo == 0 ? 0u : (lo - 1 > S ? S : lo - 1), above = lo > S ? S : lo;
        const float c0 = cdf[below], c1 = cdf[above], b0 = sp[below], b1 = sp[above];
        float t = (u - c0) / (c1 - c0);
        if (!(t == t)) t = 0.f;                                   // nan_to_num(., 0)
        if (t == INFINITY) t = 3.4028234663852886e38f;            // nan_to_num maps +-inf to the finite extremes
        if (t == -INFINITY) t = -3.4028234663852886e38f;
        t = fminf(fmaxf(t, 0.f), 1.f);
        if (on[c]) nw[k] = b0 + t * (b1 - b0);
    }
    lds_sync();
    // both lists are sorted up to rounding (the biased mapping and the inverse CDF are monotone functions evaluated
    // in fp32): enforce it, then merge by rank (coarse edges first on ties) and map back to euclidean distances
    lds_running_max_multi<CH>(sp, S + 1, lane);
    lds_running_max_multi<CH>(nw, nb, lane);
    lds_sync();
    float vv[CH];
    bool on2[CH];
    uint32_t rk[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) { const uint32_t j = 64u * c + lane; on2[c] = j <= S; vv[c] = on2[c] ? sp[j] : 0.f; }
    multi_search<CH, false>(nw, nb, vv, on2, rk);            // new bins strictly below v
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (on2[c]) {
            const float ev2 = vv[c] * far + (1.0f - vv[c]) * near;
            o[64u * c + lane + rk[c]] = ev2;
            if (o2) o2[64u * c + lane + rk[c]] = ev2;
        }
#pragma unroll
    for (int c = 0; c < CH; ++c) { const uint32_t k = 64u * c + lane; on2[c] = k < nb; vv[c] = on2[c] ? nw[k] : 0.f; }
    multi_search<CH, true>(sp, S + 1, vv, on2, rk);          // coarse edges <= v
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (on2[c]) {
            const float ev2 = vv[c] * far + (1.0f - vv[c]) * near;
            o[64u * c + lane + rk[c]] = ev2;
            if (o2) o2[64u * c + lane + rk[c]] = ev2;
        }
    lds_sync();
}

__device__ __forceinline__ void ray_sample_pdf_loops(uint32_t S, uint32_t nb, const float *__restrict__ e, const float *__restrict__ w,
                                                     float near, float far, const float *__restrict__ u_table,
                                                     const float *__restrict__ u_row, float histogram_padding, float eps,
                                                     float *__restrict__ o, float *lds, int lane) {
    float *cdf = lds;                // [S+1]
    float *sp = cdf + (S + 1);       // [S+1] spacing edges
    float *nw = sp + (S + 1);        // [nb]  new bins
    for (uint32_t j = lane; j <= S; j += 64) sp[j] = (e[j] - near) / (far - near);
    // padded weights -> pdf -> cdf
    float part = 0.f;
    for (uint32_t j = lane; j < S; j += 64) part += w[j] + histogram_padding;
    float wsum = wave_sum(part);
    const float padding = fmaxf(eps - wsum, 0.f);
    const float add = padding / (float)S;
    wsum = wsum + padding;
    float carry = 0.f;
    if (lane == 0) cdf[0] = 0.f;
    for (uint32_t base = 0; base < S; base += 64) {
        const uint32_t j = base + lane;
        const float pdf = j < S ? ((w[j] + histogram_padding) + add) / wsum : 0.f;
        const float inc = wave_incl_scan(pdf, lane);
        if (j < S) cdf[j + 1] = fminf(1.0f, carry + inc);
        carry += __shfl(inc, 63);
    }
    lds_sync();
    // inverse CDF at the quantiles
    for (uint32_t k = lane; k < nb; k += 64) {
        float u = u_table[k];
        if (u_row) u = u + u_row[k] / (float)nb;
        // searchsorted(cdf, u, side = "right"): number of entries <= u
        uint32_t lo = 0, hi = S + 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
        }
        const uint32_t below = lo == 0 ? 0u : (lo - 1 > S ? S : lo - 1), above = lo > S ? S : lo;
        const float c0 = cdf[below], c1 = cdf[above], b0 = sp[below], b1 = sp[above];
        float t = (u - c0) / (c1 - c0);
        if (!(t == t)) t = 0.f;                                   // nan_to_num(., 0)
        if (t == INFINITY) t = 3.4028234663852886e38f;            // nan_to_num maps +-inf to the finite extremes
        if (t == -INFINITY) t = -3.4028234663852886e38f;
        t = fminf(fmaxf(t, 0.f), 1.f);
        nw[k] = b0 + t * (b1 - b0);
    }
    lds_sync();
    lds_running_max(sp, S + 1, lane);
    lds_running_max(nw, nb, lane);
    lds_sync();
    for (uint32_t j = lane; j <= S; j += 64) {
        const float v = sp[j];
        uint32_t lo = 0, hi = nb;                                 // new bins strictly below v
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (nw[mid] < v) lo = mid + 1; else hi = mid; }
        o[j + lo] = v * far + (1.0f - v) * near;
    }
    for (uint32_t k = lane; k < nb; k += 64) {
        const float v = nw[k];
        uint32_t lo = 0, hi = S + 1;                              // coarse edges <= v
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sp[mid] <= v) lo = mid + 1; else hi = mid; }
        o[k + lo] = v * far + (1.0f - v) * near;
    }
    lds_sync();
}

__device__ __forceinline__ void ray_sample_pdf(uint32_t S, uint32_t nb, const float *__restrict__ e, const float *__restrict__ w,
                                               float near, float far, const float *__restrict__ u_table,
                                               const float *__restrict__ u_row, float histogram_padding, float eps,
                                               float *__restrict__ o, float *lds, int lane, float *o2 = nullptr) {
    // o2 (nullable): a second copy of the merged edges (the wave's LDS, for the matcher that follows); returns through *o2
    // only in the chunk forms -- the caller falls back to `o` otherwise (pdf_writes_second_copy)
    const uint32_t big = S + 1 > nb ? S + 1 : nb;       // wave-uniform dispatch on the chunks a lane owns
    if (big <= 64 * 3) ray_sample_pdf_chunks<3>(S, nb, e, w, near, far, u_table, u_row, histogram_padding, eps, o, lds, lane, o2);
    else if (big <= 64 * 5) ray_sample_pdf_chunks<5>(S, nb, e, w, near, far, u_table, u_row, histogram_padding, eps, o, lds, lane, o2);
    else ray_sample_pdf_loops(S, nb, e, w, near, far, u_table, u_row, histogram_padding, eps, o, lds, lane);
}
__host__ __device__ constexpr bool pdf_writes_second_copy(uint32_t S, uint32_t nb) { return (S + 1 > nb ? S + 1 : nb) <= 64 * 5; }

// RaySamples.get_weights + RGB (background blend) / accumulation / median-depth renderers of one ray (model.py:632-662):
// sigma [S], rgb [S,3] (null: weights only), e [S+1]; out_rgb3 / out_acc / out_depth: where THIS ray's results go (null: not
// written); out_w [S] (nullable; global or LDS).  Lanes stride the samples; exclusive scan of sigma * delta.
// The chunks of 64 samples form a serial chain only through their CARRIES (two scalars per chunk); their loads and their two
// wave scans are independent.  A wave that owns a ray alone (8 waves per CU in the persistent render kernel) would otherwise
// walk 2 x 6 dependent cross-lane moves per chunk with nothing to overlap them with: groups of CH chunks are processed
// together -- all loads first, the CH scans of sigma * delta interleaved, the carries in order, the CH scans of the weights
// interleaved, the median search in order.  Per sample the expressions and their order are unchanged: same bits for any CH.
template <int CH>
__device__ __forceinline__ void ray_composite_chunks(uint32_t S, const float *__restrict__ sigma, const float *__restrict__ rgb,
                                                     const float *__restrict__ e, const Background &background,
                                                     float *__restrict__ out_rgb3, float *__restrict__ out_acc,
                                                     float *__restrict__ out_depth, float *out_w, int lane) {
    float carry = 0.f;       // sum of sigma*delta of all previous samples
    float cw = 0.f;          // running sum of weights (for the median depth)
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, accw = 0.f;
    float depth = 0.f;
    bool found = false;
    for (uint32_t base0 = 0; base0 < S; base0 += 64 * CH) {
        float stv[CH], env[CH], dd[CH], inc[CH], k0[CH], k1[CH], k2[CH];
        bool ok[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint32_t j = base0 + 64u * c + lane;
            ok[c] = j < S;
            const size_t q = ok[c] ? j : S - 1;
            stv[c] = e[q]; env[c] = e[q + 1];
            const float sg = sigma[q];
            k0[c] = k1[c] = k2[c] = 0.f;
            if (rgb && ok[c]) { k0[c] = rgb[3 * q]; k1[c] = rgb[3 * q + 1]; k2[c] = rgb[3 * q + 2]; }
            dd[c] = ok[c] ? (env[c] - stv[c]) * sg : 0.f;
            inc[c] = dd[c];
        }
        wave_incl_scan_multi<CH>(inc, lane);      // inclusive scans of dd over the wave, one per chunk
        float w[CH], winc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float excl = carry + (inc[c] - dd[c]);
            float wi = (1.0f - expf(-dd[c])) * expf(-excl);
            if (!(wi == wi) || !ok[c]) wi = 0.f;  // nan_to_num
            w[c] = wi;
            winc[c] = wi;
            carry += __shfl(inc[c], 63);
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint32_t j = base0 + 64u * c + lane;
            if (out_w && ok[c]) out_w[j] = w[c];
            if (rgb) {
                float c0 = k0[c], c1 = k1[c], c2 = k2[c];
                if (background.clamp) { c0 = nan_to_num(c0); c1 = nan_to_num(c1); c2 = nan_to_num(c2); }
                r0 += w[c] * c0; r1 += w[c] * c1; r2 += w[c] * c2;
            }
            accw += w[c];
        }
        wave_incl_scan_multi<CH>(winc, lane);     // median depth: cumulative weights
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float cum = cw + winc[c];
            const uint64_t m = __ballot(ok[c] && cum >= 0.5f);
            if (!found && m) {                    // first sample whose cumulative weight reaches 0.5
                const int src = __ffsll((unsigned long long)m) - 1;
                depth = __shfl(0.5f * (stv[c] + env[c]), src);
                found = true;
            }
            cw += __shfl(winc[c], 63);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        r0 += __shfl_xor(r0, off); r1 += __shfl_xor(r1, off); r2 += __shfl_xor(r2, off); accw += __shfl_xor(accw, off);
    }
    if (!found) depth = 0.5f * (e[S - 1] + e[S]);  // searchsorted clamps to the last sample
    if (lane == 0 && out_rgb3) {
        float o0 = r0 + background.r * (1.0f - accw), o1 = r1 + background.g * (1.0f - accw), o2 = r2 + background.b * (1.0f - accw);
        if (background.clamp) { o0 = fminf(fmaxf(o0, 0.f), 1.f); o1 = fminf(fmaxf(o1, 0.f), 1.f); o2 = fminf(fmaxf(o2, 0.f), 1.f); }
        out_rgb3[0] = o0; out_rgb3[1] = o1; out_rgb3[2] = o2;
        out_acc[0] = accw;
        out_depth[0] = depth;
    }
}

__device__ __forceinline__ void ray_composite(uint32_t S, const float *__restrict__ sigma, const float *__restrict__ rgb,
                                              const float *__restrict__ e, const Background &background, float *__restrict__ out_rgb3,
                                              float *__restrict__ out_acc, float *__restrict__ out_depth, float *out_w, int lane) {
    // wave-uniform dispatch on the ray's chunk count (chunks beyond S cost scans of zeros: the groups are sized to the
    // shipped sample counts -- 128 / 256 / 257 / 513 -- with little waste)
    if (S <= 64 * 2) ray_composite_chunks<2>(S, sigma, rgb, e, background, out_rgb3, out_acc, out_depth, out_w, lane);
    else if (S <= 64 * 5) ray_composite_chunks<5>(S, sigma, rgb, e, background, out_rgb3, out_acc, out_depth, out_w, lane);
    else ray_composite_chunks<9>(S, sigma, rgb, e, background, out_rgb3, out_acc, out_depth, out_w, lane);
}

// global-memory hand-over between two steps of the SAME wave (a lane reads, or overwrites, what another lane of its wave wrote)
__device__ __forceinline__ void wave_global_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// The matcher (find_visited_cells, src/tetrahedra_tracer.cu:115-160) of one ray: its S sample distances against its n <= M
// sorted segments, entry / exit barycentrics lerped.  The per-sample two-pointer merge of the reference becomes an independent
// binary search over the running maximum of t_out (valid because the sample distances ascend: the sequential pointer equals
// "first segment whose t_out >= d"); rays whose distances do not ascend take the literal serial walk
// on lane 0.  All outputs are written by consecutive lanes, including the defaults the reference gets from torch::full / zeros
// (src/py_binding.cpp:188-191).
// MatchRows: the trace rows (all rays; `src` = this ray's row).  MatchOut: the outputs of THIS ray ([S] / [S] / [S,4] / [S,3]).
// dist_of(j): distance of sample j (a row of distances in k_find_matched, the centre of bin j of the ray's edges in the render
// kernel).  FULL: mask and cell ids too (the MLP kernels read vertex ids and barycentrics only).  PRE: dv0 holds the ray's
// first 512 bounds as load_bounds() requested them (the render kernel issues that ahead of the sampler / composite of the same
// ray, so that the rows are back when the matcher starts); otherwise they are loaded here, in place.
// tin / pmax: 2 M floats of LDS owned by the wave alone (hence lds_sync, not a block barrier).
struct MatchRows { const uint32_t *visited; const float *dist, *bary; const uint32_t *verts; };
struct MatchOut { uint32_t *cells; uint8_t *mask; uint32_t *verts; float *bary; };

__device__ __forceinline__ void load_bounds(uint32_t M, size_t src, uint32_t n, const float *dist, float2 (&dv)[8], int lane) {
    if (n > M) n = M;
    const float2 *drow = reinterpret_cast<const float2 *>(dist) + src * M;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t j = 64u * c + lane;
        dv[c] = make_float2(0.f, -INFINITY);
        if (j < n) dv[c] = drow[j];
    }
}

template <int UM, bool FULL, bool PRE, typename Dist>
__device__ __forceinline__ void ray_match(uint32_t S, uint32_t M, size_t src, uint32_t n, const MatchRows &rows, Dist dist_of,
                                          const MatchOut &out, float *tin, float *pmax, int lane, const float2 (&dv0)[8]) {
    if (n > M) n = M;
    const float2 *drow = reinterpret_cast<const float2 *>(rows.dist) + src * M;
    // do the sample distances ascend?  The loads of a whole group of 64 UM samples (with the neighbours the test needs) are
    // requested together: the wave owns its ray alone and every dependent round trip is exposed.
    bool bad = false;
    for (uint32_t base = 0; base + 1 < S; base += 64 * UM) {
        float a0[UM], a1[UM];
#pragma unroll
        for (int u = 0; u < UM; ++u) {
            const uint32_t j = base + 64 * u + lane;
            a0[u] = a1[u] = 0.f;
            if (j + 1 < S) { a0[u] = dist_of(j); a1[u] = dist_of(j + 1); }
        }
#pragma unroll
        for (int u = 0; u < UM; ++u) {
            const uint32_t j = base + 64 * u + lane;
            if (j + 1 < S) bad |= !(a0[u] <= a1[u]);
        }
    }
    // stage bounds + inclusive running max of t_out (wave scans over chunks of 64; the rows of up to 8 chunks requested at once,
    // their scans interleaved: wave_incl_max_multi)
    float carry = -INFINITY;
    for (uint32_t base0 = 0; base0 < n; base0 += 512) {
        float2 dv[8];
        float mx[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t j = base0 + 64u * c + lane;
            if (PRE && !base0) dv[c] = dv0[c];
            else { dv[c] = make_float2(0.f, -INFINITY); if (j < n) dv[c] = drow[j]; }   // (PRE: rays with more than 512 segments)
            mx[c] = dv[c].y;
        }
        wave_incl_max_multi<8>(mx, lane);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t j = base0 + 64u * c + lane;
            const float m = fmaxf(mx[c], carry);
            if (j < n) { tin[j] = dv[c].x; pmax[j] = m; }
            carry = __shfl(m, 63);
        }
    }
    const bool ascending = (__ballot(bad) == 0ull);
    lds_sync();

    if (ascending) {
        // UM sample chunks of 64 per iteration: their searches (LDS) and segment gathers (global) are independent, so the
        // dependent chain search -> gather -> store is paid once per 64 UM samples
        uint32_t top = 1;                       // largest power of two <= n (0 for n == 0)
        while ((top << 1) <= n && (top << 1) != 0) top <<= 1;
        if (n == 0) top = 0;
        const uint32_t nlast = n ? n - 1 : 0;
        for (uint32_t base = 0; base < S; base += 64 * UM) {
            float cur[UM];
            uint32_t p[UM];
#pragma unroll
            for (int u = 0; u < UM; ++u) {
                const uint32_t j = base + 64 * u + lane;
                cur[u] = j < S ? dist_of(j) : 0.f;
                p[u] = 0;
            }
            // p = number of segments whose running-max t_out is below the sample = first p with pmax[p] >= cur.  Straight-line
            // (clamped reads + selects): the UM reads of a step are issued together
            for (uint32_t bit = top; bit > 0; bit >>= 1) {
                float pv[UM];
#pragma unroll
                for (int u = 0; u < UM; ++u) { const uint32_t k = p[u] + bit - 1; pv[u] = pmax[k < nlast ? k : nlast]; }
#pragma unroll
                for (int u = 0; u < UM; ++u) p[u] = (p[u] + bit <= n && pv[u] < cur[u]) ? p[u] + bit : p[u];
            }
            bool mk[UM];
            uint32_t cell[UM];
            uint4 vv[UM];
            float t_in[UM], t_out[UM], tv[UM];
            float2 q0[UM], q1[UM], q2[UM];
#pragma unroll
            for (int u = 0; u < UM; ++u) tv[u] = tin[p[u] < nlast ? p[u] : nlast];
#pragma unroll
            for (int u = 0; u < UM; ++u) {
                const uint32_t j = base + 64 * u + lane;
                mk[u] = false; cell[u] = TN_EMPTY; vv[u] = make_uint4(TN_EMPTY, TN_EMPTY, TN_EMPTY, TN_EMPTY);
                t_in[u] = 0.f; t_out[u] = 1.f; q0[u] = q1[u] = q2[u] = make_float2(0.f, 0.f);
                if (j < S && p[u] < n && tv[u] <= cur[u]) {
                    const size_t g = src * M + p[u];
                    mk[u] = true;
                    t_in[u] = tv[u]; t_out[u] = drow[p[u]].y;
                    if (FULL) cell[u] = rows.visited[g];
                    vv[u] = *reinterpret_cast<const uint4 *>(rows.verts + 4 * g);
                    const float2 *bp = reinterpret_cast<const float2 *>(rows.bary + 6 * g);
                    q0[u] = bp[0]; q1[u] = bp[1]; q2[u] = bp[2];  // c1.xyz = q0.x q0.y q1.x ; c2.xyz = q1.y q2.x q2.y
                }
            }
#pragma unroll
            for (int u = 0; u < UM; ++u) {
                const uint32_t j = base + 64 * u + lane;
                if (j >= S) continue;
                float b0 = 0.f, b1 = 0.f, b2 = 0.f;
                if (mk[u]) {
                    const float mult = (cur[u] - t_in[u]) / (t_out[u] - t_in[u]);
                    b0 = (1 - mult) * q0[u].x + mult * q1[u].y;
                    b1 = (1 - mult) * q0[u].y + mult * q2[u].x;
                    b2 = (1 - mult) * q1[u].x + mult * q2[u].y;
                }
                if (FULL) { out.mask[j] = mk[u]; out.cells[j] = cell[u]; }
                *reinterpret_cast<uint4 *>(out.verts + 4 * (size_t)j) = vv[u];
                out.bary[3 * (size_t)j] = b0; out.bary[3 * (size_t)j + 1] = b1; out.bary[3 * (size_t)j + 2] = b2;
            }
        }
    } else {
        // defaults everywhere, then the literal pointer walk on lane 0 (src/tetrahedra_tracer.cu:129-160)
        for (uint32_t j = lane; j < S; j += 64) {
            if (FULL) { out.mask[j] = 0; out.cells[j] = TN_EMPTY; }
            *reinterpret_cast<uint4 *>(out.verts + 4 * (size_t)j) = make_uint4(TN_EMPTY, TN_EMPTY, TN_EMPTY, TN_EMPTY);
            out.bary[3 * (size_t)j] = 0.f; out.bary[3 * (size_t)j + 1] = 0.f; out.bary[3 * (size_t)j + 2] = 0.f;
        }
        wave_global_sync();
        if (lane == 0) {
            uint32_t p = 0;
            for (uint32_t j = 0; j < S; ++j) {
                const float cur = dist_of(j);
                while (p < n && drow[p].y < cur) p++;
                if (p >= n) break;
                const float2 hd = drow[p];
                if (hd.x <= cur) {
                    const size_t g = src * M + p;
                    if (FULL) { out.mask[j] = 1; out.cells[j] = rows.visited[g]; }
                    for (int k = 0; k < 4; ++k) out.verts[4 * (size_t)j + k] = rows.verts[4 * g + k];
                    const float mult = (cur - hd.x) / (hd.y - hd.x);
                    for (int k = 0; k < 3; ++k)
                        out.bary[3 * (size_t)j + k] = (1 - mult) * rows.bary[6 * g + k] + mult * rows.bary[6 * g + 3 + k];
                }
            }
        }
    }
    lds_sync();
}

}  // namespace rayops
}  // namespace tn
