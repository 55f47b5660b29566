// tn_mlp_dw_body.inc -- the body of the fp32 weight-gradient GEMM kernel (tn_mlp_grad.hip: k_dw_gemm, where the product, the
// staging and the slot layout are described), included as text INSIDE the kernel definitions: k_dw_gemm and the indexed
// head-layer GEMM of occupancy-culled training (tn_occupancy_dw.hip) are one source, and k_dw_gemm keeps the code it had as a
// plain kernel (as a shared device function it came out with another instruction order).  The including kernel provides
//   template parameters / constants  int NBM, bool EXTRA, bool INDEXED
//   arguments                        g (A, B, enc, dh, spr, part), size_t n, uint32_t slice,
//                                    INDEXED: const uint32_t *live, uint32_t num_rays
// INDEXED (with EXTRA): the streamed axis counts the SLOTS of an ascending list, slot i stands for sample live[i]; only the row
// of the direction encoding depends on it -- ray = live[slot] / spr (clamped below num_rays), re-read when it changes.
    constexpr int LD = 36;                // LDS row stride (floats): 16-byte aligned, LD / 4 odd -> conflict-free b128 reads
    constexpr int NB = NBM + (EXTRA ? 1 : 0);
    constexpr int RA = 128, RBM = 32 * NBM, RB = 32 * NB;
    __shared__ __attribute__((aligned(16))) float As[RA * LD];
    __shared__ __attribute__((aligned(16))) float Bs[RB * LD];
    __shared__ __attribute__((aligned(16))) float dhs[32];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col = tid & 31, row0 = tid >> 5;            // staging: sample of the step, quad (4 feature rows) within a pass of 8
    const int cpos = (col & 1) * 16 + (col >> 1);         // even samples first, then the odd ones
    const size_t s_begin = (size_t)blockIdx.x * slice;
    const size_t s_end = s_begin + slice < n ? s_begin + slice : n;
    float *part = g.part + (size_t)blockIdx.x * (RA * RB + 256);
    constexpr int QA = RA / 32, QBM = RBM / 32;           // quads per thread: the tiles are [F / 4][n][4] (tn_mlp_common.h)

    f32x16 acc[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    float rsum = 0.f, dv = 0.f;
    if (s_begin < n) {
        float4 ra[QA], rb[QBM];
        float re[EXTRA ? 4 : 1] = {}, rdh = 0.f;
        uint32_t e_ray = 0, e_rem = 0;   // EXTRA: ray of this thread's sample, offset of the sample within it
        const float4 *A4 = reinterpret_cast<const float4 *>(g.A), *B4 = reinterpret_cast<const float4 *>(g.B);
        auto fetch = [&](size_t s0) {
            const size_t sidx = s0 + col;
            const bool in = sidx < s_end;
            const size_t sc = in ? sidx : s_end - 1;      // clamped: loads stay unconditional, A (and dh) are zeroed
#pragma unroll
            for (int p = 0; p < QA; ++p) ra[p] = A4[(size_t)(8 * p + row0) * n + sc];
#pragma unroll
            for (int p = 0; p < QBM; ++p) rb[p] = B4[(size_t)(8 * p + row0) * n + sc];
            if constexpr (EXTRA) {
                // the encoding of the sample's ray: a thread's sample advances by 32 per step, so its ray changes every
                // spr / 32 steps -- the four values stay in registers and are re-read only then (per step: one division and
                // four gathers less; 0.87 -> 0.7x ms per 2.1 M samples, profiles/r04r_dw_ablate.txt).  Lanes beyond the
                // slice keep what they have (their A rows are zero).
                bool reload = false;
                if constexpr (INDEXED) {
                    // the list is ascending: the ray of a thread's slot changes as rarely as that of its sample does
                    if (in || s0 == s_begin) {
                        uint32_t ray = live[sc] / g.spr;
                        ray = ray < num_rays ? ray : num_rays - 1;
                        reload = s0 == s_begin || ray != e_ray;
                        e_ray = ray;
                    }
                } else if (s0 == s_begin) {
                    e_ray = (uint32_t)sc / g.spr;                 // n < 2^32 (checked by the launcher)
                    e_rem = (uint32_t)sc - e_ray * g.spr;
                    reload = true;
                } else if (in) {
                    e_rem += 32u;
                    while (e_rem >= g.spr) { e_rem -= g.spr; ++e_ray; reload = true; }
                }
                if (reload) {
                    const float *e = g.enc + (size_t)e_ray * ENC_PAD;
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int j = 8 * p + row0;
                        re[p] = j < ENC_PAD ? e[j < ENC_PAD ? j : 0] : 0.f;
                    }
                }
                rdh = row0 == 0 ? g.dh[sc] : 0.f;
                if (!in) rdh = 0.f;
            }
            if (!in) {
#pragma unroll
                for (int p = 0; p < QA; ++p) ra[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        auto put4 = [&](float *tile, int quad, const float4 &v) {
            float *q = tile + (4 * quad) * LD + cpos;
            q[0] = v.x; q[LD] = v.y; q[2 * LD] = v.z; q[3 * LD] = v.w;
        };
        fetch(s_begin);
        const int m = lane & 31, kk = lane >> 5;
        const float4 *arow = reinterpret_cast<const float4 *>(As + (32 * w + m) * LD + kk * 16);
        const float4 *brow = reinterpret_cast<const float4 *>(Bs + m * LD + kk * 16);
        const int vf = tid >> 1, vh = tid & 1;             // d wd: feature row, sample parity
        for (size_t s0 = s_begin; s0 < s_end; s0 += 32) {
            __syncthreads();   // the previous step's reads of the tiles are done
#pragma unroll
            for (int p = 0; p < QA; ++p) put4(As, 8 * p + row0, ra[p]);
#pragma unroll
            for (int p = 0; p < QBM; ++p) put4(Bs, 8 * p + row0, rb[p]);
            if constexpr (EXTRA) {
#pragma unroll
                for (int p = 0; p < 4; ++p) Bs[(RBM + 8 * p + row0) * LD + cpos] = re[p];
                if (row0 == 0) dhs[cpos] = rdh;
            }
            __syncthreads();
            if (s0 + 32 < s_end) fetch(s0 + 32);
            float4 a4[4], b4[2][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a4[q] = arow[q];
#pragma unroll
            for (int q = 0; q < 4; ++q) b4[0][q] = brow[q];
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                if (c + 1 < NB) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) b4[(c + 1) & 1][q] = brow[(c + 1) * 32 * LD / 4 + q];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 a = a4[q], b = b4[c & 1][q];
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[c], 0, 0, 0);
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[c], 0, 0, 0);
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[c], 0, 0, 0);
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[c], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) rsum += (a4[q].x + a4[q].y) + (a4[q].z + a4[q].w);
            if (EXTRA) {
                const float4 *hr = reinterpret_cast<const float4 *>(Bs + vf * LD + vh * 16);
                const float4 *dr = reinterpret_cast<const float4 *>(dhs + vh * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 x = hr[q], d = dr[q];
                    dv += (x.x * d.x + x.y * d.y) + (x.z * d.z + x.w * d.w);
                }
            }
        }
    }
    // partial sums of this block (zeros when the block had no samples: the reduction adds every slot)
    const int hh = lane >> 5;
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            part[(size_t)(32 * w + acc_feature(r, hh)) * RB + 32 * c + (lane & 31)] = acc[c][r];
    rsum += __shfl_xor(rsum, 32);
    if (lane < 32) part[RA * RB + 32 * w + lane] = rsum;
    if (EXTRA) {
        dv += __shfl_xor(dv, 1);
        if ((tid & 1) == 0) part[RA * RB + 128 + (tid >> 1)] = dv;
    } else if (tid < 128) {
        part[RA * RB + 128 + tid] = 0.f;
    }
