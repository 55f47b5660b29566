// tn_mlp_x3_dw_body.inc -- the body of the bf16x3 weight-gradient GEMM kernel (tn_mlp_x3_dw.hip: k_dw_gemm_x3, where the fetch, the
// split, the LDS rows and the MFMA order are described), included as text INSIDE the kernel definitions, as tn_mlp_dw_body.inc
// is: one source for k_dw_gemm_x3 and the indexed head-layer GEMM of tn_occupancy_dw.hip.  The including kernel provides
// int NBM, bool EXTRA, bool INDEXED; DwGemmArgs g, size_t n, uint32_t slice; INDEXED: const uint32_t *live, uint32_t num_rays.
    constexpr int ROWB = 208;             // LDS row stride in bytes: three pieces of 64 bytes + 16 (13 slots of 16 bytes: odd)
    constexpr int ROWU = ROWB / 16, ROWW = ROWB / 4;
    constexpr int ENC_PAD = mlp::ENC_PAD;
    constexpr int NB = NBM + (EXTRA ? 1 : 0);
    constexpr int RA = 128, RBM = 32 * NBM, RB = 32 * NB;
    constexpr int PA = RA / 64, PB = RBM / 64;              // passes of 16 quads
    __shared__ __attribute__((aligned(16))) uint32_t As[RA * ROWW];
    __shared__ __attribute__((aligned(16))) uint32_t Bs[RB * ROWW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int pr = tid & 15, row0 = tid >> 4;               // staging: sample pair of the step, quad within a pass of 16
    const size_t s_begin = (size_t)blockIdx.x * slice;
    const size_t s_end = s_begin + slice < n ? s_begin + slice : n;
    float *part = g.part + (size_t)blockIdx.x * (RA * RB + 256);

    f32x16 acc[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    float rs[PA][4] = {}, dv[PB][4] = {};                   // row sums of A, (EXTRA) the d wd vector: this thread's two samples
    if (s_begin < n) {
        float4 ra[PA][2], rb[PB][2];
        float re[EXTRA ? 2 : 1][2] = {}, rdh[2] = {0.f, 0.f};
        uint32_t e_ray[2] = {0, 0}, e_rem[2] = {0, 0};      // EXTRA: ray of each of the two samples, offset of the sample within it
        const float4 *A4 = reinterpret_cast<const float4 *>(g.A), *B4 = reinterpret_cast<const float4 *>(g.B);
        auto fetch = [&](size_t s0) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const size_t sidx = s0 + 2 * pr + u;
                const bool in = sidx < s_end;
                const size_t sc = in ? sidx : s_end - 1;    // clamped: loads stay unconditional, A (and dh) are zeroed
#pragma unroll
                for (int p = 0; p < PA; ++p) ra[p][u] = A4[(size_t)(16 * p + row0) * n + sc];
#pragma unroll
                for (int p = 0; p < PB; ++p) rb[p][u] = B4[(size_t)(16 * p + row0) * n + sc];
                if constexpr (EXTRA) {
                    // the encoding of the sample's ray, kept in registers and re-read only when the ray changes (k_dw_gemm)
                    bool reload = false;
                    if constexpr (INDEXED) {
                        if (in || s0 == s_begin) {
                            uint32_t ray = live[sc] / g.spr;
                            ray = ray < num_rays ? ray : num_rays - 1;
                            reload = s0 == s_begin || ray != e_ray[u];
                            e_ray[u] = ray;
                        }
                    } else if (s0 == s_begin) {
                        e_ray[u] = (uint32_t)sc / g.spr;          // n < 2^32 (checked by the launcher)
                        e_rem[u] = (uint32_t)sc - e_ray[u] * g.spr;
                        reload = true;
                    } else if (in) {
                        e_rem[u] += 32u;
                        while (e_rem[u] >= g.spr) { e_rem[u] -= g.spr; ++e_ray[u]; reload = true; }
                    }
                    if (reload) {
                        const float *e = g.enc + (size_t)e_ray[u] * ENC_PAD;
#pragma unroll
                        for (int p = 0; p < 2; ++p) {
                            const int j = 16 * p + row0;
                            re[p][u] = j < ENC_PAD ? e[j < ENC_PAD ? j : 0] : 0.f;
                        }
                    }
                    rdh[u] = in ? g.dh[sc] : 0.f;
                }
                if (!in) {
#pragma unroll
                    for (int p = 0; p < PA; ++p) ra[p][u] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        };
        // the four feature rows of a quad x this thread's two samples -> three pieces -> LDS
        auto put = [&](uint32_t *tile, int quad, const float4 &x, const float4 &y) {
            const float v[8] = {x.x, y.x, x.y, y.y, x.z, y.z, x.w, y.w};
            uint4 hi, mid, lo;
            split8(v, hi, mid, lo);
            uint32_t *q = tile + (4 * quad) * ROWW + pr;
            q[0] = hi.x; q[16] = mid.x; q[32] = lo.x;
            q[ROWW] = hi.y; q[ROWW + 16] = mid.y; q[ROWW + 32] = lo.y;
            q[2 * ROWW] = hi.z; q[2 * ROWW + 16] = mid.z; q[2 * ROWW + 32] = lo.z;
            q[3 * ROWW] = hi.w; q[3 * ROWW + 16] = mid.w; q[3 * ROWW + 32] = lo.w;
        };
        fetch(s_begin);
        const int m = lane & 31, kk = lane >> 5;
        // slot (piece P, K-step q) of a row: P * 4 + 2 q + kk
        const uint4 *arow = reinterpret_cast<const uint4 *>(As) + (32 * w + m) * ROWU + kk;
        const uint4 *brow = reinterpret_cast<const uint4 *>(Bs) + m * ROWU + kk;
        for (size_t s0 = s_begin; s0 < s_end; s0 += 32) {
            __syncthreads();   // the previous step's reads of the tiles are done
#pragma unroll
            for (int p = 0; p < PA; ++p) {
                put(As, 16 * p + row0, ra[p][0], ra[p][1]);
                const float4 x = ra[p][0], y = ra[p][1];
                rs[p][0] += x.x + y.x; rs[p][1] += x.y + y.y; rs[p][2] += x.z + y.z; rs[p][3] += x.w + y.w;
            }
#pragma unroll
            for (int p = 0; p < PB; ++p) {
                put(Bs, 16 * p + row0, rb[p][0], rb[p][1]);
                if constexpr (EXTRA) {
                    const float4 x = rb[p][0], y = rb[p][1];
                    dv[p][0] += x.x * rdh[0] + y.x * rdh[1]; dv[p][1] += x.y * rdh[0] + y.y * rdh[1];
                    dv[p][2] += x.z * rdh[0] + y.z * rdh[1]; dv[p][3] += x.w * rdh[0] + y.w * rdh[1];
                }
            }
            if constexpr (EXTRA) {
                // rows RBM + row0 and RBM + 16 + row0 of the encoding tile; the other two pairs of the split are zeros
                const float v[8] = {re[0][0], re[0][1], re[1][0], re[1][1], 0.f, 0.f, 0.f, 0.f};
                uint4 hi, mid, lo;
                split8(v, hi, mid, lo);
                uint32_t *q = Bs + (RBM + row0) * ROWW + pr;
                q[0] = hi.x; q[16] = mid.x; q[32] = lo.x;
                q[16 * ROWW] = hi.y; q[16 * ROWW + 16] = mid.y; q[16 * ROWW + 32] = lo.y;
            }
            __syncthreads();
            if (s0 + 32 < s_end) fetch(s0 + 32);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const uint4 ah = arow[2 * q], am = arow[4 + 2 * q], al = arow[8 + 2 * q];
#pragma unroll
                for (int c = 0; c + 1 < NB; c += 2) {
                    const uint4 *b0 = brow + c * 32 * ROWU + 2 * q, *b1 = b0 + 32 * ROWU;
                    const uint4 bh0 = b0[0], bm0 = b0[4], bl0 = b0[8];
                    const uint4 bh1 = b1[0], bm1 = b1[4], bl1 = b1[8];
                    acc[c] = mma(al, bh0, acc[c]);     acc[c + 1] = mma(al, bh1, acc[c + 1]);
                    acc[c] = mma(ah, bl0, acc[c]);     acc[c + 1] = mma(ah, bl1, acc[c + 1]);
                    acc[c] = mma(am, bm0, acc[c]);     acc[c + 1] = mma(am, bm1, acc[c + 1]);
                    acc[c] = mma(am, bh0, acc[c]);     acc[c + 1] = mma(am, bh1, acc[c + 1]);
                    acc[c] = mma(ah, bm0, acc[c]);     acc[c + 1] = mma(ah, bm1, acc[c + 1]);
                    acc[c] = mma(ah, bh0, acc[c]);     acc[c + 1] = mma(ah, bh1, acc[c + 1]);
                }
                if constexpr (NB & 1) {
                    constexpr int c = NB - 1;
                    const uint4 *b0 = brow + c * 32 * ROWU + 2 * q;
                    const uint4 bh0 = b0[0], bm0 = b0[4], bl0 = b0[8];
                    acc[c] = mma(al, bh0, acc[c]);
                    acc[c] = mma(ah, bl0, acc[c]);
                    acc[c] = mma(am, bm0, acc[c]);
                    acc[c] = mma(am, bh0, acc[c]);
                    acc[c] = mma(ah, bm0, acc[c]);
                    acc[c] = mma(ah, bh0, acc[c]);
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
    // the 16 sample pairs of a quad are 16 consecutive lanes
#pragma unroll
    for (int p = 0; p < PA; ++p)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            float v = rs[p][f];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
            if (pr == 0) part[RA * RB + 4 * (16 * p + row0) + f] = v;
        }
    if constexpr (EXTRA) {
        static_assert(RBM == 128, "the d wd vector has one entry per row of h3");
#pragma unroll
        for (int p = 0; p < PB; ++p)
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                float v = dv[p][f];
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
                if (pr == 0) part[RA * RB + 128 + 4 * (16 * p + row0) + f] = v;
            }
    } else if (tid < 128) {
        part[RA * RB + 128 + tid] = 0.f;
    }
