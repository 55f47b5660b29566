// tn_tet_stats.hip -- tn_tet_stats_accumulate: per-tetrahedron training statistics (sample hits, composite weight, weight x
// per-ray error) as 64-bit fixed-point sums, the signal a densification policy selects by (the rule: tn_tet_stats_core.h,
// DESIGN.md section 4.19; the statement in numpy: render.tet_stats_statement).
//
//   k_tet_stats   ONE wavefront per row (a block is one wave, as k_composite), grid-stride over the rows on at most
//                 TS_MAX_GRID blocks.  The wave calls rayops::ray_composite with rgb = nullptr and out_w = its own LDS: the
//                 weights are the composite's bits by construction and no [R, S] weights array goes through memory.  Then per
//                 chunk of 64 samples: lane j takes cells[j], its weight from LDS and forms the three integer terms; runs of
//                 equal cells (a tetrahedron's samples are consecutive on a ray) are folded into their first lane by a segmented
//                 sum over shuffles, bounded by the distance to the next run head -- so the fold is exact for ANY sequence of
//                 cells, also A B A; the last run of a chunk is carried into the next chunk instead of being written, and only run
//                 heads issue the three 64-bit integer atomic adds.
// The sums are integers: order of samples, folding and order of the atomics cannot change a byte of the result.
// Every store is an atomic on stats[3 c + k] with c < T checked (tetstats::accept); reads of cells / sigma / edges stay inside
// rows < min(num_rows, *count).  ray_index[q] must be a valid index of ray_value: that is the caller's (tn_compact_hits gives it).
// Plain C++ HIP: no inline assembly.
#include "tn_api_common.h"
#include "tn_ray_ops.h"
#include "tn_tet_stats_core.h"

namespace tn {

using namespace rayops;

namespace {

constexpr unsigned TS_MAX_GRID = 256u * 32u;   // k_composite's cap: from there on a wave strides over rows
constexpr uint32_t TS_MAX_S = 8192;            // samples per row: 32 KiB of LDS for the wave's weights

typedef unsigned long long u64;

__device__ __forceinline__ void add_run(u64 *__restrict__ stats, uint32_t c, uint32_t h, u64 w, u64 e) {
    u64 *row = stats + 3 * (size_t)c;
    atomicAdd(row, (u64)h);
    atomicAdd(row + 1, w);
    atomicAdd(row + 2, e);
}

__global__ __launch_bounds__(64) void k_tet_stats(uint32_t T, size_t R, uint32_t S, const uint32_t *__restrict__ cells,
                                                  const float *__restrict__ sigma, const float *__restrict__ edges,
                                                  const float *__restrict__ ray_value, const uint32_t *__restrict__ ray_index,
                                                  const uint32_t *__restrict__ count, u64 *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *wl = reinterpret_cast<float *>(smem);   // S floats: this row's weights
    const int lane = threadIdx.x;
    if (count) {
        const size_t live = *count;                // (the padded duplicates from *count on would be counted twice)
        R = live < R ? live : R;
    }
    const Background none = {0.f, 0.f, 0.f, 0};
    for (size_t q = blockIdx.x; q < R; q += gridDim.x) {
        ray_composite(S, sigma + q * S, nullptr, edges + q * ((size_t)S + 1), none, nullptr, nullptr, nullptr, wl, lane);
        lds_sync();
        const float v = ray_value ? ray_value[ray_index ? (size_t)ray_index[q] : q] : 1.0f;
        const uint32_t *crow = cells + q * S;
        // the open run of the chunks before (wave-uniform)
        uint32_t cc = TN_EMPTY, ch = 0;
        u64 cw = 0, ce = 0;
        for (uint32_t base = 0; base < S; base += 64) {
            const uint32_t j = base + lane;
            uint32_t c = TN_EMPTY, h = 0;
            u64 w = 0, e = 0;
            if (j < S) {
                const uint32_t ci = crow[j];
                if (tetstats::accept(ci, T)) {
                    const float wj = wl[j];
                    c = ci;
                    h = 1;
                    w = (u64)tetstats::weight_term(wj);
                    e = (u64)tetstats::error_term(wj, v);
                }
            }
            // run heads and, per lane, the number of lanes up to the next head: the fold never leaves a run
            const uint32_t pc = (uint32_t)__shfl_up((int)c, 1);
            const bool head = lane == 0 || pc != c;
            const u64 heads = __ballot(head);
            const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
            const int len = above ? __ffsll(above) : 64 - lane;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t oh = (uint32_t)__shfl_down((int)h, off);
                const u64 ow = __shfl_down(w, off);
                const u64 oe = __shfl_down(e, off);
                if (off < len) { h += oh; w += ow; e += oe; }
            }
            // the carried run continues in lane 0's, or ends here
            if (cc != TN_EMPTY && lane == 0) {
                if (c == cc) { h += ch; w += cw; e += ce; }
                else add_run(stats, cc, ch, cw, ce);
            }
            const int last = 63 - __clzll(heads);   // (bit 0 is always set)
            cc = (uint32_t)__shfl((int)c, last);
            ch = (uint32_t)__shfl((int)h, last);
            cw = __shfl(w, last);
            ce = __shfl(e, last);
            if (head && lane != last && c != TN_EMPTY) add_run(stats, c, h, w, e);
        }
        if (cc != TN_EMPTY && lane == 0) add_run(stats, cc, ch, cw, ce);
        lds_sync();   // (the next row's composite overwrites wl)
    }
}

}  // namespace

void launch_tet_stats(uint32_t T, size_t R, uint32_t S, const uint32_t *cells, const float *sigma, const float *edges,
                      const float *ray_value, const uint32_t *ray_index, const uint32_t *count, int64_t *stats, hipStream_t stream) {
    if (T == 0 || R == 0) return;
    const unsigned grid = (unsigned)(R < TS_MAX_GRID ? R : TS_MAX_GRID);
    hipLaunchKernelGGL(k_tet_stats, dim3(grid), dim3(64), (size_t)S * sizeof(float), stream, T, R, S, cells, sigma, edges, ray_value,
                       ray_index, count, reinterpret_cast<u64 *>(stats));
}

}  // namespace tn

extern "C" {

int tn_tet_stats_accumulate(uint32_t num_cells, size_t num_rows, uint32_t samples_per_ray, const uint32_t *cells, const float *sigma,
                            const float *edges, const float *ray_value, const uint32_t *ray_index, const uint32_t *count,
                            int64_t *stats, void *stream_) {
    return tn::guarded([&] {
        if (num_cells == 0 || num_rows == 0) return;
        if (samples_per_ray == 0) throw tn::Error("tet_stats_accumulate: samples_per_ray must be positive");
        if (samples_per_ray > tn::TS_MAX_S)
            throw tn::Error("tet_stats_accumulate: more than 8192 samples per ray are not supported (the wave keeps a row's weights in LDS)");
        if (num_rows >= 0xFFFFFFFFull) throw tn::Error("tet_stats_accumulate: too many rows for one call");
        if (!cells || !sigma || !edges || !stats) throw tn::Error("tet_stats_accumulate: null pointer");
        tn::launch_tet_stats(num_cells, num_rows, samples_per_ray, cells, sigma, edges, ray_value, ray_index, count, stats,
                             (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

}  // extern "C"
