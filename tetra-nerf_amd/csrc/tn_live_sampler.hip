// tn_live_sampler.hip -- the occupancy-guided coarse sampler: samples placed in LIVE tetrahedra only.
//
// The reference declares the per-tetrahedron occupancy field and never uses it (tetranerf/nerfstudio/model.py:98-99,256-265);
// tn_cull_samples skips the network below a threshold, and the samplers before this file still spread their budget over
// [near, far] of the whole mesh.  Here a ray is sampled in its LIVE-LENGTH coordinate s in [near, near + L], L = the summed
// length of its live segments (culled space closed up), and the samples are mapped back to distances inside live segments.
// The PyTorch statements render.live_lengths_statement / live_sample_bins / live_to_distance_statement are the parity
// definition; the kernels evaluate the same expressions per element in the same order, only the prefix sums are wave scans.
//
// One wavefront per HITTING ray (ray_index names its row in the trace outputs, which are read in place):
//   k_sample_live        ray_live_cum -> near_far_live = (near, near + L) + the S + 1 bin edges in the live-length coordinate
//                        (the stratification of ray_sample_coarse_nf, the very function)
//   k_live_to_distance   ray_live_cum (liveness is gathered again: nothing is kept between the two kernels, so the result
//                        cannot depend on which ran first) -> t and segment slot of n values per ray (bin centres, edges, a depth)
#include "tn_ray_ops.h"

namespace tn {

using namespace rayops;

namespace {
constexpr int LB = 256;   // 4 rays per block
}  // namespace

__global__ __launch_bounds__(LB) void k_sample_live(size_t r, uint32_t S, uint32_t M, const uint32_t *__restrict__ ray_index,
                                                    const uint32_t *__restrict__ num_visited, const uint32_t *__restrict__ visited,
                                                    const float *__restrict__ hit_dist, const float *__restrict__ occupancy, uint32_t T,
                                                    float threshold, const float *__restrict__ lin, const float *__restrict__ t_rand,
                                                    float *__restrict__ edges, float *__restrict__ near_far,
                                                    const uint32_t *__restrict__ count) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (count) { const size_t c = *count; r = c < r ? c : r; }   // device-side number of hitting rays (never beyond the launch's bound)
    float *cum = smem + (size_t)wave * (M + 1);
    for (size_t q = (size_t)blockIdx.x * (LB / 64) + wave; q < r; q += (size_t)gridDim.x * (LB / 64)) {
        const size_t ray = ray_index[q];
        const uint32_t nb = num_visited[ray];
        const LiveCum lc = ray_live_cum(M, ray, nb, visited, hit_dist, occupancy, T, threshold, cum, lane);
        const float far = nb ? lc.near + lc.L : 1.0f;
        if (lane == 0) { near_far[2 * q] = lc.near; near_far[2 * q + 1] = far; }
        ray_sample_coarse_nf(S, M, ray, nb, lc.near, far, hit_dist, lin, t_rand ? t_rand + q * (size_t)(S + 1) : nullptr, 0,
                             edges + q * (size_t)(S + 1), nullptr, nullptr, lane);
        lds_sync();      // (the next ray of this wave overwrites cum)
    }
}

__global__ __launch_bounds__(LB) void k_live_to_distance(size_t r, uint32_t n, uint32_t M, const uint32_t *__restrict__ ray_index,
                                                         const uint32_t *__restrict__ num_visited, const uint32_t *__restrict__ visited,
                                                         const float *__restrict__ hit_dist, const float *__restrict__ occupancy,
                                                         uint32_t T, float threshold, const float *__restrict__ values,
                                                         float *__restrict__ t, uint32_t *__restrict__ slot,
                                                         const uint32_t *__restrict__ count) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (count) { const size_t c = *count; r = c < r ? c : r; }
    float *cum = smem + (size_t)wave * (M + 1);
    for (size_t q = (size_t)blockIdx.x * (LB / 64) + wave; q < r; q += (size_t)gridDim.x * (LB / 64)) {
        const size_t ray = ray_index[q];
        const uint32_t nb = num_visited[ray];
        const LiveCum lc = ray_live_cum(M, ray, nb, visited, hit_dist, occupancy, T, threshold, cum, lane);
        ray_live_to_distance(n, M, ray, nb, hit_dist, values + q * (size_t)n, lc, cum, t + q * (size_t)n, slot + q * (size_t)n, lane);
        lds_sync();
    }
}

namespace {
size_t live_lds_bytes(uint32_t M, const char *what) {
    const size_t smem = (size_t)(LB / 64) * ((size_t)M + 1) * sizeof(float);
    if (smem > 64 * 1024) throw Error(std::string(what) + ": max_ray_triangles too large for the live-length sampler");
    return smem;
}
}  // namespace

void launch_sample_live(size_t r, uint32_t S, uint32_t M, const uint32_t *ray_index, const uint32_t *num_visited, const uint32_t *visited,
                        const float *hit_dist, const float *occupancy, uint32_t T, float threshold, const float *lin, const float *t_rand,
                        float *edges, float *near_far, hipStream_t stream, const uint32_t *count) {
    if (r == 0) return;
    const size_t smem = live_lds_bytes(M, "sample_live");
    const size_t blocks = (r + LB / 64 - 1) / (LB / 64);
    hipLaunchKernelGGL(k_sample_live, dim3((unsigned)(blocks < 256 * 16 ? blocks : 256 * 16)), dim3(LB), smem, stream, r, S, M, ray_index,
                       num_visited, visited, hit_dist, occupancy, T, threshold, lin, t_rand, edges, near_far, count);
}

void launch_live_to_distance(size_t r, uint32_t n, uint32_t M, const uint32_t *ray_index, const uint32_t *num_visited,
                             const uint32_t *visited, const float *hit_dist, const float *occupancy, uint32_t T, float threshold,
                             const float *values, float *t, uint32_t *slot, hipStream_t stream, const uint32_t *count) {
    if (r == 0 || n == 0) return;
    const size_t smem = live_lds_bytes(M, "live_to_distance");
    const size_t blocks = (r + LB / 64 - 1) / (LB / 64);
    hipLaunchKernelGGL(k_live_to_distance, dim3((unsigned)(blocks < 256 * 16 ? blocks : 256 * 16)), dim3(LB), smem, stream, r, n, M,
                       ray_index, num_visited, visited, hit_dist, occupancy, T, threshold, values, t, slot, count);
}

}  // namespace tn
