// tn_occupancy.hip -- the per-tetrahedron occupancy field: the reference registers a `tetrahedra_occupancy` buffer (f32
// [num_cells], tetranerf/nerfstudio/model.py:98-99,256-265) and never reads or writes it.  Three kernels finish it:
//   update   occupancy[t] = max(decay * occupancy[t], max of the densities of the samples matched to t)   (tn_occupancy_update)
//   cull     the samples whose tetrahedron is below a threshold get sigma = rgb = 0 and leave the list of samples the network
//            still has to run on: a stable compaction, ascending                                         (tn_cull_samples)
//   forward  tn_mlp_forward_gather over the listed samples only (fp32 and bf16x3)                     (tn_mlp_forward_gather_indexed)
// A sample's result depends on nothing but its own column in both arithmetics (tn_mlp.hip: one lane column per sample, the
// weights shared), so the indexed forward runs mlp_forward_group / x3::forward_group with the lane's sample index taken from the
// list: the same instruction stream on the same operands, bit for bit the unculled kernel's result at every listed sample.
#include "tn_mlp_fwd.h"
#include "tn_mlp_x3_fwd.h"

namespace tn {

namespace {

constexpr int OC_BLOCK = 256;            // update kernels: one sample / tetrahedron per thread and grid stride
constexpr unsigned OC_MAX_GRID = 2048;   // 8 blocks per CU: from 256 * 2048 elements on a thread strides

// ---- update ---------------------------------------------------------------------------------------------------------------

// every tetrahedron decays on every update.  A NaN stays a NaN and is stored with the sign bit clear, so that it also outlives
// the integer maximum below (like torch.maximum, which propagates it).
__global__ __launch_bounds__(OC_BLOCK) void k_occupancy_decay(uint32_t T, float decay, float *__restrict__ occupancy) {
    for (size_t t = (size_t)blockIdx.x * OC_BLOCK + threadIdx.x; t < T; t += (size_t)gridDim.x * OC_BLOCK) {
        const float v = decay * occupancy[t];
        occupancy[t] = v != v ? __uint_as_float(0x7FC00000u) : v;
    }
}

// scatter-max of the accepted samples (cell < T, sigma >= 0: no NaN, no negative value): the bit pattern of a float >= +0 orders
// as a signed integer like the float, is above that of every negative float and below that of a NaN with a clear sign bit, so
// ONE signed integer atomic per sample is the float maximum -- associative and commutative: the result does not depend on the
// order of the samples or of the atomics.  Consecutive samples of a ray mostly sit in the same tetrahedron: a wave first folds
// each run of equal cells into its first lane (segmented maximum by shuffles; folding any two lanes of one cell is valid), and
// only run heads reach memory.
__global__ __launch_bounds__(OC_BLOCK) void k_occupancy_scatter_max(uint32_t T, size_t n, const uint32_t *__restrict__ cells,
                                                                    const float *__restrict__ sigma, int *__restrict__ occupancy,
                                                                    uint32_t samples_per_ray, const uint32_t *__restrict__ count) {
    if (count) {
        const size_t live = (size_t)*count * samples_per_ray;
        n = live < n ? live : n;
    }
    const int lane = threadIdx.x & 63;
    // (whole waves iterate together: the shuffles below need every lane)
    for (size_t base = ((size_t)blockIdx.x * OC_BLOCK + (threadIdx.x & ~63u)); base < n; base += (size_t)gridDim.x * OC_BLOCK) {
        const size_t i = base + lane;
        uint32_t c = TN_EMPTY;
        int v = 0;
        if (i < n) {
            const uint32_t ci = cells[i];
            const float s = sigma[i];
            if (ci < T && s >= 0.0f) {
                c = ci;
                v = (int)(__float_as_uint(s) & 0x7FFFFFFFu);   // (-0 is accepted and counts as +0)
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t oc = (uint32_t)__shfl_down((int)c, off);
            const int ov = __shfl_down(v, off);
            if (lane + off < 64 && oc == c) v = ov > v ? ov : v;
        }
        const uint32_t pc = (uint32_t)__shfl_up((int)c, 1);
        if (c != TN_EMPTY && (lane == 0 || pc != c)) atomicMax(occupancy + c, v);
    }
}

// ---- cull -----------------------------------------------------------------------------------------------------------------

// A wave owns a TILE of 1024 consecutive samples, 16 steps of 64: the rank of a live sample inside a step is the number of set
// ballot bits below its lane, inside the tile the sum of the steps before -- ascending order costs nothing.  Three launches, as
// tn_compact_hits' two levels plus one: (1) live samples per tile -> scratch, (2) one block turns the tile counts into their
// exclusive prefix sums in place and leaves the total in scratch[tiles] and *live_count, (3) every wave writes its tile from
// its offset.  scratch: cull_scratch_u32(n) uint32.
constexpr int CU_BLOCK = 256, CU_STEPS = 16, CU_TILE = 64 * CU_STEPS, CU_SCAN = 1024;

// is sample i live?  culled = a valid tetrahedron id whose occupancy is below the threshold; unmatched samples (0xFFFFFFFF), ids
// >= T and a NaN occupancy (the comparison fails) are live; threshold <= 0 (or NaN) culls nothing
__device__ __forceinline__ bool sample_live(size_t i, const uint32_t *__restrict__ cells, const float *__restrict__ occupancy,
                                            uint32_t T, float threshold) {
    const uint32_t c = cells[i];
    return !(threshold > 0.0f && c < T && occupancy[c] < threshold);
}

__device__ __forceinline__ size_t counted_samples(size_t n, uint32_t samples_per_ray, const uint32_t *__restrict__ count) {
    if (!count) return n;
    const size_t live = (size_t)*count * samples_per_ray;
    return live < n ? live : n;
}

__global__ __launch_bounds__(CU_BLOCK) void k_cull_count(size_t n, uint32_t samples_per_ray, const uint32_t *__restrict__ cells,
                                                         const float *__restrict__ occupancy, uint32_t T, float threshold,
                                                         uint32_t *__restrict__ tile_live, size_t tiles,
                                                         const uint32_t *__restrict__ count) {
    n = counted_samples(n, samples_per_ray, count);
    const int lane = threadIdx.x & 63;
    const size_t tile = (size_t)blockIdx.x * (CU_BLOCK / 64) + (threadIdx.x >> 6);
    if (tile >= tiles) return;
    uint32_t c = 0;
#pragma unroll 4
    for (int st = 0; st < CU_STEPS; ++st) {
        const size_t i = tile * CU_TILE + (size_t)st * 64 + lane;
        const bool live = i < n && sample_live(i, cells, occupancy, T, threshold);
        c += (uint32_t)__popcll(__ballot(live));
    }
    if (lane == 0) tile_live[tile] = c;
}

// one block: tile_live[0 .. tiles) -> exclusive prefix sums in place, the total -> tile_live[tiles] and *live_count
__global__ __launch_bounds__(CU_SCAN) void k_cull_scan(uint32_t *__restrict__ tile_live, size_t tiles, uint32_t *__restrict__ live_count) {
    __shared__ uint32_t sm[CU_SCAN / 64];
    __shared__ uint32_t carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (size_t base = 0; base < tiles; base += CU_SCAN) {
        const size_t i = base + threadIdx.x;
        const uint32_t v = i < tiles ? tile_live[i] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, off);
            if (lane >= off) inc += o;
        }
        if (lane == 63) sm[wave] = inc;
        __syncthreads();
        uint32_t before = carry_s, tot = 0;
#pragma unroll
        for (int w = 0; w < CU_SCAN / 64; ++w) {
            const uint32_t x = sm[w];
            before += w < wave ? x : 0u;
            tot += x;
        }
        if (i < tiles) tile_live[i] = before + inc - v;
        __syncthreads();                      // (everyone has read sm and carry_s)
        if (threadIdx.x == 0) carry_s += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) { tile_live[tiles] = carry_s; *live_count = carry_s; }
}

__global__ __launch_bounds__(CU_BLOCK) void k_cull_write(size_t n, uint32_t samples_per_ray, const uint32_t *__restrict__ cells,
                                                         const float *__restrict__ occupancy, uint32_t T, float threshold,
                                                         const uint32_t *__restrict__ tile_offset, size_t tiles,
                                                         uint32_t *__restrict__ live_out, float *__restrict__ sigma,
                                                         float *__restrict__ rgb, const uint32_t *__restrict__ count) {
    n = counted_samples(n, samples_per_ray, count);
    const int lane = threadIdx.x & 63;
    const size_t tile = (size_t)blockIdx.x * (CU_BLOCK / 64) + (threadIdx.x >> 6);
    if (tile >= tiles) return;
    uint32_t pos = tile_offset[tile];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int st = 0; st < CU_STEPS; ++st) {
        const size_t i = tile * CU_TILE + (size_t)st * 64 + lane;
        if (tile * CU_TILE + (size_t)st * 64 >= n) break;   // (wave-uniform)
        const bool in = i < n;
        const bool live = in && sample_live(i, cells, occupancy, T, threshold);
        const unsigned long long m = __ballot(live);
        if (live) live_out[pos + (uint32_t)__popcll(m & below)] = (uint32_t)i;
        else if (in) {
            sigma[i] = 0.f;
            if (rgb) { rgb[3 * i] = 0.f; rgb[3 * i + 1] = 0.f; rgb[3 * i + 2] = 0.f; }
        }
        pos += (uint32_t)__popcll(m);
    }
}

// ---- indexed forward --------------------------------------------------------------------------------------------------------

// slot i of the launch computes sample live[i], i < *live_count (<= n_max, which sizes the grid); the sample bound of the
// gathers and stores is n_max, or *count rays when the ray count lives on the device too
__device__ __forceinline__ void indexed_bounds(size_t n_max, uint32_t samples_per_ray, const uint32_t *__restrict__ live_count,
                                               const uint32_t *__restrict__ count, size_t &n_live, size_t &n_samples) {
    n_samples = counted_samples(n_max, samples_per_ray, count);
    const size_t l = *live_count;
    n_live = n_samples == 0 ? 0 : (l < n_max ? l : n_max);
}

template <bool DENSITY_ONLY>
__global__ __launch_bounds__(mlp::MLP_BLOCK, 2) void k_mlp_forward_indexed(
    size_t n_max, uint32_t samples_per_ray, const uint32_t *__restrict__ live, const uint32_t *__restrict__ live_count,
    const uint32_t *__restrict__ vi, const float *__restrict__ bc, const float *__restrict__ fieldT, const float *__restrict__ hterm,
    const float *__restrict__ pk, float *__restrict__ sigma, float *__restrict__ rgb, const uint32_t *__restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *lds = reinterpret_cast<float *>(smem);
    size_t n, n_samples;
    indexed_bounds(n_max, samples_per_ray, live_count, count, n, n_samples);
    constexpr size_t GROUP = (mlp::MLP_BLOCK / 64) * 32;
    const size_t ngroups = (n + GROUP - 1) / GROUP;
    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        mlp::mlp_forward_group<true, DENSITY_ONLY, mlp::MLP_BLOCK, false, true>(lds, g, n, samples_per_ray, nullptr, vi, bc, fieldT, hterm, pk,
                                                                                sigma, rgb, mlp::FwdSave{}, nullptr, live, n_samples);
}

template <bool DENSITY_ONLY>
__global__ __launch_bounds__(x3::X3_BLOCK) void k_mlp_forward_x3_indexed(
    size_t n_max, uint32_t samples_per_ray, const uint32_t *__restrict__ live, const uint32_t *__restrict__ live_count,
    const uint32_t *__restrict__ vi, const float *__restrict__ bc, const float *__restrict__ fieldT, const float *__restrict__ enc,
    const uint4 *__restrict__ blob, float *__restrict__ sigma, float *__restrict__ rgb, const float *__restrict__ ray_bias,
    const uint32_t *__restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint4 *lds = reinterpret_cast<uint4 *>(smem);
    size_t n, n_samples;
    indexed_bounds(n_max, samples_per_ray, live_count, count, n, n_samples);
    constexpr size_t GROUP = (x3::X3_BLOCK / 64) * 32;
    const size_t ngroups = (n + GROUP - 1) / GROUP;
    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x)
        x3::forward_group<true, DENSITY_ONLY, false, true>(lds, g, n, samples_per_ray, nullptr, vi, bc, fieldT, enc, blob, sigma, rgb, ray_bias,
                                                           nullptr, live, n_samples);
}

}  // namespace

void launch_occupancy_update(uint32_t T, size_t n, const uint32_t *cells, const float *sigma, float decay, float *occupancy,
                             uint32_t samples_per_ray, const uint32_t *count, hipStream_t stream) {
    if (T == 0) return;
    const size_t tb = ((size_t)T + OC_BLOCK - 1) / OC_BLOCK;
    hipLaunchKernelGGL(k_occupancy_decay, dim3((unsigned)(tb < OC_MAX_GRID ? tb : OC_MAX_GRID)), dim3(OC_BLOCK), 0, stream, T, decay,
                       occupancy);
    if (n == 0) return;
    const size_t nb = (n + OC_BLOCK - 1) / OC_BLOCK;
    hipLaunchKernelGGL(k_occupancy_scatter_max, dim3((unsigned)(nb < OC_MAX_GRID ? nb : OC_MAX_GRID)), dim3(OC_BLOCK), 0, stream, T, n,
                       cells, sigma, reinterpret_cast<int *>(occupancy), samples_per_ray, count);
}

size_t cull_scratch_u32(size_t n) { return (n + CU_TILE - 1) / CU_TILE + 1; }

void launch_cull_samples(size_t n, uint32_t samples_per_ray, const uint32_t *cells, const float *occupancy, uint32_t T, float threshold,
                         uint32_t *live, uint32_t *live_count, float *sigma, float *rgb, uint32_t *scratch, const uint32_t *count,
                         hipStream_t stream) {
    if (n == 0) { (void)hipMemsetAsync(live_count, 0, sizeof(uint32_t), stream); return; }
    const size_t tiles = (n + CU_TILE - 1) / CU_TILE;
    const unsigned blocks = (unsigned)((tiles + CU_BLOCK / 64 - 1) / (CU_BLOCK / 64));
    hipLaunchKernelGGL(k_cull_count, dim3(blocks), dim3(CU_BLOCK), 0, stream, n, samples_per_ray, cells, occupancy, T, threshold, scratch,
                       tiles, count);
    hipLaunchKernelGGL(k_cull_scan, dim3(1), dim3(CU_SCAN), 0, stream, scratch, tiles, live_count);
    hipLaunchKernelGGL(k_cull_write, dim3(blocks), dim3(CU_BLOCK), 0, stream, n, samples_per_ray, cells, occupancy, T, threshold,
                       (const uint32_t *)scratch, tiles, live, sigma, rgb, count);
}

void launch_mlp_forward_indexed(size_t n_max, uint32_t samples_per_ray, size_t num_rays, const uint32_t *live, const uint32_t *live_count,
                                const uint32_t *vi, const float *bc, const float *fieldT, const float *dirs, const MlpPacks &w, int mode,
                                float *sigma, float *rgb, hipStream_t stream, const uint32_t *count) {
    if (n_max == 0) return;
    const bool density_only = rgb == nullptr;
    if (density_only) num_rays = 0;
    if (mode == 0) {
        launch_head_ray_term(num_rays, dirs, w, stream);
        const size_t smem = mlp::MAX_STAGE_FLOATS * sizeof(float);
        if (density_only)
            mlp::launch_group_kernel<k_mlp_forward_indexed<true>, mlp::MLP_BLOCK>(n_max, smem, stream, n_max, samples_per_ray, live, live_count, vi,
                                                                                 bc, fieldT, (const float *)w.hterm, w.pk_gather, sigma, rgb, count);
        else
            mlp::launch_group_kernel<k_mlp_forward_indexed<false>, mlp::MLP_BLOCK>(n_max, smem, stream, n_max, samples_per_ray, live, live_count, vi,
                                                                                  bc, fieldT, (const float *)w.hterm, w.pk_gather, sigma, rgb, count);
    } else {
        launch_dir_encoding(num_rays, dirs, w.enc, mlp::ENC32, stream);
        const size_t smem = x3::MAX_STAGE_U4 * sizeof(uint4);
        if (density_only)
            mlp::launch_group_kernel<k_mlp_forward_x3_indexed<true>, x3::X3_BLOCK>(n_max, smem, stream, n_max, samples_per_ray, live, live_count, vi,
                                                                                  bc, fieldT, (const float *)w.enc, w.blob, sigma, rgb,
                                                                                  w.ray_bias, count);
        else
            mlp::launch_group_kernel<k_mlp_forward_x3_indexed<false>, x3::X3_BLOCK>(n_max, smem, stream, n_max, samples_per_ray, live, live_count, vi,
                                                                                   bc, fieldT, (const float *)w.enc, w.blob, sigma, rgb,
                                                                                   w.ray_bias, count);
    }
}

}  // namespace tn
