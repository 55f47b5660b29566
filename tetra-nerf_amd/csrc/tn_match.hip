// tn_match.hip -- find_visited_cells: match S sorted sample distances of a ray against its
// <= M sorted segments and lerp the entry/exit barycentrics.
//
// Replaces find_matched_cells_kernel (src/tetrahedra_tracer.cu:115-160; 16-thread blocks,
// one thread per ray, serial over samples).  Here ONE WAVEFRONT owns a ray and runs
// rayops::ray_match (tn_ray_ops.h) -- the matcher the persistent render kernel runs too.
#include "tn_ray_ops.h"

namespace tn {

// The per-ray chain of dependent round trips (row index -> count -> bounds -> distances -> search -> gather -> store) is what
// the op waits for at every size: the NEXT ray's row index and count are requested while this one is
// matched; the matcher itself requests the bounds rows of up to 8 chunks and the distances of a whole group of 64 UM samples
// together.  The kernel keeps the grid-stride loop, that prefetch and the LDS carve.
template <int UM>
__global__ __launch_bounds__(64) void k_find_matched(size_t R, uint32_t S, uint32_t M,
                                                     const uint32_t *__restrict__ num_visited,
                                                     const uint32_t *__restrict__ visited,
                                                     const float *__restrict__ dist,
                                                     const float *__restrict__ bary,
                                                     const float *__restrict__ distances,
                                                     const uint32_t *__restrict__ verts,
                                                     uint32_t *__restrict__ cells_out,
                                                     uint32_t *__restrict__ verts_out,
                                                     uint8_t *__restrict__ mask_out,
                                                     float *__restrict__ bary_out,
                                                     const uint32_t *__restrict__ ray_index, const uint32_t *__restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (count) R = *count;      // device-side number of (hitting) rays; the grid was sized for an upper bound
    float *tin = reinterpret_cast<float *>(smem);  // [M]
    float *pmax = tin + M;                         // [M] running max of t_out
    const int lane = threadIdx.x;
    const rayops::MatchRows rows{visited, dist, bary, verts};
    const float2 no_bounds[8] = {};                // (the bounds are loaded in place: nothing was requested ahead)

    // row of the trace outputs a sample row belongs to (ray_index: the caller kept the trace rows of ALL rays and matches a
    // subset -- no compacted copy of the 26 KB rows) and its segment count, one ray ahead
    size_t ray = blockIdx.x;
    size_t src_next = 0;
    uint32_t n_next = 0;
    if (ray < R) {
        src_next = ray_index ? (size_t)ray_index[ray] : ray;
        n_next = num_visited[src_next];
    }
    for (; ray < R; ray += gridDim.x) {
        const size_t src = src_next;
        const uint32_t n = n_next;
        if (ray + gridDim.x < R) {
            src_next = ray_index ? (size_t)ray_index[ray + gridDim.x] : ray + gridDim.x;
            n_next = num_visited[src_next];
        }
        const float *srow = distances + ray * S;
        const size_t o = ray * S;
        const rayops::MatchOut out{cells_out + o, mask_out + o, verts_out + 4 * o, bary_out + 3 * o};
        rayops::ray_match<UM, true, false>(S, M, src, n, rows, [srow](uint32_t j) { return srow[j]; }, out, tin, pmax, lane, no_bounds);
    }
}

void launch_find_matched_cells(size_t R, size_t S, size_t M, const uint32_t *num_visited,
                               const uint32_t *visited, const float *dist, const float *bary,
                               const float *distances, const uint32_t *verts, uint32_t *cells_out,
                               uint32_t *verts_out, uint8_t *mask_out, float *bary_out, hipStream_t stream,
                               const uint32_t *ray_index, const uint32_t *count) {
    if (R == 0 || S == 0) return;
    const size_t smem = 2 * M * sizeof(float);
    const size_t max_blocks = 256 * 32;
    const unsigned grid = (unsigned)(R < max_blocks ? R : max_blocks);
    // the samples of a ray in ONE group where they fit: 64 UM per iteration of the search / gather / store chain
    if (S <= 256)
        hipLaunchKernelGGL(k_find_matched<4>, dim3(grid), dim3(64), smem, stream, R, (uint32_t)S, (uint32_t)M,
                           num_visited, visited, dist, bary, distances, verts, cells_out, verts_out, mask_out, bary_out, ray_index, count);
    else
        hipLaunchKernelGGL(k_find_matched<5>, dim3(grid), dim3(64), smem, stream, R, (uint32_t)S, (uint32_t)M,
                           num_visited, visited, dist, bary, distances, verts, cells_out, verts_out, mask_out, bary_out, ray_index, count);
}

}  // namespace tn
