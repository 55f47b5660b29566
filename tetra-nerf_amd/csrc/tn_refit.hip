// tn_refit.hip -- tn_update_vertices: the vertices of a loaded mesh moved, `cells` did not.
//
// load_tetrahedra's face hash, scans, Morton sort, adjacency codes and the radix-sort rounds of the face BVH are functions
// of `cells` alone.  What holds positions is recomputed here in place, each value through the element function of
// tn_build_core.h that states the build's expression for it, so a refitted table is bit-equal to a fresh build's:
//
//   walk records  k_tet_thin's star minima again, then ONE LANE PER RECORD (r, e) over the kept `order`: the lane loads the
//                 32-byte WalkHot record as two 16-byte vectors, replaces pn (the vertex opposite e) and bits 8..15 of
//                 code_hi, and stores the two vectors back -- consecutive lanes write consecutive records (the alternative,
//                 one lane per tet through rec_of_tet, scatters 128-byte pieces).  The four lanes of a tet each derive its
//                 thin exponent (four cached loads).  The lane's vertex is one of the 4T `cells` entries, each visited once:
//                 the same pass reduces max |coordinate| (scene_max) and the mesh box of binned calls.  WalkCold / WalkTet /
//                 WalkFid hold no positions.
//   face BVH      the kept binary tree and face order: boxes bottom up per level (a leaf folds core::face_box of its faces,
//                 so no per-face box array is written and read back), the leaf triangles into the existing leaf_tri, and the
//                 64-wide SoA boxes copied from the binary nodes the kept `child` rows and wide_sub name.  Route (a) of the
//                 two the collapse allows: `child`, the node count and the traversal stack bound stay, nothing is
//                 reallocated or read back.  The greedy collapse opened the nodes by the OLD box areas; any opening order
//                 gives a valid tree, only its quality drifts with the deformation.
//   hull          the nine floats of every hull face from the kept ids, the threaded tree / flat box table by the host routine
//                 of the build (build_hull_from_info) while the BVH kernels run, uploaded into the existing buffers.
//
// Meshes whose tetrahedra overlap after the move are outside what the walk certifies, exactly as for a fresh load of them.
#include <algorithm>
#include <cstring>

#include <hip/hip_runtime.h>

#include "tn_build.h"

namespace tn {

namespace {

constexpr int BT = 256;
inline unsigned grid_for(size_t n) { return (unsigned)((n + BT - 1) / BT); }
__device__ __forceinline__ size_t gid() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }

__global__ __launch_bounds__(BT) void k_refit_tet_thin(size_t T, const uint32_t *__restrict__ cells, const float *__restrict__ xyz,
                                                       uint32_t *vmin) {
    const size_t i = gid();
    if (i < T) core::tet_thin_star((uint32_t)i, cells, xyz, vmin);
}

// Seven numbers over the referenced vertices, reduced beside the record pass (its lanes visit every entry of `cells` once):
// number 0 = max |coordinate| as float bits (k_cells_check_max), 1..3 / 4..6 = max / min per axis as core::float_ordered
// (k_mesh_box: NaN coordinates skipped).  Atomics on one address serialise (~13 ns each: one per wave made this pass 0.7 ms at
// 1M tets, seven per wave on one 128-byte line 0.3 ms at any size), so the pass runs as at most RECORD_BLOCKS persistent blocks,
// each reduces through LDS to one atomic per number, and every number has a line of its own.
constexpr int N_STATS_REFIT = 7, STAT_STRIDE = 32, RECORD_BLOCKS = 1024;

// lane i: records i, i + grid, ... (i = 4r + e)
__global__ __launch_bounds__(BT) void k_refit_records(size_t n4, const uint32_t *__restrict__ order, const uint32_t *__restrict__ cells,
                                                      const float *__restrict__ xyz, const uint32_t *__restrict__ vmin, WalkHot *hot,
                                                      uint32_t *stats) {
    __shared__ uint32_t part[BT / 64][N_STATS_REFIT];
    float m = 0.f;
    uint32_t v[N_STATS_REFIT] = {0u, 0u, 0u, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (size_t i = gid(); i < n4; i += (size_t)gridDim.x * BT) {
        const uint32_t *c = cells + 4 * (size_t)order[i >> 2];
        uint4 *q = reinterpret_cast<uint4 *>(hot + i);
        union { WalkHot rec; uint4 v[2]; } u;
        u.v[0] = q[0]; u.v[1] = q[1];
        core::refit_walk_record(u.rec, (uint32_t)(i & 3), c, xyz, vmin);
        q[0] = u.v[0]; q[1] = u.v[1];
        m = fmaxf(m, fmaxf(fabsf(u.rec.pn[0]), fmaxf(fabsf(u.rec.pn[1]), fabsf(u.rec.pn[2]))));
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (u.rec.pn[a] == u.rec.pn[a]) {
                const uint32_t o = core::float_ordered(u.rec.pn[a]);
                v[1 + a] = o > v[1 + a] ? o : v[1 + a];
                v[4 + a] = o < v[4 + a] ? o : v[4 + a];
            }
    }
    v[0] = __float_as_uint(m);   // non-negative floats order as uints
#pragma unroll
    for (int k = 0; k < N_STATS_REFIT; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t w = (uint32_t)__shfl_xor((int)v[k], off);
            v[k] = k < 4 ? (w > v[k] ? w : v[k]) : (w < v[k] ? w : v[k]);
        }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < N_STATS_REFIT; ++k) part[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < N_STATS_REFIT) {
        const int k = threadIdx.x;
        uint32_t r = part[0][k];
        for (int w = 1; w < BT / 64; ++w) r = k < 4 ? (part[w][k] > r ? part[w][k] : r) : (part[w][k] < r ? part[w][k] : r);
        if (k < 4) atomicMax(stats + k * STAT_STRIDE, r);
        else atomicMin(stats + k * STAT_STRIDE, r);
    }
}

__global__ __launch_bounds__(BT) void k_refit_hull(size_t n_hull, const uint32_t *__restrict__ faces, const float *__restrict__ xyz,
                                                   uint32_t *info) {
    const size_t h = gid();
    if (h < n_hull) core::hull_face_refit(faces, xyz, info + 12 * h);
}

__global__ __launch_bounds__(BT) void k_refit_node_boxes(uint32_t first_node, uint32_t n_nodes, const core::BinNode *__restrict__ bn,
                                                         const uint32_t *__restrict__ order, const uint32_t *__restrict__ faces,
                                                         const float *__restrict__ xyz, float *node_lo, float *node_hi) {
    const size_t t = gid();
    if (t < n_nodes) core::refit_node_box(first_node + t, bn, order, faces, xyz, node_lo, node_hi);
}

// k_leaf_soa without the face ids: 64 threads = 64 / leaf_w leaves
__global__ __launch_bounds__(64) void k_refit_leaf_tri(uint32_t n_leaves, uint32_t leaf_w, uint32_t leaf_shift,
                                                       const uint32_t *__restrict__ leaf_nodes, const core::BinNode *__restrict__ bn,
                                                       const uint32_t *__restrict__ order, const uint32_t *__restrict__ faces,
                                                       const float *__restrict__ xyz, float *leaf_tri) {
    const size_t l = (size_t)blockIdx.x * (64u >> leaf_shift) + (threadIdx.x >> leaf_shift);
    const uint32_t i = threadIdx.x & (leaf_w - 1);
    if (l >= n_leaves) return;
    const core::BinNode nd = bn[leaf_nodes[l]];
    float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < nd.count) {
        const uint32_t *f = faces + 3 * (size_t)order[nd.first + i];
        for (int q = 0; q < 3; ++q)
            for (int k = 0; k < 3; ++k) v[q * 3 + k] = xyz[3 * (size_t)f[q] + k];
    }
    for (int q = 0; q < 9; ++q) leaf_tri[(l * 9 + q) * leaf_w + i] = v[q];
}

// one lane per (wide node, slot): the six SoA box rows from the binary node behind the slot's child reference
__global__ __launch_bounds__(BT) void k_refit_wide_boxes(size_t n_slots, const uint32_t *__restrict__ child,
                                                         const uint32_t *__restrict__ leaf_nodes, const uint32_t *__restrict__ wide_sub,
                                                         const float *__restrict__ node_lo, const float *__restrict__ node_hi, float *boxes) {
    const size_t j = gid();
    if (j >= n_slots) return;
    const size_t w = j / WIDE, i = j % WIDE;
    const int k = core::wide_child_node(child[j], leaf_nodes, wide_sub);
    for (int a = 0; a < 3; ++a) {
        boxes[(w * 6 + a) * WIDE + i] = k < 0 ? INFINITY : node_lo[3 * (size_t)k + a];
        boxes[(w * 6 + 3 + a) * WIDE + i] = k < 0 ? -INFINITY : node_hi[3 * (size_t)k + a];
    }
}

static_assert(N_STATS_REFIT * STAT_STRIDE == REFIT_STAT_WORDS, "RefitTables::vmin holds the seven numbers behind the V minima");

}  // namespace

void device_refit(size_t V, size_t T, const float *xyz, const uint32_t *cells, hipStream_t s, RefitTargets out, RefitTables &kept,
                  float &scene_max, float box_lo[3], float box_hi[3]) {
    // every check comes before the first launch: a refused refit leaves the tables of the old vertices whole
    const size_t n4 = 4 * T, n_hull = kept.hull_info.n / 12, n_leaves = kept.leaf_nodes.n, n_wide = kept.wide_sub.n;
    if (!kept.valid || kept.order.n != T || kept.vmin.n != V + REFIT_STAT_WORDS || kept.level_start.size() < 2 ||
        out.bvh.child.n != n_wide * WIDE || out.bvh.boxes.n != n_wide * 6 * WIDE ||
        out.bvh.leaf_tri.n != n_leaves * 9 * out.bvh.view.leaf_w || out.hull_tris.n != n_hull * 12)
        throw Error("internal: the kept refit tables do not belong to the loaded mesh");

    // ------------------------------------------------------------ walk records, max |coordinate|
    uint32_t *vmin = kept.vmin.p, *stats = kept.vmin.p + V;
    TN_HIP(hipMemsetD32Async((hipDeviceptr_t)vmin, 0x7F800000, V, s));   // +inf
    TN_HIP(hipMemsetAsync(stats, 0, 4 * STAT_STRIDE * sizeof(uint32_t), s));            // maxima
    TN_HIP(hipMemsetAsync(stats + 4 * STAT_STRIDE, 0xFF, 3 * STAT_STRIDE * sizeof(uint32_t), s));   // minima
    hipLaunchKernelGGL(k_refit_tet_thin, dim3(grid_for(T)), dim3(BT), 0, s, T, cells, xyz, vmin);
    hipLaunchKernelGGL(k_refit_records, dim3(std::min<unsigned>(grid_for(n4), RECORD_BLOCKS)), dim3(BT), 0, s, n4, kept.order.p, cells, xyz, vmin, out.hot, stats);
    // ------------------------------------------------------------ hull faces -> host
    std::vector<float> hinfo(n_hull * 12);
    uint32_t hs[REFIT_STAT_WORDS] = {}, h[N_STATS_REFIT];
    if (n_hull) {
        hipLaunchKernelGGL(k_refit_hull, dim3(grid_for(n_hull)), dim3(BT), 0, s, n_hull, out.faces, xyz, kept.hull_info.p);
        TN_HIP(hipMemcpyAsync(hinfo.data(), kept.hull_info.p, hinfo.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    TN_HIP(hipMemcpyAsync(hs, stats, sizeof hs, hipMemcpyDeviceToHost, s));
    struct Event {
        hipEvent_t e = nullptr;
        ~Event() { if (e) (void)hipEventDestroy(e); }
    } read_done;
    TN_HIP(hipEventCreateWithFlags(&read_done.e, hipEventDisableTiming));
    TN_HIP(hipEventRecord(read_done.e, s));
    // ------------------------------------------------------------ face BVH over the kept tree
    for (size_t l = kept.level_start.size() - 1; l-- > 0;) {
        const uint32_t first_node = kept.level_start[l], cnt = kept.level_start[l + 1] - kept.level_start[l];
        hipLaunchKernelGGL(k_refit_node_boxes, dim3(grid_for(cnt)), dim3(BT), 0, s, first_node, cnt, kept.bn.p, kept.face_order.p,
                           out.faces, xyz, kept.node_lo.p, kept.node_hi.p);
    }
    {
        const uint32_t leaf_w = out.bvh.view.leaf_w, leaf_shift = out.bvh.view.leaf_shift;
        const unsigned per_block = 64u >> leaf_shift;
        hipLaunchKernelGGL(k_refit_leaf_tri, dim3((unsigned)((n_leaves + per_block - 1) / per_block)), dim3(64), 0, s, (uint32_t)n_leaves,
                           leaf_w, leaf_shift, kept.leaf_nodes.p, kept.bn.p, kept.face_order.p, out.faces, xyz, out.bvh.leaf_tri.p);
    }
    hipLaunchKernelGGL(k_refit_wide_boxes, dim3(grid_for(n_wide * WIDE)), dim3(BT), 0, s, n_wide * WIDE, out.bvh.child.p,
                       kept.leaf_nodes.p, kept.wide_sub.p, kept.node_lo.p, kept.node_hi.p, out.bvh.boxes.p);
    TN_HIP(hipGetLastError());
    // ------------------------------------------------------------ hull tree on the host, beside the BVH kernels
    HostHullBvh hth;
    std::vector<float> nodes;
    hipError_t e = hipEventSynchronize(read_done.e);   // the two reads, enqueued in front of the BVH kernels
    if (e == hipSuccess && n_hull) {
        build_hull_from_info(hinfo, hth);
        nodes = hth.nodes_and_flat();
        if (nodes.size() != out.hull_nodes.n || hth.tris.size() != out.hull_tris.n)
            throw Error("internal: the hull tree changed its size in a refit");
        e = hipMemcpyAsync(out.hull_nodes.p, nodes.data(), nodes.size() * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(out.hull_tris.p, hth.tris.data(), hth.tris.size() * sizeof(float), hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // blocking, like the load: hinfo / nodes / hth go out of scope
    TN_HIP(e);
    for (int k = 0; k < N_STATS_REFIT; ++k) h[k] = hs[k * STAT_STRIDE];
    std::memcpy(&scene_max, &h[0], 4);
    for (int k = 0; k < 3; ++k) {   // (mesh_box: an axis whose every coordinate is NaN stays 0)
        const bool any = h[4 + k] <= h[1 + k];
        box_lo[k] = any ? core::ordered_float(h[4 + k]) : 0.f;
        box_hi[k] = any ? core::ordered_float(h[1 + k]) : 0.f;
    }
    out.bvh.view.scene_max = scene_max;
}

}  // namespace tn
