// tn_api_tracer.hip -- C-ABI of the tracer handle (see include/tetranerf_hip.h): load_tetrahedra, the trace_rays
// schedule (TraceCall below), the other mesh queries, statistics and options.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>

#include "tn_api_common.h"
#include "tn_build.h"
#include "tn_devbuf.h"
#include "tn_isosurface_core.h"
#include "tn_kernels.h"
#include "tn_split_core.h"
#include "tn_edge_split_core.h"
#include "tn_flip_core.h"

using tn::check_loaded;
using tn::check_pow2_M;
using tn::DeviceGuard;
using tn::guarded;

struct tn_tracer {
    int device = 0;
    // One tracer = one set of scratch buffers, counters, side streams and events: calls on the SAME handle are serialised
    // here (host section only: the kernels of two calls still queue behind each other on their streams).  ctypes releases
    // the GIL, so a viewer thread and a trainer sharing a tracer can be inside tn_trace_rays* at the same time.
    std::mutex mu;

    // ---- what load_tetrahedra builds
    struct Mesh {
        bool loaded = false;
        tn::DeviceMesh view;                 // what the kernels get: pointers into the tables below + the caller's xyz / cells
        tn::HostMesh host;                   // kept for tn_get_faces (device build: downloaded on first use)
        uint32_t bvh_max_stack = 1;
        tn::DevBuf<uint32_t> faces, face_tets;
        tn::DevWideBvh bvh;
        tn::DevBuf<tn::WalkVar> vars;        // the build's 64-byte records: split into the tables below, then released
        tn::DevBuf<tn::WalkHot> hot;
        tn::DevBuf<tn::WalkCold> cold;
        tn::DevBuf<tn::WalkTet> tets;
        tn::DevBuf<tn::WalkFid> fidt;
        tn::DevBuf<float> hull_nodes, hull_tris;
        tn::RefitTables refit;               // option "refit_tables": what tn_update_vertices needs beyond the tables above, else empty
        bool device_built = false;
    } mesh;

    // ---- exactly what tn_set_option writes.  include/tetranerf_hip.h documents the values; the measurements that chose
    //      the defaults are quoted in full in the last section of profiles/HISTORY.md (file names below: profiles/)
    struct Options {
        bool gpu_build = true;               // structures built on the device (tn_build.hip); false: the host build (tn_mesh.cpp)
        unsigned leaf_width = 16;            // faces per BVH leaf block (applies at the next load_tetrahedra)
        int writer_table = 0;                // 0: by mesh size (WALK_TET_MIN_TETS), 1: per (tet, entry face), 2: per tet
        bool refit_tables = false;           // the next device build keeps tn::RefitTables (tn_update_vertices)
        int use_walk = 1;                    // 0 never, 1 from walk_min_rays rays on, 2 always
        size_t walk_min_rays = 12288;        // crossover of BVH path and walk on 100k ... 1M tets (r02t_crossover.txt, r06y_batch_crossover.txt)
        bool walk_min_auto = true;           // ... and by mesh size above that until the option is set (TraceCall::walk_min_rays)
        bool dense_tails = true;             // false: slots >= num_visited stay unwritten on walked rows
        bool literal = true;                 // false: rays with uncertified order are re-traced through the BVH, not paired from the log
        size_t log_cap_bytes = 0;            // "log_cap_mb"; 0: a fraction of the free device memory (TraceCall::log_chunk)
        int spec_fill = 0;                   // 1: the last quarter / half of every row is filled beside the walk; off: r06r_spec_sweep.txt +-0.4 %
        unsigned spec_k0 = 0;                // override of that fill's first slot (tests)
        tn::FillRange spec{true, 0, true, tn::FillKind::Spans, 512};         // "spec_blocks": 2 blocks per CU (r04f_overlap_sweep.txt)
        unsigned walk_lds_kb = 26;           // dynamic LDS per walk block beside that fill: 6 blocks per CU, both stay resident (same sweep)
        tn::FillRange tail{false, 0, false, tn::FillKind::RowPerBlock, 0};   // "fill_blocks": -5.9 / -6.6 / -1.3 % (r06u_alloc_sweep.txt)
        unsigned writer_blocks = 0;          // grid of the segment writer (0: 2 blocks per CU)
        bool hull_flat = true;               // entry search through the flat box table in LDS (hulls of <= 1024 faces); false: threaded tree
        bool small_lds = true;               // small batches: LDS hit arrays sized for the mesh, overflow rays in a second launch
        unsigned lds_cap = 0;                // 0: from the mesh size; otherwise the entries of the small arrays (tests)
        unsigned verify_stride = 256;        // count cross-check of every n-th certified ray (r06i_stride_sweep.txt: +0.0 / +0.7 / +1.1 % against 1024) ...
        bool verify_risk = true;             // ... and of every ray inside the wide band of a certification guard,
        unsigned risk_band = 2;              // in units of the guards' 8 delta (r05e_risk_sweep.txt: band 4 costs +1.1 / +5.3 / +4.1 %)
        bool verify_inject = false;          // tests: every cross-checked ray counts as a mismatch
        unsigned literal_sort_passes = 8;    // odd-even passes over a literal ray's hits before the bitonic network (tests: 0, 1)
        int cert_ends = 2;                   // the walk's order test; 2: rules A-C below WALK_TET_MIN_TETS tets, the cluster test above (r06m_sweep*.txt)
        bool bin_rays = false;               // every eligible call is binned, as if it carried TN_TRACE_BIN_RAYS (TETRANERF_HIP_BIN_RAYS)
        bool timing = false;                 // one-chunk calls serialised on the caller's stream, an event after each kernel (tn_trace_timings)
    } opt;

    // ---- per-call device buffers and the counters of the last call
    struct Scratch {
        tn::DevBuf<uint32_t> fallback_list;  // [R] rays for the BVH all-hits kernel (small batches: the overflow rays)
        tn::DevBuf<uint32_t> walk_n;         // [R] walk -> writer / fills
        tn::DevBuf<uint4> hull_entry;        // [R] k_hull_entry -> k_trace_walk
        tn::DevBuf<uint2> literal_list;      // [R] rays whose logged hits go through the literal sort + pairing
        tn::DevBuf<uint4> hit_log;           // walk -> segment writer / literal pairing: 16 B per recorded hit, [rays / 64][M][64]
        tn::DevBuf<uint32_t> verify_list;    // [R] certified rays whose count differed: re-traced by the BVH kernel at the end of the call
        tn::DevBuf<uint32_t> risk_list;      // [R] certified rays inside the wide band of a certification guard (all cross-checked)
        // binned calls only (tn_ray_order.hip): the sort's input and output, its temporary storage, walk_n in item order
        tn::DevBuf<uint32_t> ray_keys, ray_iota, ray_keys_sorted, order, walk_n_item;   // [R] each
        tn::DevBuf<char> sort_temp;
        static constexpr int N_CTR = 2;      // 64-bit words behind the statistics: four uint32 device-side counts
        tn::DevBuf<unsigned long long> stats;   // [tn::N_STATS] counters (tn_common.h: STAT_*) + the four counts (one memset clears all)
        uint32_t *fallback_count() { return reinterpret_cast<uint32_t *>(stats.p + tn::N_STATS); }
        uint32_t *literal_count() { return fallback_count() + 1; }
        uint32_t *verify_count() { return fallback_count() + 2; }
        uint32_t *risk_count() { return fallback_count() + 3; }
        static constexpr size_t stats_bytes() { return (tn::N_STATS + N_CTR) * sizeof(unsigned long long); }
        // what the counters belong to
        size_t last_num_rays = 0;
        bool last_walk = false;
        bool last_binned = false;            // the last call walked its rays in the order scratch.order holds (tn_trace_ray_order)
        hipStream_t last_stream = nullptr;

        template <typename T>
        static void grow(tn::DevBuf<T> &b, size_t n) { if (b.n < n) b.alloc(n); }
        // The only place scratch grows, once per call and BEFORE its first launch: an allocation in the middle of
        // the overlapped schedule would synchronise the device there (hipFree / hipMalloc).  Every buffer is guarded by its
        // own size (alloc frees first: after a failed hipMalloc only that buffer is empty, and the next call grows it again).
        // R entries each: the blind sample + the risk classes can, on a degenerate mesh, name every ray.
        void reserve(size_t R, size_t log_entries, bool verify, bool risk, size_t sort_temp_bytes = 0) {
            grow(fallback_list, R);
            if (!log_entries) return;        // small batch: the overflow list only
            grow(walk_n, R); grow(literal_list, R); grow(hull_entry, R); grow(hit_log, log_entries);
            if (verify) grow(verify_list, R);
            if (risk) grow(risk_list, R);
            if (sort_temp_bytes) {           // binned call
                grow(ray_keys, R); grow(ray_iota, R); grow(ray_keys_sorted, R); grow(order, R); grow(walk_n_item, R);
                grow(sort_temp, sort_temp_bytes);
            }
        }
    } scratch;

    // ---- side streams and event edges of the one-chunk schedule (TraceCall::run_overlapped)
    struct Schedule {
        hipStream_t side = nullptr;          // literal pairing of the logged hits (beside the tail fill)
        hipStream_t aux = nullptr;           // BVH re-trace of the fallback rays (forked right after the walk)
        hipStream_t pre = nullptr;           // speculative tail fill beside the walk
        hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_start = nullptr, ev_pre = nullptr, ev_seg = nullptr, ev_aux = nullptr;
        static constexpr int N_TEV = 9;      // option "timing": an event in front of, between and behind the eight parts
        hipEvent_t tev[N_TEV] = {};
        bool tev_valid = false;
    } sched;
};

namespace {

tn_tracer *checked(tn_tracer_t t) {
    if (!t) throw tn::Error("tracer handle is null");
    return t;
}

// (+ WIDE: the traversal pops the next node before it pushes the current one's children)
void check_bvh_depth(uint32_t max_stack) {
    if (max_stack + (uint32_t)tn::WIDE > (uint32_t)tn::STACK_CAP)
        throw tn::Error("face BVH too deep for the traversal stack (" + std::to_string(max_stack) + " > " +
                        std::to_string(tn::STACK_CAP) + " entries)");
}

struct BuildCounts { size_t F = 0, n_hull = 0, n_hull_nodes = 0; };

// host build: blocking D2H of the mesh (the reference does the same: tetrahedra_tracer.cpp:255-259)
BuildCounts build_on_host(tn_tracer::Mesh &m, unsigned leaf_width, size_t V, size_t T, const float *xyz, const uint32_t *cells,
                          hipStream_t stream) {
    std::vector<float> hxyz(3 * V);
    std::vector<uint32_t> hcells(4 * T);
    TN_HIP(hipStreamSynchronize(stream));
    if (V) TN_HIP(hipMemcpy(hxyz.data(), xyz, hxyz.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (T) TN_HIP(hipMemcpy(hcells.data(), cells, hcells.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < hcells.size(); ++i)
        if (hcells[i] >= V) throw tn::Error("cells contains a vertex index that is out of bounds");

    tn::build_face_table(T, hcells.data(), m.host);
    const size_t F = m.host.face_tets.size() / 2;
    float smax = 0.f;
    for (size_t i = 0; i < hcells.size(); ++i)
        for (int k = 0; k < 3; ++k) smax = std::max(smax, std::fabs(hxyz[3 * (size_t)hcells[i] + k]));
    m.host.scene_max = smax;

    std::vector<uint32_t> all(F), hull_ids;
    for (size_t f = 0; f < F; ++f) {
        all[f] = (uint32_t)f;
        if (m.host.face_tets[2 * f + 1] == TN_EMPTY) hull_ids.push_back((uint32_t)f);
    }
    tn::HostWideBvh hb;
    tn::build_wide_bvh(hxyz.data(), m.host.faces.data(), all, hb, leaf_width);
    check_bvh_depth(hb.max_stack);
    m.bvh_max_stack = hb.max_stack;
    std::vector<tn::TetRec> recs;
    std::vector<uint32_t> rec_of_tet;
    tn::build_tet_records(T, hcells.data(), hxyz.data(), m.host, recs, rec_of_tet);
    tn::HostHullBvh hth;
    tn::build_hull_threaded(hxyz.data(), m.host.faces.data(), m.host.face_tets.data(), hull_ids, recs, rec_of_tet, hth);

    m.faces.upload(m.host.faces);
    m.face_tets.upload(m.host.face_tets);
    m.bvh.upload(hb, smax);
    {
        std::vector<tn::WalkVar> vars;
        tn::build_walk_variants(recs, vars);
        m.vars.upload(vars);
    }
    m.hull_nodes.upload(hth.nodes_and_flat());
    m.hull_tris.upload(hth.tris);
    return BuildCounts{F, hull_ids.size(), hth.nodes.size() / 8};
}

// the mesh's part of a parameter block + the rows of one launch; no counters (TraceCall::trace_params adds them)
tn::TraceParams mesh_params(const tn_tracer *t, size_t num_items, const tn::Rows &r, const float *o, const float *d) {
    tn::TraceParams p{};
    p.origins = o; p.dirs = d;
    p.faces = t->mesh.view.faces; p.face_tets = t->mesh.view.face_tets;
    p.bvh = t->mesh.view.bvh;
    p.out_num = r.num; p.out_cells = r.cells; p.out_bary = r.bary; p.out_dist = r.dist; p.out_verts = r.verts;
    p.M = r.M; p.num_items = num_items; p.ray_list = nullptr;
    return p;
}

// One tn_trace_rays call on a loaded tracer (R > 0, arguments checked, counters cleared): which path it takes, the
// parameter blocks of its launches, and the three schedules.
struct TraceCall {
    tn_tracer *t;
    size_t R;
    const float *origins, *dirs;
    tn::Rows rows;                           // the caller's five outputs
    bool dense_tails;                        // per CALL (TN_TRACE_COMPACT_ROWS), not per tracer
    hipStream_t stream;                      // the caller's
    bool binned = false;                     // run_overlapped walks the rays in the order of their keys (TN_TRACE_BIN_RAYS)

    const tn_tracer::Options &o() const { return t->opt; }
    tn_tracer::Scratch &s() const { return t->scratch; }
    const tn::DeviceMesh &mesh() const { return t->mesh.view; }
    bool verify_risk() const { return o().verify_risk && o().verify_stride; }

    // Small batches are latency-bound: a lane walking ~180 dependent steps is slower than one wavefront per ray through
    // the wide BVH (measured: 4096 rays, 300k tets: 1.5 ms vs 0.75 ms), so the walk is used from this many rays on.  The
    // BVH path's LDS hit arrays grow with the mesh and a batch then needs several rounds of waves: 8192 from 2M tets,
    // 6144 from 4M tets on (2.7 M / 6.7 M tets at 8192 rays: BVH 2.11 / 3.37 ms, walk 2.02 / 2.68;
    // profiles/r06al_big_mesh_batches.txt)
    size_t walk_min_rays() const {
        if (!o().walk_min_auto) return o().walk_min_rays;
        return mesh().T >= 4000000u ? (size_t)6144 : mesh().T >= 2000000u ? (size_t)8192 : o().walk_min_rays;
    }
    // M >= 4: the writer and the fills store 16-byte vectors into the rows; M is a power of two, so from 4 on every row
    // base is 16-byte aligned.  (use_walk == 2 forces the walk for any size; HullEntry keeps the face's slot in 24 bits)
    bool use_walk() const {
        return o().use_walk && (R >= walk_min_rays() || o().use_walk == 2) && rows.M >= 4 && mesh().n_hull > 0 &&
               mesh().n_hull < (1u << 24);
    }
    // Rays per chunk.  The log holds 16 B per hit slot; calls whose log would exceed the cap are processed in ray chunks
    // (multiples of 4096 rays, the walk's XCD run), serially.
    size_t log_chunk() const {
        size_t cap_bytes = o().log_cap_bytes;
        if (!cap_bytes) {
            // the log lives for the tracer's lifetime: at most a quarter of what is free now (plus what it already
            // holds), at most 24 GB; a call that needs more runs in chunks instead of failing in hipMalloc
            size_t free_b = 0, total_b = 0;
            TN_HIP(hipMemGetInfo(&free_b, &total_b));
            cap_bytes = std::min<size_t>((free_b + s().hit_log.n * sizeof(uint4)) / 4, (size_t)24 << 30);
        }
        const size_t chunk = std::max<size_t>(cap_bytes / ((size_t)rows.M * sizeof(uint4)) / 4096 * 4096, 4096);
        return std::min(chunk, R);
    }

    // ---- parameter blocks of the launches over rays [base, base + n): pure, no launches
    tn::TraceParams trace_params(size_t base, size_t n) const {
        tn::TraceParams q = mesh_params(t, n, rows.at(base), origins + 3 * base, dirs + 3 * base);
        q.stats = s().stats.p;
        q.compact_rows = dense_tails ? 0u : 1u;
        q.sort_passes = o().literal_sort_passes;
        return q;
    }
    tn::WalkParams walk_params(size_t base, size_t n) const {
        const tn::DeviceMesh &m = mesh();
        tn::WalkParams w{};
        w.t = trace_params(base, n);
        w.vars = m.hot;
        w.scene_max = m.bvh.scene_max;
        w.hull_nodes = m.hull_nodes; w.hull_tris = m.hull_tris; w.n_hull_nodes = m.n_hull_nodes; w.n_hull = m.n_hull;
        w.hull_flat = m.hull_nodes + 2 * (size_t)m.n_hull_nodes;
        w.n_hull_leaves = o().hull_flat ? tn::hull_flat_leaves(m.n_hull) : 0u;
        w.n_hull_groups = o().hull_flat ? tn::hull_flat_groups(m.n_hull) : 0u;
        w.ray_base = base;
        w.hull_entry = s().hull_entry.p + base; w.walk_n = s().walk_n.p + base; w.hit_log = s().hit_log.p;
        w.fallback_list = s().fallback_list.p; w.fallback_count = s().fallback_count();
        w.literal_list = o().literal ? s().literal_list.p : nullptr; w.literal_count = s().literal_count();
        w.risk_list = verify_risk() ? s().risk_list.p : nullptr; w.risk_count = s().risk_count();
        w.risk_band = (float)o().risk_band;
        if (binned) { w.order = s().order.p; w.walk_n_item = s().walk_n_item.p; }
        w.cert_ends = o().cert_ends == 2 ? (m.T >= tn::WALK_TET_MIN_TETS ? 1u : 3u) : (uint32_t)o().cert_ends;
        return w;
    }
    tn::WriteParams write_params(size_t base, size_t n) const {
        const tn::Rows r = rows.at(base);
        tn::WriteParams q{};
        q.num_rays = n; q.M = r.M; q.dense_tails = dense_tails ? 1u : 0u;
        q.walk_n = s().walk_n.p + base;
        q.hit_log = s().hit_log.p;
        q.cold = mesh().cold; q.tets = mesh().tets;
        q.out_cells = r.cells; q.out_bary = r.bary; q.out_dist = r.dist; q.out_verts = r.verts;
        if (binned) { q.walk_n = s().walk_n_item.p; q.order = s().order.p; }   // (one chunk: base == 0)
        return q;
    }

    // ---- the launches that two schedules share
    void fill_tails(size_t base, size_t n, uint32_t k_hi) const {   // [ceil32(n_r), k_hi) of the certified rows
        if (!dense_tails) return;
        tn::FillRange f = o().tail;
        f.k_split = k_hi;
        tn::launch_fill(rows.at(base), n, s().walk_n.p + base, f, stream);
    }
    void pair_literal(size_t base, size_t n, hipStream_t st) const {
        if (!o().literal) return;
        tn::launch_postprocess_log(trace_params(base, n), mesh().fidt, s().hit_log.p, s().literal_list.p, s().literal_count(), n, st,
                                   binned ? s().order.p : nullptr);
    }
    void trace_listed(const uint32_t *list, const uint32_t *count, size_t max_items, hipStream_t st) const {   // BVH kernel: whole rows
        tn::TraceParams q = trace_params(0, max_items);
        q.ray_list = list; q.item_count = count;
        tn::launch_trace_general(q, st);
    }

    // Speculative tail fill: a ray of a uniform mesh of T tets crosses at most ~3.45 T^(1/3) faces, so the
    // slots from ceil32(3.6 T^(1/3)) + 32 on are constants in (almost) every row and can be streamed BESIDE the walk
    // (VALU-issue-bound, the fill HBM-write-bound).  The walk crawls beside a saturating write stream, so only as many
    // bytes as its own duration buys are filled that way (profiles/r02p_specfill*.txt, r03a_sched.txt: +1..3 % per frame).
    // Returns the first slot of that fill (a multiple of 32), 0 for none; a row with more segments overwrites its slots.
    uint32_t spec_fill_first_slot() const {
        if (!o().spec_fill || !dense_tails) return 0;
        const uint32_t M = rows.M;
        uint32_t K0 = (((uint32_t)(3.6 * std::cbrt((double)std::max<uint32_t>(mesh().T, 1u))) + 31u) & ~31u) + 32u;
        const uint32_t quarter = (3u * M / 4u) & ~31u, half = (M / 2u) & ~31u;
        // the longer the walk (the more faces per ray), the more bytes its duration hides: the last quarter of the rows on
        // small meshes (C2: 384), the last half where rays reach beyond M/2 - 64 slots (C4: 256 measured best, 320 / 384:
        // -3.6 / -0.6 % instead of -4.9 %).  Meshes whose record tables the L2s no longer hold (the per-tet writer table's
        // threshold): the walk waits for HBM itself and hides less -- the last quarter where the estimate (which carries a
        // 32-slot margin) still allows it (C5, 1M tets: rays reach slot 346 of 384: -0.9 / -1.8 % in two runs, the last half
        // +0.4 %, profiles/r04w_c5_specfill*.txt)
        if (mesh().T >= tn::WALK_TET_MIN_TETS) K0 = K0 > quarter + 32u ? 0u : quarter;
        else K0 = K0 > quarter ? 0u : (K0 + 32u > half ? half : quarter);
        if (o().spec_k0) K0 = o().spec_k0 & ~31u;
        return K0 + 32u > M ? 0u : K0;
    }

    // One chunk, four streams:
    //   caller's: walk (hits -> log; classes) -> segment writer -> tails [ceil32(n), K0) of the certified rows -> joins
    //   `pre`:    tails [K0, M) of ALL rows, from the start of the call (speculative; only when K0 != 0)
    //   `aux`:    BVH re-trace of the handful of fallback rays (one wavefront each, pure latency) + the count
    //             cross-check, from the walk on
    //   `side`:   literal pairing of the logged hits of the rays whose order the walk did not certify, beside the fill
    // Everything that writes rows is ordered behind the speculative fill, so a ray with more than K0 segments (or a
    // literal / fallback row) simply overwrites its slots.  Option "timing": the same kernels, serialised on the caller's
    // stream with a timing event (mark) after each.  Orders that were measured and lost: last section of profiles/HISTORY.md.
    // A binned call puts the key kernel and the sort in front of the walk (same stream; counted with the walk under "timing")
    // and hands `order` to the walk, the writer and the literal pairing; every other launch sees rows and lists in the
    // caller's order and is the same launch as in an unbinned call.
    void run_overlapped() const {
        tn_tracer::Schedule &c = t->sched;
        const bool timing = o().timing;
        const hipStream_t s_pre = timing ? stream : c.pre, s_aux = timing ? stream : c.aux, s_side = timing ? stream : c.side;
        if (timing && !c.tev[0])
            for (hipEvent_t &e : c.tev) TN_HIP(hipEventCreate(&e));
        int mark_i = 0;
        auto mark = [&] { if (timing) TN_HIP(hipEventRecord(c.tev[mark_i++], stream)); };
        const uint32_t K0 = spec_fill_first_slot();
        mark();                                                   // 0: start
        if (K0) {
            TN_HIP(hipEventRecord(c.ev_start, stream));
            TN_HIP(hipStreamWaitEvent(s_pre, c.ev_start, 0));
            tn::FillRange f = o().spec;
            f.k_split = K0;
            tn::launch_fill(rows, R, s().walk_n.p, f, s_pre);
            TN_HIP(hipEventRecord(c.ev_pre, s_pre));
        }
        mark();                                                   // 1: speculative fill
        if (binned)
            tn::launch_ray_order(R, origins, dirs, tn::ray_key_box(mesh().box_lo, mesh().box_hi), s().ray_keys.p, s().ray_iota.p,
                                 s().ray_keys_sorted.p, s().order.p, s().sort_temp.p, s().sort_temp.n, stream);
        // beside a speculative fill the walk's occupancy is limited, so that both stay resident (Options::walk_lds_kb)
        tn::launch_trace_walk(walk_params(0, R), stream, K0 && !timing ? (size_t)o().walk_lds_kb * 1024 : 0);
        mark();                                                   // 2: walk
        TN_HIP(hipEventRecord(c.ev_fork, stream));
        TN_HIP(hipStreamWaitEvent(s_aux, c.ev_fork, 0));
        if (K0) {   // everything that writes rows comes after the speculative fill
            TN_HIP(hipStreamWaitEvent(s_aux, c.ev_pre, 0));
            TN_HIP(hipStreamWaitEvent(stream, c.ev_pre, 0));
        }
        trace_listed(s().fallback_list.p, s().fallback_count(), R, s_aux);
        mark();                                                   // 3: BVH re-trace of the fallback rays
        if (o().verify_stride) {
            // the count cross-check beside the writer and the fill (late form): mismatching rays -> verify_list ...
            tn::launch_verify_counts(trace_params(0, R), o().verify_stride, s().walk_n.p, s().verify_list.p, s().verify_count(), 0,
                                     s_aux, true, o().verify_inject);
            // ... and EVERY certified ray of the risk classes (inside the wide band of a guard: DESIGN.md section 2)
            if (verify_risk())
                tn::launch_verify_counts(trace_params(0, R), o().verify_stride, s().walk_n.p, s().verify_list.p, s().verify_count(), 0,
                                         s_aux, true, false, s().risk_list.p, s().risk_count(), R);
        }
        mark();                                                   // 4: count cross-check
        TN_HIP(hipEventRecord(c.ev_aux, s_aux));
        // the segment writer is enqueued BEFORE the side stream's kernel: its grid is sized for the worst case (the
        // count lives on the device) and would otherwise take every wave slot first
        tn::launch_write_segments(write_params(0, R), stream, o().writer_blocks);
        mark();                                                   // 5: segment writer
        TN_HIP(hipEventRecord(c.ev_seg, stream));
        TN_HIP(hipStreamWaitEvent(s_side, c.ev_seg, 0));     // literal pairing beside the bandwidth-bound fill, not
        pair_literal(0, R, s_side);                          // beside the latency-bound writer (r02f_sched_sweep.txt)
        mark();                                                   // 6: literal pairing of the logged hits
        fill_tails(0, R, K0 ? K0 : rows.M);
        mark();                                                   // 7: tail fill
        TN_HIP(hipEventRecord(c.ev_join, s_side));
        TN_HIP(hipStreamWaitEvent(stream, c.ev_join, 0));
        TN_HIP(hipStreamWaitEvent(stream, c.ev_aux, 0));
        // rows of the rays whose count differed (none, as far as anyone has seen): whole rows, after every other writer
        // of the call.  The count lives on the device: a small grid that finds it 0 and exits
        if (o().verify_stride) trace_listed(s().verify_list.p, s().verify_count(), 64, stream);
        mark();                                                   // 8: end
        c.tev_valid = timing;
    }

    // Several chunks: each walked, checked, written, filled and paired serially on the caller's stream (the next chunk's
    // walk reuses the log), then one BVH launch over the fallback rays of all chunks.
    void run_chunked(size_t chunk) const {
        for (size_t base = 0; base < R; base += chunk) {
            const size_t n = std::min(R - base, chunk);
            TN_HIP(hipMemsetAsync(s().literal_count(), 0, sizeof(uint32_t), stream));
            TN_HIP(hipMemsetAsync(s().risk_count(), 0, sizeof(uint32_t), stream));
            const tn::WalkParams w = walk_params(base, n);
            tn::launch_trace_walk(w, stream, 0);
            if (o().verify_stride) {   // early form: before anything that reads walk_n / the fallback list
                tn::launch_verify_counts(w.t, o().verify_stride, w.walk_n, w.fallback_list, w.fallback_count, base, stream, false,
                                         o().verify_inject);
                if (verify_risk())
                    tn::launch_verify_counts(w.t, o().verify_stride, w.walk_n, w.fallback_list, w.fallback_count, base, stream, false,
                                             false, s().risk_list.p, s().risk_count(), n);
            }
            tn::launch_write_segments(write_params(base, n), stream, o().writer_blocks);
            fill_tails(base, n, rows.M);
            pair_literal(base, n, stream);
        }
        trace_listed(s().fallback_list.p, s().fallback_count(), R, stream);
    }

    // Small batch (below walk_min_rays): one wavefront per ray through the BVH.  Latency-bound, so every ray should be
    // resident at once: LDS hit arrays sized for the hits a ray of THIS mesh is expected to have (a uniform mesh of T
    // tets: at most ~3.45 T^(1/3) faces on a ray), rays with more go through a second launch with the
    // full M-entry arrays.
    void run_small_batch() const {
        uint32_t C = 64;
        const double expect = 3.6 * std::cbrt((double)std::max<uint32_t>(mesh().T, 1u));
        while (C < expect && C < rows.M) C <<= 1;
        if (o().lds_cap) C = o().lds_cap;
        tn::TraceParams p = trace_params(0, R);
        if (o().small_lds && C < rows.M) {
            s().reserve(R, 0, false, false);
            tn::TraceParams p1 = p;
            p1.lds_cap = C; p1.overflow_list = s().fallback_list.p; p1.overflow_count = s().fallback_count();
            tn::launch_trace_general(p1, stream);
            p.ray_list = s().fallback_list.p;
            p.item_count = s().fallback_count();
        }
        tn::launch_trace_general(p, stream);
    }
};

}  // namespace

extern "C" {

int tn_tracer_create(int device, tn_tracer_t *out) {
    return guarded([&] {
        if (!out) throw tn::Error("out is null");
        int count = 0;
        TN_HIP(hipGetDeviceCount(&count));
        if (device < 0 || device >= count) throw tn::Error("The device argument must be a CUDA device.");
        DeviceGuard g(device);
        auto t = std::make_unique<tn_tracer>();
        t->device = device;
        t->opt.use_walk = tn::env_flag("TETRANERF_HIP_WALK", true) ? 1 : 0;
        t->opt.gpu_build = tn::env_flag("TETRANERF_HIP_GPU_BUILD", true);
        t->opt.bin_rays = tn::env_flag("TETRANERF_HIP_BIN_RAYS", false);
        t->scratch.stats.alloc(tn::N_STATS + tn_tracer::Scratch::N_CTR);
        TN_HIP(hipMemset(t->scratch.stats.p, 0, tn_tracer::Scratch::stats_bytes()));
        tn_tracer::Schedule &c = t->sched;
        // the side streams carry the few rays the walk does not certify: lowest priority, so that the dispatcher
        // hands wave slots to the main stream's kernels first when both have blocks waiting
        int least = 0, greatest = 0;
        TN_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        TN_HIP(hipStreamCreateWithPriority(&c.side, hipStreamNonBlocking, least));
        TN_HIP(hipStreamCreateWithPriority(&c.aux, hipStreamNonBlocking, least));
        TN_HIP(hipStreamCreateWithFlags(&c.pre, hipStreamNonBlocking));
        for (hipEvent_t *e : {&c.ev_fork, &c.ev_join, &c.ev_start, &c.ev_pre, &c.ev_seg, &c.ev_aux})
            TN_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        *out = t.release();
    });
}

int tn_tracer_destroy(tn_tracer_t tracer) {
    return guarded([&] {
        if (!tracer) return;
        DeviceGuard g(tracer->device);
        (void)hipDeviceSynchronize();
        const tn_tracer::Schedule &c = tracer->sched;
        for (hipStream_t st : {c.side, c.aux, c.pre})
            if (st) (void)hipStreamDestroy(st);
        for (hipEvent_t e : {c.ev_fork, c.ev_join, c.ev_start, c.ev_pre, c.ev_seg, c.ev_aux})
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : c.tev)
            if (e) (void)hipEventDestroy(e);
        delete tracer;
    });
}

int tn_load_tetrahedra(tn_tracer_t tracer, size_t V, size_t T, const float *xyz, const uint32_t *cells,
                       void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        DeviceGuard g(t->device);
        hipStream_t stream = (hipStream_t)stream_;
        if ((V && !xyz) || (T && !cells)) throw tn::Error("xyz / cells must not be null");
        if (V >= 0xFFFFFFFFull || T >= 0x0FFFFFFFull) throw tn::Error("mesh too large (uint32 ids)");
        // either build: refused here, ahead of the first allocation and launch (a mesh without cells has no face, no record
        // and no tree for the trace kernels to read)
        if (T == 0) throw tn::Error("load_tetrahedra needs at least one tetrahedron");
        tn_tracer::Mesh &b = t->mesh;
        b.loaded = false;
        b.host.faces.clear(); b.host.face_tets.clear();
        b.refit.release();
        b.device_built = t->opt.gpu_build;
        BuildCounts n;
        if (b.device_built) {
            // everything is built on the device from the caller's buffers (tn_build.hip)
            tn::BuildInfo bi;
            tn::device_build(V, T, xyz, cells, stream,
                             tn::BuildTargets{b.faces, b.face_tets, b.vars, b.hull_nodes, b.hull_tris, b.bvh}, bi, t->opt.leaf_width,
                             t->opt.refit_tables ? &b.refit : nullptr);
            check_bvh_depth(bi.max_stack);
            b.host.scene_max = bi.scene_max;
            b.bvh_max_stack = bi.max_stack;
            n = BuildCounts{bi.F, bi.n_hull, bi.n_hull_nodes};
        } else {
            n = build_on_host(b, t->opt.leaf_width, V, T, xyz, cells, stream);
        }

        tn::DeviceMesh &m = b.view;
        m.xyz = xyz; m.cells = cells;
        m.V = (uint32_t)V; m.T = (uint32_t)T; m.F = (uint32_t)n.F;
        m.faces = b.faces.p; m.face_tets = b.face_tets.p;
        m.bvh = b.bvh.view;
        {   // de-interleave the records by consumer (tn_common.h: WalkHot / WalkTet / WalkFid)
            const size_t n4 = b.vars.n;
            const bool per_tet = t->opt.writer_table ? t->opt.writer_table == 2 : n4 / 4 >= tn::WALK_TET_MIN_TETS;
            b.hot.alloc(n4); b.fidt.alloc(n4);
            b.cold.release(); b.tets.release();
            if (per_tet) b.tets.alloc(n4 / 4); else b.cold.alloc(n4);
            tn::launch_split_walk_records(n4, b.vars.p, b.hot.p, per_tet ? nullptr : b.cold.p, per_tet ? b.tets.p : nullptr,
                                          b.fidt.p, stream);
            TN_HIP(hipStreamSynchronize(stream));
            b.vars.release();
        }
        m.hot = b.hot.p; m.cold = b.cold.n ? b.cold.p : nullptr; m.tets = b.tets.n ? b.tets.p : nullptr; m.fidt = b.fidt.p;
        m.n_hull = (uint32_t)n.n_hull;
        m.hull_nodes = reinterpret_cast<const float4 *>(b.hull_nodes.p);
        m.hull_tris = reinterpret_cast<const float4 *>(b.hull_tris.p);
        m.n_hull_nodes = (uint32_t)n.n_hull_nodes;
        tn::mesh_box(V, T, xyz, cells, m.box_lo, m.box_hi, stream);   // one kernel for both builds: the same six numbers
        b.loaded = true;
    });
}

int tn_update_vertices(tn_tracer_t tracer, size_t V, const float *xyz, void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        tn_tracer::Mesh &b = t->mesh;
        if (!b.loaded) throw tn::Error("tn_update_vertices: no mesh is loaded; call load_tetrahedra first");
        if (!b.device_built)
            throw tn::Error("tn_update_vertices: the mesh was built on the host (option \"gpu_build\" = 0); the refit is part of the "
                            "device build: set \"gpu_build\" = 1 and load again, or reload after every move");
        if (!b.refit.valid)
            throw tn::Error("tn_update_vertices: the mesh was loaded without the refit tables; set option \"refit_tables\" = 1 "
                            "(Python: load_tetrahedra(..., refittable=True)) and load again");
        if (V != b.view.V)
            throw tn::Error("tn_update_vertices: " + std::to_string(V) + " vertices given, the loaded mesh has " +
                            std::to_string(b.view.V) + "; a mesh with other vertices or cells needs load_tetrahedra");
        if (!xyz) throw tn::Error("tn_update_vertices: xyz must not be null");
        DeviceGuard g(t->device);
        hipStream_t stream = (hipStream_t)stream_;
        tn::DeviceMesh &m = b.view;
        float smax = 0.f;
        tn::device_refit(V, m.T, xyz, m.cells, stream, tn::RefitTargets{b.hot.p, b.faces.p, b.hull_nodes, b.hull_tris, b.bvh}, b.refit,
                         smax, m.box_lo, m.box_hi);
        // what is cached by value: max |coordinate| (the BVH view every parameter block copies) and the key box of binned calls
        b.host.scene_max = smax;
        m.bvh = b.bvh.view;
        m.xyz = xyz;
    });
}

size_t tn_refit_table_bytes(tn_tracer_t tracer) {
    return tracer && tracer->mesh.loaded && tracer->mesh.refit.valid ? tracer->mesh.refit.bytes() : 0;
}

namespace {
// the checks both vertex-guard entries share (nothing is touched when one fails)
void check_guard_mesh(tn_tracer *t, const char *who, size_t V) {
    tn_tracer::Mesh &b = t->mesh;
    if (!b.loaded) throw tn::Error(std::string(who) + ": no mesh is loaded; call load_tetrahedra first");
    if (V != b.view.V)
        throw tn::Error(std::string(who) + ": " + std::to_string(V) + " vertices given, the loaded mesh has " + std::to_string(b.view.V));
}
}  // namespace

int tn_tet_quality(tn_tracer_t tracer, size_t V, const float *xyz, float *width, int8_t *orient, float *star_width, void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        check_guard_mesh(t, "tn_tet_quality", V);
        const tn::DeviceMesh &m = t->mesh.view;
        if (!xyz) throw tn::Error("tn_tet_quality: xyz must not be null");
        DeviceGuard g(t->device);
        tn::launch_tet_quality(V, m.T, m.cells, xyz, width, orient, star_width, (hipStream_t)stream_);
    });
}

int tn_limit_vertex_step(tn_tracer_t tracer, size_t V, const float *xyz_old, float *xyz_new, float fraction, float *star_width,
                         uint32_t *counters, uint32_t flags, void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        check_guard_mesh(t, "tn_limit_vertex_step", V);
        const tn::DeviceMesh &m = t->mesh.view;
        if (!xyz_old || !xyz_new || !star_width || !counters)
            throw tn::Error("tn_limit_vertex_step: xyz_old, xyz_new, star_width and counters must not be null");
        if (!(fraction > 0.f && fraction <= 0.45f))   // NaN fails both
            throw tn::Error("tn_limit_vertex_step: fraction must be in (0, 0.45]: the bound is proved for moves below half a width, "
                            "and 0.45 leaves room for the rounding of the new coordinates");
        if (flags & ~(uint32_t)TN_LIMIT_STEP_NO_VERIFY) throw tn::Error("tn_limit_vertex_step: unknown flags");
        DeviceGuard g(t->device);
        tn::launch_limit_vertex_step(V, m.T, m.cells, xyz_old, xyz_new, fraction, star_width, counters,
                                     !(flags & TN_LIMIT_STEP_NO_VERIFY), (hipStream_t)stream_);
    });
}

int tn_delaunay_check(tn_tracer_t tracer, size_t V, const float *xyz, uint32_t *counters, int8_t *face_state, uint8_t *tet_violations,
                      void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        check_guard_mesh(t, "tn_delaunay_check", V);
        const tn::DeviceMesh &m = t->mesh.view;
        if (!xyz || !counters) throw tn::Error("tn_delaunay_check: xyz and counters must not be null");
        if ((uintptr_t)tet_violations & 3u)
            throw tn::Error("tn_delaunay_check: tet_violations must be 4-byte aligned (its bytes are counted through 32-bit atomics)");
        DeviceGuard g(t->device);
        tn::launch_delaunay_check(m.T, m.F, m.cells, m.face_tets, xyz, counters, face_state, tet_violations, (hipStream_t)stream_);
    });
}

int tn_remap_tet_values(size_t V, size_t num_old_cells, const uint32_t *old_cells, const float *old_values, size_t num_new_cells,
                        const uint32_t *new_cells, float *new_values, float *star_max, void *stream_) {
    return guarded([&] {
        if (V >= 0xFFFFFFFFull) throw tn::Error("tn_remap_tet_values: too many vertices (uint32 ids)");
        if ((num_old_cells && (!old_cells || !old_values)) || (num_new_cells && (!new_cells || !new_values)) || (V && !star_max))
            throw tn::Error("tn_remap_tet_values: old_cells, old_values, new_cells, new_values and star_max must not be null");
        tn::launch_remap_tet_values(V, num_old_cells, old_cells, old_values, num_new_cells, new_cells, new_values, star_max,
                                    (hipStream_t)stream_);
    });
}

namespace {
// the checks both isosurface entries share (nothing is touched when one fails)
void check_isosurface_args(const char *who, size_t V, size_t T, const uint32_t *cells, const float *values, float level) {
    if (V >= 0xFFFFFFFFull) throw tn::Error(std::string(who) + ": too many vertices (uint32 ids)");
    if (T >= tn::iso::MAX_TETS) throw tn::Error(std::string(who) + ": num_cells must be below 2^30");
    if (!tn::iso::in_range(level)) throw tn::Error(std::string(who) + ": level must be finite and below 2^126 in magnitude");
    if (T && (!cells || (V && !values))) throw tn::Error(std::string(who) + ": cells and values must not be null");
}
}  // namespace

int tn_isosurface_count(size_t V, size_t T, const uint32_t *cells, const float *values, float level, const uint8_t *tet_mask,
                        uint32_t *tri_offsets, uint32_t *ref_offsets, void *stream_) {
    return guarded([&] {
        check_isosurface_args("tn_isosurface_count", V, T, cells, values, level);
        if (!tri_offsets || !ref_offsets) throw tn::Error("tn_isosurface_count: tri_offsets and ref_offsets must not be null");
        tn::launch_isosurface_count(V, T, cells, values, level, tet_mask, tri_offsets, ref_offsets, (hipStream_t)stream_);
    });
}

int tn_isosurface_emit(size_t V, size_t T, const float *xyz, const uint32_t *cells, const float *values, float level,
                       const uint8_t *tet_mask, const uint32_t *tri_offsets, const uint32_t *ref_offsets, size_t num_triangles,
                       size_t num_refs, uint32_t *triangles, uint32_t *triangle_tets, uint32_t *edge_vertices, float *edge_t,
                       float *positions, uint32_t *num_out_vertices, void *stream_) {
    return guarded([&] {
        check_isosurface_args("tn_isosurface_emit", V, T, cells, values, level);
        if (num_triangles > 2 * T || num_refs > 4 * T)
            throw tn::Error("tn_isosurface_emit: num_triangles / num_refs exceed what num_cells tetrahedra can emit (2 / 4 each)");
        if (!num_out_vertices || (T && (!tri_offsets || !ref_offsets)) || (T && V && !xyz) ||
            (num_triangles && (!triangles || !triangle_tets)) || (num_refs && (!edge_vertices || !edge_t || !positions)))
            throw tn::Error("tn_isosurface_emit: a null pointer beside a non-zero count");
        tn::launch_isosurface_emit(V, T, xyz, cells, values, level, tet_mask, tri_offsets, ref_offsets, num_triangles, num_refs,
                                   triangles, triangle_tets, edge_vertices, edge_t, positions, num_out_vertices,
                                   (hipStream_t)stream_);
    });
}

namespace {
// the checks the four refinement entries share (nothing is touched when one fails)
void check_refine_args(const char *who, size_t V, size_t N, float level, uint32_t round) {
    const std::string w(who);
    if (V >= 0xFFFFFFFFull) throw tn::Error(w + ": too many vertices (uint32 ids)");
    if (N > 4 * (tn::iso::MAX_TETS - 1)) throw tn::Error(w + ": more surface vertices than 2^30 tetrahedra can emit");
    if (!tn::iso::in_range(level)) throw tn::Error(w + ": level must be finite and below 2^126 in magnitude");
    if (round >= tn::iso::REFINE_MAX_ROUNDS) throw tn::Error(w + ": round must be below 8 (at most 8 rounds of refinement)");
}
void check_refine_pointer(const char *who, const void *p, size_t alignment, const char *name) {
    if (!p) throw tn::Error(std::string(who) + ": " + name + " must not be null");
    if ((uintptr_t)p & (alignment - 1))
        throw tn::Error(std::string(who) + ": " + name + " must be " + std::to_string(alignment) + "-byte aligned");
}
}  // namespace

int tn_isosurface_refine_begin(size_t V, size_t N, const uint32_t *edge_vertices, const float *values, float level,
                               float *brackets, uint8_t *frozen, void *stream_) {
    return guarded([&] {
        const char *who = "tn_isosurface_refine_begin";
        check_refine_args(who, V, N, level, 0);
        if (N == 0) return;
        check_refine_pointer(who, edge_vertices, 8, "edge_vertices");
        check_refine_pointer(who, brackets, 16, "brackets");
        check_refine_pointer(who, frozen, 1, "frozen");
        if (V && !values) throw tn::Error("tn_isosurface_refine_begin: values must not be null");
        tn::launch_isosurface_refine_begin(V, N, edge_vertices, values, level, brackets, frozen, (hipStream_t)stream_);
    });
}

int tn_isosurface_refine_points(size_t V, size_t N, uint32_t round, const uint32_t *edge_vertices, const float *brackets,
                                const uint8_t *frozen, uint32_t *vertex_indices, float *barycentric, void *stream_) {
    return guarded([&] {
        const char *who = "tn_isosurface_refine_points";
        check_refine_args(who, V, N, 0.f, round);
        if (N == 0) return;
        if (V == 0) throw tn::Error("tn_isosurface_refine_points: surface vertices without mesh vertices (the candidates name vertex 0)");
        check_refine_pointer(who, edge_vertices, 8, "edge_vertices");
        check_refine_pointer(who, brackets, 16, "brackets");
        check_refine_pointer(who, frozen, 1, "frozen");
        check_refine_pointer(who, vertex_indices, 16, "vertex_indices");
        check_refine_pointer(who, barycentric, 4, "barycentric");
        tn::launch_isosurface_refine_points(N, edge_vertices, brackets, frozen, vertex_indices, barycentric, (hipStream_t)stream_);
    });
}

int tn_isosurface_refine_select(size_t N, uint32_t round, float level, const float *densities, float *brackets, uint8_t *frozen,
                                void *stream_) {
    return guarded([&] {
        const char *who = "tn_isosurface_refine_select";
        check_refine_args(who, 0, N, level, round);
        if (N == 0) return;
        check_refine_pointer(who, densities, 4, "densities");
        check_refine_pointer(who, brackets, 16, "brackets");
        check_refine_pointer(who, frozen, 1, "frozen");
        tn::launch_isosurface_refine_select(N, level, densities, brackets, frozen, (hipStream_t)stream_);
    });
}

int tn_isosurface_refine_vertices(size_t V, size_t N, const float *xyz, const uint32_t *edge_vertices, const float *brackets,
                                  float level, float *edge_t, float *positions, void *stream_) {
    return guarded([&] {
        const char *who = "tn_isosurface_refine_vertices";
        check_refine_args(who, V, N, level, 0);
        if (N == 0) return;
        check_refine_pointer(who, edge_vertices, 8, "edge_vertices");
        check_refine_pointer(who, brackets, 16, "brackets");
        check_refine_pointer(who, edge_t, 4, "edge_t");
        check_refine_pointer(who, positions, 4, "positions");
        if (V && !xyz) throw tn::Error("tn_isosurface_refine_vertices: xyz must not be null");
        tn::launch_isosurface_refine_vertices(V, N, xyz, edge_vertices, brackets, level, edge_t, positions, (hipStream_t)stream_);
    });
}

namespace {
// the size checks the split entries share (nothing is touched when one fails); K = the new vertices the call may write
void check_split_sizes(const char *who, size_t V, size_t T, size_t K) {
    const std::string w(who);
    if (K > T) throw tn::Error(w + ": num_new exceeds num_cells (a tetrahedron is split at most once)");
    if (V >= 0xFFFFFFFFull || V + K >= 0xFFFFFFFFull) throw tn::Error(w + ": too many vertices (uint32 ids)");
    if (T >= tn::split::MAX_CELLS || T + 3 * K >= tn::split::MAX_CELLS) throw tn::Error(w + ": num_cells + 3 num_new must be below 2^30");
}
}  // namespace

int tn_split_count(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint8_t *select, uint32_t *offsets,
                   uint32_t *counters, void *stream_) {
    return guarded([&] {
        check_split_sizes("tn_split_count", V, T, 0);
        if (!offsets || !counters || (T && (!cells || !select)) || (T && V && !xyz))
            throw tn::Error("tn_split_count: a null pointer beside a non-zero count");
        tn::launch_split_count(V, T, xyz, cells, select, offsets, counters, (hipStream_t)stream_);
    });
}

int tn_split_emit(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint32_t *offsets, size_t num_new,
                  float *xyz_out, uint32_t *cells_out, uint32_t *cell_parent, uint32_t *vertex_parents, void *stream_) {
    return guarded([&] {
        check_split_sizes("tn_split_emit", V, T, num_new);
        if ((T && (!cells || !offsets || !cells_out || !cell_parent)) || (V && (!xyz || !xyz_out)) ||
            (num_new && (!xyz_out || !vertex_parents)))
            throw tn::Error("tn_split_emit: a null pointer beside a non-zero count");
        tn::launch_split_emit(V, T, xyz, cells, offsets, num_new, xyz_out, cells_out, cell_parent, vertex_parents,
                              (hipStream_t)stream_);
    });
}

int tn_split_vertex_rows(size_t rows, size_t V, size_t K, const float *values, const float *values_vm,
                         const uint32_t *vertex_parents, uint32_t new_mode, float *out, float *out_vm, void *stream_) {
    return guarded([&] {
        if (rows == 0) throw tn::Error("tn_split_vertex_rows: rows must not be 0");
        if (rows >= 0xFFFFFFFFull) throw tn::Error("tn_split_vertex_rows: too many rows");
        if (new_mode > tn::split::MODE_ZERO) throw tn::Error("tn_split_vertex_rows: unknown new_mode (0 = mean of the parents, 1 = zeros)");
        if (V >= 0xFFFFFFFFull || V + K >= 0xFFFFFFFFull) throw tn::Error("tn_split_vertex_rows: too many vertices (uint32 ids)");
        if ((V && !values) || (K && !vertex_parents) || (V + K && !out))
            throw tn::Error("tn_split_vertex_rows: a null pointer beside a non-zero count");
        tn::launch_split_vertex_rows(rows, V, K, values, values_vm, vertex_parents, new_mode, out, out_vm, (hipStream_t)stream_);
    });
}

namespace {
// the size and pointer checks both count entries share (nothing is touched when one fails)
void check_prune_count(const char *who, size_t V, size_t T, size_t F, const void *cells, const void *faces, const void *face_tets,
                       const void *dead, const void *offsets, const void *counters) {
    const std::string w(who);
    if (V >= 0xFFFFFFFFull) throw tn::Error(w + ": too many vertices (uint32 ids)");
    if (T >= tn::split::MAX_CELLS) throw tn::Error(w + ": num_cells must be below 2^30");
    if (F >= 0xFFFFFFFFull) throw tn::Error(w + ": too many faces");
    if (!offsets || !counters || (T && (!cells || !dead)) || (F && (!faces || !face_tets)))
        throw tn::Error(w + ": a null pointer beside a non-zero count");
}
}  // namespace

int tn_prune_count(tn_tracer_t tracer, size_t V, const uint8_t *dead, const uint8_t *vertex_select, uint32_t *offsets,
                   uint32_t *counters, void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        check_guard_mesh(t, "tn_prune_count", V);
        const tn::DeviceMesh &m = t->mesh.view;
        check_prune_count("tn_prune_count", V, m.T, m.F, m.cells, m.faces, m.face_tets, dead, offsets, counters);
        DeviceGuard g(t->device);
        tn::launch_prune_count(V, m.T, m.cells, m.F, m.faces, m.face_tets, dead, vertex_select, offsets, counters, (hipStream_t)stream_);
    });
}

int tn_prune_count_tables(int device, size_t V, size_t T, const uint32_t *cells, size_t F, const uint32_t *faces,
                          const uint32_t *face_tets, const uint8_t *dead, const uint8_t *vertex_select, uint32_t *offsets,
                          uint32_t *counters, void *stream_) {
    return guarded([&] {
        check_prune_count("tn_prune_count_tables", V, T, F, cells, faces, face_tets, dead, offsets, counters);
        DeviceGuard g(device);
        tn::launch_prune_count(V, T, cells, F, faces, face_tets, dead, vertex_select, offsets, counters, (hipStream_t)stream_);
    });
}

int tn_prune_emit(size_t V, const float *xyz, const uint32_t *offsets, size_t num_kept, uint32_t *new_id, uint32_t *kept_ids,
                  float *xyz_out, void *stream_) {
    return guarded([&] {
        if (V >= 0xFFFFFFFFull) throw tn::Error("tn_prune_emit: too many vertices (uint32 ids)");
        if (num_kept > V) throw tn::Error("tn_prune_emit: num_kept exceeds num_vertices");
        if ((V && (!xyz || !offsets || !new_id)) || (num_kept && (!kept_ids || !xyz_out)))
            throw tn::Error("tn_prune_emit: a null pointer beside a non-zero count");
        tn::launch_prune_emit(V, xyz, offsets, num_kept, new_id, kept_ids, xyz_out, (hipStream_t)stream_);
    });
}

int tn_prune_vertex_rows(size_t rows, size_t V, size_t num_kept, const float *values, const float *values_vm, const uint32_t *kept_ids,
                         float *out, float *out_vm, void *stream_) {
    return guarded([&] {
        if (rows == 0) throw tn::Error("tn_prune_vertex_rows: rows must not be 0");
        if (rows >= 0xFFFFFFFFull) throw tn::Error("tn_prune_vertex_rows: too many rows");
        if (V >= 0xFFFFFFFFull) throw tn::Error("tn_prune_vertex_rows: too many vertices (uint32 ids)");
        if (num_kept > V) throw tn::Error("tn_prune_vertex_rows: num_kept exceeds num_vertices");
        if (num_kept && (!kept_ids || !out || (!values && !values_vm)))
            throw tn::Error("tn_prune_vertex_rows: a null pointer beside a non-zero count");
        tn::launch_prune_vertex_rows(rows, V, num_kept, values, values_vm, kept_ids, out, out_vm, (hipStream_t)stream_);
    });
}

namespace {
// the checks both count entries of the edge split share (nothing is touched when one fails)
void check_edge_split_count(const char *who, size_t V, size_t T, size_t F, const void *xyz, const void *cells, const void *select,
                            const void *faces, const void *face_tets, const void *tet_offsets, const void *tet_edge,
                            const void *bisected, const void *edge_vertices, const void *counters) {
    const std::string w(who);
    if (V >= 0xFFFFFFFFull) throw tn::Error(w + ": too many vertices (uint32 ids)");
    if (T >= tn::esplit::MAX_CELLS) throw tn::Error(w + ": num_cells must be below 2^30");
    if (F >= 0xFFFFFFFFull) throw tn::Error(w + ": too many faces");
    if (!tet_offsets || !counters || (T && (!cells || !select || !tet_edge || !bisected || !edge_vertices)) || (T && V && !xyz) ||
        (F && (!faces || !face_tets)))
        throw tn::Error(w + ": a null pointer beside a non-zero count");
}
}  // namespace

int tn_edge_split_count_tables(int device, size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint8_t *select,
                               size_t F, const uint32_t *faces, const uint32_t *face_tets, uint32_t *tet_offsets, uint32_t *tet_edge,
                               uint8_t *bisected, uint32_t *edge_vertices, uint32_t *counters, void *stream_) {
    return guarded([&] {
        check_edge_split_count("tn_edge_split_count_tables", V, T, F, xyz, cells, select, faces, face_tets, tet_offsets, tet_edge,
                               bisected, edge_vertices, counters);
        DeviceGuard g(device);
        tn::launch_edge_split_count(V, T, xyz, cells, select, F, faces, face_tets, tet_offsets, tet_edge, bisected, edge_vertices,
                                    counters, (hipStream_t)stream_);
    });
}

int tn_edge_split_count(tn_tracer_t tracer, size_t V, const float *xyz, const uint8_t *select, uint32_t *tet_offsets,
                        uint32_t *tet_edge, uint8_t *bisected, uint32_t *edge_vertices, uint32_t *counters, void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        check_guard_mesh(t, "tn_edge_split_count", V);
        const tn::DeviceMesh &m = t->mesh.view;
        check_edge_split_count("tn_edge_split_count", V, m.T, m.F, xyz, m.cells, select, m.faces, m.face_tets, tet_offsets, tet_edge,
                               bisected, edge_vertices, counters);
        DeviceGuard g(t->device);
        tn::launch_edge_split_count(V, m.T, xyz, m.cells, select, m.F, m.faces, m.face_tets, tet_offsets, tet_edge, bisected,
                                    edge_vertices, counters, (hipStream_t)stream_);
    });
}

int tn_edge_split_emit(size_t V, size_t T, const float *xyz, const uint32_t *cells, const uint32_t *tet_offsets,
                       const uint32_t *tet_edge, const uint32_t *edge_vertices, size_t num_new, size_t num_rows, float *xyz_out,
                       uint32_t *cells_out, uint32_t *cell_parent, uint32_t *vertex_parents, void *stream_) {
    return guarded([&] {
        const std::string w("tn_edge_split_emit");
        if (num_new > T || num_rows > T) throw tn::Error(w + ": num_new or num_rows exceeds num_cells (a tetrahedron is bisected at most once)");
        if (V >= 0xFFFFFFFFull || V + num_new >= 0xFFFFFFFFull) throw tn::Error(w + ": too many vertices (uint32 ids)");
        if (T >= tn::esplit::MAX_CELLS || T + num_rows >= tn::esplit::MAX_CELLS) throw tn::Error(w + ": num_cells + num_rows must be below 2^30");
        if ((T && (!cells || !tet_offsets || !tet_edge || !cells_out || !cell_parent)) || (V && (!xyz || !xyz_out)) ||
            (num_new && (!edge_vertices || !xyz_out || !vertex_parents)) || (num_rows && !edge_vertices))
            throw tn::Error(w + ": a null pointer beside a non-zero count");
        tn::launch_edge_split_emit(V, T, xyz, cells, tet_offsets, tet_edge, edge_vertices, num_new, num_rows, xyz_out, cells_out,
                                   cell_parent, vertex_parents, (hipStream_t)stream_);
    });
}

namespace {
// the checks both count entries of the flip share (nothing is touched when one fails)
void check_flip_count(const char *who, size_t V, size_t T, size_t F, const void *xyz, const void *cells, const void *faces,
                      const void *face_tets, const void *tet_offsets, const void *tet_flip, const void *flipped, const void *face_flip,
                      const void *counters) {
    const std::string w(who);
    if (V >= 0xFFFFFFFFull) throw tn::Error(w + ": too many vertices (uint32 ids)");
    if (T >= tn::flip::MAX_CELLS) throw tn::Error(w + ": num_cells must be below 2^30");
    if (F >= 0xFFFFFFFFull) throw tn::Error(w + ": too many faces");
    if (!tet_offsets || !counters || (T && (!cells || !tet_flip || !flipped)) || (T && F && V && !xyz) ||
        (F && (!faces || !face_tets || !face_flip)))
        throw tn::Error(w + ": a null pointer beside a non-zero count");
}
}  // namespace

int tn_flip_count_tables(int device, size_t V, size_t T, const float *xyz, const uint32_t *cells, size_t F, const uint32_t *faces,
                         const uint32_t *face_tets, uint32_t *tet_offsets, uint32_t *tet_flip, uint8_t *flipped, uint32_t *face_flip,
                         uint32_t *counters, void *stream_) {
    return guarded([&] {
        check_flip_count("tn_flip_count_tables", V, T, F, xyz, cells, faces, face_tets, tet_offsets, tet_flip, flipped, face_flip, counters);
        DeviceGuard g(device);
        tn::launch_flip_count(V, T, xyz, cells, F, faces, face_tets, tet_offsets, tet_flip, flipped, face_flip, counters,
                              (hipStream_t)stream_);
    });
}

int tn_flip_count(tn_tracer_t tracer, size_t V, const float *xyz, uint32_t *tet_offsets, uint32_t *tet_flip, uint8_t *flipped,
                  uint32_t *face_flip, uint32_t *counters, void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        check_guard_mesh(t, "tn_flip_count", V);
        const tn::DeviceMesh &m = t->mesh.view;
        const float *positions = xyz ? xyz : m.xyz;   // null: the loaded vertices
        check_flip_count("tn_flip_count", V, m.T, m.F, positions, m.cells, m.faces, m.face_tets, tet_offsets, tet_flip, flipped, face_flip,
                         counters);
        DeviceGuard g(t->device);
        tn::launch_flip_count(V, m.T, positions, m.cells, m.F, m.faces, m.face_tets, tet_offsets, tet_flip, flipped, face_flip, counters,
                              (hipStream_t)stream_);
    });
}

namespace {
// the checks and the launch both emit entries of the flip share (nothing is touched when a check fails)
void checked_flip_emit(const char *who, size_t T, const uint32_t *cells, size_t F, const uint32_t *faces, const uint32_t *face_tets,
                       const uint32_t *tet_offsets, const uint32_t *tet_flip, const uint32_t *face_flip, size_t num_23, size_t num_32,
                       uint32_t *cells_out, uint32_t *cell_sources, void *stream_) {
    const std::string w(who);
    if (num_23 > F || num_32 > F) throw tn::Error(w + ": num_23 or num_32 exceeds num_faces (a face is flipped at most once)");
    if (2 * num_23 + 3 * num_32 > T) throw tn::Error(w + ": the flips need more rows than num_cells (accepted flips share no row)");
    if (T >= tn::flip::MAX_CELLS || T + num_23 >= tn::flip::MAX_CELLS) throw tn::Error(w + ": num_cells + num_23 must be below 2^30");
    if (F >= 0xFFFFFFFFull) throw tn::Error(w + ": too many faces");
    if ((T && (!cells || !tet_offsets || !tet_flip)) || (T + num_23 > num_32 && (!cells_out || !cell_sources)) ||
        (F && (!faces || !face_tets || !face_flip)))
        throw tn::Error(w + ": a null pointer beside a non-zero count");
    tn::launch_flip_emit(T, cells, F, faces, face_tets, tet_offsets, tet_flip, face_flip, num_23, num_32, cells_out, cell_sources,
                         (hipStream_t)stream_);
}
}  // namespace

int tn_flip_emit(size_t T, const uint32_t *cells, size_t F, const uint32_t *faces, const uint32_t *face_tets,
                 const uint32_t *tet_offsets, const uint32_t *tet_flip, const uint32_t *face_flip, size_t num_23, size_t num_32,
                 uint32_t *cells_out, uint32_t *cell_sources, void *stream_) {
    return guarded([&] {
        checked_flip_emit("tn_flip_emit", T, cells, F, faces, face_tets, tet_offsets, tet_flip, face_flip, num_23, num_32, cells_out,
                          cell_sources, stream_);
    });
}

int tn_flip_emit_loaded(tn_tracer_t tracer, const uint32_t *tet_offsets, const uint32_t *tet_flip, const uint32_t *face_flip,
                        size_t num_23, size_t num_32, uint32_t *cells_out, uint32_t *cell_sources, void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        if (!t->mesh.loaded) throw tn::Error("tn_flip_emit_loaded: no mesh is loaded; call load_tetrahedra first");
        const tn::DeviceMesh &m = t->mesh.view;
        DeviceGuard g(t->device);
        checked_flip_emit("tn_flip_emit_loaded", m.T, m.cells, m.F, m.faces, m.face_tets, tet_offsets, tet_flip, face_flip, num_23, num_32,
                          cells_out, cell_sources, stream_);
    });
}

int tn_face_table_count(int device, size_t V, size_t T, const uint32_t *cells, uint32_t *partner, uint32_t *face_index,
                        uint32_t *counters, void *stream_) {
    return guarded([&] {
        const std::string w("tn_face_table_count");
        if (T >= ((size_t)1 << 30)) throw tn::Error(w + ": num_cells must be below 2^30");
        if (!face_index || !counters || (T && (!cells || !partner))) throw tn::Error(w + ": a null pointer beside a non-zero count");
        DeviceGuard g(device);
        tn::launch_face_table_count(V, T, cells, partner, face_index, counters, (hipStream_t)stream_);
    });
}

int tn_face_table_emit(size_t T, const uint32_t *cells, const uint32_t *partner, const uint32_t *face_index, size_t num_faces,
                       uint32_t *faces, uint32_t *face_tets, uint32_t *tet_faces, void *stream_) {
    return guarded([&] {
        const std::string w("tn_face_table_emit");
        if (T >= ((size_t)1 << 30)) throw tn::Error(w + ": num_cells must be below 2^30");
        if (num_faces > 4 * T) throw tn::Error(w + ": num_faces exceeds 4 num_cells (a tetrahedron has four faces)");
        if ((T && (!cells || !partner || !face_index)) || (num_faces && (!faces || !face_tets)))
            throw tn::Error(w + ": a null pointer beside a non-zero count");
        tn::launch_face_table_emit(T, cells, partner, face_index, num_faces, faces, face_tets, tet_faces, (hipStream_t)stream_);
    });
}

size_t tn_num_faces(tn_tracer_t tracer) { return tracer && tracer->mesh.loaded ? tracer->mesh.view.F : 0; }

int tn_get_faces(tn_tracer_t tracer, uint32_t *faces_host, uint32_t *face_tets_host) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        check_loaded(t->mesh.loaded);
        tn_tracer::Mesh &b = t->mesh;
        const size_t F = b.view.F;
        if (b.host.face_tets.size() != 2 * F) {   // device build: the tables live on the device only
            DeviceGuard g(t->device);
            b.host.faces.resize(3 * F);
            b.host.face_tets.resize(2 * F);
            if (F) {
                TN_HIP(hipMemcpy(b.host.faces.data(), b.faces.p, b.host.faces.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
                TN_HIP(hipMemcpy(b.host.face_tets.data(), b.face_tets.p, b.host.face_tets.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            }
        }
        if (faces_host) std::memcpy(faces_host, b.host.faces.data(), b.host.faces.size() * sizeof(uint32_t));
        if (face_tets_host) std::memcpy(face_tets_host, b.host.face_tets.data(), b.host.face_tets.size() * sizeof(uint32_t));
    });
}

int tn_get_build_table(tn_tracer_t tracer, int which, void *dst, size_t *bytes) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        check_loaded(t->mesh.loaded);
        DeviceGuard g(t->device);
        const tn_tracer::Mesh &b = t->mesh;
        const void *src = nullptr;
        size_t n = 0;
        switch (which) {
            case 0: src = b.faces.p; n = b.faces.n * 4; break;
            case 1: src = b.face_tets.p; n = b.face_tets.n * 4; break;
            case 2: {   // the 64-byte records, re-assembled from the three tables (the unit of the build equality checks)
                const size_t n4 = b.hot.n;
                n = n4 * sizeof(tn::WalkVar);
                if (bytes) *bytes = n;
                if (dst && n4) {
                    std::vector<tn::WalkHot> h(n4); std::vector<tn::WalkTet> c(b.tets.n); std::vector<tn::WalkCold> cc(b.cold.n);
                    std::vector<tn::WalkFid> f(n4);
                    TN_HIP(hipMemcpy(h.data(), b.hot.p, n4 * sizeof(tn::WalkHot), hipMemcpyDeviceToHost));
                    if (!c.empty()) TN_HIP(hipMemcpy(c.data(), b.tets.p, c.size() * sizeof(tn::WalkTet), hipMemcpyDeviceToHost));
                    if (!cc.empty()) TN_HIP(hipMemcpy(cc.data(), b.cold.p, cc.size() * sizeof(tn::WalkCold), hipMemcpyDeviceToHost));
                    TN_HIP(hipMemcpy(f.data(), b.fidt.p, n4 * sizeof(tn::WalkFid), hipMemcpyDeviceToHost));
                    tn::WalkVar *o = static_cast<tn::WalkVar *>(dst);
                    for (size_t i = 0; i < n4; ++i) {
                        tn::WalkVar v{};
                        for (int k = 0; k < 3; ++k) v.pn[k] = h[i].pn[k];
                        v.nb[0] = h[i].nb0; v.nb[1] = h[i].nb1; v.nb[2] = h[i].nb2; v.code_lo = h[i].code_lo; v.code_hi = h[i].code_hi;
                        if (!c.empty()) { v.orig = c[i >> 2].orig; for (uint32_t k = 0; k < 4; ++k) v.vid[k] = c[i >> 2].vid((uint32_t)(i & 3), k); }
                        else { v.orig = cc[i].orig; for (int k = 0; k < 4; ++k) v.vid[k] = cc[i].vid[k]; }
                        v.fid0 = f[i].fid[0]; v.fid1 = f[i].fid[1]; v.fid2 = f[i].fid[2];
                        o[i] = v;
                    }
                }
                return;
            }
            case 3: src = b.hull_nodes.p; n = b.hull_nodes.n * 4; break;
            case 4: src = b.hull_tris.p; n = b.hull_tris.n * 4; break;
            case 5: src = b.bvh.child.p; n = b.bvh.child.n * 4; break;
            case 6: src = b.bvh.boxes.p; n = b.bvh.boxes.n * 4; break;
            case 7: src = b.bvh.leaf_id.p; n = b.bvh.leaf_id.n * 4; break;
            case 8: src = b.bvh.leaf_tri.p; n = b.bvh.leaf_tri.n * 4; break;
            default: throw tn::Error("unknown table");
        }
        if (bytes) *bytes = n;
        if (dst && n) TN_HIP(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    });
}

int tn_trace_rays_ex(tn_tracer_t tracer, size_t R, uint32_t M, const float *origins, const float *directions,
                     uint32_t *num_visited, uint32_t *visited, float *bary, float *dist, uint32_t *verts,
                     uint32_t flags, void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        if (flags & ~(uint32_t)(TN_TRACE_COMPACT_ROWS | TN_TRACE_BIN_RAYS)) throw tn::Error("unknown trace flag");
        check_pow2_M(M);
        check_loaded(t->mesh.loaded);
        if (M > 4096) throw tn::Error("max_ray_triangles larger than 4096 is not supported");
        if (R >= 0xFFFFFFFFull) throw tn::Error("too many rays for one call");
        if (R == 0) return;
        if (!origins || !directions || !num_visited || !visited || !bary || !dist)
            throw tn::Error("null ray / output pointer");
        DeviceGuard g(t->device);
        // dense_tails per CALL, not per tracer: a viewer thread and a trainer sharing one tracer may ask for different row forms
        TraceCall call{t, R, origins, directions, tn::Rows{num_visited, visited, bary, dist, verts, M},
                             t->opt.dense_tails && !(flags & TN_TRACE_COMPACT_ROWS), (hipStream_t)stream_};
        tn_tracer::Scratch &s = t->scratch;
        TN_HIP(hipMemsetAsync(s.stats.p, 0, tn_tracer::Scratch::stats_bytes(), call.stream));
        s.last_stream = call.stream;
        s.last_num_rays = R;
        s.last_walk = call.use_walk();
        s.last_binned = false;
        if (s.last_walk) {
            const size_t chunk = call.log_chunk();
            // binned: only a call that walks all its rays as one chunk (the BVH path and chunked calls ignore the flag)
            call.binned = s.last_binned = ((flags & TN_TRACE_BIN_RAYS) || t->opt.bin_rays) && chunk >= R;
            s.reserve(R, (chunk + 255) / 256 * 256 * (size_t)M, t->opt.verify_stride != 0, call.verify_risk(),
                      call.binned ? tn::ray_order_temp_bytes(R) : 0);
            if (chunk >= R) call.run_overlapped();
            else call.run_chunked(chunk);
        } else {
            call.run_small_batch();
        }
        TN_HIP(hipGetLastError());
    });
}

int tn_trace_rays(tn_tracer_t tracer, size_t R, uint32_t M, const float *origins, const float *directions,
                  uint32_t *num_visited, uint32_t *visited, float *bary, float *dist, uint32_t *verts,
                  void *stream_) {
    return tn_trace_rays_ex(tracer, R, M, origins, directions, num_visited, visited, bary, dist, verts, 0u, stream_);
}

int tn_postprocess_hits(tn_tracer_t tracer, size_t R, uint32_t M, const uint32_t *hit_count,
                        const uint32_t *hit_ids, const float *hit_t, const float *hit_uv,
                        uint32_t *num_visited, uint32_t *visited, float *bary, float *dist, uint32_t *verts,
                        void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        check_pow2_M(M);
        check_loaded(t->mesh.loaded);
        if (R == 0) return;
        DeviceGuard g(t->device);
        const tn::TraceParams p = mesh_params(t, R, tn::Rows{num_visited, visited, bary, dist, verts, M}, nullptr, nullptr);
        tn::launch_postprocess_hits(p, hit_count, hit_ids, hit_t, hit_uv, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_postprocess_hits_tables(int device, size_t R, uint32_t M, const uint32_t *faces, const uint32_t *face_tets,
                               const uint32_t *hit_count, const uint32_t *hit_ids, const float *hit_t,
                               const float *hit_uv, uint32_t *num_visited, uint32_t *visited, float *bary, float *dist,
                               uint32_t *verts, void *stream_) {
    return guarded([&] {
        check_pow2_M(M);
        if (!faces || !face_tets) throw tn::Error("null face table");
        if (R == 0) return;
        DeviceGuard g(device);
        tn::TraceParams p{};
        p.M = M; p.num_items = R;
        p.faces = faces; p.face_tets = face_tets;
        p.out_num = num_visited; p.out_cells = visited; p.out_bary = bary; p.out_dist = dist; p.out_verts = verts;
        tn::launch_postprocess_hits(p, hit_count, hit_ids, hit_t, hit_uv, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_trace_rays_triangles(tn_tracer_t tracer, size_t R, uint32_t M, const float *origins, const float *directions,
                            uint32_t *num_visited, uint32_t *visited, float *bary, float *dist, uint32_t *verts,
                            void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        check_pow2_M(M);
        check_loaded(t->mesh.loaded);
        if (M > 4096) throw tn::Error("max_ray_triangles larger than 4096 is not supported");
        if (R == 0) return;
        DeviceGuard g(t->device);
        const tn::TraceParams p = mesh_params(t, R, tn::Rows{num_visited, nullptr, nullptr, nullptr, nullptr, M}, origins, directions);
        tn::launch_trace_triangles(p, visited, dist, bary, verts, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_find_tetrahedra(tn_tracer_t tracer, size_t N, const float *positions, uint32_t *tetrahedra, float *bary,
                       uint32_t *verts, void *stream_) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        check_loaded(t->mesh.loaded);
        if (N == 0) return;
        DeviceGuard g(t->device);
        const tn::TraceParams p = mesh_params(t, N, tn::Rows{nullptr, nullptr, nullptr, nullptr, nullptr, 512}, nullptr, nullptr);
        tn::launch_find_tetrahedra(p, positions, tetrahedra, bary, verts, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_trace_stats(tn_tracer_t tracer, uint64_t stats[4]) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        DeviceGuard g(t->device);
        TN_HIP(hipStreamSynchronize(t->scratch.last_stream));
        unsigned long long h[tn::N_STATS];
        TN_HIP(hipMemcpy(h, t->scratch.stats.p, sizeof h, hipMemcpyDeviceToHost));
        const size_t R = t->scratch.last_num_rays;
        size_t other = R;                    // without the walk: every ray
        if (t->scratch.last_walk) {          // not certified by the walk: literal pairing of the logged hits + BVH re-trace
            uint32_t fb = 0;
            TN_HIP(hipMemcpy(&fb, t->scratch.fallback_count(), sizeof fb, hipMemcpyDeviceToHost));
            other = (uint32_t)(fb + (uint32_t)h[tn::STAT_REASON + tn::REASON_LITERAL_PAIRED]);
        }
        stats[tn::STAT_WALK] = R - other;
        stats[tn::STAT_OTHER] = other;
        stats[tn::STAT_LITERAL_BRANCH] = h[tn::STAT_LITERAL_BRANCH];
        stats[tn::STAT_OVERFLOW] = h[tn::STAT_OVERFLOW];
    });
}

int tn_trace_flag_reasons(tn_tracer_t tracer, uint64_t reasons[16]) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        DeviceGuard g(t->device);
        TN_HIP(hipStreamSynchronize(t->scratch.last_stream));
        unsigned long long h[tn::N_STATS];
        TN_HIP(hipMemcpy(h, t->scratch.stats.p, sizeof h, hipMemcpyDeviceToHost));
        for (int i = 0; i < tn::N_REASONS; ++i) reasons[i] = h[tn::STAT_REASON + i];
    });
}

int tn_trace_cross_check(tn_tracer_t tracer, uint64_t out[8]) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        if (!out) throw tn::Error("out is null");
        DeviceGuard g(t->device);
        TN_HIP(hipStreamSynchronize(t->scratch.last_stream));
        unsigned long long h[tn::N_STATS];
        TN_HIP(hipMemcpy(h, t->scratch.stats.p, sizeof h, hipMemcpyDeviceToHost));
        out[0] = t->opt.verify_stride;
        out[1] = h[tn::STAT_REASON + tn::REASON_VERIFY_CHECKED]; out[2] = h[tn::STAT_REASON + tn::REASON_VERIFY_BAD];
        out[3] = h[tn::STAT_RISK_HULL]; out[4] = h[tn::STAT_RISK_THIN];
        out[5] = h[tn::STAT_RISK_CHECKED]; out[6] = h[tn::STAT_RISK_BAD]; out[7] = 0;
    });
}

int tn_trace_ray_order(tn_tracer_t tracer, uint32_t *order_host, size_t *n) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        if (!n) throw tn::Error("n is null");
        const tn_tracer::Scratch &s = t->scratch;
        *n = s.last_binned ? s.last_num_rays : 0;
        if (!order_host || !*n) return;
        DeviceGuard g(t->device);
        TN_HIP(hipStreamSynchronize(s.last_stream));
        TN_HIP(hipMemcpy(order_host, s.order.p, *n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    });
}

int tn_trace_timings(tn_tracer_t tracer, float ms[8]) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        if (!ms) throw tn::Error("ms is null");
        const tn_tracer::Schedule &c = t->sched;
        if (!c.tev_valid) throw tn::Error("no timed call: set option \"timing\" = 1 and trace a one-chunk walk call first");
        DeviceGuard g(t->device);
        TN_HIP(hipEventSynchronize(c.tev[c.N_TEV - 1]));
        for (int i = 0; i + 1 < c.N_TEV; ++i) TN_HIP(hipEventElapsedTime(&ms[i], c.tev[i], c.tev[i + 1]));
    });
}

int tn_fill_rows(size_t R, uint32_t M, uint32_t first_slot, uint32_t *visited, float *bary, float *dist, uint32_t *verts,
                 void *stream_) {
    return guarded([&] {
        if (R == 0) return;
        if (!visited || !bary || !dist) throw tn::Error("null output pointer");
        if (M < 4 || (M & (M - 1)) != 0) throw tn::Error("max_ray_triangles must be a power of 2.");
        if (first_slot >= M) return;
        // rows are written from a 128-byte line boundary of all four arrays on (multiples of 32 slots), like the tracer's own fill;
        // any other first slot is refused rather than rounded: rounding down would overwrite up to 31 written segments
        if (first_slot & 31u) throw tn::Error("tn_fill_rows: first_slot must be a multiple of 32");
        // no per-row lookups here: one linear stream per array
        tn::launch_fill(tn::Rows{nullptr, visited, bary, dist, verts, M}, R, nullptr,
                        tn::FillRange{true, first_slot, false, tn::FillKind::Linear, 0}, (hipStream_t)stream_);
        TN_HIP(hipGetLastError());
    });
}

int tn_set_option(tn_tracer_t tracer, const char *name, int value) {
    return guarded([&] {
        tn_tracer *t = checked(tracer);
        std::lock_guard<std::mutex> lock(t->mu);
        tn_tracer::Options &o = t->opt;
        // grid options of the two fills: -2 = one linear stream per array, any other negative value = one block per row,
        // n >= 0 = n blocks of persistent waves (0: that kernel's default grid)
        auto set_grid = [](tn::FillRange &f, int v) {
            f.kind = v == -2 ? tn::FillKind::Linear : v < 0 ? tn::FillKind::RowPerBlock : tn::FillKind::Spans;
            f.blocks = v > 0 ? (unsigned)v : 0u;
        };
        const std::string k = name ? name : "";
        if (k == "gpu_build") o.gpu_build = value != 0;
        else if (k == "bin_rays") o.bin_rays = value != 0;
        else if (k == "timing") { o.timing = value != 0; t->sched.tev_valid = false; }
        else if (k == "leaf_width") {
            if (value != 16 && value != 32 && value != 64) throw tn::Error("leaf_width must be 16, 32 or 64");
            o.leaf_width = (unsigned)value;
        }
        else if (k == "walk") o.use_walk = value < 0 ? 0 : (value > 2 ? 2 : value);
        else if (k == "walk_min_rays") { o.walk_min_rays = value < 0 ? 0 : (size_t)value; o.walk_min_auto = false; }
        else if (k == "dense_tails") o.dense_tails = value != 0;
        else if (k == "literal") o.literal = value != 0;
        else if (k == "spec_fill") o.spec_fill = value != 0;
        else if (k == "spec_k0") o.spec_k0 = (unsigned)value;
        else if (k == "spec_blocks") set_grid(o.spec, value);
        else if (k == "hull_flat") o.hull_flat = value != 0;
        else if (k == "writer_blocks") o.writer_blocks = (unsigned)value;
        else if (k == "fill_blocks") set_grid(o.tail, value);
        else if (k == "walk_lds_kb") o.walk_lds_kb = (unsigned)value;
        else if (k == "small_lds") o.small_lds = value != 0;
        else if (k == "lds_cap") {
            if (value < 0 || (value & (value - 1)) != 0 || (value && value < 8)) throw tn::Error("lds_cap must be 0 or a power of two >= 8");
            o.lds_cap = (unsigned)value;
        }
        else if (k == "writer_table") o.writer_table = value;   // applies at the next load_tetrahedra
        else if (k == "refit_tables") o.refit_tables = value != 0;   // applies at the next load_tetrahedra
        else if (k == "cert_ends") { if (value < 0 || value > 3) throw tn::Error("cert_ends must be 0 .. 3"); o.cert_ends = value; }
        else if (k == "verify_inject") o.verify_inject = value != 0;
        else if (k == "literal_sort_passes") o.literal_sort_passes = value < 0 ? 0u : (unsigned)value;
        else if (k == "verify_stride") o.verify_stride = value < 0 ? 0u : (unsigned)value;
        else if (k == "verify_risk") o.verify_risk = value != 0;
        else if (k == "risk_band") o.risk_band = value < 1 ? 1u : (unsigned)value;
        else if (k == "log_cap_mb") o.log_cap_bytes = value <= 0 ? 0 : (size_t)value << 20;
        else throw tn::Error("unknown option " + (name ? k : std::string("(null)")));
    });
}

}  // extern "C"
