// CPU emulation of the REFIT (tetra-nerf_amd/csrc/tn_refit.hip) -- test infrastructure, in the pattern of gpu_build_emul.cpp.
// The device build is emulated on vertices A (the element functions of tn_build_core.h in plain loops), the refit's element
// functions move the tables to vertices B, and the result is compared with an emulated build on B:
//   - pn and the thin exponent of the record of every (caller tet id, entry face) are the bytes of a fresh build's;
//   - every other byte of every record is untouched;
//   - the face BVH keeps its invariants (every face in exactly one leaf, every slot's box tight around what is below it);
//   - the hull triangles equal the fresh build's, face by face (positions, local face, caller tet id of the record);
//   - a refit back to A restores every table byte for byte.
// Input file: u64 V, u64 T, f32 xyzA[3V], f32 xyzB[3V], u32 cells[4T].  Prints "OK ...".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>

#include "tn_build.h"

namespace tn { void set_error(const std::string &) {} }

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) { std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); return false; } \
    } while (0)

using namespace tn;

struct Tables {
    // topology
    std::vector<uint32_t> faces, face_tets, tet_face, order, rec_of_tet, face_order, leaf_nodes, level_start, child, wide_sub, leaf_id;
    std::vector<core::BinNode> bn;
    // geometry
    std::vector<WalkVar> vars;
    std::vector<uint32_t> hull_info;   // [n_hull][12]
    HostHullBvh hull;
    std::vector<float> node_lo, node_hi, boxes, leaf_tri;
    float scene_max = 0.f;
    uint32_t leaf_w = 16;
};

static float scene_max_of(const std::vector<uint32_t> &cells, const float *xyz) {
    float m = 0.f;
    for (uint32_t v : cells)
        for (int k = 0; k < 3; ++k) m = std::max(m, std::fabs(xyz[3 * (size_t)v + k]));
    return m;
}

static void leaf_triangles(Tables &t, const float *xyz, bool ids) {
    const size_t n_leaves = t.leaf_nodes.size();
    t.leaf_tri.assign(n_leaves * 9 * t.leaf_w, 0.f);
    if (ids) t.leaf_id.assign(n_leaves * t.leaf_w, TN_EMPTY);
    for (size_t l = 0; l < n_leaves; ++l) {
        const core::BinNode nd = t.bn[t.leaf_nodes[l]];
        for (uint32_t i = 0; i < nd.count; ++i) {
            const uint32_t fid = t.face_order[nd.first + i];
            if (ids) t.leaf_id[l * t.leaf_w + i] = fid;
            for (int q = 0; q < 3; ++q)
                for (int k = 0; k < 3; ++k) t.leaf_tri[(l * 9 + q * 3 + k) * t.leaf_w + i] = xyz[3 * (size_t)t.faces[3 * (size_t)fid + q] + k];
        }
    }
}

// the device build of tn_build.hip, emulated (gpu_build_emul.cpp checks this sequence against the host build)
static bool build(size_t V, size_t T, const float *xyz, const std::vector<uint32_t> &cells, uint32_t leaf_w, Tables &t) {
    t.leaf_w = leaf_w;
    const size_t n4 = 4 * T;
    size_t cap = 16;
    while (cap < 8 * T + 16) cap <<= 1;
    std::vector<uint32_t> slot(cap, TN_EMPTY), partner(n4, TN_EMPTY), first(n4), fidx(n4);
    t.tet_face.assign(n4, TN_EMPTY);
    uint32_t flags = 0;
    for (size_t i = 0; i < n4; ++i) core::face_hash_insert((uint32_t)i, cells.data(), slot.data(), cap - 1, partner.data(), &flags);
    CHECK(!(flags & core::FLAG_TRIPLE_FACE));
    for (size_t i = 0; i < n4; ++i) first[i] = core::face_is_first((uint32_t)i, partner.data()) ? 1u : 0u;
    std::exclusive_scan(first.begin(), first.end(), fidx.begin(), 0u);
    const size_t F = fidx[n4 - 1] + first[n4 - 1];
    t.faces.assign(3 * F, 0); t.face_tets.assign(2 * F, 0);
    for (size_t i = 0; i < n4; ++i)
        if (first[i]) core::face_emit((uint32_t)i, fidx[i], cells.data(), partner.data(), t.faces.data(), t.face_tets.data(), t.tet_face.data());
    // Morton order, walk records, thin exponent
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < T; ++i) {
        float c[3];
        core::tet_centroid((uint32_t)i, cells.data(), xyz, c);
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], c[a]); hi[a] = std::max(hi[a], c[a]); }
    }
    std::vector<std::pair<uint64_t, uint32_t>> keyed(T);
    for (size_t i = 0; i < T; ++i) {
        float c[3];
        core::tet_centroid((uint32_t)i, cells.data(), xyz, c);
        keyed[i] = {core::morton63(c, lo, hi), (uint32_t)i};
    }
    std::stable_sort(keyed.begin(), keyed.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    t.order.resize(T); t.rec_of_tet.resize(T);
    for (size_t r = 0; r < T; ++r) { t.order[r] = keyed[r].second; t.rec_of_tet[keyed[r].second] = (uint32_t)r; }
    t.vars.resize(n4);
    for (size_t i = 0; i < n4; ++i)
        t.vars[i] = core::walk_var_of((uint32_t)(i >> 2), (uint32_t)(i & 3), t.order.data(), t.rec_of_tet.data(), cells.data(), xyz,
                                      t.tet_face.data(), t.faces.data(), t.face_tets.data(), &flags);
    {
        std::vector<uint32_t> vmin(V, 0x7F800000u);
        for (size_t k = 0; k < T; ++k) {
            const uint32_t *c = cells.data() + 4 * k;
            float p[4][3];
            for (int q = 0; q < 4; ++q) for (int a = 0; a < 3; ++a) p[q][a] = xyz[3 * (size_t)c[q] + a];
            const uint32_t bits = core::tet_min_height_bits(p);
            for (int q = 0; q < 4; ++q) core::atomic_min_u32(&vmin[c[q]], bits);
        }
        for (size_t k = 0; k < T; ++k) {
            const uint32_t *c = cells.data() + 4 * k;
            const uint32_t e = core::thin_exponent(vmin[c[0]], vmin[c[1]], vmin[c[2]], vmin[c[3]]);
            for (uint32_t q = 0; q < 4; ++q) t.vars[4 * (size_t)t.rec_of_tet[k] + q].code_hi |= e << core::THIN_SHIFT;
        }
    }
    CHECK(!(flags & core::FLAG_INTERNAL));
    // hull
    t.hull_info.clear();
    for (size_t f = 0; f < F; ++f)
        if (t.face_tets[2 * f + 1] == TN_EMPTY) {
            t.hull_info.resize(t.hull_info.size() + 12);
            core::hull_face_info((uint32_t)f, t.faces.data(), t.face_tets.data(), t.tet_face.data(), t.rec_of_tet.data(), xyz,
                                 &t.hull_info[t.hull_info.size() - 12], &flags);
        }
    {
        std::vector<float> info(t.hull_info.size());
        std::memcpy(info.data(), t.hull_info.data(), info.size() * 4);
        build_hull_from_info(info, t.hull);
    }
    // face BVH
    std::vector<std::vector<uint32_t>> frontier;
    build_bin_topology(F, t.bn, frontier, t.level_start, t.leaf_nodes, leaf_w);
    std::vector<float> fb(6 * F), cen(3 * F);
    for (size_t f = 0; f < F; ++f) core::face_box((uint32_t)f, t.faces.data(), xyz, &fb[6 * f], &cen[3 * f]);
    std::vector<uint32_t> ord(F);
    std::iota(ord.begin(), ord.end(), 0u);
    for (size_t l = 0; l + 1 < frontier.size(); ++l) {
        std::vector<uint64_t> keys(F);
        for (size_t s = 0; s < frontier[l].size(); ++s) {
            const core::BinNode &nd = t.bn[frontier[l][s]];
            float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (uint32_t i = nd.first; i < nd.first + nd.count; ++i)
                for (int a = 0; a < 3; ++a) { clo[a] = std::min(clo[a], cen[3 * (size_t)ord[i] + a]); chi[a] = std::max(chi[a], cen[3 * (size_t)ord[i] + a]); }
            const int ax = core::split_axis(clo, chi);
            for (uint32_t i = nd.first; i < nd.first + nd.count; ++i)
                keys[i] = ((uint64_t)s << 32) | core::float_ordered(cen[3 * (size_t)ord[i] + ax]);
        }
        std::vector<uint32_t> perm(F), nxt(F);
        std::iota(perm.begin(), perm.end(), 0u);
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
        for (size_t i = 0; i < F; ++i) nxt[i] = ord[perm[i]];
        ord.swap(nxt);
    }
    t.face_order = ord;
    const size_t nn = t.bn.size();
    t.node_lo.assign(3 * nn, 0.f); t.node_hi.assign(3 * nn, 0.f);
    for (size_t k = nn; k-- > 0;) {   // k_node_boxes
        float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (t.bn[k].left < 0) {
            for (uint32_t i = t.bn[k].first; i < t.bn[k].first + t.bn[k].count; ++i)
                for (int a = 0; a < 3; ++a) { blo[a] = fminf(blo[a], fb[6 * (size_t)ord[i] + a]); bhi[a] = fmaxf(bhi[a], fb[6 * (size_t)ord[i] + 3 + a]); }
        } else {
            for (int a = 0; a < 3; ++a) {
                blo[a] = fminf(t.node_lo[3 * (size_t)t.bn[k].left + a], t.node_lo[3 * (size_t)t.bn[k].right + a]);
                bhi[a] = fmaxf(t.node_hi[3 * (size_t)t.bn[k].left + a], t.node_hi[3 * (size_t)t.bn[k].right + a]);
            }
        }
        for (int a = 0; a < 3; ++a) { t.node_lo[3 * k + a] = blo[a]; t.node_hi[3 * k + a] = bhi[a]; }
    }
    leaf_triangles(t, xyz, true);
    // k_collapse, wide node by wide node
    const core::BinTreeView tree{t.bn.data(), t.node_lo.data(), t.node_hi.data()};
    t.wide_sub.assign(1, 0u);
    t.child.clear(); t.boxes.clear();
    for (size_t w = 0; w < t.wide_sub.size(); ++w) {
        int kids[WIDE];
        const int nk = core::collapse_node((int)t.wide_sub[w], tree, kids);
        t.child.resize((w + 1) * WIDE, TN_EMPTY);
        t.boxes.resize((w + 1) * 6 * WIDE);
        for (int i = 0; i < WIDE; ++i) {
            float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
            if (i < nk) {
                const int k = kids[i];
                for (int a = 0; a < 3; ++a) { blo[a] = t.node_lo[3 * (size_t)k + a]; bhi[a] = t.node_hi[3 * (size_t)k + a]; }
                if (t.bn[k].left < 0) t.child[w * WIDE + i] = 0x80000000u | (uint32_t)t.bn[k].leaf;
                else { t.child[w * WIDE + i] = (uint32_t)t.wide_sub.size(); t.wide_sub.push_back((uint32_t)k); }
            }
            for (int a = 0; a < 3; ++a) { t.boxes[(w * 6 + a) * WIDE + i] = blo[a]; t.boxes[(w * 6 + 3 + a) * WIDE + i] = bhi[a]; }
        }
    }
    t.scene_max = scene_max_of(cells, xyz);
    return true;
}

// tn_refit.hip: device_refit, kernel by kernel
static bool refit(size_t V, size_t T, const float *xyz, const std::vector<uint32_t> &cells, Tables &t) {
    std::vector<uint32_t> vmin(V, 0x7F800000u);
    for (size_t i = T; i-- > 0;) core::tet_thin_star((uint32_t)i, cells.data(), xyz, vmin.data());   // (the atomic minimum commutes)
    for (size_t i = 0; i < 4 * T; ++i)
        core::refit_walk_record(t.vars[i], (uint32_t)(i & 3), cells.data() + 4 * (size_t)t.order[i >> 2], xyz, vmin.data());
    for (size_t h = 0; h < t.hull_info.size() / 12; ++h) core::hull_face_refit(t.faces.data(), xyz, &t.hull_info[12 * h]);
    {
        std::vector<float> info(t.hull_info.size());
        std::memcpy(info.data(), t.hull_info.data(), info.size() * 4);
        const size_t n_nodes = t.hull.nodes.size(), n_flat = t.hull.flat.size(), n_tris = t.hull.tris.size();
        build_hull_from_info(info, t.hull);
        CHECK(t.hull.nodes.size() == n_nodes && t.hull.flat.size() == n_flat && t.hull.tris.size() == n_tris);
    }
    for (size_t l = t.level_start.size() - 1; l-- > 0;)
        for (uint32_t k = t.level_start[l]; k < t.level_start[l + 1]; ++k)
            core::refit_node_box(k, t.bn.data(), t.face_order.data(), t.faces.data(), xyz, t.node_lo.data(), t.node_hi.data());
    leaf_triangles(t, xyz, false);
    for (size_t j = 0; j < t.child.size(); ++j) {
        const size_t w = j / WIDE, i = j % WIDE;
        const int k = core::wide_child_node(t.child[j], t.leaf_nodes.data(), t.wide_sub.data());
        for (int a = 0; a < 3; ++a) {
            t.boxes[(w * 6 + a) * WIDE + i] = k < 0 ? INFINITY : t.node_lo[3 * (size_t)k + a];
            t.boxes[(w * 6 + 3 + a) * WIDE + i] = k < 0 ? -INFINITY : t.node_hi[3 * (size_t)k + a];
        }
    }
    t.scene_max = scene_max_of(cells, xyz);
    return true;
}

// the invariants tests/test_build_gpu.py::_check_bvh states
static bool check_bvh(const Tables &t) {
    const size_t F = t.faces.size() / 3, n_wide = t.child.size() / WIDE, n_leaves = t.leaf_nodes.size(), lw = t.leaf_w;
    std::vector<uint8_t> seen_face(F, 0), seen_leaf(n_leaves, 0), seen_node(n_wide, 0);
    size_t faces_seen = 0;
    for (uint32_t id : t.leaf_id)
        if (id != TN_EMPTY) { CHECK(id < F && !seen_face[id]); seen_face[id] = 1; ++faces_seen; }
    CHECK(faces_seen == F);
    seen_node[0] = 1;
    for (size_t w = 0; w < n_wide; ++w)
        for (size_t i = 0; i < (size_t)WIDE; ++i) {
            const uint32_t ch = t.child[w * WIDE + i];
            float lo[3], hi[3], wlo[3] = {INFINITY, INFINITY, INFINITY}, whi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int a = 0; a < 3; ++a) { lo[a] = t.boxes[(w * 6 + a) * WIDE + i]; hi[a] = t.boxes[(w * 6 + 3 + a) * WIDE + i]; }
            if (ch == TN_EMPTY) { CHECK(lo[0] == INFINITY && hi[0] == -INFINITY); continue; }
            if (ch >> 31) {
                const size_t l = ch & 0x7FFFFFFFu;
                CHECK(l < n_leaves && !seen_leaf[l]);
                seen_leaf[l] = 1;
                for (size_t s = 0; s < lw; ++s)
                    if (t.leaf_id[l * lw + s] != TN_EMPTY)
                        for (int q = 0; q < 3; ++q)
                            for (int a = 0; a < 3; ++a) {
                                const float x = t.leaf_tri[(l * 9 + q * 3 + a) * lw + s];
                                wlo[a] = std::min(wlo[a], x); whi[a] = std::max(whi[a], x);
                            }
            } else {
                CHECK(ch > w && ch < n_wide && !seen_node[ch]);
                seen_node[ch] = 1;
                for (size_t s = 0; s < (size_t)WIDE; ++s)
                    if (t.child[(size_t)ch * WIDE + s] != TN_EMPTY)
                        for (int a = 0; a < 3; ++a) {
                            wlo[a] = std::min(wlo[a], t.boxes[((size_t)ch * 6 + a) * WIDE + s]);
                            whi[a] = std::max(whi[a], t.boxes[((size_t)ch * 6 + 3 + a) * WIDE + s]);
                        }
            }
            for (int a = 0; a < 3; ++a) CHECK(wlo[a] == lo[a] && whi[a] == hi[a]);   // tight
        }
    for (uint8_t s : seen_leaf) CHECK(s);
    for (uint8_t s : seen_node) CHECK(s);
    return true;
}

template <class T>
static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static bool same_tables(const Tables &a, const Tables &b) {
    CHECK(same(a.vars, b.vars));
    CHECK(same(a.hull_info, b.hull_info));
    CHECK(same(a.hull.nodes, b.hull.nodes) && same(a.hull.tris, b.hull.tris) && same(a.hull.flat, b.hull.flat));
    CHECK(same(a.node_lo, b.node_lo) && same(a.node_hi, b.node_hi));
    CHECK(same(a.boxes, b.boxes) && same(a.leaf_tri, b.leaf_tri) && same(a.leaf_id, b.leaf_id) && same(a.child, b.child));
    CHECK(same(a.faces, b.faces) && same(a.face_tets, b.face_tets) && same(a.order, b.order) && same(a.face_order, b.face_order));
    CHECK(std::memcmp(&a.scene_max, &b.scene_max, 4) == 0);
    return true;
}

static WalkVar topology_of(WalkVar v) {   // the record with its two geometry fields cleared
    for (int a = 0; a < 3; ++a) v.pn[a] = 0.f;
    v.code_hi &= ~(0xFFu << core::THIN_SHIFT);
    return v;
}

static bool run(size_t V, size_t T, const std::vector<float> &A, const std::vector<float> &B, const std::vector<uint32_t> &cells,
                uint32_t leaf_w) {
    Tables first, t, fresh;
    CHECK(build(V, T, A.data(), cells, leaf_w, first));
    CHECK(build(V, T, A.data(), cells, leaf_w, t));
    CHECK(build(V, T, B.data(), cells, leaf_w, fresh));
    CHECK(check_bvh(first) && check_bvh(fresh));
    // a refit to the vertices of the load changes no byte
    CHECK(refit(V, T, A.data(), cells, t));
    CHECK(same_tables(t, first));
    CHECK(refit(V, T, B.data(), cells, t));
    size_t moved = 0;
    for (size_t orig = 0; orig < T; ++orig)
        for (uint32_t e = 0; e < 4; ++e) {
            const WalkVar &r = t.vars[4 * (size_t)t.rec_of_tet[orig] + e], &f = fresh.vars[4 * (size_t)fresh.rec_of_tet[orig] + e];
            const WalkVar &o = first.vars[4 * (size_t)first.rec_of_tet[orig] + e];
            CHECK(r.orig == orig && f.orig == orig);
            CHECK(std::memcmp(r.pn, f.pn, 12) == 0);                                                            // geometry: a fresh build's
            CHECK(((r.code_hi >> core::THIN_SHIFT) & 0xFFu) == ((f.code_hi >> core::THIN_SHIFT) & 0xFFu));
            const WalkVar a = topology_of(r), b = topology_of(o);
            CHECK(std::memcmp(&a, &b, sizeof(WalkVar)) == 0);                                                   // topology: untouched
            moved += std::memcmp(r.pn, o.pn, 12) != 0;
        }
    CHECK(check_bvh(t));
    CHECK(same(t.faces, fresh.faces) && same(t.face_tets, fresh.face_tets) && same(t.leaf_id, first.leaf_id) && same(t.child, first.child));
    CHECK(std::memcmp(&t.scene_max, &fresh.scene_max, 4) == 0);
    {   // hull triangles, keyed by face id: positions and local face as in a fresh build, the record names the same caller tet
        std::map<uint32_t, const float *> by_fid;
        auto word = [](const float *p) { uint32_t u; std::memcpy(&u, p, 4); return u; };
        for (size_t h = 0; h < fresh.hull.tris.size() / 12; ++h) by_fid[word(&fresh.hull.tris[12 * h + 3])] = &fresh.hull.tris[12 * h];
        CHECK(by_fid.size() == t.hull.tris.size() / 12);
        for (size_t h = 0; h < t.hull.tris.size() / 12; ++h) {
            const float *r = &t.hull.tris[12 * h];
            const auto it = by_fid.find(word(r + 3));
            CHECK(it != by_fid.end());
            const float *f = it->second;
            for (int v = 0; v < 3; ++v) CHECK(std::memcmp(r + 4 * v, f + 4 * v, 12) == 0);
            CHECK(word(r + 11) == word(f + 11) && t.order[word(r + 7)] == fresh.order[word(f + 7)]);
        }
    }
    CHECK(refit(V, T, A.data(), cells, t));   // round trip
    CHECK(same_tables(t, first));
    std::printf("OK tets %zu records %zu (%zu moved) hull %zu wide_nodes %zu leaves %zu\n", T, 4 * T, moved, t.hull_info.size() / 12,
                t.child.size() / WIDE, t.leaf_nodes.size());
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const uint32_t leaf_w = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 16u;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t V = 0, T = 0;
    if (std::fread(&V, 8, 1, f) != 1 || std::fread(&T, 8, 1, f) != 1) return 2;
    std::vector<float> A(3 * V), B(3 * V);
    std::vector<uint32_t> cells(4 * T);
    if (std::fread(A.data(), 4, A.size(), f) != A.size() || std::fread(B.data(), 4, B.size(), f) != B.size() ||
        std::fread(cells.data(), 4, cells.size(), f) != cells.size())
        return 2;
    std::fclose(f);
    return run(V, T, A, B, cells, leaf_w) ? 0 : 1;
}
