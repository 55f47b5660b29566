// CPU emulation of the EDGE SPLIT (tetra-nerf_amd/csrc/tn_edge_split.hip) -- test infrastructure, in the pattern of split_emul.cpp.
// The kernels are plain loops over the element functions of tn_edge_split_core.h, which are the kernels' bodies; the sort is
// std::sort, the scans are running sums, an atomicOr is an |=.  tests/test_edge_split.py compares every output bit for bit with
// the numpy statement (geometry.split_edges_statement).
// Input file:  u64 V, u64 T, u64 F, f32 xyz[3V], u32 cells[4T], u8 select[T], u32 faces[3F], u32 face_tets[2F].
// Output file: u32 counters[10], u32 tet_offsets[T+1], u32 tet_edge[T], u8 bisected[T], u32 edge_vertices[2 K_v], f32
//              xyz_out[3(V+K_v)], u32 cells_out[4(T+K_t)], u32 cell_parent[T+K_t], u32 vertex_parents[4 K_v]
//              (K_v = counters[8], K_t = counters[9]).  Prints "OK ...".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tn_edge_split_core.h"

using namespace tn;

static bool read_all(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_all(std::FILE *f, const void *p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: edge_split_emul IN OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t V64 = 0, T64 = 0, F64 = 0;
    if (!read_all(f, &V64, 8) || !read_all(f, &T64, 8) || !read_all(f, &F64, 8)) return 2;
    const size_t V = V64, T = T64, F = F64;
    // exact-size heap arrays: a read or write one element outside is the sanitizer's to see
    std::vector<float> xyz(3 * V);
    std::vector<uint32_t> cells(4 * T), faces(3 * F), face_tets(2 * F);
    std::vector<uint8_t> select(T);
    if (!read_all(f, xyz.data(), 12 * V) || !read_all(f, cells.data(), 16 * T) || !read_all(f, select.data(), T) ||
        !read_all(f, faces.data(), 12 * F) || !read_all(f, face_tets.data(), 8 * F))
        return 2;
    std::fclose(f);
    if (T >= esplit::MAX_CELLS || V >= 0xFFFFFFFFull || F >= 0xFFFFFFFFull) { std::fprintf(stderr, "refused\n"); return 3; }
    const uint32_t Vu = (uint32_t)V;

    std::vector<uint32_t> counters(esplit::NUM_COUNTERS, 0u), tet_offsets(T + 1, 0u), tet_edge(T, esplit::EMPTY);
    std::vector<uint8_t> bisected(T, 0);
    // k_esplit_nominate, the sort, k_esplit_heads and its scan, k_esplit_compact
    std::vector<uint64_t> keys(T);
    for (size_t t = 0; t < T; ++t) {
        const esplit::Nomination v = esplit::nominate(select[t] != 0, &cells[4 * t], Vu, xyz.data(), &keys[t]);
        counters[esplit::ASKED] += v != esplit::NOT_ASKED;
        counters[esplit::ASKED_ID] += v == esplit::ASKED_REFUSED_ID;
        counters[esplit::ASKED_FLAT] += v == esplit::ASKED_REFUSED_FLAT;
    }
    std::sort(keys.begin(), keys.end());
    std::vector<uint64_t> cand;
    for (size_t i = 0; i < T; ++i)
        if (keys[i] < esplit::sentinel(Vu) && (i == 0 || keys[i] != keys[i - 1])) cand.push_back(keys[i]);
    const uint32_t C = (uint32_t)cand.size();
    std::vector<uint32_t> eflags(C, 0u), winner(T, esplit::EMPTY);
    // k_esplit_rows
    for (size_t t = 0; t < T; ++t) {
        uint32_t found[6], flag[6];
        winner[t] = esplit::judge_row(&cells[4 * t], Vu, xyz.data(), cand.data(), C, found, flag);
        for (int e = 0; e < 6; ++e)
            if (found[e] != esplit::EMPTY && flag[e]) eflags.at(found[e]) |= flag[e];
    }
    // k_esplit_hull
    for (size_t i = 0; i < F && C; ++i) {
        if (face_tets[2 * i + 1] != esplit::EMPTY) continue;
        for (int k = 0; k < 3; ++k) {
            const uint32_t at = esplit::find(cand.data(), C, iso::edge_key(faces[3 * i + k], faces[3 * i + (k + 1) % 3]));
            if (at != esplit::EMPTY) eflags.at(at) |= esplit::FLAG_HULL;
        }
    }
    // k_esplit_classify, its scan, k_esplit_edges
    std::vector<uint32_t> rank(C + 1, 0u), edge_vertices;
    for (uint32_t i = 0; i < C; ++i) {
        const esplit::Counter v = esplit::classify(eflags[i]);
        counters[esplit::CANDIDATES] += 1u;
        counters[v] += 1u;
        rank[i + 1] = rank[i] + (v == esplit::ACCEPTED);
        if (v == esplit::ACCEPTED) {
            edge_vertices.push_back((uint32_t)(cand[i] >> 32));
            edge_vertices.push_back((uint32_t)cand[i]);
        }
    }
    // k_esplit_tets and its scan
    for (size_t t = 0; t < T; ++t) {
        const uint32_t w = winner[t];
        const bool b = w < C && rank[w + 1] != rank[w];
        bisected[t] = b;
        tet_edge[t] = b ? rank[w] : esplit::EMPTY;
        tet_offsets[t + 1] = tet_offsets[t] + b;
        counters[esplit::BISECTED] += b;
    }
    const size_t Kv = counters[esplit::ACCEPTED], Kt = counters[esplit::BISECTED];
    if (T + Kt >= esplit::MAX_CELLS || V + Kv >= 0xFFFFFFFFull) { std::fprintf(stderr, "refused\n"); return 3; }

    // the copy of the old vertices, k_esplit_vertices, k_esplit_cells
    std::vector<float> xyz_out(3 * (V + Kv));
    std::vector<uint32_t> cells_out(4 * (T + Kt)), cell_parent(T + Kt), vertex_parents(4 * Kv);
    for (size_t i = 0; i < 3 * V; ++i) xyz_out[i] = xyz[i];
    for (size_t j = 0; j < Kv; ++j) {
        const uint32_t lo = edge_vertices[2 * j], hi = edge_vertices[2 * j + 1];
        float m[3] = {0.f, 0.f, 0.f};
        if (lo < V && hi < V) esplit::midpoint(&xyz[3 * (size_t)lo], &xyz[3 * (size_t)hi], m);
        for (int k = 0; k < 3; ++k) xyz_out[3 * (V + j) + k] = m[k];
        for (int k = 0; k < 4; ++k) vertex_parents[4 * j + k] = k & 1 ? hi : lo;
    }
    for (size_t t = 0; t < T; ++t) {
        const uint32_t *c = &cells[4 * t];
        uint32_t child0[4], child1[4];
        const size_t k = tet_offsets[t];
        const bool b = tet_offsets[t + 1] > tet_offsets[t] && k < Kt;
        for (int j = 0; j < 4; ++j) child0[j] = child1[j] = c[j];
        if (b) {
            const uint32_t j = tet_edge[t];
            int slot_lo, slot_hi;
            if (j < Kv && esplit::slots_of(c, edge_vertices[2 * (size_t)j], edge_vertices[2 * (size_t)j + 1], slot_lo, slot_hi)) {
                split::child_row(c, slot_hi, Vu + j, child0);
                split::child_row(c, slot_lo, Vu + j, child1);
            }
            for (int i = 0; i < 4; ++i) cells_out[4 * (T + k) + i] = child1[i];
            cell_parent[T + k] = (uint32_t)t;
        }
        for (int i = 0; i < 4; ++i) cells_out[4 * t + i] = child0[i];
        cell_parent[t] = (uint32_t)t;
    }

    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    const bool ok = write_all(f, counters.data(), 4 * esplit::NUM_COUNTERS) && write_all(f, tet_offsets.data(), 4 * (T + 1)) &&
                    write_all(f, tet_edge.data(), 4 * T) && write_all(f, bisected.data(), T) &&
                    write_all(f, edge_vertices.data(), 8 * Kv) && write_all(f, xyz_out.data(), 12 * (V + Kv)) &&
                    write_all(f, cells_out.data(), 16 * (T + Kt)) && write_all(f, cell_parent.data(), 4 * (T + Kt)) &&
                    write_all(f, vertex_parents.data(), 16 * Kv);
    if (std::fclose(f) != 0 || !ok) return 2;
    std::printf("OK tets %llu asked %u candidates %u accepted %llu bisected %llu\n", (unsigned long long)T, counters[0], C,
                (unsigned long long)Kv, (unsigned long long)Kt);
    return 0;
}
