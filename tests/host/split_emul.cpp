// CPU emulation of the TETRAHEDRON SPLIT (tetra-nerf_amd/csrc/tn_split.hip) -- test infrastructure, in the pattern of
// isosurface_emul.cpp.  The kernels are plain loops over the element functions of tn_split_core.h, which are the kernels' bodies;
// the scan is a running sum.  tests/test_split.py compares every output bit for bit with the numpy statements
// (geometry.split_tetrahedra_statement, geometry.split_vertex_rows_statement).
// Input file:  u64 V, u64 T, u64 rows, u64 new_mode, f32 xyz[3V], u32 cells[4T], u8 select[T], f32 values[rows * V].
// Output file: u32 offsets[T+1], u32 counters[4], f32 xyz_out[3(V+K)], u32 cells_out[4(T+3K)], u32 cell_parent[T+3K],
//              u32 vertex_parents[4K], f32 out[rows * (V+K)], f32 out_vm[(V+K) * rows]   (K = offsets[T]).  Prints "OK ...".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tn_split_core.h"

using namespace tn;

static bool read_all(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_all(std::FILE *f, const void *p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: split_emul IN OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t V64 = 0, T64 = 0, rows64 = 0, mode64 = 0;
    if (!read_all(f, &V64, 8) || !read_all(f, &T64, 8) || !read_all(f, &rows64, 8) || !read_all(f, &mode64, 8)) return 2;
    const size_t V = V64, T = T64, rows = rows64;
    // exact-size heap arrays: a read or write one element outside is the sanitizer's to see
    std::vector<float> xyz(3 * V), values(rows * V);
    std::vector<uint32_t> cells(4 * T);
    std::vector<uint8_t> select(T);
    if (!read_all(f, xyz.data(), 12 * V) || !read_all(f, cells.data(), 16 * T) || !read_all(f, select.data(), T) ||
        !read_all(f, values.data(), 4 * rows * V))
        return 2;
    std::fclose(f);
    if (T >= split::MAX_CELLS || V >= 0xFFFFFFFFull || mode64 > split::MODE_ZERO) { std::fprintf(stderr, "refused\n"); return 3; }

    // k_split_flags and the exclusive scan
    std::vector<uint32_t> offsets(T + 1, 0u), counters(4, 0u);
    for (size_t t = 0; t < T; ++t) {
        float cen[3];
        const split::Verdict v = split::judge(select[t] != 0, &cells[4 * t], (uint32_t)V, xyz.data(), cen);
        offsets[t + 1] = offsets[t] + (v == split::ACCEPTED);
        counters[0] += v != split::NOT_ASKED;
        counters[1] += v == split::ACCEPTED;
        counters[2] += v == split::REFUSED_FLAT;
        counters[3] += v == split::REFUSED_ID;
    }
    const size_t K = offsets[T];
    if (T + 3 * K >= split::MAX_CELLS || V + K >= 0xFFFFFFFFull) { std::fprintf(stderr, "refused\n"); return 3; }

    // the copy of the old vertices and k_split_cells
    std::vector<float> xyz_out(3 * (V + K));
    std::vector<uint32_t> cells_out(4 * (T + 3 * K)), cell_parent(T + 3 * K), vertex_parents(4 * K);
    for (size_t i = 0; i < 3 * V; ++i) xyz_out[i] = xyz[i];
    for (size_t t = 0; t < T; ++t) {
        const uint32_t *c = &cells[4 * t];
        const size_t k = offsets[t];
        const bool accepted = offsets[t + 1] > offsets[t] && k < K;
        cell_parent[t] = (uint32_t)t;
        if (!accepted) {
            for (int j = 0; j < 4; ++j) cells_out[4 * t + j] = c[j];
            continue;
        }
        float cen[3] = {0.f, 0.f, 0.f};
        if (iso::ids_ok(c, (uint32_t)V)) {
            float p[4][3];
            for (int j = 0; j < 4; ++j) for (int a = 0; a < 3; ++a) p[j][a] = xyz[3 * (size_t)c[j] + a];
            split::centroid(p, cen);
        }
        const uint32_t v = (uint32_t)V + (uint32_t)k;
        for (int a = 0; a < 3; ++a) xyz_out[3 * (size_t)v + a] = cen[a];
        for (int j = 0; j < 4; ++j) vertex_parents[4 * k + j] = c[j];
        for (int i = 0; i < 4; ++i) {
            const size_t row = split::child_slot(T, t, k, i);
            uint32_t child[4];
            split::child_row(c, i, v, child);
            for (int j = 0; j < 4; ++j) cells_out[4 * row + j] = child[j];
            cell_parent[row] = (uint32_t)t;
        }
    }

    // k_split_copy_rows and k_split_new_columns
    std::vector<float> out(rows * (V + K)), out_vm((V + K) * rows);
    for (size_t r = 0; r < rows; ++r) {
        for (size_t i = 0; i < V; ++i) out[r * (V + K) + i] = values[r * V + i];
        for (size_t k = 0; k < K; ++k) {
            const uint32_t *p = &vertex_parents[4 * k];
            float v = 0.f;
            if (mode64 == split::MODE_MEAN && iso::ids_ok(p, (uint32_t)V))
                v = split::mean4(values[r * V + p[0]], values[r * V + p[1]], values[r * V + p[2]], values[r * V + p[3]]);
            out[r * (V + K) + V + k] = v;
        }
        for (size_t i = 0; i < V + K; ++i) out_vm[i * rows + r] = out[r * (V + K) + i];
    }

    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    const bool ok = write_all(f, offsets.data(), 4 * (T + 1)) && write_all(f, counters.data(), 16) &&
                    write_all(f, xyz_out.data(), 12 * (V + K)) && write_all(f, cells_out.data(), 16 * (T + 3 * K)) &&
                    write_all(f, cell_parent.data(), 4 * (T + 3 * K)) && write_all(f, vertex_parents.data(), 16 * K) &&
                    write_all(f, out.data(), 4 * rows * (V + K)) && write_all(f, out_vm.data(), 4 * rows * (V + K));
    if (std::fclose(f) != 0 || !ok) return 2;
    std::printf("OK tets %llu asked %u accepted %llu\n", (unsigned long long)T, counters[0], (unsigned long long)K);
    return 0;
}
