// CPU emulation of VERTEX PRUNING (tetra-nerf_amd/csrc/tn_prune.hip) -- test infrastructure, in the pattern of split_emul.cpp.
// The kernels are plain loops over the element functions of tn_prune_core.h, which are the kernels' bodies; the scan is a running
// sum.  tests/test_prune.py compares every output bit for bit with the numpy statements (geometry.prune_vertices_statement,
// geometry.prune_vertex_rows_statement).
// Input file:  u64 V, u64 T, u64 F, u64 rows, u64 has_select, f32 xyz[3V], u32 cells[4T], u8 dead[T], u32 faces[3F],
//              u32 face_tets[2F], u8 select[has_select ? V : 0], f32 values[rows * V].
// Output file: u32 offsets[V+1], u32 counters[5], u32 new_id[V], u32 kept_ids[V'], f32 xyz_out[3V'], f32 out[rows * V'],
//              f32 out_vm[V' * rows]   (V' = offsets[V]).  Prints "OK ...".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tn_prune_core.h"

using namespace tn;

static bool read_all(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_all(std::FILE *f, const void *p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: prune_emul IN OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t h[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 5; ++i)
        if (!read_all(f, &h[i], 8)) return 2;
    const size_t V = h[0], T = h[1], F = h[2], rows = h[3];
    const bool has_select = h[4] != 0;
    if (V >= 0xFFFFFFFFull) { std::fprintf(stderr, "refused\n"); return 3; }
    // exact-size heap arrays: a read or write one element outside is the sanitizer's to see
    std::vector<float> xyz(3 * V), values(rows * V);
    std::vector<uint32_t> cells(4 * T), faces(3 * F), face_tets(2 * F);
    std::vector<uint8_t> dead(T), select(has_select ? V : 0);
    if (!read_all(f, xyz.data(), 12 * V) || !read_all(f, cells.data(), 16 * T) || !read_all(f, dead.data(), T) ||
        !read_all(f, faces.data(), 12 * F) || !read_all(f, face_tets.data(), 8 * F) || !read_all(f, select.data(), select.size()) ||
        !read_all(f, values.data(), 4 * rows * V))
        return 2;
    std::fclose(f);

    // k_prune_mark_tets, k_prune_mark_faces
    std::vector<uint8_t> named(V, 0), live(V, 0), hull(V, 0);
    for (size_t t = 0; t < T; ++t) prune::mark_tet(&cells[4 * t], dead[t] != 0, (uint32_t)V, named.data(), live.data());
    for (size_t i = 0; i < F; ++i) prune::mark_face(&faces[3 * i], face_tets[2 * i + 1], (uint32_t)V, hull.data());

    // k_prune_classify and the exclusive scan
    std::vector<uint32_t> offsets(V + 1, 0u), counters(prune::NUM_COUNTERS, 0u);
    for (size_t v = 0; v < V; ++v) {
        const prune::Outcome o = prune::classify(!has_select || select[v] != 0, named[v] != 0, live[v] != 0, hull[v] != 0);
        offsets[v + 1] = offsets[v] + (o != prune::REMOVED);
        prune::count(o, counters.data());
    }
    const size_t Vp = offsets[V];

    // k_prune_emit
    std::vector<uint32_t> new_id(V), kept_ids(Vp);
    std::vector<float> xyz_out(3 * Vp);
    for (size_t v = 0; v < V; ++v) {
        const uint32_t j = offsets[v];
        const bool kept = offsets[v + 1] > j && j < Vp;
        new_id[v] = kept ? j : prune::EMPTY;
        if (!kept) continue;
        kept_ids[j] = (uint32_t)v;
        for (int a = 0; a < 3; ++a) xyz_out[3 * (size_t)j + a] = xyz[3 * v + a];
    }

    // k_prune_rows
    std::vector<float> out(rows * Vp), out_vm(Vp * rows);
    for (size_t r = 0; r < rows; ++r)
        for (size_t j = 0; j < Vp; ++j) {
            const uint32_t id = kept_ids[j];
            const float v = id < V ? values[r * V + id] : 0.f;
            out[r * Vp + j] = v;
            out_vm[j * rows + r] = v;
        }

    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    const bool ok = write_all(f, offsets.data(), 4 * (V + 1)) && write_all(f, counters.data(), 4 * prune::NUM_COUNTERS) &&
                    write_all(f, new_id.data(), 4 * V) && write_all(f, kept_ids.data(), 4 * Vp) &&
                    write_all(f, xyz_out.data(), 12 * Vp) && write_all(f, out.data(), 4 * rows * Vp) &&
                    write_all(f, out_vm.data(), 4 * rows * Vp);
    if (std::fclose(f) != 0 || !ok) return 2;
    std::printf("OK vertices %llu asked %u removed %u\n", (unsigned long long)V, counters[0], counters[1]);
    return 0;
}
