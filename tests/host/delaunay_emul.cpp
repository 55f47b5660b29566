// CPU emulation of the DELAUNAY MONITOR and the per-tetrahedron STATE TRANSFER (tetra-nerf_amd/csrc/tn_delaunay.hip) -- test
// infrastructure, in the pattern of vertex_guard_emul.cpp.  The three kernels are plain loops over the element functions of
// tn_delaunay_core.h, which are the kernels' bodies; tests/test_delaunay.py compares every output bit for bit with the numpy
// statement (geometry.py).
// Input file:  u64 V, u64 T, u64 F, u64 T2, f32 xyz[3V], u32 cells[4T], u32 face_tets[2F], f32 values[T], u32 new_cells[4 T2].
// Output file: i8 face_state[F], u8 tet_violations[T], u32 counters[4], u32 star_max[V], u32 new_values[T2].  Prints "OK ...".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tn_delaunay_core.h"

using namespace tn;

static constexpr uint32_t EMPTY = 0xFFFFFFFFu;

static bool read_all(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_all(std::FILE *f, const void *p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: delaunay_emul IN OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t V = 0, T = 0, F = 0, T2 = 0;
    if (!read_all(f, &V, 8) || !read_all(f, &T, 8) || !read_all(f, &F, 8) || !read_all(f, &T2, 8)) return 2;
    std::vector<float> xyz(3 * V), values(T);
    std::vector<uint32_t> cells(4 * T), face_tets(2 * F), new_cells(4 * T2);
    if (!read_all(f, xyz.data(), 12 * V) || !read_all(f, cells.data(), 16 * T) || !read_all(f, face_tets.data(), 8 * F) ||
        !read_all(f, values.data(), 4 * T) || !read_all(f, new_cells.data(), 16 * T2))
        return 2;
    std::fclose(f);
    for (uint32_t c : cells)
        if (c >= V) { std::fprintf(stderr, "cell id out of range\n"); return 2; }
    for (size_t i = 0; i < 2 * F; ++i)
        if (face_tets[i] >= T && !((i & 1) && face_tets[i] == EMPTY)) { std::fprintf(stderr, "face_tets out of range\n"); return 2; }

    // k_delaunay_faces (after the two fills with 0)
    std::vector<int8_t> face_state(F);
    std::vector<uint32_t> viol_words((T + 3) / 4, 0u);
    uint32_t counters[4] = {0, 0, 0, 0};
    for (size_t fi = 0; fi < F; ++fi) {
        const uint32_t t0 = face_tets[2 * fi], t1 = face_tets[2 * fi + 1];
        int state = delaunay::HULL;
        if (t1 != EMPTY) {
            const uint32_t *c0 = &cells[4 * (size_t)t0], *c1 = &cells[4 * (size_t)t1];
            const uint32_t ev = delaunay::opposite_vertex(c0, c1);
            float p[4][3], e[3];
            for (int k = 0; k < 4; ++k) for (int a = 0; a < 3; ++a) p[k][a] = xyz[3 * (size_t)c0[k] + a];
            for (int a = 0; a < 3; ++a) e[a] = xyz[3 * (size_t)ev + a];
            const delaunay::Verdict v = delaunay::face_verdict(p, e);
            state = v.state;
            counters[0] += 1;
            counters[1] += state == delaunay::VIOLATED;
            counters[2] += state == delaunay::UNCERTAIN;
            counters[3] += v.inverted;
            if (state == delaunay::VIOLATED) {
                viol_words[t0 >> 2] += 1u << (8 * (t0 & 3));
                viol_words[t1 >> 2] += 1u << (8 * (t1 & 3));
            }
        }
        face_state[fi] = (int8_t)state;
    }
    std::vector<uint8_t> tet_violations(T);
    for (size_t t = 0; t < T; ++t) tet_violations[t] = (uint8_t)(viol_words[t >> 2] >> (8 * (t & 3)));

    // k_star_max (after the fill with 0), then k_remap
    std::vector<uint32_t> star(V, 0u), out(T2);
    for (size_t i = 0; i < T; ++i) {
        uint32_t bits;
        std::memcpy(&bits, &values[i], 4);
        if (bits == 0) continue;
        for (int k = 0; k < 4; ++k) {
            const uint32_t v = cells[4 * i + k];
            if (v < V) star[v] = delaunay::max_bits(star[v], bits);
        }
    }
    for (size_t i = 0; i < T2; ++i) {
        uint32_t m = 0;
        for (int k = 0; k < 4; ++k) {
            const uint32_t v = new_cells[4 * i + k];
            m = delaunay::max_bits(m, v < V ? star[v] : 0u);
        }
        out[i] = m;
    }

    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    const bool ok = write_all(f, face_state.data(), F) && write_all(f, tet_violations.data(), T) && write_all(f, counters, 16) &&
                    write_all(f, star.data(), 4 * V) && write_all(f, out.data(), 4 * T2);
    if (std::fclose(f) != 0 || !ok) return 2;
    std::printf("OK faces %llu interior %u violated %u uncertain %u inverted %u\n", (unsigned long long)F, counters[0], counters[1],
                counters[2], counters[3]);
    return 0;
}
