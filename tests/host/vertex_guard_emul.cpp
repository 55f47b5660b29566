// CPU emulation of the VERTEX STEP LIMITER (tetra-nerf_amd/csrc/tn_vertex_guard.hip) -- test infrastructure, in the pattern of
// refit_emul.cpp.  The three kernels are plain loops over the element functions of tn_vertex_guard_core.h, which are the kernels'
// bodies; tests/test_vertex_guard.py compares every output bit for bit with the torch statement (geometry.py).
// Input file:  u64 V, u64 T, f32 fraction, u32 flags (bit 0: skip the verify pass), f32 xyz_old[3V], f32 xyz_new[3V], u32 cells[4T].
// Output file: u32 star_width[V], u32 width[T], i8 orient[T], f32 xyz_out[3V], u32 counters[4].  Prints "OK ...".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tn_vertex_guard_core.h"

using namespace tn;

static bool read_all(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_all(std::FILE *f, const void *p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

static void gather(const uint32_t *c, const float *xyz, float p[4][3]) {
    for (int k = 0; k < 4; ++k) for (int a = 0; a < 3; ++a) p[k][a] = xyz[3 * (size_t)c[k] + a];
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: vertex_guard_emul IN OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t V = 0, T = 0;
    float fraction = 0.f;
    uint32_t flags = 0;
    if (!read_all(f, &V, 8) || !read_all(f, &T, 8) || !read_all(f, &fraction, 4) || !read_all(f, &flags, 4)) return 2;
    std::vector<float> xo(3 * V), xn(3 * V);
    std::vector<uint32_t> cells(4 * T);
    if (!read_all(f, xo.data(), 12 * V) || !read_all(f, xn.data(), 12 * V) || !read_all(f, cells.data(), 16 * T)) return 2;
    std::fclose(f);
    for (uint32_t c : cells)
        if (c >= V) { std::fprintf(stderr, "cell id out of range\n"); return 2; }

    // k_star_width (after the +inf fill)
    std::vector<uint32_t> star(V, guard::INF_BITS), width(T);
    std::vector<int8_t> orient(T);
    for (size_t i = 0; i < T; ++i) {
        float p[4][3];
        gather(&cells[4 * i], xo.data(), p);
        const guard::WidthOrient r = guard::tet_width_orient(p);
        width[i] = r.width_bits;
        orient[i] = (int8_t)r.orient;
        for (int k = 0; k < 4; ++k) {
            uint32_t &m = star[cells[4 * i + k]];
            m = r.width_bits < m ? r.width_bits : m;
        }
    }
    // k_clamp_vertices
    uint32_t counters[4] = {0, 0, 0, 0};
    for (size_t v = 0; v < V; ++v) {
        float sw, out[3];
        std::memcpy(&sw, &star[v], 4);
        int kind;
        guard::clamp_vertex(&xo[3 * v], &xn[3 * v], sw, fraction, out, &kind);
        if (kind == guard::CLAMPED || kind == guard::FROZEN_MOVED)
            for (int a = 0; a < 3; ++a) xn[3 * v + a] = out[a];
        counters[0] += kind == guard::CLAMPED;
        counters[1] += kind == guard::FROZEN_MOVED;
    }
    // k_verify_orient
    if (!(flags & 1u))
        for (size_t i = 0; i < T; ++i) {
            float p[4][3];
            gather(&cells[4 * i], xo.data(), p);
            const int before = guard::tet_orient(p);
            gather(&cells[4 * i], xn.data(), p);
            const int after = guard::tet_orient(p);
            counters[2] += before * after < 0;
            counters[3] += before != 0 && after == 0;
        }

    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    const bool ok = write_all(f, star.data(), 4 * V) && write_all(f, width.data(), 4 * T) && write_all(f, orient.data(), T) &&
                    write_all(f, xn.data(), 12 * V) && write_all(f, counters, 16);
    if (std::fclose(f) != 0 || !ok) return 2;
    std::printf("OK vertices %llu tets %llu clamped %u frozen_moved %u flipped %u collapsed %u\n", (unsigned long long)V,
                (unsigned long long)T, counters[0], counters[1], counters[2], counters[3]);
    return 0;
}
