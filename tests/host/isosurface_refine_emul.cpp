// CPU emulation of the ISOSURFACE REFINEMENT (tetra-nerf_amd/csrc/tn_isosurface_refine.hip) -- test infrastructure, in the pattern
// of isosurface_emul.cpp.  The four kernels are plain loops over the element functions of tn_isosurface_core.h, which are the
// kernels' bodies.  tests/test_isosurface_refine.py compares every output bit for bit with the numpy statement
// (geometry.isosurface_refine_statement).
// Input file:  u64 V, u64 N, u64 rounds, u64 kind, f32 level, u32 pad, f32 xyz[3V], u32 edge_vertices[2N], f32 values[V], and for
//              kind 0 the densities f32 [rounds][N][7] the caller's network gave at the candidates; kind 1 evaluates
//              -(|p|^2) at p = xa + t (xb - xa) in fp32, one rounding per operation, summed x, y, z in that order.
// Output file: per round r = 0 .. rounds - 1: u32 vertex_indices[N][7][4], f32 barycentric[N][7][3]; then for r = 0 .. rounds:
//              f32 brackets[N][4], u8 flags[N]; then f32 edge_t[N], f32 positions[3N].  Prints "OK ...".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tn_isosurface_core.h"

using namespace tn;

static bool read_all(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_all(std::FILE *f, const void *p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

constexpr int C = iso::REFINE_CANDIDATES;

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: isosurface_refine_emul IN OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t V64 = 0, N = 0, rounds = 0, kind = 0;
    float level = 0.f;
    uint32_t pad = 0;
    if (!read_all(f, &V64, 8) || !read_all(f, &N, 8) || !read_all(f, &rounds, 8) || !read_all(f, &kind, 8) || !read_all(f, &level, 4) ||
        !read_all(f, &pad, 4))
        return 2;
    if (!iso::in_range(level) || rounds > iso::REFINE_MAX_ROUNDS || V64 >= 0xFFFFFFFFull || kind > 1) { std::fprintf(stderr, "refused\n"); return 3; }
    const uint32_t V = (uint32_t)V64;
    std::vector<float> xyz(3 * V64), values(V64), given(kind == 0 ? rounds * N * C : 0);
    std::vector<uint32_t> ev(2 * N);
    if (!read_all(f, xyz.data(), 12 * V64) || !read_all(f, ev.data(), 8 * N) || !read_all(f, values.data(), 4 * V64) ||
        !read_all(f, given.data(), 4 * given.size()))
        return 2;
    std::fclose(f);
    if (N && V == 0 && rounds) { std::fprintf(stderr, "refused\n"); return 3; }   // tn_isosurface_refine_points: candidates name vertex 0

    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    bool ok = true;

    // k_iso_refine_begin
    std::vector<iso::Bracket> brackets(N);
    std::vector<uint8_t> flags(N);
    for (size_t i = 0; i < N; ++i) flags[i] = iso::refine_begin(ev[2 * i], ev[2 * i + 1], V, values.data(), level, brackets[i]);

    std::vector<uint32_t> vi(4 * C * N);
    std::vector<float> bc(3 * C * N), dens(C * N);
    std::vector<std::vector<iso::Bracket>> history{brackets};
    std::vector<std::vector<uint8_t>> flag_history{flags};
    for (uint64_t r = 0; r < rounds; ++r) {
        // k_iso_refine_points
        for (size_t i = 0; i < N * C; ++i) {
            const size_t v = i / C;
            const int j = (int)(i - v * C) + 1;
            uint32_t a = ev[2 * v], b = ev[2 * v + 1];
            if (flags[v] & iso::REFINE_BAD_IDS) a = b = 0u;
            vi[4 * i] = a; vi[4 * i + 1] = b; vi[4 * i + 2] = a; vi[4 * i + 3] = a;
            bc[3 * i] = iso::refine_candidate(brackets[v].t_lo, brackets[v].t_hi, j);
            bc[3 * i + 1] = 0.f;
            bc[3 * i + 2] = 0.f;
        }
        ok = ok && write_all(f, vi.data(), 4 * vi.size()) && write_all(f, bc.data(), 4 * bc.size());
        // the caller's densities
        for (size_t i = 0; i < N * C; ++i) {
            if (kind == 0) { dens[i] = given[r * N * C + i]; continue; }
            const uint32_t a = vi[4 * i], b = vi[4 * i + 1];
            float sum = 0.f;
            for (int k = 0; k < 3; ++k) {
                const float xa = xyz[3 * (size_t)a + k], xb = xyz[3 * (size_t)b + k];
                const float p = iso::fadd(xa, iso::fmul(bc[3 * i], iso::fsub(xb, xa)));
                sum = k ? iso::fadd(sum, iso::fmul(p, p)) : iso::fmul(p, p);
            }
            dens[i] = -sum;
        }
        // k_iso_refine_select
        for (size_t i = 0; i < N; ++i) {
            if (flags[i]) continue;
            iso::Bracket br = brackets[i];
            const uint8_t now = iso::refine_select(br, &dens[C * i], level, flags[i]);
            if (now) flags[i] = now;
            else brackets[i] = br;
        }
        history.push_back(brackets);
        flag_history.push_back(flags);
    }
    for (size_t r = 0; r < history.size(); ++r)
        ok = ok && write_all(f, history[r].data(), 16 * N) && write_all(f, flag_history[r].data(), N);

    // k_iso_refine_vertices
    std::vector<float> edge_t(N), positions(3 * N);
    for (size_t i = 0; i < N; ++i) {
        const uint32_t a = ev[2 * i], b = ev[2 * i + 1];
        float t = 0.f, p[3] = {0.f, 0.f, 0.f};
        if (a < V && b < V) t = iso::refine_vertex(brackets[i], level, &xyz[3 * (size_t)a], &xyz[3 * (size_t)b], p);
        edge_t[i] = t;
        for (int k = 0; k < 3; ++k) positions[3 * i + k] = p[k];
    }
    ok = ok && write_all(f, edge_t.data(), 4 * N) && write_all(f, positions.data(), 12 * N);
    if (std::fclose(f) != 0 || !ok) return 2;
    std::printf("OK vertices %llu rounds %llu\n", (unsigned long long)N, (unsigned long long)rounds);
    return 0;
}
