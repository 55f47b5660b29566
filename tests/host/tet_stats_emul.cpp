// CPU emulation of the PER-TETRAHEDRON TRAINING STATISTICS kernel (tetra-nerf_amd/csrc/tn_tet_stats.hip) -- test infrastructure,
// in the pattern of split_emul.cpp.  The three scalar rules are tn_tet_stats_core.h's, the very functions the kernel calls; the
// wave is modelled lane by lane: 64 lanes per chunk, run heads from a ballot, the segmented sum in six shuffle steps bounded by
// the distance to the next head (every step reads the values of the step before, as a shuffle does), the open run carried from
// chunk to chunk, and an "atomic" is a plain add behind a bounds check.  The weights are an INPUT (the kernel takes them from
// rayops::ray_composite; the host's expf is not the device's).  tests/test_tet_stats.py compares the output with the numpy
// statement (render.tet_stats_statement) byte for byte.
// Input file:  u64 T, rows, S, count, has_ray_index, rays (0: no ray_value); u32 cells[rows * S], f32 weights[rows * S],
//              u32 ray_index[rows] (if has_ray_index), f32 ray_value[rays], i64 stats[3 T].
// Output file: i64 stats[3 T].  Prints "OK <atomic adds issued>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tn_tet_stats_core.h"

using namespace tn;

static bool read_all(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

static std::vector<int64_t> stats;
static uint64_t adds = 0;

static void add_run(uint32_t c, uint32_t h, uint64_t w, uint64_t e) {
    if (3 * (size_t)c + 2 >= stats.size()) { std::fprintf(stderr, "atomic outside stats: cell %u\n", c); std::exit(4); }
    stats[3 * (size_t)c] = (int64_t)((uint64_t)stats[3 * (size_t)c] + h);
    stats[3 * (size_t)c + 1] = (int64_t)((uint64_t)stats[3 * (size_t)c + 1] + w);
    stats[3 * (size_t)c + 2] = (int64_t)((uint64_t)stats[3 * (size_t)c + 2] + e);
    adds += 3;
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: tet_stats_emul IN OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t hdr[6];
    if (!read_all(f, hdr, sizeof hdr)) return 2;
    const size_t T64 = hdr[0], rows = hdr[1], S = hdr[2], rays = hdr[5];
    const bool has_index = hdr[4] != 0;
    if (T64 >= 0xFFFFFFFFull || S == 0) { std::fprintf(stderr, "refused\n"); return 3; }
    const uint32_t T = (uint32_t)T64, EMPTY = 0xFFFFFFFFu;
    // exact-size heap arrays: a read or write one element outside is the sanitizer's to see
    std::vector<uint32_t> cells(rows * S), ray_index(has_index ? rows : 0);
    std::vector<float> weights(rows * S), ray_value(rays);
    stats.resize(3 * (size_t)T);
    if (!read_all(f, cells.data(), 4 * rows * S) || !read_all(f, weights.data(), 4 * rows * S) ||
        !read_all(f, ray_index.data(), 4 * ray_index.size()) || !read_all(f, ray_value.data(), 4 * rays) ||
        !read_all(f, stats.data(), 8 * stats.size()))
        return 2;
    std::fclose(f);

    const size_t R = hdr[3] < rows ? (size_t)hdr[3] : rows;     // rows from *count on are not read
    for (size_t q = 0; q < R; ++q) {
        const float v = rays ? ray_value.at(has_index ? ray_index[q] : q) : 1.0f;
        uint32_t cc = EMPTY, ch = 0;
        uint64_t cw = 0, ce = 0;
        for (size_t base = 0; base < S; base += 64) {
            uint32_t c[64], h[64];
            uint64_t w[64], e[64];
            for (int lane = 0; lane < 64; ++lane) {
                const size_t j = base + lane;
                c[lane] = EMPTY; h[lane] = 0; w[lane] = 0; e[lane] = 0;
                if (j < S && tetstats::accept(cells[q * S + j], T)) {
                    const float wj = weights[q * S + j];
                    c[lane] = cells[q * S + j];
                    h[lane] = 1;
                    w[lane] = (uint64_t)tetstats::weight_term(wj);
                    e[lane] = (uint64_t)tetstats::error_term(wj, v);
                }
            }
            uint64_t heads = 0;
            for (int lane = 0; lane < 64; ++lane)
                if (lane == 0 || c[lane - 1] != c[lane]) heads |= 1ull << lane;
            int len[64];
            for (int lane = 0; lane < 64; ++lane) {
                const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
                len[lane] = above ? __builtin_ffsll((long long)above) : 64 - lane;
            }
            for (int off = 1; off < 64; off <<= 1) {
                uint32_t oh[64];
                uint64_t ow[64], oe[64];
                for (int lane = 0; lane < 64; ++lane) {              // __shfl_down: a lane past the wave reads its own value
                    const int src = lane + off < 64 ? lane + off : lane;
                    oh[lane] = h[src]; ow[lane] = w[src]; oe[lane] = e[src];
                }
                for (int lane = 0; lane < 64; ++lane)
                    if (off < len[lane]) { h[lane] += oh[lane]; w[lane] += ow[lane]; e[lane] += oe[lane]; }
            }
            if (cc != EMPTY) {
                if (c[0] == cc) { h[0] += ch; w[0] += cw; e[0] += ce; }
                else add_run(cc, ch, cw, ce);
            }
            const int last = 63 - __builtin_clzll(heads);
            cc = c[last]; ch = h[last]; cw = w[last]; ce = e[last];
            for (int lane = 0; lane < 64; ++lane)
                if ((heads >> lane & 1) && lane != last && c[lane] != EMPTY) add_run(c[lane], h[lane], w[lane], e[lane]);
        }
        if (cc != EMPTY) add_run(cc, ch, cw, ce);
    }

    std::FILE *g = std::fopen(argv[2], "wb");
    if (!g) { std::perror(argv[2]); return 2; }
    if (stats.size() && std::fwrite(stats.data(), 8, stats.size(), g) != stats.size()) return 2;
    std::fclose(g);
    std::printf("OK %llu\n", (unsigned long long)adds);
    return 0;
}
