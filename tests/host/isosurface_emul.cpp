// CPU emulation of the ISOSURFACE EXTRACTION (tetra-nerf_amd/csrc/tn_isosurface.hip) -- test infrastructure, in the pattern of
// delaunay_emul.cpp.  The kernels are plain loops over the element functions of tn_isosurface_core.h, which are the kernels'
// bodies; the scans are running sums and the radix sort is a stable sort on the same key bits.  tests/test_isosurface.py compares
// every output bit for bit with the numpy statement (geometry.isosurface_statement).
// Input file:  u64 V, u64 T, u64 has_mask, f32 level, u32 pad, f32 xyz[3V], u32 cells[4T], f32 values[V], u8 mask[T] (if has_mask).
// Output file: u32 tri_offsets[T+1], u32 ref_offsets[T+1], u64 N, u32 triangles[3M], u32 triangle_tets[M], u32 edge_vertices[2N],
//              f32 edge_t[N], f32 positions[3N]  (M = tri_offsets[T]).  Prints "OK ...".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "tn_isosurface_core.h"

using namespace tn;

static bool read_all(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_all(std::FILE *f, const void *p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

struct Mesh {
    uint64_t V = 0, T = 0;
    float level = 0.f;
    std::vector<float> xyz, values;
    std::vector<uint32_t> cells;
    std::vector<uint8_t> mask;
    bool has_mask = false;
};

// tet_case of the kernels
static iso::TetCase tet_case(const Mesh &m, size_t t, uint32_t c[4]) {
    const iso::TetCase none{0u, 0u, 0u, 0u};
    if (m.has_mask && m.mask[t] == 0) return none;
    for (int k = 0; k < 4; ++k) c[k] = m.cells[4 * t + k];
    if (!iso::ids_ok(c, (uint32_t)m.V)) return none;
    float v[4];
    for (int k = 0; k < 4; ++k) v[k] = m.values[c[k]];
    return iso::classify(v, m.level);
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: isosurface_emul IN OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    Mesh m;
    uint64_t has_mask = 0;
    uint32_t pad = 0;
    if (!read_all(f, &m.V, 8) || !read_all(f, &m.T, 8) || !read_all(f, &has_mask, 8) || !read_all(f, &m.level, 4) || !read_all(f, &pad, 4))
        return 2;
    m.has_mask = has_mask != 0;
    m.xyz.resize(3 * m.V); m.values.resize(m.V); m.cells.resize(4 * m.T); m.mask.resize(m.has_mask ? m.T : 0);
    if (!read_all(f, m.xyz.data(), 12 * m.V) || !read_all(f, m.cells.data(), 16 * m.T) || !read_all(f, m.values.data(), 4 * m.V) ||
        !read_all(f, m.mask.data(), m.mask.size()))
        return 2;
    std::fclose(f);
    if (!iso::in_range(m.level) || m.T >= iso::MAX_TETS || m.V >= 0xFFFFFFFFull) { std::fprintf(stderr, "refused\n"); return 3; }
    const size_t T = m.T;
    const uint32_t V = (uint32_t)m.V;

    // k_iso_count and the two exclusive scans
    std::vector<uint32_t> tri_offsets(T + 1, 0u), ref_offsets(T + 1, 0u);
    for (size_t t = 0; t < T; ++t) {
        uint32_t c[4];
        const iso::TetCase k = tet_case(m, t, c);
        tri_offsets[t + 1] = tri_offsets[t] + k.ntri;
        ref_offsets[t + 1] = ref_offsets[t] + k.nref;
    }
    const size_t M = tri_offsets[T], R = ref_offsets[T];

    // k_iso_fill, k_iso_keys
    std::vector<uint64_t> keys(R, ~0ull);
    std::vector<uint32_t> slots(R);
    std::iota(slots.begin(), slots.end(), 0u);
    for (size_t t = 0; t < T; ++t) {
        uint32_t c[4];
        const iso::TetCase k = tet_case(m, t, c);
        size_t slot = ref_offsets[t];
        for (int e = 0; e < 6; ++e)
            if ((k.cross >> e) & 1u) {
                if (slot < R) keys[slot] = iso::edge_key(c[iso::EDGE_CORNERS[e][0]], c[iso::EDGE_CORNERS[e][1]]);
                ++slot;
            }
    }
    // the radix sort: stable, on bits [0, 32 + bit_width(V - 1))
    unsigned end_bit = 32;
    for (uint64_t v = V > 1 ? V - 1 : 0; v; v >>= 1) ++end_bit;
    const uint64_t bits = end_bit >= 64 ? ~0ull : ((1ull << end_bit) - 1);
    std::stable_sort(slots.begin(), slots.end(), [&](uint32_t a, uint32_t b) { return (keys[a] & bits) < (keys[b] & bits); });
    std::vector<uint64_t> sorted_keys(R);
    for (size_t i = 0; i < R; ++i) sorted_keys[i] = keys[slots[i]];

    // k_iso_heads, the scan, k_iso_vertices
    std::vector<uint32_t> below(R + 1, 0u), slot_id(R, 0u);
    for (size_t i = 0; i < R; ++i) below[i + 1] = below[i] + (i == 0 || sorted_keys[i] != sorted_keys[i - 1]);
    const uint64_t N = R ? below[R] : 0;
    std::vector<uint32_t> edge_vertices(2 * N);
    std::vector<float> edge_t(N), positions(3 * N);
    for (size_t i = 0; i < R; ++i) {
        const uint32_t id = below[i + 1] - 1u;
        if (slots[i] < R) slot_id[slots[i]] = id;
        if (below[i + 1] != below[i]) {
            const uint32_t a = (uint32_t)(sorted_keys[i] >> 32), b = (uint32_t)sorted_keys[i];
            float t = 0.f, p[3] = {0.f, 0.f, 0.f};
            if (a < V && b < V) t = iso::edge_vertex(m.values[a], m.values[b], m.level, &m.xyz[3 * (size_t)a], &m.xyz[3 * (size_t)b], p);
            edge_vertices[2 * (size_t)id] = a;
            edge_vertices[2 * (size_t)id + 1] = b;
            edge_t[id] = t;
            for (int k = 0; k < 3; ++k) positions[3 * (size_t)id + k] = p[k];
        }
    }

    // k_iso_triangles
    std::vector<uint32_t> triangles(3 * M), triangle_tets(M);
    for (size_t t = 0; t < T; ++t) {
        uint32_t c[4];
        const iso::TetCase k = tet_case(m, t, c);
        if (k.ntri == 0) continue;
        float p[4][3];
        for (int j = 0; j < 4; ++j) for (int a = 0; a < 3; ++a) p[j][a] = m.xyz[3 * (size_t)c[j] + a];
        const bool negative = guard::tet_orient(p) < 0;
        for (uint32_t row = 0; row < k.ntri; ++row) {
            const size_t tri = tri_offsets[t] + row;
            if (tri >= M) break;
            for (int j = 0; j < 3; ++j) {
                const size_t slot = ref_offsets[t] + iso::edge_rank(k.cross, iso::TRI_TABLE[k.code][row][iso::tri_corner(j, negative)]);
                triangles[3 * tri + j] = slot < R ? slot_id[slot] : 0u;
            }
            triangle_tets[tri] = (uint32_t)t;
        }
    }

    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    const bool ok = write_all(f, tri_offsets.data(), 4 * (T + 1)) && write_all(f, ref_offsets.data(), 4 * (T + 1)) && write_all(f, &N, 8) &&
                    write_all(f, triangles.data(), 12 * M) && write_all(f, triangle_tets.data(), 4 * M) &&
                    write_all(f, edge_vertices.data(), 8 * N) && write_all(f, edge_t.data(), 4 * N) && write_all(f, positions.data(), 12 * N);
    if (std::fclose(f) != 0 || !ok) return 2;
    std::printf("OK tets %llu triangles %llu refs %llu vertices %llu\n", (unsigned long long)T, (unsigned long long)M,
                (unsigned long long)R, (unsigned long long)N);
    return 0;
}
