// face_table_emul.cpp -- tn_face_table_count / tn_face_table_emit (csrc/tn_build.hip) on the CPU: the element functions of
// csrc/tn_build_core.h (face_hash_insert, face_is_first, face_emit) called in a loop where the kernels call them per lane.  The
// sightings go into the hash once in ascending order and once in a fixed shuffled order: the pairs, and with them the whole
// table, must not depend on the schedule (with a face in three rows only the flag is compared: which two pair is left open).
// Stand-alone (its own main), so that it can be built with -fsanitize=address,undefined and run as it is.
//
//   face_table_emul in.bin out.bin
//   in.bin   u64 V, u64 T, u32 cells[4T]
//   out.bin  u32 counters[4], partner[4T], face_index[4T + 1], faces[3F], face_tets[2F], tet_faces[4T]   (F = counters[0])
// Prints "OK ..." and returns 0; anything else is a failure.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "tn_build_core.h"

using namespace tn;

namespace {

struct Table {
    std::vector<uint32_t> partner, face_index, faces, face_tets, tet_faces;
    uint32_t counters[4] = {0, 0, 0, 0};
};

// the launcher and its kernels, one loop per kernel; `order` is the schedule of k_face_hash
Table build(uint64_t V, size_t T, const std::vector<uint32_t> &cells, const std::vector<uint32_t> &order) {
    const size_t n4 = 4 * T;
    Table t;
    size_t cap = 16;
    while (cap < 8 * T + 16) cap <<= 1;
    std::vector<uint32_t> slot(cap, TN_EMPTY), first(n4 + 1, 0u);
    t.partner.assign(n4, TN_EMPTY);
    t.face_index.assign(n4 + 1, 0u);
    for (uint32_t i : order) core::face_hash_insert(i, cells.data(), slot.data(), cap - 1, t.partner.data(), &t.counters[2]);   // k_face_hash
    for (size_t i = 0; i < n4; ++i) first[i] = core::face_is_first((uint32_t)i, t.partner.data()) ? 1u : 0u;                    // k_face_first
    for (size_t i = 0; i < n4; ++i) {                                                                                           // k_face_table_counters
        t.counters[0] += core::face_is_first((uint32_t)i, t.partner.data()) ? 1u : 0u;
        t.counters[1] += t.partner[i] == TN_EMPTY ? 1u : 0u;
        if ((uint64_t)cells[i] >= V) t.counters[2] |= core::FLAG_CELL_OOB;
    }
    std::exclusive_scan(first.begin(), first.end(), t.face_index.begin(), 0u);
    const uint32_t F = t.face_index[n4];                                          // the caller's read-back
    t.faces.assign(3 * (size_t)F, 0x7F7F7F7Fu);
    t.face_tets.assign(2 * (size_t)F, 0x7F7F7F7Fu);
    t.tet_faces.assign(n4, 0x7F7F7F7Fu);
    for (size_t i = 0; i < n4; ++i) {                                                                                           // k_face_table_emit
        const uint32_t p = t.partner[i];
        if (p != TN_EMPTY && (p >= n4 || p <= i)) continue;
        const uint32_t f = t.face_index[i];
        if (f < F) core::face_emit((uint32_t)i, f, cells.data(), t.partner.data(), t.faces.data(), t.face_tets.data(), t.tet_faces.data());
    }
    return t;
}

bool put(std::FILE *f, const std::vector<uint32_t> &v) { return v.empty() || std::fwrite(v.data(), 4, v.size(), f) == v.size(); }

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::printf("usage: face_table_emul in.bin out.bin\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    uint64_t head[2];
    if (!f || std::fread(head, 8, 2, f) != 2) { std::printf("ERROR cannot read %s\n", argv[1]); return 2; }
    const uint64_t V = head[0];
    const size_t T = (size_t)head[1], n4 = 4 * T;
    std::vector<uint32_t> cells(n4);
    if (n4 && std::fread(cells.data(), 4, n4, f) != n4) { std::printf("ERROR short input\n"); return 2; }
    std::fclose(f);

    std::vector<uint32_t> ascending(n4), shuffled(n4);
    std::iota(ascending.begin(), ascending.end(), 0u);
    shuffled = ascending;
    uint64_t state = 0x9E3779B97F4A7C15ull;                                       // Fisher-Yates on a fixed 64-bit LCG
    for (size_t i = n4; i > 1; --i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(shuffled[i - 1], shuffled[(size_t)((state >> 33) % i)]);
    }
    const Table a = build(V, T, cells, ascending), b = build(V, T, cells, shuffled);
    for (int k = 0; k < 4; ++k)
        if (a.counters[k] != b.counters[k]) { std::printf("ERROR counter %d depends on the schedule: %u vs %u\n", k, a.counters[k], b.counters[k]); return 1; }
    if (!(a.counters[2] & core::FLAG_TRIPLE_FACE) &&
        (a.partner != b.partner || a.face_index != b.face_index || a.faces != b.faces || a.face_tets != b.face_tets || a.tet_faces != b.tet_faces)) {
        std::printf("ERROR the table depends on the schedule\n");
        return 1;
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(a.counters, 4, 4, f) != 4 || !put(f, a.partner) || !put(f, a.face_index) || !put(f, a.faces) || !put(f, a.face_tets) ||
        !put(f, a.tet_faces)) { std::printf("ERROR cannot write %s\n", argv[2]); return 2; }
    std::fclose(f);
    std::printf("OK T %zu F %u hull %u flags %u\n", T, a.counters[0], a.counters[1], a.counters[2]);
    return 0;
}
