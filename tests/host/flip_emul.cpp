// CPU emulation of the DELAUNAY REPAIR BY FLIPS (tetra-nerf_amd/csrc/tn_flip.hip) -- test infrastructure, in the pattern of
// edge_split_emul.cpp.  The kernels are plain loops over the element functions of tn_flip_core.h, which are the kernels' bodies;
// the scans are running sums, an atomicMin is a min.  tests/test_flip.py compares every output bit for bit with the numpy
// statement (geometry.flip_faces_statement).
// Input file:  u64 V, u64 T, u64 F, f32 xyz[3V], u32 cells[4T], u32 faces[3F], u32 face_tets[2F].
// Output file: u32 counters[10], u32 tet_offsets[T+1], u32 tet_flip[T], u8 flipped[T], u32 face_flip[3F], u32 cells_out[4T'],
//              u32 cell_sources[3T'] (T' = T + counters[8] - counters[9]).  Prints "OK ...".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tn_flip_core.h"

using namespace tn;

static bool read_all(std::FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_all(std::FILE *f, const void *p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: flip_emul IN OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint64_t V64 = 0, T64 = 0, F64 = 0;
    if (!read_all(f, &V64, 8) || !read_all(f, &T64, 8) || !read_all(f, &F64, 8)) return 2;
    const size_t V = V64, T = T64, F = F64;
    // exact-size heap arrays: a read or write one element outside is the sanitizer's to see
    std::vector<float> xyz(3 * V);
    std::vector<uint32_t> cells(4 * T), faces(3 * F), face_tets(2 * F);
    if (!read_all(f, xyz.data(), 12 * V) || !read_all(f, cells.data(), 16 * T) || !read_all(f, faces.data(), 12 * F) ||
        !read_all(f, face_tets.data(), 8 * F))
        return 2;
    std::fclose(f);
    if (T >= flip::MAX_CELLS || V >= 0xFFFFFFFFull || F >= 0xFFFFFFFFull) { std::fprintf(stderr, "refused\n"); return 3; }
    const uint32_t Vu = (uint32_t)V;

    std::vector<uint32_t> counters(flip::NUM_COUNTERS, 0u), tet_offsets(T + 1, 0u), tet_flip(T, flip::EMPTY), face_flip(3 * F);
    std::vector<uint8_t> flipped(T, 0);
    // k_flip_tet_faces
    std::vector<uint32_t> tet_faces(4 * T, flip::EMPTY), claim(T, flip::EMPTY), kind(F), third(F);
    for (size_t i = 0; i < F; ++i)
        for (int side = 0; side < 2; ++side) {
            const uint32_t t = face_tets[2 * i + side];
            if (t >= T) continue;
            const int slot = flip::apex_slot(&cells[4 * (size_t)t], &faces[3 * i]);
            if (slot >= 0) tet_faces[4 * (size_t)t + slot] = (uint32_t)i;
        }
    // k_flip_judge
    for (size_t i = 0; i < F; ++i) {
        const uint32_t t0 = face_tets[2 * i], t1 = face_tets[2 * i + 1];
        uint32_t k = flip::K_HULL, t2 = flip::EMPTY;
        if (t1 != flip::EMPTY) {
            k = flip::K_ID;
            if (t0 < T && t1 < T) {
                const uint32_t *ids = &faces[3 * i], *c0 = &cells[4 * (size_t)t0], *c1 = &cells[4 * (size_t)t1];
                const flip::Face r = flip::judge_face(ids, c0, c1, Vu, xyz.data());
                k = r.kind;
                if (k >= flip::FLIP32 && k < flip::FLIP32 + 3) {
                    t2 = flip::find_t2(ids, (int)(k - flip::FLIP32), r.d, r.e, t0, t1, c0, c1, T, F, cells.data(), face_tets.data(),
                                       tet_faces.data());
                    if (t2 == flip::EMPTY) k = flip::K_UNFLIPPABLE;
                }
                if (k < flip::K_HULL) {
                    claim.at(t0) = std::min(claim.at(t0), (uint32_t)i);
                    claim.at(t1) = std::min(claim.at(t1), (uint32_t)i);
                    if (t2 != flip::EMPTY) claim.at(t2) = std::min(claim.at(t2), (uint32_t)i);
                }
            }
            counters[flip::INTERIOR] += 1u;
            counters[flip::VIOLATED] += k < flip::K_HULL || k >= flip::K_INVALID;
            counters[flip::VERDICT_UNCERTAIN] += k == flip::K_VERDICT_UNCERTAIN;
            counters[flip::REFUSED_ID] += k == flip::K_ID;
            counters[flip::REFUSED_INVALID] += k == flip::K_INVALID;
            counters[flip::REFUSED_UNCERTAIN] += k == flip::K_UNCERTAIN;
            counters[flip::REFUSED_UNFLIPPABLE] += k == flip::K_UNFLIPPABLE;
        }
        kind[i] = k;
        third[i] = t2;
    }
    // k_flip_decide, its scan, k_flip_ranks
    uint32_t rank = 0;
    for (size_t i = 0; i < F; ++i) {
        uint32_t code = flip::NONE, t2 = flip::EMPTY;
        if (kind[i] != flip::NONE && kind[i] < flip::K_HULL) {
            const uint32_t t0 = face_tets[2 * i], t1 = face_tets[2 * i + 1];
            const bool won = claim.at(t0) == i && claim.at(t1) == i && (third[i] == flip::EMPTY || claim.at(third[i]) == i);
            if (won) { code = kind[i]; t2 = third[i]; }
            counters[flip::REFUSED_LOST] += !won;
            counters[flip::ACCEPTED_23] += won && kind[i] == flip::FLIP23;
            counters[flip::ACCEPTED_32] += won && kind[i] != flip::FLIP23;
        }
        face_flip[3 * i] = code;
        face_flip[3 * i + 1] = t2;
        face_flip[3 * i + 2] = code == flip::FLIP23 ? rank : flip::EMPTY;
        rank += code == flip::FLIP23;
    }
    // k_flip_tets and its scan
    for (size_t t = 0; t < T; ++t) {
        const uint32_t i = claim[t];
        const bool taken = i < F && face_flip[3 * (size_t)i] != flip::NONE;
        const bool kept = !taken || face_tets[2 * (size_t)i] == t || face_tets[2 * (size_t)i + 1] == t;
        tet_flip[t] = taken ? i : flip::EMPTY;
        flipped[t] = taken;
        tet_offsets[t + 1] = tet_offsets[t] + kept;
    }
    const size_t K23 = counters[flip::ACCEPTED_23], K32 = counters[flip::ACCEPTED_32];
    if (T + K23 >= flip::MAX_CELLS || 2 * K23 + 3 * K32 > T) { std::fprintf(stderr, "refused\n"); return 3; }

    // k_flip_cells
    const size_t kept_rows = T - K32, rows = kept_rows + K23;
    std::vector<uint32_t> cells_out(4 * rows), cell_sources(3 * rows);
    for (size_t t = 0; t < T; ++t) {
        const size_t at = tet_offsets[t];
        if (at >= rows) continue;
        uint32_t c[4], src[3] = {(uint32_t)t, flip::EMPTY, flip::EMPTY};
        for (int j = 0; j < 4; ++j) c[j] = cells[4 * t + j];
        const uint32_t i = tet_flip[t];
        if (i < F) {
            const uint32_t code = face_flip[3 * (size_t)i], t2 = face_flip[3 * (size_t)i + 1], rk = face_flip[3 * (size_t)i + 2];
            const uint32_t t0 = face_tets[2 * (size_t)i], t1 = face_tets[2 * (size_t)i + 1];
            int ks[3];
            const int good = flip::good_edges(code, ks);
            if (good && t0 < T && t1 < T && (t == t0 || t == t1 || t == t2)) {
                if (t != t0 && t != t1) continue;
                const uint32_t *ids = &faces[3 * (size_t)i], *c0 = &cells[4 * (size_t)t0], *c1 = &cells[4 * (size_t)t1];
                const int s0 = flip::apex_slot(c0, ids), s1 = flip::apex_slot(c1, ids);
                if (s0 >= 0 && s1 >= 0) {
                    const uint32_t d = c0[s0], e = c1[s1];
                    src[0] = t0;
                    src[1] = t1;
                    src[2] = good == 2 ? t2 : flip::EMPTY;
                    flip::child_row(ids, ks[t == t0 ? 0 : 1], d, e, c);
                    if (good == 3 && t == t1 && rk < K23) {
                        uint32_t c2[4];
                        flip::child_row(ids, ks[2], d, e, c2);
                        const size_t tail = kept_rows + rk;
                        for (int j = 0; j < 4; ++j) cells_out.at(4 * tail + j) = c2[j];
                        for (int j = 0; j < 3; ++j) cell_sources.at(3 * tail + j) = src[j];
                    }
                }
            }
        }
        for (int j = 0; j < 4; ++j) cells_out.at(4 * at + j) = c[j];
        for (int j = 0; j < 3; ++j) cell_sources.at(3 * at + j) = src[j];
    }

    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    const bool ok = write_all(f, counters.data(), 4 * flip::NUM_COUNTERS) && write_all(f, tet_offsets.data(), 4 * (T + 1)) &&
                    write_all(f, tet_flip.data(), 4 * T) && write_all(f, flipped.data(), T) && write_all(f, face_flip.data(), 12 * F) &&
                    write_all(f, cells_out.data(), 16 * rows) && write_all(f, cell_sources.data(), 12 * rows);
    if (std::fclose(f) != 0 || !ok) return 2;
    std::printf("OK tets %llu faces %llu violated %u flips 2-3 %llu 3-2 %llu\n", (unsigned long long)T, (unsigned long long)F,
                counters[flip::VIOLATED], (unsigned long long)K23, (unsigned long long)K32);
    return 0;
}
