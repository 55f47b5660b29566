// tn_flip.hip -- tn_flip_count(_tables) and tn_flip_emit: the Delaunay repair by bistellar flips.  A certainly violated interior
// face is removed by a 2-3 or a 3-2 flip; no vertex is added or moved (the rule: tn_flip_core.h).
//
//   k_flip_tet_faces  lane per face: writes its id into tet_faces[t, slot] of its one or two rows (preset to EMPTY); every
//                     (t, slot) has one writer in a face table of the cells, so there is no atomic.
//   k_flip_judge      lane per face: face_tets (8 B), faces (12 B), two cell rows (32 B), five position gathers, the verdict and up
//                     to five orientations in double; a 3-2 candidate looks its third row up through tet_faces / face_tets; a
//                     flippable candidate claims its 2 or 3 rows by atomicMin of its id (preset EMPTY: the result does not depend
//                     on an order).  Writes the face's kind and t2; counts interior / violated / verdict uncertain / refused id /
//                     invalid / uncertain / unflippable.
//   k_flip_decide     lane per face slot [0, F]: a flippable candidate that holds every one of its rows is accepted: face_flip's
//                     code and t2, the 2-3 flag for the scan (slot F writes the 0 the scan turns into K23); counts lost / accepted
//                     2-3 / accepted 3-2.  An exclusive scan ranks the accepted 2-3 flips.
//   k_flip_ranks      lane per face: face_flip's rank.
//   k_flip_tets       lane per tetrahedron slot [0, T]: tet_flip, the flipped byte, and the kept flag whose exclusive scan is
//                     tet_offsets.
//   k_flip_cells      (emit) lane per tetrahedron: copies its row, or writes the child that takes its place (t1 of a 2-3 flip
//                     also the appended one), with cell_sources.
//
// Every kernel is a grid-stride loop on at most FLIP_BLOCKS blocks (tn_mesh_ops.h).  The atomics are the ten counters (one add per
// block and counter) and the claims (atomicMin).  Scratch is ONE stream-ordered allocation (the count entries alone need any).
// Every store is bounded by the counts the caller passed, every id is checked against V, T or F before it is an address.  Nothing
// is read back here.  The byte output is one byte store per lane: no read-modify-write of a shared word.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "tn_build.h"
#include "tn_mesh_ops.h"
#include "tn_flip_core.h"

namespace tn {

namespace {

constexpr int BT = 256;
constexpr unsigned FLIP_BLOCKS = 1024;   // grid cap of every kernel here (TetrahedraTracer.FLIP_GRID_LANES = FLIP_BLOCKS * BT)

__device__ __forceinline__ void load4(const uint32_t *__restrict__ cells, size_t t, uint32_t c[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = cells[4 * t + k];
}
__device__ __forceinline__ void load3(const uint32_t *__restrict__ faces, size_t f, uint32_t v[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = faces[3 * f + k];
}

__global__ __launch_bounds__(BT) void k_flip_tet_faces(size_t F, size_t T, const uint32_t *__restrict__ faces,
                                                       const uint32_t *__restrict__ face_tets, const uint32_t *__restrict__ cells,
                                                       uint32_t *__restrict__ tet_faces) {
    for (size_t f = gid(); f < F; f += stride<BT>()) {
        uint32_t ids[3];
        load3(faces, f, ids);
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const uint32_t t = face_tets[2 * f + side];
            if (t >= T) continue;
            uint32_t c[4];
            load4(cells, t, c);
            const int slot = flip::apex_slot(c, ids);
            if (slot >= 0) tet_faces[4 * (size_t)t + slot] = (uint32_t)f;
        }
    }
}

__global__ __launch_bounds__(BT) void k_flip_judge(size_t F, size_t T, uint32_t V, const float *__restrict__ xyz,
                                                   const uint32_t *__restrict__ cells, const uint32_t *__restrict__ faces,
                                                   const uint32_t *__restrict__ face_tets, const uint32_t *__restrict__ tet_faces,
                                                   uint32_t *__restrict__ kind_out, uint32_t *__restrict__ t2_out, uint32_t *claim,
                                                   uint32_t *__restrict__ counters) {
    uint32_t n[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};   // interior, violated, verdict uncertain, refused id / invalid / uncertain / unflippable
    for (size_t f = gid(); f < F; f += stride<BT>()) {
        const uint32_t t0 = face_tets[2 * f], t1 = face_tets[2 * f + 1];
        uint32_t kind = flip::K_HULL, t2 = flip::EMPTY;
        if (t1 != flip::EMPTY) {
            kind = flip::K_ID;
            if (t0 < T && t1 < T) {
                uint32_t ids[3], c0[4], c1[4];
                load3(faces, f, ids);
                load4(cells, t0, c0);
                load4(cells, t1, c1);
                const flip::Face r = flip::judge_face(ids, c0, c1, V, xyz);
                kind = r.kind;
                if (kind >= flip::FLIP32 && kind < flip::FLIP32 + 3) {
                    t2 = flip::find_t2(ids, (int)(kind - flip::FLIP32), r.d, r.e, t0, t1, c0, c1, T, F, cells, face_tets, tet_faces);
                    if (t2 == flip::EMPTY) kind = flip::K_UNFLIPPABLE;
                }
                if (kind < flip::K_HULL) {   // flippable: t0, t1 < T, and t2 < T where it is not EMPTY
                    atomicMin(claim + t0, (uint32_t)f);
                    atomicMin(claim + t1, (uint32_t)f);
                    if (t2 != flip::EMPTY) atomicMin(claim + t2, (uint32_t)f);
                }
            }
            n[0] += 1u;
            n[1] += kind < flip::K_HULL || kind >= flip::K_INVALID;
            n[2] += kind == flip::K_VERDICT_UNCERTAIN;
            n[3] += kind == flip::K_ID;
            n[4] += kind == flip::K_INVALID;
            n[5] += kind == flip::K_UNCERTAIN;
            n[6] += kind == flip::K_UNFLIPPABLE;
        }
        kind_out[f] = kind;
        t2_out[f] = t2;
    }
    block_count<BT>(n, counters + flip::INTERIOR);
}

__global__ __launch_bounds__(BT) void k_flip_decide(size_t F, size_t T, const uint32_t *__restrict__ face_tets,
                                                    const uint32_t *__restrict__ kind_in, const uint32_t *__restrict__ t2_in,
                                                    const uint32_t *__restrict__ claim, uint32_t *__restrict__ face_flip,
                                                    uint32_t *__restrict__ flags, uint32_t *__restrict__ counters) {
    uint32_t n[3] = {0u, 0u, 0u};   // lost, accepted 2-3, accepted 3-2
    for (size_t f = gid(); f <= F; f += stride<BT>()) {
        uint32_t code = flip::NONE, t2 = flip::EMPTY;
        if (f < F) {
            const uint32_t kind = kind_in[f];
            if (kind != flip::NONE && kind < flip::K_HULL) {   // (its rows were checked against T before they were claimed)
                const uint32_t t0 = face_tets[2 * f], t1 = face_tets[2 * f + 1], third = t2_in[f];
                const bool won = claim[t0] == f && claim[t1] == f && (third == flip::EMPTY || claim[third] == f);
                if (won) { code = kind; t2 = third; }
                n[0] += !won;
                n[1] += won && kind == flip::FLIP23;
                n[2] += won && kind != flip::FLIP23;
            }
            face_flip[3 * f] = code;
            face_flip[3 * f + 1] = t2;
        }
        flags[f] = code == flip::FLIP23;
    }
    block_count<BT>(n, counters + flip::REFUSED_LOST);
}

__global__ __launch_bounds__(BT) void k_flip_ranks(size_t F, const uint32_t *__restrict__ rank, uint32_t *__restrict__ face_flip) {
    for (size_t f = gid(); f < F; f += stride<BT>()) face_flip[3 * f + 2] = face_flip[3 * f] == flip::FLIP23 ? rank[f] : flip::EMPTY;
}

__global__ __launch_bounds__(BT) void k_flip_tets(size_t T, size_t F, const uint32_t *__restrict__ claim,
                                                  const uint32_t *__restrict__ face_flip, const uint32_t *__restrict__ face_tets,
                                                  uint32_t *__restrict__ tet_flip, uint8_t *__restrict__ flipped,
                                                  uint32_t *__restrict__ flags) {
    for (size_t t = gid(); t <= T; t += stride<BT>()) {
        bool kept = false;
        if (t < T) {
            const uint32_t f = claim[t];   // EMPTY, or a face id < F
            const bool taken = f < F && face_flip[3 * (size_t)f] != flip::NONE;
            kept = !taken || face_tets[2 * (size_t)f] == t || face_tets[2 * (size_t)f + 1] == t;
            tet_flip[t] = taken ? f : flip::EMPTY;
            flipped[t] = taken;
        }
        flags[t] = kept;
    }
}

__global__ __launch_bounds__(BT) void k_flip_cells(size_t T, size_t F, const uint32_t *__restrict__ cells,
                                                   const uint32_t *__restrict__ faces, const uint32_t *__restrict__ face_tets,
                                                   const uint32_t *__restrict__ tet_offsets, const uint32_t *__restrict__ tet_flip,
                                                   const uint32_t *__restrict__ face_flip, size_t num_23, size_t num_32,
                                                   uint32_t *__restrict__ cells_out, uint32_t *__restrict__ cell_sources) {
    const size_t kept = T - num_32, rows = kept + num_23;   // (num_32 <= T: checked by the entry)
    for (size_t t = gid(); t < T; t += stride<BT>()) {
        const size_t at = tet_offsets[t];
        if (at >= rows) continue;   // (only where the caller changed the arrays between the two entries)
        uint32_t c[4], src[3] = {(uint32_t)t, flip::EMPTY, flip::EMPTY};
        load4(cells, t, c);
        const uint32_t f = tet_flip[t];
        if (f < F) {
            const uint32_t code = face_flip[3 * (size_t)f], t2 = face_flip[3 * (size_t)f + 1], rank = face_flip[3 * (size_t)f + 2];
            const uint32_t t0 = face_tets[2 * (size_t)f], t1 = face_tets[2 * (size_t)f + 1];
            int ks[3];
            const int good = flip::good_edges(code, ks);
            if (good && t0 < T && t1 < T && (t == t0 || t == t1 || t == t2)) {
                if (t != t0 && t != t1) continue;   // the deleted third row of a 3-2 flip
                uint32_t ids[3], c0[4], c1[4];
                load3(faces, f, ids);
                load4(cells, t0, c0);
                load4(cells, t1, c1);
                const int s0 = flip::apex_slot(c0, ids), s1 = flip::apex_slot(c1, ids);
                if (s0 >= 0 && s1 >= 0) {
                    const uint32_t d = c0[s0], e = c1[s1];
                    src[0] = t0;
                    src[1] = t1;
                    src[2] = good == 2 ? t2 : flip::EMPTY;
                    flip::child_row(ids, ks[t == t0 ? 0 : 1], d, e, c);
                    if (good == 3 && t == t1 && rank < num_23) {
                        uint32_t c2[4];
                        flip::child_row(ids, ks[2], d, e, c2);
                        const size_t tail = kept + rank;   // < rows
#pragma unroll
                        for (int i = 0; i < 4; ++i) cells_out[4 * tail + i] = c2[i];
#pragma unroll
                        for (int i = 0; i < 3; ++i) cell_sources[3 * tail + i] = src[i];
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) cells_out[4 * at + i] = c[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) cell_sources[3 * at + i] = src[i];
    }
}

}  // namespace

void launch_flip_count(size_t V, size_t T, const float *xyz, const uint32_t *cells, size_t F, const uint32_t *faces,
                       const uint32_t *face_tets, uint32_t *tet_offsets, uint32_t *tet_flip, uint8_t *flipped, uint32_t *face_flip,
                       uint32_t *counters, hipStream_t s) {
    TN_HIP(hipMemsetAsync(counters, 0, flip::NUM_COUNTERS * sizeof(uint32_t), s));
    // (T == 0 or F == 0 take the same path: every loop is empty and tet_offsets comes out as the scan of the one flag 0)
    const size_t nt = T + 1, nf = F + 1, n = std::max(nt, nf);
    const size_t tmp_bytes = std::max(scan_bytes(nt, s), scan_bytes(nf, s));   // one scratch for both scans: the larger of what each asks for
    const size_t tf_bytes = align256(4 * T * sizeof(uint32_t)), t_bytes = align256(nt * sizeof(uint32_t)), f_bytes = align256(nf * sizeof(uint32_t));
    const size_t n_bytes = align256(n * sizeof(uint32_t));
    // tet_faces | claims | kinds | third rows | flags to scan | the ranks of the 2-3 flips | rocprim's scratch
    AsyncBytes all(tf_bytes + t_bytes + 2 * f_bytes + n_bytes + f_bytes + tmp_bytes, s);
    uint32_t *tet_faces = all.at<uint32_t>(), *claim = all.at<uint32_t>(tf_bytes), *kind = all.at<uint32_t>(tf_bytes + t_bytes);
    uint32_t *third = all.at<uint32_t>(tf_bytes + t_bytes + f_bytes), *flags = all.at<uint32_t>(tf_bytes + t_bytes + 2 * f_bytes);
    uint32_t *rank = all.at<uint32_t>(tf_bytes + t_bytes + 2 * f_bytes + n_bytes);
    void *tmp = all.p + tf_bytes + t_bytes + 3 * f_bytes + n_bytes;
    const dim3 grid_f(grid_for<BT, FLIP_BLOCKS>(std::max<size_t>(F, 1))), grid_nf(grid_for<BT, FLIP_BLOCKS>(nf)), grid_nt(grid_for<BT, FLIP_BLOCKS>(nt));
    const dim3 block(BT);

    TN_HIP(hipMemsetAsync(tet_faces, 0xFF, tf_bytes + t_bytes, s));   // tet_faces and the claims: EMPTY
    if (F) {
        hipLaunchKernelGGL(k_flip_tet_faces, grid_f, block, 0, s, F, T, faces, face_tets, cells, tet_faces);
        hipLaunchKernelGGL(k_flip_judge, grid_f, block, 0, s, F, T, (uint32_t)V, xyz, cells, faces, face_tets, tet_faces, kind, third,
                           claim, counters);
    }
    hipLaunchKernelGGL(k_flip_decide, grid_nf, block, 0, s, F, T, face_tets, kind, third, claim, face_flip, flags, counters);
    TN_HIP(hipGetLastError());
    scan(tmp, tmp_bytes, flags, rank, nf, s);
    if (F) hipLaunchKernelGGL(k_flip_ranks, grid_f, block, 0, s, F, rank, face_flip);
    hipLaunchKernelGGL(k_flip_tets, grid_nt, block, 0, s, T, F, claim, face_flip, face_tets, tet_flip, flipped, flags);
    TN_HIP(hipGetLastError());
    scan(tmp, tmp_bytes, flags, tet_offsets, nt, s);
}

void launch_flip_emit(size_t T, const uint32_t *cells, size_t F, const uint32_t *faces, const uint32_t *face_tets,
                      const uint32_t *tet_offsets, const uint32_t *tet_flip, const uint32_t *face_flip, size_t num_23, size_t num_32,
                      uint32_t *cells_out, uint32_t *cell_sources, hipStream_t s) {
    if (T)
        hipLaunchKernelGGL(k_flip_cells, dim3(grid_for<BT, FLIP_BLOCKS>(T)), dim3(BT), 0, s, T, F, cells, faces, face_tets, tet_offsets,
                           tet_flip, face_flip, num_23, num_32, cells_out, cell_sources);
    TN_HIP(hipGetLastError());
}

}  // namespace tn
