// tn_fill.hip -- the constant tails of the trace rows: three kernels that write the same bytes, and their launcher.
// k_write_segments (tn_trace_walk.hip) writes a certified row up to the next multiple of 32 slots; everything behind it
// is visited / verts = TN_EMPTY, bary / dist = 0 and comes from here.
#include "tn_device.h"
#include "tn_kernels.h"

namespace tn {

namespace {

// fill dwords [start, end) of `base` with `value`; base 16-byte aligned.  Wave-cooperative.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool NT = false>
__device__ __forceinline__ void fill_dwords(uint32_t *__restrict__ base, uint32_t start, uint32_t end, uint32_t value, int lane) {
    const uint32_t a0 = (start + 3u) & ~3u;  // first 16-B aligned dword
    const uint32_t head_end = a0 < end ? a0 : end;
    if (start + lane < head_end) base[start + lane] = value;
    if (a0 >= end) return;
    const uint32_t a1 = end & ~3u;
    u32x4 *b4 = reinterpret_cast<u32x4 *>(base);
    const u32x4 v4 = {value, value, value, value};
    for (uint32_t i = (a0 >> 2) + lane; i < (a1 >> 2); i += 64) {
        // plain stores: nontemporal ones measured slower for a pure write stream running alone; NT = the fill that
        // streams BESIDE the walk (the walk's records then stay in the XCD's L2)
        if constexpr (NT) __builtin_nontemporal_store(v4, b4 + i);
        else b4[i] = v4;
    }
    if (a1 + lane < end) base[a1 + lane] = value;
}

}  // namespace

// Constant tails: pure streaming stores (16 B per lane, whole 128-byte lines), a contiguous span of rows per wave.
// This is the bulk of the bytes of a trace_rays call (88 % at M = 512) and runs at the write ceiling.  Two uses:
//   all_rows = 1: slots [k_split, M) of EVERY row -- needs nothing from the walk, so it streams beside it (speculative
//                 fill, tn_api_tracer.hip).  Rows of literal / fallback rays and rays with more than k_split segments are
//                 included: the kernels that write those slots are ordered behind this one.
//   all_rows = 0: slots [ceil32(n), k_split) of the certified rows (k_write_segments has written [0, ceil32(n))).
template <bool NT>
__global__ __launch_bounds__(256) void k_fill_range(size_t num_rays, uint32_t M, uint32_t all_rows, uint32_t k_split,
                                                    const uint32_t *__restrict__ walk_n, const uint32_t *__restrict__ out_num,
                                                    uint32_t *__restrict__ out_cells,
                                                    float *__restrict__ out_bary, float *__restrict__ out_dist,
                                                    uint32_t *__restrict__ out_verts) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // row span, row bases: scalar
    const size_t nwaves = (size_t)gridDim.x * 4;
    const size_t span = (num_rays + nwaves - 1) / nwaves;   // consecutive rows are consecutive in memory
    const size_t r0 = ((size_t)blockIdx.x * 4 + wave) * span;
    const size_t r1 = r0 + span < num_rays ? r0 + span : num_rays;
    for (size_t r = r0; r < r1; ++r) {
        uint32_t lo = k_split, hi = M;
        if (!all_rows) {
            if (walk_n[r] == TN_EMPTY) continue;  // literal / fallback ray: those kernels write the whole row
            lo = (out_num[r] + 31u) & ~31u;
            if (lo > M) lo = M;
            hi = k_split;
        }
        if (lo >= hi) continue;
        fill_dwords<NT>(out_cells + r * M, lo, hi, TN_EMPTY, lane);
        fill_dwords<NT>(reinterpret_cast<uint32_t *>(out_dist + r * M * 2), 2 * lo, 2 * hi, 0u, lane);
        fill_dwords<NT>(reinterpret_cast<uint32_t *>(out_bary + r * M * 6), 6 * lo, 6 * hi, 0u, lane);
        if (out_verts) fill_dwords<NT>(out_verts + r * M * 4, 4 * lo, 4 * hi, TN_EMPTY, lane);
    }
}

// The same rows with the work cut FINE: one block per row, its four waves take 6-8 KB each (cells + distances | first half
// of the barycentrics | second half | vertex ids), six to eight 1 KB store instructions per wave and the block is gone.
// Rows in flight form one moving window per array and the dispatcher balances the channels: with long-lived waves that
// own fixed spans of rows the same 17 GB took 2.40 ... 3.07 ms depending on WHERE the driver had put the pages (fresh
// allocations of the same rows in one process, profiles/r06s_placement.txt), torch's own one-store-per-thread fill of the
// same pages 2.43 ... 2.50 ms (profiles/r06s_torch_fill.txt).
template <bool NT>
__global__ __launch_bounds__(256) void k_fill_rows_fine(size_t num_rays, uint32_t M, uint32_t all_rows, uint32_t k_split,
                                                        const uint32_t *__restrict__ walk_n, const uint32_t *__restrict__ out_num,
                                                        uint32_t *__restrict__ out_cells,
                                                        float *__restrict__ out_bary, float *__restrict__ out_dist,
                                                        uint32_t *__restrict__ out_verts) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const size_t r = blockIdx.x;
    uint32_t lo = k_split, hi = M;
    if (!all_rows) {
        if (walk_n[r] == TN_EMPTY) return;        // literal / fallback ray: those kernels write the whole row
        lo = (out_num[r] + 31u) & ~31u;
        if (lo > M) lo = M;
        hi = k_split;
    }
    if (lo >= hi) return;
    const uint32_t mid = 6u * lo + ((3u * (hi - lo) + 3u) & ~3u);   // 16-byte aligned when lo is
    uint32_t *bary = reinterpret_cast<uint32_t *>(out_bary + r * M * 6);
    if (wave == 0) {
        fill_dwords<NT>(out_cells + r * M, lo, hi, TN_EMPTY, lane);
        fill_dwords<NT>(reinterpret_cast<uint32_t *>(out_dist + r * M * 2), 2 * lo, 2 * hi, 0u, lane);
    } else if (wave == 1) {
        fill_dwords<NT>(bary, 6 * lo, mid < 6 * hi ? mid : 6 * hi, 0u, lane);
    } else if (wave == 2) {
        if (mid < 6 * hi) fill_dwords<NT>(bary, mid, 6 * hi, 0u, lane);
    } else if (out_verts) {
        fill_dwords<NT>(out_verts + r * M * 4, 4 * lo, 4 * hi, TN_EMPTY, lane);
    }
}

// The same rows as ONE LINEAR STREAM PER ARRAY, the arrays one after the other, one 16-byte store per thread and the thread
// is gone (round 6, the last of the fill experiments and the first to explain them).  Fresh allocations of the same rows
// in one process (same virtual addresses, new physical pages) moved every fill that writes the four arrays IN STEP -- rows
// dealt to persistent waves, a block per row, even torch-style one-store blocks interleaved 1 : 2 : 6 : 4 -- between 5.6 and
// 7.1 TB/s, while a single linear stream (this order; torch's own fill) stays at 7.0 - 7.15 TB/s wherever the pages lie
// (profiles/r06s_flat_fill.txt, r06s_torch_fill.txt, r06s_placement.txt).
//   block -> (array, 256 consecutive 16-byte units of it); a row holds M/4, M/2, 3M/2, M units (cells, distances,
//   barycentrics, vertex ids): powers of two and 3 x a power of two, so the row of a unit costs a shift (and a division by 3).
template <bool NT, bool UNI>
__global__ __launch_bounds__(256) void k_fill_linear(size_t num_rays, uint32_t M, uint32_t all_rows, uint32_t k_split, uint32_t log2_m4,
                                                     unsigned long long n_bary, unsigned long long n_verts, unsigned long long n_dist,
                                                     const uint32_t *__restrict__ walk_n, const uint32_t *__restrict__ out_num,
                                                     uint32_t *__restrict__ out_cells, float *__restrict__ out_bary,
                                                     float *__restrict__ out_dist, uint32_t *__restrict__ out_verts) {
    // n_bary / n_verts / n_dist: first block of the NEXT array (blocks are dealt bary, verts, dist, cells: largest first)
    unsigned long long b = blockIdx.x;
    u32x4 *base; uint32_t w4, sh; uint32_t val; bool three = false;     // w4 = 16-byte units per 4 slots; units per row = (M/4 << sh) (x3)
    if (b < n_bary) { base = reinterpret_cast<u32x4 *>(out_bary); w4 = 6; sh = 1; three = true; val = 0u; }
    else if (b < n_verts) { b -= n_bary; base = reinterpret_cast<u32x4 *>(out_verts); w4 = 4; sh = 2; val = TN_EMPTY; }
    else if (b < n_dist) { b -= n_verts; base = reinterpret_cast<u32x4 *>(out_dist); w4 = 2; sh = 1; val = 0u; }
    else { b -= n_dist; base = reinterpret_cast<u32x4 *>(out_cells); w4 = 1; sh = 0; val = TN_EMPTY; }
    const unsigned long long g = b * 256ull + threadIdx.x;             // unit of the array
    const uint32_t q = (uint32_t)(g >> (log2_m4 + sh));                // (x3 arrays: the row's third; else the row)
    const uint32_t row = three ? q / 3u : q;
    if (row >= num_rays) return;
    const uint32_t upr = (three ? 3u : 1u) << (log2_m4 + sh);          // units per row
    const uint32_t off = (uint32_t)(g - (unsigned long long)row * upr);
    uint32_t lo = k_split, hi = M;
    if (!all_rows) {
        // (a per-row lookup in front of the one store: the wave then lives for a load latency per KB and the fill is bound by
        // THAT -- 6.0 instead of 3.3 ms per C2 frame; four chunks per block with the lookups up front: 4.2 ms and the pure
        // fill falls to 6.0 - 6.5 TB/s; the lookup through the scalar cache (this code): 5.4 ms; a block per row with the
        // arrays one after the other: 4.1 ms, steadier (3.97 - 4.21) but never below the block-per-row fill of all four
        // arrays (3.24 - 4.02); profiles/r06ac_linear_sweep*.txt, r06ae_*.txt.  So the tracer's tail fill, which needs
        // the lookup, stays with k_fill_rows_fine, and this kernel serves tn_fill_rows and option fill_blocks = -2)
        uint32_t wn, n;
        if constexpr (UNI) {   // M >= 256: a wave's 64 units lie in one row -> the lookup goes through the scalar cache
            const uint32_t rs = (uint32_t)__builtin_amdgcn_readfirstlane((int)row);
            wn = walk_n[rs]; n = out_num[rs];
        } else {
            wn = walk_n[row]; n = out_num[row];
        }
        if (wn == TN_EMPTY) return;               // literal / fallback ray: those kernels write the whole row
        lo = (n + 31u) & ~31u;
        if (lo > M) lo = M;
        hi = k_split;
    }
    // lo, hi are multiples of 4 slots: [lo, hi) slots = [lo / 4 * w4, hi / 4 * w4) units
    if (off < (lo >> 2) * w4 || off >= (hi >> 2) * w4) return;
    const u32x4 v4 = {val, val, val, val};
    if constexpr (NT) __builtin_nontemporal_store(v4, base + g);
    else base[g] = v4;
}

namespace {
// the <true> (nontemporal stores) or <false> instantiation of a fill kernel
template <typename Kernel>
Kernel store_kind(bool nontemporal, Kernel nt, Kernel plain) { return nontemporal ? nt : plain; }
}  // namespace

void launch_fill(const Rows &rows, size_t num_rays, const uint32_t *walk_n, const FillRange &f, hipStream_t stream) {
    if (num_rays == 0) return;
    const uint32_t M = rows.M, all_rows = f.all_rows ? 1u : 0u;
    // one launch per piece of at most `cap` rows (grid limits of the two kernels whose grid grows with the rows)
    auto for_pieces = [&](size_t cap, auto &&launch) {
        for (size_t base = 0; base < num_rays; base += cap)
            launch(rows.at(base), walk_n ? walk_n + base : nullptr, num_rays - base < cap ? num_rays - base : cap);
    };
    switch (f.kind) {
    case FillKind::Linear: {
        if (M < 4 || (M & (M - 1)) != 0) throw Error("k_fill_linear: M must be a power of two >= 4");
        uint32_t log2_m4 = 0;
        while ((4u << log2_m4) < M) ++log2_m4;
        const auto kern = M >= 256 ? store_kind(f.nontemporal, k_fill_linear<true, true>, k_fill_linear<false, true>)
                                   : store_kind(f.nontemporal, k_fill_linear<true, false>, k_fill_linear<false, false>);
        // 2^21 rows x 13 M / 1024 blocks (1.1e8 at M = 4096) stays below 2^31
        for_pieces(0x200000u, [&](const Rows &r, const uint32_t *wn, size_t n) {
            const unsigned long long u_cells = (unsigned long long)n * (M / 4);
            auto blocks_of = [](unsigned long long units) { return (units + 255ull) / 256ull; };
            const unsigned long long nb = blocks_of(6 * u_cells), nv = nb + (r.verts ? blocks_of(4 * u_cells) : 0ull),
                                     nd = nv + blocks_of(2 * u_cells), total = nd + blocks_of(u_cells);
            if (total > 0x7FFFFFFFull) throw Error("k_fill_linear: grid too large");
            hipLaunchKernelGGL(kern, dim3((unsigned)total), dim3(256), 0, stream, n, M, all_rows, f.k_split, log2_m4, nb, nv, nd,
                               wn, r.num, r.cells, r.bary, r.dist, r.verts);
        });
        return;
    }
    case FillKind::RowPerBlock: {
        const auto kern = store_kind(f.nontemporal, k_fill_rows_fine<true>, k_fill_rows_fine<false>);
        for_pieces(0x40000000u, [&](const Rows &r, const uint32_t *wn, size_t n) {     // grid.x limit
            hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(256), 0, stream, n, M, all_rows, f.k_split, wn, r.num, r.cells, r.bary,
                               r.dist, r.verts);
        });
        return;
    }
    case FillKind::Spans: {
        size_t blocks = (num_rays + 3) / 4;           // >= one ray per wave
        // after the writer: 2 blocks (8 waves) per CU hold the write ceiling, and the latency-bound kernels running beside
        // the fill are less starved than with 8 per CU (profiles/r01_fill_grid.txt); beside the walk: 2048 blocks
        // (profiles/r02p_specfill2.txt)
        const size_t cap = f.blocks ? f.blocks : (f.all_rows ? 2048 : 256 * 2);
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(store_kind(f.nontemporal, k_fill_range<true>, k_fill_range<false>), dim3((unsigned)blocks), dim3(256), 0,
                           stream, num_rays, M, all_rows, f.k_split, walk_n, rows.num, rows.cells, rows.bary, rows.dist, rows.verts);
        return;
    }
    }
}

}  // namespace tn
