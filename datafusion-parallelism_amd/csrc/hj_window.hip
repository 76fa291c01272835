// hj_window.hip — pair plan (scan + compaction) and pair window for gfx950.
//
// The reference's get_matching_indices (src/shared/shared.rs:29-47) emits a probe batch's
// pairs in one piece. Here the pairs of one probe call can be had in slices of the canonical
// order: a plan says how many pairs every matched row has and where they start, a window
// writes pairs [lo, lo + capacity) from it. The plan's first pass (the lookup) is
// pair_plan_lookup_kernel in hj_match.hip; this file needs the table only for the
// duplicate segments and the explicit ids (hj_device.h).
//
//   pass 2  pair_plan_scan_kernel     one workgroup: exclusive scan of the blocks' (matched,
//                                     pairs) totals, the header, offsets[m] and *d_total.
//                                     A launch of its own: no workgroup ever waits for another.
//   pass 3  pair_plan_compact_kernel  one workgroup per block of kPlanBlockRows rows: the
//                                     matched rows' (row, ref) and the exclusive prefix of
//                                     their pair counts, at the block's scanned base.
//   window  pair_window_kernel        one workgroup per kWinTile output pairs. Wave 0 finds
//                                     the matched row holding the tile's first rank by a
//                                     64-ary search of `offsets`. Every matched row has at
//                                     least one pair, so the tile touches at most kWinTile
//                                     consecutive entries whatever the probe's hit rate: their
//                                     start positions are scattered into LDS and max-scanned,
//                                     which gives every output position its entry. Stores are
//                                     contiguous; a hot key's segment is read contiguously.
//                                     The work depends on the capacity and log(m), not on n,
//                                     on the misses or on pair_lo.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hj_device.h"
#include "hj_launch.h"
#include "hj_util.h"

namespace dfp {

namespace {
constexpr int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }
}  // namespace

PlanLayout pair_plan_layout(int64_t n) {
    PlanLayout L;
    L.nblocks = (n + kPlanBlockRows - 1) / kPlanBlockRows;
    L.offsets = kPlanHeaderBytes;
    L.entries = L.offsets + align16(8 * (n + 1));
    L.refs = L.entries + align16(8 * n);
    L.counts = L.refs + align16(4 * n);
    L.blocks = L.counts + align16(4 * n);
    L.bytes = L.blocks + align16(16 * L.nblocks);
    return L;
}

__global__ void __launch_bounds__(kPlanScanThreads)
pair_plan_scan_kernel(unsigned long long* __restrict__ btot, int64_t nblocks, unsigned long long* __restrict__ header,
                      unsigned long long* __restrict__ offsets, long long* __restrict__ d_total) {
    __shared__ unsigned long long s_w[kPlanScanThreads / 64];
    unsigned long long run_m, run_p;
    scan_block_totals(btot, nblocks, s_w, &run_m, &run_p);
    if (threadIdx.x == 0) {
        header[0] = run_m;
        header[1] = run_p;
        offsets[run_m] = run_p;  // run_m <= n: the offsets hold n + 1 words
        if (d_total != nullptr) *d_total = (long long)run_p;
    }
}

constexpr int kCompactThreads = kPlanBlockRows / 4;

__global__ void __launch_bounds__(kCompactThreads)
pair_plan_compact_kernel(const uint32_t* __restrict__ refs, const uint32_t* __restrict__ counts, bool svec, int64_t n,
                         const unsigned long long* __restrict__ btot, uint2* __restrict__ entries,
                         unsigned long long* __restrict__ offsets) {
    __shared__ unsigned long long s_m[kCompactThreads / 64], s_p[kCompactThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * kPlanBlockRows + (int64_t)threadIdx.x * 4;
    uint32_t ref[4] = {kMiss, kMiss, kMiss, kMiss}, cnt[4] = {0, 0, 0, 0};
    load4_u32(refs, row0, n, svec, ref);
    load4_u32(counts, row0, n, svec, cnt);
    uint32_t mc = 0;
    unsigned long long pc = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        mc += cnt[q] != 0;
        pc += cnt[q];
    }
    const uint32_t im = wave_incl_scan_dpp(mc);
    const unsigned long long ip = wave_incl_scan<unsigned long long>(pc);
    if (lane == 63) { s_m[wave] = im; s_p[wave] = ip; }
    __syncthreads();
    unsigned long long e = btot[2 * (int64_t)blockIdx.x] + (im - mc);
    unsigned long long o = btot[2 * (int64_t)blockIdx.x + 1] + (ip - pc);
    for (int w = 0; w < wave; ++w) { e += s_m[w]; o += s_p[w]; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (cnt[q] != 0) {  // a row of the block, so e < the block's base + its matched rows <= n
            entries[e] = make_uint2((uint32_t)(row0 + q), ref[q]);
            offsets[e] = o;
            ++e;
            o += cnt[q];
        }
    }
}

hipError_t launch_pair_plan_finish(void* plan, int64_t n, int64_t* d_total, hipStream_t s) {
    const PlanLayout L = pair_plan_layout(n);
    char* p = static_cast<char*>(plan);
    unsigned long long* header = reinterpret_cast<unsigned long long*>(p);
    unsigned long long* offsets = reinterpret_cast<unsigned long long*>(p + L.offsets);
    unsigned long long* btot = reinterpret_cast<unsigned long long*>(p + L.blocks);
    pair_plan_scan_kernel<<<1, kPlanScanThreads, 0, s>>>(btot, L.nblocks, header, offsets, reinterpret_cast<long long*>(d_total));
    if (L.nblocks > 0) {
        const bool svec = (reinterpret_cast<uintptr_t>(plan) & 15) == 0;
        pair_plan_compact_kernel<<<(unsigned)L.nblocks, kCompactThreads, 0, s>>>(
            reinterpret_cast<const uint32_t*>(p + L.refs), reinterpret_cast<const uint32_t*>(p + L.counts), svec, n, btot,
            reinterpret_cast<uint2*>(p + L.entries), offsets);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// window
// ---------------------------------------------------------------------------
constexpr int kWinThreads = 256;
constexpr int kWinPer = kWinTile / kWinThreads;  // consecutive LDS positions per thread in the max-scan
constexpr int kWinPosBits = 11;
static_assert((1 << kWinPosBits) == kWinTile, "an LDS word packs (entry in tile, start in tile)");
static_assert(kWinPer == 8, "the scan reads its positions as two 16-byte LDS words");

template <bool HAS_ROW_IDS, bool HAS_PROBE_IDS>
__global__ void __launch_bounds__(kWinThreads)
pair_window_kernel(const uint32_t* __restrict__ dup_rows, const uint64_t* __restrict__ row_ids, uint32_t off_mask,
                   const unsigned long long* __restrict__ header, const unsigned long long* __restrict__ offsets,
                   const uint2* __restrict__ entries, const uint32_t* __restrict__ probe_ids, uint32_t pbase,
                   unsigned long long pair_lo, unsigned long long cap, uint64_t* __restrict__ out_b,
                   uint32_t* __restrict__ out_p, long long* __restrict__ d_written) {
    // s_seg[i]: (entry - e0) << 11 | start position, of the entry that starts at output
    // position i of the tile (0 elsewhere); after the max-scan, of the entry that holds i
    __shared__ __attribute__((aligned(16))) uint32_t s_seg[kWinTile];
    __shared__ uint32_t s_w[kWinThreads / 64];
    __shared__ unsigned long long s_e0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = header[0], total = header[1];
    unsigned long long w = pair_lo < total ? total - pair_lo : 0ull;
    w = w < cap ? w : cap;
    if (blockIdx.x == 0 && threadIdx.x == 0 && d_written != nullptr) *d_written = (long long)w;
    const unsigned long long t0 = (unsigned long long)blockIdx.x * kWinTile;
    if (t0 >= w) return;  // the whole workgroup: the grid follows the capacity, not the pairs
    const uint32_t len = (uint32_t)(w - t0 < (unsigned long long)kWinTile ? w - t0 : (unsigned long long)kWinTile);
    const unsigned long long r0 = pair_lo + t0;  // rank of the tile's first pair, < total
    if (wave == 0) {
        // offsets[lo] <= r0 < offsets[hi] (offsets[0] = 0, offsets[m] = total > r0; m >= 1):
        // 64 probes per round split [lo, hi) into pieces of `step` entries
        unsigned long long lo = 0, hi = m;
        while (hi - lo > 1) {
            const unsigned long long step = (hi - lo + 63) >> 6;
            const unsigned long long idx = lo + (unsigned long long)(lane + 1) * step;
            const bool le = idx < hi && offsets[idx] <= r0;  // true for a prefix of the lanes
            const unsigned long long c = (unsigned long long)__popcll(__ballot(le));
            lo += c * step;
            hi = hi < lo + step ? hi : lo + step;
        }
        if (lane == 0) s_e0 = lo;
    }
#pragma unroll
    for (int k = 0; k < kWinPer; ++k) s_seg[threadIdx.x + k * kWinThreads] = 0u;
    __syncthreads();
    const unsigned long long e0 = s_e0;
    // entry e0 + j (j >= 1) starts at position offsets[e0 + j] - r0 >= j of the tile
    const unsigned long long navail = m - e0;
#pragma unroll
    for (int k = 0; k < kWinPer; ++k) {
        const uint32_t j = threadIdx.x + k * kWinThreads;
        if (j >= 1 && j < len && j < navail) {
            const unsigned long long st = offsets[e0 + j] - r0;
            if (st < len) s_seg[st] = (j << kWinPosBits) | (uint32_t)st;
        }
    }
    __syncthreads();
    {   // inclusive max-scan of s_seg: entries and their starts ascend together
        uint4 a = *reinterpret_cast<const uint4*>(s_seg + threadIdx.x * kWinPer);
        uint4 b = *reinterpret_cast<const uint4*>(s_seg + threadIdx.x * kWinPer + 4);
        a.y = max(a.y, a.x); a.z = max(a.z, a.y); a.w = max(a.w, a.z);
        b.x = max(b.x, a.w); b.y = max(b.y, b.x); b.z = max(b.z, b.y); b.w = max(b.w, b.z);
        const uint32_t im = wave_incl_max_dpp(b.w);
        if (lane == 63) s_w[wave] = im;
        uint32_t pre = __shfl_up(im, 1u, 64);
        if (lane == 0) pre = 0u;
        __syncthreads();
        for (int v = 0; v < wave; ++v) pre = max(pre, s_w[v]);
        a.x = max(a.x, pre); a.y = max(a.y, pre); a.z = max(a.z, pre); a.w = max(a.w, pre);
        b.x = max(b.x, pre); b.y = max(b.y, pre); b.z = max(b.z, pre); b.w = max(b.w, pre);
        *reinterpret_cast<uint4*>(s_seg + threadIdx.x * kWinPer) = a;
        *reinterpret_cast<uint4*>(s_seg + threadIdx.x * kWinPer + 4) = b;
    }
    __syncthreads();
    const unsigned long long d0 = r0 - offsets[e0];  // pairs of entry e0 before the tile, < its count < 2^32
#pragma unroll
    for (int k = 0; k < kWinPer; ++k) {
        const uint32_t i = threadIdx.x + k * kWinThreads;
        if (i < len) {
            const uint32_t pk = s_seg[i];
            const uint32_t j = pk >> kWinPosBits, st = pk & (kWinTile - 1);
            const uint2 e = entries[e0 + j];  // j < navail: only entries below m were scattered
            const uint32_t rank = i - st + (j == 0 ? (uint32_t)d0 : 0u);
            const uint32_t ref = e.y;
            const uint32_t br = (ref & kDupFlag) ? dup_ref_row(dup_rows, ref, off_mask, rank) : ref;
            out_b[t0 + i] = HAS_ROW_IDS ? row_ids[br] : (uint64_t)br;
            out_p[t0 + i] = HAS_PROBE_IDS ? probe_ids[e.x] : e.x + pbase;
        }
    }
}

hipError_t launch_pair_window(const TableView& tv, const void* plan, int64_t n, const uint32_t* probe_ids,
                              uint32_t probe_base, int64_t pair_lo, int64_t capacity, uint64_t* out_b,
                              uint32_t* out_p, int64_t* d_written, hipStream_t s) {
    const PlanLayout L = pair_plan_layout(n);
    const char* p = static_cast<const char*>(plan);
    const int64_t tiles = std::max<int64_t>((capacity + kWinTile - 1) / kWinTile, 1);  // tile 0 writes *d_written
    if (tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const unsigned long long* header = reinterpret_cast<const unsigned long long*>(p);
    const unsigned long long* offsets = reinterpret_cast<const unsigned long long*>(p + L.offsets);
    const uint2* entries = reinterpret_cast<const uint2*>(p + L.entries);
#define DFP_WIN(RI, PI)                                                                                        \
    pair_window_kernel<RI, PI><<<(unsigned)tiles, kWinThreads, 0, s>>>(                                        \
        tv.dup_rows, tv.row_ids, tv.off_mask, header, offsets, entries, probe_ids, probe_base,                 \
        (unsigned long long)pair_lo, (unsigned long long)capacity, out_b, out_p, reinterpret_cast<long long*>(d_written))
    if (tv.row_ids != nullptr) {
        if (probe_ids != nullptr) DFP_WIN(true, true); else DFP_WIN(true, false);
    } else {
        if (probe_ids != nullptr) DFP_WIN(false, true); else DFP_WIN(false, false);
    }
#undef DFP_WIN
    return hipGetLastError();
}

}  // namespace dfp
