// hj_match.hip — the match probe and pair plan family for gfx950: kernels that run the pair
// probe's lookup (lookup4, hj_lookup.h) over blocks of kMatchRows rows and stop before the
// emission.
//
//   probe_match_kernel               per row whether and how often its key occurs; build marks
//   probe_match_filtered_kernel      the same over the pairs that pass a pair predicate
//   pair_plan_lookup_kernel          pass 1 of the pair plan (the rest: hj_window.hip)
//   pair_plan_filtered_count_kernel  the filtered pair plan: count walk,
//   pair_plan_filtered_scan_kernel   scan of the block totals,
//   pair_window_filtered_kernel      emit walk
//
// One copy each of what they share: the tile's lookup (match_tile), the bitmap words
// (store_bitmap_words), the per-workgroup sums (block_sums), the count walk (mf_count4) with
// the emit walk that re-walks it (mf_emit4) below it, and the host's dispatch over key width,
// validity and options (dispatch_bools). The four-value loads and stores and the scan of the
// block totals are in hj_util.h, shared with hj_window.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "hj_device.h"
#include "hj_launch.h"
#include "hj_lookup.h"
#include "hj_pairpred.h"
#include "hj_util.h"

namespace dfp {

// ---------------------------------------------------------------------------
// match probe: per probe row whether, and how often, its key occurs in the table; no
// pairs. The lookup of the pair probe (lookup4), stopped before the emission: what the
// reference's semi and anti joins keep of get_matching_indices once get_semi_indices /
// get_anti_indices and ConcurrentBitSet::set_ones have folded the pairs into flags
// (src/operator/probe_lookup_implementation/right_semi.rs:74-125, left_semi.rs:112-164,
// src/shared/datafusion_private.rs:85-135). One launch: lookup, counts, bitmap words, build
// marks, statistics. No look-back, scan or ordering: a grid-stride loop over blocks of
// kMatchRows rows.
//
// Bitmap layout. lookup4 gives a lane four consecutive rows (one 16- or 32-byte key load,
// four bucket lines in flight per lane before the first compare), so a wave covers 256
// rows = four bitmap words, and the lane's four match bits are a nibble of one of them.
// The kernel keeps lookup4 - its memory-level parallelism is what a random table read
// lives on - and assembles the words from four ballots (ballot q: bit L = row 4L + q):
// word w = the bits 16w..16w+15 of each ballot spread to every fourth bit, OR'ed at shift
// q. That is ~20 scalar-uniform ALU operations per 256 rows in lanes 0-3, against a
// reload of the keys in ballot order (filter_test_kernel's layout) that would give up the
// vector key load and three of the four lines in flight.
//
// Build marks (MARK). Singles and keys of <= kRunMaxRows rows (every run ref among them)
// are marked directly: <= 9 byte stores per probe row. A larger key is claimed once per
// call by an atomic OR into the call's own zeroed claim bitmap - indexed by the key's
// position in a direct-addressed table, by its duplicate-segment offset / 8 in a hashed
// one (segments of >= 10 rows are >= 11 words apart) - and only the claimer walks its
// segment: by itself up to 64 rows, with the whole wave beyond. m probe rows of a key of c
// rows so cost m claim tests + c stores, not m * c. The flags themselves are never the
// claim: they may hold anything before the call, and are only ever stored 1.
// ---------------------------------------------------------------------------
constexpr int kMatchThreads = 256;
constexpr int kMatchWaves = kMatchThreads / 64;
constexpr int kMatchRows = kMatchThreads * 4;  // rows of one block iteration (16 bitmap words)
constexpr int kMatchMaxBlocks = 2048;
constexpr uint32_t kMatchLaneWalk = 64;        // a claimed segment beyond this is walked by the wave
static_assert(kPlanBlockRows == kMatchRows, "a plan block is one iteration of the match probe's workgroup");

// Refs and resolved row counts of the lane's rows row0 .. row0 + 3. ref and cnt hold kMiss and
// 0 on entry, lookup4's contract, and keep them for a row without a match, null or past n.
template <typename K, bool HAS_VALID>
__device__ __forceinline__ void match_tile(const TableView& tv, const void* __restrict__ keys,
                                           const uint8_t* __restrict__ valid, int64_t voff, int64_t n, bool vec,
                                           int64_t row0, uint32_t (&ref)[4], uint32_t (&cnt)[4]) {
    if (row0 < n) lookup4<K, HAS_VALID>(tv, keys, valid, voff, n, vec, row0, ref, cnt);
#pragma unroll
    for (int q = 0; q < 4; ++q) cnt[q] = resolve_count(tv.dup_rows, ref[q], cnt[q], tv.off_mask);
}

// bit j of the low 16 bits -> bit 4j
__device__ __forceinline__ unsigned long long spread16_by4(unsigned long long x) {
    x &= 0xFFFFull;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

// The four bitmap words of the wave's 256 rows from wrow0 (a multiple of 256; bit[q]: the
// lane's row q), words below nwords only; out may be null. The whole wave calls it. A row
// >= n has bit[q] false, so the tail bits are 0.
__device__ __forceinline__ void store_bitmap_words(const bool (&bit)[4], int64_t wrow0, int64_t nwords,
                                                   unsigned long long* __restrict__ out) {
    if (out == nullptr) return;
    const int lane = threadIdx.x & 63;
    unsigned long long b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = __ballot(bit[q]);
    if (lane < 4) {  // lane w assembles word w of the wave's four
        unsigned long long word = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) word |= spread16_by4(b[q] >> (16 * lane)) << q;
        const int64_t widx = (wrow0 >> 6) + lane;
        if (widx < nwords) out[widx] = word;
    }
}

// The workgroup's sums of N per-thread values: wave reduction, LDS, thread 0. Returns whether
// the caller is thread 0, the only one whose out[] is written. s: N * kMatchWaves words of
// LDS, rewritten by the next call: a barrier in between where thread 0 may still be reading.
template <int N>
__device__ __forceinline__ bool block_sums(const unsigned long long* v, unsigned long long* s,
                                           unsigned long long* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long w[N];
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = wave_sum<unsigned long long>(v[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) s[i * kMatchWaves + wave] = w[i];
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        unsigned long long t = 0;
        for (int k = 0; k < kMatchWaves; ++k) t += s[i * kMatchWaves + k];
        out[i] = t;
    }
    return true;
}

__device__ __forceinline__ void match_mark(const TableView& tv, uint32_t row, uint8_t* __restrict__ flags,
                                           uint64_t nflags) {
    const uint64_t id = tv.row_ids != nullptr ? tv.row_ids[row] : (uint64_t)row;
    if (id < nflags) flags[id] = 1;  // idempotent byte stores: no atomics needed
}

// COUNTS and MARK select the optional outputs at compile time (the marking's registers and
// the count stores leave the other instantiations); the bitmap's presence is a wave-uniform
// test of its pointer around four ballots and one store, not worth doubling the variants.
template <typename K, bool HAS_VALID, bool COUNTS, bool MARK>
__global__ void __launch_bounds__(kMatchThreads)
probe_match_kernel(TableView tv, const void* __restrict__ keys, const uint8_t* __restrict__ valid, int64_t voff,
                   int64_t n, bool vec, unsigned long long* __restrict__ out_bitmap, uint32_t* __restrict__ out_counts,
                   bool cvec, uint8_t* __restrict__ flags, uint64_t nflags, uint32_t* __restrict__ claim,
                   unsigned long long* __restrict__ stats) {
    __shared__ unsigned long long s_sum[2 * kMatchWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nwords = (n + 63) >> 6;
    unsigned long long matched = 0, pairs = 0;
    for (int64_t blk0 = (int64_t)blockIdx.x * kMatchRows; blk0 < n; blk0 += (int64_t)gridDim.x * kMatchRows) {
        const int64_t wrow0 = blk0 + (int64_t)wave * 256;
        if (wrow0 >= n) continue;  // the whole wave: no word of the bitmap starts here
        const int64_t row0 = wrow0 + (int64_t)lane * 4;
        uint32_t ref[4] = {kMiss, kMiss, kMiss, kMiss}, cnt[4] = {0, 0, 0, 0};
        match_tile<K, HAS_VALID>(tv, keys, valid, voff, n, vec, row0, ref, cnt);
        bool hit[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            hit[q] = ref[q] != kMiss;
            matched += hit[q];
            pairs += cnt[q];
        }
        store_bitmap_words(hit, wrow0, nwords, out_bitmap);
        if constexpr (COUNTS) store4_u32(out_counts, row0, n, cvec, cnt);
        if constexpr (MARK) {
            bool big[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t r = ref[q], c = cnt[q];
                big[q] = false;
                if (r == kMiss) continue;
                if (!(r & kDupFlag)) {
                    match_mark(tv, r, flags, nflags);
                } else if (c <= kRunMaxRows) {
                    for (uint32_t j = 0; j < c; ++j)
                        match_mark(tv, dup_ref_row(tv.dup_rows, r, tv.off_mask, j), flags, nflags);
                } else {
                    const uint32_t off = r & tv.off_mask;
                    uint32_t ci = off >> 3;
                    if (tv.dense != nullptr)  // a matched row: row0 + q < n and the key is in range
                        ci = (uint32_t)((uint64_t)(int64_t) reinterpret_cast<const K*>(keys)[row0 + q] -
                                        (uint64_t)tv.dmin);
                    uint32_t* w = claim + (ci >> 5);
                    const uint32_t bit = 1u << (ci & 31);
                    // most rows of a hot key find it claimed: test before the read-modify-write
                    bool mine = false;
                    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
                        mine = !(atomicOr(w, bit) & bit);
                    if (mine) {
                        if (c <= kMatchLaneWalk) {
                            for (uint32_t j = 0; j < c; ++j) match_mark(tv, tv.dup_rows[off + 1 + j], flags, nflags);
                        } else {
                            big[q] = true;
                        }
                    }
                }
            }
            // segments of more than kMatchLaneWalk rows: the wave walks them one after another
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned long long m = __ballot(big[q]);
                while (m) {
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const uint32_t off = __shfl(ref[q] & tv.off_mask, src, 64);
                    const uint32_t c = __shfl(cnt[q], src, 64);
                    for (uint32_t j = lane; j < c; j += 64) match_mark(tv, tv.dup_rows[off + 1 + j], flags, nflags);
                }
            }
        }
    }
    // statistics: one atomic pair per workgroup
    const unsigned long long v[2] = {matched, pairs};
    unsigned long long t[2];
    if (block_sums<2>(v, s_sum, t)) {
        if (t[0]) atomicAdd(stats, t[0]);
        if (t[1]) atomicAdd(stats + 1, t[1]);
    }
}

// ---------------------------------------------------------------------------
// filtered match probe: the match probe's outputs over F, the pairs of the probe that pass
// a pair predicate, in place of all its pairs S. What the reference's semi and anti joins
// keep once apply_join_filter_to_indices (src/shared/datafusion_private.rs:295-328) has
// dropped the failing pairs and get_semi_indices / set_ones have folded the rest into flags
// (right_semi.rs:74-125, left_semi.rs:112-164; the filter runs before any marking,
// full.rs:140-175). The skeleton is probe_match_kernel's: match_tile, the bitmap words, one
// atomic per workgroup and statistic. Between the lookup and the outputs every matched row
// walks its key's build rows and evaluates the predicate (pf_pair_passes) in registers
// (mf_count4): no pair is written.
//
// The walk. A key of <= kMatchLaneWalk rows is walked by the lane that owns the probe row
// (a single row: one step). Larger keys are taken by the wave one after another: lane L
// evaluates candidates L, L + 64, ... and a ballot per round gives the owner the count.
// The four rows of a lane are taken in a rolled loop (the refs picked by selects on the
// scalar loop counter), so the predicate's code exists twice per kernel, not eight times.
//
// MODE. kMfExists (no counts, no flags): a row's walk stops at its first passing pair - the
// lane's loop by itself, the wave's rounds on the first non-zero ballot, wave-uniformly.
// kMfFull: every candidate is evaluated, counted, and its build row marked. With flags as
// the only output (flags_only) a candidate whose flag reads 1, or whose id the flags do not
// cover, is skipped unevaluated: flags are only ever stored 1, so a stale 0 costs one
// evaluation and nothing else. There is no claim bitmap: under a predicate different probe
// rows of a key pass different build rows.
// ---------------------------------------------------------------------------
constexpr int kMfExists = 0, kMfFull = 1;

__device__ __forceinline__ uint32_t mf_sel4(const uint32_t (&a)[4], int q) {
    return q == 0 ? a[0] : (q == 1 ? a[1] : (q == 2 ? a[2] : a[3]));
}
__device__ __forceinline__ void mf_put4(uint32_t (&a)[4], int q, uint32_t v) {
    a[0] = q == 0 ? v : a[0];
    a[1] = q == 1 ? v : a[1];
    a[2] = q == 2 ? v : a[2];
    a[3] = q == 3 ? v : a[3];
}

// whether the pair (build row `row`, probe row `prow`) is in F; kMfFull marks it
template <bool BYTES, int MODE>
__device__ __forceinline__ bool mf_candidate(const TableView& tv, const PairPred& pr, uint32_t row, uint32_t prow,
                                             uint8_t* flags, uint64_t nflags, bool flags_only) {
    const uint64_t id = tv.row_ids != nullptr ? tv.row_ids[row] : (uint64_t)row;
    if constexpr (MODE == kMfFull) {
        if (flags_only && (id >= nflags || flags[id] != 0)) return false;  // a racy read: see above
    }
    const bool pass = pf_pair_passes<BYTES>(pr, true, id, prow);  // an id >= build_rows fails unread
    if constexpr (MODE == kMfFull) {
        if (pass && id < nflags) flags[id] = 1;  // nflags is 0 without flags
    }
    return pass;
}

// The split of the two walks: a key of c candidates is walked by the lane that owns the row
// (c = 0: no step), else by the wave.
__device__ __forceinline__ bool mf_lane_walked(uint32_t c) { return c <= kMatchLaneWalk; }

// The count walk. hit[q] = the pairs in F of the lane's row q (kMfExists: 0 / 1), whose
// candidates are candidate j = row j of ref[q] for j < cnt[q], in ascending j. The whole wave
// calls it; wrow0 is the wave's first row.
template <bool BYTES, int MODE>
__device__ __forceinline__ void mf_count4(const TableView& tv, const PairPred& pr, const uint32_t (&ref)[4],
                                          const uint32_t (&cnt)[4], int64_t wrow0, uint8_t* flags, uint64_t nflags,
                                          bool flags_only, uint32_t (&hit)[4]) {
    const int lane = threadIdx.x & 63;
    const int64_t row0 = wrow0 + (int64_t)lane * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) hit[q] = 0;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {  // keys the owning lane walks
        const uint32_t r = mf_sel4(ref, q), c = mf_sel4(cnt, q);
        uint32_t h = 0;
        if (c != 0 && mf_lane_walked(c)) {  // a matched row: row0 + q < n
            const uint32_t prow = (uint32_t)(row0 + q);
            for (uint32_t j = 0; j < c; ++j) {
                const uint32_t row = (r & kDupFlag) ? dup_ref_row(tv.dup_rows, r, tv.off_mask, j) : r;
                if (mf_candidate<BYTES, MODE>(tv, pr, row, prow, flags, nflags, flags_only)) {
                    ++h;
                    if (MODE == kMfExists) break;
                }
            }
        }
        mf_put4(hit, q, h);
    }
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {  // larger keys: the wave walks them one after another
        const uint32_t r = mf_sel4(ref, q), c = mf_sel4(cnt, q);
        uint32_t h = mf_sel4(hit, q);
        unsigned long long m = __ballot(!mf_lane_walked(c));
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint32_t sr = __shfl(r, src, 64), sc = __shfl(c, src, 64);
            const uint32_t prow = (uint32_t)(wrow0 + (int64_t)src * 4 + q);
            uint32_t tot = 0;
            for (uint32_t j0 = 0; j0 < sc; j0 += 64) {  // sc <= the build's rows < 2^32 - 64
                const uint32_t j = j0 + (uint32_t)lane;
                bool pass = false;
                if (j < sc)
                    pass = mf_candidate<BYTES, MODE>(tv, pr, dup_ref_row(tv.dup_rows, sr, tv.off_mask, j), prow,
                                                     flags, nflags, flags_only);
                const unsigned long long b = __ballot(pass);
                tot += (uint32_t)__popcll(b);
                if (MODE == kMfExists && b != 0) break;  // wave-uniform
            }
            if (lane == src) h = tot;
        }
        mf_put4(hit, q, h);
    }
}

// The emit walk: mf_count4's walk again, for the rows with cnt[q] != 0. fc[q]: the row's count
// from the count walk; off: the rank of the first pair of the lane's rows, so row q's passing
// pair k (< fc[q]) has rank off + fc[0] + .. + fc[q - 1] + k and is stored at out[rank - pair_lo]
// where pair_lo <= rank < hi. A row's walk ends once its pairs or the window are exhausted.
// Nothing is marked.
// Invariant: the same lane / wave split (mf_lane_walked) and the same order of j as the count
// walk, over cnt[q] = ref_count(ref[q]), which equals the count walk's resolved count.
template <bool BYTES, bool HAS_PROBE_IDS>
__device__ __forceinline__ void mf_emit4(const TableView& tv, const PairPred& pr, const uint32_t (&ref)[4],
                                         const uint32_t (&cnt)[4], const uint32_t (&fc)[4],
                                         unsigned long long off, int64_t wrow0,
                                         const uint32_t* __restrict__ probe_ids, uint32_t pbase,
                                         unsigned long long pair_lo, unsigned long long hi,
                                         uint64_t* __restrict__ out_b, uint32_t* __restrict__ out_p) {
    const int lane = threadIdx.x & 63;
    const int64_t row0 = wrow0 + (int64_t)lane * 4;
    unsigned long long o = off;  // rank of row q's first pair
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {  // keys the owning lane walks: adjacent lanes' rows are adjacent ranks
        const uint32_t r = mf_sel4(ref, q), c = mf_sel4(cnt, q), f = mf_sel4(fc, q);
        if (c != 0 && mf_lane_walked(c)) {
            const uint32_t prow = (uint32_t)(row0 + q);
            const uint32_t pid = HAS_PROBE_IDS ? probe_ids[prow] : prow + pbase;
            uint32_t k = 0;
            for (uint32_t j = 0; j < c && k < f && o + k < hi; ++j) {
                const uint32_t row = (r & kDupFlag) ? dup_ref_row(tv.dup_rows, r, tv.off_mask, j) : r;
                const uint64_t id = tv.row_ids != nullptr ? tv.row_ids[row] : (uint64_t)row;
                if (pf_pair_passes<BYTES>(pr, true, id, prow)) {
                    const unsigned long long rank = o + k;
                    if (rank >= pair_lo) {  // rank < hi: the loop's condition
                        out_b[rank - pair_lo] = id;
                        out_p[rank - pair_lo] = pid;
                    }
                    ++k;
                }
            }
        }
        o += f;
    }
    o = off;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {  // larger keys: the wave walks them, a round's stores are contiguous
        const uint32_t r = mf_sel4(ref, q), c = mf_sel4(cnt, q), f = mf_sel4(fc, q);
        unsigned long long m = __ballot(!mf_lane_walked(c));
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint32_t sr = __shfl(r, src, 64), sc = __shfl(c, src, 64), sf = __shfl(f, src, 64);
            const unsigned long long so = __shfl(o, src, 64);
            const uint32_t prow = (uint32_t)(wrow0 + (int64_t)src * 4 + q);
            const uint32_t pid = HAS_PROBE_IDS ? probe_ids[prow] : prow + pbase;
            uint32_t tot = 0;  // the row's passing pairs before this round
            for (uint32_t j0 = 0; j0 < sc && tot < sf && so + tot < hi; j0 += 64) {  // wave-uniform
                const uint32_t j = j0 + (uint32_t)lane;
                bool pass = false;
                uint64_t id = 0;
                if (j < sc) {
                    const uint32_t row = dup_ref_row(tv.dup_rows, sr, tv.off_mask, j);
                    id = tv.row_ids != nullptr ? tv.row_ids[row] : (uint64_t)row;
                    pass = pf_pair_passes<BYTES>(pr, true, id, prow);
                }
                const unsigned long long b = __ballot(pass);
                const uint32_t k = tot + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
                const unsigned long long rank = so + k;
                if (pass && k < sf && rank >= pair_lo && rank < hi) {
                    out_b[rank - pair_lo] = id;
                    out_p[rank - pair_lo] = pid;
                }
                tot += (uint32_t)__popcll(b);
            }
        }
        o += f;
    }
}

// stat_mask: bit 0 = stats[0] is asked for, bit 1 = stats[1]; stats[2] always (stats may be null)
template <typename K, bool HAS_VALID, bool BYTES, int MODE>
__global__ void __launch_bounds__(kMatchThreads)
probe_match_filtered_kernel(TableView tv, PairPred pr, const void* __restrict__ keys,
                            const uint8_t* __restrict__ valid, int64_t voff, int64_t n, bool vec,
                            unsigned long long* __restrict__ out_bitmap, uint32_t* __restrict__ out_counts, bool cvec,
                            uint8_t* flags, uint64_t nflags, bool flags_only, unsigned long long* __restrict__ stats,
                            int stat_mask) {
    __shared__ unsigned long long s_sum[3 * kMatchWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nwords = (n + 63) >> 6;
    unsigned long long matched = 0, pairs = 0, cand = 0;
    for (int64_t blk0 = (int64_t)blockIdx.x * kMatchRows; blk0 < n; blk0 += (int64_t)gridDim.x * kMatchRows) {
        const int64_t wrow0 = blk0 + (int64_t)wave * 256;
        if (wrow0 >= n) continue;  // the whole wave: no word of the bitmap starts here
        const int64_t row0 = wrow0 + (int64_t)lane * 4;
        uint32_t ref[4] = {kMiss, kMiss, kMiss, kMiss}, cnt[4] = {0, 0, 0, 0}, hit[4];
        match_tile<K, HAS_VALID>(tv, keys, valid, voff, n, vec, row0, ref, cnt);
        mf_count4<BYTES, MODE>(tv, pr, ref, cnt, wrow0, flags, nflags, flags_only, hit);
        bool any[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cand += cnt[q];
            any[q] = hit[q] != 0;
            matched += any[q];
            pairs += hit[q];
        }
        store_bitmap_words(any, wrow0, nwords, out_bitmap);
        if constexpr (MODE == kMfFull) {
            if (out_counts != nullptr) store4_u32(out_counts, row0, n, cvec, hit);
        }
    }
    // statistics: one atomic per workgroup and statistic; |F| only where the walk counted it
    constexpr int kSums = MODE == kMfFull ? 3 : 2;
    const unsigned long long v[3] = {matched, cand, pairs};
    unsigned long long t[3] = {0, 0, 0};
    if (block_sums<kSums>(v, s_sum, t) && stats != nullptr) {
        if (t[0] && (stat_mask & 1)) atomicAdd(stats, t[0]);
        if (t[2] && (stat_mask & 2)) atomicAdd(stats + 1, t[2]);
        if (t[1]) atomicAdd(stats + 2, t[1]);
    }
}

// ---------------------------------------------------------------------------
// pair plan, pass 1: the match probe's lookup, kept per row. Every row's ref and resolved
// pair count go to the plan's scratch, and every block of kPlanBlockRows rows leaves its
// (matched rows, pairs) totals; the scan of those totals and the compaction are launches
// of their own (hj_window.hip), so no workgroup waits for another. Where the reference's
// get_matching_indices (src/shared/shared.rs:29-47) emits a probe batch's pairs in one
// piece, the plan keeps "how many pairs, and where" and the windows emit them in slices.
// ---------------------------------------------------------------------------
template <typename K, bool HAS_VALID>
__global__ void __launch_bounds__(kMatchThreads)
pair_plan_lookup_kernel(TableView tv, const void* __restrict__ keys, const uint8_t* __restrict__ valid, int64_t voff,
                        int64_t n, bool vec, uint32_t* __restrict__ refs, uint32_t* __restrict__ counts, bool svec,
                        unsigned long long* __restrict__ btot) {
    __shared__ unsigned long long s_sum[2 * kMatchWaves];
    for (int64_t blk = blockIdx.x; blk * kMatchRows < n; blk += gridDim.x) {
        const int64_t row0 = blk * kMatchRows + (int64_t)threadIdx.x * 4;
        uint32_t ref[4] = {kMiss, kMiss, kMiss, kMiss}, cnt[4] = {0, 0, 0, 0};
        match_tile<K, HAS_VALID>(tv, keys, valid, voff, n, vec, row0, ref, cnt);
        unsigned long long v[2] = {0, 0};  // matched rows, pairs
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[0] += cnt[q] != 0;
            v[1] += cnt[q];
        }
        store4_u32(refs, row0, n, svec, ref);
        store4_u32(counts, row0, n, svec, cnt);
        block_sums<2>(v, s_sum, btot + 2 * blk);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// filtered pair plan: the pair plan under a pair predicate, whose windows hold F, the pairs
// of the probe that pass it, not S. What lookup_inner_join_probe_batch (inner.rs:79-129)
// keeps of get_matching_indices (src/shared/shared.rs:29-47) once
// apply_join_filter_to_indices (src/shared/datafusion_private.rs:295-328) has dropped the
// failing pairs - the filter before any marking, as in full.rs:140-175 - without S ever
// reaching memory. Count -> scan -> write, every pass a launch of its own: no workgroup
// waits for another.
//
//   count  pair_plan_filtered_count_kernel  probe_match_filtered_kernel's full walk (no
//          first-pass exit, no flag skip: the counts are exact). Keeps every row's ref and
//          F-count and, per block of kPlanBlockRows rows, (rows with a pair in F, its pairs
//          in F); bitmap and flags as the filtered match probe writes them; |S| by one
//          atomic per workgroup into the plan's header.
//   scan   pair_plan_filtered_scan_kernel   one workgroup: exclusive scan of the block
//          totals in place, the grand totals behind the last block, the header and d_stats.
//   emit   pair_window_filtered_kernel      the same grid of blocks. A block whose scanned
//          range misses the window leaves after two loads. Otherwise its rows' F-counts
//          are scanned (64-bit ranks) and every row whose passing pairs meet the window
//          walks its candidates again (mf_emit4): pair k of the row goes to rank offset + k.
//          Rows without a pair in F are never walked again.
// ---------------------------------------------------------------------------
FilteredPlanLayout pair_plan_filtered_layout(int64_t n) {
    FilteredPlanLayout L;
    L.nblocks = (n + kPlanBlockRows - 1) / kPlanBlockRows;
    L.refs = kPlanHeaderBytes;
    L.counts = L.refs + ((4 * n + 15) & ~(int64_t)15);
    L.blocks = L.counts + ((4 * n + 15) & ~(int64_t)15);
    L.bytes = L.blocks + 16 * (L.nblocks + 1);
    return L;
}

template <typename K, bool HAS_VALID, bool BYTES>
__global__ void __launch_bounds__(kMatchThreads)
pair_plan_filtered_count_kernel(TableView tv, PairPred pr, const void* __restrict__ keys,
                                const uint8_t* __restrict__ valid, int64_t voff, int64_t n, bool vec,
                                unsigned long long* __restrict__ out_bitmap, uint8_t* flags, uint64_t nflags,
                                uint32_t* __restrict__ refs, uint32_t* __restrict__ counts, bool svec,
                                unsigned long long* __restrict__ btot, unsigned long long* __restrict__ cand_total) {
    __shared__ unsigned long long s_sum[2 * kMatchWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nwords = (n + 63) >> 6;
    unsigned long long cand = 0;
    for (int64_t blk = blockIdx.x; blk * kMatchRows < n; blk += gridDim.x) {
        const int64_t wrow0 = blk * kMatchRows + (int64_t)wave * 256;
        const int64_t row0 = wrow0 + (int64_t)lane * 4;
        unsigned long long v[2] = {0, 0};  // rows with a pair in F, pairs in F
        if (wrow0 < n) {  // the whole wave (a wave past n only joins the block's totals)
            uint32_t ref[4] = {kMiss, kMiss, kMiss, kMiss}, cnt[4] = {0, 0, 0, 0}, hit[4];
            match_tile<K, HAS_VALID>(tv, keys, valid, voff, n, vec, row0, ref, cnt);
            mf_count4<BYTES, kMfFull>(tv, pr, ref, cnt, wrow0, flags, nflags, false, hit);
            bool any[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                cand += cnt[q];
                any[q] = hit[q] != 0;
                v[0] += any[q];
                v[1] += hit[q];
            }
            store_bitmap_words(any, wrow0, nwords, out_bitmap);
            store4_u32(refs, row0, n, svec, ref);
            store4_u32(counts, row0, n, svec, hit);
        }
        block_sums<2>(v, s_sum, btot + 2 * blk);
        __syncthreads();
    }
    // |S|: one atomic per workgroup
    unsigned long long tc;
    if (block_sums<1>(&cand, s_sum, &tc) && tc) atomicAdd(cand_total, tc);
}

// header: [0] rows with a pair in F, [1] |F|, [2] |S| (zeroed before the count, which adds to
// it); btot[2 * nblocks], btot[2 * nblocks + 1]: the same totals, so that block b's range of
// ranks is [btot[2b + 1], btot[2b + 3]) for every b
__global__ void __launch_bounds__(kPlanScanThreads)
pair_plan_filtered_scan_kernel(unsigned long long* __restrict__ btot, int64_t nblocks,
                               unsigned long long* __restrict__ header, long long* __restrict__ d_stats) {
    __shared__ unsigned long long s_w[kPlanScanThreads / 64];
    unsigned long long run_m, run_p;
    scan_block_totals(btot, nblocks, s_w, &run_m, &run_p);
    if (threadIdx.x == 0) {
        btot[2 * nblocks] = run_m;
        btot[2 * nblocks + 1] = run_p;
        header[0] = run_m;
        header[1] = run_p;
        if (d_stats != nullptr) {
            d_stats[0] = (long long)run_m;
            d_stats[1] = (long long)run_p;
            d_stats[2] = (long long)header[2];
        }
    }
}

// Inclusive wave64 scan of a u64 < 2^40 in two DPP scans: the low 24 bits (64 lanes: < 2^30)
// and the bits above them (< 2^16 each: < 2^22). A lane's four F-counts are below 2^34.
__device__ __forceinline__ unsigned long long wave_incl_scan40_dpp(unsigned long long v) {
    const uint32_t lo = wave_incl_scan_dpp((uint32_t)v & 0xFFFFFFu);
    const uint32_t hi = wave_incl_scan_dpp((uint32_t)(v >> 24));
    return ((unsigned long long)hi << 24) + lo;
}

template <bool BYTES, bool HAS_PROBE_IDS>
__global__ void __launch_bounds__(kMatchThreads)
pair_window_filtered_kernel(TableView tv, PairPred pr, const uint32_t* __restrict__ refs,
                            const uint32_t* __restrict__ counts, bool svec, int64_t n, int64_t nblocks,
                            const unsigned long long* __restrict__ btot, const uint32_t* __restrict__ probe_ids,
                            uint32_t pbase, unsigned long long pair_lo, unsigned long long cap,
                            uint64_t* __restrict__ out_b, uint32_t* __restrict__ out_p,
                            long long* __restrict__ d_written) {
    __shared__ unsigned long long s_w[kMatchWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0 && d_written != nullptr) {
        const unsigned long long total = btot[2 * nblocks + 1];
        const unsigned long long w = pair_lo < total ? total - pair_lo : 0ull;
        *d_written = (long long)(w < cap ? w : cap);
    }
    if ((int64_t)blockIdx.x >= nblocks || cap == 0) return;
    // the block's ranks [base, next) against the window [pair_lo, hi); every rank is below
    // |F|, so the window's end needs no clamp (pair_lo < 2^63, cap <= 2^42: no overflow)
    const unsigned long long base = btot[2 * (int64_t)blockIdx.x + 1], next = btot[2 * (int64_t)blockIdx.x + 3];
    const unsigned long long hi = pair_lo + cap;
    if (next <= pair_lo || base >= hi) return;  // the whole workgroup
    const int64_t wrow0 = (int64_t)blockIdx.x * kPlanBlockRows + (int64_t)wave * 256;
    const int64_t row0 = wrow0 + (int64_t)lane * 4;
    uint32_t ref[4] = {kMiss, kMiss, kMiss, kMiss}, fc[4] = {0, 0, 0, 0};
    load4_u32(refs, row0, n, svec, ref);
    load4_u32(counts, row0, n, svec, fc);
    // 64-bit exclusive prefix of the F-counts inside the block
    const unsigned long long mine = (unsigned long long)fc[0] + fc[1] + fc[2] + fc[3];
    const unsigned long long incl = wave_incl_scan40_dpp(mine);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    unsigned long long off = base + (incl - mine);
    for (int w = 0; w < wave; ++w) off += s_w[w];
    // cnt[q]: the row's candidates if any of its passing pairs [o, end) is in the window, else
    // 0 (the row is not walked). The plan does not keep the candidate count: a table layout
    // whose lookup count ref_count cannot recover from the ref would have to store it (as
    // pair_plan_lookup_kernel does).
    uint32_t cnt[4];
    unsigned long long end = off;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned long long o = end;
        end += fc[q];
        const bool in = fc[q] != 0 && end > pair_lo && o < hi;
        cnt[q] = in ? ref_count(tv.dup_rows, ref[q], tv.off_mask) : 0u;
    }
    mf_emit4<BYTES, HAS_PROBE_IDS>(tv, pr, ref, cnt, fc, off, wrow0, probe_ids, pbase, pair_lo, hi, out_b, out_p);
}

// ---------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------
namespace {

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): runtime options to template
// arguments, every combination instantiated
template <typename F>
void dispatch_bools(F&& f) {
    f();
}
template <typename F, typename... B>
void dispatch_bools(F&& f, bool b, B... rest) {
    if (b) dispatch_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else dispatch_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// the key type of a dispatch on key_bytes == 8
template <bool WIDE>
using KeyOf = std::conditional_t<WIDE, int64_t, int32_t>;

unsigned match_grid(int64_t n) {
    return (unsigned)std::min<int64_t>((n + kMatchRows - 1) / kMatchRows, kMatchMaxBlocks);
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int64_t probe_match_workspace(uint64_t claim_bits) {
    return kMatchWsHeader + (int64_t)((claim_bits + 63) / 64) * 8;
}

hipError_t launch_probe_match(int key_bytes, const TableView& tv, const void* keys, const uint8_t* valid, int64_t voff,
                              int64_t n, uint8_t* out_bitmap, uint32_t* out_counts, uint8_t* flags, int64_t nflags,
                              int64_t* d_stats, void* workspace, uint64_t claim_bits, hipStream_t s) {
    // workspace: [0, 16) the statistics of a caller that passes none, then the claim bitmap
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(d_stats != nullptr ? (void*)d_stats : workspace);
    hipError_t e = hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    if (n <= 0) return hipSuccess;
    const bool mark = flags != nullptr && nflags > 0;
    uint32_t* claim = reinterpret_cast<uint32_t*>((char*)workspace + kMatchWsHeader);
    if (mark) {
        e = hipMemsetAsync(claim, 0, (size_t)((claim_bits + 63) / 64) * 8, s);
        if (e != hipSuccess) return e;
    }
    dispatch_bools(
        [&](auto wide, auto hv, auto cn, auto mk) {
            probe_match_kernel<KeyOf<wide.value>, hv.value, cn.value, mk.value><<<match_grid(n), kMatchThreads, 0, s>>>(
                tv, keys, valid, voff, n, aligned16(keys), reinterpret_cast<unsigned long long*>(out_bitmap),
                out_counts, aligned16(out_counts), flags, (uint64_t)nflags, claim, stats);
        },
        key_bytes == 8, valid != nullptr, out_counts != nullptr, mark);
    return hipGetLastError();
}

hipError_t launch_probe_match_filtered(int key_bytes, const TableView& tv, const PairPred& pr, const void* keys,
                                       const uint8_t* valid, int64_t voff, int64_t n, uint8_t* out_bitmap,
                                       uint32_t* out_counts, uint8_t* flags, int64_t nflags, int64_t* d_stats,
                                       hipStream_t s) {
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(d_stats);
    const int stat_mask = ((out_bitmap != nullptr || out_counts != nullptr) ? 1 : 0) | (out_counts != nullptr ? 2 : 0);
    if (stats != nullptr) {
        hipError_t e = hipMemsetAsync(stats, 0, 3 * sizeof(unsigned long long), s);
        // the statistics nobody asked the walk for read -1: [1], or [0] and [1]
        if (e == hipSuccess && stat_mask != 3)
            e = hipMemsetAsync(stats + (stat_mask & 1), 0xFF, (size_t)(2 - (stat_mask & 1)) * 8, s);
        if (e != hipSuccess) return e;
    }
    if (n <= 0) return hipSuccess;
    const bool mark = flags != nullptr && nflags > 0;
    const bool flags_only = mark && out_bitmap == nullptr && out_counts == nullptr;
    dispatch_bools(
        [&](auto wide, auto hv, auto by, auto full) {
            probe_match_filtered_kernel<KeyOf<wide.value>, hv.value, by.value, full.value ? kMfFull : kMfExists>
                <<<match_grid(n), kMatchThreads, 0, s>>>(
                    tv, pr, keys, valid, voff, n, aligned16(keys), reinterpret_cast<unsigned long long*>(out_bitmap),
                    out_counts, aligned16(out_counts), mark ? flags : nullptr, mark ? (uint64_t)nflags : 0, flags_only,
                    stats, stat_mask);
        },
        key_bytes == 8, valid != nullptr, pf_has_bytes(pr), out_counts != nullptr || mark);
    return hipGetLastError();
}

hipError_t launch_pair_plan_lookup(int key_bytes, const TableView& tv, const void* keys, const uint8_t* valid,
                                   int64_t voff, int64_t n, uint32_t* refs, uint32_t* counts,
                                   unsigned long long* btot, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const bool svec = aligned16(refs) && aligned16(counts);
    dispatch_bools(
        [&](auto wide, auto hv) {
            pair_plan_lookup_kernel<KeyOf<wide.value>, hv.value><<<match_grid(n), kMatchThreads, 0, s>>>(
                tv, keys, valid, voff, n, aligned16(keys), refs, counts, svec, btot);
        },
        key_bytes == 8, valid != nullptr);
    return hipGetLastError();
}

hipError_t launch_pair_plan_filtered(int key_bytes, const TableView& tv, const PairPred& pr, const void* keys,
                                     const uint8_t* valid, int64_t voff, int64_t n, void* plan, uint8_t* out_bitmap,
                                     uint8_t* flags, int64_t nflags, int64_t* d_stats, hipStream_t s) {
    const FilteredPlanLayout L = pair_plan_filtered_layout(n);
    char* p = static_cast<char*>(plan);
    unsigned long long* header = reinterpret_cast<unsigned long long*>(p);
    unsigned long long* btot = reinterpret_cast<unsigned long long*>(p + L.blocks);
    hipError_t e = hipMemsetAsync(header, 0, kPlanHeaderBytes, s);
    if (e != hipSuccess) return e;
    if (n > 0) {
        const bool mark = flags != nullptr && nflags > 0;
        dispatch_bools(
            [&](auto wide, auto hv, auto by) {
                pair_plan_filtered_count_kernel<KeyOf<wide.value>, hv.value, by.value>
                    <<<match_grid(n), kMatchThreads, 0, s>>>(
                        tv, pr, keys, valid, voff, n, aligned16(keys), reinterpret_cast<unsigned long long*>(out_bitmap),
                        mark ? flags : nullptr, mark ? (uint64_t)nflags : 0, reinterpret_cast<uint32_t*>(p + L.refs),
                        reinterpret_cast<uint32_t*>(p + L.counts), aligned16(plan), btot, header + 2);
            },
            key_bytes == 8, valid != nullptr, pf_has_bytes(pr));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    pair_plan_filtered_scan_kernel<<<1, kPlanScanThreads, 0, s>>>(btot, L.nblocks, header,
                                                                  reinterpret_cast<long long*>(d_stats));
    return hipGetLastError();
}

hipError_t launch_pair_window_filtered(const TableView& tv, const PairPred& pr, const void* plan, int64_t n,
                                       const uint32_t* probe_ids, uint32_t probe_base, int64_t pair_lo,
                                       int64_t capacity, uint64_t* out_b, uint32_t* out_p, int64_t* d_written,
                                       hipStream_t s) {
    const FilteredPlanLayout L = pair_plan_filtered_layout(n);
    const char* p = static_cast<const char*>(plan);
    const unsigned grid = (unsigned)std::max<int64_t>(L.nblocks, 1);  // block 0 writes *d_written
    dispatch_bools(
        [&](auto by, auto pi) {
            pair_window_filtered_kernel<by.value, pi.value><<<grid, kMatchThreads, 0, s>>>(
                tv, pr, reinterpret_cast<const uint32_t*>(p + L.refs), reinterpret_cast<const uint32_t*>(p + L.counts),
                aligned16(plan), n, L.nblocks, reinterpret_cast<const unsigned long long*>(p + L.blocks), probe_ids,
                probe_base, (unsigned long long)pair_lo, (unsigned long long)capacity, out_b, out_p,
                reinterpret_cast<long long*>(d_written));
        },
        pf_has_bytes(pr), probe_ids != nullptr);
    return hipGetLastError();
}

}  // namespace dfp
