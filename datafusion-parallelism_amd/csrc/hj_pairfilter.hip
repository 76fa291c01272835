// hj_pairfilter.hip — gfx950 kernels of the pair filter (include/hj.h, "pair filter"): a
// conjunction of typed comparisons between build columns, probe columns and constants,
// evaluated on candidate pairs. Replaces apply_join_filter_to_indices
// (src/shared/datafusion_private.rs:295-328) for predicates of that form.
//
//   pair_eval_kernel      one pair per lane, whole waves of 64 pairs: the wave's 64 results
//                         are one ballot word (lane 0 stores it, no atomics on the bitmap);
//                         the popcounts go to the tile's total (select) or to the count (test).
//                         The predicate travels as a kernel argument, so every descriptor -
//                         class, width, op, column - is wave-uniform and the switches over
//                         them are scalar branches; only the operand gathers and the BYTES
//                         compare loop are per lane. BYTES = false leaves that loop out.
//   pair_compact_kernel   per tile of 4096 pairs: re-reads the tile's 64 ballot words and
//                         writes each passing pair at its rank (compact_words_tile of
//                         hj_compact.h). No workgroup waits on another.
//
// HBM-bound: 12 bytes of pair read per candidate, the operand gathers, one bit written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hj_compact.h"
#include "hj_device.h"
#include "hj_launch.h"
#include "hj_pairpred.h"
#include "hj_util.h"

namespace dfp {

constexpr unsigned kPfMaxGrid = 4096;  // grid-stride over the tiles beyond this

// words: the ballot words, word w covers pairs [64 w, 64 w + 64); only words < nwords are
// stored (test: ceil(n / 64); select: every word of every tile). ttot (select): the tile's
// passing pairs; d_count (test): += the block's passing pairs, zeroed by the launcher.
template <bool BYTES>
__global__ void __launch_bounds__(kCwThreads)
pair_eval_kernel(PairPred pr, const uint64_t* __restrict__ bidx, const uint32_t* __restrict__ pidx, int64_t n,
                 int64_t ntiles, unsigned long long* __restrict__ words, int64_t nwords,
                 unsigned long long* __restrict__ ttot, unsigned long long* __restrict__ d_count) {
    const int lane = threadIdx.x & 63;
    unsigned long long block_cnt = 0;  // thread 0's
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t tile0 = tile * kCwTile;
        unsigned int cnt = 0;
#pragma unroll 1
        for (int s0 = 0; s0 < kCwSteps; ++s0) {
            const int64_t i = tile0 + (int64_t)s0 * kCwThreads + threadIdx.x;
            const bool live = i < n;
            uint64_t b = 0;
            uint32_t p = 0;
            if (live) {
                b = bidx[i];
                p = pidx[i];
            }
            const bool pass = pf_pair_passes<BYTES>(pr, live, b, p);
            const unsigned long long word = __ballot(pass);  // whole wave: EXEC is full here
            const int64_t w = (i - lane) >> 6;
            if (lane == 0) {
                if (w < nwords) words[w] = word;
                cnt += (unsigned int)__popcll(word);
            }
        }
        const unsigned long long t = block_count_sum(cnt);  // thread 0's, else 0
        if (threadIdx.x == 0 && ttot != nullptr) ttot[tile] = t;
        block_cnt += t;
        __syncthreads();
    }
    if (threadIdx.x == 0 && d_count != nullptr && block_cnt != 0) atomicAdd(d_count, block_cnt);
}

// toff: the scanned tile totals; out_b / out_p hold n elements and every position is below
// the total <= n; a set bit names a pair < n (the evaluate kernel sets none past n)
__global__ void __launch_bounds__(kCwThreads)
pair_compact_kernel(const uint64_t* __restrict__ bidx, const uint32_t* __restrict__ pidx, int64_t ntiles,
                    const unsigned long long* __restrict__ words, const unsigned long long* __restrict__ toff,
                    uint64_t* __restrict__ out_b, uint32_t* __restrict__ out_p) {
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
        compact_words_tile(words + tile * kCwWords, toff[tile], tile * kCwTile, [&](int64_t i, unsigned long long pos) {
            out_b[pos] = bidx[i];
            out_p[pos] = pidx[i];
        });
}

hipError_t launch_compact_pairs(const uint64_t* bidx, const uint32_t* pidx, int64_t nt,
                                const unsigned long long* words, const unsigned long long* toff, uint64_t* out_b,
                                uint32_t* out_p, hipStream_t s) {
    const unsigned grid = (unsigned)std::min<int64_t>(nt, (int64_t)kPfMaxGrid * 16);
    pair_compact_kernel<<<grid, kCwThreads, 0, s>>>(bidx, pidx, nt, words, toff, out_b, out_p);
    return hipGetLastError();
}

bool pf_has_bytes(const PairPred& pr) {
    for (int t = 0; t < pr.nterms; ++t)
        if (pr.t[t].cls == kPfBytes) return true;
    return false;
}

static hipError_t pf_eval(const PairPred& pr, const uint64_t* bidx, const uint32_t* pidx, int64_t n, int64_t nt,
                          unsigned long long* words, int64_t nwords, unsigned long long* ttot,
                          unsigned long long* d_count, hipStream_t s) {
    const unsigned grid = (unsigned)std::min<int64_t>(nt, kPfMaxGrid);
    if (pf_has_bytes(pr))
        pair_eval_kernel<true><<<grid, kCwThreads, 0, s>>>(pr, bidx, pidx, n, nt, words, nwords, ttot, d_count);
    else
        pair_eval_kernel<false><<<grid, kCwThreads, 0, s>>>(pr, bidx, pidx, n, nt, words, nwords, ttot, d_count);
    return hipGetLastError();
}

hipError_t launch_pair_filter_test(const PairPred& pr, const uint64_t* bidx, const uint32_t* pidx, int64_t n,
                                   uint8_t* out_bitmap, int64_t* d_count, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_count, 0, 8, s);
    if (e != hipSuccess || n <= 0) return e;
    return pf_eval(pr, bidx, pidx, n, compact_tiles(n), (unsigned long long*)out_bitmap, (n + 63) / 64, nullptr,
                   (unsigned long long*)d_count, s);
}

// tile totals u64[nt + 2], ballot words u64[64 nt], the scan's scratch: about one bit per pair
int64_t pair_filter_workspace(int64_t n) { return compact_ws_bytes(compact_tiles(n), kCwWords); }

hipError_t launch_pair_filter_select(const PairPred& pr, const uint64_t* bidx, const uint32_t* pidx, int64_t n,
                                     uint64_t* out_b, uint32_t* out_p, int64_t* d_count, void* workspace,
                                     hipStream_t s) {
    const int64_t nt = compact_tiles(n);
    if (nt == 0) return hipMemsetAsync(d_count, 0, 8, s);
    const CompactWs w = compact_ws_carve(workspace, nt, kCwWords);
    hipError_t e = pf_eval(pr, bidx, pidx, n, nt, w.words, nt * kCwWords, w.tcnt, nullptr, s);
    if (e != hipSuccess) return e;
    if ((e = compact_scan(w, nt, d_count, s)) != hipSuccess) return e;
    return launch_compact_pairs(bidx, pidx, nt, w.words, w.tcnt, out_b, out_p, s);
}

}  // namespace dfp
