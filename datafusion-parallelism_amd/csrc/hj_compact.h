// hj_compact.h — the ordered stream compaction of the select paths (for the kernel files):
// count per tile, scan of the tile totals, ordered write. Host: the workspace and the scan.
// Device: for tiles stored as 64 ballot words; a new select-like primitive writes a count
// kernel (ballot words + tile totals) and an emit for compact_words_tile.
#pragma once
#include "hj_launch.h"
#include "hj_util.h"

namespace dfp {

constexpr int kCwThreads = 256;
constexpr int kCwWaves = kCwThreads / 64;
constexpr int kCwWords = 64;                    // ballot words (of 64 items) per tile
constexpr int kCwTile = kCwWords * 64;          // 4096 items
constexpr int kCwSteps = kCwWords / kCwWaves;   // steps of kCwThreads items per tile
static_assert(kCwWords == 64 && kCwWaves == 4, "wave 0 scans one word per lane; block_count_sum");

inline int64_t compact_tiles(int64_t n) { return n <= 0 ? 0 : (n + kCwTile - 1) / kCwTile; }

// tcnt u64[nt + 2] (tile totals, scanned in place), words u64[nt * words_per_tile] (0 for the
// paths that store none), the scan's scratch; the slack covers the carve's alignment to 8
struct CompactWs { unsigned long long* tcnt; unsigned long long* words; void* scan; };

inline int64_t compact_ws_bytes(int64_t nt, int words_per_tile) {  // a multiple of 8, monotone
    return 8 * (nt + 2) + 8 * nt * words_per_tile + scan_scratch_bytes(nt) + 512;
}

inline CompactWs compact_ws_carve(void* workspace, int64_t nt, int words_per_tile) {
    unsigned long long* t = (unsigned long long*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
    return CompactWs{t, t + (nt + 2), t + (nt + 2) + nt * words_per_tile};
}

// tcnt[t] = items before tile t, *d_count = all of them
inline hipError_t compact_scan(const CompactWs& w, int64_t nt, int64_t* d_count, hipStream_t s) {
    return launch_scan_u64(w.tcnt, nt, w.scan, (unsigned long long*)d_count, s);
}

// Thread 0: the sum of `cnt` of lane 0 of every wave of the workgroup (kCwThreads); the other
// threads: 0. A caller that comes here again puts a __syncthreads() in between.
__device__ __forceinline__ unsigned long long block_count_sum(unsigned int cnt) {
    __shared__ unsigned int s_c[kCwWaves];
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = cnt;
    __syncthreads();
    return threadIdx.x == 0 ? (unsigned long long)s_c[0] + s_c[1] + s_c[2] + s_c[3] : 0;
}

// The ordered write of one tile by a workgroup of kCwThreads. Bit l of tile_words[j] = item
// item0 + 64 j + l is kept; t0 = kept items before the tile. emit(item, pos) runs once per
// kept item, pos = t0 + its rank in the tile (wave 0 scans the words' popcounts, a lane adds
// its rank within the word). Ends with the barrier a grid-striding caller needs.
template <class Emit>
__device__ __forceinline__ void compact_words_tile(const unsigned long long* __restrict__ tile_words,
                                                   unsigned long long t0, int64_t item0, Emit emit) {
    __shared__ unsigned long long s_b[kCwWords];
    __shared__ unsigned int s_off[kCwWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {
        const unsigned long long b = tile_words[lane];
        const unsigned int c = (unsigned int)__popcll(b);
        s_b[lane] = b;
        s_off[lane] = wave_incl_scan(c) - c;
    }
    __syncthreads();
    for (int j = wave; j < kCwWords; j += kCwWaves) {
        const unsigned long long b = s_b[j];
        if (b == 0) continue;
        if ((b >> lane) & 1)
            emit(item0 + (int64_t)j * 64 + lane, t0 + s_off[j] + (unsigned int)__popcll(b & ((1ull << lane) - 1)));
    }
    __syncthreads();
}

}  // namespace dfp
