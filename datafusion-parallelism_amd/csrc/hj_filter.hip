// hj_filter.hip — gfx950 kernels of the device key filter (include/hj.h, "key filter"):
// a bitmap over the build key range (exact) or a one-word blocked Bloom filter, filled
// from the build keys and tested ahead of the probe so that probe rows without a match
// never read the table. No reference counterpart: the reference probes every row
// (lookup_implementation_3.rs:22-59).
//
//   filter_add_kernel      one 64-bit OR per valid build key; bits only ever get set, so
//                          a plain load first skips the atomic when the mask is already
//                          there (duplicates, and for a bitmap the neighbours' bits)
//   filter_test_kernel     64 consecutive rows per wave and step, the ballot stored as one
//                          8-byte word of the Arrow bitmap
//   filter_select_*        ordered compaction of the passing rows (keys + u32 ids): count
//                          per 4096-row tile (the ballots kept in the workspace), scan,
//                          write - the shared compaction of hj_compact.h
//
// All streaming work bound by the key reads; the filter words are a gather.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hj_compact.h"
#include "hj_launch.h"
#include "hj_util.h"

namespace dfp {

// word and mask of key k; false: k is outside a RANGE filter (never present)
template <bool RANGE>
__device__ __forceinline__ bool filter_locate(const FilterView& f, int64_t k, uint64_t* w, unsigned long long* m) {
    if constexpr (RANGE) {
        const uint64_t d = (uint64_t)k - (uint64_t)f.lo;
        *w = d >> 6;
        *m = 1ull << (d & 63);
        return d <= f.span;
    } else {
        const uint64_t h = mix64((uint64_t)k);
        *w = ((h >> 32) * f.nwords) >> 32;
        *m = (1ull << (h & 63)) | (1ull << ((h >> 6) & 63)) | (1ull << ((h >> 12) & 63)) | (1ull << ((h >> 18) & 63));
        return true;
    }
}

template <bool RANGE>
__device__ __forceinline__ bool filter_has(const FilterView& f, int64_t k) {
    uint64_t w;
    unsigned long long m;
    if (!filter_locate<RANGE>(f, k, &w, &m)) return false;
    return (f.words[w] & m) == m;
}

// four consecutive keys of one thread, widened to int64 (one 16- or 32-byte load when the
// column is 16-byte aligned and the four rows exist)
template <typename K>
__device__ __forceinline__ void filter_load4(const K* kp, int64_t row0, int64_t n, bool vec, int64_t (&k)[4]) {
    if (vec && row0 + 4 <= n) {
        if constexpr (sizeof(K) == 8) {
            const longlong2 a = *reinterpret_cast<const longlong2*>(kp + row0);
            const longlong2 b = *reinterpret_cast<const longlong2*>(kp + row0 + 2);
            k[0] = a.x; k[1] = a.y; k[2] = b.x; k[3] = b.y;
        } else {
            const int4 a = *reinterpret_cast<const int4*>(kp + row0);
            k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] = (row0 + q < n) ? (int64_t)kp[row0 + q] : 0;
    }
}

// ---------------------------------------------------------------------------
// add
// ---------------------------------------------------------------------------
constexpr int kAddThreads = 256;

// Shapes measured on C4's build side (profiles/key_filter_kernels.txt): the atomic without
// the load first ties this one, and merging the masks of the lanes of a wave that hit the
// same word before the atomic is slower (1.6 keys per word leave little to merge).
template <typename K, bool HAS_VALID, bool RANGE>
__global__ void __launch_bounds__(kAddThreads)
filter_add_kernel(FilterView f, const K* __restrict__ keys, const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                  unsigned long long* dropped) {
    const bool vec = (reinterpret_cast<uintptr_t>(keys) & 15) == 0;
    unsigned int drop = 0;
    const int64_t stride = (int64_t)gridDim.x * kAddThreads * 4;
    for (int64_t base = (int64_t)blockIdx.x * kAddThreads * 4; base < n; base += stride) {
        const int64_t row0 = base + (int64_t)threadIdx.x * 4;
        int64_t k[4];
        filter_load4<K>(keys, row0, n, vec, k);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool on = (row0 + q < n) && (!HAS_VALID || bit_valid(valid, voff, row0 + q));
            uint64_t w;
            unsigned long long m;
            const bool in = filter_locate<RANGE>(f, k[q], &w, &m);
            drop += on && !in;
            // bits only ever get set: a word that already holds the mask needs no atomic
            if (on && in && (f.words[w] & m) != m) atomicOr(&f.words[w], m);
        }
    }
    if (RANGE) {
        const unsigned int t = wave_sum(drop);
        if ((threadIdx.x & 63) == 0 && t != 0) atomicAdd(dropped, (unsigned long long)t);
    }
}

static unsigned stream_grid(int64_t n, int rows_per_block) {
    // a few resident workgroups per CU, grid-stride over the rest
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + rows_per_block - 1) / rows_per_block, 256 * 16));
}

template <typename K, bool HAS_VALID, bool RANGE>
static void add_dispatch(const FilterView& f, const void* keys, const uint8_t* valid, int64_t voff, int64_t n,
                         unsigned long long* dropped, hipStream_t s) {
    filter_add_kernel<K, HAS_VALID, RANGE><<<stream_grid(n, kAddThreads * 4), kAddThreads, 0, s>>>(
        f, (const K*)keys, valid, voff, n, dropped);
}

#define DFP_FILTER_DISPATCH(FN, ...)                                                       \
    do {                                                                                   \
        const bool hv_ = valid != nullptr;                                                 \
        if (key_bytes == 8) {                                                              \
            if (f.range) { if (hv_) FN<int64_t, true, true>(__VA_ARGS__); else FN<int64_t, false, true>(__VA_ARGS__); }   \
            else         { if (hv_) FN<int64_t, true, false>(__VA_ARGS__); else FN<int64_t, false, false>(__VA_ARGS__); } \
        } else {                                                                           \
            if (f.range) { if (hv_) FN<int32_t, true, true>(__VA_ARGS__); else FN<int32_t, false, true>(__VA_ARGS__); }   \
            else         { if (hv_) FN<int32_t, true, false>(__VA_ARGS__); else FN<int32_t, false, false>(__VA_ARGS__); } \
        }                                                                                  \
    } while (0)

hipError_t launch_filter_add(const FilterView& f, int key_bytes, const void* keys, const uint8_t* valid, int64_t voff,
                             int64_t n, unsigned long long* dropped, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    DFP_FILTER_DISPATCH(add_dispatch, f, keys, valid, voff, n, dropped, s);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// test: Arrow bitmap of the rows that are valid and present, and their number
// ---------------------------------------------------------------------------
constexpr int kTestThreads = kCwThreads;  // block_count_sum's workgroup
constexpr int kTestSteps = 4;  // key loads in flight per lane

template <typename K, bool HAS_VALID, bool RANGE>
__global__ void __launch_bounds__(kTestThreads)
filter_test_kernel(FilterView f, const K* __restrict__ keys, const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                   unsigned long long* __restrict__ out, unsigned long long* __restrict__ d_count) {
    const int lane = threadIdx.x & 63;
    unsigned int cnt = 0;  // lane 0 of each wave counts its words' bits
    const int64_t span = (int64_t)kTestThreads * kTestSteps;
    for (int64_t base = (int64_t)blockIdx.x * span; base < n; base += (int64_t)gridDim.x * span) {
        K k[kTestSteps];
#pragma unroll
        for (int u = 0; u < kTestSteps; ++u) {
            const int64_t row = base + u * kTestThreads + threadIdx.x;
            k[u] = row < n ? keys[row] : (K)0;
        }
#pragma unroll
        for (int u = 0; u < kTestSteps; ++u) {
            const int64_t row = base + u * kTestThreads + threadIdx.x;
            const bool ok = row < n && (!HAS_VALID || bit_valid(valid, voff, row)) && filter_has<RANGE>(f, (int64_t)k[u]);
            const unsigned long long b = __ballot(ok);
            const int64_t wave_row0 = row - lane;
            if (lane == 0 && wave_row0 < n) {
                out[wave_row0 >> 6] = b;
                cnt += (unsigned int)__popcll(b);
            }
        }
    }
    const unsigned long long t = block_count_sum(cnt);
    if (threadIdx.x == 0 && t != 0) atomicAdd(d_count, t);
}

template <typename K, bool HAS_VALID, bool RANGE>
static void test_dispatch(const FilterView& f, const void* keys, const uint8_t* valid, int64_t voff, int64_t n,
                          unsigned long long* out, unsigned long long* d_count, hipStream_t s) {
    filter_test_kernel<K, HAS_VALID, RANGE><<<stream_grid(n, kTestThreads * kTestSteps), kTestThreads, 0, s>>>(
        f, (const K*)keys, valid, voff, n, out, d_count);
}

hipError_t launch_filter_test(const FilterView& f, int key_bytes, const void* keys, const uint8_t* valid, int64_t voff,
                              int64_t n, uint8_t* out_bitmap, int64_t* d_count, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_count, 0, 8, s);
    if (e != hipSuccess || n <= 0) return e;
    DFP_FILTER_DISPATCH(test_dispatch, f, keys, valid, voff, n, (unsigned long long*)out_bitmap,
                        (unsigned long long*)d_count, s);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// select: the passing rows' keys and ids probe_base + row, in row order
// ---------------------------------------------------------------------------
static_assert(kCwSteps % 4 == 0, "the count kernel loads keys in batches of four steps");

// pass 1: word j of tile t covers rows t * 4096 + j * 64 ..; ballots[t * 64 + j], tcnt[t]
template <typename K, bool HAS_VALID, bool RANGE>
__global__ void __launch_bounds__(kCwThreads)
filter_select_count_kernel(FilterView f, const K* __restrict__ keys, const uint8_t* __restrict__ valid, int64_t voff,
                           int64_t n, unsigned long long* __restrict__ ballots, unsigned long long* __restrict__ tcnt) {
    const int lane = threadIdx.x & 63;
    const int64_t tile0 = (int64_t)blockIdx.x * kCwTile;
    unsigned int cnt = 0;
#pragma unroll 1
    for (int s0 = 0; s0 < kCwSteps; s0 += 4) {
        K k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t row = tile0 + (int64_t)(s0 + u) * kCwThreads + threadIdx.x;
            k[u] = row < n ? keys[row] : (K)0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t row = tile0 + (int64_t)(s0 + u) * kCwThreads + threadIdx.x;
            const bool ok = row < n && (!HAS_VALID || bit_valid(valid, voff, row)) && filter_has<RANGE>(f, (int64_t)k[u]);
            const unsigned long long b = __ballot(ok);
            if (lane == 0) {
                ballots[(int64_t)blockIdx.x * kCwWords + (s0 + u) * kCwWaves + (threadIdx.x >> 6)] = b;
                cnt += (unsigned int)__popcll(b);
            }
        }
    }
    const unsigned long long t = block_count_sum(cnt);
    if (threadIdx.x == 0) tcnt[blockIdx.x] = t;
}

// pass 2: toff = the scanned tile counts; out_keys / out_ids hold `n` elements and the
// positions are < the total <= n
template <typename K>
__global__ void __launch_bounds__(kCwThreads)
filter_select_write_kernel(const K* __restrict__ keys, int64_t n, uint32_t probe_base,
                           const unsigned long long* __restrict__ ballots, const unsigned long long* __restrict__ toff,
                           K* __restrict__ out_keys, uint32_t* __restrict__ out_ids) {
    // a set bit names a row < n: pass 1 sets no bit past n
    compact_words_tile(ballots + (int64_t)blockIdx.x * kCwWords, toff[blockIdx.x], (int64_t)blockIdx.x * kCwTile,
                       [&](int64_t row, unsigned long long pos) {
                           out_keys[pos] = keys[row];
                           out_ids[pos] = probe_base + (uint32_t)row;
                       });
}

int64_t filter_select_workspace(int64_t n) { return compact_ws_bytes(compact_tiles(n), kCwWords); }

template <typename K, bool HAS_VALID, bool RANGE>
static void select_dispatch(const FilterView& f, const void* keys, const uint8_t* valid, int64_t voff, int64_t n,
                            int64_t nt, unsigned long long* ballots, unsigned long long* tcnt, hipStream_t s) {
    filter_select_count_kernel<K, HAS_VALID, RANGE><<<(unsigned)nt, kCwThreads, 0, s>>>(f, (const K*)keys, valid, voff,
                                                                                      n, ballots, tcnt);
}

hipError_t launch_filter_select(const FilterView& f, int key_bytes, const void* keys, const uint8_t* valid,
                                int64_t voff, int64_t n, uint32_t probe_base, void* out_keys, uint32_t* out_ids,
                                int64_t* d_count, void* workspace, hipStream_t s) {
    const int64_t nt = compact_tiles(n);
    if (nt == 0) return hipMemsetAsync(d_count, 0, 8, s);
    const CompactWs w = compact_ws_carve(workspace, nt, kCwWords);
    DFP_FILTER_DISPATCH(select_dispatch, f, keys, valid, voff, n, nt, w.words, w.tcnt, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = compact_scan(w, nt, d_count, s)) != hipSuccess) return e;
    if (key_bytes == 8)
        filter_select_write_kernel<int64_t><<<(unsigned)nt, kCwThreads, 0, s>>>(
            (const int64_t*)keys, n, probe_base, w.words, w.tcnt, (int64_t*)out_keys, out_ids);
    else
        filter_select_write_kernel<int32_t><<<(unsigned)nt, kCwThreads, 0, s>>>(
            (const int32_t*)keys, n, probe_base, w.words, w.tcnt, (int32_t*)out_keys, out_ids);
    return hipGetLastError();
}

}  // namespace dfp
