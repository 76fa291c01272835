// hj_lookup.h — the table lookup of four consecutive probe rows per lane (lookup4) and the
// row count behind a match ref, shared by the pair probes (hj_kernels.hip) and the match
// probe and pair plan family (hj_match.hip). Table layout: hj_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hj_device.h"
#include "hj_util.h"

namespace dfp {

// home bucket of a key's stored form (no rehash)
__device__ __forceinline__ uint32_t stored_bucket(unsigned long long sk, uint32_t nb) { return bucket_of(sk, nb); }

typedef long long v2i64 __attribute__((ext_vector_type(2)));

template <typename K, bool NT = false>
__device__ __forceinline__ void load4(const void* keys, int64_t row0, int64_t n, bool vec, int64_t (&k)[4]) {
    const K* kp = reinterpret_cast<const K*>(keys);
    if (vec && row0 + 4 <= n) {
        if constexpr (sizeof(K) == 8) {
            const v2i64* p = reinterpret_cast<const v2i64*>(kp + row0);
            v2i64 a, b;
            if constexpr (NT) {
                a = __builtin_nontemporal_load(p);
                b = __builtin_nontemporal_load(p + 1);
            } else {
                a = p[0];
                b = p[1];
            }
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

// count of build rows behind a match ref
__device__ __forceinline__ uint32_t ref_count(const uint32_t* dup_rows, uint32_t ref, uint32_t off_mask) {
    const uint32_t c = ref_count_inline(ref, off_mask);
    return c == kCountUnknown ? dup_rows[ref & off_mask] : c;
}

// One bucket line: ref of `sk` if present, else kMiss; *more = the line is full, does
// not hold the key, and some insert passed it (meta bit 0): look at the next bucket of
// the chunk. Slots fill in order and are never freed, so an empty slot ends a key's probe
// sequence, and so does a full bucket that no insert ever passed. Branch-free.
__device__ __forceinline__ uint32_t scan_line(const uint4& a0, const uint4& a1, const uint4& a2, const uint4& a3,
                                              unsigned long long sk, bool* more, uint32_t* cnt) {
    const unsigned long long k0 = ((unsigned long long)a0.y << 32) | a0.x;
    const unsigned long long k1 = ((unsigned long long)a0.w << 32) | a0.z;
    const unsigned long long k2 = ((unsigned long long)a1.y << 32) | a1.x;
    const unsigned long long k3 = ((unsigned long long)a1.w << 32) | a1.z;
    const unsigned long long k4 = ((unsigned long long)a2.y << 32) | a2.x;
    const bool e0 = k0 == sk, e1 = k1 == sk, e2 = k2 == sk, e3 = k3 == sk, e4 = k4 == sk;
    const bool z = (k0 == 0) | (k1 == 0) | (k2 == 0) | (k3 == 0) | (k4 == 0);
    uint32_t ref = e4 ? a3.z : kMiss;
    ref = e3 ? a3.y : ref;
    ref = e2 ? a3.x : ref;
    ref = e1 ? a2.w : ref;
    ref = e0 ? a2.z : ref;
    *more = (ref == kMiss) & !z & ((a3.w & 1u) != 0);
    // row count: 0 miss, 1 single row, the inline meta count of a duplicated key, or
    // kCountUnknown (read dup_rows[off])
    const uint32_t m = a3.w;
    uint32_t c = e4 ? (m >> 25) : 0u;
    c = e3 ? (m >> 19) : c;
    c = e2 ? (m >> 13) : c;
    c = e1 ? (m >> 7) : c;
    c = e0 ? (m >> 1) : c;
    c &= 63u;
    *cnt = ref == kMiss ? 0u : (!(ref & kDupFlag) ? 1u : (c ? c : kCountUnknown));
    return ref;
}

// Refs of the four probe rows row0..row0+3 (kMiss: no match, null, or past n).
template <typename K, bool HAS_VALID, bool NT = false>
__device__ __forceinline__ void lookup4(const TableView& tv, const void* __restrict__ keys,
                                        const uint8_t* __restrict__ valid, int64_t voff, int64_t n, bool vec,
                                        int64_t row0, uint32_t (&ref)[4], uint32_t (&cnt)[4]) {
    if (tv.dense != nullptr) {  // direct-addressed table: range check + one 4-byte read per row
        int64_t k[4];
        load4<K, NT>(keys, row0, n, vec, k);
        uint32_t r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool in = (row0 + q < n) && (!HAS_VALID || bit_valid(valid, voff, row0 + q));
            const uint64_t idx = (uint64_t)k[q] - (uint64_t)tv.dmin;
            r[q] = (in && idx < tv.drange) ? tv.dense[idx] : kMiss;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ref[q] = r[q];
            // packed dense refs carry counts <= 15 (or a run) in bits 24-30 (kPackedMask tables)
            cnt[q] = ref_count_inline(r[q], tv.off_mask);
        }
        return;
    }
    const Bucket* __restrict__ tbl = tv.tbl;
    const uint32_t cmask = (1u << tv.clog2) - 1;
    int64_t k[4];
    load4<K, NT>(keys, row0, n, vec, k);
    bool in[4];
    unsigned long long sk[4];
    uint32_t b[4];
    uint4 L0[4], L1[4], L2[4], L3[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        in[q] = (row0 + q < n) && (!HAS_VALID || bit_valid(valid, voff, row0 + q));
        sk[q] = stored_key(k[q]);
        b[q] = (in[q] && sk[q] != 0) ? stored_bucket(sk[q], tv.nb) : tv.nb;
    }
    // issue the 64-byte bucket line of all four rows before any compare (MLP)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4* p = reinterpret_cast<const uint4*>(tbl + b[q]);
        L0[q] = p[0]; L1[q] = p[1]; L2[q] = p[2]; L3[q] = p[3];
    }
    bool more[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        ref[q] = scan_line(L0[q], L1[q], L2[q], L3[q], sk[q], &more[q], &cnt[q]);
        if (sk[q] == 0) {  // key 0: the side bucket (ref[0] = word 10, meta = word 15 = rows)
            ref[q] = L3[q].w ? L2[q].z : kMiss;
            cnt[q] = L3[q].w;
            more[q] = false;
        }
        if (!in[q]) { ref[q] = kMiss; cnt[q] = 0; more[q] = false; }
    }
    // rare: the home line is full and does not hold the key
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t bb = b[q];
        for (uint32_t probes = 0; more[q] && probes < cmask; ++probes) {
            bb = (bb & ~cmask) | ((bb + 1) & cmask);
            const uint4* p = reinterpret_cast<const uint4*>(tbl + bb);
            ref[q] = scan_line(p[0], p[1], p[2], p[3], sk[q], &more[q], &cnt[q]);
        }
    }
}

__device__ __forceinline__ uint32_t resolve_count(const uint32_t* dup_rows, uint32_t ref, uint32_t cnt,
                                                  uint32_t off_mask) {
    return cnt == kCountUnknown ? dup_rows[ref & off_mask] : cnt;
}

}  // namespace dfp
