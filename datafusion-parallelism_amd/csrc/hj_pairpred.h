// hj_pairpred.h — the device side of the pair pass rule (include/hj.h, "pair filter"): whether
// one pair (build row, probe row) passes a PairPred. Shared by the kernels that evaluate a
// predicate on pairs in memory (hj_pairfilter.hip) and on the candidates of a lookup
// (hj_match.hip, the filtered match probe and pair plan). The predicate travels as a kernel argument, so
// every descriptor - class, width, op, column - is wave-uniform and the switches over them
// are scalar branches; only the operand gathers and the BYTES compare loop are per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hj_launch.h"
#include "hj_util.h"

namespace dfp {

// One fixed-width operand as 64 bits, sign- (INT) or zero-extended; the column is
// wave-uniform, so the width switch and the alignment test are scalar branches.
__device__ __forceinline__ uint64_t pf_fixed_bits(const KeyCol& c, int64_t row, bool sign) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(c.values) + row * c.width;
    const bool aligned = (reinterpret_cast<uintptr_t>(c.values) & (uintptr_t)(c.width - 1)) == 0;
    uint64_t v;
    if (aligned) {
        switch (c.width) {
            case 1: v = *p; break;
            case 2: v = *reinterpret_cast<const uint16_t*>(p); break;
            case 4: v = *reinterpret_cast<const uint32_t*>(p); break;
            default: v = *reinterpret_cast<const uint64_t*>(p); break;
        }
    } else {
        v = 0;
        for (int i = 0; i < c.width; ++i) v |= (uint64_t)p[i] << (8 * i);
    }
    if (sign && c.width < 8) {
        const int sh = 64 - 8 * c.width;
        v = (uint64_t)((int64_t)(v << sh) >> sh);
    }
    return v;
}

// The comparison key of one fixed-width operand: signed order of the keys = the class's
// order of the values. INT: the value; UINT: the value with the top bit flipped; FLOAT: the
// double's totalOrder key b ^ ((b >> 63) & INT64_MAX), a float32 widened first.
__device__ __forceinline__ int64_t pf_float_key(uint64_t bits) {
    const int64_t b = (int64_t)bits;
    return b ^ ((b >> 63) & INT64_MAX);
}

__device__ __forceinline__ int64_t pf_fixed_key(const KeyCol& c, int64_t row, int cls) {
    if (cls == kPfFloat) {
        uint64_t bits = pf_fixed_bits(c, row, false);
        if (c.width == 4) bits = (uint64_t)__double_as_longlong((double)__uint_as_float((uint32_t)bits));
        return pf_float_key(bits);
    }
    const uint64_t v = pf_fixed_bits(c, row, cls == kPfInt);
    return (int64_t)(cls == kPfUint ? v ^ (1ull << 63) : v);
}

__device__ __forceinline__ int64_t pf_const_key(int64_t k, int cls) {
    if (cls == kPfFloat) return pf_float_key((uint64_t)k);
    return cls == kPfUint ? (int64_t)((uint64_t)k ^ (1ull << 63)) : k;
}

__device__ __forceinline__ void pf_var_range(const KeyCol& c, int64_t row, int64_t* a, int64_t* b) {
    if (c.offset_bytes == 8) {
        const int64_t* o = reinterpret_cast<const int64_t*>(c.offsets);
        *a = o[row];
        *b = o[row + 1];
    } else {
        const int32_t* o = reinterpret_cast<const int32_t*>(c.offsets);
        *a = o[row];
        *b = o[row + 1];
    }
}

// -1 / 0 / 1: lexicographic order on unsigned bytes, a proper prefix is smaller
__device__ __forceinline__ int pf_bytes_cmp(const KeyCol& x, int64_t xr, const KeyCol& y, int64_t yr) {
    int64_t xa, xb, ya, yb;
    pf_var_range(x, xr, &xa, &xb);
    pf_var_range(y, yr, &ya, &yb);
    const uint8_t* xp = reinterpret_cast<const uint8_t*>(x.values) + xa;
    const uint8_t* yp = reinterpret_cast<const uint8_t*>(y.values) + ya;
    const int64_t lx = xb - xa, ly = yb - ya, m = lx < ly ? lx : ly;
    for (int64_t i = 0; i < m; ++i) {
        const int d = (int)xp[i] - (int)yp[i];
        if (d != 0) return d < 0 ? -1 : 1;
    }
    return lx < ly ? -1 : (lx > ly ? 1 : 0);
}

__device__ __forceinline__ bool pf_compare(int op, int64_t x, int64_t y) {
    switch (op) {
        case 0: return x == y;
        case 1: return x != y;
        case 2: return x < y;
        case 3: return x <= y;
        case 4: return x > y;
        default: return x >= y;
    }
}

// whether pair (b, p) passes every term; `live` is false for lanes past n
template <bool BYTES>
__device__ __forceinline__ bool pf_pair_passes(const PairPred& pr, bool live, uint64_t b, uint32_t p) {
    bool pass = live && b < (uint64_t)pr.build_rows && (int64_t)p < pr.probe_rows;
    for (int t = 0; t < pr.nterms; ++t) {  // uniform trip count and descriptors
        const PairTerm& tm = pr.t[t];
        const KeyCol& lc = tm.lhs_side == kPfBuild ? pr.b[tm.lhs_col] : pr.p[tm.lhs_col];
        const int64_t lrow = tm.lhs_side == kPfBuild ? (int64_t)b : (int64_t)p;
        const bool rconst = tm.rhs_side == kPfConst;
        const KeyCol& rc = tm.rhs_side == kPfBuild ? pr.b[rconst ? 0 : tm.rhs_col] : pr.p[rconst ? 0 : tm.rhs_col];
        const int64_t rrow = tm.rhs_side == kPfBuild ? (int64_t)b : (int64_t)p;
        if (pass) {  // per lane: a failed or out-of-range pair dereferences nothing
            bool ok = bit_valid(lc.valid, lc.voff, lrow) && (rconst || bit_valid(rc.valid, rc.voff, rrow));
            if (ok) {
                int64_t x, y;
                if (BYTES && tm.cls == kPfBytes) {
                    x = pf_bytes_cmp(lc, lrow, rc, rrow);
                    y = 0;
                } else {
                    x = pf_fixed_key(lc, lrow, tm.cls);
                    y = rconst ? pf_const_key(tm.rhs_const, tm.cls) : pf_fixed_key(rc, rrow, tm.cls);
                }
                ok = pf_compare(tm.op, x, y);
            }
            pass = ok;
        }
    }
    return pass;
}

}  // namespace dfp
