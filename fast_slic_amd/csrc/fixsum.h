// fixsum.h -- the exact fixed-point accumulator of float sums (pool.hip: the tiles' partials; region.hip: the nodes of a group).
// kPoolLimbs int64 words, one 32-bit limb each, bit 0 of limb 0 weighs 2^kPoolLsb (pool.h); limb j of an accumulator is at
// a[j * lstride].  Adds are integer atomics, so the order of arrival cannot change a bit; fix_to_float rounds once.  Device code
// only.  tests/pool_ref.py states the model (exact_sum_bits), tests/test_gpu_pool_exact.py pins the bits.  Internal to the library.
#pragma once
#include "pool.h"

namespace fslic {

// Adds the finite f32 s exactly (down to 2^kPoolLsb) to the fixed-point accumulator at a (limb j at a[j * lstride]): its 24-bit
// mantissa lands on one or two limbs, one no-return 64-bit integer atomic each.  Magnitudes below 2^kPoolLsb are truncated (towards
// zero, symmetric in sign).  A NaN / Inf partial adds 2^40 to the top limb, which makes the entry +inf (unspecified by contract).
static __device__ __forceinline__ void fix_add(unsigned long long* a, size_t lstride, float s) {
    const uint32_t u = __float_as_uint(s);
    const uint32_t ex = (u >> 23) & 0xFFu;
    if (ex == 0xFFu) { atomicAdd(a + (size_t)(kPoolLimbs - 1) * lstride, 1ull << 40); return; }
    if (ex == 0u) return;                                   // zero, subnormals: below 2^-126
    unsigned long long m = (u & 0x7FFFFFu) | 0x800000u;     // s = m * 2^(ex - 150)
    int sh = (int)ex - 150 - kPoolLsb;                      // fixed-point position of m's bit 0
    if (sh < 0) {
        if (sh <= -24) return;
        m >>= -sh;
        sh = 0;
    }
    const int li = sh >> 5;                                 // ex <= 254: li <= 6, and m << (sh & 31) < 2^32 when li == 6
    m <<= (sh & 31);
    unsigned long long lo = m & 0xFFFFFFFFull, hi = m >> 32;
    if (u >> 31) { lo = 0ull - lo; hi = 0ull - hi; }
    if (lo) atomicAdd(a + (size_t)li * lstride, lo);
    if (hi && li + 1 < kPoolLimbs) atomicAdd(a + (size_t)(li + 1) * lstride, hi);
}

// The accumulator (kPoolLimbs words, a[j * lstride]) rounded once to the nearest f32 (ties to even); >= 2^128: +-inf.
static __device__ __forceinline__ float fix_to_float(const unsigned long long* a, size_t lstride) {
    uint32_t m[kPoolLimbs];
    long long carry = 0;
#pragma unroll
    for (int j = 0; j < kPoolLimbs - 1; ++j) {              // limbs 0..5 into [0, 2^32), the sign in the top word
        const long long t = (long long)a[(size_t)j * lstride] + carry;
        m[j] = (uint32_t)t;
        carry = t >> 32;
    }
    long long top = (long long)a[(size_t)(kPoolLimbs - 1) * lstride] + carry;
    const bool neg = top < 0;
    if (neg) {                                              // magnitude: ~x + 1 over all limbs
        unsigned long long c = 1;
#pragma unroll
        for (int j = 0; j < kPoolLimbs - 1; ++j) {
            const unsigned long long t = (unsigned long long)(uint32_t)~m[j] + c;
            m[j] = (uint32_t)t;
            c = t >> 32;
        }
        top = ~top + (long long)c;
    }
    if (top >= (1ll << 32)) return neg ? -__builtin_inff() : __builtin_inff();
    m[kPoolLimbs - 1] = (uint32_t)top;
    int j = -1;
#pragma unroll
    for (int i = 0; i < kPoolLimbs; ++i) if (m[i] != 0u) j = i;
    if (j < 0) return 0.0f;
    uint32_t w2 = 0, w1 = 0, w0 = 0;                        // the highest non-zero limb and the two below it (no dynamic index)
    bool sticky = false;
#pragma unroll
    for (int i = 0; i < kPoolLimbs; ++i) {
        if (i == j) w2 = m[i];
        if (i == j - 1) w1 = m[i];
        if (i == j - 2) w0 = m[i];
        if (i < j - 2 && m[i] != 0u) sticky = true;
    }
    const int b = 31 - __clz(w2);
    const unsigned long long hw = ((unsigned long long)w2 << 32) | w1;                          // leading one at bit 32 + b
    const unsigned long long hi = (hw << (31 - b)) | ((unsigned long long)w0 >> (b + 1));      // leading one at bit 63
    sticky = sticky || ((unsigned long long)w0 & ((1ull << (b + 1)) - 1ull)) != 0ull;
    unsigned long long mant = hi >> 40;
    const unsigned long long rest = hi & ((1ull << 40) - 1ull), half = 1ull << 39;
    int P = 32 * j + b;                                     // fixed-point position of the leading one
    if (rest > half || (rest == half && (sticky || (mant & 1ull)))) {
        if (++mant == (1ull << 24)) { mant >>= 1; ++P; }
    }
    const float f = ldexpf((float)(uint32_t)mant, P - 23 + kPoolLsb);   // exact: 24 bits, at least 2^-96 (inf beyond f32)
    return neg ? -f : f;
}

}  // namespace fslic
