// floor(a / eps) without an integer division, from a reciprocal computed once per ε.
//
// Every Bellman-Ford relaxation measures an arc in units of ε: floor(x / ε) + 1.
// Scaled prices need 64 bits, so `/` and `%` there are the compiler's 64-bit
// software division (~135 instructions on gfx950) in the middle of the chain
// record → length → atomic. ε is fixed for a whole phase; its reciprocal is
// computed once on the host (Ctl::inv) and the quotient comes from one double
// multiply, a floor and an integer correction.
//
// Why one correction step each way is enough. Let x = a / eps (exact),
// t = fl(fl(a) · inv) with inv = fl(1 / fl(eps)). Each fl() is one rounding to
// double, relative error ≤ u = 2⁻⁵³: the conversion of a, the conversion of eps
// (exact below 2⁵³), the reciprocal, the product. So t = x·(1 + δ) with
// |δ| ≤ (1 + u)⁴ − 1 < 2⁻⁵⁰. The fast path is taken only when |t| < 2⁴¹; then
// |x| < 2⁴¹ / (1 − 2⁻⁵⁰) and |t − x| < 2⁻⁵⁰ · 2⁴¹ · (1 + 2⁻⁴⁹) < 2⁻⁸ < 1.
// Two reals less than 1 apart have floors at most 1 apart, so q = floor(t) is
// floor(x) − 1, floor(x) or floor(x) + 1, and the remainder r = a − q·eps lies
// in [−eps, 2·eps): r < 0 means q is one too large, r ≥ eps one too small.
// q·eps is within 2·eps of a, and |a| < 2⁶² with eps ≤ 2⁶⁰ (include/ksmcmf.h,
// range contract) keeps it inside 64 bits; it is formed in unsigned arithmetic
// all the same. floor(t) is an integer of magnitude ≤ 2⁴¹, so adding 1.5·2⁵² is
// exact and leaves it, in two's complement, in the sum's low 51 mantissa bits.
//
// |t| ≥ 2⁴¹ (saturated lengths: the prices of cut-off nodes; costs far above ε
// in the last phases) takes the division. The branch is rare and in practice
// wave-uniform.
//
// -DKS_LEN_DIV: the division always (A/B builds only).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KS_LEN_FN __host__ __device__ __forceinline__
#else
#define KS_LEN_FN inline
#endif
#ifndef KS_LEN_FALLBACK_HOOK   // tests count the calls that take the division
#define KS_LEN_FALLBACK_HOOK()
#endif

// floor(a / eps) for eps ≥ 1, inv = 1.0 / (double)eps.
KS_LEN_FN long long ks_floordiv_inv(long long a, long long eps, double inv) {
#ifndef KS_LEN_DIV
    const double t = (double)a * inv;
    if (__builtin_fabs(t) < 0x1p41) {
        union {
            double d;
            unsigned long long u;
        } m;
        m.d = __builtin_floor(t) + 0x1.8p52;
        long long q = (long long)(m.u << 13) >> 13;   // the low 51 bits, sign-extended
        const long long r = (long long)((unsigned long long)a - (unsigned long long)q * (unsigned long long)eps);
        q -= r < 0 ? 1 : 0;
        q += r >= eps ? 1 : 0;
        return q;
    }
    KS_LEN_FALLBACK_HOOK();
#else
    (void)inv;
#endif
    long long q = a / eps;
    if ((a % eps) != 0 && a < 0) --q;
    return q;
}
