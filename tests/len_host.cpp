// TEST INFRASTRUCTURE: ks_len.h compiled for the host (tests/test_len_cpu.py).
// Counts the calls that took the division so the test can see both branches run.
static long long g_fallbacks = 0;
#define KS_LEN_FALLBACK_HOOK() (++g_fallbacks)
#include "../ksched_amd/csrc/ks_len.h"

extern "C" {
// out[i] = floor(a[i] / eps[i]); inv is 1.0 / (double)eps as the engine's host computes it
void len_floordiv(const long long* a, const long long* eps, long long* out, long long n) {
    for (long long i = 0; i < n; ++i) out[i] = ks_floordiv_inv(a[i], eps[i], 1.0 / (double)eps[i]);
}
long long len_fallbacks() { return g_fallbacks; }
void len_reset() { g_fallbacks = 0; }
}
