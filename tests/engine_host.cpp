// TEST INFRASTRUCTURE: ks_engine_impl.h compiled for the host (tests/test_engine_shapes_cpu.py),
// so the test-side restatements of degree_class, class_lanes, win_batches and win_slots and of
// the constants are compared with the header itself.
// (g++ has no __hip_atomic_* builtins; the header's one device-only helper that names them
// is never called here)
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_fetch_add(p, v, order, scope) __atomic_fetch_add(p, v, order)
#include "../ksched_amd/csrc/ks_engine_impl.h"

extern "C" {
void engine_classes(const int* cap, int* out, int n) {
    for (int i = 0; i < n; ++i) out[i] = ks::impl::degree_class(cap[i]);
}
void engine_windows(int* lanes, int* batches, int* slots) {   // NGC entries each
    for (int c = 0; c < ks::impl::NGC; ++c) {
        lanes[c] = ks::impl::class_lanes(c);
        batches[c] = ks::impl::win_batches(c);
        slots[c] = ks::impl::win_slots(c);
    }
}
// BLK, WAVE, WPB, NGC, HEAVY_MIN, CHUNK, HSPLIT, WPW, HUB_LDS, BX_CAP, CCLS
void engine_constants(int* out) {
    using namespace ks::impl;
    const int v[] = {BLK, WAVE, WPB, NGC, HEAVY_MIN, CHUNK, HSPLIT, WPW, HUB_LDS, BX_CAP, CCLS};
    for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}
}
