// grid_sync.hip — what a kernel boundary costs against a grid barrier inside one
// persistent launch, at the engine's grid sizes (a config-3 solve is
// ~3,500 dependent launches of ~10 µs).
//
//   A  back-to-back launches of a kernel of G workgroups × 256 threads whose waves
//      read one window of frontier flags (121k flag bytes in all, every flag 0)
//      and exit: the per-launch floor of a sparse round or sweep;
//   B  one cooperative launch of G workgroups running K grid-stride passes over the
//      same flags, a grid barrier after each (agent-scope release before the
//      arrival, acquire after), in three barrier shapes:
//        0 flat: every workgroup polls the arrival counter;
//        1 flat + release word: the last arrival bumps a generation word, the
//          others poll it;
//        2 per-XCD then global: arrivals count per XCD (blockIdx % 8), the last of
//          each XCD arrives at the global counter, whose last arrival bumps the
//          generation word.
// Every spin has a wall-clock deadline (s_memrealtime, 100 MHz), so a grid that
// could not be co-resident ends instead of hanging.
//
//   C  `grid_sync occupancy`: the floor of A at the config-3 sparse grids (2,350
//      and 2,800 workgroups) and the engine kernels' register footprints, with
//      working waves at the front or at the back of the grid (see mode C below).
//
//   hipcc --offload-arch=gfx950 -O3 tools/calib/grid_sync.hip -o /tmp/grid_sync && /tmp/grid_sync [occupancy]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));           \
            return 1;                                                              \
        }                                                                          \
    } while (0)

constexpr int NFLAG = 121252;

__device__ __forceinline__ int scan_flags(const unsigned char* flags, int vb, int nvb, unsigned char* out) {
    // one 64-byte window per wave, grid-stride over the windows
    const int lane = threadIdx.x & 63;
    const int nw = (NFLAG + 63) / 64;
    int any = 0;
    for (int w = vb * 4 + (threadIdx.x >> 6); w < nw; w += nvb * 4) {
        const int i = w * 64 + lane;
        const int f = i < NFLAG ? flags[i] : 0;
        if (__ballot(f != 0)) any = 1;
    }
    if (any && threadIdx.x == 0) out[vb] = 1;
    return any;
}

__global__ __launch_bounds__(256) void k_launch(const unsigned char* flags, unsigned char* out) {
    scan_flags(flags, blockIdx.x, gridDim.x, out);
}

__device__ __forceinline__ bool spin_until(const unsigned* w, unsigned target, unsigned long long deadline) {
    while (__hip_atomic_load(w, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (__builtin_amdgcn_s_memrealtime() > deadline) return false;
    }
    return true;
}
// relaxed polling (no cache invalidation per poll), one acquire fence once it passes
__device__ __forceinline__ bool spin_relaxed(const unsigned* w, unsigned target, unsigned long long deadline) {
    while (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (__builtin_amdgcn_s_memrealtime() > deadline) return false;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return true;
}

template <int SHAPE>
__global__ __launch_bounds__(256) void k_persist(const unsigned char* flags, unsigned char* out, unsigned* sync,
                                                 int k, unsigned long long* tout, int* timeout) {
    const unsigned long long deadline = __builtin_amdgcn_s_memrealtime() + 300000000ULL;   // 3 s
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    unsigned* ctr = sync;            // flat counter
    unsigned* gen = sync + 16;       // generation word
    unsigned* xc = sync + 32;        // per-XCD counters (stride 16 words: separate lines)
    const int G = gridDim.x;
    const int x = blockIdx.x & 7;
    const int per_x = G / 8 + ((G & 7) > x ? 1 : 0);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 1; i <= k; ++i) {
        scan_flags(flags, blockIdx.x, G, out);
        __syncthreads();
        if (threadIdx.x == 0) {
            bool ok = true;
            if (SHAPE == 0) {
                __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                ok = spin_until(ctr, (unsigned)G * (unsigned)i, deadline);
            } else if (SHAPE == 1) {
                const unsigned old = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
                if (old == (unsigned)G * (unsigned)i - 1)
                    __hip_atomic_store(gen, (unsigned)i, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                else
                    ok = spin_until(gen, (unsigned)i, deadline);
            } else if (SHAPE == 3) {   // flat, relaxed polling
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = spin_relaxed(ctr, (unsigned)G * (unsigned)i, deadline);
            } else if (SHAPE == 4) {   // flat + generation word, relaxed polling
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                const unsigned old = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (old == (unsigned)G * (unsigned)i - 1)
                    __hip_atomic_store(gen, (unsigned)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else
                    ok = spin_relaxed(gen, (unsigned)i, deadline);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            } else if (SHAPE == 5) {   // no fences at all (the floor of the arrival / poll traffic)
                const unsigned old = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (old == (unsigned)G * (unsigned)i - 1)
                    __hip_atomic_store(gen, (unsigned)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else
                    while (__hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)i) {
                        __builtin_amdgcn_s_sleep(1);
                        if (__builtin_amdgcn_s_memrealtime() > deadline) { ok = false; break; }
                    }
            } else {
                const unsigned old = __hip_atomic_fetch_add(xc + 16 * x, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
                if (old == (unsigned)per_x * (unsigned)i - 1) {
                    const unsigned o2 = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
                    if (o2 == 8u * (unsigned)i - 1)
                        __hip_atomic_store(gen, (unsigned)i, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    else
                        ok = spin_until(gen, (unsigned)i, deadline);
                } else {
                    ok = spin_until(gen, (unsigned)i, deadline);
                }
            }
            if (!ok) bad = 1;
        }
        __syncthreads();
        if (bad) break;
    }
    if (threadIdx.x == 0) {
        if (bad) atomicOr(timeout, 1);
        tout[blockIdx.x] = __builtin_amdgcn_s_memrealtime() - t0;
    }
}

// ---------------------------------------------------------------- mode C ---
//   C  (`grid_sync occupancy`) the floor of A at the engine's sparse grids and
//      register footprints: does a launch whose grid exceeds what is resident at
//      once pay for the second residency pass, and does it matter where in the
//      grid the working waves sit? The kernel is the engine's sparse prologue:
//      each wave loads the flag bytes of its WPW windows (strided across the
//      grid, all loads issued together), ballots them and exits when none is set.
//      NV pins the kernel's VGPR allocation (a write to v[NV-1]: registers, no
//      scratch), so one source runs at occupancy 8, 5 and 4 waves/SIMD.
//      A window whose flags are set makes its wave follow a chain of
//      dependent loads per lane (random lines of a 16 MB table: a working
//      window's arc → record → distance … chain). The host sets 1 % of the
//      waves' first windows, at the front of the grid or at the back. The chain
//      is 5 loads (a working window of the engine) and 20 loads: at 5 the kernel
//      is shorter than the launch-to-launch floor, which hides it; at 20 the
//      working waves outlast the floor as the engine's 11–20 µs launches do, and
//      a wait for residency ahead of them would show.
constexpr int OCC_TABLE = 1 << 22;   // ints

template <int NV>
__device__ __forceinline__ void pin_vgprs() {
    static_assert(NV == 64 || NV == 96 || NV == 116, "one of the measured footprints");
    if (NV == 64) asm volatile("v_mov_b32 v63, 0" ::: "v63");
    if (NV == 96) asm volatile("v_mov_b32 v95, 0" ::: "v95");
    if (NV == 116) asm volatile("v_mov_b32 v115, 0" ::: "v115");
}

template <int NV, int WPW>
__global__ __launch_bounds__(256) void k_occ(const unsigned char* __restrict__ flags, int nwin,
                                             const int* __restrict__ table, int chain, unsigned char* out) {
    pin_vgprs<NV>();
    const int lane = threadIdx.x & 63;
    const int tw = gridDim.x * 4;
    const int w0 = blockIdx.x * 4 + (threadIdx.x >> 6);
    int f[WPW];
#pragma unroll
    for (int j = 0; j < WPW; ++j) {
        const int w = w0 + j * tw;
        f[j] = w < nwin ? flags[(size_t)w * 64 + lane] : 0;
    }
    unsigned long long mk[WPW];
#pragma unroll
    for (int j = 0; j < WPW; ++j) mk[j] = __ballot(f[j] != 0);
    int acc = 0;
#pragma unroll
    for (int j = 0; j < WPW; ++j) {
        if (!mk[j]) continue;
        int i = (int)(((unsigned)(w0 + j * tw) * 64u + (unsigned)lane) * 2654435761u >> 10);   // < 2^22
        for (int k = 0; k < chain; ++k) i = table[i];
        acc |= i;
    }
    if (acc < 0) out[0] = 1;   // (never: table entries are indices; keeps the chain alive)
}

template <int NV, int WPW>
static int occ_setting(const char* place, int G, int nwin, int nwork, const unsigned char* flags, const int* table,
                       int chain, unsigned char* out, hipEvent_t a, hipEvent_t b, bool& first) {
    int per_cu = 0;
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_occ<NV, WPW>, 256, 0));
    const int L = 2000;
    for (int rep = 0; rep < 3; ++rep) {
        for (int i = 0; i < 50; ++i) hipLaunchKernelGGL((k_occ<NV, WPW>), dim3(G), dim3(256), 0, 0, flags, nwin, table, chain, out);
        CK(hipEventRecord(a, 0));
        for (int i = 0; i < L; ++i) hipLaunchKernelGGL((k_occ<NV, WPW>), dim3(G), dim3(256), 0, 0, flags, nwin, table, chain, out);
        CK(hipEventRecord(b, 0));
        CK(hipEventSynchronize(b));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, a, b));
        std::printf("%s {\"mode\": \"occupancy\", \"workgroups\": %d, \"windows_per_wave\": %d, \"vgprs\": %d, "
                    "\"workgroups_per_cu\": %d, \"working_waves\": %d, \"chain\": %d, \"placement\": \"%s\", \"rep\": %d, "
                    "\"us_per_launch\": %.3f}",
                    first ? "" : ",\n", G, WPW, NV, per_cu, nwork, nwork ? chain : 0, place, rep, ms * 1000.0 / L);
        first = false;
    }
    return 0;
}

static int occupancy_mode() {
    int ncu = 0;
    CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
    const int GMAX = 2800, NWIN = GMAX * 4 * 2;
    unsigned char *flags, *out;
    int* table;
    CK(hipMalloc(&flags, (size_t)NWIN * 64));
    CK(hipMalloc(&out, 64));
    CK(hipMalloc(&table, (size_t)OCC_TABLE * sizeof(int)));
    {
        std::vector<int> h(OCC_TABLE);
        unsigned x = 12345;
        for (int i = 0; i < OCC_TABLE; ++i) {
            x = x * 1664525u + 1013904223u;
            h[i] = (int)(x >> 10);   // < 2^22
        }
        CK(hipMemcpy(table, h.data(), (size_t)OCC_TABLE * sizeof(int), hipMemcpyHostToDevice));
    }
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    std::printf("{\"rows\": [\n");
    bool first = true;
    // the engine's config-3 sparse grids at WPW 2 (k_bf_round 2,350; k_sweep 2,800
    // workgroups), and the same windows at WPW 4 (half the grid)
    for (int G2 : {2350, 2800}) {
        const int nwin = G2 * 4 * 2;
        const int nwork = G2 * 4 / 100;   // 1 % of the waves of the WPW-2 grid, in every setting
        for (int wpw : {2, 4}) {
            const int G = G2 * 2 / wpw;
            const int tw = G * 4;
            for (int pc = 0; pc < 5; ++pc) {   // no working wave; front and back at each chain length
                const int place = pc == 0 ? 0 : 1 + (pc - 1) % 2;
                const int chain = pc < 3 ? 5 : 20;
                CK(hipMemset(flags, 0, (size_t)NWIN * 64));
                // a working wave's first window is flagged: windows [0, nwork) are the first
                // windows of the grid's first waves, [tw − nwork, tw) of its last
                if (place == 1) CK(hipMemset(flags, 1, (size_t)nwork * 64));
                if (place == 2) CK(hipMemset(flags + (size_t)(tw - nwork) * 64, 1, (size_t)nwork * 64));
                const char* pn = place == 0 ? "none" : place == 1 ? "front" : "back";
                const int nw = place ? nwork : 0;
#define OCC_RUN(NV, W) if (occ_setting<NV, W>(pn, G, nwin, nw, flags, table, chain, out, a, b, first)) return 1
                if (wpw == 2) {
                    OCC_RUN(64, 2);
                    OCC_RUN(96, 2);
                    OCC_RUN(116, 2);
                } else {
                    OCC_RUN(64, 4);
                    OCC_RUN(96, 4);
                    OCC_RUN(116, 4);
                }
#undef OCC_RUN
            }
        }
    }
    std::printf("\n], \"cus\": %d}\n", ncu);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "occupancy") return occupancy_mode();
    unsigned char *flags, *out;
    unsigned* sync;
    unsigned long long* tout;
    int* timeout;
    CK(hipMalloc(&flags, NFLAG));
    CK(hipMalloc(&out, 1 << 16));
    CK(hipMalloc(&sync, 4096));
    CK(hipMalloc(&tout, 8192 * sizeof(unsigned long long)));
    CK(hipMalloc(&timeout, sizeof(int)));
    CK(hipMemset(flags, 0, NFLAG));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    std::printf("{\"rows\": [\n");
    bool first = true;
    const int L = 2000;
    for (int G : {256, 2304}) {
        for (int rep = 0; rep < 1; ++rep) {
            for (int i = 0; i < 50; ++i) hipLaunchKernelGGL(k_launch, dim3(G), dim3(256), 0, 0, flags, out);
            CK(hipEventRecord(a, 0));
            for (int i = 0; i < L; ++i) hipLaunchKernelGGL(k_launch, dim3(G), dim3(256), 0, 0, flags, out);
            CK(hipEventRecord(b, 0));
            CK(hipEventSynchronize(b));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, a, b));
            std::printf("%s {\"mode\": \"launches\", \"workgroups\": %d, \"rep\": %d, \"us_per_step\": %.3f}",
                        first ? "" : ",\n", G, rep, ms * 1000.0 / L);
            first = false;
        }
    }
    int dev = 0, ncu = 0, per_cu = 0;
    CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_persist<2>, 256, 0));
    const int K = 2000;
    for (int shape = 3; shape < 6; ++shape) {
        for (int G : {64, 128, 256, 512}) {
            if (G > ncu * per_cu) continue;
            for (int rep = 0; rep < 2; ++rep) {
                CK(hipMemset(sync, 0, 4096));
                CK(hipMemset(timeout, 0, sizeof(int)));
                int k = K;
                void* args[] = {&flags, &out, &sync, &k, &tout, &timeout};
                const void* fn = shape == 3 ? (const void*)k_persist<3>
                                 : shape == 4 ? (const void*)k_persist<4> : (const void*)k_persist<5>;
                CK(hipEventRecord(a, 0));
                CK(hipLaunchCooperativeKernel(fn, dim3(G), dim3(256), args, 0, 0));
                CK(hipEventRecord(b, 0));
                CK(hipEventSynchronize(b));
                float ms = 0;
                CK(hipEventElapsedTime(&ms, a, b));
                int to = 0;
                CK(hipMemcpy(&to, timeout, sizeof(int), hipMemcpyDeviceToHost));
                std::vector<unsigned long long> h(G);
                CK(hipMemcpy(h.data(), tout, G * sizeof(unsigned long long), hipMemcpyDeviceToHost));
                unsigned long long mx = 0;
                for (auto t : h) mx = t > mx ? t : mx;
                std::printf(",\n {\"mode\": \"barrier\", \"shape\": %d, \"workgroups\": %d, \"rep\": %d, "
                            "\"us_per_step\": %.3f, \"event_us_per_step\": %.3f, \"timeout\": %d}",
                            shape, G, rep, mx / 100.0 / K, ms * 1000.0 / K, to);
            }
        }
    }
    std::printf("\n], \"cus\": %d, \"blocks_per_cu\": %d}\n", ncu, per_cu);
    return 0;
}
