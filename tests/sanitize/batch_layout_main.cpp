// Stand-alone check of the batch layout helpers (ks_batch_node_offsets,
// ks_batch_translate_deltas) for a sanitizer build: the edge cases of
// tests/test_batch_rounds_cpu.py with exactly sized heap buffers, so a write past an
// array or a read before a check shows under -fsanitize=address,undefined. Host code
// only: no device is opened. Build (from the repository root, after the library's
// objects exist in ksched_amd/build):
//
//   SAN="-Xarch_host -fsanitize=address,undefined"
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Iinclude $SAN \
//       -c ksched_amd/csrc/ks_batch.hip -o /tmp/ks_batch_san.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude $SAN \
//       -c tests/sanitize/batch_layout_main.cpp -o /tmp/batch_layout_main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/batch_layout_main.o /tmp/ks_batch_san.o \
//       $(ls ksched_amd/build/lib_*.o | grep -v ks_batch) -ldl -o /tmp/batch_layout_san
//   /tmp/batch_layout_san
#include <cstdio>
#include <cstring>
#include <vector>

#include "ksmcmf.h"

static int fails = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++fails;                                                     \
        }                                                                \
    } while (0)

static std::vector<ks_delta> stream() {
    std::vector<ks_delta> d(5);
    std::memset(d.data(), 0, d.size() * sizeof(ks_delta));
    const int kinds[5] = {KS_ADD_NODE, KS_REMOVE_NODE, KS_SET_EXCESS, KS_ADD_ARC, KS_UPDATE_ARC};
    const uint64_t id[5] = {10, 3, 1, 0, 0}, src[5] = {0, 0, 0, 10, 4}, dst[5] = {0, 0, 0, 2, 10};
    for (int i = 0; i < 5; ++i) {
        d[i].kind = kinds[i];
        d[i].id = id[i];
        d[i].src = src[i];
        d[i].dst = dst[i];
        d[i].cap = 1;
        d[i].cost = 7;
        d[i].excess = -5;
    }
    return d;
}

int main() {
    {   // offsets: spare 0 is the running sum; spare s adds i·s; k = 0 writes one entry
        const std::vector<uint64_t> mx = {2432, 1217, 612, 2432, 368, 1217};
        std::vector<int64_t> off0(mx.size() + 1), off(mx.size() + 1);
        CHECK(ks_batch_node_offsets(mx.data(), mx.size(), 0, off0.data()) == KS_OK);
        int64_t sum = 0;
        for (size_t i = 0; i < mx.size(); ++i) {
            CHECK(off0[i] == sum);
            sum += (int64_t)mx[i];
        }
        CHECK(off0[mx.size()] == sum);
        for (size_t spare : {size_t(1), size_t(16), size_t(256)}) {
            CHECK(ks_batch_node_offsets(mx.data(), mx.size(), spare, off.data()) == KS_OK);
            for (size_t i = 0; i <= mx.size(); ++i) CHECK(off[i] == off0[i] + (int64_t)(i * spare));
        }
        std::vector<int64_t> one(1, -1);
        CHECK(ks_batch_node_offsets(nullptr, 0, 7, one.data()) == KS_OK && one[0] == 0);
        CHECK(ks_batch_node_offsets(nullptr, 2, 0, one.data()) == KS_E_INVALID);
        CHECK(ks_batch_node_offsets(mx.data(), 2, 0, nullptr) == KS_E_INVALID);
    }
    {   // translate: every kind's ids move, the rest stays
        const std::vector<ks_delta> d = stream();
        std::vector<ks_delta> out(d.size());
        CHECK(ks_batch_translate_deltas(100, 110, d.data(), d.size(), out.data()) == KS_OK);
        const uint64_t id[5] = {110, 103, 101, 0, 0}, src[5] = {0, 0, 0, 110, 104}, dst[5] = {0, 0, 0, 102, 110};
        for (int i = 0; i < 5; ++i) {
            CHECK(out[i].id == id[i] && out[i].src == src[i] && out[i].dst == dst[i]);
            CHECK(out[i].kind == d[i].kind && out[i].cap == 1 && out[i].cost == 7 && out[i].excess == -5);
        }
    }
    {   // ids 0 and hi − lo + 1 are refused and out is untouched; hi − lo itself passes
        for (int rec = 0; rec < 5; ++rec)
            for (int field = 0; field < 2; ++field)
                for (uint64_t bad : {uint64_t(0), uint64_t(11)}) {
                    std::vector<ks_delta> d = stream();
                    const bool arc = rec >= 3;
                    uint64_t& f = arc ? (field ? d[rec].dst : d[rec].src) : d[rec].id;
                    f = bad;
                    std::vector<ks_delta> out(d.size());
                    std::memset(out.data(), 0x5a, out.size() * sizeof(ks_delta));
                    const std::vector<ks_delta> before = out;
                    CHECK(ks_batch_translate_deltas(100, 110, d.data(), d.size(), out.data()) == KS_E_RANGE);
                    CHECK(std::memcmp(out.data(), before.data(), out.size() * sizeof(ks_delta)) == 0);
                    f = 10;
                    CHECK(ks_batch_translate_deltas(100, 110, d.data(), d.size(), out.data()) == KS_OK);
                }
    }
    {   // out == in; a refused in-place call leaves the stream as it was
        std::vector<ks_delta> d = stream(), want(5);
        CHECK(ks_batch_translate_deltas(40, 50, d.data(), d.size(), want.data()) == KS_OK);
        CHECK(ks_batch_translate_deltas(40, 50, d.data(), d.size(), d.data()) == KS_OK);
        CHECK(std::memcmp(d.data(), want.data(), d.size() * sizeof(ks_delta)) == 0);
        std::vector<ks_delta> e = stream();
        e[3].dst = 11;
        const std::vector<ks_delta> keep = e;
        CHECK(ks_batch_translate_deltas(40, 50, e.data(), e.size(), e.data()) == KS_E_RANGE);
        CHECK(std::memcmp(e.data(), keep.data(), e.size() * sizeof(ks_delta)) == 0);
    }
    {   // empty stream, bad arguments
        CHECK(ks_batch_translate_deltas(5, 9, nullptr, 0, nullptr) == KS_OK);
        std::vector<ks_delta> d = stream();
        CHECK(ks_batch_translate_deltas(9, 5, d.data(), d.size(), d.data()) == KS_E_INVALID);
        CHECK(ks_batch_translate_deltas(0, 20, d.data(), d.size(), nullptr) == KS_E_INVALID);
    }
    std::printf(fails ? "batch layout: %d check(s) failed\n" : "batch layout: all checks passed\n", fails);
    return fails ? 1 : 0;
}
