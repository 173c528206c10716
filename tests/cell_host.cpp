// TEST INFRASTRUCTURE: ks_cell.h compiled for the host (tests/test_cell_shapes_cpu.py),
// so the test-side restatement of cell_class is compared with the function itself.
#include "../ksched_amd/csrc/ks_cell.h"

extern "C" {
void cell_classes(const int* cap, int* out, int n) {
    for (int i = 0; i < n; ++i) out[i] = ks::cell_class(cap[i]);
}
int cell_max_pos() { return ks::CELL_MAX_POS; }
int cell_ncls() { return ks::CELL_NCLS; }
int cell_threads() { return ks::CELL_THREADS; }
}
