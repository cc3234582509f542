// TEST INFRASTRUCTURE ONLY -- the static item split of the persistent strip kernels (csrc/bf3_split.h: xcd_item_run is
// `__host__ __device__`), run on the host exactly as the device runs it.  Compiled by tests/test_xcd_item_run.py; never loaded by
// the product package.
#include "../../habitat-lab_amd/csrc/bf3_split.h"

extern "C" void hc_xcd_item_run(int items, int block, int grid, int* first, int* last) {
    hab::xcd_item_run(items, block, grid, *first, *last);
}
