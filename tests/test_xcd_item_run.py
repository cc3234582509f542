"""CPU: xcd_item_run (csrc/bf3_split.h), the static split of a persistent grid's items over XCDs and workgroups, run on the host.

The split decides which strips a workgroup of the strip kernels works on and, under the sign schedule, which of them negate their
sum; no GPU test looks at it directly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostcheck_items") / "libhab_hostcheck_items.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(HERE, "hostcheck_items", "xcd_item_run.hip"), "-o", so])
    return C.CDLL(so)


def test_xcd_item_run_partitions_the_items(hc):
    """Over the blocks of a persistent grid the runs [first, last) are disjoint and cover every item once, block b's run lies inside
    the eighth of XCD b & 7, the runs of an XCD follow each other in block order, and every run equals the expressions the four strip
    kernels carried before the split was shared."""
    first, last = C.c_int(), C.c_int()
    for items in (0, 1, 7, 8, 9, 63, 64, 65, 1000, 30720):
        for grid in range(8, 257, 8):
            per_xcd = (items + 7) >> 3
            seen = np.zeros(items, dtype=np.int32)
            end_of = [x * per_xcd for x in range(8)]  # where the previous block of the XCD stopped
            for b in range(grid):
                hc.hc_xcd_item_run(items, b, grid, C.byref(first), C.byref(last))
                f, l = first.value, last.value
                # the kernels' own four lines, restated
                xcd, jw, wg_per_xcd = b & 7, b >> 3, grid >> 3
                per_wg = (per_xcd + wg_per_xcd - 1) // wg_per_xcd
                xcd_end = min(items, (xcd + 1) * per_xcd)
                ref_first = min(xcd_end, xcd * per_xcd + jw * per_wg)
                assert (f, l) == (ref_first, min(xcd_end, ref_first + per_wg)), (items, grid, b)
                assert f <= l, (items, grid, b)
                if f < l:
                    assert xcd * per_xcd <= f and l <= xcd_end, (items, grid, b)
                    assert f == end_of[xcd], (items, grid, b)  # block order inside the XCD, no gap
                    end_of[xcd] = l
                    seen[f:l] += 1
            assert (seen == 1).all(), (items, grid)
