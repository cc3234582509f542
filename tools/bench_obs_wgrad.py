#!/usr/bin/env python3
"""conv1's weight gradient at the C2 minibatch shape (2048 frames of 256x256 RGB-D), the im2col form (mask MP_OBS, obs_wgrad_bf3.h)
against the strip form (default mask, obs_wgrad_strip.h) in one process: HIP-event time per call (kernel + split-K pass), the form
that ran, and whether dw / db are bitwise equal.  Also the target of the `rocprofv3 --pmc` passes of profiles/r17_conv1_wgrad_sq_counters.txt.
usage: python tools/bench_obs_wgrad.py [frames] [rounds]"""
import ctypes as C, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd import _lib
L = _lib.lib()
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
H = W = 256
torch.manual_seed(0)
rgb = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda")
depth = torch.rand(B, H, W, 1, device="cuda")
dy = torch.randn(B, 63, 63, 32, device="cuda")
ws = torch.empty(1 << 24, device="cuda")
default = L.hab_set_matrix_path(-1)
def run(mask, n):
    L.hab_set_matrix_path(mask)
    dw = torch.empty(32, 4, 8, 8, device="cuda"); db = torch.empty(32, device="cuda")
    args = (P(rgb), P(depth), None, P(dy), P(dw), P(db), B, H, W, 32, 8, 8, 4, 0, P(ws), ws.numel())
    form = L.hab_obs_conv2d_wgrad_form(*args)
    _lib.check(L.hab_obs_conv2d_wgrad(*args, S()))
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        _lib.check(L.hab_obs_conv2d_wgrad(*args, S()))
    b.record(); torch.cuda.synchronize()
    return form, a.elapsed_time(b) / n * 1e3, dw, db
for r in range(rounds):
    f1, t1, dw1, db1 = run(2, 10)
    f2, t2, dw2, db2 = run(default, 10)
    print(f"round {r}: im2col form {f1}: {t1:8.1f} us   strip form {f2}: {t2:8.1f} us   equal {torch.equal(dw1, dw2) and torch.equal(db1, db2)}", flush=True)
L.hab_set_matrix_path(default)
