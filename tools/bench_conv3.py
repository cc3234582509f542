#!/usr/bin/env python3
"""conv3 (3x3/1 64->32 at 30x30) and ResNet layer1 (3x3/1/1 32->32 at 32x32) forward / data gradient at rollout and learner batch sizes
(development aid).  usage: python tools/bench_conv3.py"""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd import _lib  # noqa: E402

L = _lib.lib()
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


ws = torch.empty(1 << 26, device="cuda")
for name, H, Cc, Cout, pad in (("conv3 64>32 @30", 30, 64, 32, 0), ("layer1 32>32 @32", 32, 32, 32, 1)):
    for B in (64, 512, 1024):
        Ho = H + 2 * pad - 2
        x = torch.randn(B, H, H, Cc, device="cuda")
        wf = torch.randn(Cout, 3, 3, Cc, device="cuda") * 0.05
        wd = torch.randn(Cc, 3, 3, Cout, device="cuda") * 0.05
        b = torch.zeros(Cout, device="cuda")
        y = torch.empty(B, Ho, Ho, Cout, device="cuda")
        dx = torch.empty(B, H, H, Cc, device="cuda")
        fl = 2.0 * B * Ho * Ho * Cout * 9 * Cc
        t = timeit(lambda: _lib.check(L.hab_conv2d_fwd(P(x), P(wf), P(b), P(y), B, H, H, Cc, Cout, 3, 3, 1, pad, 1, P(ws), ws.numel(), S())))
        ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), wf.permute(0, 3, 1, 2).double(), padding=pad).relu().permute(0, 2, 3, 1)
        err = float((y.double() - ref).abs().max() / ref.abs().max())
        line = f"{name:18s} B {B:5d} fwd {t * 1e3:8.1f} us {fl / t / 1e9:7.1f} TF/s  rel err {err:.1e}"
        if Cc == Cout:
            t = timeit(lambda: _lib.check(L.hab_conv2d_dgrad(P(y), P(wd), None, None, P(dx), B, H, H, Cc, Cout, 3, 3, 1, pad, P(ws), ws.numel(), S())))
            line += f" | dgrad {t * 1e3:8.1f} us {fl / t / 1e9:7.1f} TF/s"
        print(line, flush=True)

# conv3's data gradient (dX 30x30x64 <- dY 28x28x32, ReLU mask fused) with and without the strip kernel (matrix-path bit 9)
FORMS = {0: "general", 1: "conv2 strip", 2: "conv3 strip"}
prev = L.hab_set_matrix_path(-1)
for B in (64, 512, 1024):
    dy = torch.randn(B, 28, 28, 32, device="cuda")
    wd = torch.randn(64, 3, 3, 32, device="cuda") * 0.05
    mask = torch.randn(B, 30, 30, 64, device="cuda")
    dx = torch.empty(B, 30, 30, 64, device="cuda")
    fl = 2.0 * B * 28 * 28 * 32 * 9 * 64
    ref = torch.nn.functional.conv_transpose2d(dy.permute(0, 3, 1, 2).double(), wd.permute(3, 0, 1, 2).double()).permute(0, 2, 3, 1) * (mask > 0)
    for mode in (prev & ~512, prev | 513):
        L.hab_set_matrix_path(mode)
        args = (P(dy), P(wd), P(mask), None, P(dx), B, 30, 30, 64, 32, 3, 3, 1, 0, P(ws), ws.numel())
        form = L.hab_conv2d_dgrad_form(*args)
        t = timeit(lambda: _lib.check(L.hab_conv2d_dgrad(*args, S())))
        err = float((dx.double() - ref).abs().max() / ref.abs().max())
        print(f"conv3 dgrad 32>64 @30 B {B:5d} mask {mode:5d} {FORMS[form]:12s} {t * 1e3:8.1f} us {fl / t / 1e9:7.1f} TF/s  rel err {err:.1e}", flush=True)
L.hab_set_matrix_path(prev)
