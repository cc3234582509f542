"""GPU: SimpleCNN conv3's data gradient on the strip kernel (csrc/conv3_dgrad_strip.h, matrix-path bit 9 with bit 0) against a float64
conv2d backward and against the general kernels that the same call runs without bit 9 (bitwise where those run without split-K: the
strip kernel repeats their accumulation chain and sign schedule).  The form is asserted through
hab_conv2d_dgrad_form under both masks, so a silent fall-back cannot pass."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from habitat_amd import _lib  # noqa: E402

FULL, NO_STRIP = 2047, 2047 & ~512
GENERAL, CONV3_STRIP = 0, 2


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def err_vs(ref64, y):  # the norm-wise error of tests/test_gpu_bf3.py
    ref = ref64.double()
    return ((y.double().cpu() - ref).abs().max() / ref.abs().max()).item()


class Problem:
    """One data-gradient call: heavy-tailed dY, float64 reference computed once."""

    def __init__(self, B, H, W, Cc=64, Cout=32, pad=0, mask=True, add=False, seed=8):
        torch.manual_seed(seed)
        self.B, self.H, self.W, self.Cc, self.Cout, self.pad = B, H, W, Cc, Cout, pad
        Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
        dy = torch.randn(B, Cout, Ho, Wo) * torch.rand(B, Cout, Ho, Wo).pow(3) * 20
        w = torch.randn(Cout, Cc, 3, 3) / np.sqrt(Cc * 9)
        x = torch.zeros(B, Cc, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w.double(), None, stride=1, padding=pad).backward(dy.double())
        ref = x.grad.permute(0, 2, 3, 1)
        m = torch.randn(B, H, W, Cc) if mask else None
        a = torch.randn(B, H, W, Cc) if add else None
        if a is not None:
            ref = ref + a.double()
        if m is not None:
            ref = ref * (m > 0)
        self.ref = ref
        self.mask_cpu = m
        self.dy = dy.permute(0, 2, 3, 1).contiguous().cuda()
        self.wd = w.permute(1, 2, 3, 0).contiguous().cuda()
        self.mask = m.cuda() if m is not None else None
        self.add = a.cuda() if a is not None else None
        self.ws = torch.zeros(1 << 22, device="cuda")

    def args(self, dx):
        return (P(self.dy), P(self.wd), P(self.mask), P(self.add), P(dx), self.B, self.H, self.W, self.Cc, self.Cout, 3, 3, 1, self.pad,
                P(self.ws), self.ws.numel())

    def run(self, L, mode):
        """(form, dX) under matrix-path mask `mode`; dX is pre-filled with NaN sentinels."""
        prev = L.hab_set_matrix_path(-1)
        try:
            L.hab_set_matrix_path(mode)
            dx = torch.full((self.B, self.H, self.W, self.Cc), float("nan"), device="cuda")
            form = L.hab_conv2d_dgrad_form(*self.args(dx))
            _lib.check(L.hab_conv2d_dgrad(*self.args(dx), S()))
            torch.cuda.synchronize()
            return form, dx
        finally:
            L.hab_set_matrix_path(prev)


def check_against_reference(pr, dx0, dx_old, dx_new):
    e0, e_old, e_new = err_vs(pr.ref, dx0), err_vs(pr.ref, dx_old), err_vs(pr.ref, dx_new)
    diff = ((dx_new.double() - dx_old.double()).abs().max().cpu() / pr.ref.abs().max()).item()
    print(f"e(mode 0) {e0:.3e}  e_old {e_old:.3e}  e_new {e_new:.3e}  |new - old| {diff:.3e}  bitwise {torch.equal(dx_new, dx_old)}")
    for dx in (dx_old, dx_new):
        assert not torch.isnan(dx).any(), "a sentinel was not overwritten"
        if pr.mask_cpu is not None:
            assert (dx.cpu()[pr.mask_cpu <= 0] == 0).all()
    assert e_new <= 2 * e0 + 2e-7, (e0, e_new)
    assert e_new < 3e-6
    assert e_old <= 2 * e0 + 2e-7, (e0, e_old)
    assert diff <= e_new + e_old, (diff, e_new, e_old)


CASES = {
    "bench": dict(B=16, H=30, W=30),               # compile-time geometry; 80 items, fewer than workgroups
    "many": dict(B=60, H=30, W=30),                # 300 items: some workgroups take two (prefetch across items and a frame boundary)
    "ragged": dict(B=20, H=21, W=19),              # runtime geometry; last strip partial; W < 30
    "tiny": dict(B=16, H=3, W=3),                  # dY 1 x 1: every tap but one falls on the zero border
    "wide32": dict(B=16, H=8, W=32),               # the full 32-pixel tile; right border columns
    "nomask": dict(B=16, H=30, W=30, mask=False),  # the path without a mask
}


@pytest.mark.parametrize("name", list(CASES))
def test_conv3_dgrad_strip_as_accurate_as_fp32_path(L, name):
    pr = Problem(**CASES[name])
    _, dx0 = pr.run(L, 0)
    f_old, dx_old = pr.run(L, NO_STRIP)
    f_new, dx_new = pr.run(L, FULL)
    assert (f_old, f_new) == (GENERAL, CONV3_STRIP)
    check_against_reference(pr, dx0, dx_old, dx_new)
    if name == "many":  # 54 000 pixels = 422 tiles: the general form runs without split-K there, and the strip kernel repeats its chain
        assert torch.equal(dx_new, dx_old), "not bitwise equal to the unsplit general form"
    f_again, dx_again = pr.run(L, FULL)
    assert f_again == CONV3_STRIP and torch.equal(dx_again, dx_new), "two runs of the strip kernel differ"


REFUSALS = {
    "add": dict(B=16, H=30, W=30, add=True),
    "c32": dict(B=16, H=30, W=30, Cc=32, Cout=32),
    "pad1": dict(B=16, H=30, W=30, pad=1),
    "w33": dict(B=16, H=8, W=33),
    "b8": dict(B=8, H=30, W=30),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_calls_the_strip_kernel_does_not_serve_keep_the_general_form(L, name):
    pr = Problem(**REFUSALS[name])
    _, dx0 = pr.run(L, 0)
    f_old, dx_old = pr.run(L, NO_STRIP)
    f_new, dx_new = pr.run(L, FULL)
    assert (f_old, f_new) == (GENERAL, GENERAL)
    check_against_reference(pr, dx0, dx_old, dx_new)
