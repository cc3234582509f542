"""GPU: the folded form of SimpleCNN conv2's strip kernels (csrc/conv2_fwd_strip.h, csrc/conv2_dgrad_strip.h: a tile's sums, epilogue
and stores inside the next tile's MFMA interval) against their plain form (matrix-path bit 14) bit for bit, and against a float64
conv2d forward / backward under the bar of tests/test_gpu_bf3.py.  The forms are asserted through hab_conv2d_fwd_form /
hab_conv2d_dgrad_form, so a silent fall-back cannot pass; the outputs are pre-filled with NaN, so a tile that is never folded, or
folded with another tile's base or extent, shows."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from habitat_amd import _lib  # noqa: E402

FULL, PLAIN = 2047, 2047 | 1 << 14
FWD_GENERAL, FWD_STRIP, FWD_STRIP_PLAIN = 0, 1, 2
DGRAD_GENERAL, DGRAD_STRIP, DGRAD_STRIP_PLAIN = 0, 1, 3

# (B, H, W): 63 x 63 is the compile-time geometry, everything else the runtime one.  Strips per frame: 15 forward / 16 backward at 63.
SHAPES = {
    "one_strip_per_run": (16, 63, 63),   # 240 / 256 strips on 256 workgroups: the prologue's stage and the final fold alone
    "runs_cross_frames": (40, 63, 63),   # runs of two or three strips that cross a frame
    "short_last_strip": (16, 20, 20),    # forward Ho = 9: the last strip holds one row, the pending tile's extent differs from its successor's
    "one_pixel": (19, 4, 5),             # one output pixel, one tile per strip
    "rt_20x31": (17, 20, 31),            # non-square runtime geometry
    "rt_33x14": (16, 33, 14),
}


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def err_vs(ref64, y):  # the norm-wise error of tests/test_gpu_bf3.py
    return ((y.double().cpu() - ref64).abs().max() / ref64.abs().max()).item()


def under(L, mode, fn):
    prev = L.hab_set_matrix_path(mode)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        L.hab_set_matrix_path(prev)


class Forward:
    """One forward call: heavy-tailed input, the float64 reference without bias / ReLU computed once."""

    def __init__(self, B, H, W):
        torch.manual_seed(12)
        self.B, self.H, self.W = B, H, W
        x = torch.randn(B, 32, H, W) * torch.rand(B, 32, H, W).pow(4) * 50
        w = torch.randn(64, 32, 4, 4) / np.sqrt(32 * 16)
        self.b = torch.randn(64)
        self.lin = F.conv2d(x.double(), w.double(), None, stride=2).permute(0, 2, 3, 1).contiguous()
        self.x = x.permute(0, 2, 3, 1).contiguous().cuda()
        self.wf = w.permute(0, 2, 3, 1).contiguous().cuda()  # [co][kh][kw][ci]
        self.bd = self.b.cuda()
        self.ws = torch.zeros(1 << 20, device="cuda")

    def ref(self, relu, bias):
        r = self.lin + self.b.double() if bias else self.lin
        return F.relu(r) if relu else r

    def run(self, L, mode, relu, bias):
        def go():
            y = torch.full(self.lin.shape, float("nan"), device="cuda")
            a = (P(self.x), P(self.wf), P(self.bd if bias else None), P(y), self.B, self.H, self.W, 32, 64, 4, 4, 2, 0, relu, P(self.ws),
                 self.ws.numel())
            form = L.hab_conv2d_fwd_form(*a)
            _lib.check(L.hab_conv2d_fwd(*a, S()))
            return form, y
        return under(L, mode, go)


class Dgrad:
    """One data-gradient call: heavy-tailed dY, the float64 reference without mask computed once."""

    def __init__(self, B, H, W):
        torch.manual_seed(13)
        self.B, self.H, self.W = B, H, W
        Ho, Wo = (H - 4) // 2 + 1, (W - 4) // 2 + 1
        w = torch.randn(64, 32, 4, 4) / np.sqrt(32 * 16)
        dy = torch.randn(B, 64, Ho, Wo) * torch.rand(B, 64, Ho, Wo).pow(3) * 20
        x = torch.zeros(B, 32, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w.double(), None, stride=2).backward(dy.double())
        self.lin = x.grad.permute(0, 2, 3, 1).contiguous()
        self.mask_cpu = torch.randn(B, H, W, 32)
        self.dy = dy.permute(0, 2, 3, 1).contiguous().cuda()
        self.wd = w.permute(1, 2, 3, 0).contiguous().cuda()  # [ci][kh][kw][co]
        self.mask = self.mask_cpu.cuda()
        self.ws = torch.zeros(1 << 20, device="cuda")

    def ref(self, mask):
        return self.lin * (self.mask_cpu > 0) if mask else self.lin

    def run(self, L, mode, mask):
        def go():
            dx = torch.full((self.B, self.H, self.W, 32), float("nan"), device="cuda")
            a = (P(self.dy), P(self.wd), P(self.mask if mask else None), None, P(dx), self.B, self.H, self.W, 32, 64, 4, 4, 2, 0, P(self.ws),
                 self.ws.numel())
            form = L.hab_conv2d_dgrad_form(*a)
            _lib.check(L.hab_conv2d_dgrad(*a, S()))
            return form, dx
        return under(L, mode, go)


def check(ref, y0, y_plain, y_fold, y_again):
    assert not torch.isnan(y_fold).any() and not torch.isnan(y_plain).any(), "a sentinel was not overwritten"
    assert torch.equal(y_fold, y_plain), "the folded and the plain form differ"
    assert torch.equal(y_fold, y_again), "two runs of the folded form differ"
    e0, e = err_vs(ref, y0), err_vs(ref, y_fold)
    print(f"e(mode 0) {e0:.3e}  e {e:.3e}")
    assert e <= 2 * e0 + 2e-7 and e < 3e-6, (e0, e)


@pytest.fixture(scope="module")
def fwd_problems():
    return {}


@pytest.fixture(scope="module")
def dgrad_problems():
    return {}


def cached(store, cls, name):
    if name not in store:
        store[name] = cls(*SHAPES[name])
    return store[name]


@pytest.mark.parametrize("relu,bias", [(1, True), (0, True), (1, False)], ids=["relu", "linear", "nobias"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_folded_equals_plain_and_is_as_accurate_as_fp32_path(L, fwd_problems, name, relu, bias):
    pr = cached(fwd_problems, Forward, name)
    _, y0 = pr.run(L, 0, relu, bias)
    f_plain, y_plain = pr.run(L, PLAIN, relu, bias)
    f_fold, y_fold = pr.run(L, FULL, relu, bias)
    f_again, y_again = pr.run(L, FULL, relu, bias)
    assert (f_plain, f_fold, f_again) == (FWD_STRIP_PLAIN, FWD_STRIP, FWD_STRIP)
    check(pr.ref(relu, bias), y0, y_plain, y_fold, y_again)


@pytest.mark.parametrize("mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_data_gradient_folded_equals_plain_and_is_as_accurate_as_fp32_path(L, dgrad_problems, name, mask):
    pr = cached(dgrad_problems, Dgrad, name)
    _, d0 = pr.run(L, 0, mask)
    f_plain, d_plain = pr.run(L, PLAIN, mask)
    f_fold, d_fold = pr.run(L, FULL, mask)
    f_again, d_again = pr.run(L, FULL, mask)
    assert (f_plain, f_fold, f_again) == (DGRAD_STRIP_PLAIN, DGRAD_STRIP, DGRAD_STRIP)
    check(pr.ref(mask), d0, d_plain, d_fold, d_again)
    if mask:
        assert (d_fold.cpu()[pr.mask_cpu <= 0] == 0).all()
    if (pr.H, pr.W) == (63, 63):  # the half-empty last cell row and cell column: h = 62 and w = 62 have no odd neighbour
        ref = pr.ref(mask)
        for sl in ((slice(None), 62), (slice(None), slice(None), 62)):
            d = (d_fold.double().cpu()[sl] - ref[sl]).abs().max().item()
            assert d <= 3e-6 * ref.abs().max().item(), d


def test_bits_8_and_9_alone_select_the_folded_form_and_eight_frames_the_general_one(L, fwd_problems, dgrad_problems):
    fw, dg = cached(fwd_problems, Forward, "one_strip_per_run"), cached(dgrad_problems, Dgrad, "one_strip_per_run")
    assert fw.run(L, 1 | 256, 1, True)[0] == FWD_STRIP
    assert fw.run(L, 1 | 256 | 1 << 14, 1, True)[0] == FWD_STRIP_PLAIN
    assert fw.run(L, 1 | 1 << 14, 1, True)[0] == FWD_GENERAL
    assert dg.run(L, 1 | 512, True)[0] == DGRAD_STRIP
    assert dg.run(L, 1 | 512 | 1 << 14, True)[0] == DGRAD_STRIP_PLAIN
    assert dg.run(L, 1 | 1 << 14, True)[0] == DGRAD_GENERAL
    fw8, dg8 = Forward(8, 20, 20), Dgrad(8, 20, 20)
    for mode in (FULL, PLAIN):
        f, y = fw8.run(L, mode, 1, True)
        assert f == FWD_GENERAL and err_vs(fw8.ref(1, True), y) < 3e-6
        f, d = dg8.run(L, mode, True)
        assert f == DGRAD_GENERAL and err_vs(dg8.ref(True), d) < 3e-6
