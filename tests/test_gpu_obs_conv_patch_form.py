"""The two forms of the patch-resident first convolution (csrc/obs_conv_patch.h): the one that runs -- tile-invariant load addressing
through a per-tile buffer descriptor, scalar tile decode, the sign schedule applied where the patch is written, the epilogue negating by
one XOR -- and the plain form behind the test-only matrix-path bit 13.  Both feed the same bf16 operands to the same MFMAs in the same
order, so their outputs must be BIT-identical at every shape at which one of those pieces can go wrong, and the form that runs must be
as accurate against float64 as the fp32 MFMA path (the bar of test_gpu_bf3.py's patch test)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from habitat_amd import _lib  # noqa: E402

DEFAULT, PLAIN = 2047, 2047 | 1 << 13
FORM_OTHER, FORM_PATCH, FORM_PATCH_PLAIN = 0, 1, 2  # HAB_OBS_FWD_FORM_*


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


_KEEP = []


def P(t):
    """Device pointer of a tensor for a ctypes call; the tensor stays alive for the next few dozen calls."""
    if t is None:
        return None
    _KEEP.append(t)
    if len(_KEEP) > 96:
        del _KEEP[:48]
    return C.c_void_p(t.data_ptr())


S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _with_path(L, mode, fn):
    prev = L.hab_set_matrix_path(-1)
    try:
        L.hab_set_matrix_path(mode)
        return fn()
    finally:
        L.hab_set_matrix_path(prev)


def err_vs(ref64, y):
    return ((y.double().cpu() - ref64).abs().max() / ref64.abs().max()).item()


@functools.lru_cache(maxsize=None)
def problem(B, H, W, Cout):
    """Inputs of one geometry and its float64 convolution without bias, [B][Ho][Wo][Cout]: computed once, shared, never written."""
    g = torch.Generator().manual_seed(1000 * B + H + W + Cout)
    rgb = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    depth = torch.rand(B, H, W, 1, generator=g) * torch.rand(B, H, W, 1, generator=g).pow(3)
    w = torch.randn(Cout, 4, 8, 8, generator=g) / 16
    b = torch.randn(Cout, generator=g)
    x = torch.cat([rgb.double() / 255.0, depth.double()], -1).permute(0, 3, 1, 2)
    pre = F.conv2d(x, w.double(), None, stride=4).permute(0, 2, 3, 1).contiguous()
    return dict(rgb=rgb.cuda(), depth=depth.cuda(), wf=w.permute(0, 2, 3, 1).contiguous().cuda(), b=b, bd=b.cuda(), pre=pre)


def run_forms(L, B, H, W, Cout=32, relu=1, bias=True, rows=None, arena=None):
    """Runs the call on the fp32 path, the form that runs and the plain form; asserts the reported forms, bitwise equality of the two
    forms (and of two runs of the first) and the float64 bar.  rows: frame -> arena row of an `arena`-frame observation set."""
    q = problem(arena or B, H, W, Cout)
    ref = q["pre"] if rows is None else q["pre"][torch.tensor(rows)]
    if bias:
        ref = ref + q["b"].double()
    if relu:
        ref = F.relu(ref)
    rows_d = None if rows is None else torch.tensor(rows, dtype=torch.int32).cuda()
    ws = torch.zeros(1 << 22, device="cuda")
    bd = q["bd"] if bias else None

    def args(y):
        return (P(q["rgb"]), P(q["depth"]), P(rows_d), P(q["wf"]), P(bd), P(y), B, H, W, Cout, 8, 8, 4, 0, relu, P(ws), ws.numel())

    def run():
        y = torch.full(ref.shape, -7.0, device="cuda")  # a pixel or channel quad the kernel leaves out keeps the sentinel
        _lib.check(L.hab_obs_conv2d_fwd(*args(y), S()))
        return y

    def form():
        return L.hab_obs_conv2d_fwd_form(*args(torch.empty(ref.shape, device="cuda")))

    assert _with_path(L, DEFAULT, form) == FORM_PATCH
    assert _with_path(L, PLAIN, form) == FORM_PATCH_PLAIN
    assert _with_path(L, 2 | 64, form) == FORM_PATCH
    y_f32, y_new, y_plain = _with_path(L, 0, run), _with_path(L, DEFAULT, run), _with_path(L, PLAIN, run)
    assert torch.equal(y_new, y_plain)
    assert torch.equal(y_new, _with_path(L, DEFAULT, run))
    e_f32, e = err_vs(ref, y_f32), err_vs(ref, y_new)
    print(f"B={B} H={H} W={W} Cout={Cout} relu={relu} bias={bias} rows={rows is not None}: e_f32={e_f32:.3e} e={e:.3e}")
    assert e <= 2 * e_f32 + 2e-7 and e < 3e-6, (e_f32, e)


@pytest.mark.parametrize("B,H,W", [
    (3, 96, 128),    # Wo = 31: second 32-pixel half empty; 640 units: slots 3, 4 partly / wholly off; Ho = 23: last tile reads rows past the image
    (5, 44, 44),     # 220 units (< one per thread); 3 tiles per image: the tile parity changes from image to image
    (2, 12, 256),    # full width, fewer output rows than a tile
    (3, 256, 256),   # benchmark geometry, one tile per group
    (40, 256, 256),  # ... 1-3 tiles per group, unequal tile counts of the two groups: next-tile prefetch, n_first / n_mine tails
])
def test_patch_forms_bitwise_equal_and_as_accurate_as_fp32_path(L, B, H, W):
    run_forms(L, B, H, W)


def test_patch_forms_through_rows_that_repeat_an_arena_row(L):
    run_forms(L, 7, 96, 128, rows=[3, 0, 3, 6, 1, 3, 5], arena=7)


@pytest.mark.parametrize("opts", [dict(relu=0), dict(bias=False), dict(Cout=20)], ids=["no_relu", "null_bias", "cout20"])
def test_patch_forms_epilogue_options(L, opts):
    """Without ReLU (the negated zeros of odd tiles reach the output), without bias, and with Cout = 20 (the n + 3 >= N quads)."""
    run_forms(L, 3, 96, 128, **opts)


def test_cout_36_is_not_a_patch_form_under_either_mask(L):
    q = problem(3, 96, 128, 36)
    y = torch.empty(3, 23, 31, 36, device="cuda")
    ws = torch.zeros(1 << 22, device="cuda")
    form = lambda: L.hab_obs_conv2d_fwd_form(P(q["rgb"]), P(q["depth"]), None, P(q["wf"]), P(q["bd"]), P(y), 3, 96, 128, 36, 8, 8, 4, 0, 1,
                                             P(ws), ws.numel())
    assert _with_path(L, DEFAULT, form) == FORM_OTHER
    assert _with_path(L, PLAIN, form) == FORM_OTHER
