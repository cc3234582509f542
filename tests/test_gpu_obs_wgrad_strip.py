"""conv1's weight gradient with the observation rows resident in LDS (csrc/obs_wgrad_strip.h, mask MP_OBS | MP_OBS_PATCH) against the
im2col form it replaces (csrc/obs_wgrad_bf3.h, mask MP_OBS): `dw` and `db` bitwise equal for the same arguments and workspace, the
float64 bar of tests/test_gpu_bf3.py::test_obs_wgrad_bf3_as_accurate_as_fp32_path, and the form that ran asserted through
`hab_obs_conv2d_wgrad_form` (host code, the launcher's own rule) so that a silent fallback cannot pass the comparison.

The shapes are the smallest at which the staging can go wrong (the bf16 path needs more than 4096 output pixels):
  ring    84x84, 52 frames: 1040 tiles over 512 workgroups, 3 each, 20 output rows per frame -- runs begin inside a frame and cross
          frame boundaries: reload of all 8 rows, reuse of 4
  bench   256x256, 25 frames: 1575 tiles, 4 per workgroup, 63 rows per frame; Wo = 63, one padded pixel per tile
  wide    64x320: Wo = 79, two 64-pixel blocks per output row on the same input rows, the second 15 pixels wide
  narrow  128x40 with Cout = 16: Wo = 9, most k-groups empty, half the dY columns absent
  rows    `ring` through a frame -> arena-row indirection that permutes the frames and repeats one
  cout36 / stride8  shapes the new form refuses: Cout = 36 runs the igemm tiles, 8x8 / stride 8 the im2col form, under either mask"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from habitat_amd import _lib  # noqa: E402

MP_OBS, MP_OBS_PATCH = 1 << 1, 1 << 6
IGEMM, IM2COL, STRIP = 0, 1, 2  # HAB_OBS_WGRAD_FORM_*

# name -> (B, H, W, Cout, stride, rows indirection, forms under (0, MP_OBS, MP_OBS | MP_OBS_PATCH))
CASES = {
    "ring": (52, 84, 84, 32, 4, False, (IGEMM, IM2COL, STRIP)),
    "bench": (25, 256, 256, 32, 4, False, (IGEMM, IM2COL, STRIP)),
    "wide": (8, 64, 320, 32, 4, False, (IGEMM, IM2COL, STRIP)),
    "narrow": (16, 128, 40, 16, 4, False, (IGEMM, IM2COL, STRIP)),
    "rows": (52, 84, 84, 32, 4, True, (IGEMM, IM2COL, STRIP)),
    "cout36": (52, 84, 84, 36, 4, False, (IGEMM, IGEMM, IGEMM)),
    "stride8": (40, 96, 96, 32, 8, False, (IGEMM, IM2COL, IM2COL)),
}

_KEEP = []


def P(t):
    if t is None:
        return None
    _KEEP.append(t)
    if len(_KEEP) > 64:
        del _KEEP[:32]
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("name", list(CASES))
def test_strip_form_bitwise_equal_to_im2col_form(name):
    B, H, W, Cout, stride, indirect, forms = CASES[name]
    L = _lib.lib()
    torch.manual_seed(11)
    Ho, Wo = (H - 8) // stride + 1, (W - 8) // stride + 1
    assert B * Ho * Wo > 4096
    nrows = B + 2 if indirect else B
    rgb = torch.randint(0, 256, (nrows, H, W, 3), dtype=torch.uint8)
    depth = torch.rand(nrows, H, W, 1)
    rows = None
    if indirect:
        rows = torch.randperm(nrows)[:B]
        rows[B // 2] = rows[3]  # one arena row serves two frames
    sel = rows if indirect else slice(None)
    x = torch.cat([rgb[sel].double() / 255.0, depth[sel].double()], -1).permute(0, 3, 1, 2)
    dy = torch.randn(B, Ho, Wo, Cout) * torch.rand(B, Ho, Wo, Cout).pow(3)
    w = torch.zeros(Cout, 4, 8, 8, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, stride=stride).backward(dy.double().permute(0, 3, 1, 2))
    ref = torch.cat([w.grad.flatten(), dy.double().sum((0, 1, 2))])

    rg, dp, dyd = rgb.cuda(), depth.cuda(), dy.cuda()
    rw = rows.int().cuda() if indirect else None
    ws = torch.zeros(1 << 23, device="cuda")  # the same workspace for every form: the same partition into slabs
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out, ran = {}, {}
    prev = L.hab_set_matrix_path(-1)
    try:
        for mask in (0, MP_OBS, MP_OBS | MP_OBS_PATCH):
            L.hab_set_matrix_path(mask)
            dw = torch.full((Cout, 4, 8, 8), 3.0, device="cuda")
            db = torch.full((Cout,), 3.0, device="cuda")
            args = (P(rg), P(dp), P(rw), P(dyd), P(dw), P(db), B, H, W, Cout, 8, 8, stride, 0, P(ws), ws.numel())
            ran[mask] = L.hab_obs_conv2d_wgrad_form(*args)
            _lib.check(L.hab_obs_conv2d_wgrad(*args, stream))
            out[mask] = (dw, db)
    finally:
        L.hab_set_matrix_path(prev)
    torch.cuda.synchronize()

    assert tuple(ran[m] for m in (0, MP_OBS, MP_OBS | MP_OBS_PATCH)) == forms, (name, ran)
    (dw1, db1), (dw2, db2) = out[MP_OBS], out[MP_OBS | MP_OBS_PATCH]
    ndw, ndb = int((dw1 != dw2).sum()), int((db1 != db2).sum())
    print(name, "differing dw / db elements:", ndw, ndb)
    assert torch.equal(dw1, dw2), (name, ndw, (dw1 - dw2).abs().max().item())
    assert torch.equal(db1, db2), (name, ndb)

    def err(pair):
        y = torch.cat([pair[0].flatten(), pair[1]]).double().cpu()
        return ((y - ref).abs().max() / ref.abs().max()).item()

    e0, e1 = err(out[0]), err(out[MP_OBS | MP_OBS_PATCH])
    print(name, "error vs float64: fp32 path %.3g, new form %.3g" % (e0, e1))
    assert e1 <= 2 * e0 + 2e-7, (name, e0, e1)
    assert e1 < 3e-6, (name, e1)
