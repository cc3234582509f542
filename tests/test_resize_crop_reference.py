"""CPU: the plain resize + crop reference (tests/resize_crop_reference.py) against ATen, bitwise, on every case of its table, so
that the reference the GPU kernels are held to and the library the project promises to match guard each other without a GPU.
Also: the three float-scale nearest cases really differ from exact integer division, and the kernel-form table against the
launcher's own rule (`hab_obs_resize_crop_form` is host code)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from resize_crop_reference import (AREA, CASES, DTYPES, FLOAT_SCALE_CASES, FORMS, NEAREST, make_input, nearest_index, plain_ref,
                                   reference, window_of)

DTYPE_CODE = {"u8": 0, "f32": 1, "i32": 2}  # HAB_DTYPE_*


def aten_ref(x, rh, rw, window, mode):
    """What the reference library computes: F.interpolate on the float NCHW view, the cast back, the slice.  x: numpy NHWC."""
    t = torch.tensor(np.asarray(x))
    y0, x0, oh, ow = window
    r = F.interpolate(t.permute(0, 3, 1, 2).float(), size=(rh, rw), mode="area" if mode == AREA else "nearest")
    return r.to(t.dtype).permute(0, 2, 3, 1)[:, y0:y0 + oh, x0:x0 + ow].contiguous()


@pytest.mark.parametrize("name", list(CASES))
def test_plain_reference_is_aten_bitwise(name):
    dtype, shape, (rh, rw), _, mode, _ = CASES[name]
    x = make_input(name)
    assert x.dtype == DTYPES[dtype] and x.shape == shape
    want = aten_ref(x, rh, rw, window_of(name), mode)
    got = torch.tensor(np.asarray(reference(name)))
    assert got.dtype == want.dtype and got.shape == want.shape == (shape[0], *window_of(name)[2:], shape[3])
    assert torch.equal(got, want), (name, int((got != want).sum()))


@pytest.mark.parametrize("name", FLOAT_SCALE_CASES)
def test_float_scale_cases_differ_from_integer_division(name):
    _, (n, h, w, c), (rh, rw), _, mode, _ = CASES[name]
    assert mode == NEAREST
    y0, x0, oh, ow = window_of(name)
    rows, cols = nearest_index(h, rh, y0, oh), nearest_index(w, rw, x0, ow)
    rows_int, cols_int = np.arange(y0, y0 + oh) * h // rh, np.arange(x0, x0 + ow) * w // rw
    assert (rows != rows_int).any() or (cols != cols_int).any(), name
    # and on the seeded input the two rules give different images
    x = make_input(name)
    assert not np.array_equal(reference(name), x[:, rows_int[:, None], cols_int[None, :], :]), name


def test_area_reference_on_a_hand_computed_window():
    """3 x 5 -> 2 x 2: windows rows [0,2) [1,3), columns [0,3) [2,5); the sum order shows in fp32 with one large element."""
    x = np.array([[1e8, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 3]], dtype=np.float32).reshape(1, 3, 5, 1)
    got = plain_ref(x, 2, 2, (0, 0, 2, 2), AREA).reshape(2, 2)
    s = np.float32(1e8)
    for _ in range(5):
        s = np.float32(s + np.float32(1))  # 1e8 + 1 rounds back to 1e8: the row-major order loses every later 1
    assert s == np.float32(1e8)
    assert got[0, 0] == np.float32(np.float32(s / np.float32(2)) / np.float32(3))
    assert got[1, 1] == np.float32(np.float32(np.float32(8) / np.float32(2)) / np.float32(3))
    assert got[0, 1] == 1 and got[1, 0] == 1
    u = (np.arange(15, dtype=np.uint8) * 17).reshape(1, 3, 5, 1)
    assert plain_ref(u, 2, 2, (1, 1, 1, 1), AREA).item() == int(np.float32(np.float32(np.float32(1071) / np.float32(2)) / np.float32(3)))


def test_form_table_is_the_launcher_rule():
    """Host only: the query launches nothing and does not read `src`.  A 4-byte aligned buffer stands in for the device tensor."""
    from habitat_amd import _lib
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.uint32)
    p = buf.ctypes.data
    assert p % 4 == 0

    def form(name, ptr=p):
        dtype, (n, h, w, c), (rh, rw), _, mode, _ = CASES[name]
        return L.hab_obs_resize_crop_form(C.c_void_p(ptr), DTYPE_CODE[dtype], n, h, w, c, rh, rw, mode)
    got = {name: form(name) for name in CASES}
    assert got == {name: FORMS[v[5]] for name, v in CASES.items()}
    # a source that does not start on a dword: neither the packed rgb nor the tile kernel
    assert all(form(name, p + 1) == FORMS["generic"] for name in CASES)
    q = L.hab_obs_resize_crop_form
    assert q(C.c_void_p(p), 0, 2, 8, 8, 5, 4, 4, AREA) == -2 and q(C.c_void_p(p), 0, 2, 8, 8, 5, 4, 4, NEAREST) == -2  # C > 4
    assert q(C.c_void_p(p), 0, 2, 8, 8, 3, 4, 4, 2) == -1 and q(None, 0, 2, 8, 8, 3, 4, 4, AREA) == -1
    assert q(C.c_void_p(p), 0, 0, 8, 8, 3, 4, 4, AREA) == -1 and q(C.c_void_p(p), 0, 2, 8, 8, 3, 0, 4, AREA) == -1
    assert q(C.c_void_p(p), 7, 2, 8, 8, 3, 4, 4, AREA) == -2
