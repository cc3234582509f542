"""Plain restatement of the fused resize + crop (`hab_obs_resize_crop`), shared by tests/test_resize_crop_reference.py (CPU: pinned
to ATen) and tests/test_gpu_resize_crop.py (GPU: the three kernel forms pinned to it, bitwise).  numpy only.

`area_ref` is F.interpolate(mode="area") = adaptive_avg_pool2d on the float NCHW view, the cast back and the slice: integer window
bounds, an fp32 sum taken one element after the other in row-major window order from +0, `sum / kh / kw` with both quotients
rounded to fp32, truncation to the sensor dtype.  `nearest_ref` is upsample_nearest's fp32 scale rule and a gather.

`CASES` is the table of shapes at which the launcher takes each of its kernels and each of their edges (window width 4 of the packed
rgb kernel; the tile kernel for 1-byte types, ragged tiles, unaligned crops, 3 / 4 float channels, wide fp32 windows, int32, the
LDS refusal; the generic kernel at odd pitches and 2 channels; nearest at sizes where the fp32 scale differs from exact integer
division; both grid-stride caps).  `form` is the kernel the launcher's rule gives for the shape."""
import functools

import numpy as np

AREA, NEAREST = 0, 1
FORMS = {"generic": 0, "tile": 1, "rgb8": 2}
DTYPES = {"u8": np.uint8, "f32": np.float32, "i32": np.int32}

# name -> (dtype, (N, H, W, C), (resized_h, resized_w), window (y0, x0, oh, ow) or None = the whole resized image, mode, form)
CASES = {
    "rgb8_kw4": ("u8", (2, 30, 52, 3), (12, 21), None, AREA, "rgb8"),
    "rgb8_kw4_crop": ("u8", (3, 31, 52, 3), (13, 21), (2, 3, 9, 15), AREA, "rgb8"),
    "u8c3_tile_4x": ("u8", (2, 48, 64, 3), (12, 16), None, AREA, "tile"),
    "u8c3_tile_ragged": ("u8", (3, 50, 68, 3), (13, 18), (1, 2, 11, 13), AREA, "tile"),
    "u8c3_tile_multi": ("u8", (2, 150, 212, 3), (37, 53), (3, 5, 30, 41), AREA, "tile"),
    "u8c4_tile": ("u8", (2, 40, 52, 4), (17, 23), (1, 1, 15, 20), AREA, "tile"),
    "u8c1_tile": ("u8", (2, 40, 52, 1), (17, 23), None, AREA, "tile"),
    "u8c1_generic": ("u8", (2, 40, 53, 1), (17, 23), None, AREA, "generic"),
    "u8c2_generic": ("u8", (2, 40, 52, 2), (17, 23), None, AREA, "generic"),
    "u8c3_oddpitch": ("u8", (1, 37, 53, 3), (12, 17), None, AREA, "generic"),
    "f32c1_tile_4x": ("f32", (3, 95, 131, 1), (22, 30), (1, 2, 19, 27), AREA, "tile"),
    "f32c1_tile_multi": ("f32", (2, 150, 260, 1), (37, 65), (2, 3, 33, 60), AREA, "tile"),
    "f32c3_tile": ("f32", (2, 61, 83, 3), (19, 26), None, AREA, "tile"),
    "f32c4_tile": ("f32", (2, 61, 83, 4), (19, 26), (3, 4, 11, 20), AREA, "tile"),
    "f32c1_up": ("f32", (2, 19, 23, 1), (41, 50), (5, 6, 30, 40), AREA, "tile"),
    "f32c4_lds_overflow": ("f32", (1, 160, 160, 4), (16, 16), None, AREA, "generic"),
    "f32c2_generic": ("f32", (2, 33, 47, 2), (9, 13), None, AREA, "generic"),
    "i32c1_area": ("i32", (2, 40, 52, 1), (17, 23), (1, 1, 15, 20), AREA, "tile"),
    "rgb8_stride_cap": ("u8", (1, 64, 64, 3), (4100, 4100), None, AREA, "rgb8"),
    "near_u8c3": ("u8", (2, 37, 53, 3), (20, 29), (1, 2, 18, 25), NEAREST, "generic"),
    "near_f32_2x": ("f32", (2, 17, 23, 1), (34, 40), None, NEAREST, "generic"),
    "near_scale_down": ("i32", (2, 26, 39, 1), (22, 33), None, NEAREST, "generic"),
    "near_scale_up": ("u8", (2, 14, 21, 3), (46, 69), None, NEAREST, "generic"),
    "near_scale_mixed": ("i32", (1, 52, 39, 1), (44, 66), (1, 2, 40, 60), NEAREST, "generic"),
    "near_stride_cap": ("i32", (17, 128, 128, 1), (512, 512), None, NEAREST, "generic"),
}
AREA_CASES = [k for k, v in CASES.items() if v[4] == AREA]
NEAREST_CASES = [k for k, v in CASES.items() if v[4] == NEAREST]
FLOAT_SCALE_CASES = ("near_scale_down", "near_scale_up", "near_scale_mixed")  # the fp32 scale rule differs from dst * in // out
SLOW_REFERENCE = ("rgb8_stride_cap",)  # seconds of plain numpy: the GPU tests take ATen's CPU result for it


def window_of(name):
    _, _, (rh, rw), window, _, _ = CASES[name]
    return tuple(window) if window is not None else (0, 0, rh, rw)


def random_input(dtype, shape, seed):
    """uint8 uniform in 0..255, int32 uniform in 0..2^20, float32 uniform in [0, 10)."""
    rng = np.random.default_rng(seed)
    if dtype == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if dtype == "i32":
        return rng.integers(0, 1 << 20, shape, dtype=np.int32)
    v = rng.random(shape, dtype=np.float32) * np.float32(10)
    return np.minimum(v, np.nextafter(np.float32(10), np.float32(0)))


@functools.lru_cache(maxsize=None)
def make_input(name):
    """The seeded source (N, H, W, C) of a case; read-only, shared."""
    x = random_input(CASES[name][0], CASES[name][1], seed=1000 + list(CASES).index(name))
    x.setflags(write=False)
    return x


def area_windows(n_in, n_out, lo, cnt):
    """adaptive_avg_pool2d: output index i in [lo, lo + cnt) covers [floor(i * in / out), ceil((i + 1) * in / out)) -> (start, length)."""
    i = np.arange(lo, lo + cnt, dtype=np.int64)
    start = (i * n_in) // n_out
    end = -((-(i + 1) * n_in) // n_out)
    return start, end - start


def area_ref(x, rh, rw, window):
    n, h, w, c = x.shape
    y0, x0, oh, ow = window
    ys, kh = area_windows(h, rh, y0, oh)
    xs, kw = area_windows(w, rw, x0, ow)
    acc = np.zeros((n, oh, ow, c), dtype=np.float32)
    for dy in range(int(kh.max())):
        rows = np.minimum(ys + dy, h - 1)
        for dx in range(int(kw.max())):
            cols = np.minimum(xs + dx, w - 1)
            v = x[:, rows[:, None], cols[None, :], :].astype(np.float32)
            inside = ((dy < kh)[:, None] & (dx < kw)[None, :])[None, :, :, None]
            acc = np.where(inside, acc + v, acc)  # fp32 add, one window element after the other
    q = acc / kh.astype(np.float32)[None, :, None, None]
    q = q / kw.astype(np.float32)[None, None, :, None]
    assert q.dtype == np.float32
    return q.astype(x.dtype)  # non-negative and in range: truncation


def nearest_index(n_in, n_out, lo, cnt):
    """min(int(floor(fp32(dst) * (fp32(in) / fp32(out)))), in - 1), every step rounded to fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(lo, lo + cnt).astype(np.float32)
    prod = dst * scale
    assert prod.dtype == np.float32
    return np.minimum(np.floor(prod).astype(np.int64), n_in - 1)


def nearest_ref(x, rh, rw, window):
    n, h, w, c = x.shape
    y0, x0, oh, ow = window
    rows, cols = nearest_index(h, rh, y0, oh), nearest_index(w, rw, x0, ow)
    return np.ascontiguousarray(x[:, rows[:, None], cols[None, :], :])


def plain_ref(x, rh, rw, window, mode):
    return area_ref(x, rh, rw, window) if mode == AREA else nearest_ref(x, rh, rw, window)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The plain reference of a case, computed once; read-only, shared."""
    _, _, (rh, rw), _, mode, _ = CASES[name]
    out = plain_ref(make_input(name), rh, rw, window_of(name), mode)
    out.setflags(write=False)
    return out
