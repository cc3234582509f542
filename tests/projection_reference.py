"""float64 restatement of the cube-map projection transformers (CubeMap2Equirect / CubeMap2Fisheye), shared by
tests/test_projection_host.py and tests/test_gpu_projection.py.

`grid_sample_reference` is the reference's own form: six grids (filled with 2.0, i.e. outside every face, where a face is not
assigned), F.grid_sample(bilinear, padding zeros, align_corners=True) on the float64 NCHW stack, a sum over the faces.
`four_tap_reference` is the single-face four-tap form that the kernel uses.  Both read the table the transformer built (fp32
coordinates, taken to float64 as they are), so what they pin is the sampling, and the tables themselves are pinned by the checks of
tests/test_projection_host.py."""
import functools

import torch
import torch.nn.functional as F

# name -> (face size, kind, (out_h, out_w), fov, params)
GEOMETRIES = {
    "A": (16, "equirect", (16, 32), None, None),
    "B": (9, "equirect", (13, 29), None, None),
    "C": (16, "fisheye", (20, 20), 180, (0.2, 0.2, 0.2)),
    "D": (9, "fisheye", (17, 23), 150, (0.2, -0.27, 0.57)),
}
FACE_KEYS = tuple(f"s_{f}" for f in ("back", "down", "front", "left", "right", "up"))


def make_transformer(name, **kw):
    from habitat_amd.common.obs_transformers import CubeMap2Equirect, CubeMap2Fisheye
    size, kind, out_hw, fov, params = GEOMETRIES[name]
    uuids = kw.pop("sensor_uuids", list(FACE_KEYS))
    if kind == "equirect":
        return CubeMap2Equirect(uuids, out_hw, **kw)
    return CubeMap2Fisheye(uuids, out_hw, fov, params, **kw)


@functools.lru_cache(maxsize=None)
def tables(name):
    """-> (face (h, w) int32, gx, gy (h, w) fp32, z-factor (H, W) fp32, packed (h*w, 3) int32) as the transformer builds them."""
    size, _, out_hw, _, _ = GEOMETRIES[name]
    packed, zf = make_transformer(name).host_tables(size)
    face = packed[:, 0].reshape(out_hw).clone()
    gx = packed[:, 1].clone().view(torch.float32).reshape(out_hw)
    gy = packed[:, 2].clone().view(torch.float32).reshape(out_hw)
    return face, gx, gy, zf, packed


def grid_sample_reference(faces, face, gx, gy, zfactor=None):
    """faces: six (N, H, W, C) tensors -> (N, h, w, C) float64."""
    n, H, W, C = faces[0].shape
    h, w = face.shape
    x = torch.stack([f.double() for f in faces], 1).permute(0, 1, 4, 2, 3)  # N, 6, C, H, W
    if zfactor is not None:
        x = x * zfactor.double()
    grids = torch.full((len(faces), h, w, 2), 2.0, dtype=torch.float64)
    for i in range(len(faces)):
        m = face == i
        grids[i, ..., 0][m] = gx.double()[m]
        grids[i, ..., 1][m] = gy.double()[m]
    out = F.grid_sample(x.reshape(n * len(faces), C, H, W), grids.repeat(n, 1, 1, 1), mode="bilinear", padding_mode="zeros",
                        align_corners=True)
    return out.view(n, len(faces), C, h, w).sum(1).permute(0, 2, 3, 1).contiguous()


def four_tap_reference(faces, face, gx, gy, zfactor=None):
    """The kernel's form in float64: one face per pixel, taps nw, ne, sw, se, a tap outside the face contributes 0."""
    n, H, W, C = faces[0].shape
    h, w = face.shape
    x = torch.stack([f.double() for f in faces], 0)  # 6, N, H, W, C
    if zfactor is not None:
        x = x * zfactor.double()[None, None, :, :, None]
    ix = ((gx.double() + 1) / 2) * (W - 1)
    iy = ((gy.double() + 1) / 2) * (H - 1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    x1, y1 = x0 + 1, y0 + 1
    out = torch.zeros(n, h, w, C, dtype=torch.float64)
    fidx = face.long().clamp(min=0)
    for xt, yt, wt in ((x0, y0, (x1 - ix) * (y1 - iy)), (x1, y0, (ix - x0) * (y1 - iy)), (x0, y1, (x1 - ix) * (iy - y0)),
                       (x1, y1, (ix - x0) * (iy - y0))):
        ok = (face >= 0) & (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
        xi, yi = xt.long().clamp(0, W - 1), yt.long().clamp(0, H - 1)
        v = x[fidx, :, yi, xi]  # h, w, N, C
        out += torch.where(ok[..., None, None], v * wt[..., None, None], torch.zeros((), dtype=torch.float64)).permute(2, 0, 1, 3)
    return out
