"""Observation transformers of the PPO path on the device (N4).

Plugin surface of habitat_baselines/common/obs_transformers.py: `ObservationTransformer` (:47-66), the registered
`ResizeShortestEdge` (:69-148) and `CenterCropper` (:151-231) with the reference's constructor / `from_config` /
`transform_observation_space` / `forward` semantics, `get_active_obs_transforms` (:1201-1224),
`apply_obs_transforms_batch` (:1227-1233) and `apply_obs_transforms_obs_space` (:1236-1242).

The reference resizes with permute -> float -> F.interpolate("area" | "nearest") -> cast -> permute and crops with a slice, one
sensor at a time.  Here every (sensor, transform) is one `hab_obs_resize_crop` launch, and `apply_obs_transforms_batch` FUSES a
ResizeShortestEdge that is directly followed by a CenterCropper on the same sensor into a single launch that only computes the
pixels surviving the crop (640x480 -> 341x256 -> 256x256 for the ObjectNav sensors).  Results are bit-identical to the
reference's CPU output for each of the three kernels the launcher chooses among (tests/test_gpu_resize_crop.py, against the plain
restatement of tests/resize_crop_reference.py; tests/test_obs_transformers.py against the reference's golden outputs).

Projection transformers (N6): `CubeMap2Equirect` and `CubeMap2Fisheye` (:239-1199) turn six cube-face cameras into one panorama or
one fisheye frame.  The reference stacks the six sensors, permutes, converts to float, multiplies depth by a z-factor, runs
F.grid_sample(bilinear, zeros, align_corners=True) against six precomputed grids, sums over the faces, casts and permutes back.
Here the six grids are folded on the host into ONE table {face, gx, gy} per output pixel (a pixel belongs to the first face that
sees its ray, so the reference's sum has a single non-zero term) and every sensor group is one `hab_obs_project` launch that reads
the six NHWC sensors where they lie and writes the target once in the sensor's dtype.  `Equirect2CubeMap` is not provided.

The geometry below is this project's statement of the reference classes; it is pinned to a float64 restatement
(tests/projection_reference.py), not to goldens of the live reference.  All of it is torch fp32 on the CPU, built once per
transformer and face size and uploaded.

  Axes: x right, y down, z forward.  A camera has a rotation R whose rows are (right, down, forward) in world coordinates, with
  right = down x forward; a camera point is cam = R . world.
  Cube faces, in sensor order BACK, DOWN, FRONT, LEFT, RIGHT, UP, as (forward, down): (-z, +y), (+y, -z), (+z, +y), (-x, +y),
  (+x, +y), (-y, +z).  Faces are square and of one size H = W.
  Perspective projection of a unit ray p onto a face: c = R.p, f = max(H, W)/2, img = f * c / |c_z|, gx = 2*(img_x + W/2)/W - 1,
  gy likewise with H; the ray is valid when max(|gx|, |gy|) <= 1 and c_z > 0.
  Depth factor of face texel (v, u): x = u + 0.5 - W/2, y = v + 0.5 - H/2, zf = sqrt(x^2 + y^2 + f^2) / f (z-depth -> distance from
  the optical centre); applied only to groups whose target name contains `depth_key`.
  Equirect unprojection of output pixel (v, u) of an (h, w) image: theta = (u + 0.5)*2pi/w - pi, phi = (v + 0.5)*pi/h - pi/2, ray =
  (cos phi sin theta, sin phi, cos phi cos theta); every pixel is valid.
  Fisheye unprojection (double-sphere model; fov in degrees, cx = w/2, cy = h/2, fx = fy = params[0]*min(h, w), xi = params[1],
  alpha = params[2]): mx = (u + 0.5 - cx)/fx, my = (v + 0.5 - cy)/fy, r2 = mx^2 + my^2,
  mz = (1 - alpha^2 r2) / (alpha*sqrt(1 - (2 alpha - 1) r2) + 1 - alpha), k = (mz*xi + sqrt(mz^2 + (1 - xi^2) r2)) / (mz^2 + r2),
  ray = (k*mx, k*my, k*mz - xi) normalised; valid when r2 <= 1/(2 alpha - 1) (only for alpha > 0.5) and ray_z >= cos(fov/2).
  Assignment: the faces are visited in order; a pixel takes the first face on which its ray is valid and is then closed to later
  faces (the reference's `not_assigned_mask`).  Pixels with no valid ray, or no face, get face = -1 and are written as 0."""
from __future__ import annotations

import abc
import copy
import ctypes
import math
import numbers
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from habitat_amd import _lib
from habitat_amd.common import spaces
from habitat_amd.common.baseline_registry import baseline_registry
from habitat_amd.utils.logging import logger

_DTYPES = {torch.uint8: 0, torch.float32: 1, torch.int32: 2}
AREA, NEAREST = 0, 1


def get_image_height_width(img, channels_last: bool = False) -> Tuple[int, int]:
    """utils/common.py:560-575."""
    shape = img.shape
    if len(shape) < 3 or len(shape) > 5:
        raise NotImplementedError()
    return (shape[-3], shape[-2]) if channels_last else (shape[-2], shape[-1])


def overwrite_gym_box_shape(box, shape):
    """utils/common.py:578-592: same channel count and value range, new (h, w)."""
    if box.shape == tuple(shape):
        return box
    shape = tuple(shape) + tuple(box.shape[len(shape):])
    low = box.low if np.isscalar(box.low) else np.min(box.low)
    high = box.high if np.isscalar(box.high) else np.max(box.high)
    return spaces.Box(low=low, high=high, shape=shape, dtype=box.dtype)


def resized_extent(h: int, w: int, size: int) -> Tuple[int, int]:
    """utils/common.py:512-515."""
    scale = size / min(h, w)
    return int(h * scale), int(w * scale)


def center_window(h: int, w: int, size: Tuple[int, int]) -> Tuple[int, int]:
    """utils/common.py:550-553 -> (starty, startx)."""
    cropy, cropx = size
    return h // 2 - (cropy // 2), w // 2 - (cropx // 2)


def resize_crop(obs: torch.Tensor, resized: Tuple[int, int], window: Tuple[int, int, int, int], mode: int,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch: NHWC `obs` virtually resized to `resized` = (h, w), window (y0, x0, oh, ow) of that written NHWC."""
    if not obs.is_cuda:
        raise _lib.HabError("obs transformers run on the device: the batch must be a CUDA tensor (no CPU execution path)")
    if obs.dtype not in _DTYPES:
        raise _lib.HabError(f"unsupported sensor dtype {obs.dtype}")
    squeeze = obs.dim() == 3
    x = (obs.unsqueeze(0) if squeeze else obs).contiguous()
    lead = x.shape[:-3]
    x = x.reshape(-1, *x.shape[-3:])
    n, h, w, c = x.shape
    y0, x0, oh, ow = window
    if out is None:
        out = torch.empty((n, oh, ow, c), dtype=obs.dtype, device=obs.device)
    assert out.is_contiguous() and out.numel() == n * oh * ow * c and out.dtype == obs.dtype
    _lib.check(_lib.lib().hab_obs_resize_crop(_lib.ptr(x), _lib.ptr(out), _DTYPES[obs.dtype], n, h, w, c, resized[0], resized[1],
                                              y0, x0, oh, ow, mode, _lib.stream_ptr()), "hab_obs_resize_crop")
    res = out.reshape(*lead, oh, ow, c)
    return res.squeeze(0) if squeeze else res


class ObservationTransformer(torch.nn.Module, metaclass=abc.ABCMeta):
    def transform_observation_space(self, observation_space, **kwargs):
        return observation_space

    @classmethod
    @abc.abstractmethod
    def from_config(cls, config):
        pass

    def forward(self, observations: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return observations


@baseline_registry.register_obs_transformer()
class ResizeShortestEdge(ObservationTransformer):
    def __init__(self, size: int, channels_last: bool = True, trans_keys: Tuple[str, ...] = ("rgb", "depth", "semantic"),
                 semantic_key: str = "semantic"):
        super().__init__()
        if not channels_last:
            raise _lib.HabError("ResizeShortestEdge: the device kernels take NHWC sensors (channels_last=True)")
        self._size = size
        self.channels_last = channels_last
        self.trans_keys = tuple(trans_keys)
        self.semantic_key = semantic_key

    def transform_observation_space(self, observation_space, **kwargs):
        observation_space = copy.deepcopy(observation_space)
        if self._size:
            for key in observation_space.spaces:
                if key in self.trans_keys:
                    h, w = get_image_height_width(observation_space.spaces[key], channels_last=True)
                    if self._size == min(h, w):
                        continue
                    new_size = resized_extent(h, w, self._size)
                    logger.info("Resizing observation of %s: from %s to %s" % (key, (h, w), new_size))
                    observation_space.spaces[key] = overwrite_gym_box_shape(observation_space.spaces[key], new_size)
        return observation_space

    def mode_of(self, sensor: str) -> int:
        return NEAREST if self.semantic_key in sensor else AREA

    @torch.no_grad()
    def forward(self, observations):
        if self._size is not None:
            for sensor in self.trans_keys:
                if sensor in observations:
                    h, w = get_image_height_width(observations[sensor], channels_last=True)
                    rh, rw = resized_extent(h, w, self._size)
                    observations[sensor] = resize_crop(observations[sensor], (rh, rw), (0, 0, rh, rw), self.mode_of(sensor))
        return observations

    @classmethod
    def from_config(cls, config):
        return cls(config.size, config.get("channels_last", True), config.get("trans_keys", ("rgb", "depth", "semantic")),
                   config.get("semantic_key", "semantic"))


@baseline_registry.register_obs_transformer()
class CenterCropper(ObservationTransformer):
    """obs_transformers.py:151-231.  One difference, on purpose: a crop larger than the image is refused with a `HabError` (alone or
    fused behind a ResizeShortestEdge).  The reference's slice silently returns an image smaller than the observation space says."""

    def __init__(self, size: Union[numbers.Integral, Tuple[int, int]], channels_last: bool = True,
                 trans_keys: Tuple[str, ...] = ("rgb", "depth", "semantic")):
        super().__init__()
        if not channels_last:
            raise _lib.HabError("CenterCropper: the device kernels take NHWC sensors (channels_last=True)")
        if isinstance(size, numbers.Integral):
            size = (int(size), int(size))
        assert len(size) == 2, "forced input size must be len of 2 (h, w)"
        self._size = tuple(int(s) for s in size)
        self.channels_last = channels_last
        self.trans_keys = tuple(trans_keys)

    def transform_observation_space(self, observation_space, **kwargs):
        observation_space = copy.deepcopy(observation_space)
        if self._size:
            for key in observation_space.spaces:
                if key in self.trans_keys and tuple(observation_space.spaces[key].shape[-3:-1]) != self._size:
                    h, w = get_image_height_width(observation_space.spaces[key], channels_last=True)
                    logger.info("Center cropping observation size of %s from %s to %s" % (key, (h, w), self._size))
                    observation_space.spaces[key] = overwrite_gym_box_shape(observation_space.spaces[key], self._size)
        return observation_space

    @torch.no_grad()
    def forward(self, observations):
        if self._size is not None:
            for sensor in self.trans_keys:
                if sensor in observations:
                    h, w = get_image_height_width(observations[sensor], channels_last=True)
                    y0, x0 = center_window(h, w, self._size)
                    observations[sensor] = resize_crop(observations[sensor], (h, w), (y0, x0, *self._size), NEAREST)
        return observations

    @classmethod
    def from_config(cls, config):
        return cls((config.height, config.width), config.get("channels_last", True),
                   config.get("trans_keys", ("rgb", "depth", "semantic")))


# ------------------------------------------------------------------------------------------------------------------------------------
# Projection transformers: geometry (host, torch fp32) and the plugin classes
# ------------------------------------------------------------------------------------------------------------------------------------
# (forward, down) of each face in world coordinates, in sensor order BACK, DOWN, FRONT, LEFT, RIGHT, UP
_FACE_AXES = (((0., 0., -1.), (0., 1., 0.)), ((0., 1., 0.), (0., 0., -1.)), ((0., 0., 1.), (0., 1., 0.)),
              ((-1., 0., 0.), (0., 1., 0.)), ((1., 0., 0.), (0., 1., 0.)), ((0., -1., 0.), (0., 0., 1.)))


def cube_face_rotations() -> torch.Tensor:
    """(6, 3, 3): rows (right, down, forward) of every face, right = down x forward."""
    rots = []
    for fwd, down in _FACE_AXES:
        f, d = torch.tensor(fwd), torch.tensor(down)
        rots.append(torch.stack([torch.linalg.cross(d, f), d, f]))
    return torch.stack(rots)


def perspective_project(rays: torch.Tensor, rot: torch.Tensor, height: int, width: int):
    """Unit rays (..., 3) onto a face -> (gx, gy, valid)."""
    c = rays @ rot.T
    f = max(height, width) / 2
    img = f * c / c[..., 2:3].abs()
    gx = 2 * (img[..., 0] + width / 2) / width - 1
    gy = 2 * (img[..., 1] + height / 2) / height - 1
    valid = (torch.maximum(gx.abs(), gy.abs()) <= 1) & (c[..., 2] > 0)
    return gx, gy, valid


def perspective_depth_factor(height: int, width: int) -> torch.Tensor:
    """(H, W) fp32: distance from the optical centre per unit of z-depth."""
    f = max(height, width) / 2
    y = torch.arange(height, dtype=torch.float32) + 0.5 - height / 2
    x = torch.arange(width, dtype=torch.float32) + 0.5 - width / 2
    return torch.sqrt(x[None, :] ** 2 + y[:, None] ** 2 + f ** 2) / f


def equirect_rays(height: int, width: int):
    """-> (rays (h, w, 3), valid (h, w))."""
    theta = (torch.arange(width, dtype=torch.float32) + 0.5) * (2 * math.pi / width) - math.pi
    phi = (torch.arange(height, dtype=torch.float32) + 0.5) * (math.pi / height) - math.pi / 2
    phi, theta = torch.meshgrid(phi, theta, indexing="ij")
    rays = torch.stack([torch.cos(phi) * torch.sin(theta), torch.sin(phi), torch.cos(phi) * torch.cos(theta)], -1)
    return rays, torch.ones(height, width, dtype=torch.bool)


def fisheye_rays(height: int, width: int, fov: float, params: Sequence[float]):
    """Double-sphere unprojection -> (rays (h, w, 3), valid (h, w))."""
    f, xi, alpha = (float(p) for p in params)
    fx = fy = f * min(height, width)
    my = (torch.arange(height, dtype=torch.float32) + 0.5 - height / 2) / fy
    mx = (torch.arange(width, dtype=torch.float32) + 0.5 - width / 2) / fx
    my, mx = torch.meshgrid(my, mx, indexing="ij")
    r2 = mx * mx + my * my
    mz = (1 - alpha * alpha * r2) / (alpha * torch.sqrt(1 - (2 * alpha - 1) * r2) + 1 - alpha)
    k = (mz * xi + torch.sqrt(mz * mz + (1 - xi * xi) * r2)) / (mz * mz + r2)
    rays = torch.stack([k * mx, k * my, k * mz - xi], -1)
    rays = rays / torch.linalg.norm(rays, dim=-1, keepdim=True)
    valid = rays[..., 2] >= math.cos(math.radians(fov) / 2)
    if alpha > 0.5:
        valid = valid & (r2 <= 1 / (2 * alpha - 1))
    return rays, valid


def build_projection_table(rays: torch.Tensor, valid: torch.Tensor, face_h: int, face_w: int):
    """First-valid-face assignment -> (face (h, w) int32, gx, gy (h, w) fp32); face = -1 (and g = 0) where there is no source."""
    face = torch.full(valid.shape, -1, dtype=torch.int32)
    gx, gy = torch.zeros(valid.shape), torch.zeros(valid.shape)
    not_assigned = valid.clone()
    for i, rot in enumerate(cube_face_rotations()):
        fx, fy, ok = perspective_project(rays, rot, face_h, face_w)
        take = ok & not_assigned
        face[take] = i
        gx[take], gy[take] = fx[take], fy[take]
        not_assigned &= ~take
    return face, gx, gy


def pack_projection_table(face: torch.Tensor, gx: torch.Tensor, gy: torch.Tensor) -> torch.Tensor:
    """(h*w, 3) int32 = the kernel's {int32 face; float gx; float gy} entries."""
    return torch.stack([face.reshape(-1).to(torch.int32), gx.reshape(-1).float().view(torch.int32),
                        gy.reshape(-1).float().view(torch.int32)], 1).contiguous()


def project_faces(faces: Sequence[torch.Tensor], table: torch.Tensor, out_hw: Tuple[int, int],
                  zfactor: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch: the (..., H, W, C) NHWC face sensors gathered through `table` into (..., h, w, C) of the faces' dtype."""
    f0 = faces[0]
    _check_face("projection", [(str(i), tuple(f.shape), f.dtype) for i, f in enumerate(faces)])
    if any(not f.is_cuda for f in faces):
        raise _lib.HabError("obs transformers run on the device: the batch must be a CUDA tensor (no CPU execution path)")
    lead, (h, w, c) = f0.shape[:-3], f0.shape[-3:]
    flat = [f.contiguous().reshape(-1, h, w, c) for f in faces]  # kept alive until the launch is enqueued
    n = flat[0].shape[0]
    oh, ow = out_hw
    if out is None:
        out = torch.empty((n, oh, ow, c), dtype=f0.dtype, device=f0.device)
    assert out.is_contiguous() and out.numel() == n * oh * ow * c and out.dtype == f0.dtype
    assert table.is_cuda and table.dtype == torch.int32 and table.is_contiguous() and table.numel() == oh * ow * 3
    assert zfactor is None or (zfactor.is_cuda and zfactor.dtype == torch.float32 and zfactor.is_contiguous() and zfactor.numel() == h * w)
    srcs = (ctypes.c_void_p * len(flat))(*[f.data_ptr() for f in flat])
    _lib.check(_lib.lib().hab_obs_project(srcs, len(flat), _lib.ptr(out), _DTYPES[f0.dtype], n, h, w, c, _lib.ptr(table),
                                          _lib.ptr(zfactor), oh, ow, _lib.stream_ptr()), "hab_obs_project")
    return out.reshape(*lead, oh, ow, c)


class ProjectionTransformer(ObservationTransformer):
    """Six cube-face sensors per group -> one target per group (obs_transformers.py:845-1010).  `sensor_uuids` lists the groups one
    after the other, each in the order BACK, DOWN, FRONT, LEFT, RIGHT, UP; `target_uuids` defaults to the first sensor of each group.
    `channels_last` is accepted for signature compatibility only: either value means NHWC sensors, which is what the env sources
    and `batch_obs` produce and what the kernel reads.  `drop_inputs` (an extension; the default keeps the reference's behaviour)
    removes the face sensors that are not targets from the observation space and from the batch, so that the rollout does not store
    six faces per panorama and the policy sees visual sensors of one size."""

    def __init__(self, sensor_uuids: Sequence[str], out_shape: Tuple[int, int], channels_last: bool = False,
                 target_uuids: Optional[Sequence[str]] = None, depth_key: str = "depth", drop_inputs: bool = False):
        super().__init__()
        sensor_uuids = list(sensor_uuids)
        if len(sensor_uuids) == 0 or len(sensor_uuids) % 6 != 0:
            raise _lib.HabError(f"{len(sensor_uuids)}: length of sensors is not a multiple of 6 (and not empty)")
        if len(out_shape) != 2 or min(out_shape) <= 0:
            raise _lib.HabError(f"the output shape must be (height, width), got {tuple(out_shape)}")
        self.sensor_uuids = sensor_uuids
        self.num_groups = len(sensor_uuids) // 6
        self.target_uuids = list(target_uuids) if target_uuids is not None else sensor_uuids[::6]
        if len(self.target_uuids) != self.num_groups:
            raise _lib.HabError(f"target_uuids has {len(self.target_uuids)} names for {self.num_groups} groups of six sensors")
        self.out_shape = (int(out_shape[0]), int(out_shape[1]))
        self.channels_last = channels_last
        self.depth_key = depth_key
        self.drop_inputs = bool(drop_inputs)
        self._host_tables: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}     # face size -> (table, z-factor) on the host
        self._device_tables: Dict[Tuple[int, torch.device], Tuple[torch.Tensor, torch.Tensor]] = {}

    def output_rays(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (unit rays (h, w, 3), valid (h, w)) of the output image."""
        raise NotImplementedError

    def host_tables(self, face_size: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if face_size not in self._host_tables:
            rays, valid = self.output_rays()
            table = pack_projection_table(*build_projection_table(rays, valid, face_size, face_size))
            self._host_tables[face_size] = (table, perspective_depth_factor(face_size, face_size).contiguous())
        return self._host_tables[face_size]

    def _tables_on(self, face_size: int, device: torch.device):
        key = (face_size, device)
        if key not in self._device_tables:
            self._device_tables[key] = tuple(t.to(device) for t in self.host_tables(face_size))
        return self._device_tables[key]

    def _groups(self):
        return [(self.target_uuids[i], self.sensor_uuids[6 * i:6 * i + 6]) for i in range(self.num_groups)]

    def _dropped(self):
        return [k for k in self.sensor_uuids if k not in self.target_uuids] if self.drop_inputs else []

    def transform_observation_space(self, observation_space, **kwargs):
        observation_space = copy.deepcopy(observation_space)
        for target, group in self._groups():
            for k in group:
                if k not in observation_space.spaces:
                    raise _lib.HabError(f"{type(self).__name__}: sensor {k} is not in the observation space")
            box = observation_space.spaces[group[0]]
            _check_face(target, [(k, tuple(observation_space.spaces[k].shape), observation_space.spaces[k].dtype) for k in group])
            logger.info("Overwrite sensor: %s from size of %s to image of %s" % (target, tuple(box.shape[-3:-1]), self.out_shape))
            observation_space.spaces[target] = overwrite_gym_box_shape(box, self.out_shape)
        for k in self._dropped():
            del observation_space.spaces[k]
        return observation_space

    @torch.no_grad()
    def forward(self, observations):
        for target, group in self._groups():
            faces = [observations[k] for k in group]
            _check_face(target, [(k, tuple(f.shape), f.dtype) for k, f in zip(group, faces)])
            if not faces[0].is_cuda:  # before any table is built for that device
                raise _lib.HabError("obs transformers run on the device: the batch must be a CUDA tensor (no CPU execution path)")
            table, zf = self._tables_on(faces[0].shape[-2], faces[0].device)
            observations[target] = project_faces(faces, table, self.out_shape, zf if self.depth_key in target else None)
        for k in self._dropped():
            observations.pop(k, None)
        return observations


def _check_face(target, faces):
    """`faces`: (name, shape, dtype) of the six sensors of one group."""
    _, shape0, dtype0 = faces[0]
    if any(shape != shape0 or dtype != dtype0 for _, shape, dtype in faces):
        raise _lib.HabError(f"{target}: the faces of one group differ in shape or dtype: " + ", ".join(f"{k} {s}:{d}" for k, s, d in faces))
    if len(shape0) < 3:
        raise _lib.HabError(f"{target}: projection transformers take (..., H, W, C) sensors, got shape {shape0}")
    if shape0[-3] != shape0[-2]:
        raise _lib.HabError(f"{target}: cube faces are square, got {shape0[-3]} x {shape0[-2]}")
    if shape0[-1] > 4:
        raise _lib.HabError(f"{target}: projection transformers take at most 4 channels, got {shape0[-1]}")
    if str(dtype0).replace("torch.", "") not in ("uint8", "float32"):
        raise _lib.HabError(f"{target}: projection transformers take uint8 or float32 sensors, not {dtype0}")


@baseline_registry.register_obs_transformer()
class CubeMap2Equirect(ProjectionTransformer):
    """Six cube faces -> an equirectangular panorama of `eq_shape` = (height, width) (obs_transformers.py:1013-1068)."""

    def __init__(self, sensor_uuids: Sequence[str], eq_shape: Tuple[int, int], channels_last: bool = False,
                 target_uuids: Optional[Sequence[str]] = None, depth_key: str = "depth", drop_inputs: bool = False):
        super().__init__(sensor_uuids, eq_shape, channels_last, target_uuids, depth_key, drop_inputs)

    def output_rays(self):
        return equirect_rays(*self.out_shape)

    @classmethod
    def from_config(cls, config):
        return cls(config.sensor_uuids, eq_shape=(config.height, config.width), target_uuids=config.get("target_uuids", None),
                   depth_key=config.get("depth_key", "depth"), drop_inputs=config.get("drop_inputs", False))


@baseline_registry.register_obs_transformer()
class CubeMap2Fisheye(ProjectionTransformer):
    """Six cube faces -> a double-sphere fisheye frame of `fish_shape` = (height, width), field of view `fish_fov` degrees,
    `fish_params` = (f, xi, alpha) (obs_transformers.py:1071-1142)."""

    def __init__(self, sensor_uuids: Sequence[str], fish_shape: Tuple[int, int], fish_fov: float, fish_params: Sequence[float],
                 channels_last: bool = False, target_uuids: Optional[Sequence[str]] = None, depth_key: str = "depth",
                 drop_inputs: bool = False):
        super().__init__(sensor_uuids, fish_shape, channels_last, target_uuids, depth_key, drop_inputs)
        if len(fish_params) != 3:
            raise _lib.HabError(f"fish_params is (f, xi, alpha), got {tuple(fish_params)}")
        self.fish_fov = float(fish_fov)
        self.fish_params = tuple(float(p) for p in fish_params)

    def output_rays(self):
        return fisheye_rays(*self.out_shape, self.fish_fov, self.fish_params)

    @classmethod
    def from_config(cls, config):
        return cls(config.sensor_uuids, (config.height, config.width), config.get("fov", 180), config.get("params", (0.2, 0.2, 0.2)),
                   target_uuids=config.get("target_uuids", None), depth_key=config.get("depth_key", "depth"),
                   drop_inputs=config.get("drop_inputs", False))


def get_active_obs_transforms(config, agent_name: Optional[str] = None) -> List[ObservationTransformer]:
    active = []
    policies = config.habitat_baselines.rl.policy
    agent_name = list(policies.keys())[0]
    conf = policies[agent_name].get("obs_transforms", None) or {}
    for tcfg in conf.values():
        cls = baseline_registry.get_obs_transformer(tcfg.type)
        if cls is None:
            raise ValueError(f"Unkown ObservationTransform with name {tcfg.type}.")
        active.append(cls.from_config(tcfg))
    return active


def apply_obs_transforms_batch(batch: Dict[str, torch.Tensor], obs_transforms: Iterable[ObservationTransformer]):
    """Applies the transformers in order; ResizeShortestEdge directly followed by CenterCropper is fused per sensor."""
    ts = list(obs_transforms)
    i = 0
    while i < len(ts):
        t = ts[i]
        nxt = ts[i + 1] if i + 1 < len(ts) else None
        if (isinstance(t, ResizeShortestEdge) and isinstance(nxt, CenterCropper) and t._size is not None and nxt._size is not None
                and not isinstance(batch, torch.Tensor)):
            for sensor in set(t.trans_keys) | set(nxt.trans_keys):
                if sensor not in batch:
                    continue
                if sensor in t.trans_keys and sensor in nxt.trans_keys:
                    h, w = get_image_height_width(batch[sensor], channels_last=True)
                    rh, rw = resized_extent(h, w, t._size)
                    y0, x0 = center_window(rh, rw, nxt._size)
                    if y0 >= 0 and x0 >= 0 and y0 + nxt._size[0] <= rh and x0 + nxt._size[1] <= rw:
                        batch[sensor] = resize_crop(batch[sensor], (rh, rw), (y0, x0, *nxt._size), t.mode_of(sensor))
                        continue
                # not fusable for this sensor: the two transformers one after the other
                one = {sensor: batch[sensor]}
                if sensor in t.trans_keys:
                    one = ResizeShortestEdge(t._size, True, (sensor,), t.semantic_key)(one)
                if sensor in nxt.trans_keys:
                    one = CenterCropper(nxt._size, True, (sensor,))(one)
                batch[sensor] = one[sensor]
            i += 2
            continue
        batch = t(batch)
        i += 1
    return batch


def apply_obs_transforms_obs_space(obs_space, obs_transforms: Iterable[ObservationTransformer]):
    for t in obs_transforms:
        obs_space = t.transform_observation_space(obs_space)
    return obs_space
