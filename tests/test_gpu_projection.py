"""CubeMap2Equirect / CubeMap2Fisheye on the device: `hab_obs_project` against the float64 restatement
(tests/projection_reference.py) on the same fp32 table, the plugin classes, the C entry point's error codes, and two update cycles
of the trainer on six-face observations.

float32 bound: |gpu - ref64| <= 2^-21 * (H + W) * max|zf * v|.  `ix` carries at most two fp32 roundings of a value below W, so each
weight is off by about 2^-23 * W, and likewise for H; the four weight errors add to at most 2^-22 * (W + H); the factor 2 covers the
roundings of the products and of the sum.  uint8: |gpu - floor(ref64)| <= 1 everywhere, and equality wherever ref64 is farther from
an integer than 255 * 2^-21 * (H + W) (the same bound at the largest uint8 value); the elements this leaves out are at most 5 %."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from projection_reference import GEOMETRIES, grid_sample_reference, tables

pytestmark = pytest.mark.gpu

FACES = ("back", "down", "front", "left", "right", "up")
RGB = [f"rgb_{f}" for f in FACES]
DEPTH = [f"depth_{f}" for f in FACES]
BATCHES = (1, 3, 5)
# (dtype, channels, with z-factor)
VARIANTS = {"u8c3": (torch.uint8, 3, False), "u8c1": (torch.uint8, 1, False), "f32c1z": (torch.float32, 1, True),
            "f32c4": (torch.float32, 4, False)}


def _host_faces(size, dtype, c, n, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return [torch.randint(0, 256, (n, size, size, c), generator=g, dtype=torch.uint8) for _ in range(6)]
    return [torch.rand(n, size, size, c, generator=g) * 10 for _ in range(6)]


@functools.lru_cache(maxsize=None)
def _case(name, variant, n):
    """Seeded faces of the case and their float64 reference, computed once and shared."""
    size = GEOMETRIES[name][0]
    dtype, c, use_zf = VARIANTS[variant]
    face, gx, gy, zf, _ = tables(name)
    faces = _host_faces(size, dtype, c, n, seed=1000 * n + len(variant) + size)
    ref = grid_sample_reference(faces, face, gx, gy, zf if use_zf else None)
    return faces, ref


def _project(name, faces, use_zf):
    from habitat_amd.common.obs_transformers import project_faces
    _, _, _, zf, packed = tables(name)
    dev = [f.cuda() for f in faces]  # six separately allocated face tensors
    out = project_faces(dev, packed.cuda(), GEOMETRIES[name][2], zf.cuda() if use_zf else None)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_kernel_vs_float64(name, variant):
    size = GEOMETRIES[name][0]
    dtype, c, use_zf = VARIANTS[variant]
    face, _, _, zf, _ = tables(name)
    assigned = (face >= 0)[None, :, :, None]
    for n in BATCHES:
        faces, ref = _case(name, variant, n)
        got = _project(name, faces, use_zf)
        assert got.dtype == dtype and got.shape == ref.shape == (n, *face.shape, c)
        assert bool((got[~assigned.expand_as(got)] == 0).all())  # no source: exactly 0
        if dtype == torch.float32:
            vmax = max(float(((f.double() * zf.double()[None, :, :, None]) if use_zf else f.double()).abs().max()) for f in faces)
            bound = 2.0 ** -21 * (2 * size) * vmax
            err = float((got.double() - ref).abs().max())
            print(f"{name} {variant} N={n}: max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.4f}")
            assert err <= bound, (name, variant, n, err, bound)
        else:
            _check_uint8(got, ref, size, assigned, (name, variant, n))


def _check_uint8(got, ref, size, assigned, what):
    want = torch.floor(ref)
    diff = (got.double() - want).abs()
    assert float(diff.max()) <= 1, what
    exempt = (ref - torch.round(ref)).abs() <= 255 * 2.0 ** -21 * (2 * size)
    assert bool((diff[~exempt] == 0).all()), (what, int((diff[~exempt] != 0).sum()))
    mask = assigned.expand_as(ref)
    share = float((exempt & mask).sum()) / float(mask.sum())
    print(f"{what}: exempt share {share:.4f}, +-1 inside it {int((diff != 0).sum())}")
    assert share <= 0.05, (what, share)


def test_fallback_kernel_paths():
    """Packed uint8 rgb and one-channel float32 normally fetch both horizontal taps of a row with one load.  Faces that do not
    start on a 4-byte boundary, and faces one texel wide, take the one-load-per-tap kernel: the same bits."""
    from habitat_amd.common.obs_transformers import project_faces
    _, _, _, _, packed = tables("A")
    faces, _ = _case("A", "u8c3", 3)
    want = _project("A", faces, False)
    shifted = []
    for f in faces:
        buf = torch.empty(f.numel() + 1, dtype=torch.uint8, device="cuda")
        view = buf[1:].view(f.shape)
        view.copy_(f)
        assert view.data_ptr() % 4 == 1 and view.is_contiguous()
        shifted.append(view)
    assert torch.equal(project_faces(shifted, packed.cuda(), GEOMETRIES["A"][2]).cpu(), want)
    # 1 x 1 faces: x1 = y1 = 1 lies outside, the only texel has weight 1 at g = (0, 0); entry 3 has no source
    table = torch.tensor([[5, 0, 0], [0, 0, 0], [2, 0, 0], [-1, 0, 0]], dtype=torch.int32).cuda()
    tiny = [torch.full((2, 1, 1, 1), float(k + 1), device="cuda") for k in range(6)]
    zf = torch.full((1, 1), 3.0, device="cuda")
    assert project_faces(tiny, table, (2, 2)).flatten().tolist() == [6.0, 1.0, 3.0, 0.0] * 2
    assert project_faces(tiny, table, (2, 2), zf).flatten().tolist() == [18.0, 3.0, 9.0, 0.0] * 2


def test_transformer_classes():
    from habitat_amd import _lib
    from habitat_amd.common.obs_transformers import CenterCropper, CubeMap2Equirect, apply_obs_transforms_batch
    size, (h, w), n = 16, (16, 32), 3
    face, gx, gy, zf, _ = tables("A")
    rgb = _host_faces(size, torch.uint8, 3, n, seed=7)
    depth = _host_faces(size, torch.float32, 1, n, seed=8)
    batch = {k: v.cuda() for k, v in zip(RGB + DEPTH, rgb + depth)}
    batch["gps"] = torch.arange(2 * n, dtype=torch.float32, device="cuda").reshape(n, 2)
    t = CubeMap2Equirect(RGB + DEPTH, (h, w), target_uuids=["rgb", "depth"])
    out = t(dict(batch))
    assert set(out) == set(batch) | {"rgb", "depth"}  # the reference keeps the faces
    assert out["rgb"].dtype == torch.uint8 and out["rgb"].shape == (n, h, w, 3)
    assert out["depth"].dtype == torch.float32 and out["depth"].shape == (n, h, w, 1)
    assert torch.equal(out["gps"], batch["gps"]) and out["rgb_up"] is batch["rgb_up"]  # untouched keys pass through
    # the depth group is z-corrected and the rgb group is not
    bound = 2.0 ** -21 * (2 * size) * max(float((f * zf[None, :, :, None]).abs().max()) for f in depth)
    ref_z, ref_plain = (grid_sample_reference(depth, face, gx, gy, z) for z in (zf, None))
    assert float((out["depth"].cpu().double() - ref_z).abs().max()) <= bound
    assert float((ref_z - ref_plain).abs().max()) > 100 * bound  # the two references are far apart: the check above tells them apart
    _check_uint8(out["rgb"].cpu(), grid_sample_reference(rgb, face, gx, gy, None), size, (face >= 0)[None, :, :, None], "class rgb")
    # a target named like one of its faces overwrites it (the reference's default target_uuids)
    d = CubeMap2Equirect(RGB, (h, w))(dict(batch))
    assert torch.equal(d["rgb_back"], out["rgb"]) and d["rgb_down"] is batch["rgb_down"]
    # drop_inputs: only the targets (and what the transformer does not own) remain
    dropped = CubeMap2Equirect(RGB + DEPTH, (h, w), target_uuids=["rgb", "depth"], drop_inputs=True)(dict(batch))
    assert sorted(dropped) == ["depth", "gps", "rgb"]
    assert torch.equal(dropped["rgb"], out["rgb"]) and torch.equal(dropped["depth"], out["depth"])
    # a CenterCropper after it crops the panorama
    crop = apply_obs_transforms_batch(dict(batch), [t, CenterCropper((8, 12), trans_keys=("rgb", "depth"))])
    assert torch.equal(crop["rgb"], out["rgb"][:, 4:12, 10:22]) and torch.equal(crop["depth"], out["depth"][:, 4:12, 10:22])
    assert crop["rgb_back"].shape == (n, size, size, 3)
    # leading dimensions (T, N, H, W, C) and a single frame (H, W, C)
    five = t({k: (v.reshape(1, n, *v.shape[1:]) if k != "gps" else v) for k, v in batch.items()})
    assert five["rgb"].shape == (1, n, h, w, 3) and torch.equal(five["rgb"][0], out["rgb"])
    one = t({k: v[1] for k, v in batch.items()})
    assert one["depth"].shape == (h, w, 1) and torch.equal(one["depth"], out["depth"][1])
    with pytest.raises(_lib.HabError, match="CUDA tensor"):
        t({k: v.cpu() for k, v in batch.items()})


def test_entry_point_error_codes():
    from habitat_amd import _lib
    L = _lib.lib()
    _, _, _, zf, packed = tables("A")
    faces = [torch.zeros(2, 16, 16, 4, device="cuda") for _ in range(7)]
    dst = torch.zeros(2, 16, 32, 4, device="cuda")
    tab, zf = packed.cuda(), zf.cuda()
    P, S = _lib.ptr, _lib.stream_ptr()
    srcs = (C.c_void_p * 7)(*[f.data_ptr() for f in faces])

    def call(src=srcs, n_src=6, dst_=dst, dtype=_lib.DTYPE_F32, N=2, H=16, W=16, Cn=4, table=tab, z=zf, oh=16, ow=32):
        return L.hab_obs_project(src, n_src, P(dst_), dtype, N, H, W, Cn, P(table), P(z), oh, ow, S)
    assert call() == 0 and call(z=None) == 0 and call(dtype=_lib.DTYPE_U8, Cn=1) == 0
    assert call(src=None) == -1 and call(dst_=None) == -1 and call(table=None) == -1
    holes = (C.c_void_p * 6)(*[faces[0].data_ptr(), None, faces[2].data_ptr(), None, None, None])
    assert call(src=holes) == -1                       # a null pointer inside the array
    assert call(n_src=7) == -1 and call(n_src=0) == -1
    assert call(Cn=5) == -1 and call(Cn=0) == -1
    assert call(N=0) == -1 and call(H=0) == -1 and call(oh=-1) == -1
    assert call(dtype=_lib.DTYPE_I32) == -2 and call(dtype=7) == -2
    torch.cuda.synchronize()
    # fewer than six sources: a table that only names faces below n_src
    small = torch.tensor([[0, 0, 0], [1, 0, 0], [-1, 0, 0]], dtype=torch.int32).cuda()  # g = (0, 0): the centre of the face
    a = torch.full((1, 3, 3, 1), 2.0, device="cuda")
    b = torch.full((1, 3, 3, 1), 5.0, device="cuda")
    two = (C.c_void_p * 2)(a.data_ptr(), b.data_ptr())
    out = torch.full((1, 1, 3, 1), -1.0, device="cuda")
    assert L.hab_obs_project(two, 2, P(out), _lib.DTYPE_F32, 1, 3, 3, 1, P(small), None, 1, 3, S) == 0
    assert out.flatten().tolist() == [2.0, 5.0, 0.0]


def test_trainer_on_cubemap_host_env(tmp_path):
    """Two update cycles through the YAML entry point with worker processes that emit six 32 x 32 cube faces per sensor; a
    CubeMap2Fisheye to 64 x 64 with named targets and drop_inputs feeds a ResNet18 policy: finite losses, parameters move."""
    from habitat_amd.config.default import get_config
    from habitat_amd.common.baseline_registry import baseline_registry
    from habitat_amd.common.obs_transformers import CubeMap2Fisheye
    import habitat_amd.rl.ppo.ppo_trainer  # noqa: F401
    N, T, size, out = 2, 4, 32, 64
    pre = "habitat_baselines.rl.policy.main_agent.obs_transforms.cube2fish."
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=3",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          "habitat_baselines.rl.ppo.hidden_size=64", f"habitat_baselines.checkpoint_folder={tmp_path}",
          "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000", "habitat_baselines.rl.ddppo.backbone=resnet18",
          "habitat_baselines.rl.ppo.num_mini_batch=1",
          "habitat_baselines.vector_env_factory._target_=habitat_amd.common.env_factory.ProcessVectorEnvFactory",
          "habitat_baselines.vector_env_factory.make_env_fn=habitat_amd.core.host_env.make_cubemap_host_env",
          pre + "type=CubeMap2Fisheye", pre + f"height={out}", pre + f"width={out}",
          pre + "sensor_uuids=[" + ",".join(RGB + DEPTH) + "]", pre + "target_uuids=[rgb,depth]", pre + "drop_inputs=true"]
    for sname in ("rgb", "depth"):
        ov += [f"habitat.simulator.sensors.{sname}.height={size}", f"habitat.simulator.sensors.{sname}.width={size}"]
    cfg = get_config("pointnav/ddppo_pointnav.yaml", ov)
    cfg.habitat.simulator.sensors.pop("semantic", None)
    trainer = baseline_registry.get_trainer(cfg.habitat_baselines.trainer_name)(cfg)
    trainer._init_train()
    try:
        assert [type(t) for t in trainer.obs_transforms] == [CubeMap2Fisheye]
        pol = trainer._agent.actor_critic
        assert [v[0] for v in pol.visual_sensors] == ["rgb", "depth"]
        obs = trainer._agent.rollouts.buffers["observations"]
        assert sorted(obs.keys()) == ["depth", "pointgoal_with_gps_compass", "rgb"]
        assert obs["rgb"].shape[-3:] == (out, out, 3) and obs["depth"].shape[-3:] == (out, out, 1)
        assert obs["rgb"].dtype == torch.uint8 and obs["depth"].dtype == torch.float32
        before = pol.engine.params_flat.clone()
        for _ in range(2):
            losses = trainer.run_update_cycle()
            assert all(np.isfinite(x) for x in losses.values()), losses
        assert trainer.num_steps_done == 2 * N * T and trainer.num_updates_done == 2
        assert float((pol.engine.params_flat - before).abs().max()) > 0
        # what the policy saw is a fisheye frame: the corners lie outside the field of view, the centre does not
        assert float(obs["rgb"][:, :, 0, 0].float().abs().max()) == 0 and float(obs["rgb"][:, :, out // 2, out // 2].float().max()) > 0
    finally:
        trainer.envs.close()
