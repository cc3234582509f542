"""`hab_obs_resize_crop` on the device: every kernel form (packed uint8 rgb, LDS tile, generic grid-stride) at the shapes of
tests/resize_crop_reference.py::CASES, bitwise against the plain reference (itself pinned to ATen on the CPU by
tests/test_resize_crop_reference.py), with the form that ran asserted through `hab_obs_resize_crop_form`; the `out=` destination,
the branches of `apply_obs_transforms_batch`, the refusals, and the HAB_OBS_NO_TILE / HAB_OBS_NO_RGB8 switches in a fresh process.
Comparisons are `torch.equal`: there is no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from resize_crop_reference import (AREA, AREA_CASES, CASES, FORMS, NEAREST, SLOW_REFERENCE, area_ref, make_input, random_input,
                                   reference, window_of)
from test_resize_crop_reference import DTYPE_CODE, aten_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(name):
    return torch.tensor(np.asarray(make_input(name)))


def _want(name):
    """The plain reference; ATen's CPU result for the one case whose plain reference takes seconds (the CPU test compares the two)."""
    if name in SLOW_REFERENCE:
        _, _, (rh, rw), _, mode, _ = CASES[name]
        return aten_ref(make_input(name), rh, rw, window_of(name), mode)
    return torch.tensor(np.asarray(reference(name)))


def _form(dev, name):
    from habitat_amd import _lib
    dtype, (n, h, w, c), (rh, rw), _, mode, _ = CASES[name]
    assert dev.is_contiguous()
    return _lib.lib().hab_obs_resize_crop_form(_lib.ptr(dev), DTYPE_CODE[dtype], n, h, w, c, rh, rw, mode)


def _run_case(name, want_form):
    from habitat_amd.common.obs_transformers import resize_crop
    _, _, resized, _, mode, _ = CASES[name]
    x = _host(name)
    dev = x.cuda()
    assert _form(dev, name) == FORMS[want_form], (name, "kernel form", _form(dev, name), want_form)
    got = resize_crop(dev, resized, window_of(name), mode)
    torch.cuda.synchronize()
    want = _want(name)
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    bad = got.cpu() != want
    assert not bool(bad.any()), (name, want_form, int(bad.sum()), bad.nonzero()[:8].tolist())
    assert torch.equal(dev.cpu(), x), (name, "the source was modified")


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_forms_vs_plain_reference(name):
    _run_case(name, CASES[name][5])


@pytest.mark.parametrize("name", ["rgb8_kw4_crop", "u8c3_tile_ragged", "f32c1_tile_multi", "u8c3_oddpitch", "near_scale_mixed"])
def test_out_destination_is_written_completely_and_only(name):
    """`out=` is a row of a larger contiguous buffer (a rollout-storage row).  With two different pre-fills the row equals the
    reference both times, so every element of it was written, and the rows before and after it keep the pre-fill."""
    from habitat_amd.common.obs_transformers import resize_crop
    _, _, resized, _, mode, _ = CASES[name]
    dev, want = _host(name).cuda(), _want(name)
    for fill in (0, 97):
        buf = torch.full((3, *want.shape), fill, dtype=want.dtype, device="cuda")
        res = resize_crop(dev, resized, window_of(name), mode, out=buf[1])
        torch.cuda.synchronize()
        assert res.data_ptr() == buf[1].data_ptr()
        assert torch.equal(buf[1].cpu(), want), (name, fill)
        assert bool((buf[0] == fill).all()) and bool((buf[2] == fill).all()), (name, fill, "a neighbouring row was written")


def test_transformer_branches_in_one_call():
    """ResizeShortestEdge(rgb, depth) then CenterCropper(rgb, semantic): rgb is fused, depth is resized only, semantic is cropped only
    (the "not fusable for this sensor" branch), the vector passes through."""
    from habitat_amd.common.obs_transformers import CenterCropper, ResizeShortestEdge, apply_obs_transforms_batch
    n, h, w, size, crop = 2, 40, 56, 20, (16, 18)
    host = {"rgb": random_input("u8", (n, h, w, 3), 11), "depth": random_input("f32", (n, h, w, 1), 12),
            "semantic": random_input("i32", (n, h, w, 1), 13)}
    batch = {k: torch.tensor(v).cuda() for k, v in host.items()}
    batch["gps"] = torch.arange(2.0 * n, device="cuda").reshape(n, 2)
    ts = [ResizeShortestEdge(size, trans_keys=("rgb", "depth")), CenterCropper(crop, trans_keys=("rgb", "semantic"))]
    out = apply_obs_transforms_batch(dict(batch), ts)
    torch.cuda.synchronize()
    rh, rw = 20, 28                                  # int(40 * 20 / 40), int(56 * 20 / 40)
    want = {"rgb": area_ref(host["rgb"], rh, rw, (rh // 2 - 8, rw // 2 - 9, *crop)),
            "depth": area_ref(host["depth"], rh, rw, (0, 0, rh, rw)),
            "semantic": host["semantic"][:, h // 2 - 8:h // 2 + 8, w // 2 - 9:w // 2 + 9]}
    assert sorted(out) == ["depth", "gps", "rgb", "semantic"] and out["gps"] is batch["gps"]
    for k, v in want.items():
        assert out[k].dtype == batch[k].dtype and tuple(out[k].shape) == v.shape, (k, out[k].shape, v.shape)
        assert np.array_equal(out[k].cpu().numpy(), v), k
        assert np.array_equal(batch[k].cpu().numpy(), host[k]), (k, "the source was modified")
    # the two transformers one after the other give the same
    seq = ts[1](ts[0](dict(batch)))
    assert all(torch.equal(seq[k], out[k]) for k in want)


def test_refusals_are_loud_and_leave_the_destination_untouched():
    from habitat_amd import _lib
    from habitat_amd.common.obs_transformers import CenterCropper, ResizeShortestEdge, apply_obs_transforms_batch, resize_crop
    n, h, w = 2, 40, 56
    rgb = torch.tensor(random_input("u8", (n, h, w, 3), 21)).cuda()
    keep = rgb.clone()
    # a crop larger than the image: the reference's slice would silently return a smaller image
    batch = {"rgb": rgb}
    with pytest.raises(_lib.HabError):
        CenterCropper((50, 18), trans_keys=("rgb",))(batch)
    assert batch["rgb"] is rgb
    with pytest.raises(_lib.HabError):  # 40 x 56 -> 20 x 28, then a 30-row crop
        apply_obs_transforms_batch(batch, [ResizeShortestEdge(20, trans_keys=("rgb",)), CenterCropper((30, 18), trans_keys=("rgb",))])
    assert batch["rgb"] is rgb
    out = torch.full((n, 50, 18, 3), 97, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.HabError):
        resize_crop(rgb, (h, w), (-5, 19, 50, 18), NEAREST, out=out)
    assert bool((out == 97).all())
    # five channels, either mode; a mode that does not exist
    five = torch.tensor(random_input("u8", (1, 8, 8, 5), 22)).cuda()
    out5 = torch.full((1, 4, 4, 5), 97, dtype=torch.uint8, device="cuda")
    for mode in (AREA, NEAREST):
        with pytest.raises(_lib.HabError):
            resize_crop(five, (4, 4), (0, 0, 4, 4), mode, out=out5)
    out3 = torch.full((n, 20, 28, 3), 97, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.HabError):
        resize_crop(rgb, (20, 28), (0, 0, 20, 28), 2, out=out3)
    torch.cuda.synchronize()
    assert bool((out5 == 97).all()) and bool((out3 == 97).all()) and torch.equal(rgb, keep)
    # ... and the device still works
    assert torch.equal(resize_crop(rgb, (h, w), (0, 0, h, w), NEAREST), keep)


def switch_child():
    """Runs in a fresh process with HAB_OBS_NO_TILE=1 HAB_OBS_NO_RGB8=1: every area case but the large one takes the generic kernel
    and gives the plain reference's bits."""
    assert os.environ.get("HAB_OBS_NO_TILE") and os.environ.get("HAB_OBS_NO_RGB8")
    done = 0
    for name in AREA_CASES:
        if name in SLOW_REFERENCE:
            continue
        _run_case(name, "generic")
        done += 1
    print(f"SWITCHES_OK {done}")


def test_switches_send_every_area_case_to_the_generic_kernel():
    """HAB_OBS_NO_TILE / HAB_OBS_NO_RGB8 are read once per process, so one fresh child.  The only place the generic kernel meets 3- and
    4-channel tiles, wide fp32 windows and packed rgb; with the form test it also shows that the three kernels agree."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "habitat-lab_amd"), os.path.join(ROOT, "tests")]),
               HAB_OBS_NO_TILE="1", HAB_OBS_NO_RGB8="1")
    out = subprocess.run([sys.executable, "-c", "import test_gpu_resize_crop as t; t.switch_child()"], env=env, capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("SWITCHES_OK")]
    assert lines and int(lines[-1].split()[1]) == len(AREA_CASES) - len(SLOW_REFERENCE) == 18, out.stdout[-2000:]
