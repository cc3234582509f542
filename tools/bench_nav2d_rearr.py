#!/usr/bin/env python3
"""One Nav2DRearr-v0 step (hab_nav2d_rearr_step: nav2d_rearr_step_kernel, one thread per env, then the rearrangement form of
nav2d_render_kernel) with and without images, beside the Nav2DObj-v0 entry at one object (hab_nav2d_obj_step, M = 1: the sibling
whose render also has one cylinder), 64 envs, 8 obstacles.  The images are head_depth alone and head_rgb + head_depth against depth
alone and rgb + depth (the object task's semantic image is left out: this task has none).  The actions are one fixed random sequence
over all six actions of either task (MOVE_FORWARD most often, a STOP now and then), so episodes end inside the timed windows, as in a
rollout.  All runs are warmed up and then alternated in one process; every window of INNER calls is timed with device events; the
median and the range of the windows are printed.
usage: python tools/bench_nav2d_rearr.py [envs] [size] [windows]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import Nav2DObjVectorEnv, Nav2DRearrVectorEnv  # noqa: E402

INNER = 10  # calls per timed window: a single launch of a few microseconds would time the enqueue
W_HOLDING = 64  # HAB_NAV2D_REARR_W_HOLDING


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(INNER):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / INNER  # us per call


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 64
    size = int(argv[1]) if len(argv) > 1 else 128
    windows = int(argv[2]) if len(argv) > 2 else 30
    assert torch.cuda.is_available(), "bench_nav2d_rearr needs a GPU"
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    acts = torch.multinomial(torch.tensor([0.02, 0.5, 0.15, 0.15, 0.09, 0.09]), INNER * n, replacement=True, generator=g).view(INNER, n).to(dev)
    K = 8
    kw = dict(seed=100, num_obstacles=K, turn_angle=10, max_episode_steps=500, use_rgb=True, use_depth=True, device=dev)
    rearr = {k: Nav2DRearrVectorEnv(n, size, size, **kw) for k in ("no images", "depth", "rgb + depth")}
    obj = {k: Nav2DObjVectorEnv(n, size, size, num_objects=1, num_categories=1, **kw) for k in rearr}
    rgb, depth = torch.empty(n, size, size, 3, dtype=torch.uint8, device=dev), torch.empty(n, size, size, 1, device=dev)
    vec_r = {"obj_start_sensor": torch.empty(n, 2, device=dev), "obj_goal_sensor": torch.empty(n, 2, device=dev),
             "is_holding": torch.empty(n, 1, device=dev)}
    vec_o = {"objectgoal": torch.empty(n, 1, dtype=torch.int64, device=dev), "gps": torch.empty(n, 2, device=dev),
             "compass": torch.empty(n, 1, device=dev)}
    rows_r = {"no images": vec_r, "depth": dict(vec_r, head_depth=depth), "rgb + depth": dict(vec_r, head_rgb=rgb, head_depth=depth)}
    rows_o = {"no images": vec_o, "depth": dict(vec_o, depth=depth), "rgb + depth": dict(vec_o, rgb=rgb, depth=depth)}
    rew, nd = torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    runs = {}
    for k in rearr:
        rearr[k].reset_into_obs(rows_r[k])
        obj[k].reset_into_obs(rows_o[k])
        runs[f"rearr, {k}"] = lambda i, k=k: rearr[k].step_into_obs(rows_r[k], rew, nd, actions=acts[i])
        runs[f"obj M=1, {k}"] = lambda i, k=k: obj[k].step_into_obs(rows_o[k], rew, nd, actions=acts[i])
    print(f"# {n} envs, {K} obstacles, {size} x {size}, {windows} windows of {INNER} calls")
    for _ in range(3):
        for fn in runs.values():
            timed(fn)
    times = {k: [] for k in runs}
    for _ in range(windows):
        for k, fn in runs.items():  # alternated: drift of the clocks hits all of them alike
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:24s} median {med[k]:8.1f} us  range [{min(v):.1f}, {max(v):.1f}] us")
    for k in rearr:
        print(f"{k}: rearr / obj M=1 = {med[f'rearr, {k}'] / med[f'obj M=1, {k}']:.2f}")
    held = torch.stack([e._state[:, W_HOLDING] for e in rearr.values()]).float().mean().item()
    print(f"share of envs holding the object at the end: {held:.2f}")


if __name__ == "__main__":
    main()
