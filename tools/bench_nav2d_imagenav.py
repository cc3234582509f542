#!/usr/bin/env python3
"""What does Nav2DImageNav-v0's second view cost?  A step with images at 256 envs, in one process, all variants warmed up and then
alternated; every window of INNER calls is timed with device events and the median and the range of the windows are printed:

  nav2d                  hab_nav2d_step with rgb + depth (one view, the GOAL form of the render, with the marker)
  imagenav, goal NULL    hab_nav2d_imagenav_step with rgb + depth and goal_rgb NULL (one view, markerless; the second view's
                         workgroups leave at once)
  imagenav               the same with goal_rgb: both views in one launch
  imagenav, goal only    rgb and depth NULL: the second view alone
  imagenav + copy        goal NULL, then a device copy of an (N, H, W, 3) uint8 image into the goal_rgb row: what a cached goal
                         image would cost at every step, without the redraw at an episode's beginning (a lower bound of that variant)

at the sizes of SIZES.  The actions are uniform over the three moving ones, so episodes end at the limit of 500 steps alone.  The
number to read is (imagenav - imagenav, goal NULL) / (imagenav, goal NULL): the second view relative to one.  Nothing is asserted.
usage: python tools/bench_nav2d_imagenav.py [windows]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import GOAL_UUID, Nav2DImageNavVectorEnv, Nav2DVectorEnv  # noqa: E402

INNER = 10  # calls per timed window
N = 256
SIZES = ((64, 64), (128, 128))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(INNER):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / INNER  # us per call


def main():
    windows = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    assert torch.cuda.is_available(), "bench_nav2d_imagenav needs a GPU"
    dev = "cuda"
    kw = dict(seed=100, num_obstacles=8, max_episode_steps=500, device=dev)
    g = torch.Generator().manual_seed(0)
    acts = torch.randint(1, 4, (INNER, N), generator=g).to(dev)
    rew, nd = torch.empty(N, device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
    runs, keep = {}, []
    for H, W in SIZES:
        rgb, depth = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev), torch.empty(N, H, W, 1, device=dev)
        goal_rgb, cache = torch.empty_like(rgb), torch.zeros_like(rgb)
        vec = dict(gps=torch.empty(N, 2, device=dev), compass=torch.empty(N, 1, device=dev))
        nav = Nav2DVectorEnv(N, H, W, **kw)
        nobs = {"rgb": rgb, "depth": depth, GOAL_UUID: torch.empty(N, 2, device=dev)}
        nav.reset_into_obs(nobs)
        env = Nav2DImageNavVectorEnv(N, H, W, **kw)
        one, both, only = dict(vec, rgb=rgb, depth=depth), dict(vec, rgb=rgb, depth=depth, goal_rgb=goal_rgb), dict(vec, goal_rgb=goal_rgb)
        env.reset_into_obs(both)
        step = lambda e, o: (lambda i: e.step_into_obs(o, rew, nd, actions=acts[i]))
        tag = f"{H}x{W}"
        runs[f"{tag} nav2d"] = step(nav, nobs)
        runs[f"{tag} imagenav, goal NULL"] = step(env, one)
        runs[f"{tag} imagenav"] = step(env, both)
        runs[f"{tag} imagenav, goal only"] = step(env, only)
        runs[f"{tag} imagenav + copy"] = lambda i, e=env, o=one, dst=goal_rgb, src=cache: (e.step_into_obs(o, rew, nd, actions=acts[i]),
                                                                                             dst.copy_(src))
        keep += [nav, env]
    for _ in range(3):
        for fn in runs.values():
            timed(fn)
    times = {k: [] for k in runs}
    for _ in range(windows):
        for k, fn in runs.items():  # alternated: drift of the clocks hits all of them alike
            times[k].append(timed(fn))
    print(f"# step with images, {N} envs, 8 obstacles, {windows} windows of {INNER} calls")
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        print(f"{k:32s} median {med[k]:8.1f} us  range [{min(v):.1f}, {max(v):.1f}] us")
    for H, W in SIZES:
        t = f"{H}x{W}"
        one, both = med[f"{t} imagenav, goal NULL"], med[f"{t} imagenav"]
        print(f"{t}: second view / one view = {(both - one) / one:.3f}; imagenav / nav2d = {both / med[f'{t} nav2d']:.3f}; "
              f"copy variant / one view = {(med[f'{t} imagenav + copy'] - one) / one:.3f}")


if __name__ == "__main__":
    main()
