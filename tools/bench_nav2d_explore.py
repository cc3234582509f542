#!/usr/bin/env python3
"""Nav2DExplore-v0's step without images (hab_nav2d_explore_step: one workgroup of 1024 threads per env sweeps the coverage layer inside
the visibility disc's bounding box, counts the new cells and, where an episode ends, clears the layer, counts its free cells and does
the first reveal) beside Nav2D-v0's step without images (hab_nav2d_step: one thread per env, nothing to sweep) at the same env count,
in one process: all are warmed up and then alternated; every window of INNER calls is timed with device events and the median and the
range of the windows are printed.  G in {32, 64, 128} and N in {16, 256}; the actions are uniform over the three moving ones, so
episodes end at the limit of 500 steps alone.  A further explore env per N has an episode limit of 8 steps at G = 64, so that one env
in eight begins an episode (a full sweep) in every call.  Nothing is asserted.
usage: python tools/bench_nav2d_explore.py [windows]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import GOAL_UUID, Nav2DExploreVectorEnv, Nav2DVectorEnv  # noqa: E402

INNER = 10  # calls per timed window
RESOLUTIONS, ENV_COUNTS = (32, 64, 128), (16, 256)


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
    assert torch.cuda.is_available(), "bench_nav2d_explore needs a GPU"
    dev = "cuda"
    kw = dict(seed=100, num_obstacles=8, max_episode_steps=500, use_rgb=False, use_depth=False, device=dev)
    g = torch.Generator().manual_seed(0)
    runs, keep = {}, []
    for n in ENV_COUNTS:
        acts = torch.randint(1, 4, (INNER, n), generator=g).to(dev)
        rew, nd = torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        nav = Nav2DVectorEnv(n, 0, 0, **kw)
        nobs = {GOAL_UUID: torch.empty(n, 2, device=dev)}
        nav.reset_into_obs(nobs)
        runs[f"nav2d          N={n:3d}"] = lambda i, e=nav, o=nobs, a=acts, r=rew, d=nd: e.step_into_obs(o, r, d, actions=a[i])
        eobs = dict(gps=torch.empty(n, 2, device=dev), compass=torch.empty(n, 1, device=dev))
        for G in RESOLUTIONS:
            env = Nav2DExploreVectorEnv(n, 0, 0, coverage_resolution=G, **kw)
            env.reset_into_obs(eobs)
            runs[f"explore G={G:3d}  N={n:3d}"] = lambda i, e=env, o=eobs, a=acts, r=rew, d=nd: e.step_into_obs(o, r, d, actions=a[i])
            keep.append(env)
        short = Nav2DExploreVectorEnv(n, 0, 0, coverage_resolution=64, **dict(kw, max_episode_steps=8))
        short.reset_into_obs(eobs)
        runs[f"explore G= 64  N={n:3d}, episodes of 8"] = lambda i, e=short, o=eobs, a=acts, r=rew, d=nd: e.step_into_obs(o, r, d, actions=a[i])
        keep += [nav, short]
    for _ in range(3):
        for fn in runs.values():
            timed(fn)
    times = {k: [] for k in runs}
    for _ in range(windows):
        for k, fn in runs.items():  # alternated: drift of the clocks hits all of them alike
            times[k].append(timed(fn))
    print(f"# step without images, 8 obstacles, visibility 3 m, {windows} windows of {INNER} calls")
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        print(f"{k:40s} median {med[k]:8.1f} us  range [{min(v):.1f}, {max(v):.1f}] us")
    for n in ENV_COUNTS:
        for G in RESOLUTIONS:
            print(f"ratio explore G={G} / nav2d, N={n}: {med[f'explore G={G:3d}  N={n:3d}'] / med[f'nav2d          N={n:3d}']:.3f}")


if __name__ == "__main__":
    main()
