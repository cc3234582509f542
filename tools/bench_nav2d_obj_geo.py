#!/usr/bin/env python3
"""One Nav2DObj-v0 step WITHOUT images in the geodesic distance mode (hab_nav2d_obj_step_geo: nav2d_obj_geo_step_kernel, one
wavefront per env, then nav2d_obj_geo_build_kernel for the envs whose episode ended) beside the Euclidean entry
(hab_nav2d_obj_step, one thread per env), 64 envs, 8 obstacles, at 3 and at 8 objects.  The actions are one fixed random sequence (all
six actions, a STOP now and then), so episodes end and fields are rebuilt inside the timed windows, as in a rollout.  The two entries
are warmed up and then alternated in one process; every window of INNER calls is timed with device events; the median and the range
of the windows are printed.  Two more runs separate the build kernel: hab_nav2d_obj_geo_build for all 64 envs (what a reset costs)
and with only_ended on states where no episode has just ended (the launch whose workgroups all leave at once, which every step pays).
usage: python tools/bench_nav2d_obj_geo.py [envs] [windows]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd import _lib  # noqa: E402
from habitat_amd._lib import check, ptr, stream_ptr  # noqa: E402
from habitat_amd.common.env_factory import Nav2DObjVectorEnv  # noqa: E402

INNER = 10  # calls per timed window: a single launch of a few microseconds would time the enqueue
W_SWEEPS = 65  # HAB_NAV2D_OBJ_GEO_W_SWEEPS


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
    windows = int(argv[1]) if len(argv) > 1 else 30
    assert torch.cuda.is_available(), "bench_nav2d_obj_geo needs a GPU"
    dev = "cuda"
    L = _lib.lib()
    g = torch.Generator().manual_seed(0)
    acts = torch.multinomial(torch.tensor([0.02, 0.5, 0.2, 0.2, 0.04, 0.04]), INNER * n, replacement=True, generator=g).view(INNER, n).to(dev)
    obs = {"objectgoal": torch.empty(n, 1, dtype=torch.int64, device=dev), "gps": torch.empty(n, 2, device=dev),
           "compass": torch.empty(n, 1, device=dev)}
    rew, nd = torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    K = 8
    print(f"# {n} envs, {K} obstacles, no images, {windows} windows of {INNER} calls")
    for M in (3, 8):
        # the image size only sizes the env's own buffers: no image row is handed to a step, so nothing is rendered
        kw = dict(seed=100, num_obstacles=K, turn_angle=10, max_episode_steps=500, num_objects=M, num_categories=4, device=dev)
        euc = Nav2DObjVectorEnv(n, 8, 8, **kw)
        geo = Nav2DObjVectorEnv(n, 8, 8, distance="geodesic", **kw)
        # the build alone works on the records of a geodesic env that is never stepped: a world per env, `ended` clear
        still = Nav2DObjVectorEnv(n, 8, 8, distance="geodesic", **kw)
        for e in (euc, geo, still):
            e.reset_into_obs(obs)
        stride = still._state.shape[1] * 4

        def build(only_ended):
            check(L.hab_nav2d_obj_geo_build(ptr(still._state), stride, ptr(still._geo), None, only_ended, n, K, M, stream_ptr()),
                  "obj_geo_build")

        runs = {
            "euclidean step": lambda i: euc.step_into_obs(obs, rew, nd, actions=acts[i]),
            "geodesic step": lambda i: geo.step_into_obs(obs, rew, nd, actions=acts[i]),
            "build, all envs": lambda i: build(0),
            "build, none ended": lambda i: build(1),
        }
        for _ in range(3):
            for fn in runs.values():
                timed(fn)
        times = {k: [] for k in runs}
        for _ in range(windows):
            for k, fn in runs.items():  # alternated: drift of the clocks hits all of them alike
                times[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            print(f"M={M} {k:18s} median {med[k]:8.1f} us  range [{min(v):.1f}, {max(v):.1f}] us")
        sweeps = geo._geo[:, W_SWEEPS].float()
        print(f"M={M} geodesic / euclidean step: {med['geodesic step'] / med['euclidean step']:.2f}; "
              f"sweeps of the current fields: mean {sweeps.mean().item():.1f}, max {int(sweeps.max().item())}; "
              f"lost steps of the running episodes: {int(geo._geo[:, W_SWEEPS + 1].sum().item())}")


if __name__ == "__main__":
    main()
