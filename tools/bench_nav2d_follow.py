#!/usr/bin/env python3
"""One call of the shortest-path follower (hab_nav2d_follow: nav2d_follow_kernel, one wavefront per env, one candidate heading per
lane) beside one Nav2D-v0 step WITHOUT images in the geodesic distance mode (hab_nav2d_step_geo, the yardstick: it runs ONE
geodesic query per env, the follower one per free candidate heading), at N = 64 and 1024 envs, 12, 36 and 360 headings (turn_angle
30, 10, 1) and 3 and 8 obstacles.  The env first runs 10 steps under the follower, so the records are those of running episodes;
the follower is then timed on those records (it writes neither state nor field), the step with one fixed random action sequence
(all four actions, a STOP now and then, so fields are rebuilt inside the timed windows).  The two are warmed up and then alternated
in one process; every window of INNER calls is timed with device events; the median and the range of the windows are printed.
usage: python tools/bench_nav2d_follow.py [windows]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import Nav2DVectorEnv  # noqa: E402

INNER = 10  # calls per timed window: a single launch of a few microseconds would time the enqueue


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
    assert torch.cuda.is_available(), "bench_nav2d_follow needs a GPU"
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    print(f"# no images, {windows} windows of {INNER} calls, us per call: median [min, max]")
    for n in (64, 1024):
        acts = torch.multinomial(torch.tensor([0.02, 0.58, 0.2, 0.2]), INNER * n, replacement=True, generator=g).view(INNER, n).to(dev)
        rew, nd = torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        out, next_d, status = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        for turn in (30, 10, 1):
            for K in (3, 8):
                kw = dict(seed=100, num_obstacles=K, turn_angle=turn, max_episode_steps=500, device=dev, distance="geodesic")
                fol, geo = Nav2DVectorEnv(n, 0, 0, use_rgb=False, use_depth=False, **kw), Nav2DVectorEnv(n, 0, 0, use_rgb=False, use_depth=False, **kw)
                for e in (fol, geo):
                    e.reset_into_obs({})
                for _ in range(10):
                    fol.step_into_obs({}, rew, nd, actions=fol.follower_actions(out=out))
                runs = {
                    "follower": lambda i: fol.follower_actions(out=out, next_d=next_d, status=status),
                    "geodesic step": lambda i: geo.step_into_obs({}, rew, nd, actions=acts[i]),
                }
                for _ in range(3):
                    for fn in runs.values():
                        timed(fn)
                times = {k: [] for k in runs}
                for _ in range(windows):
                    for k, fn in runs.items():  # alternated: drift of the clocks hits both alike
                        times[k].append(timed(fn))
                med = {k: statistics.median(v) for k, v in times.items()}
                going = int((status == 0).sum().item())
                print(f"N={n:4d} nh={360 // turn:3d} K={K} " + "  ".join(f"{k} {med[k]:7.1f} [{min(v):.1f}, {max(v):.1f}]" for k, v in times.items())
                      + f"  follower / step {med['follower'] / med['geodesic step']:.2f}  (GO in {going} of {n} envs)")


if __name__ == "__main__":
    main()
