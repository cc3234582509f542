#!/usr/bin/env python3
"""One call of the pick-and-place oracle (hab_nav2d_rearr_oracle: nav2d_rearr_oracle_kernel, one wavefront per env, one candidate
heading per lane) beside one Nav2DRearr-v0 step WITHOUT images in the geodesic distance mode (hab_nav2d_rearr_step_geo, the
yardstick, measured in the same process), at N = 64 and 1024 envs, 8 obstacles, 36 and 12 headings (turn_angle 10, 30).  The env
first runs 40 steps under the oracle, so the records are those of running episodes that are out of phase with one another; the
oracle is then timed on those records (it writes neither state nor field), the step with one fixed random action sequence (all six
actions, a STOP now and then, so fields are rebuilt inside the timed windows).  The two are warmed up and then alternated in one
process; every window of INNER calls is timed with device events; the median and the range of the windows are printed, and the share
of the envs in each of the kernel's three paths on the timed records.
usage: python tools/bench_nav2d_rearr_oracle.py [windows]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import Nav2DRearrVectorEnv  # noqa: E402

INNER = 10  # calls per timed window: a single launch of a few microseconds would time the enqueue
W_PX, W_OBJ, W_HOLDING = 0, 62, 64  # HAB_NAV2D_W_PX, HAB_NAV2D_REARR_W_OBJ, HAB_NAV2D_REARR_W_HOLDING
ARRIVED, UNREACHABLE = 1, 2


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(INNER):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / INNER  # us per call


def path_shares(env, status):
    """The share of the envs that ran the dot test, the forward search over DO, the place search (with the forward search over DG
    behind it where nothing was eligible), and no search at all (ARRIVED, UNREACHABLE)."""
    pos = env._state[:, [W_PX, W_PX + 1, W_OBJ, W_OBJ + 1]].view(torch.float32)
    near = ((pos[:, 2] - pos[:, 0]) ** 2 + (pos[:, 3] - pos[:, 1]) ** 2).sqrt() < 1.0
    holding = env._state[:, W_HOLDING] != 0
    none = (status == ARRIVED) | (status == UNREACHABLE)
    n = float(env.num_envs)
    return tuple(float(m.sum()) / n for m in (~none & ~holding & near, ~none & ~holding & ~near, ~none & holding, none))


def main():
    windows = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    assert torch.cuda.is_available(), "bench_nav2d_rearr_oracle needs a GPU"
    dev, K = "cuda", 8
    g = torch.Generator().manual_seed(0)
    print(f"# {K} obstacles, no images, {windows} windows of {INNER} calls, us per call: median [min, max]")
    for n in (64, 1024):
        acts = torch.multinomial(torch.tensor([0.02, 0.5, 0.15, 0.15, 0.09, 0.09]), INNER * n, replacement=True, generator=g).view(INNER, n).to(dev)
        rew, nd = torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        out, next_d, status = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        for turn in (10, 30):
            kw = dict(seed=100, num_obstacles=K, turn_angle=turn, max_episode_steps=500, use_rgb=False, use_depth=False, device=dev,
                      distance="geodesic")
            ora, geo = Nav2DRearrVectorEnv(n, 0, 0, **kw), Nav2DRearrVectorEnv(n, 0, 0, **kw)
            for e in (ora, geo):
                e.reset_into_obs({})
            for _ in range(40):
                ora.step_into_obs({}, rew, nd, actions=ora.oracle_actions(out=out))
            runs = {
                "oracle": lambda i: ora.oracle_actions(out=out, next_d=next_d, status=status),
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
            dot, fwd, place, none = path_shares(ora, status)
            print(f"N={n:4d} nh={360 // turn:3d} K={K} " + "  ".join(f"{k} {med[k]:7.1f} [{min(v):.1f}, {max(v):.1f}]" for k, v in times.items())
                  + f"  oracle / step {med['oracle'] / med['geodesic step']:.2f}  paths: dot test {100 * dot:.1f} %, forward over DO "
                  f"{100 * fwd:.1f} %, place search {100 * place:.1f} %, none {100 * none:.1f} %", flush=True)


if __name__ == "__main__":
    main()
