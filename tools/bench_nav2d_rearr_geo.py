#!/usr/bin/env python3
"""One step of Nav2DRearr-v0 and of Nav2DRearrVel-v0 without images, the Euclidean entry (hab_nav2d_rearr_step /
hab_nav2d_rearr_vel_step: one thread per env) beside the geodesic entry (hab_nav2d_rearr_step_geo / hab_nav2d_rearr_vel_step_geo:
nav2d_rearr_geo_step_kernel, one wavefront per env, a successful PLACE rebuilding the object's field inside it, then
nav2d_rearr_geo_build_kernel for the envs whose episode ended) in the same run, at N = 64 and N = 1024, 8 obstacles, turn_angle 10.
The actions are one fixed random sequence per task -- all six actions with MOVE_FORWARD most often and a STOP now and then; velocity
rows with the grip closed or open at random -- so episodes end and objects are put down inside the timed windows, as in a rollout.
All runs are warmed up and then alternated in one process; every window of INNER calls is timed with device events; the median and the
range of the windows are printed, and from an untimed replay of the same sequence the share of env-steps that rebuilt a field: at a
PLACE, inside the step, and at an episode's end, in the build launch.
usage: python tools/bench_nav2d_rearr_geo.py [windows]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import Nav2DRearrVectorEnv, Nav2DRearrVelVectorEnv  # noqa: E402

INNER = 10  # calls per timed window: a single launch of a few microseconds would time the enqueue
W_ENDED, W_HOLDING = 11, 64  # HAB_NAV2D_W_ENDED, HAB_NAV2D_REARR_W_HOLDING


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
    assert torch.cuda.is_available(), "bench_nav2d_rearr_geo needs a GPU"
    dev, K = "cuda", 8
    g = torch.Generator().manual_seed(0)
    runs, shares = {}, {}
    for n in (64, 1024):
        acts = torch.multinomial(torch.tensor([0.02, 0.5, 0.15, 0.15, 0.09, 0.09]), INNER * n, replacement=True, generator=g).view(INNER, n)
        vacts = torch.rand(INNER, n, 3, generator=g) * 2.5 - 1.25
        vacts[..., 0] = torch.where(acts == 0, torch.full((INNER, n), -1.0), vacts[..., 0].abs())  # stops where the other task has STOP
        vacts[..., 1] = torch.where(vacts[..., 0] < 0, torch.zeros(INNER, n), vacts[..., 1])
        acts, vacts = acts.to(dev), vacts.to(dev).contiguous()
        kw = dict(seed=100, num_obstacles=K, turn_angle=10, max_episode_steps=500, use_rgb=False, use_depth=False, device=dev)
        rows = {"obj_start_sensor": torch.empty(n, 2, device=dev), "obj_goal_sensor": torch.empty(n, 2, device=dev),
                "is_holding": torch.empty(n, 1, device=dev)}
        rew, nd = torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        for task, cls, a, more in (("rearr", Nav2DRearrVectorEnv, acts, {}),
                                   ("rearr vel", Nav2DRearrVelVectorEnv, vacts, dict(max_turn_angle=30, min_abs_ang_speed=10))):
            for distance in ("euclidean", "geodesic"):
                env = cls(n, 0, 0, distance=distance, **kw, **more)
                env.reset_into_obs(rows)
                runs[f"{task}, N = {n}, {distance}"] = lambda i, env=env, a=a, rows=rows, rew=rew, nd=nd: env.step_into_obs(rows, rew, nd, actions=a[i])
            # the share of env-steps with a rebuild, from an untimed replay of what the timed windows will run
            env = cls(n, 0, 0, distance="geodesic", **kw, **more)
            env.reset_into_obs(rows)
            placed = ended = 0
            steps = INNER * (3 + windows)
            for s in range(steps):
                before = env._state[:, W_HOLDING].clone()
                env.step_into_obs(rows, rew, nd, actions=a[s % INNER])
                over = env._state[:, W_ENDED] != 0
                placed += int(((before == 1) & (env._state[:, W_HOLDING] == 0) & ~over).sum())
                ended += int(over.sum())
            shares[f"{task}, N = {n}"] = (placed / (steps * n), ended / (steps * n))
    print(f"# {K} obstacles, no images, {windows} windows of {INNER} calls")
    for _ in range(3):
        for fn in runs.values():
            timed(fn)
    times = {k: [] for k in runs}
    for _ in range(windows):
        for k, fn in runs.items():  # alternated: drift of the clocks hits all of them alike
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        n = int(k.split("N = ")[1].split(",")[0])
        print(f"{k:34s} median {med[k]:8.1f} us  range [{min(v):.1f}, {max(v):.1f}] us  {n / med[k] * 1e6:12.0f} env-steps/s")
    for k, (placed, ended) in shares.items():
        print(f"{k}: geodesic / euclidean = {med[k + ', geodesic'] / med[k + ', euclidean']:.2f}; env-steps that rebuilt the object's field "
              f"at a PLACE {100 * placed:.2f} %, that ended an episode (both fields built) {100 * ended:.2f} %")


if __name__ == "__main__":
    main()
