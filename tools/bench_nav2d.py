#!/usr/bin/env python3
"""Nav2D-v0 step + render (hab_nav2d_step: 64 envs, 256x256 rgb u8 + depth f32, 8 obstacles) beside hab_synth_step at the same shape.
hab_synth_step is a pure store kernel that writes the same bytes (a hash per word, nothing read), so it is the yardstick for a render
that is meant to be store-bound.  Both are warmed up and then alternated in one process; every window of INNER calls is timed with
device events and the median and the range of the windows are printed, with the bytes written per second.  The Nav2D actions are a
fixed random sequence (all four actions), so episodes end and worlds are regenerated inside the timed windows, as in a rollout; the
reset (advance = 0) is timed separately.
With --vel the pair is instead Nav2DVel-v0 (hab_nav2d_vel_step, turn_angle 1: a 360-heading ray table) beside hab_nav2d_step at the same
shape: the render kernel is shared, so the medians are expected to agree within the spread of the windows.  Its actions are uniform in
[-0.9, 1] x [-1, 1], which stops about as often as the discrete sequence does.  Three more runs separate the parts: the velocity task
on 36 headings (the discrete task's ray table size) and both step kernels without images.
With --obj the runs are Nav2DObj-v0 (hab_nav2d_obj_step, 8 obstacles, 8 objects of 4 categories, six actions) with and without the
`semantic` plane (11 against 7 bytes per pixel), beside hab_nav2d_step: the same render kernel in its object form.
usage: python tools/bench_nav2d.py [--vel | --obj] [envs] [size] [windows]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import (GOAL_UUID, Nav2DObjVectorEnv, Nav2DVectorEnv, Nav2DVelVectorEnv,  # noqa: E402
                                            SyntheticVectorEnv)

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
    argv = [a for a in sys.argv[1:] if a not in ("--vel", "--obj")]
    vel, objects = "--vel" in sys.argv[1:], "--obj" in sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 64
    size = int(argv[1]) if len(argv) > 1 else 256
    windows = int(argv[2]) if len(argv) > 2 else 30
    assert torch.cuda.is_available(), "bench_nav2d needs a GPU"
    dev = "cuda"
    nav = Nav2DVectorEnv(n, size, size, seed=100, num_obstacles=8, turn_angle=10, max_episode_steps=500, device=dev)
    syn = SyntheticVectorEnv(n, size, size, seed=100, device=dev)
    obs = {"rgb": torch.empty(n, size, size, 3, dtype=torch.uint8, device=dev), "depth": torch.empty(n, size, size, 1, device=dev),
           GOAL_UUID: torch.empty(n, 2, device=dev)}
    rew, nd = torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(0)
    # mostly moving actions, a STOP now and then: episodes of a few dozen steps
    acts = torch.multinomial(torch.tensor([0.02, 0.58, 0.2, 0.2]), INNER * n, replacement=True, generator=g).view(INNER, n).to(dev)
    runs = {
        "nav2d step+render": lambda i: nav.step_into_obs(obs, rew, nd, actions=acts[i]),
        "nav2d reset+render": lambda i: nav.reset_into_obs(obs),
        "hab_synth_step": lambda i: syn.step_into_obs(obs, rew, nd),
    }
    if vel:
        kw = dict(seed=100, num_obstacles=8, max_episode_steps=500, device=dev)
        nvel = Nav2DVelVectorEnv(n, size, size, **kw)
        # the same task on Nav2D-v0's 36 headings (M = S = 1), and both steps without images: what the ray table and the step cost
        nvel36 = Nav2DVelVectorEnv(n, size, size, turn_angle=10, max_turn_angle=10, min_abs_ang_speed=10, **kw)
        nav0 = Nav2DVectorEnv(n, 0, 0, use_rgb=False, use_depth=False, turn_angle=10, **kw)
        nvel0 = Nav2DVelVectorEnv(n, 0, 0, use_rgb=False, use_depth=False, **kw)
        goal = {GOAL_UUID: obs[GOAL_UUID]}
        lo = torch.tensor([-0.9, -1.0])
        vacts = (lo + (1.0 - lo) * torch.rand(INNER, n, 2, generator=g)).to(dev)
        runs = {"nav2d step+render": runs["nav2d step+render"],
                "nav2dvel step+render": lambda i: nvel.step_into_obs(obs, rew, nd, actions=vacts[i]),
                "nav2dvel, 36 headings": lambda i: nvel36.step_into_obs(obs, rew, nd, actions=vacts[i]),
                "nav2d step only": lambda i: nav0.step_into_obs(goal, rew, nd, actions=acts[i]),
                "nav2dvel step only": lambda i: nvel0.step_into_obs(goal, rew, nd, actions=vacts[i])}
        for e in (nvel, nvel36):
            e.reset_into_obs(obs)
        for e in (nav0, nvel0):
            e.reset_into_obs(goal)
    if objects:
        nobj = Nav2DObjVectorEnv(n, size, size, seed=100, num_obstacles=8, turn_angle=10, max_episode_steps=500, num_objects=8,
                                 num_categories=4, num_actions=6, device=dev)
        oobs = {"rgb": obs["rgb"], "depth": obs["depth"], "semantic": torch.empty(n, size, size, 1, dtype=torch.int32, device=dev),
                "objectgoal": torch.empty(n, 1, dtype=torch.int64, device=dev), "gps": torch.empty(n, 2, device=dev),
                "compass": torch.empty(n, 1, device=dev)}
        no_sem = {k: v for k, v in oobs.items() if k != "semantic"}
        oacts = torch.multinomial(torch.tensor([0.02, 0.5, 0.2, 0.2, 0.04, 0.04]), INNER * n, replacement=True,
                                  generator=g).view(INNER, n).to(dev)
        runs = {"nav2d step+render": runs["nav2d step+render"],
                "nav2dobj with semantic": lambda i: nobj.step_into_obs(oobs, rew, nd, actions=oacts[i]),
                "nav2dobj without": lambda i: nobj.step_into_obs(no_sem, rew, nd, actions=oacts[i])}
        nobj.reset_into_obs(oobs)
    nav.reset_into_obs(obs)
    syn.reset_into_obs(obs)
    for _ in range(3):
        for fn in runs.values():
            timed(fn)
    times = {k: [] for k in runs}
    for _ in range(windows):
        for k, fn in runs.items():  # alternated: drift of the clocks hits all of them alike
            times[k].append(timed(fn))
    nbytes = n * size * size * 7
    print(f"# {n} envs, {size}x{size} rgb + depth, {nbytes / 1e6:.1f} MB written per call, {windows} windows of {INNER} calls")
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        print(f"{k:22s} median {med[k]:8.1f} us  range [{min(v):.1f}, {max(v):.1f}] us  {nbytes / med[k] / 1e3:7.1f} GB/s written")
    if objects:
        print("bytes per pixel: 11 with semantic, 7 without (the GB/s column counts 7 for every row)")
        print(f"ratio nav2dobj with semantic / without: {med['nav2dobj with semantic'] / med['nav2dobj without']:.3f}")
        print(f"ratio nav2dobj without semantic / nav2d step+render: {med['nav2dobj without'] / med['nav2d step+render']:.3f}")
    elif vel:
        print(f"ratio nav2dvel step+render / nav2d step+render: {med['nav2dvel step+render'] / med['nav2d step+render']:.3f}")
    else:
        print(f"ratio nav2d step+render / hab_synth_step: {med['nav2d step+render'] / med['hab_synth_step']:.2f}")


if __name__ == "__main__":
    main()
