#!/usr/bin/env python3
"""Nav2DSocial-v0's step (hab_nav2d_social_step: one wavefront per env, the person's hop as an arg-min over the graph, a field rebuilt
inside the step whenever a waypoint is reached) beside Nav2DVel-v0's (hab_nav2d_vel_step: one thread per env) at the same shape, in
one process, as tools/bench_nav2d.py --vel does: both are warmed up and then alternated; every window of INNER calls is timed with
device events and the median and the range of the windows are printed.  The pair is run with images (head_depth beside depth, the
render kernel shared) and without (the step and build kernels alone).  A third social env has an episode limit of 8 steps, so that
every call ends episodes and the build kernel's launch, which otherwise leaves at once, rebuilds a field for one env in eight.  The
actions are uniform in [-0.9, 1] x [-1, 1].  The counts of arrivals, rebuilds and waits over the timed windows are printed too.
Nothing is asserted.
usage: python tools/bench_nav2d_social.py [envs] [size] [windows]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import GOAL_UUID, Nav2DSocialVectorEnv, Nav2DVelVectorEnv  # noqa: E402

INNER = 10  # calls per timed window
W_ARRIVALS, W_WAITS, W_REBUILDS, W_EPISODE = 66, 67, 70, 10  # HAB_NAV2D_SOCIAL_W_*, HAB_NAV2D_W_EPISODE


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
    size = int(argv[1]) if len(argv) > 1 else 64
    windows = int(argv[2]) if len(argv) > 2 else 30
    assert torch.cuda.is_available(), "bench_nav2d_social needs a GPU"
    dev = "cuda"
    kw = dict(seed=100, num_obstacles=8, max_episode_steps=500, device=dev)
    vel = Nav2DVelVectorEnv(n, size, size, use_rgb=False, **kw)
    vel0 = Nav2DVelVectorEnv(n, 0, 0, use_rgb=False, use_depth=False, **kw)
    soc = Nav2DSocialVectorEnv(n, size, size, **kw)
    soc0 = Nav2DSocialVectorEnv(n, 0, 0, use_depth=False, **kw)
    short = Nav2DSocialVectorEnv(n, 0, 0, use_depth=False, **dict(kw, max_episode_steps=8))
    depth = torch.empty(n, size, size, 1, device=dev)
    vobs = {"depth": depth, GOAL_UUID: torch.empty(n, 2, device=dev)}
    sobs = {"head_depth": depth, "person_sensor": torch.empty(n, 2, device=dev), "person_visible": torch.empty(n, 1, device=dev)}
    vobs0, sobs0 = {GOAL_UUID: vobs[GOAL_UUID]}, {k: v for k, v in sobs.items() if k != "head_depth"}
    rew, nd = torch.empty(n, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    g = torch.Generator().manual_seed(0)
    lo = torch.tensor([-0.9, -1.0])
    acts = (lo + (1.0 - lo) * torch.rand(INNER, n, 2, generator=g)).to(dev)
    runs = {"nav2dvel step+render": lambda i: vel.step_into_obs(vobs, rew, nd, actions=acts[i]),
            "nav2dsocial step+render": lambda i: soc.step_into_obs(sobs, rew, nd, actions=acts[i]),
            "nav2dvel step only": lambda i: vel0.step_into_obs(vobs0, rew, nd, actions=acts[i]),
            "nav2dsocial step only": lambda i: soc0.step_into_obs(sobs0, rew, nd, actions=acts[i]),
            "nav2dsocial, episodes of 8": lambda i: short.step_into_obs(sobs0, rew, nd, actions=acts[i])}
    vel.reset_into_obs(vobs)
    vel0.reset_into_obs(vobs0)
    soc.reset_into_obs(sobs)
    for e in (soc0, short):
        e.reset_into_obs(sobs0)
    for _ in range(3):
        for fn in runs.values():
            timed(fn)
    times = {k: [] for k in runs}
    for _ in range(windows):
        for k, fn in runs.items():  # alternated: drift of the clocks hits all of them alike
            times[k].append(timed(fn))
    st = soc0._state.cpu()
    events = dict(arrivals=int(st[:, W_ARRIVALS].sum()), rebuilds=int(st[:, W_REBUILDS].sum()), waits=int(st[:, W_WAITS].sum()),
                  episodes=int(st[:, W_EPISODE].sum()), short_episodes=int(short._state[:, W_EPISODE].sum()))
    print(f"# {n} envs, {size}x{size} depth, 8 obstacles, {windows} windows of {INNER} calls")
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        print(f"{k:28s} median {med[k]:8.1f} us  range [{min(v):.1f}, {max(v):.1f}] us")
    print(f"ratio nav2dsocial / nav2dvel, step+render: {med['nav2dsocial step+render'] / med['nav2dvel step+render']:.3f}")
    print(f"ratio nav2dsocial / nav2dvel, step only: {med['nav2dsocial step only'] / med['nav2dvel step only']:.3f}")
    print(f"ratio episodes of 8 / episodes of 500, step only: {med['nav2dsocial, episodes of 8'] / med['nav2dsocial step only']:.3f}")
    print("of the running episodes of the step-only env (arrivals, rebuilds, waits) and episodes begun:", events)


if __name__ == "__main__":
    main()
