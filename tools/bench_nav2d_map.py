#!/usr/bin/env python3
"""The cost of the top-down map (hab_nav2d_map_update after every step entry; hab_nav2d_map_frame for the video frames) on each Nav2D
task: the task's env is built twice from its YAML through SyntheticVectorEnvFactory, once with
habitat.task.measurements.top_down_map (map_resolution S) and once without, which is the step path of an env that never heard of the
map.  Both are warmed up and then alternated in one process; every window of INNER steps is timed with device events, and the median
and the range of the windows are printed with the ratio of the medians.  `render_frames` is timed alone in the same way.  The actions
are uniform over the task's action space.  Nothing is asserted.
usage: python tools/bench_nav2d_map.py [envs=256] [S=128] [windows=30]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import SyntheticVectorEnvFactory  # noqa: E402
from habitat_amd.config.default import get_config  # noqa: E402

INNER = 10  # steps per timed window
YAMLS = ("pointnav/ppo_nav2d.yaml", "pointnav/ppo_nav2d_vel.yaml", "objectnav/ddppo_nav2d_objectnav.yaml",
         "rearrange/ddppo_nav2d_rearrange.yaml", "rearrange/ddppo_nav2d_rearrange_vel.yaml", "social_nav/ddppo_nav2d_social.yaml")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(INNER):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / INNER  # us per call


def random_actions(env, generator):
    n = env.num_envs
    if env._action_dtype == torch.int64:
        return torch.randint(0, env.num_actions, (INNER, n), generator=generator).cuda()
    return (2.0 * torch.rand(INNER, *env._actions_host.shape, generator=generator) - 1.0).cuda()


def main():
    argv = sys.argv[1:]
    n = int(argv[0]) if len(argv) > 0 else 256
    S = int(argv[1]) if len(argv) > 1 else 128
    windows = int(argv[2]) if len(argv) > 2 else 30
    assert torch.cuda.is_available(), "bench_nav2d_map needs a GPU"
    factory = SyntheticVectorEnvFactory()
    result = dict(envs=n, map_resolution=S, windows=windows, inner=INNER, tasks={})
    for yaml in YAMLS:
        base = [f"habitat_baselines.num_environments={n}"]
        plain = factory.construct_envs(get_config(yaml, base), device="cuda")
        mapped = factory.construct_envs(get_config(yaml, base + [f"habitat.task.measurements.top_down_map.map_resolution={S}"]),
                                        device="cuda")
        assert plain._map is None and mapped._map is not None
        acts = random_actions(plain, torch.Generator().manual_seed(0))
        runs = {}
        for name, env in (("without", plain), ("with", mapped)):
            env.reset_into_obs(env._own_obs())
            runs[name] = lambda i, env=env: env.step_into_obs(env._own_obs(), env._rew, env._nd, actions=acts[i])
        frames = torch.empty(n, *mapped.frame_size(), 3, dtype=torch.uint8, device="cuda")
        runs["frames"] = lambda i: mapped.render_frames(out=frames)
        for _ in range(3):  # every kernel of every run, before any window
            for fn in runs.values():
                timed(fn)
        times = {k: [] for k in runs}
        for _ in range(windows):  # alternated, so that a drift of the machine meets all three alike
            for k, fn in runs.items():
                times[k].append(timed(fn))
        row = {k: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for k, v in times.items()}
        row["ratio"] = row["with"]["median_us"] / row["without"]["median_us"]
        row["frame_shape"] = list(frames.shape)
        result["tasks"][plain._name] = row
        print(f"{plain._name:14s} image {plain.H}x{plain.W}: step {row['without']['median_us']:8.1f} us "
              f"[{row['without']['min_us']:.1f}, {row['without']['max_us']:.1f}]  with map {row['with']['median_us']:8.1f} us "
              f"[{row['with']['min_us']:.1f}, {row['with']['max_us']:.1f}]  ratio {row['ratio']:.3f}  render_frames "
              f"{row['frames']['median_us']:8.1f} us [{row['frames']['min_us']:.1f}, {row['frames']['max_us']:.1f}] for {tuple(frames.shape)}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
