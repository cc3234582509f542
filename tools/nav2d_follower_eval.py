#!/usr/bin/env python3
"""What a perfect agent scores on the Nav2D point-goal worlds: the shortest-path follower (habitat_amd/common/
shortest_path_follower.py) run on the device path of Nav2D-v0 from config/pointnav/ppo_nav2d_geodesic.yaml and of Nav2DVel-v0 from
config/pointnav/ppo_nav2d_vel.yaml with `habitat.synthetic.distance_to_goal=geodesic`, without images.  One JSON line per task: the
means of success, spl, distance_to_goal and collisions over the episodes that ended, and the counts episodes, unreachable (walled-off
goals, given up at once), stuck, steps.  These are the oracle rows beside a learning run's `success` and `spl`.
usage: python tools/nav2d_follower_eval.py [episodes] [envs] [further config overrides ...]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import SyntheticVectorEnvFactory  # noqa: E402
from habitat_amd.common.shortest_path_follower import ShortestPathFollower  # noqa: E402
from habitat_amd.config.default import get_config  # noqa: E402

TASKS = (("Nav2D-v0", "pointnav/ppo_nav2d_geodesic.yaml", ()),
         ("Nav2DVel-v0", "pointnav/ppo_nav2d_vel.yaml", ("habitat.synthetic.distance_to_goal=geodesic",)))


def main():
    argv = sys.argv[1:]
    episodes = int(argv[0]) if len(argv) > 0 else 2000
    envs = int(argv[1]) if len(argv) > 1 else 256
    assert torch.cuda.is_available(), "nav2d_follower_eval needs a GPU"
    for task, yaml, extra in TASKS:
        cfg = get_config(yaml, [f"habitat_baselines.num_environments={envs}", *extra, *argv[2:]])
        env = SyntheticVectorEnvFactory(use_rgb=False, use_depth=False).construct_envs(cfg, device="cuda")
        out = ShortestPathFollower(env).evaluate(episodes)
        syn = cfg.habitat.synthetic
        print(json.dumps(dict(task=task, config=yaml, num_obstacles=env.num_obstacles, turn_angle=env.turn_angle,
                              max_turn_angle=getattr(syn, "max_turn_angle", None), envs=envs,
                              **{k: (round(v, 6) if isinstance(v, float) else v) for k, v in out.items()})))


if __name__ == "__main__":
    main()
