#!/usr/bin/env python3
"""What a competent agent scores on Nav2DRearr-v0 under the task's own rules: the pick-and-place oracle
(habitat_amd/common/rearrange_oracle.py) run on the device path of the task from config/rearrange/ddppo_nav2d_rearrange_geodesic.yaml
(3 obstacles, 10 degrees), without images, with `start_holding` off and on, and at 8 obstacles and 30 degrees.  One JSON line per
row: the means of success, did_pick_object, object_to_goal_distance and collisions over the episodes that ended, the counts
episodes, unreachable (walled-off places, given up at once), stuck, steps, and steps_per_episode.  These are the oracle rows beside
a learning run's `success`.
usage: python tools/nav2d_rearr_oracle_eval.py [episodes] [envs] [further config overrides ...]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd.common.env_factory import SyntheticVectorEnvFactory  # noqa: E402
from habitat_amd.common.rearrange_oracle import RearrangeOracle  # noqa: E402
from habitat_amd.config.default import get_config  # noqa: E402

YAML = "rearrange/ddppo_nav2d_rearrange_geodesic.yaml"
COARSE = ("habitat.synthetic.num_obstacles=8", "habitat.synthetic.turn_angle=30")
ROWS = ((), ("habitat.synthetic.start_holding=True",), COARSE, COARSE + ("habitat.synthetic.start_holding=True",))


def main():
    argv = sys.argv[1:]
    episodes = int(argv[0]) if len(argv) > 0 else 2000
    envs = int(argv[1]) if len(argv) > 1 else 256
    assert torch.cuda.is_available(), "nav2d_rearr_oracle_eval needs a GPU"
    for extra in ROWS:
        cfg = get_config(YAML, [f"habitat_baselines.num_environments={envs}", *extra, *argv[2:]])
        env = SyntheticVectorEnvFactory(use_rgb=False, use_depth=False).construct_envs(cfg, device="cuda")
        out = RearrangeOracle(env).evaluate(episodes)
        out["steps_per_episode"] = out["steps"] / out["episodes"]
        print(json.dumps(dict(task="Nav2DRearr-v0", config=YAML, num_obstacles=env.num_obstacles, turn_angle=env.turn_angle,
                              start_holding=env.start_holding, envs=envs,
                              **{k: (round(v, 6) if isinstance(v, float) else v) for k, v in out.items()})), flush=True)


if __name__ == "__main__":
    main()
