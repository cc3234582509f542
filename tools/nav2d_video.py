#!/usr/bin/env python3
"""Episode videos of a Nav2D task without a checkpoint: the envs of a config are stepped by a random agent or by the task's teacher
(`expert_actions`: the shortest-path follower of Nav2D-v0, the pick-and-place oracle of Nav2DRearr-v0, both in the geodesic distance
mode) and every finished episode is written as the evaluator writes it (habitat_amd/rl/ppo/evaluator.py: write_episode_video), one
file `episode={id}-ckpt=0-{measure}={value}...` per episode: observation, depth, and the top-down map with the trajectory and the fog
of war.  The measurement `habitat.task.measurements.top_down_map` is added where the config has none.
usage: python tools/nav2d_video.py --config pointnav/dagger_nav2d_geodesic.yaml --agent teacher --episodes 4 --out videos
       [--envs 4] [--height 128] [--fps 10] [overrides ...]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
from habitat_amd import _lib  # noqa: E402
from habitat_amd.common.env_factory import SyntheticVectorEnvFactory  # noqa: E402
from habitat_amd.config.default import Config, get_config  # noqa: E402
from habitat_amd.rl.ppo.evaluator import write_episode_video  # noqa: E402


def random_actions(env, generator):
    if env._action_dtype == torch.int64:
        # STOP a tenth as often as it would be drawn, so that a random episode shows some of the world
        p = torch.ones(env.num_actions)
        p[0] = 0.1
        return torch.multinomial(p, env.num_envs, replacement=True, generator=generator).cuda()
    return (2.0 * torch.rand(*env._actions_host.shape, generator=generator) - 1.0).cuda()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--agent", choices=("random", "teacher"), default="random")
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--out", required=True)
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--fps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args(argv)
    cfg = get_config(args.config, [f"habitat_baselines.num_environments={args.envs}"] + args.overrides)
    if not str(cfg.habitat.task.type).lower().startswith("nav2d"):
        raise _lib.HabError(f"nav2d_video: {args.config} is no Nav2D task ({cfg.habitat.task.type}); only those have a world to draw")
    if getattr(cfg.habitat.task.measurements, "top_down_map", None) is None:
        cfg.habitat.task.measurements["top_down_map"] = Config()
    # the config's own switches of the synthetic factory (use_rgb, use_depth), where it names that factory
    factory = cfg.habitat_baselines.vector_env_factory
    switches = {k: v for k, v in factory.items() if k != "_target_"} if str(factory["_target_"]).endswith(".SyntheticVectorEnvFactory") else {}
    env = SyntheticVectorEnvFactory(**switches).construct_envs(cfg, device="cuda")
    generator = torch.Generator().manual_seed(args.seed)
    obs = env._own_obs()
    env.reset_into_obs(obs)
    frames = [[f] for f in env.render_frames(height=args.height).cpu().numpy()]
    ids = [e["episode_id"] for e in env.current_episodes()]
    written = []
    while len(written) < args.episodes:
        actions = env.expert_actions() if args.agent == "teacher" else random_actions(env, generator)
        env.step_into_obs(obs, env._rew, env._nd, actions=actions)
        new = env.render_frames(height=args.height).cpu().numpy()
        infos, next_ids = env.step_infos_host(range(env.num_envs)), [e["episode_id"] for e in env.current_episodes()]
        for i, info in enumerate(infos):
            if info and len(written) < args.episodes:  # the ending step's frame opens the next episode
                written.append(write_episode_video(frames[i], args.out, ids[i], 0, info, args.fps))
                print(written[-1], f"({len(frames[i])} frames)")
            if info:
                frames[i], ids[i] = [], next_ids[i]
            frames[i].append(new[i])
    return written


if __name__ == "__main__":
    main()
