#!/usr/bin/env python3
"""Does the goal arrive through the image?  Nav2DImageNav-v0 learned by PPO (imagenav/ddppo_nav2d_imagenav.yaml) and by DAgger from
the shortest-path follower (imagenav/dagger_nav2d_imagenav_geodesic.yaml): PointNavResNetPolicy with ResNet18 on rgb + depth + goal_rgb
(7 channels, early fusion), gps and compass through their embeddings, hidden 128, one recurrent layer, turn_angle 30, K = 3 obstacles,
max_episode_steps 64, success_distance 1.0, geodesic distance, 32 envs x 32 steps at 64 x 64, lr 5e-4, 4 epochs x 2 minibatches.  For
DAgger beta falls 1 -> 0 over the first half of the updates.

After training a pure-policy window follows: no update (beta = 0 for DAgger), `--window` rollouts; reported are the success, spl and
distance_to_goal of the episodes that end inside it.  Beside every run stands its control, the same run in which goal_rgb is zeroed
before the policy sees it (in training and in the window): the policy then has gps and compass but nothing that tells the goal, and
the difference between run and control (a two-proportion z of the window's successes) is what the goal image carries.  The follower's
own row comes from ShortestPathFollower.evaluate on envs of the same config.  Nothing is asserted.
usage: python tools/nav2d_imagenav_learning.py [--updates U] [--seeds S [S ...]] [--window R] [--every K] [--methods ppo dagger]"""
import argparse
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))

N, T = 32, 32
W_LAST = 12  # HAB_NAV2D_W_LAST_MEASURES: success, spl, distance_to_goal, collisions of the episode that ended last
YAMLS = dict(ppo="imagenav/ddppo_nav2d_imagenav.yaml", dagger="imagenav/dagger_nav2d_imagenav_geodesic.yaml")


def two_proportion_z(a0, n0, a1, n1):
    """z of the proportion a1 / n1 against a0 / n0 with the pooled variance."""
    p0, p1, p = a0 / max(n0, 1), a1 / max(n1, 1), (a0 + a1) / max(n0 + n1, 1)
    se = math.sqrt(max(p * (1.0 - p) * (1.0 / max(n0, 1) + 1.0 / max(n1, 1)), 1e-300))
    return (p1 - p0) / se


def overrides(folder, seed, updates, method, lr=5.0e-4, max_steps=64, size=64, obstacles=3):
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=100000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          "habitat_baselines.rl.ppo.hidden_size=128", f"habitat_baselines.checkpoint_folder={folder}", "habitat_baselines.log_interval=100000",
          f"habitat_baselines.tensorboard_dir={folder}/tb", "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000",
          "habitat_baselines.trainer_name=ppo", f"habitat.environment.max_episode_steps={max_steps}",
          f"habitat.synthetic.num_obstacles={obstacles}", "habitat.synthetic.turn_angle=30", f"habitat.seed={seed}",
          f"habitat_baselines.rl.ppo.lr={lr}", "habitat_baselines.rl.ppo.ppo_epoch=4", "habitat_baselines.rl.ppo.num_mini_batch=2",
          "habitat_baselines.rl.ddppo.num_recurrent_layers=1"]
    ov += [f"habitat.simulator.sensors.{s}.{d}={size}" for s in ("rgb", "depth") for d in ("height", "width")]
    if method == "dagger":
        ov += ["habitat_baselines.rl.imitation.beta_start=1.0", "habitat_baselines.rl.imitation.beta_end=0.0",
               f"habitat_baselines.rl.imitation.beta_decay_updates={max(updates // 2, 1)}"]
    return ov


def learning_run(folder, method="dagger", seed=100, updates=60, window=8, every=0, zero_goal=False):
    from habitat_amd.common.baseline_registry import baseline_registry
    from habitat_amd.config.default import get_config
    import habitat_amd.rl.ppo.ppo_trainer  # noqa: F401
    cfg = get_config(YAMLS[method], overrides(folder, seed, updates, method))
    torch.manual_seed(seed)
    trainer = baseline_registry.get_trainer("ppo")(cfg)
    trainer._init_train()
    policy = trainer._agent.actor_critic
    assert [v[0] for v in policy.visual_sensors] == ["rgb", "depth", "goal_rgb"] and trainer._device_envs
    assert (type(trainer._agent.updater).__name__ == "DAgger") == (method == "dagger")
    envs = trainer.envs
    last = torch.zeros(T, N, 4, device=envs._state.device)
    orig_step, orig_reset, t_of = envs.step_into_obs, envs.reset_into_obs, [0]

    def blind(obs):  # the control: the policy never sees the goal image
        if zero_goal and "goal_rgb" in obs:
            obs["goal_rgb"].zero_()

    def step_into_obs(obs, *a, **kw):  # the measures of an episode that ends stay in the record until the env's next one ends
        orig_step(obs, *a, **kw)
        blind(obs)
        last[t_of[0] % T].copy_(envs._state[:, W_LAST:W_LAST + 4].contiguous().view(torch.float32))
        t_of[0] += 1

    def reset_into_obs(obs):
        orig_reset(obs)
        blind(obs)

    envs.step_into_obs, envs.reset_into_obs = step_into_obs, reset_into_obs
    if zero_goal:
        blind(trainer._agent.rollouts.buffers["observations"])   # the first observations were written by _init_train
    t0 = time.time()
    for u in range(updates):
        m = trainer.run_update_cycle()
        if every and (u + 1) % every == 0:
            extra = f"  beta {m['imitation_beta']:.2f}  agreement {m['imitation_agreement']:.3f}" if method == "dagger" else ""
            print(f"update {u + 1}: {time.time() - t0:.1f} s  action_loss {m['action_loss']:.4f}{extra}", flush=True)
    seconds = time.time() - t0
    if method == "dagger":
        im = trainer._imitation["cfg"]
        im.beta_start = im.beta_end = 0.0
    trainer._agent.eval()
    st, B = trainer._agent.rollouts, trainer._agent.rollouts.buffers
    ends = []  # (success, spl, distance_to_goal) of every episode that ends inside the window
    for _ in range(window):
        trainer.collect_rollout()
        masks, words = B["masks"][: T + 1].cpu().numpy().reshape(T + 1, N).astype(bool), last.cpu().numpy()
        ends += [tuple(float(x) for x in words[t, n, :3]) for t in range(T) for n in np.nonzero(~masks[t + 1])[0]]
        st.after_update()
    w = np.array(ends, np.float64).reshape(-1, 3)
    trainer.envs.close()
    return dict(method=method, zero_goal=zero_goal, seed=seed, updates=updates, seconds=seconds, window_episodes=len(ends),
                window_successes=int(w[:, 0].sum()), window_success=float(w[:, 0].mean()) if len(ends) else float("nan"),
                window_spl=float(w[:, 1].mean()) if len(ends) else float("nan"),
                window_distance_to_goal=float(w[:, 2].mean()) if len(ends) else float("nan"))


def oracle_row(seed, episodes=256):
    """The follower's own score on envs of the learning runs' config."""
    from habitat_amd.common.env_factory import instantiate
    from habitat_amd.common.shortest_path_follower import ShortestPathFollower
    from habitat_amd.config.default import get_config
    cfg = get_config(YAMLS["ppo"], overrides("unused", seed, 1, "ppo"))
    env = instantiate(cfg.habitat_baselines.vector_env_factory).construct_envs(cfg, device="cuda")
    return ShortestPathFollower(env).evaluate(episodes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=60)
    ap.add_argument("--seeds", type=int, nargs="+", default=[100, 101, 102])
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--methods", nargs="+", default=["ppo", "dagger"], choices=sorted(YAMLS))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nav2d_imagenav_learning needs a GPU"
    fmt = lambda r: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
    print("nav2dimagenav follower:", fmt(oracle_row(a.seeds[0])), flush=True)
    for seed in a.seeds:
        for method in a.methods:
            pair = []
            for zero_goal in (False, True):
                with tempfile.TemporaryDirectory() as folder:
                    pair.append(learning_run(folder, method, seed, a.updates, a.window, a.every, zero_goal))
                print(f"nav2dimagenav {method}{' control' if zero_goal else ''}:", fmt(pair[-1]), flush=True)
            run, ctl = pair
            z = two_proportion_z(ctl["window_successes"], ctl["window_episodes"], run["window_successes"], run["window_episodes"])
            print(f"nav2dimagenav {method} seed {seed}: success {run['window_success']:.3f} with the goal image, "
                  f"{ctl['window_success']:.3f} with it zeroed, z {z:.2f}", flush=True)


if __name__ == "__main__":
    main()
