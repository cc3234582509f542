#!/usr/bin/env python3
"""Does the loop learn to explore?  PPOTrainer with PointNavResNetPolicy on Nav2DExplore-v0 from exploration/ddppo_nav2d_explore.yaml
(ResNet18 on depth at 64 x 64, gps and compass through their embeddings, no objectgoal), 32 envs x 32 steps.  The reward is the area
seen for the first time, so nothing tells the agent where to go: its recurrent state is the only record of where it has been.
Reported: the `coverage` of the episodes that ended in the last 5 updates against the coverage of as many episodes of a uniformly
random policy on envs of the same config, by the two-sample z the sibling learning runs use; and the same z of the per-episode returns
of the last 5 updates against the first 5.  Nothing is asserted.
usage: python tools/nav2d_explore_learning.py [--updates U] [--seed S] [--lr LR] [--max-steps E] [--every K]"""
import argparse
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nav2d_rearr_learning import N, T, W_LAST  # noqa: E402

YAML = "exploration/ddppo_nav2d_explore.yaml"


def episode_ends(rewards, masks, last, carry):
    """Per-episode (return, coverage, num_steps) of the episodes that END inside one (T, N) rollout; `carry` (N,) holds the partial
    returns, `last` (T, N, 4) the record's last-measures words after each step."""
    out = []
    for t in range(rewards.shape[0]):
        carry += rewards[t]
        for n in np.nonzero(~masks[t + 1])[0]:
            out.append((carry[n], float(last[t, n, 0]), float(last[t, n, 3])))
            carry[n] = 0.0
    return out


def two_sample_z(a, b):
    """(mean(a) - mean(b)) over the standard error of the difference."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a.mean() - b.mean()) / math.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))


def random_coverage(cfg, episodes, seed):
    """The coverage of the first `episodes` episodes that end under uniformly random actions, on envs of the same config."""
    from habitat_amd.common.env_factory import instantiate
    env = instantiate(cfg.habitat_baselines.vector_env_factory).construct_envs(cfg, device="cuda")
    obs = {k: v for k, v in env._own_obs().items() if k in ("gps", "compass")}   # the measures need no image
    env.reset_into_obs(obs)
    g = torch.Generator().manual_seed(seed)
    out = []
    while len(out) < episodes:
        env.step_into_obs(obs, env._rew, env._nd, actions=torch.randint(0, 4, (env.num_envs,), generator=g).cuda())
        ended = (env._nd == 0).cpu().numpy()
        last = env._state[:, W_LAST:W_LAST + 4].contiguous().view(torch.float32).cpu().numpy()
        out += [float(last[n, 0]) for n in np.nonzero(ended)[0]]
    return out[:episodes]


def learning_run(folder, seed=100, updates=100, lr=2.5e-4, max_steps=64, every=0):
    from habitat_amd.common.baseline_registry import baseline_registry
    from habitat_amd.config.default import get_config
    import habitat_amd.rl.ppo.ppo_trainer  # noqa: F401
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=100000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          f"habitat_baselines.checkpoint_folder={folder}", "habitat_baselines.log_interval=100000",
          f"habitat_baselines.tensorboard_dir={folder}/tb", "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000",
          "habitat_baselines.trainer_name=ppo", f"habitat.environment.max_episode_steps={max_steps}", f"habitat.seed={seed}",
          f"habitat_baselines.rl.ppo.lr={lr}"]
    cfg = get_config(YAML, ov)
    torch.manual_seed(seed)
    trainer = baseline_registry.get_trainer("ppo")(cfg)
    trainer._init_train()
    policy = trainer._agent.actor_critic
    assert list(trainer.envs.observation_spaces[0].spaces) == ["depth", "gps", "compass"]
    assert type(policy).__name__ == "PointNavResNetPolicy" and trainer._device_envs and not policy.is_blind
    envs = trainer.envs
    last = torch.zeros(T, N, 4, device=envs._state.device)
    orig_step = envs.step_into_obs
    t_of = [0]

    def step_into_obs(*a, **kw):  # the measures of an episode that ends stay in the record until the env's next one ends
        orig_step(*a, **kw)
        last[t_of[0] % T].copy_(envs._state[:, W_LAST:W_LAST + 4].contiguous().view(torch.float32))
        t_of[0] += 1

    envs.step_into_obs = step_into_obs
    snap, orig = {}, trainer._update_agent

    def update():  # after_update overwrites row 0, so the finished rollout is copied right before the update
        B = trainer._agent.rollouts.buffers
        snap.update(rewards=B["rewards"][:T].clone(), masks=B["masks"][: T + 1].clone(), last=last.clone())
        return orig()

    trainer._update_agent = update
    carry, per_update, t0 = np.zeros(N), [], time.time()
    for u in range(updates):
        trainer.run_update_cycle()
        per_update.append(episode_ends(snap["rewards"].cpu().numpy().reshape(T, N).astype(np.float64),
                                       snap["masks"].cpu().numpy().reshape(T + 1, N).astype(bool), snap["last"].cpu().numpy(), carry))
        if every and (u + 1) % every == 0 and u >= 9:
            tail = np.array([e for w in per_update[-5:] for e in w])
            print(f"update {u + 1}: {time.time() - t0:.1f} s  return {tail[:, 0].mean():.3f}  coverage {tail[:, 1].mean():.4f}  "
                  f"steps {tail[:, 2].mean():.1f}", flush=True)
    seconds = time.time() - t0
    trainer.envs.close()
    first = np.array([e for w in per_update[:5] for e in w])
    tail = np.array([e for w in per_update[-5:] for e in w])
    rand = random_coverage(cfg, len(tail), seed + 1)
    return dict(seed=seed, updates=updates, lr=lr, max_episode_steps=max_steps, seconds=seconds, episodes_first=len(first),
                episodes_last=len(tail), return_first=first[:, 0].mean(), return_last=tail[:, 0].mean(),
                z_return=two_sample_z(tail[:, 0], first[:, 0]), coverage_first=first[:, 1].mean(), coverage_last=tail[:, 1].mean(),
                steps_last=tail[:, 2].mean(), coverage_random=float(np.mean(rand)), z_coverage_vs_random=two_sample_z(tail[:, 1], rand))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--seed", type=int, default=100)
    ap.add_argument("--lr", type=float, default=2.5e-4)
    ap.add_argument("--max-steps", type=int, default=64)
    ap.add_argument("--every", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nav2d_explore_learning needs a GPU"
    with tempfile.TemporaryDirectory() as folder:
        r = learning_run(folder, a.seed, a.updates, a.lr, a.max_steps, a.every)
    print("nav2dexplore learning:", {k: (round(float(v), 4) if isinstance(v, (float, np.floating)) else v) for k, v in r.items()})


if __name__ == "__main__":
    main()
