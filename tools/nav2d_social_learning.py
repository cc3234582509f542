#!/usr/bin/env python3
"""Does the loop learn to find and follow a walking person?  PPOTrainer with PointNavResNetPolicy and the Gaussian head on
Nav2DSocial-v0 (social_nav/ddppo_nav2d_social.yaml), 32 envs x 32 steps.  The test's settings: a BLIND policy on the two fused sensors
(fuse_keys = person_sensor, person_visible: D = 3), person_always_visible, no obstacles, turn_angle 10 with turns of up to 30 degrees,
a short episode limit.  The reward is no potential once the person is found: the return can only keep rising by staying between 1 and
2 m and facing them, step after step, while they walk.  `--yaml-settings` runs the file's own: ResNet18 on head_depth at 64 x 64 with
the sensors zero while the person is hidden, three obstacles, turn_angle 1.
Criterion (the family's, tests/test_gpu_nav2d.py::test_the_loop_learns): the per-episode returns of the last 5 updates against the
first 5 of one seed, two-sample z >= 5, the mean return higher; and the mean following_rate higher.  has_found_person is printed.
usage: python tools/nav2d_social_learning.py [--updates U] [--seed S] [--lr LR] [--max-steps E] [--every K] [--yaml-settings]"""
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

PARAMS = (10, 30, 10)  # turn_angle, max_turn_angle, min_abs_ang_speed of the test's settings


def episode_ends(rewards, masks, last, carry):
    """Per-episode (return, has_found_person, following_rate) of the episodes that END inside one (T, N) rollout; `carry` (N,) holds
    the partial returns, `last` (T, N, 4) the record's last-measures words after each step."""
    out = []
    for t in range(rewards.shape[0]):
        carry += rewards[t]
        for n in np.nonzero(~masks[t + 1])[0]:
            out.append((carry[n], float(last[t, n, 0]), float(last[t, n, 1])))
            carry[n] = 0.0
    return out


def z_of(per_update):
    first = np.array([e for u in per_update[:5] for e in u])
    last = np.array([e for u in per_update[-5:] for e in u])
    z = (last[:, 0].mean() - first[:, 0].mean()) / math.sqrt(first[:, 0].var(ddof=1) / len(first) + last[:, 0].var(ddof=1) / len(last))
    return dict(episodes_first=len(first), episodes_last=len(last), return_first=first[:, 0].mean(), return_last=last[:, 0].mean(),
                found_first=first[:, 1].mean(), found_last=last[:, 1].mean(), following_first=first[:, 2].mean(),
                following_last=last[:, 2].mean(), z=z)


def criterion(r):
    return r["z"] >= 5.0 and r["return_last"] > r["return_first"] and r["following_last"] > r["following_first"]


def learning_run(folder, seed=100, updates=100, lr=5.0e-4, max_steps=48, every=0, yaml_settings=False):
    from habitat_amd.common.baseline_registry import baseline_registry
    from habitat_amd.config.default import get_config
    import habitat_amd.rl.ppo.ppo_trainer  # noqa: F401
    assert max_steps <= 4 * T, "episodes end at the limit alone: the first five updates must hold whole episodes"
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=100000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          "habitat_baselines.rl.ppo.hidden_size=128", f"habitat_baselines.checkpoint_folder={folder}", "habitat_baselines.log_interval=100000",
          f"habitat_baselines.tensorboard_dir={folder}/tb", "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000",
          "habitat_baselines.trainer_name=ppo", f"habitat.environment.max_episode_steps={max_steps}", f"habitat.seed={seed}",
          f"habitat_baselines.rl.ppo.lr={lr}", "habitat_baselines.rl.ppo.ppo_epoch=4", "habitat_baselines.rl.ppo.num_mini_batch=2",
          "habitat_baselines.rl.ppo.clip_param=0.2", "habitat_baselines.rl.ddppo.num_recurrent_layers=1"]
    if not yaml_settings:
        turn, max_turn, min_ang = PARAMS
        ov += ["habitat.synthetic.num_obstacles=0", f"habitat.synthetic.turn_angle={turn}", f"habitat.synthetic.max_turn_angle={max_turn}",
               f"habitat.synthetic.min_abs_ang_speed={min_ang}", "habitat.synthetic.person_always_visible=True",
               "habitat_baselines.rl.policy.main_agent.fuse_keys=[person_sensor,person_visible]"]
    cfg = get_config("social_nav/ddppo_nav2d_social.yaml", ov)
    torch.manual_seed(seed)
    trainer = baseline_registry.get_trainer("ppo")(cfg)
    trainer._init_train()
    policy = trainer._agent.actor_critic
    assert list(trainer.envs.observation_spaces[0].spaces) == ["head_depth", "person_sensor", "person_visible"]
    assert type(policy).__name__ == "PointNavResNetPolicy" and trainer._device_envs and policy.is_blind == (not yaml_settings)
    assert [k for k, _ in policy.fused_sensors] == ["person_sensor", "person_visible"]
    assert policy.action_distribution_type == "gaussian" and trainer.envs.action_spaces[0].shape == (2,)
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
        assert B["actions"].dtype == torch.float32 and B["actions"].shape[-1] == 2
        snap.update(rewards=B["rewards"][:T].clone(), masks=B["masks"][: T + 1].clone(), last=last.clone())
        return orig()

    trainer._update_agent = update
    carry, per_update, t0 = np.zeros(N), [], time.time()
    for u in range(updates):
        trainer.run_update_cycle()
        per_update.append(episode_ends(snap["rewards"].cpu().numpy().reshape(T, N).astype(np.float64),
                                       snap["masks"].cpu().numpy().reshape(T + 1, N).astype(bool), snap["last"].cpu().numpy(), carry))
        if every and (u + 1) % every == 0 and u >= 9:
            r = z_of(per_update)
            print(f"update {u + 1}: {time.time() - t0:.1f} s  return {r['return_first']:.3f} -> {r['return_last']:.3f}  found "
                  f"{r['found_first']:.3f} -> {r['found_last']:.3f}  following_rate {r['following_first']:.3f} -> "
                  f"{r['following_last']:.3f}  z {r['z']:.2f}", flush=True)
    trainer.envs.close()
    return dict(seed=seed, updates=updates, lr=lr, max_episode_steps=max_steps, yaml_settings=bool(yaml_settings),
                seconds=time.time() - t0, **z_of(per_update))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--seed", type=int, default=100)
    ap.add_argument("--lr", type=float, default=5.0e-4)
    ap.add_argument("--max-steps", type=int, default=48)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--yaml-settings", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nav2d_social_learning needs a GPU"
    with tempfile.TemporaryDirectory() as folder:
        r = learning_run(folder, a.seed, a.updates, a.lr, a.max_steps, a.every, a.yaml_settings)
    print("nav2dsocial learning:", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
    print("criterion met" if criterion(r) else "criterion NOT met")


if __name__ == "__main__":
    main()
