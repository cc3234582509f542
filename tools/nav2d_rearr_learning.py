#!/usr/bin/env python3
"""Does the loop learn through the fused 1-D sensors?  PPOTrainer with PointNavResNetPolicy (ResNet18) on Nav2DRearr-v0 with
head_depth and the three fused sensors (obj_start_sensor, obj_goal_sensor, is_holding: D = 5), start_holding, no obstacles,
turn_angle 30, a short episode limit, 32 envs x 32 steps at 64 x 64.  The goal is in no image: head_depth shows the four walls and
nothing else while the object is held, so the return can only rise through the fused columns of the recurrent input.  Criterion
(tests/test_gpu_nav2d.py::test_the_loop_learns): the per-episode returns of the last 5 updates against the first 5 of one seed,
two-sample z >= 5, the mean return higher; and the mean final object_to_goal_distance lower.  Success is printed.  Prints the run's
dictionary, the wall time, and a line every `--every` updates.
usage: python tools/nav2d_rearr_learning.py [--updates U] [--seed S] [--lr LR] [--max-steps E] [--size P] [--every K]"""
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

N, T = 32, 32
W_LAST = 12  # HAB_NAV2D_W_LAST_MEASURES: success, did_pick_object, object_to_goal_distance, collisions of the episode that ended last


def episode_ends(rewards, masks, last, carry):
    """Per-episode (return, success, final object_to_goal_distance) of the episodes that END inside one (T, N) rollout; `carry` (N,)
    holds the partial returns, `last` (T, N, 4) the record's last-measures words after each step."""
    out = []
    for t in range(rewards.shape[0]):
        carry += rewards[t]
        for n in np.nonzero(~masks[t + 1])[0]:
            out.append((carry[n], float(last[t, n, 0]), float(last[t, n, 2])))
            carry[n] = 0.0
    return out


def z_of(per_update):
    first = np.array([e for u in per_update[:5] for e in u])
    last = np.array([e for u in per_update[-5:] for e in u])
    z = (last[:, 0].mean() - first[:, 0].mean()) / math.sqrt(first[:, 0].var(ddof=1) / len(first) + last[:, 0].var(ddof=1) / len(last))
    return dict(episodes_first=len(first), episodes_last=len(last), return_first=first[:, 0].mean(), return_last=last[:, 0].mean(),
                success_first=first[:, 1].mean(), success_last=last[:, 1].mean(), distance_first=first[:, 2].mean(),
                distance_last=last[:, 2].mean(), z=z)


def learning_run(folder, seed=100, updates=100, lr=5.0e-4, max_steps=48, size=64, every=0, obstacles=0, distance="euclidean"):
    from habitat_amd.common.baseline_registry import baseline_registry
    from habitat_amd.config.default import get_config
    import habitat_amd.rl.ppo.ppo_trainer  # noqa: F401
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=100000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          "habitat_baselines.rl.ppo.hidden_size=128", f"habitat_baselines.checkpoint_folder={folder}", "habitat_baselines.log_interval=100000",
          f"habitat_baselines.tensorboard_dir={folder}/tb", "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000",
          "habitat_baselines.trainer_name=ppo", f"habitat.environment.max_episode_steps={max_steps}",
          f"habitat.synthetic.num_obstacles={obstacles}", f"habitat.synthetic.distance_to_goal={distance}",
          "habitat.synthetic.turn_angle=30", "habitat.synthetic.start_holding=True", f"habitat.seed={seed}",
          f"habitat_baselines.rl.ppo.lr={lr}", "habitat_baselines.rl.ppo.ppo_epoch=4", "habitat_baselines.rl.ppo.num_mini_batch=2",
          "habitat_baselines.rl.ppo.clip_param=0.2", "habitat_baselines.rl.ddppo.num_recurrent_layers=1",
          f"habitat.simulator.sensors.head_depth.height={size}", f"habitat.simulator.sensors.head_depth.width={size}"]
    cfg = get_config("rearrange/ddppo_nav2d_rearrange.yaml", ov)
    torch.manual_seed(seed)
    trainer = baseline_registry.get_trainer("ppo")(cfg)
    trainer._init_train()
    assert list(trainer.envs.observation_spaces[0].spaces) == ["head_depth", "obj_start_sensor", "obj_goal_sensor", "is_holding"]
    assert type(trainer._agent.actor_critic).__name__ == "PointNavResNetPolicy" and trainer._device_envs
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
            r = z_of(per_update)
            print(f"update {u + 1}: {time.time() - t0:.1f} s  return {r['return_first']:.3f} -> {r['return_last']:.3f}  success "
                  f"{r['success_first']:.3f} -> {r['success_last']:.3f}  distance {r['distance_first']:.3f} -> {r['distance_last']:.3f}  "
                  f"z {r['z']:.2f}", flush=True)
    trainer.envs.close()
    return dict(seed=seed, updates=updates, lr=lr, max_episode_steps=max_steps, size=size, num_obstacles=obstacles, distance=distance,
                seconds=time.time() - t0, **z_of(per_update))


def criterion(r):
    return r["z"] >= 5.0 and r["return_last"] > r["return_first"] and r["distance_last"] < r["distance_first"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--seed", type=int, default=100)
    ap.add_argument("--lr", type=float, default=5.0e-4)
    ap.add_argument("--max-steps", type=int, default=48)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--every", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nav2d_rearr_learning needs a GPU"
    with tempfile.TemporaryDirectory() as folder:
        r = learning_run(folder, a.seed, a.updates, a.lr, a.max_steps, a.size, a.every)
    print("nav2drearr learning:", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
    print("criterion met" if criterion(r) else "criterion NOT met")


if __name__ == "__main__":
    main()
