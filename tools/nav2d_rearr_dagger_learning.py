#!/usr/bin/env python3
"""Can the policy express the oracle?  The rearrangement learning run in geodesic mode (the geodesic leg of
tools/nav2d_rearr_geo_learning.py: PointNavResNetPolicy with ResNet18 on head_depth and the three fused sensors, hidden 128, one
recurrent layer, start_holding, turn_angle 30, K = 3 obstacles, max_episode_steps 48, 32 envs x 32 steps at 64 x 64, lr 5e-4, 4 epochs
x 2 minibatches) taught by DAgger from rearrange/dagger_nav2d_rearrange_geodesic.yaml: the env's pick-and-place oracle labels every
visited state, beta falls 1 -> 0 over the first half of the updates, the DAgger updater clones the labels.

Criterion (the family's, applied to `imitation_agreement`): the agree / total counts of the last 5 updates against the first 5, a
two-proportion z >= 5 with the agreement higher, and a lower `action_loss`.  After training a pure-policy window follows: beta = 0, no
update, `--window` rollouts; its success, did_pick_object and object_to_goal_distance are what PPO's run of the same sizes and seed
(tools/nav2d_rearr_geo_learning.py, geodesic leg) and the oracle's own row are set beside.  `--ppo` runs that PPO run too, `--oracle`
the same window with beta = 1.
usage: python tools/nav2d_rearr_dagger_learning.py [--updates U] [--seeds S [S ...]] [--window R] [--every K] [--ppo] [--oracle]"""
import argparse
import importlib.util
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
spec = importlib.util.spec_from_file_location("nav2d_rearr_learning", os.path.join(HERE, "nav2d_rearr_learning.py"))
base = importlib.util.module_from_spec(spec)
spec.loader.exec_module(base)

N, T, W_LAST = base.N, base.T, base.W_LAST
YAML = "rearrange/dagger_nav2d_rearrange_geodesic.yaml"


def two_proportion_z(a0, n0, a1, n1):
    """z of the proportion a1 / n1 against a0 / n0 with the pooled variance."""
    p0, p1, p = a0 / max(n0, 1), a1 / max(n1, 1), (a0 + a1) / max(n0 + n1, 1)
    se = math.sqrt(max(p * (1.0 - p) * (1.0 / max(n0, 1) + 1.0 / max(n1, 1)), 1e-300))
    return (p1 - p0) / se


def overrides(folder, seed, updates, lr=5.0e-4, max_steps=48, size=64, obstacles=3):
    return [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=100000",
            "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
            "habitat_baselines.rl.ppo.hidden_size=128", f"habitat_baselines.checkpoint_folder={folder}", "habitat_baselines.log_interval=100000",
            f"habitat_baselines.tensorboard_dir={folder}/tb", "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000",
            "habitat_baselines.trainer_name=ppo", f"habitat.environment.max_episode_steps={max_steps}",
            f"habitat.synthetic.num_obstacles={obstacles}", "habitat.synthetic.turn_angle=30", "habitat.synthetic.start_holding=True",
            f"habitat.seed={seed}", f"habitat_baselines.rl.ppo.lr={lr}", "habitat_baselines.rl.ppo.ppo_epoch=4",
            "habitat_baselines.rl.ppo.num_mini_batch=2", "habitat_baselines.rl.ddppo.num_recurrent_layers=1",
            f"habitat.simulator.sensors.head_depth.height={size}", f"habitat.simulator.sensors.head_depth.width={size}",
            "habitat_baselines.rl.imitation.beta_start=1.0", "habitat_baselines.rl.imitation.beta_end=0.0",
            f"habitat_baselines.rl.imitation.beta_decay_updates={max(updates // 2, 1)}"]


def learning_run(folder, seed=100, updates=60, window=8, every=0, window_beta=0.0):
    from habitat_amd.common.baseline_registry import baseline_registry
    from habitat_amd.config.default import get_config
    import habitat_amd.rl.ppo.ppo_trainer  # noqa: F401
    cfg = get_config(YAML, overrides(folder, seed, updates))
    torch.manual_seed(seed)
    trainer = baseline_registry.get_trainer("ppo")(cfg)
    trainer._init_train()
    assert type(trainer._agent.updater).__name__ == "DAgger" and trainer._device_envs and trainer._imitation is not None
    envs = trainer.envs
    last = torch.zeros(T, N, 4, device=envs._state.device)
    orig_step, t_of = envs.step_into_obs, [0]

    def step_into_obs(*a, **kw):  # the measures of an episode that ends stay in the record until the env's next one ends
        orig_step(*a, **kw)
        last[t_of[0] % T].copy_(envs._state[:, W_LAST:W_LAST + 4].contiguous().view(torch.float32))
        t_of[0] += 1

    envs.step_into_obs = step_into_obs
    counts, losses, t0 = [], [], time.time()
    for u in range(updates):
        m = trainer.run_update_cycle()
        counts.append(trainer._imitation["counts"])
        losses.append(m["action_loss"])
        if every and (u + 1) % every == 0:
            print(f"update {u + 1}: {time.time() - t0:.1f} s  beta {m['imitation_beta']:.2f}  agreement {m['imitation_agreement']:.3f}  "
                  f"action_loss {m['action_loss']:.4f}  expert_prob_mean {m['expert_prob_mean']:.3f}", flush=True)
    seconds = time.time() - t0
    a0, n0 = (sum(c[i] for c in counts[:5]) for i in (0, 1))
    a1, n1 = (sum(c[i] for c in counts[-5:]) for i in (0, 1))
    # the pure-policy window: beta = 0 (window_beta = 1 gives the oracle's own row), no update; the storage is rolled over as an
    # update would
    im = trainer._imitation["cfg"]
    im.beta_start = im.beta_end = float(window_beta)
    trainer._agent.eval()
    st, B = trainer._agent.rollouts, trainer._agent.rollouts.buffers
    ends = []  # (success, did_pick_object, object_to_goal_distance) of every episode that ends inside the window
    for _ in range(window):
        trainer.collect_rollout()
        masks, words = B["masks"][: T + 1].cpu().numpy().reshape(T + 1, N).astype(bool), last.cpu().numpy()
        ends += [tuple(float(x) for x in words[t, n, :3]) for t in range(T) for n in np.nonzero(~masks[t + 1])[0]]
        st.after_update()
    lastw = np.array(ends, np.float64).reshape(-1, 3)
    trainer.envs.close()
    return dict(seed=seed, updates=updates, seconds=seconds, agree_first=a0, total_first=n0, agree_last=a1, total_last=n1,
                agreement_first=a0 / max(n0, 1), agreement_last=a1 / max(n1, 1), z=two_proportion_z(a0, n0, a1, n1),
                action_loss_first=float(np.mean(losses[:5])), action_loss_last=float(np.mean(losses[-5:])),
                window_episodes=len(ends), window_success=float(lastw[:, 0].mean()) if len(ends) else float("nan"),
                window_did_pick_object=float(lastw[:, 1].mean()) if len(ends) else float("nan"),
                window_object_to_goal_distance=float(lastw[:, 2].mean()) if len(ends) else float("nan"))


def criterion(r):
    return r["z"] >= 5.0 and r["agreement_last"] > r["agreement_first"] and r["action_loss_last"] < r["action_loss_first"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=60)
    ap.add_argument("--seeds", type=int, nargs="+", default=[100])
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--ppo", action="store_true", help="also the PPO run of the same sizes, seed and update count (geodesic leg)")
    ap.add_argument("--oracle", action="store_true", help="also the oracle's own row: the same window with beta = 1")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nav2d_rearr_dagger_learning needs a GPU"
    for seed in a.seeds:
        with tempfile.TemporaryDirectory() as folder:
            r = learning_run(folder, seed, a.updates, a.window, a.every)
        print("nav2drearr dagger:", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}, flush=True)
        print("criterion met" if criterion(r) else "criterion NOT met", flush=True)
        if a.oracle:
            with tempfile.TemporaryDirectory() as folder:
                o = learning_run(folder, seed, 5, a.window, 0, window_beta=1.0)
            print("nav2drearr oracle:", {k: round(v, 4) for k, v in o.items() if k.startswith("window_")}, flush=True)
        if a.ppo:
            with tempfile.TemporaryDirectory() as folder:
                p = base.learning_run(folder, seed=seed, updates=a.updates, max_steps=48, obstacles=3, distance="geodesic")
            print("nav2drearr ppo   :", {k: (round(float(v), 4) if isinstance(v, (float, np.floating)) else v) for k, v in p.items()}, flush=True)


if __name__ == "__main__":
    main()
