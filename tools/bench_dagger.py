#!/usr/bin/env python3
"""What DAgger costs.  From rearrange/dagger_nav2d_rearrange_geodesic.yaml and its PPO sibling at the same sizes: microseconds per call
of the teacher's label (`expert_actions`) plus the mix (`hab_dagger_mix`) beside the env step they precede, and milliseconds per
minibatch of the DAgger updater beside the PPO updater's, the two trainers' updates alternated in one process, medians with their
ranges.  The figures are reported, not asserted.
usage: python tools/bench_dagger.py [--envs N] [--steps T] [--size P] [--calls C] [--cycles R]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "habitat-lab_amd"))


def make_trainer(yaml, folder, a):
    from habitat_amd.common.baseline_registry import baseline_registry
    from habitat_amd.config.default import get_config
    import habitat_amd.rl.ppo.ppo_trainer  # noqa: F401
    ov = [f"habitat_baselines.num_environments={a.envs}", f"habitat_baselines.rl.ppo.num_steps={a.steps}", "habitat_baselines.num_updates=100000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          f"habitat_baselines.checkpoint_folder={folder}", "habitat_baselines.log_interval=100000", f"habitat_baselines.tensorboard_dir={folder}/tb",
          "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000", "habitat_baselines.trainer_name=ppo",
          f"habitat.simulator.sensors.head_depth.height={a.size}", f"habitat.simulator.sensors.head_depth.width={a.size}"]
    cfg = get_config(yaml, ov)
    torch.manual_seed(cfg.habitat.seed)
    trainer = baseline_registry.get_trainer("ppo")(cfg)
    trainer._init_train()
    return trainer


def device_us(fn, calls):
    for _ in range(10):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls, (time.perf_counter() - t0) * 1e6 / calls


def timed_update(trainer):
    """One rollout, its returns, then the updater's update alone between two synchronisations -> milliseconds per minibatch."""
    trainer._agent.eval()
    trainer.collect_rollout()
    st = trainer._agent.rollouts
    last = st.get_last_step()
    nv = trainer._agent.actor_critic.get_value({k: v.contiguous() for k, v in last["observations"].items()},
                                               last["recurrent_hidden_states"], last["prev_actions"], last["masks"])
    st.compute_returns(nv, trainer._ppo_cfg.use_gae, trainer._ppo_cfg.gamma, trainer._ppo_cfg.tau)
    trainer._agent.train()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer._agent.updater.update(st)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    st.after_update()
    return ms / (trainer._ppo_cfg.ppo_epoch * trainer._ppo_cfg.num_mini_batch)


def alternated_minibatch_ms(trainers, cycles):
    """The trainers' updates alternated in one process, `cycles` each after two warm-up updates each -> (median, min, max) per trainer."""
    for _ in range(2):
        for tr in trainers:
            tr.run_update_cycle()
    ms = [[] for _ in trainers]
    for _ in range(cycles):
        for i, tr in enumerate(trainers):
            ms[i].append(timed_update(tr))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--cycles", type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dagger needs a GPU"
    from habitat_amd import _lib
    with tempfile.TemporaryDirectory() as folder:
        tr = make_trainer("rearrange/dagger_nav2d_rearrange_geodesic.yaml", folder, a)
        B, im, envs, N = tr._agent.rollouts.buffers, tr._imitation, tr.envs, tr.envs.num_envs
        im["u"] = torch.rand(a.steps, N, device=tr.device)
        acts = B["actions"][0].clone()

        def label_and_mix():
            envs.expert_actions(out=B["expert_actions"][0], status=im["status"])
            _lib.check(_lib.lib().hab_dagger_mix(_lib.ptr(acts), _lib.ptr(B["expert_actions"][0]), _lib.ptr(im["status"]),
                                                 _lib.ptr(B["masks"][0]), _lib.ptr(im["u"][0]), None, 0.5, 1.0, _lib.ptr(im["prev_expert"]),
                                                 _lib.ptr(B["expert_weights"][0]), _lib.ptr(im["agree"]), N, _lib.stream_ptr()))

        obs = {k: v[1] for k, v in B["observations"].items()}

        def step():
            envs.step_into_obs(obs, B["rewards"][0], B["masks"][1], actions=acts)

        lm, st = device_us(label_and_mix, a.calls), device_us(step, a.calls)
        print(f"label + mix: {lm[0]:.1f} us on the device, {lm[1]:.1f} us per call on the host   env step: {st[0]:.1f} us on the device, "
              f"{st[1]:.1f} us per call on the host   ({N} envs, {a.size} x {a.size})", flush=True)
        im["agree"].zero_()
        with tempfile.TemporaryDirectory() as folder2:
            ppo = make_trainer("rearrange/ddppo_nav2d_rearrange_geodesic.yaml", folder2, a)
            (dm, dlo, dhi), (pm, plo, phi) = alternated_minibatch_ms([tr, ppo], a.cycles)
            ppo.envs.close()
        tr.envs.close()
    print(f"minibatch ({a.envs} envs x {a.steps} steps / num_mini_batch, updates alternated, median (min .. max) of {a.cycles}): "
          f"DAgger {dm:.2f} ({dlo:.2f} .. {dhi:.2f}) ms, PPO {pm:.2f} ({plo:.2f} .. {phi:.2f}) ms", flush=True)


if __name__ == "__main__":
    main()
