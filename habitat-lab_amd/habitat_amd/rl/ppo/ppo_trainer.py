"""PPOTrainer (registered as "ppo" and "ddppo"): the DD-PPO training loop of
habitat_baselines/rl/ppo/ppo_trainer.py:70-911 -- rollout collection, GAE, PPO update, preemptive
synchronisation of stragglers, statistics reduction, logging, checkpoint / resume.

Two rollout paths with identical semantics:
  * device path (env source offers `step_into`, e.g. SyntheticVectorEnv): the policy reads arena row t and
    writes values / actions / log-probs / hidden state straight into the arena, the env source writes
    row t+1; the action-sampling noise of the whole rollout is pre-drawn from the CPU generator (the same
    stream torch.multinomial would consume step by step).  No device->host transfer inside the rollout.
  * host path (any VectorEnv): the reference's per-env async_step_at / wait_step_at protocol
    (ppo_trainer.py:343-482) with batch_obs-style staging.
"""
from __future__ import annotations

import contextlib
import os
import random
import time
from collections import defaultdict, deque
from typing import Dict, Optional

import numpy as np
import torch

from habitat_amd import _lib
from habitat_amd.common.base_trainer import BaseRLTrainer
from habitat_amd.common.baseline_registry import baseline_registry
from habitat_amd.common.env_factory import instantiate
from habitat_amd.common.obs_transformers import (apply_obs_transforms_batch, apply_obs_transforms_obs_space,
                                                 get_active_obs_transforms)
from habitat_amd.common.spaces import is_continuous_action_space
from habitat_amd.config.default import Config, read_write
from habitat_amd.rl.ddppo.ddp_utils import (EXIT, StoreCounterPoller, get_distrib_size, init_distrib_slurm, load_resume_state, pin_rank_affinity, rank0_only,
                                            requeue_job, save_resume_state)
from habitat_amd.rl.ppo.policy import VISUAL_FEATURES_KEY
from habitat_amd.rl.ppo.single_agent_access_mgr import EnvironmentSpec
from habitat_amd.utils.logging import get_writer, logger
from habitat_amd.utils.timing import g_timer

import habitat_amd.rl.ddppo  # noqa: F401  (registers DDPPO)
import habitat_amd.rl.ppo  # noqa: F401  (registers policies / PPO)
import habitat_amd.rl.ppo.single_agent_access_mgr  # noqa: F401
import habitat_amd.rl.ver  # noqa: F401  (registers VERRolloutStorage)


def host_env_action(act: torch.Tensor, action_space):
    """What the host path hands an env for one env's action row (ppo_trainer.py, _compute_actions_and_step_envs): a continuous action
    clipped to the Box as a numpy array, a discrete one as a Python int.  The rollout keeps the unclipped action."""
    if is_continuous_action_space(action_space):
        return np.clip(act.numpy(), action_space.low, action_space.high)
    return act.item()


def batch_obs(observations, device):
    """utils/common.py:244-310: list of per-env obs dicts -> dict of batched tensors (largest sensor first, pinned
    staging, non-blocking upload).  Sensor values may be numpy arrays / scalars (the simulator's CPU sensors) or torch tensors on any
    device (GPU-to-GPU sensors): tensors are stacked where they live and moved once."""
    first = observations[0]
    size = lambda v: v.numel() * v.element_size() if torch.is_tensor(v) else np.asarray(v).nbytes
    keys = sorted(first.keys(), key=lambda k: -size(first[k]))
    device = torch.device(device)
    out = {}
    for k in keys:
        if torch.is_tensor(first[k]):
            out[k] = torch.stack([o[k] for o in observations]).to(device, non_blocking=True)
            continue
        t = torch.from_numpy(np.stack([np.asarray(o[k]) for o in observations]))
        if device.type == "cuda":
            t = t.pin_memory().to(device, non_blocking=True)
        out[k] = t
    return out


# ---- imitation (DAgger): habitat_baselines.rl.imitation --------------------------------------------------------------------------
def imitation_settings(config):
    """The `habitat_baselines.rl.imitation` block where it is enabled, else None (absent block included)."""
    im = config.habitat_baselines.rl.get("imitation")
    return im if im is not None and im.get("enabled", False) else None


def imitation_beta(im, updates_done: int) -> float:
    """The share of steps that execute the teacher's action: linear in the number of updates done, beta_start at 0, beta_end from
    beta_decay_updates on.  num_updates_done is part of the resume state, so a resumed run continues the line."""
    decay = float(im.beta_decay_updates)
    frac = 1.0 if decay <= 0 else min(max(updates_done / decay, 0.0), 1.0)
    return float(im.beta_start + (im.beta_end - im.beta_start) * frac)


def refuse_imitation_config(config, ver: bool = False, distributed: bool = False):
    """What of an imitation run can be refused from the configuration alone; returns the enabled block or None."""
    hb = config.habitat_baselines
    im = imitation_settings(config)
    names = (hb.updater_name, hb.rollout_storage_name)
    if im is None:
        if hb.updater_name in ("DAgger", "DDDAgger") or hb.distrib_updater_name == "DDDAgger" or hb.rollout_storage_name == "ImitationRolloutStorage":
            raise _lib.HabError("imitation: updater DAgger and ImitationRolloutStorage need habitat_baselines.rl.imitation.enabled=True "
                                "(without it nothing labels the rollout)")
        return None
    if ver:
        raise _lib.HabError("imitation: the VER trainer is not supported (its storage and loss carry importance weights the BC loss has "
                            "no place for); use trainer_name ppo or ddppo")
    if names != ("DAgger", "ImitationRolloutStorage"):
        raise _lib.HabError(f"imitation: updater_name / rollout_storage_name must be the pair DAgger / ImitationRolloutStorage, the "
                            f"configuration has {names[0]} / {names[1]}")
    if distributed and hb.distrib_updater_name != "DDDAgger":
        raise _lib.HabError(f"imitation: a distributed run needs distrib_updater_name DDDAgger, the configuration has "
                            f"{hb.distrib_updater_name}")
    if hb.rl.ppo.use_double_buffered_sampler:
        raise _lib.HabError("imitation: use_double_buffered_sampler is not supported (the teacher labels all envs in one launch)")
    for k in ("beta_start", "beta_end"):
        if not 0.0 <= float(im[k]) <= 1.0:
            raise _lib.HabError(f"imitation: {k} {im[k]!r} must lie in [0, 1]")
    if not (np.isfinite(float(im.inflection_weight_coef)) and float(im.inflection_weight_coef) >= 0.0):
        raise _lib.HabError(f"imitation: inflection_weight_coef {im.inflection_weight_coef!r} must be finite and >= 0")
    return im


def refuse_imitation_envs(envs, device_envs: bool, probe: bool = True) -> None:
    """What of an imitation run can be refused once the envs exist.  The contract of an env source that can teach is one method,
    `expert_actions(out=None, mask=None, next_d=None, status=None)`, which raises HabError with its reason where it cannot (a task
    without a teacher, the Euclidean mode); `probe` makes that one call, after the envs' first reset."""
    if not device_envs:
        raise _lib.HabError("imitation: the host rollout path is not supported: the teacher labels the envs on the device, so the env "
                            "source must offer step_into_obs and the trainer must run on a GPU")
    if not hasattr(envs, "expert_actions"):
        raise _lib.HabError(f"imitation: {type(envs).__name__}: the env source has no expert_actions (no teacher)")
    if not probe:
        return
    try:  # one probing call (the teacher reads the env's records and writes none): an env that cannot teach says why itself
        envs.expert_actions()
    except _lib.HabError as err:
        raise _lib.HabError(f"imitation: {err}") from err


@baseline_registry.register_trainer(name="ddppo")
@baseline_registry.register_trainer(name="ppo")
class PPOTrainer(BaseRLTrainer):
    supported_tasks = ["Nav-v0", "ObjectNav-v1", "Nav2D-v0", "Nav2DObj-v0", "Nav2DRearr-v0", "Nav2DRearrVel-v0", "Nav2DSocial-v0",
                       "Nav2DExplore-v0", "Nav2DImageNav-v0"]
    SHORT_ROLLOUT_THRESHOLD: float = 0.25

    def __init__(self, config=None):
        super().__init__(config)
        self._agent = None
        self.envs = None
        self.obs_transforms = []
        self._env_spec = None
        self._is_distributed = get_distrib_size()[2] > 1
        self._straggler_delay_s = 0.0  # test hook: artificial per-step delay on this rank

    # ---- collectives -----------------------------------------------------------------------------------
    def _all_reduce(self, t: torch.Tensor) -> torch.Tensor:
        if not self._is_distributed:
            return t
        orig = t.device
        t = t.to(device=self.device)
        torch.distributed.all_reduce(t)
        return t.to(device=orig)

    # ---- construction ------------------------------------------------------------------------------------
    def _init_envs(self, config=None, is_eval: bool = False):
        config = config or self.config
        factory = instantiate(config.habitat_baselines.vector_env_factory)
        kw = {}
        if "device" in factory.construct_envs.__code__.co_varnames:
            kw["device"] = self.device
        self.envs = factory.construct_envs(config, workers_ignore_signals=False,
                                           enforce_scenes_greater_eq_environments=is_eval,
                                           is_first_rank=(not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0),
                                           **kw)
        self._env_spec = EnvironmentSpec(self.envs.observation_spaces[0], self.envs.action_spaces[0], self.envs.orig_action_spaces[0])
        # ppo_trainer.py:110-115: the policy and the rollout storage see the TRANSFORMED observation space
        self.obs_transforms = get_active_obs_transforms(config)
        self._env_spec.observation_space = apply_obs_transforms_obs_space(self._env_spec.observation_space, self.obs_transforms)
        self._rank0_keys = set()
        self._single_proc_infos = {}

    def _create_agent(self, resume_state, **kwargs):
        cls = baseline_registry.get_agent_access_mgr(self.config.habitat_baselines.rl.agent.type)
        return cls(config=self.config, env_spec=self._env_spec, is_distrib=self._is_distributed, device=self.device,
                   resume_state=resume_state, num_envs=self.envs.num_envs, percent_done_fn=self.percent_done, **kwargs)

    def _init_train(self, resume_state=None):
        if resume_state is None:
            resume_state = load_resume_state(self.config)
        hb = self.config.habitat_baselines
        if resume_state is not None and not hb.load_resume_state_config:
            raise FileExistsError("habitat_baselines.load_resume_state_config=False but a previous training run exists in "
                                  f"{hb.checkpoint_folder}")
        if hb.rl.ddppo.force_distributed:
            self._is_distributed = True
        imitation = refuse_imitation_config(self.config, distributed=self._is_distributed)
        self._add_preemption_signal_handlers()
        if self._is_distributed:
            local_rank, tcp_store = init_distrib_slurm(hb.rl.ddppo.distrib_backend)
            # each rank's launch thread (and its env workers) on its own block of host cores; the masks are compared through the store:
            # no collective may run before the rank has selected its GPU (below)
            pin_rank_affinity(local_rank, store=tcp_store)
            if rank0_only():
                logger.info("Initialized DD-PPO with {} workers".format(torch.distributed.get_world_size()))
            with read_write(self.config):
                # one GPU per rank; ranks wrap around when a box has fewer devices than ranks (debug runs on one GPU)
                hb.torch_gpu_id = local_rank % max(1, torch.cuda.device_count()) if torch.cuda.is_available() else local_rank
                # make sure every env of every rank gets a unique seed (ppo_trainer.py:208-211)
                self.config.habitat.seed += torch.distributed.get_rank() * hb.num_environments
            random.seed(self.config.habitat.seed)
            np.random.seed(self.config.habitat.seed)
            torch.manual_seed(self.config.habitat.seed)
            self.num_rollouts_done_store = torch.distributed.PrefixStore("rollout_tracker", tcp_store)
            self.num_rollouts_done_store.set("num_done", "0")
        if torch.cuda.is_available():
            self.device = torch.device("cuda", hb.torch_gpu_id)
            torch.cuda.set_device(self.device)
        else:
            self.device = torch.device("cpu")
        self._init_envs()
        if imitation is not None:
            refuse_imitation_envs(self.envs, hasattr(self.envs, "step_into_obs") and self.device.type == "cuda", probe=False)
        if rank0_only() and not os.path.isdir(hb.checkpoint_folder):
            os.makedirs(hb.checkpoint_folder, exist_ok=True)
        self._agent = self._create_agent(resume_state)
        if self._is_distributed:
            self._agent.init_distributed(find_unused_params=False)
        self._agent.post_init()
        self._ppo_cfg = hb.rl.ppo
        # frozen visual encoder (ppo_trainer.py:261-279): the rollout stores the encoder's output next to the sensors
        self._is_static_encoder = not hb.rl.ddppo.train_encoder
        self._encoder = self._agent.actor_critic.visual_encoder if self._is_static_encoder else None
        self._device_envs = hasattr(self.envs, "step_into_obs") and self.device.type == "cuda"
        st = self._agent.rollouts
        N = self.envs.num_envs
        # obs transforms on the device-env path (ppo_trainer.py:421 `apply_obs_transforms_batch` after every env step): the env source
        # writes the sensors at their own size into a staging row, the transforms (device kernels, common/obs_transformers.py) write
        # the rollout row
        self._raw_obs = None
        if self._device_envs and self.obs_transforms:
            raw_space = self.envs.observation_spaces[0]
            self._raw_obs = {k: torch.zeros((N,) + tuple(sp.shape), dtype=getattr(torch, np.dtype(sp.dtype).name), device=self.device)
                             for k, sp in raw_space.spaces.items()}
        if self._device_envs:
            o0 = st.buffers["observations"]
            self._device_obs_into({k: v[0] for k, v in o0.items() if k != VISUAL_FEATURES_KEY}, self.envs.reset_into_obs)
            if self._is_static_encoder:
                self._agent.actor_critic.encode_visual({k: v[0] for k, v in o0.items()}, out=o0[VISUAL_FEATURES_KEY][0])
            stat_dev = self.device
        else:
            observations = self.envs.post_step(self.envs.reset())
            batch = apply_obs_transforms_batch(batch_obs(observations, self.device), self.obs_transforms)
            if self._is_static_encoder:
                batch[VISUAL_FEATURES_KEY] = self._encoder(batch)
            st.insert_first_observations(batch)
            stat_dev = torch.device("cpu")
        self.current_episode_reward = torch.zeros(N, 1, device=stat_dev)
        self.running_episode_stats = dict(count=torch.zeros(N, 1, device=stat_dev), reward=torch.zeros(N, 1, device=stat_dev))
        self.window_episode_stats = defaultdict(lambda: deque(maxlen=self._ppo_cfg.reward_window_size))
        self._measure_base = None  # see _coalesce_post_step
        self._imitation = None
        if imitation is not None:
            refuse_imitation_envs(self.envs, self._device_envs)  # the probing call, now that the envs hold their first episodes
            # DAgger: what the rollout step needs beside the storage's two rows.  prev_expert is the mix kernel's carry (the label of
            # each env's previous step, -1 before the first) and belongs to the resume state; agree = (agreements, weighted samples)
            # since the last update
            self._imitation = dict(cfg=imitation, beta=imitation_beta(imitation, self.num_updates_done), u=None, counts=(0, 0),
                                   prev_expert=torch.full((N,), -1, dtype=torch.int64, device=self.device),
                                   status=torch.zeros(N, dtype=torch.int32, device=self.device),
                                   agree=torch.zeros(2, dtype=torch.int64, device=self.device))
            if resume_state is not None and "imitation_prev_expert" in resume_state.get("requeue_stats", {}):
                self._imitation["prev_expert"].copy_(resume_state["requeue_stats"]["imitation_prev_expert"])
            self._agent.updater.rollout_counters = self._imitation["agree"]  # read with the updater's metrics, in its one transfer
        self.t_start = time.time()

    # ---- checkpoints ---------------------------------------------------------------------------------------
    @rank0_only
    def save_checkpoint(self, file_name: str, extra_state: Optional[Dict] = None) -> None:
        checkpoint = {**self._agent.get_save_state(), "config": self.config.to_dict() if hasattr(self.config, "to_dict") else self.config}
        if extra_state is not None:
            checkpoint["extra_state"] = extra_state
        folder = self.config.habitat_baselines.checkpoint_folder
        torch.save(checkpoint, os.path.join(folder, file_name))
        torch.save(checkpoint, os.path.join(folder, "latest.pth"))

    def load_checkpoint(self, checkpoint_path: str, *args, **kwargs) -> Dict:
        kwargs.setdefault("weights_only", False)
        return torch.load(checkpoint_path, *args, **kwargs)

    # ---- rollout: device path ---------------------------------------------------------------------------------
    def _draw_rollout_noise(self, T: int):
        """T successive (N, A) Exp(1) draws from the CPU generator = the draws torch.multinomial would make."""
        ac = self._agent.actor_critic
        N, A = self.envs.num_envs, ac.dim_actions
        if getattr(ac, "action_distribution_type", "categorical") == "gaussian":  # CustomNormal.rsample's N(0, 1) draws
            q = torch.stack([torch.empty(N, A).normal_() for _ in range(T)])
        else:
            q = torch.stack([torch.empty(N, A).exponential_(1) for _ in range(T)])
        return q.pin_memory().to(self.device, non_blocking=True)

    def _device_obs_into(self, rows, emit):
        """`emit(dict of (N, ...) device tensors)` writes the env source's observations; with obs transforms they go through a
        sensor-sized staging row and the transforms write the (transformed-size) rollout rows."""
        if self._raw_obs is None:
            emit(rows)
            return
        emit(self._raw_obs)
        out = apply_obs_transforms_batch(dict(self._raw_obs), self.obs_transforms)
        for k, v in rows.items():
            v.copy_(out[k])

    def _device_rollout_step(self, t: int, noise: torch.Tensor):
        st = self._agent.rollouts
        B = st.buffers
        ac = self._agent.actor_critic
        obs = B["observations"]
        with g_timer.avg_time("trainer.sample_action"):
            ac.act({k: v[t] for k, v in obs.items()}, B["recurrent_hidden_states"][t], B["prev_actions"][t], B["masks"][t],
                   exp_noise=noise[t],
                   out=dict(values=B["value_preds"][t], actions=B["actions"][t], action_log_probs=B["action_log_probs"][t],
                            rnn_hidden_states=B["recurrent_hidden_states"][t + 1]))
        im = getattr(self, "_imitation", None)
        if im is not None:
            # DAgger: the env's teacher labels the state the policy just acted in (it reads the env's records and writes none), then
            # one launch weighs the label and replaces the sampled action by it where u < beta.  The env, the episode bookkeeping
            # and prev_actions[t + 1] below see the EXECUTED action; action_log_probs[t] stays the policy sample's and is unused.
            with g_timer.avg_time("trainer.imitation_label"):
                self.envs.expert_actions(out=B["expert_actions"][t], status=im["status"])
                _lib.check(_lib.lib().hab_dagger_mix(
                    _lib.ptr(B["actions"][t]), _lib.ptr(B["expert_actions"][t]), _lib.ptr(im["status"]), _lib.ptr(B["masks"][t]),
                    _lib.ptr(im["u"][t]), None, float(im["beta"]), float(im["cfg"].inflection_weight_coef), _lib.ptr(im["prev_expert"]),
                    _lib.ptr(B["expert_weights"][t]), _lib.ptr(im["agree"]), self.envs.num_envs, _lib.stream_ptr()), "hab_dagger_mix")
        with g_timer.avg_time("trainer.step_env"):
            # an env whose observations depend on the actions (consumes_actions, e.g. Nav2DVectorEnv) is handed the row the policy
            # just wrote for THIS step
            kw = dict(actions=B["actions"][t]) if getattr(self.envs, "consumes_actions", False) else {}
            self._device_obs_into({k: v[t + 1] for k, v in obs.items() if k != VISUAL_FEATURES_KEY},
                                  lambda rows: self.envs.step_into_obs(rows, B["rewards"][t], B["masks"][t + 1], **kw))
            if self._is_static_encoder:  # ppo_trainer.py:467-471
                ac.encode_visual({k: v[t + 1] for k, v in obs.items()}, out=obs[VISUAL_FEATURES_KEY][t + 1])
        with g_timer.avg_time("trainer.update_stats"):
            # episode bookkeeping (ppo_trainer.py:417-446) and prev_actions[t+1] = actions[t], one launch
            acts = B["actions"][t]
            discrete = acts.dtype == torch.int64
            if not discrete:  # continuous actions (float rows): plain row copy
                B["prev_actions"][t + 1].copy_(acts)
            _lib.check(_lib.lib().hab_rollout_step_stats(
                _lib.ptr(B["rewards"][t]), _lib.ptr(B["masks"][t + 1]), _lib.ptr(self.current_episode_reward),
                _lib.ptr(self.running_episode_stats["reward"]), _lib.ptr(self.running_episode_stats["count"]),
                _lib.ptr(acts) if discrete else None, _lib.ptr(B["prev_actions"][t + 1]) if discrete else None, self.envs.num_envs,
                acts.shape[-1], _lib.stream_ptr()))
        st.advance_rollout()
        return self.envs.num_envs

    # ---- rollout: host path (ppo_trainer.py:343-482) -------------------------------------------------------------
    def _compute_actions_and_step_envs(self, buffer_index: int = 0):
        num_envs = self.envs.num_envs
        nb = self._agent.nbuffers
        env_slice = slice(int(buffer_index * num_envs / nb), int((buffer_index + 1) * num_envs / nb))
        with g_timer.avg_time("trainer.sample_action"):
            step_batch = self._agent.rollouts.get_current_step(env_slice, buffer_index)
            action_data = self._agent.actor_critic.act(
                {k: v.contiguous() for k, v in step_batch["observations"].items()}, step_batch["recurrent_hidden_states"],
                step_batch["prev_actions"], step_batch["masks"])
        with g_timer.avg_time("trainer.obs_insert"):
            for index_env, act in zip(range(env_slice.start, env_slice.stop), action_data.env_actions.cpu().unbind(0)):
                self.envs.async_step_at(index_env, host_env_action(act, self._env_spec.action_space))
            self._agent.rollouts.insert(next_recurrent_hidden_states=action_data.rnn_hidden_states, actions=action_data.actions,
                                        action_log_probs=action_data.action_log_probs, value_preds=action_data.values,
                                        buffer_index=buffer_index)

    def _collect_environment_result(self, buffer_index: int = 0):
        num_envs = self.envs.num_envs
        nb = self._agent.nbuffers
        env_slice = slice(int(buffer_index * num_envs / nb), int((buffer_index + 1) * num_envs / nb))
        with g_timer.avg_time("trainer.step_env"):
            outputs = [self.envs.wait_step_at(i) for i in range(env_slice.start, env_slice.stop)]
            observations, rewards_l, dones, infos = [list(x) for x in zip(*outputs)]
        with g_timer.avg_time("trainer.update_stats"):
            observations = self.envs.post_step(observations)
            slab_keys = set(getattr(self.envs, "shared_obs_keys", ()))
            if slab_keys:
                # shared-memory observation plane (core/vector_env.py): one H2D copy per sensor from the rows the workers wrote
                batch = self.envs.batched_obs(env_slice, self.device)
                if any(k not in slab_keys for k in observations[0]):
                    batch.update(batch_obs([{k: v for k, v in o.items() if k not in slab_keys} for o in observations], self.device))
            else:
                batch = batch_obs(observations, self.device)
            batch = apply_obs_transforms_batch(batch, self.obs_transforms)  # ppo_trainer.py:421
            if self._is_static_encoder:  # ppo_trainer.py:467-471
                batch[VISUAL_FEATURES_KEY] = self._encoder(batch)
            cdev = self.current_episode_reward.device
            rewards = torch.tensor(rewards_l, dtype=torch.float, device=cdev).unsqueeze(1)
            not_done_masks = torch.tensor([[not d] for d in dones], dtype=torch.bool, device=cdev)
            done_masks = torch.logical_not(not_done_masks)
            self.current_episode_reward[env_slice] += rewards
            cur = self.current_episode_reward[env_slice]
            self.running_episode_stats["reward"][env_slice] += cur.where(done_masks, cur.new_zeros(()))
            self.running_episode_stats["count"][env_slice] += done_masks.float()
            # the keys of every env's info, not only of env 0's: an env may report its measures only with the step that ends an
            # episode (Nav2DVectorEnv) and {} otherwise; a missing value counts 0 and is masked out below unless that env is done
            for k in dict.fromkeys(k for i in infos for k in (i or {})):
                vals = [(i or {}).get(k, 0.0) for i in infos]
                if all(isinstance(v, (int, float)) for v in vals):
                    v = torch.tensor(vals, dtype=torch.float, device=cdev).unsqueeze(1)
                    if k not in self.running_episode_stats:
                        self.running_episode_stats[k] = torch.zeros_like(self.running_episode_stats["count"])
                    self.running_episode_stats[k][env_slice] += v.where(done_masks, v.new_zeros(()))
            self.current_episode_reward[env_slice].masked_fill_(done_masks, 0.0)
        self._agent.rollouts.insert(next_observations=batch, rewards=rewards.to(self.device), next_masks=not_done_masks.to(self.device),
                                    buffer_index=buffer_index)
        self._agent.rollouts.advance_rollout(buffer_index)
        return env_slice.stop - env_slice.start

    # ---- update ----------------------------------------------------------------------------------------------------
    def _update_agent(self):
        with g_timer.avg_time("trainer.update_agent"):
            st = self._agent.rollouts
            last = st.get_last_step()
            next_value = self._agent.actor_critic.get_value({k: v.contiguous() for k, v in last["observations"].items()},
                                                            last["recurrent_hidden_states"], last["prev_actions"], last["masks"])
            st.compute_returns(next_value, self._ppo_cfg.use_gae, self._ppo_cfg.gamma, self._ppo_cfg.tau)
            self._agent.train()
            losses = self._agent.updater.update(st)
            st.after_update()
            self._agent.after_update()
            im = getattr(self, "_imitation", None)
            if im is not None:  # the rollout's agreement counters came to the host in the updater's one read, which also zeroed them
                agreed, counted = im["counts"] = self._agent.updater.last_rollout_counts
                losses = dict(losses, imitation_agreement=agreed / max(counted, 1), imitation_beta=float(im["beta"]))
        return losses

    def _coalesce_post_step(self, losses: Dict[str, float], count_steps_delta: int) -> Dict[str, float]:
        sums = getattr(getattr(self, "envs", None), "measure_sums", None) if getattr(self, "_device_envs", False) else None
        if sums is not None:  # device path: the env accumulates its episode measures itself (the host path reads them from infos)
            count = self.running_episode_stats["count"]
            if getattr(self, "_measure_base", None) is None:
                # the env's sums count from its construction; what the statistics held before that (restored by a resume, else
                # nothing) stays underneath them, so that the window's differences never run backwards
                self._measure_base = {k: self.running_episode_stats.get(k, torch.zeros_like(count)).clone() for k in self.envs.measure_names}
            for i, k in enumerate(self.envs.measure_names):
                self.running_episode_stats[k] = self._measure_base[k] + sums[i].to(count).unsqueeze(1)
        order = sorted(self.running_episode_stats.keys())
        stats = torch.stack([self.running_episode_stats[k] for k in order], 0)
        stats = self._all_reduce(stats)
        stats_cpu = stats.cpu()
        for i, k in enumerate(order):
            self.window_episode_stats[k].append(stats_cpu[i])
        if self._is_distributed:
            names = sorted(losses.keys())
            t = torch.tensor([losses[k] for k in names] + [count_steps_delta], device="cpu", dtype=torch.float32)
            t = self._all_reduce(t)
            count_steps_delta = int(t[-1].item())
            t /= torch.distributed.get_world_size()
            losses = {k: t[i].item() for i, k in enumerate(names)}
        if self._is_distributed and rank0_only():
            self.num_rollouts_done_store.set("num_done", "0")
        self.num_steps_done += count_steps_delta
        return losses

    @rank0_only
    def _training_log(self, writer, losses: Dict[str, float], prev_time: int = 0):
        deltas = {k: ((v[-1] - v[0]).sum().item() if len(v) > 1 else v[0].sum().item()) for k, v in self.window_episode_stats.items()}
        deltas["count"] = max(deltas["count"], 1.0)
        writer.add_scalar("reward", deltas["reward"] / deltas["count"], self.num_steps_done)
        for k, v in deltas.items():
            if k not in {"reward", "count"}:
                writer.add_scalar(f"metrics/{k}", v / deltas["count"], self.num_steps_done)
        for k, v in losses.items():
            writer.add_scalar(f"learner/{k}", v, self.num_steps_done)
        fps = self.num_steps_done / ((time.time() - self.t_start) + prev_time)
        writer.add_scalar("perf/fps", fps, self.num_steps_done)
        for name, val in g_timer.items():
            writer.add_scalar(f"perf/{name}", val.mean, self.num_steps_done)
        self.last_fps = fps
        if self.num_updates_done % self.config.habitat_baselines.log_interval == 0:
            logger.info("update: {}\tfps: {:.3f}\t".format(self.num_updates_done, fps))
            logger.info(f"Num updates: {self.num_updates_done}\tNum frames {self.num_steps_done}")
            logger.info("Average window size: {}  {}".format(
                len(self.window_episode_stats["count"]),
                "  ".join("{}: {:.3f}".format(k, v / deltas["count"]) for k, v in deltas.items() if k != "count")))
            logger.info("\tPerf Stats: " + " ".join(f"{k}: {v.mean:.3f}" for k, v in g_timer.items()))

    def should_end_early(self, rollout_step) -> bool:
        """DD-PPO preemptive synchronisation of stragglers (ppo_trainer.py:641-653)."""
        if not self._is_distributed:
            return False
        if rollout_step < self.config.habitat_baselines.rl.ppo.num_steps * self.SHORT_ROLLOUT_THRESHOLD:
            return False
        poller = getattr(self, "_num_done_poller", None)  # active inside device-path rollouts only (ddp_utils.StoreCounterPoller)
        num_done = poller.read() if poller is not None else int(self.num_rollouts_done_store.get("num_done"))
        return num_done >= self.config.habitat_baselines.rl.ddppo.sync_frac * torch.distributed.get_world_size()

    # ---- main loop (ppo_trainer.py:656-801) ----------------------------------------------------------------------------
    def train(self) -> None:
        resume_state = load_resume_state(self.config)
        self._init_train(resume_state)
        count_checkpoints, prev_time = 0, 0
        if self._is_distributed:
            torch.distributed.barrier()
        if resume_state is not None:
            rs = resume_state["requeue_stats"]
            self.num_steps_done, self.num_updates_done = rs["num_steps_done"], rs["num_updates_done"]
            self._last_checkpoint_percent = rs["_last_checkpoint_percent"]
            count_checkpoints, prev_time = rs["count_checkpoints"], rs["prev_time"]
            self.running_episode_stats = {k: v.to(self.current_episode_reward.device) for k, v in rs["running_episode_stats"].items()}
            self.window_episode_stats.update(rs["window_episode_stats"])
        with (get_writer(self.config, flush_secs=self.flush_secs) if rank0_only() else contextlib.nullcontext()) as writer:
            while not self.is_done():
                if rank0_only() and self._should_save_resume_state():
                    requeue_stats = dict(count_checkpoints=count_checkpoints, num_steps_done=self.num_steps_done,
                                         num_updates_done=self.num_updates_done, _last_checkpoint_percent=self._last_checkpoint_percent,
                                         prev_time=(time.time() - self.t_start) + prev_time,
                                         running_episode_stats={k: v.cpu() for k, v in self.running_episode_stats.items()},
                                         window_episode_stats=dict(self.window_episode_stats))
                    if getattr(self, "_imitation", None) is not None:
                        requeue_stats["imitation_prev_expert"] = self._imitation["prev_expert"].cpu()
                    save_resume_state(dict(**self._agent.get_resume_state(), config=self.config.to_dict(), requeue_stats=requeue_stats),
                                      self.config)
                if EXIT.is_set():
                    self.envs.close()
                    requeue_job()
                    return
                losses = self.run_update_cycle()
                self._training_log(writer, losses, prev_time)
                if rank0_only() and self.should_checkpoint():
                    self.save_checkpoint(f"ckpt.{count_checkpoints}.pth",
                                         dict(step=self.num_steps_done, wall_time=(time.time() - self.t_start) + prev_time))
                    count_checkpoints += 1
            self.envs.close()
            self.shutdown()

    def shutdown(self) -> None:
        """Teardown of what the trainer started besides the envs: the straggler-counter polling thread must be joined BEFORE the
        process group / rendezvous store is destroyed (it may sit inside a blocking TCPStore call)."""
        poller = getattr(self, "_num_done_poller", None)
        if poller is not None:
            poller.stop()
            self._num_done_poller = None

    def run_update_cycle(self) -> Dict[str, float]:
        """One full cycle of the hot path: rollout collection -> GAE -> PPO update -> statistics reduction."""
        self._agent.pre_rollout()
        self._agent.eval()
        count_steps_delta = self.collect_rollout()
        self.local_steps_done = getattr(self, "local_steps_done", 0) + count_steps_delta  # this rank only (num_steps_done is global)
        if self._is_distributed:
            self.num_rollouts_done_store.add("num_done", 1)
        losses = self._update_agent()
        self.num_updates_done += 1
        return self._coalesce_post_step(losses, count_steps_delta)

    def collect_rollout(self) -> int:
        """One rollout of up to num_steps steps (ends early under should_end_early).  Returns env-steps collected."""
        T = self._ppo_cfg.num_steps
        count = 0
        with g_timer.avg_time("trainer.rollout_collect"):
            if self._device_envs:
                noise = self._draw_rollout_noise(T)
                im = getattr(self, "_imitation", None)
                if im is not None:  # the mix's uniforms, (T, N) in [0, 1) from the CPU generator after the sampling noise
                    im["beta"] = imitation_beta(im["cfg"], self.num_updates_done)
                    im["u"] = torch.rand(T, self.envs.num_envs).pin_memory().to(self.device, non_blocking=True)
                # a rollout step is ~200 us of GPU work: the straggler counter is read through a cached poller, not one TCP round
                # trip per step (at most 0.5 ms older than the reference's per-step query)
                polling = contextlib.nullcontext()
                if self._is_distributed:
                    if getattr(self, "_num_done_poller", None) is None:
                        self._num_done_poller = StoreCounterPoller(self.num_rollouts_done_store, "num_done")
                    polling = self._num_done_poller.polling()
                with polling:
                    for step in range(T):
                        count += self._device_rollout_step(step, noise)
                        if self._straggler_delay_s:
                            time.sleep(self._straggler_delay_s)
                        if self.should_end_early(step + 1):
                            break
            else:
                nb = self._agent.nbuffers
                for b in range(nb):
                    self._compute_actions_and_step_envs(b)
                for step in range(T):
                    is_last = self.should_end_early(step + 1) or (step + 1) == T
                    for b in range(nb):
                        count += self._collect_environment_result(b)
                        if not is_last:
                            self._compute_actions_and_step_envs(b)
                    if is_last:
                        break
        return count

    def _eval_checkpoint(self, checkpoint_path: str, writer, checkpoint_index: int = 0) -> None:
        """ppo_trainer.py:803-902: load one checkpoint, rebuild envs + agent from its configuration, run the evaluator."""
        if self._is_distributed:
            raise RuntimeError("Evaluation does not support distributed mode")
        hb = self.config.habitat_baselines
        if hb.eval.should_load_ckpt:
            ckpt_dict = self.load_checkpoint(checkpoint_path, map_location="cpu")
            logger.info(f"Loaded checkpoint trained for {ckpt_dict.get('extra_state', {}).get('step')} steps")
        else:
            ckpt_dict = {"config": None}
        config = self._get_resume_state_config_or_new_config(ckpt_dict.get("config") if hb.eval.use_ckpt_config else None)
        with read_write(config):
            config.habitat.dataset.split = hb.eval.split
            # as the reference's eval does: a video needs the map, so the measurement is added before the envs are built
            if len(hb.eval.video_option) > 0 and getattr(config.habitat.task.measurements, "top_down_map", None) is None:
                config.habitat.task.measurements["top_down_map"] = Config()
        self.device = torch.device("cuda", hb.torch_gpu_id) if torch.cuda.is_available() else torch.device("cpu")
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        self._init_envs(config, is_eval=True)
        self._agent = self._create_agent(None)
        if self._agent.actor_critic.should_load_agent_state and hb.eval.should_load_ckpt:
            self._agent.load_state_dict(ckpt_dict)
        step_id = checkpoint_index
        if "extra_state" in ckpt_dict and "step" in ckpt_dict["extra_state"]:
            step_id = ckpt_dict["extra_state"]["step"]
        evaluator = instantiate(hb.evaluator)
        from habitat_amd.rl.ppo.evaluator import Evaluator
        assert isinstance(evaluator, Evaluator)
        self.last_eval_stats = evaluator.evaluate_agent(self._agent, self.envs, self.config, checkpoint_index, step_id, writer, self.device,
                                                        self.obs_transforms, self._env_spec, self._rank0_keys)
        self.envs.close()
