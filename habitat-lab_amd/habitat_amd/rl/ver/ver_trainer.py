"""VERTrainer (registered as "ver"): Variable Experience Rollouts, habitat_baselines/rl/ver/ver_trainer.py:66-580.

A rollout collects a fixed number of STEPS (num_envs * num_steps; the first one fills the whole buffer) from whichever environments
deliver them: the inference worker batches the environments whose step has arrived, so slow environments do not hold the policy
(or the other environments) up.  The update is PPO on the linear step buffer with importance weights for the uneven per-environment
sampling (VERRolloutStorage / `hab_ppo_loss_ver`), the learning-rate schedule is the reference's cosine decay.

Arrangement (ver_trainer.py:261-337): `rl.ver.num_inference_workers` inference workers batch the arrived environment steps.  They
are threads of this process with their own HIP stream over the one device arena (rl/ver/inference_worker.py); without
`overlap_rollouts_and_learn` worker 0 is the trainer's own thread (`main_is_iw`) and the learner updates in place between rollouts.
With `overlap_rollouts_and_learn=True` every worker is a thread, the finished rollout is copied into the learner's private arena
(`learning_rollouts`) and the workers start on the next rollout while the learner works on the previous one (ver_trainer.py:504-530);
the workers act with the parameters of the last COMPLETED policy version, which the learner publishes after every update.
Environment workers are the process-per-environment VectorEnv workers (shared-memory observation plane) or, for the synthetic
benchmark source, the device-resident generator.

Straggler preemption (ver_trainer.py:158,224-233, rl/ver/preemption_decider.py): started whenever `variable_experience` is on, as the
reference does.  Checked on the CPU: the schedule's arithmetic against the reference's own function, the worker protocol with deadlines,
the collectives at world sizes 2 and 8 with an injected 3x slower rank (tests/test_distributed_gloo.py); on one GPU the trainer runs with
it (tests/test_gpu_ver.py).  HAB_VER_PREEMPTION=0 switches it off: every rollout then collects its full step quota and under VER +
DD-PPO every rank waits at the barrier of `_update_agent` for the slowest rank's quota (runs that must reproduce a rollout bit for bit
across modes -- the overlapped-vs-sequential test -- do that, since a deadline depends on wall-clock step times)."""
from __future__ import annotations

import contextlib
import math
import os
import random
import time
from typing import Dict, Optional

import numpy as np
import torch

from habitat_amd import _lib
from habitat_amd.common.baseline_registry import baseline_registry
from habitat_amd.common.env_factory import instantiate
from habitat_amd.common.obs_transformers import apply_obs_transforms_obs_space, get_active_obs_transforms
from habitat_amd.config.default import read_write
from habitat_amd.rl.ddppo.ddp_utils import (EXIT, get_distrib_size, init_distrib_slurm, load_resume_state, rank0_only, requeue_job,
                                            save_resume_state)
from habitat_amd.rl.ppo.ppo_trainer import PPOTrainer, refuse_imitation_config
from habitat_amd.rl.ppo.single_agent_access_mgr import EnvironmentSpec
from habitat_amd.rl.ver.inference_worker import (InferenceWorker, InferenceWorkerPool, InferenceWorkerSync, PublishedWeights,
                                                 RequestQueue)
from habitat_amd.rl.ver.preemption_decider import PreemptionDecider
from habitat_amd.rl.ver.report_worker import ReportWorker
from habitat_amd.rl.ver.transport import DeviceEnvTransport, VectorEnvTransport
from habitat_amd.rl.ver.ver_rollout_storage import VERRolloutStorage
from habitat_amd.utils.logging import get_writer, logger
from habitat_amd.utils.timing import Timing


def cosine_decay(progress: float) -> float:
    """ver_trainer.py:57-63."""
    progress = min(max(progress, 0.0), 1.0)
    return (1.0 + math.cos(progress * math.pi)) / 2.0


@baseline_registry.register_trainer(name="ver")
class VERTrainer(PPOTrainer):
    def _create_agent(self, resume_state, **kwargs):
        cls = baseline_registry.get_agent_access_mgr(self.config.habitat_baselines.rl.agent.type)
        return cls(config=self.config, env_spec=self._env_spec, is_distrib=self._is_distributed, device=self.device,
                   resume_state=resume_state, num_envs=self.config.habitat_baselines.num_environments,
                   percent_done_fn=self.percent_done, **kwargs)

    def _init_train(self, resume_state=None):
        hb = self.config.habitat_baselines
        refuse_imitation_config(self.config, ver=True)
        if self._is_distributed:
            local_rank, world_rank, _ = get_distrib_size()
            with read_write(self.config):
                hb.torch_gpu_id = local_rank % max(1, torch.cuda.device_count()) if torch.cuda.is_available() else local_rank
                self.config.habitat.seed += world_rank * hb.num_environments  # ver_trainer.py:96-99
        random.seed(self.config.habitat.seed)
        np.random.seed(self.config.habitat.seed)
        torch.manual_seed(self.config.habitat.seed)
        if hb.rl.ddppo.force_distributed:
            self._is_distributed = True
        self._add_preemption_signal_handlers()
        if self._is_distributed:
            init_distrib_slurm(hb.rl.ddppo.distrib_backend)
            if rank0_only():
                logger.info("Initialized VER+DD-PPO with {} workers".format(torch.distributed.get_world_size()))
        else:
            logger.info("Initialized VER")
        self.device = torch.device("cuda", hb.torch_gpu_id) if torch.cuda.is_available() else torch.device("cpu")
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        if self.device.type != "cuda":
            raise _lib.HabError("the VER trainer needs a GPU (no CPU execution path)")
        self._my_t_zero = time.perf_counter()
        self._init_envs()  # environment workers (vector_env_factory) + observation-space bookkeeping of the parent
        self.ver_config = hb.rl.ver
        n_iw = int(self.ver_config.num_inference_workers)
        overlap = bool(self.ver_config.overlap_rollouts_and_learn)
        if n_iw < 1:
            raise _lib.HabError("rl.ver.num_inference_workers must be >= 1")
        if rank0_only() and not os.path.isdir(hb.checkpoint_folder):
            os.makedirs(hb.checkpoint_folder, exist_ok=True)
        self._agent = self._create_agent(resume_state, lr_schedule_fn=cosine_decay)
        ppo_cfg = hb.rl.ppo
        self._ppo_cfg = ppo_cfg

        def create_ver_rollouts(num_envs, env_spec, actor_critic, policy_action_space, config, device):
            return VERRolloutStorage(numsteps=ppo_cfg.num_steps, num_envs=num_envs,
                                     observation_space=self._agent.rollout_obs_space(env_spec, actor_critic),
                                     action_space=policy_action_space, actor_critic=actor_critic,
                                     variable_experience=self.ver_config.variable_experience, device=device)

        self._agent.post_init(create_ver_rollouts)
        # overlapped collection: the learner works on its own copy of the finished rollout (ver_trainer.py:265-269)
        self.learning_rollouts = (create_ver_rollouts(hb.num_environments, self._env_spec, self._agent.actor_critic,
                                                      self._agent.policy_action_space, self.config, self.device)
                                  if overlap else self._agent.rollouts)
        if self._is_distributed:
            self._agent.init_distributed(find_unused_params=False)
        has_report_state = resume_state is not None and "report_worker_state" in resume_state.get("requeue_stats", {})
        self._writer_cm = get_writer(self.config, flush_secs=self.flush_secs) if rank0_only() else contextlib.nullcontext()
        self._writer = self._writer_cm.__enter__()
        self.report_worker = ReportWorker(self.config, self._my_t_zero, self.num_steps_done, writer=self._writer)
        if has_report_state and resume_state["requeue_stats"]["report_worker_state"] is not None:
            self.report_worker.load_state_dict(resume_state["requeue_stats"]["report_worker_state"])
        if hasattr(self.envs, "step_into_obs"):  # device-resident synthetic source
            speeds = getattr(self.config.habitat, "synthetic", {}).get("ver_speeds", None)
            self.transport = DeviceEnvTransport(self.envs, self.report_worker, speeds=speeds, seed=self.config.habitat.seed)
        else:
            self.transport = VectorEnvTransport(self.envs, self.report_worker)
        # ---- inference workers (ver_trainer.py:261-349) ---------------------------------------------------------------------------
        main_is_iw = not overlap
        self._overlap, self._main_is_iw = overlap, main_is_iw
        self._iw_sync = InferenceWorkerSync(n_iw)
        self._iw_queue = RequestQueue(self.transport)
        self._published = PublishedWeights(self._agent.actor_critic.engine) if (n_iw > 1 or overlap) else None
        self._decider = None
        if os.environ.get("HAB_VER_PREEMPTION", "1") != "0" and self.ver_config.variable_experience:
            world = torch.distributed.get_world_size() if self._is_distributed else 1
            rank = torch.distributed.get_rank() if self._is_distributed else 0
            # host-side numpy arrays travel: a gloo group next to the RCCL one (the reference's decider opens its own, :331-334)
            group = torch.distributed.new_group(backend="gloo") if world > 1 else None
            self._decider = PreemptionDecider(self.config, self._my_t_zero, rank, world, group=group, report=self.report_worker)
        self.inference_workers = []
        for i in range(n_iw):
            own_thread = not (main_is_iw and i == 0)
            pol, stream = self._agent.actor_critic, None
            if own_thread:
                pol, stream = self._private_policy(n_iw), torch.cuda.Stream(device=self.device)
            self.inference_workers.append(InferenceWorker(self.config, pol, self._agent.rollouts, self.transport, self.device,
                                                          self.obs_transforms, num_inference_workers=n_iw, report=self.report_worker,
                                                          worker_idx=i, iw_sync=self._iw_sync, queue=self._iw_queue,
                                                          published=self._published if own_thread else None, stream=stream,
                                                          decider=self._decider))
        self.inference_worker = self.inference_workers[0]
        if self._is_distributed:
            torch.distributed.barrier()
        # every environment starts with its first observation on the table (environment_worker.py:148-160): the requests go into
        # the shared queue, from which the workers take them
        self._iw_queue.put_many(self.transport.start_experience_collection())
        torch.cuda.current_stream().synchronize()  # first observations are in HBM before any worker stream reads them
        self.report_worker.start_collection()
        self._iw_pool = InferenceWorkerPool(self.inference_workers, self._iw_sync, self._iw_queue, main_is_iw)
        if self._decider is not None and overlap:
            self._decider.start_rollout()
        self._iw_pool.start()
        self.timer = Timing()
        self._learning_time = 0.0

    def _private_policy(self, n_iw: int):
        """A policy object of the same class and configuration on its own engine (own activation workspace, sized for inference
        batches only), holding the learner's current parameters (inference_worker.py:90-101)."""
        hb = self.config.habitat_baselines
        cls = baseline_registry.get_policy(hb.rl.policy[self._agent.agent_name].name)
        with torch.random.fork_rng(devices=[]):  # the initialisers' draws (overwritten below) must not move the trainer's generator
            pol = cls.from_config(self.config, self._env_spec.observation_space, self._env_spec.action_space,
                                  orig_action_space=self._env_spec.orig_action_space, agent_name=self._agent.agent_name)
        kw = pol._engine_kwargs
        kw["max_frames"] = max(int(kw.get("max_envs", 1)), 2)  # act() only: no minibatch-sized workspace
        pol.aux_loss_modules.clear()
        pol.to(self.device)
        pol.eval()
        self._published.load_into(pol.engine)
        return pol

    def shutdown(self) -> None:
        """Stops the inference-worker threads (idempotent)."""
        if getattr(self, "_iw_pool", None) is not None:
            self._iw_pool.shutdown()
        super().shutdown()

    # ---- learner (ver_trainer.py:377-428) ---------------------------------------------------------------------------------------------
    def _update_agent(self):
        ppo_cfg = self._ppo_cfg
        with self.timer.avg_time("learn"):
            t0 = time.perf_counter()
            with self.timer.avg_time("compute returns"):
                self.learning_rollouts.compute_returns(ppo_cfg.use_gae, ppo_cfg.gamma, ppo_cfg.tau)
            t_returns = time.perf_counter() - t0
            if self._is_distributed:
                with self.timer.avg_time("synchronize"):
                    torch.distributed.barrier()
            t1 = time.perf_counter()
            with self.timer.avg_time("update agent"):
                self._agent.train()
                losses = self._agent.updater.update(self.learning_rollouts)
            with self.timer.avg_time("after update"):
                if self._published is not None:  # ver_trainer.py:402-410: the new weights become visible to the other workers
                    self._published.publish(self._agent.actor_critic.engine)
                if not self._overlap:
                    self.learning_rollouts.after_update()
                    # The version moves BEFORE the workers are released: a private-engine worker reloads the published weights only
                    # when it sees `cpu_current_policy_version` change, and the holder of the replay requests steps the moment it
                    # wakes up -- released first, it would act (values that bootstrap the returns, the actions that open the next
                    # rollout) on the previous parameters while stamping the steps with the new version.  The workers are parked
                    # here, so nothing races the increment (the reference's non-overlapped workers share the learner's live tensors).
                    self._agent.rollouts.increment_policy_version()
                    if self._decider is not None:
                        self._decider.start_rollout()  # armed before the first batch of the rollout is stepped (its step times count)
                    self._iw_pool.start_next(self.device)  # after the buffer reordering has drained: worker streams write slots next
                else:
                    self._agent.rollouts.increment_policy_version()
        self._learning_time = (time.perf_counter() - t1) + t_returns
        self._agent.after_update()
        if self._decider is not None:
            self._decider.learner_time(self._learning_time)
        return losses

    def collect_rollout(self) -> int:
        """One VER rollout: inference batches until the arena has its quota of steps."""
        ro = self._agent.rollouts
        if self._main_is_iw:
            self._agent.eval()
        if self._decider is not None and not self._overlap and not self._decider.started:
            self._decider.start_rollout()  # the very first rollout (later ones are armed in _update_agent, before the workers wake)
        with self.timer.avg_time("rollout"):
            self._iw_pool.collect(ro)
            ro.after_rollout()
            if self._overlap:
                with self.timer.avg_time("overlap_transfers"):
                    self.learning_rollouts.copy(ro)
        n = int(ro.num_steps_collected[0])
        if self._decider is not None:
            self._decider.end_rollout(int(ro.num_steps_to_collect))
        self.report_worker.num_steps_collected(n)
        if self._overlap:  # ver_trainer.py:524-530: the workers go on with the next rollout while the learner works on this one
            with self.timer.avg_time("overlap_transfers"):
                ro.after_update()
                self._iw_pool.start_next(self.device)
                if self._decider is not None:
                    self._decider.start_rollout()
        return n

    def run_update_cycle(self) -> Dict[str, float]:
        self._agent.pre_rollout()
        n = self.collect_rollout()
        self.local_steps_done = getattr(self, "local_steps_done", 0) + n
        losses = self._update_agent()
        self.report_worker.learner_timing(self.timer)
        self.report_worker.learner_update(losses)
        self.timer = Timing()
        self.num_steps_done = int(self.report_worker.num_steps_done)
        self.num_updates_done += 1
        return losses

    def train(self) -> None:
        self.num_steps_done = 0
        resume_state = load_resume_state(self.config)
        if resume_state is not None:
            if not self.config.habitat_baselines.load_resume_state_config:
                raise FileExistsError("habitat_baselines.load_resume_state_config=False but a previous training run exists in "
                                      f"{self.config.habitat_baselines.checkpoint_folder}")
            self.config = self._get_resume_state_config_or_new_config(resume_state["config"])
            rs = resume_state["requeue_stats"]
            self.num_steps_done, self.num_updates_done = rs["num_steps_done"], rs["num_updates_done"]
        self._init_train(resume_state)
        count_checkpoints = 0
        if resume_state is not None:
            self._last_checkpoint_percent = resume_state["requeue_stats"]["_last_checkpoint_percent"]
            count_checkpoints = resume_state["requeue_stats"]["count_checkpoints"]
        try:
            while not self.is_done():
                if rank0_only() and self._should_save_resume_state():
                    requeue_stats = dict(count_checkpoints=count_checkpoints, num_steps_done=self.num_steps_done,
                                         num_updates_done=self.num_updates_done, _last_checkpoint_percent=self._last_checkpoint_percent,
                                         report_worker_state=self.report_worker.state_dict())
                    save_resume_state({**self._agent.get_resume_state(), "config": self.config.to_dict(), "requeue_stats": requeue_stats},
                                      self.config)
                if EXIT.is_set():
                    self.envs.close()
                    requeue_job()
                    return
                self.run_update_cycle()
                if rank0_only() and self.should_checkpoint():
                    self.save_checkpoint(f"ckpt.{count_checkpoints}.pth",
                                         dict(step=self.num_steps_done, wall_time=self.report_worker.time_taken))
                    count_checkpoints += 1
            self.window_episode_stats = self.report_worker.get_window_episode_stats()
        finally:
            self.shutdown()
            self.envs.close()
            self._writer_cm.__exit__(None, None, None)
            if self._is_distributed:
                torch.distributed.barrier()
