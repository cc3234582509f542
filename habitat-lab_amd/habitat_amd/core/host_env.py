"""A CPU stand-in for one simulator-backed environment (the `RLEnv` a VectorEnv worker owns: habitat/core/env.py:337-430):
numpy-generated RGB-D + pointgoal observations of the benchmark's sizes, Bernoulli episode ends, a step budget.  It exists so
that the process-per-env transport (core/vector_env.py) and the trainer's host path can be exercised and timed end to end
without habitat-sim; it makes no attempt to be a navigation task.  `task="rearrange"` emits the observation set of a rearrangement
skill instead (two named depth cameras and raw 1-D robot-state sensors, no goal sensor with an embedding; discrete actions).
`task="cubemap"` emits the six cube-face cameras of a 360-degree agent (`rgb_back` ... `rgb_up`, `depth_back` ... `depth_up`, the
face order of CubeMap2Equirect / CubeMap2Fisheye) plus the pointgoal sensor."""
from __future__ import annotations

import numpy as np

from habitat_amd.common import spaces

GOAL_UUID = "pointgoal_with_gps_compass"
CUBE_FACES = ("back", "down", "front", "left", "right", "up")  # the sensor order of the cube-map obs transformers


class Episode:
    """The two fields of habitat.core.dataset.Episode the trainer / evaluator read (habitat_evaluator.py:223-262)."""

    def __init__(self, episode_id: str, scene_id: str):
        self.episode_id, self.scene_id = episode_id, scene_id

    def __eq__(self, other):
        return isinstance(other, Episode) and (self.episode_id, self.scene_id) == (other.episode_id, other.scene_id)

    def __repr__(self):
        return f"Episode({self.scene_id}, {self.episode_id})"


class HostSyntheticNavEnv:
    def __init__(self, seed: int = 0, height: int = 256, width: int = 256, use_rgb: bool = True, use_depth: bool = True,
                 num_actions: int = 4, max_episode_steps: int = 500, p_done: float = 1.0 / 25.0, work_us: int = 0,
                 num_episodes: int = 0, task: str = "pointnav"):
        assert task in ("pointnav", "rearrange", "cubemap"), task
        self._task = task
        self._rng = np.random.default_rng(seed)
        self._seed = seed
        self._h, self._w, self._use_rgb, self._use_depth = height, width, use_rgb, use_depth
        self._max_steps, self._p_done, self._work_us = max_episode_steps, p_done, work_us
        sp = {}
        fmin, fmax = np.finfo(np.float32).min, np.finfo(np.float32).max
        if task == "rearrange":  # the sensors of the reference's rearrangement skills (head / arm cameras, joint state, holding flag, goal)
            sp["head_depth"] = spaces.Box(0.0, 1.0, (height, width, 1), np.float32)
            sp["arm_depth"] = spaces.Box(0.0, 1.0, (height, width, 1), np.float32)
            sp["joint"] = spaces.Box(fmin, fmax, (7,), np.float32)
            sp["is_holding"] = spaces.Box(0.0, 1.0, (1,), np.float32)
            sp["goal_to_agent_gps_compass"] = spaces.Box(fmin, fmax, (2,), np.float32)
        elif task == "cubemap":
            for face in CUBE_FACES:
                sp[f"rgb_{face}"] = spaces.Box(0, 255, (height, width, 3), np.uint8)
            for face in CUBE_FACES:
                sp[f"depth_{face}"] = spaces.Box(0.0, 1.0, (height, width, 1), np.float32)
            sp[GOAL_UUID] = spaces.Box(fmin, fmax, (2,), np.float32)
        else:
            if use_rgb:
                sp["rgb"] = spaces.Box(0, 255, (height, width, 3), np.uint8)
            if use_depth:
                sp["depth"] = spaces.Box(0.0, 1.0, (height, width, 1), np.float32)
            sp[GOAL_UUID] = spaces.Box(fmin, fmax, (2,), np.float32)
        self.observation_space = spaces.Dict(sp)
        self.action_space = spaces.Discrete(num_actions)
        self.original_action_space = self.action_space
        self._num_episodes = num_episodes  # > 0: a finite episode list that is cycled, like a dataset split
        self.number_of_episodes = num_episodes if num_episodes > 0 else 1 << 30
        self.episodes = ()
        self._t = 0
        self._episode = 0
        self.episode_over = False
        self._ret = 0.0

    @property
    def current_episode(self):
        eid = self._episode % self._num_episodes if self._num_episodes > 0 else self._episode
        return Episode(episode_id=str(eid), scene_id=f"synthetic-{self._seed}")

    def _obs(self):
        o = {}
        if self._task == "rearrange":
            o["head_depth"] = self._rng.random((self._h, self._w, 1), dtype=np.float32)
            o["arm_depth"] = self._rng.random((self._h, self._w, 1), dtype=np.float32)
            o["joint"] = self._rng.uniform(-np.pi, np.pi, 7).astype(np.float32)
            o["is_holding"] = np.array([float(self._rng.random() < 0.5)], dtype=np.float32)
            o["goal_to_agent_gps_compass"] = np.array([self._rng.uniform(0.0, 10.0), self._rng.uniform(-np.pi, np.pi)], dtype=np.float32)
            return o
        if self._task == "cubemap":
            for face in CUBE_FACES:
                o[f"rgb_{face}"] = self._rng.integers(0, 256, (self._h, self._w, 3), dtype=np.uint8)
            for face in CUBE_FACES:
                o[f"depth_{face}"] = self._rng.random((self._h, self._w, 1), dtype=np.float32)
            o[GOAL_UUID] = np.array([self._rng.uniform(0.0, 10.0), self._rng.uniform(-np.pi, np.pi)], dtype=np.float32)
            return o
        if self._use_rgb:
            o["rgb"] = self._rng.integers(0, 256, (self._h, self._w, 3), dtype=np.uint8)
        if self._use_depth:
            o["depth"] = self._rng.random((self._h, self._w, 1), dtype=np.float32)
        o[GOAL_UUID] = np.array([self._rng.uniform(0.0, 10.0), self._rng.uniform(-np.pi, np.pi)], dtype=np.float32)
        return o

    def reset(self):
        self._t, self._ret, self.episode_over = 0, 0.0, False
        self._episode += 1
        return self._obs()

    def step(self, action):
        if isinstance(action, dict):
            action = action.get("action", 0)
        assert 0 <= int(action) < self.action_space.n, f"invalid action {action}"
        if self._work_us:  # stand-in for simulator time
            import time
            time.sleep(self._work_us * 1e-6)
        self._t += 1
        reward = float(self._rng.standard_normal())
        self._ret += reward
        done = bool(self._rng.random() < self._p_done) or self._t >= self._max_steps
        self.episode_over = done
        info = {"episode_return": self._ret, "num_steps": float(self._t)}  # measures are present at every step, like habitat's
        return self._obs(), reward, done, info

    def get_metrics(self):
        return {"episode_return": self._ret, "num_steps": float(self._t)}

    def close(self):
        pass


def make_host_env(seed, height, width, use_rgb, use_depth, num_actions, max_episode_steps, work_us=0, num_episodes=0, task="pointnav"):
    return HostSyntheticNavEnv(seed=seed, height=height, width=width, use_rgb=use_rgb, use_depth=use_depth, num_actions=num_actions,
                               max_episode_steps=max_episode_steps, work_us=work_us, num_episodes=num_episodes, task=task)


def make_rearrange_host_env(seed, height, width, use_rgb, use_depth, num_actions, max_episode_steps, work_us=0, num_episodes=0):
    """`vector_env_factory.make_env_fn` form of `task="rearrange"` (the sensor sizes come from the configured simulator sensors)."""
    return make_host_env(seed, height, width, use_rgb, use_depth, num_actions, max_episode_steps, work_us, num_episodes, task="rearrange")


def make_cubemap_host_env(seed, height, width, use_rgb, use_depth, num_actions, max_episode_steps, work_us=0, num_episodes=0):
    """`vector_env_factory.make_env_fn` form of `task="cubemap"` (the face size comes from the configured simulator sensors)."""
    return make_host_env(seed, height, width, use_rgb, use_depth, num_actions, max_episode_steps, work_us, num_episodes, task="cubemap")
