"""Environment source boundary.

`VectorEnvFactory.construct_envs(...) -> VectorEnv` is the reference's hook
(habitat_baselines/common/env_factory.py:14-38, selected through
``habitat_baselines.vector_env_factory._target_``).  The benchmark of this path uses synthetic
observations (BASELINE.json), so this module provides `SyntheticVectorEnvFactory` / `SyntheticVectorEnv`:
a VectorEnv-API object (habitat/core/vector_env.py:229-232,380-410,451-484: num_envs,
observation_spaces, action_spaces, orig_action_spaces, reset, async_step_at, wait_step_at, post_step,
close) whose observations are produced ON THE DEVICE by `hab_synth_step` -- bit-identical to
oracle/synth.py -- and which additionally offers `step_into(...)`, writing the next observations,
rewards and masks straight into rollout-arena rows with no host round trip.  Any other object with the
VectorEnv API (e.g. habitat's own process-per-env VectorEnv) can be returned by a user factory; the
trainer then uses the generic host path."""
from __future__ import annotations

import abc
import importlib
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from habitat_amd import _lib
from habitat_amd._lib import check, ptr, stream_ptr
from habitat_amd.common import spaces

GOAL_UUID = "pointgoal_with_gps_compass"
NUM_SEMANTIC_IDS, NUM_OBJECT_CATEGORIES = 40, 21  # synthetic ObjectNav sensor ranges


class VectorEnvFactory(abc.ABC):
    @abc.abstractmethod
    def construct_envs(self, config, workers_ignore_signals: bool = False, enforce_scenes_greater_eq_environments: bool = False,
                       is_first_rank: bool = True):
        ...


def instantiate(target_cfg):
    """hydra.utils.instantiate for a `{_target_: 'pkg.mod.Class', **kwargs}` node."""
    target = target_cfg["_target_"]
    mod, _, name = target.rpartition(".")
    cls = getattr(importlib.import_module(mod), name)
    return cls(**{k: v for k, v in target_cfg.items() if k != "_target_"})


class SyntheticVectorEnv:
    def __init__(self, num_envs: int, height: int, width: int, seed: int = 100, env_offset: int = 0, use_rgb: bool = True,
                 use_depth: bool = True, num_actions: int = 4, device="cuda", task: str = "pointnav"):
        self.num_envs, self.H, self.W = num_envs, height, width
        self.seed, self.env_offset = int(seed) & 0xFFFFFFFF, int(env_offset)
        self.use_rgb, self.use_depth, self.task = use_rgb, use_depth, task
        self.device = torch.device(device)
        d = {}
        rgb_key, depth_key = ("head_rgb", "head_depth") if task in ("rearrange", "social") else ("rgb", "depth")
        if use_rgb:
            d[rgb_key] = spaces.Box(0, 255, (height, width, 3), np.uint8)
        if use_depth:
            d[depth_key] = spaces.Box(0.0, 1.0, (height, width, 1), np.float32)
        fmin, fmax = np.finfo(np.float32).min, np.finfo(np.float32).max
        if task == "rearrange":  # sensor set of Nav2DRearr-v0: the head camera and three raw 1-D sensors, no goal sensor
            d["obj_start_sensor"] = spaces.Box(fmin, fmax, (2,), np.float32)
            d["obj_goal_sensor"] = spaces.Box(fmin, fmax, (2,), np.float32)
            d["is_holding"] = spaces.Box(0.0, 1.0, (1,), np.float32)
        elif task == "social":  # sensor set of Nav2DSocial-v0: the head camera and two raw 1-D sensors, no goal sensor
            d["person_sensor"] = spaces.Box(fmin, fmax, (2,), np.float32)
            d["person_visible"] = spaces.Box(0.0, 1.0, (1,), np.float32)
        elif task == "explore":  # sensor set of Nav2DExplore-v0: the camera, then gps and compass; no goal input at all
            d["gps"] = spaces.Box(fmin, fmax, (2,), np.float32)
            d["compass"] = spaces.Box(-np.pi, np.pi, (1,), np.float32)
        elif task == "imagenav":  # sensor set of Nav2DImageNav-v0: the camera, the goal as a second image, then gps and compass
            d["goal_rgb"] = spaces.Box(0, 255, (height, width, 3), np.uint8)
            d["gps"] = spaces.Box(fmin, fmax, (2,), np.float32)
            d["compass"] = spaces.Box(-np.pi, np.pi, (1,), np.float32)
        elif task == "objectnav":  # sensor set of the ObjectNav experiments (rgb, depth, semantic + objectgoal, compass, gps)
            d["semantic"] = spaces.Box(0, NUM_SEMANTIC_IDS - 1, (height, width, 1), np.int32)
            d["objectgoal"] = spaces.Box(0, NUM_OBJECT_CATEGORIES - 1, (1,), np.int64)
            d["compass"] = spaces.Box(-np.pi, np.pi, (1,), np.float32)
            d["gps"] = spaces.Box(fmin, fmax, (2,), np.float32)
        else:
            d[GOAL_UUID] = spaces.Box(fmin, fmax, (2,), np.float32)
        self.observation_spaces = [spaces.Dict(d) for _ in range(num_envs)]
        self.action_spaces = [spaces.Discrete(num_actions) for _ in range(num_envs)]
        self.orig_action_spaces = self.action_spaces
        self.number_of_episodes = [None] * num_envs
        if self.device.type != "cuda":
            raise _lib.HabError("SyntheticVectorEnv generates observations on the GPU; no GPU device given")
        dev = self.device
        self._t = torch.zeros(num_envs, dtype=torch.int64, device=dev)
        self._since = torch.zeros(num_envs, dtype=torch.int64, device=dev)
        self._rgb = torch.zeros(num_envs, height, width, 3, dtype=torch.uint8, device=dev) if use_rgb else None
        self._depth = torch.zeros(num_envs, height, width, 1, device=dev) if use_depth else None
        self._goal = torch.zeros(num_envs, 2, device=dev) if task not in ("objectnav", "rearrange", "social", "explore", "imagenav") else None
        self._obj = {}
        if task == "objectnav":
            self._obj = dict(semantic=torch.zeros(num_envs, height, width, 1, dtype=torch.int32, device=dev),
                             objectgoal=torch.zeros(num_envs, 1, dtype=torch.int64, device=dev),
                             compass=torch.zeros(num_envs, 1, device=dev), gps=torch.zeros(num_envs, 2, device=dev))
        elif task == "rearrange":
            self._obj = dict(obj_start_sensor=torch.zeros(num_envs, 2, device=dev), obj_goal_sensor=torch.zeros(num_envs, 2, device=dev),
                             is_holding=torch.zeros(num_envs, 1, device=dev))
        elif task == "explore":
            self._obj = dict(gps=torch.zeros(num_envs, 2, device=dev), compass=torch.zeros(num_envs, 1, device=dev))
        elif task == "imagenav":
            self._obj = dict(goal_rgb=torch.zeros(num_envs, height, width, 3, dtype=torch.uint8, device=dev),
                             gps=torch.zeros(num_envs, 2, device=dev), compass=torch.zeros(num_envs, 1, device=dev))
        elif task == "social":
            self._obj = dict(person_sensor=torch.zeros(num_envs, 2, device=dev), person_visible=torch.zeros(num_envs, 1, device=dev))
        self._rew = torch.zeros(num_envs, device=dev)
        self._nd = torch.zeros(num_envs, dtype=torch.uint8, device=dev)
        self._pending: set = set()      # envs with an outstanding async_step_at (host path)
        self._host_cache = None
        self._tmp = None

    # ---- device fast path ---------------------------------------------------------------------
    def _emit(self, rgb, depth, goal, reward, not_done, advance: int):
        check(_lib.lib().hab_synth_step(ptr(rgb), ptr(depth), ptr(goal), ptr(reward), ptr(not_done), ptr(self._t), ptr(self._since),
                                        self.seed, self.env_offset, self.num_envs, self.H, self.W, advance, stream_ptr()),
              "hab_synth_step")

    def _emit_objectnav(self, obs):
        if self.task != "objectnav":
            return
        check(_lib.lib().hab_synth_objectnav_sensors(ptr(obs.get("semantic")), ptr(obs.get("objectgoal")), ptr(obs.get("compass")),
                                                     ptr(obs.get("gps")), ptr(self._t), self.seed, self.env_offset, self.num_envs,
                                                     self.H, self.W, stream_ptr()), "hab_synth_objectnav_sensors")

    def reset_into(self, rgb, depth, goal):
        """Resets all envs and writes their first observations into the given (N, ...) device tensors."""
        self._t.zero_()
        self._since.zero_()
        self._emit(rgb, depth, goal, None, None, 0)

    def step_into(self, rgb, depth, goal, reward, not_done):
        """Advances all envs one step (actions do not influence synthetic observations) and writes the new
        observations / rewards (N,) / not-done masks (N,) bytes straight into the given device tensors."""
        self._emit(rgb, depth, goal, reward, not_done, 1)

    def reset_into_obs(self, obs):
        """Dict form: `obs` maps sensor uuid -> (N, ...) device tensor (a rollout-arena row)."""
        self.reset_into(obs.get("rgb"), obs.get("depth"), obs.get(GOAL_UUID))
        self._emit_objectnav(obs)

    def step_into_obs(self, obs, reward, not_done):
        self.step_into(obs.get("rgb"), obs.get("depth"), obs.get(GOAL_UUID), reward, not_done)
        self._emit_objectnav(obs)

    # ---- VectorEnv API (host path) ----------------------------------------------------------------
    def _host_obs(self) -> List[Dict[str, np.ndarray]]:
        rgb = self._rgb.cpu().numpy() if self.use_rgb else None
        depth = self._depth.cpu().numpy() if self.use_depth else None
        goal = self._goal.cpu().numpy() if self._goal is not None else None
        extra = {k: v.cpu().numpy() for k, v in self._obj.items()}
        out = []
        for i in range(self.num_envs):
            o = {}
            if self.use_rgb:
                o["rgb"] = rgb[i]
            if self.use_depth:
                o["depth"] = depth[i]
            for k, v in extra.items():
                o[k] = v[i]
            if goal is not None:
                o[GOAL_UUID] = goal[i]
            out.append(o)
        return out

    def _own_obs(self):
        o = dict(self._obj)
        if self.use_rgb:
            o["rgb"] = self._rgb
        if self.use_depth:
            o["depth"] = self._depth
        if self._goal is not None:
            o[GOAL_UUID] = self._goal
        return o

    def reset(self):
        self.reset_into_obs(self._own_obs())
        return self._host_obs()

    def async_step_at(self, index_env: int, action) -> None:
        if index_env in self._pending:
            raise _lib.HabError(f"env {index_env}: async_step_at called twice without wait_step_at")
        self._pending.add(int(index_env))

    def advance_on_device(self) -> List[int]:
        """Advances exactly the envs whose step was requested, entirely on the device (no host copy of any observation): their new
        observations / rewards / not-done bytes are in the env's own tensors afterwards.  All envs (the usual case): one generator
        launch into the env's own tensors.  A subset (VER batches, the double-buffered sampler's halves, ppo_trainer.py:743-768): the
        generator runs on scratch copies of the per-env clocks / tensors and only the requested rows are taken over.  Returns the ids."""
        ids = sorted(self._pending)
        self._pending.clear()
        if len(ids) == self.num_envs:
            self.step_into_obs(self._own_obs(), self._rew, self._nd)
        elif ids:
            own = self._own_obs()
            if self._tmp is None:
                self._tmp = ({k: torch.empty_like(v) for k, v in own.items()}, torch.empty_like(self._rew), torch.empty_like(self._nd))
            tobs, trew, tnd = self._tmp
            t0, s0 = self._t.clone(), self._since.clone()
            self.step_into_obs(tobs, trew, tnd)
            sel = torch.tensor(ids, device=self.device)
            keep = torch.ones(self.num_envs, dtype=torch.bool, device=self.device)
            keep[sel] = False
            self._t[keep], self._since[keep] = t0[keep], s0[keep]
            for k, v in own.items():
                v[sel] = tobs[k][sel]
            self._rew[sel], self._nd[sel] = trew[sel], tnd[sel]
        return ids

    def step_results_host(self):
        """(rewards (N,), not-done (N,)) of the last steps as host arrays: the two small per-env vectors the host-side episode
        accounting needs (one device->host copy each; observations stay in HBM)."""
        return self._rew.cpu().numpy(), self._nd.cpu().numpy()

    def _advance_pending(self):
        """Host path (VectorEnv.wait_step_at): device advance + the host copies of the observations the caller asked for."""
        ids = self.advance_on_device()
        obs = self._host_obs()
        rew, nd = self.step_results_host()
        if self._host_cache is None or len(ids) == self.num_envs:
            self._host_cache = (obs, rew.copy(), nd.copy())
        else:
            c_obs, c_rew, c_nd = self._host_cache
            for i in ids:
                c_obs[i], c_rew[i], c_nd[i] = obs[i], rew[i], nd[i]

    def wait_step_at(self, index_env: int):
        if index_env in self._pending:  # every env requested so far advances on the first wait
            self._advance_pending()
        obs, rew, nd = self._host_cache
        return obs[index_env], float(rew[index_env]), not bool(nd[index_env]), {}

    def post_step(self, observations):
        return observations

    def close(self):
        pass


NAV2D_MEASURES = ("success", "spl", "distance_to_goal", "collisions")
NAV2D_MAX_OBSTACLES = 8
# 4-byte words of a state record (include/habitat_amd.h: HAB_NAV2D_W_EPISODE, _ENDED, _LAST_MEASURES), the ones this module
# reads; csrc/nav2d.hip asserts the record's member offsets against the header's
_W_EPISODE, _W_ENDED, _W_LAST = 10, 11, 12


NAV2D_DISTANCES = ("euclidean", "geodesic")

# the top-down map (include/habitat_amd.h: HAB_NAV2D_MAP_*): the resolution's range, which words of a task's record tell its targets,
# the cell codes and the colour of every code, rows (r, g, b) of HAB_NAV2D_MAP_COLORS
NAV2D_MAP_MIN_RESOLUTION, NAV2D_MAP_MAX_RESOLUTION = 16, 512
NAV2D_MAP_TASK_GOAL, NAV2D_MAP_TASK_OBJ, NAV2D_MAP_TASK_REARR, NAV2D_MAP_TASK_SOCIAL, NAV2D_MAP_TASK_EXPLORE = 0, 1, 2, 3, 4
NAV2D_MAP_CODES = dict(occupied=0, free=1, start=4, target=6, trajectory=10, object=16, carried=20, person=21, agent=22, tick=23)
NAV2D_MAP_COLORS = np.full((32, 3), (255, 0, 255), dtype=np.uint8)
for _code, _rgb in (("occupied", (64, 64, 64)), ("free", (200, 200, 200)), ("start", (50, 50, 200)), ("target", (255, 32, 32)),
                    ("trajectory", (0, 160, 208)), ("object", (240, 160, 32)), ("carried", (255, 200, 0)), ("person", (200, 0, 200)),
                    ("agent", (0, 160, 0)), ("tick", (0, 64, 0))):
    NAV2D_MAP_COLORS[NAV2D_MAP_CODES[_code]] = _rgb
NAV2D_MAP_DEFAULTS = dict(map_resolution=128, visibility_dist=5.0, draw_fog=True, fov=90)


def nav2d_map_parameters(top_down_map, who: str = "Nav2D"):
    """Checks the `top_down_map` keyword of a Nav2D env, a mapping with any of map_resolution, visibility_dist, draw_fog and fov (other
    keys of habitat's measurement are accepted and not read), and returns (map_resolution, visibility_dist, draw_fog), or None where
    the keyword is None."""
    if top_down_map is None:
        return None
    if not isinstance(top_down_map, dict):
        raise _lib.HabError(f"{who}: top_down_map {top_down_map!r} must be None or a mapping of the measurement's keys")
    S, vis, draw, fov = (top_down_map.get(k, v) for k, v in NAV2D_MAP_DEFAULTS.items())
    if not whole(S) or not NAV2D_MAP_MIN_RESOLUTION <= S <= NAV2D_MAP_MAX_RESOLUTION:
        raise _lib.HabError(f"{who}: top_down_map.map_resolution {S!r} must be a whole number in {NAV2D_MAP_MIN_RESOLUTION}.."
                            f"{NAV2D_MAP_MAX_RESOLUTION}")
    if (isinstance(vis, bool) or not isinstance(vis, (int, float, np.integer, np.floating)) or not np.isfinite(np.float32(vis))
            or not float(np.float32(vis)) > 0.0):
        raise _lib.HabError(f"{who}: top_down_map.visibility_dist {vis!r} must be a positive finite length in metres")
    if isinstance(fov, bool) or not isinstance(fov, (int, float, np.integer, np.floating)) or float(fov) != 90.0:
        raise _lib.HabError(f"{who}: top_down_map.fov {fov!r} must be 90: the wedge of the fog of war is the camera's field of view")
    if not isinstance(draw, (bool, np.bool_)):
        raise _lib.HabError(f"{who}: top_down_map.draw_fog {draw!r} must be true or false")
    return int(S), float(np.float32(vis)), bool(draw)


def nav2d_distance(distance, who: str = "Nav2D") -> str:
    if not isinstance(distance, str) or distance not in NAV2D_DISTANCES:
        raise _lib.HabError(f"{who}: distance {distance!r} must be one of {', '.join(map(repr, NAV2D_DISTANCES))}")
    return distance


def whole(v) -> bool:
    """Whether v is a whole number (a bool is none)."""
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def nav2d_num_headings(turn_angle) -> int:
    if not whole(turn_angle) or turn_angle <= 0 or 360 % int(turn_angle) != 0:
        raise _lib.HabError(f"Nav2D: turn_angle {turn_angle!r} must be a positive whole number of degrees that divides 360")
    return 360 // int(turn_angle)


def nav2d_tables(turn_angle: int, height: int, width: int):
    """The host tables of the Nav2D kernels, computed in float64 and rounded once: dirs (nh, 2) = (cos, sin) of heading h; and, for
    a rendered env, ray (nh, W, 2) = world direction of column u's ray at heading h (column 0 leftmost, 90 degree horizontal field of
    view), col_cos (W,) = cosine between that ray and the optical axis, tanv (H,) = tangent of row v's elevation (row 0 on top, square
    pixels).  No angle is evaluated on the device."""
    nh = nav2d_num_headings(turn_angle)
    a = np.arange(nh, dtype=np.float64) * (2.0 * np.pi / nh)
    dirs = np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32)
    if height <= 0 or width <= 0:
        return dirs, None, None, None
    au = np.arctan(1.0 - 2.0 * (np.arange(width, dtype=np.float64) + 0.5) / width)
    th = a[:, None] + au[None, :]
    ray = np.stack([np.cos(th), np.sin(th)], 2).astype(np.float32)
    tanv = ((1.0 - 2.0 * (np.arange(height, dtype=np.float64) + 0.5) / height) * (height / width)).astype(np.float32)
    return dirs, ray, np.cos(au).astype(np.float32), tanv


class Nav2DVectorEnv(SyntheticVectorEnv):
    """Nav2D-v0: a small 2-D point-goal world whose reward depends on the actions, simulated and rendered on the device
    (csrc/nav2d.hip) and written straight into rollout rows.  It is a measurement source like the hashed tasks, not a simulator port.
    tests/nav2d_reference.py restates all of the following in numpy; the kernels match it bit for bit, phi excepted.

    World.  One per (env, episode), a function of (seed, env_offset + env, episode index) through mix32 / stream_key / u01 with the
    stream ids 16 (obstacles), 17 (start), 18 (goal), 19 (heading), 20 (obstacle colours); word i of a stream is
    mix32(stream_key(seed, id, env, episode) ^ i) and u_i its u01.
      * Arena: the square [0, 8] x [0, 8] m.  K = num_obstacles in 0..8 axis-aligned rectangles; rectangle k has the centre
        (2 + 4 u_4k, 2 + 4 u_4k+1) and the half extents (0.25 + 0.75 u_4k+2, 0.25 + 0.75 u_4k+3), so the outer ring of width 1 m
        is always free.
      * The agent is a disc of radius 0.1 m.  A position is free when it lies in [0.1, 7.9]^2 and not strictly inside any rectangle
        grown by 0.1 on every side (a box test: corners are not rounded).
      * Start: the first free candidate (0.1 + 7.8 u_2j, 0.1 + 7.8 u_2j+1), j = 0..15, of the start stream, else (0.5, 0.5).
        Goal: the first candidate of the goal stream that is free and at least 1 m from the start, else (7.5, 7.5).
      * Heading: an index h in [0, 360 / turn_angle), initially word 0 of the heading stream modulo that count; turn_angle is a
        whole number of degrees dividing 360 (default 10).  The direction of h is row h of a (cos, sin) table of h * turn_angle
        computed in float64 on the host and rounded to float32.
    Actions.  Discrete(4) in habitat's order: 0 STOP, 1 MOVE_FORWARD, 2 TURN_LEFT (h + 1), 3 TURN_RIGHT (h - 1).  Forward:
      p' = p + 0.25 * dir (a float32 multiply, then a separate float32 add), taken if p' is free; otherwise the agent stays and a
      collision is counted.  The episode ends on STOP or when its step count reaches habitat.environment.max_episode_steps.
    Reward and measures (habitat's PointNav defaults).  d = float32 Euclidean distance to the goal, sqrt(dx * dx + dy * dy);
      success = STOP and d < 0.2; reward = (-0.01 + (d_prev - d_new)) + 2.5 * success; path_length grows by 0.25 per accepted
      forward.  At the episode's end spl = success * d_start / max(d_start, path_length) -- in the default distance mode the
      STRAIGHT-LINE SPL: d_start is the Euclidean distance, so with obstacles it overstates habitat's; see Distance below --
      distance_to_goal = d and collisions = the count.  On done the next episode's world is generated, its first observation is what the step returns and not_done = 0.
    Sensors.
      * pointgoal_with_gps_compass = (rho, phi): rho = d; phi = atan2f(cross, dot) of the goal offset in the agent frame, left
        positive: dot = dx * c + dy * s, cross = c * dy - s * dx.  phi is the one quantity that is not bitwise (atan2f is not
        correctly rounded).
      * depth (H, W, 1) float32 in [0, 1]: pinhole camera, 90 degree horizontal field of view, square pixels, 1.25 m above the floor
        under a 2.5 m ceiling.  Per column a ray-vs-slab intersection against the four walls and the K rectangles gives the hit
        distance t; z_wall = t * cos(column angle).  depth = min(z_wall(u), 1.25 / |tan_v|) / 10, clipped to 1.
      * rgb (H, W, 3) uint8: floor and ceiling constants, a colour per wall, obstacle k's colour from word k of the colour stream; a
        red goal marker, a cylinder of radius 0.2 m around the goal from floor to ceiling, drawn in rgb ONLY (depth stays what the
        agent collides with); each colour is scaled by 1 - z / 10 and truncated.
      * Without rgb and depth nothing is rendered and the observation space is the goal sensor alone.

    Distance (`distance`, from `habitat.synthetic.distance_to_goal`).  "euclidean", the default, is all of the above.  "geodesic"
      changes the d of the reward, the success test, distance_to_goal and the SPL numerator -- nothing else: the world, the goal
      sensor and the render stay -- to the shortest path round the obstacles, as habitat defines these measures.
      tests/nav2d_geo_reference.py restates it in numpy; `nav2d_geo_build_kernel` and the geodesic forms of the step kernels match it
      bit for bit.  Every operation is one float32 rounding in the written order.
      * Boxes.  Obstacle k has the inflated box X0 = x0 - 0.1, Y0 = y0 - 0.1, X1 = x1 + 0.1, Y1 = y1 + 0.1 (the expressions of the
        free test) and the visibility box, that box shrunk by E = 2^-10 m: lx = X0 + E, ly = Y0 + E, hx = X1 - E, hy = Y1 - E.
      * visible(a, b) unless the segment meets the open visibility box of some obstacle, by the separating-axis test
        cx = (lx + hx) * 0.5, ex = (hx - lx) * 0.5, mx = (ax + bx) * 0.5 - cx, sx = (bx - ax) * 0.5, the same for y; blocked iff
        |mx| < ex + |sx| and |my| < ey + |sy| and |sx * my - sy * mx| < ex * |sy| + ey * |sx|.  A shortest path touches inflated
        boxes only at corners and along sides, so it clears every shrunk box by E, about a thousand times the test's rounding
        error: no valid edge is lost, and the result lies between the exact geodesic of the world shrunk by E and the world's own.
        The arena walls never block: free space is inside the convex [0.1, 7.9]^2 and no inflated box reaches a wall.
      * Nodes.  Node 4k + j is corner j of inflated box k in the order (X0, Y0), (X1, Y0), (X0, Y1), (X1, Y1), valid iff free.
      * Field.  D[i] = +inf for invalid nodes; else the least over node paths i -> ... -> goal of the sum rounded from the goal
        outwards, fl(w(i, j) + D[j]) with w = the Euclidean d where visible; the last hop is d(node, goal) where visible.  It is
        the fixed point of Jacobi sweeps D <- min(D, min_j fl(w[i][j] + D[j])), run until one changes nothing, at most 4K.
      * geo(p) = the least of d(p, goal) if visible and fl(d(p, c_i) + D[i]) over the nodes with finite D[i] that p sees; +inf
        if there is none.
      * When an episode begins the field is built and g0 = geo(start).  g0 finite: d_start = d_prev = g0 and every step's d is
        geo(p); where that is +inf (the agent hopped across a sliver into an enclosed pocket) d = d_prev and the episode's
        lost-step counter goes up.  g0 infinite (the goal is walled off): the episode keeps the Euclidean d throughout.
      The field records (`_geo`, (N, 40) int32: D, reachable, sweeps, lost steps) exist in this mode only.

    Top-down map (`top_down_map`, from `habitat.task.measurements.top_down_map`; every Nav2D task has it).  None, the default:
      nothing is allocated and nothing is launched.  dict(map_resolution=128, visibility_dist=5.0, draw_fog=True): the env owns
      `_map`, `_fog` (uint8 (N, S, S)) and `_map_rec` ((N, 8) int32) and `hab_nav2d_map_update` runs after every step entry on its
      stream with its mask and advance (csrc/nav2d_map.hip; tests/nav2d_map_reference.py restates it, the kernels match it byte for
      byte).  `top_down_map()` returns habitat's four fields, `render_frames()` the video frames; neither goes into the infos.
      Every float operation is one float32 rounding in the written order; only the cell size divides.
      * Grid.  S = map_resolution, a whole number in 16..512; cell = 8 / S; cell (r, c) has the centre x = (c + 0.5) * cell,
        y = (S - 1 - r + 0.5) * cell: row 0 is the top, y is up.  "In a disc of radius R at q" is dx * dx + dy * dy <= R * R.
      * Static layer, written when an episode begins: 0 where the centre is strictly inside a raw rectangle, else 1; then 16 in a
        disc of 0.3 m at every object of Nav2DObj-v0 that is not of the target category; then 6 over that: a disc of 0.2 m at
        (GX, GY) (Nav2D-v0, Nav2DVel-v0) or at the goal place (the rearrangement tasks), discs of 0.3 m at the objects of the
        target category (Nav2DObj-v0), nothing for Nav2DSocial-v0 and Nav2DExplore-v0; then 4 over all in a disc of 0.15 m at the start.  The
        rearrangement object and the person move, so they are in the frame, not in the map.
      * Trajectory, code 10, over every code but 4 and 6.  A cell is on the segment a -> b when its centre is within
        w = 0.75 * cell of it: e = centre - a, s = b - a, len2 = s.s; hit iff e.e <= w * w, or the same at b, or len2 > 0 and
        0 <= e.s <= len2 and cross * cross <= (w * w) * len2 with cross = sx * ey - sy * ex.  When an episode begins the start is
        drawn as a segment of no length, so the agent's own cell is never shown occupied; on a step that did not end the episode
        the segment from the record's previous position to the new one is drawn, then previous = new.
      * Fog of war.  `_fog` is 1 where the cell has been seen in the episode.  A cell is seen at a step when its centre is not
        strictly inside a rectangle, dx * dx + dy * dy <= vis * vis for (dx, dy) = centre - p, it lies in the camera's 90 degree
        wedge (dot = dx * c + dy * s > 0 and |c * dy - s * dx| <= dot for the heading's (c, s)) or within 0.25 m, and the segment
        p -> centre meets no open raw rectangle by the separating-axis expression of `visible` above on (x0, y0, x1, y1) itself,
        neither grown nor shrunk.  Cylinders (objects, the person) do not block sight in the map, and occupied cells are never
        marked: both are part of the definition.
      * Episode boundaries.  At a reset, and for a stepped env whose step ended an episode, both layers are cleared, the new
        episode's static layer is written with the record's current position as the start, and the first reveal is done from it.
        So the finished episode's last move is never drawn: a STOP does not move, an end at the step limit loses one segment.
        An env whose mask byte is clear keeps map, fog and record.
      * Frame (`render_frames`, one launch of `nav2d_map_frame_kernel` for all envs), uint8 (N, Hf, Wf, 3), panels left to right:
        the rgb image if the env has one, upscaled by nearest neighbour (source row (r * H) / Hf, panel width Wp = (Hf * W) / H,
        source column (c * W) / Wp); depth likewise as grey (int)(d * 255); the map at Hf x Hf, pixel (r, c) showing cell
        ((r * S) / Hf, (c * S) / Hf) in the colour NAV2D_MAP_COLORS gives its code.  Overlays at cell granularity, later ones on
        top: the rearrangement object, resting or carried (0.3 m, code 20), the person (0.3 m, 21), the agent (0.2 m, 22), the
        heading tick (cells within 0.08 m of p -> p + 0.45 * dir, 23).  With draw_fog a free cell (code 1) that has not been seen
        is shown at half brightness, each channel >> 1; occupied cells, markers and overlays always at full brightness.

    Besides the VectorEnv API this env consumes actions (`consumes_actions`): `step_into_obs(obs, reward, not_done, actions=...)`
    on the device path; `async_step_at(i, a)` records a, and `advance_on_device` steps exactly the pending envs with their recorded
    actions through the kernels' per-env mask.  `measure_sums` holds the device-side running sums of the four measures."""

    consumes_actions = True
    measure_names = NAV2D_MEASURES
    # what a subclass with another sensor set changes: the observation set SyntheticVectorEnv builds ("nav2d": the point-goal set,
    # "objectnav", "rearrange": head camera + object start / goal / holding, "social": head camera + person sensor / visible),
    # whether an image is rendered
    # without rgb and depth, and the size of a state record
    _sensor_set = "nav2d"
    _renders_without_rgb_depth = False
    _state_bytes = "hab_nav2d_state_bytes"
    _geo_bytes = "hab_nav2d_geo_bytes"  # the size of a field record of the geodesic mode
    num_actions = 4
    # what a subclass with another step changes: the name in the refusals, the library's entries (Euclidean, geodesic; a subclass
    # whose _entries names the Euclidean one alone names the geodesic one in _geo_entry), what
    # `actions` has to be (with _actions_shaped), and the two hooks _sensor_rows and _task_parameters
    _name = "Nav2D"
    _entries = ("hab_nav2d_step", "hab_nav2d_step_geo")
    _geo_entry = None
    _action_dtype, _action_text = torch.int64, "int64 device tensor of shape (N,) or (N, 1)"
    # the library's shortest-path follower of the task (`follower_actions`), None where the task has none, and the shape of its
    # actions after the env count
    _follow_entry = "hab_nav2d_follow"
    _follow_shape = ()

    def __init__(self, num_envs: int, height: int, width: int, seed: int = 100, env_offset: int = 0, use_rgb: bool = True,
                 use_depth: bool = True, num_actions: int = 4, device="cuda", num_obstacles: int = 3, turn_angle: int = 10,
                 max_episode_steps: int = 500, distance: str = "euclidean", top_down_map=None):
        self.num_headings = nav2d_num_headings(turn_angle)
        self.distance = nav2d_distance(distance)
        self.map_parameters = nav2d_map_parameters(top_down_map, self._name)
        if not 0 <= int(num_obstacles) <= NAV2D_MAX_OBSTACLES:
            raise _lib.HabError(f"Nav2D: num_obstacles {num_obstacles} outside 0..{NAV2D_MAX_OBSTACLES}")
        if num_actions != 4:
            raise _lib.HabError(f"Nav2D: the action space is Discrete(4) (STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT), got {num_actions}")
        if int(max_episode_steps) <= 0:
            raise _lib.HabError(f"Nav2D: max_episode_steps {max_episode_steps} must be positive")
        if not (use_rgb or use_depth or self._renders_without_rgb_depth):
            height = width = 0
        super().__init__(num_envs, height, width, seed=seed, env_offset=env_offset, use_rgb=use_rgb, use_depth=use_depth,
                         num_actions=num_actions, device=device, task=self._sensor_set)
        self.num_obstacles, self.turn_angle, self.max_episode_steps = int(num_obstacles), int(turn_angle), int(max_episode_steps)
        dev = self.device
        self._tables = [None if t is None else torch.from_numpy(t).to(dev) for t in nav2d_tables(self.turn_angle, height, width)]
        words = getattr(_lib.lib(), self._state_bytes)() // 4
        self._state = torch.zeros(num_envs, words, dtype=torch.int32, device=dev)
        self.measure_sums = torch.zeros(len(NAV2D_MEASURES), num_envs, device=dev)
        self._geo = None
        if self.distance == "geodesic":
            self._geo = torch.zeros(num_envs, getattr(_lib.lib(), self._geo_bytes)() // 4, dtype=torch.int32, device=dev)
        self._actions_host = np.zeros(num_envs, dtype=np.int64)
        self._infos: List[dict] = [{} for _ in range(num_envs)]
        self.number_of_episodes = [1 << 30] * num_envs  # episodes are generated, never repeated
        # the step entry and the arguments that no call changes, before and after the ones _launch is given
        self._entry = self._entries[0] if self._geo is None else (self._geo_entry or self._entries[1])
        self._step = getattr(_lib.lib(), self._entry)
        field = () if self._geo is None else (ptr(self._geo),)
        self._head = (ptr(self._state), *field, *map(ptr, self._tables))
        self._tail = (ptr(self.measure_sums), self.seed, self.env_offset, self.num_envs, self.H, self.W, self.num_obstacles,
                      self.num_headings, self.max_episode_steps, *self._task_parameters())
        # the top-down map: its layers and records exist, and its update is launched, only where the keyword asks for it
        self._map = self._fog = self._map_rec = self._map_update = None
        if self.map_parameters is not None:
            S, vis, _ = self.map_parameters
            self._map = torch.zeros(num_envs, S, S, dtype=torch.uint8, device=dev)
            self._fog = torch.zeros(num_envs, S, S, dtype=torch.uint8, device=dev)
            self._map_rec = torch.zeros(num_envs, _lib.lib().hab_nav2d_map_rec_bytes() // 4, dtype=torch.int32, device=dev)
            self._map_update = (ptr(self._state), words * 4, ptr(self._tables[0])), (
                ptr(self._map), ptr(self._fog), ptr(self._map_rec), num_envs, S, self.num_obstacles, self.num_headings, self._map_task,
                getattr(self, "num_objects", 0), vis)

    # ---- device fast path ---------------------------------------------------------------------
    def _actions_shaped(self, actions) -> bool:
        return actions.numel() == self.num_envs

    def _sensor_rows(self, obs):
        """The pointers of the entry's sensor destinations, in its order."""
        return ptr(obs.get("rgb")), ptr(obs.get("depth")), ptr(obs.get(GOAL_UUID))

    def _task_parameters(self):
        """The entry's arguments between max_episode_steps and advance; read once, when the env is built."""
        return ()

    def _launch(self, obs, reward, not_done, actions, mask, advance: int):
        if actions is not None and not (actions.dtype == self._action_dtype and self._actions_shaped(actions) and actions.is_contiguous()
                                        and actions.is_cuda):
            raise _lib.HabError(f"{self._name}: actions must be a contiguous {self._action_text}")
        check(self._step(*self._head, ptr(actions), ptr(mask), *self._sensor_rows(obs), ptr(reward), ptr(not_done), *self._tail, advance,
                         stream_ptr()), self._entry)
        if self._map_update is not None:
            records, layers = self._map_update
            check(_lib.lib().hab_nav2d_map_update(*records, ptr(mask), *layers, advance, stream_ptr()), "hab_nav2d_map_update")
            self._frame_obs = obs

    # ---- the top-down map -----------------------------------------------------------------------
    _map_task = NAV2D_MAP_TASK_GOAL  # which words of the record tell the targets (HAB_NAV2D_MAP_TASK_*)
    _frame_keys = ("rgb", "depth")   # the observations of the frame's first two panels
    _frame_obs = None                # the rows the last launch wrote its observations into

    def _need_map(self, method: str):
        if self._map is None:
            raise _lib.HabError(f"{self._name}: {method} needs the top-down map: build the env with top_down_map=dict(...) "
                                "(habitat.task.measurements.top_down_map in a config)")

    def top_down_map(self):
        """The measure's four fields as device tensors: `map` uint8 (N, S, S) of cell codes, `fog_of_war_mask` uint8 (N, S, S),
        `agent_map_coord` int64 (N, 2) = (row, column) of the agent's cell, `agent_angle` float32 (N,) = the heading's angle in
        radians from the host table.  The first two are the env's own tensors, not copies."""
        self._need_map("top_down_map()")
        S = self.map_parameters[0]
        pos = self._state[:, 0:2].view(torch.float32)
        cell = (pos / float(np.float32(8.0) / np.float32(S))).floor().to(torch.int64).clamp_(0, S - 1)  # a float32 division
        angles = torch.arange(self.num_headings, device=self._state.device, dtype=torch.float64) * (2.0 * np.pi / self.num_headings)
        return dict(map=self._map, fog_of_war_mask=self._fog, agent_map_coord=torch.stack([S - 1 - cell[:, 1], cell[:, 0]], 1),
                    agent_angle=angles.to(torch.float32)[self._state[:, 7].long()])

    def frame_size(self, height=None):
        """(rows, columns) of a frame of `render_frames`; the default height is the larger of the image height and 128 rows."""
        height = max(self.H, 128) if height is None else height
        if not whole(height) or height <= 0:
            raise _lib.HabError(f"{self._name}: render_frames: height {height!r} must be a positive whole number")
        width = _lib.lib().hab_nav2d_map_frame_width(int(height), self.H, self.W, int(self.use_rgb), int(self.use_depth))
        check(min(width, 0), "hab_nav2d_map_frame_width")
        return int(height), width

    def render_frames(self, out=None, height=None):
        """The video frame of every env, uint8 (N, height, width, 3), composed on the device in one launch: the env's rgb and depth
        (those of the rows its last step or reset wrote) upscaled by nearest neighbour, then the map with the fog of war and the
        overlays (see the class docstring, Top-down map).  `out` receives the frames (allocated if None) and is returned."""
        self._need_map("render_frames()")
        Hf, Wf = self.frame_size(height)
        N, dev = self.num_envs, self._state.device
        if out is None:
            out = torch.empty(N, Hf, Wf, 3, dtype=torch.uint8, device=dev)
        if not (tuple(out.shape) == (N, Hf, Wf, 3) and out.dtype == torch.uint8 and out.is_contiguous() and out.device == dev):
            raise _lib.HabError(f"{self._name}: render_frames: `out` must be a contiguous uint8 tensor of shape {(N, Hf, Wf, 3)} on {dev}")
        obs = self._frame_obs or {}
        rgb, depth = (obs.get(k) if use else None for k, use in zip(self._frame_keys, (self.use_rgb, self.use_depth)))
        if (self.use_rgb and rgb is None) or (self.use_depth and depth is None):
            raise _lib.HabError(f"{self._name}: render_frames: the last step or reset wrote no {' / '.join(self._frame_keys)} rows; "
                                "reset the env first")
        S, _, draw_fog = self.map_parameters
        check(_lib.lib().hab_nav2d_map_frame(ptr(self._state), self._state.shape[1] * 4, ptr(self._tables[0]), ptr(self._map),
                                             ptr(self._fog), ptr(rgb), ptr(depth), ptr(out), N, S, self.H, self.W, Hf, Wf,
                                             self.num_headings, self._map_task, int(draw_fog), stream_ptr()), "hab_nav2d_map_frame")
        return out

    def reset_into_obs(self, obs):
        self._launch(obs, None, None, None, None, 0)

    def step_into_obs(self, obs, reward, not_done, actions=None, mask=None):
        """One step of every env (or of the envs whose `mask` byte is set) with the task's `actions` (Nav2D-v0: int64 (N,) / (N, 1)):
        the new observations, rewards (N,) and not-done bytes (N,) go straight into the given device tensors."""
        if actions is None:
            raise _lib.HabError(f"{self._name}: step_into_obs needs the actions of the step")
        self._launch(obs, reward, not_done, actions, mask, 1)

    # ---- the shortest-path follower -------------------------------------------------------------
    def _follow_parameters(self):
        """The follower entry's arguments between num_headings and the stream."""
        return ()

    def follower_actions(self, out=None, mask=None, next_d=None, status=None):
        """The actions of the shortest-path follower (habitat's ShortestPathFollower.get_next_action for every env at once): a greedy
        step down the geodesic distance, computed on the device from the env's own records, in the dtype and shape `step_into_obs`
        takes.  tests/nav2d_follow_reference.py states the rule; the kernel matches it bit for bit.  In short: STOP where the episode
        is unreachable, where D_PREV < 0.2 (the success test of the stop then holds) and where no forward of 0.25 m at any heading
        lowers the distance (STUCK); else the heading whose forward leads to the lowest distance, then the fewest turns, then left:
        forward if the agent faces it, else a turn towards it.
        `out` receives the actions (allocated if None) and is returned; `mask` (uint8 (N,)) selects envs, the outputs of the others
        stay untouched; `next_d` (float32 (N,)) receives the distance the env will report after the step of a GO (D_PREV where
        ARRIVED, +inf otherwise), `status` (int32 (N,)) the code 0 GO, 1 ARRIVED, 2 UNREACHABLE, 3 STUCK.  Only Nav2D-v0,
        Nav2DVel-v0 and Nav2DImageNav-v0 (Nav2D-v0's follower on its longer record) in the geodesic distance mode have a follower."""
        if self._follow_entry is None:
            raise _lib.HabError(f"{self._name}: the task has no shortest-path follower (Nav2D-v0 and Nav2DVel-v0 have one)")
        if self.distance != "geodesic":
            raise _lib.HabError(f"{self._name}: the shortest-path follower needs `distance_to_goal: geodesic`, the env has "
                                f"{self.distance!r}")
        return self._advised_actions(self._follow_entry, "follower_actions", self._follow_shape, self._follow_parameters(), out, mask,
                                     next_d, status)

    # ---- the teacher (DAgger) -------------------------------------------------------------------
    _expert_method = "follower_actions"  # which of the task's advisers labels the learner's states; None where the task has none

    def expert_actions(self, out=None, mask=None, next_d=None, status=None):
        """One discrete teacher action per env for imitation (the DAgger updater): `follower_actions` on Nav2D-v0 and Nav2DImageNav-v0, `oracle_actions` on
        Nav2DRearr-v0, with their arguments; `status` holds HAB_NAV2D_ORACLE_* codes, of which the follower's four are the first
        four.  Every other Nav2D task refuses: the velocity tasks' advice is a float row, Nav2DObj-v0 and Nav2DSocial-v0 have no
        adviser.  The Euclidean distance mode refuses as the two advisers do."""
        if self._expert_method is None:
            raise _lib.HabError(f"{self._name}: the task has no discrete teacher for imitation (Nav2D-v0 has the shortest-path follower, "
                                "Nav2DRearr-v0 the pick-and-place oracle)")
        return getattr(self, self._expert_method)(out=out, mask=mask, next_d=next_d, status=status)

    def _advised_actions(self, entry, method, shape, parameters, out, mask, next_d, status):
        """What `follower_actions` and `oracle_actions` share: the checks of the four tensors, then the library's `entry` on the env's
        records.  `shape` is the shape of one env's action, `parameters` the entry's arguments between num_headings and the stream."""
        N, dev = self.num_envs, self._state.device
        if out is None:
            out = torch.zeros((N, *shape), dtype=self._action_dtype, device=dev)
        wanted = ((out, self._action_dtype, self._actions_shaped, "out"), (mask, torch.uint8, None, "mask"),
                  (next_d, torch.float32, None, "next_d"), (status, torch.int32, None, "status"))
        for t, dtype, shaped, what in wanted:
            if t is None:
                continue
            ok = shaped(t) if shaped else tuple(t.shape) == (N,)
            if not (ok and t.dtype == dtype and t.is_contiguous() and t.device == dev):
                raise _lib.HabError(f"{self._name}: {method}: `{what}` must be a contiguous {dtype} tensor for {N} envs on {dev}")
        check(getattr(_lib.lib(), entry)(ptr(self._state), self._state.shape[1] * 4, ptr(self._geo), ptr(self._tables[0]), ptr(mask),
                                         ptr(out), ptr(next_d), ptr(status), N, self.num_obstacles, self.num_headings, *parameters,
                                         stream_ptr()), entry)
        return out

    def reset_into(self, rgb, depth, goal):
        self.reset_into_obs({k: v for k, v in (("rgb", rgb), ("depth", depth), (GOAL_UUID, goal)) if v is not None})

    def step_into(self, rgb, depth, goal, reward, not_done, actions=None, mask=None):
        self.step_into_obs({k: v for k, v in (("rgb", rgb), ("depth", depth), (GOAL_UUID, goal)) if v is not None}, reward, not_done,
                           actions=actions, mask=mask)

    # ---- VectorEnv API (host path) ----------------------------------------------------------------
    def async_step_at(self, index_env: int, action) -> None:
        if isinstance(action, dict):
            action = action["action"]
        a = np.asarray(action)
        top = self.num_actions - 1
        if a.size != 1 or not (np.issubdtype(a.dtype, np.integer) or float(a.item()).is_integer()) or not 0 <= int(a.item()) <= top:
            raise _lib.HabError(f"Nav2D: env {index_env}: action {action!r} outside 0..{top}")
        super().async_step_at(index_env, action)
        self._actions_host[int(index_env)] = int(a.item())

    def advance_on_device(self) -> List[int]:
        """Steps exactly the envs whose step was requested, with their recorded actions, through the kernels' per-env mask: no
        scratch copies, untouched envs keep state and observations.  Returns the ids."""
        ids = sorted(self._pending)
        self._pending.clear()
        if ids:
            actions = torch.from_numpy(self._actions_host.copy()).to(self.device)
            mask = None
            if len(ids) != self.num_envs:
                m = np.zeros(self.num_envs, dtype=np.uint8)
                m[ids] = 1
                mask = torch.from_numpy(m).to(self.device)
            self.step_into_obs(self._own_obs(), self._rew, self._nd, actions=actions, mask=mask)
        return ids

    def step_infos_host(self, ids) -> List[dict]:
        """The scalar infos of the last step of envs `ids`: the four measures where that step ended an episode, else {}."""
        rec = self._state[:, _W_ENDED:_W_LAST + len(NAV2D_MEASURES)].cpu()
        last = rec[:, 1:].contiguous().view(torch.float32).numpy()
        return [dict(zip(NAV2D_MEASURES, (float(x) for x in last[i]))) if int(rec[i, 0]) else {} for i in ids]

    def _advance_pending(self):
        ids = sorted(self._pending)
        super()._advance_pending()
        for i, info in zip(ids, self.step_infos_host(ids)):
            self._infos[i] = info

    def wait_step_at(self, index_env: int):
        obs, rew, done, _ = super().wait_step_at(index_env)
        return obs, rew, done, dict(self._infos[index_env])

    def step(self, actions):
        """VectorEnv.step: all envs, one action each."""
        for i, a in enumerate(actions):
            self.async_step_at(i, a)
        return [self.wait_step_at(i) for i in range(self.num_envs)]

    def current_episodes(self):
        ep = self._state[:, _W_EPISODE].cpu().numpy()
        return [dict(scene_id="nav2d", episode_id=f"{self.env_offset + i}:{int(ep[i])}") for i in range(self.num_envs)]

    def pause_at(self, index: int):
        raise _lib.HabError("Nav2D: episodes are generated and never repeat, so no env is ever paused")


def nav2d_vel_parameters(turn_angle, max_turn_angle, min_abs_lin_speed, min_abs_ang_speed, who: str = "Nav2DVel"):
    """Checks the `habitat.synthetic` keys of Nav2DVel-v0 (and of `who`, a task with the same motion) and returns (num_headings, M, S):
    the largest turn of one step and the smallest turn that is not a stop, both in heading quanta."""
    nh = nav2d_num_headings(turn_angle)
    if not whole(max_turn_angle) or max_turn_angle <= 0 or max_turn_angle % turn_angle != 0 or max_turn_angle > 180:
        raise _lib.HabError(f"{who}: max_turn_angle {max_turn_angle!r} must be a positive multiple of turn_angle {turn_angle} "
                            "(whole degrees), at most 180")
    if not whole(min_abs_ang_speed) or min_abs_ang_speed <= 0 or min_abs_ang_speed % turn_angle != 0 or min_abs_ang_speed > max_turn_angle:
        raise _lib.HabError(f"{who}: min_abs_ang_speed {min_abs_ang_speed!r} must be a positive multiple of turn_angle {turn_angle} "
                            f"(whole degrees), at most max_turn_angle {max_turn_angle}")
    if (isinstance(min_abs_lin_speed, bool) or not isinstance(min_abs_lin_speed, (int, float, np.integer, np.floating))
            or not 0.0 < float(min_abs_lin_speed) <= 0.25):
        raise _lib.HabError(f"{who}: min_abs_lin_speed {min_abs_lin_speed!r} must be a length in (0, 0.25] metres")
    return nh, int(max_turn_angle) // int(turn_angle), int(min_abs_ang_speed) // int(turn_angle)


class Nav2DVelVectorEnv(Nav2DVectorEnv):
    """Nav2DVel-v0: Nav2D-v0 under velocity control, the source whose reward depends on CONTINUOUS actions.  World generation, the
    free-space test, sensors, rendering, the reward formula, the four measures, the state record and the (seed, env, episode) streams
    are Nav2D-v0's (see Nav2DVectorEnv); only the action and the physics of one step differ.  The parameter names follow habitat's
    `velocity_control` action (inputs in [-1, 1] scaled to a linear and an angular range, a stop when both speeds are below their
    minima, sliding along obstacles); the reference's source is not at hand, so the statement below IS this project's specification.
    tests/nav2d_vel_reference.py restates it in numpy and `nav2d_vel_step_kernel` (csrc/nav2d.hip) matches it bit for bit, phi excepted.
    No angle is evaluated on the device: the heading stays an index into the host tables.

    Parameters (`habitat.synthetic`): turn_angle (default 1), the heading quantum, whole degrees dividing 360; max_turn_angle (10), a
    positive multiple of turn_angle, at most 180, M = max_turn_angle / turn_angle; min_abs_lin_speed (0.025) metres in (0, 0.25];
    min_abs_ang_speed (5) degrees, a positive multiple of turn_angle, at most max_turn_angle, S = min_abs_ang_speed / turn_angle;
    allow_sliding (true).
    Action space: Box(-1, 1, (2,), float32), a = (a_lin, a_ang).
    One step (every written operation one float32 rounding, no fused multiply-add):
      1. per component c = min(max(a, -1), 1), and c = 0 for a non-finite a;
      2. step length l = (c_lin + 1) * 0.125: one add, then one multiply, so l is in [0, 0.25];
      3. turn dh = (int) rint(c_ang * M): one float32 multiply rounded half to even; positive is left (TURN_LEFT is h + 1);
      4. stop = (l < min_abs_lin_speed) and (|dh| < S); on stop nothing moves;
      5. otherwise h = (h + dh) mod num_headings and, with (c, s) = dirs[h], the target is nx = px + l * c, ny = py + l * s.  A free
         target is taken and path_length grows by l.  A blocked one counts one collision; then, with sliding, (nx, py) is taken if free
         (path_length grows by |nx - px|), else (px, ny) if free (by |ny - py|), else the agent stays;
      6. distance, reward ((-0.01 + (d_prev - d)) + 2.5 * success, success = stop and d < 0.2), step count,
         done = stop or steps >= max_episode_steps, the measures and their sums, the next episode's world on done and the goal sensor
         are exactly Nav2D-v0's with `stop` in the place of STOP.

    `distance="geodesic"` is Nav2D-v0's geodesic mode, word for word (see Nav2DVectorEnv, Distance): the d of step 6 becomes the
    shortest path round the obstacles; tests/nav2d_geo_reference.py restates it for this task too.

    `step_into_obs(obs, reward, not_done, actions=...)` takes the (N, 2) float32 rows (a_lin, a_ang) the policy stored; the env clamps,
    so the stored action stays unclipped.  `async_step_at(i, a)` takes a length-2 array (or {"action": array})."""

    _name = "Nav2DVel"
    _entries = ("hab_nav2d_vel_step", "hab_nav2d_vel_step_geo")
    _follow_entry, _follow_shape = "hab_nav2d_vel_follow", (2,)
    _expert_method = None  # the velocity follower answers a float row: see Nav2DVectorEnv.expert_actions
    _action_dtype, _action_text = torch.float32, "float32 device tensor of shape (N, 2)"

    def __init__(self, num_envs: int, height: int, width: int, seed: int = 100, env_offset: int = 0, use_rgb: bool = True,
                 use_depth: bool = True, num_actions: int = 1, device="cuda", num_obstacles: int = 3, turn_angle: int = 1,
                 max_episode_steps: int = 500, max_turn_angle: int = 10, min_abs_lin_speed: float = 0.025, min_abs_ang_speed: int = 5,
                 allow_sliding: bool = True, distance: str = "euclidean", top_down_map=None):
        _, self.max_turn_steps, self.stop_turn_steps = nav2d_vel_parameters(turn_angle, max_turn_angle, min_abs_lin_speed,
                                                                            min_abs_ang_speed)
        if not isinstance(allow_sliding, (bool, np.bool_)):
            raise _lib.HabError(f"Nav2DVel: allow_sliding {allow_sliding!r} must be true or false")
        if num_actions != 1:
            raise _lib.HabError(f"Nav2DVel: the task has the one action velocity_control, got {num_actions} actions")
        self.max_turn_angle, self.min_abs_ang_speed = int(max_turn_angle), int(min_abs_ang_speed)
        self.min_abs_lin_speed, self.allow_sliding = float(min_abs_lin_speed), bool(allow_sliding)
        super().__init__(num_envs, height, width, seed=seed, env_offset=env_offset, use_rgb=use_rgb, use_depth=use_depth, device=device,
                         num_obstacles=num_obstacles, turn_angle=turn_angle, max_episode_steps=max_episode_steps,
                         distance=nav2d_distance(distance, "Nav2DVel"), top_down_map=top_down_map)
        self.action_spaces = [spaces.Box(-1.0, 1.0, (2,), np.float32) for _ in range(num_envs)]
        self.orig_action_spaces = self.action_spaces
        self._actions_host = np.zeros((num_envs, 2), dtype=np.float32)

    def _actions_shaped(self, actions) -> bool:
        return tuple(actions.shape) == (self.num_envs, 2)

    def _task_parameters(self):
        return self.max_turn_steps, self.stop_turn_steps, self.min_abs_lin_speed, int(self.allow_sliding)

    def _follow_parameters(self):
        return (self.max_turn_steps,)

    def async_step_at(self, index_env: int, action) -> None:
        if isinstance(action, dict):
            action = action["action"]
        try:
            a = np.asarray(action, dtype=np.float32)
        except (TypeError, ValueError):
            a = None
        if a is None or a.shape != (2,):
            raise _lib.HabError(f"Nav2DVel: env {index_env}: action {action!r} is not a length-2 array (a_lin, a_ang)")
        SyntheticVectorEnv.async_step_at(self, index_env, action)
        self._actions_host[int(index_env)] = a


NAV2D_MAX_OBJECTS, NAV2D_MAX_CATEGORIES = 8, NUM_OBJECT_CATEGORIES


def nav2d_compass_table(turn_angle: int):
    """(num_headings,) float32: the compass reading after k left turns, k * turn_angle in (-pi, pi] (k above the half turn counts as
    k - num_headings), computed in float64 and rounded once."""
    nh = nav2d_num_headings(turn_angle)
    k = np.arange(nh, dtype=np.int64)
    k = np.where(2 * k > nh, k - nh, k)
    return (k.astype(np.float64) * (2.0 * np.pi / nh)).astype(np.float32)


class Nav2DObjVectorEnv(Nav2DVectorEnv):
    """Nav2DObj-v0: Nav2D-v0's world with objects in it and the ObjectNav sensor set, the source on which a policy can only learn by
    looking.  There is no goal position and no goal sensor: the agent is told a category (`objectgoal`) and has to STOP within 1 m of
    the centre of an object of that category, which it can find in `semantic` / `depth` / `rgb` alone.  Arena, rectangles, start,
    heading, the box free test, streams 16-20 and the 0.25 m forward step are Nav2D-v0's (see Nav2DVectorEnv).
    tests/nav2d_obj_reference.py restates the task in numpy; `nav2d_obj_step_kernel` and the object form of `nav2d_render_kernel`
    (csrc/nav2d.hip) match it bit for bit on every output -- no angle function runs on the device.

    Parameters (`habitat.synthetic`): num_objects M in 1..8 (default 3), num_categories C in 1..21 (default 4), besides Nav2D-v0's.
    Objects.  Upright cylinders of radius 0.3 m from floor to ceiling, placed after the start from the streams 21 (positions, 16
      candidates (0.1 + 7.8 u, 0.1 + 7.8 u') per object), 22 (categories) and 23 (target).  Object j takes its first candidate that
      lies in [0.5, 7.5]^2, is not strictly inside a rectangle grown by 0.3 m, is at least 1 m from the start and at least 1 m from
      every earlier object; failing all 16, the first of 28 fixed points one metre apart on the square through (0.5, 0.5) and
      (7.5, 7.5) that keeps the two distances (one always does, see the restatement).  Its category is word j of stream 22 modulo C.
      A position closer than 0.4 m to a centre is not free.
    Target.  The category of object (word 0 of stream 23 modulo M).  d = the distance to the nearest centre of that category; the
      nearest instance may change during an episode.
    Actions.  Discrete(4) or Discrete(6) in habitat's order; LOOK_UP and LOOK_DOWN change nothing and cost a step.
    Reward, end of an episode and the four measures are Nav2D-v0's with this d; success = STOP and d < 1.0.
    Sensors.  objectgoal int64 (1,); gps float32 (2,) = (dot, cross) of position - start in the start heading's frame; compass
      float32 (1,) = (heading - start heading) * turn_angle in (-pi, pi] from a host table; depth and rgb as Nav2D-v0 with the
      cylinders as geometry (a fixed colour per category) and no goal marker; semantic int32 (H, W, 1): floor 0, ceiling 1, walls 2,
      rectangles 3, an object 4 + category.  The observation-space ranges are the hashed ObjectNav task's, so the same policy is built.
      `semantic` is always rendered, also without rgb and depth.  `step_into_obs` writes any of rgb, depth, semantic, objectgoal, gps,
      compass, whichever rows `obs` holds; `actions` is int64 (N,) / (N, 1) as for Nav2D-v0.

    Distance (`distance`, from `habitat.synthetic.distance_to_goal`).  "euclidean", the default, is all of the above.  "geodesic"
      changes the d of the reward, the success test (STOP and d < 1.0), distance_to_goal and d_start / the SPL numerator -- nothing
      else: world, objects, target, physics, sensors and render stay -- to the shortest path to the nearest instance of the target
      category, habitat's ObjectNav definition.  It is Nav2D-v0's geodesic mode (see Nav2DVectorEnv, Distance: boxes, the
      separating-axis test, E = 2^-10, one float32 rounding per operation) with a field that has several targets.
      tests/nav2d_obj_geo_reference.py restates it; `nav2d_obj_geo_build_kernel` and `nav2d_obj_geo_step_kernel` match it bit for bit.
      * Obstacles of the graph.  The K rectangles grown by the agent radius, with Nav2D-v0's expressions, and for object m the
        axis-aligned square [ox - 0.4, ox + 0.4] x [oy - 0.4, oy + 0.4], the bounding square of its keep-out disc: up to 16 boxes.
        The visibility boxes are these shrunk by E.  The square is a deliberate over-approximation of the disc: every path of the
        boxed world is a path of the real one, up to E at the four tangent points, and the graph stays one of boxes.
      * Nodes.  64: node 4k + j is corner j of rectangle box k, node 32 + 4m + j corner j of object m's square, in the corner order
        (X0, Y0), (X1, Y0), (X0, Y1), (X1, Y1).  A node is valid iff it is free (arena, rectangles, discs).
      * Targets.  The centres of all objects of the target category.  The square of object t does not block a segment that ends at
        centre t; only that box is left out for that segment, all others block it as usual.
      * Field.  D[i] = +inf for invalid nodes, else the least rounded path sum from node i to any target centre: the last hop is
        the min over the target centres the node sees, then Jacobi sweeps D <- min(D, min_j fl(w[i][j] + D[j])) until one changes
        nothing, at most 4 (K + M).
      * geo(p) = the least of d(p, c_t) over the target centres p sees (own box t ignored) and fl(d(p, node_i) + D[i]) over the
        nodes with finite D that p sees; +inf if p sees none of these.  A position in the sliver between a disc and its square
        sees nothing through that box: a lost step by Nav2D-v0's rule, unless it is the target's own sliver, where the centre is seen.
      * Episode.  As Nav2D-v0: the field is built at the beginning and g0 = geo(start).  g0 finite: d_start = d_prev = g0 and every
        step's d is geo(p); where that is +inf, d = d_prev and the lost-step counter goes up.  g0 infinite: the episode keeps the
        Euclidean nearest-centre distance throughout.  The state words (gx, gy) stay the Euclidean-nearest centre in both modes.
      The field records (`_geo`, (N, 72) int32: 64 D, reachable, sweeps, lost steps, five zeros) exist in this mode only.  The field
      is built on the device, so in this mode the class itself refuses a device that is no GPU."""

    _name = "Nav2DObj"
    _expert_method = None  # no teacher: see Nav2DVectorEnv.expert_actions
    _entries = ("hab_nav2d_obj_step", "hab_nav2d_obj_step_geo")
    _follow_entry = None  # no shortest-path follower: see Nav2DVectorEnv.follower_actions
    _sensor_set = "objectnav"
    _map_task = NAV2D_MAP_TASK_OBJ
    _renders_without_rgb_depth = True
    _state_bytes = "hab_nav2d_obj_state_bytes"
    _geo_bytes = "hab_nav2d_obj_geo_bytes"

    def __init__(self, num_envs: int, height: int, width: int, seed: int = 100, env_offset: int = 0, use_rgb: bool = True,
                 use_depth: bool = True, num_actions: int = 6, device="cuda", num_obstacles: int = 3, turn_angle: int = 10,
                 max_episode_steps: int = 500, num_objects: int = 3, num_categories: int = 4, distance: str = "euclidean", top_down_map=None):
        if nav2d_distance(distance, "Nav2DObj") == "geodesic" and torch.device(device).type != "cuda":
            raise _lib.HabError("Nav2DObj: distance 'geodesic' builds its field on the GPU; no GPU device given")
        if not whole(num_objects) or not 1 <= num_objects <= NAV2D_MAX_OBJECTS:
            raise _lib.HabError(f"Nav2DObj: num_objects {num_objects!r} outside 1..{NAV2D_MAX_OBJECTS}")
        if not whole(num_categories) or not 1 <= num_categories <= NAV2D_MAX_CATEGORIES:
            raise _lib.HabError(f"Nav2DObj: num_categories {num_categories!r} outside 1..{NAV2D_MAX_CATEGORIES}")
        if num_actions not in (4, 6):
            raise _lib.HabError("Nav2DObj: the action space is Discrete(4) (STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT) or Discrete(6) "
                                f"(with LOOK_UP, LOOK_DOWN), got {num_actions}")
        if int(height) <= 0 or int(width) <= 0:
            raise _lib.HabError(f"Nav2DObj: the semantic image is always rendered, so the image size {height} x {width} must be positive")
        self.num_objects, self.num_categories, self.num_actions = int(num_objects), int(num_categories), int(num_actions)
        super().__init__(num_envs, height, width, seed=seed, env_offset=env_offset, use_rgb=use_rgb, use_depth=use_depth, device=device,
                         num_obstacles=num_obstacles, turn_angle=turn_angle, max_episode_steps=max_episode_steps, distance=distance,
                         top_down_map=top_down_map)
        self.task = "nav2dobj"
        self.action_spaces = [spaces.Discrete(self.num_actions) for _ in range(num_envs)]
        self.orig_action_spaces = self.action_spaces
        self._compass_table = torch.from_numpy(nav2d_compass_table(self.turn_angle)).to(self.device)

    def _sensor_rows(self, obs):
        return (ptr(obs.get("rgb")), ptr(obs.get("depth")), ptr(obs.get("semantic")), ptr(obs.get("objectgoal")), ptr(obs.get("gps")),
                ptr(obs.get("compass")), ptr(self._compass_table))

    def _task_parameters(self):
        return self.num_objects, self.num_categories, self.num_actions

    def reset_into(self, rgb, depth, goal):
        raise _lib.HabError("Nav2DObj: the task has no pointgoal sensor; use reset_into_obs with the ObjectNav sensor rows")

    def step_into(self, rgb, depth, goal, reward, not_done, actions=None, mask=None):
        raise _lib.HabError("Nav2DObj: the task has no pointgoal sensor; use step_into_obs with the ObjectNav sensor rows")


NAV2D_REARR_MEASURES = ("success", "did_pick_object", "object_to_goal_distance", "collisions")
NAV2D_REARR_SENSORS = ("head_rgb", "head_depth", "obj_start_sensor", "obj_goal_sensor", "is_holding")


class Nav2DRearrVectorEnv(Nav2DVectorEnv):
    """Nav2DRearr-v0: a pick-and-place task in Nav2D-v0's world, read through the rearrangement observation set: `head_depth` (and
    optionally `head_rgb`) for the visual encoder and three raw float32 1-D sensors that PointNavResNetPolicy fuses into its recurrent
    input.  The goal exists only in those sensors, so the task can be solved only through the fused columns.  Arena, rectangles, start,
    heading, the box free test, streams 16-20, the 0.25 m forward step and the turn table are Nav2D-v0's (see Nav2DVectorEnv).
    tests/nav2d_rearr_reference.py restates the task in numpy; `nav2d_rearr_step_kernel` and the rearrangement form of
    `nav2d_render_kernel` (csrc/nav2d.hip) match it bit for bit on every output -- no angle function runs on the device, every float32
    operation is one rounding in the written order.

    Parameters (`habitat.synthetic`): start_holding (bool, default false), besides Nav2D-v0's num_obstacles and turn_angle, and
      distance_to_goal (see Distance below; "euclidean", the default, is what the following paragraphs describe).
    Places.  The object's start o0 and the goal g are the positions Nav2DObj-v0 gives objects 0 and 1 of the same (seed, env, episode)
      world with num_objects = 2 (see Nav2DObjVectorEnv, Objects: stream 21, 16 candidates, the box [0.5, 7.5]^2, not strictly inside
      a rectangle grown by 0.3 m, at least 1 m from the start and from the earlier object, the 28-slot ring).  Categories and the target
      stream are not used.  The goal is a place, not geometry: it never blocks the agent and is never in depth.
    Object and holding.  An upright cylinder of radius 0.3 m at o, initially o0, and a flag h, initially start_holding.  While h = 1
      the object travels with the agent: it is no geometry, blocks nothing, is not rendered and o = p.  While h = 0 a position closer
      than 0.4 m to o is not free (Nav2DObj-v0's keep-out).
    Actions.  Discrete(6): 0 STOP, 1 MOVE_FORWARD, 2 TURN_LEFT, 3 TURN_RIGHT, 4 PICK, 5 PLACE.  MOVE_FORWARD is Nav2D-v0's with this
      free test; a refused move counts a collision.  With (c, s) the heading's table row, PICK succeeds iff h = 0, d(p, o) < 1.0 and
      (ox - px) * c + (oy - py) * s > 0 (the front half-plane); then h = 1.  PLACE succeeds iff h = 1 and q = p + 0.5 * dir (a float32
      multiply, then a separate add) lies in [0.5, 7.5]^2 and not strictly inside a rectangle grown by 0.3 m; then o = q and h = 0.  A
      refused PICK or PLACE changes nothing but the record's `invalid` counter.
    Reward.  a = d(p, o), 0 while holding; b = d(o, g); Phi = a + b;
      reward = ((-0.01 + (Phi_prev - Phi)) + 1.0 * [this step made the episode's first successful PICK]) + 2.5 * success,
      success = STOP and h = 0 and b < 0.5.  The episode ends on STOP or at max_episode_steps; on done the next episode's world is
      generated, its first observation is what the step returns and not_done = 0.
    Measures.  success; did_pick_object, 1 if h was ever 1 in the episode (so 1 under start_holding); object_to_goal_distance = b at
      the end; collisions.
    Sensors, in observation-space order.  head_rgb (H, W, 3) uint8, optional; head_depth (H, W, 1) float32; obj_start_sensor (2,)
      float32 = (dot, cross) of o0 - p in the heading's frame (dot = dx * c + dy * s, cross = c * dy - s * dx), which refers to the
      START position as habitat's sensor does and goes stale once the object has been moved -- after a misplaced PLACE the object can
      be found again only in the image; obj_goal_sensor (2,) the same for g; is_holding (1,) in {0, 1}.  head_depth is Nav2D-v0's depth
      with the cylinder as geometry while h = 0 (Nav2DObj-v0's ray-circle test); head_rgb is the same with the object in category 0's
      colour and the goal drawn as Nav2D-v0's red marker cylinder (radius 0.2 m), in rgb only.  There is no pointgoal, gps or compass.
      Without head_rgb and head_depth nothing is rendered.

    Distance (`distance`, from `habitat.synthetic.distance_to_goal`).  "geodesic" changes the d inside Phi, the success test b < 0.5,
      object_to_goal_distance and d_prev / d_start -- nothing else: world, places, physics, the PICK and PLACE rules, sensors, render and
      the state record stay -- to shortest paths round the obstacles, as habitat defines its rearrangement navigation rewards.
      tests/nav2d_rearr_geo_reference.py restates it; `nav2d_rearr_geo_build_kernel` and `nav2d_rearr_geo_step_kernel` match it bit for
      bit.  Every float32 operation is one rounding in the written order.
      * Graph.  Nav2D-v0's, word for word (see Nav2DVectorEnv, Distance): the K rectangles grown by the agent radius, visibility
        boxes shrunk by E = 2^-10, the separating-axis test, the 4K corner nodes; a node is valid iff it is free by Nav2D-v0's box
        test.  The object is never an obstacle of the graph and never invalidates a node: leg b is walked carrying the object, which
        is then no geometry; leg a ends at the object, so its own keep-out is left out, as Nav2DObj-v0 leaves out the target's own
        square; and there is no second object.  So a path of leg a may pass within 0.4 m of o -- where the agent is already within
        the 1.0 m reach.  o0, g and every placed q lie outside the rectangles grown by 0.3 m, so all segment ends are ordinary
        points of the graph.
      * Two fields per env.  DG[32] towards the goal g, built when an episode begins.  DO[32] towards the object's resting place,
        built whenever the object comes to rest: at the beginning of an episode without start_holding (target o0) and at every
        successful PLACE (target q).  While the object has not rested in the episode, DO is +inf in all words and sweeps_obj = 0.
        Both are Nav2D-v0's field: last hops, then Jacobi sweeps until one changes nothing, at most 4K.
      * geo_T(x) is Nav2D-v0's geo from the point x with the target T and its field.
      * Terms after the physics of a step.  Holding: a = 0, b = geo_g(p).  Not holding: a = geo_o(p), and b is the value evaluated
        when the object came to rest, kept while it rests: geo_g(o0) from the episode's beginning, geo_g(q) from a PLACE.  A PLACE
        step is, in order: o = q, holding = 0, build DO towards q, b = geo_g(q), a = geo_q(p).  A PICK step: a = 0, b = geo_g(p).
        Phi = a + b.
      * Lost steps.  A term that comes out +inf keeps the value it had after the previous step, and the step counts once in
        lost_steps.  The previous a and b are kept in the field record.
      * Episode.  At its beginning the fields are built and a0 = geo_o0(start), b0 = geo_g(o0); under start_holding a0 = 0 and
        b0 = geo_g(start).  Both finite: reachable = 1 and d_start = d_prev = a0 + b0.  Otherwise reachable = 0 and the episode keeps
        the Euclidean Phi, b and success test throughout (Nav2D-v0's rule for a walled-off goal); no field is rebuilt in such an
        episode, and the record keeps a0 and b0 as they came out.
      * At K = 0 there are no nodes, every geo is the direct distance and all outputs are bitwise those of the Euclidean mode.
      The field records (`_geo`, (N, 72) int32: 32 DG, 32 DO, a, b, reachable, sweeps_goal, sweeps_obj, lost_steps, rebuilds -- the
      successful PLACEs that rebuilt DO -- and one zero; HAB_NAV2D_REARR_GEO_W_*) exist in this mode only.  The fields are built on
      the device, so in this mode the class itself refuses a device that is no GPU.

    `step_into_obs` writes whichever of the five rows `obs` holds; `actions` is int64 (N,) / (N, 1) as for Nav2D-v0.  The record's
    words beyond Nav2D-v0's are named in include/habitat_amd.h (HAB_NAV2D_REARR_W_*).  In the geodesic mode `oracle_actions` returns
    the actions of the pick-and-place oracle (common/rearrange_oracle.py)."""

    _name = "Nav2DRearr"
    _entries = ("hab_nav2d_rearr_step",)
    _follow_entry = None  # no shortest-path follower: see Nav2DVectorEnv.follower_actions
    _oracle_entry = "hab_nav2d_rearr_oracle"  # the library's pick-and-place oracle of the task (`oracle_actions`), None where it has none
    _expert_method = "oracle_actions"
    _geo_entry = "hab_nav2d_rearr_step_geo"
    _geo_bytes = "hab_nav2d_rearr_geo_bytes"
    _sensor_set = "rearrange"
    _map_task, _frame_keys = NAV2D_MAP_TASK_REARR, ("head_rgb", "head_depth")
    _state_bytes = "hab_nav2d_rearr_state_bytes"
    measure_names = NAV2D_REARR_MEASURES
    num_actions = 6

    def __init__(self, num_envs: int, height: int, width: int, seed: int = 100, env_offset: int = 0, use_rgb: bool = False,
                 use_depth: bool = True, num_actions: int = 6, device="cuda", num_obstacles: int = 3, turn_angle: int = 10,
                 max_episode_steps: int = 500, start_holding: bool = False, distance: str = "euclidean", top_down_map=None):
        self._check_distance(distance, device)
        if not isinstance(start_holding, (bool, np.bool_)):
            raise _lib.HabError(f"Nav2DRearr: start_holding {start_holding!r} must be true or false")
        if num_actions != 6:
            raise _lib.HabError("Nav2DRearr: the action space is Discrete(6) (STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT, PICK, PLACE), "
                                f"got {num_actions}")
        if (use_rgb or use_depth) and (int(height) <= 0 or int(width) <= 0):
            raise _lib.HabError(f"Nav2DRearr: the image size {height} x {width} must be positive")
        self.start_holding = bool(start_holding)
        super().__init__(num_envs, height, width, seed=seed, env_offset=env_offset, use_rgb=use_rgb, use_depth=use_depth, device=device,
                         num_obstacles=num_obstacles, turn_angle=turn_angle, max_episode_steps=max_episode_steps, distance=distance,
                         top_down_map=top_down_map)
        self.task = "nav2drearr"
        self.action_spaces = [spaces.Discrete(6) for _ in range(num_envs)]
        self.orig_action_spaces = self.action_spaces

    @classmethod
    def _check_distance(cls, distance, device):
        """The geodesic mode builds its fields on the device: refused where that is no GPU, before the device is touched."""
        if nav2d_distance(distance, cls._name) == "geodesic" and torch.device(device).type != "cuda":
            raise _lib.HabError(f"{cls._name}: distance 'geodesic' builds its fields on the GPU; without a GPU device the task has "
                                "Euclidean distances only")

    def oracle_actions(self, out=None, mask=None, next_d=None, status=None):
        """The actions of the pick-and-place oracle, one per env, computed on the device from the env's own records (which it does
        not write) in the dtype and shape `step_into_obs` takes: go to the object down the field DO, PICK, carry it down DG, PLACE
        where it will rest within the success distance, STOP.  tests/nav2d_rearr_oracle_reference.py states the rule;
        `nav2d_rearr_oracle_kernel` matches it bit for bit.  In short, with "the fewest turns" the least (|delta|, delta < 0) of the
        signed turns from the heading: STOP where the episode is unreachable and where the object rests with b < 0.5 (ARRIVED: the
        success test of that stop holds).  Not holding: within the 1.0 m reach the heading that has the object ahead by the PICK
        rule's dot test and the fewest turns wins, PICK if the agent faces it, else a turn; out of reach a greedy step down geo_o
        as `follower_actions` takes it, below the term a, with the task's free test.  Holding: every heading whose PLACE would be
        accepted and leave the object with geo_g(q) < 0.5 is eligible and the fewest turns win, PLACE if the agent faces it, else a
        turn; where none is eligible a greedy step down geo_g below the term b.  STOP where no forward lowers the leg's term
        (STUCK, an honest give-up).
        `out` receives the actions (allocated if None) and is returned; `mask` (uint8 (N,)) selects envs, the outputs of the others
        stay untouched; `next_d` (float32 (N,)) receives the leg's term as the env will report it after the step (a not holding, b
        holding; 0 at a PICK, geo_g(q) at a PLACE, b where ARRIVED, +inf where UNREACHABLE or STUCK), `status` (int32 (N,)) the code
        0 GO, 1 ARRIVED, 2 UNREACHABLE, 3 STUCK, 4 PICK, 5 PLACE.  Only Nav2DRearr-v0 in the geodesic distance mode has the oracle."""
        if self._oracle_entry is None:
            raise _lib.HabError(f"{self._name}: the task has no pick-and-place oracle (Nav2DRearr-v0 has one: under velocity and grip "
                                "control turning to face and then gripping is not one step's choice)")
        if self.distance != "geodesic":
            raise _lib.HabError(f"{self._name}: the pick-and-place oracle needs `distance_to_goal: geodesic`, the env has "
                                f"{self.distance!r}")
        return self._advised_actions(self._oracle_entry, "oracle_actions", (), (), out, mask, next_d, status)

    def _sensor_rows(self, obs):
        return tuple(ptr(obs.get(k)) for k in NAV2D_REARR_SENSORS)

    def _task_parameters(self):
        return (int(self.start_holding),)

    def _own_obs(self):
        o = {}
        if self.use_rgb:
            o["head_rgb"] = self._rgb
        if self.use_depth:
            o["head_depth"] = self._depth
        o.update(self._obj)
        return o

    def _host_obs(self) -> List[Dict[str, np.ndarray]]:
        host = {k: v.cpu().numpy() for k, v in self._own_obs().items()}
        return [{k: v[i] for k, v in host.items()} for i in range(self.num_envs)]

    def step_infos_host(self, ids) -> List[dict]:
        """The scalar infos of the last step of envs `ids`: this task's four measures where that step ended an episode, else {}."""
        return [dict(zip(NAV2D_REARR_MEASURES, info.values())) if info else {} for info in super().step_infos_host(ids)]

    def reset_into(self, rgb, depth, goal):
        raise _lib.HabError("Nav2DRearr: the task has no pointgoal sensor; use reset_into_obs with the rearrangement sensor rows")

    def step_into(self, rgb, depth, goal, reward, not_done, actions=None, mask=None):
        raise _lib.HabError("Nav2DRearr: the task has no pointgoal sensor; use step_into_obs with the rearrangement sensor rows")


class Nav2DRearrVelVectorEnv(Nav2DRearrVectorEnv):
    """Nav2DRearrVel-v0: pick and place under velocity and grip control, the source on which the Gaussian head, the previous-action
    embedding, float action storage and the fused sensor columns run together.  The task is Nav2DRearr-v0 word for word (see
    Nav2DRearrVectorEnv) except the action and the physics of one step.  What stays the same: world, places, object, holding flag,
    `start_holding`, keep-out 0.4 m, reach 1.0 m, arm 0.5 m, potential Phi = d(p, o) + d(o, g), pick bonus, success radius 0.5 m, the
    four measures, the five sensors, rendering, the state record, streams, and the two distance modes: `distance="geodesic"` is
    Nav2DRearr-v0's geodesic mode, word for word (see Nav2DRearrVectorEnv, Distance), with `stop` in STOP's place;
    tests/nav2d_rearr_geo_reference.py restates it for this task too.
    tests/nav2d_rearr_vel_reference.py restates the task in numpy; `nav2d_rearr_vel_step_kernel` (csrc/nav2d.hip) matches it bit for
    bit on every output.  No angle function runs on the device; the heading stays an index into the host tables.

    Parameters (`habitat.synthetic`): Nav2DVel-v0's motion parameters (see Nav2DVelVectorEnv): turn_angle (default 1 here as there),
      max_turn_angle, min_abs_lin_speed, min_abs_ang_speed, allow_sliding, checked by `nav2d_vel_parameters`, giving M and S; and
      Nav2DRearr-v0's start_holding and num_obstacles.
    Action space: Box(-1, 1, (3,), float32), a = (a_lin, a_ang, a_grip).
    One step (every written float32 operation is one rounding, no fused multiply-add), in this order:
      1. per component c = min(max(a, -1), 1), and c = 0 for a non-finite a: Nav2DVel-v0's step 1, on three components;
      2. l = (c_lin + 1) * 0.125; dh = (int) rint(c_ang * M); stop = (l < min_abs_lin_speed) and (|dh| < S): Nav2DVel-v0's steps 2-4,
         bit for bit;
      3. if not stop: h = (h + dh) mod num_headings and, with (c, s) = dirs[h], the target is (px + l * c, py + l * s).  A position is
         free iff Nav2D-v0's box test holds and (holding or not d(pos, o) < 0.4): Nav2DRearr-v0's MOVE_FORWARD test.  A free target
         is taken and path grows by l.  A blocked target counts one collision; with sliding (nx, py) is then tried, else (px, ny),
         exactly as Nav2DVel-v0's step 5 with this free test and its path increments.  On stop nothing moves;
      4. grip, evaluated on every step (stop or not), after step 3, with the new position and the new heading's (c, s):
         c_grip > 0 and holding = 0 is a PICK attempt under Nav2DRearr-v0's rule: it needs d(p, o) < 1.0 and
         (ox - px) * c + (oy - py) * s > 0; on success holding = held = 1, picks += 1 and first_pick = (picks was 0); on refusal
         invalid += 1.  c_grip < 0 and holding = 1 is a PLACE attempt under Nav2DRearr-v0's rule: it needs q = p + 0.5 * dir inside
         [0.5, 7.5]^2 and not strictly inside a grown rectangle; on success o = q and holding = 0; on refusal invalid += 1.  Every
         other combination -- c_grip == 0, c_grip > 0 while holding, c_grip < 0 with empty hands -- changes nothing and counts
         nothing.  While holding, o = p;
      5. end of step: Nav2DRearr-v0's, with `stop` in STOP's place: reward = ((-0.01 + (Phi_prev - Phi)) + 1.0 * first_pick) +
         2.5 * success; success = stop and holding = 0 and b < 0.5, so "release and stand still" in one step can succeed;
         done = stop or steps >= max_episode_steps; measures, sums, the next episode's world on done and the three vector sensors
         are as there.

    `step_into_obs(obs, reward, not_done, actions=...)` takes the (N, 3) float32 rows the policy stored; the env clamps, so the stored
    action stays unclipped.  `async_step_at(i, a)` takes a length-3 array (or {"action": array})."""

    _name = "Nav2DRearrVel"
    _entries = ("hab_nav2d_rearr_vel_step",)
    _oracle_entry = None  # no pick-and-place oracle: see Nav2DRearrVectorEnv.oracle_actions
    _expert_method = None  # no discrete teacher: see Nav2DVectorEnv.expert_actions
    _geo_entry = "hab_nav2d_rearr_vel_step_geo"
    _action_dtype, _action_text = torch.float32, "float32 device tensor of shape (N, 3)"
    num_actions = 1

    def __init__(self, num_envs: int, height: int, width: int, seed: int = 100, env_offset: int = 0, use_rgb: bool = False,
                 use_depth: bool = True, num_actions: int = 1, device="cuda", num_obstacles: int = 3, turn_angle: int = 1,
                 max_episode_steps: int = 500, start_holding: bool = False, max_turn_angle: int = 10, min_abs_lin_speed: float = 0.025,
                 min_abs_ang_speed: int = 5, allow_sliding: bool = True, distance: str = "euclidean", top_down_map=None):
        _, self.max_turn_steps, self.stop_turn_steps = nav2d_vel_parameters(turn_angle, max_turn_angle, min_abs_lin_speed,
                                                                            min_abs_ang_speed, "Nav2DRearrVel")
        if not isinstance(allow_sliding, (bool, np.bool_)):
            raise _lib.HabError(f"Nav2DRearrVel: allow_sliding {allow_sliding!r} must be true or false")
        if not isinstance(start_holding, (bool, np.bool_)):
            raise _lib.HabError(f"Nav2DRearrVel: start_holding {start_holding!r} must be true or false")
        if num_actions != 1:
            raise _lib.HabError(f"Nav2DRearrVel: the task has the one action velocity_control (with its grip component), got {num_actions} actions")
        if (use_rgb or use_depth) and (int(height) <= 0 or int(width) <= 0):
            raise _lib.HabError(f"Nav2DRearrVel: the image size {height} x {width} must be positive")
        self.max_turn_angle, self.min_abs_ang_speed = int(max_turn_angle), int(min_abs_ang_speed)
        self.min_abs_lin_speed, self.allow_sliding = float(min_abs_lin_speed), bool(allow_sliding)
        super().__init__(num_envs, height, width, seed=seed, env_offset=env_offset, use_rgb=use_rgb, use_depth=use_depth, device=device,
                         num_obstacles=num_obstacles, turn_angle=turn_angle, max_episode_steps=max_episode_steps,
                         start_holding=start_holding, distance=distance, top_down_map=top_down_map)
        self.task = "nav2drearrvel"
        self.action_spaces = [spaces.Box(-1.0, 1.0, (3,), np.float32) for _ in range(num_envs)]
        self.orig_action_spaces = self.action_spaces
        self._actions_host = np.zeros((num_envs, 3), dtype=np.float32)

    def _actions_shaped(self, actions) -> bool:
        return tuple(actions.shape) == (self.num_envs, 3)

    def _task_parameters(self):
        return (int(self.start_holding), self.max_turn_steps, self.stop_turn_steps, self.min_abs_lin_speed, int(self.allow_sliding))

    def async_step_at(self, index_env: int, action) -> None:
        if isinstance(action, dict):
            action = action["action"]
        try:
            a = np.asarray(action, dtype=np.float32)
        except (TypeError, ValueError):
            a = None
        if a is None or a.shape != (3,):
            raise _lib.HabError(f"Nav2DRearrVel: env {index_env}: action {action!r} is not a length-3 array (a_lin, a_ang, a_grip)")
        SyntheticVectorEnv.async_step_at(self, index_env, action)
        self._actions_host[int(index_env)] = a

    def reset_into(self, rgb, depth, goal):
        raise _lib.HabError("Nav2DRearrVel: the task has no pointgoal sensor; use reset_into_obs with the rearrangement sensor rows")

    def step_into(self, rgb, depth, goal, reward, not_done, actions=None, mask=None):
        raise _lib.HabError("Nav2DRearrVel: the task has no pointgoal sensor; use step_into_obs with the rearrangement sensor rows")


NAV2D_SOCIAL_MEASURES = ("has_found_person", "following_rate", "first_encounter_steps", "collisions")
NAV2D_SOCIAL_SENSORS = ("head_rgb", "head_depth", "person_sensor", "person_visible")


class Nav2DSocialVectorEnv(Nav2DVectorEnv):
    """Nav2DSocial-v0: find a person who walks about Nav2D-v0's world, then stay near and facing them.  It is the one source whose
    world changes on its own, whose reward is no potential, whose fused sensor is absent for most of an episode and whose episodes
    end at the step limit alone.  Read through `head_depth` (and optionally `head_rgb`) and two raw float32 1-D sensors that
    PointNavResNetPolicy fuses into its recurrent input, under Nav2DVel-v0's velocity control.  A measurement source, not a simulator.
    tests/nav2d_social_reference.py restates the task in numpy; `nav2d_social_step_kernel`, `nav2d_social_build_kernel` and the
    social form of `nav2d_render_kernel` (csrc/nav2d.hip) match it bit for bit on every output -- no angle function runs on the
    device, every float32 operation is one rounding in the written order, division and square root are correctly rounded.

    World.  Nav2D-v0's, unchanged (see Nav2DVectorEnv): the arena, K = num_obstacles rectangles, start, heading table, streams
      16-20 and the 0.1 m box free test.  There is no goal; the record's (gx, gy) are zero.
    Person.  An upright cylinder of radius 0.3 m at h.  Initially h is the position Nav2DObj-v0 gives object 0 of the same
      (seed, env, episode) world with num_objects = 1 (see Nav2DObjVectorEnv, Objects: stream 21, 16 candidates, the box
      [0.5, 7.5]^2, not strictly inside a rectangle grown by 0.3 m, at least 1 m from the start, the 28-slot ring).  A position
      closer than 0.4 m to h is not free for the agent (the keep-out of the rearrangement object); a refused move counts a collision.
      The person walks as a POINT on Nav2D-v0's visibility graph (see Nav2DVectorEnv, Distance: boxes grown by the agent's 0.1 m,
      visibility boxes shrunk by E = 2^-10, the separating-axis test, the 4K corner nodes valid iff free), so the rendered cylinder
      may overlap a rectangle's corner by up to 0.2 m; depth is the minimum over hits either way.
    Waypoints.  Waypoint j = 0, 1, ... of an episode comes from stream 24, keyed by (seed, 24, env, episode): candidate i = 0..15 is
      (0.1 + 7.8 u_2(16j+i), 0.1 + 7.8 u_2(16j+i)+1), and the waypoint is the first candidate that lies in [0.5, 7.5]^2, is not
      strictly inside a rectangle grown by 0.3 m and is at least 1 m (float32 d >= 1) from the person's current position; failing
      all 16, the first of Nav2DObj-v0's 28 ring slots that passes the same three tests (an open disc of radius 1 holds at most three
      slots, so one does).  The field DW[32] towards the waypoint is Nav2D-v0's field (last hops, then Jacobi sweeps until one
      changes nothing, at most 4K), built when an episode begins and again inside the step whenever the waypoint changes.  It is
      stored per env in the record; graph weights are computed only when a field is built.
    Parameters (`habitat.synthetic`): Nav2DVel-v0's turn_angle (default 1), max_turn_angle (10), min_abs_lin_speed (0.025),
      min_abs_ang_speed (5), allow_sliding (true), checked by `nav2d_vel_parameters`; person_speed v in (0, 0.25] metres per step
      (default 0.125); person_always_visible (bool, default false); num_obstacles.
    Action space: Box(-1, 1, (2,), float32), a = (a_lin, a_ang).
    One step, in this order:
      1. The agent moves against the person's OLD position: Nav2DVel-v0's steps 1-5 (`vel_clamp`, `vel_decode`, `vel_move`) with
         this task's free test.  The velocity stop is standing still; it never ends the episode.
      2. The person moves against the agent's NEW position.  Candidate i < 32 is node c_i with the value fl(d(h, c_i) + DW[i]) where
         DW[i] is finite, h sees c_i and d(h, c_i) is not exactly 0 (a person standing on node i would otherwise tie with its own
         zero-length hop at the field's fixed point and never leave).  Candidate 32 is the waypoint w with the value d(h, w) where h
         sees it.  The least value wins; ties go to the waypoint, then to the lowest node index.  No candidate: the person stays,
         waypoint j + 1 is drawn, its field built and person_lost goes up.  Otherwise, with t the chosen hop's end, L = d(h, t):
         h' = t exactly if L <= v, else h' = h + (v / L) * (t - h) (one division, then a multiply and an add per component); what is
         left of the step is dropped.  If d(h', p) < 0.4 the person stays and person_waits goes up.  Otherwise h = h', and if h
         equals the waypoint in both coordinates, waypoint j + 1 is drawn (from the new h), DW rebuilt in this same step and
         arrivals goes up.
      3. Terms.  d = float32 Euclidean d(p, h); (dot, cross) = h - p in the heading's frame (dot = dx * c + dy * s,
         cross = c * dy - s * dx); facing = dot > 0 and |cross| <= dot, the camera's 90 degree field of view; sees = facing and the
         graph's visible(p, h); following = 1.0 <= d <= 2.0 and sees; found is sticky, set by the first step that is following.
      4. reward = ((-0.01 + (d_prev - d) * [found was 0 before this step]) + 2.5 * [this step set found]) + 0.1 * following, in
         float32 in this order; d_prev = d after every step.
      5. The step count goes up; the episode ends when it reaches habitat.environment.max_episode_steps, and only then.  On done the
         next episode's world, person, waypoint 0 and field are generated, its first observation is what the step returns and
         not_done = 0.
      After every step d(p, h) >= 0.4.
    Measures.  has_found_person; following_rate = following steps / episode steps (one float32 division); first_encounter_steps =
      the step count (from 1) of the step that set found, or the episode's step count if none did; collisions.
    Sensors, in observation-space order.  head_rgb (H, W, 3) uint8, optional; head_depth (H, W, 1) float32; person_sensor (2,)
      float32 = (dot, cross) while sees, else (0, 0); person_visible (1,) float32 = sees.  With person_always_visible both are given
      as if the person were seen on every step: person_sensor = (dot, cross) and person_visible = 1; the reward still uses sees.
      That mode makes the task solvable blind and is for the learning test.  head_depth is Nav2D-v0's depth with the person's
      cylinder as geometry (Nav2DObj-v0's ray-circle test); head_rgb is the same with the person in category 0's colour.  Nothing is
      drawn in rgb only.  Without head_rgb and head_depth nothing is rendered.
    Distance.  Euclidean d only: `distance="geodesic"` is refused, because the target moves every step and would need a field per
      step.  The fields are built on the device, so the class itself refuses a device that is no GPU.

    `step_into_obs` writes whichever of the four rows `obs` holds; `actions` are the (N, 2) float32 rows the policy stored (the env
    clamps).  The record's words beyond Nav2D-v0's are named in include/habitat_amd.h (HAB_NAV2D_SOCIAL_W_*): the start, the person,
    the waypoint and its index j, found, the following steps, the step that set found, arrivals, person_waits, person_lost, the sweeps
    of the last build, the builds inside steps of the episode (`rebuilds`), one zero and DW."""

    _name = "Nav2DSocial"
    _expert_method = None  # no teacher: see Nav2DVectorEnv.expert_actions
    _entries = ("hab_nav2d_social_step",)
    _follow_entry = None  # no shortest-path follower: see Nav2DVectorEnv.follower_actions
    _sensor_set = "social"
    _map_task, _frame_keys = NAV2D_MAP_TASK_SOCIAL, ("head_rgb", "head_depth")
    _state_bytes = "hab_nav2d_social_state_bytes"
    _action_dtype, _action_text = torch.float32, "float32 device tensor of shape (N, 2)"
    measure_names = NAV2D_SOCIAL_MEASURES
    num_actions = 1

    def __init__(self, num_envs: int, height: int, width: int, seed: int = 100, env_offset: int = 0, use_rgb: bool = False,
                 use_depth: bool = True, num_actions: int = 1, device="cuda", num_obstacles: int = 3, turn_angle: int = 1,
                 max_episode_steps: int = 500, max_turn_angle: int = 10, min_abs_lin_speed: float = 0.025, min_abs_ang_speed: int = 5,
                 allow_sliding: bool = True, person_speed: float = 0.125, person_always_visible: bool = False,
                 distance: str = "euclidean", top_down_map=None):
        if nav2d_distance(distance, "Nav2DSocial") == "geodesic":
            raise _lib.HabError("Nav2DSocial: distance 'geodesic' is refused: the target moves every step, so it would need a field "
                                "per step; the task has the Euclidean distance only")
        _, self.max_turn_steps, self.stop_turn_steps = nav2d_vel_parameters(turn_angle, max_turn_angle, min_abs_lin_speed,
                                                                            min_abs_ang_speed, "Nav2DSocial")
        if not isinstance(allow_sliding, (bool, np.bool_)):
            raise _lib.HabError(f"Nav2DSocial: allow_sliding {allow_sliding!r} must be true or false")
        if not isinstance(person_always_visible, (bool, np.bool_)):
            raise _lib.HabError(f"Nav2DSocial: person_always_visible {person_always_visible!r} must be true or false")
        if (isinstance(person_speed, bool) or not isinstance(person_speed, (int, float, np.integer, np.floating))
                or not 0.0 < float(np.float32(person_speed)) <= 0.25):
            raise _lib.HabError(f"Nav2DSocial: person_speed {person_speed!r} must be a length in (0, 0.25] metres")
        if num_actions != 1:
            raise _lib.HabError(f"Nav2DSocial: the task has the one action velocity_control, got {num_actions} actions")
        if (use_rgb or use_depth) and (int(height) <= 0 or int(width) <= 0):
            raise _lib.HabError(f"Nav2DSocial: the image size {height} x {width} must be positive")
        self.max_turn_angle, self.min_abs_ang_speed = int(max_turn_angle), int(min_abs_ang_speed)
        self.min_abs_lin_speed, self.allow_sliding = float(min_abs_lin_speed), bool(allow_sliding)
        self.person_speed, self.person_always_visible = float(person_speed), bool(person_always_visible)
        try:
            super().__init__(num_envs, height, width, seed=seed, env_offset=env_offset, use_rgb=use_rgb, use_depth=use_depth, device=device,
                             num_obstacles=num_obstacles, turn_angle=turn_angle, max_episode_steps=max_episode_steps,
                             top_down_map=top_down_map)
        except _lib.HabError as err:
            # Nav2D-v0's own parameter refusals come first and stand; the one that is left where the spaces exist is the device's
            if torch.device(device).type != "cuda" and hasattr(self, "observation_spaces"):
                raise _lib.HabError("Nav2DSocial: the person's fields are built on the GPU; no GPU device given") from err
            raise
        self.task = "nav2dsocial"
        self.action_spaces = [spaces.Box(-1.0, 1.0, (2,), np.float32) for _ in range(num_envs)]
        self.orig_action_spaces = self.action_spaces
        self._actions_host = np.zeros((num_envs, 2), dtype=np.float32)

    def _actions_shaped(self, actions) -> bool:
        return tuple(actions.shape) == (self.num_envs, 2)

    def _sensor_rows(self, obs):
        return tuple(ptr(obs.get(k)) for k in NAV2D_SOCIAL_SENSORS)

    def _task_parameters(self):
        return (self.max_turn_steps, self.stop_turn_steps, self.min_abs_lin_speed, int(self.allow_sliding), self.person_speed,
                int(self.person_always_visible))

    def _own_obs(self):
        o = {}
        if self.use_rgb:
            o["head_rgb"] = self._rgb
        if self.use_depth:
            o["head_depth"] = self._depth
        o.update(self._obj)
        return o

    def _host_obs(self) -> List[Dict[str, np.ndarray]]:
        host = {k: v.cpu().numpy() for k, v in self._own_obs().items()}
        return [{k: v[i] for k, v in host.items()} for i in range(self.num_envs)]

    def async_step_at(self, index_env: int, action) -> None:
        if isinstance(action, dict):
            action = action["action"]
        try:
            a = np.asarray(action, dtype=np.float32)
        except (TypeError, ValueError):
            a = None
        if a is None or a.shape != (2,):
            raise _lib.HabError(f"Nav2DSocial: env {index_env}: action {action!r} is not a length-2 array (a_lin, a_ang)")
        SyntheticVectorEnv.async_step_at(self, index_env, action)
        self._actions_host[int(index_env)] = a

    def step_infos_host(self, ids) -> List[dict]:
        """The scalar infos of the last step of envs `ids`: this task's four measures where that step ended an episode, else {}."""
        return [dict(zip(NAV2D_SOCIAL_MEASURES, info.values())) if info else {} for info in super().step_infos_host(ids)]

    def reset_into(self, rgb, depth, goal):
        raise _lib.HabError("Nav2DSocial: the task has no pointgoal sensor; use reset_into_obs with the task's sensor rows")

    def step_into(self, rgb, depth, goal, reward, not_done, actions=None, mask=None):
        raise _lib.HabError("Nav2DSocial: the task has no pointgoal sensor; use step_into_obs with the task's sensor rows")


NAV2D_EXPLORE_MEASURES = ("coverage", "area_seen", "collisions", "num_steps")
NAV2D_EXPLORE_SENSORS = ("rgb", "depth", "gps", "compass")
NAV2D_EXPLORE_MIN_RESOLUTION, NAV2D_EXPLORE_MAX_RESOLUTION = 16, 512  # HAB_NAV2D_EXPLORE_MIN_RESOLUTION, _MAX_RESOLUTION


def nav2d_explore_parameters(coverage_resolution, visibility_dist, coverage_reward, who: str = "Nav2DExplore"):
    """Checks the three `habitat.synthetic` keys of Nav2DExplore-v0 and returns (G, visibility_dist, rc): the layer's resolution, the
    visibility as the float32 the kernel is given, and the reward of one cell, coverage_reward * cell ** 2 computed in float64 from
    the float32 cell size 8 / G and rounded once to float32."""
    number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
    G = coverage_resolution
    if not whole(G) or not NAV2D_EXPLORE_MIN_RESOLUTION <= G <= NAV2D_EXPLORE_MAX_RESOLUTION:
        raise _lib.HabError(f"{who}: coverage_resolution {G!r} must be a whole number in {NAV2D_EXPLORE_MIN_RESOLUTION}.."
                            f"{NAV2D_EXPLORE_MAX_RESOLUTION}")
    with np.errstate(over="ignore"):
        if not number(visibility_dist) or not np.isfinite(np.float32(visibility_dist)) or not float(np.float32(visibility_dist)) > 0.0:
            raise _lib.HabError(f"{who}: visibility_dist {visibility_dist!r} must be a positive finite length in metres")
        if not number(coverage_reward) or not np.isfinite(np.float32(coverage_reward)) or not float(coverage_reward) >= 0.0:
            raise _lib.HabError(f"{who}: coverage_reward {coverage_reward!r} must be a finite reward per square metre, >= 0")
    cell = np.float32(8.0) / np.float32(G)
    return int(G), float(np.float32(visibility_dist)), float(np.float32(float(coverage_reward) * float(cell) ** 2))


class Nav2DExploreVectorEnv(Nav2DVectorEnv):
    """Nav2DExplore-v0: area coverage in Nav2D-v0's world.  The agent is told no goal at all; the reward of a step is the area it saw
    for the first time in the episode, a dense reward that is no potential and never telescopes; and a recurrent policy's memory is the
    only record of where it has been.  The seen-area layer is kept on the device: it is the fog of war of the top-down map, made the
    task.  Read through `depth` (and optionally `rgb`), `gps` and `compass` by PointNavResNetPolicy, without `objectgoal`.  A
    measurement source, not a simulator.  tests/nav2d_explore_reference.py restates the task in numpy; `nav2d_explore_step_kernel` and
    the markerless form of `nav2d_render_kernel` (csrc/nav2d.hip) match it bit for bit on every output -- no angle function runs on the
    device, every float32 operation is one rounding in the written order, and the count of new cells is an integer sum.

    World, physics and controls.  Everything is Nav2D-v0's (see Nav2DVectorEnv): the arena, K <= 8 rectangles, the start, the heading
      table, the box free test, the 0.25 m forward step, turns of turn_angle, the collision count and streams 16-20.  There is no
      goal: the record's (gx, gy) are 0.  The action space is Discrete(4) in habitat's order; any other action count is refused.  The
      geodesic distance mode is refused by name, because there is no target.
    Coverage layer.  One uint8 layer per env of shape (G, G), G = habitat.synthetic.coverage_resolution, a whole number in 16..512
      (default 64), in the top-down map's cell geometry: cell = fl(8 / fl(G)), cell (r, c) has the centre x = (c + 0.5) * cell,
      y = (G - 1 - r + 0.5) * cell, row 0 on top.  A cell becomes seen by exactly the fog of war's rule (see Nav2DVectorEnv,
      Top-down map) with vis = habitat.synthetic.visibility_dist, a positive finite float32 (default 3.0): the centre is not strictly
      inside a raw rectangle, d2 = dx * dx + dy * dy <= vis * vis, it lies in the 90 degree wedge (dot > 0 and |cross| <= dot) or
      d2 <= 0.25 * 0.25, and the segment from the agent to the centre meets no open raw rectangle.
    Beginning of an episode.  1. The layer is cleared.  2. free_cells = the number of unoccupied cell centres.  3. The first reveal is
      done from the start pose; it earns nothing.  4. seen_cells = the count after that reveal.  5. The start pose (sx, sy, h0) is
      recorded for gps and compass.
    One step, in this order.  1. Nav2D-v0's discrete move; STOP moves nothing.  2. The reveal from the new pose; new = the number of
      cells this step turned from 0 to 1.  3. reward = fl(-0.01f + fl(rc * (float)new)), where the host computes rc in float64 as
      coverage_reward * cell ** 2 and rounds it once to float32; habitat.synthetic.coverage_reward is finite and >= 0, given per
      square metre (default 0.1).  4. The step count goes up; the episode ends on STOP or at habitat.environment.max_episode_steps;
      neither end carries a bonus.  5. On an end the measures are added into the sums, the next episode begins as above and
      not_done = 0; the observations then describe the new episode.
    Measures, in this order.  coverage = fl((float)seen_cells / (float)free_cells); area_seen = fl(fl(cell * cell) *
      (float)seen_cells); collisions; num_steps.
    Sensors.  rgb (H, W, 3) uint8, optional; depth (H, W, 1) float32; gps (2,) and compass (1,) float32, Nav2DObj-v0's expressions
      and its host compass table.  The images are Nav2D-v0's geometry with nothing drawn beyond it: there is no goal cylinder.
      Nothing is rendered when neither image is asked for.

    `coverage()` returns the layers, uint8 (N, G, G), the env's own device tensor.  `step_into_obs` writes whichever of the four rows
    `obs` holds; `actions` is int64 (N,) / (N, 1) as for Nav2D-v0.  The record's words beyond Nav2D-v0's are named in
    include/habitat_amd.h (HAB_NAV2D_EXPLORE_W_*): start x, start y, start heading, free_cells, seen_cells, and last_new, the `new`
    of the last step (0 after a reset).  The task has no follower, no teacher and no oracle.  With the `top_down_map` keyword the map
    shows no marker, and its fog of war at the same resolution and visibility equals the coverage layer."""

    _name = "Nav2DExplore"
    _expert_method = None  # no teacher: see Nav2DVectorEnv.expert_actions
    _entries = ("hab_nav2d_explore_step",)
    _follow_entry = None  # no shortest-path follower: see Nav2DVectorEnv.follower_actions
    _sensor_set = "explore"
    _map_task = NAV2D_MAP_TASK_EXPLORE
    _state_bytes = "hab_nav2d_explore_state_bytes"
    measure_names = NAV2D_EXPLORE_MEASURES

    def __init__(self, num_envs: int, height: int, width: int, seed: int = 100, env_offset: int = 0, use_rgb: bool = False,
                 use_depth: bool = True, num_actions: int = 4, device="cuda", num_obstacles: int = 3, turn_angle: int = 10,
                 max_episode_steps: int = 500, coverage_resolution: int = 64, visibility_dist: float = 3.0,
                 coverage_reward: float = 0.1, distance: str = "euclidean", top_down_map=None):
        if nav2d_distance(distance, "Nav2DExplore") == "geodesic":
            raise _lib.HabError("Nav2DExplore: distance 'geodesic' is refused: the task has no target to take a distance to")
        self.coverage_resolution, self.visibility_dist, self._cell_reward = nav2d_explore_parameters(coverage_resolution, visibility_dist,
                                                                                                     coverage_reward)
        self.coverage_reward = float(coverage_reward)
        if num_actions != 4:
            raise _lib.HabError("Nav2DExplore: the action space is Discrete(4) (STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT), got "
                                f"{num_actions}")
        if (use_rgb or use_depth) and (int(height) <= 0 or int(width) <= 0):
            raise _lib.HabError(f"Nav2DExplore: the image size {height} x {width} must be positive")
        try:
            super().__init__(num_envs, height, width, seed=seed, env_offset=env_offset, use_rgb=use_rgb, use_depth=use_depth, device=device,
                             num_obstacles=num_obstacles, turn_angle=turn_angle, max_episode_steps=max_episode_steps,
                             top_down_map=top_down_map)
        except _lib.HabError as err:
            # Nav2D-v0's own parameter refusals come first and stand; the one that is left where the spaces exist is the device's
            if torch.device(device).type != "cuda" and hasattr(self, "observation_spaces"):
                raise _lib.HabError("Nav2DExplore: the coverage layer is kept on the GPU; no GPU device given") from err
            raise
        self.task = "nav2dexplore"
        G = self.coverage_resolution
        self._coverage = torch.zeros(num_envs, G, G, dtype=torch.uint8, device=self.device)
        self._compass_table = torch.from_numpy(nav2d_compass_table(self.turn_angle)).to(self.device)

    def coverage(self):
        """The coverage layers, uint8 (N, G, G): 1 where the cell has been seen in the env's running episode.  The env's own device
        tensor, not a copy."""
        return self._coverage

    def _sensor_rows(self, obs):
        return (*(ptr(obs.get(k)) for k in NAV2D_EXPLORE_SENSORS), ptr(self._compass_table), ptr(self._coverage))

    def _task_parameters(self):
        return self.coverage_resolution, self.visibility_dist, self._cell_reward

    def step_infos_host(self, ids) -> List[dict]:
        """The scalar infos of the last step of envs `ids`: this task's four measures where that step ended an episode, else {}."""
        return [dict(zip(NAV2D_EXPLORE_MEASURES, info.values())) if info else {} for info in super().step_infos_host(ids)]

    def reset_into(self, rgb, depth, goal):
        raise _lib.HabError("Nav2DExplore: the task has no pointgoal sensor; use reset_into_obs with the task's sensor rows")

    def step_into(self, rgb, depth, goal, reward, not_done, actions=None, mask=None):
        raise _lib.HabError("Nav2DExplore: the task has no pointgoal sensor; use step_into_obs with the task's sensor rows")


NAV2D_IMAGENAV_SENSORS = ("rgb", "depth", "goal_rgb", "gps", "compass")
NAV2D_FOLLOWER_STOP_DISTANCE = 0.2  # below this D_PREV the shortest-path follower stops (see Nav2DVectorEnv.follower_actions)


def nav2d_imagenav_success_distance(success_distance, distance: str, who: str = "Nav2DImageNav") -> float:
    """Checks `habitat.synthetic.success_distance` of Nav2DImageNav-v0 and returns it as the float32 the kernel is given.  In the
    geodesic mode a value below the follower's stop distance is refused: the follower would stop outside the success radius."""
    number = isinstance(success_distance, (int, float, np.integer, np.floating)) and not isinstance(success_distance, bool)
    with np.errstate(over="ignore"):
        if not number or not np.isfinite(np.float32(success_distance)) or not float(np.float32(success_distance)) > 0.0:
            raise _lib.HabError(f"{who}: success_distance {success_distance!r} must be a positive finite length in metres")
    if distance == "geodesic" and np.float32(success_distance) < np.float32(NAV2D_FOLLOWER_STOP_DISTANCE):
        raise _lib.HabError(f"{who}: success_distance {success_distance!r} is below {NAV2D_FOLLOWER_STOP_DISTANCE}, the distance at "
                            "which the shortest-path follower of the geodesic mode stops: its episodes would end outside the radius")
    return float(np.float32(success_distance))


class Nav2DImageNavVectorEnv(Nav2DVectorEnv):
    """Nav2DImageNav-v0: Nav2D-v0 with the goal given only as an image.  The place to reach is told by `goal_rgb`, the picture the
    task's camera takes from there, and in no other way: there is no pointgoal sensor.  It is the early-fusion form of ImageNav:
    PointNavResNetPolicy stacks `rgb` (3), `depth` (1) and `goal_rgb` (3) along the channels, 7 of its encoder's 8, and one encoder
    reads both views.  The sensor is deliberately not called `imagegoal`: that name (and `instance_imagegoal`) is refused by both
    policies, because the reference builds a second encoder for it.  A measurement source, not a simulator.
    tests/nav2d_imagenav_reference.py restates the task in numpy; `nav2d_imagenav_step_kernel` and the IMAGENAV form of
    `nav2d_render_kernel` (csrc/nav2d.hip) match it bit for bit on every output.

    World, physics and controls.  Everything is Nav2D-v0's, bit for bit (see Nav2DVectorEnv): the arena, K <= 8 rectangles, the start,
      the goal position (gx, gy), the heading table, the box free test, the moves, the collision count, the step limit, Discrete(4)
      and streams 16-20.  Any other action count is refused.
    Goal view.  When an episode begins, gh = mix32(stream_key(seed, 25, env, episode) ^ 0) % num_headings, the expression the start
      heading uses on stream 19.  `goal_rgb` is what the camera sees from (gx, gy) with heading gh: the same pinhole, tables, shading
      and truncation as the agent's view, without any marker.  It is a pure function of the record, constant within an episode, and
      drawn again at every step by the same launch that draws the agent's view (view 1 of the IMAGENAV form); the env keeps no image.
    Reward, success, measures.  Nav2D-v0's: reward = (-0.01 + (d_prev - d)) + 2.5 * success; success = STOP with
      d < success_distance; measures success, spl, distance_to_goal, collisions.  habitat.synthetic.success_distance is a positive
      finite float32, default 1.0 (the distance the object task uses); with 0.2 every reward, not-done byte and measure is bitwise
      Nav2D-v0's under the same seed and actions.  Both distance modes exist (`distance`, habitat.synthetic.distance_to_goal); the
      geodesic one uses Nav2D-v0's field records, hab_nav2d_geo_build with this record's stride.
    Sensors, in this order.  rgb (H, W, 3) uint8, required: use_rgb=False is refused; depth (H, W, 1) float32, optional; goal_rgb
      (H, W, 3) uint8; gps (2,) and compass (1,) float32, Nav2DObj-v0's expressions and host compass table, relative to the start
      pose.  The agent's rgb carries NO goal cylinder: its pixels are the markerless geometry of Nav2DExplore-v0, not Nav2D-v0's.
    Follower, teacher, map.  In the geodesic mode `follower_actions` is Nav2D-v0's follower on this record and `expert_actions` is
      that follower; in the Euclidean mode both refuse as Nav2D-v0's do.  The follower stops where D_PREV < 0.2, which is inside
      every success distance >= 0.2; a success_distance below 0.2 is refused in the geodesic mode.  The top-down map and the frames
      use Nav2D-v0's map task code (the goal disc at (gx, gy)); the goal image is not part of a frame.

    The record's words beyond Nav2D-v0's are named in include/habitat_amd.h (HAB_NAV2D_IMAGENAV_W_*): gh, then the start pose
    (sx, sy, h0).  `step_into_obs` writes whichever of the five rows `obs` holds.  A non-GPU device is refused by name, as for every
    Nav2D task; on a GPU device the VectorEnv API (the host path: `reset`, `step`, `async_step_at` / `wait_step_at`) works as
    Nav2D-v0's does, with `goal_rgb` among the host observations."""

    _name = "Nav2DImageNav"
    _entries = ("hab_nav2d_imagenav_step", "hab_nav2d_imagenav_step_geo")
    _sensor_set = "imagenav"
    _state_bytes = "hab_nav2d_imagenav_state_bytes"

    def __init__(self, num_envs: int, height: int, width: int, seed: int = 100, env_offset: int = 0, use_rgb: bool = True,
                 use_depth: bool = True, num_actions: int = 4, device="cuda", num_obstacles: int = 3, turn_angle: int = 10,
                 max_episode_steps: int = 500, success_distance: float = 1.0, distance: str = "euclidean", top_down_map=None):
        if not use_rgb:
            raise _lib.HabError("Nav2DImageNav: the rgb sensor is required: the goal image is given in its size and the policy "
                                "compares the two views")
        if num_actions != 4:
            raise _lib.HabError("Nav2DImageNav: the action space is Discrete(4) (STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT), got "
                                f"{num_actions}")
        if int(height) <= 0 or int(width) <= 0:
            raise _lib.HabError(f"Nav2DImageNav: the image size {height} x {width} must be positive")
        self.success_distance = nav2d_imagenav_success_distance(success_distance, nav2d_distance(distance, "Nav2DImageNav"))
        try:
            super().__init__(num_envs, height, width, seed=seed, env_offset=env_offset, use_rgb=use_rgb, use_depth=use_depth, device=device,
                             num_obstacles=num_obstacles, turn_angle=turn_angle, max_episode_steps=max_episode_steps, distance=distance,
                             top_down_map=top_down_map)
        except _lib.HabError as err:
            # Nav2D-v0's own parameter refusals come first and stand; the one that is left where the spaces exist is the device's
            if torch.device(device).type != "cuda" and hasattr(self, "observation_spaces"):
                raise _lib.HabError("Nav2DImageNav: both views are rendered on the GPU; no GPU device given") from err
            raise
        self.task = "nav2dimagenav"
        self._compass_table = torch.from_numpy(nav2d_compass_table(self.turn_angle)).to(self.device)

    def _sensor_rows(self, obs):
        return (*(ptr(obs.get(k)) for k in NAV2D_IMAGENAV_SENSORS), ptr(self._compass_table))

    def _task_parameters(self):
        return (self.success_distance,)

    def reset_into(self, rgb, depth, goal):
        raise _lib.HabError("Nav2DImageNav: the task has no pointgoal sensor; use reset_into_obs with the task's sensor rows")

    def step_into(self, rgb, depth, goal, reward, not_done, actions=None, mask=None):
        raise _lib.HabError("Nav2DImageNav: the task has no pointgoal sensor; use step_into_obs with the task's sensor rows")


class SyntheticVectorEnvFactory(VectorEnvFactory):
    """Default `_target_`: N synthetic PointNav envs sized from habitat.simulator.sensors.*; per-rank env ids are
    offset by rank * num_environments exactly like the reference offsets the seed (ppo_trainer.py:208-211).  A
    `habitat.task.type` starting with "nav2d" (any case) selects the Nav2D-v0 task, whose num_obstacles / turn_angle come from
    `habitat.synthetic` and whose episode limit from `habitat.environment.max_episode_steps`; one starting with "nav2dvel" selects
    Nav2DVel-v0, its velocity-controlled variant (Nav2DVelVectorEnv), with the further `habitat.synthetic` keys named there; one
    starting with "nav2dobj" selects Nav2DObj-v0 (Nav2DObjVectorEnv: objects, a target category, the ObjectNav sensor set), which
    reads num_objects / num_categories too and takes its image size from the rgb, else the depth, else the semantic sensor.
    `habitat.synthetic.distance_to_goal` ("euclidean", the default, or "geodesic") is the distance mode of every Nav2D task.
    A type starting with "nav2drearr" selects Nav2DRearr-v0 (Nav2DRearrVectorEnv: pick and place, the rearrangement sensor set), which
    reads start_holding too and takes its image size from the head_rgb, else the head_depth sensor; in the geodesic mode both terms
    of its potential are shortest paths.  A type
    starting with "nav2drearrvel" -- tested before "nav2drearr", which keeps its meaning for everything else -- selects
    Nav2DRearrVel-v0 (Nav2DRearrVelVectorEnv: that task under velocity and grip control), which reads Nav2DVel-v0's keys and
    start_holding and takes its image size like Nav2DRearr-v0.  A type starting with "nav2dsocial" -- tested before "nav2d" -- selects
    Nav2DSocial-v0 (Nav2DSocialVectorEnv: find and follow a walking person), which reads Nav2DVel-v0's keys, person_speed and
    person_always_visible, takes its image size like Nav2DRearr-v0 and has the Euclidean distance mode only.  A type starting with
    "nav2dexplore" -- tested before "nav2d" too -- selects Nav2DExplore-v0 (Nav2DExploreVectorEnv: area coverage, no goal input), which
    reads coverage_resolution, visibility_dist and coverage_reward, takes its image size like Nav2D-v0 and has the Euclidean mode only.
    A type starting with "nav2dimagenav" -- tested before "nav2d" as well -- selects Nav2DImageNav-v0 (Nav2DImageNavVectorEnv: the goal
    given only as the image `goal_rgb`), which reads success_distance, takes its image size from the rgb sensor, which it requires, and
    has both distance modes.
    `habitat.task.measurements.top_down_map`, where that key is present, becomes the `top_down_map` keyword of any Nav2D task with
    whichever of map_resolution, visibility_dist, draw_fog and fov it holds (see Nav2DVectorEnv, Top-down map)."""

    def __init__(self, use_rgb: bool = True, use_depth: bool = True):
        self.use_rgb, self.use_depth = use_rgb, use_depth

    def construct_envs(self, config, workers_ignore_signals: bool = False, enforce_scenes_greater_eq_environments: bool = False,
                       is_first_rank: bool = True, device="cuda", env_offset: int = 0):
        hb, hab = config.habitat_baselines, config.habitat
        sens = hab.simulator.sensors
        use_rgb = self.use_rgb and "rgb" in sens
        use_depth = self.use_depth and "depth" in sens
        task_type = str(hab.task.type).lower()
        if task_type.startswith("nav2d"):
            ref = sens["rgb"] if use_rgb else (sens["depth"] if use_depth else dict(height=0, width=0))
            syn = getattr(hab, "synthetic", {})
            distance = getattr(syn, "distance_to_goal", "euclidean")
            kw = dict(seed=int(hab.seed), env_offset=env_offset, use_rgb=use_rgb, use_depth=use_depth, num_actions=len(hab.task.actions),
                      device=device, num_obstacles=getattr(syn, "num_obstacles", 3), turn_angle=getattr(syn, "turn_angle", 10),
                      max_episode_steps=getattr(hab.environment, "max_episode_steps", 500), distance=distance)
            tdm = getattr(getattr(hab.task, "measurements", {}), "top_down_map", None)
            if tdm is not None:  # the measure: any of its keys may be missing (see nav2d_map_parameters)
                kw.update(top_down_map={k: getattr(tdm, k) for k in NAV2D_MAP_DEFAULTS if getattr(tdm, k, None) is not None})
            make = Nav2DVectorEnv
            if task_type.startswith("nav2dimagenav"):
                make = Nav2DImageNavVectorEnv
                ref = sens["rgb"] if use_rgb else dict(height=0, width=0)  # the goal image has the rgb sensor's size
                kw.update(success_distance=getattr(syn, "success_distance", 1.0))
            elif task_type.startswith("nav2dexplore"):
                make = Nav2DExploreVectorEnv
                kw.update(coverage_resolution=getattr(syn, "coverage_resolution", 64), visibility_dist=getattr(syn, "visibility_dist", 3.0),
                          coverage_reward=getattr(syn, "coverage_reward", 0.1))
            elif task_type.startswith("nav2dsocial"):
                use_rgb, use_depth = self.use_rgb and "head_rgb" in sens, self.use_depth and "head_depth" in sens
                ref = sens["head_rgb"] if use_rgb else (sens["head_depth"] if use_depth else dict(height=0, width=0))
                make = Nav2DSocialVectorEnv
                kw.update(use_rgb=use_rgb, use_depth=use_depth, turn_angle=getattr(syn, "turn_angle", 1),
                          max_turn_angle=getattr(syn, "max_turn_angle", 10), min_abs_lin_speed=getattr(syn, "min_abs_lin_speed", 0.025),
                          min_abs_ang_speed=getattr(syn, "min_abs_ang_speed", 5), allow_sliding=getattr(syn, "allow_sliding", True),
                          person_speed=getattr(syn, "person_speed", 0.125),
                          person_always_visible=getattr(syn, "person_always_visible", False))
            elif task_type.startswith("nav2drearr"):
                use_rgb, use_depth = self.use_rgb and "head_rgb" in sens, self.use_depth and "head_depth" in sens
                ref = sens["head_rgb"] if use_rgb else (sens["head_depth"] if use_depth else dict(height=0, width=0))
                make = Nav2DRearrVectorEnv
                kw.update(use_rgb=use_rgb, use_depth=use_depth, start_holding=getattr(syn, "start_holding", False))
                if task_type.startswith("nav2drearrvel"):
                    make = Nav2DRearrVelVectorEnv
                    kw.update(turn_angle=getattr(syn, "turn_angle", 1), max_turn_angle=getattr(syn, "max_turn_angle", 10),
                              min_abs_lin_speed=getattr(syn, "min_abs_lin_speed", 0.025),
                              min_abs_ang_speed=getattr(syn, "min_abs_ang_speed", 5), allow_sliding=getattr(syn, "allow_sliding", True))
            elif task_type.startswith("nav2dobj"):
                if not (use_rgb or use_depth):
                    if "semantic" not in sens:
                        raise _lib.HabError("Nav2DObj: no rgb, depth or semantic sensor gives the image size")
                    ref = sens["semantic"]
                make = Nav2DObjVectorEnv
                kw.update(num_objects=getattr(syn, "num_objects", 3), num_categories=getattr(syn, "num_categories", 4))
            elif task_type.startswith("nav2dvel"):
                make = Nav2DVelVectorEnv
                kw.update(turn_angle=getattr(syn, "turn_angle", 1), max_turn_angle=getattr(syn, "max_turn_angle", 10),
                          min_abs_lin_speed=getattr(syn, "min_abs_lin_speed", 0.025),
                          min_abs_ang_speed=getattr(syn, "min_abs_ang_speed", 5), allow_sliding=getattr(syn, "allow_sliding", True))
            return make(int(hb.num_environments), int(ref["height"]), int(ref["width"]), **kw)
        ref = sens["rgb"] if use_rgb else sens["depth"]
        task = "objectnav" if str(hab.task.type).lower().startswith("objectnav") else "pointnav"
        return SyntheticVectorEnv(int(hb.num_environments), int(ref.height), int(ref.width), seed=int(hab.seed),
                                  env_offset=env_offset, use_rgb=use_rgb, use_depth=use_depth,
                                  num_actions=len(hab.task.actions), device=device, task=task)


class ProcessVectorEnvFactory(VectorEnvFactory):
    """`_target_: habitat_amd.common.env_factory.ProcessVectorEnvFactory`: one worker PROCESS per environment behind the
    reference's VectorEnv API (core/vector_env.py), observations through the shared-memory plane.  The worker env is
    `core.host_env.HostSyntheticNavEnv` unless `make_env_fn` names another constructor ('pkg.mod.fn'); with habitat-sim the
    reference's `make_gym_from_config` goes here (habitat_baselines/common/habitat_env_factory.py:80-119)."""

    def __init__(self, make_env_fn: Optional[str] = None, shared_obs: bool = True, start_method: str = "forkserver", work_us: int = 0):
        self.make_env_fn, self.shared_obs, self.start_method, self.work_us = make_env_fn, shared_obs, start_method, work_us

    def construct_envs(self, config, workers_ignore_signals: bool = False, enforce_scenes_greater_eq_environments: bool = False,
                       is_first_rank: bool = True, env_offset: int = 0):
        from habitat_amd.core.host_env import make_host_env
        from habitat_amd.core.vector_env import VectorEnv
        hb, hab = config.habitat_baselines, config.habitat
        sens = hab.simulator.sensors
        use_rgb, use_depth = "rgb" in sens, "depth" in sens
        ref = sens["rgb"] if use_rgb else sens["depth"]
        fn = make_host_env
        if self.make_env_fn:
            mod, _, name = self.make_env_fn.rpartition(".")
            fn = getattr(importlib.import_module(mod), name)
        n = int(hb.num_environments)
        args = [(int(hab.seed) + env_offset + i, int(ref.height), int(ref.width), use_rgb, use_depth, len(hab.task.actions),
                 int(hab.environment.max_episode_steps), self.work_us) for i in range(n)]
        return VectorEnv(fn, args, auto_reset_done=True, multiprocessing_start_method=self.start_method,
                         workers_ignore_signals=workers_ignore_signals, shared_obs=self.shared_obs)
