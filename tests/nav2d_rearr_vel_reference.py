"""Plain-numpy restatement of the Nav2DRearrVel-v0 task (habitat_amd/common/env_factory.py: Nav2DRearrVelVectorEnv), shared by
tests/test_nav2d_rearr_vel_host.py and tests/test_gpu_nav2d_rearr_vel.py.  This file is the specification: `nav2d_rearr_vel_step_kernel`
and the rearrangement form of `nav2d_render_kernel` (habitat-lab_amd/csrc/nav2d.hip) reproduce every output bit for bit.  Every written
operation is one float32 rounding, no fused multiply-add.

Nav2DRearrVel-v0 is Nav2DRearr-v0 (tests/nav2d_rearr_reference.py: world, places, object, holding flag, potential, measures, sensors,
render, state record; imported, not restated) under Nav2DVel-v0's velocity control (tests/nav2d_vel_reference.py: the clamp, the step
length and the turn rule; imported, not restated) plus one grip component.

One step with the action a = (a_lin, a_ang, a_grip):
  1. c = min(max(a, -1), 1) per component, 0 for a non-finite one;
  2. l = (c_lin + 1) * 0.125; dh = (int) rint(c_ang * M); stop = l < min_abs_lin_speed and |dh| < S;
  3. unless stop: h = (h + dh) mod nh; target (px + l * c, py + l * s) with (c, s) = dirs[h].  Free (Nav2DRearr-v0's test: the box test
     and, unless holding, not dist(., o) < 0.4): taken, path += l.  Blocked: one collision, and with sliding (nx, py) if free
     (path += |nx - px|), else (px, ny) if free (path += |ny - py|), else stay;
  4. grip, on every step, with the new position and the new heading's (c, s): c_grip > 0 and holding = 0 is a PICK attempt (needs
     dist(p, o) < 1.0 and (ox - px) * c + (oy - py) * s > 0; success: holding = held = 1, picks += 1, first_pick = picks was 0; refusal:
     invalid += 1); c_grip < 0 and holding = 1 a PLACE attempt (needs q = (px + 0.5 * c, py + 0.5 * s) in [0.5, 7.5]^2 and not strictly
     inside a rectangle grown by 0.3; success: o = q, holding = 0; refusal: invalid += 1); every other combination changes and counts
     nothing; while holding, o = p;
  5. reward = ((-0.01 + (Phi_prev - Phi)) + 1.0 * first_pick) + 2.5 * success, success = stop and holding = 0 and b < 0.5;
     done = stop or steps >= max_episode_steps; measures, sums and the next world as Nav2DRearr-v0."""
from __future__ import annotations

import math

import numpy as np

import nav2d_rearr_reference as A
import nav2d_reference as R
import nav2d_vel_reference as V
from nav2d_obj_reference import OBJ_HI, OBJ_LO
from nav2d_reference import F, HI, LO, dist
from nav2d_rearr_reference import MEASURES, SENSORS, frame, in_grown_rect  # noqa: F401

NUM_COMPONENTS = 3
# every branch of the task: what a test asserts the scripted runs reach
EVENTS = ("forward_free", "forward_free_holding", "blocked_object", "blocked_rect", "blocked_wall", "slide_x", "slide_y", "slide_refused",
          "turn_left", "turn_right", "turn_max", "pick_bonus", "pick_again", "pick_far", "pick_behind", "place_ok", "place_outside_box",
          "place_in_rect", "noop_zero", "noop_pick_holding", "noop_place_empty", "successes", "stop_holding", "stop_too_far", "timeouts")
# what the scripts also reach and the tests also read
OTHER_COUNTERS = ("stops", "clamped", "nonfinite", "ties", "release_and_stop", "object_visible", "marker_visible")


def check_parameters(turn_angle, max_turn_angle, min_abs_lin_speed, min_abs_ang_speed, allow_sliding, start_holding):
    """-> (nh, M, S); ValueError naming the rule otherwise."""
    out = V.check_parameters(turn_angle, max_turn_angle, min_abs_lin_speed, min_abs_ang_speed)
    if not isinstance(allow_sliding, (bool, np.bool_)):
        raise ValueError(f"allow_sliding {allow_sliding!r} must be true or false")
    A.check_parameters(start_holding)
    return out


def decode(action, M):
    """Steps 1-2: (l, dh, c_grip, tie), the first two by Nav2DVel-v0's `decode`."""
    a = np.asarray(action, dtype=np.float32).reshape(NUM_COMPONENTS)
    _, _, l, dh, tie = V.decode(a[:2], M)
    return l, dh, V.clamp(a[2]), tie


class Nav2DRearrVelEnv(A.Nav2DRearrEnv):
    """One env, the interface of nav2d_rearr_reference.Nav2DRearrEnv: `step((a_lin, a_ang, a_grip))` -> (obs, reward, done, info)."""

    def __init__(self, seed, env, turn_angle=1, max_turn_angle=10, min_abs_lin_speed=0.025, min_abs_ang_speed=5, allow_sliding=True,
                 start_holding=False, **kw):
        _, self.M, self.S = check_parameters(turn_angle, max_turn_angle, min_abs_lin_speed, min_abs_ang_speed, allow_sliding, start_holding)
        super().__init__(seed, env, turn_angle=turn_angle, start_holding=start_holding, **kw)
        self.min_lin, self.allow_sliding = F(min_abs_lin_speed), bool(allow_sliding)
        self.counters.update({k: 0 for k in EVENTS + OTHER_COUNTERS})
        self.last_dh = 0

    def step(self, action):
        a = np.asarray(action, dtype=np.float32)
        if a.shape != (NUM_COMPONENTS,):
            raise ValueError(f"action {action!r} is not (a_lin, a_ang, a_grip)")
        w, cnt = self.world, self.counters
        l, dh, c_grip, tie = decode(a, self.M)
        cnt["clamped"] += int(any(np.isfinite(x) and abs(x) > 1 for x in a))
        cnt["nonfinite"] += int(not np.isfinite(a).all())
        cnt["ties"] += int(tie)
        self.last_dh = dh
        stop = bool(l < self.min_lin and abs(dh) < self.S)
        if not stop:
            self.h = (self.h + dh) % self.nh
            cnt["turn_left"] += int(dh > 0)
            cnt["turn_right"] += int(dh < 0)
            cnt["turn_max"] += int(abs(dh) == self.M)
            c, s = self.dirs[self.h]
            nx, ny = F(self.px + F(l * c)), F(self.py + F(l * s))   # multiply, then a separate add
            if self.is_free(nx, ny):
                self.px, self.py, self.path = nx, ny, F(self.path + l)
                cnt["forward_free_holding" if self.holding else "forward_free"] += 1
            else:
                self.collisions += 1
                inside = nx >= LO and nx <= HI and ny >= LO and ny <= HI
                cnt["blocked_wall" if not inside else ("blocked_rect" if not R.is_free(nx, ny, w.rects) else "blocked_object")] += 1
                if self.allow_sliding and self.is_free(nx, self.py):
                    self.path = F(self.path + F(abs(F(nx - self.px))))
                    self.px = nx
                    cnt["slide_x"] += 1
                elif self.allow_sliding and self.is_free(self.px, ny):
                    self.path = F(self.path + F(abs(F(ny - self.py))))
                    self.py = ny
                    cnt["slide_y"] += 1
                elif self.allow_sliding:
                    cnt["slide_refused"] += 1
        # the grip, with the new position and the new heading
        c, s = self.dirs[self.h]
        first_pick = False
        if c_grip > 0 and not self.holding:
            dx, dy = F(self.ox - self.px), F(self.oy - self.py)
            near = dist(self.px, self.py, self.ox, self.oy) < A.REACH
            ahead = F(F(dx * c) + F(dy * s)) > 0
            if near and ahead:
                first_pick = self.picks == 0
                self.holding = self.held = 1
                self.picks += 1
                cnt["pick_bonus" if first_pick else "pick_again"] += 1
            else:
                self.invalid += 1
                cnt["pick_far" if not near else "pick_behind"] += 1
        elif c_grip < 0 and self.holding:
            qx, qy = F(self.px + F(A.ARM * c)), F(self.py + F(A.ARM * s))
            inside = qx >= OBJ_LO and qx <= OBJ_HI and qy >= OBJ_LO and qy <= OBJ_HI
            if inside and not in_grown_rect(qx, qy, w.rects):
                self.ox, self.oy, self.holding = qx, qy, 0
                cnt["place_ok"] += 1
                cnt["release_and_stop"] += int(stop)
            else:
                self.invalid += 1
                cnt["place_outside_box" if not inside else "place_in_rect"] += 1
        else:
            cnt["noop_zero" if c_grip == 0 else ("noop_pick_holding" if c_grip > 0 else "noop_place_empty")] += 1
        if self.holding:
            self.ox, self.oy = self.px, self.py
        # from here on Nav2DRearr-v0's end of a step, `stop` in the place of a == STOP
        phi, b = self.potential()
        success = stop and not self.holding and b < A.SUCCESS_DIST
        if stop and not success:
            cnt["stop_holding" if self.holding else "stop_too_far"] += 1
        reward = F(F(F(R.SLACK + F(self.phi_prev - phi)) + (A.PICK_REWARD if first_pick else F(0.0))) + (R.SUCCESS_REWARD if success else F(0.0)))
        self.phi_prev = phi
        self.steps += 1
        done = stop or self.steps >= self.max_steps
        self.ended = int(done)
        cnt["stops"] += int(stop)
        info = {}
        if done:
            info = dict(success=float(success), did_pick_object=float(self.held), object_to_goal_distance=float(b),
                        collisions=float(self.collisions))
            self.last_measures = [F(info[k]) for k in MEASURES]
            self.last = dict(phi_start=self.phi_start, phi_end=phi, length=self.steps, success=bool(success), picks=self.picks,
                             invalid=self.invalid)
            for k in MEASURES:
                self.sums[k] = F(self.sums[k] + F(info[k]))
            cnt["episodes"] += 1
            cnt["successes"] += int(success)
            cnt["timeouts"] += int(not stop)
            self.episode += 1
            self._begin()
        return self.observe(), reward, done, info


# ---- scripted action sources -----------------------------------------------------------------------------------------------------
def _steer(v, max_turn_angle, keep):
    """(a_lin, a_ang) towards the (dot, cross) offset v: turn as far as one step allows, slowly while the offset is more than one
    step's turn away, else at the speed that brings it to the distance `keep`, never below a quarter of the full step."""
    rho, phi_deg = math.hypot(float(v[0]), float(v[1])), math.degrees(math.atan2(float(v[1]), float(v[0])))
    a_ang = min(max(phi_deg / max_turn_angle, -1.0), 1.0)
    a_lin = min(1.0, max(-0.5, (rho - keep) / 0.125 - 1.0)) if abs(phi_deg) <= max_turn_angle else -0.5
    return a_lin, a_ang


class SensorFollower:
    """Reads the three vector sensors only: drive to the object by obj_start_sensor with the grip closed, carry it to the goal by
    obj_goal_sensor until the goal is about an arm's length ahead, then release and stand still in one step."""

    def __init__(self, max_turn_angle):
        self.max_turn = max_turn_angle

    def __call__(self, obs, env=None):
        if obs["is_holding"][0] > 0:
            v = obs["obj_goal_sensor"]
            rho, phi_deg = math.hypot(float(v[0]), float(v[1])), math.degrees(math.atan2(float(v[1]), float(v[0])))
            if 0.1 < rho < 0.9 and abs(phi_deg) < 20.0:
                return (-1.0, 0.0, -1.0)
            return _steer(v, self.max_turn, 0.5) + (1.0,)
        return _steer(obs["obj_start_sensor"], self.max_turn, 0.5) + (1.0,)

    def episode_ended(self):
        pass


class RandomActions:
    """Each step either uniform in [-1.25, 1.25]^3 with a component in twenty replaced by nan, +inf or -inf, or three draws from
    Nav2DVel-v0's grid of multiples of 0.05 (where c_ang * M falls on exact halves and the grip on exact zeros)."""

    def __init__(self, rng):
        self.rng = rng

    def __call__(self, obs, env=None):
        if self.rng.randint(0, 2):
            return V.GRID[self.rng.randint(0, len(V.GRID), size=NUM_COMPONENTS)]
        a = self.rng.uniform(-1.25, 1.25, size=NUM_COMPONENTS).astype(np.float32)
        for i in range(NUM_COMPONENTS):
            if self.rng.randint(0, 20) == 0:
                a[i] = (np.nan, np.inf, -np.inf)[self.rng.randint(0, 3)]
        return a

    def episode_ended(self):
        pass


class GripEverywhere:
    """Never stops: drives at random, closing the grip while its hands are empty and opening it while they are full three steps in
    four, wherever it is; after a release it often drives on into the object."""

    def __init__(self, rng):
        self.rng = rng

    def __call__(self, obs, env=None):
        holding = obs["is_holding"][0] > 0
        u = self.rng.randint(0, 8)
        grip = (-1.0 if holding else 1.0) if u < 6 else (0.0, self.rng.uniform(0.1, 1.25) * (1.0 if holding else -1.0))[u - 6]
        return (self.rng.uniform(-0.5, 1.25), self.rng.uniform(-1.25, 1.25), grip)

    def episode_ended(self):
        pass


class WallHugger:
    """Full speed ahead with the grip closed until a move is blocked, then a release against whatever blocked it, a few full turns to
    the left, and on."""

    def __init__(self, rng):
        self.rng, self.queue, self.collisions = rng, [], 0

    def __call__(self, obs, env=None):
        if env.collisions != self.collisions:
            self.collisions = env.collisions
            self.queue = [(1.0, 0.0, -1.0)] + [(-0.5, 1.0, 0.0)] * int(self.rng.randint(1, 4))
        if self.queue:
            return self.queue.pop(0)
        return (1.0, 0.0, 1.0)

    def episode_ended(self):
        self.collisions, self.queue = 0, []


SCRIPTS = ("sensor", "random", "grip", "wall")


def make_script(kind, max_turn_angle, rng):
    if kind == "sensor":
        return SensorFollower(max_turn_angle)
    if kind == "random":
        return RandomActions(rng)
    if kind == "grip":
        return GripEverywhere(rng)
    if kind == "wall":
        return WallHugger(rng)
    raise ValueError(kind)


def rollout(kind, seed, num_envs, steps, turn_angle=1, max_turn_angle=10, rng_seed=0, **env_kw):
    """As nav2d_rearr_reference.rollout, with actions (steps, N, 3) float32 and dh (steps, N)."""
    envs = [Nav2DRearrVelEnv(seed, n, turn_angle=turn_angle, max_turn_angle=max_turn_angle, **env_kw) for n in range(num_envs)]
    rng = np.random.RandomState(rng_seed)
    scripts = [make_script(kind, max_turn_angle, rng) for _ in envs]
    obs = [[e.reset() for e in envs]]
    out = dict(actions=np.zeros((steps, num_envs, NUM_COMPONENTS), np.float32), rewards=np.zeros((steps, num_envs), np.float32),
               dones=np.zeros((steps, num_envs), bool), infos=[], sums=np.zeros((steps, len(MEASURES), num_envs), np.float32),
               dh=np.zeros((steps, num_envs), np.int64), states=[[e.state_words() for e in envs]])
    for t in range(steps):
        a = np.array([sc(o, e) for sc, o, e in zip(scripts, obs[-1], envs)], dtype=np.float32)
        res = [e.step(x) for e, x in zip(envs, a)]
        for sc, r in zip(scripts, res):
            if r[2]:
                sc.episode_ended()
        out["actions"][t] = a
        obs.append([r[0] for r in res])
        out["rewards"][t] = [r[1] for r in res]
        out["dones"][t] = [r[2] for r in res]
        out["infos"].append([r[3] for r in res])
        out["sums"][t] = [[e.sums[k] for e in envs] for k in MEASURES]
        out["dh"][t] = [e.last_dh for e in envs]
        out["states"].append([e.state_words() for e in envs])
    out["obs"] = obs
    out["counters"] = {k: sum(e.counters[k] for e in envs) for k in envs[0].counters}
    out["envs"] = envs
    return out


# The scripted runs tests/test_gpu_nav2d_rearr_vel.py holds the kernels to: every combination of K in {0, 3, 8}, the two parameter sets
# (turn_angle, max_turn_angle, min_abs_ang_speed), start_holding and allow_sliding in both values.  tests/test_nav2d_rearr_vel_host.py
# asserts that the union of the four scripts over these cases reaches every event in EVENTS on the restatement alone.
SCRIPT_ENVS, SCRIPT_STEPS, SCRIPT_MAX_EPISODE_STEPS = A.SCRIPT_ENVS, A.SCRIPT_STEPS, A.SCRIPT_MAX_EPISODE_STEPS
PARAMETER_SETS = [(1, 10, 5), (10, 30, 10)]
SCRIPT_CASES = [(K, p, sh, sl) for K in (0, 3, 8) for p in PARAMETER_SETS for sh in (False, True) for sl in (False, True)]


def case_id(case):
    K, (turn, max_turn, min_ang), sh, sl = case
    return f"K{K}-turn{turn}-{max_turn}-{min_ang}-hold{int(sh)}-slide{int(sl)}"


def script_seed(kind, case=None):
    return 1


def case_kw(case):
    """The env keywords of one case."""
    K, (turn, max_turn, min_ang), sh, sl = case
    return dict(turn_angle=turn, max_turn_angle=max_turn, min_abs_ang_speed=min_ang, num_obstacles=K, start_holding=sh, allow_sliding=sl)


def script_rollout(kind, case, H=0, W=0, **kw):
    return rollout(kind, script_seed(kind, case), SCRIPT_ENVS, SCRIPT_STEPS, max_episode_steps=SCRIPT_MAX_EPISODE_STEPS, H=H, W=W,
                   **case_kw(case), **kw)
