"""Plain-numpy restatement of the Nav2DVel-v0 task (habitat_amd/common/env_factory.py: Nav2DVelVectorEnv), shared by
tests/test_nav2d_vel_host.py and tests/test_gpu_nav2d_vel.py.  Nav2DVel-v0 is Nav2D-v0 (tests/nav2d_reference.py) with a continuous
action and another physics of one step; world, free-space test, distance, sensors, render, reward formula, measures and the
(seed, env, episode) streams are imported from that module, not restated.  The names of the parameters follow habitat's
`velocity_control` action, whose source is not at hand: the statement here IS this project's specification, and the kernel
`nav2d_vel_step_kernel` (habitat-lab_amd/csrc/nav2d.hip) reproduces it bit for bit (phi = atan2f excepted, as for Nav2D-v0).  Every
written operation is one float32 rounding, no fused multiply-add.

One step with the action a = (a_lin, a_ang):
  1. c = min(max(a, -1), 1) per component, 0 for a non-finite one;
  2. step length l = (c_lin + 1) * 0.125 (an add, then a multiply), in [0, 0.25];
  3. turn dh = (int) rint(c_ang * M), M = max_turn_angle / turn_angle, ties to even, left positive;
  4. stop = l < min_abs_lin_speed and |dh| < S, S = min_abs_ang_speed / turn_angle; on stop nothing moves;
  5. else h = (h + dh) mod nh; target (px + l * c, py + l * s) with (c, s) = dirs[h]; free: taken, path += l; blocked: one collision,
     and with sliding (nx, py) if free (path += |nx - px|), else (px, ny) if free (path += |ny - py|), else stay;
  6. distance, reward, step count, done, measures, sums and the next world exactly as Nav2D-v0 with `stop` in STOP's place."""
from __future__ import annotations

import math

import numpy as np

import nav2d_reference as R
from nav2d_reference import F, MEASURES, dist, heading_table, is_free, make_world, num_headings, ray_tables, render  # noqa: F401

HALF_RANGE = F(0.125)     # l = (c_lin + 1) * HALF_RANGE, so the longest step is Nav2D-v0's FORWARD
ONE = F(1.0)
EVENTS = ("slide_x", "slide_y", "blocked", "stops", "successes", "timeouts", "clamped", "ties", "zero_length")


def check_parameters(turn_angle, max_turn_angle, min_abs_lin_speed, min_abs_ang_speed):
    """-> (nh, M, S); ValueError naming the rule otherwise."""
    nh = num_headings(turn_angle)
    whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not whole(max_turn_angle) or max_turn_angle <= 0 or max_turn_angle % turn_angle != 0 or max_turn_angle > 180:
        raise ValueError(f"max_turn_angle {max_turn_angle!r} must be a positive multiple of turn_angle {turn_angle}, at most 180")
    if not whole(min_abs_ang_speed) or min_abs_ang_speed <= 0 or min_abs_ang_speed % turn_angle != 0 or min_abs_ang_speed > max_turn_angle:
        raise ValueError(f"min_abs_ang_speed {min_abs_ang_speed!r} must be a positive multiple of turn_angle {turn_angle}, at most "
                         f"max_turn_angle {max_turn_angle}")
    if not (isinstance(min_abs_lin_speed, (int, float, np.floating)) and 0.0 < float(min_abs_lin_speed) <= 0.25):
        raise ValueError(f"min_abs_lin_speed {min_abs_lin_speed!r} must be in (0, 0.25]")
    return nh, int(max_turn_angle) // int(turn_angle), int(min_abs_ang_speed) // int(turn_angle)


def clamp(a):
    """Step 1 for one component, float32 in and out."""
    a = F(a)
    return F(min(max(a, F(-1.0)), ONE)) if np.isfinite(a) else F(0.0)


def decode(action, M):
    """Steps 1-3: (c_lin, c_ang, l, dh, tie)."""
    a = np.asarray(action, dtype=np.float32).reshape(2)
    c_lin, c_ang = clamp(a[0]), clamp(a[1])
    l = F(F(c_lin + ONE) * HALF_RANGE)
    q = F(c_ang * F(M))
    tie = bool(abs(float(q)) % 1.0 == 0.5)
    return c_lin, c_ang, l, int(np.rint(q)), tie


class Nav2DVelEnv(R.Nav2DEnv):
    """One env, the interface of nav2d_reference.Nav2DEnv: `reset()` -> obs; `step((a_lin, a_ang))` -> (obs, reward, done, info)."""

    def __init__(self, seed, env, turn_angle=1, max_turn_angle=10, min_abs_lin_speed=0.025, min_abs_ang_speed=5, allow_sliding=True,
                 **kw):
        _, self.M, self.S = check_parameters(turn_angle, max_turn_angle, min_abs_lin_speed, min_abs_ang_speed)
        super().__init__(seed, env, turn_angle=turn_angle, **kw)
        self.min_lin, self.allow_sliding = F(min_abs_lin_speed), bool(allow_sliding)
        self.counters.update({k: 0 for k in EVENTS})
        self.last_dh = 0

    def step(self, action):
        a = np.asarray(action, dtype=np.float32)
        if a.shape != (2,):
            raise ValueError(f"action {action!r} is not (a_lin, a_ang)")
        w, cnt = self.world, self.counters
        c_lin, c_ang, l, dh, tie = decode(a, self.M)
        cnt["clamped"] += int((np.isfinite(a[0]) and c_lin != a[0]) or (np.isfinite(a[1]) and c_ang != a[1]))
        cnt["ties"] += int(tie)
        cnt["zero_length"] += int(l == 0)
        self.last_dh = dh
        stop = bool(l < self.min_lin and abs(dh) < self.S)
        if not stop:
            self.h = (self.h + dh) % self.nh
            c, s = self.dirs[self.h]
            nx, ny = F(self.px + F(l * c)), F(self.py + F(l * s))   # multiply, then a separate add
            if is_free(nx, ny, w.rects):
                self.px, self.py, self.path = nx, ny, F(self.path + l)
            else:
                self.collisions += 1
                inside = nx >= R.LO and nx <= R.HI and ny >= R.LO and ny <= R.HI
                cnt["obstacle_collisions" if inside else "wall_collisions"] += 1
                if self.allow_sliding and is_free(nx, self.py, w.rects):
                    self.path = F(self.path + F(abs(F(nx - self.px))))
                    self.px = nx
                    cnt["slide_x"] += 1
                elif self.allow_sliding and is_free(self.px, ny, w.rects):
                    self.path = F(self.path + F(abs(F(ny - self.py))))
                    self.py = ny
                    cnt["slide_y"] += 1
                else:
                    cnt["blocked"] += 1
        # from here on Nav2D-v0's end of a step, `stop` in the place of a == STOP
        d = dist(self.px, self.py, w.gx, w.gy)
        success = stop and d < R.SUCCESS_DIST
        reward = F(F(R.SLACK + F(self.d_prev - d)) + (R.SUCCESS_REWARD if success else F(0.0)))
        self.d_prev = d
        self.steps += 1
        done = stop or self.steps >= self.max_steps
        cnt["stops"] += int(stop)
        info = {}
        if done:
            spl = F(self.d_start / max(self.d_start, self.path)) if success else F(0.0)
            info = dict(success=float(success), spl=float(spl), distance_to_goal=float(d), collisions=float(self.collisions))
            self.last = dict(d_start=self.d_start, d_end=d, length=self.steps, success=bool(success), path=self.path)
            for k in MEASURES:
                self.sums[k] = F(self.sums[k] + F(info[k]))
            cnt["episodes"] += 1
            cnt["successes"] += int(success)
            cnt["timeouts"] += int(not stop)
            self.episode += 1
            self._begin()
        return self.observe(), reward, done, info


def greedy_action(goal_sensor, max_turn_angle):
    """The scripted controller: stop inside the success radius; else turn towards the goal as far as one step allows, at full speed
    scaled down near the goal once the goal is within one step's turn, slowly while it is not."""
    rho, phi_deg = float(goal_sensor[0]), math.degrees(float(goal_sensor[1]))
    if rho < 0.2:
        return (-1.0, 0.0)
    a_ang = min(max(phi_deg / max_turn_angle, -1.0), 1.0)
    a_lin = min(1.0, rho / 0.125 - 1.0) if abs(phi_deg) <= max_turn_angle else -0.5
    return (a_lin, a_ang)


SCRIPTS = ("forward", "greedy", "random", "grid")
GRID = (np.arange(-24, 25, dtype=np.float64) * 0.05).astype(np.float32)   # the multiples of 0.05 in [-1.2, 1.2]


def rollout(kind, seed, num_envs, steps, turn_angle=1, max_turn_angle=10, rng_seed=0, **env_kw):
    """`num_envs` restated envs for `steps` steps under one of the SCRIPTS, recorded like nav2d_reference.rollout: actions
    (steps, N, 2) float32, obs[t] (t = 0 the reset), rewards / dones (steps, N), infos[t][n], measure sums (steps, 4, N), dh (steps, N)
    and the summed event counters.  'forward' is (1, 0) always; 'greedy' is `greedy_action` on the restatement's own goal sensor;
    'random' is uniform in [-1.25, 1.25]^2; 'grid' draws each component from GRID (where c_ang * M falls on exact halves)."""
    envs = [Nav2DVelEnv(seed, n, turn_angle=turn_angle, max_turn_angle=max_turn_angle, **env_kw) for n in range(num_envs)]
    rng = np.random.RandomState(rng_seed)
    obs = [[e.reset() for e in envs]]
    out = dict(actions=np.zeros((steps, num_envs, 2), np.float32), rewards=np.zeros((steps, num_envs), np.float32),
               dones=np.zeros((steps, num_envs), bool), infos=[], sums=np.zeros((steps, len(MEASURES), num_envs), np.float32),
               dh=np.zeros((steps, num_envs), np.int64))
    for t in range(steps):
        if kind == "forward":
            a = np.tile(np.array([1.0, 0.0], np.float32), (num_envs, 1))
        elif kind == "greedy":
            a = np.array([greedy_action(o["pointgoal_with_gps_compass"], max_turn_angle) for o in obs[-1]], dtype=np.float32)
        elif kind == "random":
            a = rng.uniform(-1.25, 1.25, size=(num_envs, 2)).astype(np.float32)
        elif kind == "grid":
            a = GRID[rng.randint(0, len(GRID), size=(num_envs, 2))]
        else:
            raise ValueError(kind)
        res = [e.step(x) for e, x in zip(envs, a)]
        out["actions"][t] = a
        obs.append([r[0] for r in res])
        out["rewards"][t] = [r[1] for r in res]
        out["dones"][t] = [r[2] for r in res]
        out["infos"].append([r[3] for r in res])
        out["sums"][t] = [[e.sums[k] for e in envs] for k in MEASURES]
        out["dh"][t] = [e.last_dh for e in envs]
    out["obs"] = obs
    out["counters"] = {k: sum(e.counters[k] for e in envs) for k in envs[0].counters}
    out["envs"] = envs
    return out


# The scripted runs tests/test_gpu_nav2d_vel.py holds the kernel to: shapes as nav2d_reference's SCRIPT_*, K in {0, 3, 8} crossed with
# the two parameter sets (turn_angle, max_turn_angle, min_abs_ang_speed).  Over the four scripts and three K of a parameter set every
# counter of EVENTS is at least 1 (tests/test_nav2d_vel_host.py asserts it); the seeds are the first of 1, 2, ... at which that holds.
SCRIPT_ENVS, SCRIPT_STEPS, SCRIPT_MAX_EPISODE_STEPS = R.SCRIPT_ENVS, R.SCRIPT_STEPS, R.SCRIPT_MAX_EPISODE_STEPS
PARAMETER_SETS = [(1, 10, 5), (5, 30, 10)]
SCRIPT_CASES = [(K, p) for K in (0, 3, 8) for p in PARAMETER_SETS]


def script_seed(kind, K, params=None):
    return 1


def script_rollout(kind, K, params, H=0, W=0, **kw):
    turn, max_turn, min_ang = params
    return rollout(kind, script_seed(kind, K, params), SCRIPT_ENVS, SCRIPT_STEPS, turn_angle=turn, max_turn_angle=max_turn,
                   min_abs_ang_speed=min_ang, num_obstacles=K, max_episode_steps=SCRIPT_MAX_EPISODE_STEPS, H=H, W=W, **kw)
