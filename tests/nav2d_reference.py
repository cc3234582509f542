"""Plain-numpy restatement of the Nav2D-v0 task (habitat_amd/common/env_factory.py: Nav2DVectorEnv), shared by
tests/test_nav2d_host.py and tests/test_gpu_nav2d.py.  This file is the specification the HIP kernels
(habitat-lab_amd/csrc/nav2d.hip) are held to: every quantity below is computed with one float32 rounding per written operation
(no fused multiply-add), so the kernels reproduce it bit for bit.  The single exception is `phi = atan2f(cross, dot)`: the
restatement keeps the float32 `(cross, dot)` pair so that a test can bound the kernel's phi against a float64 atan2.

The definition itself (world, actions, reward, measures, sensors) is stated in Nav2DVectorEnv's module docstring; the
comments here only say which operation order is the pinned one."""
from __future__ import annotations

import math

import numpy as np

F = np.float32
GOLD = np.uint32(0x9E3779B9)
# stream ids (the `sensor` argument of stream_key); 0..8 belong to the hashed pointnav / objectnav tasks
S_OBST, S_START, S_GOAL, S_HEAD, S_COLOR = 16, 17, 18, 19, 20
MAX_OBSTACLES, CANDIDATES = 8, 16
ARENA, RADIUS, FORWARD, SUCCESS_DIST, SLACK, SUCCESS_REWARD = F(8.0), F(0.1), F(0.25), F(0.2), F(-0.01), F(2.5)
LO, HI = F(0.1), F(7.9)
CAM_H, DEPTH_SCALE, MARKER_R2 = F(1.25), F(10.0), F(0.2) * F(0.2)
STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT = 0, 1, 2, 3
WALL_RGB = np.array([[200, 180, 150], [150, 200, 180], [180, 150, 200], [200, 200, 150]], dtype=np.uint8)  # +x, -x, +y, -y
CEIL_RGB, FLOOR_RGB, MARKER_RGB = (np.array(c, dtype=np.uint8) for c in ((230, 230, 240), (110, 100, 90), (255, 32, 32)))
MEASURES = ("success", "spl", "distance_to_goal", "collisions")
INF = F(np.inf)


def mix(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def stream_key(seed, sensor, env, t):
    with np.errstate(over="ignore"):
        h = mix(np.uint32(seed & 0xFFFFFFFF) + GOLD * np.uint32(sensor + 1))
        h = mix(h ^ np.uint32(env & 0xFFFFFFFF))
        h = mix(h ^ np.uint32(t & 0xFFFFFFFF))
    return h


def words(seed, sensor, env, t, n):
    return mix(stream_key(seed, sensor, env, t) ^ np.arange(n, dtype=np.uint32))


def u01(w):
    return (w >> np.uint32(8)).astype(np.float32) * F(2.0 ** -24)


# ---- host tables (float64, rounded once) ------------------------------------------------------------------------------------
def num_headings(turn_angle):
    if not isinstance(turn_angle, (int, np.integer)) or turn_angle <= 0 or 360 % int(turn_angle) != 0:
        raise ValueError(f"turn_angle {turn_angle!r} must be a positive integer number of degrees that divides 360")
    return 360 // int(turn_angle)


def heading_table(turn_angle):
    """(nh, 2) float32 (cos, sin) of heading h * turn_angle degrees."""
    nh = num_headings(turn_angle)
    a = np.arange(nh, dtype=np.float64) * (2.0 * math.pi / nh)
    return np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32)


def ray_tables(turn_angle, H, W):
    """ray (nh, W, 2): world direction of column u's ray at heading h (column 0 is the leftmost, 90 degree horizontal field of
    view, pinhole); cosf (W,): cosine between that ray and the optical axis; tanv (H,): tangent of row v's elevation (row 0 is the
    top; square pixels, so the vertical half extent is H / W)."""
    nh = num_headings(turn_angle)
    tu = 1.0 - 2.0 * (np.arange(W, dtype=np.float64) + 0.5) / W
    au = np.arctan(tu)
    th = np.arange(nh, dtype=np.float64)[:, None] * (2.0 * math.pi / nh) + au[None, :]
    ray = np.stack([np.cos(th), np.sin(th)], 2).astype(np.float32)
    cosf = np.cos(au).astype(np.float32)
    tanv = ((1.0 - 2.0 * (np.arange(H, dtype=np.float64) + 0.5) / H) * (H / W)).astype(np.float32)
    return ray, cosf, tanv


# ---- world ------------------------------------------------------------------------------------------------------------------
def is_free(x, y, rects):
    """Box test: inside [0.1, 7.9]^2 and not strictly inside any rectangle inflated by the agent radius."""
    if not (x >= LO and x <= HI and y >= LO and y <= HI):
        return False
    for x0, y0, x1, y1 in rects:
        if x > x0 - RADIUS and x < x1 + RADIUS and y > y0 - RADIUS and y < y1 + RADIUS:
            return False
    return True


def dist(ax, ay, bx, by):
    dx, dy = F(bx - ax), F(by - ay)
    return F(np.sqrt(F(F(dx * dx) + F(dy * dy))))


class World:
    __slots__ = ("rects", "colors", "sx", "sy", "gx", "gy", "h", "start_fallback", "goal_fallback")


def make_world(seed, env, episode, K, nh, candidates=CANDIDATES):
    w = World()
    u = u01(words(seed, S_OBST, env, episode, 4 * MAX_OBSTACLES))
    cw = words(seed, S_COLOR, env, episode, MAX_OBSTACLES)
    w.rects, w.colors = [], []
    for k in range(K):
        cx, cy = F(F(2.0) + F(F(4.0) * u[4 * k])), F(F(2.0) + F(F(4.0) * u[4 * k + 1]))
        hx, hy = F(F(0.25) + F(F(0.75) * u[4 * k + 2])), F(F(0.25) + F(F(0.75) * u[4 * k + 3]))
        w.rects.append((F(cx - hx), F(cy - hy), F(cx + hx), F(cy + hy)))
        c = int(cw[k])
        w.colors.append((64 + (c & 127), 64 + ((c >> 8) & 127), 64 + ((c >> 16) & 127)))
    us = u01(words(seed, S_START, env, episode, 2 * CANDIDATES))
    ug = u01(words(seed, S_GOAL, env, episode, 2 * CANDIDATES))
    w.sx, w.sy, w.start_fallback = F(0.5), F(0.5), True
    for j in range(candidates):
        x, y = F(LO + F(F(7.8) * us[2 * j])), F(LO + F(F(7.8) * us[2 * j + 1]))
        if is_free(x, y, w.rects):
            w.sx, w.sy, w.start_fallback = x, y, False
            break
    w.gx, w.gy, w.goal_fallback = F(7.5), F(7.5), True
    for j in range(candidates):
        x, y = F(LO + F(F(7.8) * ug[2 * j])), F(LO + F(F(7.8) * ug[2 * j + 1]))
        if is_free(x, y, w.rects) and dist(w.sx, w.sy, x, y) >= F(1.0):
            w.gx, w.gy, w.goal_fallback = x, y, False
            break
    w.h = int(words(seed, S_HEAD, env, episode, 1)[0] % np.uint32(nh))
    return w


# ---- rendering --------------------------------------------------------------------------------------------------------------
def _slab(lo, hi, p, d, inv):
    """Entry / exit parameters of the ray p + t d through [lo, hi] on one axis, vectors over the columns."""
    t0, t1 = (lo - p) * inv, (hi - p) * inv  # float32 products; lanes with d == 0 are overwritten below
    tmin, tmax = np.minimum(t0, t1), np.maximum(t0, t1)
    inside = (p > lo) and (p < hi)
    z = d == 0
    tmin = np.where(z, -INF if inside else INF, tmin)
    tmax = np.where(z, INF if inside else -INF, tmax)
    return tmin.astype(np.float32), tmax.astype(np.float32)


def column_hits(px, py, gx, gy, h, rects, ray, cosf):
    """Per column: z_wall (what depth sees), hit id (0..3 walls, 4 + k obstacles), z_rgb and marker flag (what rgb sees)."""
    d = ray[h]
    dx, dy = d[:, 0], d[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ix, iy = F(1.0) / dx, F(1.0) / dy
        tx = np.where(dx > 0, F(ARENA - px) * ix, np.where(dx < 0, F(F(0.0) - px) * ix, INF)).astype(np.float32)
        ty = np.where(dy > 0, F(ARENA - py) * iy, np.where(dy < 0, F(F(0.0) - py) * iy, INF)).astype(np.float32)
        t = np.where(tx <= ty, tx, ty)
        hit = np.where(tx <= ty, np.where(dx > 0, 0, 1), np.where(dy > 0, 2, 3)).astype(np.int32)
        for k, (x0, y0, x1, y1) in enumerate(rects):
            axn, axx = _slab(x0, x1, px, dx, ix)
            ayn, ayx = _slab(y0, y1, py, dy, iy)
            tn, tm = np.maximum(axn, ayn), np.minimum(axx, ayx)
            ok = (tn <= tm) & (tn > 0) & (tn < t)
            t = np.where(ok, tn, t)
            hit = np.where(ok, 4 + k, hit)
    z_wall = (t * cosf).astype(np.float32)
    # goal marker: vertical cylinder of radius 0.2 around the goal, nearest intersection, ray direction taken as unit length
    ox, oy = F(px - gx), F(py - gy)
    b = (ox * dx).astype(np.float32) + (oy * dy).astype(np.float32)
    c = F(F(F(ox * ox) + F(oy * oy)) - MARKER_R2)
    disc = (b * b).astype(np.float32) - c
    with np.errstate(invalid="ignore"):
        tm = (-b - np.sqrt(np.maximum(disc, F(0.0)))).astype(np.float32)
    marker = (disc >= 0) & (tm > 0) & (tm < t)
    z_rgb = np.where(marker, (tm * cosf).astype(np.float32), z_wall).astype(np.float32)
    return z_wall, hit, z_rgb, marker


def _shade(color, depth01):
    """uint8 colour (.., 3) scaled by 1 - depth, truncated."""
    s = (F(1.0) - depth01).astype(np.float32)
    return (color.astype(np.float32) * s[..., None]).astype(np.float32).astype(np.uint8)


def render(px, py, gx, gy, h, rects, colors, ray, cosf, tanv, want_rgb=True, want_depth=True):
    z_wall, hit, z_rgb, marker = column_hits(px, py, gx, gy, h, rects, ray, cosf)
    with np.errstate(divide="ignore"):
        zf = (CAM_H / np.abs(tanv)).astype(np.float32)                      # (H,) floor / ceiling z-depth of the row
    d_wall = np.minimum(z_wall / DEPTH_SCALE, F(1.0)).astype(np.float32)    # (W,)
    d_rgbw = np.minimum(z_rgb / DEPTH_SCALE, F(1.0)).astype(np.float32)
    d_flat = np.minimum(zf / DEPTH_SCALE, F(1.0)).astype(np.float32)        # (H,)
    out = {}
    if want_depth:
        out["depth"] = np.where(z_wall[None, :] <= zf[:, None], d_wall[None, :], d_flat[:, None]).astype(np.float32)[..., None]
    if want_rgb:
        palette = np.concatenate([WALL_RGB, np.array(colors, dtype=np.uint8).reshape(-1, 3)], 0)
        base = np.where(marker[:, None], MARKER_RGB[None, :], palette[hit])
        c_wall = _shade(base, d_rgbw)                                        # (W, 3)
        flat = np.where((tanv > 0)[:, None], CEIL_RGB[None, :], FLOOR_RGB[None, :])
        c_flat = _shade(flat, d_flat)                                        # (H, 3)
        out["rgb"] = np.where((z_rgb[None, :] <= zf[:, None])[..., None], c_wall[None, :, :], c_flat[:, None, :]).astype(np.uint8)
    return out


# ---- the task ---------------------------------------------------------------------------------------------------------------
class Nav2DEnv:
    """One env: `reset()` -> obs; `step(a)` -> (obs, reward float32, done, info).  obs holds 'pointgoal_with_gps_compass' (rho and
    a float64-atan2 phi rounded to float32), 'cross_dot' (the float32 pair phi is taken of) and, when asked, 'rgb' / 'depth'.  After
    a done the observation is the next episode's first one and `info` carries the four measures of the episode that ended."""

    def __init__(self, seed, env, H=0, W=0, num_obstacles=3, turn_angle=10, max_episode_steps=500, use_rgb=True, use_depth=True,
                 candidates=CANDIDATES):
        if not 0 <= int(num_obstacles) <= MAX_OBSTACLES:
            raise ValueError(f"num_obstacles {num_obstacles} outside 0..{MAX_OBSTACLES}")
        self.seed, self.env, self.H, self.W, self.K = int(seed) & 0xFFFFFFFF, int(env), H, W, int(num_obstacles)
        self.nh, self.max_steps, self.candidates = num_headings(turn_angle), int(max_episode_steps), candidates
        self.use_rgb, self.use_depth = use_rgb and H > 0, use_depth and H > 0
        self.dirs = heading_table(turn_angle)
        if self.use_rgb or self.use_depth:
            self.ray, self.cosf, self.tanv = ray_tables(turn_angle, H, W)
        self.sums = {k: F(0.0) for k in MEASURES}
        self.episode = 0
        self.counters = dict(episodes=0, successes=0, wall_collisions=0, obstacle_collisions=0, timeouts=0, start_fallbacks=0,
                             goal_fallbacks=0)

    def _begin(self):
        w = self.world = make_world(self.seed, self.env, self.episode, self.K, self.nh, self.candidates)
        self.px, self.py, self.h = w.sx, w.sy, w.h
        self.d_start = self.d_prev = dist(self.px, self.py, w.gx, w.gy)
        self.path, self.steps, self.collisions = F(0.0), 0, 0
        self.counters["start_fallbacks"] += int(w.start_fallback)
        self.counters["goal_fallbacks"] += int(w.goal_fallback)

    def reset(self):
        self.episode = 0
        self._begin()
        return self.observe()

    def observe(self):
        w = self.world
        c, s = self.dirs[self.h]
        dx, dy = F(w.gx - self.px), F(w.gy - self.py)
        dot = F(F(dx * c) + F(dy * s))
        cross = F(F(c * dy) - F(s * dx))
        rho = dist(self.px, self.py, w.gx, w.gy)
        o = {"pointgoal_with_gps_compass": np.array([rho, F(math.atan2(float(cross), float(dot)))], dtype=np.float32),
             "cross_dot": np.array([cross, dot], dtype=np.float32)}
        if self.use_rgb or self.use_depth:
            o.update(render(self.px, self.py, w.gx, w.gy, self.h, w.rects, w.colors, self.ray, self.cosf, self.tanv,
                            self.use_rgb, self.use_depth))
        return o

    def step(self, action):
        a = int(action)
        if a < 0 or a > 3:
            raise ValueError(f"action {action!r} outside 0..3")
        w = self.world
        if a == MOVE_FORWARD:
            c, s = self.dirs[self.h]
            nx, ny = F(self.px + F(FORWARD * c)), F(self.py + F(FORWARD * s))   # multiply, then a separate add
            if is_free(nx, ny, w.rects):
                self.px, self.py, self.path = nx, ny, F(self.path + FORWARD)
            else:
                self.collisions += 1
                inside = nx >= LO and nx <= HI and ny >= LO and ny <= HI
                self.counters["obstacle_collisions" if inside else "wall_collisions"] += 1
        elif a == TURN_LEFT:
            self.h = (self.h + 1) % self.nh
        elif a == TURN_RIGHT:
            self.h = (self.h + self.nh - 1) % self.nh
        d = dist(self.px, self.py, w.gx, w.gy)
        success = a == STOP and d < SUCCESS_DIST
        reward = F(F(SLACK + F(self.d_prev - d)) + (SUCCESS_REWARD if success else F(0.0)))
        self.d_prev = d
        self.steps += 1
        done = a == STOP or self.steps >= self.max_steps
        info = {}
        if done:
            spl = F(self.d_start / max(self.d_start, self.path)) if success else F(0.0)
            info = dict(success=float(success), spl=float(spl), distance_to_goal=float(d), collisions=float(self.collisions))
            self.last = dict(d_start=self.d_start, d_end=d, length=self.steps, success=bool(success))
            for k in MEASURES:
                self.sums[k] = F(self.sums[k] + F(info[k]))
            self.counters["episodes"] += 1
            self.counters["successes"] += int(success)
            self.counters["timeouts"] += int(a != STOP)
            self.episode += 1
            self._begin()
        return self.observe(), reward, done, info


def greedy_action(goal_sensor, turn_angle):
    """The scripted controller of the tests: STOP inside the success radius, turn towards the goal until |phi| <= turn / 2, else
    go forward."""
    rho, phi = float(goal_sensor[0]), float(goal_sensor[1])
    if rho < 0.2:
        return STOP
    if abs(phi) <= math.radians(turn_angle) / 2.0:
        return MOVE_FORWARD
    return TURN_LEFT if phi > 0 else TURN_RIGHT


# ---- scripted rollouts shared by the host and the GPU tests --------------------------------------------------------------------
SCRIPTS = ("forward", "greedy", "never_stop", "random")


def rollout(kind, seed, num_envs, steps, turn_angle=10, rng_seed=0, **env_kw):
    """Runs `num_envs` restated envs for `steps` steps under one of the SCRIPTS and records everything a test compares:
    actions (steps, N) int64, obs[t] (list over envs, t = 0 the reset), rewards / dones (steps, N), infos[t][n], measure sums
    (steps, 4, N) after each step, and the summed event counters.  'forward' only moves forward; 'greedy' is `greedy_action` on the
    restatement's own goal sensor; 'never_stop' draws from the three moving actions; 'random' draws from all four."""
    envs = [Nav2DEnv(seed, n, turn_angle=turn_angle, **env_kw) for n in range(num_envs)]
    rng = np.random.RandomState(rng_seed)
    obs = [[e.reset() for e in envs]]
    out = dict(actions=np.zeros((steps, num_envs), np.int64), rewards=np.zeros((steps, num_envs), np.float32),
               dones=np.zeros((steps, num_envs), bool), infos=[], sums=np.zeros((steps, len(MEASURES), num_envs), np.float32))
    for t in range(steps):
        if kind == "forward":
            a = [MOVE_FORWARD] * num_envs
        elif kind == "greedy":
            a = [greedy_action(o["pointgoal_with_gps_compass"], turn_angle) for o in obs[-1]]
        elif kind == "never_stop":
            a = list(rng.randint(1, 4, size=num_envs))
        else:
            a = list(rng.randint(0, 4, size=num_envs))
        res = [e.step(x) for e, x in zip(envs, a)]
        out["actions"][t] = a
        obs.append([r[0] for r in res])
        out["rewards"][t] = [r[1] for r in res]
        out["dones"][t] = [r[2] for r in res]
        out["infos"].append([r[3] for r in res])
        out["sums"][t] = [[e.sums[k] for e in envs] for k in MEASURES]
    out["obs"] = obs
    out["counters"] = {k: sum(e.counters[k] for e in envs) for k in envs[0].counters}
    out["envs"] = envs
    return out


# The shapes of the scripted runs that tests/test_gpu_nav2d.py holds the kernels to, and the seeds at which each script shows the
# event it is there for (searched on the CPU, seeds 1, 2, ...; tests/test_nav2d_host.py asserts the counters).
SCRIPT_ENVS, SCRIPT_STEPS, SCRIPT_MAX_EPISODE_STEPS = 5, 60, 12
SCRIPT_CASES = [(K, turn) for K in (0, 3, 8) for turn in (10, 30)]


def script_seed(kind, K):
    return 2 if (kind == "greedy" and K == 3) else 1
