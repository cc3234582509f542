"""Plain-numpy restatement of the Nav2DObj-v0 task (habitat_amd/common/env_factory.py: Nav2DObjVectorEnv), shared by
tests/test_nav2d_obj_host.py and tests/test_gpu_nav2d_obj.py.  This file is the specification: `nav2d_obj_step_kernel` and the
object instantiation of `nav2d_render_kernel` (habitat-lab_amd/csrc/nav2d.hip) reproduce every output bit for bit -- no angle
function runs on the device, so there is no exception.  Every written operation is one float32 rounding, no fused multiply-add.

Nav2DObj-v0 is Nav2D-v0's world (tests/nav2d_reference.py: arena, rectangles, start, heading, the box free test, streams 16-20, the
0.25 m forward step; imported, not restated) with objects in it and no goal position: the agent is told a category and has to find an
object of it in its images.

Objects.  M = num_objects in 1..8 upright cylinders of radius 0.3 m from floor to ceiling, placed after the start.  Streams: 21
  positions, 22 categories, 23 target.  Candidate i (0..15) of object j is (0.1 + 7.8 u_2(16j+i), 0.1 + 7.8 u_2(16j+i)+1) of stream
  21.  Object j takes its first candidate that lies in [0.5, 7.5]^2, is not strictly inside a rectangle grown by 0.3 on every side,
  is at least 1 m from the start and at least 1 m from every earlier object (float32 `dist`, >= 1).
  Fallback: an object with no such candidate takes the first slot q = 0..27 of the RING that is at least 1 m from the start and from
  every earlier object.  The ring is the 28 points one metre apart on the square through (0.5, 0.5) and (7.5, 7.5), counter-clockwise
  from (0.5, 0.5); all coordinates are exact in float32.  Rectangles lie in [1, 7]^2, so grown by 0.3 they never reach a slot.  An
  open disc of radius 1 holds at most three slots (three only round a corner), so the start and seven earlier objects rule out at
  most 24 of the 28: a slot always fits.  Hence every object is always placed, the spacing rules hold for fallback objects too, the
  start stays free (every centre is >= 1 m > 0.4 m away) and the target category always has an instance.
  Category of object j: word j of stream 22 modulo C = num_categories, C in 1..21.
  Objects block the agent: a position is free when Nav2D-v0's box test holds and `dist` to every centre is >= 0.4.
Target.  category[word 0 of stream 23 modulo M].  d = the smallest `dist` from the agent to a centre of the target category (the
  first of equally near ones); the nearest instance may change during an episode.  Its centre is kept in the state words (gx, gy).
Actions.  Discrete(4) or Discrete(6) in habitat's order: STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT, LOOK_UP, LOOK_DOWN; the two
  looks change nothing and cost a step.
Reward, end, measures: Nav2D-v0's with this d; success = STOP and d < 1.0.
Sensors.  objectgoal int64 (1,) = the target category.  gps float32 (2,) = (dot, cross) of p - start in the start heading's frame,
  dot = dx * c + dy * s, cross = c * dy - s * dx with (c, s) = dirs[h0].  compass float32 (1,) = COMPASS[(h - h0) mod nh], the table
  of k * turn_angle in (-pi, pi] (k > nh / 2 counts as k - nh) computed in float64 and rounded once.  depth: Nav2D-v0's, with the
  cylinders as geometry: after walls and rectangles, object j = 0..M-1 in order replaces the column's hit when the goal marker's
  ray-circle test (radius 0.3) gives a nearer positive t.  rgb: Nav2D-v0's without the goal marker; an object has its category's
  colour `category_color`, the same in every episode.  semantic int32 (H, W, 1): floor 0, ceiling 1, walls 2, rectangles 3, an
  object 4 + category; a pixel shows the column's hit where depth does."""
from __future__ import annotations

import math

import numpy as np

import nav2d_reference as R
from nav2d_reference import F, INF, LO, HI, MEASURES, dist, heading_table, mix, num_headings, ray_tables, u01, words  # noqa: F401

S_OBJ_POS, S_OBJ_CAT, S_OBJ_TARGET = 21, 22, 23
MAX_OBJECTS, MAX_CATEGORIES, CANDIDATES, RING_SLOTS = 8, 21, 16, 28
OBJ_R, OBJ_BLOCK, OBJ_LO, OBJ_HI, OBJ_APART, SUCCESS_DIST = F(0.3), F(0.4), F(0.5), F(7.5), F(1.0), F(1.0)
OBJ_R2 = F(OBJ_R * OBJ_R)
STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT, LOOK_UP, LOOK_DOWN = range(6)
SEM_FLOOR, SEM_CEILING, SEM_WALL, SEM_RECT, SEM_OBJECT = 0, 1, 2, 3, 4
HIT_OBJECT = 4 + R.MAX_OBSTACLES   # hit ids: 0..3 walls, 4 + k rectangles, HIT_OBJECT + j objects
EVENTS = ("stop_too_far", "blocked_object", "blocked_rect", "blocked_wall", "nearest_changes", "objects_hidden", "objects_visible",
          "object_fallbacks", "looks")


def check_parameters(num_objects, num_categories, num_actions):
    whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not whole(num_objects) or not 1 <= num_objects <= MAX_OBJECTS:
        raise ValueError(f"num_objects {num_objects!r} outside 1..{MAX_OBJECTS}")
    if not whole(num_categories) or not 1 <= num_categories <= MAX_CATEGORIES:
        raise ValueError(f"num_categories {num_categories!r} outside 1..{MAX_CATEGORIES}")
    if num_actions not in (4, 6):
        raise ValueError(f"num_actions {num_actions!r} is neither 4 nor 6")


def compass_table(turn_angle):
    """(nh,) float32: k * turn_angle in (-pi, pi], k counted as k - nh above the half turn."""
    nh = num_headings(turn_angle)
    k = np.arange(nh, dtype=np.int64)
    k = np.where(2 * k > nh, k - nh, k)
    return (k.astype(np.float64) * (2.0 * math.pi / nh)).astype(np.float32)


def category_color(cat):
    c = int(mix(np.uint32((0x0B7EC700 + int(cat)) & 0xFFFFFFFF)))
    return (128 + (c & 127), 128 + ((c >> 8) & 127), 128 + ((c >> 16) & 127))


def ring_slot(q):
    side, i = divmod(q, 7)
    i = F(i)
    x = (F(F(0.5) + i), F(7.5), F(F(7.5) - i), F(0.5))[side]
    y = (F(0.5), F(F(0.5) + i), F(7.5), F(F(7.5) - i))[side]
    return x, y


def _fits(x, y, sx, sy, objects):
    if not dist(sx, sy, x, y) >= OBJ_APART:
        return False
    return all(dist(ox, oy, x, y) >= OBJ_APART for ox, oy in objects)


def make_world(seed, env, episode, K, nh, M, C, candidates=R.CANDIDATES, obj_candidates=CANDIDATES):
    """Nav2D-v0's world (its goal is not used) with .objects [(x, y)], .cats, .target and .object_fallbacks."""
    w = R.make_world(seed, env, episode, K, nh, candidates)
    u = u01(words(seed, S_OBJ_POS, env, episode, 2 * CANDIDATES * MAX_OBJECTS))
    cw = words(seed, S_OBJ_CAT, env, episode, MAX_OBJECTS)
    objects, cats, fallbacks = [], [], 0
    for j in range(M):
        spot = None
        for i in range(obj_candidates):
            x, y = F(LO + F(F(7.8) * u[2 * (CANDIDATES * j + i)])), F(LO + F(F(7.8) * u[2 * (CANDIDATES * j + i) + 1]))
            if not (x >= OBJ_LO and x <= OBJ_HI and y >= OBJ_LO and y <= OBJ_HI):
                continue
            if any(x > F(x0 - OBJ_R) and x < F(x1 + OBJ_R) and y > F(y0 - OBJ_R) and y < F(y1 + OBJ_R) for x0, y0, x1, y1 in w.rects):
                continue
            if _fits(x, y, w.sx, w.sy, objects):
                spot = (x, y)
                break
        if spot is None:
            fallbacks += 1
            for q in range(RING_SLOTS):
                spot = ring_slot(q)
                if _fits(spot[0], spot[1], w.sx, w.sy, objects):
                    break
        objects.append(spot)
        cats.append(int(cw[j] % np.uint32(C)))
    target = cats[int(words(seed, S_OBJ_TARGET, env, episode, 1)[0] % np.uint32(M))]
    return w, objects, cats, target, fallbacks


def is_free(x, y, rects, objects):
    return R.is_free(x, y, rects) and all(not dist(x, y, ox, oy) < OBJ_BLOCK for ox, oy in objects)


def nearest_target(px, py, objects, cats, target):
    """(d, index): the first of equally near instances wins."""
    best, idx = INF, -1
    for j, (ox, oy) in enumerate(objects):
        if cats[j] != target:
            continue
        d = dist(px, py, ox, oy)
        if d < best:
            best, idx = d, j
    return best, idx


# ---- rendering --------------------------------------------------------------------------------------------------------------
def column_hits(px, py, h, rects, objects, ray, cosf):
    """Per column: z (what all three images see) and the hit id.  Walls and rectangles as nav2d_reference.column_hits, then the
    cylinders with its goal-marker test, ray direction taken as unit length."""
    d = ray[h]
    dx, dy = d[:, 0], d[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ix, iy = F(1.0) / dx, F(1.0) / dy
        tx = np.where(dx > 0, F(R.ARENA - px) * ix, np.where(dx < 0, F(F(0.0) - px) * ix, INF)).astype(np.float32)
        ty = np.where(dy > 0, F(R.ARENA - py) * iy, np.where(dy < 0, F(F(0.0) - py) * iy, INF)).astype(np.float32)
        t = np.where(tx <= ty, tx, ty)
        hit = np.where(tx <= ty, np.where(dx > 0, 0, 1), np.where(dy > 0, 2, 3)).astype(np.int32)
        for k, (x0, y0, x1, y1) in enumerate(rects):
            axn, axx = R._slab(x0, x1, px, dx, ix)
            ayn, ayx = R._slab(y0, y1, py, dy, iy)
            tn, tm = np.maximum(axn, ayn), np.minimum(axx, ayx)
            ok = (tn <= tm) & (tn > 0) & (tn < t)
            t = np.where(ok, tn, t)
            hit = np.where(ok, 4 + k, hit)
        for j, (cx, cy) in enumerate(objects):
            ox, oy = F(px - cx), F(py - cy)
            b = (ox * dx).astype(np.float32) + (oy * dy).astype(np.float32)
            c = F(F(F(ox * ox) + F(oy * oy)) - OBJ_R2)
            disc = (b * b).astype(np.float32) - c
            to = (-b - np.sqrt(np.maximum(disc, F(0.0)))).astype(np.float32)
            ok = (disc >= 0) & (to > 0) & (to < t)
            t = np.where(ok, to, t).astype(np.float32)
            hit = np.where(ok, HIT_OBJECT + j, hit)
    return (t * cosf).astype(np.float32), hit


def render(px, py, h, rects, colors, objects, cats, ray, cosf, tanv, want_rgb=True, want_depth=True, want_semantic=True):
    z, hit = column_hits(px, py, h, rects, objects, ray, cosf)
    with np.errstate(divide="ignore"):
        zf = (R.CAM_H / np.abs(tanv)).astype(np.float32)
    d_wall = np.minimum(z / R.DEPTH_SCALE, F(1.0)).astype(np.float32)
    d_flat = np.minimum(zf / R.DEPTH_SCALE, F(1.0)).astype(np.float32)
    wall = z[None, :] <= zf[:, None]                                        # (H, W): the column's hit is what the pixel shows
    out = {"hit": hit}
    if want_depth:
        out["depth"] = np.where(wall, d_wall[None, :], d_flat[:, None]).astype(np.float32)[..., None]
    if want_rgb:
        rect_rgb = np.zeros((R.MAX_OBSTACLES, 3), np.uint8)
        rect_rgb[:len(colors)] = np.array(colors, dtype=np.uint8).reshape(-1, 3)
        palette = np.concatenate([R.WALL_RGB, rect_rgb, np.array([category_color(c) for c in cats], dtype=np.uint8).reshape(-1, 3)], 0)
        c_wall = R._shade(palette[hit], d_wall)
        flat = np.where((tanv > 0)[:, None], R.CEIL_RGB[None, :], R.FLOOR_RGB[None, :])
        c_flat = R._shade(flat, d_flat)
        out["rgb"] = np.where(wall[..., None], c_wall[None, :, :], c_flat[:, None, :]).astype(np.uint8)
    if want_semantic:
        ids = np.array([SEM_WALL] * 4 + [SEM_RECT] * R.MAX_OBSTACLES + [SEM_OBJECT + c for c in cats], dtype=np.int32)
        s_flat = np.where(tanv > 0, SEM_CEILING, SEM_FLOOR).astype(np.int32)
        out["semantic"] = np.where(wall, ids[hit][None, :], s_flat[:, None]).astype(np.int32)[..., None]
    return out


def _segment_crosses_rect(ax, ay, bx, by, rect):
    """float64 slab test of the segment a -> b against one rectangle (event bookkeeping only, not part of the task)."""
    x0, y0, x1, y1 = (float(v) for v in rect)
    t0, t1 = 0.0, 1.0
    for p, d, lo, hi in ((ax, bx - ax, x0, x1), (ay, by - ay, y0, y1)):
        if d == 0.0:
            if not lo < p < hi:
                return False
            continue
        a, b = (lo - p) / d, (hi - p) / d
        t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
    return t0 < t1


# ---- the task ---------------------------------------------------------------------------------------------------------------
class Nav2DObjEnv(R.Nav2DEnv):
    """One env, the interface of nav2d_reference.Nav2DEnv.  obs holds 'objectgoal', 'gps', 'compass' and, when asked, 'rgb' / 'depth' /
    'semantic'.  `state_words()` is what the device record holds for this env."""

    def __init__(self, seed, env, H=0, W=0, num_objects=3, num_categories=4, num_actions=6, turn_angle=10, use_rgb=True,
                 use_depth=True, use_semantic=True, obj_candidates=CANDIDATES, **kw):
        check_parameters(num_objects, num_categories, num_actions)
        super().__init__(seed, env, H=H, W=W, turn_angle=turn_angle, use_rgb=use_rgb, use_depth=use_depth, **kw)
        self.M, self.C, self.num_actions, self.obj_candidates = int(num_objects), int(num_categories), int(num_actions), obj_candidates
        self.use_semantic = use_semantic and H > 0
        if self.use_semantic and not (self.use_rgb or self.use_depth):
            self.ray, self.cosf, self.tanv = ray_tables(turn_angle, H, W)
        self.compass = compass_table(turn_angle)
        self.counters.update({k: 0 for k in EVENTS})
        self.ended = 0
        self.last_measures = [F(0.0)] * 4

    def _begin(self):
        w, self.objects, self.cats, self.target, fb = make_world(self.seed, self.env, self.episode, self.K, self.nh, self.M, self.C,
                                                                 self.candidates, self.obj_candidates)
        self.world = w
        self.px, self.py, self.h = w.sx, w.sy, w.h
        self.sx, self.sy, self.h0 = w.sx, w.sy, w.h
        d, self.nearest = nearest_target(self.px, self.py, self.objects, self.cats, self.target)
        self.d_start = self.d_prev = d
        self.path, self.steps, self.collisions = F(0.0), 0, 0
        self.counters["start_fallbacks"] += int(w.start_fallback)
        self.counters["object_fallbacks"] += fb

    def reset(self):
        self.ended, self.last_measures = 0, [F(0.0)] * 4
        return super().reset()

    def observe(self):
        w = self.world
        c, s = self.dirs[self.h0]
        dx, dy = F(self.px - self.sx), F(self.py - self.sy)
        o = {"objectgoal": np.array([self.target], dtype=np.int64),
             "gps": np.array([F(F(dx * c) + F(dy * s)), F(F(c * dy) - F(s * dx))], dtype=np.float32),
             "compass": np.array([self.compass[(self.h - self.h0) % self.nh]], dtype=np.float32)}
        if self.use_rgb or self.use_depth or self.use_semantic:
            r = render(self.px, self.py, self.h, w.rects, w.colors, self.objects, self.cats, self.ray, self.cosf, self.tanv,
                       self.use_rgb, self.use_depth, self.use_semantic)
            seen = set(int(x) - HIT_OBJECT for x in np.unique(r.pop("hit")) if x >= HIT_OBJECT)
            self.counters["objects_visible"] += len(seen)
            hc, hs = (float(v) for v in self.dirs[self.h])
            for j, (ox, oy) in enumerate(self.objects):     # in the field of view, in no column, a rectangle in between
                vx, vy = float(ox) - float(self.px), float(oy) - float(self.py)
                ahead, side = vx * hc + vy * hs, hc * vy - hs * vx
                if j not in seen and ahead > 0 and abs(side) < ahead and any(
                        _segment_crosses_rect(float(self.px), float(self.py), float(ox), float(oy), rc) for rc in w.rects):
                    self.counters["objects_hidden"] += 1
            o.update(r)
        return o

    def step(self, action):
        a = int(action)
        if a < 0 or a >= self.num_actions:
            raise ValueError(f"action {action!r} outside 0..{self.num_actions - 1}")
        w, cnt = self.world, self.counters
        if a == MOVE_FORWARD:
            c, s = self.dirs[self.h]
            nx, ny = F(self.px + F(R.FORWARD * c)), F(self.py + F(R.FORWARD * s))   # multiply, then a separate add
            if is_free(nx, ny, w.rects, self.objects):
                self.px, self.py, self.path = nx, ny, F(self.path + R.FORWARD)
            else:
                self.collisions += 1
                inside = nx >= LO and nx <= HI and ny >= LO and ny <= HI
                cnt["blocked_wall" if not inside else ("blocked_rect" if not R.is_free(nx, ny, w.rects) else "blocked_object")] += 1
        elif a == TURN_LEFT:
            self.h = (self.h + 1) % self.nh
        elif a == TURN_RIGHT:
            self.h = (self.h + self.nh - 1) % self.nh
        else:
            cnt["looks"] += int(a >= LOOK_UP)
        # from here on Nav2D-v0's end of a step with the distance to the nearest instance and the 1 m success radius
        d, idx = nearest_target(self.px, self.py, self.objects, self.cats, self.target)
        cnt["nearest_changes"] += int(idx != self.nearest)
        self.nearest = idx
        success = a == STOP and d < SUCCESS_DIST
        cnt["stop_too_far"] += int(a == STOP and not success)
        reward = F(F(R.SLACK + F(self.d_prev - d)) + (R.SUCCESS_REWARD if success else F(0.0)))
        self.d_prev = d
        self.steps += 1
        done = a == STOP or self.steps >= self.max_steps
        self.ended = int(done)
        info = {}
        if done:
            spl = F(self.d_start / max(self.d_start, self.path)) if success else F(0.0)
            info = dict(success=float(success), spl=float(spl), distance_to_goal=float(d), collisions=float(self.collisions))
            self.last_measures = [F(info[k]) for k in MEASURES]
            self.last = dict(d_start=self.d_start, d_end=d, length=self.steps, success=bool(success))
            for k in MEASURES:
                self.sums[k] = F(self.sums[k] + F(info[k]))
            cnt["episodes"] += 1
            cnt["successes"] += int(success)
            cnt["timeouts"] += int(a != STOP)
            self.episode += 1
            self._begin()
        return self.observe(), reward, done, info

    def state_words(self):
        """The named words of the device record (include/habitat_amd.h), as a dict of numpy scalars / arrays."""
        gx, gy = self.objects[self.nearest]
        obj = np.zeros((MAX_OBJECTS, 2), np.float32)
        obj[:self.M] = np.array(self.objects, dtype=np.float32)
        cat = np.full(MAX_OBJECTS, -1, np.int32)
        cat[:self.M] = self.cats
        return dict(pos=np.array([self.px, self.py, gx, gy], np.float32),
                    ints=np.array([self.h, self.steps, self.collisions, self.episode, self.ended], np.int32),
                    last=np.array(self.last_measures, np.float32), start=np.array([self.sx, self.sy], np.float32),
                    start_heading_target=np.array([self.h0, self.target], np.int32), objects=obj, categories=cat)


def greedy_action(e, turn_angle):
    """The scripted controller.  It reads the world directly (the task has no goal vector): STOP inside the success radius, turn
    towards the nearest instance of the target until it is within half a turn, else go forward."""
    d, idx = nearest_target(e.px, e.py, e.objects, e.cats, e.target)
    if d < SUCCESS_DIST:
        return STOP
    ox, oy = e.objects[idx]
    c, s = (float(v) for v in e.dirs[e.h])
    dx, dy = float(ox) - float(e.px), float(oy) - float(e.py)
    phi = math.atan2(c * dy - s * dx, dx * c + dy * s)
    if abs(phi) <= math.radians(turn_angle) / 2.0:
        return MOVE_FORWARD
    return TURN_LEFT if phi > 0 else TURN_RIGHT


# ---- scripted rollouts shared by the host and the GPU tests --------------------------------------------------------------------
SCRIPTS = R.SCRIPTS   # forward, greedy, never_stop, random


def rollout(kind, seed, num_envs, steps, turn_angle=10, rng_seed=0, **env_kw):
    """As nav2d_reference.rollout; additionally `states[t][n]` = state_words() after the reset (t = 0) and after every step."""
    envs = [Nav2DObjEnv(seed, n, turn_angle=turn_angle, **env_kw) for n in range(num_envs)]
    na = envs[0].num_actions
    rng = np.random.RandomState(rng_seed)
    obs = [[e.reset() for e in envs]]
    out = dict(actions=np.zeros((steps, num_envs), np.int64), rewards=np.zeros((steps, num_envs), np.float32),
               dones=np.zeros((steps, num_envs), bool), infos=[], sums=np.zeros((steps, len(MEASURES), num_envs), np.float32),
               states=[[e.state_words() for e in envs]])
    for t in range(steps):
        if kind == "forward":
            a = [MOVE_FORWARD] * num_envs
        elif kind == "greedy":
            a = [greedy_action(e, turn_angle) for e in envs]
        elif kind == "never_stop":
            a = list(rng.randint(1, na, size=num_envs))
        elif kind == "random":
            a = list(rng.randint(0, na, size=num_envs))
        else:
            raise ValueError(kind)
        res = [e.step(x) for e, x in zip(envs, a)]
        out["actions"][t] = a
        obs.append([r[0] for r in res])
        out["rewards"][t] = [r[1] for r in res]
        out["dones"][t] = [r[2] for r in res]
        out["infos"].append([r[3] for r in res])
        out["sums"][t] = [[e.sums[k] for e in envs] for k in MEASURES]
        out["states"].append([e.state_words() for e in envs])
    out["obs"] = obs
    out["counters"] = {k: sum(e.counters[k] for e in envs) for k in envs[0].counters}
    out["envs"] = envs
    return out


# The scripted runs tests/test_gpu_nav2d_obj.py holds the kernels to: shapes as nav2d_reference's SCRIPT_*, every combination of
# K in {0, 3, 8}, turn in {10, 30}, M in {1, 3, 8}, C in {1, 4}; six actions where M is odd, four where it is even (M = 8).
# tests/test_nav2d_obj_host.py asserts that over these runs every event the scripts are there for happens; the seeds are the first of
# 1, 2, ... at which that holds.
SCRIPT_ENVS, SCRIPT_STEPS, SCRIPT_MAX_EPISODE_STEPS = R.SCRIPT_ENVS, R.SCRIPT_STEPS, R.SCRIPT_MAX_EPISODE_STEPS
SCRIPT_CASES = [(K, turn, M, C) for K in (0, 3, 8) for turn in (10, 30) for M in (1, 3, 8) for C in (1, 4)]


def script_seed(kind, case=None):
    return 1


def script_rollout(kind, case, H=0, W=0, **kw):
    K, turn, M, C = case
    return rollout(kind, script_seed(kind, case), SCRIPT_ENVS, SCRIPT_STEPS, turn_angle=turn, num_obstacles=K, num_objects=M,
                   num_categories=C, num_actions=4 if M == 8 else 6, max_episode_steps=SCRIPT_MAX_EPISODE_STEPS, H=H, W=W, **kw)
