"""Plain-numpy restatement of the Nav2DExplore-v0 task (habitat_amd/common/env_factory.py: Nav2DExploreVectorEnv), shared by
tests/test_nav2d_explore_host.py and tests/test_gpu_nav2d_explore.py.  This file is the specification: `nav2d_explore_step_kernel` and
the markerless form of `nav2d_render_kernel` (habitat-lab_amd/csrc/nav2d.hip) reproduce every output bit for bit -- no angle function
runs on the device, every written operation is one float32 rounding, no fused multiply-add, and the count of new cells is an integer.

World, physics and controls are Nav2D-v0's (tests/nav2d_reference.py, imported, not restated): the arena, K <= 8 rectangles, the start,
the heading table, `is_free`, the 0.25 m forward step, turns of turn_angle, the collision count and streams 16-20.  There is no goal:
the record's (gx, gy) are 0.  Discrete(4) in habitat's order; the geodesic distance mode does not exist.

Coverage layer.  uint8 (G, G) per env, G = coverage_resolution in 16..512 (default 64), in the cell geometry of
  tests/nav2d_map_reference.py (`cell_size`, `centres`: row 0 on top).  A cell becomes seen by exactly that file's `reveal` with
  vis_dist = visibility_dist (a positive finite float32, default 3.0); `reveal`, `centres`, `occupied` and `cell_size` are imported.
Beginning of an episode.  The layer is cleared; free_cells = the unoccupied cell centres; the first reveal from the start pose earns
  nothing; seen_cells = the count after it; the start pose (sx, sy, h0) is recorded for gps and compass.
One step.  Nav2D-v0's discrete move (STOP moves nothing); the reveal from the new pose, new = the cells it turned from 0 to 1;
  reward = fl(-0.01f + fl(rc * (float)new)) with rc = float32(coverage_reward * float64(cell) ** 2), coverage_reward finite and >= 0
  per square metre (default 0.1); the step count goes up; the episode ends on STOP or at max_episode_steps, without a bonus.  On an
  end the measures go into the sums, the next episode begins as above and the observations are the new episode's.
Measures.  coverage = fl((float)seen_cells / (float)free_cells); area_seen = fl(fl(cell * cell) * (float)seen_cells); collisions;
  num_steps.
Sensors.  rgb (optional), depth: Nav2D-v0's geometry with nothing drawn beyond it (Nav2DObj-v0's render without objects); gps (2,)
  and compass (1,): Nav2DObj-v0's expressions and host table.  Nothing is rendered when neither image is asked for."""
from __future__ import annotations

import functools

import numpy as np

import nav2d_map_reference as M
import nav2d_obj_reference as O
import nav2d_reference as R
from nav2d_map_reference import cell_size, centres, occupied, reveal
from nav2d_reference import F

MEASURES = ("coverage", "area_seen", "collisions", "num_steps")
MIN_RESOLUTION, MAX_RESOLUTION = 16, 512
STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT = range(4)
SLACK = F(-0.01)
TASK_EXPLORE = 4                      # the top-down map's task code: no marker, no overlay beyond the agent and its tick
STATE_WORDS = 62                      # a Nav2D-v0 record (56 words), then the six below
W_START_X, W_START_Y, W_START_HEADING, W_FREE_CELLS, W_SEEN_CELLS, W_LAST_NEW = 56, 57, 58, 59, 60, 61


def check_parameters(coverage_resolution, visibility_dist, coverage_reward, num_actions):
    number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
    G = coverage_resolution
    if not isinstance(G, (int, np.integer)) or isinstance(G, bool) or not MIN_RESOLUTION <= G <= MAX_RESOLUTION:
        raise ValueError(f"coverage_resolution {G!r} must be a whole number in {MIN_RESOLUTION}..{MAX_RESOLUTION}")
    with np.errstate(over="ignore"):
        if not number(visibility_dist) or not np.isfinite(F(visibility_dist)) or not F(visibility_dist) > 0:
            raise ValueError(f"visibility_dist {visibility_dist!r} must be a positive finite float32")
        if not number(coverage_reward) or not np.isfinite(F(coverage_reward)) or not float(coverage_reward) >= 0:
            raise ValueError(f"coverage_reward {coverage_reward!r} must be finite and >= 0")
    if num_actions != 4:
        raise ValueError(f"num_actions {num_actions!r} is not 4")


def reward_per_cell(coverage_reward, G):
    """rc: float64 coverage_reward * cell ** 2, rounded once."""
    return F(float(coverage_reward) * float(cell_size(G)) ** 2)


def view(e):
    """What `reveal` and the top-down map read of the env: no markers and no moving thing."""
    v = M.View()
    v.px, v.py, v.episode, v.rects = F(e.px), F(e.py), int(e.episode), [tuple(F(a) for a in r) for r in e.world.rects]
    v.c, v.s = (F(a) for a in e.dirs[e.h])
    v.markers, v.thing = [], None
    return v


class Nav2DExploreEnv(R.Nav2DEnv):
    """One env, the interface of nav2d_reference.Nav2DEnv.  obs holds 'gps', 'compass' and, when asked, 'rgb' / 'depth'; `layer` is
    the coverage layer; `record()` is the device record of this env."""

    def __init__(self, seed, env, H=0, W=0, coverage_resolution=64, visibility_dist=3.0, coverage_reward=0.1, num_actions=4,
                 turn_angle=10, **kw):
        check_parameters(coverage_resolution, visibility_dist, coverage_reward, num_actions)
        super().__init__(seed, env, H=H, W=W, turn_angle=turn_angle, **kw)
        self.G, self.vis = int(coverage_resolution), float(F(visibility_dist))
        self.cell, self.rc = cell_size(self.G), reward_per_cell(coverage_reward, self.G)
        self.compass = O.compass_table(turn_angle)
        self.layer = np.zeros((self.G, self.G), np.uint8)
        self.sums = {k: F(0.0) for k in MEASURES}
        self.counters = dict(episodes=0, stops=0, timeouts=0, collisions=0, steps_new=0, steps_nothing_new=0, first_reveals_differ=0)
        self.ended, self.last_new, self.last_measures, self.first_reveal = 0, 0, [F(0.0)] * 4, None

    def _begin_layer(self):
        """Steps 1-5 of the beginning of an episode, from the current pose."""
        X, Y = centres(self.G)
        self.layer[...] = 0
        self.free_cells = int(np.count_nonzero(~occupied(X, Y, view(self).rects)))
        reveal(self.layer, view(self), self.G, self.vis)
        self.seen_cells = int(self.layer.sum())
        self.sx, self.sy, self.h0 = self.px, self.py, self.h
        if self.first_reveal is not None:
            self.counters["first_reveals_differ"] += int(not np.array_equal(self.first_reveal, self.layer))
        self.first_reveal = self.layer.copy()

    def _begin(self):
        w = self.world = R.make_world(self.seed, self.env, self.episode, self.K, self.nh, self.candidates)
        self.px, self.py, self.h = w.sx, w.sy, w.h
        self.path, self.steps, self.collisions = F(0.0), 0, 0
        self._begin_layer()

    def place(self, rects, px, py, h):
        """A hand-made world: these raw rectangles and this pose, from which an episode begins."""
        w = self.world
        w.rects = [tuple(F(a) for a in r) for r in rects]
        w.colors = [(64 + k, 96, 128) for k in range(len(rects))]
        self.K, self.px, self.py, self.h = len(rects), F(px), F(py), int(h)
        self.path, self.steps, self.collisions = F(0.0), 0, 0
        self.first_reveal = None
        self._begin_layer()

    def reset(self):
        self.ended, self.last_new, self.last_measures, self.first_reveal = 0, 0, [F(0.0)] * 4, None
        return super().reset()

    def observe(self):
        w = self.world
        c, s = self.dirs[self.h0]
        dx, dy = F(self.px - self.sx), F(self.py - self.sy)
        o = {"gps": np.array([F(F(dx * c) + F(dy * s)), F(F(c * dy) - F(s * dx))], dtype=np.float32),
             "compass": np.array([self.compass[(self.h - self.h0) % self.nh]], dtype=np.float32)}
        if self.use_rgb or self.use_depth:
            r = O.render(self.px, self.py, self.h, w.rects, w.colors, [], [], self.ray, self.cosf, self.tanv, self.use_rgb,
                         self.use_depth, False)
            r.pop("hit")
            o.update(r)
        return o

    def step(self, action):
        a = int(action)
        if a < 0 or a > 3:
            raise ValueError(f"action {action!r} outside 0..3")
        w, cnt = self.world, self.counters
        if a == MOVE_FORWARD:
            c, s = self.dirs[self.h]
            nx, ny = F(self.px + F(R.FORWARD * c)), F(self.py + F(R.FORWARD * s))   # multiply, then a separate add
            if R.is_free(nx, ny, w.rects):
                self.px, self.py, self.path = nx, ny, F(self.path + R.FORWARD)
            else:
                self.collisions += 1
                cnt["collisions"] += 1
        elif a == TURN_LEFT:
            self.h = (self.h + 1) % self.nh
        elif a == TURN_RIGHT:
            self.h = (self.h + self.nh - 1) % self.nh
        before = self.layer.copy()
        reveal(self.layer, view(self), self.G, self.vis)
        new = int(np.count_nonzero((before == 0) & (self.layer == 1)))
        reward = F(SLACK + F(self.rc * F(new)))
        self.seen_cells += new
        self.last_new = new
        cnt["steps_new" if new else "steps_nothing_new"] += 1
        self.steps += 1
        done = a == STOP or self.steps >= self.max_steps
        self.ended = int(done)
        info = {}
        if done:
            info = dict(coverage=float(F(F(self.seen_cells) / F(self.free_cells))),
                        area_seen=float(F(F(self.cell * self.cell) * F(self.seen_cells))), collisions=float(self.collisions),
                        num_steps=float(self.steps))
            self.last_measures = [F(info[k]) for k in MEASURES]
            for k in MEASURES:
                self.sums[k] = F(self.sums[k] + F(info[k]))
            cnt["episodes"] += 1
            cnt["stops" if a == STOP else "timeouts"] += 1
            self.episode += 1
            self._begin()
        return self.observe(), reward, done, info

    def record(self):
        """The device record (include/habitat_amd.h: a Nav2D-v0 record, then HAB_NAV2D_EXPLORE_W_*) as 62 int32 words."""
        f = np.zeros(STATE_WORDS, np.float32)
        i = f.view(np.int32)
        f[0:2] = [self.px, self.py]                                    # (gx, gy), d_prev and d_start stay 0
        f[6] = self.path
        i[7:12] = [self.h, self.steps, self.collisions, self.episode, self.ended]
        f[12:16] = self.last_measures
        for k, (r, c) in enumerate(zip(self.world.rects, self.world.colors)):
            f[16 + 4 * k:20 + 4 * k] = r
            i[48 + k] = c[0] | c[1] << 8 | c[2] << 16
        f[W_START_X:W_START_Y + 1] = [self.sx, self.sy]
        i[W_START_HEADING:] = [self.h0, self.free_cells, self.seen_cells, self.last_new]
        return i.copy()


# ---- scripted rollouts shared by the host and the GPU tests --------------------------------------------------------------------
SCRIPTS = ("forward", "never_stop", "random")


def rollout(kind, seed, num_envs, steps, rng_seed=0, **env_kw):
    """As nav2d_reference.rollout; additionally records[t] (N, 62) int32 and layers[t] (N, G, G) after the reset (t = 0) and after
    every step, and news (steps, N), the cells each step saw first.  'forward' only moves forward, 'never_stop' draws from the three
    moving actions, 'random' from all four."""
    envs = [Nav2DExploreEnv(seed, n, **env_kw) for n in range(num_envs)]
    rng = np.random.RandomState(rng_seed)
    obs = [[e.reset() for e in envs]]
    out = dict(actions=np.zeros((steps, num_envs), np.int64), rewards=np.zeros((steps, num_envs), np.float32),
               dones=np.zeros((steps, num_envs), bool), infos=[], sums=np.zeros((steps, len(MEASURES), num_envs), np.float32),
               news=np.zeros((steps, num_envs), np.int64), records=[np.stack([e.record() for e in envs])],
               layers=[np.stack([e.layer for e in envs])])
    for t in range(steps):
        if kind == "forward":
            a = [MOVE_FORWARD] * num_envs
        elif kind == "never_stop":
            a = list(rng.randint(1, 4, size=num_envs))
        elif kind == "random":
            a = list(rng.randint(0, 4, size=num_envs))
        else:
            raise ValueError(kind)
        res = [e.step(x) for e, x in zip(envs, a)]
        out["actions"][t] = a
        obs.append([r[0] for r in res])
        out["rewards"][t] = [r[1] for r in res]
        out["dones"][t] = [r[2] for r in res]
        out["infos"].append([r[3] for r in res])
        out["sums"][t] = [[e.sums[k] for e in envs] for k in MEASURES]
        out["news"][t] = [e.last_new for e in envs]
        out["records"].append(np.stack([e.record() for e in envs]))
        out["layers"].append(np.stack([e.layer for e in envs]))
    out["obs"] = obs
    out["counters"] = {k: sum(e.counters[k] for e in envs) for k in envs[0].counters}
    out["envs"] = envs
    return out


# The scripted runs tests/test_gpu_nav2d_explore.py holds the kernels to: nav2d_reference's shapes (5 envs, 60 steps, episodes of 12
# steps) at every K in {0, 3, 8} and turn in {10, 30}.  The layer's shape, the visibility and the image size go round the FORMS, so
# that every one of them occurs; 30 makes the rows straddle the words of the sweep.  tests/test_nav2d_explore_host.py asserts that
# the three scripts of every case together show every event they are there for; the seeds are the first of 1, 2, ... at which
# that holds.
SCRIPT_ENVS, SCRIPT_STEPS, SCRIPT_MAX_EPISODE_STEPS = R.SCRIPT_ENVS, R.SCRIPT_STEPS, R.SCRIPT_MAX_EPISODE_STEPS
SCRIPT_CASES = [(K, turn) for K in (0, 3, 8) for turn in (10, 30)]
FORMS = [(G, vis, size) for G in (16, 30, 64) for vis in (1.0, 3.0) for size in ((12, 20), (9, 18))]
SCRIPT_EVENTS = ("stops", "timeouts", "collisions", "steps_new", "steps_nothing_new", "first_reveals_differ")


def script_seed(kind, case=None):
    return 1


def script_form(kind, case):
    """The (G, visibility_dist, (H, W)) of one scripted run: the forms in turn over the cases and their scripts."""
    return FORMS[(SCRIPT_CASES.index(case) * len(SCRIPTS) + SCRIPTS.index(kind)) % len(FORMS)]


@functools.lru_cache(maxsize=None)
def script_rollout(kind, case, images=True):
    K, turn = case
    G, vis, (H, W) = script_form(kind, case)
    return rollout(kind, script_seed(kind, case), SCRIPT_ENVS, SCRIPT_STEPS, turn_angle=turn, num_obstacles=K, coverage_resolution=G,
                   visibility_dist=vis, max_episode_steps=SCRIPT_MAX_EPISODE_STEPS, H=H if images else 0, W=W if images else 0)


# ---- the top-down map of the task (tests/nav2d_map_reference.py's update and frame, on this task's view) ---------------------------
class MapOf:
    """Keeps the maps of restated envs the way Nav2DVectorEnv._launch does: `begin()` after a reset, `after_step(dones, mask)` after
    a step; `map`, `fog` (N, S, S) and `rec` (N, 8) afterwards."""

    def __init__(self, envs, S, vis_dist):
        self.envs, self.S, self.vis = envs, S, vis_dist
        n = len(envs)
        self.map, self.fog = np.zeros((n, S, S), np.uint8), np.zeros((n, S, S), np.uint8)
        self.rec = np.zeros((n, M.REC_WORDS), np.int32)

    def begin(self):
        for n, e in enumerate(self.envs):
            M.update(self.map[n], self.fog[n], self.rec[n], view(e), self.S, self.vis, True)

    def after_step(self, dones, mask=None):
        for n, e in enumerate(self.envs):
            if mask is None or mask[n]:
                M.update(self.map[n], self.fog[n], self.rec[n], view(e), self.S, self.vis, bool(dones[n]))

    def frames(self, Hf, obs, use_rgb, use_depth, draw_fog=True):
        return np.stack([M.frame(self.map[n], self.fog[n], view(e), self.S, Hf, obs[n]["rgb"] if use_rgb else None,
                                 obs[n]["depth"] if use_depth else None, draw_fog) for n, e in enumerate(self.envs)])
