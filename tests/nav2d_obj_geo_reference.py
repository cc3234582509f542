"""Plain-numpy restatement of the geodesic distance mode of Nav2DObj-v0 (habitat_amd/common/env_factory.py: Nav2DObjVectorEnv with
`distance="geodesic"`), shared by tests/test_nav2d_obj_geo_host.py and tests/test_gpu_nav2d_obj_geo.py.  This file is the
specification `nav2d_obj_geo_build_kernel` and `nav2d_obj_geo_step_kernel` (habitat-lab_amd/csrc/nav2d.hip) are held to: every float
operation below is one float32 rounding, no fused multiply-add, in the written order.  World, objects, target, physics, sensors and
render are those of tests/nav2d_obj_reference.py; boxes, the visibility test and `dist` are those of tests/nav2d_geo_reference.py.
Only the d of the reward, the success test (STOP and d < 1.0), `distance_to_goal` and d_start / the SPL numerator change: d is the
shortest path round the obstacles to the nearest instance of the target category.

Boxes.  The K rectangles grown by the agent radius (nav2d_geo_reference.inflated), then for object m the axis-aligned square
  [ox - 0.4, ox + 0.4] x [oy - 0.4, oy + 0.4], the bounding square of the keep-out disc of radius OBJ_BLOCK: up to 16 boxes.  The
  visibility boxes are these shrunk by E = 2^-10 m with the same expressions (lx = X0 + E, ..., hy = Y1 - E), and visible(a, b) is
  nav2d_geo_reference.visible over them.  The square over-approximates the disc, so every path of the boxed world is a path of the
  real one (up to E at the four tangent points).
Nodes.  64.  Node 4k + j is corner j of rectangle box k, node 32 + 4m + j corner j of object m's square, both in the order
  (X0, Y0), (X1, Y0), (X0, Y1), (X1, Y1).  A node is valid iff nav2d_obj_reference.is_free holds for it (arena, rectangles, discs).
Targets.  The centres of all objects of the target category.  The square of object t does not block a segment that ends at centre
  t; only that box is left out, and only for that segment.
Field.  D[i] = +inf for invalid nodes; else the least rounded path sum from node i to any target centre: the last hop is the min
  over the target centres the node sees of dist(node, centre), then Jacobi sweeps D <- min(D, min_j fl(w[i][j] + D[j])) until one
  changes nothing; the sweep count includes that one and is capped at 4 (K + M).
Query.  geo(p) = min(dist(p, c_t) over the target centres p sees, own box ignored; fl(dist(p, node_i) + D[i]) over the nodes with
  finite D that p sees); +inf if p sees none.  A position in the sliver between a disc and its square sees nothing through that
  box: a lost step, unless it is the target's own sliver, where the centre is seen.
Episode.  As nav2d_geo_reference: the field is built at the beginning, g0 = geo(start).  g0 finite: d_start = d_prev = g0, every
  step's d is geo(p), and where that is +inf d = d_prev and the lost-step counter goes up.  g0 infinite: the episode keeps the
  Euclidean nearest-centre distance throughout.  (gx, gy) stay the Euclidean-nearest centre in both modes.
Field record (HAB_NAV2D_OBJ_GEO_BYTES = 288): words 0..63 D, 64 reachable, 65 sweeps, 66 lost steps, 67..71 zero."""
from __future__ import annotations

import math

import numpy as np

import nav2d_geo_reference as G
import nav2d_obj_reference as O
import nav2d_reference as R
from nav2d_geo_reference import E, dist_v, visible
from nav2d_obj_reference import OBJ_BLOCK, STOP, MOVE_FORWARD, TURN_LEFT, TURN_RIGHT, LOOK_UP
from nav2d_reference import F, INF, MEASURES, dist

NODES, RECT_NODES = 64, 4 * R.MAX_OBSTACLES
GEO_WORDS, W_REACHABLE, W_SWEEPS, W_LOST = 72, 64, 65, 66
GEO_EVENTS = ("unreachable", "detours", "lost_steps", "waypoint_changes", "rebuilds")


def target_index(t):
    """The waypoint index that stands for the centre of object t (negative, so no node)."""
    return -1 - t


def object_squares(objects):
    return [(F(ox - OBJ_BLOCK), F(oy - OBJ_BLOCK), F(ox + OBJ_BLOCK), F(oy + OBJ_BLOCK)) for ox, oy in objects]


def boxes(rects, objects):
    """The K grown rectangles, then the M squares."""
    return G.inflated(rects) + object_squares(objects)


def visibility_boxes(rects, objects):
    return [(F(X0 + E), F(Y0 + E), F(X1 - E), F(Y1 - E)) for X0, Y0, X1, Y1 in boxes(rects, objects)]


def nodes(rects, objects):
    """(x (64,), y (64,), valid (64,)); the nodes of k >= K and m >= M are (0, 0, False)."""
    x, y, ok = np.zeros(NODES, np.float32), np.zeros(NODES, np.float32), np.zeros(NODES, bool)
    for first, group in ((0, G.inflated(rects)), (RECT_NODES, object_squares(objects))):
        for k, (X0, Y0, X1, Y1) in enumerate(group):
            for j, (cx, cy) in enumerate(((X0, Y0), (X1, Y0), (X0, Y1), (X1, Y1))):
                i = first + 4 * k + j
                x[i], y[i], ok[i] = cx, cy, O.is_free(cx, cy, rects, objects)
    return x, y, ok


class Field:
    """The graph and the field of one world: what hab_nav2d_obj_geo_build computes, and the queries on it."""

    def __init__(self, rects, objects, cats, target, order="jacobi"):
        self.K, self.M = len(rects), len(objects)
        self.objects = [(F(ox), F(oy)) for ox, oy in objects]
        self.targets = [t for t in range(self.M) if cats[t] == target]
        self.vb = visibility_boxes(rects, objects)
        self.vb_without = {t: self.vb[:self.K + t] + self.vb[self.K + t + 1:] for t in self.targets}
        self.x, self.y, self.ok = nodes(rects, objects)
        x, y, ok = self.x, self.y, self.ok
        see = visible(x[:, None], y[:, None], x[None, :], y[None, :], self.vb) & ok[:, None] & ok[None, :] & ~np.eye(NODES, dtype=bool)
        self.w = np.where(see, dist_v(x[:, None], y[:, None], x[None, :], y[None, :]), INF).astype(np.float32)
        D = np.full(NODES, INF, np.float32)
        for t in self.targets:
            cx, cy = self.objects[t]
            hop = np.where(ok & visible(x, y, cx, cy, self.vb_without[t]), dist_v(x, y, cx, cy), INF).astype(np.float32)
            D = np.minimum(D, hop)
        self.last_hop = D.copy()
        sweeps = 0
        while sweeps < 4 * (self.K + self.M):
            sweeps += 1
            if order == "jacobi":
                new = np.minimum(D, (self.w + D[None, :]).min(1))
            else:
                new = D.copy()
                for i in range(NODES):
                    new[i] = min(new[i], (self.w[i] + new).min())
            changed = not np.array_equal(new, D)
            D = new.astype(np.float32)
            if not changed:
                break
        self.D, self.sweeps = D, sweeps

    def candidates(self, px, py):
        """[(index, value)]: target_index(t) with dist(p, c_t) for the target centres p sees, then every node with finite D p sees."""
        px, py, out = F(px), F(py), []
        for t in self.targets:
            cx, cy = self.objects[t]
            if visible(px, py, cx, cy, self.vb_without[t]):
                out.append((target_index(t), dist(px, py, cx, cy)))
        see = np.isfinite(self.D) & visible(px, py, self.x, self.y, self.vb)
        v = (dist_v(px, py, self.x, self.y) + self.D).astype(np.float32)
        return out + [(int(i), v[i]) for i in np.nonzero(see)[0]]

    def geo(self, px, py):
        best = INF
        for _, v in self.candidates(px, py):
            if v < best:
                best = v
        return best

    def waypoint(self, px, py):
        """-> (index, x, y): the first node of the shortest path from p, target_index(t) for a centre.  The first among equal values
        wins (centres come first); nodes equal to p are skipped; None if p sees nothing."""
        best = None
        for i, v in self.candidates(px, py):
            if i >= 0 and self.x[i] == px and self.y[i] == py:
                continue
            if best is None or v < best[1]:
                best = (i, v)
        if best is None:
            return None
        i = best[0]
        return (i,) + (self.objects[-1 - i] if i < 0 else (self.x[i], self.y[i]))


class Nav2DObjGeoEnv(O.Nav2DObjEnv):
    """Nav2DObj-v0 in geodesic mode; the interface of nav2d_obj_reference.Nav2DObjEnv."""

    def __init__(self, seed, env, **kw):
        super().__init__(seed, env, **kw)
        self.counters.update({k: 0 for k in GEO_EVENTS})

    def _begin(self):
        super()._begin()
        self.build()

    def build(self):
        """The field of the current world and g0 of the current position; what hab_nav2d_obj_geo_build does to one env."""
        self.field = Field(self.world.rects, self.objects, self.cats, self.target)
        g0 = self.field.geo(self.px, self.py)
        self.reachable, self.lost_steps = bool(np.isfinite(g0)), 0
        straight, _ = O.nearest_target(self.px, self.py, self.objects, self.cats, self.target)
        if self.reachable:
            self.d_start = self.d_prev = g0
        self.counters["rebuilds"] += 1
        self.counters["unreachable"] += int(not self.reachable)
        self.counters["detours"] += int(self.reachable and float(g0) > 1.02 * float(straight))

    def begin_with(self, rects, objects, cats, target, sx, sy, h=0):
        """A hand-made world (tests) in the generated one's place."""
        w = R.World()
        w.rects, w.colors = [tuple(F(v) for v in r) for r in rects], [(64, 64, 64)] * len(rects)
        w.sx, w.sy, w.gx, w.gy, w.h, w.start_fallback, w.goal_fallback = F(sx), F(sy), F(7.5), F(7.5), int(h), False, False
        self.world, self.K = w, len(rects)
        self.objects, self.cats, self.target, self.M = [(F(x), F(y)) for x, y in objects], list(cats), int(target), len(objects)
        self.px, self.py, self.h = w.sx, w.sy, w.h
        self.sx, self.sy, self.h0 = w.sx, w.sy, w.h
        d, self.nearest = O.nearest_target(self.px, self.py, self.objects, self.cats, self.target)
        self.d_start = self.d_prev = d
        self.path, self.steps, self.collisions = F(0.0), 0, 0
        self.build()
        return self.observe()

    def field_record(self):
        rec = np.zeros(GEO_WORDS, np.int32)
        rec[:NODES] = self.field.D.view(np.int32)
        rec[W_REACHABLE], rec[W_SWEEPS], rec[W_LOST] = int(self.reachable), self.field.sweeps, self.lost_steps
        return rec

    def geo_here(self):
        return self.field.geo(self.px, self.py)

    def waypoint_here(self):
        return self.field.waypoint(self.px, self.py) if self.reachable else None

    def step(self, action):
        a = int(action)
        if a < 0 or a >= self.num_actions:
            raise ValueError(f"action {action!r} outside 0..{self.num_actions - 1}")
        w, cnt = self.world, self.counters
        if a == MOVE_FORWARD:
            c, s = self.dirs[self.h]
            nx, ny = F(self.px + F(R.FORWARD * c)), F(self.py + F(R.FORWARD * s))
            if O.is_free(nx, ny, w.rects, self.objects):
                self.px, self.py, self.path = nx, ny, F(self.path + R.FORWARD)
            else:
                self.collisions += 1
                inside = nx >= R.LO and nx <= R.HI and ny >= R.LO and ny <= R.HI
                cnt["blocked_wall" if not inside else ("blocked_rect" if not R.is_free(nx, ny, w.rects) else "blocked_object")] += 1
        elif a == TURN_LEFT:
            self.h = (self.h + 1) % self.nh
        elif a == TURN_RIGHT:
            self.h = (self.h + self.nh - 1) % self.nh
        else:
            cnt["looks"] += int(a >= LOOK_UP)
        d, idx = O.nearest_target(self.px, self.py, self.objects, self.cats, self.target)
        cnt["nearest_changes"] += int(idx != self.nearest)
        self.nearest = idx
        if self.reachable:
            d = self.geo_here()
            if not np.isfinite(d):
                d = self.d_prev
                self.lost_steps += 1
                cnt["lost_steps"] += 1
        success = a == STOP and d < O.SUCCESS_DIST
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
            self.last = dict(d_start=self.d_start, d_end=d, length=self.steps, success=bool(success), path=self.path)
            for k in MEASURES:
                self.sums[k] = F(self.sums[k] + F(info[k]))
            cnt["episodes"] += 1
            cnt["successes"] += int(success)
            cnt["timeouts"] += int(a != STOP)
            self.episode += 1
            self._begin()
        return self.observe(), reward, done, info

    def state_words(self):
        """nav2d_obj_reference's named words and `dist` = (d_prev, d_start, path), words 4..6 of the record."""
        return dict(super().state_words(), dist=np.array([self.d_prev, self.d_start, self.path], np.float32))


# ---- scripts ------------------------------------------------------------------------------------------------------------------
def waypoint_action(e, turn_angle):
    """Steer to the first node of the shortest path; STOP at geo < 1.0.  Where the episode is unreachable or the position sees
    nothing, nav2d_obj_reference.greedy_action."""
    wp = e.waypoint_here()
    if wp is None:
        return O.greedy_action(e, turn_angle)
    last = getattr(e, "_wp", None)
    e.counters["waypoint_changes"] += int(last is not None and last[0] == e.episode and last[1] != wp[0])
    e._wp = (e.episode, wp[0])
    if float(e.geo_here()) < float(O.SUCCESS_DIST):
        return STOP
    _, phi = G.polar_to(e, wp[1], wp[2])
    if abs(phi) <= math.radians(turn_angle) / 2.0:
        return MOVE_FORWARD
    return TURN_LEFT if phi > 0 else TURN_RIGHT


SCRIPTS = O.SCRIPTS + ("waypoint",)


def rollout(kind, seed, num_envs, steps, turn_angle=10, rng_seed=0, **env_kw):
    """nav2d_obj_reference.rollout in geodesic mode, with the script 'waypoint' besides and, per step, `fields` (steps + 1, N, 72)
    int32: the field records, row 0 after the reset."""
    envs = [Nav2DObjGeoEnv(seed, n, turn_angle=turn_angle, **env_kw) for n in range(num_envs)]
    na = envs[0].num_actions
    rng = np.random.RandomState(rng_seed)
    obs = [[e.reset() for e in envs]]
    out = dict(actions=np.zeros((steps, num_envs), np.int64), rewards=np.zeros((steps, num_envs), np.float32),
               dones=np.zeros((steps, num_envs), bool), infos=[], sums=np.zeros((steps, len(MEASURES), num_envs), np.float32),
               fields=np.zeros((steps + 1, num_envs, GEO_WORDS), np.int32), states=[[e.state_words() for e in envs]])
    out["fields"][0] = [e.field_record() for e in envs]
    for t in range(steps):
        if kind == "forward":
            a = [MOVE_FORWARD] * num_envs
        elif kind == "greedy":
            a = [O.greedy_action(e, turn_angle) for e in envs]
        elif kind == "waypoint":
            a = [waypoint_action(e, turn_angle) for e in envs]
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
        out["fields"][t + 1] = [e.field_record() for e in envs]
        out["states"].append([e.state_words() for e in envs])
    out["obs"] = obs
    out["counters"] = {k: sum(e.counters[k] for e in envs) for k in envs[0].counters}
    out["envs"] = envs
    return out


# The scripted runs tests/test_gpu_nav2d_obj_geo.py holds the kernels to: nav2d_obj_reference's cases (K, turn, M, C; six actions where
# M is odd, four at M = 8), 5 envs x 60 steps.  Every script runs with an episode limit of 60; the drawn ones (no steering) run once
# more with nav2d_obj_reference's limit of 12, which gives every env several episode ends and field rebuilds.
# tests/test_nav2d_obj_geo_host.py asserts the conditions on these inputs (no unreachable world, lost steps under 5 % of each run's
# steps) and the events they are there for.  SCRIPT_SEED = 16 is the first of 1, 2, ... at which both conditions hold: at each of
# 1..15 some run has a script that walks into the sliver of an object that is no target and stays there (`forward`, `greedy` and the
# drawn scripts do not steer out of it), which loses 15 steps of the run's 300 or more.  The events hold at 16 as well.
SCRIPT_ENVS, SCRIPT_STEPS, SCRIPT_MAX_EPISODE_STEPS = O.SCRIPT_ENVS, O.SCRIPT_STEPS, 60
SHORT_EPISODE_STEPS = O.SCRIPT_MAX_EPISODE_STEPS
SCRIPT_SEED = 16
SCRIPT_CASES = O.SCRIPT_CASES
DRAWN = ("forward", "never_stop", "random")
SCRIPT_RUNS = [(k, SCRIPT_MAX_EPISODE_STEPS) for k in SCRIPTS] + [(k, SHORT_EPISODE_STEPS) for k in DRAWN]


def script_rollout(kind, case, limit=SCRIPT_MAX_EPISODE_STEPS, H=0, W=0, **kw):
    K, turn, M, C = case
    return rollout(kind, SCRIPT_SEED, SCRIPT_ENVS, SCRIPT_STEPS, turn_angle=turn, num_obstacles=K, num_objects=M, num_categories=C,
                   num_actions=4 if M == 8 else 6, max_episode_steps=limit, H=H, W=W, **kw)


# ---- hand-made worlds -----------------------------------------------------------------------------------------------------------
# Each: rects, objects, cats, target, start.
# The target inside nav2d_geo_reference's ring of rectangles: unreachable from outside, the episode stays Euclidean.
WALLED = dict(rects=G.RING, objects=[(4.0, 4.0), (6.5, 1.5)], cats=[0, 1], target=0, start=(1.0, 1.0))
# Object 0 (not the target) and object 1 (the target) far apart.  SLIVER_OTHER is a free position inside object 0's square, outside
# its disc: it sees nothing.  SLIVER_OWN is the same in the target's square: it sees the target's centre.
SLIVERS = dict(rects=[], objects=[(2.0, 2.0), (6.0, 6.0)], cats=[1, 0], target=0, start=(4.0, 1.0))
SLIVER_OTHER, SLIVER_OWN = (2.35, 2.35), (6.35, 6.35)
# Two instances of the target: object 0 is the nearer in a straight line, behind a long wall; object 1 is the nearer along a path.
DECOY = dict(rects=[(0.3, 3.0, 6.5, 3.4)], objects=[(2.0, 4.5), (6.0, 1.0)], cats=[0, 0], target=0, start=(2.0, 1.5))
# Object 0's square corner (X1, Y1) lies inside the grown rectangle: no node.
INSIDE = dict(rects=[(2.3, 2.3, 4.0, 4.0)], objects=[(1.9, 1.9), (6.0, 6.0)], cats=[1, 0], target=0, start=(1.0, 6.0))


def hand_made(world, **kw):
    e = Nav2DObjGeoEnv(1, 0, use_rgb=False, use_depth=False, use_semantic=False, num_objects=len(world["objects"]),
                       num_categories=max(world["cats"]) + 1, **kw)
    e.reset()
    e.begin_with(world["rects"], world["objects"], world["cats"], world["target"], *world["start"])
    return e
