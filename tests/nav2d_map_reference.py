"""Plain-numpy restatement of the top-down map of the Nav2D tasks, its fog of war and the video frame (habitat_amd/common/env_factory.py:
Nav2DVectorEnv, "Top-down map"), shared by tests/test_nav2d_map_host.py and tests/test_gpu_nav2d_map.py.  This file is the
specification `nav2d_map_update_kernel` and `nav2d_map_frame_kernel` (habitat-lab_amd/csrc/nav2d_map.hip) are held to: every float
operation below is one float32 rounding in the written order, nothing divides except the cell size 8 / S (one correctly rounded
division on the host), the rest is integer work, so the kernels reproduce every byte.

The map reads the tasks through their restated envs (nav2d_reference.py and its five siblings, imported, not edited): `view(task, e)`
picks out of an env object what the kernels read out of its record.  `MapRun` steps a list of such envs and keeps their maps the way
`Nav2DVectorEnv._launch` does: the step, then the update with the step's mask and `advance`."""
from __future__ import annotations

import functools

import numpy as np

import nav2d_geo_reference as G
import nav2d_obj_reference as O
import nav2d_rearr_reference as A
import nav2d_rearr_vel_reference as B
import nav2d_reference as R
import nav2d_social_reference as P
import nav2d_vel_reference as V

F = np.float32
HALF, ARENA = F(0.5), F(8.0)
MIN_RESOLUTION, MAX_RESOLUTION = 16, 512
OCCUPIED, FREE, START, TARGET, TRAJECTORY, OBJECT = 0, 1, 4, 6, 10, 16   # cell codes (habitat's where it has them)
CARRIED, PERSON, AGENT, TICK = 20, 21, 22, 23                               # the frame's overlays
START_R2, GOAL_R2, OBJ_R2, NEAR_R2 = F(0.15) * F(0.15), F(0.2) * F(0.2), F(0.3) * F(0.3), F(0.25) * F(0.25)
AGENT_R2, TICK_R2 = F(0.2) * F(0.2), F(0.08) * F(0.08)
TRAJ_W, TICK_LEN = F(0.75), F(0.45)
REC_WORDS, W_EPISODE, W_START_X, W_START_Y, W_PREV_X, W_PREV_Y = 8, 0, 1, 2, 3, 4
TASK_GOAL, TASK_OBJ, TASK_REARR, TASK_SOCIAL = 0, 1, 2, 3

_NONE = (255, 0, 255)   # a code without a meaning
COLORS = np.array([_NONE] * 32, dtype=np.uint8)
COLORS[[OCCUPIED, FREE, START, TARGET, TRAJECTORY, OBJECT, CARRIED, PERSON, AGENT, TICK]] = [
    (64, 64, 64), (200, 200, 200), (50, 50, 200), (255, 32, 32), (0, 160, 208), (240, 160, 32), (255, 200, 0), (200, 0, 200), (0, 160, 0),
    (0, 64, 0)]


# ---- the six tasks: the env class, its scripts and cases, the env keywords of a case, the map's task code ------------------------------
class Task:
    def __init__(self, name, module, cls, code, moving, turning, seed, env_kw):
        self.name, self.module, self.cls, self.code, self.moving, self.turning = name, module, cls, code, moving, turning
        self.scripts, self.cases, self.steps, self.envs = module.SCRIPTS, module.SCRIPT_CASES, module.SCRIPT_STEPS, module.SCRIPT_ENVS
        self.seed, self._env_kw = seed, env_kw

    def env_kw(self, case, limit=None):
        return dict(self._env_kw(case), max_episode_steps=self.module.SCRIPT_MAX_EPISODE_STEPS if limit is None else limit)

    def make_envs(self, kind, case, num_envs=None, limit=None, **kw):
        n = self.envs if num_envs is None else num_envs
        return [self.cls(self.seed(kind, case), i, **self.env_kw(case, limit), **kw) for i in range(n)]

    def actions(self, kind, case, num_envs=None, steps=None, limit=None):
        """The actions (steps, N, ...) that the task's own scripted rollout of `kind` takes at `case`."""
        out = self.module.rollout(kind, self.seed(kind, case), self.envs if num_envs is None else num_envs,
                                  self.steps if steps is None else steps, **self.env_kw(case, limit))
        return out["actions"], out["envs"]


def _vel_kw(case):
    K, (turn, max_turn, min_ang) = case
    return dict(turn_angle=turn, max_turn_angle=max_turn, min_abs_ang_speed=min_ang, num_obstacles=K)


def _obj_kw(case):
    K, turn, M, C = case
    return dict(turn_angle=turn, num_obstacles=K, num_objects=M, num_categories=C, num_actions=4 if M == 8 else 6)


TASKS = {
    "nav2d": Task("nav2d", R, R.Nav2DEnv, TASK_GOAL, "forward", "random", lambda kind, case: R.script_seed(kind, case[0]),
                  lambda case: dict(turn_angle=case[1], num_obstacles=case[0])),
    "vel": Task("vel", V, V.Nav2DVelEnv, TASK_GOAL, "forward", "random", lambda kind, case: V.script_seed(kind, case[0], case[1]), _vel_kw),
    "obj": Task("obj", O, O.Nav2DObjEnv, TASK_OBJ, "forward", "random", lambda kind, case: O.script_seed(kind, case), _obj_kw),
    "rearr": Task("rearr", A, A.Nav2DRearrEnv, TASK_REARR, "sensor", "random", lambda kind, case: A.script_seed(kind, case),
                  lambda case: dict(turn_angle=case[1], num_obstacles=case[0], start_holding=case[2])),
    "rearr_vel": Task("rearr_vel", B, B.Nav2DRearrVelEnv, TASK_REARR, "sensor", "random", lambda kind, case: B.script_seed(kind, case),
                      B.case_kw),
    "social": Task("social", P, P.Nav2DSocialEnv, TASK_SOCIAL, "forward", "random", lambda kind, case: P.SCRIPT_SEED, P.case_kw),
}


class View:
    """What the kernels read of one env's record: pose, heading direction, episode, rectangles, the static markers (x, y, r2, code)
    in the record's order, and the moving thing of the frame (the rearrangement object / the person), None where there is none."""
    __slots__ = ("px", "py", "c", "s", "episode", "rects", "markers", "thing")


def view(task, e):
    v = View()
    v.px, v.py, v.episode, v.rects = F(e.px), F(e.py), int(e.episode), [tuple(F(a) for a in r) for r in e.world.rects]
    v.c, v.s = (F(a) for a in e.dirs[e.h])
    v.thing = None
    if task == TASK_GOAL:
        v.markers = [(F(e.world.gx), F(e.world.gy), GOAL_R2, TARGET)]
    elif task == TASK_OBJ:
        v.markers = [(F(x), F(y), OBJ_R2, TARGET if int(c) == int(e.target) else OBJECT) for (x, y), c in zip(e.objects, e.cats)]
    elif task == TASK_REARR:
        v.markers = [(F(e.gx), F(e.gy), GOAL_R2, TARGET)]
        v.thing = (F(e.ox), F(e.oy), CARRIED)
    else:
        v.markers = []
        v.thing = (F(e.hx), F(e.hy), PERSON)
    return v


# ---- geometry ----------------------------------------------------------------------------------------------------------------
def check_resolution(S):
    if not isinstance(S, (int, np.integer)) or isinstance(S, bool) or not MIN_RESOLUTION <= S <= MAX_RESOLUTION:
        raise ValueError(f"map_resolution {S!r} must be a whole number in {MIN_RESOLUTION}..{MAX_RESOLUTION}")


def cell_size(S):
    return F(ARENA / F(S))


@functools.lru_cache(maxsize=None)
def centres(S):
    """(X (1, S), Y (S, 1)), read-only: the centre of cell (r, c) is x = (c + 0.5) * cell, y = (S - 1 - r + 0.5) * cell: row 0 on
    top, y up."""
    cell = cell_size(S)
    x = (np.arange(S, dtype=np.float32) + HALF) * cell
    y = (np.arange(S - 1, -1, -1, dtype=np.float32) + HALF) * cell
    return x[None, :], y[:, None]


def in_disc(X, Y, cx, cy, r2):
    dx, dy = X - cx, Y - cy
    return dx * dx + dy * dy <= r2


def near_segment(X, Y, ax, ay, bx, by, w2):
    """Within sqrt(w2) of the segment a -> b, without a division: the end points, then the strip between them (len2 > 0 only)."""
    ex, ey = X - ax, Y - ay
    sx, sy = F(bx - ax), F(by - ay)
    len2 = F(F(sx * sx) + F(sy * sy))
    dot, cross = ex * sx + ey * sy, sx * ey - sy * ex
    strip = (dot >= 0) & (dot <= len2) & (cross * cross <= F(w2 * len2)) if len2 > 0 else False
    return (ex * ex + ey * ey <= w2) | in_disc(X, Y, bx, by, w2) | strip


def occupied(X, Y, rects):
    occ = np.zeros(np.broadcast(X, Y).shape, bool)
    for x0, y0, x1, y1 in rects:
        occ |= (X > x0) & (X < x1) & (Y > y0) & (Y < y1)
    return occ


def static_layer(v, S):
    """Occupied / free, then the other objects (16), the targets (6) over them, the start (4) over all."""
    X, Y = centres(S)
    m = np.where(occupied(X, Y, v.rects), OCCUPIED, FREE).astype(np.uint8)
    for x, y, r2, code in v.markers:
        m[in_disc(X, Y, x, y, r2) & (m != TARGET)] = code
    m[np.broadcast_to(in_disc(X, Y, v.px, v.py, START_R2), m.shape)] = START
    return m


def draw_trajectory(m, ax, ay, bx, by, S):
    X, Y = centres(S)
    w = F(TRAJ_W * cell_size(S))
    m[near_segment(X, Y, ax, ay, bx, by, F(w * w)) & (m != START) & (m != TARGET)] = TRAJECTORY


def reveal(fog, v, S, vis_dist):
    """Marks the cells seen from the view's pose: not occupied, within vis_dist, inside the 90 degree wedge or within 0.25 m, and the
    segment from the agent to the centre meets no open raw rectangle (the geodesic mode's `visible` on the rectangles themselves)."""
    X, Y = centres(S)
    dx, dy = X - v.px, Y - v.py
    d2 = dx * dx + dy * dy
    dot, cross = dx * v.c + dy * v.s, v.c * dy - v.s * dx
    cand = (fog == 0) & (d2 <= F(F(vis_dist) * F(vis_dist))) & ((d2 <= NEAR_R2) | ((dot > 0) & (np.abs(cross) <= dot)))
    cand &= ~occupied(X, Y, v.rects)
    rr, cc = np.nonzero(cand)
    if rr.size:
        ok = np.atleast_1d(G.visible(v.px, v.py, X[0, cc], Y[rr, 0], v.rects))
        fog[rr[ok], cc[ok]] = 1


def update(m, fog, rec, v, S, vis_dist, begin):
    """One env's update after a step entry.  begin (a reset, or the step ended an episode): both layers are cleared, the static layer
    is written, the record takes the new episode and its start, the start point is drawn as a segment of no length, and the first
    reveal is done from it.  Otherwise the segment from the record's position to the new one is drawn, then the reveal."""
    if begin:
        m[...] = static_layer(v, S)
        fog[...] = 0
        rec[:] = 0
        rec[W_EPISODE] = v.episode
        rec[W_START_X:W_START_Y + 1] = np.array([v.px, v.py], np.float32).view(np.int32)
        ax, ay = v.px, v.py
    else:
        ax, ay = rec[W_PREV_X:W_PREV_Y + 1].view(np.float32)
    draw_trajectory(m, ax, ay, v.px, v.py, S)
    rec[W_PREV_X:W_PREV_Y + 1] = np.array([v.px, v.py], np.float32).view(np.int32)
    reveal(fog, v, S, vis_dist)


# ---- the frame -----------------------------------------------------------------------------------------------------------------
def panel_width(Hf, H, W):
    return (Hf * W) // H


def frame_width(Hf, H, W, has_rgb, has_depth):
    return Hf + (int(bool(has_rgb)) + int(bool(has_depth))) * (panel_width(Hf, H, W) if (has_rgb or has_depth) else 0)


def map_panel_codes(m, v, S):
    """The map with the overlays, at cell granularity, later ones on top: the object / the person (0.3 m), the agent (0.2 m), the
    heading tick (cells within 0.08 m of p -> p + 0.45 * dir)."""
    X, Y = centres(S)
    code = m.copy()
    if v.thing is not None:
        code[in_disc(X, Y, v.thing[0], v.thing[1], OBJ_R2)] = v.thing[2]
    code[in_disc(X, Y, v.px, v.py, AGENT_R2)] = AGENT
    qx, qy = F(v.px + F(TICK_LEN * v.c)), F(v.py + F(TICK_LEN * v.s))
    code[near_segment(X, Y, v.px, v.py, qx, qy, TICK_R2)] = TICK
    return code


def frame(m, fog, v, S, Hf, rgb=None, depth=None, draw_fog=True):
    """(Hf, Wf, 3) uint8: rgb and depth (grey = (int)(d * 255)) upscaled by nearest neighbour -- source row (r * H) / Hf, source column
    (c * W) / panel width -- then the map at Hf x Hf, cell ((r * S) / Hf, (c * S) / Hf); a free cell that was never seen at half
    brightness (each channel >> 1)."""
    r = np.arange(Hf)
    panels = []
    if rgb is not None or depth is not None:
        H, W = (rgb if rgb is not None else depth).shape[:2]
        Wp = panel_width(Hf, H, W)
        sr, sc = (r * H) // Hf, (np.arange(Wp) * W) // Wp
        if rgb is not None:
            panels.append(rgb[sr][:, sc])
        if depth is not None:
            g = np.clip((depth.reshape(H, W)[sr][:, sc].astype(np.float32) * F(255.0)).astype(np.int32), 0, 255).astype(np.uint8)
            panels.append(np.repeat(g[..., None], 3, 2))
    code = map_panel_codes(m, v, S)
    col = COLORS[code & 31]
    if draw_fog:
        dim = (code == FREE) & (fog == 0)
        col = np.where(dim[..., None], col >> 1, col)
    cr = (r * S) // Hf
    panels.append(col[cr][:, cr])
    return np.ascontiguousarray(np.concatenate(panels, 1), dtype=np.uint8)


# ---- a run -----------------------------------------------------------------------------------------------------------------------
class MapRun:
    """Steps restated envs and keeps their maps: `reset()`, then `step(actions, mask=None)`; `map`, `fog` (N, S, S) uint8 and `rec`
    (N, 8) int32 afterwards.  `obs[n]` is env n's last observation, `dones[n]` whether its last step ended an episode."""

    def __init__(self, task, envs, S, vis_dist=5.0, draw_fog=True):
        check_resolution(S)
        self.task, self.envs, self.S, self.vis, self.draw_fog = task, envs, S, vis_dist, draw_fog
        n = len(envs)
        self.map, self.fog = np.zeros((n, S, S), np.uint8), np.zeros((n, S, S), np.uint8)
        self.rec = np.zeros((n, REC_WORDS), np.int32)
        self.obs, self.dones = [None] * n, [False] * n

    def views(self):
        return [view(self.task, e) for e in self.envs]

    def reset(self):
        for n, e in enumerate(self.envs):
            self.obs[n], self.dones[n] = e.reset(), False
            update(self.map[n], self.fog[n], self.rec[n], view(self.task, e), self.S, self.vis, True)

    def step(self, actions, mask=None):
        for n, e in enumerate(self.envs):
            if mask is not None and not mask[n]:
                continue
            self.obs[n], _, done, _ = e.step(actions[n])
            self.dones[n] = bool(done)
            update(self.map[n], self.fog[n], self.rec[n], view(self.task, e), self.S, self.vis, self.dones[n])

    def frames(self, Hf, rgb_key=None, depth_key=None):
        out = []
        for n, e in enumerate(self.envs):
            o = self.obs[n]
            out.append(frame(self.map[n], self.fog[n], view(self.task, e), self.S, Hf, o[rgb_key] if rgb_key else None,
                             o[depth_key] if depth_key else None, self.draw_fog))
        return np.stack(out)
