"""CPU: the geodesic distance mode of Nav2DRearr-v0 / Nav2DRearrVel-v0 on its numpy restatement (tests/nav2d_rearr_geo_reference.py):
both float32 fields against float64 shortest paths from both sides, telescoping rewards, the PICK jump, the K = 0 limit, hand-made
worlds (walled-off goal and object, a PLACE into an enclosed pocket), the event coverage of the scripted runs that
tests/test_gpu_nav2d_rearr_geo.py replays on the device, and the Python layer: refusal, factory, YAMLs, header and signature table."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import nav2d_geo_reference as G
import nav2d_rearr_geo_reference as RG
import nav2d_rearr_reference as A
import nav2d_rearr_vel_reference as B
import nav2d_reference as R
from test_nav2d_geo_host import Graph64

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the relative error of a field value or a query: at most 33 hops, each a rounded dist and a rounded add (test_nav2d_geo_host.py)
REL = 40 * 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


@functools.lru_cache(maxsize=None)
def geo_run(kind, case):
    return RG.script_rollout(kind, case)


@functools.lru_cache(maxsize=None)
def vel_geo_run(kind, case):
    return RG.vel_script_rollout(kind, case)


# ---- the fields against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 8])
def test_both_fields_lie_between_two_float64_geodesics(K):
    """The worlds and places of seed 1, envs 0..11, episodes 0..2, for the goal target (DG) and the object target (DO): at the agent's
    start, at the other place and at 3 random free points, g_E (1 - b) <= geo_T <= g_0 (1 + b) with b = 40 * 2^-24, g_0 and g_E the
    float64 shortest paths of tests/test_nav2d_geo_host.py (boxes shrunk by 1e-9 with the nodes on the inflated corners; boxes and
    nodes shrunk by 2^-10).  No query is infinite: none of these worlds is unreachable."""
    worst_hi = worst_lo = -1.0
    for env in range(12):
        for ep in range(3):
            w, o0, g, _ = A.places(1, env, ep, K, 36)
            rng = np.random.RandomState(1000 * env + 10 * ep + K)
            pts = [(w.sx, w.sy)]
            while len(pts) < 4:
                x, y = (F(v) for v in rng.uniform(0.1, 7.9, 2))
                if R.is_free(x, y, w.rects):
                    pts.append((x, y))
            for (tx, ty), other in ((g, o0), (o0, g)):
                D, sweeps = RG.build_field(w.rects, tx, ty)
                assert 1 <= sweeps <= 4 * K and np.all(np.isinf(D[4 * K:]))
                g0, gE = Graph64(w.rects, tx, ty, 1e-9, 0.0), Graph64(w.rects, tx, ty, 2.0 ** -10, 2.0 ** -10)
                for x, y in pts + [other]:
                    v = float(RG.geo(x, y, w.rects, tx, ty, D))
                    hi, lo = g0.geo(x, y), gE.geo(x, y)
                    assert np.isfinite(v) and np.isfinite(hi) and np.isfinite(lo)
                    assert lo * (1 - REL) <= v <= hi * (1 + REL), (env, ep, x, y, lo, v, hi)
                    worst_hi, worst_lo = max(worst_hi, v / hi - 1), max(worst_lo, 1 - v / lo)
    print(f"nav2d rearr geo K={K}: geo / g_0 - 1 <= {worst_hi:.3e}, 1 - geo / g_E <= {worst_lo:.3e} (bound {REL:.3e})")


# ---- rewards ----------------------------------------------------------------------------------------------------------------------
def episodes(e, script, count):
    """Runs `count` episodes; yields (phi_0, [(reward, phi_before, phi_after)], info, last)."""
    obs = e.observe()
    for _ in range(count):
        phi0, steps = float(e.phi_start), []
        while True:
            before = float(e.phi_prev)
            obs, r, done, info = e.step(script(obs, e))
            steps.append((float(r), before, float(e.last["phi_end"]) if done else float(e.phi_prev)))
            if done:
                script.episode_ended()
                break
        yield phi0, steps, info, e.last


@pytest.mark.parametrize("vel", [False, True], ids=["discrete", "velocity"])
def test_rewards_telescope(vel):
    """Per episode, in float64: sum r = -0.01 * len + Phi_0 - Phi_T + 1.0 * [a first PICK happened] + 2.5 * success.  Each Phi is the
    same float32 where it is subtracted and where it is subtracted from, so the potentials cancel exactly and what is left are the
    roundings of each step's reward, each at most 2^-24 of the rounded value: with d = Phi_prev - Phi these are |d|, then
    |d| + 0.01, then |d| + 1.01 on the step with the pick bonus and |d| + 3.51 on the step with the success bonus, and -0.01 itself
    is off by less than 2^-31 as a float32.  So the bound is sum over the steps of 2^-24 (4 |d| + 4.6) + 2^-31.  The geodesic
    potential is larger than the Euclidean one and drops by whole metres at a PICK, which this bound follows step by step."""
    rng = np.random.RandomState(1)
    seen, detours = set(), 0
    for kind, sh, K in (("waypoint", False, 3), ("waypoint", True, 8), ("grip" if vel else "pickplace", True, 3), ("random", False, 8)):
        kw = dict(num_obstacles=K, start_holding=sh, max_episode_steps=80, use_rgb=False, use_depth=False)
        if vel:
            e = RG.Nav2DRearrVelGeoEnv(11, 1, turn_angle=10, max_turn_angle=30, min_abs_ang_speed=10, **kw)
            sc = RG.VelWaypoint(30) if kind == "waypoint" else B.make_script(kind, 30, rng)
        else:
            e = RG.Nav2DRearrGeoEnv(11, 1, turn_angle=30, **kw)
            sc = RG.Waypoint(30) if kind == "waypoint" else A.make_script(kind, 30, rng)
        e.reset()
        for phi0, steps, info, L in episodes(e, sc, 8):
            n, total = len(steps), sum(s[0] for s in steps)
            closed = -0.01 * n + phi0 - float(L["phi_end"]) + 1.0 * (L["picks"] > 0) + 2.5 * info["success"]
            bound = sum(2.0 ** -24 * (4 * abs(s[1] - s[2]) + 4.6) + 2.0 ** -31 for s in steps)
            assert L["length"] == n and abs(total - closed) <= bound, (kind, total, closed, bound)
            seen.add((L["picks"] > 0, info["success"]))
        detours += e.counters["detours"]
    assert {(True, 1.0), (False, 1.0), (False, 0.0)} <= seen and detours > 0


def test_the_potential_does_not_rise_at_a_pick():
    """At a successful PICK Phi goes from geo_o(p) + geo_g(o) to geo_g(p), and the jump Phi_before - Phi_after is at least minus the
    float32 bound: each of the three geo values is off by at most b = 40 * 2^-24 of itself (the bound of the field test above) and
    the sum of the two terms rounds by at most 2^-24 of it, so with g_0 and g_E the two float64 shortest paths from p to g the bound
    is b (g_0 + g_E) + 2^-24 Phi_before.  It presumes the triangle inequality of one metric; the float32 graph lies between two, of
    worlds that differ by E, and the picks of the drawn runs have jumps of millimetres to metres, far from either.  So the second
    half holds the same bound where the jump is about 0: start, object and goal in one line of sight, the object exactly on the line
    and up to a millimetre off it to both sides."""
    rng = np.random.RandomState(2)
    picks, smallest = 0, np.inf
    for kind, K in (("waypoint", 3), ("waypoint", 8), ("pickplace", 8)):
        for env in range(4):
            e = RG.Nav2DRearrGeoEnv(1, env, turn_angle=30, num_obstacles=K, max_episode_steps=60, use_rgb=False, use_depth=False)
            e.reset()
            sc = RG.Waypoint(30) if kind == "waypoint" else A.make_script(kind, 30, rng)
            obs = e.observe()
            for _ in range(150):
                held, before, p, goal, rects, reachable = e.holding, float(e.phi_prev), (e.px, e.py), (e.gx, e.gy), e.world.rects, e.reachable
                picked_before = e.picks
                obs, r, done, info = e.step(sc(obs, e))
                if done:
                    sc.episode_ended()
                    continue
                if not held and e.holding and e.picks == picked_before + 1 and reachable:
                    after = float(e.phi_prev)
                    g0, gE = Graph64(rects, goal[0], goal[1], 1e-9, 0.0).geo(*p), Graph64(rects, goal[0], goal[1], 2.0 ** -10, 2.0 ** -10).geo(*p)
                    fp = REL * (g0 + gE) + 2.0 ** -24 * before
                    assert before - after >= -fp, (kind, K, env, before, after, g0, gE)
                    picks += 1
                    smallest = min(smallest, before - after)
    print(f"nav2d rearr geo: {picks} picks in the drawn runs, smallest jump {smallest:.3e}")
    assert picks >= 10
    near = []
    for dy in [0.0] + [s * v for v in (2.0 ** -20, 1e-5, 1e-4, 1e-3) for s in (1, -1)]:
        w = RG.in_line(dy)
        e = RG.hand_made(w, turn_angle=30)
        before, (gx, gy) = float(e.phi_prev), w["g"]
        assert e.reachable and bits(e.a) == bits(R.dist(e.px, e.py, e.ox, e.oy)) and bits(e.b) == bits(R.dist(e.ox, e.oy, e.gx, e.gy))
        e.step(A.PICK)
        after = float(e.phi_prev)
        assert e.holding and e.picks == 1 and bits(e.phi_prev) == bits(R.dist(e.px, e.py, e.gx, e.gy))
        g0, gE = Graph64(e.world.rects, gx, gy, 1e-9, 0.0).geo(e.px, e.py), Graph64(e.world.rects, gx, gy, 2.0 ** -10, 2.0 ** -10).geo(e.px, e.py)
        assert before - after >= -(REL * (g0 + gE) + 2.0 ** -24 * before), (dy, before, after)
        near.append(before - after)
    print("nav2d rearr geo: jumps of the in-line picks", ["%.2e" % v for v in near])
    assert max(abs(v) for v in near) < 1e-5   # these picks are where the inequality could fail: the jump is rounding alone


# ---- limits and hand-made worlds --------------------------------------------------------------------------------------------------
def assert_same_outputs(a, b, what):
    for k in ("rewards", "sums"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)
    same_actions = np.array_equal(bits(a["actions"]), bits(b["actions"])) if a["actions"].dtype == np.float32 else np.array_equal(a["actions"], b["actions"])
    assert np.array_equal(a["dones"], b["dones"]) and same_actions and a["infos"] == b["infos"], what   # drawn actions hold nan
    for row_a, row_b in zip(a["states"], b["states"]):
        for sa, sb in zip(row_a, row_b):
            assert all(np.array_equal(bits(sa[k]) if sa[k].dtype == np.float32 else sa[k], bits(sb[k]) if sb[k].dtype == np.float32 else sb[k])
                       for k in sa), what
    for row_a, row_b in zip(a["obs"], b["obs"]):
        for oa, ob in zip(row_a, row_b):
            assert all(np.array_equal(oa[k], ob[k]) for k in oa), what


def test_no_obstacles_is_the_euclidean_restatement_bitwise():
    """K = 0: no nodes, no sweeps, every geo the direct distance.  Every output of every Euclidean script over the K = 0 cases of both
    tasks -- actions (the scripts read the same observations), rewards, dones, infos, measure sums, the named state words, the
    vector sensors -- equals the Euclidean restatement's bit for bit; the record holds +inf fields and the two Euclidean terms."""
    D, sweeps = RG.build_field([], F(7.5), F(7.5))
    assert sweeps == 0 and np.all(np.isinf(D))
    for case in [c for c in RG.SCRIPT_CASES if c[0] == 0]:
        for kind in A.SCRIPTS:
            a = geo_run(kind, case)
            assert_same_outputs(a, A.script_rollout(kind, case), (kind, case))
            f = a["fields"]
            assert np.all(np.isinf(f[:, :, :64].view(np.float32))) and not f[:, :, RG.W_SWEEPS_GOAL:RG.W_LOST + 1].any() and f[:, :, RG.W_REACHABLE].all()
            for t, row in enumerate(a["states"]):
                for n, s in enumerate(row):
                    assert np.array_equal(bits(f[t, n, RG.W_A:RG.W_B + 1].view(np.float32).sum(dtype=np.float32)), bits(s["potential"][0]))
    for case in [c for c in RG.VEL_SCRIPT_CASES if c[0] == 0]:
        for kind in B.SCRIPTS:
            assert_same_outputs(vel_geo_run(kind, case), B.script_rollout(kind, case), (kind, case))


@pytest.mark.parametrize("world", ["WALLED_GOAL", "WALLED_OBJECT", "WALLED_GOAL_HOLDING"])
def test_walled_off_worlds_stay_euclidean(world):
    """nav2d_geo_reference's ring round the goal, or round the object: a term is +inf at the beginning, reachable = 0, d_start stays
    the Euclidean Phi_0 and every step's Phi, b and reward are the Euclidean ones; the record keeps a0 and b0 as they came out, no
    lost step is counted and a PLACE (the third world begins holding) rebuilds nothing."""
    spec = dict(RG.WALLED_GOAL, start_holding=True) if world == "WALLED_GOAL_HOLDING" else getattr(RG, world)
    e = RG.hand_made(spec, turn_angle=30, max_episode_steps=40)
    assert not e.reachable and e.counters["unreachable"] == 1 and not (np.isfinite(e.a) and np.isfinite(e.b))
    euclid = A.Nav2DRearrEnv.potential(e)
    assert bits(e.phi_start) == bits(euclid[0]) == bits(e.phi_prev)
    record = e.field_record()
    rng, places = np.random.RandomState(3), 0
    for t in range(30):
        a = A.PLACE if (world == "WALLED_GOAL_HOLDING" and t == 3) else int(rng.randint(1, 6))
        prev, held = e.phi_prev, e.holding
        _, r, done, _ = e.step(a)
        assert not done
        phi, b = A.Nav2DRearrEnv.potential(e)
        assert bits(e.phi_prev) == bits(phi)
        assert bits(r) == bits(F(F(F(R.SLACK + F(prev - phi)) + (A.PICK_REWARD if (e.picks == 1 and e.holding and not held) else F(0.0))) + F(0.0)))
        assert np.array_equal(e.field_record(), record)
        places += int(held and not e.holding)
    assert (places >= 1 if world == "WALLED_GOAL_HOLDING" else places == 0) and e.rebuilds == 0 and e.lost_steps == 0


@pytest.mark.parametrize("vel", [False, True], ids=["discrete", "velocity"])
def test_an_unreachable_episode_succeeds_by_the_euclidean_distance(vel):
    """WALLED_START: the agent begins inside the ring of thin walls, holding, the goal just outside: b0 is +inf, the episode is
    unreachable.  A PLACE across the wall puts the object 0.07 m from the goal in a straight line -- no path leads there -- and the
    STOP after it succeeds by the Euclidean b < 0.5, with the Euclidean b as object_to_goal_distance; nothing is rebuilt or lost."""
    kw = dict(turn_angle=10, max_turn_angle=30, min_abs_ang_speed=10) if vel else dict(turn_angle=30)
    e = RG.hand_made(RG.WALLED_START, vel=vel, **kw)
    assert not e.reachable and e.holding and np.isinf(e.b) and bits(e.a) == bits(F(0.0)) and np.isfinite(e.DG).any()
    assert bits(e.phi_start) == bits(A.Nav2DRearrEnv.potential(e)[0])
    record = e.field_record()
    place, stop = ((-0.5, 0.0, -1.0), (-1.0, 0.0, 0.0)) if vel else (A.PLACE, A.STOP)   # velocity: a slow move into the wall, refused
    prev = e.phi_prev
    _, r, done, _ = e.step(np.array(place, np.float32) if vel else place)
    phi, b = A.Nav2DRearrEnv.potential(e)
    assert not done and not e.holding and e.invalid == 0 and float(b) < 0.1 and np.array_equal(e.field_record(), record)
    assert bits(e.phi_prev) == bits(phi) and bits(r) == bits(F(F(R.SLACK + F(prev - phi)) + F(0.0)) + F(0.0))
    _, r, done, info = e.step(np.array(stop, np.float32) if vel else stop)
    assert done and info["success"] == 1.0 and info["object_to_goal_distance"] == float(b)
    assert bits(r) == bits(F(F(F(R.SLACK + F(phi - phi)) + F(0.0)) + R.SUCCESS_REWARD))
    assert e.counters["rebuilds"] == 0 and e.counters["lost_steps"] == 0 and e.counters["unreachable"] == 1 + int(not e.reachable)


def test_overlapping_rectangles_are_reachable():
    e = RG.hand_made(RG.OVERLAPPING)
    x, y, ok = G.nodes(e.world.rects)
    no_node, node = [3, 4], [0, 1, 2, 5, 6, 7]   # each rectangle has one grown corner strictly inside the other's grown box
    assert e.reachable and not ok[no_node].any() and np.isinf(e.DG[no_node]).all() and np.isinf(e.DO[no_node]).all()
    assert np.isfinite(e.DG[node]).all() and np.isfinite(e.DO[node]).all()
    assert float(e.phi_start) > float(A.Nav2DRearrEnv.potential(e)[0]) + RG.DETOUR and e.counters["detours"] == 1


@pytest.mark.parametrize("vel", [False, True], ids=["discrete", "velocity"])
def test_start_holding_has_no_object_field_until_the_first_place(vel):
    """Under start_holding DO is +inf in all 32 words and sweeps_obj = 0 from the beginning of the episode until the first successful
    PLACE, which builds it towards q; a = 0 throughout the carrying."""
    kw = dict(num_obstacles=3, start_holding=True, max_episode_steps=200, use_rgb=False, use_depth=False)
    e = RG.Nav2DRearrVelGeoEnv(1, 2, turn_angle=10, max_turn_angle=30, min_abs_ang_speed=10, **kw) if vel else RG.Nav2DRearrGeoEnv(1, 2, turn_angle=30, **kw)
    e.reset()
    forward, place, turn = ((1.0, 0.0, 0.0), (1.0, 0.0, -1.0), (-0.5, 1.0, 0.0)) if vel else (A.MOVE_FORWARD, A.PLACE, A.TURN_LEFT)
    for t in range(6):
        rec = e.field_record()
        assert np.all(np.isinf(rec[RG.W_DO:RG.W_DO + 32].view(np.float32))) and rec[RG.W_SWEEPS_OBJ] == 0 and rec[RG.W_REBUILDS] == 0
        assert rec[RG.W_A] == 0 and e.reachable and rec[RG.W_SWEEPS_GOAL] >= 1
        e.step(forward)
    for _ in range(12):   # a PLACE into a rectangle or beyond the box is refused: turn and try again
        e.step(place)
        if not e.holding:
            break
        assert np.all(np.isinf(e.DO)) and e.sweeps_obj == 0
        e.step(turn)
    rec = e.field_record()
    assert not e.holding and rec[RG.W_REBUILDS] == 1 and rec[RG.W_SWEEPS_OBJ] >= 1 and np.isfinite(rec[RG.W_DO:RG.W_DO + 32].view(np.float32)).any()
    D, sweeps = RG.build_field(e.world.rects, e.ox, e.oy)
    assert np.array_equal(bits(D), rec[RG.W_DO:RG.W_DO + 32]) and sweeps == rec[RG.W_SWEEPS_OBJ]
    assert bits(e.b) == bits(RG.geo(e.ox, e.oy, e.world.rects, e.gx, e.gy, e.DG)) and float(e.a) > 0.4


def test_a_place_into_an_enclosed_pocket_is_a_lost_step():
    """POCKET: the agent reaches across a 0.05 m wall.  The PLACE succeeds and rebuilds DO, in which no node is finite; neither
    geo_q(p) nor geo_g(q) exists, so a stays 0, b stays geo_g(p), the step counts once as lost and its reward is the slack alone.
    From then on every step is lost and Phi stands still; a PICK across the wall brings both terms back."""
    e = RG.hand_made(RG.POCKET, turn_angle=30)
    assert e.reachable and e.holding and bits(e.a) == bits(F(0.0))
    b0 = e.b
    _, r, done, _ = e.step(A.PLACE)
    assert not e.holding and e.invalid == 0 and e.rebuilds == 1 and e.lost_steps == 1 and np.all(np.isinf(e.DO)) and not done
    assert bits(e.a) == bits(F(0.0)) and bits(e.b) == bits(b0) and bits(r) == bits(F(R.SLACK + F(0.0)))
    _, r, _, _ = e.step(A.TURN_LEFT)
    _, r, _, _ = e.step(A.TURN_RIGHT)
    assert e.lost_steps == 3 and bits(r) == bits(F(R.SLACK + F(0.0)))
    _, r, _, _ = e.step(A.PICK)
    assert e.holding and e.lost_steps == 3 and bits(e.b) == bits(b0) and e.counters["repicks_after_place"] == 1
    assert e.counters["lost_steps"] == 3 and e.counters["rebuilds"] == 1


# ---- the scripted runs ------------------------------------------------------------------------------------------------------------
MINIMUM = dict(detours=20, rebuilds=50, repicks_after_place=20, waypoint_successes=20, waypoint_rebuilds=20)


@pytest.mark.parametrize("vel", [False, True], ids=["discrete", "velocity"])
def test_scripted_runs_reach_the_events(vel):
    """A condition on the inputs of tests/test_gpu_nav2d_rearr_geo.py, on the restatement alone: over the task's SCRIPT_CASES, the
    four Euclidean scripts plus 'waypoint' at SCRIPT_SEED reach at least MINIMUM of each event that drawn worlds can reach -- episodes
    whose geodesic Phi_0 exceeds the straight one by more than 0.05 m, PLACEs that rebuilt DO, PICKs after a PLACE, successes and
    rebuilds of the waypoint script -- and every run ends episodes.  No drawn world of these runs is unreachable and none loses a
    step: those two are reached by the hand-made worlds above.  At K = 0 nothing is a detour."""
    cases, scripts, run = (RG.VEL_SCRIPT_CASES, RG.VEL_SCRIPTS, vel_geo_run) if vel else (RG.SCRIPT_CASES, RG.SCRIPTS, geo_run)
    total = {k: 0 for k in RG.GEO_EVENTS}
    way = dict(successes=0, rebuilds=0)
    for case in cases:
        for kind in scripts:
            r = run(kind, case)
            c = r["counters"]
            assert r["dones"].sum() >= RG.SCRIPT_ENVS and r["fields"].shape == (RG.SCRIPT_STEPS + 1, RG.SCRIPT_ENVS, RG.GEO_WORDS)
            assert case[0] > 0 or c["detours"] == 0
            for k in total:
                total[k] += c[k]
            if kind == "waypoint":
                way["successes"] += c["successes"]
                way["rebuilds"] += c["rebuilds"]
    print("nav2d rearr geo events:", "velocity" if vel else "discrete", total, way)
    assert total["unreachable"] == 0 and total["lost_steps"] == 0
    assert all(total[k] >= MINIMUM[k] for k in ("detours", "rebuilds", "repicks_after_place"))
    assert way["successes"] >= MINIMUM["waypoint_successes"] and way["rebuilds"] >= MINIMUM["waypoint_rebuilds"]


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
def test_the_library_has_the_field_record():
    """Fails without the feature: the entry does not resolve."""
    from habitat_amd import _lib
    L = _lib.lib()
    assert L.hab_nav2d_rearr_geo_bytes() == 4 * RG.GEO_WORDS == 288
    for name in ("hab_nav2d_rearr_geo_build", "hab_nav2d_rearr_step_geo", "hab_nav2d_rearr_vel_step_geo"):
        assert hasattr(L, name)


def test_refusal_without_a_gpu_and_its_wording():
    """Both classes refuse the mode on a device that is no GPU before touching the device, in the issue's words; every other refusal
    comes as before, and the mode itself is accepted: the next refusal of a CPU device is the base class's."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    for cls, name in ((EF.Nav2DRearrVectorEnv, "Nav2DRearr"), (EF.Nav2DRearrVelVectorEnv, "Nav2DRearrVel")):
        with pytest.raises(_lib.HabError) as err:
            cls(2, 8, 8, device="cpu", distance="geodesic")
        assert str(err.value) == (f"{name}: distance 'geodesic' builds its fields on the GPU; without a GPU device the task has "
                                  "Euclidean distances only")
        with pytest.raises(_lib.HabError, match="distance 'manhattan' must be one of"):
            cls(2, 8, 8, device="cpu", distance="manhattan")
        with pytest.raises(_lib.HabError, match="start_holding"):
            cls(2, 8, 8, device="cpu", distance="euclidean", start_holding=1)
        assert cls._geo_entry == cls._entries[0] + "_geo" and len(cls._entries) == 1 and cls._geo_bytes == "hab_nav2d_rearr_geo_bytes"


def test_factory_choice_from_the_geodesic_yamls(monkeypatch):
    """Fails without the feature: the files do not exist.  Each new YAML is its sibling with distance_to_goal = geodesic, and the
    factory hands that to the task's class."""
    from habitat_amd.common import env_factory as EF
    from habitat_amd.config.default import get_config
    made = []
    for cls in ("Nav2DRearrVectorEnv", "Nav2DRearrVelVectorEnv"):
        monkeypatch.setattr(EF, cls, lambda *a, _n=cls, **kw: made.append((_n, a, kw)) or _n)
    for stem, cls in (("ddppo_nav2d_rearrange", "Nav2DRearrVectorEnv"), ("ddppo_nav2d_rearrange_vel", "Nav2DRearrVelVectorEnv")):
        cfg, sibling = get_config(f"rearrange/{stem}_geodesic.yaml"), get_config(f"rearrange/{stem}.yaml")
        assert cfg.habitat.synthetic.distance_to_goal == "geodesic" and sibling.habitat.synthetic.distance_to_goal == "euclidean"
        assert cfg.habitat.task == sibling.habitat.task and cfg.habitat.simulator == sibling.habitat.simulator
        assert cfg.habitat.environment == sibling.habitat.environment and cfg.habitat_baselines == sibling.habitat_baselines
        assert {k: v for k, v in cfg.habitat.synthetic.items() if k != "distance_to_goal"} == {
            k: v for k, v in sibling.habitat.synthetic.items() if k != "distance_to_goal"}
        assert EF.SyntheticVectorEnvFactory().construct_envs(cfg, device="cpu") == cls
        _, args, kw = made[-1]
        assert args == (16, 128, 128) and kw["distance"] == "geodesic" and kw["start_holding"] is False and kw["num_obstacles"] == 3
    assert "refuses the geodesic" not in EF.SyntheticVectorEnvFactory.__doc__


def test_header_and_signature_table_agree():
    """The header's prototypes of the four new entries and the ctypes table: the same number of arguments, pointers where the header
    has pointers, size_t, uint32, float and int in their places; the step entries are their Euclidean siblings with `geo` after
    `state`; the named words of the field record are the restatement's."""
    from habitat_amd import _lib
    text = open(os.path.join(ROOT, "include", "habitat_amd.h")).read()
    kinds = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float, "int": ctypes.c_int}

    def names_and_types(entry):
        m = re.search(r"int %s\((.*?)\);" % entry, text, re.S)
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
        restype, argtypes = _lib.SIGNATURES[entry]
        assert restype is ctypes.c_int and len(params) == len(argtypes), entry
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if ("*" in p or p.startswith("hipStream_t")) else kinds[p.split()[0]]
            assert t is want, (entry, p)
        return [p.split()[-1].lstrip("*") for p in params]

    assert names_and_types("hab_nav2d_rearr_geo_build") == ["state", "state_stride_bytes", "geo", "mask", "only_ended", "N", "num_obstacles",
                                                             "start_holding", "stream"]
    for entry in ("hab_nav2d_rearr_step", "hab_nav2d_rearr_vel_step"):
        plain, geo = names_and_types(entry), names_and_types(entry + "_geo")
        assert geo == plain[:1] + ["geo"] + plain[1:]
        assert _lib.SIGNATURES[entry + "_geo"][1] == _lib.SIGNATURES[entry][1][:1] + [ctypes.c_void_p] + _lib.SIGNATURES[entry][1][1:]
    assert _lib.SIGNATURES["hab_nav2d_rearr_geo_bytes"] == (ctypes.c_int, [])
    words = {k: int(v) for k, v in re.findall(r"#define HAB_NAV2D_REARR_GEO_(\w+) +(\d+)", text)}
    assert words == dict(BYTES=4 * RG.GEO_WORDS, W_DG=RG.W_DG, W_DO=RG.W_DO, W_A=RG.W_A, W_B=RG.W_B, W_REACHABLE=RG.W_REACHABLE,
                         W_SWEEPS_GOAL=RG.W_SWEEPS_GOAL, W_SWEEPS_OBJ=RG.W_SWEEPS_OBJ, W_LOST_STEPS=RG.W_LOST, W_REBUILDS=RG.W_REBUILDS)
    assert (words["W_REBUILDS"] + 2) * 4 == words["BYTES"] and RG.STATE_WORDS * 4 == int(
        re.search(r"#define HAB_NAV2D_REARR_STATE_BYTES (\d+)", text).group(1))
