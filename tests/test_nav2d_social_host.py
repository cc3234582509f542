"""CPU: the Nav2DSocial-v0 task on its numpy restatement (tests/nav2d_social_reference.py): the world's invariants, the person's walk
against float64 shortest paths from both sides, every rule at its boundary on hand-made worlds, the event coverage of the scripted
runs that tests/test_gpu_nav2d_social.py replays on the device, and the refusals and the wiring of the Python layer."""
import collections
import functools
import os
import re

import numpy as np
import pytest

import nav2d_geo_reference as G
import nav2d_reference as R
import nav2d_social_reference as S
from test_nav2d_geo_host import Graph64

F = np.float32
E = float(G.E)


@functools.lru_cache(maxsize=None)
def run(kind, case):
    return S.script_rollout(kind, case)


def hand(rects, start, person, h=0, waypoint=None, **kw):
    """A restated env in a hand-made world: the agent at `start` with heading index h (turn_angle 10), the person at `person`."""
    kw = dict(dict(turn_angle=10, max_turn_angle=30, min_abs_ang_speed=10), **kw)
    e = S.Nav2DSocialEnv(1, 0, num_obstacles=len(rects), **kw)
    e.reset()
    e.begin_with(rects, start[0], start[1], person[0], person[1], h=h, waypoint=waypoint)
    return e


STILL, FULL = (-1.0, 0.0), (1.0, 0.0)


# ---- invariants -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 3, 8])
def test_world_invariants(K):
    """After every step of the random and the charging script: the agent is free by Nav2D-v0's test and by the keep-out,
    d(p, h) >= 0.4, and the person lies inside no open visibility box; an episode ends at the step limit and nowhere else."""
    for kind in ("random", "charge"):
        envs = [S.Nav2DSocialEnv(3, n, num_obstacles=K, max_episode_steps=25, turn_angle=10, max_turn_angle=30, min_abs_ang_speed=10)
                for n in range(4)]
        for e in envs:
            e.reset()
        rng = np.random.RandomState(K)
        for t in range(75):
            for e in envs:
                a = rng.uniform(-1.25, 1.25, 2) if kind == "random" else S.charge_action(e, 30)
                _, _, done, info = e.step(a)
                assert done == ((t + 1) % 25 == 0) and bool(info) == done
                assert R.is_free(e.px, e.py, e.world.rects) and e.is_free(e.px, e.py)
                assert R.dist(e.px, e.py, e.hx, e.hy) >= S.KEEP_OUT
                for lx, ly, hx, hy in G.visibility_boxes(e.world.rects):
                    assert not (lx < e.hx < hx and ly < e.hy < hy), (kind, t)
                assert 0.5 <= e.wx <= 7.5 and 0.5 <= e.wy <= 7.5 and not S.in_grown_rect(e.wx, e.wy, e.world.rects)


# ---- the walk against float64 ---------------------------------------------------------------------------------------------------------
def test_the_walk_lies_between_two_float64_shortest_paths():
    """Every completed leg (waypoint drawn to arrival, wait steps removed) of the still, greedy and forward scripts at K = 3 and 8, with T steps
    of which n landed on the end of their hop (the arrival included), against g_0, the float64 shortest path from the leg's start to
    its waypoint with the boxes shrunk by 1e-9, and g_E, the same in the world shrunk by E (Graph64 of tests/test_nav2d_geo_host.py):
        (T - n) v <= g_0 + b_hi      and      T v >= g_E - b_lo.
    Derivation.  One step: L is five roundings of relative 2^-24 (two differences, two squares rounded before a rounded sum, one
    root: at most 3 * 2^-24 in all), f = fl(v / L) one more, and each coordinate fl(h + fl(f * fl(t - h))) two relative ones on a
    product below v and one absolute half ulp of a coordinate below 8, 2^-22.  So a step that does not land is v long within
    delta = 8 * 2^-24 * v + 2^-21 and at most that far off its edge; a step that lands is at most v (1 + 3 * 2^-24) long.
    Upper side.  With g(h) the least candidate value at h: a step that does not land leaves its target t a candidate (h' is within
    2^-21 of an edge that clears every shrunk box; edges along an inflated side clear it by E = 2^-10), so
    g(h') <= fl(d(h', t) + DW[t]) <= (g(h) - v + delta)(1 + 2 * 2^-24); a landing on node t gives g(t) <= DW[t] <= g(h), since DW is
    the sweeps' fixed point and the visibility test is symmetric in its two points.  g ends at 0, so (T - n) v <= g(start) +
    T (delta + 2^-22 g_0), and g(start) = geo(start) <= g_0 (1 + 40 * 2^-24) by test_field_lies_between_two_float64_geodesics.
    Hence b_hi = 40 * 2^-24 g_0 + T (delta + 2^-22 g_0).
    Lower side.  The walked polyline avoids every box shrunk by E + 2^-20, so it is no shorter than g_E', the shortest path of that
    world, and it is at most T (v + delta) long.  Hence b_lo = T delta + (g_E - g_E'), the second term computed per leg."""
    worst_hi = worst_lo = -np.inf
    legs = 0
    for case in S.SCRIPT_CASES:
        if case[0] == 0:
            continue
        for kind in ("still", "greedy", "forward"):
            for e in run(kind, case)["envs"]:
                for leg in e.legs:
                    T, n, v = leg["steps"] - leg["waits"], leg["hops"], float(e.v)
                    assert 1 <= n <= T
                    (sx, sy), (wx, wy) = leg["start"], leg["target"]
                    g0 = Graph64(leg["rects"], wx, wy, 1e-9, 0.0).geo(sx, sy)
                    gE = Graph64(leg["rects"], wx, wy, E, E).geo(sx, sy)
                    gE2 = Graph64(leg["rects"], wx, wy, E + 2.0 ** -20, E + 2.0 ** -20).geo(sx, sy)
                    assert np.isfinite(g0) and gE2 <= gE <= g0 + 1e-12
                    delta = 8 * 2.0 ** -24 * v + 2.0 ** -21
                    b_hi = 40 * 2.0 ** -24 * g0 + T * (delta + 2.0 ** -22 * g0)
                    b_lo = T * delta + (gE - gE2)
                    assert (T - n) * v <= g0 + b_hi, (case, kind, leg, g0)
                    assert T * v >= gE - b_lo, (case, kind, leg, gE)
                    worst_hi, worst_lo = max(worst_hi, (T - n) * v - g0), max(worst_lo, gE - T * v)
                    legs += 1
    assert legs >= 50
    print(f"nav2d social walk: {legs} legs, (T - n) v - g_0 <= {worst_hi:.3e}, g_E - T v <= {worst_lo:.3e}")


# ---- rules at their boundaries ----------------------------------------------------------------------------------------------------------
SQUARE = [(3.0, 3.0, 5.0, 5.0)]


def test_a_person_on_a_node_leaves_it():
    """The person stands exactly on node 0 with the waypoint round the corner.  Node 0 at distance 0 would have the value DW[0], which
    is the value of the real hop by the field's fixed point: it is no candidate, and the person walks on."""
    x, y, ok = G.nodes([tuple(F(v) for v in SQUARE[0])])
    e = hand(SQUARE, (1.0, 7.0), (x[0], y[0]), waypoint=(7.0, 7.0))
    cands = dict(S.hop_candidates(e.hx, e.hy, e.world.rects, e.wx, e.wy, e.DW))
    assert ok[0] and np.isfinite(e.DW[0]) and 0 not in cands and S.WAYPOINT not in cands and cands
    assert min(cands.values()) == e.DW[0]      # the zero hop would have tied with the real one
    e.step(STILL)
    assert (e.hx, e.hy) != (x[0], y[0]) and e.person_lost == 0
    assert abs(float(R.dist(x[0], y[0], e.hx, e.hy)) - 0.125) < 1e-6


def test_ties_go_to_the_waypoint_then_to_the_lowest_node():
    """A square about (4, 4): from (1, 4) to (7, 4) the hops over nodes 0 and 2 have the same float32 value and node 0 is taken.  Along
    the line of the inflated box's lower side the direct hop and the hops over nodes 0 and 1 all have the value 6: the waypoint wins."""
    e = hand(SQUARE, (1.0, 7.0), (1.0, 4.0), waypoint=(7.0, 4.0))
    cands = S.hop_candidates(e.hx, e.hy, e.world.rects, e.wx, e.wy, e.DW)
    assert [i for i, _ in cands] == [0, 2] and cands[0][1] == cands[1][1]
    assert S.choose_hop(e.hx, e.hy, e.world.rects, e.wx, e.wy, e.DW)[0] == 0
    e.step(STILL)
    assert e.hy < 4.0
    _, y, _ = G.nodes(e.world.rects)
    e = hand(SQUARE, (1.0, 7.0), (1.0, y[0]), waypoint=(7.0, y[0]))
    cands = S.hop_candidates(e.hx, e.hy, e.world.rects, e.wx, e.wy, e.DW)
    assert [i for i, _ in cands][:3] == [S.WAYPOINT, 0, 1] and cands[0][1] == cands[1][1] == cands[2][1] == 6.0
    assert S.choose_hop(e.hx, e.hy, e.world.rects, e.wx, e.wy, e.DW)[0] == S.WAYPOINT


def test_a_short_hop_lands_exactly():
    """L <= v: the person is on the hop's end in both coordinates and the rest of the step is dropped; L just above v: a step of v."""
    e = hand([], (7.0, 7.0), (2.0, 2.0), waypoint=(2.09375, 2.0625))
    assert R.dist(e.hx, e.hy, e.wx, e.wy) < e.v
    e.step(STILL)
    assert e.arrivals == 1 and (e.hx, e.hy) == (F(2.09375), F(2.0625)) and e.wp_index == 1 and e.rebuilds == 1
    assert R.dist(e.hx, e.hy, e.wx, e.wy) >= 1.0
    e = hand([], (7.0, 7.0), (2.0, 2.0), waypoint=(2.125, 2.0))       # L == v exactly
    e.step(STILL)
    assert e.arrivals == 1 and (e.hx, e.hy) == (F(2.125), F(2.0))
    e = hand([], (7.0, 7.0), (2.0, 2.0), waypoint=(np.nextafter(F(2.125), F(3)), 2.0))
    e.step(STILL)
    assert e.arrivals == 0 and e.hy == 2.0 and abs(float(e.hx) - 2.125) < 1e-6 and e.hx != e.wx


def test_the_person_waits_below_the_keep_out_and_not_at_it():
    """The person at (0.75, 1) walks towards (0.5, 1): the next position is (0.625, 1) exactly.  An agent standing exactly 0.4 m
    (float32) from it is not in the way, one a float nearer is, step after step."""
    xs = [F(0.225)]
    for _ in range(8):
        xs = [np.nextafter(xs[0], F(0))] + xs + [np.nextafter(xs[-1], F(1))]
    at = max(x for x in xs if R.dist(F(0.625), F(1.0), x, F(1.0)) == S.KEEP_OUT)
    e = hand([], (at, 1.0), (0.75, 1.0), waypoint=(0.5, 1.0))
    e.step(STILL)
    assert e.person_waits == 0 and (e.hx, e.hy) == (F(0.625), F(1.0)) and R.dist(e.px, e.py, e.hx, e.hy) == S.KEEP_OUT
    near = next(x for x in xs if x > at and R.dist(F(0.625), F(1.0), x, F(1.0)) < S.KEEP_OUT)
    e = hand([], (near, 1.0), (0.75, 1.0), waypoint=(0.5, 1.0))
    for _ in range(3):
        e.step(STILL)
    assert e.person_waits == 3 and (e.hx, e.hy) == (0.75, 1.0) and e.arrivals == 0 and e.counters["waits"] == 3


def at_offset(dx, dy, rects=(), **kw):
    """An env whose agent looks along +x from (2, 2) with the person at (2 + dx, 2 + dy)."""
    return hand(list(rects), (2.0, 2.0), (F(2.0) + F(dx), F(2.0) + F(dy)), h=0, **kw)


def test_following_at_its_boundaries():
    """The agent at (px, 2) looks along +x; d = 1.0 and d = 2.0 follow, a float inside 1.0 or beyond 2.0 does not; |cross| = dot
    faces, a float more does not; behind and abeam do not."""
    up = lambda x: np.nextafter(F(x), F(9))
    for px, hx, hy, want in ((2.0, 3.0, 2.0, True), (up(2.0), 3.0, 2.0, False), (2.0, 4.0, 2.0, True), (2.0, up(4.0), 2.0, False),
                             (2.0, 3.0, 3.0, True), (2.0, 3.0, 1.0, True), (2.0, 3.0, up(3.0), False), (2.0, 0.5, 2.0, False),
                             (2.0, 2.0, 3.5, False)):
        e = hand([], (px, 2.0), (hx, hy), h=0)
        d, dot, cross, facing, sees, following = e.terms()
        assert following == want and sees == facing, (px, hx, hy)
        assert (dot, cross) == (F(F(hx) - F(px)), F(F(hy) - F(2.0))) and d == R.dist(px, 2.0, hx, hy)
    assert hand([], (2.0, 2.0), (3.0, 2.0)).terms()[0] == 1.0 and hand([], (2.0, 2.0), (4.0, 2.0)).terms()[0] == 2.0
    assert hand([], (up(2.0), 2.0), (3.0, 2.0)).terms()[0] < 1.0 and hand([], (2.0, 2.0), (up(4.0), 2.0)).terms()[0] > 2.0


def test_sees_stops_at_a_thin_wall():
    """A thin wall between the agent and the person, who is straight ahead at 1.5 m: facing, not seen, not following; both vector
    sensors are zero; with person_always_visible they are given, and the reward is the same."""
    wall = [(2.7, 1.0, 2.8, 3.0)]
    e, a = at_offset(1.5, 0.0, wall), at_offset(1.5, 0.0, wall, person_always_visible=True)
    d, dot, cross, facing, sees, following = e.terms()
    assert facing and not sees and not following and d == 1.5
    o, oa = e.observe(), a.observe()
    assert o["person_sensor"].tolist() == [0.0, 0.0] and o["person_visible"].tolist() == [0.0]
    assert oa["person_sensor"].tolist() == [1.5, 0.0] and oa["person_visible"].tolist() == [1.0]
    (o, r, _, _), (oa, ra, _, _) = e.step(STILL), a.step(STILL)
    assert r == ra and e.found == a.found == 0 and e.counters["facing_not_seen"] == 1
    assert o["person_visible"][0] == 0.0 and oa["person_visible"][0] == 1.0
    assert at_offset(1.5, 0.0).terms()[4:] == (True, True)      # without the wall


def test_the_four_terms_of_the_reward():
    """K = 0, the agent looks along +x and stands still, the person walks along +x away from it at 0.125 m a step."""
    v, slack = F(0.125), F(-0.01)
    # neither found nor following: the slack and the potential
    e = at_offset(2.5, 0.0, waypoint=(7.0, 2.0))
    _, r, _, _ = e.step(STILL)
    assert e.found == 0 and r == F(slack + F(F(2.5) - F(2.625))) == F(-0.135)
    # the step that sets found: the potential still counts, plus 2.5, plus 0.1
    e = at_offset(1.0, 0.0, waypoint=(7.0, 2.0))
    _, r, _, _ = e.step(STILL)
    assert e.found == 1 and e.first_encounter == 1 and r == F(F(F(slack + F(-0.125)) + F(2.5)) + F(0.1))
    # found before, following: no potential, 0.1
    _, r, _, _ = e.step(STILL)
    assert e.following_steps == 2 and r == F(F(slack + F(0.0)) + F(0.1))
    # found before, not following (the person has walked out of range): the slack alone; found stays
    while R.dist(e.px, e.py, e.hx, e.hy) <= 2.0:
        _, r, _, _ = e.step(STILL)
    assert r == slack and e.found == 1 and e.first_encounter == 1
    # approaching after found earns nothing either
    _, r, _, _ = e.step(FULL)
    assert r == slack or r == F(slack + F(0.1))


def test_found_is_sticky_and_first_encounter_steps():
    e = at_offset(1.5, 0.0, waypoint=(7.0, 2.0), max_episode_steps=6)
    e.step(STILL)
    assert e.found == 1
    for _ in range(4):
        e.step((-1.0, 1.0))      # turns away, 30 degrees a step
        assert e.found == 1
    assert not e.terms()[3]
    _, _, done, info = e.step(STILL)
    assert done and info == dict(has_found_person=1.0, following_rate=float(F(F(info["following_rate"] * 6) / F(6))),
                                 first_encounter_steps=1.0, collisions=0.0) and 0 < info["following_rate"] < 1
    # never found: the episode's step count
    e = hand([], (6.0, 2.0), (2.0, 2.0), h=0, waypoint=(2.0, 7.0), max_episode_steps=4)      # the person is behind the agent
    for _ in range(4):
        _, _, done, info = e.step(STILL)
    assert done and info == dict(has_found_person=0.0, following_rate=0.0, first_encounter_steps=4.0, collisions=0.0)


def test_without_obstacles_the_person_walks_straight():
    e = hand([], (7.0, 1.0), (1.0, 1.0), waypoint=(6.0, 6.0))
    assert e.sweeps == 0 and np.isinf(e.DW).all()
    for t in range(1, 40):
        e.step(STILL)
        assert abs(float(e.hx) - float(e.hy)) < 1e-5 and abs(float(e.hx) - (1.0 + t * 0.125 / np.sqrt(2))) < 1e-4
    assert e.arrivals == 0 and e.person_lost == 0


def test_a_walled_off_waypoint_is_given_up():
    """The waypoint inside a ring of four rectangles, the person outside: no candidate, so the person stays, person_lost counts, the
    next waypoint is drawn and its field built."""
    e = hand(G.RING, (1.0, 7.0), G.RING_OUTSIDE, waypoint=G.RING_INSIDE)
    assert not S.hop_candidates(e.hx, e.hy, e.world.rects, e.wx, e.wy, e.DW) and np.isinf(e.DW).all()
    e.step(STILL)
    assert e.person_lost == 1 and e.wp_index == 1 and e.rebuilds == 1 and (e.hx, e.hy) == G.RING_OUTSIDE
    assert (e.wx, e.wy) != G.RING_INSIDE and R.dist(e.hx, e.hy, e.wx, e.wy) >= 1.0
    rec = e.record()
    assert rec[S.W_PERSON_LOST] == 1 and rec[S.W_WAYPOINT_INDEX] == 1 and rec[S.W_REBUILDS] == 1 and rec[S.W_SWEEPS] == e.sweeps


def test_waypoints_keep_their_rules():
    """Every waypoint of 40 worlds: inside [0.5, 7.5]^2, in no rectangle grown by 0.3 m, at least 1 m from the person; a person who
    crowds the candidates' box gets a ring slot."""
    for env in range(40):
        w, objects, _, _, _ = S.O.make_world(5, env, 0, 8, 36, 1, 1)
        for j in range(4):
            x, y, _ = S.draw_waypoint(5, env, 0, j, objects[0][0], objects[0][1], w.rects)
            assert S.waypoint_fits(x, y, objects[0][0], objects[0][1], w.rects)
    big = [(1.0, 1.0, 7.0, 7.0)]
    x, y, fb = S.draw_waypoint(5, 0, 0, 0, F(0.5), F(0.5), big)
    assert fb and (x, y) == (1.5, 0.5)      # slot 0 is the person's own place, slot 1 the first one a metre away


# ---- the scripts ------------------------------------------------------------------------------------------------------------------------
def test_scripts_reach_every_event():
    """Over the scripts and cases that the GPU test replays, each event occurs at least 3 times (person_lost is covered by the
    hand-made world above)."""
    total = collections.Counter()
    for case in S.SCRIPT_CASES:
        for kind in ("forward", "greedy", "random", "grid", "still"):
            total.update(run(kind, case)["counters"])
    print("nav2d social events:", {k: total[k] for k in S.EVENTS + S.OTHER_COUNTERS})
    for k in S.EVENTS:
        assert total[k] >= 3, k
    per_K = {K: collections.Counter() for K in (0, 3, 8)}
    for case in S.SCRIPT_CASES:
        for kind in ("forward", "greedy", "random", "grid", "still"):
            per_K[case[0]].update(run(kind, case)["counters"])
    assert per_K[0]["node_hops"] == 0 and per_K[0]["facing_not_seen"] == 0 and per_K[3]["node_hops"] >= 3 and per_K[8]["node_hops"] >= 3


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Every parameter the env refuses, with a message that names the task, before the device is touched; the geodesic mode, with
    the reason; a device that is no GPU; and the restatement alike."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    bad = [(dict(distance="geodesic"), "field per step"), (dict(distance="manhattan"), "distance"), (dict(num_actions=4), "velocity_control"),
           (dict(turn_angle=7), "turn_angle"), (dict(turn_angle=0), "turn_angle"), (dict(num_obstacles=9), "num_obstacles"),
           (dict(num_obstacles=-1), "num_obstacles"), (dict(max_episode_steps=0), "max_episode_steps"),
           (dict(max_turn_angle=0), "max_turn_angle"), (dict(max_turn_angle=181), "max_turn_angle"), (dict(max_turn_angle=10.0), "max_turn_angle"),
           (dict(turn_angle=4, max_turn_angle=10), "max_turn_angle"), (dict(min_abs_ang_speed=0), "min_abs_ang_speed"),
           (dict(min_abs_ang_speed=11), "min_abs_ang_speed"), (dict(min_abs_lin_speed=0.0), "min_abs_lin_speed"),
           (dict(min_abs_lin_speed=0.26), "min_abs_lin_speed"), (dict(min_abs_lin_speed=True), "min_abs_lin_speed"),
           (dict(allow_sliding=1), "allow_sliding"), (dict(person_speed=0.0), "person_speed"), (dict(person_speed=-0.1), "person_speed"),
           (dict(person_speed=0.26), "person_speed"), (dict(person_speed="slow"), "person_speed"), (dict(person_speed=True), "person_speed"),
           (dict(person_speed=float("nan")), "person_speed"), (dict(person_always_visible=1), "person_always_visible"),
           (dict(person_always_visible="yes"), "person_always_visible")]
    for kw, text in bad:
        with pytest.raises(_lib.HabError, match=text) as err:
            EF.Nav2DSocialVectorEnv(2, 8, 8, device="cpu", **kw)
        assert "Nav2DSocial" in str(err.value) or text in ("turn_angle", "num_obstacles", "max_episode_steps"), kw
        assert "Nav2DVel:" not in str(err.value), kw
    for size in ((0, 8), (8, 0)):
        with pytest.raises(_lib.HabError, match="image size"):
            EF.Nav2DSocialVectorEnv(2, *size, device="cpu")
    for kw in (dict(), dict(person_speed=0.25, person_always_visible=True, num_obstacles=8, turn_angle=10, max_turn_angle=30, min_abs_ang_speed=10)):
        with pytest.raises(_lib.HabError, match="Nav2DSocial.*built on the GPU"):   # valid parameters: only the missing device is refused
            EF.Nav2DSocialVectorEnv(2, 8, 8, device="cpu", **kw)
    for kw in (dict(turn_angle=7), dict(person_speed=0.0), dict(person_speed=0.3), dict(person_always_visible=1), dict(allow_sliding=1),
               dict(min_abs_ang_speed=11), dict(num_obstacles=9)):
        with pytest.raises(ValueError):
            S.Nav2DSocialEnv(1, 0, **kw)
    e = S.Nav2DSocialEnv(1, 0)
    e.reset()
    for a in ((0.0,), (0.0, 0.0, 0.0), 1, [[0.0, 0.0]]):
        with pytest.raises(ValueError):
            e.step(a)
    # the host path takes a length-2 array or {"action": array}; the goal-sensor forms and pausing are refused
    env = EF.Nav2DSocialVectorEnv.__new__(EF.Nav2DSocialVectorEnv)
    env.num_envs, env._pending, env._actions_host = 3, set(), np.zeros((3, 2), np.float32)
    env.async_step_at(0, np.array([0.5, -2.0], np.float32))
    env.async_step_at(2, {"action": [0.25, 0.0]})
    assert env._pending == {0, 2} and env._actions_host.tolist() == [[0.5, -2.0], [0.0, 0.0], [0.25, 0.0]]
    for a in (1, [0.0], [0.0] * 3, [[0.0, 0.0]], "abc", None):
        with pytest.raises(_lib.HabError, match="length-2"):
            env.async_step_at(1, a)
    for call in (lambda: env.reset_into(None, None, None), lambda: env.step_into(None, None, None, None, None),
                 lambda: env.step_into_obs({}, None, None), lambda: env.pause_at(0)):
        with pytest.raises(_lib.HabError, match="Nav2D"):
            call()


def test_factory_choice_and_yaml(monkeypatch):
    """The YAML loads with every key the task reads; a habitat.task.type starting with "nav2dsocial" (any case) picks the new env --
    it built Nav2D-v0 before -- while the other Nav2D tasks keep theirs; the keys reach the class; the image size comes from head_rgb,
    else head_depth, else nothing is rendered; the geodesic key is refused.  The constructors are replaced by recorders."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    from habitat_amd.config.default import get_config
    from habitat_amd.rl.ppo.ppo_trainer import PPOTrainer
    assert "Nav2DSocial-v0" in PPOTrainer.supported_tasks
    name = "social_nav/ddppo_nav2d_social.yaml"
    cfg = get_config(name)
    hab, hb = cfg.habitat, cfg.habitat_baselines
    assert hab.task.type == "Nav2DSocial-v0" and list(hab.task.actions) == ["velocity_control"]
    assert hab.simulator.sensors.head_depth.height == hab.simulator.sensors.head_depth.width == 64 and "head_rgb" not in hab.simulator.sensors
    agent = hb.rl.policy.main_agent
    assert agent.name == "PointNavResNetPolicy" and agent.action_distribution_type == "gaussian" and hb.rl.ddppo.backbone == "resnet18"
    assert list(agent.fuse_keys) == ["head_depth", "person_sensor", "person_visible"]
    vel = get_config("pointnav/ppo_nav2d_vel.yaml")
    assert dict(agent.action_dist) == dict(vel.habitat_baselines.rl.policy.main_agent.action_dist)
    syn = {k: hab.synthetic[k] for k in ("turn_angle", "max_turn_angle", "min_abs_lin_speed", "min_abs_ang_speed", "allow_sliding")}
    assert syn == {k: vel.habitat.synthetic[k] for k in syn}
    assert hab.synthetic.person_speed == 0.125 and hab.synthetic.person_always_visible is False and hab.synthetic.distance_to_goal == "euclidean"
    made = []
    for cls in ("Nav2DSocialVectorEnv", "Nav2DRearrVelVectorEnv", "Nav2DRearrVectorEnv", "Nav2DObjVectorEnv", "Nav2DVelVectorEnv",
                "Nav2DVectorEnv", "SyntheticVectorEnv"):
        monkeypatch.setattr(EF, cls, lambda *a, _n=cls, **kw: made.append((_n, a, kw)) or _n)
    factory = EF.SyntheticVectorEnvFactory()
    assert factory.construct_envs(cfg, device="cpu") == "Nav2DSocialVectorEnv"
    _, args, kw = made[-1]
    assert args == (16, 64, 64) and kw["num_actions"] == 1 and kw["max_episode_steps"] == 200
    assert {k: kw[k] for k in ("num_obstacles", "turn_angle", "max_turn_angle", "min_abs_lin_speed", "min_abs_ang_speed", "allow_sliding",
                               "person_speed", "person_always_visible", "use_rgb", "use_depth", "distance")} == dict(
        num_obstacles=3, turn_angle=1, max_turn_angle=10, min_abs_lin_speed=0.025, min_abs_ang_speed=5, allow_sliding=True,
        person_speed=0.125, person_always_visible=False, use_rgb=False, use_depth=True, distance="euclidean")
    for task_type, want in (("nav2dsocial", "Nav2DSocialVectorEnv"), ("NAV2DSOCIAL-v7", "Nav2DSocialVectorEnv"),
                            ("Nav2DSocia-v0", "Nav2DVectorEnv"), ("Nav2DRearrVel-v0", "Nav2DRearrVelVectorEnv"),
                            ("Nav2DRearr-v0", "Nav2DRearrVectorEnv"), ("Nav2DVel-v0", "Nav2DVelVectorEnv"), ("Nav2D-v0", "Nav2DVectorEnv")):
        assert factory.construct_envs(get_config(name, [f"habitat.task.type={task_type}"]), device="cpu") == want, task_type
    # the image size: head_rgb first, then head_depth, then none
    both = get_config(name, ["habitat.simulator.sensors.head_rgb.height=32", "habitat.simulator.sensors.head_rgb.width=48"])
    assert factory.construct_envs(both, device="cpu") == "Nav2DSocialVectorEnv" and made[-1][1] == (16, 32, 48) and made[-1][2]["use_rgb"]
    assert EF.SyntheticVectorEnvFactory(use_rgb=False, use_depth=False).construct_envs(both, device="cpu") == "Nav2DSocialVectorEnv"
    assert made[-1][1] == (16, 0, 0) and not made[-1][2]["use_rgb"] and not made[-1][2]["use_depth"]
    # the keys reach the class
    ov = get_config(name, ["habitat.synthetic.person_speed=0.2", "habitat.synthetic.person_always_visible=True"])
    factory.construct_envs(ov, device="cpu")
    assert made[-1][2]["person_speed"] == 0.2 and made[-1][2]["person_always_visible"] is True
    monkeypatch.undo()
    with pytest.raises(_lib.HabError, match="target moves every step"):
        factory.construct_envs(get_config(name, ["habitat.synthetic.distance_to_goal=geodesic"]), device="cpu")
    with pytest.raises(_lib.HabError, match="Nav2DSocial"):     # and no longer Nav2D-v0's refusal of a missing GPU
        factory.construct_envs(cfg, device="cpu")


def test_the_yaml_gives_a_box_of_two(monkeypatch):
    """The factory on the YAML with the device side of the constructor stubbed out (no GPU here): a Nav2DSocialVectorEnv whose action
    space is Box(-1, 1, (2,), float32), with a float32 (N, 2) host action table and the entry's task parameters in the entry's order."""
    import torch
    from habitat_amd.common import env_factory as EF, spaces
    from habitat_amd.config.default import get_config

    def fake_init(self, num_envs, height, width, **kw):
        self.num_envs, self.received = num_envs, dict(kw, height=height, width=width)
        self.action_spaces = [EF.spaces.Discrete(4)] * num_envs
    monkeypatch.setattr(EF.Nav2DVectorEnv, "__init__", fake_init)
    cfg = get_config("social_nav/ddppo_nav2d_social.yaml", ["habitat.synthetic.turn_angle=5", "habitat.synthetic.max_turn_angle=30",
                                                            "habitat.synthetic.min_abs_ang_speed=10", "habitat.synthetic.person_speed=0.25"])
    env = EF.SyntheticVectorEnvFactory().construct_envs(cfg, device="cpu")
    assert type(env) is EF.Nav2DSocialVectorEnv and env.consumes_actions and env.task == "nav2dsocial"
    assert len(env.action_spaces) == 16 and env.orig_action_spaces is env.action_spaces
    for sp in env.action_spaces:
        assert isinstance(sp, EF.spaces.Box) and sp.shape == (2,) and sp.dtype == np.float32
        assert sp.low.tolist() == [-1.0] * 2 and sp.high.tolist() == [1.0] * 2
        assert spaces.is_continuous_action_space(sp) and spaces.get_action_space_info(sp) == ((2,), False)
    assert env._actions_host.shape == (16, 2) and env._actions_host.dtype == np.float32
    assert env.received["turn_angle"] == 5 and (env.received["height"], env.received["width"]) == (64, 64) and "distance" not in env.received
    assert env._task_parameters() == (6, 2, 0.025, 1, 0.25, 0)
    assert env._entries == ("hab_nav2d_social_step",) and env._action_dtype is torch.float32 and env._sensor_set == "social"
    assert env._state_bytes == "hab_nav2d_social_state_bytes" and env.measure_names == S.MEASURES and env.num_actions == 1
    assert env._actions_shaped(torch.zeros(16, 2)) and not env._actions_shaped(torch.zeros(16, 3)) and not env._actions_shaped(torch.zeros(32))


def test_observation_space_and_policy_tables():
    """The sensor set "social" of SyntheticVectorEnv, built before the constructor asks for the device, which is what is missing here;
    resolve_sensors on it gives the visual table [head_rgb?, head_depth] and the fused widths (2, 1): D = 3; the YAML's fuse_keys give
    the same tables, and the two vectors alone a blind policy."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    from habitat_amd.config.default import get_config
    from habitat_amd.rl.ppo.policy import resolve_sensors
    for use_rgb in (False, True):
        env = EF.SyntheticVectorEnv.__new__(EF.SyntheticVectorEnv)
        with pytest.raises(_lib.HabError, match="GPU"):
            EF.SyntheticVectorEnv.__init__(env, 3, 10, 12, use_rgb=use_rgb, device="cpu", task=EF.Nav2DSocialVectorEnv._sensor_set)
        sp = env.observation_spaces[0]
        want = (["head_rgb"] if use_rgb else []) + ["head_depth", "person_sensor", "person_visible"]
        assert list(sp.spaces) == want and (env.H, env.W) == (10, 12)
        assert sp["head_depth"].shape == (10, 12, 1) and sp["head_depth"].dtype == np.float32
        assert sp["person_sensor"].shape == (2,) and sp["person_visible"].shape == (1,)
        assert all(sp[k].dtype == np.float32 for k in want[-2:]) and sp["person_visible"].low.min() == 0.0 and sp["person_visible"].high.max() == 1.0
        visual, fused = resolve_sensors(sp)
        assert [v[0] for v in visual] == want[:-2] and [v[2] for v in visual] == ([3, 1] if use_rgb else [1])
        assert fused == [("person_sensor", 2), ("person_visible", 1)]
        if not use_rgb:
            keys = list(get_config("social_nav/ddppo_nav2d_social.yaml").habitat_baselines.rl.policy.main_agent.fuse_keys)
            assert resolve_sensors(sp, keys) == (visual, fused)
            assert resolve_sensors(sp, ["person_sensor", "person_visible"]) == ([], fused)
    assert EF.NAV2D_SOCIAL_SENSORS == S.SENSORS and EF.NAV2D_SOCIAL_MEASURES == S.MEASURES


def test_header_and_signature_table_agree():
    """The header's prototype of hab_nav2d_social_step and the ctypes table: the same number of arguments, pointers where the header
    has pointers, the two uint32, the floats and the ints in their places; the arguments are hab_nav2d_vel_step's with the two vector
    sensors in the goal sensor's place and person_speed, person_always_visible before advance; the named words are the restatement's."""
    from habitat_amd import _lib
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "habitat_amd.h")).read()

    def names_of(entry):
        m = re.search(r"int %s\((.*?)\);" % entry, text, re.S)
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
        return params, [p.split()[-1].lstrip("*") for p in params]

    params, names = names_of("hab_nav2d_social_step")
    restype, argtypes = _lib.SIGNATURES["hab_nav2d_social_step"]
    assert restype is ctypes.c_int and len(params) == len(argtypes) == 30
    for p, t in zip(params, argtypes):
        if "*" in p or p.startswith("hipStream_t"):
            assert t is ctypes.c_void_p, p
        elif p.startswith("uint32_t"):
            assert t is ctypes.c_uint32, p
        elif p.startswith("float "):
            assert t is ctypes.c_float, p
        else:
            assert p.startswith("int ") and t is ctypes.c_int, p
    _, vel = names_of("hab_nav2d_vel_step")
    want = [{"rgb": "head_rgb", "depth": "head_depth"}.get(n, n) for n in vel]
    i, j = want.index("goal"), want.index("advance")
    assert names == want[:i] + ["person_sensor", "person_visible"] + want[i + 1:j] + ["person_speed", "person_always_visible"] + want[j:]
    assert params[names.index("actions")].startswith("const float*") and params[names.index("person_speed")].startswith("float ")
    words = dict(re.findall(r"#define HAB_NAV2D_SOCIAL_(\w+) (\d+)", text))
    assert {k: int(v) for k, v in words.items()} == dict(
        STATE_BYTES=4 * S.STATE_WORDS, W_START=S.W_START, W_PERSON=S.W_PERSON, W_WAYPOINT=S.W_WAYPOINT, W_WAYPOINT_INDEX=S.W_WAYPOINT_INDEX,
        W_FOUND=S.W_FOUND, W_FOLLOWING_STEPS=S.W_FOLLOWING_STEPS, W_FIRST_ENCOUNTER=S.W_FIRST_ENCOUNTER, W_ARRIVALS=S.W_ARRIVALS,
        W_PERSON_WAITS=S.W_PERSON_WAITS, W_PERSON_LOST=S.W_PERSON_LOST, W_SWEEPS=S.W_SWEEPS, W_REBUILDS=S.W_REBUILDS, W_DW=S.W_DW)
    assert _lib.lib().hab_nav2d_social_state_bytes() == 4 * S.STATE_WORDS
