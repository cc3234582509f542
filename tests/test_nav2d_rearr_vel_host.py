"""CPU: the Nav2DRearrVel-v0 restatement (tests/nav2d_rearr_vel_reference.py) holds its own invariants, the scripted sequences the GPU
tests replay reach every branch of the task, and the Python surface (parameters, factory, YAML, action and observation space, signature
table) behaves without a device."""
import functools
import os
import re

import numpy as np
import pytest

import nav2d_obj_reference as O
import nav2d_reference as R
import nav2d_rearr_reference as A
import nav2d_rearr_vel_reference as B
import nav2d_vel_reference as V

F = np.float32
ONE_TURN = dict(turn_angle=30, max_turn_angle=30, min_abs_ang_speed=30)   # M = S = 1: a_ang = +-1 is one heading, anything less none


def blind(seed=3, env=0, **kw):
    e = B.Nav2DRearrVelEnv(seed, env, **dict(dict(num_obstacles=3, max_episode_steps=40), **kw))
    e.reset()
    return e


def put(e, px, py, h, ox=None, oy=None, holding=0):
    """Moves the agent (and the unheld object) of a K = 0 env to a chosen pose; the potential is brought up to date."""
    e.px, e.py, e.h, e.holding = F(px), F(py), h % e.nh, holding
    e.ox, e.oy = (e.px, e.py) if holding else (F(ox), F(oy))
    e.held = max(e.held, holding)
    e.phi_prev = e.potential()[0]
    return e


def grip_at(e, h, grip):
    """One step that is no stop and moves nothing: a zero-length move (c_lin = -1, so l = 0 and the target is p itself) after one
    turn to the left that ends at heading h, with the grip component `grip`.  For envs built with ONE_TURN."""
    e.h = (h - 1) % e.nh
    p = (e.px, e.py)
    out = e.step((-1.0, 1.0, grip))
    assert not out[2] and e.h == h % e.nh and (e.px, e.py) == p and e.last_dh == 1
    return out


@pytest.mark.parametrize("K,start_holding,sliding", [(0, False, True), (3, True, True), (8, False, False), (8, True, True)])
def test_world_invariants(K, start_holding, sliding):
    """500 steps each of the four scripts: after every step the agent is free, never within 0.4 m of an unheld object, a placed object
    is inside its box and outside the grown rectangles, h is 0 or 1, a held object is at p, and the path length grew by at most the
    step length."""
    rng = np.random.RandomState(K)
    counters = {}
    for params in B.PARAMETER_SETS:
        turn, max_turn, min_ang = params
        for kind in B.SCRIPTS:
            e = blind(seed=7, num_obstacles=K, start_holding=start_holding, allow_sliding=sliding, turn_angle=turn, max_turn_angle=max_turn,
                      min_abs_ang_speed=min_ang, max_episode_steps=100)
            sc, obs = B.make_script(kind, max_turn, rng), e.observe()
            for _ in range(500):
                path, episode = e.path, e.episode
                a = sc(obs, e)
                obs, _, done, _ = e.step(a)
                if done:
                    sc.episode_ended()
                assert e.holding in (0, 1) and e.held in (0, 1) and e.held >= e.holding
                assert R.is_free(e.px, e.py, e.world.rects)
                if e.episode == episode:
                    assert path <= e.path <= F(path + B.decode(a, e.M)[0])
                if e.holding:
                    assert (e.ox, e.oy) == (e.px, e.py) and obs["is_holding"][0] == 1.0
                else:
                    assert not R.dist(e.px, e.py, e.ox, e.oy) < O.OBJ_BLOCK and obs["is_holding"][0] == 0.0
                    assert 0.5 <= e.ox <= 7.5 and 0.5 <= e.oy <= 7.5 and not A.in_grown_rect(e.ox, e.oy, e.world.rects)
            counters = {k: counters.get(k, 0) + v for k, v in e.counters.items()}
    assert counters["place_ok"] > 0 and counters["pick_bonus"] > 0 and counters["episodes"] >= 15
    assert (counters["slide_x"] + counters["slide_y"] > 0) == sliding


def test_rewards_telescope():
    """Per episode, in float64: sum r = -0.01 * len + Phi_0 - Phi_T + 1.0 * [a first PICK happened] + 2.5 * success.  The bound is
    derived as Nav2DRearr-v0's test derives its own: each Phi is the same float32 in both of its terms, so the potentials cancel
    exactly and what is left are the roundings of each step's reward.  Phi < 32.  One step changes it by less than 2.25: the move
    changes d(p, o) or d(p, g) by at most 0.25; a PICK after it replaces d(p, o) + d(o, g) by d(p, g), which the triangle inequality
    puts within d(p, o) < 1 of d(o, g), so the step's change is below 0.25 + 2 * 1; a PLACE after it replaces d(p, g) by
    0.5 + d(q, g), within 0.5 + 0.5.  So Phi_prev - Phi (below 4) rounds by at most 2^-23, -0.01 + that (below 4) by at most 2^-23 and
    -0.01 itself is off by less than 2^-31 as a float32; adding the bonuses is exact where they are 0 and rounds by at most 2^-23
    (the pick, a sum below 4) and 2^-22 (the success, a sum below 8) on the one step each that carries them."""
    rng = np.random.RandomState(1)
    seen = set()
    for kind, sh, K in (("sensor", True, 0), ("sensor", False, 3), ("grip", True, 3), ("random", False, 8), ("wall", True, 8)):
        e = blind(seed=11, env=1, num_obstacles=K, start_holding=sh, turn_angle=10, max_turn_angle=30, min_abs_ang_speed=10,
                  max_episode_steps=80)
        sc, obs = B.make_script(kind, 30, rng), e.observe()
        for _ in range(10):
            phi0, total, n = float(e.phi_start), 0.0, 0
            while True:
                obs, r, done, info = e.step(sc(obs, e))
                total, n = total + float(r), n + 1
                if done:
                    sc.episode_ended()
                    break
            L = e.last
            bonus = L["picks"] > 0
            closed = -0.01 * n + phi0 - float(L["phi_end"]) + 1.0 * bonus + 2.5 * info["success"]
            bound = n * (2.0 ** -23 + 2.0 ** -23 + 2.0 ** -31) + 2.0 ** -23 + 2.0 ** -22
            assert L["length"] == n and abs(total - closed) <= bound, (kind, total, closed, bound)
            seen.add((bonus, info["success"]))
    assert {(True, 1.0), (False, 1.0), (False, 0.0), (True, 0.0)} <= seen


def phi_of(e, px, py, ox, oy):
    return F(R.dist(F(px), F(py), F(ox), F(oy)) + R.dist(F(ox), F(oy), e.gx, e.gy))


def test_pick_rules_at_their_boundaries():
    """Reach just below and at 1.0; the front half-plane just above and at 0; the bonus on the first PICK of an episode only.  A
    refused PICK changes nothing but `invalid`."""
    e = blind(num_obstacles=0, **ONE_TURN)
    below = float(np.nextafter(F(3.0), F(0.0)))
    put(e, 2.0, 2.0, 0, below, 2.0)                        # d = 1 - 2^-22, the nearest this pose comes to 1 from below: in reach
    assert F(1.0) - R.dist(e.px, e.py, e.ox, e.oy) == F(2.0 ** -22)
    _, r, _, _ = grip_at(e, 0, 1.0)
    assert e.holding == 1 and e.held == 1 and e.picks == 1 and e.invalid == 0 and (e.ox, e.oy) == (e.px, e.py)
    assert r == F(F(F(R.SLACK + F(phi_of(e, 2.0, 2.0, below, 2.0) - e.phi_prev)) + F(1.0)) + F(0.0))
    put(e, 2.0, 2.0, 0, 3.0, 2.0)                          # d = 1.0 exactly: out of reach
    before = e.state_words()
    grip_at(e, 0, 1.0)
    after = e.state_words()
    assert e.holding == 0 and e.invalid == 1 and after["flags"].tolist() == [0, 1, 1, 1] and e.counters["pick_far"] == 1
    assert np.array_equal(before["pos"], after["pos"]) and np.array_equal(before["places"], after["places"])
    above = float(np.nextafter(F(2.0), F(3.0)))
    put(e, 2.0, 2.0, 0, 2.0, 2.5)                          # abeam: dx = 0, so dot = 0 * 1 + 0.5 * 0 = 0, not > 0
    grip_at(e, 0, 1.0)
    assert e.holding == 0 and e.invalid == 2 and e.counters["pick_behind"] == 1
    put(e, 2.0, 2.0, 0, above, 2.5)                        # dx = 2^-22: dot is just above 0
    grip_at(e, 0, 1.0)
    assert e.holding == 1 and e.invalid == 2 and e.picks == 2 and e.counters["pick_again"] == 1
    put(e, 2.0, 2.0, 0, 1.5, 2.0)                          # behind: dot < 0
    grip_at(e, 0, 0.01)
    assert e.holding == 0 and e.invalid == 3 and e.counters["pick_behind"] == 2
    grip_at(e, 6, 0.01)                                    # the same pose seen after the half turn: ahead (any positive grip closes)
    assert e.holding == 1 and e.picks == 3
    # the second PICK of an episode carries no bonus: the PLACE puts the object back where it was picked from
    e2 = blind(num_obstacles=0, **ONE_TURN)
    put(e2, 2.0, 2.0, 0, 2.5, 2.0)
    _, r1, _, _ = grip_at(e2, 0, 1.0)
    grip_at(e2, 0, -1.0)
    assert (e2.ox, e2.oy) == (2.5, 2.0) and e2.holding == 0
    _, r2, _, _ = grip_at(e2, 0, 1.0)
    assert e2.picks == 2 and r1 == F(r2 + F(1.0)) and r2 < 0.5 and e2.counters["pick_again"] == 1 and e2.counters["pick_bonus"] == 1


def test_place_rules_at_their_boundaries():
    """q on the arena box's edge and one float beyond it; q on the edge of a grown rectangle and one float inside it; a successful
    PLACE puts o at p + 0.5 * dir, multiply then add."""
    e = blind(num_obstacles=0, **ONE_TURN)
    put(e, 7.0, 2.0, 0, holding=1)                         # q.x = 7.5: on the box's edge, inside
    grip_at(e, 0, -1.0)
    assert e.holding == 0 and (e.ox, e.oy) == (7.5, 2.0) and e.invalid == 0 and e.counters["place_ok"] == 1
    beyond = float(np.nextafter(F(7.0), F(8.0)))
    put(e, beyond, 2.0, 0, holding=1)                      # q.x = 7.5 + 2^-21 > 7.5
    assert F(F(beyond) + F(0.5)) > F(7.5)
    grip_at(e, 0, -1.0)
    assert e.holding == 1 and e.invalid == 1 and e.counters["place_outside_box"] == 1 and (e.ox, e.oy) == (e.px, e.py)
    put(e, 2.0, 0.75, 9, holding=1)                        # heading 270 degrees: q.y = 0.75 + 0.5 * (-1) = 0.25 < 0.5
    grip_at(e, 9, -1.0)
    assert e.holding == 1 and e.invalid == 2 and e.counters["place_outside_box"] == 2
    e = blind(num_obstacles=0, **ONE_TURN)
    e.world.rects = [(F(3.0), F(3.0), F(4.0), F(4.0))]
    edge = F(F(3.0) - O.OBJ_R)                             # the grown rectangle's left side, the expression of the test
    on = F(edge - F(0.5))
    assert F(on + F(0.5)) == edge and R.is_free(on, F(3.5), e.world.rects)
    put(e, on, 3.5, 0, holding=1)                          # q.x = the edge itself: not strictly inside
    grip_at(e, 0, -1.0)
    assert e.holding == 0 and (e.ox, e.oy) == (edge, 3.5) and e.invalid == 0
    inside = np.nextafter(on, F(8.0))
    assert F(inside + F(0.5)) > edge
    put(e, inside, 3.5, 0, holding=1)                      # q.x one float past the edge: strictly inside
    grip_at(e, 0, -1.0)
    assert e.holding == 1 and e.invalid == 1 and e.counters["place_in_rect"] == 1
    c, s = e.dirs[1]
    put(e, 5.0, 5.0, 1, holding=1)
    grip_at(e, 1, -0.01)                                   # any negative grip opens
    assert (e.ox, e.oy) == (F(F(5.0) + F(F(0.5) * c)), F(F(5.0) + F(F(0.5) * s))) and e.holding == 0
    assert not R.dist(e.px, e.py, e.ox, e.oy) < O.OBJ_BLOCK


def test_noop_grips_change_and_count_nothing():
    """c_grip == 0 (also -0, nan and the infinities, which act as 0), c_grip > 0 while holding and c_grip < 0 with empty hands leave
    holding, the object, picks and `invalid` alone, in reach of the object and facing a wall alike."""
    e = blind(num_obstacles=0, **ONE_TURN)
    put(e, 2.0, 2.0, 0, 2.5, 2.0)                          # the object in reach and ahead
    for g in (0.0, -0.0, np.nan, -1.0, -0.3, -7.0):
        grip_at(e, 0, g)
        assert e.holding == 0 and (e.ox, e.oy) == (2.5, 2.0)
    put(e, 7.4, 2.0, 0, holding=1)                         # a PLACE here would be refused: q.x = 7.9
    for g in (0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, 0.3, 7.0):
        grip_at(e, 0, g)
        assert e.holding == 1 and (e.ox, e.oy) == (e.px, e.py)
    assert e.invalid == 0 and e.picks == 0 and e.state_words()["flags"].tolist() == [1, 1, 0, 0]
    c = e.counters
    assert (c["noop_zero"], c["noop_place_empty"], c["noop_pick_holding"]) == (3 + 5, 3, 3)
    grip_at(e, 0, -np.float32(1e-30))                      # the smallest grips still count: a refused PLACE
    assert e.invalid == 1 and e.holding == 1


@pytest.mark.parametrize("start_holding", [False, True])
def test_start_holding_and_did_pick_object(start_holding):
    """Under start_holding every episode begins with h = 1, o = p, Phi_0 = d(p, g) and did_pick_object = 1 whatever happens; without
    it the measure is 1 exactly in the episodes with a successful PICK."""
    e = blind(seed=5, num_obstacles=3, start_holding=start_holding, turn_angle=10, max_turn_angle=30, min_abs_ang_speed=10,
              max_episode_steps=30)
    rng = np.random.RandomState(2)
    sc, obs, infos = B.make_script("sensor", 30, rng), e.observe(), []
    for _ in range(12):
        assert e.holding == int(start_holding) == e.held and e.picks == 0
        assert (e.ox, e.oy) == ((e.px, e.py) if start_holding else (e.o0x, e.o0y))
        assert e.phi_start == (R.dist(e.px, e.py, e.gx, e.gy) if start_holding else
                               F(R.dist(e.px, e.py, e.o0x, e.o0y) + R.dist(e.o0x, e.o0y, e.gx, e.gy)))
        while True:
            obs, _, done, info = e.step(sc(obs, e))
            if done:
                infos.append(dict(info, picks=e.last["picks"]))
                break
    if start_holding:
        assert all(i["did_pick_object"] == 1.0 for i in infos)
    else:
        assert all(i["did_pick_object"] == float(i["picks"] > 0) for i in infos) and {i["did_pick_object"] for i in infos} == {0.0, 1.0}
    e = blind(seed=5, num_obstacles=0, start_holding=start_holding, max_episode_steps=3)
    for _ in range(3):
        _, _, done, info = e.step((-1.0, 1.0, 0.0))        # turns on the spot until the step limit
    assert done and info["did_pick_object"] == float(start_holding) and info["success"] == 0.0 and e.counters["timeouts"] == 1


def test_release_and_stop_succeeds_in_one_step():
    """(a_lin, a_ang, a_grip) = (-1, 0, -1) is a stop and a release: the grip is evaluated on the stop step too, so holding the object
    half a metre in front of the goal it ends the episode with success and the 2.5; the same stop with the grip closed, or too far
    from the goal, ends it without."""
    def at_goal(grip, back=0.5):
        e = blind(seed=4, num_obstacles=0, start_holding=True, **ONE_TURN)
        put(e, e.gx - F(back), e.gy, 0, holding=1)
        phi_prev, g = e.phi_prev, (e.gx, e.gy)
        _, r, done, info = e.step((-1.0, 0.0, grip))
        return e, phi_prev, g, r, done, info

    e, phi_prev, (gx, gy), r, done, info = at_goal(-1.0)
    q = F(F(gx - F(0.5)) + F(F(0.5) * F(1.0)))
    b = R.dist(q, gy, gx, gy)
    phi = F(R.dist(F(gx - F(0.5)), gy, q, gy) + b)
    assert done and info == dict(success=1.0, did_pick_object=1.0, object_to_goal_distance=float(b), collisions=0.0) and b < 0.5
    assert r == F(F(F(R.SLACK + F(phi_prev - phi)) + F(0.0)) + R.SUCCESS_REWARD)
    assert e.counters["release_and_stop"] == 1 and e.counters["successes"] == 1 and e.episode == 1 and e.steps == 0
    e, _, _, r, done, info = at_goal(1.0)                  # the grip stays closed: a stop while holding
    assert done and info["success"] == 0.0 and r == R.SLACK and e.counters["stop_holding"] == 1
    e, _, _, r, done, info = at_goal(-1.0, back=1.5)       # released a metre short of the goal
    assert done and info["success"] == 0.0 and info["object_to_goal_distance"] == 1.0 and e.counters["stop_too_far"] == 1
    e = blind(seed=4, num_obstacles=0, start_holding=True, **ONE_TURN)
    put(e, e.gx - F(0.5), e.gy, 0, holding=1)
    assert not e.step((-1.0, 1.0, -1.0))[2] and e.holding == 0 and e.counters["successes"] == 0   # no stop, no success: it turned


def twin_steps(a, b, **kw):
    """The state words, reward, done and sensors of one step with action a and of one with b, on two copies of one env."""
    out = []
    for act in (a, b):
        e = blind(seed=6, num_obstacles=3, **kw)
        for warm in ((1.0, 0.3, 1.0), (0.5, -0.6, -1.0)):
            e.step(warm)
        o, r, done, _ = e.step(act)
        out.append((e.state_words(), r, done, o))
    return out


def same(x, y):
    return (all(np.array_equal(x[0][k].view(np.int32), y[0][k].view(np.int32)) for k in x[0]) and x[1] == y[1] and x[2] == y[2]
            and all(np.array_equal(x[3][k], y[3][k]) for k in x[3]))


def test_clamp_ties_and_nonfinite_components():
    """Components outside the Box act as the nearest bound; a non-finite component acts as 0; rint(c_ang * M) rounds halves to even;
    the step length is (c_lin + 1) * 0.125, an add and then a multiply."""
    for a, b in (((3.0, -7.0, 5.0), (1.0, -1.0, 1.0)), ((-1.5, 1.0001, -1e30), (-1.0, 1.0, -1.0)),
                 ((np.nan, 0.4, 1.0), (0.0, 0.4, 1.0)), ((0.4, np.inf, 1.0), (0.4, 0.0, 1.0)), ((0.4, -np.inf, -1.0), (0.4, 0.0, -1.0)),
                 ((0.4, 0.4, np.nan), (0.4, 0.4, 0.0)), ((0.4, 0.4, np.inf), (0.4, 0.4, 0.0)), ((0.4, 0.4, -np.inf), (0.4, 0.4, 0.0)),
                 ((np.nan, np.nan, np.nan), (0.0, 0.0, 0.0))):
        assert same(*twin_steps(a, b)), (a, b)
    assert not same(*twin_steps((0.4, 0.4, 1.0), (0.4, 0.5, 1.0)))   # the comparison can tell actions apart
    for M, a_ang, dh in ((10, 0.25, 2), (10, 0.35, 4), (10, 0.75, 8), (10, -0.25, -2), (10, -0.75, -8), (10, 0.05, 0), (10, 0.15, 2),
                         (3, 0.5, 2), (3, -0.5, -2), (3, 0.1666, 0), (3, 0.1667, 1)):
        l, got, grip, tie = B.decode((0.0, a_ang, 0.5), M)
        assert got == dh and got == int(np.rint(F(F(a_ang) * F(M)))) and l == F(0.125) and grip == F(0.5), (M, a_ang)
    assert B.decode((0.0, 0.25, 0.0), 10)[3] and B.decode((0.0, 0.5, 0.0), 3)[3] and not B.decode((0.0, 0.3, 0.0), 10)[3]
    for a_lin in (-1.0, -0.8, -0.3, 0.0, 0.123, 1.0, 9.0):
        c = V.clamp(a_lin)
        assert B.decode((a_lin, 0.0, 0.0), 10)[0] == F(F(c + F(1.0)) * F(0.125))
    e = blind(num_obstacles=0)
    e.step((0.0, 0.25, 0.0))
    assert e.last_dh == 2 and e.counters["ties"] == 1
    # the decode is Nav2DVel-v0's own
    for a in ((0.3, -0.45), (7.0, np.nan), (-0.81, 0.449)):
        assert B.decode(a + (0.0,), 10)[:2] == V.decode(a, 10)[2:4]


def test_stop_rule_and_sliding():
    """stop = l < min_abs_lin_speed and |dh| < S: a slow step with a turn of S quanta is no stop, nor is a step of min_abs_lin_speed
    with no turn; on a stop nothing moves.  A move blocked by the wall slides along it when sliding is allowed, and counts one
    collision either way."""
    # M = 10, S = 5: rint(4.4) = 4 and rint(4.5) = 4 (the tie goes to the even 4) are below S, rint(4.6) = 5 is not; the float32 -0.8
    # lies below -0.8, so l(-0.8) is just under the float32 0.025 and l(-0.79) is above it
    assert F(F(F(-0.8) + F(1.0)) * F(0.125)) < F(0.025) < F(F(F(-0.79) + F(1.0)) * F(0.125))
    for a, stop in (((-0.81, 0.44, 0.0), True), ((-0.81, 0.45, 0.0), True), ((-0.81, 0.46, 0.0), False), ((-0.81, -0.46, 0.0), False),
                    ((-0.8, 0.0, 0.0), True), ((-0.79, 0.0, 0.0), False), ((-1.0, 0.0, 0.0), True)):
        e = blind(num_obstacles=0)
        pose = (e.px, e.py, e.h)
        _, _, done, _ = e.step(a)
        assert done == stop and (e.counters["stops"] == 1) == stop, a
        if stop:
            assert e.last["length"] == 1
        else:
            assert (e.px, e.py, e.h) != pose or a[0] == -1.0
    for sliding in (True, False):
        e = blind(num_obstacles=0, allow_sliding=sliding, **ONE_TURN)
        put(e, 7.8, 4.0, 0, 2.0, 2.0)
        e.h = 0                                             # heading 30 degrees after the turn: into the east wall, with a y component
        e.step((1.0, 1.0, 0.0))
        c, s = e.dirs[1]
        assert e.collisions == 1 and e.px == F(7.8) and e.counters["blocked_wall"] == 1
        assert (e.py, e.path) == ((F(F(4.0) + F(F(0.25) * s)), F(abs(F(F(F(4.0) + F(F(0.25) * s)) - F(4.0))))) if sliding else (F(4.0), F(0.0)))
        assert e.counters["slide_y"] == int(sliding) and e.counters["slide_refused"] == 0
    # the unheld object blocks the move and both slides; held, it blocks nothing
    e = blind(num_obstacles=0, **ONE_TURN)
    put(e, 2.0, 2.0, 0, 2.35, 2.25)                        # 0.43 m away; at heading 30 degrees the target (2.217, 2.125) is 0.18 m
    e.step((1.0, 1.0, 0.0))                                # from it, (2.217, 2.0) 0.28 m and (2.0, 2.125) 0.37 m
    assert (e.px, e.py, e.h) == (2.0, 2.0, 1) and e.counters["blocked_object"] == 1 and e.counters["slide_refused"] == 1
    assert e.collisions == 1 and e.path == 0.0
    put(e, 2.0, 2.0, 0, holding=1)
    e.step((1.0, 1.0, 0.0))
    c, s = e.dirs[1]
    assert (e.px, e.py) == (F(F(2.0) + F(F(0.25) * c)), F(F(2.0) + F(F(0.25) * s))) and (e.ox, e.oy) == (e.px, e.py)
    assert e.counters["forward_free_holding"] == 1 and e.path == F(0.25)


def test_sensors_follow_the_new_heading():
    """The three vector sensors after a step are Nav2DRearr-v0's expressions at the new position and the new heading."""
    e = blind(seed=8, num_obstacles=0)
    for a in ((1.0, 1.0, 1.0), (0.2, -0.35, -1.0), (1.0, 0.0, 0.0), (-0.5, 1.0, 1.0)):
        o, _, done, _ = e.step(a)
        assert not done
        c, s = e.dirs[e.h]
        for key, (x, y) in (("obj_start_sensor", (e.o0x, e.o0y)), ("obj_goal_sensor", (e.gx, e.gy))):
            dx, dy = F(x - e.px), F(y - e.py)
            assert o[key].dtype == np.float32 and o[key].tolist() == [F(F(dx * c) + F(dy * s)), F(F(c * dy) - F(s * dx))], key
        assert o["is_holding"].tolist() == [float(e.holding)] and set(o) == {"obj_start_sensor", "obj_goal_sensor", "is_holding"}


@functools.lru_cache(maxsize=None)
def script_counters():
    total, per = {}, {}
    for case in B.SCRIPT_CASES:
        for kind in B.SCRIPTS:
            c = B.script_rollout(kind, case)["counters"]
            per[(kind, case)] = c
            for k, v in c.items():
                total[k] = total.get(k, 0) + v
    return total, per


def test_scripts_reach_every_event():
    """The union of the four scripts over SCRIPT_CASES reaches every event the GPU test relies on: free moves holding and not,
    moves blocked by object, rectangle and wall, both slides and the refused one, both turn signs and |dh| = M, the first and a later
    PICK, PICKs refused far and behind, PLACE accepted and refused by wall and rectangle, each no-op grip combination, a stop with
    success, while holding and too far, and the time-out.  The two image events are reached by one rendered run."""
    total, per = script_counters()
    assert set(B.EVENTS) >= {"forward_free", "forward_free_holding", "blocked_object", "blocked_rect", "blocked_wall", "slide_x",
                             "slide_y", "slide_refused", "turn_left", "turn_right", "turn_max", "pick_bonus", "pick_again", "pick_far",
                             "pick_behind", "place_ok", "place_outside_box", "place_in_rect", "noop_zero", "noop_pick_holding",
                             "noop_place_empty", "successes", "stop_holding", "stop_too_far", "timeouts"}
    for k in B.EVENTS:
        assert total[k] >= 1, (k, total)
    for k in ("clamped", "nonfinite", "ties", "release_and_stop"):
        assert total[k] >= 1, k
    for sh in (False, True):   # the sensor follower solves the task from the sensors alone, in both modes and under both parameter sets
        for p in B.PARAMETER_SETS:
            assert sum(per[("sensor", c)]["successes"] for c in B.SCRIPT_CASES if c[2] == sh and c[1] == p) >= 1
    for sl in (False, True):   # slides happen exactly where they are allowed; every case ends episodes
        slides = sum(per[(k, c)][s] for k in B.SCRIPTS for c in B.SCRIPT_CASES if c[3] == sl for s in ("slide_x", "slide_y", "slide_refused"))
        assert (slides > 0) == sl
    assert all(sum(per[(k, c)]["episodes"] for k in B.SCRIPTS) >= B.SCRIPT_ENVS for c in B.SCRIPT_CASES)
    r = B.script_rollout("random", (8, (10, 30, 10), False, True), H=6, W=10)["counters"]
    assert r["object_visible"] >= 1 and r["marker_visible"] >= 1
    assert len(B.SCRIPT_CASES) == 24 == len(set(B.SCRIPT_CASES)) and B.PARAMETER_SETS == [(1, 10, 5), (10, 30, 10)]
    assert {c[0] for c in B.SCRIPT_CASES} == {0, 3, 8} and {c[1] for c in B.SCRIPT_CASES} == set(B.PARAMETER_SETS)
    assert {c[2] for c in B.SCRIPT_CASES} == {False, True} == {c[3] for c in B.SCRIPT_CASES}
    assert (B.SCRIPT_ENVS, B.SCRIPT_STEPS) == (5, 72)


VALID = dict(device="cpu")


def test_refusals():
    """Every parameter the env refuses, refused with a message that names the task before the device is touched, and by the
    restatement alike."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    bad = [(dict(start_holding=1), "start_holding"), (dict(start_holding="yes"), "start_holding"), (dict(start_holding=None), "start_holding"),
           (dict(distance="geodesic"), "Euclidean"), (dict(distance="manhattan"), "distance"), (dict(num_actions=6), "velocity_control"),
           (dict(num_actions=2), "velocity_control"), (dict(turn_angle=7), "turn_angle"), (dict(turn_angle=0), "turn_angle"),
           (dict(num_obstacles=9), "num_obstacles"), (dict(num_obstacles=-1), "num_obstacles"), (dict(max_episode_steps=0), "max_episode_steps"),
           (dict(max_turn_angle=0), "max_turn_angle"), (dict(max_turn_angle=181), "max_turn_angle"), (dict(max_turn_angle=10.0), "max_turn_angle"),
           (dict(turn_angle=4, max_turn_angle=10), "max_turn_angle"), (dict(min_abs_ang_speed=0), "min_abs_ang_speed"),
           (dict(min_abs_ang_speed=11), "min_abs_ang_speed"), (dict(turn_angle=2, min_abs_ang_speed=5), "min_abs_ang_speed"),
           (dict(min_abs_lin_speed=0.0), "min_abs_lin_speed"), (dict(min_abs_lin_speed=0.26), "min_abs_lin_speed"),
           (dict(min_abs_lin_speed="slow"), "min_abs_lin_speed"), (dict(min_abs_lin_speed=True), "min_abs_lin_speed"),
           (dict(allow_sliding=1), "allow_sliding"), (dict(allow_sliding="no"), "allow_sliding")]
    for kw, text in bad:
        with pytest.raises(_lib.HabError, match=text) as err:
            EF.Nav2DRearrVelVectorEnv(2, 8, 8, device="cpu", **kw)
        assert "Nav2DVel:" not in str(err.value), kw
    for size in ((0, 8), (8, 0)):
        with pytest.raises(_lib.HabError, match="image size"):
            EF.Nav2DRearrVelVectorEnv(2, *size, device="cpu")
    with pytest.raises(_lib.HabError, match="GPU"):   # valid parameters: only the missing device is refused
        EF.Nav2DRearrVelVectorEnv(2, 8, 8, device="cpu", start_holding=True, num_obstacles=8, turn_angle=10, max_turn_angle=30,
                                  min_abs_ang_speed=10, allow_sliding=False, min_abs_lin_speed=0.25)
    with pytest.raises(_lib.HabError, match="GPU"):   # no image at all needs no size
        EF.Nav2DRearrVelVectorEnv(2, 0, 0, device="cpu", use_depth=False)
    for kw in (dict(start_holding=1), dict(turn_angle=7), dict(num_obstacles=9), dict(max_turn_angle=181), dict(min_abs_ang_speed=11),
               dict(min_abs_lin_speed=0.0), dict(allow_sliding=1)):
        with pytest.raises(ValueError):
            B.Nav2DRearrVelEnv(1, 0, **kw)
    e = blind()
    for a in ((0.0, 0.0), (0.0, 0.0, 0.0, 0.0), 1, [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError):
            e.step(a)
    # the host path takes a length-3 array or {"action": array}; the goal-sensor forms and pausing are refused
    env = EF.Nav2DRearrVelVectorEnv.__new__(EF.Nav2DRearrVelVectorEnv)
    env.num_envs, env._pending, env._actions_host = 3, set(), np.zeros((3, 3), np.float32)
    env.async_step_at(0, np.array([0.5, -2.0, 1.0], np.float32))
    env.async_step_at(2, {"action": [0.25, 0.0, -1.0]})
    assert env._pending == {0, 2} and env._actions_host.tolist() == [[0.5, -2.0, 1.0], [0.0, 0.0, 0.0], [0.25, 0.0, -1.0]]
    for a in (1, [0.0, 0.0], [0.0] * 4, [[0.0, 0.0, 0.0]], "abc", None):
        with pytest.raises(_lib.HabError, match="length-3"):
            env.async_step_at(1, a)
    with pytest.raises(_lib.HabError, match="twice"):
        env.async_step_at(0, [0.0, 0.0, 0.0])
    for call in (lambda: env.reset_into(None, None, None), lambda: env.step_into(None, None, None, None, None),
                 lambda: env.step_into_obs({}, None, None), lambda: env.pause_at(0)):
        with pytest.raises(_lib.HabError, match="Nav2D"):
            call()


def test_factory_choice_and_yaml(monkeypatch):
    """The YAML loads with every key the task reads; a habitat.task.type starting with "nav2drearrvel" (any case) picks the new env
    while Nav2DRearr-v0 and the other Nav2D tasks keep theirs; the Nav2DVel keys and start_holding reach the class; the image size
    comes from head_rgb, else head_depth, else nothing is rendered.  The constructors are replaced by recorders: the envs themselves
    need a GPU."""
    from habitat_amd.common import env_factory as EF
    from habitat_amd.config.default import get_config
    from habitat_amd.rl.ppo.ppo_trainer import PPOTrainer
    assert "Nav2DRearrVel-v0" in PPOTrainer.supported_tasks
    name = "rearrange/ddppo_nav2d_rearrange_vel.yaml"
    cfg = get_config(name)
    hab, hb = cfg.habitat, cfg.habitat_baselines
    assert hab.task.type == "Nav2DRearrVel-v0" and list(hab.task.actions) == ["velocity_control"]
    assert hab.simulator.sensors.head_depth.height == hab.simulator.sensors.head_depth.width == 128 and "head_rgb" not in hab.simulator.sensors
    assert list(hab.task.lab_sensors) == ["obj_start_sensor", "obj_goal_sensor", "is_holding"]
    agent = hb.rl.policy.main_agent
    assert agent.name == "PointNavResNetPolicy" and agent.action_distribution_type == "gaussian" and hb.rl.ddppo.backbone == "resnet18"
    # the action_dist block of ppo_nav2d_vel.yaml, the rest of ddppo_nav2d_rearrange.yaml
    vel, rearr = get_config("pointnav/ppo_nav2d_vel.yaml"), get_config("rearrange/ddppo_nav2d_rearrange.yaml")
    assert dict(agent.action_dist) == dict(vel.habitat_baselines.rl.policy.main_agent.action_dist)
    assert dict(hb.rl.ppo) == dict(rearr.habitat_baselines.rl.ppo) and dict(hb.rl.ddppo) == dict(rearr.habitat_baselines.rl.ddppo)
    assert getattr(agent, "fuse_keys", None) == getattr(rearr.habitat_baselines.rl.policy.main_agent, "fuse_keys", None)
    syn = {k: hab.synthetic[k] for k in ("turn_angle", "max_turn_angle", "min_abs_lin_speed", "min_abs_ang_speed", "allow_sliding")}
    assert syn == {k: vel.habitat.synthetic[k] for k in syn} and hab.synthetic.start_holding is False
    assert hab.synthetic.num_obstacles == 3 and hab.synthetic.distance_to_goal == "euclidean" and hab.environment.max_episode_steps == 200
    made = []
    for cls in ("Nav2DRearrVelVectorEnv", "Nav2DRearrVectorEnv", "Nav2DObjVectorEnv", "Nav2DVelVectorEnv", "Nav2DVectorEnv", "SyntheticVectorEnv"):
        monkeypatch.setattr(EF, cls, lambda *a, _n=cls, **kw: made.append((_n, a, kw)) or _n)
    factory = EF.SyntheticVectorEnvFactory()
    assert factory.construct_envs(cfg, device="cpu") == "Nav2DRearrVelVectorEnv"
    _, args, kw = made[-1]
    assert args == (16, 128, 128) and kw["num_actions"] == 1 and kw["max_episode_steps"] == 200
    assert {k: kw[k] for k in ("num_obstacles", "turn_angle", "max_turn_angle", "min_abs_lin_speed", "min_abs_ang_speed", "allow_sliding",
                               "start_holding", "use_rgb", "use_depth", "distance")} == dict(
        num_obstacles=3, turn_angle=1, max_turn_angle=10, min_abs_lin_speed=0.025, min_abs_ang_speed=5, allow_sliding=True,
        start_holding=False, use_rgb=False, use_depth=True, distance="euclidean")
    for task_type, want in (("nav2drearrvel", "Nav2DRearrVelVectorEnv"), ("NAV2DREARRVEL-v3", "Nav2DRearrVelVectorEnv"),
                            ("Nav2DRearr-v0", "Nav2DRearrVectorEnv"), ("nav2drearr", "Nav2DRearrVectorEnv"),
                            ("Nav2DRearrVe-v0", "Nav2DRearrVectorEnv"), ("Nav2DVel-v0", "Nav2DVelVectorEnv"),
                            ("Nav2DObj-v0", "Nav2DObjVectorEnv"), ("Nav2D-v0", "Nav2DVectorEnv")):
        ov = [f"habitat.task.type={task_type}"] + (["habitat.simulator.sensors.semantic.height=8", "habitat.simulator.sensors.semantic.width=8"]
                                                   if "Obj" in task_type else [])
        assert factory.construct_envs(get_config(name, ov), device="cpu") == want, task_type
        if want == "Nav2DRearrVectorEnv":   # the discrete task is given none of the velocity keys
            assert "max_turn_angle" not in made[-1][2] and "allow_sliding" not in made[-1][2]
    # the discrete task's own YAML still yields the discrete class
    assert factory.construct_envs(rearr, device="cpu") == "Nav2DRearrVectorEnv" and made[-1][2]["num_actions"] == 6
    # without the keys the defaults are Nav2DVel-v0's, turn_angle 1 among them
    bare = get_config(name)
    for k in ("turn_angle", "max_turn_angle", "min_abs_lin_speed", "min_abs_ang_speed", "allow_sliding", "start_holding"):
        del bare.habitat.synthetic[k]
    assert factory.construct_envs(bare, device="cpu") == "Nav2DRearrVelVectorEnv"
    assert {k: made[-1][2][k] for k in ("turn_angle", "max_turn_angle", "min_abs_lin_speed", "min_abs_ang_speed", "allow_sliding",
                                        "start_holding")} == dict(turn_angle=1, max_turn_angle=10, min_abs_lin_speed=0.025,
                                                                  min_abs_ang_speed=5, allow_sliding=True, start_holding=False)
    sizes = ["habitat.simulator.sensors.head_rgb.height=40", "habitat.simulator.sensors.head_rgb.width=44",
             "habitat.simulator.sensors.head_depth.height=48", "habitat.simulator.sensors.head_depth.width=52",
             "habitat.synthetic.start_holding=True", "habitat.synthetic.distance_to_goal=geodesic", "habitat.synthetic.allow_sliding=False",
             "habitat.synthetic.turn_angle=10", "habitat.synthetic.max_turn_angle=30", "habitat.synthetic.min_abs_ang_speed=10"]
    c = get_config(name, sizes)
    for flags, want, use in ((dict(), (40, 44), (True, True)), (dict(use_rgb=False), (48, 52), (False, True)),
                             (dict(use_rgb=False, use_depth=False), (0, 0), (False, False))):
        assert EF.SyntheticVectorEnvFactory(**flags).construct_envs(c, device="cpu") == "Nav2DRearrVelVectorEnv"
        _, args, kw = made[-1]
        assert args[1:] == want and (kw["use_rgb"], kw["use_depth"]) == use and kw["start_holding"] is True and kw["distance"] == "geodesic"
        assert (kw["allow_sliding"], kw["turn_angle"], kw["max_turn_angle"], kw["min_abs_ang_speed"]) == (False, 10, 30, 10)


def test_the_yaml_gives_a_box_of_three(monkeypatch):
    """The factory on the YAML with the device side of the constructor stubbed out (no GPU here): a Nav2DRearrVelVectorEnv whose
    action space is Box(-1, 1, (3,), float32), which the policy side reads as continuous with three dimensions, with a float32 (N, 3)
    host action table and the entry's task parameters in the entry's order."""
    from habitat_amd.common import env_factory as EF, spaces
    from habitat_amd.config.default import get_config

    def fake_init(self, num_envs, height, width, **kw):
        self.num_envs, self.received = num_envs, dict(kw, height=height, width=width)
        self.action_spaces = [EF.spaces.Discrete(4)] * num_envs
    monkeypatch.setattr(EF.Nav2DVectorEnv, "__init__", fake_init)
    cfg = get_config("rearrange/ddppo_nav2d_rearrange_vel.yaml", ["habitat.synthetic.start_holding=True", "habitat.synthetic.turn_angle=5",
                                                                  "habitat.synthetic.max_turn_angle=30", "habitat.synthetic.min_abs_ang_speed=10"])
    env = EF.SyntheticVectorEnvFactory().construct_envs(cfg, device="cpu")
    assert type(env) is EF.Nav2DRearrVelVectorEnv and isinstance(env, EF.Nav2DRearrVectorEnv) and env.consumes_actions
    assert len(env.action_spaces) == 16 and env.orig_action_spaces is env.action_spaces
    for sp in env.action_spaces:
        assert isinstance(sp, EF.spaces.Box) and sp.shape == (3,) and sp.dtype == np.float32
        assert sp.low.tolist() == [-1.0] * 3 and sp.high.tolist() == [1.0] * 3
        assert spaces.is_continuous_action_space(sp) and spaces.get_action_space_info(sp) == ((3,), False)
    assert env._actions_host.shape == (16, 3) and env._actions_host.dtype == np.float32
    assert env.received["turn_angle"] == 5 and (env.received["height"], env.received["width"]) == (128, 128) and "num_actions" not in env.received
    assert env._task_parameters() == (1, 6, 2, 0.025, 1) and env.task == "nav2drearrvel"
    assert env._entries == ("hab_nav2d_rearr_vel_step",) and env._action_dtype is __import__("torch").float32
    assert env._state_bytes == "hab_nav2d_rearr_state_bytes" and env.measure_names == A.MEASURES and env.num_actions == 1
    import torch
    assert env._actions_shaped(torch.zeros(16, 3)) and not env._actions_shaped(torch.zeros(16, 2)) and not env._actions_shaped(torch.zeros(48))
    # the discrete class is as it was
    assert EF.Nav2DRearrVectorEnv._entries == ("hab_nav2d_rearr_step",) and EF.Nav2DRearrVectorEnv.num_actions == 6
    assert EF.Nav2DRearrVectorEnv._action_dtype is torch.int64


def test_observation_space_and_policy_tables():
    """The observation space in its order, built before the constructor asks for the device, which is what is missing here;
    resolve_sensors on it gives the visual table [head_rgb?, head_depth] and the fused widths (2, 2, 1): D = 5, as Nav2DRearr-v0."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    from habitat_amd.rl.ppo.policy import resolve_sensors
    for use_rgb in (False, True):
        env = EF.Nav2DRearrVelVectorEnv.__new__(EF.Nav2DRearrVelVectorEnv)
        with pytest.raises(_lib.HabError, match="GPU"):
            env.__init__(3, 10, 12, device="cpu", use_rgb=use_rgb, turn_angle=5)
        sp = env.observation_spaces[0]
        want = (["head_rgb"] if use_rgb else []) + ["head_depth", "obj_start_sensor", "obj_goal_sensor", "is_holding"]
        assert list(sp.spaces) == want and (env.H, env.W) == (10, 12)
        assert sp["head_depth"].shape == (10, 12, 1) and sp["head_depth"].dtype == np.float32
        assert sp["obj_start_sensor"].shape == sp["obj_goal_sensor"].shape == (2,) and sp["is_holding"].shape == (1,)
        assert all(sp[k].dtype == np.float32 for k in want[-3:]) and sp["is_holding"].low.min() == 0.0 and sp["is_holding"].high.max() == 1.0
        if use_rgb:
            assert sp["head_rgb"].shape == (10, 12, 3) and sp["head_rgb"].dtype == np.uint8
        visual, fused = resolve_sensors(sp)
        assert [v[0] for v in visual] == want[:-3] and [v[2] for v in visual] == ([3, 1] if use_rgb else [1])
        assert fused == [("obj_start_sensor", 2), ("obj_goal_sensor", 2), ("is_holding", 1)] and sum(f[1] for f in fused) == 5
    env = EF.Nav2DRearrVelVectorEnv.__new__(EF.Nav2DRearrVelVectorEnv)
    with pytest.raises(_lib.HabError, match="GPU"):
        env.__init__(3, 10, 12, device="cpu", use_rgb=False, use_depth=False)
    assert list(env.observation_spaces[0].spaces) == ["obj_start_sensor", "obj_goal_sensor", "is_holding"] and (env.H, env.W) == (0, 0)
    assert EF.NAV2D_REARR_SENSORS == B.SENSORS == A.SENSORS


def test_header_and_signature_table_agree():
    """The header's prototype of hab_nav2d_rearr_vel_step and the ctypes table: the same number of arguments, pointers where the
    header has pointers, the two uint32, the float and the ints in their places; the arguments are hab_nav2d_rearr_step's with the
    four of hab_nav2d_vel_step after start_holding; the record is Nav2DRearr-v0's."""
    from habitat_amd import _lib
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "habitat_amd.h")).read()

    def names_of(entry):
        m = re.search(r"int %s\((.*?)\);" % entry, text, re.S)
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
        return params, [p.split()[-1].lstrip("*") for p in params]

    params, names = names_of("hab_nav2d_rearr_vel_step")
    restype, argtypes = _lib.SIGNATURES["hab_nav2d_rearr_vel_step"]
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
    _, rearr = names_of("hab_nav2d_rearr_step")
    _, vel = names_of("hab_nav2d_vel_step")
    i = rearr.index("start_holding") + 1
    four = ["max_turn_steps", "stop_turn_steps", "min_abs_lin_speed", "allow_sliding"]
    assert names == rearr[:i] + four + rearr[i:] and vel[vel.index("max_episode_steps") + 1:][:4] == four
    assert params[names.index("actions")].startswith("const float*") and params[names.index("min_abs_lin_speed")].startswith("float ")
    assert hasattr(_lib, "SIGNATURES") and "hab_nav2d_rearr_vel_state_bytes" not in _lib.SIGNATURES   # the record is Nav2DRearr-v0's
