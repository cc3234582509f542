"""CPU: the Nav2DRearr-v0 restatement (tests/nav2d_rearr_reference.py) holds its own invariants, the scripted sequences the GPU tests
replay reach every branch of the task, and the Python surface (parameters, factory, YAML, observation space, signature table) behaves
without a device."""
import functools
import os
import re

import numpy as np
import pytest

import nav2d_obj_reference as O
import nav2d_reference as R
import nav2d_rearr_reference as A

F = np.float32


def blind(seed=3, env=0, **kw):
    e = A.Nav2DRearrEnv(seed, env, **dict(dict(num_obstacles=3, max_episode_steps=40), **kw))
    e.reset()
    return e


def put(e, px, py, h, ox=None, oy=None, holding=0):
    """Moves the agent (and the unheld object) of a K = 0 env to a chosen pose; the potential is brought up to date."""
    e.px, e.py, e.h, e.holding = F(px), F(py), h, holding
    e.ox, e.oy = (e.px, e.py) if holding else (F(ox), F(oy))
    e.held = max(e.held, holding)
    e.phi_prev = e.potential()[0]
    return e


@pytest.mark.parametrize("K", [0, 3, 8])
def test_placement_is_nav2dobj_objects_0_and_1(K):
    """o0 and g are objects 0 and 1 of Nav2DObj-v0's world with M = 2, whatever its categories: positions, start and rectangles."""
    for env in range(10):
        for episode in range(3):
            w, objects, _, _, fb = O.make_world(9, env, episode, K, 36, 2, 4)
            e = A.Nav2DRearrEnv(9, env, num_obstacles=K)
            e.episode = episode
            e._begin()
            assert (e.o0x, e.o0y) == objects[0] and (e.gx, e.gy) == objects[1] and (e.ox, e.oy) == objects[0]
            assert (e.px, e.py, e.h) == (w.sx, w.sy, w.h) and e.world.rects == w.rects
            assert R.dist(e.o0x, e.o0y, e.gx, e.gy) >= 1.0 and R.dist(e.px, e.py, e.gx, e.gy) >= 1.0


@pytest.mark.parametrize("K,start_holding", [(0, False), (3, True), (8, False), (8, True)])
def test_world_invariants(K, start_holding):
    """600 steps each of the PICK / PLACE-everywhere script, the random one and the sensor follower (about twenty episodes in all):
    the agent is always free, never within 0.4 m of an unheld object, a placed object is inside its box and outside the grown
    rectangles, h is 0 or 1 and a held object is at p."""
    rng = np.random.RandomState(K)
    counters = {}
    for kind in ("pickplace", "random", "sensor"):
        e = blind(seed=7, num_obstacles=K, start_holding=start_holding, turn_angle=30, max_episode_steps=100)
        sc, obs = A.make_script(kind, 30, rng), e.observe()
        for _ in range(600):
            obs, _, done, _ = e.step(sc(obs, e))
            if done:
                sc.episode_ended()
            assert e.holding in (0, 1) and e.held in (0, 1) and e.held >= e.holding
            assert R.is_free(e.px, e.py, e.world.rects)
            if e.holding:
                assert (e.ox, e.oy) == (e.px, e.py) and obs["is_holding"][0] == 1.0
            else:
                assert not R.dist(e.px, e.py, e.ox, e.oy) < O.OBJ_BLOCK and obs["is_holding"][0] == 0.0
                assert 0.5 <= e.ox <= 7.5 and 0.5 <= e.oy <= 7.5 and not A.in_grown_rect(e.ox, e.oy, e.world.rects)
        counters = {k: counters.get(k, 0) + v for k, v in e.counters.items()}
    assert counters["place_ok"] > 0 and counters["pick_ok"] > 0 and counters["episodes"] >= 15


def test_rewards_telescope():
    """Per episode, in float64: sum r = -0.01 * len + Phi_0 - Phi_T + 1.0 * [a first PICK happened] + 2.5 * success.  The bound is
    derived as Nav2D-v0's test derives its own: each Phi is the same float32 in both of its terms, so the potentials cancel exactly and
    what is left are the roundings of each step's reward.  Phi < 32 and one step changes it by less than 2 (a PICK moves the object by
    less than 1 m, a PLACE by 0.5 m, a forward step by 0.25 m), so Phi_prev - Phi rounds by at most 2^-24, -0.01 + that (below 4) by
    at most 2^-23 and -0.01 itself is off by less than 2^-31 as a float32; adding the bonuses is exact where they are 0 and rounds by
    at most 2^-23 (the pick, a sum below 4) and 2^-22 (the success, a sum below 8) on the one step each that carries them."""
    rng = np.random.RandomState(1)
    seen = set()
    for kind, sh, K in (("sensor", True, 0), ("sensor", False, 3), ("pickplace", True, 3), ("random", False, 8)):
        e = blind(seed=11, env=1, num_obstacles=K, start_holding=sh, turn_angle=30, max_episode_steps=80)
        sc, obs = A.make_script(kind, 30, rng), e.observe()
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
            bound = n * (2.0 ** -24 + 2.0 ** -23 + 2.0 ** -31) + 2.0 ** -23 + 2.0 ** -22
            assert L["length"] == n and abs(total - closed) <= bound, (kind, total, closed, bound)
            seen.add((bonus, info["success"]))
    assert {(True, 1.0), (False, 1.0), (False, 0.0), (True, 0.0)} <= seen


def test_pick_rules():
    """Reach at the boundary, behind the agent, while holding; a refused PICK changes nothing but `invalid`."""
    e = blind(num_obstacles=0, turn_angle=30)
    below = float(np.nextafter(F(3.0), F(0.0)))
    put(e, 2.0, 2.0, 0, below, 2.0)                        # d = 1 - 2^-22, the nearest this pose comes to 1 from below: in reach
    assert F(1.0) - R.dist(e.px, e.py, e.ox, e.oy) == F(2.0 ** -22)
    _, r, _, _ = e.step(A.PICK)
    assert e.holding == 1 and e.picks == 1 and e.invalid == 0 and (e.ox, e.oy) == (e.px, e.py)
    assert r == F(F(F(R.SLACK + F(e_phi_before(e, 2.0, 2.0, below, 2.0) - e.phi_prev)) + F(1.0)) + F(0.0))
    _, _, _, _ = e.step(A.PICK)                            # while holding
    assert e.invalid == 1 and e.holding == 1 and e.picks == 1
    put(e, 2.0, 2.0, 0, 3.0, 2.0)                          # d = 1.0 exactly: out of reach
    before = e.state_words()
    e.step(A.PICK)
    after = e.state_words()
    assert e.holding == 0 and e.invalid == 2 and after["flags"].tolist() == [0, 1, 1, 2]
    assert np.array_equal(before["pos"], after["pos"]) and np.array_equal(before["places"], after["places"])
    put(e, 2.0, 2.0, 0, 1.5, 2.0)                          # behind: dot < 0
    e.step(A.PICK)
    assert e.holding == 0 and e.invalid == 3
    put(e, 2.0, 2.0, 3, 2.5, 2.0)                          # heading 90 degrees: the object is exactly abeam, dot = cos(90) * 0.5 > 0 or not
    c, s = e.dirs[3]
    ahead = F(F(F(0.5) * c) + F(F(0.0) * s)) > 0
    e.step(A.PICK)
    assert e.holding == int(ahead)
    e2 = blind(num_obstacles=0, turn_angle=30)
    put(e2, 2.0, 2.0, 0, 2.5, 2.0)
    _, r1, _, _ = e2.step(A.PICK)
    e2.step(A.PLACE)
    _, r2, _, _ = e2.step(A.PICK)                          # the second PICK of the episode carries no bonus
    # the PLACE put the object back where it was, so both PICKs change the potential alike and differ by the bonus alone
    assert e2.picks == 2 and r1 == F(r2 + F(1.0)) and r2 < 0.5 and e2.counters["pick_again"] == 1 and e2.counters["pick_bonus"] == 1


def e_phi_before(e, px, py, ox, oy):
    return F(R.dist(F(px), F(py), F(ox), F(oy)) + R.dist(F(ox), F(oy), e.gx, e.gy))


def test_place_rules():
    """Inside a rectangle, outside the box, while not holding; a successful PLACE puts o at p + 0.5 * dir."""
    e = blind(num_obstacles=0, turn_angle=30)
    put(e, 2.0, 2.0, 0, 5.0, 5.0)
    e.step(A.PLACE)                                        # not holding
    assert e.invalid == 1 and (e.ox, e.oy) == (5.0, 5.0)
    put(e, 7.25, 2.0, 0, holding=1)                        # q.x = 7.75 > 7.5
    e.step(A.PLACE)
    assert e.holding == 1 and e.invalid == 2 and e.counters["place_outside_box"] == 1
    put(e, 7.0, 2.0, 0, holding=1)                         # q.x = 7.5: on the box's edge, inside
    e.step(A.PLACE)
    assert e.holding == 0 and (e.ox, e.oy) == (7.5, 2.0) and e.invalid == 2
    e = blind(num_obstacles=0, turn_angle=30)
    e.world.rects = [(F(3.0), F(3.0), F(4.0), F(4.0))]
    put(e, 2.25, 3.5, 0, holding=1)                        # q = (2.75, 3.5): strictly inside the rectangle grown by 0.3
    e.step(A.PLACE)
    assert e.holding == 1 and e.counters["place_in_rect"] == 1 and e.invalid == 1
    put(e, 2.2, 3.5, 0, holding=1)                         # q.x = fl(2.2 + 0.5) <= fl(3 - 0.3): not strictly inside
    q = F(F(2.2) + F(0.5))
    inside = q > F(F(3.0) - O.OBJ_R)
    e.step(A.PLACE)
    assert e.holding == int(inside)
    c, s = e.dirs[1]
    put(e, 5.0, 5.0, 1, holding=1)
    e.step(A.PLACE)
    assert (e.ox, e.oy) == (F(F(5.0) + F(F(0.5) * c)), F(F(5.0) + F(F(0.5) * s))) and e.holding == 0
    assert not R.dist(e.px, e.py, e.ox, e.oy) < O.OBJ_BLOCK


@pytest.mark.parametrize("start_holding", [False, True])
def test_start_holding_and_did_pick_object(start_holding):
    """Under start_holding every episode begins with h = 1, o = p, Phi_0 = d(p, g) and did_pick_object = 1 whatever happens; without
    it the measure is 1 exactly in the episodes with a successful PICK."""
    e = blind(seed=5, num_obstacles=3, start_holding=start_holding, turn_angle=30, max_episode_steps=30)
    rng = np.random.RandomState(2)
    sc, obs, infos = A.make_script("sensor", 30, rng), e.observe(), []
    for _ in range(12):
        assert e.holding == int(start_holding) == e.held and e.picks == 0
        assert (e.ox, e.oy) == ((e.px, e.py) if start_holding else (e.o0x, e.o0y))
        assert e.phi_start == (R.dist(e.px, e.py, e.gx, e.gy) if start_holding else
                               F(R.dist(e.px, e.py, e.o0x, e.o0y) + R.dist(e.o0x, e.o0y, e.gx, e.gy)))
        while True:
            obs, _, done, info = e.step(sc(obs, e))
            if done:
                sc.episode_ended()
                infos.append(dict(info, picks=e.last["picks"]))
                break
    if start_holding:
        assert all(i["did_pick_object"] == 1.0 for i in infos)
    else:
        assert all(i["did_pick_object"] == float(i["picks"] > 0) for i in infos) and {i["did_pick_object"] for i in infos} == {0.0, 1.0}
    e = blind(seed=5, num_obstacles=0, start_holding=start_holding, max_episode_steps=3)
    for _ in range(3):
        _, _, done, info = e.step(A.TURN_LEFT)
    assert done and info["did_pick_object"] == float(start_holding) and info["success"] == 0.0


def test_sensors_at_reset_and_after_each_action():
    """obj_start_sensor and obj_goal_sensor are (dot, cross) of o0 - p and g - p in the current heading's frame, term by term;
    is_holding is h.  After each action type; a PLACE elsewhere leaves obj_start_sensor at the START position."""
    e = blind(seed=8, num_obstacles=0, turn_angle=30)
    put(e, 3.0, 3.0, 0, 3.5, 3.0)

    def check(o):
        c, s = e.dirs[e.h]
        for key, (x, y) in (("obj_start_sensor", (e.o0x, e.o0y)), ("obj_goal_sensor", (e.gx, e.gy))):
            dx, dy = F(x - e.px), F(y - e.py)
            assert o[key].dtype == np.float32 and o[key].tolist() == [F(F(dx * c) + F(dy * s)), F(F(c * dy) - F(s * dx))], key
        assert o["is_holding"].tolist() == [float(e.holding)] and o["is_holding"].dtype == np.float32
        assert set(o) == {"obj_start_sensor", "obj_goal_sensor", "is_holding"}

    check(e.observe())
    start0 = (e.o0x, e.o0y)
    for a in (A.TURN_LEFT, A.PICK, A.MOVE_FORWARD, A.TURN_RIGHT, A.TURN_RIGHT, A.MOVE_FORWARD, A.PLACE, A.MOVE_FORWARD, A.PICK, A.PLACE):
        o, _, done, _ = e.step(a)
        assert not done
        check(o)
    assert e.counters["place_ok"] == 2 and (e.o0x, e.o0y) == start0 and (e.ox, e.oy) != start0
    # a rotation by one turn rotates both vectors and keeps their lengths (to rounding)
    a0 = e.observe()["obj_goal_sensor"].astype(np.float64)
    a1 = e.step(A.TURN_LEFT)[0]["obj_goal_sensor"].astype(np.float64)
    assert abs(np.hypot(*a0) - np.hypot(*a1)) < 1e-5
    o = e.step(A.STOP)[0]                                   # the next episode's first observation
    assert e.steps == 0 and e.episode == 1
    check(o)


def test_render_object_and_marker():
    """The unheld object is geometry in head_depth and head_rgb; held, it is in neither.  The goal marker changes head_rgb alone."""
    H, W = 12, 20
    e = A.Nav2DRearrEnv(2, 0, H=H, W=W, num_obstacles=0, turn_angle=30)
    e.reset()
    put(e, 2.0, 4.0, 0, 3.0, 4.0)                          # the object one metre straight ahead
    e.gx, e.gy = F(6.0), F(4.0)                             # the goal behind it: hidden by the cylinder
    o = e.observe()
    mid = o["head_depth"][H // 2, W // 2, 0]
    assert abs(float(mid) * 10.0 - 0.7) < 0.05 and e.counters["object_visible"] == 1 and e.counters["marker_visible"] == 0
    assert tuple(o["head_rgb"][H // 2, W // 2]) == tuple(R._shade(np.array(O.category_color(0), np.uint8), F(mid)))
    e.holding, e.ox, e.oy = 1, e.px, e.py
    held = e.observe()
    assert e.counters["object_visible"] == 1 and e.counters["marker_visible"] == 1
    assert float(held["head_depth"][H // 2, W // 2, 0]) * 10.0 > 5.9           # the far wall
    red = held["head_rgb"][H // 2, W // 2]
    assert red[0] > 2 * red[1] and red[0] > 2 * red[2]
    e.gx, e.gy = F(2.0), F(7.0)                             # the goal out of view: depth unchanged, rgb without red
    away = e.observe()
    assert np.array_equal(away["head_depth"], held["head_depth"]) and not np.array_equal(away["head_rgb"], held["head_rgb"])
    assert held["head_depth"].shape == (H, W, 1) and held["head_rgb"].shape == (H, W, 3)
    e = A.Nav2DRearrEnv(2, 0, H=0, W=0)
    assert set(e.reset()) == {"obj_start_sensor", "obj_goal_sensor", "is_holding"}


@functools.lru_cache(maxsize=None)
def script_counters():
    total = {}
    per = {}
    for case in A.SCRIPT_CASES:
        for kind in A.SCRIPTS:
            c = A.script_rollout(kind, case)["counters"]
            per[(kind, case)] = c
            for k, v in c.items():
                total[k] = total.get(k, 0) + v
    return total, per


def test_scripts_reach_every_event():
    """The union of the four scripts over SCRIPT_CASES reaches every branch listed under Actions and Reward: success, both failed
    STOPs, the step limit, the three kinds of refused move (the unheld object among them), every PICK and PLACE outcome, the pick
    bonus and a later PICK without it.  The two image events are reached by one rendered run."""
    total, per = script_counters()
    for k in A.EVENTS:
        if k not in ("object_visible", "marker_visible"):
            assert total[k] >= 1, (k, total)
    assert total["episodes"] > 0 and total["timeouts"] > 0
    for sh in (False, True):   # the sensor follower solves the task from the sensors alone, in both modes
        assert sum(per[("sensor", c)]["successes"] for c in A.SCRIPT_CASES if c[2] == sh) >= 1
    assert sum(per[("wall", c)]["place_outside_box"] + per[("wall", c)]["place_in_rect"] for c in A.SCRIPT_CASES) >= 1
    r = A.script_rollout("random", (8, 10, False), H=6, W=10)["counters"]
    assert r["object_visible"] >= 1 and r["marker_visible"] >= 1
    assert all(len(case) == 3 for case in A.SCRIPT_CASES) and len(A.SCRIPT_CASES) == 12
    assert {c[0] for c in A.SCRIPT_CASES} == {0, 3, 8} and {c[1] for c in A.SCRIPT_CASES} == {10, 30} and {c[2] for c in A.SCRIPT_CASES} == {False, True}


def test_refusals():
    """Every parameter the env refuses, refused with a message before the device is touched, and by the restatement alike."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    bad = [(dict(start_holding=1), "start_holding"), (dict(start_holding="yes"), "start_holding"), (dict(start_holding=None), "start_holding"),
           (dict(distance="geodesic"), "Euclidean"), (dict(distance="manhattan"), "distance"), (dict(num_actions=4), "Discrete"),
           (dict(num_actions=7), "Discrete"), (dict(turn_angle=7), "turn_angle"), (dict(num_obstacles=9), "num_obstacles"),
           (dict(num_obstacles=-1), "num_obstacles"), (dict(max_episode_steps=0), "max_episode_steps")]
    for kw, text in bad:
        with pytest.raises(_lib.HabError, match=text):
            EF.Nav2DRearrVectorEnv(2, 8, 8, device="cpu", **kw)
    for size in ((0, 8), (8, 0)):
        with pytest.raises(_lib.HabError, match="image size"):
            EF.Nav2DRearrVectorEnv(2, *size, device="cpu")
    with pytest.raises(_lib.HabError, match="GPU"):   # valid parameters: only the missing device is refused
        EF.Nav2DRearrVectorEnv(2, 8, 8, device="cpu", start_holding=True, num_obstacles=8, turn_angle=30)
    with pytest.raises(_lib.HabError, match="GPU"):   # no image at all needs no size
        EF.Nav2DRearrVectorEnv(2, 0, 0, device="cpu", use_depth=False)
    for kw in (dict(start_holding=1), dict(turn_angle=7), dict(num_obstacles=9)):
        with pytest.raises(ValueError):
            A.Nav2DRearrEnv(1, 0, **kw)
    e = blind()
    for a in (-1, 6):
        with pytest.raises(ValueError):
            e.step(a)
    # the host path checks actions against 0..5; the goal-sensor forms and pausing are refused
    env = EF.Nav2DRearrVectorEnv.__new__(EF.Nav2DRearrVectorEnv)
    env.num_envs, env._pending, env._actions_host = 3, set(), np.zeros(3, np.int64)
    env.async_step_at(0, 5)
    env.async_step_at(2, {"action": np.array([4])})
    assert env._pending == {0, 2} and env._actions_host.tolist() == [5, 0, 4]
    for a in (6, -1, 0.5, [1, 2]):
        with pytest.raises(_lib.HabError):
            env.async_step_at(1, a)
    for call in (lambda: env.reset_into(None, None, None), lambda: env.step_into(None, None, None, None, None),
                 lambda: env.step_into_obs({}, None, None), lambda: env.pause_at(0)):
        with pytest.raises(_lib.HabError):
            call()


def test_factory_choice_yaml_and_image_size(monkeypatch):
    """The YAML loads with every key the task reads; habitat.task.type picks the env (any case) while the other Nav2D tasks keep
    theirs; the image size comes from head_rgb, else head_depth, else nothing is rendered; start_holding and the refused geodesic
    mode reach the class.  The constructors are replaced by recorders: the envs themselves need a GPU."""
    from habitat_amd.common import env_factory as EF
    from habitat_amd.config.default import get_config
    from habitat_amd.rl.ppo.ppo_trainer import PPOTrainer
    assert "Nav2DRearr-v0" in PPOTrainer.supported_tasks
    name = "rearrange/ddppo_nav2d_rearrange.yaml"
    cfg = get_config(name)
    hab, hb = cfg.habitat, cfg.habitat_baselines
    assert hab.task.type == "Nav2DRearr-v0" and list(hab.task.actions) == ["stop", "move_forward", "turn_left", "turn_right", "pick", "place"]
    assert hab.simulator.sensors.head_depth.height == hab.simulator.sensors.head_depth.width == 128 and "head_rgb" not in hab.simulator.sensors
    assert hab.synthetic.start_holding is False and hab.synthetic.distance_to_goal == "euclidean" and hab.environment.max_episode_steps == 200
    assert hb.rl.ddppo.backbone == "resnet18" and hb.rl.policy.main_agent.name == "PointNavResNetPolicy" and hb.trainer_name == "ddppo"
    made = []
    for cls in ("Nav2DRearrVectorEnv", "Nav2DObjVectorEnv", "Nav2DVelVectorEnv", "Nav2DVectorEnv", "SyntheticVectorEnv"):
        monkeypatch.setattr(EF, cls, lambda *a, _n=cls, **kw: made.append((_n, a, kw)) or _n)
    factory = EF.SyntheticVectorEnvFactory()
    assert factory.construct_envs(cfg, device="cpu") == "Nav2DRearrVectorEnv"
    _, args, kw = made[-1]
    assert args == (16, 128, 128) and kw["num_actions"] == 6 and kw["max_episode_steps"] == 200
    assert {k: kw[k] for k in ("num_obstacles", "turn_angle", "start_holding", "use_rgb", "use_depth", "distance")} == dict(
        num_obstacles=3, turn_angle=10, start_holding=False, use_rgb=False, use_depth=True, distance="euclidean")
    for task_type, want in (("nav2drearr", "Nav2DRearrVectorEnv"), ("NAV2DREARR-v1", "Nav2DRearrVectorEnv"),
                            ("Nav2DObj-v0", "Nav2DObjVectorEnv"), ("Nav2D-v0", "Nav2DVectorEnv")):
        ov = [f"habitat.task.type={task_type}"] + (["habitat.simulator.sensors.semantic.height=8", "habitat.simulator.sensors.semantic.width=8"]
                                                   if "Obj" in task_type else [])
        assert factory.construct_envs(get_config(name, ov), device="cpu") == want, task_type
    sizes = ["habitat.simulator.sensors.head_rgb.height=40", "habitat.simulator.sensors.head_rgb.width=44",
             "habitat.simulator.sensors.head_depth.height=48", "habitat.simulator.sensors.head_depth.width=52",
             "habitat.synthetic.start_holding=True", "habitat.synthetic.distance_to_goal=geodesic"]
    c = get_config(name, sizes)
    for flags, want, use in ((dict(), (40, 44), (True, True)), (dict(use_rgb=False), (48, 52), (False, True)),
                             (dict(use_rgb=False, use_depth=False), (0, 0), (False, False))):
        assert EF.SyntheticVectorEnvFactory(**flags).construct_envs(c, device="cpu") == "Nav2DRearrVectorEnv"
        _, args, kw = made[-1]
        assert args[1:] == want and (kw["use_rgb"], kw["use_depth"]) == use and kw["start_holding"] is True and kw["distance"] == "geodesic"


def test_observation_space_and_policy_tables():
    """The observation space in its order, built before the constructor asks for the device, which is what is missing here;
    resolve_sensors on it gives the visual table [head_rgb?, head_depth] and the fused widths (2, 2, 1): D = 5."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    from habitat_amd.rl.ppo.policy import resolve_sensors
    for use_rgb in (False, True):
        env = EF.Nav2DRearrVectorEnv.__new__(EF.Nav2DRearrVectorEnv)
        with pytest.raises(_lib.HabError, match="GPU"):
            env.__init__(3, 10, 12, device="cpu", use_rgb=use_rgb, turn_angle=30)
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
    env = EF.Nav2DRearrVectorEnv.__new__(EF.Nav2DRearrVectorEnv)
    with pytest.raises(_lib.HabError, match="GPU"):
        env.__init__(3, 10, 12, device="cpu", use_rgb=False, use_depth=False)
    assert list(env.observation_spaces[0].spaces) == ["obj_start_sensor", "obj_goal_sensor", "is_holding"] and (env.H, env.W) == (0, 0)
    assert EF.Nav2DRearrVectorEnv.consumes_actions and EF.Nav2DRearrVectorEnv.measure_names == A.MEASURES
    assert EF.Nav2DRearrVectorEnv.num_actions == 6 and EF.NAV2D_REARR_SENSORS == A.SENSORS


def test_header_and_signature_table_agree():
    """The header's prototype of hab_nav2d_rearr_step and the ctypes table: the same number of arguments, pointers where the header
    has pointers, the two uint32 and the eight int in their places; the record's named words are those the restatement's
    state_words() are compared at."""
    from habitat_amd import _lib
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "habitat_amd.h")).read()
    m = re.search(r"int hab_nav2d_rearr_step\((.*?)\);", text, re.S)
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    restype, argtypes = _lib.SIGNATURES["hab_nav2d_rearr_step"]
    assert restype is ctypes.c_int and len(params) == len(argtypes) == 26
    for p, t in zip(params, argtypes):
        if "*" in p or p.startswith("hipStream_t"):
            assert t is ctypes.c_void_p, p
        elif p.startswith("uint32_t"):
            assert t is ctypes.c_uint32, p
        else:
            assert p.startswith("int ") and t is ctypes.c_int, p
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["state", "dirs", "ray", "col_cos", "tanv", "actions", "mask", "head_rgb", "head_depth", "obj_start", "obj_goal",
                     "is_holding", "reward", "not_done", "measure_sums", "seed", "env_offset", "N", "H", "W", "num_obstacles",
                     "num_headings", "max_episode_steps", "start_holding", "advance", "stream"]
    assert _lib.SIGNATURES["hab_nav2d_rearr_state_bytes"] == (ctypes.c_int, [])
    words = {k: int(v) for k, v in re.findall(r"#define HAB_NAV2D_REARR_(\w+) (\d+)", text)}
    assert words == dict(STATE_BYTES=272, W_START=56, W_OBJ_START=58, W_GOAL=60, W_OBJ=62, W_HOLDING=64, W_HELD=65, W_PICKS=66,
                         W_INVALID=67)
    assert (words["W_INVALID"] + 1) * 4 == words["STATE_BYTES"] and words["W_START"] * 4 == int(re.search(r"#define HAB_NAV2D_STATE_BYTES (\d+)", text).group(1))
