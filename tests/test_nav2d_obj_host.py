"""CPU: the Nav2DObj-v0 restatement (tests/nav2d_obj_reference.py) holds its own invariants, the scripted sequences the GPU tests
replay show every event they are there for, and the Python surface (parameters, factory, tables) behaves without a device."""
import collections
import functools
import math

import numpy as np
import pytest

import nav2d_obj_reference as O
import nav2d_reference as R

F = np.float32


def blind(seed=3, env=0, **kw):
    e = O.Nav2DObjEnv(seed, env, **dict(dict(num_obstacles=3, num_objects=3, num_categories=4, max_episode_steps=40), **kw))
    e.reset()
    return e


def assert_world_invariants(w, objects, cats, target, M, C):
    assert len(objects) == len(cats) == M and all(0 <= c < C for c in cats) and target in cats
    assert O.is_free(w.sx, w.sy, w.rects, objects)                                   # the start is free
    for j, (x, y) in enumerate(objects):
        assert 0.5 <= x <= 7.5 and 0.5 <= y <= 7.5
        assert R.dist(w.sx, w.sy, x, y) >= 1.0
        assert not any(x > x0 - O.OBJ_R and x < x1 + O.OBJ_R and y > y0 - O.OBJ_R and y < y1 + O.OBJ_R for x0, y0, x1, y1 in w.rects)
        for ox, oy in objects[:j]:
            assert R.dist(ox, oy, x, y) >= 1.0


@pytest.mark.parametrize("K,M,C", [(0, 1, 1), (3, 3, 4), (8, 8, 4), (8, 8, 21)])
def test_world_invariants(K, M, C):
    """The start is free, objects are at least 1 m apart, at least 1 m from the start and clear of the grown rectangles, and the
    target category is present, over 300 worlds per parameter set."""
    for env in range(30):
        for episode in range(10):
            w, objects, cats, target, _ = O.make_world(7, env, episode, K, 36, M, C)
            assert_world_invariants(w, objects, cats, target, M, C)


def test_category_colours_are_fixed_and_distinct():
    cols = [O.category_color(c) for c in range(O.MAX_CATEGORIES)]
    assert len(set(cols)) == O.MAX_CATEGORIES and all(128 <= v <= 255 for c in cols for v in c)
    a, b = blind(seed=1), blind(seed=2)
    assert O.category_color(a.cats[0]) == O.category_color(a.cats[0]) and a.objects != b.objects


@pytest.mark.parametrize("obj_candidates", [0, 1, 2])
def test_fallback_rule(obj_candidates):
    """With few candidates objects fall back to the ring: every invariant still holds, fallback objects sit on ring slots, and with
    no candidate at all the objects are the first fitting slots in order."""
    ring = [O.ring_slot(q) for q in range(O.RING_SLOTS)]
    assert len(set(ring)) == 28 and all(min(x, y) == 0.5 or max(x, y) == 7.5 for x, y in ring)
    for a, b in zip(ring, ring[1:] + ring[:1]):
        assert R.dist(*a, *b) == 1.0
    fallbacks = 0
    for env in range(40):
        w, objects, cats, target, fb = O.make_world(11, env, 0, 8, 36, 8, 4, obj_candidates=obj_candidates)
        assert_world_invariants(w, objects, cats, target, 8, 4)
        fallbacks += fb
        assert sum(o in ring for o in objects) >= fb
        if obj_candidates == 0:
            assert fb == 8 and all(o in ring for o in objects)
            qs = [ring.index(o) for o in objects]
            assert qs == sorted(qs)
    assert fallbacks > 0
    full = sum(O.make_world(11, env, 0, 8, 36, 8, 4)[4] for env in range(40))
    assert full < fallbacks


def test_rewards_telescope():
    """Over an episode the rewards sum to d_start - d_end plus the slack per step and the bonus on success, whichever instance is
    the nearest at each step."""
    rng = np.random.RandomState(0)
    outcomes = set()
    for script in ("greedy", "random", "wander"):   # wander never stops: long episodes across several nearest instances
        e = blind(seed=4, turn_angle=30, num_objects=8, num_categories=1 if script == "wander" else 2, num_actions=6)
        for _ in range(12):
            d_start, acc, steps = float(e.d_start), 0.0, 0
            while True:
                _, r, done, info = e.step(O.greedy_action(e, 30) if script == "greedy" else rng.randint(int(script == "wander"), 6))
                acc, steps = acc + float(r), steps + 1
                if done:
                    break
            want = (d_start - info["distance_to_goal"]) - 0.01 * steps + 2.5 * info["success"]
            assert math.isclose(acc, want, rel_tol=0, abs_tol=1e-5 * steps), (script, e.episode)
            outcomes.add((script, info["success"]))
        assert e.counters["nearest_changes"] > 0 or script != "wander"
    assert ("greedy", 1.0) in outcomes and ("random", 0.0) in outcomes


def test_looks_change_nothing_but_the_step_count():
    e = blind(num_actions=6)
    for a in (O.LOOK_UP, O.LOOK_DOWN, O.LOOK_UP):
        before = e.state_words()
        o0 = e.observe()
        o, r, done, _ = e.step(a)
        after = e.state_words()
        assert not done and r == F(-0.01)
        assert after["ints"][1] == before["ints"][1] + 1
        after["ints"][1] = before["ints"][1]
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        assert all(np.array_equal(o[k], o0[k]) for k in o0)
    with pytest.raises(ValueError):
        blind(num_actions=4).step(O.LOOK_UP)


@pytest.mark.parametrize("turn", [10, 30])
def test_gps_and_compass(turn):
    """(0, 0) and 0 at a reset; the compass follows the turns through (-pi, pi] and wraps at the half turn, at both turn angles; gps is
    the forward distance along the start heading after moving forward without turning."""
    nh = 360 // turn
    tab = O.compass_table(turn)
    assert tab.shape == (nh,) and tab[0] == 0 and tab[nh // 2] == F(math.pi) and tab.max() == F(math.pi) and tab.min() > -F(math.pi)
    assert np.allclose(tab[1:nh // 2], np.radians(turn * np.arange(1, nh // 2)), rtol=1e-6)
    assert np.allclose(tab[nh // 2 + 1:], -np.radians(turn * np.arange(nh // 2 - 1, 0, -1)), rtol=1e-6)
    e = blind(turn_angle=turn, num_obstacles=0, num_objects=1, max_episode_steps=10 * nh)
    o = e.observe()
    assert o["gps"].tolist() == [0.0, 0.0] and o["compass"].tolist() == [0.0] and o["objectgoal"].dtype == np.int64
    for k in range(1, nh + 1):            # a full left circle: +turn ... +pi, then the negative half back to 0
        o = e.step(O.TURN_LEFT)[0]
        assert o["compass"][0] == tab[k % nh]
        assert (o["compass"][0] > 0) == (0 < k <= nh // 2) and o["gps"].tolist() == [0.0, 0.0]
    for k in range(1, nh // 2 + 2):       # a right half circle and one more: -turn ... then +pi, +pi - turn
        o = e.step(O.TURN_RIGHT)[0]
        assert o["compass"][0] == tab[(-k) % nh]
    assert o["compass"][0] == tab[nh // 2 - 1] > 0
    e = blind(turn_angle=turn, num_obstacles=0, num_objects=1, seed=5)
    moved = 0
    for _ in range(3):
        before = (e.px, e.py)
        o = e.step(O.MOVE_FORWARD)[0]
        moved += int((e.px, e.py) != before)
        assert abs(o["gps"][0] - 0.25 * moved) < 1e-5 and abs(o["gps"][1]) < 1e-5 and o["compass"][0] == 0
    assert moved > 0
    o = e.step(O.TURN_LEFT)[0]
    assert abs(o["gps"][0] - 0.25 * moved) < 1e-5   # gps is in the START heading's frame: a turn does not move it


def test_semantic_ids_and_geometry():
    """The three images agree on what a pixel shows: semantic ids are floor 0, ceiling 1 (upper half), walls 2, rectangles 3, objects
    4 + category; depth at an object pixel is below what the same column had without objects."""
    e = O.Nav2DObjEnv(1, 0, H=12, W=20, num_obstacles=3, num_objects=8, num_categories=4, turn_angle=30)
    seen = set()
    for ep in range(6):
        e.episode = ep
        e._begin()
        for h in range(e.nh):
            e.h = h
            o = e.observe()
            sem = o["semantic"][..., 0]
            seen |= set(np.unique(sem).tolist())
            assert set(np.unique(sem[:6]).tolist()) & {O.SEM_FLOOR} == set() and set(np.unique(sem[6:]).tolist()) & {O.SEM_CEILING} == set()
            bare = O.render(e.px, e.py, e.h, e.world.rects, e.world.colors, [], [], e.ray, e.cosf, e.tanv)
            obj = sem >= O.SEM_OBJECT
            assert np.all(o["depth"][..., 0][obj] <= bare["depth"][..., 0][obj])
            assert np.array_equal(o["depth"][~obj.any(0)[None, :].repeat(12, 0)], bare["depth"][~obj.any(0)[None, :].repeat(12, 0)])
            for c in set(sem[obj].tolist()):
                col = np.array(O.category_color(c - O.SEM_OBJECT))
                px = o["rgb"][sem == c]
                assert np.all(px <= col) and px.max() > 0
    assert {0, 1, 2, 3} <= seen and len(seen) > 4 and max(seen) <= O.SEM_OBJECT + 3


@functools.lru_cache(maxsize=None)
def script_counters():
    total = collections.Counter()
    per_script = {k: collections.Counter() for k in O.SCRIPTS}
    for case in O.SCRIPT_CASES[::5] + [(8, 30, 8, 1), (3, 10, 8, 4)]:   # a spread over the cases (every K, turn, M and C occurs)
        for kind in O.SCRIPTS:
            c = O.script_rollout(kind, case, H=12, W=20)["counters"]
            total.update(c)
            per_script[kind].update(c)
    return total, per_script


def test_scripts_show_every_event():
    """Over the scripted sequences of the GPU tests: success, STOP too far, timeout, blocked by an object, a rectangle and a wall,
    the nearest instance changing, an object hidden behind a rectangle and an object visible in the image all happen."""
    total, per_script = script_counters()
    for k in ("successes", "stop_too_far", "timeouts", "blocked_object", "blocked_rect", "blocked_wall", "nearest_changes",
              "objects_hidden", "objects_visible", "looks", "episodes"):
        assert total[k] >= 1, (k, dict(total))
    assert per_script["greedy"]["successes"] >= 1 and per_script["random"]["stop_too_far"] >= 1
    assert per_script["never_stop"]["timeouts"] >= 1 and per_script["never_stop"]["successes"] == 0
    assert per_script["forward"]["blocked_wall"] + per_script["forward"]["blocked_rect"] + per_script["forward"]["blocked_object"] >= 1


def test_refusals(monkeypatch):
    """Every parameter the env refuses, refused before the device is touched, and by the restatement alike."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    bad = [dict(num_objects=0), dict(num_objects=9), dict(num_objects=2.0), dict(num_objects=True), dict(num_categories=0),
           dict(num_categories=22), dict(num_categories=1.5), dict(num_actions=5), dict(num_actions=1), dict(num_actions=7),
           dict(turn_angle=7), dict(num_obstacles=9), dict(max_episode_steps=0)]
    for kw in bad:
        with pytest.raises(_lib.HabError):
            EF.Nav2DObjVectorEnv(2, 8, 8, device="cpu", **kw)
        ref_kw = {k: v for k, v in kw.items() if k in ("num_objects", "num_categories", "num_actions", "turn_angle", "num_obstacles")}
        if ref_kw:
            with pytest.raises(ValueError):
                O.Nav2DObjEnv(1, 0, **ref_kw)
    for size in ((0, 8), (8, 0)):
        with pytest.raises(_lib.HabError, match="semantic"):
            EF.Nav2DObjVectorEnv(2, *size, device="cpu")
    with pytest.raises(_lib.HabError, match="GPU"):   # valid parameters: only the missing device is refused
        EF.Nav2DObjVectorEnv(2, 8, 8, device="cpu", num_objects=8, num_categories=21, num_actions=4)
    # the host path checks actions against 0..num_actions-1; the goal-sensor forms and pausing are refused
    for n_act in (4, 6):
        env = EF.Nav2DObjVectorEnv.__new__(EF.Nav2DObjVectorEnv)
        env.num_envs, env._pending, env._actions_host, env.num_actions = 3, set(), np.zeros(3, np.int64), n_act
        env.async_step_at(0, n_act - 1)
        env.async_step_at(2, {"action": np.array([1])})
        assert env._pending == {0, 2} and env._actions_host.tolist() == [n_act - 1, 0, 1]
        for a in (n_act, -1, 0.5, [1, 2], 6):
            with pytest.raises(_lib.HabError):
                env.async_step_at(1, a)
        with pytest.raises(_lib.HabError):
            env.async_step_at(0, 1)   # twice without wait_step_at
        for call in (lambda: env.reset_into(None, None, None), lambda: env.step_into(None, None, None, None, None),
                     lambda: env.step_into_obs({}, None, None), lambda: env.pause_at(0)):
            with pytest.raises(_lib.HabError):
                call()


def test_factory_choice_and_config(monkeypatch):
    """habitat.task.type picks the env: 'Nav2DObj-v0' / 'nav2dobj' the new one, while 'Nav2D-v0' and 'Nav2DVel-v0' still get their own
    classes and 'ObjectNav-v1' the hashed source.  The image size comes from rgb, else depth, else semantic.  The constructors are
    replaced by recorders: the envs themselves need a GPU."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    from habitat_amd.config.default import get_config
    from habitat_amd.rl.ppo.ppo_trainer import PPOTrainer
    assert "Nav2DObj-v0" in PPOTrainer.supported_tasks
    name = "objectnav/ddppo_nav2d_objectnav.yaml"
    cfg = get_config(name)
    hab = cfg.habitat
    assert hab.task.type == "Nav2DObj-v0" and len(hab.task.actions) == 6 and list(hab.task.lab_sensors) == ["objectgoal", "compass", "gps"]
    assert all(hab.simulator.sensors[s].height == hab.simulator.sensors[s].width == 128 for s in ("rgb", "depth", "semantic"))
    assert cfg.habitat_baselines.rl.ddppo.backbone == "resnet18"
    assert cfg.habitat_baselines.rl.policy.main_agent.name == "PointNavResNetPolicy"
    made = []
    for cls in ("Nav2DObjVectorEnv", "Nav2DVelVectorEnv", "Nav2DVectorEnv", "SyntheticVectorEnv"):
        monkeypatch.setattr(EF, cls, lambda *a, _n=cls, **kw: made.append((_n, a, kw)) or _n)
    factory = EF.SyntheticVectorEnvFactory()
    assert factory.construct_envs(cfg, device="cpu") == "Nav2DObjVectorEnv"
    _, args, kw = made[-1]
    assert args == (16, 128, 128) and kw["num_actions"] == 6 and kw["max_episode_steps"] == 200
    assert {k: kw[k] for k in ("num_obstacles", "turn_angle", "num_objects", "num_categories", "use_rgb", "use_depth")} == dict(
        num_obstacles=3, turn_angle=10, num_objects=3, num_categories=4, use_rgb=True, use_depth=True)
    for task_type, want in (("nav2dobj", "Nav2DObjVectorEnv"), ("NAV2DOBJ-v1", "Nav2DObjVectorEnv"), ("ObjectNav-v1", "SyntheticVectorEnv")):
        assert factory.construct_envs(get_config(name, [f"habitat.task.type={task_type}"]), device="cpu") == want, task_type
    assert factory.construct_envs(get_config("pointnav/ppo_nav2d.yaml"), device="cpu") == "Nav2DVectorEnv"
    assert factory.construct_envs(get_config("pointnav/ppo_nav2d_vel.yaml"), device="cpu") == "Nav2DVelVectorEnv"
    # the image size: rgb, else depth, else semantic
    sizes = ["habitat.simulator.sensors.rgb.height=40", "habitat.simulator.sensors.rgb.width=44", "habitat.simulator.sensors.depth.height=48",
             "habitat.simulator.sensors.depth.width=52", "habitat.simulator.sensors.semantic.height=56",
             "habitat.simulator.sensors.semantic.width=60", "habitat.synthetic.num_objects=8", "habitat.synthetic.num_categories=21"]
    c = get_config(name, sizes)
    for flags, want in ((dict(), (40, 44)), (dict(use_rgb=False), (48, 52)), (dict(use_rgb=False, use_depth=False), (56, 60))):
        assert EF.SyntheticVectorEnvFactory(**flags).construct_envs(c, device="cpu") == "Nav2DObjVectorEnv"
        _, args, kw = made[-1]
        assert args[1:] == want and (kw["num_objects"], kw["num_categories"]) == (8, 21)
        assert (kw["use_rgb"], kw["use_depth"]) == (flags.get("use_rgb", True), flags.get("use_depth", True))


def test_observation_space_and_tables():
    """The ObjectNav observation space with the hashed task's ranges (40 ids, 21 categories), also without rgb and depth -- it is
    built before the constructor asks for the device, which is what is missing here; the host tables' shapes; the library's table."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    for use in ((True, True), (False, False), (False, True)):
        env = EF.Nav2DObjVectorEnv.__new__(EF.Nav2DObjVectorEnv)
        with pytest.raises(_lib.HabError, match="GPU"):
            env.__init__(3, 10, 12, device="cpu", use_rgb=use[0], use_depth=use[1], turn_angle=30)
        sp = env.observation_spaces[0].spaces
        want = {"semantic", "objectgoal", "compass", "gps"} | ({"rgb"} if use[0] else set()) | ({"depth"} if use[1] else set())
        assert set(sp) == want and EF.GOAL_UUID not in sp and (env.H, env.W) == (10, 12)
        assert sp["semantic"].shape == (10, 12, 1) and sp["semantic"].dtype == np.int32 and sp["semantic"].high.max() == 39
        assert sp["objectgoal"].shape == (1,) and sp["objectgoal"].dtype == np.int64 and sp["objectgoal"].high.max() == 20
        assert sp["gps"].shape == (2,) and sp["compass"].shape == (1,)
    assert EF.Nav2DObjVectorEnv.consumes_actions and EF.Nav2DObjVectorEnv.measure_names == R.MEASURES
    dirs, ray, col_cos, tanv = EF.nav2d_tables(30, 10, 12)
    assert dirs.shape == (12, 2) and ray.shape == (12, 12, 2) and col_cos.shape == (12,) and tanv.shape == (10,)
    rt, ct, tv = O.ray_tables(30, 10, 12)
    assert np.array_equal(ray, rt) and np.array_equal(col_cos, ct) and np.array_equal(tanv, tv) and np.array_equal(dirs, O.heading_table(30))
    for turn in (10, 30, 1, 120):
        tab = EF.nav2d_compass_table(turn)
        assert tab.shape == (360 // turn,) and tab.dtype == np.float32 and np.array_equal(tab, O.compass_table(turn))
    restype, argtypes = _lib.SIGNATURES["hab_nav2d_obj_step"]
    assert len(argtypes) == 30 and _lib.SIGNATURES["hab_nav2d_obj_state_bytes"][1] == []
