"""CPU tests of Nav2DImageNav-v0: the numpy restatement tests/nav2d_imagenav_reference.py against the pieces it is built from
(Nav2D-v0's and its geodesic mode's restatements, the object task's gps / compass, Nav2DExplore-v0's markerless view), and the Python
surface of the task (refusals, factory, YAMLs, observation space, header)."""
import collections
import os
import re

import numpy as np
import pytest

import nav2d_explore_reference as X
import nav2d_geo_reference as G
import nav2d_imagenav_reference as I
import nav2d_obj_reference as O
import nav2d_reference as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def explore_view(e, px, py, h):
    """What Nav2DExplore-v0's restatement draws of the world of `e` from the pose (px, py, h)."""
    x = X.Nav2DExploreEnv(e.seed, e.env, H=e.H, W=e.W, num_obstacles=e.K, turn_angle=360 // e.nh, use_rgb=True)
    x.reset()
    x.world, x.px, x.py, x.h = e.world, px, py, h
    return x.observe()


# ---- the goal view ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distance", ["euclidean", "geodesic"])
@pytest.mark.parametrize("K,turn,size", [(0, 10, (12, 20)), (3, 30, (9, 18)), (8, 10, (9, 18))])
def test_goal_view_is_the_markerless_view_from_the_goal_and_changes_only_with_the_episode(distance, K, turn, size):
    out = I.rollout("random", 5, 4, 40, distance=distance, turn_angle=turn, num_obstacles=K, max_episode_steps=7, H=size[0], W=size[1],
                    rng_seed=K)
    obs, dones = out["obs"], out["dones"]
    assert dones.any() and out["counters"]["goal_views_differ"] >= 1
    envs = [I.make_env(5, n, distance, turn_angle=turn, num_obstacles=K, max_episode_steps=7, H=size[0], W=size[1]) for n in range(4)]
    for e in envs:
        e.reset()
    for t in range(41):
        for n, e in enumerate(envs):
            o, w = obs[t][n], e.world
            ref = explore_view(e, w.gx, w.gy, e.gh)
            assert np.array_equal(o["goal_rgb"], ref["rgb"]) and o["goal_rgb"].dtype == np.uint8 and o["goal_rgb"].shape == size + (3,)
            mine = explore_view(e, e.px, e.py, e.h)
            assert np.array_equal(o["rgb"], mine["rgb"]) and np.array_equal(o["depth"], mine["depth"])
            assert set(o) == set(I.SENSORS)
            if t and not dones[t - 1, n]:
                assert np.array_equal(o["goal_rgb"], obs[t - 1][n]["goal_rgb"])
            assert e.gh == I.goal_heading(5, n, e.episode, e.nh) and 0 <= e.gh < e.nh
            rec = e.record()
            assert rec[I.W_GOAL_HEADING] == e.gh and rec.shape == (I.STATE_WORDS,)
        if t < 40:
            for n, e in enumerate(envs):
                e.step(out["actions"][t, n])


def test_the_agent_s_view_carries_no_goal_cylinder():
    """The goal straight ahead at 1.5 m: Nav2D-v0 draws its red cylinder there, this task does not; the depth is the same."""
    e = I.Nav2DImageNavEnv(1, 0, H=12, W=20, num_obstacles=0, turn_angle=30)
    e.reset()
    o = e.place([], 2.0, 4.0, 3.5, 4.0, h=0, gh=3)
    with_marker = R.render(e.px, e.py, F(3.5), F(4.0), 0, [], [], e.ray, e.cosf, e.tanv)
    _, _, _, marker = R.column_hits(e.px, e.py, F(3.5), F(4.0), 0, [], e.ray, e.cosf)
    assert marker.any() and not marker.all()     # Nav2D-v0 would draw its cylinder in the middle columns
    assert np.array_equal(o["depth"], with_marker["depth"])
    differs = np.any(o["rgb"] != with_marker["rgb"], axis=(0, 2))
    assert differs.any() and not differs[~marker].any()
    far = R.render(e.px, e.py, F(0.5), F(4.0), 0, [], [], e.ray, e.cosf, e.tanv)      # a marker behind the camera
    assert np.array_equal(o["rgb"], far["rgb"])
    # the agent at the goal with the goal heading sees the goal image
    o = e.place([(5.0, 3.0, 6.0, 5.0)], 3.5, 4.0, 3.5, 4.0, h=5, gh=5)
    assert np.array_equal(o["rgb"], o["goal_rgb"])
    o = e.place([(5.0, 3.0, 6.0, 5.0)], 3.5, 4.0, 3.5, 4.0, h=5, gh=6)
    assert not np.array_equal(o["rgb"], o["goal_rgb"])


@pytest.mark.parametrize("turn", [10, 30])
def test_goal_heading_takes_every_index(turn):
    nh = 360 // turn
    seen = collections.Counter(I.goal_heading(3, 1, ep, nh) for ep in range(400))
    assert set(seen) == set(range(nh))
    # stream 25 is its own: not the start heading's draw
    w = [R.make_world(3, 1, ep, 0, nh).h for ep in range(400)]
    assert w != [I.goal_heading(3, 1, ep, nh) for ep in range(400)]
    assert I.S_GOAL_HEAD == 25 and I.S_GOAL_HEAD not in (R.S_OBST, R.S_START, R.S_GOAL, R.S_HEAD, R.S_COLOR, 21, 22, 23, 24)


# ---- the tie to Nav2D-v0 ---------------------------------------------------------------------------------------------------------------
def same_run(a, b):
    assert np.array_equal(a["rewards"].view(np.int32), b["rewards"].view(np.int32)) and np.array_equal(a["dones"], b["dones"])
    assert np.array_equal(a["sums"].view(np.int32), b["sums"].view(np.int32))
    for ia, ib in zip(a["infos"], b["infos"]):
        assert [{k: F(v).view(np.int32) for k, v in x.items()} for x in ia] == [{k: F(v).view(np.int32) for k, v in x.items()} for x in ib]


@pytest.mark.parametrize("case", R.SCRIPT_CASES)
def test_success_distance_0p2_is_nav2d_bitwise_euclidean(case):
    K, turn = case
    for kind in R.SCRIPTS:
        ref = R.rollout(kind, R.script_seed(kind, K), R.SCRIPT_ENVS, R.SCRIPT_STEPS, turn_angle=turn, num_obstacles=K,
                        max_episode_steps=R.SCRIPT_MAX_EPISODE_STEPS, H=0, W=0)
        out = I.rollout(None, R.script_seed(kind, K), R.SCRIPT_ENVS, R.SCRIPT_STEPS, turn_angle=turn, num_obstacles=K,
                        max_episode_steps=R.SCRIPT_MAX_EPISODE_STEPS, H=2, W=2, success_distance=0.2, actions=ref["actions"])
        same_run(out, ref)
        assert ref["dones"].any()


@pytest.mark.parametrize("case", G.SCRIPT_CASES)
def test_success_distance_0p2_is_nav2d_bitwise_geodesic(case):
    K, turn = case
    for kind, limit in G.SCRIPT_RUNS:
        ref = G.script_rollout(kind, K, turn, limit)
        out = I.rollout(None, G.SCRIPT_SEED, G.SCRIPT_ENVS, G.SCRIPT_STEPS, distance="geodesic", turn_angle=turn, num_obstacles=K,
                        max_episode_steps=limit, H=2, W=2, success_distance=0.2, actions=ref["actions"])
        same_run(out, ref)
        assert np.array_equal(np.stack(out["fields"]), ref["fields"])
        for t, row in enumerate(ref["states"]):
            for n, st in enumerate(row):
                rec = out["records"][t][n]
                assert rec[:7].view(np.float32).tolist() == [F(v) for v in st[:7]] and rec[7:11].tolist() == list(st[7:])


# ---- success at the boundary ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distance", ["euclidean", "geodesic"])
@pytest.mark.parametrize("sd", [0.2, 1.0, 0.75])
def test_success_at_the_boundary(distance, sd):
    sx, sy = F(sd), F(4.0)        # 2 * sd - sd is exactly sd in float32, and sqrt(fl(x * x)) == x
    at = F(F(2.0) * F(sd))
    seen = set()
    for gx in (np.nextafter(at, F(0)), at, np.nextafter(at, F(9))):
        e = I.make_env(1, 0, distance, H=2, W=2, num_obstacles=0, success_distance=sd)
        e.reset()
        e.place([], sx, sy, gx, sy)
        d = R.dist(sx, sy, gx, sy)
        _, reward, done, info = e.step(I.STOP)
        want = bool(d < F(sd))
        seen.add((bool(d < F(sd)), bool(d == F(sd))))
        assert done and info["success"] == float(want) and info["distance_to_goal"] == float(d)
        assert reward == F(F(F(-0.01) + F(d - d)) + (F(2.5) if want else F(0.0)))
        assert info["spl"] == (1.0 if want else 0.0)
    assert seen == {(True, False), (False, True), (False, False)}, seen   # below succeeds; d == success_distance and above fail


def test_default_success_distance_is_the_object_task_s():
    e = I.Nav2DImageNavEnv(1, 0)
    assert e.success_distance == F(1.0) and I.DEFAULT_SUCCESS_DISTANCE == 1.0


# ---- the scripted sequences ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", I.SCRIPT_CASES)
def test_scripts_show_every_event(case):
    """The four scripts of a case together: a success, a STOP that fails, a step-limit end, a collision and a rollover whose goal view
    differs from the previous episode's."""
    total = collections.Counter()
    for kind in I.SCRIPTS:
        out = I.script_rollout(kind, case)
        total.update(out["counters"])
        assert out["records"][0].shape == (I.SCRIPT_ENVS, I.STATE_WORDS) and len(out["records"]) == I.SCRIPT_STEPS + 1
    for k in I.SCRIPT_EVENTS:
        assert total[k] >= 1, (k, dict(total))


def test_script_forms_cover_every_shape():
    forms = {I.script_form(kind, case) for case in I.SCRIPT_CASES for kind in I.SCRIPTS}
    assert forms == set(I.FORMS) and len(I.FORMS) == 8
    assert {f[0] for f in forms} == {0.2, 1.0} and {f[1] for f in forms} == {"euclidean", "geodesic"}
    assert {f[2] for f in forms} == {(12, 20), (9, 18)}


# ---- gps and compass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("turn", [10, 30])
def test_gps_and_compass_are_the_object_task_s(turn):
    nh = 360 // turn
    tab = O.compass_table(turn)
    e = I.Nav2DImageNavEnv(7, 0, H=2, W=2, num_obstacles=0, turn_angle=turn, max_episode_steps=10 * nh)
    o = e.reset()
    assert o["gps"].tolist() == [0.0, 0.0] and o["compass"].tolist() == [0.0] and (e.sx, e.sy, e.h0) == (e.px, e.py, e.h)
    rng = np.random.RandomState(turn)
    wrapped = set()
    for _ in range(4 * nh):
        o = e.step(int(rng.randint(1, 4)))[0]
        c, s = e.dirs[e.h0]
        dx, dy = F(e.px - e.sx), F(e.py - e.sy)
        assert o["gps"].tolist() == [F(F(dx * c) + F(dy * s)), F(F(c * dy) - F(s * dx))] and o["gps"].dtype == np.float32
        assert o["compass"].tolist() == [tab[(e.h - e.h0) % nh]]
        wrapped.add(np.sign(o["compass"][0]))
    assert (e.px, e.py) != (e.sx, e.sy) and wrapped >= {-1.0, 1.0}
    e.h = (e.h0 + nh // 2) % nh                  # half a turn from the start heading: +pi, not -pi
    assert e.observe()["compass"][0] == F(np.pi)


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
BAD = [(dict(use_rgb=False), "rgb"), (dict(num_actions=6), "Discrete"), (dict(num_actions=1), "Discrete"),
       (dict(success_distance=0.0), "success_distance"), (dict(success_distance=-1.0), "success_distance"),
       (dict(success_distance=float("inf")), "success_distance"), (dict(success_distance=float("nan")), "success_distance"),
       (dict(success_distance=1e39), "success_distance"), (dict(success_distance="near"), "success_distance"),
       (dict(success_distance=None), "success_distance"), (dict(success_distance=True), "success_distance"),
       (dict(success_distance=0.19, distance="geodesic"), "follower"), (dict(distance="manhattan"), "distance")]


@pytest.mark.parametrize("kw,word", BAD)
def test_refusals_name_the_task_and_the_parameter(kw, word):
    """Every parameter out of range is refused by name, before the device is touched, and by the restatement alike."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    with pytest.raises(_lib.HabError, match=word) as err:
        EF.Nav2DImageNavVectorEnv(2, 8, 8, device="cpu", **kw)
    assert "Nav2DImageNav:" in str(err.value)
    with pytest.raises(ValueError):
        I.make_env(1, 0, kw.get("distance", "euclidean"), **{k: v for k, v in kw.items() if k != "distance"})


def test_other_refusals():
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    for kw in (dict(turn_angle=7), dict(num_obstacles=9), dict(max_episode_steps=0), dict(top_down_map="yes")):
        with pytest.raises(_lib.HabError):
            EF.Nav2DImageNavVectorEnv(2, 8, 8, device="cpu", **kw)
    for size in ((0, 8), (8, 0), (-1, 8)):
        with pytest.raises(_lib.HabError, match="Nav2DImageNav.*image size"):
            EF.Nav2DImageNavVectorEnv(2, *size, device="cpu")
        with pytest.raises(ValueError):
            I.Nav2DImageNavEnv(1, 0, H=size[0], W=size[1])
    # valid parameters: only the missing device is refused; 0.19 is fine in the Euclidean mode, 0.2 in the geodesic one
    for kw in (dict(), dict(success_distance=0.19), dict(success_distance=0.2, distance="geodesic"), dict(use_depth=False)):
        with pytest.raises(_lib.HabError, match="Nav2DImageNav.*GPU"):
            EF.Nav2DImageNavVectorEnv(2, 8, 8, device="cpu", **kw)
    env = EF.Nav2DImageNavVectorEnv.__new__(EF.Nav2DImageNavVectorEnv)
    env.num_envs, env._pending, env._actions_host, env.distance = 3, set(), np.zeros(3, np.int64), "euclidean"
    env.async_step_at(0, 3)
    env.async_step_at(2, {"action": np.array([1])})
    assert env._pending == {0, 2} and env._actions_host.tolist() == [3, 0, 1]
    for a in (4, -1, 0.5, [1, 2]):
        with pytest.raises(_lib.HabError):
            env.async_step_at(1, a)
    for call in (lambda: env.reset_into(None, None, None), lambda: env.step_into(None, None, None, None, None)):
        with pytest.raises(_lib.HabError, match="Nav2DImageNav: the task has no pointgoal sensor"):
            call()
    with pytest.raises(_lib.HabError, match="Nav2DImageNav.*actions"):
        env.step_into_obs({}, None, None)


def test_teacher_and_follower():
    """In the geodesic mode the teacher is Nav2D-v0's follower on this record; in the Euclidean mode both refuse by name."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    cls = EF.Nav2DImageNavVectorEnv
    assert cls._expert_method == "follower_actions" and cls._follow_entry == "hab_nav2d_follow" == EF.Nav2DVectorEnv._follow_entry
    assert cls._entries == ("hab_nav2d_imagenav_step", "hab_nav2d_imagenav_step_geo") and cls._map_task == EF.NAV2D_MAP_TASK_GOAL == I.TASK_GOAL
    assert cls._geo_bytes == "hab_nav2d_geo_bytes" and cls.measure_names == I.MEASURES and cls._frame_keys == ("rgb", "depth")
    env = cls.__new__(cls)
    env.distance = "euclidean"
    for call in (env.follower_actions, env.expert_actions):
        with pytest.raises(_lib.HabError, match="Nav2DImageNav: the shortest-path follower needs `distance_to_goal: geodesic`"):
            call()
    called = []
    env.distance = "geodesic"
    env._advised_actions = lambda entry, method, *a: called.append((entry, method)) or "acts"
    assert env.expert_actions() == "acts" and called == [("hab_nav2d_follow", "follower_actions")]
    assert F(EF.NAV2D_FOLLOWER_STOP_DISTANCE) == I.FOLLOWER_STOP_DISTANCE == R.SUCCESS_DIST
    for sd in (0.2, 1, np.float32(0.3), 2.5):
        assert EF.nav2d_imagenav_success_distance(sd, "geodesic") == float(F(sd))


def test_factory_choice_and_configs(monkeypatch):
    """habitat.task.type picks the env: a type starting with 'nav2dimagenav' (any case) the new one -- the prefix is tested before
    'nav2d' -- while the sibling tasks keep their classes.  Both YAMLs load.  The constructors are replaced by recorders: the envs
    themselves need a GPU."""
    from habitat_amd.common import env_factory as EF
    from habitat_amd.config.default import get_config
    from habitat_amd.rl.ppo.ppo_trainer import PPOTrainer
    assert "Nav2DImageNav-v0" in PPOTrainer.supported_tasks
    names = ("imagenav/ddppo_nav2d_imagenav.yaml", "imagenav/dagger_nav2d_imagenav_geodesic.yaml")
    made = []
    classes = ("Nav2DImageNavVectorEnv", "Nav2DExploreVectorEnv", "Nav2DSocialVectorEnv", "Nav2DRearrVelVectorEnv", "Nav2DRearrVectorEnv",
               "Nav2DObjVectorEnv", "Nav2DVelVectorEnv", "Nav2DVectorEnv", "SyntheticVectorEnv")
    cfgs = [get_config(n) for n in names]
    for cfg in cfgs:
        hab, hb = cfg.habitat, cfg.habitat_baselines
        assert hab.task.type == "Nav2DImageNav-v0" and list(hab.task.actions) == ["stop", "move_forward", "turn_left", "turn_right"]
        assert list(hab.task.lab_sensors) == ["gps", "compass"] and hab.environment.max_episode_steps == 200
        s = hab.simulator.sensors
        assert s.rgb.height == s.rgb.width == s.depth.height == s.depth.width == 64
        assert hb.rl.ddppo.backbone == "resnet18" and hb.rl.policy.main_agent.name == "PointNavResNetPolicy"
        assert hab.synthetic.success_distance == 1.0 and hab.synthetic.distance_to_goal == "geodesic"
    dag = cfgs[1].habitat_baselines
    assert dag.updater_name == "DAgger" and dag.rollout_storage_name == "ImitationRolloutStorage" and dag.rl.imitation.enabled
    assert not getattr(getattr(cfgs[0].habitat_baselines.rl, "imitation", None), "enabled", False)
    for cls in classes:
        monkeypatch.setattr(EF, cls, lambda *a, _n=cls, **kw: made.append((_n, a, kw)) or _n)
    for cfg in cfgs:
        factory = EF.instantiate(cfg.habitat_baselines.vector_env_factory)
        assert factory.construct_envs(cfg, device="cpu") == "Nav2DImageNavVectorEnv"
        _, args, kw = made[-1]
        assert args == (16, 64, 64) and kw["num_actions"] == 4 and kw["max_episode_steps"] == 200
        assert {k: kw[k] for k in ("num_obstacles", "turn_angle", "success_distance", "use_rgb", "use_depth", "distance")} == dict(
            num_obstacles=3, turn_angle=10, success_distance=1.0, use_rgb=True, use_depth=True, distance="geodesic")
        assert "top_down_map" not in kw
    name = names[0]
    ov = ["habitat.synthetic.success_distance=0.5", "habitat.task.measurements.top_down_map.map_resolution=30"]
    for task_type, want in (("nav2dimagenav", "Nav2DImageNavVectorEnv"), ("NAV2DIMAGENAV-v1", "Nav2DImageNavVectorEnv"),
                            ("Nav2DImageNavigation", "Nav2DImageNavVectorEnv"), ("Nav2DImage-v0", "Nav2DVectorEnv"),
                            ("Nav2D-v0", "Nav2DVectorEnv"), ("Nav2DExplore-v0", "Nav2DExploreVectorEnv")):
        assert factory.construct_envs(get_config(name, ov + [f"habitat.task.type={task_type}"]), device="cpu") == want, task_type
        _, _, kw = made[-1]
        assert kw["top_down_map"] == dict(map_resolution=30)
        assert kw.get("success_distance") == (0.5 if want == "Nav2DImageNavVectorEnv" else None)
    for yaml, want in (("pointnav/ppo_nav2d.yaml", "Nav2DVectorEnv"), ("pointnav/ppo_nav2d_vel.yaml", "Nav2DVelVectorEnv"),
                       ("objectnav/ddppo_nav2d_objectnav.yaml", "Nav2DObjVectorEnv"), ("rearrange/ddppo_nav2d_rearrange.yaml", "Nav2DRearrVectorEnv"),
                       ("social_nav/ddppo_nav2d_social.yaml", "Nav2DSocialVectorEnv"), ("exploration/ddppo_nav2d_explore.yaml", "Nav2DExploreVectorEnv")):
        assert EF.SyntheticVectorEnvFactory().construct_envs(get_config(yaml), device="cpu") == want
    # the image size is the rgb sensor's; without the key the default success distance; without rgb the class itself refuses
    c = get_config(name, ["habitat.simulator.sensors.rgb.height=40", "habitat.simulator.sensors.rgb.width=44"])
    del c.habitat.synthetic["success_distance"]
    assert EF.SyntheticVectorEnvFactory().construct_envs(c, device="cpu") == "Nav2DImageNavVectorEnv"
    assert made[-1][1][1:] == (40, 44) and made[-1][2]["success_distance"] == 1.0
    assert EF.SyntheticVectorEnvFactory(use_rgb=False).construct_envs(cfgs[0], device="cpu") == "Nav2DImageNavVectorEnv"
    assert made[-1][2]["use_rgb"] is False and made[-1][1][1:] == (0, 0)


def test_observation_space():
    """rgb, depth, goal_rgb, gps, compass in this order: three visual rows of 3 + 1 + 3 = 7 channels and no fused row; the spaces are
    built before the constructor asks for the device, which is what is missing here."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    from habitat_amd.rl.ppo.policy import GOAL_SENSOR_KEYS, resolve_sensors
    for use_depth in (True, False):
        env = EF.Nav2DImageNavVectorEnv.__new__(EF.Nav2DImageNavVectorEnv)
        with pytest.raises(_lib.HabError, match="GPU"):
            env.__init__(3, 10, 12, device="cpu", use_depth=use_depth, turn_angle=30)
        sp = env.observation_spaces[0].spaces
        assert list(sp) == ["rgb"] + (["depth"] if use_depth else []) + ["goal_rgb", "gps", "compass"]
        assert list(sp) == [k for k in I.SENSORS if k in sp] == [k for k in EF.NAV2D_IMAGENAV_SENSORS if k in sp]
        assert sp["goal_rgb"].shape == sp["rgb"].shape == (10, 12, 3) and sp["goal_rgb"].dtype == np.uint8 and sp["goal_rgb"].high.max() == 255
        assert sp["gps"].shape == (2,) and sp["compass"].shape == (1,) and sp["gps"].dtype == sp["compass"].dtype == np.float32
        assert (env.H, env.W) == (10, 12) and env.action_spaces[0].n == 4 and env.success_distance == 1.0
        visual, fused = resolve_sensors(env.observation_spaces[0])
        assert [v[0] for v in visual] == [k for k in ("rgb", "depth", "goal_rgb") if k in sp] and fused == []
        assert sum(v[2] for v in visual) == (7 if use_depth else 6)
        if use_depth:
            assert [(v[1], v[2]) for v in visual] == [(_lib.DTYPE_U8, 3), (_lib.DTYPE_F32, 1), (_lib.DTYPE_U8, 3)]
            assert visual[0][3] == visual[2][3] == float(F(1.0 / 255.0)) and visual[1][3] == 1.0
    assert "goal_rgb" not in GOAL_SENSOR_KEYS and "imagegoal" not in sp
    assert EF.Nav2DImageNavVectorEnv.consumes_actions and np.array_equal(EF.nav2d_compass_table(30), O.compass_table(30))


def test_header_binding_and_tables_agree():
    from habitat_amd import _lib
    src = open(os.path.join(ROOT, "include", "habitat_amd.h")).read()
    d = {k: int(v, 0) for k, v in re.findall(r"#define (HAB_NAV2D_(?:IMAGENAV|GEO|STATE)_?[A-Z0-9_]*) (-?(?:0x)?[0-9A-Fa-f]+)\b", src)}
    L = _lib.lib()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("hab_nav2d_imagenav_state_bytes", "hab_nav2d_imagenav_step", "hab_nav2d_imagenav_step_geo"):
        decl = re.search(name + r"\((.*?)\);", plain, flags=re.S).group(1)
        count = 0 if decl.strip() == "void" else decl.count(",") + 1
        assert count == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name)
    # hab_nav2d_explore_step's arguments without coverage, G, visibility_dist and rc, plus goal_rgb and success_distance
    exp, img, geo = (_lib.SIGNATURES[k][1] for k in ("hab_nav2d_explore_step", "hab_nav2d_imagenav_step", "hab_nav2d_imagenav_step_geo"))
    assert len(img) == len(exp) - 4 + 2 == 27 and img.count(_lib.c_float) == 1 and img[-1] is _lib.vp and img[-3] is _lib.c_float
    assert geo == [_lib.vp] + img
    assert L.hab_nav2d_imagenav_state_bytes() == d["HAB_NAV2D_IMAGENAV_STATE_BYTES"] == 4 * I.STATE_WORDS == L.hab_nav2d_state_bytes() + 16
    names = ("GOAL_HEADING", "START_X", "START_Y", "START_HEADING")
    assert [d[f"HAB_NAV2D_IMAGENAV_W_{k}"] for k in names] == [I.W_GOAL_HEADING, I.W_START_X, I.W_START_Y, I.W_START_HEADING] == list(range(56, 60))
    assert L.hab_nav2d_geo_bytes() == d["HAB_NAV2D_GEO_BYTES"] == 4 * G.GEO_WORDS
