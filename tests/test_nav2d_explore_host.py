"""CPU: the Nav2DExplore-v0 restatement (tests/nav2d_explore_reference.py) holds its own invariants on random and hand-made worlds,
the scripted sequences the GPU tests replay show every event they are there for, and the Python surface (parameters, factory, YAML,
observation space, header and binding) behaves without a device."""
import collections
import os
import re

import numpy as np
import pytest

import nav2d_explore_reference as X
import nav2d_map_reference as M
import nav2d_obj_reference as O
import nav2d_reference as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fresh(seed=3, env=0, **kw):
    e = X.Nav2DExploreEnv(seed, env, **dict(dict(num_obstacles=3, coverage_resolution=32, max_episode_steps=40), **kw))
    e.reset()
    return e


def cell_of(G, x, y):
    """(row, column) of the cell whose centre is (x, y)."""
    X_, Y_ = M.centres(G)
    c, r = np.nonzero(X_[0] == F(x))[0], np.nonzero(Y_[:, 0] == F(y))[0]
    assert c.size == 1 and r.size == 1, (x, y)
    return int(r[0]), int(c[0])


# ---- invariants on random worlds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,G,vis", [(0, 16, 1.0), (3, 30, 3.0), (8, 64, 3.0), (8, 33, 100.0)])
def test_layer_invariants_and_rewards(K, G, vis):
    """Within an episode the layer only grows; seen cells are unoccupied cells; seen_cells is the layer's sum after every step; the
    first reveal earns nothing (an episode's `new`s add up to what was seen after the first reveal); every reward is the formula,
    bit for bit, from the recorded `new`; a STOP and a refused forward see nothing new."""
    rng = np.random.RandomState(K + G)
    e = fresh(seed=5, num_obstacles=K, coverage_resolution=G, visibility_dist=vis, turn_angle=30, max_episode_steps=25)
    Xc, Yc = M.centres(G)
    rc = F(0.1 * float(M.cell_size(G)) ** 2)
    assert e.rc == rc and e.rc.dtype == np.float32
    stops = refused = ends = 0
    for _ in range(6):
        free = ~M.occupied(Xc, Yc, X.view(e).rects)
        assert e.free_cells == int(free.sum()) > 0 and e.seen_cells == int(e.layer.sum()) > 0 and e.steps == 0
        assert (e.sx, e.sy, e.h0) == (e.px, e.py, e.h) and set(np.unique(e.layer)) <= {0, 1}
        first, news = e.seen_cells, 0
        while True:
            before, pose, collisions = e.layer.copy(), (e.px, e.py, e.h), e.collisions
            a = int(rng.randint(0, 4)) if rng.rand() < 0.9 else X.MOVE_FORWARD
            seen_before = e.seen_cells
            _, r, done, info = e.step(a)
            new = e.last_new
            assert r == F(F(-0.01) + F(rc * F(new))) and r.dtype == np.float32
            news += new
            if a == X.STOP or (a == X.MOVE_FORWARD and (done or e.collisions == collisions + 1)):
                if not done and a == X.MOVE_FORWARD:
                    assert (e.px, e.py, e.h) == pose and new == 0
                    refused += 1
                if a == X.STOP:
                    assert new == 0 and done
                    stops += 1
            if done:
                assert info["coverage"] == float(F(F(seen_before + new) / F(int(free.sum()))))
                assert news == seen_before + new - first
                ends += 1
                break
            assert np.all(e.layer >= before) and not np.any(e.layer[~free]) and e.seen_cells == int(e.layer.sum()) == seen_before + new
            assert new == int(e.layer.sum()) - int(before.sum())
    assert stops > 0 and ends == 6


# ---- hand-made worlds -------------------------------------------------------------------------------------------------------------------
def placed(G, vis, rects, px, py, h, turn=10):
    e = X.Nav2DExploreEnv(1, 0, num_obstacles=0, coverage_resolution=G, visibility_dist=vis, turn_angle=turn, max_episode_steps=1000)
    e.reset()
    e.place(rects, px, py, h)
    return e


def test_a_thin_wall_hides_the_cells_behind_it():
    """G = 16 (cells of 0.5 m), the agent at (2, 4) facing east, a wall 0.1 m thick from y = 2 to 6 at x = 3: the cell before the
    wall is seen, the cells right behind it are not, and all of them are without the wall."""
    wall = [(3.0, 2.0, 3.1, 6.0)]
    e, bare = placed(16, 5.0, wall, 2.0, 4.0, 0), placed(16, 5.0, [], 2.0, 4.0, 0)
    assert e.free_cells == bare.free_cells == 256   # no centre lies inside the wall
    assert e.layer[cell_of(16, 2.75, 4.25)] == 1 and bare.layer[cell_of(16, 2.75, 4.25)] == 1
    for x in (3.25, 3.75, 4.25):
        for y in (3.75, 4.25):
            assert e.layer[cell_of(16, x, y)] == 0 and bare.layer[cell_of(16, x, y)] == 1, (x, y)
    assert e.seen_cells < bare.seen_cells
    # a shorter wall, from y = 2 to 4.1: the segment to (3.25, 4.25) passes x = 3 .. 3.1 above it, the one to (3.25, 3.75) does not
    short = placed(16, 5.0, [(3.0, 2.0, 3.1, 4.1)], 2.0, 4.0, 0)
    assert short.layer[cell_of(16, 3.25, 4.25)] == 1 and short.layer[cell_of(16, 3.25, 3.75)] == 0


def test_the_wedge_edge_is_seen():
    """Heading 0 has the direction (1, 0) exactly, so dot = dx and cross = dy: the centre at dx = dy = 1 (|cross| == dot) is seen, on
    both edges, and the next centre outside is not."""
    e = placed(16, 5.0, [], 2.25, 2.25, 0)
    assert tuple(e.dirs[0]) == (1.0, 0.0)
    assert e.layer[cell_of(16, 3.25, 3.25)] == 1 and e.layer[cell_of(16, 3.25, 1.25)] == 1
    assert e.layer[cell_of(16, 3.25, 3.75)] == 0 and e.layer[cell_of(16, 3.25, 0.75)] == 0
    assert e.layer[cell_of(16, 1.25, 2.25)] == 0   # behind, farther than 0.25 m


def test_the_visibility_radius_is_inclusive():
    """The centre at dx = 2, dy = 0 has d2 = 4: seen with vis = 2 (d2 == vis * vis), not seen with the float32 below 2, whose
    square rounds below 4."""
    r, c = cell_of(16, 4.25, 2.25)
    assert placed(16, 2.0, [], 2.25, 2.25, 0).layer[r, c] == 1
    below = np.nextafter(F(2.0), F(0.0))
    assert F(below * below) < F(4.0)
    e = placed(16, float(below), [], 2.25, 2.25, 0)
    assert e.vis == float(below) and e.layer[r, c] == 0 and e.layer[cell_of(16, 3.75, 2.25)] == 1


def test_a_centre_behind_the_agent_within_a_quarter_metre_is_seen():
    """G = 64 (cells of 0.125 m), the agent on a centre facing east: the centres 0.125 m and 0.25 m behind it are seen (d2 <= 0.25 *
    0.25, the second one with equality), the one 0.375 m behind is not."""
    p = 2.0625
    e = placed(64, 3.0, [], p, p, 0)
    assert e.layer[cell_of(64, p - 0.125, p)] == 1 and e.layer[cell_of(64, p - 0.25, p)] == 1 and e.layer[cell_of(64, p - 0.375, p)] == 0
    assert e.layer[cell_of(64, p - 0.125, p + 0.125)] == 1 and e.layer[cell_of(64, p, p)] == 1


@pytest.mark.parametrize("turn", [10, 30])
def test_a_full_turn_reveals_exactly_the_disc(turn):
    """K = 0: after a full turn in place the layer is exactly the centres with d2 <= vis * vis, and every step's reward is its `new`."""
    G, vis = 30, 2.0
    e = placed(G, vis, [], 3.3, 4.1, 0, turn=turn)
    Xc, Yc = M.centres(G)
    dx, dy = Xc - F(3.3), Yc - F(4.1)
    disc = (dx * dx + dy * dy <= F(F(vis) * F(vis))).astype(np.uint8)
    assert e.seen_cells < int(disc.sum())
    total = e.seen_cells
    for _ in range(360 // turn):
        _, r, done, _ = e.step(X.TURN_LEFT)
        total += e.last_new
        assert not done and r == F(F(-0.01) + F(e.rc * F(e.last_new)))
    assert np.array_equal(e.layer, disc) and e.seen_cells == total == int(disc.sum()) and e.h == 0
    assert e.step(X.TURN_RIGHT)[1] == F(-0.01) and e.last_new == 0


# ---- ends, measures, sensors ------------------------------------------------------------------------------------------------------------
def test_ends_and_measures():
    """STOP and the step limit both end an episode, without a bonus; the four measures are the definitions; the sums add them up; the
    observation after an end is the next episode's first."""
    e = fresh(seed=2, num_obstacles=3, coverage_resolution=30, max_episode_steps=5, turn_angle=30)
    cell = M.cell_size(30)
    sums = {k: F(0.0) for k in X.MEASURES}
    for script in ([X.MOVE_FORWARD, X.TURN_LEFT, X.STOP], [X.MOVE_FORWARD] * 5, [X.TURN_RIGHT, X.MOVE_FORWARD, X.TURN_RIGHT, X.MOVE_FORWARD,
                                                                                X.TURN_LEFT]):
        episode, free = e.episode, e.free_cells
        for i, a in enumerate(script):
            seen = e.seen_cells
            o, r, done, info = e.step(a)
            assert done == (i + 1 == len(script)) and r == F(F(-0.01) + F(e.rc * F(e.last_new)))
        seen += e.last_new
        assert info == dict(coverage=float(F(F(seen) / F(free))), area_seen=float(F(F(cell * cell) * F(seen))),
                            collisions=info["collisions"], num_steps=float(len(script)))
        assert info["collisions"] == float(int(info["collisions"])) and 0 <= info["collisions"] <= len(script)
        assert e.episode == episode + 1 and e.steps == 0 and e.ended == 1
        assert o["gps"].tolist() == [0.0, 0.0] and o["compass"].tolist() == [0.0]
        for k in X.MEASURES:
            sums[k] = F(sums[k] + F(info[k]))
        assert e.sums == sums and e.last_measures == [F(info[k]) for k in X.MEASURES]
    rec = e.record()
    assert rec.shape == (X.STATE_WORDS,) and rec[11] == 1 and rec[X.W_FREE_CELLS] == e.free_cells and rec[X.W_SEEN_CELLS] == e.seen_cells
    assert rec[2:6].tolist() == [0, 0, 0, 0]   # no goal, no distance


def test_collisions_are_counted():
    e = placed(16, 1.0, [], 0.2, 4.0, 18)   # facing west at the wall
    _, r, done, _ = e.step(X.MOVE_FORWARD)
    assert e.collisions == 1 and (e.px, e.py) == (F(0.2), F(4.0)) and e.last_new == 0 and r == F(-0.01) and not done


@pytest.mark.parametrize("turn", [10, 30])
def test_gps_and_compass_are_the_object_task_s(turn):
    """gps = (dot, cross) of position - start in the start heading's frame, compass = the host table's row (h - h0) mod nh: Nav2DObj-v0's
    expressions, evaluated here on their own."""
    nh = 360 // turn
    tab = O.compass_table(turn)
    e = fresh(seed=7, num_obstacles=0, turn_angle=turn, max_episode_steps=10 * nh)
    rng = np.random.RandomState(turn)
    for _ in range(4 * nh):
        o = e.step(int(rng.randint(1, 4)))[0]
        c, s = e.dirs[e.h0]
        dx, dy = F(e.px - e.sx), F(e.py - e.sy)
        assert o["gps"].tolist() == [F(F(dx * c) + F(dy * s)), F(F(c * dy) - F(s * dx))] and o["gps"].dtype == np.float32
        assert o["compass"].tolist() == [tab[(e.h - e.h0) % nh]] and set(o) == {"gps", "compass"}
    assert (e.px, e.py) != (e.sx, e.sy)


def test_images_have_no_marker():
    """rgb and depth are Nav2DObj-v0's render without objects: Nav2D-v0's depth, and an rgb in which no goal cylinder stands, not even
    the one Nav2D-v0 would draw at the record's (0, 0)."""
    e = X.Nav2DExploreEnv(1, 0, H=12, W=20, num_obstacles=3, turn_angle=30, use_rgb=True)
    o = e.reset()
    e.place([], 0.3, 0.3, 7)    # looking into the corner at (0, 0)
    o = e.observe()
    with_marker = R.render(e.px, e.py, F(0.0), F(0.0), e.h, [], [], e.ray, e.cosf, e.tanv)
    assert np.array_equal(o["depth"], with_marker["depth"]) and not np.array_equal(o["rgb"], with_marker["rgb"])
    assert not np.any(np.all(o["rgb"] == np.array([255, 32, 32], np.uint8), -1)) and o["rgb"].shape == (12, 20, 3)
    plain = X.Nav2DExploreEnv(1, 0, H=0, W=0)
    assert set(plain.reset()) == {"gps", "compass"}


# ---- the scripted sequences --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.SCRIPT_CASES)
def test_scripts_show_every_event(case):
    """The three scripts of a case together: a STOP end, a step-limit end, a collision, a step that saw something new, a step that saw
    nothing new and a rollover whose first reveal differs from the previous episode's."""
    total = collections.Counter()
    for kind in X.SCRIPTS:
        out = X.script_rollout(kind, case, False)
        total.update(out["counters"])
        assert out["records"][0].shape == (X.SCRIPT_ENVS, X.STATE_WORDS) and len(out["layers"]) == X.SCRIPT_STEPS + 1
        rc = out["envs"][0].rc
        assert np.array_equal(out["rewards"], (F(-0.01) + (rc * out["news"].astype(np.float32)).astype(np.float32)).astype(np.float32))
    for k in X.SCRIPT_EVENTS:
        assert total[k] >= 1, (k, dict(total))


def test_script_forms_cover_every_shape():
    forms = {X.script_form(kind, case) for case in X.SCRIPT_CASES for kind in X.SCRIPTS}
    assert forms == set(X.FORMS) and len(X.FORMS) == 12
    assert {f[0] for f in forms} == {16, 30, 64} and {f[1] for f in forms} == {1.0, 3.0} and {f[2] for f in forms} == {(12, 20), (9, 18)}


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
BAD = [(dict(coverage_resolution=15), "coverage_resolution"), (dict(coverage_resolution=513), "coverage_resolution"),
       (dict(coverage_resolution=64.0), "coverage_resolution"), (dict(coverage_resolution=True), "coverage_resolution"),
       (dict(visibility_dist=0.0), "visibility_dist"), (dict(visibility_dist=-1.0), "visibility_dist"),
       (dict(visibility_dist=float("inf")), "visibility_dist"), (dict(visibility_dist=float("nan")), "visibility_dist"),
       (dict(visibility_dist=1e39), "visibility_dist"), (dict(visibility_dist="far"), "visibility_dist"),
       (dict(coverage_reward=-0.1), "coverage_reward"), (dict(coverage_reward=float("inf")), "coverage_reward"),
       (dict(coverage_reward=float("nan")), "coverage_reward"), (dict(coverage_reward=None), "coverage_reward"),
       (dict(num_actions=6), "Discrete"), (dict(num_actions=1), "Discrete"), (dict(distance="geodesic"), "geodesic"),
       (dict(distance="manhattan"), "distance")]


@pytest.mark.parametrize("kw,word", BAD)
def test_refusals_name_the_task_and_the_parameter(kw, word):
    """Every parameter out of range is refused by name, before the device is touched, and by the restatement alike."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    with pytest.raises(_lib.HabError, match=word) as err:
        EF.Nav2DExploreVectorEnv(2, 8, 8, device="cpu", **kw)
    assert "Nav2DExplore:" in str(err.value)
    if "distance" not in kw:
        with pytest.raises(ValueError):
            X.Nav2DExploreEnv(1, 0, **kw)


def test_other_refusals():
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    for kw in (dict(turn_angle=7), dict(num_obstacles=9), dict(max_episode_steps=0), dict(top_down_map="yes")):
        with pytest.raises(_lib.HabError):
            EF.Nav2DExploreVectorEnv(2, 8, 8, device="cpu", **kw)
    for size in ((0, 8), (8, 0)):
        with pytest.raises(_lib.HabError, match="Nav2DExplore.*image size"):
            EF.Nav2DExploreVectorEnv(2, *size, device="cpu")
    for kw in (dict(), dict(coverage_resolution=16, visibility_dist=0.5, coverage_reward=0), dict(coverage_resolution=512, use_depth=False)):
        with pytest.raises(_lib.HabError, match="Nav2DExplore.*GPU"):   # valid parameters: only the missing device is refused
            EF.Nav2DExploreVectorEnv(2, 8, 8, device="cpu", **kw)
    env = EF.Nav2DExploreVectorEnv.__new__(EF.Nav2DExploreVectorEnv)
    env.num_envs, env._pending, env._actions_host, env.distance = 3, set(), np.zeros(3, np.int64), "euclidean"
    env.async_step_at(0, 3)
    env.async_step_at(2, {"action": np.array([1])})
    assert env._pending == {0, 2} and env._actions_host.tolist() == [3, 0, 1]
    for a in (4, -1, 0.5, [1, 2]):
        with pytest.raises(_lib.HabError):
            env.async_step_at(1, a)
    for call in (lambda: env.reset_into(None, None, None), lambda: env.step_into(None, None, None, None, None),
                 lambda: env.step_into_obs({}, None, None), lambda: env.pause_at(0), env.follower_actions, env.expert_actions):
        with pytest.raises(_lib.HabError, match="Nav2DExplore|Nav2D:"):
            call()
    for call in (env.follower_actions, env.expert_actions, lambda: env.reset_into(None, None, None)):
        with pytest.raises(_lib.HabError, match="Nav2DExplore:"):
            call()
    assert EF.Nav2DExploreVectorEnv._follow_entry is None and EF.Nav2DExploreVectorEnv._expert_method is None
    assert not hasattr(EF.Nav2DExploreVectorEnv, "oracle_actions")


def test_parameters_and_the_cell_reward():
    from habitat_amd.common import env_factory as EF
    for G, vis, cr in ((64, 3.0, 0.1), (16, 1, 1), (30, np.float32(0.3), 0), (512, 2.5, 7.25)):
        g, v, rc = EF.nav2d_explore_parameters(G, vis, cr)
        assert (g, v) == (G, float(F(vis))) and F(rc) == rc == float(X.reward_per_cell(cr, G))
        assert F(rc) == F(float(cr) * float(F(8.0) / F(G)) ** 2)
    assert EF.NAV2D_EXPLORE_MEASURES == X.MEASURES and EF.Nav2DExploreVectorEnv.measure_names == X.MEASURES
    assert (EF.NAV2D_EXPLORE_MIN_RESOLUTION, EF.NAV2D_EXPLORE_MAX_RESOLUTION) == (X.MIN_RESOLUTION, X.MAX_RESOLUTION)


def test_factory_choice_and_config(monkeypatch):
    """habitat.task.type picks the env: a type starting with 'nav2dexplore' (any case) the new one -- the prefix is tested before
    'nav2d' -- while the sibling tasks keep their classes.  The YAML: PointNavResNetPolicy, resnet18, depth 64 x 64 with gps and
    compass, Discrete(4), episodes of 200 steps.  The constructors are replaced by recorders: the envs themselves need a GPU."""
    from habitat_amd.common import env_factory as EF
    from habitat_amd.config.default import get_config
    from habitat_amd.rl.ppo.ppo_trainer import PPOTrainer
    assert "Nav2DExplore-v0" in PPOTrainer.supported_tasks
    name = "exploration/ddppo_nav2d_explore.yaml"
    cfg = get_config(name)
    hab, hb = cfg.habitat, cfg.habitat_baselines
    assert hab.task.type == "Nav2DExplore-v0" and list(hab.task.actions) == ["stop", "move_forward", "turn_left", "turn_right"]
    assert list(hab.task.lab_sensors) == ["gps", "compass"] and hab.environment.max_episode_steps == 200
    assert hab.simulator.sensors.depth.height == hab.simulator.sensors.depth.width == 64
    assert hb.rl.ddppo.backbone == "resnet18" and hb.rl.policy.main_agent.name == "PointNavResNetPolicy"
    assert (hab.synthetic.coverage_resolution, hab.synthetic.visibility_dist, hab.synthetic.coverage_reward) == (64, 3.0, 0.1)
    made = []
    classes = ("Nav2DExploreVectorEnv", "Nav2DSocialVectorEnv", "Nav2DRearrVelVectorEnv", "Nav2DRearrVectorEnv", "Nav2DObjVectorEnv",
               "Nav2DVelVectorEnv", "Nav2DVectorEnv", "SyntheticVectorEnv")
    for cls in classes:
        monkeypatch.setattr(EF, cls, lambda *a, _n=cls, **kw: made.append((_n, a, kw)) or _n)
    factory = EF.instantiate(hb.vector_env_factory)
    assert factory.construct_envs(cfg, device="cpu") == "Nav2DExploreVectorEnv"
    _, args, kw = made[-1]
    assert args == (16, 64, 64) and kw["num_actions"] == 4 and kw["max_episode_steps"] == 200
    assert {k: kw[k] for k in ("num_obstacles", "turn_angle", "coverage_resolution", "visibility_dist", "coverage_reward", "use_rgb",
                               "use_depth", "distance")} == dict(num_obstacles=3, turn_angle=10, coverage_resolution=64, visibility_dist=3.0,
                                                                 coverage_reward=0.1, use_rgb=False, use_depth=True, distance="euclidean")
    assert "top_down_map" not in kw
    ov = ["habitat.synthetic.coverage_resolution=30", "habitat.synthetic.visibility_dist=1.5", "habitat.synthetic.coverage_reward=2",
          "habitat.task.measurements.top_down_map.map_resolution=30"]
    for task_type, want in (("nav2dexplore", "Nav2DExploreVectorEnv"), ("NAV2DEXPLORE-v1", "Nav2DExploreVectorEnv"),
                            ("Nav2DExplorer", "Nav2DExploreVectorEnv"), ("Nav2DExp-v0", "Nav2DVectorEnv"), ("Nav2D-v0", "Nav2DVectorEnv")):
        assert factory.construct_envs(get_config(name, ov + [f"habitat.task.type={task_type}"]), device="cpu") == want, task_type
        _, _, kw = made[-1]
        assert kw["top_down_map"] == dict(map_resolution=30)
        if want == "Nav2DExploreVectorEnv":
            assert (kw["coverage_resolution"], kw["visibility_dist"], kw["coverage_reward"]) == (30, 1.5, 2)
        else:
            assert "coverage_resolution" not in kw
    for yaml, want in (("pointnav/ppo_nav2d.yaml", "Nav2DVectorEnv"), ("pointnav/ppo_nav2d_vel.yaml", "Nav2DVelVectorEnv"),
                       ("objectnav/ddppo_nav2d_objectnav.yaml", "Nav2DObjVectorEnv"), ("rearrange/ddppo_nav2d_rearrange.yaml", "Nav2DRearrVectorEnv"),
                       ("social_nav/ddppo_nav2d_social.yaml", "Nav2DSocialVectorEnv")):
        assert EF.SyntheticVectorEnvFactory().construct_envs(get_config(yaml), device="cpu") == want
    # with the colour image: an rgb entry and the factory's switch
    c = get_config(name, ["habitat.simulator.sensors.rgb.height=40", "habitat.simulator.sensors.rgb.width=44",
                          "habitat_baselines.vector_env_factory.use_rgb=true"])
    assert EF.instantiate(c.habitat_baselines.vector_env_factory).construct_envs(c, device="cpu") == "Nav2DExploreVectorEnv"
    assert made[-1][1][1:] == (40, 44) and made[-1][2]["use_rgb"] is True


def test_observation_space():
    """depth, gps, compass in this order, rgb first where it is asked for, and no goal input of any kind; the spaces are built before
    the constructor asks for the device, which is what is missing here."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    from habitat_amd.rl.ppo.policy import resolve_sensors
    for use in ((False, True), (True, True), (False, False)):
        env = EF.Nav2DExploreVectorEnv.__new__(EF.Nav2DExploreVectorEnv)
        with pytest.raises(_lib.HabError, match="GPU"):
            env.__init__(3, 10, 12, device="cpu", use_rgb=use[0], use_depth=use[1], turn_angle=30)
        sp = env.observation_spaces[0].spaces
        assert list(sp) == (["rgb"] if use[0] else []) + (["depth"] if use[1] else []) + ["gps", "compass"]
        assert sp["gps"].shape == (2,) and sp["compass"].shape == (1,) and sp["gps"].dtype == sp["compass"].dtype == np.float32
        assert (env.H, env.W) == ((10, 12) if any(use) else (0, 0)) and env.action_spaces[0].n == 4
        if use[1]:
            assert sp["depth"].shape == (10, 12, 1)
        visual, fused = resolve_sensors(env.observation_spaces[0])
        assert [v[0] for v in visual] == [k for k in ("rgb", "depth") if k in sp] and fused == []   # gps, compass: their own embeddings
    assert EF.Nav2DExploreVectorEnv.consumes_actions and np.array_equal(EF.nav2d_compass_table(30), O.compass_table(30))


def test_header_binding_and_tables_agree():
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    src = open(os.path.join(ROOT, "include", "habitat_amd.h")).read()
    d = {k: int(v, 0) for k, v in re.findall(r"#define (HAB_NAV2D_(?:EXPLORE|MAP_TASK)_[A-Z0-9_]+) (-?(?:0x)?[0-9A-Fa-f]+)\b", src)}
    L = _lib.lib()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("hab_nav2d_explore_state_bytes", "hab_nav2d_explore_step"):
        decl = re.search(name + r"\((.*?)\);", plain, flags=re.S).group(1)
        count = 0 if decl.strip() == "void" else decl.count(",") + 1
        assert count == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name)
    # hab_nav2d_obj_step's arguments without semantic, objectgoal, num_objects, num_categories and num_actions, plus the layer, G,
    # visibility_dist and rc
    obj, exp = _lib.SIGNATURES["hab_nav2d_obj_step"][1], _lib.SIGNATURES["hab_nav2d_explore_step"][1]
    assert len(exp) == len(obj) - 5 + 4 == 29 and exp.count(_lib.c_float) == 2 and exp[-1] is _lib.vp
    assert L.hab_nav2d_explore_state_bytes() == d["HAB_NAV2D_EXPLORE_STATE_BYTES"] == 4 * X.STATE_WORDS == L.hab_nav2d_state_bytes() + 24
    names = ("START_X", "START_Y", "START_HEADING", "FREE_CELLS", "SEEN_CELLS", "LAST_NEW")
    assert [d[f"HAB_NAV2D_EXPLORE_W_{k}"] for k in names] == [X.W_START_X, X.W_START_Y, X.W_START_HEADING, X.W_FREE_CELLS, X.W_SEEN_CELLS,
                                                            X.W_LAST_NEW] == list(range(56, 62))
    assert (d["HAB_NAV2D_EXPLORE_MIN_RESOLUTION"], d["HAB_NAV2D_EXPLORE_MAX_RESOLUTION"]) == (X.MIN_RESOLUTION, X.MAX_RESOLUTION) == (
        M.MIN_RESOLUTION, M.MAX_RESOLUTION)
    assert d["HAB_NAV2D_MAP_TASK_EXPLORE"] == X.TASK_EXPLORE == EF.NAV2D_MAP_TASK_EXPLORE == EF.Nav2DExploreVectorEnv._map_task == 4
    assert X.TASK_EXPLORE not in (M.TASK_GOAL, M.TASK_OBJ, M.TASK_REARR, M.TASK_SOCIAL)


def test_the_map_of_the_task_has_no_marker():
    """The top-down map through tests/nav2d_map_reference.py on this task's view: occupied and free cells, the start and the
    trajectory, no target and no object; its fog of war at the layer's resolution and visibility is the coverage layer."""
    envs = [fresh(seed=4, env=n, num_obstacles=8, coverage_resolution=40, visibility_dist=2.5, max_episode_steps=6) for n in range(3)]
    maps = X.MapOf(envs, 40, 2.5)
    maps.begin()
    rng = np.random.RandomState(1)
    for _ in range(15):
        dones = [e.step(int(rng.randint(0, 4)))[2] for e in envs]
        maps.after_step(dones)
        assert np.array_equal(maps.fog, np.stack([e.layer for e in envs]))
        assert set(np.unique(maps.map)) <= {M.OCCUPIED, M.FREE, M.START, M.TRAJECTORY}
    fr = maps.frames(24, None, False, False)
    assert fr.shape == (3, 24, 24, 3) and np.any(np.all(fr == M.COLORS[M.AGENT], -1))
