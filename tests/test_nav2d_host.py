"""CPU: properties of the Nav2D-v0 task on its numpy restatement (tests/nav2d_reference.py), and the event coverage of the scripted
action sequences that tests/test_gpu_nav2d.py replays on the device."""
import math

import numpy as np
import pytest

import nav2d_reference as R


@pytest.mark.parametrize("K", [0, 3, 8])
def test_agent_stays_in_free_space(K):
    """2000 random steps (no STOP bias: all four actions) per K: after every step the agent is inside [0.1, 7.9]^2 and outside every
    rectangle grown by the agent radius."""
    env = R.Nav2DEnv(7, 0, num_obstacles=K, max_episode_steps=100, use_rgb=False, use_depth=False)
    env.reset()
    rng = np.random.RandomState(K)
    moved = 0
    for _ in range(2000):
        before = (env.px, env.py)
        env.step(rng.choice([1, 1, 1, 2, 3, 0], p=[0.3, 0.2, 0.2, 0.14, 0.14, 0.02]))
        moved += (env.px, env.py) != before
        assert R.LO <= env.px <= R.HI and R.LO <= env.py <= R.HI
        for x0, y0, x1, y1 in env.world.rects:
            assert not (x0 - R.RADIUS < env.px < x1 + R.RADIUS and y0 - R.RADIUS < env.py < y1 + R.RADIUS)
        assert len(env.world.rects) == K
    assert moved > 200 and env.counters["episodes"] > 5
    if K:
        assert env.counters["obstacle_collisions"] + env.counters["wall_collisions"] > 0


def test_rewards_telescope():
    """Per episode, in float64: sum r = d_start - d_end - 0.01 * len + 2.5 * success.  Bound: a step's reward is three float32
    roundings, of d_prev - d (|.| <= 0.25 + rounding, so error <= ulp(0.25) / 2 = 2^-26 ... taken as 2^-25), of -0.01 + that
    (|.| < 0.5: <= 2^-26) and of the sum with the bonus (|.| < 4: <= 2^-23); -0.01 itself is off by < 2^-31 as a float32.  The
    distances cancel exactly in the telescoped sum because each d is the same float32 in both of its terms.  So
    |sum r - closed form| <= len * (2^-25 + 2^-26 + 2^-31) + 2^-23 for the one step that carries the bonus."""
    for K, script in ((0, "greedy"), (8, "greedy"), (3, "random")):
        env = R.Nav2DEnv(11, 1, num_obstacles=K, turn_angle=30, max_episode_steps=80, use_rgb=False, use_depth=False)
        env.reset()
        rng = np.random.RandomState(5)
        total, episodes, d0 = 0.0, 0, float(env.d_start)
        o = env.observe()
        for _ in range(1500):
            a = R.greedy_action(o["pointgoal_with_gps_compass"], 30) if script == "greedy" else rng.randint(0, 4)
            o, r, done, info = env.step(a)
            total += float(r)
            if done:
                L = env.last
                assert float(L["d_start"]) == d0
                closed = float(L["d_start"]) - float(L["d_end"]) - 0.01 * L["length"] + 2.5 * L["success"]
                bound = L["length"] * (2.0 ** -25 + 2.0 ** -26 + 2.0 ** -31) + 2.0 ** -23
                assert abs(total - closed) <= bound, (total, closed, bound)
                assert info["success"] == float(L["success"]) and info["distance_to_goal"] == float(L["d_end"])
                if L["success"]:
                    assert 0.0 < info["spl"] <= 1.0
                else:
                    assert info["spl"] == 0.0
                total, episodes, d0 = 0.0, episodes + 1, float(env.d_start)
        assert episodes >= 10


def test_fallback_corners():
    """The fallback start (0.5, 0.5) / goal (7.5, 7.5) is reached with K = 8 and a PATCHED candidate count of 1 (one rejection
    suffices); with the task's 16 candidates no seed within reach of a CPU search rejects them all.  The corners are free for every
    world because rectangles stay inside [1, 7]^2."""
    starts = goals = 0
    for env in range(200):
        w = R.make_world(3, env, 0, 8, 36, candidates=1)
        assert R.is_free(w.sx, w.sy, w.rects) and R.is_free(w.gx, w.gy, w.rects)
        if w.start_fallback:
            assert (w.sx, w.sy) == (R.F(0.5), R.F(0.5))
            starts += 1
        if w.goal_fallback:
            assert (w.gx, w.gy) == (R.F(7.5), R.F(7.5))
            goals += 1
        else:
            assert R.dist(w.sx, w.sy, w.gx, w.gy) >= 1.0
        full = R.make_world(3, env, 0, 8, 36)
        assert not full.start_fallback and not full.goal_fallback
    assert starts > 10 and goals > 10


@pytest.mark.parametrize("K,turn", R.SCRIPT_CASES)
def test_scripted_sequences_cover_their_events(K, turn):
    kw = dict(turn_angle=turn, num_obstacles=K, max_episode_steps=R.SCRIPT_MAX_EPISODE_STEPS, use_rgb=False, use_depth=False)
    c = {k: R.rollout(k, R.script_seed(k, K), R.SCRIPT_ENVS, R.SCRIPT_STEPS, **kw)["counters"] for k in R.SCRIPTS}
    assert c["forward"]["wall_collisions"] > 0 and c["forward"]["timeouts"] == c["forward"]["episodes"] > 0
    assert c["greedy"]["successes"] > 0
    if K == 8:
        assert c["greedy"]["obstacle_collisions"] > 0
    assert c["never_stop"]["timeouts"] == c["never_stop"]["episodes"] >= R.SCRIPT_ENVS * (R.SCRIPT_STEPS // R.SCRIPT_MAX_EPISODE_STEPS)
    assert c["random"]["episodes"] > c["random"]["timeouts"]  # STOP ends episodes too


def test_greedy_succeeds_without_obstacles():
    """With K = 0 and room to finish, the greedy controller succeeds in every episode and its SPL is close to 1."""
    r = R.rollout("greedy", 4, 3, 400, turn_angle=10, num_obstacles=0, max_episode_steps=200, use_rgb=False, use_depth=False)
    infos = [i for row in r["infos"] for i in row if i]
    assert len(infos) >= 6 and all(i["success"] == 1.0 and i["spl"] > 0.9 and i["collisions"] == 0.0 for i in infos)


def test_table_shapes_and_frames():
    assert R.heading_table(10).shape == (36, 2) and R.heading_table(30).shape == (12, 2)
    ray, cosf, tanv = R.ray_tables(30, 9, 18)
    assert ray.shape == (12, 18, 2) and cosf.shape == (18,) and tanv.shape == (9,)
    assert all(a.dtype == np.float32 for a in (ray, cosf, tanv, R.heading_table(10)))
    assert tanv[4] == 0.0 and tanv[0] > 0 > tanv[-1]                       # odd H: the middle row looks at the horizon
    d = R.heading_table(30)
    # column 0 is to the LEFT of the optical axis (positive cross product with the heading), the last column to the right
    assert d[0, 0] * ray[0, 0, 1] - d[0, 1] * ray[0, 0, 0] > 0 > d[0, 0] * ray[0, -1, 1] - d[0, 1] * ray[0, -1, 0]
    assert np.allclose(np.hypot(ray[..., 0], ray[..., 1]), 1.0, atol=1e-6)
    # TURN_LEFT raises phi's complement: a goal straight ahead moves to the right (phi < 0) after a left turn
    env = R.Nav2DEnv(1, 0, num_obstacles=0, turn_angle=30, use_rgb=False, use_depth=False)
    env.reset()
    phi0 = env.observe()["pointgoal_with_gps_compass"][1]
    phi1 = env.step(R.TURN_LEFT)[0]["pointgoal_with_gps_compass"][1]
    assert math.isclose(((phi0 - phi1) + math.pi) % (2 * math.pi) - math.pi, math.radians(30), abs_tol=1e-5)


def test_render_is_consistent():
    """depth in [0, 1]; the goal marker changes rgb only; floor and ceiling rows take their constants' shades."""
    env = R.Nav2DEnv(2, 0, H=12, W=20, num_obstacles=3, turn_angle=10)
    o = env.reset()
    assert o["depth"].shape == (12, 20, 1) and o["depth"].dtype == np.float32 and o["rgb"].shape == (12, 20, 3) and o["rgb"].dtype == np.uint8
    assert o["depth"].min() > 0.0 and o["depth"].max() <= 1.0
    seen = 0
    for _ in range(36):
        o = env.step(R.TURN_LEFT)[0]
        w = env.world
        far = R.render(env.px, env.py, R.F(-50.0), R.F(-50.0), env.h, w.rects, w.colors, env.ray, env.cosf, env.tanv)
        assert np.array_equal(far["depth"], o["depth"])
        seen += not np.array_equal(far["rgb"], o["rgb"])
    assert 0 < seen < 36


def test_refusals():
    with pytest.raises(ValueError):
        R.Nav2DEnv(1, 0, turn_angle=7)
    with pytest.raises(ValueError):
        R.Nav2DEnv(1, 0, num_obstacles=9)
    env = R.Nav2DEnv(1, 0, use_rgb=False, use_depth=False)
    env.reset()
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            env.step(bad)
    from habitat_amd import _lib
    from habitat_amd.common.env_factory import Nav2DVectorEnv, nav2d_tables
    with pytest.raises(_lib.HabError):
        Nav2DVectorEnv(2, 8, 8, turn_angle=7, device="cpu")
    with pytest.raises(_lib.HabError):
        Nav2DVectorEnv(2, 8, 8, num_obstacles=9, device="cpu")
    with pytest.raises(_lib.HabError):
        Nav2DVectorEnv(2, 8, 8, num_actions=6, device="cpu")
    # the env's host tables are the restatement's, bit for bit
    for got, want in zip(nav2d_tables(30, 9, 18), (R.heading_table(30),) + R.ray_tables(30, 9, 18)):
        assert got.dtype == np.float32 and np.array_equal(got, want)


def test_factory_selects_the_task_only_by_its_type():
    from habitat_amd.config.default import get_config
    cfg = get_config("pointnav/ppo_nav2d.yaml")
    assert cfg.habitat.task.type == "Nav2D-v0" and len(cfg.habitat.task.actions) == 4
    assert cfg.habitat.simulator.sensors.rgb.height == cfg.habitat.simulator.sensors.depth.width == 64
    assert cfg.habitat.synthetic.num_obstacles == 3 and cfg.habitat.synthetic.turn_angle == 10
