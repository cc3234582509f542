"""GPU: the Nav2DImageNav-v0 kernels against the numpy restatement (tests/nav2d_imagenav_reference.py), bit for bit on every output --
rgb, depth, goal_rgb, gps, compass, reward, not-done, the whole record, the measure sums and, in the geodesic mode, the field record --
hand-made records written into the device state, what the task composes from Nav2D-v0 (the follower, the field build, the top-down
map, the frames), the entries' refusals, and the seams that carry the task: both trainers, DAgger and the evaluator."""
import functools
import math

import numpy as np
import pytest
import torch

import nav2d_follow_reference as FW
import nav2d_imagenav_reference as I
import nav2d_map_reference as M
from test_gpu_nav2d import make_trainer

pytestmark = pytest.mark.gpu
SENSORS = I.SENSORS
IMAGES = ("rgb", "depth", "goal_rgb")
F = np.float32


def make_env(N, H, W, seed, K=3, turn=10, sd=1.0, distance="euclidean", max_steps=12, **kw):
    from habitat_amd.common.env_factory import Nav2DImageNavVectorEnv
    return Nav2DImageNavVectorEnv(N, H, W, seed=seed, num_obstacles=K, turn_angle=turn, max_episode_steps=max_steps, success_distance=sd,
                                  distance=distance, device="cuda", **kw)


def stacked(ref, key):
    return np.stack([np.stack([o[key] for o in row]) for row in ref["obs"]])  # (T + 1, N, ...)


def empty_rows(T, N, H, W, want, offsets=None, dev="cuda"):
    """(T + 1, N, ...) rows like a rollout arena's.  `offsets` {key: bytes} places a uint8 image's rows that many bytes behind a
    16-byte aligned address, so that the colour sweep meets every alignment."""
    shapes = dict(rgb=((H, W, 3), torch.uint8, 7), depth=((H, W, 1), torch.float32, -1.0), goal_rgb=((H, W, 3), torch.uint8, 9),
                  gps=((2,), torch.float32, -9.0), compass=((1,), torch.float32, -9.0))
    rows = {}
    for k in want:
        shape, dtype, fill = shapes[k]
        off = (offsets or {}).get(k, 0)
        if off:
            count = (T + 1) * N * int(np.prod(shape))
            buf = torch.full((count + 32,), fill, dtype=dtype, device=dev)
            start = (-buf.data_ptr()) % 16 + off
            rows[k] = buf[start:start + count].view((T + 1, N) + shape)
            assert rows[k].data_ptr() % 16 == off
        else:
            rows[k] = torch.full((T + 1, N) + shape, fill, dtype=dtype, device=dev)
    return rows


def run_device(ref, env, want=SENSORS, masks=None, offsets=None):
    """Replays ref's actions on the device, every step written straight into its own row of separately allocated (T + 1, N, ...)
    tensors; the records (and the field records) are copied after the reset and after every step."""
    T, N = ref["actions"].shape
    dev = "cuda"
    rows = empty_rows(T, N, env.H, env.W, want, offsets)
    rew = torch.full((T, N), 99.0, device=dev)
    nd = torch.full((T, N), 5, dtype=torch.uint8, device=dev)
    sums = torch.zeros(T, 4, N, device=dev)
    states = torch.zeros(T + 1, N, I.STATE_WORDS, dtype=torch.int32, device=dev)
    fields = None if env._geo is None else torch.zeros((T + 1,) + tuple(env._geo.shape), dtype=torch.int32, device=dev)
    actions = torch.from_numpy(ref["actions"]).to(dev).unsqueeze(-1)       # (T, N, 1), the layout of the rollout's action rows
    env.reset_into_obs({k: v[0] for k, v in rows.items()})
    states[0].copy_(env._state)
    if fields is not None:
        fields[0].copy_(env._geo)
    for t in range(T):
        env.step_into_obs({k: v[t + 1] for k, v in rows.items()}, rew[t], nd[t], actions=actions[t],
                          mask=None if masks is None else masks[t])
        sums[t].copy_(env.measure_sums)
        states[t + 1].copy_(env._state)
        if fields is not None:
            fields[t + 1].copy_(env._geo)
    torch.cuda.synchronize()
    return ({k: v.cpu() for k, v in rows.items()}, rew.cpu(), nd.cpu(), sums.cpu(), states.cpu(),
            None if fields is None else fields.cpu())


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_matches(ref, rows, rew, nd, sums, states, fields):
    for k, v in rows.items():
        exp = torch.from_numpy(stacked(ref, k))
        assert v.dtype == exp.dtype and v.shape == exp.shape, k
        assert torch.equal(bits(v), bits(exp)), k
    assert torch.equal(bits(rew), bits(torch.from_numpy(ref["rewards"]))), "reward"
    assert torch.equal(nd, torch.from_numpy((~ref["dones"]).astype(np.uint8))), "not_done"
    assert torch.equal(bits(sums), bits(torch.from_numpy(ref["sums"]))), "measure sums"
    assert torch.equal(states, torch.from_numpy(np.stack(ref["records"]))), "records"
    assert (fields is None) == (ref["fields"] is None)
    if fields is not None:
        assert torch.equal(fields, torch.from_numpy(np.stack(ref["fields"]))), "field records"


def replay(ref, seed, K, turn, sd, distance, H, W, want=SENSORS, offsets=None, max_steps=12, **kw):
    env = make_env(ref["actions"].shape[1], H, W, seed, K=K, turn=turn, sd=sd, distance=distance, max_steps=max_steps, **kw)
    assert_matches(ref, *run_device(ref, env, want=want, offsets=offsets))
    return env


@pytest.mark.parametrize("kind", I.SCRIPTS)
@pytest.mark.parametrize("case", I.SCRIPT_CASES, ids=lambda c: "K{}-turn{}".format(*c))
def test_kernels_bitwise(case, kind):
    """Every step of a scripted sequence, 60 steps of 5 envs: every output is equal to the restatement's bit for bit.  The
    (success_distance, distance mode, image size) of a run go round I.FORMS, so both entries run at both success distances and both
    sizes; at 9 x 18 an image has 486 bytes, so successive envs' colour images start at two alignments and both the aligned groups
    and the edge pixels of the colour sweep run."""
    ref = I.script_rollout(kind, case)
    sd, distance, (H, W) = I.script_form(kind, case)
    assert ref["dones"].sum() >= (1 if kind == "greedy" else I.SCRIPT_ENVS * 4)
    replay(ref, I.SCRIPT_SEED, case[0], case[1], sd, distance, H, W, max_steps=I.script_limit(kind))


@pytest.mark.parametrize("distance", ["euclidean", "geodesic"])
@pytest.mark.parametrize("sd", I.SUCCESS_DISTANCES)
@pytest.mark.parametrize("size", I.SIZES, ids=lambda s: "{}x{}".format(*s))
def test_every_form_with_the_steering_script(distance, sd, size):
    """'greedy' (the script whose episodes succeed) at K = 8, turn 30 in every combination of entry, success distance and size."""
    case = (8, 30)
    ref = I.script_rollout("greedy", case, (sd, distance, size))
    assert ref["counters"]["successes"] >= 1
    replay(ref, I.SCRIPT_SEED, 8, 30, sd, distance, size[0], size[1], max_steps=I.script_limit("greedy"))


@functools.lru_cache(maxsize=None)
def small(N=5, T=30, H=9, W=18, K=8, turn=30, seed=2, kind="random", sd=1.0, distance="euclidean", use_depth=True):
    return I.rollout(kind, seed, N, T, distance=distance, turn_angle=turn, num_obstacles=K, success_distance=sd, max_episode_steps=12,
                     H=H, W=W, use_depth=use_depth)


@pytest.mark.parametrize("offsets", [(0, 0), (1, 3), (2, 1), (3, 2)], ids=lambda o: "rgb+{}-goal+{}".format(*o))
def test_render_with_several_row_tiles(offsets):
    """70 x 66 is two tiles of the render (63 and 7 rows) with W % 4 = 2, both views; the rgb and goal_rgb rows start 0..3 bytes behind
    an aligned address, so the three-dword groups and the edge pixels meet every alignment: 3 envs, 12 random steps, all bitwise."""
    ref = small(N=3, T=12, H=70, W=66, seed=5)
    replay(ref, 5, 8, 30, 1.0, "euclidean", 70, 66, offsets=dict(rgb=offsets[0], goal_rgb=offsets[1]))


@pytest.mark.parametrize("H", [5, 1])
def test_one_column(H):
    ref = small(N=3, T=12, H=H, W=1, seed=4, distance="geodesic")
    replay(ref, 4, 8, 30, 1.0, "geodesic", H, 1, offsets=dict(rgb=1, goal_rgb=2))


@pytest.mark.parametrize("distance", ["euclidean", "geodesic"])
@pytest.mark.parametrize("missing", IMAGES + ("gps", "compass", "images", "all"))
def test_missing_destinations(missing, distance):
    """Each destination NULL in turn, no image at all (nothing is rendered) and no observation destination at all: what is asked for
    is still exact, and so are reward, record and field."""
    want = tuple(k for k in SENSORS if not (k == missing or (missing == "images" and k in IMAGES) or missing == "all"))
    replay(small(distance=distance), 2, 8, 30, 1.0, distance, 9, 18, want=want)


def test_without_the_depth_sensor():
    ref = small(use_depth=False)
    env = replay(ref, 2, 8, 30, 1.0, "euclidean", 9, 18, want=("rgb", "goal_rgb", "gps", "compass"), use_depth=False)
    assert list(env.observation_spaces[0].spaces) == ["rgb", "goal_rgb", "gps", "compass"] and env._depth is None


@pytest.mark.parametrize("N", [1, 70])
def test_env_counts(N):
    distance = "geodesic" if N == 70 else "euclidean"
    ref = small(N=N, T=14, distance=distance)
    replay(ref, 2, 8, 30, 1.0, distance, 9, 18)


@pytest.mark.parametrize("distance", ["euclidean", "geodesic"])
def test_mask_leaves_unselected_envs_untouched(distance):
    """Steps 3..8 leave every third env unstepped while its neighbours' episodes end: its record, field, rows, reward and not-done
    byte keep what they held, and the stepped envs match a restatement that skips the same steps."""
    N, T = 7, 14
    envs = [I.make_env(3, n, distance, H=9, W=18, num_obstacles=3, turn_angle=30, max_episode_steps=4) for n in range(N)]
    env = make_env(N, 9, 18, 3, K=3, turn=30, distance=distance, max_steps=4)
    rows = env._own_obs()
    obs = [e.reset() for e in envs]
    env.reset_into_obs(rows)
    rng = np.random.RandomState(0)
    rew, nd = torch.full((N,), 42.0, device="cuda"), torch.full((N,), 9, dtype=torch.uint8, device="cuda")
    want_rew, want_nd = np.full(N, 42.0, np.float32), np.full(N, 9, np.uint8)
    for t in range(T):
        mask = np.ones(N, np.uint8)
        if 3 <= t < 9:
            mask[1::3] = 0
        a = rng.randint(0, 4, size=N)
        for n, e in enumerate(envs):
            if mask[n]:
                obs[n], r, done, _ = e.step(a[n])
                want_rew[n], want_nd[n] = r, 0 if done else 1
        env.step_into_obs(rows, rew, nd, actions=torch.from_numpy(a).cuda(), mask=torch.from_numpy(mask).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(env._state.cpu().numpy(), np.stack([e.record() for e in envs])), t
        if distance == "geodesic":
            assert np.array_equal(env._geo.cpu().numpy(), np.stack([e.field_record() for e in envs])), t
        assert np.array_equal(rew.cpu().numpy().view(np.int32), want_rew.view(np.int32)) and np.array_equal(nd.cpu().numpy(), want_nd)
        for k in SENSORS:
            assert np.array_equal(rows[k].cpu().numpy().reshape(N, -1), np.stack([o[k].reshape(-1) for o in obs])), (k, t)
        assert np.array_equal(env.measure_sums.cpu().numpy(), np.array([[e.sums[k] for e in envs] for k in I.MEASURES], np.float32))


# ---- hand-made records written into the device state ------------------------------------------------------------------------------
WALL = (5.0, 3.0, 6.0, 5.0)
HAND_MADE = {  # rects, start x, y, goal x, y, heading, goal heading (turn 10)
    "agent at the goal pose": ([WALL], 3.5, 4.0, 3.5, 4.0, 5, 5),
    "a rectangle at arm's length of the goal": ([WALL], 1.0, 1.0, 4.5, 4.0, 9, 0),
    "the goal in a corner, looking into it": ([], 4.0, 4.0, 0.1, 0.1, 0, 22),
    "the goal in a corner, looking out": ([WALL, (2.0, 5.5, 3.0, 6.5)], 4.0, 2.0, 7.9, 7.9, 3, 22),
}


@pytest.mark.parametrize("distance", ["euclidean", "geodesic"])
@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_records(name, distance):
    """A record the restatement began, written into the device state (and, in the geodesic mode, its field built by the build entry on
    this stride): a turn left, a turn back, a forward and a stop, with every row and the record the restatement's after each."""
    from habitat_amd import _lib
    from habitat_amd._lib import ptr, stream_ptr
    rects, sx, sy, gx, gy, h, gh = HAND_MADE[name]
    H, W = 12, 20
    e = I.make_env(1, 0, distance, H=H, W=W, num_obstacles=0, max_episode_steps=1000)
    e.reset()
    o = e.place(rects, sx, sy, gx, gy, h, gh)
    env = make_env(1, H, W, 1, K=len(rects), distance=distance, max_steps=1000)
    rows = env._own_obs()
    env.reset_into_obs(rows)
    env._state.copy_(torch.from_numpy(e.record()[None]))
    if distance == "geodesic":
        assert _lib.lib().hab_nav2d_geo_build(ptr(env._state), I.STATE_WORDS * 4, ptr(env._geo), None, 0, 1, len(rects), stream_ptr()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(env._geo.cpu().numpy()[0], e.field_record())
        assert np.array_equal(env._state.cpu().numpy()[0], e.record())       # d_start = d_prev = g0
    rew, nd = torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.uint8, device="cuda")
    for a in (I.TURN_LEFT, I.TURN_RIGHT, I.MOVE_FORWARD, I.STOP):
        o_prev = o
        o, r, done, _ = e.step(a)
        env.step_into_obs(rows, rew, nd, actions=torch.tensor([a], device="cuda"))
        torch.cuda.synchronize()
        got = {k: rows[k].cpu().numpy()[0] for k in SENSORS}
        if done:
            break   # the next world is the stream's, with K = 0 rectangles here and len(rects) there
        for k in SENSORS:
            assert np.array_equal(got[k].reshape(o[k].shape), o[k]), (k, a)
        assert np.array_equal(got["goal_rgb"], o_prev["goal_rgb"])           # constant within the episode
        assert np.array_equal(env._state.cpu().numpy()[0], e.record())
        assert rew.cpu().numpy().view(np.int32)[0] == np.array([r], np.float32).view(np.int32)[0] and int(nd[0]) == 1
        if name == "agent at the goal pose":
            same = np.array_equal(got["rgb"], got["goal_rgb"])
            assert same == (a == I.TURN_RIGHT)         # back at the goal pose: the two rows are equal bytewise
    assert done and a == I.STOP and int(nd[0]) == 0
    assert env._state.cpu().numpy()[0, 12:16].view(np.float32).tolist() == [float(v) for v in e.last_measures]
    if name == "a rectangle at arm's length of the goal":
        # the wall, 0.5 m ahead and 2 m wide, fills the 90 degree view at the one depth 0.05: its colour (64, 96, 128) times 0.95
        assert np.unique(o_prev["goal_rgb"].reshape(-1, 3), axis=0).tolist() == [[60, 91, 121]]


# ---- what the task composes from Nav2D-v0 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sd", [0.2, 1.0])
def test_follower_actions_and_a_driven_episode(sd):
    """follower_actions / expert_actions on this env equal tests/nav2d_follow_reference.py on the record, status and next distance
    included, and episodes driven by them end in success."""
    N, T = 6, 120
    envs = [I.make_env(5, n, "geodesic", H=2, W=2, num_obstacles=8, turn_angle=10, success_distance=sd, max_episode_steps=200)
            for n in range(N)]
    env = make_env(N, 2, 2, 5, K=8, turn=10, sd=sd, distance="geodesic", max_steps=200)
    for e in envs:
        e.reset()
    env.reset_into_obs({})
    rew, nd = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    status, next_d = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, device="cuda")
    infos = []
    for t in range(T):
        dec = [FW.follow(e) for e in envs]
        want = np.array([FW.discrete_action(d[0], d[1]) for d in dec], np.int64)
        acts = (env.follower_actions if t % 2 else env.expert_actions)(next_d=next_d, status=status)
        assert np.array_equal(acts.cpu().numpy(), want), t
        assert status.cpu().tolist() == [d[0] for d in dec]
        assert np.array_equal(next_d.cpu().numpy().view(np.int32), np.array([d[2] for d in dec], np.float32).view(np.int32))
        env.step_into_obs({}, rew, nd, actions=acts)
        for n, e in enumerate(envs):
            info = e.step(want[n])[3]
            if info:
                infos.append((info, dec[n][0]))
        assert np.array_equal(env._state.cpu().numpy(), np.stack([e.record() for e in envs])), t
    arrived = [i for i, s in infos if s == FW.STATUS_NAMES.index("ARRIVED")]
    assert len(arrived) >= N and all(i["success"] == 1.0 and i["distance_to_goal"] < 0.2 for i in arrived)


def test_shortest_path_follower_evaluates():
    from habitat_amd.common.shortest_path_follower import ShortestPathFollower
    env = make_env(16, 8, 8, 11, K=3, distance="geodesic", max_steps=200)
    out = ShortestPathFollower(env).evaluate(32)
    assert out["episodes"] >= 32 and set(I.MEASURES) <= set(out)
    gave_up = out["unreachable"] + out["stuck"]
    assert out["success"] >= 1.0 - gave_up / out["episodes"] - 1e-9 and out["success"] > 0.8 and 0.5 < out["spl"] <= 1.0
    from habitat_amd import _lib
    with pytest.raises(_lib.HabError, match="Nav2DImageNav.*geodesic"):
        ShortestPathFollower(make_env(2, 8, 8, 11))


def map_of(envs, S, vis):
    n = len(envs)
    return np.zeros((n, S, S), np.uint8), np.zeros((n, S, S), np.uint8), np.zeros((n, M.REC_WORDS), np.int32)


@pytest.mark.parametrize("distance", ["euclidean", "geodesic"])
def test_top_down_map_and_frames(distance):
    """The env with the `top_down_map` keyword equals tests/nav2d_map_reference.py with Nav2D-v0's task code (the goal disc at
    (gx, gy)) after the reset and after every step, and render_frames() equals its frame of rgb, depth and the map: the goal image
    is not part of it."""
    N, T, S, vis, H, W = 3, 10, 40, 2.5, 12, 20
    envs = [I.make_env(6, n, distance, H=H, W=W, num_obstacles=8, turn_angle=30, max_episode_steps=4) for n in range(N)]
    env = make_env(N, H, W, 6, K=8, turn=30, distance=distance, max_steps=4, top_down_map=dict(map_resolution=S, visibility_dist=vis))
    assert env._map_task == M.TASK_GOAL
    m, fog, rec = map_of(envs, S, vis)
    obs = [e.reset() for e in envs]
    for n, e in enumerate(envs):
        M.update(m[n], fog[n], rec[n], M.view(M.TASK_GOAL, e), S, vis, True)
    rows = env._own_obs()
    env.reset_into_obs(rows)
    rng = np.random.RandomState(3)
    for t in range(T + 1):
        got = env.render_frames(height=24).cpu().numpy()
        want = np.stack([M.frame(m[n], fog[n], M.view(M.TASK_GOAL, e), S, 24, obs[n]["rgb"], obs[n]["depth"], True)
                         for n, e in enumerate(envs)])
        assert got.shape == want.shape == (N, 24, M.frame_width(24, H, W, True, True), 3) and np.array_equal(got, want), t
        tdm = env.top_down_map()
        assert np.array_equal(tdm["map"].cpu().numpy(), m) and np.array_equal(tdm["fog_of_war_mask"].cpu().numpy(), fog)
        assert np.array_equal(env._map_rec.cpu().numpy(), rec)
        a = rng.randint(0, 4, size=N)
        res = [e.step(x) for e, x in zip(envs, a)]
        obs = [r[0] for r in res]
        for n, e in enumerate(envs):
            M.update(m[n], fog[n], rec[n], M.view(M.TASK_GOAL, e), S, vis, bool(res[n][2]))
        env.step_into_obs(rows, env._rew, env._nd, actions=torch.from_numpy(a).cuda())
    assert M.TARGET in np.unique(m)


def test_host_path_observations_and_infos():
    """The VectorEnv API on the GPU device: reset() and step() hand over host copies of all five sensors and the four measures."""
    N = 3
    envs = [I.make_env(8, n, "geodesic", H=9, W=18, num_obstacles=3, max_episode_steps=3) for n in range(N)]
    env = make_env(N, 9, 18, 8, K=3, distance="geodesic", max_steps=3)
    obs = env.reset()
    want = [e.reset() for e in envs]
    rng = np.random.RandomState(1)
    for t in range(7):
        for n in range(N):
            assert list(obs[n]) == list(SENSORS)
            for k in SENSORS:
                assert np.array_equal(obs[n][k].reshape(want[n][k].shape), want[n][k]), (t, n, k)
        a = rng.randint(1, 4, size=N)
        res = env.step([int(x) for x in a])
        ref = [e.step(x) for e, x in zip(envs, a)]
        obs, want = [r[0] for r in res], [r[0] for r in ref]
        for n in range(N):
            assert res[n][1] == float(ref[n][1]) and res[n][2] == ref[n][2] and res[n][3] == ref[n][3]
    env.close()


def test_entry_refusals_launch_nothing():
    """Both entries refuse a NULL or misaligned record, a success distance that is not positive / not finite, a compass without its
    table, a missing or misaligned field (the geodesic entry) and what hab_nav2d_step refuses; nothing runs.  A NULL rgb, depth or
    goal_rgb only skips that destination.  The class refuses actions that are no int64 (N,) device tensor, by name."""
    from habitat_amd import _lib
    from habitat_amd._lib import ptr, stream_ptr
    N, H, W = 3, 9, 18
    plus = lambda p, k: type(p)(p.value + k)
    ERR_ARG = -1
    for distance in ("euclidean", "geodesic"):
        env = make_env(N, H, W, 1, K=3, turn=30, distance=distance)
        rows = env._own_obs()
        env.reset_into_obs(rows)
        torch.cuda.synchronize()
        state = env._state.clone()
        actions = torch.ones(N, dtype=torch.int64, device="cuda")
        rew, nd = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
        tabs = env._tables
        base = dict(state=ptr(env._state))
        if distance == "geodesic":
            base.update(geo=ptr(env._geo))
        base.update(dirs=ptr(tabs[0]), ray=ptr(tabs[1]), col_cos=ptr(tabs[2]), tanv=ptr(tabs[3]), actions=ptr(actions), mask=None,
                    rgb=ptr(rows["rgb"]), depth=ptr(rows["depth"]), goal_rgb=ptr(rows["goal_rgb"]), gps=ptr(rows["gps"]),
                    compass=ptr(rows["compass"]), ctab=ptr(env._compass_table), reward=ptr(rew), not_done=ptr(nd),
                    sums=ptr(env.measure_sums), seed=1, offset=0, N=N, H=H, W=W, K=3, nh=12, max_steps=12, sd=1.0, advance=1)
        entry = getattr(_lib.lib(), env._entry)

        def call(**kw):
            a = dict(base, **kw)
            return entry(*(a[k] for k in base), stream_ptr())

        bad = [dict(state=None), dict(state=plus(base["state"], 2)), dict(sd=0.0), dict(sd=-1.0), dict(sd=float("inf")),
               dict(sd=float("nan")), dict(ctab=None), dict(dirs=None), dict(N=0), dict(K=9), dict(K=-1), dict(nh=0), dict(max_steps=0),
               dict(actions=None), dict(reward=None), dict(not_done=None), dict(ray=None), dict(H=0), dict(W=0),
               dict(depth=plus(base["depth"], 2)), dict(rgb=None, depth=None, ray=None)]   # goal_rgb alone still needs the tables
        if distance == "geodesic":
            bad += [dict(geo=None), dict(geo=plus(base["geo"], 2))]
        for kw in bad:
            assert call(**kw) == ERR_ARG, kw
        unsupported = call(W=4096)
        assert unsupported not in (0, ERR_ARG) and call(N=70000) == unsupported
        assert call(N=70000, rgb=None, depth=None) == unsupported          # N <= 65535 with any image, the goal image included
        torch.cuda.synchronize()
        assert torch.equal(env._state, state)                                                          # nothing ran
        assert call() == 0 and call(advance=0, actions=None, reward=None, not_done=None) == 0 and call(sd=0.01) == 0
        assert call(rgb=None) == 0 and call(depth=None) == 0 and call(goal_rgb=None) == 0
        assert call(rgb=None, depth=None, goal_rgb=None, ray=None, col_cos=None, tanv=None, H=0, W=0) == 0
        assert call(gps=None, compass=None, ctab=None, sums=None) == 0
        torch.cuda.synchronize()
        for wrong in (torch.zeros(N, device="cuda"), torch.zeros(N + 1, dtype=torch.int64, device="cuda"), torch.zeros(N, dtype=torch.int64),
                      torch.zeros(N, 2, dtype=torch.int64, device="cuda")[:, 0]):
            with pytest.raises(_lib.HabError, match="Nav2DImageNav"):
                env.step_into_obs({}, rew, nd, actions=wrong)
        if distance == "euclidean":
            for call_ in (env.follower_actions, env.expert_actions):
                with pytest.raises(_lib.HabError, match="Nav2DImageNav.*geodesic"):
                    call_()
        torch.cuda.synchronize()


# ---- the seams: trainers, DAgger, evaluator ------------------------------------------------------------------------------------------
TRAINED = SENSORS   # the YAML's sensors
YAML, DAGGER_YAML = "imagenav/ddppo_nav2d_imagenav.yaml", "imagenav/dagger_nav2d_imagenav_geodesic.yaml"


def overrides(tmp_path, N, T, K=3, max_steps=12, seed=100, size=64, hidden=64):
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=1000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          f"habitat_baselines.rl.ppo.hidden_size={hidden}", f"habitat_baselines.checkpoint_folder={tmp_path}",
          "habitat_baselines.log_interval=1000", f"habitat_baselines.tensorboard_dir={tmp_path}/tb",
          "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000", "habitat_baselines.trainer_name=ppo",
          f"habitat.environment.max_episode_steps={max_steps}", f"habitat.synthetic.num_obstacles={K}", f"habitat.seed={seed}"]
    return ov + [f"habitat.simulator.sensors.{s}.{d}={size}" for s in ("rgb", "depth") for d in ("height", "width")]


def imagenav_config(tmp_path, N, T, extra=(), **kw):
    from habitat_amd.config.default import get_config
    return get_config(YAML, overrides(tmp_path, N, T, **kw) + list(extra))


def restated_envs(cfg, **kw):
    hab = cfg.habitat
    N, size, syn = cfg.habitat_baselines.num_environments, hab.simulator.sensors.rgb.height, hab.synthetic
    kw = dict(dict(H=size, W=size), **kw)
    envs = [I.make_env(hab.seed, n, syn.distance_to_goal, num_obstacles=syn.num_obstacles, turn_angle=syn.turn_angle,
                       success_distance=syn.success_distance, max_episode_steps=hab.environment.max_episode_steps, **kw) for n in range(N)]
    return envs, [e.reset() for e in envs]


def assert_obs(dev_obs, index, o, what):
    for k in TRAINED:
        assert torch.equal(dev_obs[k][index].cpu().reshape(o[k].shape), torch.from_numpy(o[k])), f"{what}: {k}"


def snapshot_before_update(trainer):
    """RolloutStorage.after_update copies row T of every buffer over row 0, so the finished rollout is cloned right before the update."""
    snap, orig = {}, trainer._update_agent

    def update():
        B = trainer._agent.rollouts.buffers
        snap.update({k: B[k].clone() for k in ("actions", "rewards", "masks")})
        snap["observations"] = {k: v.clone() for k, v in B["observations"].items() if k in TRAINED}
        return orig()

    trainer._update_agent = update
    return snap


def test_trainer_hands_over_the_stored_action(tmp_path):
    """Two update cycles of PPOTrainer on the device path from ddppo_nav2d_imagenav.yaml (4 envs, 8 steps, episodes of 12, ResNet18 at
    64 x 64 on rgb + depth + goal_rgb = 7 channels of two dtypes, gps and compass through their embeddings), then the stored actions
    replayed through the restatement from the same seed: every stored row of all five sensors, reward and mask is equal, bit for bit.
    The window statistics carry the four measures."""
    from habitat_amd.common.env_factory import Nav2DImageNavVectorEnv
    N, T = 4, 8
    cfg = imagenav_config(tmp_path, N, T)
    trainer = make_trainer(cfg)
    assert trainer._device_envs and trainer.envs.consumes_actions and isinstance(trainer.envs, Nav2DImageNavVectorEnv)
    policy = trainer._agent.actor_critic
    assert type(policy).__name__ == "PointNavResNetPolicy" and not policy.is_blind and policy.fused_sensors == ()
    assert [(v[0], v[2]) for v in policy.visual_sensors] == [("rgb", 3), ("depth", 1), ("goal_rgb", 3)]
    assert list(trainer._env_spec.observation_space.spaces) == list(TRAINED)
    renvs, obs = restated_envs(cfg)
    infos, snap, used = [], snapshot_before_update(trainer), []
    for cycle in range(2):
        row0 = trainer._agent.rollouts.buffers["observations"]
        assert set(TRAINED) <= set(row0)
        for n in range(N):
            assert_obs({k: row0[k][0] for k in TRAINED}, n, obs[n], f"cycle {cycle} row 0 env {n}")
        losses = trainer.run_update_cycle()
        assert all(np.isfinite(v) for v in losses.values())
        actions = snap["actions"][:T].cpu().numpy().reshape(T, N)
        rewards, masks = snap["rewards"][:T].cpu().numpy().reshape(T, N), snap["masks"][: T + 1].cpu().numpy().reshape(T + 1, N)
        used.append(actions)
        for t in range(T):
            for n, e in enumerate(renvs):
                o, r, done, info = e.step(actions[t, n])
                assert rewards[t, n] == r, f"reward step {t} env {n}"
                assert bool(masks[t + 1, n]) == (not done), f"mask step {t} env {n}"
                assert_obs({k: snap["observations"][k][t + 1] for k in TRAINED}, n, o, f"cycle {cycle} step {t} env {n}")
                obs[n] = o
                if info:
                    infos.append(info)
    assert len(set(np.stack(used).reshape(-1).tolist())) >= 3
    assert len(infos) >= N  # max_episode_steps = 12 < 16 steps: every env ended an episode
    stats = {k: float(v[-1].sum()) for k, v in trainer.window_episode_stats.items()}
    assert stats["count"] == len(infos)
    for k in I.MEASURES:
        assert math.isclose(stats[k], sum(i[k] for i in infos), rel_tol=1e-5, abs_tol=1e-6), k
    assert np.array_equal(trainer.envs._state.cpu().numpy(), np.stack([e.record() for e in renvs]))
    trainer.envs.close()


def test_ver_transport_hands_over_the_stored_action(tmp_path):
    """One VERTrainer rollout on the device-resident source (4 envs, 8 steps): in the VER arena the slots of an env, ordered by
    (episode, step), replay through the restatement with all five sensors compared."""
    N, T = 4, 8
    cfg = imagenav_config(tmp_path, N, T, max_steps=5, extra=["habitat_baselines.trainer_name=ver", "habitat_baselines.rl.ver.num_inference_workers=1"])
    trainer = make_trainer(cfg, "ver")
    ended = []
    orig = trainer.report_worker.episode_end
    trainer.report_worker.episode_end = lambda d: (ended.append(d), orig(d))[1]
    trainer._agent.pre_rollout()
    trainer.collect_rollout()
    Bf = trainer._agent.rollouts.buffers
    ids = {k: Bf[k].view(-1).cpu().numpy() for k in ("environment_ids", "episode_ids", "step_ids")}
    actions, rewards, masks = Bf["actions"].view(-1).cpu().numpy(), Bf["rewards"].view(-1).cpu().numpy(), Bf["masks"].view(-1).cpu().numpy()
    renvs, obs = restated_envs(cfg)
    flat = {k: Bf["observations"][k].reshape((-1,) + obs[0][k].shape) for k in TRAINED}   # one row per slot of the arena
    checked, ref_infos = 0, {}
    for n, e in enumerate(renvs):
        slots = sorted(np.nonzero(ids["environment_ids"] == n)[0], key=lambda s: (ids["episode_ids"][s], ids["step_ids"][s]))
        assert len(slots) >= 2
        o, done, episode = obs[n], True, 0   # the first observation comes with mask False
        for i, s in enumerate(slots):
            assert ids["episode_ids"][s] == episode and bool(masks[s]) == (not done), (n, i)
            assert_obs(flat, int(s), o, f"env {n} slot {i}")
            if i + 1 == len(slots):
                break  # the reward of the last slot arrives with the next rollout
            o, r, done, info = e.step(actions[s])
            assert rewards[s] == r, f"reward env {n} slot {i}"
            if done:
                ref_infos[(n, episode)] = info
                episode += 1
            checked += 1
    assert checked >= N * (T - 1)
    assert len(ended) == len(ref_infos) > 0
    seen = {}
    for d in ended:
        seen[d["env_idx"]] = seen.get(d["env_idx"], -1) + 1
        assert d["info"] == ref_infos[(d["env_idx"], seen[d["env_idx"]])]
    trainer.shutdown()
    trainer.envs.close()


def test_dagger_labels_are_the_follower_s(tmp_path):
    """Two update cycles from dagger_nav2d_imagenav_geodesic.yaml (4 envs x 8 steps, beta 0.5 throughout): tests/test_gpu_dagger.py's
    replay, with the follower's restatement on this task's restated envs as the teacher -- labels, weights, executed actions, rewards
    and masks."""
    from habitat_amd.config.default import get_config
    from test_gpu_dagger import replay as dagger_replay
    N, T = 4, 8
    ov = overrides(tmp_path, N, T, max_steps=40, hidden=128) + [
        "habitat_baselines.rl.imitation.beta_start=0.5", "habitat_baselines.rl.imitation.beta_end=0.5",
        "habitat_baselines.rl.imitation.inflection_weight_coef=3.2"]
    cfg = get_config(DAGGER_YAML, ov)
    trainer = make_trainer(cfg)
    assert type(trainer._agent.updater).__name__ == "DAgger" and type(trainer._agent.rollouts).__name__ == "ImitationRolloutStorage"
    assert trainer._device_envs and type(trainer.envs).__name__ == "Nav2DImageNavVectorEnv" and trainer.envs.distance == "geodesic"
    renvs, _ = restated_envs(cfg, H=2, W=2)

    def teacher(e):
        d = FW.follow(e)
        return FW.discrete_action(d[0], d[1]), d[0]

    dagger_replay(trainer, cfg, renvs, teacher, 2, N, T)
    trainer.envs.close()


def test_evaluator_reports_the_measures(tmp_path):
    """A short HabitatEvaluator run: every recorded episode carries success, spl, distance_to_goal and collisions, equal to the
    restatement's for the actions the evaluator handed over, and the aggregate is their mean."""
    from habitat_amd.rl.ppo.evaluator import HabitatEvaluator
    N = 4
    cfg = imagenav_config(tmp_path, N, 8, max_steps=6, extra=["habitat_baselines.test_episode_count=8"])
    trainer = make_trainer(cfg)
    envs, taken = trainer.envs, []
    orig_step = envs.step
    envs.step = lambda actions: (taken.append([int(np.asarray(a).item()) for a in actions]), orig_step(actions))[1]

    class Writer:
        scalars = {}

        def add_scalar(self, k, v, step):
            self.scalars[k] = v

    ev = HabitatEvaluator()
    torch.manual_seed(3)
    agg = ev.evaluate_agent(trainer._agent, envs, cfg, 0, 0, Writer(), trainer.device, [], trainer._env_spec, set())
    assert set(I.MEASURES) | {"reward"} <= set(agg)
    renvs, _ = restated_envs(cfg, H=2, W=2)
    want, ret = {}, [0.0] * N
    for acts in taken:
        for n, e in enumerate(renvs):
            episode = e.episode
            _, r, done, info = e.step(acts[n])
            ret[n] += float(r)
            if done:
                want[f"{n}:{episode}"] = dict(info, reward=ret[n])
                ret[n] = 0.0
    assert len(ev.last_stats_episodes) >= 8 and len(ev.last_stats_episodes) == len(want)
    for ((scene, episode_id), count), stats in ev.last_stats_episodes.items():
        assert scene == "nav2d" and count == 1
        w = want[episode_id]
        assert {k: stats[k] for k in I.MEASURES} == {k: w[k] for k in I.MEASURES}, episode_id
        assert math.isclose(stats["reward"], w["reward"], rel_tol=1e-5, abs_tol=1e-6)
    for k in I.MEASURES:
        assert math.isclose(agg[k], float(np.mean([w[k] for w in want.values()])), rel_tol=1e-6, abs_tol=1e-9)
        assert Writer.scalars[f"eval_metrics/{k}"] == agg[k]
    envs.close()
