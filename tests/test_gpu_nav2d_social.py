"""GPU: the Nav2DSocial-v0 kernels against the numpy restatement (tests/nav2d_social_reference.py), bit for bit on every output, the
record's 32 field words included, and the seams that carry the task's float actions, the head camera, the two fused 1-D sensors and
the measures: the trainer's device path, its host path, the VER transport and the evaluator, with the ResNet18 policy and the
Gaussian head social_nav/ddppo_nav2d_social.yaml builds; then the learning run."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import nav2d_social_reference as S
from test_gpu_nav2d import HostOnlyEnvs, make_trainer

pytestmark = pytest.mark.gpu
SENSORS = S.SENSORS
IMAGES = ("head_rgb", "head_depth")
WORDS = S.STATE_WORDS
GPU_SCRIPTS = ("forward", "greedy", "random", "grid", "still")


def make_env(N, H, W, seed, case, max_steps=S.SCRIPT_MAX_EPISODE_STEPS, **kw):
    from habitat_amd.common.env_factory import Nav2DSocialVectorEnv
    return Nav2DSocialVectorEnv(N, H, W, seed=seed, max_episode_steps=max_steps, use_rgb=H > 0, use_depth=H > 0, device="cuda",
                                **S.case_kw(case), **kw)


@functools.lru_cache(maxsize=None)
def reference(kind, case, H, W):
    return S.script_rollout(kind, case, H=H, W=W)


def stacked(ref, key):
    return np.stack([np.stack([o[key] for o in row]) for row in ref["obs"]])  # (T + 1, N, ...)


def empty_rows(T, N, H, W, want, dev="cuda"):
    shapes = dict(head_rgb=((H, W, 3), torch.uint8, 7), head_depth=((H, W, 1), torch.float32, -1.0),
                  person_sensor=((2,), torch.float32, -9.0), person_visible=((1,), torch.float32, -9.0))
    return {k: torch.full((T + 1, N) + shapes[k][0], shapes[k][2], dtype=shapes[k][1], device=dev) for k in want}


def run_device(ref, case, H, W, seed, want=SENSORS, max_steps=S.SCRIPT_MAX_EPISODE_STEPS, shift=0, **kw):
    """Replays ref's actions on the device, every step written straight into its own row of separately allocated (T + 1, N, ...)
    tensors, like a rollout arena; the state records are copied after the reset and after every step.  `shift`: the (T, N, 2) action
    tensor is a view that starts that many floats into its buffer."""
    T, N, _ = ref["actions"].shape
    env = make_env(N, H, W, seed, case, max_steps=max_steps, **kw)
    dev = "cuda"
    rows = empty_rows(T, N, H, W, want)
    rew = torch.full((T, N), 99.0, device=dev)
    nd = torch.full((T, N), 5, dtype=torch.uint8, device=dev)
    sums = torch.zeros(T, 4, N, device=dev)
    states = torch.zeros(T + 1, N, WORDS, dtype=torch.int32, device=dev)
    assert env._state.shape == (N, WORDS)
    buffer = torch.zeros(T * N * 2 + shift, device=dev)
    actions = buffer[shift:].view(T, N, 2)                                   # the layout of the rollout's action rows
    actions.copy_(torch.from_numpy(ref["actions"]))
    env.reset_into_obs({k: v[0] for k, v in rows.items()})
    states[0].copy_(env._state)
    for t in range(T):
        env.step_into_obs({k: v[t + 1] for k, v in rows.items()}, rew[t], nd[t], actions=actions[t])
        sums[t].copy_(env.measure_sums)
        states[t + 1].copy_(env._state)
    torch.cuda.synchronize()
    return env, {k: v.cpu() for k, v in rows.items()}, rew.cpu(), nd.cpu(), sums.cpu(), states.cpu(), actions


def assert_matches(ref, rows, rew, nd, sums, states=None):
    for k, v in rows.items():
        exp = torch.from_numpy(stacked(ref, k))
        assert v.dtype == exp.dtype and v.shape == exp.shape, k
        assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v,
                           exp.view(torch.int32) if exp.dtype == torch.float32 else exp), k
    assert torch.equal(rew.view(torch.int32), torch.from_numpy(ref["rewards"]).view(torch.int32)), "reward"
    assert torch.equal(nd, torch.from_numpy((~ref["dones"]).astype(np.uint8))), "not_done"
    assert torch.equal(sums.view(torch.int32), torch.from_numpy(ref["sums"]).view(torch.int32)), "measure sums"
    if states is not None:   # every named word of the record, the 32 of DW among them, after the reset and after every step
        got, exp = states.numpy()[:, :, S.NAMED_WORDS], ref["records"][:, :, S.NAMED_WORDS]
        bad = np.argwhere(got != exp)
        assert bad.size == 0, f"record words differ first at (step, env, word) {bad[0].tolist()} -> word {S.NAMED_WORDS[bad[0][2]]}"


@pytest.mark.parametrize("H,W", [(12, 20), (9, 18)])
@pytest.mark.parametrize("case", S.SCRIPT_CASES, ids=S.case_id)
def test_kernels_bitwise(case, H, W):
    """Every step of the five scripted sequences (forward, greedy towards the person, random in [-1.25, 1.25]^2, grid, stand still),
    60 steps of 5 envs with max_episode_steps = 30 (one reset each): head_rgb, head_depth, person_sensor, person_visible, reward,
    not_done, the four measure sums and every named word of the record -- the person, the waypoint and its index, found, the counters
    and all 32 words of DW -- are equal to the restatement's bit for bit.  Both widths put the first pixel of later envs off 16-byte
    alignment for depth, (9, 18) also has W % 4 != 0."""
    seen = 0
    for kind in GPU_SCRIPTS:
        ref = reference(kind, case, H, W)
        assert ref["dones"].sum() == 2 * S.SCRIPT_ENVS
        _, rows, rew, nd, sums, states, _ = run_device(ref, case, H, W, S.SCRIPT_SEED)
        assert_matches(ref, rows, rew, nd, sums, states)
        seen += ref["counters"]["object_visible"]
    assert seen > 0   # the images show the person


BUSY = (8, (10, 30, 10), 0.2)     # the case of the render checks
SMALL = (3, (10, 30, 10), 0.125)  # the case of the smaller checks


def test_render_with_several_row_tiles():
    """70 x 66 is two row tiles (63 and 7 rows) with W % 4 = 2 and tile boundaries off every alignment: 3 envs, 20 steps, K = 8."""
    H, W, N, T = 70, 66, 3, 20
    ref = S.rollout("greedy", 5, N, T, max_episode_steps=S.SCRIPT_MAX_EPISODE_STEPS, H=H, W=W, **S.case_kw(BUSY))
    _, rows, rew, nd, sums, states, _ = run_device(ref, BUSY, H, W, 5)
    assert_matches(ref, rows, rew, nd, sums, states)


def test_render_one_column_many_rows():
    """W = 1 is the shape with the most rows per tile: 4100 x 1 is five tiles (the last of 4 rows).  2 envs, 3 random steps."""
    H, W, N, T = 4100, 1, 2, 3
    ref = S.rollout("random", 7, N, T, max_episode_steps=S.SCRIPT_MAX_EPISODE_STEPS, H=H, W=W, **S.case_kw(SMALL))
    _, rows, rew, nd, sums, states, _ = run_device(ref, SMALL, H, W, 7)
    assert_matches(ref, rows, rew, nd, sums, states)


@pytest.mark.parametrize("missing", SENSORS + ("images", "all"))
def test_missing_destinations(missing):
    """Each destination NULL in turn, no image at all (nothing is rendered) and no observation destination at all: what is asked for
    is still exact, the record included."""
    H, W = 9, 18
    want = tuple(k for k in SENSORS if not (k == missing or (missing == "images" and k in IMAGES) or missing == "all"))
    ref = reference("random", SMALL, H, W)
    _, rows, rew, nd, sums, states, _ = run_device(ref, SMALL, H, W, S.SCRIPT_SEED, want=want)
    assert set(rows) == set(want)
    assert_matches(ref, rows, rew, nd, sums, states)


def test_an_env_without_images():
    """Without head_rgb and head_depth the env renders nothing and needs no tables; the vector sensors, rewards and records stay exact."""
    ref = reference("greedy", SMALL, 0, 0)
    env, rows, rew, nd, sums, states, _ = run_device(ref, SMALL, 0, 0, S.SCRIPT_SEED, want=("person_sensor", "person_visible"))
    assert list(env.observation_spaces[0].spaces) == ["person_sensor", "person_visible"]
    assert_matches(ref, rows, rew, nd, sums, states)


def test_person_always_visible():
    """person_always_visible gives both vector sensors on every step; rewards, measures and records are those of the default mode."""
    H, W = 9, 18
    ref = S.script_rollout("random", SMALL, H=H, W=W, person_always_visible=True)
    hidden = reference("random", SMALL, H, W)
    assert np.array_equal(ref["rewards"], hidden["rewards"]) and not np.array_equal(stacked(ref, "person_visible"), stacked(hidden, "person_visible"))
    assert (stacked(ref, "person_visible") == 1).all()
    _, rows, rew, nd, sums, states, _ = run_device(ref, SMALL, H, W, S.SCRIPT_SEED, person_always_visible=True)
    assert_matches(ref, rows, rew, nd, sums, states)


@pytest.mark.parametrize("N", [1, 70])
def test_one_env_and_seventy(N):
    """N = 1 and N = 70 (one wavefront each; more envs than one workgroup of the thread-per-env siblings): 12 random steps at an
    episode limit of 6, all outputs bitwise."""
    H, W, T = 9, 18, 12
    ref = S.rollout("random", 4, N, T, max_episode_steps=6, H=H, W=W, **S.case_kw(SMALL))
    assert ref["actions"].shape == (T, N, 2) and ref["dones"].sum() == 2 * N
    _, rows, rew, nd, sums, states, _ = run_device(ref, SMALL, H, W, 4, max_steps=6)
    assert_matches(ref, rows, rew, nd, sums, states)


def test_non_finite_and_out_of_range_components():
    """nan, +inf, -inf act as 0 and +-3.0 as +-1, in either component: 16 steps whose actions cycle through them, bitwise."""
    H, W, N, T = 9, 18, 5, 16
    special = np.array([np.nan, np.inf, -np.inf, 3.0, -3.0, 0.5], np.float32)
    envs = [S.Nav2DSocialEnv(3, n, H=H, W=W, max_episode_steps=10, **S.case_kw(SMALL)) for n in range(N)]
    ref = dict(actions=np.zeros((T, N, 2), np.float32), rewards=np.zeros((T, N), np.float32), dones=np.zeros((T, N), bool),
               sums=np.zeros((T, 4, N), np.float32), records=np.zeros((T + 1, N, WORDS), np.int32), obs=[[e.reset() for e in envs]])
    ref["records"][0] = [e.record() for e in envs]
    for t in range(T):
        a = np.stack([special[(t + np.arange(N)) % 6], special[(t // 2 + 2 * np.arange(N)) % 6]], 1).astype(np.float32)
        if t % 2:
            a = a[:, ::-1].copy()
        res = [e.step(x) for e, x in zip(envs, a)]
        ref["actions"][t], ref["rewards"][t], ref["dones"][t] = a, [r[1] for r in res], [r[2] for r in res]
        ref["obs"].append([r[0] for r in res])
        ref["sums"][t] = [[e.sums[k] for e in envs] for k in S.MEASURES]
        ref["records"][t + 1] = [e.record() for e in envs]
    assert not np.isfinite(ref["actions"]).all() and (np.abs(ref["actions"][np.isfinite(ref["actions"])]) == 3).any()
    _, rows, rew, nd, sums, states, _ = run_device(ref, SMALL, H, W, 3, max_steps=10)
    assert_matches(ref, rows, rew, nd, sums, states)


def test_action_rows_that_are_only_four_byte_aligned():
    """The action tensor is a view that starts one float into its buffer: every row begins 4 bytes past an 8-byte boundary."""
    H, W = 9, 18
    ref = reference("random", SMALL, H, W)
    _, rows, rew, nd, sums, states, actions = run_device(ref, SMALL, H, W, S.SCRIPT_SEED, shift=1)
    assert actions.data_ptr() % 8 == 4 and actions[1].data_ptr() % 8 == 4 and actions.is_contiguous()
    assert_matches(ref, rows, rew, nd, sums, states)


def test_mask_steps_only_the_selected_envs():
    """With the mask selecting envs {1, 3}: the record (DW included), observations, reward, not_done and measure sums of envs
    {0, 2, 4} keep every bit, and envs {1, 3} get exactly the restatement's step.  Through async_step_at / advance_on_device."""
    case, H, W, N = BUSY, 9, 18, 5
    ref = reference("greedy", case, H, W)
    env = make_env(N, H, W, S.SCRIPT_SEED, case)
    renvs = [S.Nav2DSocialEnv(S.SCRIPT_SEED, n, H=H, W=W, max_episode_steps=S.SCRIPT_MAX_EPISODE_STEPS, **S.case_kw(case)) for n in range(N)]
    for e in renvs:
        e.reset()
    env.reset()
    for t in range(20):
        for n in range(N):
            env.async_step_at(n, ref["actions"][t, n])
        assert env.advance_on_device() == list(range(N))
        for n, e in enumerate(renvs):
            e.step(ref["actions"][t, n])
    sel, rest = [1, 3], [0, 2, 4]
    for t in range(20, 44):   # past the selected envs' episode end at their step 30
        before = dict(state=env._state.clone(), rew=env._rew.clone(), nd=env._nd.clone(), sums=env.measure_sums.clone(),
                      **{k: v.clone() for k, v in env._own_obs().items()})
        for n in sel:
            env.async_step_at(n, {"action": ref["actions"][t, n]})
        assert env.advance_on_device() == sel
        after = dict(state=env._state, rew=env._rew, nd=env._nd, sums=env.measure_sums, **env._own_obs())
        assert set(SENSORS) <= set(after)
        for k, v in after.items():
            a, b = (v[:, rest], before[k][:, rest]) if k == "sums" else (v[rest], before[k][rest])
            assert torch.equal(a, b), f"step {t}: {k} of an unselected env changed"
        own = env._own_obs()
        for n in sel:
            o, r, done, _ = renvs[n].step(ref["actions"][t, n])
            for k in SENSORS:
                assert torch.equal(own[k][n].cpu(), torch.from_numpy(o[k])), (t, n, k)
            assert env._rew[n].item() == r and bool(env._nd[n].item()) == (not done)
            assert np.array_equal(env._state[n].cpu().numpy()[S.NAMED_WORDS], renvs[n].record()[S.NAMED_WORDS]), (t, n)
            assert [env.measure_sums[m, n].item() for m in range(4)] == [float(renvs[n].sums[k]) for k in S.MEASURES]
    assert sum(renvs[n].counters["episodes"] for n in sel) == len(sel)


def hand_made(n, rects, start, person, waypoint, h=0):
    """Restated env n in a hand-made world (tests/test_nav2d_social_host.py uses the same ones)."""
    e = S.Nav2DSocialEnv(1, n, H=9, W=18, num_obstacles=len(rects), turn_angle=10, max_turn_angle=30, min_abs_ang_speed=10)
    e.reset()
    e.begin_with(rects, start[0], start[1], person[0], person[1], h=h, waypoint=waypoint)
    return e


def run_hand_made(renvs, steps=3):
    """The restated envs' records, rectangles included, written over the device records after a reset; then `steps` steps of standing
    still on both sides, everything bitwise."""
    N, K, H, W = len(renvs), renvs[0].K, 9, 18
    env = make_env(N, H, W, 1, (K, (10, 30, 10), 0.125))
    rows = empty_rows(steps, N, H, W, SENSORS)
    env.reset_into_obs({k: v[0] for k, v in rows.items()})
    for n, e in enumerate(renvs):
        rec = torch.from_numpy(e.record())
        f = rec.view(torch.float32)
        for k, r in enumerate(e.world.rects):
            f[16 + 4 * k:20 + 4 * k] = torch.tensor([float(v) for v in r])
            rec[48 + k] = sum(int(c) << (8 * i) for i, c in enumerate(e.world.colors[k]))
        env._state[n].copy_(rec)
    rew, nd = torch.zeros(steps, N, device="cuda"), torch.zeros(steps, N, dtype=torch.uint8, device="cuda")
    still = torch.tensor([[-1.0, 0.0]] * N, device="cuda")
    for t in range(steps):
        env.step_into_obs({k: v[t + 1] for k, v in rows.items()}, rew[t], nd[t], actions=still)
        got = env._state.cpu().numpy()
        for n, e in enumerate(renvs):
            o, r, done, _ = e.step((-1.0, 0.0))
            assert np.array_equal(got[n][S.NAMED_WORDS], e.record()[S.NAMED_WORDS]), (t, n)
            assert rew[t, n].item() == r and bool(nd[t, n].item()) == (not done)
            for k in SENSORS:
                assert torch.equal(rows[k][t + 1, n].cpu(), torch.from_numpy(o[k])), (t, n, k)
    return env


def test_hand_made_worlds_on_the_device():
    """The rules that random worlds do not reach, on the device: a person exactly on a node leaves it (the zero hop is no candidate);
    two nodes of the same float32 value, the lower index taken; the waypoint, node 0 and node 1 all at the value 6, the waypoint
    taken; a hop of exactly v lands exactly and draws the next waypoint; an agent exactly 0.4 m from the person's next position is
    not in the way, one a float nearer is; and a walled-off waypoint is given up for the next one (person_lost)."""
    square = [(3.0, 3.0, 5.0, 5.0)]
    x, y, _ = S.G.nodes([tuple(np.float32(v) for v in square[0])])
    renvs = [hand_made(0, square, (1.0, 7.0), (x[0], y[0]), (7.0, 7.0)), hand_made(1, square, (1.0, 7.0), (1.0, 4.0), (7.0, 4.0)),
             hand_made(2, square, (1.0, 7.0), (1.0, y[0]), (7.0, y[0]))]
    assert len({v for _, v in S.hop_candidates(renvs[2].hx, renvs[2].hy, square, 7.0, y[0], renvs[2].DW)[:3]}) == 1
    run_hand_made(renvs)
    assert renvs[0].hx != x[0] and renvs[1].hy < 4.0 and renvs[2].hy == y[0] and renvs[2].hx > 1.3
    at = np.float32(0.225)
    while S.dist(np.float32(0.625), np.float32(1.0), at, np.float32(1.0)) < S.KEEP_OUT:
        at = np.nextafter(at, np.float32(0))
    near = np.nextafter(at, np.float32(1))
    while not S.dist(np.float32(0.625), np.float32(1.0), near, np.float32(1.0)) < S.KEEP_OUT:
        near = np.nextafter(near, np.float32(1))
    renvs = [hand_made(0, [], (7.0, 7.0), (2.0, 2.0), (2.125, 2.0)), hand_made(1, [], (at, 1.0), (0.75, 1.0), (0.5, 1.0)),
             hand_made(2, [], (near, 1.0), (0.75, 1.0), (0.5, 1.0))]
    run_hand_made(renvs)
    # env 1: the first step is taken at exactly 0.4 m; the next hop would end 0.275 m from the agent and is waited out
    assert renvs[0].arrivals == 1 and renvs[1].person_waits == 2 and renvs[1].hx == np.float32(0.625) and renvs[2].person_waits == 3
    renvs = [hand_made(0, S.G.RING, (1.0, 7.0), S.G.RING_OUTSIDE, S.G.RING_INSIDE)]
    run_hand_made(renvs)
    assert renvs[0].person_lost >= 1 and renvs[0].wp_index >= 1


def test_host_path_observations_and_infos():
    """reset() / step() through the VectorEnv API: the host observations carry the four sensors in observation-space order, equal to
    the restatement's, and the infos of the steps that end an episode carry this task's four measures."""
    H, W, N = 9, 18, 3
    env = make_env(N, H, W, 2, SMALL, max_steps=5)
    renvs = [S.Nav2DSocialEnv(2, n, H=H, W=W, max_episode_steps=5, **S.case_kw(SMALL)) for n in range(N)]
    obs = env.reset()
    for n, e in enumerate(renvs):
        o = e.reset()
        assert list(obs[n]) == list(SENSORS) and all(np.array_equal(obs[n][k], o[k]) for k in SENSORS)
    rng, ended = np.random.RandomState(0), 0
    for t in range(12):
        acts = rng.uniform(-1.25, 1.25, size=(N, 2)).astype(np.float32)
        res = env.step(list(acts))
        for n, e in enumerate(renvs):
            o, r, done, info = e.step(acts[n])
            ho, hr, hdone, hinfo = res[n]
            assert all(np.array_equal(ho[k], o[k]) for k in SENSORS) and hr == r and hdone == done
            assert hinfo == info and (not done or list(hinfo) == list(S.MEASURES))
            ended += int(done)
    assert ended == 2 * N


def test_entry_refusals_are_return_codes():
    """hab_nav2d_social_step refuses, with a return code and without a launch: what hab_nav2d_vel_step refuses (missing state / tables,
    parameters outside their ranges, a step without actions, reward or not_done, an image without its tables or size, unaligned depth,
    a width above the maximum, more envs than the render's grid takes, turn counts outside their ranges), an action pointer that is
    not 4-byte aligned, a person_speed outside (0, 0.25] and a person_always_visible that is neither 0 nor 1."""
    from habitat_amd import _lib
    from habitat_amd._lib import ptr, stream_ptr
    L = _lib.lib()
    N, H, W = 2, 8, 8
    env = make_env(N, H, W, 1, SMALL)
    env.reset()
    dirs, ray, col_cos, tanv = env._tables
    rows = {k: v[0] for k, v in empty_rows(0, N, H, W, SENSORS).items()}
    act = torch.zeros(N * 2 + 1, device="cuda")
    rew, nd = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    f = ctypes.c_float
    base = dict(state=ptr(env._state), dirs=ptr(dirs), ray=ptr(ray), col_cos=ptr(col_cos), tanv=ptr(tanv), actions=ptr(act), mask=None,
                head_rgb=ptr(rows["head_rgb"]), head_depth=ptr(rows["head_depth"]), person_sensor=ptr(rows["person_sensor"]),
                person_visible=ptr(rows["person_visible"]), reward=ptr(rew), not_done=ptr(nd), sums=ptr(env.measure_sums), seed=1,
                env_offset=0, N=N, H=H, W=W, K=3, nh=36, max_steps=10, max_turn=3, stop_turn=1, min_lin=f(0.025), sliding=1,
                speed=f(0.125), always=0, advance=1)

    def plus(p, nbytes):
        return ctypes.c_void_p((p.value if isinstance(p, ctypes.c_void_p) else int(p)) + nbytes)

    state = env._state.clone()

    def call(**kw):
        return L.hab_nav2d_social_step(*dict(base, **kw).values(), stream_ptr())

    ERR_ARG = call(state=None)
    assert ERR_ARG != 0
    for kw in (dict(dirs=None), dict(N=0), dict(nh=0), dict(max_steps=0), dict(K=-1), dict(K=9), dict(actions=None), dict(reward=None),
               dict(not_done=None), dict(ray=None), dict(col_cos=None), dict(tanv=None), dict(H=0), dict(W=0),
               dict(head_rgb=None, tanv=None), dict(head_depth=plus(base["head_depth"], 2)), dict(actions=plus(base["actions"], 1)),
               dict(actions=plus(base["actions"], 2)), dict(actions=plus(base["actions"], 3)), dict(max_turn=0), dict(max_turn=-1),
               dict(max_turn=19), dict(max_turn=6, nh=10), dict(stop_turn=0), dict(stop_turn=4), dict(speed=f(0.0)), dict(speed=f(-0.1)),
               dict(speed=f(0.26)), dict(speed=f(float("nan"))), dict(speed=f(float("inf"))), dict(always=2), dict(always=-1)):
        assert call(**kw) == ERR_ARG, kw
    unsupported = call(W=4096)
    assert unsupported not in (0, ERR_ARG) and call(N=70000) == unsupported
    torch.cuda.synchronize()
    assert torch.equal(env._state, state)                     # nothing ran
    assert call() == 0 and call(advance=0, actions=None, reward=None, not_done=None) == 0 and call(always=1) == 0
    assert call(actions=plus(base["actions"], 4)) == 0        # rows that are 4-byte and not 8-byte aligned
    assert call(max_turn=18, stop_turn=18) == 0 and call(sliding=0) == 0 and call(speed=f(0.25)) == 0
    # what needs no image needs no tables either
    assert call(head_rgb=None, head_depth=None, ray=None, col_cos=None, tanv=None, H=0, W=0) == 0
    assert call(person_sensor=None, person_visible=None, sums=None) == 0
    torch.cuda.synchronize()
    # the class refuses what is no (N, 2) float32 device tensor
    for bad in (torch.zeros(N, dtype=torch.int64, device="cuda"), torch.zeros(N, 3, device="cuda"), torch.zeros(N, 2),
                torch.zeros(N, 4, device="cuda")[:, ::2], torch.zeros(N, 2, dtype=torch.float64, device="cuda")):
        with pytest.raises(_lib.HabError, match="Nav2DSocial"):
            env.step_into_obs({}, rew, nd, actions=bad)
    torch.cuda.synchronize()


# ---- the seams: trainer (device path, host path), VER transport, evaluator -------------------------------------------------------
SIZE = 64


def social_config(tmp_path, N, T, K=3, max_steps=12, seed=100, size=SIZE, hidden=64, extra=()):
    from habitat_amd.config.default import get_config
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=1000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          f"habitat_baselines.rl.ppo.hidden_size={hidden}", f"habitat_baselines.checkpoint_folder={tmp_path}",
          "habitat_baselines.log_interval=1000", f"habitat_baselines.tensorboard_dir={tmp_path}/tb",
          "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000", "habitat_baselines.trainer_name=ppo",
          f"habitat.environment.max_episode_steps={max_steps}", f"habitat.synthetic.num_obstacles={K}", f"habitat.seed={seed}",
          f"habitat.simulator.sensors.head_depth.height={size}", f"habitat.simulator.sensors.head_depth.width={size}"]
    return get_config("social_nav/ddppo_nav2d_social.yaml", ov + list(extra))


TRAINED = ("head_depth", "person_sensor", "person_visible")   # the YAML's sensors


def restated_envs(cfg, **kw):
    hab = cfg.habitat
    N, size, syn = cfg.habitat_baselines.num_environments, hab.simulator.sensors.head_depth.height, hab.synthetic
    kw = dict(dict(H=size, W=size, use_rgb=False), **kw)
    envs = [S.Nav2DSocialEnv(hab.seed, n, num_obstacles=syn.num_obstacles, turn_angle=syn.turn_angle, max_turn_angle=syn.max_turn_angle,
                             min_abs_lin_speed=syn.min_abs_lin_speed, min_abs_ang_speed=syn.min_abs_ang_speed,
                             allow_sliding=syn.allow_sliding, person_speed=syn.person_speed,
                             person_always_visible=syn.person_always_visible, max_episode_steps=hab.environment.max_episode_steps, **kw)
            for n in range(N)]
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


def assert_actions_vary(actions, renvs):
    e = renvs[0]
    dec = [S.V.decode(a, e.M) for a in actions.reshape(-1, 2)]
    assert len({d[3] for d in dec}) >= 3 and len({float(d[2]) for d in dec}) >= 3


def HostOnlyNav2DSocialFactory(**kw):  # the `_target_` of the host-path run
    from habitat_amd.common.env_factory import SyntheticVectorEnvFactory

    class Factory(SyntheticVectorEnvFactory):
        def construct_envs(self, config, workers_ignore_signals=False, enforce_scenes_greater_eq_environments=False, is_first_rank=True,
                           device="cuda", env_offset=0):
            return HostOnlyEnvs(super().construct_envs(config, workers_ignore_signals, enforce_scenes_greater_eq_environments,
                                                       is_first_rank, device=device, env_offset=env_offset))
    return Factory(**kw)


@pytest.mark.parametrize("path", ["device", "host"])
def test_trainer_hands_over_the_stored_action(path, tmp_path):
    """Two update cycles of PPOTrainer from ddppo_nav2d_social.yaml (4 envs, 8 steps, episodes of 12, ResNet18 on head_depth at 64 x 64
    with the two 1-D sensors fused, the Gaussian head over two components), then the stored float actions replayed through the
    restatement from the same seed: every stored head_depth row, both vector sensors, reward and mask are equal, bit for bit.  Once on
    the device path, once on the host path.  The window statistics carry the four measures."""
    from habitat_amd.common.env_factory import Nav2DSocialVectorEnv
    from habitat_amd.common.spaces import Box
    N, T = 4, 8
    extra = [f"habitat_baselines.vector_env_factory._target_={__name__}.HostOnlyNav2DSocialFactory"] if path == "host" else []
    cfg = social_config(tmp_path, N, T, extra=extra)
    trainer = make_trainer(cfg)
    assert trainer._device_envs == (path == "device") and trainer.envs.consumes_actions
    assert isinstance(getattr(trainer.envs, "_envs", trainer.envs), Nav2DSocialVectorEnv)
    policy = trainer._agent.actor_critic
    assert type(policy).__name__ == "PointNavResNetPolicy" and policy.action_distribution_type == "gaussian" and not policy.is_blind
    assert [k for k, _ in policy.fused_sensors] == ["person_sensor", "person_visible"]
    assert isinstance(trainer._env_spec.action_space, Box) and trainer._env_spec.action_space.shape == (2,)
    renvs, obs = restated_envs(cfg)
    infos, snap, used = [], snapshot_before_update(trainer), []
    for cycle in range(2):
        row0 = trainer._agent.rollouts.buffers["observations"]
        assert set(TRAINED) <= set(row0)
        for n in range(N):
            assert_obs({k: row0[k][0] for k in TRAINED}, n, obs[n], f"cycle {cycle} row 0 env {n}")
        losses = trainer.run_update_cycle()
        assert all(np.isfinite(v) for v in losses.values())
        assert snap["actions"].dtype == torch.float32 and snap["actions"].shape[-1] == 2
        actions = snap["actions"][:T].cpu().numpy().reshape(T, N, 2)
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
    assert_actions_vary(np.stack(used), renvs)
    assert len(infos) == N  # max_episode_steps = 12 < 16 steps: every env ended one episode, at the limit
    stats = {k: float(v[-1].sum()) for k, v in trainer.window_episode_stats.items()}
    assert stats["count"] == len(infos)
    for k in S.MEASURES:
        assert math.isclose(stats[k], sum(i[k] for i in infos), rel_tol=1e-5, abs_tol=1e-6), k
    trainer.envs.close()


def test_ver_transport_hands_over_the_stored_action(tmp_path):
    """One VERTrainer rollout on the device-resident Nav2DSocial source (4 envs, 8 steps): in the VER arena the slots of an env,
    ordered by (episode, step), replay through the restatement.  The report worker received the measures of the episodes that ended."""
    N, T = 4, 8
    cfg = social_config(tmp_path, N, T, max_steps=5, extra=["habitat_baselines.trainer_name=ver", "habitat_baselines.rl.ver.num_inference_workers=1"])
    trainer = make_trainer(cfg, "ver")
    ended = []
    orig = trainer.report_worker.episode_end
    trainer.report_worker.episode_end = lambda d: (ended.append(d), orig(d))[1]
    trainer._agent.pre_rollout()
    trainer.collect_rollout()
    Bf = trainer._agent.rollouts.buffers
    ids = {k: Bf[k].view(-1).cpu().numpy() for k in ("environment_ids", "episode_ids", "step_ids")}
    assert Bf["actions"].dtype == torch.float32
    actions, rewards, masks = Bf["actions"].view(-1, 2).cpu().numpy(), Bf["rewards"].view(-1).cpu().numpy(), Bf["masks"].view(-1).cpu().numpy()
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


def test_evaluator_reports_the_measures(tmp_path):
    """A short HabitatEvaluator run with the Gaussian head on the Nav2DSocial env: every recorded episode carries has_found_person,
    following_rate, first_encounter_steps and collisions, equal to the restatement's for the actions the evaluator handed over, and
    the aggregate is their mean."""
    from habitat_amd.rl.ppo.evaluator import HabitatEvaluator
    N = 4
    cfg = social_config(tmp_path, N, 8, max_steps=6, extra=["habitat_baselines.test_episode_count=8"])
    trainer = make_trainer(cfg)
    envs, taken = trainer.envs, []
    orig_step = envs.step
    envs.step = lambda actions: (taken.append([np.array(a) for a in actions]), orig_step(actions))[1]

    class Writer:
        scalars = {}

        def add_scalar(self, k, v, step):
            self.scalars[k] = v

    ev = HabitatEvaluator()
    torch.manual_seed(3)
    agg = ev.evaluate_agent(trainer._agent, envs, cfg, 0, 0, Writer(), trainer.device, [], trainer._env_spec, set())
    assert set(S.MEASURES) | {"reward"} <= set(agg)
    assert all(a.shape == (2,) and a.dtype == np.float32 and np.abs(a).max() <= 1.0 for acts in taken for a in acts)
    renvs, _ = restated_envs(cfg, H=0, W=0)
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
        assert {k: stats[k] for k in S.MEASURES} == {k: w[k] for k in S.MEASURES}, episode_id
        assert math.isclose(stats["reward"], w["reward"], rel_tol=1e-5, abs_tol=1e-6)
    for k in S.MEASURES:
        assert math.isclose(agg[k], float(np.mean([w[k] for w in want.values()])), rel_tol=1e-6, abs_tol=1e-9)
        assert Writer.scalars[f"eval_metrics/{k}"] == agg[k]
    envs.close()


# ---- the loop learns to find and follow ------------------------------------------------------------------------------------------
LEARN_UPDATES = 100


@pytest.mark.parametrize("seed", [100, 101, 102])
def test_the_loop_learns_to_find_and_follow(seed, tmp_path):
    """PPOTrainer with a blind PointNavResNetPolicy (hidden 128, one recurrent layer, the Gaussian head over two components) on the
    two fused sensors with person_always_visible: K = 0, turn_angle 10 with max_turn_angle 30 and min_abs_ang_speed 10,
    max_episode_steps 48, 32 envs x 32 steps, lr 5e-4, 4 epochs x 2 minibatches, clip 0.2, LEARN_UPDATES updates
    (tools/nav2d_social_learning.py is the run), three seeds.  The family's criterion: the per-episode returns of the last 5 updates
    against the first 5 of the same run give a two-sample z >= 5 with the mean return higher; and the mean following_rate is higher."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "nav2d_social_learning", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "nav2d_social_learning.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    r = tool.learning_run(str(tmp_path), seed=seed, updates=LEARN_UPDATES)
    print("nav2dsocial learning:", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
    assert r["z"] >= 5.0 and r["return_last"] > r["return_first"] and r["following_last"] > r["following_first"], r
