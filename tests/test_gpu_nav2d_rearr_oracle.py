"""GPU: the pick-and-place oracle of Nav2DRearr-v0 (nav2d_rearr_oracle_kernel, hab_nav2d_rearr_oracle,
Nav2DRearrVectorEnv.oracle_actions, RearrangeOracle) against the numpy restatement (tests/nav2d_rearr_oracle_reference.py), bit for
bit: in closed loop with the env's own step, on hand-made records, on records written from restated runs under the mask, with
missing outputs and a wider stride, and every refusal of the entry."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nav2d_rearr_geo_reference as RG
import nav2d_rearr_oracle_reference as OR
import nav2d_rearr_reference as A
import nav2d_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
STATE_WORDS, GEO_WORDS = RG.STATE_WORDS, RG.GEO_WORDS
FINE_DIRS = R.heading_table(1)
CASES = [(K, turn, sh) for K in (0, 3, 8) for turn in (10, 30) for sh in (False, True)]


def dirs_of(turn):
    from habitat_amd.common.env_factory import nav2d_tables
    d = nav2d_tables(turn, 0, 0)[0]
    assert np.array_equal(d, R.heading_table(turn))
    return torch.from_numpy(d).to(DEV)


def device_env(N, K, turn, start_holding, seed, max_steps=500, distance="geodesic", vel=False):
    from habitat_amd.common import env_factory as EF
    cls = EF.Nav2DRearrVelVectorEnv if vel else EF.Nav2DRearrVectorEnv
    return cls(N, 0, 0, seed=seed, num_obstacles=K, turn_angle=turn, max_episode_steps=max_steps, start_holding=start_holding, use_rgb=False,
               use_depth=False, device=DEV, distance=distance)


def call(state, geo, dirs, K, mask=None, actions=None, next_d=None, status=None, stride=None, N=None):
    """One call of the entry on device tensors -> the return code."""
    from habitat_amd import _lib
    from habitat_amd._lib import ptr, stream_ptr
    N = state.shape[0] if N is None else N
    stride = state.shape[1] * 4 if stride is None else stride
    return _lib.lib().hab_nav2d_rearr_oracle(ptr(state), stride, ptr(geo), ptr(dirs), ptr(mask), ptr(actions), ptr(next_d), ptr(status), N, K,
                                             dirs.shape[0], stream_ptr())


def outputs(N, fill=-7):
    """(actions, next_d, status) of N envs between two guard elements, all pre-filled: a sentinel in the integers, NaN in next_d."""
    a, nd, st = (torch.full((N + 2,), fill, dtype=torch.int64, device=DEV), torch.full((N + 2,), float("nan"), device=DEV),
                 torch.full((N + 2,), fill, dtype=torch.int32, device=DEV))
    return (a, nd, st), (a[1:N + 1], nd[1:N + 1], st[1:N + 1])


def expected(answers):
    return (np.array([OR.action_of(d) for d in answers], np.int64), np.array([d[2] for d in answers], np.float32),
            np.array([d[0] for d in answers], np.int32))


def assert_answers(got, want, what, sel=None, fill=-7):
    """Bitwise, where `sel` (default: everywhere) selects; elsewhere the pre-filled values, bitwise too."""
    a, nd, st = (t.cpu().numpy() for t in got)
    sel = np.ones(len(a), bool) if sel is None else sel
    assert np.array_equal(st[sel], want[2][sel]), f"{what}: status {st[sel]} != {want[2][sel]}"
    assert np.array_equal(nd.view(np.int32)[sel], want[1].view(np.int32)[sel]), f"{what}: next_d"
    assert np.array_equal(a[sel], want[0][sel]), f"{what}: actions"
    nan = np.full(1, np.nan, np.float32).view(np.int32)[0]
    assert np.all(a[~sel] == fill) and np.all(st[~sel] == fill) and np.all(nd.view(np.int32)[~sel] == nan), f"{what}: unselected outputs"


def assert_guards(whole, fill=-7):
    a, nd, st = (t.cpu().numpy() for t in whole)
    nan = np.full(1, np.nan, np.float32).view(np.int32)[0]
    for g in (0, -1):
        assert a[g] == fill and st[g] == fill and nd.view(np.int32)[g] == nan, "a guard element was written"


# ---- closed loop: the device env under the device's answers, the restated env under the restatement's ---------------------------------
def closed_loop_on_device(env, T):
    """-> actions, next_d, status (T, N), rewards, not-done (T, N), field records (T + 1, N, 72), state records (T + 1, N, 68)."""
    N = env.num_envs
    acts, next_d = torch.zeros((T, N), dtype=torch.int64, device=DEV), torch.zeros(T, N, device=DEV)
    status = torch.zeros(T, N, dtype=torch.int32, device=DEV)
    rew, nd = torch.zeros(T, N, device=DEV), torch.zeros(T, N, dtype=torch.uint8, device=DEV)
    fields = torch.zeros(T + 1, N, GEO_WORDS, dtype=torch.int32, device=DEV)
    states = torch.zeros(T + 1, N, STATE_WORDS, dtype=torch.int32, device=DEV)
    env.reset_into_obs({})
    fields[0].copy_(env._geo)
    states[0].copy_(env._state)
    for t in range(T):
        a = env.oracle_actions(out=acts[t], next_d=next_d[t], status=status[t])
        assert a.data_ptr() == acts[t].data_ptr()
        env.step_into_obs({}, rew[t], nd[t], actions=a)
        fields[t + 1].copy_(env._geo)
        states[t + 1].copy_(env._state)
    torch.cuda.synchronize()
    return tuple(v.cpu().numpy() for v in (acts, next_d, status, rew, nd, fields, states))


def assert_closed_loop(ref, got, what):
    acts, next_d, status, rew, nd, fields, _ = got
    for t in range(acts.shape[0]):
        assert np.array_equal(status[t], ref["status"][t]), f"{what} step {t}: status {status[t]} != {ref['status'][t]}"
        assert np.array_equal(acts[t], ref["actions"][t]), f"{what} step {t}: action"
        assert np.array_equal(next_d[t].view(np.int32), ref["next_d"][t].view(np.int32)), f"{what} step {t}: next_d"
        assert np.array_equal(fields[t + 1], ref["fields"][t + 1]), f"{what} step {t}: field record"
    assert np.array_equal(rew.view(np.int32), ref["rewards"].view(np.int32)) and np.array_equal(nd, (~ref["dones"]).astype(np.uint8))


@pytest.mark.parametrize("K,turn,start_holding", CASES, ids=lambda v: str(int(v)))
def test_closed_loop(K, turn, start_holding):
    """N = 24, 160 steps of `oracle_actions()` feeding `step_into_obs`: every action, status and next_d, every word of the field
    records, every reward and not-done byte equals the restatement's closed loop; episodes end, and all that end ARRIVED succeed."""
    N, T, seed = 24, 160, 5
    ref = OR.closed_loop(OR.restated_envs(seed, N, K, turn, start_holding), T)
    got = closed_loop_on_device(device_env(N, K, turn, start_holding, seed), T)
    assert_closed_loop(ref, got, f"K={K} turn={turn} start_holding={start_holding}")
    c, st = ref["counters"], ref["status"]
    assert c["timeouts"] == 0 and c["episodes"] == int(np.isin(st, OR.ENDS).sum()) >= N and c["successes"] == int((st == OR.ARRIVED).sum())
    assert (st == OR.PLACE).sum() >= c["successes"] >= N // 2 and ((st == OR.PICK).sum() >= N // 2 or start_holding)
    assert c["blocked_object"] + c["blocked_rect"] + c["blocked_wall"] == 0
    assert sum(c[k] for k in ("pick_far", "pick_behind", "pick_holding", "place_in_rect", "place_outside_box", "place_not_holding")) == 0


def test_closed_loop_at_360_headings():
    """turn_angle = 1, the most headings the task accepts: six passes of the lanes, the last a partial one, with the env's step in
    the loop; 8 envs, 120 steps, K = 8.  At one degree a step most of such a run is turning towards the first winner;
    test_written_records_at_360_headings covers the paths it does not reach."""
    N, T, K, seed = 8, 120, 8, 5
    ref = OR.closed_loop(OR.restated_envs(seed, N, K, 1, False), T)
    got = closed_loop_on_device(device_env(N, K, 1, False, seed), T)
    assert_closed_loop(ref, got, "nh=360")
    acts = ref["actions"]
    assert all((acts == a).sum() >= N for a in (A.MOVE_FORWARD, A.TURN_LEFT, A.TURN_RIGHT))


# ---- records written into device memory --------------------------------------------------------------------------------------------
def test_hand_made_records():
    """The records of tests/test_nav2d_rearr_oracle_host.py written into device state and field records: the rule's answer in each."""
    for case in OR.hand_made_cases():
        name, turn = case[0], case[1]
        e = OR.hand_made_env(case)
        answer = OR.oracle(e)
        assert answer[:2] == case[-1], name
        whole, got = outputs(1)
        state, geo = torch.from_numpy(e.state_record()[None]).to(DEV), torch.from_numpy(e.field_record()[None]).to(DEV)
        assert call(state, geo, dirs_of(turn), len(e.world.rects), None, *got) == 0
        assert_answers(got, expected([answer]), name)
        assert_guards(whole)


def answer_of(e, dirs):
    """The rule on the records of the restated env `e` with the heading table `dirs`, which need not be the env's own."""
    return OR.decide(e.px, e.py, e.h, e.world.rects, (e.gx, e.gy), (e.ox, e.oy), e.holding, e.DG, e.DO, e.a, e.b, e.reachable, dirs)


@functools.lru_cache(maxsize=None)
def snapshots(count=70, K=8, turn=10, steps=70):
    """`count` records of 10 restated envs under the oracle (envs 0..4 without start_holding, 5..9 with it) over `steps` steps: up to
    30 records whose answer is not GO, spread over the run, behind GO records spread alike -> (states (count, 68), fields
    (count, 72), the answers at the envs' own 36 headings, the answers at 360 headings)."""
    envs = [RG.Nav2DRearrGeoEnv(1, n, num_obstacles=K, turn_angle=turn, start_holding=n >= 5, use_rgb=False, use_depth=False) for n in range(10)]
    for e in envs:
        e.reset()
    go, other = [], []
    for _ in range(steps):
        for e in envs:
            d = OR.oracle(e)
            (go if d[0] == OR.GO else other).append((e.state_record(), e.field_record(), d, answer_of(e, FINE_DIRS)))
            e.step(OR.action_of(d))
    other = other[:: max(1, len(other) // 30)][:30]
    go = go[:: len(go) // (count - len(other))][: count - len(other)]
    out = go + other
    assert len(out) == count
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), [o[2] for o in out], [o[3] for o in out]


@pytest.mark.parametrize("N", [70, 1])
def test_entry_on_written_records(N):
    """N = 70 and N = 1: the answers are the restatement's, the guard elements stay, and state and field records are byte for byte
    what they were."""
    state, geo, answers, _ = snapshots()
    want = tuple(w[-N:] for w in expected(answers))
    ds, dg = torch.from_numpy(state[-N:].copy()).to(DEV), torch.from_numpy(geo[-N:].copy()).to(DEV)
    whole, got = outputs(N)
    assert call(ds, dg, dirs_of(10), 8, None, *got) == 0
    assert_answers(got, want, f"N={N}")
    assert_guards(whole)
    assert ds.cpu().numpy().tobytes() == state[-N:].tobytes() and dg.cpu().numpy().tobytes() == geo[-N:].tobytes()
    if N == 70:
        st = want[2]
        assert all((st == code).sum() >= 2 for code in (OR.GO, OR.ARRIVED, OR.PICK, OR.PLACE)) and (want[0] == A.MOVE_FORWARD).sum() >= 10
        assert (want[0] == A.TURN_LEFT).sum() >= 3 and (want[0] == A.TURN_RIGHT).sum() >= 3


def test_written_records_at_360_headings():
    """The same 70 records read with the table of 360 headings (the HEADING word then counts degrees): six passes of the lanes, the
    last a partial one, in each of the three paths, PICK and PLACE among the answers."""
    state, geo, _, fine = snapshots()
    want = expected(fine)
    whole, got = outputs(70)
    assert call(torch.from_numpy(state).to(DEV), torch.from_numpy(geo).to(DEV), dirs_of(1), 8, None, *got) == 0
    assert_answers(got, want, "nh=360")
    assert_guards(whole)
    assert all((want[2] == code).sum() >= 1 for code in (OR.GO, OR.ARRIVED, OR.PICK, OR.PLACE))


def test_mask_missing_outputs_and_stride():
    """The mask leaves the outputs of unselected envs untouched, NaN and sentinel bits included; next_d and status may be NULL, each
    alone and both; records of 72 words with a pattern after the 68 give the same answers."""
    K, turn, N = 8, 10, 70
    state, geo, answers, _ = snapshots()
    want = expected(answers)
    dirs, ds, dg = dirs_of(turn), torch.from_numpy(state).to(DEV), torch.from_numpy(geo).to(DEV)
    sel = np.random.RandomState(3).rand(N) < 0.5
    whole, got = outputs(N)
    assert call(ds, dg, dirs, K, torch.from_numpy(sel.astype(np.uint8)).to(DEV), *got) == 0
    assert_answers(got, want, "mask", sel=sel)
    assert_guards(whole)
    for keep in ("next_d", "status", None):
        whole, (a, nd, st) = outputs(N)
        assert call(ds, dg, dirs, K, None, a, nd if keep == "next_d" else None, st if keep == "status" else None) == 0
        assert np.array_equal(a.cpu().numpy(), want[0])
        got_nd, got_st = nd.cpu().numpy(), st.cpu().numpy()     # what was not handed in keeps its fill
        assert np.array_equal(got_nd.view(np.int32), want[1].view(np.int32)) if keep == "next_d" else np.isnan(got_nd).all()
        assert np.array_equal(got_st, want[2]) if keep == "status" else np.all(got_st == -7)
        assert_guards(whole)
    wide = np.full((N, STATE_WORDS + 4), 0x5A5A5A5A, np.int32)
    wide[:, :STATE_WORDS] = state
    whole, got = outputs(N)
    assert call(torch.from_numpy(wide).to(DEV), dg, dirs, K, None, *got) == 0
    assert_answers(got, want, "stride 288")


def test_entry_refusals_are_return_codes():
    """The entry refuses, with the argument error's code and without a launch: state, geo, dirs or actions NULL or misaligned; actions
    not 8-byte aligned; next_d or status misaligned; a stride below the rearrangement record or no multiple of 4; N <= 0; K outside
    0..8; num_headings <= 0."""
    from habitat_amd import _lib
    from habitat_amd._lib import ptr, stream_ptr
    L = _lib.lib()
    N, K = 4, 8
    state, geo, _, _ = snapshots()
    ds, dg, dirs = torch.from_numpy(state[:N].copy()).to(DEV), torch.from_numpy(geo[:N].copy()).to(DEV), dirs_of(10)
    ERR_ARG = L.hab_nav2d_rearr_geo_build(None, 4 * STATE_WORDS, ptr(dg), None, 0, N, K, 0, stream_ptr())
    assert ERR_ARG != 0

    def plus(p, nbytes):
        return ctypes.c_void_p(p.value + nbytes)

    _, (a, nd, st) = outputs(N + 1)
    base = dict(state=ptr(ds), stride=4 * STATE_WORDS, geo=ptr(dg), dirs=ptr(dirs), mask=None, actions=ptr(a), next_d=ptr(nd), status=ptr(st),
                N=N, K=K, nh=36)
    go = lambda **kw: L.hab_nav2d_rearr_oracle(*dict(base, **kw).values(), stream_ptr())  # noqa: E731
    assert go() == 0 and go(next_d=None, status=None) == 0 and go(stride=4 * STATE_WORDS + 4) == 0
    bad = [dict(state=None), dict(geo=None), dict(dirs=None), dict(actions=None), dict(state=plus(base["state"], 2)),
           dict(geo=plus(base["geo"], 2)), dict(dirs=plus(base["dirs"], 2)), dict(actions=plus(base["actions"], 4)),
           dict(actions=plus(base["actions"], 2)), dict(next_d=plus(base["next_d"], 2)), dict(status=plus(base["status"], 1)),
           dict(stride=224), dict(stride=4 * STATE_WORDS - 4), dict(stride=4 * STATE_WORDS + 2), dict(stride=0), dict(N=0), dict(N=-1),
           dict(K=9), dict(K=-1), dict(nh=0), dict(nh=-36)]
    for kw in bad:
        assert go(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()


# ---- the env's method and the oracle class -----------------------------------------------------------------------------------------
def test_oracle_actions_arguments():
    """A fresh int64 (N,) tensor where `out` is None, which `step_into_obs` takes; a wrong dtype, shape or device is refused; the
    Euclidean env and the velocity task refuse by name."""
    from habitat_amd import _lib
    env = device_env(3, 3, 10, False, 1)
    env.reset_into_obs({})
    a = env.oracle_actions()
    assert tuple(a.shape) == (3,) and a.dtype == torch.int64 and a.is_cuda
    env.step_into_obs({}, torch.zeros(3, device=DEV), torch.zeros(3, dtype=torch.uint8, device=DEV), actions=a)
    for kw in (dict(out=torch.zeros(3, dtype=torch.int32, device=DEV)), dict(out=torch.zeros(4, dtype=torch.int64, device=DEV)),
               dict(out=torch.zeros(3, dtype=torch.int64)), dict(mask=torch.zeros(3, dtype=torch.bool, device=DEV)),
               dict(next_d=torch.zeros(3, dtype=torch.float64, device=DEV)), dict(status=torch.zeros(3, dtype=torch.int64, device=DEV)),
               dict(status=torch.zeros(2, dtype=torch.int32, device=DEV))):
        with pytest.raises(_lib.HabError, match="Nav2DRearr: oracle_actions"):
            env.oracle_actions(**kw)
    with pytest.raises(_lib.HabError, match="needs `distance_to_goal: geodesic`"):
        device_env(3, 3, 10, False, 1, distance="euclidean").oracle_actions()
    with pytest.raises(_lib.HabError, match="Nav2DRearrVel:.*no pick-and-place oracle"):
        device_env(3, 3, 1, False, 1, vel=True).oracle_actions()
    with pytest.raises(_lib.HabError, match="no shortest-path follower"):
        env.follower_actions()


def test_rearrange_oracle_evaluate():
    """N = 32, K = 3, at least 40 episodes: the measure means and the counts equal those of the restatement's closed loop for the same
    seeds up to the step at which the fortieth episode ended."""
    from habitat_amd.common.rearrange_oracle import RearrangeOracle
    N, K, turn, seed, want_eps = 32, 3, 30, 5, 40
    ref = OR.closed_loop(OR.restated_envs(seed, N, K, turn, False), 90)
    ended = np.cumsum(ref["dones"].sum(1))
    t = int(np.argmax(ended >= want_eps))
    assert ended[t] >= want_eps
    oracle = RearrangeOracle(device_env(N, K, turn, False, seed))
    a = oracle.get_next_actions()          # before any reset: zeroed records are "unreachable", nothing is read out of bounds
    assert a.data_ptr() == oracle.get_next_actions().data_ptr() and bool((oracle.status == OR.UNREACHABLE).all())
    out = oracle.evaluate(want_eps)
    episodes = int(ended[t])
    st = ref["status"][: t + 1]
    assert out["episodes"] == episodes and out["steps"] == (t + 1) * N
    assert out["unreachable"] == int((st == OR.UNREACHABLE).sum()) and out["stuck"] == int((st == OR.STUCK).sum())
    for i, k in enumerate(A.MEASURES):
        assert out[k] == float(ref["sums"][t][i].astype(np.float64).sum()) / episodes, k
    assert out["success"] == float((st == OR.ARRIVED).sum()) / episodes and out["collisions"] == 0.0
    assert np.array_equal(oracle.status.cpu().numpy(), ref["status"][t]) and oracle.next_distance.dtype == torch.float32
