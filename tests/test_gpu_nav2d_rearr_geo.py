"""GPU: the geodesic distance mode of Nav2DRearr-v0 and Nav2DRearrVel-v0 -- hab_nav2d_rearr_step_geo, hab_nav2d_rearr_vel_step_geo and
hab_nav2d_rearr_geo_build -- against the numpy restatement (tests/nav2d_rearr_geo_reference.py), bit for bit on every output: images,
the three vector sensors, reward, not-done, the named state words, the measure sums and all 72 words of the field record; then the
seams that carry the mode: both trainers from the new YAMLs and the evaluator."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import nav2d_rearr_geo_reference as RG
import nav2d_rearr_reference as A
import nav2d_rearr_vel_reference as B
from test_gpu_nav2d import HostOnlyEnvs, make_trainer
from test_gpu_nav2d_rearr import IMAGES, SENSORS, WORDS, assert_matches, assert_obs, empty_rows, snapshot_before_update

pytestmark = pytest.mark.gpu
DEV = "cuda"
VECTORS = tuple(k for k in SENSORS if k not in IMAGES)
SIZES = [(12, 20), (9, 18), (0, 0)]   # both image shapes of the Euclidean tests, and no image at all
F = np.float32


class Task:
    """What differs between the two tasks for these tests."""

    def __init__(self, vel):
        self.vel, self.name = vel, "Nav2DRearrVel" if vel else "Nav2DRearr"
        self.scripts, self.cases = (RG.VEL_SCRIPTS, RG.VEL_SCRIPT_CASES) if vel else (RG.SCRIPTS, RG.SCRIPT_CASES)
        self.yaml = "rearrange/ddppo_nav2d_rearrange_vel_geodesic.yaml" if vel else "rearrange/ddppo_nav2d_rearrange_geodesic.yaml"
        self.entry = "hab_nav2d_rearr_vel_step" if vel else "hab_nav2d_rearr_step"

    def case_kw(self, case):
        if self.vel:
            return B.case_kw(case)
        K, turn, sh = case
        return dict(num_obstacles=K, turn_angle=turn, start_holding=sh)

    def case_id(self, case):
        return B.case_id(case) if self.vel else "K{}-turn{}-hold{:d}".format(*case)

    def env_class(self):
        from habitat_amd.common import env_factory as EF
        return EF.Nav2DRearrVelVectorEnv if self.vel else EF.Nav2DRearrVectorEnv

    def make_env(self, N, H, W, seed, case, max_steps=RG.SCRIPT_MAX_EPISODE_STEPS, distance="geodesic"):
        return self.env_class()(N, H, W, seed=seed, max_episode_steps=max_steps, use_rgb=H > 0, use_depth=H > 0, device=DEV,
                                distance=distance, **self.case_kw(case))

    def restated(self, seed, n, case, **kw):
        cls = RG.Nav2DRearrVelGeoEnv if self.vel else RG.Nav2DRearrGeoEnv
        return cls(seed, n, **dict(self.case_kw(case), **kw))

    def rollout(self, kind, seed, N, T, case, **kw):
        return (RG.vel_rollout if self.vel else RG.rollout)(kind, seed, N, T, **dict(self.case_kw(case), **kw))

    def device_actions(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        return t if self.vel else t.unsqueeze(-1)   # the layout of the rollout's action rows


TASKS = {"discrete": Task(False), "velocity": Task(True)}
ALL_CASES = [pytest.param(name, case, i, id=f"{name}-{t.case_id(case)}") for name, t in TASKS.items() for i, case in enumerate(t.cases)]


@functools.lru_cache(maxsize=None)
def reference(task, kind, case, H, W):
    t = TASKS[task]
    return (RG.vel_script_rollout if t.vel else RG.script_rollout)(kind, case, H=H, W=W)


def run_device(t, ref, case, H, W, seed, want=None, max_steps=RG.SCRIPT_MAX_EPISODE_STEPS, distance="geodesic"):
    """Replays ref's actions on the device, every step written straight into its own row of separately allocated (T + 1, N, ...)
    tensors, like a rollout arena; the state and field records are copied after the reset and after every step."""
    T, N = ref["actions"].shape[:2]
    want = (SENSORS if H > 0 else VECTORS) if want is None else want
    env = t.make_env(N, H, W, seed, case, max_steps=max_steps, distance=distance)
    rows = empty_rows(T, N, H, W, want)
    rew = torch.full((T, N), 99.0, device=DEV)
    nd = torch.full((T, N), 5, dtype=torch.uint8, device=DEV)
    sums = torch.zeros(T, 4, N, device=DEV)
    states = torch.zeros(T + 1, N, WORDS, dtype=torch.int32, device=DEV)
    geo = distance == "geodesic"
    fields = torch.zeros(T + 1, N, RG.GEO_WORDS, dtype=torch.int32, device=DEV)
    assert env._state.shape == (N, WORDS) and (env._geo.shape == (N, RG.GEO_WORDS) if geo else env._geo is None)
    actions = t.device_actions(ref["actions"])
    env.reset_into_obs({k: v[0] for k, v in rows.items()})
    states[0].copy_(env._state)
    if geo:
        fields[0].copy_(env._geo)
    for s in range(T):
        env.step_into_obs({k: v[s + 1] for k, v in rows.items()}, rew[s], nd[s], actions=actions[s])
        sums[s].copy_(env.measure_sums)
        states[s + 1].copy_(env._state)
        if geo:
            fields[s + 1].copy_(env._geo)
    torch.cuda.synchronize()
    return env, {k: v.cpu() for k, v in rows.items()}, rew.cpu(), nd.cpu(), sums.cpu(), states.cpu(), fields.cpu()


def assert_fields(ref, fields, what=""):
    """All 72 words of every record after the reset and after every step, as bits."""
    got, exp = fields.numpy(), ref["fields"]
    if not np.array_equal(got, exp):
        s, n, w = (int(v[0]) for v in np.nonzero(got != exp))
        raise AssertionError(f"{what}: field record differs first at step {s} env {n} word {w}: {got[s, n, w]} != {exp[s, n, w]}")


def assert_all(ref, out, what=""):
    _, rows, rew, nd, sums, states, fields = out
    assert_matches(ref, rows, rew, nd, sums, states)
    assert_fields(ref, fields, what)


# ---- fails without the feature ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", TASKS)
def test_the_env_accepts_the_geodesic_mode(task):
    t = TASKS[task]
    env = t.make_env(3, 8, 8, 1, t.cases[-1])   # K = 8
    assert env.distance == "geodesic" and env._geo.shape == (3, RG.GEO_WORDS) and env._geo.dtype == torch.int32
    assert env._entry == t.entry + "_geo"
    env.reset()
    torch.cuda.synchronize()
    geo = env._geo.cpu().numpy()
    assert (geo[:, RG.W_SWEEPS_GOAL] >= 1).all() and set(geo[:, RG.W_REACHABLE].tolist()) <= {0, 1} and not geo[:, RG.W_LOST:].any()


# ---- the kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,case,index", ALL_CASES)
def test_kernels_bitwise(task, case, index):
    """Every step of the task's four Euclidean scripts and of 'waypoint', 72 steps of 5 envs with max_episode_steps = 36 (at least
    one reset each, so the build that follows an episode's end runs, and the PLACEs rebuild DO inside the step): images, the three
    vector sensors, reward, not_done, the named state words, the four measure sums and all 72 words of the field record are equal to
    the restatement's bit for bit.  The image size goes round 12 x 20, 9 x 18 and none over scripts and cases, so every script meets
    every size.  tests/test_nav2d_rearr_geo_host.py asserts the events these inputs reach."""
    t = TASKS[task]
    for i, kind in enumerate(t.scripts):
        H, W = SIZES[(i + index) % len(SIZES)]
        ref = reference(task, kind, case, H, W)
        assert ref["dones"].sum() >= RG.SCRIPT_ENVS
        assert_all(ref, run_device(t, ref, case, H, W, RG.SCRIPT_SEED), f"{kind} {H}x{W}")


@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("task", TASKS)
def test_one_env_three_and_seventy(task, N):
    """N = 1, 3 and 70 workgroups: 12 drawn steps with episodes of 6 at K = 8, 9 x 18 images, all outputs bitwise."""
    t = TASKS[task]
    case = t.cases[-4]   # K = 8, not holding at the start
    assert case[0] == 8
    ref = t.rollout("pickplace" if not t.vel else "grip", 4, N, 12, case, max_episode_steps=6, H=9, W=18)
    assert ref["dones"].sum() >= N
    assert_all(ref, run_device(t, ref, case, 9, 18, 4, max_steps=6), f"N={N}")


@pytest.mark.parametrize("missing", SENSORS + ("images", "all"))
@pytest.mark.parametrize("task", TASKS)
def test_missing_destinations(task, missing):
    """Each destination NULL in turn, no image at all and no observation destination at all: what is asked for is still exact, the
    fields included."""
    t = TASKS[task]
    case, (H, W) = t.cases[len(t.cases) // 2], (9, 18)   # K = 3
    want = tuple(k for k in SENSORS if not (k == missing or (missing == "images" and k in IMAGES) or missing == "all"))
    ref = reference(task, "random", case, H, W)
    out = run_device(t, ref, case, H, W, RG.SCRIPT_SEED, want=want)
    assert set(out[1]) == set(want)
    assert_all(ref, out, missing)


@pytest.mark.parametrize("task", TASKS)
def test_mask_steps_only_the_selected_envs(task):
    """With the mask selecting envs {1, 3}: state, field, observations, reward, not_done and measure sums of envs {0, 2, 4} keep every
    bit -- neither the step nor the build that follows it touches them, although some of them ended an episode earlier -- and envs
    {1, 3} get exactly the restatement's step, fields included."""
    t = TASKS[task]
    case, (H, W), N = t.cases[-1], (9, 18), 5   # K = 8, start_holding
    kind = "grip" if t.vel else "pickplace"
    ref = reference(task, kind, case, H, W)
    env = t.make_env(N, H, W, RG.SCRIPT_SEED, case)
    renvs = [t.restated(RG.SCRIPT_SEED, n, case, H=H, W=W, max_episode_steps=RG.SCRIPT_MAX_EPISODE_STEPS) for n in range(N)]
    for e in renvs:
        e.reset()
    env.reset()
    for s in range(40):
        for n in range(N):
            env.async_step_at(n, ref["actions"][s, n])
        assert env.advance_on_device() == list(range(N))
        for n, e in enumerate(renvs):
            e.step(ref["actions"][s, n])
    sel, rest = [1, 3], [0, 2, 4]
    for s in range(40, 60):
        before = dict(state=env._state.clone(), geo=env._geo.clone(), rew=env._rew.clone(), nd=env._nd.clone(),
                      sums=env.measure_sums.clone(), **{k: v.clone() for k, v in env._own_obs().items()})
        for n in sel:
            env.async_step_at(n, ref["actions"][s, n])
        assert env.advance_on_device() == sel
        after = dict(state=env._state, geo=env._geo, rew=env._rew, nd=env._nd, sums=env.measure_sums, **env._own_obs())
        for k, v in after.items():
            a, b = (v[:, rest], before[k][:, rest]) if k == "sums" else (v[rest], before[k][rest])
            assert torch.equal(a, b), f"step {s}: {k} of an unselected env changed"
        own, geo = env._own_obs(), env._geo.cpu().numpy()
        for n in sel:
            o, r, done, _ = renvs[n].step(ref["actions"][s, n])
            for k in SENSORS:
                assert torch.equal(own[k][n].cpu(), torch.from_numpy(o[k])), (s, n, k)
            assert env._rew[n].item() == r and bool(env._nd[n].item()) == (not done)
            assert np.array_equal(geo[n], renvs[n].field_record()), (s, n)
    assert sum(renvs[n].counters["episodes"] for n in sel) >= 2 and sum(renvs[n].counters["rebuilds"] for n in sel) >= 1


@pytest.mark.parametrize("task", TASKS)
def test_no_obstacles_is_the_euclidean_entry_bitwise(task):
    """K = 0: the geodesic entry against hab_nav2d_rearr_step / hab_nav2d_rearr_vel_step on the device, the same actions: images,
    sensors, reward, not_done, measure sums and every word of the state records are equal bit for bit."""
    t = TASKS[task]
    for case in [c for c in t.cases if c[0] == 0][:2]:
        for kind in t.scripts[:4]:
            ref = reference(task, kind, case, 9, 18)
            g = run_device(t, ref, case, 9, 18, RG.SCRIPT_SEED)
            e = run_device(t, ref, case, 9, 18, RG.SCRIPT_SEED, distance="euclidean")
            for k in SENSORS:
                assert torch.equal(g[1][k], e[1][k]), (kind, k)
            for i, name in ((2, "reward"), (4, "sums"), (5, "states")):
                assert torch.equal(g[i].view(torch.int32), e[i].view(torch.int32)), (kind, name)
            assert torch.equal(g[3], e[3])
            assert_fields(ref, g[6], kind)


# ---- the build entry on hand-written records --------------------------------------------------------------------------------------
def build(state, geo, K, start_holding, mask=None, only_ended=0, stride=None):
    from habitat_amd import _lib
    from habitat_amd._lib import ptr, stream_ptr
    rc = _lib.lib().hab_nav2d_rearr_geo_build(ptr(state), 4 * state.shape[1] if stride is None else stride, ptr(geo), ptr(mask), only_ended,
                                              state.shape[0], K, start_holding, stream_ptr())
    torch.cuda.synchronize()
    return rc


HAND_MADE = ("WALLED_GOAL", "WALLED_OBJECT", "OVERLAPPING", "POCKET")


@pytest.mark.parametrize("stride_words", [WORDS, WORDS + 12])
def test_build_entry_on_hand_written_records(stride_words):
    """hab_nav2d_rearr_geo_build on the state records of the hand-made worlds, written word by word, at the record's own stride and
    at a larger one: the field records -- two unreachable ones among them, whose terms are +inf as they came out -- and d_start /
    d_prev are the restatement's.  Then the mask and only_ended: records that are not selected keep every word."""
    envs = [RG.hand_made(getattr(RG, name)) for name in HAND_MADE if not getattr(RG, name).get("start_holding")]
    K = 4
    assert [e.reachable for e in envs] == [False, False, True]
    state = torch.zeros(len(envs), stride_words, dtype=torch.int32, device=DEV)
    want_state = np.stack([e.state_record() for e in envs])
    euclid = want_state.copy()
    for i, e in enumerate(envs):   # what rearr_begin leaves: the straight potential
        euclid[i, 4:6] = np.array([A.Nav2DRearrEnv.potential(e)[0]] * 2, F).view(np.int32)
    state[:, :WORDS] = torch.from_numpy(euclid)
    state[:, WORDS:] = 77
    geo = torch.full((len(envs), RG.GEO_WORDS), 55, dtype=torch.int32, device=DEV)
    for e in envs:
        assert e.K <= K
    # the three worlds have 4, 4 and 2 rectangles: one launch per K
    for k in sorted({e.K for e in envs}):
        mask = torch.tensor([int(e.K == k) for e in envs], dtype=torch.uint8, device=DEV)
        assert build(state, geo, k, 0, mask=mask) == 0
    assert np.array_equal(geo.cpu().numpy(), np.stack([e.field_record() for e in envs]))
    assert np.array_equal(state[:, :WORDS].cpu().numpy(), want_state) and bool((state[:, WORDS:] == 77).all())
    # only_ended: no record has its `ended` word set, so nothing is written; then one is set and only that record is built
    geo.fill_(55)
    assert build(state, geo, 4, 0, only_ended=1) == 0 and bool((geo == 55).all())
    state[0, 11] = 1
    assert build(state, geo, 4, 0, only_ended=1) == 0
    assert np.array_equal(geo[0].cpu().numpy(), envs[0].field_record()) and bool((geo[1:] == 55).all())


@pytest.mark.parametrize("world", ["POCKET", "WALLED_START"])
@pytest.mark.parametrize("task", TASKS)
def test_a_place_across_the_thin_wall_on_the_device(task, world):
    """The two worlds with a ring of thin walls on the device: the hand-written record, built (start_holding: DO stays +inf), then
    three steps through the step entry, every word as the restatement has it.  POCKET: a PLACE into the ring, whose rebuild inside the
    step gives a field without a finite word; both terms keep their values, the steps count as lost, the reward is the slack alone.
    WALLED_START: an unreachable episode, so the Euclidean branch of the geodesic step: a PLACE out of the ring next to the goal
    rebuilds nothing, the STOP after it succeeds by the Euclidean b < 0.5, and the next world and its fields follow."""
    t = TASKS[task]
    w = getattr(RG, world)
    kw = dict(turn_angle=10, max_turn_angle=30, min_abs_ang_speed=10) if t.vel else dict(turn_angle=30)
    e = RG.hand_made(w, vel=t.vel, max_episode_steps=50, **kw)
    case = (4, (10, 30, 10), True, True) if t.vel else (4, 30, True)
    env = t.make_env(1, 0, 0, 1, case, max_steps=50)
    env.reset()
    env._state[0] = torch.from_numpy(e.state_record()).to(DEV)
    assert build(env._state, env._geo, 4, 1) == 0
    assert np.array_equal(env._geo[0].cpu().numpy(), e.field_record()) and np.array_equal(env._state[0].cpu().numpy(), e.state_record())
    rows = {k: v[0] for k, v in empty_rows(0, 1, 0, 0, VECTORS).items()}
    rew, nd = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.uint8, device=DEV)
    # velocity: a slow move into the wall (refused: the agent stays) with the grip open, so that the step is no stop
    steps = [(-0.5, 0.0, -1.0), (-0.5, 1.0, 0.0), (-0.5, -1.0, 0.0)] if t.vel else [A.PLACE, A.TURN_LEFT, A.TURN_RIGHT]
    if world == "WALLED_START":
        assert not e.reachable
        steps = [steps[0], (-1.0, 0.0, 0.0) if t.vel else A.STOP, steps[1]]
    successes = 0
    for a in steps:
        o, r, done, _ = e.step(np.array(a, np.float32) if t.vel else a)
        act = torch.tensor([a], dtype=torch.float32 if t.vel else torch.int64, device=DEV)
        env.step_into_obs(rows, rew, nd, actions=act)
        torch.cuda.synchronize()
        assert rew.item() == r and bool(nd.item()) == (not done)
        assert np.array_equal(env._geo[0].cpu().numpy(), e.field_record()) and np.array_equal(env._state[0].cpu().numpy(), e.state_record())
        for k in VECTORS:
            assert torch.equal(rows[k][0].cpu(), torch.from_numpy(o[k])), k
        successes += int(done and e.last["success"])
    if world == "POCKET":
        assert e.rebuilds == 1 and e.lost_steps >= 1 and not e.holding and np.all(np.isinf(e.DO))
    else:
        assert successes == 1 and e.episode == 1 and e.counters["rebuilds"] == 0 and env.measure_sums[0, 0].item() == 1.0


# ---- the entries' refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", TASKS)
def test_entry_refusals_are_return_codes(task):
    """The geodesic step entry refuses what its Euclidean sibling refuses and, besides, a missing or misaligned field; the build
    entry refuses missing or misaligned pointers, a stride below the rearrangement record's or no multiple of 4, K outside 0..8, N <= 0
    and a start_holding that is neither 0 nor 1 -- with a return code and without a launch."""
    from habitat_amd import _lib
    from habitat_amd._lib import ptr, stream_ptr
    t = TASKS[task]
    L = _lib.lib()
    N, H, W = 2, 8, 8
    assert L.hab_nav2d_rearr_geo_bytes() == 4 * RG.GEO_WORDS
    env = t.make_env(N, H, W, 1, t.cases[len(t.cases) // 2])
    env.reset()
    dirs, ray, col_cos, tanv = env._tables
    rows = {k: v[0] for k, v in empty_rows(0, N, H, W, SENSORS).items()}
    act = torch.zeros(N, 3, device=DEV) if t.vel else torch.zeros(N, dtype=torch.int64, device=DEV)
    rew, nd = torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)
    base = dict(state=ptr(env._state), geo=ptr(env._geo), dirs=ptr(dirs), ray=ptr(ray), col_cos=ptr(col_cos), tanv=ptr(tanv),
                actions=ptr(act), mask=None, head_rgb=ptr(rows["head_rgb"]), head_depth=ptr(rows["head_depth"]),
                obj_start=ptr(rows["obj_start_sensor"]), obj_goal=ptr(rows["obj_goal_sensor"]), is_holding=ptr(rows["is_holding"]),
                reward=ptr(rew), not_done=ptr(nd), sums=ptr(env.measure_sums), seed=1, env_offset=0, N=N, H=H, W=W, K=3,
                nh=env.num_headings, max_steps=10, start_holding=1)
    if t.vel:
        base.update(max_turn=3, stop_turn=1, min_lin=0.025, sliding=1)
    base["advance"] = 1
    step = getattr(L, t.entry + "_geo")

    def call(**kw):
        return step(*dict(base, **kw).values(), stream_ptr())

    def plus(p, nbytes):
        return ctypes.c_void_p((p.value if isinstance(p, ctypes.c_void_p) else int(p)) + nbytes)

    assert call() == 0 and call(advance=0, actions=None, reward=None, not_done=None) == 0 and call(start_holding=0) == 0
    ERR_ARG = call(state=None)
    assert ERR_ARG != 0
    bad = [dict(geo=None), dict(geo=plus(base["geo"], 2)), dict(dirs=None), dict(N=0), dict(nh=0), dict(max_steps=0), dict(K=-1), dict(K=9),
           dict(actions=None), dict(reward=None), dict(not_done=None), dict(ray=None), dict(H=0), dict(head_depth=plus(base["head_depth"], 2)),
           dict(start_holding=2), dict(start_holding=-1)]
    if t.vel:
        bad += [dict(actions=plus(base["actions"], 2)), dict(max_turn=0), dict(stop_turn=4), dict(max_turn=env.num_headings)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    unsupported = call(W=4096)
    assert unsupported not in (0, ERR_ARG) and call(N=70000) == unsupported
    assert call(head_rgb=None, head_depth=None, ray=None, col_cos=None, tanv=None, H=0, W=0) == 0
    assert call(obj_start=None, obj_goal=None, is_holding=None, sums=None) == 0
    # the build entry
    state, geo = env._state, env._geo

    def b(state_p=ptr(state), stride=4 * WORDS, geo_p=ptr(geo), n=N, K=3, sh=0):
        return L.hab_nav2d_rearr_geo_build(state_p, stride, geo_p, None, 0, n, K, sh, stream_ptr())

    assert b() == 0 and b(sh=1) == 0
    for kw in (dict(state_p=None), dict(geo_p=None), dict(geo_p=plus(ptr(geo), 2)), dict(state_p=plus(ptr(state), 2)), dict(stride=4 * WORDS - 4),
               dict(stride=4 * WORDS + 2), dict(stride=224), dict(n=0), dict(K=-1), dict(K=9), dict(sh=2), dict(sh=-1)):
        assert b(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()


# ---- the seams: trainer (device path, host path), VER transport, evaluator -------------------------------------------------------
SIZE = 64


def geo_config(t, tmp_path, N, T, K=8, start_holding=False, max_steps=12, seed=100, extra=()):
    from habitat_amd.config.default import get_config
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=1000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          "habitat_baselines.rl.ppo.hidden_size=64", f"habitat_baselines.checkpoint_folder={tmp_path}",
          "habitat_baselines.log_interval=1000", f"habitat_baselines.tensorboard_dir={tmp_path}/tb",
          "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000", "habitat_baselines.trainer_name=ppo",
          f"habitat.environment.max_episode_steps={max_steps}", f"habitat.synthetic.num_obstacles={K}",
          f"habitat.synthetic.start_holding={start_holding}", f"habitat.seed={seed}"]
    for s in IMAGES:   # head_rgb is added to the file's head_depth, so that all five sensors are in the rollout
        ov += [f"habitat.simulator.sensors.{s}.height={SIZE}", f"habitat.simulator.sensors.{s}.width={SIZE}"]
    cfg = get_config(t.yaml, ov + list(extra))
    assert cfg.habitat.synthetic.distance_to_goal == "geodesic"
    return cfg


def restated_envs(t, cfg, **kw):
    hab = cfg.habitat
    N, size, syn = cfg.habitat_baselines.num_environments, hab.simulator.sensors.head_depth.height, hab.synthetic
    kw = dict(dict(H=size, W=size, num_obstacles=syn.num_obstacles, turn_angle=syn.turn_angle, start_holding=syn.start_holding,
                   max_episode_steps=hab.environment.max_episode_steps), **kw)
    if t.vel:
        kw.update(max_turn_angle=syn.max_turn_angle, min_abs_lin_speed=syn.min_abs_lin_speed, min_abs_ang_speed=syn.min_abs_ang_speed,
                  allow_sliding=syn.allow_sliding)
    cls = RG.Nav2DRearrVelGeoEnv if t.vel else RG.Nav2DRearrGeoEnv
    envs = [cls(hab.seed, n, **kw) for n in range(N)]
    return envs, [e.reset() for e in envs]


def HostOnlyGeoFactory(**kw):  # the `_target_` of the host-path runs
    from habitat_amd.common.env_factory import SyntheticVectorEnvFactory

    class Factory(SyntheticVectorEnvFactory):
        def construct_envs(self, config, workers_ignore_signals=False, enforce_scenes_greater_eq_environments=False, is_first_rank=True,
                           device="cuda", env_offset=0):
            return HostOnlyEnvs(super().construct_envs(config, workers_ignore_signals, enforce_scenes_greater_eq_environments,
                                                       is_first_rank, device=device, env_offset=env_offset))
    return Factory(**kw)


def stored_actions(t, buf, shape):
    a = buf.cpu().numpy()
    return a.reshape(shape + (3,)) if t.vel else a.reshape(shape)


@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("task", TASKS)
def test_trainer_replay(task, path, tmp_path):
    """Two update cycles of PPOTrainer from the task's geodesic YAML (4 envs, 8 steps, episodes of 12, K = 8, ResNet18 on head_rgb +
    head_depth at 64 x 64 with the three 1-D sensors fused), then the stored actions replayed through the geodesic restatement from
    the same seed: every stored observation (all five sensors, every step), reward and mask is equal, bit for bit, and the env's field
    records are the restatement's at the end.  Once on the device path, once on the host path."""
    t = TASKS[task]
    N, T = 4, 8
    extra = [f"habitat_baselines.vector_env_factory._target_={__name__}.HostOnlyGeoFactory"] if path == "host" else []
    cfg = geo_config(t, tmp_path, N, T, extra=extra)
    trainer = make_trainer(cfg)
    inner = getattr(trainer.envs, "_envs", trainer.envs)
    assert trainer._device_envs == (path == "device") and isinstance(inner, t.env_class()) and inner.distance == "geodesic"
    renvs, obs = restated_envs(t, cfg)
    infos, snap = [], snapshot_before_update(trainer)
    for cycle in range(2):
        row0 = trainer._agent.rollouts.buffers["observations"]
        for n in range(N):
            assert_obs({k: row0[k][0] for k in SENSORS}, n, obs[n], f"cycle {cycle} row 0 env {n}")
        losses = trainer.run_update_cycle()
        assert all(np.isfinite(v) for v in losses.values())
        actions = stored_actions(t, snap["actions"][:T], (T, N))
        rewards, masks = snap["rewards"][:T].cpu().numpy().reshape(T, N), snap["masks"][: T + 1].cpu().numpy().reshape(T + 1, N)
        for s in range(T):
            for n, e in enumerate(renvs):
                o, r, done, info = e.step(actions[s, n])
                assert rewards[s, n] == r, f"reward step {s} env {n}"
                assert bool(masks[s + 1, n]) == (not done), f"mask step {s} env {n}"
                assert_obs({k: snap["observations"][k][s + 1] for k in SENSORS}, n, o, f"cycle {cycle} step {s} env {n}")
                obs[n] = o
                if info:
                    infos.append(info)
    assert np.array_equal(inner._geo.cpu().numpy(), np.stack([e.field_record() for e in renvs]))
    assert len(infos) >= N and sum(e.counters["detours"] for e in renvs) > 0
    stats = {k: float(v[-1].sum()) for k, v in trainer.window_episode_stats.items()}
    assert stats["count"] == len(infos)
    for k in RG.MEASURES:
        assert math.isclose(stats[k], sum(i[k] for i in infos), rel_tol=1e-5, abs_tol=1e-6), k
    trainer.envs.close()


@pytest.mark.parametrize("task", TASKS)
def test_ver_trainer_replay(task, tmp_path):
    """One VERTrainer cycle from the task's geodesic YAML (4 envs, 8 steps, start_holding, episodes of 5): in the VER arena the slots
    of an env, ordered by (episode, step), replay through the geodesic restatement -- the slot's observation (all five sensors), then
    its stored action, whose reward is in the same slot and whose mask / next observation are in the env's next slot."""
    t = TASKS[task]
    N, T = 4, 8
    cfg = geo_config(t, tmp_path, N, T, max_steps=5, start_holding=True,
                     extra=["habitat_baselines.trainer_name=ver", "habitat_baselines.rl.ver.num_inference_workers=1"])
    trainer = make_trainer(cfg, "ver")
    ended = []
    orig = trainer.report_worker.episode_end
    trainer.report_worker.episode_end = lambda d: (ended.append(d), orig(d))[1]
    trainer._agent.pre_rollout()
    trainer.collect_rollout()
    Bf = trainer._agent.rollouts.buffers
    ids = {k: Bf[k].view(-1).cpu().numpy() for k in ("environment_ids", "episode_ids", "step_ids")}
    rewards, masks = Bf["rewards"].view(-1).cpu().numpy(), Bf["masks"].view(-1).cpu().numpy()
    actions = stored_actions(t, Bf["actions"], (len(rewards),))
    renvs, obs = restated_envs(t, cfg)
    flat = {k: Bf["observations"][k].reshape((-1,) + obs[0][k].shape) for k in SENSORS}
    checked, ref_infos = 0, {}
    for n, e in enumerate(renvs):
        slots = sorted(np.nonzero(ids["environment_ids"] == n)[0], key=lambda s: (ids["episode_ids"][s], ids["step_ids"][s]))
        assert len(slots) >= 2
        o, done, episode = obs[n], True, 0
        for i, s in enumerate(slots):
            assert ids["episode_ids"][s] == episode and bool(masks[s]) == (not done), (n, i)
            assert_obs(flat, int(s), o, f"env {n} slot {i}")
            if i + 1 == len(slots):
                break
            o, r, done, info = e.step(actions[s])
            assert rewards[s] == r, f"reward env {n} slot {i}"
            if done:
                ref_infos[(n, episode)] = info
                episode += 1
            checked += 1
    assert checked >= N * (T - 1) and len(ended) == len(ref_infos) > 0
    seen = {}
    for d in ended:
        seen[d["env_idx"]] = seen.get(d["env_idx"], -1) + 1
        assert d["info"] == ref_infos[(d["env_idx"], seen[d["env_idx"]])]
    losses = trainer._update_agent()
    assert all(np.isfinite(v) for v in losses.values())
    trainer.shutdown()
    trainer.envs.close()


@pytest.mark.parametrize("task", TASKS)
def test_evaluator_reports_the_measures(task, tmp_path):
    """A short HabitatEvaluator run in the geodesic mode: every recorded episode carries the four measures, object_to_goal_distance
    the geodesic b, equal to the restatement's for the actions the evaluator took, and the aggregate is their mean."""
    from habitat_amd.rl.ppo.evaluator import HabitatEvaluator
    t = TASKS[task]
    N = 4
    cfg = geo_config(t, tmp_path, N, 8, max_steps=6, extra=["habitat_baselines.test_episode_count=8"])
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
    assert set(RG.MEASURES) | {"reward"} <= set(agg)
    renvs, _ = restated_envs(t, cfg, H=0, W=0)
    want, ret = {}, [0.0] * N
    for acts in taken:
        for n, e in enumerate(renvs):
            episode = e.episode
            _, r, done, info = e.step(acts[n] if t.vel else int(acts[n]))
            ret[n] += float(r)
            if done:
                want[f"{n}:{episode}"] = dict(info, reward=ret[n])
                ret[n] = 0.0
    assert len(ev.last_stats_episodes) >= 8 and len(ev.last_stats_episodes) == len(want)
    for ((scene, episode_id), count), stats in ev.last_stats_episodes.items():
        assert scene == "nav2d" and count == 1
        w = want[episode_id]
        assert {k: stats[k] for k in RG.MEASURES} == {k: w[k] for k in RG.MEASURES}, episode_id
        assert math.isclose(stats["reward"], w["reward"], rel_tol=1e-5, abs_tol=1e-6)
    for k in RG.MEASURES:
        assert math.isclose(agg[k], float(np.mean([w[k] for w in want.values()])), rel_tol=1e-6, abs_tol=1e-9)
    envs.close()
