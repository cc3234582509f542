"""GPU: the geodesic distance mode of Nav2DObj-v0 (nav2d_obj_geo_build_kernel, nav2d_obj_geo_step_kernel) against the numpy
restatement (tests/nav2d_obj_geo_reference.py), bit for bit, and the seams that carry it: the mask, the direct build entry, the
entries' refusals, the trainers and the evaluator."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import nav2d_obj_geo_reference as P
import nav2d_obj_reference as O
import nav2d_reference as R
from test_gpu_nav2d import make_trainer
from test_gpu_nav2d_obj import (IMAGES, SENSORS, W_CAT, W_H0, W_INTS, W_LAST, W_OBJ, W_POS, W_START, WORDS, assert_obs, assert_states,
                                empty_rows, snapshot_before_update, stacked)

pytestmark = pytest.mark.gpu
DEV = "cuda"
VECTORS = ("objectgoal", "gps", "compass")
W_DIST, W_ENDED, W_RECTS = slice(4, 7), 11, 16        # d_prev, d_start, path; ended; the rectangles (include/habitat_amd.h)
F = np.float32


def make_env(N, H, W, seed, case, max_steps, distance="geodesic", num_actions=None):
    from habitat_amd.common.env_factory import Nav2DObjVectorEnv
    K, turn, M, C = case
    return Nav2DObjVectorEnv(N, H, W, seed=seed, num_obstacles=K, turn_angle=turn, max_episode_steps=max_steps, num_objects=M,
                             num_categories=C, num_actions=num_actions or (4 if M == 8 else 6), device=DEV, distance=distance)


@functools.lru_cache(maxsize=None)
def reference(kind, case, limit=P.SCRIPT_MAX_EPISODE_STEPS):
    return P.script_rollout(kind, case, limit)


def run_device(ref, case, seed, max_steps, distance="geodesic", H=0, W=0, num_actions=None):
    """Replays ref's actions, every step into its own row of (T + 1, N, ...) tensors; the state and field records are copied after
    the reset and after every step.  Without H and W no image row is given and nothing is rendered."""
    T, N = ref["actions"].shape
    env = make_env(N, H or 8, W or 8, seed, case, max_steps, distance=distance, num_actions=num_actions)
    rows = empty_rows(T, N, H, W, SENSORS if H else VECTORS)
    rew, nd = torch.full((T, N), 99.0, device=DEV), torch.full((T, N), 5, dtype=torch.uint8, device=DEV)
    sums = torch.zeros(T, 4, N, device=DEV)
    states = torch.zeros(T + 1, N, WORDS, dtype=torch.int32, device=DEV)
    fields = torch.zeros(T + 1, N, P.GEO_WORDS, dtype=torch.int32, device=DEV)
    actions = torch.from_numpy(ref["actions"]).to(DEV).unsqueeze(-1)
    env.reset_into_obs({k: v[0] for k, v in rows.items()})
    for t in range(T + 1):
        if t:
            env.step_into_obs({k: v[t] for k, v in rows.items()}, rew[t - 1], nd[t - 1], actions=actions[t - 1])
            sums[t - 1].copy_(env.measure_sums)
        states[t].copy_(env._state)
        if env._geo is not None:
            fields[t].copy_(env._geo)
    torch.cuda.synchronize()
    return env, dict({k: v.cpu() for k, v in rows.items()}, rew=rew.cpu(), nd=nd.cpu(), sums=sums.cpu(), states=states.cpu(),
                     fields=fields.cpu().numpy())


def assert_matches(ref, out, what):
    """Reward, not-done, the named state words with d_prev / d_start / path, the measure sums, every sensor row given and the whole
    field record, as bits, after the reset and after every step."""
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    for k in SENSORS:
        if k in out:
            exp = torch.from_numpy(stacked(ref, k))
            assert out[k].dtype == exp.dtype and torch.equal(bits(out[k]), bits(exp)), f"{what}: {k}"
    assert torch.equal(bits(out["rew"]), bits(torch.from_numpy(ref["rewards"]))), f"{what}: reward"
    assert torch.equal(out["nd"], torch.from_numpy((~ref["dones"]).astype(np.uint8))), f"{what}: not_done"
    assert torch.equal(bits(out["sums"]), bits(torch.from_numpy(ref["sums"]))), f"{what}: measure sums"
    assert_states(ref, out["states"])
    want = np.stack([np.stack([s["dist"] for s in row]) for row in ref["states"]]).view(np.int32)
    got = out["states"].numpy()[:, :, W_DIST]
    for t in range(len(want)):
        assert np.array_equal(got[t], want[t]), f"{what}: d_prev d_start path after step {t}"
        assert np.array_equal(out["fields"][t], ref["fields"][t]), f"{what}: field record after step {t}"


@pytest.mark.parametrize("case", P.SCRIPT_CASES, ids=lambda c: "K{}-turn{}-M{}-C{}".format(*c))
def test_kernels_bitwise(case):
    """The five scripts, 60 steps of 5 envs with an episode limit of 60, and the three drawn scripts once more with episodes of 12
    (P.SCRIPT_RUNS: every env then ends several episodes and has its field rebuilt): everything `assert_matches` names is the
    restatement's, bit for bit.  Six actions where M is odd, four at M = 8, as in the Euclidean cases."""
    for kind, limit in P.SCRIPT_RUNS:
        ref = reference(kind, case, limit)
        _, out = run_device(ref, case, P.SCRIPT_SEED, limit)
        assert_matches(ref, out, f"{kind} / {limit}")


def test_render_is_the_euclidean_entry_s():
    """12 x 20, K = 8, M = 8, the `never_stop` actions with episodes of 12 (episodes end by the step limit alone, so both modes walk
    through the same positions and worlds): rgb, depth, semantic and the three vector sensors of the geodesic entry equal those of
    the Euclidean entry at every step, as do the state words that the distance does not enter."""
    case, H, W = (8, 10, 8, 4), 12, 20
    ref = reference("never_stop", case, P.SHORT_EPISODE_STEPS)
    _, geo = run_device(ref, case, P.SCRIPT_SEED, P.SHORT_EPISODE_STEPS, H=H, W=W)
    _, euc = run_device(ref, case, P.SCRIPT_SEED, P.SHORT_EPISODE_STEPS, distance="euclidean", H=H, W=W)
    same = [0, 1, 2, 3, 6] + list(range(7, 12)) + list(range(W_RECTS, WORDS))        # all but d_prev, d_start and the measures
    assert torch.equal(geo["states"][:, :, same], euc["states"][:, :, same])
    assert not torch.equal(geo["states"][:, :, 5], euc["states"][:, :, 5])          # d_start does differ: the mode is on
    for k in SENSORS:
        assert torch.equal(geo[k], euc[k]), k
    assert geo["rgb"].float().std() > 1 and geo["depth"].min() > 0 and int(geo["semantic"].max()) >= O.SEM_OBJECT


def test_mask_leaves_unselected_envs_alone():
    """N = 5, K = 8, M = 3, episodes of 12 under `never_stop`: after step 12 every env has `ended` set.  Then only envs {1, 3} step:
    envs {0, 2, 4} keep every bit of state, field, sensors, reward, not_done and sums -- their fields are overwritten with a pattern
    first, so a rebuild that a stale `ended` triggered would show -- and envs {1, 3} get the restatement's step."""
    case, N = (8, 10, 3, 4), 5
    ref = reference("never_stop", case, P.SHORT_EPISODE_STEPS)
    env = make_env(N, 8, 8, P.SCRIPT_SEED, case, P.SHORT_EPISODE_STEPS)
    obs = {k: v[0] for k, v in empty_rows(0, N, 0, 0, VECTORS).items()}
    rew, nd = torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)
    actions = torch.from_numpy(ref["actions"]).to(DEV).unsqueeze(-1)
    env.reset_into_obs(obs)
    for t in range(12):
        env.step_into_obs(obs, rew, nd, actions=actions[t])
    assert env._state[:, W_ENDED].cpu().tolist() == [1] * N
    sel, rest = [1, 3], [0, 2, 4]
    mask = torch.zeros(N, dtype=torch.uint8, device=DEV)
    mask[sel] = 1
    env._geo[rest] = 0x5A5A5A5A
    for t in range(12, 26):
        before = dict(state=env._state.clone(), geo=env._geo.clone(), rew=rew.clone(), nd=nd.clone(), sums=env.measure_sums.clone(),
                      **{k: v.clone() for k, v in obs.items()})
        env.step_into_obs(obs, rew, nd, actions=actions[t], mask=mask)
        after = dict(state=env._state, geo=env._geo, rew=rew, nd=nd, sums=env.measure_sums, **obs)
        for k, v in after.items():
            a, b = (v[:, rest], before[k][:, rest]) if k == "sums" else (v[rest], before[k][rest])
            assert torch.equal(a, b), f"step {t}: {k} of an unselected env changed"
        got = env._state.cpu().numpy()
        for n in sel:
            assert np.array_equal(got[n, W_DIST], ref["states"][t + 1][n]["dist"].view(np.int32)), (t, n)
            assert np.array_equal(env._geo[n].cpu().numpy(), ref["fields"][t + 1][n]), (t, n)
            assert rew[n].item() == ref["rewards"][t, n] and bool(nd[n].item()) == (not ref["dones"][t, n])
            assert torch.equal(obs["gps"][n].cpu(), torch.from_numpy(ref["obs"][t + 1][n]["gps"]))
    assert ref["dones"][12:26, sel].sum() >= 2      # the selected envs ended an episode, and got a new field, under the mask


def write_world(state, n, world, pos=None):
    """Writes a hand-made world of the restatement into record n of an (N, 84) int32 state tensor on the host."""
    f = state.view(np.float32)
    rects, objects, cats = world["rects"], world["objects"], world["cats"]
    px, py = pos or world["start"]
    d, idx = O.nearest_target(F(px), F(py), [(F(x), F(y)) for x, y in objects], cats, world["target"])
    f[n, 0:4] = (px, py) + tuple(objects[idx])
    f[n, 4] = f[n, 5] = d
    f[n, 6] = 0.0
    state[n, 7:12] = 0
    f[n, W_RECTS:W_RECTS + 32] = 0.0
    f[n, W_RECTS:W_RECTS + 4 * len(rects)] = np.array(rects, np.float32).reshape(-1)
    f[n, W_START] = world["start"]
    state[n, W_H0] = (0, world["target"])
    f[n, W_OBJ] = 0.0
    f[n, 60:60 + 2 * len(objects)] = np.array(objects, np.float32).reshape(-1)
    state[n, W_CAT] = -1
    state[n, 76:76 + len(cats)] = cats


def test_direct_build_on_hand_made_worlds():
    """hab_nav2d_obj_geo_build on states the test wrote, each world with its own K and M.  The walled-off target: unreachable, the
    record says so and d_start stays the straight line.  Two instances: d_start is the path to the one that is farther in a straight
    line, (gx, gy) stay the nearer.  A node inside another box: +inf.  The slivers: from a position in another object's sliver the
    build finds nothing (unreachable); in the target's own the centre.  Then, in the reachable sliver world, one step from a lost
    position keeps d_prev, pays -0.01 and counts.  A stride above the record's size and only_ended are honoured."""
    from habitat_amd import _lib
    from habitat_amd._lib import check, ptr, stream_ptr
    L = _lib.lib()
    worlds = [P.WALLED, P.DECOY, P.INSIDE, P.SLIVERS]
    for world in worlds:
        K, M = len(world["rects"]), len(world["objects"])
        env = make_env(3, 8, 8, 1, (K, 10, M, max(world["cats"]) + 1), 30)
        env.reset()
        state = env._state.cpu().numpy()
        write_world(state, 0, world)
        write_world(state, 1, world, pos=P.SLIVER_OTHER if world is P.SLIVERS else None)
        write_world(state, 2, world, pos=P.SLIVER_OWN if world is P.SLIVERS else None)
        env._state.copy_(torch.from_numpy(state))
        env._geo.fill_(-1)
        check(L.hab_nav2d_obj_geo_build(ptr(env._state), WORDS * 4, ptr(env._geo), None, 0, 3, K, M, stream_ptr()), "obj_geo_build")
        refs = [P.hand_made(world, max_episode_steps=30) for _ in range(3)]
        if world is P.SLIVERS:
            for e, pos in zip(refs[1:], (P.SLIVER_OTHER, P.SLIVER_OWN)):
                e.px, e.py = F(pos[0]), F(pos[1])
                e.d_start = e.d_prev = O.nearest_target(e.px, e.py, e.objects, e.cats, e.target)[0]
                e.build()
            assert refs[0].reachable and not refs[1].reachable and refs[2].reachable
        got, field = env._state.cpu().numpy(), env._geo.cpu().numpy()
        for n, e in enumerate(refs):
            assert np.array_equal(field[n], e.field_record()), (world, n)
            assert got[n, 4:6].view(np.float32).tolist() == [e.d_prev, e.d_start], (world, n)
        assert np.array_equal(got[:, W_POS], state[:, W_POS])
        if world is P.WALLED:
            assert field[0, P.W_REACHABLE] == 0
        if world is P.SLIVERS:
            # env 0 is moved into the other object's sliver, then one TURN_LEFT for all three
            moved = got.copy()
            moved.view(np.float32)[0, 0:2] = P.SLIVER_OTHER
            env._state.copy_(torch.from_numpy(moved))
            refs[0].px, refs[0].py = F(P.SLIVER_OTHER[0]), F(P.SLIVER_OTHER[1])
            rew, nd = torch.zeros(3, device=DEV), torch.zeros(3, dtype=torch.uint8, device=DEV)
            env.step_into_obs({}, rew, nd, actions=torch.full((3,), O.TURN_LEFT, dtype=torch.int64, device=DEV))
            want = [e.step(O.TURN_LEFT) for e in refs]
            got, field = env._state.cpu().numpy(), env._geo.cpu().numpy()
            assert rew.cpu().tolist() == [float(w[1]) for w in want] and rew[0].item() == F(-0.01)
            assert field[:, P.W_LOST].tolist() == [1, 0, 0]
            for n, e in enumerate(refs):
                assert np.array_equal(field[n], e.field_record()) and got[n, 4:5].view(np.float32)[0] == e.d_prev
    # a stride above the record's size; only_ended builds env 1 alone
    wide = np.zeros((2, WORDS + 4), np.int32)
    for n in range(2):
        write_world(wide, n, P.INSIDE)
    wide[1, W_ENDED] = 1
    dstate, dgeo = torch.from_numpy(wide).to(DEV), torch.full((2, P.GEO_WORDS), 7, dtype=torch.int32, device=DEV)
    check(L.hab_nav2d_obj_geo_build(ptr(dstate), 4 * (WORDS + 4), ptr(dgeo), None, 1, 2, 1, 2, stream_ptr()), "obj_geo_build")
    e = P.hand_made(P.INSIDE)
    assert dgeo[0].cpu().tolist() == [7] * P.GEO_WORDS and np.array_equal(dgeo[1].cpu().numpy(), e.field_record())
    assert dstate[1, 4:6].cpu().numpy().view(np.float32).tolist() == [e.d_prev, e.d_start]
    assert torch.equal(dstate[0].cpu(), torch.from_numpy(wide[0]))


@pytest.mark.parametrize("N", [1, 70])
def test_one_env_and_many(N):
    """N = 1 and N = 70: 6 random steps with episodes of 3, K = 3, M = 3, bitwise."""
    case = (3, 30, 3, 4)
    ref = P.rollout("random", 2, N, 6, turn_angle=30, num_obstacles=3, num_objects=3, num_categories=4, num_actions=6,
                    max_episode_steps=3)
    _, out = run_device(ref, case, 2, 3)
    assert_matches(ref, out, f"N={N}")
    assert ref["dones"].sum() >= N


def test_entry_refusals_are_return_codes():
    """hab_nav2d_obj_step_geo and hab_nav2d_obj_geo_build refuse with the argument error's code and without a launch: the common
    checks, then geo NULL or not 4-byte aligned, then what hab_nav2d_obj_step refuses; the build also a stride below the record's
    size or no multiple of 4, and num_objects outside 1..8."""
    from habitat_amd import _lib
    from habitat_amd._lib import ptr, stream_ptr
    L = _lib.lib()
    N, H, W = 2, 8, 8
    env = make_env(N, H, W, 1, (3, 30, 3, 4), 10)
    env.reset()
    dirs, ray, col_cos, tanv = env._tables
    rows = {k: v[0] for k, v in empty_rows(0, N, H, W, SENSORS).items()}
    act = torch.zeros(N, dtype=torch.int64, device=DEV)
    rew, nd = torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)
    base = dict(state=ptr(env._state), geo=ptr(env._geo), dirs=ptr(dirs), ray=ptr(ray), col_cos=ptr(col_cos), tanv=ptr(tanv),
                actions=ptr(act), mask=None, rgb=ptr(rows["rgb"]), depth=ptr(rows["depth"]), semantic=ptr(rows["semantic"]),
                objectgoal=ptr(rows["objectgoal"]), gps=ptr(rows["gps"]), compass=ptr(rows["compass"]),
                compass_table=ptr(env._compass_table), reward=ptr(rew), not_done=ptr(nd), sums=ptr(env.measure_sums), seed=1,
                env_offset=0, N=N, H=H, W=W, K=3, nh=12, max_steps=10, M=3, C=4, num_actions=6, advance=1)

    def call(**kw):
        return L.hab_nav2d_obj_step_geo(*dict(base, **kw).values(), stream_ptr())

    def plus(p, nbytes):
        return ctypes.c_void_p(p.value + nbytes)

    bbase = dict(state=ptr(env._state), stride=4 * WORDS, geo=ptr(env._geo), mask=None, only_ended=0, N=N, K=3, M=3)
    build = lambda **kw: L.hab_nav2d_obj_geo_build(*dict(bbase, **kw).values(), stream_ptr())
    assert call() == 0 and build() == 0 and call(advance=0, actions=None, reward=None, not_done=None) == 0
    plain = dict(base)
    plain.pop("geo")
    ERR_ARG = L.hab_nav2d_obj_step(*dict(plain, state=None).values(), stream_ptr())
    assert ERR_ARG != 0
    for kw in (dict(geo=None), dict(geo=plus(base["geo"], 2)), dict(geo=plus(base["geo"], 1)), dict(state=None), dict(dirs=None),
               dict(N=0), dict(nh=0), dict(max_steps=0), dict(K=-1), dict(K=9), dict(actions=None), dict(reward=None),
               dict(not_done=None), dict(ray=None), dict(H=0), dict(depth=plus(base["depth"], 2)),
               dict(semantic=plus(base["semantic"], 2)), dict(compass_table=None), dict(M=0), dict(M=9), dict(C=0), dict(C=22),
               dict(num_actions=5)):
        assert call(**kw) == ERR_ARG, kw
    unsupported = call(W=4096)
    assert unsupported not in (0, ERR_ARG) and call(W=4096, geo=None) == unsupported      # the common checks come first
    assert call(geo=None, M=0) == ERR_ARG
    assert call(rgb=None, depth=None, semantic=None, ray=None, col_cos=None, tanv=None, H=0, W=0) == 0
    for kw in (dict(geo=None), dict(geo=plus(base["geo"], 2)), dict(state=None), dict(stride=4 * WORDS - 4), dict(stride=4 * WORDS + 2),
               dict(stride=224), dict(stride=0), dict(N=0), dict(K=9), dict(K=-1), dict(M=0), dict(M=9)):
        assert build(**kw) == ERR_ARG, kw
    assert build(only_ended=1) == 0
    torch.cuda.synchronize()
    assert make_env(2, 8, 8, 1, (3, 30, 3, 4), 10, distance="euclidean")._geo is None
    assert tuple(env._geo.shape) == (N, P.GEO_WORDS)


# ---- the seams: trainer (device path, host path), VER transport, evaluator -----------------------------------------------------------
SIZE = 64


def geo_config(tmp_path, N, T, max_steps=12, seed=100, extra=()):
    from habitat_amd.config.default import get_config
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=1000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          "habitat_baselines.rl.ppo.hidden_size=64", f"habitat_baselines.checkpoint_folder={tmp_path}", "habitat_baselines.log_interval=1000",
          f"habitat_baselines.tensorboard_dir={tmp_path}/tb", "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000",
          "habitat_baselines.trainer_name=ppo", f"habitat.environment.max_episode_steps={max_steps}", f"habitat.seed={seed}"]
    for s in IMAGES:
        ov += [f"habitat.simulator.sensors.{s}.height={SIZE}", f"habitat.simulator.sensors.{s}.width={SIZE}"]
    return get_config("objectnav/ddppo_nav2d_objectnav_geodesic.yaml", ov + list(extra))


def restated_envs(cfg, **kw):
    hab, syn = cfg.habitat, cfg.habitat.synthetic
    assert syn.distance_to_goal == "geodesic" and syn.num_obstacles == 8
    kw = dict(dict(H=SIZE, W=SIZE), **kw)
    envs = [P.Nav2DObjGeoEnv(hab.seed, n, num_obstacles=syn.num_obstacles, turn_angle=syn.turn_angle, num_objects=syn.num_objects,
                             num_categories=syn.num_categories, num_actions=len(hab.task.actions),
                             max_episode_steps=hab.environment.max_episode_steps, **kw)
            for n in range(cfg.habitat_baselines.num_environments)]
    return envs, [e.reset() for e in envs]


@pytest.mark.parametrize("path", ["device", "host"])
def test_trainer_replay(path, tmp_path):
    """One update cycle of PPOTrainer from ddppo_nav2d_objectnav_geodesic.yaml (8 envs, 16 steps, episodes of 12, ResNet18 at
    64 x 64), then the stored actions replayed through the restatement: stored rewards, masks and all six sensor rows of every step
    are equal; the window statistics carry the restatement's measures.  Once on the device path, once on the host's."""
    N, T = 8, 16
    extra = ["habitat_baselines.vector_env_factory._target_=test_gpu_nav2d_obj.HostOnlyNav2DObjFactory"] if path == "host" else []
    cfg = geo_config(tmp_path, N, T, extra=extra)
    trainer = make_trainer(cfg)
    assert trainer._device_envs == (path == "device") and type(trainer._agent.actor_critic).__name__ == "PointNavResNetPolicy"
    assert getattr(trainer.envs, "_envs", trainer.envs).distance == "geodesic"
    renvs, obs = restated_envs(cfg)
    infos, snap = [], snapshot_before_update(trainer)
    row0 = trainer._agent.rollouts.buffers["observations"]
    for n in range(N):
        assert_obs({k: row0[k][0] for k in SENSORS}, n, obs[n], f"row 0 env {n}")
    losses = trainer.run_update_cycle()
    assert all(np.isfinite(v) for v in losses.values())
    actions = snap["actions"][:T].cpu().numpy().reshape(T, N)
    rewards, masks = snap["rewards"][:T].cpu().numpy().reshape(T, N), snap["masks"][: T + 1].cpu().numpy().reshape(T + 1, N)
    for t in range(T):
        for n, e in enumerate(renvs):
            o, r, done, info = e.step(actions[t, n])
            assert rewards[t, n] == r, f"reward step {t} env {n}"
            assert bool(masks[t + 1, n]) == (not done), f"mask step {t} env {n}"
            assert_obs({k: snap["observations"][k][t + 1] for k in SENSORS}, n, o, f"step {t} env {n}")
            if info:
                infos.append(info)
    assert len(set(actions.reshape(-1).tolist())) >= 3 and len(infos) >= N
    assert sum(e.counters["detours"] for e in renvs) > 0       # worlds in which the two distances differ
    stats = {k: float(v[-1].sum()) for k, v in trainer.window_episode_stats.items()}
    assert stats["count"] == len(infos)
    for k in O.MEASURES:
        assert math.isclose(stats[k], sum(i[k] for i in infos), rel_tol=1e-5, abs_tol=1e-6), k
    trainer.envs.close()


def test_ver_trainer_replay(tmp_path):
    """One VERTrainer rollout from the same YAML (8 envs, 16 steps, episodes of 12): the slots of an env, ordered by (episode, step),
    replay through the restatement -- the six sensors of the slot, its stored action, the reward in the same slot, the mask in the
    env's next slot.  The report worker received the restatement's measures for the episodes that ended."""
    N, T = 8, 16
    cfg = geo_config(tmp_path, N, T, extra=["habitat_baselines.trainer_name=ver", "habitat_baselines.rl.ver.num_inference_workers=1"])
    trainer = make_trainer(cfg, "ver")
    ended = []
    orig = trainer.report_worker.episode_end
    trainer.report_worker.episode_end = lambda d: (ended.append(d), orig(d))[1]
    trainer._agent.pre_rollout()
    trainer.collect_rollout()
    B = trainer._agent.rollouts.buffers
    ids = {k: B[k].view(-1).cpu().numpy() for k in ("environment_ids", "episode_ids", "step_ids")}
    actions, rewards, masks = B["actions"].view(-1).cpu().numpy(), B["rewards"].view(-1).cpu().numpy(), B["masks"].view(-1).cpu().numpy()
    renvs, obs = restated_envs(cfg)
    flat = {k: B["observations"][k].reshape((-1,) + obs[0][k].shape) for k in SENSORS}
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
    assert checked >= N * (T - 1) and len(set(actions.tolist())) >= 3
    assert len(ended) == len(ref_infos) > 0
    seen = {}
    for d in ended:
        seen[d["env_idx"]] = seen.get(d["env_idx"], -1) + 1
        assert d["info"] == ref_infos[(d["env_idx"], seen[d["env_idx"]])]
    trainer.shutdown()
    trainer.envs.close()


def test_evaluator_reports_the_measures(tmp_path):
    """A short HabitatEvaluator run on the geodesic env: every recorded episode carries the four measures, equal to the
    restatement's for the actions the evaluator took."""
    from habitat_amd.rl.ppo.evaluator import HabitatEvaluator
    N = 8
    cfg = geo_config(tmp_path, N, 16, max_steps=6, extra=["habitat_baselines.test_episode_count=16"])
    trainer = make_trainer(cfg)
    envs, taken = trainer.envs, []
    orig_step = envs.step
    envs.step = lambda actions: (taken.append(list(actions)), orig_step(actions))[1]

    class Writer:
        def add_scalar(self, k, v, step):
            pass

    ev = HabitatEvaluator()
    torch.manual_seed(3)
    agg = ev.evaluate_agent(trainer._agent, envs, cfg, 0, 0, Writer(), trainer.device, [], trainer._env_spec, set())
    renvs, _ = restated_envs(cfg, H=0, W=0)
    want = {}
    for acts in taken:
        for n, e in enumerate(renvs):
            episode = e.episode
            _, _, done, info = e.step(acts[n])
            if done:
                want[f"{n}:{episode}"] = info
    assert len(ev.last_stats_episodes) >= 16 and len(ev.last_stats_episodes) == len(want)
    for ((scene, episode_id), _), stats in ev.last_stats_episodes.items():
        assert {k: stats[k] for k in O.MEASURES} == want[episode_id], episode_id
    for k in O.MEASURES:
        assert math.isclose(agg[k], float(np.mean([w[k] for w in want.values()])), rel_tol=1e-6, abs_tol=1e-9)
    assert sum(e.counters["detours"] for e in renvs) > 0
    envs.close()
