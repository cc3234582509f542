"""GPU: the Nav2DRearrVel-v0 step kernel against the numpy restatement (tests/nav2d_rearr_vel_reference.py), bit for bit on every
output, and the seams that carry the task's float actions, the head camera, the three fused 1-D sensors and the measures: the trainer's
device path, its host path, the VER transport and the evaluator, all with the ResNet18 policy and the Gaussian head the new YAML
builds -- the Gaussian head, the Linear(3, 32) previous-action embedding, float action storage and the fused sensor columns in one
run; then the learning run."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import nav2d_rearr_vel_reference as B
from test_gpu_nav2d import HostOnlyEnvs, make_trainer
from test_gpu_nav2d_rearr import IMAGES, WORDS, assert_matches, assert_obs, empty_rows, snapshot_before_update

pytestmark = pytest.mark.gpu
SENSORS = B.SENSORS


def make_env(N, H, W, seed, case, max_steps=B.SCRIPT_MAX_EPISODE_STEPS, **kw):
    from habitat_amd.common.env_factory import Nav2DRearrVelVectorEnv
    return Nav2DRearrVelVectorEnv(N, H, W, seed=seed, max_episode_steps=max_steps, use_rgb=True, use_depth=True, device="cuda",
                                  **B.case_kw(case), **kw)


@functools.lru_cache(maxsize=None)
def reference(kind, case, H, W):
    return B.script_rollout(kind, case, H=H, W=W)


def run_device(ref, case, H, W, seed, want=SENSORS, max_steps=B.SCRIPT_MAX_EPISODE_STEPS, shift=0):
    """Replays ref's actions on the device, every step written straight into its own row of separately allocated (T + 1, N, ...)
    tensors, like a rollout arena; the state records are copied after the reset and after every step.  `shift`: the (T, N, 3) action
    tensor is a view that starts that many floats into its buffer."""
    T, N, _ = ref["actions"].shape
    env = make_env(N, H, W, seed, case, max_steps=max_steps)
    dev = "cuda"
    rows = empty_rows(T, N, H, W, want)
    rew = torch.full((T, N), 99.0, device=dev)
    nd = torch.full((T, N), 5, dtype=torch.uint8, device=dev)
    sums = torch.zeros(T, 4, N, device=dev)
    states = torch.zeros(T + 1, N, WORDS, dtype=torch.int32, device=dev)
    assert env._state.shape == (N, WORDS)
    buffer = torch.zeros(T * N * 3 + shift, device=dev)
    actions = buffer[shift:].view(T, N, 3)                                   # the layout of the rollout's action rows
    actions.copy_(torch.from_numpy(ref["actions"]))
    env.reset_into_obs({k: v[0] for k, v in rows.items()})
    states[0].copy_(env._state)
    for t in range(T):
        env.step_into_obs({k: v[t + 1] for k, v in rows.items()}, rew[t], nd[t], actions=actions[t])
        sums[t].copy_(env.measure_sums)
        states[t + 1].copy_(env._state)
    torch.cuda.synchronize()
    return env, {k: v.cpu() for k, v in rows.items()}, rew.cpu(), nd.cpu(), sums.cpu(), states.cpu(), actions


@pytest.mark.parametrize("H,W", [(12, 20), (9, 18)])
@pytest.mark.parametrize("case", B.SCRIPT_CASES, ids=B.case_id)
def test_kernels_bitwise(case, H, W):
    """Every step of the four scripted sequences, 72 steps of 5 envs with max_episode_steps = 36 (at least one reset each): head_rgb,
    head_depth, obj_start_sensor, obj_goal_sensor, is_holding, reward, not_done, the named state words (h, o, picks, invalid, the path
    length and Phi_prev among them) and the four measure sums are equal to the restatement's bit for bit.  The scripts hold components
    outside the Box, non-finite ones and exact halves of c_ang * M (tests/test_nav2d_rearr_vel_host.py asserts the events they reach).
    Both widths put the first pixel of later envs off 16-byte alignment for depth, (9, 18) also has W % 4 != 0."""
    for kind in B.SCRIPTS:
        ref = reference(kind, case, H, W)
        assert ref["dones"].sum() >= B.SCRIPT_ENVS
        _, rows, rew, nd, sums, states, _ = run_device(ref, case, H, W, B.script_seed(kind, case))
        assert_matches(ref, rows, rew, nd, sums, states)
    c = [reference(k, case, H, W)["counters"] for k in B.SCRIPTS]
    assert sum(x["object_visible"] for x in c) > 0 and sum(x["marker_visible"] for x in c) > 0   # the images show what they are there for


GRIPPY = (8, (10, 30, 10), True, True)    # the case of the render checks: K = 8, turns of up to 30 degrees, start_holding, sliding
SMALL = (3, (10, 30, 10), True, False)    # the case of the smaller checks


def test_render_with_several_row_tiles():
    """The launcher gives a workgroup max(4, ceil(4096 / W)) rows, so the shapes above are one tile per env.  70 x 66 is two tiles (63
    and 7 rows) with W % 4 = 2 and tile boundaries off every alignment: 3 envs, 20 steps of the grip-everywhere script, K = 8, all
    outputs bitwise."""
    H, W, N, T = 70, 66, 3, 20
    ref = B.rollout("grip", 5, N, T, max_episode_steps=B.SCRIPT_MAX_EPISODE_STEPS, H=H, W=W, **B.case_kw(GRIPPY))
    assert ref["counters"]["place_ok"] > 0
    _, rows, rew, nd, sums, states, _ = run_device(ref, GRIPPY, H, W, 5)
    assert_matches(ref, rows, rew, nd, sums, states)


def test_render_one_column_many_rows():
    """W = 1 is the shape with the most rows per tile: the launcher caps a tile at 1024 rows, so 4100 x 1 is five tiles (the last of
    4 rows).  2 envs, 3 random steps, all outputs bitwise."""
    H, W, case, N, T = 4100, 1, (3, (10, 30, 10), False, True), 2, 3
    ref = B.rollout("random", 7, N, T, max_episode_steps=B.SCRIPT_MAX_EPISODE_STEPS, H=H, W=W, **B.case_kw(case))
    _, rows, rew, nd, sums, states, _ = run_device(ref, case, H, W, 7)
    assert_matches(ref, rows, rew, nd, sums, states)


@pytest.mark.parametrize("missing", SENSORS + ("images", "all"))
def test_missing_destinations(missing):
    """Each destination NULL in turn, no image at all (nothing is rendered) and no observation destination at all: what is asked for
    is still exact."""
    H, W = 9, 18
    want = tuple(k for k in SENSORS if not (k == missing or (missing == "images" and k in IMAGES) or missing == "all"))
    ref = reference("random", SMALL, H, W)
    _, rows, rew, nd, sums, states, _ = run_device(ref, SMALL, H, W, B.script_seed("random", SMALL), want=want)
    assert set(rows) == set(want)
    assert_matches(ref, rows, rew, nd, sums, states)


@pytest.mark.parametrize("N", [1, 70])
def test_one_env_and_more_than_one_block(N):
    """N = 1 and N = 70 (two workgroups of the step kernel, the second with 6 envs): 12 random steps, all outputs bitwise."""
    H, W, case, T = 9, 18, (3, (10, 30, 10), False, True), 12
    ref = B.rollout("random", 4, N, T, max_episode_steps=6, H=H, W=W, **B.case_kw(case))
    assert ref["actions"].shape == (T, N, 3) and ref["dones"].sum() >= N
    _, rows, rew, nd, sums, states, _ = run_device(ref, case, H, W, 4, max_steps=6)
    assert_matches(ref, rows, rew, nd, sums, states)


def test_action_rows_that_are_only_four_byte_aligned():
    """The action tensor is a view that starts one float into its buffer: with 5 envs the rows of the even steps begin 4 bytes past
    an 8-byte boundary, and within any step two rows in three are not 16-byte aligned.  All outputs bitwise, as from the aligned
    tensor."""
    H, W = 9, 18
    ref = reference("random", SMALL, H, W)
    _, rows, rew, nd, sums, states, actions = run_device(ref, SMALL, H, W, B.script_seed("random", SMALL), shift=1)
    assert actions.data_ptr() % 8 == 4 and actions[2].data_ptr() % 8 == 4 and actions[0, 1].data_ptr() % 8 == 0 and actions.is_contiguous()
    assert_matches(ref, rows, rew, nd, sums, states)


def test_mask_steps_only_the_selected_envs():
    """With the mask selecting envs {1, 3}: state, observations, reward, not_done and measure sums of envs {0, 2, 4} keep every bit,
    and envs {1, 3} get exactly the restatement's step.  Checked through async_step_at / advance_on_device, the subset path of VER
    and the double-buffered sampler."""
    case, H, W, N = GRIPPY, 9, 18, 5
    seed = B.script_seed("grip", case)
    ref = reference("grip", case, H, W)
    env = make_env(N, H, W, seed, case)
    renvs = [B.Nav2DRearrVelEnv(seed, n, H=H, W=W, max_episode_steps=B.SCRIPT_MAX_EPISODE_STEPS, **B.case_kw(case)) for n in range(N)]
    for e in renvs:
        e.reset()
    env.reset()
    for t in range(40):   # all envs, through the host-path protocol, past the first episode ends
        for n in range(N):
            env.async_step_at(n, ref["actions"][t, n])
        assert env.advance_on_device() == list(range(N))
        for n, e in enumerate(renvs):
            e.step(ref["actions"][t, n])
    sel, rest = [1, 3], [0, 2, 4]
    for t in range(40, 56):
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
            assert [env.measure_sums[m, n].item() for m in range(4)] == [float(renvs[n].sums[k]) for k in B.MEASURES]
    assert sum(e.counters["episodes"] for e in renvs) >= N


def test_host_path_observations_and_infos():
    """reset() / step() through the VectorEnv API: the host observations carry the five sensors in observation-space order, equal to
    the restatement's, and the infos of the steps that end an episode carry this task's four measures."""
    case, H, W, N = (3, (10, 30, 10), False, True), 9, 18, 3
    env = make_env(N, H, W, 2, case, max_steps=5)
    renvs = [B.Nav2DRearrVelEnv(2, n, H=H, W=W, max_episode_steps=5, **B.case_kw(case)) for n in range(N)]
    obs = env.reset()
    for n, e in enumerate(renvs):
        o = e.reset()
        assert list(obs[n]) == list(SENSORS) and all(np.array_equal(obs[n][k], o[k]) for k in SENSORS)
    rng, ended = np.random.RandomState(0), 0
    for t in range(12):
        acts = rng.uniform(-1.25, 1.25, size=(N, 3)).astype(np.float32)
        res = env.step(list(acts))
        for n, e in enumerate(renvs):
            o, r, done, info = e.step(acts[n])
            ho, hr, hdone, hinfo = res[n]
            assert all(np.array_equal(ho[k], o[k]) for k in SENSORS) and hr == r and hdone == done
            assert hinfo == info and (not done or list(hinfo) == list(B.MEASURES))
            ended += int(done)
    assert ended >= 2 * N


def test_entry_refusals_are_return_codes():
    """hab_nav2d_rearr_vel_step refuses, with a return code and without a launch: what hab_nav2d_rearr_step refuses (missing state /
    tables, parameters outside their ranges, a step without actions, reward or not_done, an image without its tables or size,
    unaligned depth, a start_holding that is neither 0 nor 1, a width above the maximum, more envs than the render's grid takes), turn
    counts outside Nav2DVel-v0's ranges, and an action pointer that is not 4-byte aligned; one that is 4-byte aligned and no more
    is taken."""
    from habitat_amd import _lib
    from habitat_amd._lib import ptr, stream_ptr
    L = _lib.lib()
    N, H, W = 2, 8, 8
    env = make_env(N, H, W, 1, SMALL)
    env.reset()
    dirs, ray, col_cos, tanv = env._tables
    rows = {k: v[0] for k, v in empty_rows(0, N, H, W, SENSORS).items()}
    act = torch.zeros(N * 3 + 1, device="cuda")
    rew, nd = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    base = dict(state=ptr(env._state), dirs=ptr(dirs), ray=ptr(ray), col_cos=ptr(col_cos), tanv=ptr(tanv), actions=ptr(act), mask=None,
                head_rgb=ptr(rows["head_rgb"]), head_depth=ptr(rows["head_depth"]), obj_start=ptr(rows["obj_start_sensor"]),
                obj_goal=ptr(rows["obj_goal_sensor"]), is_holding=ptr(rows["is_holding"]), reward=ptr(rew), not_done=ptr(nd),
                sums=ptr(env.measure_sums), seed=1, env_offset=0, N=N, H=H, W=W, K=3, nh=36, max_steps=10, start_holding=1, max_turn=3,
                stop_turn=1, min_lin=ctypes.c_float(0.025), sliding=1, advance=1)

    def plus(p, nbytes):
        return ctypes.c_void_p((p.value if isinstance(p, ctypes.c_void_p) else int(p)) + nbytes)

    state = env._state.clone()
    refused = []

    def call(**kw):
        rc = L.hab_nav2d_rearr_vel_step(*dict(base, **kw).values(), stream_ptr())
        if rc != 0:
            refused.append(kw)
        return rc

    ERR_ARG = call(state=None)
    assert ERR_ARG != 0
    for kw in (dict(dirs=None), dict(N=0), dict(nh=0), dict(max_steps=0), dict(K=-1), dict(K=9), dict(actions=None), dict(reward=None),
               dict(not_done=None), dict(ray=None), dict(col_cos=None), dict(tanv=None), dict(H=0), dict(W=0),
               dict(head_rgb=None, tanv=None), dict(head_depth=plus(base["head_depth"], 2)), dict(start_holding=2),
               dict(start_holding=-1), dict(actions=plus(base["actions"], 1)), dict(actions=plus(base["actions"], 2)),
               dict(actions=plus(base["actions"], 3)), dict(max_turn=0), dict(max_turn=-1), dict(max_turn=19), dict(max_turn=6, nh=10),
               dict(stop_turn=0), dict(stop_turn=4)):
        assert call(**kw) == ERR_ARG, kw
    unsupported = call(W=4096)
    assert unsupported not in (0, ERR_ARG) and call(N=70000) == unsupported
    torch.cuda.synchronize()
    assert torch.equal(env._state, state)                     # nothing ran
    assert call() == 0 and call(advance=0, actions=None, reward=None, not_done=None) == 0 and call(start_holding=0) == 0
    assert call(actions=plus(base["actions"], 4)) == 0        # rows that are 4-byte and not 8-byte aligned
    assert call(max_turn=18, stop_turn=18) == 0 and call(sliding=0) == 0
    # what needs no image needs no tables either
    assert call(head_rgb=None, head_depth=None, ray=None, col_cos=None, tanv=None, H=0, W=0) == 0
    assert call(obj_start=None, obj_goal=None, is_holding=None, sums=None) == 0
    torch.cuda.synchronize()
    # the class refuses what is no (N, 3) float32 device tensor
    for bad in (torch.zeros(N, dtype=torch.int64, device="cuda"), torch.zeros(N, 2, device="cuda"), torch.zeros(N, 3),
                torch.zeros(N, 6, device="cuda")[:, ::2], torch.zeros(N, 3, dtype=torch.float64, device="cuda")):
        with pytest.raises(_lib.HabError, match="Nav2DRearrVel"):
            env.step_into_obs({}, rew, nd, actions=bad)
    torch.cuda.synchronize()


# ---- the seams: trainer (device path, host path), VER transport, evaluator -------------------------------------------------------
SIZE = 64
DEFAULTS = (1, 10, 5)


def vel_config(tmp_path, N, T, K=3, params=DEFAULTS, start_holding=False, max_steps=12, seed=100, size=SIZE, hidden=64, extra=()):
    from habitat_amd.config.default import get_config
    turn, max_turn, min_ang = params
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=1000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          f"habitat_baselines.rl.ppo.hidden_size={hidden}", f"habitat_baselines.checkpoint_folder={tmp_path}",
          "habitat_baselines.log_interval=1000", f"habitat_baselines.tensorboard_dir={tmp_path}/tb",
          "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000", "habitat_baselines.trainer_name=ppo",
          f"habitat.environment.max_episode_steps={max_steps}", f"habitat.synthetic.num_obstacles={K}",
          f"habitat.synthetic.turn_angle={turn}", f"habitat.synthetic.max_turn_angle={max_turn}",
          f"habitat.synthetic.min_abs_ang_speed={min_ang}", f"habitat.synthetic.start_holding={start_holding}", f"habitat.seed={seed}"]
    for s in IMAGES:   # head_rgb is added to the file's head_depth, so that all five sensors are in the rollout
        ov += [f"habitat.simulator.sensors.{s}.height={size}", f"habitat.simulator.sensors.{s}.width={size}"]
    return get_config("rearrange/ddppo_nav2d_rearrange_vel.yaml", ov + list(extra))


def restated_envs(cfg, **kw):
    hab = cfg.habitat
    N, size, syn = cfg.habitat_baselines.num_environments, hab.simulator.sensors.head_depth.height, hab.synthetic
    kw = dict(dict(H=size, W=size), **kw)
    envs = [B.Nav2DRearrVelEnv(hab.seed, n, num_obstacles=syn.num_obstacles, turn_angle=syn.turn_angle, max_turn_angle=syn.max_turn_angle,
                               min_abs_lin_speed=syn.min_abs_lin_speed, min_abs_ang_speed=syn.min_abs_ang_speed,
                               allow_sliding=syn.allow_sliding, start_holding=syn.start_holding,
                               max_episode_steps=hab.environment.max_episode_steps, **kw) for n in range(N)]
    return envs, [e.reset() for e in envs]


def assert_actions_vary(actions, renvs):
    """The stored (.., 3) float actions decode to at least 3 distinct turns, to grips of both signs and to both stops and moves: a
    constant action could not pass."""
    e = renvs[0]
    dec = [B.decode(a, e.M) for a in actions.reshape(-1, 3)]
    stops = [bool(l < e.min_lin and abs(dh) < e.S) for l, dh, _, _ in dec]
    assert len({dh for _, dh, _, _ in dec}) >= 3 and any(stops) and not all(stops)
    assert any(g > 0 for _, _, g, _ in dec) and any(g < 0 for _, _, g, _ in dec)


def HostOnlyNav2DRearrVelFactory(**kw):  # the `_target_` of the host-path run
    from habitat_amd.common.env_factory import SyntheticVectorEnvFactory

    class Factory(SyntheticVectorEnvFactory):
        def construct_envs(self, config, workers_ignore_signals=False, enforce_scenes_greater_eq_environments=False, is_first_rank=True,
                           device="cuda", env_offset=0):
            return HostOnlyEnvs(super().construct_envs(config, workers_ignore_signals, enforce_scenes_greater_eq_environments,
                                                       is_first_rank, device=device, env_offset=env_offset))
    return Factory(**kw)


@pytest.mark.parametrize("path", ["device", "host"])
def test_trainer_hands_over_the_stored_action(path, tmp_path):
    """Two update cycles of PPOTrainer from ddppo_nav2d_rearrange_vel.yaml (4 envs, 8 steps, episodes of 12, ResNet18 on head_rgb +
    head_depth at 64 x 64 with the three 1-D sensors fused, the Gaussian head over three components), then the stored float actions
    replayed through the restatement from the same seed: every stored observation (all five sensors, every step), reward and mask is
    equal, bit for bit.  Once on the device path, where the env is given the stored rows themselves, once on the host path, where it
    receives the array clipped to the Box and the rollout keeps the unclipped action.  The window statistics carry the four measures,
    equal to the restatement's sums over the episodes that ended."""
    from habitat_amd.common.env_factory import Nav2DRearrVelVectorEnv
    from habitat_amd.common.spaces import Box
    N, T = 4, 8
    extra = [f"habitat_baselines.vector_env_factory._target_={__name__}.HostOnlyNav2DRearrVelFactory"] if path == "host" else []
    cfg = vel_config(tmp_path, N, T, extra=extra)
    trainer = make_trainer(cfg)
    assert trainer._device_envs == (path == "device") and trainer.envs.consumes_actions
    assert isinstance(getattr(trainer.envs, "_envs", trainer.envs), Nav2DRearrVelVectorEnv)
    policy = trainer._agent.actor_critic
    assert type(policy).__name__ == "PointNavResNetPolicy" and policy.action_distribution_type == "gaussian"
    assert isinstance(trainer._env_spec.action_space, Box) and trainer._env_spec.action_space.shape == (3,)
    renvs, obs = restated_envs(cfg)
    infos, snap, used = [], snapshot_before_update(trainer), []
    for cycle in range(2):
        row0 = trainer._agent.rollouts.buffers["observations"]
        assert set(SENSORS) <= set(row0)
        for n in range(N):  # the row the rollout starts from: the reset, then the last observation of the previous rollout
            assert_obs({k: row0[k][0] for k in SENSORS}, n, obs[n], f"cycle {cycle} row 0 env {n}")
        losses = trainer.run_update_cycle()
        assert all(np.isfinite(v) for v in losses.values())
        assert snap["actions"].dtype == torch.float32 and snap["actions"].shape[-1] == 3
        actions = snap["actions"][:T].cpu().numpy().reshape(T, N, 3)
        rewards, masks = snap["rewards"][:T].cpu().numpy().reshape(T, N), snap["masks"][: T + 1].cpu().numpy().reshape(T + 1, N)
        used.append(actions)
        for t in range(T):
            for n, e in enumerate(renvs):
                o, r, done, info = e.step(actions[t, n])
                assert rewards[t, n] == r, f"reward step {t} env {n}"
                assert bool(masks[t + 1, n]) == (not done), f"mask step {t} env {n}"
                assert_obs({k: snap["observations"][k][t + 1] for k in SENSORS}, n, o, f"cycle {cycle} step {t} env {n}")
                obs[n] = o
                if info:
                    infos.append(info)
    used = np.stack(used)
    assert_actions_vary(used, renvs)
    assert (np.abs(used) > 1).sum() > 0  # the rollout keeps actions outside the Box: they are stored unclipped
    assert len(infos) >= N  # max_episode_steps = 12 < 16 steps: every env ended an episode
    stats = {k: float(v[-1].sum()) for k, v in trainer.window_episode_stats.items()}
    assert stats["count"] == len(infos)
    for k in B.MEASURES:
        assert math.isclose(stats[k], sum(i[k] for i in infos), rel_tol=1e-5, abs_tol=1e-6), k
    trainer.envs.close()


def test_ver_transport_hands_over_the_stored_action(tmp_path):
    """One VERTrainer cycle on the device-resident Nav2DRearrVel source (4 envs, 8 steps, start_holding): in the VER arena the slots
    of an env, ordered by (episode, step), replay through the restatement -- observation of the slot (all five sensors), then its
    stored float action, whose reward is in the same slot and whose mask / next observation are in the env's next slot.  The report
    worker received the measures of the episodes that ended."""
    N, T = 4, 8
    cfg = vel_config(tmp_path, N, T, max_steps=5, start_holding=True,
                     extra=["habitat_baselines.trainer_name=ver", "habitat_baselines.rl.ver.num_inference_workers=1"])
    trainer = make_trainer(cfg, "ver")
    ended = []
    orig = trainer.report_worker.episode_end
    trainer.report_worker.episode_end = lambda d: (ended.append(d), orig(d))[1]
    trainer._agent.pre_rollout()
    trainer.collect_rollout()
    Bf = trainer._agent.rollouts.buffers
    ids = {k: Bf[k].view(-1).cpu().numpy() for k in ("environment_ids", "episode_ids", "step_ids")}
    assert Bf["actions"].dtype == torch.float32
    actions, rewards, masks = Bf["actions"].view(-1, 3).cpu().numpy(), Bf["rewards"].view(-1).cpu().numpy(), Bf["masks"].view(-1).cpu().numpy()
    renvs, obs = restated_envs(cfg)
    flat = {k: Bf["observations"][k].reshape((-1,) + obs[0][k].shape) for k in SENSORS}   # one row per slot of the arena
    checked, ref_infos, used = 0, {}, []
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
            used.append(actions[s])
            assert rewards[s] == r, f"reward env {n} slot {i}"
            if done:
                ref_infos[(n, episode)] = info
                episode += 1
            checked += 1
    assert checked >= N * (T - 1)
    assert_actions_vary(np.array(used), renvs)
    assert len(ended) == len(ref_infos) > 0
    seen = {}
    for d in ended:
        seen[d["env_idx"]] = seen.get(d["env_idx"], -1) + 1
        assert d["info"] == ref_infos[(d["env_idx"], seen[d["env_idx"]])]
    losses = trainer._update_agent()
    assert all(np.isfinite(v) for v in losses.values())
    trainer.shutdown()
    trainer.envs.close()


def test_evaluator_reports_the_measures(tmp_path):
    """A short HabitatEvaluator run with the Gaussian head on the Nav2DRearrVel env: every recorded episode carries success,
    did_pick_object, object_to_goal_distance and collisions, equal to the restatement's for the actions the evaluator handed over --
    length-3 float32 arrays clipped to the Box -- and the aggregate is their mean."""
    from habitat_amd.rl.ppo.evaluator import HabitatEvaluator
    N = 4
    cfg = vel_config(tmp_path, N, 8, max_steps=6, extra=["habitat_baselines.test_episode_count=8"])
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
    assert set(B.MEASURES) | {"reward"} <= set(agg)
    assert all(a.shape == (3,) and a.dtype == np.float32 and np.abs(a).max() <= 1.0 for acts in taken for a in acts)
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
        assert {k: stats[k] for k in B.MEASURES} == {k: w[k] for k in B.MEASURES}, episode_id
        assert math.isclose(stats["reward"], w["reward"], rel_tol=1e-5, abs_tol=1e-6)
    for k in B.MEASURES:
        assert math.isclose(agg[k], float(np.mean([w[k] for w in want.values()])), rel_tol=1e-6, abs_tol=1e-9)
        assert Writer.scalars[f"eval_metrics/{k}"] == agg[k]
    envs.close()


# ---- the loop learns under velocity and grip control ------------------------------------------------------------------------------
LEARN_UPDATES = 100


def test_the_loop_learns_under_velocity_and_grip_control(tmp_path):
    """PPOTrainer with PointNavResNetPolicy (ResNet18, hidden 128, one recurrent layer, the Gaussian head over three components) on
    head_depth + the three fused sensors at 64 x 64: start_holding, K = 0, turn_angle 10 with max_turn_angle 30 and min_abs_ang_speed
    10, sliding, max_episode_steps 48, 32 envs x 32 steps, seed 100, lr 5e-4, 4 epochs x 2 minibatches, clip 0.2, LEARN_UPDATES updates
    (tools/nav2d_rearr_vel_learning.py is the run).  The goal is in no image and the action is continuous, so the return can only rise
    through the fused columns and the Gaussian head.  The family's criterion, as test_the_loop_learns_through_the_fused_sensors
    states it: the per-episode returns of the last 5 updates against the first 5 of the same seed give a two-sample z >= 5 with the
    mean return higher; and the mean final object_to_goal_distance is lower.  Success is printed.
    Measured on one MI355X in one session: tests/test_gpu_nav2d.py::test_the_loop_learns (blind SimpleCNN) 2.45 s, so the budget was
    9.8 s (the discrete sibling's test took 4.46 s there); one run of this tool, read at its line for 100 updates: 4.5 s, return
    0.064 -> 3.54, final object_to_goal_distance 4.13 m -> 0.88 m, z = 18.5, success 0.0 -> 0.065 (z = 16.8 already after 30 updates;
    after 150: 6.7 s, 4.41, 0.62 m, z = 23.4, success 0.225).  Unlike the discrete task, where success stayed 0 within these updates,
    the release and the stop are here one action, (-1, 0, -1), and the policy begins to find it."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "nav2d_rearr_vel_learning", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "nav2d_rearr_vel_learning.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    r = tool.learning_run(str(tmp_path), seed=100, updates=LEARN_UPDATES)
    print("nav2drearrvel learning:", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
    assert r["z"] >= 5.0 and r["return_last"] > r["return_first"] and r["distance_last"] < r["distance_first"], r
