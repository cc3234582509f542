"""GPU: the Nav2DVel-v0 step kernel against its numpy restatement (tests/nav2d_vel_reference.py), bit for bit, and the seams that carry
a continuous action from the Gaussian head to the env: the trainer's device path, its host path, the VER transport and the
evaluator.  The render kernel is Nav2D-v0's and is held by tests/test_gpu_nav2d.py at more shapes; small images suffice here."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import nav2d_vel_reference as V
from test_gpu_nav2d import assert_goal, episode_returns, make_trainer, phi_error_ulps, snapshot_before_update, stacked

pytestmark = pytest.mark.gpu
GOAL = "pointgoal_with_gps_compass"
# phi by the rule of tests/test_gpu_nav2d.py: float64 atan2 of the bitwise float32 (cross, dot), 4 ulp.  The largest error over the
# inputs of test_kernels_bitwise here is printed by it.
PHI_ULPS = 4.0
H, W = 12, 20
DEFAULTS = (1, 10, 5)


def make_env(N, H, W, seed, K, params=DEFAULTS, max_steps=V.SCRIPT_MAX_EPISODE_STEPS, **kw):
    from habitat_amd.common.env_factory import Nav2DVelVectorEnv
    turn, max_turn, min_ang = params
    return Nav2DVelVectorEnv(N, H, W, seed=seed, num_obstacles=K, turn_angle=turn, max_turn_angle=max_turn, min_abs_ang_speed=min_ang,
                             max_episode_steps=max_steps, device="cuda", **kw)


@functools.lru_cache(maxsize=None)
def reference(kind, K, params, H, W, allow_sliding=True):
    return V.script_rollout(kind, K, params, H=H, W=W, allow_sliding=allow_sliding)


def run_device(ref, K, params, H, W, seed, want=("rgb", "depth", GOAL), actions=None, **kw):
    """Replays ref's actions on the device, every step written straight into its own row of separately allocated (T + 1, N, ...)
    tensors, the actions as (T, N, 2) float rows, like a rollout arena."""
    actions = ref["actions"] if actions is None else actions
    T, N = actions.shape[:2]
    env = make_env(N, H, W, seed, K, params, **kw)
    dev = "cuda"
    rows = {}
    if "rgb" in want:
        rows["rgb"] = torch.full((T + 1, N, H, W, 3), 7, dtype=torch.uint8, device=dev)
    if "depth" in want:
        rows["depth"] = torch.full((T + 1, N, H, W, 1), -1.0, device=dev)
    if GOAL in want:
        rows[GOAL] = torch.full((T + 1, N, 2), -9.0, device=dev)
    rew = torch.full((T, N), 99.0, device=dev)
    nd = torch.full((T, N), 5, dtype=torch.uint8, device=dev)
    sums = torch.zeros(T, 4, N, device=dev)
    acts = torch.from_numpy(actions).to(dev)
    env.reset_into_obs({k: v[0] for k, v in rows.items()})
    for t in range(T):
        env.step_into_obs({k: v[t + 1] for k, v in rows.items()}, rew[t], nd[t], actions=acts[t])
        sums[t].copy_(env.measure_sums)
    torch.cuda.synchronize()
    return env, {k: v.cpu() for k, v in rows.items()}, rew.cpu(), nd.cpu(), sums.cpu()


def assert_matches(ref, rows, rew, nd, sums):
    worst = 0.0
    if "rgb" in rows:
        assert torch.equal(rows["rgb"], torch.from_numpy(stacked(ref, "rgb"))), "rgb"
    if "depth" in rows:
        assert torch.equal(rows["depth"], torch.from_numpy(stacked(ref, "depth"))), "depth"
    if GOAL in rows:
        g = stacked(ref, GOAL)
        assert torch.equal(rows[GOAL][..., 0], torch.from_numpy(g[..., 0])), "rho"
        worst = phi_error_ulps(rows[GOAL][..., 1].numpy(), stacked(ref, "cross_dot"))
    assert torch.equal(rew, torch.from_numpy(ref["rewards"])), "reward"
    assert torch.equal(nd, torch.from_numpy((~ref["dones"]).astype(np.uint8))), "not_done"
    assert torch.equal(sums, torch.from_numpy(ref["sums"])), "measure sums"
    return worst


@pytest.mark.parametrize("K,params", V.SCRIPT_CASES)
def test_kernels_bitwise(K, params):
    """Every step of the four scripted sequences, 60 steps of 5 envs with max_episode_steps = 12, 12 x 20 rgb + depth: rgb, depth, rho,
    reward, not_done and the four measure sums are equal to the restatement's bit for bit; phi within PHI_ULPS."""
    worst = 0.0
    for kind in V.SCRIPTS:
        ref = reference(kind, K, params, H, W)
        _, rows, rew, nd, sums = run_device(ref, K, params, H, W, V.script_seed(kind, K, params))
        worst = max(worst, assert_matches(ref, rows, rew, nd, sums))
    print(f"nav2dvel phi: largest error {worst:.3f} ulp (K={K}, params={params})")
    assert worst <= PHI_ULPS


def test_kernel_bitwise_without_images():
    """No sensor size at all (H = W = 0, the blind env): nothing is rendered, everything else is exact."""
    K, params = 8, (5, 30, 10)
    ref = reference("grid", K, params, 0, 0)
    env, rows, rew, nd, sums = run_device(ref, K, params, 0, 0, V.script_seed("grid", K, params), want=(GOAL,), use_rgb=False, use_depth=False)
    assert set(env.observation_spaces[0].spaces) == {GOAL}
    assert assert_matches(ref, rows, rew, nd, sums) <= PHI_ULPS


def test_sliding_off():
    K, params = 8, DEFAULTS
    ref = reference("random", K, params, H, W, allow_sliding=False)
    assert ref["counters"]["blocked"] > 0 and ref["counters"]["slide_x"] == ref["counters"]["slide_y"] == 0
    _, rows, rew, nd, sums = run_device(ref, K, params, H, W, V.script_seed("random", K, params), allow_sliding=False)
    assert assert_matches(ref, rows, rew, nd, sums) <= PHI_ULPS
    assert not np.array_equal(ref["rewards"], reference("random", K, params, H, W)["rewards"])  # the switch matters on this case


@pytest.mark.parametrize("want", [("depth", GOAL), ("rgb", GOAL), (GOAL,)])
def test_missing_destinations(want):
    """No rgb, no depth, the goal sensor only: what is asked for is still exact."""
    K, params = 3, (5, 30, 10)
    ref = reference("random", K, params, H, W)
    _, rows, rew, nd, sums = run_device(ref, K, params, H, W, V.script_seed("random", K, params), want=want)
    assert set(rows) == set(want)
    assert assert_matches(ref, rows, rew, nd, sums) <= PHI_ULPS


def test_non_finite_and_out_of_range_components():
    """A direct call with NaN, +inf, -inf and +-3.0 components: a non-finite component acts as 0, the others are clamped, exactly as
    in the restatement."""
    K, params, N = 3, DEFAULTS, 8
    nan, inf = np.nan, np.inf
    table = np.array([[nan, 0.5], [0.5, nan], [inf, -0.3], [0.2, inf], [-inf, -inf], [3.0, -3.0], [-3.0, 3.0], [nan, nan], [3.0, 0.05],
                      [-3.0, 0.0]], np.float32)
    rng = np.random.RandomState(0)
    actions = table[rng.randint(0, len(table), size=(24, N))]
    seed = 3
    renvs = [V.Nav2DVelEnv(seed, n, H=H, W=W, num_obstacles=K, max_episode_steps=V.SCRIPT_MAX_EPISODE_STEPS) for n in range(N)]
    ref = dict(obs=[[e.reset() for e in renvs]], rewards=np.zeros((24, N), np.float32), dones=np.zeros((24, N), bool),
               sums=np.zeros((24, 4, N), np.float32))
    for t in range(24):
        res = [e.step(a) for e, a in zip(renvs, actions[t])]
        ref["obs"].append([r[0] for r in res])
        ref["rewards"][t], ref["dones"][t] = [r[1] for r in res], [r[2] for r in res]
        ref["sums"][t] = [[e.sums[k] for e in renvs] for k in V.MEASURES]
    assert sum(e.counters["stops"] for e in renvs) > 0 and sum(e.counters["clamped"] for e in renvs) > 0
    _, rows, rew, nd, sums = run_device(ref, K, params, H, W, seed, actions=actions)
    assert assert_matches(ref, rows, rew, nd, sums) <= PHI_ULPS


def test_mask_steps_only_the_selected_envs():
    """With the mask selecting envs {1, 3}: state, observations, reward, not_done and measure sums of envs {0, 2, 4} keep every bit,
    and envs {1, 3} get exactly the restatement's step, through async_step_at / advance_on_device."""
    K, params, N = 8, DEFAULTS, 5
    seed = V.script_seed("random", K, params)
    ref = reference("random", K, params, H, W)
    env = make_env(N, H, W, seed, K, params)
    renvs = [V.Nav2DVelEnv(seed, n, H=H, W=W, num_obstacles=K, max_episode_steps=V.SCRIPT_MAX_EPISODE_STEPS) for n in range(N)]
    for e in renvs:
        e.reset()
    env.reset()
    for t in range(14):
        for n in range(N):
            env.async_step_at(n, ref["actions"][t, n])
        assert env.advance_on_device() == list(range(N))
        for n, e in enumerate(renvs):
            e.step(ref["actions"][t, n])
    sel, rest = [1, 3], [0, 2, 4]
    for t in range(14, 30):
        before = dict(state=env._state.clone(), rew=env._rew.clone(), nd=env._nd.clone(), sums=env.measure_sums.clone(),
                      **{k: v.clone() for k, v in env._own_obs().items()})
        for n in sel:
            env.async_step_at(n, {"action": ref["actions"][t, n]})
        assert env.advance_on_device() == sel
        after = dict(state=env._state, rew=env._rew, nd=env._nd, sums=env.measure_sums, **env._own_obs())
        for k, v in after.items():
            a, b = (v[:, rest], before[k][:, rest]) if k == "sums" else (v[rest], before[k][rest])
            assert torch.equal(a, b), f"step {t}: {k} of an unselected env changed"
        for n in sel:
            o, r, done, _ = renvs[n].step(ref["actions"][t, n])
            assert torch.equal(env._rgb[n].cpu(), torch.from_numpy(o["rgb"])) and torch.equal(env._depth[n].cpu(), torch.from_numpy(o["depth"]))
            assert env._goal[n, 0].item() == o[GOAL][0] and env._rew[n].item() == r and bool(env._nd[n].item()) == (not done)
            assert [env.measure_sums[m, n].item() for m in range(4)] == [float(renvs[n].sums[k]) for k in V.MEASURES]
    assert sum(e.counters["episodes"] for e in renvs) > N


def test_entry_point_refusals():
    """Return codes of hab_nav2d_vel_step; each of these returns before anything is launched."""
    from habitat_amd import _lib
    from habitat_amd._lib import ptr
    N = 4
    env = make_env(N, 0, 0, 1, 0, use_rgb=False, use_depth=False)
    dirs = env._tables[0]
    acts = torch.zeros(N + 1, 2, device="cuda")
    rew, nd = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    state = env._state.clone()

    def call(actions, max_turn=10, stop_turn=5, nh=360, advance=1):
        return _lib.lib().hab_nav2d_vel_step(ptr(env._state), ptr(dirs), None, None, None, actions,
                                             None, None, None, None, ptr(rew), ptr(nd), None, 1, 0, N, 0, 0, 0, nh, 12, max_turn, stop_turn,
                                             ctypes.c_float(0.025), 1, advance, _lib.stream_ptr())
    ok = ptr(acts)
    assert call(None) == -1                                   # null actions on advance
    assert call(ctypes.c_void_p(ok.value + 4)) == -1          # a row must be 8-byte aligned
    for m in (0, -1, 181, 360):
        assert call(ok, max_turn=m) == -1                     # max_turn_steps outside 1 .. num_headings / 2
    assert call(ok, max_turn=6, nh=10) == -1
    for s in (0, 11):
        assert call(ok, stop_turn=s) == -1                    # stop_turn_steps outside 1 .. max_turn_steps
    torch.cuda.synchronize()
    assert torch.equal(env._state, state)                     # nothing ran
    assert call(None, advance=0) == 0 and call(ok) == 0 and call(ok, max_turn=180, stop_turn=180) == 0
    with pytest.raises(_lib.HabError):
        env.step_into_obs({}, rew, nd, actions=torch.zeros(N, dtype=torch.int64, device="cuda"))
    with pytest.raises(_lib.HabError):
        env.step_into_obs({}, rew, nd, actions=acts[:N, :1])
    with pytest.raises(_lib.HabError):
        env.step_into_obs({}, rew, nd, actions=torch.zeros(N, 2))
    torch.cuda.synchronize()


# ---- the seams: trainer (device path, host path), VER transport, evaluator -------------------------------------------------------
SIZE = 64  # what the cube-map trainer test runs ResNet18 at


def vel_config(tmp_path, N, T, K=3, params=DEFAULTS, max_steps=12, seed=100, size=SIZE, hidden=64, extra=()):
    from habitat_amd.config.default import get_config
    turn, max_turn, min_ang = params
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=1000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          f"habitat_baselines.rl.ppo.hidden_size={hidden}", f"habitat_baselines.checkpoint_folder={tmp_path}",
          "habitat_baselines.log_interval=1000", f"habitat_baselines.tensorboard_dir={tmp_path}/tb",
          "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000",
          f"habitat.environment.max_episode_steps={max_steps}", f"habitat.synthetic.num_obstacles={K}",
          f"habitat.synthetic.turn_angle={turn}", f"habitat.synthetic.max_turn_angle={max_turn}",
          f"habitat.synthetic.min_abs_ang_speed={min_ang}", f"habitat.seed={seed}"]
    for s in ("rgb", "depth"):
        ov += [f"habitat.simulator.sensors.{s}.height={size}", f"habitat.simulator.sensors.{s}.width={size}"]
    return get_config("pointnav/ppo_nav2d_vel.yaml", ov + list(extra))


def restated_envs(cfg, **kw):
    hab = cfg.habitat
    N, size, syn = cfg.habitat_baselines.num_environments, hab.simulator.sensors.depth.height, hab.synthetic
    kw = dict(dict(H=size, W=size, use_rgb=False), **kw)  # the replays compare depth rows; rgb is held bitwise by the kernel tests
    envs = [V.Nav2DVelEnv(hab.seed, n, num_obstacles=syn.num_obstacles, turn_angle=syn.turn_angle, max_turn_angle=syn.max_turn_angle,
                          min_abs_lin_speed=syn.min_abs_lin_speed, min_abs_ang_speed=syn.min_abs_ang_speed,
                          allow_sliding=syn.allow_sliding, max_episode_steps=hab.environment.max_episode_steps, **kw) for n in range(N)]
    return envs, [e.reset() for e in envs]


def assert_actions_vary(actions, renvs):
    """The stored (.., 2) float actions decode to at least 3 distinct turns and to both stops and moves, and are not clipped."""
    e = renvs[0]
    dec = [V.decode(a, e.M) for a in actions.reshape(-1, 2)]
    stops = [bool(l < e.min_lin and abs(dh) < e.S) for _, _, l, dh, _ in dec]
    assert len({dh for _, _, _, dh, _ in dec}) >= 3 and any(stops) and not all(stops)


def replay_rollout(B, T, renvs, obs0, depth_steps):
    """Replays the stored float actions of one (T + 1, N) rollout through the restatement, which stands at `obs0`: for every step the
    stored reward, mask and goal sensor (and the depth row at `depth_steps`) must be what the restatement returns for the STORED
    action of that step."""
    N = len(renvs)
    actions = B["actions"][:T].cpu().numpy().reshape(T, N, 2)
    assert actions.dtype == np.float32
    rewards, masks = B["rewards"][:T].cpu().numpy().reshape(T, N), B["masks"][: T + 1].cpu().numpy().reshape(T + 1, N)
    goal, depth = B["observations"][GOAL][: T + 1].cpu(), B["observations"]["depth"][: T + 1].cpu()
    obs, infos = list(obs0), []
    assert_actions_vary(actions, renvs)
    for t in range(T):
        for n, e in enumerate(renvs):
            o, r, done, info = e.step(actions[t, n])
            assert rewards[t, n] == r, f"reward step {t} env {n}"
            assert bool(masks[t + 1, n]) == (not done), f"mask step {t} env {n}"
            assert_goal(goal[t + 1, n], o, f"goal step {t} env {n}")
            if t in depth_steps:
                assert torch.equal(depth[t + 1, n], torch.from_numpy(o["depth"])), f"depth step {t} env {n}"
            obs[n] = o
            if info:
                infos.append(info)
    return obs, infos


class HostOnlyEnvs:
    """A Nav2DVel env that shows the VectorEnv API only, so that the trainer takes its host path (async_step_at / wait_step_at)."""

    def __init__(self, envs):
        self._envs = envs

    def __getattr__(self, k):
        if k in ("step_into_obs", "reset_into_obs", "step_into", "reset_into", "measure_sums", "advance_on_device"):
            raise AttributeError(k)
        return getattr(self._envs, k)


def HostOnlyNav2DVelFactory(**kw):  # the `_target_` of the host-path run
    from habitat_amd.common.env_factory import SyntheticVectorEnvFactory

    class Factory(SyntheticVectorEnvFactory):
        def construct_envs(self, config, workers_ignore_signals=False, enforce_scenes_greater_eq_environments=False, is_first_rank=True,
                           device="cuda", env_offset=0):
            return HostOnlyEnvs(super().construct_envs(config, workers_ignore_signals, enforce_scenes_greater_eq_environments,
                                                       is_first_rank, device=device, env_offset=env_offset))
    return Factory(**kw)


@pytest.mark.parametrize("path", ["device", "host"])
def test_trainer_hands_over_the_stored_action(path, tmp_path):
    """Two update cycles of PPOTrainer from ppo_nav2d_vel.yaml (8 envs, 16 steps, episodes of 12, ResNet18 with the Gaussian head at
    64 x 64), then the stored float actions replayed through the restatement from the same seed: stored rewards, masks, goal sensor
    and the depth rows of steps 0, 7 and 15 are equal.  Once on the device path, once on the host path, where the env receives the
    clipped array and the rollout keeps the unclipped action."""
    from habitat_amd.common.env_factory import Nav2DVelVectorEnv
    from habitat_amd.common.spaces import Box
    N, T = 8, 16
    extra = [f"habitat_baselines.vector_env_factory._target_={__name__}.HostOnlyNav2DVelFactory"] if path == "host" else []
    trainer = make_trainer(cfg := vel_config(tmp_path, N, T, extra=extra))
    assert trainer._device_envs == (path == "device") and trainer.envs.consumes_actions
    assert isinstance(trainer.envs._envs if path == "host" else trainer.envs, Nav2DVelVectorEnv)
    assert isinstance(trainer._env_spec.action_space, Box) and trainer._agent.actor_critic.action_distribution_type == "gaussian"
    renvs, obs = restated_envs(cfg)
    infos, snap, beyond = [], snapshot_before_update(trainer), 0
    for cycle in range(2):
        row0 = trainer._agent.rollouts.buffers["observations"]
        for n in range(N):
            assert_goal(row0[GOAL][0, n], obs[n], f"cycle {cycle} row 0 env {n}")
            assert torch.equal(row0["depth"][0, n].cpu(), torch.from_numpy(obs[n]["depth"])), f"cycle {cycle} row 0 depth env {n}"
        losses = trainer.run_update_cycle()
        assert all(np.isfinite(v) for v in losses.values())
        obs, got = replay_rollout(snap, T, renvs, obs, depth_steps=(0, 7, 15))
        infos += got
        beyond += int((snap["actions"][:T].abs() > 1).sum())
    assert beyond > 0  # the rollout keeps actions outside the Box: they are stored unclipped
    assert len(infos) >= N
    stats = {k: float(v[-1].sum()) for k, v in trainer.window_episode_stats.items()}
    assert stats["count"] == len(infos)
    for k in V.MEASURES:
        assert math.isclose(stats[k], sum(i[k] for i in infos), rel_tol=1e-5, abs_tol=1e-6), k
    trainer.envs.close()


def test_ver_transport_hands_over_the_stored_action(tmp_path):
    """One VERTrainer rollout on the device-resident Nav2DVel source: in the VER arena the slots of an env, ordered by (episode, step),
    replay through the restatement -- observation of the slot, then its stored float action, whose reward is in the same slot and
    whose mask / next observation are in the env's next slot."""
    N, T = 8, 16
    cfg = vel_config(tmp_path, N, T, extra=["habitat_baselines.trainer_name=ver", "habitat_baselines.rl.ver.num_inference_workers=1"])
    trainer = make_trainer(cfg, "ver")
    trainer._agent.pre_rollout()
    trainer.collect_rollout()
    B = trainer._agent.rollouts.buffers
    ids = {k: B[k].view(-1).cpu().numpy() for k in ("environment_ids", "episode_ids", "step_ids")}
    actions, rewards, masks = B["actions"].view(-1, 2).cpu().numpy(), B["rewards"].view(-1).cpu().numpy(), B["masks"].view(-1).cpu().numpy()
    goal = B["observations"][GOAL].view(-1, 2).cpu()
    depth = B["observations"]["depth"].view(-1, SIZE, SIZE, 1).cpu()
    renvs, obs = restated_envs(cfg)
    checked, used = 0, []
    for n, e in enumerate(renvs):
        slots = sorted(np.nonzero(ids["environment_ids"] == n)[0], key=lambda s: (ids["episode_ids"][s], ids["step_ids"][s]))
        assert len(slots) >= 2
        o, done, episode = obs[n], True, 0   # the first observation comes with mask False
        for i, s in enumerate(slots):
            assert ids["episode_ids"][s] == episode and bool(masks[s]) == (not done), (n, i)
            assert_goal(goal[s], o, f"env {n} slot {i}")
            assert torch.equal(depth[s], torch.from_numpy(o["depth"])), f"depth env {n} slot {i}"
            if i + 1 == len(slots):
                break  # the reward of the last slot arrives with the next rollout
            o, r, done, _ = e.step(actions[s])
            used.append(actions[s])
            assert rewards[s] == r, f"reward env {n} slot {i}"
            episode += int(done)
            checked += 1
    assert checked >= N * (T - 1)
    assert_actions_vary(np.array(used), renvs)
    losses = trainer._update_agent()
    assert all(np.isfinite(v) for v in losses.values())
    trainer.shutdown()
    trainer.envs.close()


def test_evaluator_reports_the_measures(tmp_path):
    """A short HabitatEvaluator run with the Gaussian head on the (blind) Nav2DVel env: every recorded episode carries the four
    measures, equal to the restatement's for the actions the evaluator handed over -- arrays clipped to the Box."""
    from habitat_amd.rl.ppo.evaluator import HabitatEvaluator
    N = 4
    cfg = vel_config(tmp_path, N, 8, K=8, extra=["habitat_baselines.test_episode_count=10", "habitat_baselines.vector_env_factory.use_rgb=False",
                                                 "habitat_baselines.vector_env_factory.use_depth=False"])
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
    assert set(V.MEASURES) | {"reward"} <= set(agg)
    assert all(a.shape == (2,) and a.dtype == np.float32 and np.abs(a).max() <= 1.0 for acts in taken for a in acts)
    assert any(np.abs(a).max() == 1.0 for acts in taken for a in acts)  # N(0, 1) draws: some were clipped
    renvs, _ = restated_envs(cfg, H=0, W=0, use_depth=False)
    want, ret = {}, [0.0] * N
    for acts in taken:
        for n, e in enumerate(renvs):
            episode = e.episode
            _, r, done, info = e.step(acts[n])
            ret[n] += float(r)
            if done:
                want[f"{n}:{episode}"] = dict(info, reward=ret[n])
                ret[n] = 0.0
    assert len(ev.last_stats_episodes) >= 10 and len(ev.last_stats_episodes) == len(want)
    for ((scene, episode_id), count), stats in ev.last_stats_episodes.items():
        assert scene == "nav2d" and count == 1
        w = want[episode_id]
        assert {k: stats[k] for k in V.MEASURES} == {k: w[k] for k in V.MEASURES}, episode_id
        assert math.isclose(stats["reward"], w["reward"], rel_tol=1e-5, abs_tol=1e-6)
    for k in V.MEASURES:
        assert math.isclose(agg[k], float(np.mean([w[k] for w in want.values()])), rel_tol=1e-6, abs_tol=1e-9)
    envs.close()


# ---- the loop learns ---------------------------------------------------------------------------------------------------------------
LEARN_UPDATES = 100
LEARN_PARAMS = (5, 30, 10)   # turn_angle, max_turn_angle, min_abs_ang_speed
LEARN_MAX_STEPS = 48
LEARN_HIDDEN = 64
LEARN_PPO = ("habitat_baselines.rl.ppo.lr=1.0e-3", "habitat_baselines.rl.ppo.ppo_epoch=4", "habitat_baselines.rl.ppo.num_mini_batch=2",
             "habitat_baselines.rl.ppo.clip_param=0.2")


def learning_run(tmp_path, seed, updates=LEARN_UPDATES, ppo=LEARN_PPO, params=LEARN_PARAMS, max_steps=LEARN_MAX_STEPS, hidden=LEARN_HIDDEN):
    N, T = 32, 32
    cfg = vel_config(tmp_path, N, T, K=0, params=params, max_steps=max_steps, seed=seed, hidden=hidden,
                     extra=["habitat_baselines.vector_env_factory.use_rgb=False", "habitat_baselines.vector_env_factory.use_depth=False",
                            *ppo])
    trainer = make_trainer(cfg)
    assert set(trainer.envs.observation_spaces[0].spaces) == {GOAL}  # no image sensors: the blind PointNavResNetPolicy
    assert trainer._agent.actor_critic.action_distribution_type == "gaussian"
    carry, per_update, B = np.zeros(N), [], snapshot_before_update(trainer)
    for _ in range(updates):
        trainer.run_update_cycle()
        per_update.append(episode_returns(B["rewards"][:T].cpu().numpy().reshape(T, N).astype(np.float64),
                                          B["masks"][: T + 1].cpu().numpy().reshape(T + 1, N).astype(bool), carry))
    trainer.envs.close()
    first = np.array([e for u in per_update[:5] for e in u])
    last = np.array([e for u in per_update[-5:] for e in u])
    z = (last[:, 0].mean() - first[:, 0].mean()) / math.sqrt(first[:, 0].var(ddof=1) / len(first) + last[:, 0].var(ddof=1) / len(last))
    return dict(seed=seed, updates=updates, episodes_first=len(first), episodes_last=len(last), return_first=first[:, 0].mean(),
                return_last=last[:, 0].mean(), success_first=first[:, 1].mean(), success_last=last[:, 1].mean(), z=z)


def test_the_loop_learns(tmp_path):
    """PPOTrainer on the blind PointNavResNetPolicy (no image sensors, hidden 64) with the Gaussian head in the YAML's action_dist
    options, Nav2DVel-v0 with K = 0, turn_angle 5, max_turn_angle 30, min_abs_ang_speed 10, max_episode_steps 48, 32 envs x 32 steps,
    lr 1e-3, 4 epochs, 2 mini-batches, clip 0.2, seed 100, LEARN_UPDATES updates.  The per-episode returns of the last 5 updates
    against those of the first 5 of the same run: two-sample z >= 5, mean return and mean success both higher at the end (measured
    for the seeds 100, 101, 102: z = 46.4, 41.7, 38.8; success 0.00 -> 0.96, 0.01 -> 0.97, 0.00 -> 0.92)."""
    r = learning_run(tmp_path, 100)
    print("nav2dvel learning:", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
    assert r["z"] >= 5.0 and r["return_last"] > r["return_first"] and r["success_last"] > r["success_first"], r
