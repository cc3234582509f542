"""GPU: the Nav2DExplore-v0 kernel against the numpy restatement (tests/nav2d_explore_reference.py), bit for bit on every output --
rgb, depth, gps, compass, reward, not-done, the whole record, the measure sums and the whole coverage layer -- the cross-check of the
layer against the top-down map's fog of war, the entry's refusals, and the seams that carry the task: the trainer's device path, its
host path, the VER transport, the evaluator and the video frames."""
import functools
import math

import numpy as np
import pytest
import torch

import nav2d_explore_reference as X
import nav2d_map_reference as M
from test_gpu_nav2d import make_trainer

pytestmark = pytest.mark.gpu
SENSORS = ("rgb", "depth", "gps", "compass")
IMAGES = ("rgb", "depth")
F = np.float32


def make_env(N, H, W, seed, K=3, turn=10, G=64, vis=3.0, max_steps=X.SCRIPT_MAX_EPISODE_STEPS, **kw):
    from habitat_amd.common.env_factory import Nav2DExploreVectorEnv
    kw = dict(dict(use_rgb=H > 0, use_depth=H > 0), **kw)
    return Nav2DExploreVectorEnv(N, H, W, seed=seed, num_obstacles=K, turn_angle=turn, max_episode_steps=max_steps, coverage_resolution=G,
                                 visibility_dist=vis, device="cuda", **kw)


def stacked(ref, key):
    return np.stack([np.stack([o[key] for o in row]) for row in ref["obs"]])  # (T + 1, N, ...)


def empty_rows(T, N, H, W, want, dev="cuda"):
    shapes = dict(rgb=((H, W, 3), torch.uint8, 7), depth=((H, W, 1), torch.float32, -1.0), gps=((2,), torch.float32, -9.0),
                  compass=((1,), torch.float32, -9.0))
    return {k: torch.full((T + 1, N) + shapes[k][0], shapes[k][2], dtype=shapes[k][1], device=dev) for k in want}


def run_device(ref, env, want=SENSORS, masks=None):
    """Replays ref's actions on the device, every step written straight into its own row of separately allocated (T + 1, N, ...)
    tensors, like a rollout arena; the records and the layers are copied after the reset and after every step."""
    T, N = ref["actions"].shape
    dev, G = "cuda", env.coverage_resolution
    rows = empty_rows(T, N, env.H, env.W, want)
    rew = torch.full((T, N), 99.0, device=dev)
    nd = torch.full((T, N), 5, dtype=torch.uint8, device=dev)
    sums = torch.zeros(T, 4, N, device=dev)
    states = torch.zeros(T + 1, N, X.STATE_WORDS, dtype=torch.int32, device=dev)
    layers = torch.zeros(T + 1, N, G, G, dtype=torch.uint8, device=dev)
    actions = torch.from_numpy(ref["actions"]).to(dev).unsqueeze(-1)       # (T, N, 1), the layout of the rollout's action rows
    env.reset_into_obs({k: v[0] for k, v in rows.items()})
    states[0].copy_(env._state)
    layers[0].copy_(env.coverage())
    for t in range(T):
        env.step_into_obs({k: v[t + 1] for k, v in rows.items()}, rew[t], nd[t], actions=actions[t],
                          mask=None if masks is None else masks[t])
        sums[t].copy_(env.measure_sums)
        states[t + 1].copy_(env._state)
        layers[t + 1].copy_(env.coverage())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in rows.items()}, rew.cpu(), nd.cpu(), sums.cpu(), states.cpu(), layers.cpu()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_matches(ref, rows, rew, nd, sums, states, layers):
    for k, v in rows.items():
        exp = torch.from_numpy(stacked(ref, k))
        assert v.dtype == exp.dtype and v.shape == exp.shape, k
        assert torch.equal(bits(v), bits(exp)), k
    assert torch.equal(bits(rew), bits(torch.from_numpy(ref["rewards"]))), "reward"
    assert torch.equal(nd, torch.from_numpy((~ref["dones"]).astype(np.uint8))), "not_done"
    assert torch.equal(bits(sums), bits(torch.from_numpy(ref["sums"]))), "measure sums"
    assert torch.equal(states, torch.from_numpy(np.stack(ref["records"]))), "records"
    assert torch.equal(layers, torch.from_numpy(np.stack(ref["layers"]))), "coverage layers"


def replay(ref, seed, K, turn, G, vis, H, W, want=SENSORS, prepare=None, **kw):
    env = make_env(ref["actions"].shape[1], H, W, seed, K=K, turn=turn, G=G, vis=vis, **kw)
    if prepare:
        prepare(env)
    assert_matches(ref, *run_device(ref, env, want=tuple(k for k in want if H > 0 or k not in IMAGES)))
    return env


@pytest.mark.parametrize("kind", X.SCRIPTS)
@pytest.mark.parametrize("case", X.SCRIPT_CASES, ids=lambda c: "K{}-turn{}".format(*c))
def test_kernels_bitwise(case, kind):
    """Every step of a scripted sequence, 60 steps of 5 envs with max_episode_steps = 12 (several rollovers each): every output is
    equal to the restatement's bit for bit.  The (G, visibility_dist, image size) of a run go round X.FORMS: G = 30 makes rows
    straddle the words of the sweep, 9 x 18 leaves image rows unaligned, visibility 1.0 makes the bounding box a small part of the
    layer."""
    ref = X.script_rollout(kind, case)
    G, vis, (H, W) = X.script_form(kind, case)
    assert ref["dones"].sum() >= X.SCRIPT_ENVS * 4 and ref["news"].max() > 0
    replay(ref, X.script_seed(kind, case), case[0], case[1], G, vis, H, W, use_rgb=True)


@functools.lru_cache(maxsize=None)
def small(N=5, T=30, G=30, vis=3.0, H=9, W=18, K=8, turn=30, seed=2, kind="random", use_rgb=True):
    return X.rollout(kind, seed, N, T, turn_angle=turn, num_obstacles=K, coverage_resolution=G, visibility_dist=vis,
                     max_episode_steps=X.SCRIPT_MAX_EPISODE_STEPS, H=H, W=W, use_rgb=use_rgb)


@pytest.mark.parametrize("G", [16, 30, 64, 33])
def test_byte_path(G):
    """A layer pointer offset by one byte takes the byte path at every G; G = 33 (G * G odd) takes it at any alignment."""
    ref = small(G=G, H=0, W=0)

    def offset(env):
        N = env.num_envs
        buf = torch.zeros(N * G * G + (0 if G == 33 else 1), dtype=torch.uint8, device="cuda")
        env._coverage = buf[buf.numel() - N * G * G:].view(N, G, G)
        assert env._coverage.data_ptr() % 4 == (0 if G == 33 else 1)
    replay(ref, 2, 8, 30, G, 3.0, 0, 0, prepare=offset)


def test_render_with_several_row_tiles():
    """70 x 66 is two tiles of the render (63 and 7 rows) with W % 4 = 2: 3 envs, 20 random steps, all outputs bitwise."""
    ref = small(N=3, T=20, G=16, H=70, W=66, seed=5)
    replay(ref, 5, 8, 30, 16, 3.0, 70, 66, use_rgb=True)


@pytest.mark.parametrize("missing", SENSORS + ("images", "all"))
def test_missing_destinations(missing):
    """Each destination NULL in turn, no image at all (nothing is rendered) and no observation destination at all: what is asked for
    is still exact, and so are reward, record and layer."""
    want = tuple(k for k in SENSORS if not (k == missing or (missing == "images" and k in IMAGES) or missing == "all"))
    replay(small(), 2, 8, 30, 30, 3.0, 9, 18, want=want, use_rgb=True)


@pytest.mark.parametrize("N", [1, 70])
def test_env_counts(N):
    ref = small(N=N, T=14, G=30 if N == 1 else 16, vis=1.0)
    replay(ref, 2, 8, 30, 30 if N == 1 else 16, 1.0, 9, 18, use_rgb=True)


def test_a_large_layer_and_an_unbounded_visibility():
    """G = 512 (64 words per thread at a beginning) with a visibility far beyond the arena: the bounding box is the whole layer."""
    ref = small(N=2, T=6, G=512, vis=1.0e18, H=0, W=0, K=3)
    replay(ref, 2, 3, 30, 512, 1.0e18, 0, 0)


def test_mask_leaves_unselected_envs_untouched():
    """Steps 3..8 leave every third env unstepped while its neighbours' episodes end: its layer, record, rows, reward and not-done byte
    keep what they held, and the stepped envs match a restatement that skips the same steps."""
    N, T, G = 7, 14, 30
    envs = [X.Nav2DExploreEnv(3, n, H=9, W=18, num_obstacles=3, turn_angle=30, coverage_resolution=G, visibility_dist=2.0,
                              max_episode_steps=4) for n in range(N)]
    env = make_env(N, 9, 18, 3, K=3, turn=30, G=G, vis=2.0, max_steps=4)
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
        assert np.array_equal(env.coverage().cpu().numpy(), np.stack([e.layer for e in envs])), t
        assert np.array_equal(rew.cpu().numpy().view(np.int32), want_rew.view(np.int32)) and np.array_equal(nd.cpu().numpy(), want_nd)
        for k in ("depth", "gps", "compass"):
            assert np.array_equal(rows[k].cpu().numpy().reshape(N, -1), np.stack([o[k].reshape(-1) for o in obs])), (k, t)
        assert np.array_equal(env.measure_sums.cpu().numpy(), np.array([[e.sums[k] for e in envs] for k in X.MEASURES], np.float32))


HAND_MADE = [  # (G, vis, rects, px, py, heading at turn 10): the worlds of tests/test_nav2d_explore_host.py
    (16, 5.0, [(3.0, 2.0, 3.1, 6.0)], 2.0, 4.0, 0), (16, 5.0, [], 2.25, 2.25, 0), (16, 2.0, [], 2.25, 2.25, 0),
    (16, float(np.nextafter(F(2.0), F(0.0))), [], 2.25, 2.25, 0), (64, 3.0, [], 2.0625, 2.0625, 0), (30, 2.0, [], 3.3, 4.1, 0)]


@pytest.mark.parametrize("world", range(len(HAND_MADE)))
def test_hand_made_worlds(world):
    """The hand-made worlds written into device records: a full turn to the left and back one step, from a record and a layer that
    the restatement began; record, layer, reward and sensors are the restatement's after every step.  (A thin wall, the wedge's edge,
    d2 == vis * vis and the float32 below, a centre behind the agent, the disc of a full turn.)"""
    G, vis, rects, px, py, h = HAND_MADE[world]
    e = X.Nav2DExploreEnv(1, 0, num_obstacles=0, coverage_resolution=G, visibility_dist=vis, max_episode_steps=1000)
    e.reset()
    e.place(rects, px, py, h)
    env = make_env(1, 0, 0, 1, K=len(rects), G=G, vis=vis, max_steps=1000)
    rows = env._own_obs()
    env.reset_into_obs(rows)
    env._state.copy_(torch.from_numpy(e.record()[None]))
    env.coverage().copy_(torch.from_numpy(e.layer[None]))
    rew, nd = torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.uint8, device="cuda")
    for a in [X.TURN_LEFT] * 36 + [X.TURN_RIGHT, X.MOVE_FORWARD, X.STOP]:
        o, r, done, _ = e.step(a)
        env.step_into_obs(rows, rew, nd, actions=torch.tensor([a], device="cuda"))
        torch.cuda.synchronize()
        if done:
            break   # the next world is the stream's, with K = 0 rectangles here and len(rects) there
        assert np.array_equal(env._state.cpu().numpy()[0], e.record()) and np.array_equal(env.coverage().cpu().numpy()[0], e.layer)
        assert rew.cpu().numpy().view(np.int32)[0] == np.array([r], np.float32).view(np.int32)[0] and int(nd[0]) == 1
        assert np.array_equal(rows["gps"].cpu().numpy()[0], o["gps"]) and np.array_equal(rows["compass"].cpu().numpy()[0], o["compass"])
    assert done and int(nd[0]) == 0 and float(rew[0]) == float(r)
    assert env._state.cpu().numpy()[0, 12:16].view(np.float32).tolist() == [float(v) for v in e.last_measures]


@pytest.mark.parametrize("G,vis,K", [(16, 1.0, 0), (30, 3.0, 8), (64, 2.5, 3)])
def test_the_layer_is_the_map_s_fog_of_war(G, vis, K):
    """The env's `top_down_map` keyword at the layer's resolution and visibility: after the reset and after every masked step entry
    top_down_map()['fog_of_war_mask'] equals coverage().  The map's update was written independently of the step's sweep."""
    N = 6
    env = make_env(N, 9, 18, 4, K=K, turn=30, G=G, vis=vis, max_steps=5, top_down_map=dict(map_resolution=G, visibility_dist=vis))
    rows = env._own_obs()
    env.reset_into_obs(rows)
    rng = np.random.RandomState(G)
    assert torch.equal(env.top_down_map()["fog_of_war_mask"], env.coverage()) and int(env.coverage().sum()) > 0
    for t in range(16):
        mask = torch.from_numpy((rng.rand(N) < 0.8).astype(np.uint8)).cuda()
        env.step_into_obs(rows, env._rew, env._nd, actions=torch.from_numpy(rng.randint(0, 4, size=N)).cuda(), mask=mask)
        assert torch.equal(env.top_down_map()["fog_of_war_mask"], env.coverage()), t
        assert torch.equal(env.coverage().view(N, -1).sum(1).int(), env._state[:, X.W_SEEN_CELLS]), t
    assert int(env._state[:, 10].min()) >= 1


def test_render_frames_bytewise():
    """render_frames() of the task against nav2d_map_reference.frame on this task's view (no marker, the agent and its tick), byte for
    byte, after the reset and after every step; with and without the image panels."""
    N, T, S = 3, 10, 40
    for H, W, rgb in ((12, 20, True), (9, 18, False), (0, 0, False)):
        envs = [X.Nav2DExploreEnv(6, n, H=H, W=W, num_obstacles=8, turn_angle=30, coverage_resolution=16, max_episode_steps=4,
                                  use_rgb=rgb) for n in range(N)]
        env = make_env(N, H, W, 6, K=8, turn=30, G=16, max_steps=4, use_rgb=rgb, top_down_map=dict(map_resolution=S, visibility_dist=2.5))
        maps = X.MapOf(envs, S, 2.5)
        obs = [e.reset() for e in envs]
        maps.begin()
        rows = env._own_obs()
        env.reset_into_obs(rows)
        rng = np.random.RandomState(3)
        for t in range(T + 1):
            got = env.render_frames(height=24).cpu().numpy()
            want = maps.frames(24, obs, rgb, H > 0)
            assert got.shape == want.shape and np.array_equal(got, want), (H, t)
            assert np.array_equal(env._map.cpu().numpy(), maps.map) and np.array_equal(env._map_rec.cpu().numpy(), maps.rec)
            a = rng.randint(0, 4, size=N)
            res = [e.step(x) for e, x in zip(envs, a)]
            obs = [r[0] for r in res]
            maps.after_step([r[2] for r in res])
            env.step_into_obs(rows, env._rew, env._nd, actions=torch.from_numpy(a).cuda())
        assert set(np.unique(maps.map)) <= {M.OCCUPIED, M.FREE, M.START, M.TRAJECTORY}


def test_entry_refusals_launch_nothing():
    """The entry refuses a NULL or misaligned record, a NULL layer, G outside 16..512, a visibility or a cell reward that is not
    positive / not finite, a compass without its table, and what hab_nav2d_step refuses; nothing runs.  The class refuses actions that
    are no int64 (N,) device tensor, by name."""
    from habitat_amd import _lib
    from habitat_amd._lib import ptr, stream_ptr
    N, H, W, G = 3, 9, 18, 30
    env = make_env(N, H, W, 1, K=3, turn=30, G=G, use_rgb=True)
    rows = env._own_obs()
    env.reset_into_obs(rows)
    torch.cuda.synchronize()
    state, layer = env._state.clone(), env.coverage().clone()
    actions = torch.ones(N, dtype=torch.int64, device="cuda")
    rew, nd = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    tabs = env._tables
    base = dict(state=ptr(env._state), dirs=ptr(tabs[0]), ray=ptr(tabs[1]), col_cos=ptr(tabs[2]), tanv=ptr(tabs[3]), actions=ptr(actions),
                mask=None, rgb=ptr(rows["rgb"]), depth=ptr(rows["depth"]), gps=ptr(rows["gps"]), compass=ptr(rows["compass"]),
                ctab=ptr(env._compass_table), layer=ptr(env.coverage()), reward=ptr(rew), not_done=ptr(nd), sums=ptr(env.measure_sums),
                seed=1, offset=0, N=N, H=H, W=W, K=3, nh=12, max_steps=12, G=G, vis=3.0, rc=0.01, advance=1)
    plus = lambda p, k: type(p)(p.value + k)

    def call(**kw):
        a = dict(base, **kw)
        return _lib.lib().hab_nav2d_explore_step(*(a[k] for k in base), stream_ptr())

    ERR_ARG = -1
    for kw in (dict(state=None), dict(state=plus(base["state"], 2)), dict(layer=None), dict(G=15), dict(G=513), dict(G=0), dict(vis=0.0),
               dict(vis=-1.0), dict(vis=float("inf")), dict(vis=float("nan")), dict(rc=-0.5), dict(rc=float("inf")), dict(rc=float("nan")),
               dict(ctab=None), dict(dirs=None), dict(N=0), dict(K=9), dict(K=-1), dict(nh=0), dict(max_steps=0), dict(actions=None),
               dict(reward=None), dict(not_done=None), dict(ray=None), dict(H=0), dict(depth=plus(base["depth"], 2))):
        assert call(**kw) == ERR_ARG, kw
    unsupported = call(W=4096)
    assert unsupported not in (0, ERR_ARG) and call(N=70000) == unsupported
    torch.cuda.synchronize()
    assert torch.equal(env._state, state) and torch.equal(env.coverage(), layer)                     # nothing ran
    assert call() == 0 and call(advance=0, actions=None, reward=None, not_done=None) == 0 and call(rc=0.0) == 0
    assert call(rgb=None, depth=None, ray=None, col_cos=None, tanv=None, H=0, W=0) == 0    # what needs no image needs no tables
    assert call(gps=None, compass=None, ctab=None, sums=None) == 0
    torch.cuda.synchronize()
    for bad in (torch.zeros(N, device="cuda"), torch.zeros(N + 1, dtype=torch.int64, device="cuda"), torch.zeros(N, dtype=torch.int64),
                torch.zeros(N, 2, dtype=torch.int64, device="cuda")[:, 0]):
        with pytest.raises(_lib.HabError, match="Nav2DExplore"):
            env.step_into_obs({}, rew, nd, actions=bad)
    for call_ in (env.follower_actions, env.expert_actions):
        with pytest.raises(_lib.HabError, match="Nav2DExplore"):
            call_()
    torch.cuda.synchronize()


# ---- the seams: trainer (device path, host path), VER transport, evaluator -------------------------------------------------------
TRAINED = ("depth", "gps", "compass")   # the YAML's sensors


def explore_config(tmp_path, N, T, K=3, max_steps=12, seed=100, size=64, hidden=64, extra=()):
    from habitat_amd.config.default import get_config
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=1000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          f"habitat_baselines.rl.ppo.hidden_size={hidden}", f"habitat_baselines.checkpoint_folder={tmp_path}",
          "habitat_baselines.log_interval=1000", f"habitat_baselines.tensorboard_dir={tmp_path}/tb",
          "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000", "habitat_baselines.trainer_name=ppo",
          f"habitat.environment.max_episode_steps={max_steps}", f"habitat.synthetic.num_obstacles={K}", f"habitat.seed={seed}",
          f"habitat.simulator.sensors.depth.height={size}", f"habitat.simulator.sensors.depth.width={size}"]
    return get_config("exploration/ddppo_nav2d_explore.yaml", ov + list(extra))


def restated_envs(cfg, **kw):
    hab = cfg.habitat
    N, size, syn = cfg.habitat_baselines.num_environments, hab.simulator.sensors.depth.height, hab.synthetic
    kw = dict(dict(H=size, W=size, use_rgb=False), **kw)
    envs = [X.Nav2DExploreEnv(hab.seed, n, num_obstacles=syn.num_obstacles, turn_angle=syn.turn_angle,
                              coverage_resolution=syn.coverage_resolution, visibility_dist=syn.visibility_dist,
                              coverage_reward=syn.coverage_reward, max_episode_steps=hab.environment.max_episode_steps, **kw)
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


@pytest.mark.parametrize("path", ["device", "host"])
def test_trainer_hands_over_the_stored_action(path, tmp_path):
    """Two update cycles of PPOTrainer from ddppo_nav2d_explore.yaml (4 envs, 8 steps, episodes of 12, ResNet18 on depth at 64 x 64,
    gps and compass through their embeddings, no objectgoal), then the stored actions replayed through the restatement from the same
    seed: every stored depth row, gps, compass, reward and mask are equal, bit for bit.  Once on the device path, once on the host
    path.  The window statistics carry the four measures."""
    from habitat_amd.common.env_factory import Nav2DExploreVectorEnv
    N, T = 4, 8
    extra = ["habitat_baselines.vector_env_factory._target_=test_gpu_nav2d.HostOnlyNav2DFactory"] if path == "host" else []
    cfg = explore_config(tmp_path, N, T, extra=extra)
    trainer = make_trainer(cfg)
    assert trainer._device_envs == (path == "device") and trainer.envs.consumes_actions
    assert isinstance(getattr(trainer.envs, "_envs", trainer.envs), Nav2DExploreVectorEnv)
    policy = trainer._agent.actor_critic
    assert type(policy).__name__ == "PointNavResNetPolicy" and not policy.is_blind and policy.fused_sensors == ()
    assert [v[0] for v in policy.visual_sensors] == ["depth"]
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
    for k in X.MEASURES:
        assert math.isclose(stats[k], sum(i[k] for i in infos), rel_tol=1e-5, abs_tol=1e-6), k
    inner = getattr(trainer.envs, "_envs", trainer.envs)
    assert np.array_equal(inner.coverage().cpu().numpy(), np.stack([e.layer for e in renvs]))
    trainer.envs.close()


def test_ver_transport_hands_over_the_stored_action(tmp_path):
    """One VERTrainer rollout on the device-resident Nav2DExplore source (4 envs, 8 steps): in the VER arena the slots of an env,
    ordered by (episode, step), replay through the restatement.  The report worker received the measures of the episodes that ended."""
    N, T = 4, 8
    cfg = explore_config(tmp_path, N, T, max_steps=5, extra=["habitat_baselines.trainer_name=ver", "habitat_baselines.rl.ver.num_inference_workers=1"])
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


def test_evaluator_reports_the_measures(tmp_path):
    """A short HabitatEvaluator run on the Nav2DExplore env: every recorded episode carries coverage, area_seen, collisions and
    num_steps, equal to the restatement's for the actions the evaluator handed over, and the aggregate is their mean."""
    from habitat_amd.rl.ppo.evaluator import HabitatEvaluator
    N = 4
    cfg = explore_config(tmp_path, N, 8, max_steps=6, extra=["habitat_baselines.test_episode_count=8"])
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
    assert set(X.MEASURES) | {"reward"} <= set(agg)
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
        assert {k: stats[k] for k in X.MEASURES} == {k: w[k] for k in X.MEASURES}, episode_id
        assert math.isclose(stats["reward"], w["reward"], rel_tol=1e-5, abs_tol=1e-6)
    for k in X.MEASURES:
        assert math.isclose(agg[k], float(np.mean([w[k] for w in want.values()])), rel_tol=1e-6, abs_tol=1e-9)
        assert Writer.scalars[f"eval_metrics/{k}"] == agg[k]
    envs.close()
