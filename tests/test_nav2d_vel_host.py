"""CPU: properties of the Nav2DVel-v0 task on its numpy restatement (tests/nav2d_vel_reference.py), the event coverage of the
scripted action sequences that tests/test_gpu_nav2d_vel.py replays on the device, the refusals of Nav2DVelVectorEnv and of the
factory, and what the trainer's host path hands an env for a continuous action."""
import types

import numpy as np
import pytest
import torch

import nav2d_reference as R
import nav2d_vel_reference as V

F = np.float32


def blind(seed=7, env=0, **kw):
    e = V.Nav2DVelEnv(seed, env, use_rgb=False, use_depth=False, **kw)
    e.reset()
    return e


def snapshot(e):
    return (e.px, e.py, e.h, e.path, e.steps, e.collisions, e.episode)


@pytest.mark.parametrize("K", [0, 3, 8])
@pytest.mark.parametrize("params", V.PARAMETER_SETS)
def test_invariants(K, params):
    """1500 random steps (uniform in [-1.25, 1.25]^2, so a part is clamped): after every step the agent is in free space and
    |dh| <= M; per episode path <= 0.25 * steps (float32 sum of at most `steps` terms <= 0.25: relative slack 2^-23 * steps) and the
    rewards telescope to d_start - d_end - 0.01 * length + 2.5 * success within nav2d's bound for a float32 reward: three roundings a
    step, len * (2^-25 + 2^-26 + 2^-31) + 2^-23."""
    turn, max_turn, min_ang = params
    e = blind(num_obstacles=K, turn_angle=turn, max_turn_angle=max_turn, min_abs_ang_speed=min_ang, max_episode_steps=40)
    rng = np.random.RandomState(K)
    total, episodes, moved = 0.0, 0, 0
    for _ in range(1500):
        before = (e.px, e.py)
        _, r, done, info = e.step(rng.uniform(-1.25, 1.25, 2).astype(np.float32))
        assert abs(e.last_dh) <= e.M
        total += float(r)
        if done:
            L = e.last
            closed = float(L["d_start"]) - float(L["d_end"]) - 0.01 * L["length"] + 2.5 * L["success"]
            assert abs(total - closed) <= L["length"] * (2.0 ** -25 + 2.0 ** -26 + 2.0 ** -31) + 2.0 ** -23, (total, closed)
            assert float(L["path"]) <= 0.25 * L["length"] * (1.0 + L["length"] * 2.0 ** -23)
            assert info["spl"] == 0.0 or (info["success"] == 1.0 and 0.0 < info["spl"] <= 1.0)
            total, episodes = 0.0, episodes + 1
        else:
            moved += (e.px, e.py) != before
        assert R.is_free(e.px, e.py, e.world.rects) and 0 <= e.h < e.nh
    assert episodes > 20 and moved > 200


def test_clamp_gives_identical_trajectories():
    a, b = blind(num_obstacles=8, max_episode_steps=30), blind(num_obstacles=8, max_episode_steps=30)
    rng = np.random.RandomState(1)
    clamped = 0
    for _ in range(400):
        x = rng.uniform(-3.0, 3.0, 2).astype(np.float32)
        ra, rb = a.step(x), b.step(np.clip(x, -1.0, 1.0))
        clamped += bool((np.abs(x) > 1).any())
        assert snapshot(a) == snapshot(b) and ra[1] == rb[1] and ra[2] == rb[2] and ra[3] == rb[3]
    assert clamped > 100 and a.counters["clamped"] == clamped and b.counters["clamped"] == 0


def test_ties_round_to_even():
    """c_ang * M exactly half-way rounds to the even neighbour: with M = 10, 0.05 -> 0.5 -> 0, 0.15 -> 1.5 -> 2, -0.25 -> -2.5 -> -2
    (each product is the exact half in float32: asserted, since 0.05 and 0.15 are not binary fractions)."""
    for a_ang, q, dh in ((0.05, 0.5, 0), (0.15, 1.5, 2), (-0.25, -2.5, -2), (0.25, 2.5, 2), (0.35, 3.5, 4)):
        assert F(F(a_ang) * F(10)) == F(q)
        _, _, _, got, tie = V.decode((0.0, a_ang), 10)
        assert got == dh and tie
    e = blind(num_obstacles=0)
    h = e.h
    e.step((1.0, 0.15))
    assert e.h == (h + 2) % 360 and e.counters["ties"] == 1


def test_non_finite_component_acts_as_zero():
    for bad in (np.nan, np.inf, -np.inf):
        for comp in (0, 1):
            a, b = blind(num_obstacles=3), blind(num_obstacles=3)
            x = np.array([0.4, -0.7], np.float32)
            y = x.copy()
            x[comp], y[comp] = bad, 0.0
            for _ in range(5):
                ra, rb = a.step(x), b.step(y)
                assert snapshot(a) == snapshot(b) and ra[1] == rb[1] and ra[2] == rb[2]
            assert a.counters["clamped"] == 0


def test_sliding_off_never_moves_a_blocked_agent():
    e = blind(num_obstacles=8, allow_sliding=False, max_episode_steps=30)
    s = blind(num_obstacles=8, allow_sliding=True, max_episode_steps=30)
    rng = np.random.RandomState(3)
    blocked = 0
    for _ in range(1500):
        before, collisions, episode = (e.px, e.py), e.collisions, e.episode
        e.step((1.0, float(rng.uniform(-1, 1))))
        if e.episode == episode and e.collisions > collisions:
            blocked += 1
            assert (e.px, e.py) == before
        s.step((1.0, float(rng.uniform(-1, 1))))
    assert blocked > 20 and e.counters["slide_x"] == e.counters["slide_y"] == 0 and e.counters["blocked"] >= blocked
    assert s.counters["slide_x"] > 0 and s.counters["slide_y"] > 0


def test_stop_is_reachable_for_the_defaults():
    """(-1, 0) stops; a length above the minimum does not; a turn of S quanta does not.  The greedy controller reaches the goal."""
    e = blind(num_obstacles=0)
    assert (e.M, e.S) == (10, 5) and e.min_lin == F(0.025)
    before = snapshot(e)
    _, r, done, info = e.step((-1.0, 0.0))
    assert done and e.counters["stops"] == 1 and info["success"] == 0.0 and r == F(-0.01) and e.episode == before[-1] + 1
    assert not e.step((-0.75, 0.0))[2]     # l = 0.25 * 0.125 = 0.03125 exactly, not below the minimum
    assert e.step((-0.81, 0.44))[2]        # l < 0.025 and dh = 4 < 5
    assert not e.step((-1.0, 0.5))[2]      # dh = 5: a turn in place
    r = V.rollout("greedy", 4, 3, 300, num_obstacles=0, max_episode_steps=150, use_rgb=False, use_depth=False)
    infos = [i for row in r["infos"] for i in row if i]
    assert len(infos) >= 3 and all(i["success"] == 1.0 and 0.0 < i["spl"] <= 1.0 for i in infos)


@pytest.mark.parametrize("params", V.PARAMETER_SETS)
def test_scripted_sequences_cover_their_events(params):
    """Over the four scripts and the three K of a parameter set every event counter is at least 1; ties come from 'grid' only."""
    total = dict.fromkeys(V.EVENTS, 0)
    for K in (0, 3, 8):
        for kind in V.SCRIPTS:
            r = V.script_rollout(kind, K, params)
            c = r["counters"]
            for k in V.EVENTS:
                total[k] += c[k]
            assert c["ties"] == 0 or kind == "grid"
            assert r["dones"].sum() >= V.SCRIPT_ENVS * 4
            if kind in ("random", "grid"):
                assert c["clamped"] > 50 and c["zero_length"] > 0 and c["timeouts"] > 0 and c["stops"] > 0
                assert len(set(r["dh"].reshape(-1).tolist())) >= 5
    print(f"nav2dvel script events {params}: {total}")
    assert all(total[k] >= 1 for k in V.EVENTS), total
    assert total["slide_x"] >= 10 and total["slide_y"] >= 10


def test_refusals():
    from habitat_amd import _lib
    from habitat_amd.common.env_factory import Nav2DVelVectorEnv, nav2d_vel_parameters
    assert nav2d_vel_parameters(1, 10, 0.025, 5) == (360, 10, 5) and nav2d_vel_parameters(5, 30, 0.25, 10) == (72, 6, 2)
    assert nav2d_vel_parameters(10, 180, 0.1, 180) == (36, 18, 18)
    bad = [dict(turn_angle=7), dict(turn_angle=1.0), dict(max_turn_angle=0), dict(max_turn_angle=181), dict(max_turn_angle=10.0),
           dict(turn_angle=4, max_turn_angle=10), dict(turn_angle=90, max_turn_angle=270, min_abs_ang_speed=90),
           dict(min_abs_ang_speed=0), dict(min_abs_ang_speed=11), dict(turn_angle=2, min_abs_ang_speed=5), dict(min_abs_ang_speed=2.5),
           dict(min_abs_lin_speed=0.0), dict(min_abs_lin_speed=-0.1), dict(min_abs_lin_speed=0.26), dict(min_abs_lin_speed=float("nan")),
           dict(min_abs_lin_speed="0.1"), dict(allow_sliding=1), dict(num_actions=4), dict(num_obstacles=9), dict(max_episode_steps=0)]
    for kw in bad:
        with pytest.raises(_lib.HabError):
            Nav2DVelVectorEnv(2, 8, 8, device="cpu", **kw)
        ref_kw = {k: v for k, v in kw.items() if k in ("turn_angle", "max_turn_angle", "min_abs_ang_speed", "min_abs_lin_speed")}
        if ref_kw:
            with pytest.raises(ValueError):
                V.Nav2DVelEnv(1, 0, **ref_kw)
    with pytest.raises(_lib.HabError, match="GPU"):   # valid parameters: only the missing device is refused
        Nav2DVelVectorEnv(2, 8, 8, device="cpu")
    e = blind()
    for bad_action in (0.5, (0.1, 0.2, 0.3), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            e.step(bad_action)


def bare_env(N=3):
    """A Nav2DVelVectorEnv without its device side: what async_step_at needs."""
    from habitat_amd.common.env_factory import Nav2DVelVectorEnv
    env = Nav2DVelVectorEnv.__new__(Nav2DVelVectorEnv)
    env.num_envs, env._pending, env._actions_host = N, set(), np.zeros((N, 2), np.float32)
    return env


def test_async_step_at_takes_a_length_2_array_only():
    from habitat_amd import _lib
    env = bare_env()
    env.async_step_at(0, np.array([0.25, -3.0], np.float32))
    env.async_step_at(2, {"action": [1.0, np.nan]})
    assert env._pending == {0, 2} and env._actions_host[0].tolist() == [0.25, -3.0] and env._actions_host[2, 0] == 1.0
    assert np.isnan(env._actions_host[2, 1]) and env._actions_host.dtype == np.float32
    for bad in (1, 0.5, np.float32(0.5), [0.1], [0.1, 0.2, 0.3], np.zeros((1, 2)), np.zeros((2, 1)), "ab", None):
        with pytest.raises(_lib.HabError):
            env.async_step_at(1, bad)
    assert env._pending == {0, 2}
    with pytest.raises(_lib.HabError):
        env.async_step_at(0, [0.0, 0.0])   # twice without wait_step_at


def test_factory_choice_and_config(monkeypatch):
    """habitat.task.type picks the env: 'Nav2DVel-v0' and 'nav2dvel' the new one, 'Nav2D-v0' the discrete one, 'PointNav-v0' the
    hashed source.  The constructors are replaced by recorders: the envs themselves need a GPU."""
    from habitat_amd.common import env_factory as EF
    from habitat_amd.common import spaces
    from habitat_amd.config.default import get_config
    cfg = get_config("pointnav/ppo_nav2d_vel.yaml")
    hab, main = cfg.habitat, cfg.habitat_baselines.rl.policy.main_agent
    assert hab.task.type == "Nav2DVel-v0" and list(hab.task.actions) == ["velocity_control"]
    assert hab.simulator.sensors.rgb.height == hab.simulator.sensors.depth.width == 64
    assert (hab.synthetic.turn_angle, hab.synthetic.max_turn_angle, hab.synthetic.min_abs_lin_speed, hab.synthetic.min_abs_ang_speed,
            hab.synthetic.allow_sliding) == (1, 10, 0.025, 5, True)
    assert main.name == "PointNavResNetPolicy" and main.action_distribution_type == "gaussian"
    assert cfg.habitat_baselines.rl.ddppo.backbone == "resnet18"
    made = []
    for name in ("Nav2DVelVectorEnv", "Nav2DVectorEnv", "SyntheticVectorEnv"):
        monkeypatch.setattr(EF, name, lambda *a, _n=name, **kw: made.append((_n, a, kw)) or _n)
    factory = EF.SyntheticVectorEnvFactory()
    assert factory.construct_envs(cfg, device="cpu") == "Nav2DVelVectorEnv"
    name, args, kw = made[-1]
    assert args == (16, 64, 64) and kw["num_actions"] == 1 and kw["max_episode_steps"] == 200 and kw["num_obstacles"] == 3
    assert {k: kw[k] for k in ("turn_angle", "max_turn_angle", "min_abs_lin_speed", "min_abs_ang_speed", "allow_sliding")} == dict(
        turn_angle=1, max_turn_angle=10, min_abs_lin_speed=0.025, min_abs_ang_speed=5, allow_sliding=True)
    for task_type, want in (("nav2dvel", "Nav2DVelVectorEnv"), ("NAV2DVEL-v1", "Nav2DVelVectorEnv"), ("Nav2D-v0", "Nav2DVectorEnv"),
                            ("PointNav-v0", "SyntheticVectorEnv")):
        c = get_config("pointnav/ppo_nav2d_vel.yaml", [f"habitat.task.type={task_type}"])
        assert factory.construct_envs(c, device="cpu") == want, task_type
    c = get_config("pointnav/ppo_nav2d.yaml")
    assert factory.construct_envs(c, device="cpu") == "Nav2DVectorEnv" and "max_turn_angle" not in made[-1][2]
    monkeypatch.undo()
    # the action space is the Box: built before anything touches the device
    sp = EF.spaces.Box(-1.0, 1.0, (2,), np.float32)
    assert spaces.is_continuous_action_space(sp) and spaces.get_action_space_info(sp) == ((2,), False)


def test_action_space_is_the_box(monkeypatch):
    """The env's constructor with the device side stubbed out (no GPU here): Box(-1, 1, (2,), float32), consumes_actions, and a
    float32 (N, 2) host action table."""
    from habitat_amd.common import env_factory as EF

    def fake_init(self, num_envs, height, width, **kw):
        self.num_envs, self.received = num_envs, kw
        self.action_spaces = [EF.spaces.Discrete(4)] * num_envs
    monkeypatch.setattr(EF.Nav2DVectorEnv, "__init__", fake_init)
    env = EF.Nav2DVelVectorEnv(3, 8, 8, turn_angle=5, max_turn_angle=30, min_abs_ang_speed=10, allow_sliding=False)
    assert env.consumes_actions and (env.max_turn_steps, env.stop_turn_steps, env.allow_sliding) == (6, 2, False)
    assert len(env.action_spaces) == 3 and env.orig_action_spaces is env.action_spaces
    for sp in env.action_spaces:
        assert isinstance(sp, EF.spaces.Box) and sp.shape == (2,) and sp.dtype == np.float32
        assert sp.low.tolist() == [-1.0, -1.0] and sp.high.tolist() == [1.0, 1.0]
    assert env._actions_host.shape == (3, 2) and env._actions_host.dtype == np.float32
    assert env.received["turn_angle"] == 5 and "num_actions" not in env.received


class RecordingEnvs:
    num_envs = 3

    def __init__(self):
        self.got = []

    def async_step_at(self, i, a):
        self.got.append((i, a))


def host_step(action_space, actions):
    """PPOTrainer._compute_actions_and_step_envs on stubs: returns what async_step_at received and what the rollout was given."""
    from habitat_amd.rl.ppo.policy import PolicyActionData
    from habitat_amd.rl.ppo.ppo_trainer import PPOTrainer
    inserted = {}
    data = PolicyActionData(actions=actions, values=torch.zeros(3, 1), action_log_probs=torch.zeros(3, 1), rnn_hidden_states=torch.zeros(3, 1, 4))
    rollouts = types.SimpleNamespace(
        get_current_step=lambda env_slice, buffer_index: dict(observations={}, recurrent_hidden_states=None, prev_actions=None, masks=None),
        insert=lambda **kw: inserted.update(kw))
    trainer = PPOTrainer.__new__(PPOTrainer)
    trainer.envs = RecordingEnvs()
    trainer._env_spec = types.SimpleNamespace(action_space=action_space)
    trainer._agent = types.SimpleNamespace(nbuffers=1, rollouts=rollouts, actor_critic=types.SimpleNamespace(act=lambda *a, **kw: data))
    trainer._compute_actions_and_step_envs()
    return trainer.envs.got, inserted


def test_host_path_clips_a_continuous_action_and_passes_the_array():
    from habitat_amd.common import spaces
    acts = torch.tensor([[0.25, -0.5], [1.75, -3.0], [-1.0, 1.0]])
    got, inserted = host_step(spaces.Box(-1.0, 1.0, (2,), np.float32), acts.clone())
    assert [i for i, _ in got] == [0, 1, 2]
    for (_, a), want in zip(got, np.clip(acts.numpy(), -1.0, 1.0)):
        assert isinstance(a, np.ndarray) and a.shape == (2,) and a.dtype == np.float32 and np.array_equal(a, want)
    assert torch.equal(inserted["actions"], acts)   # the stored action stays unclipped
    # per-component bounds are honoured
    got, _ = host_step(spaces.Box(np.array([-0.5, 0.0], np.float32), np.array([0.5, 2.0], np.float32)), acts.clone())
    assert [a.tolist() for _, a in got] == [[0.25, 0.0], [0.5, 0.0], [-0.5, 1.0]]
    # a discrete action is a Python int, as before
    got, _ = host_step(spaces.Discrete(4), torch.tensor([[3], [0], [2]]))
    assert [(i, a) for i, a in got] == [(0, 3), (1, 0), (2, 2)] and all(type(a) is int for _, a in got)


def test_ver_transport_keeps_the_array_whole():
    """DeviceEnvTransport.send_action / poll hand a (2,) action to async_step_at as the array it was given."""
    from habitat_amd.rl.ver.transport import DeviceEnvTransport

    class Envs(RecordingEnvs):
        def advance_on_device(self):
            pass

        def step_results_host(self):
            return np.zeros(3, np.float32), np.ones(3, np.uint8)

    tr = DeviceEnvTransport(Envs())
    batch = np.array([[0.5, -1.5], [0.0, 0.25], [2.0, 2.0]], np.float32)   # the inference worker's one host copy of a batch
    for i in (2, 0):
        tr.send_action(i, batch[i])
    assert sorted(tr.poll(0.0, 8)) == [0, 2]
    got = dict(tr.envs.got)
    assert set(got) == {0, 2} and all(isinstance(a, np.ndarray) and a.shape == (2,) for a in got.values())
    assert np.array_equal(got[0], batch[0]) and np.array_equal(got[2], batch[2])
