"""CPU: DAgger without a GPU.  The mix rule and the loss as tests/dagger_reference.py states them (their own properties on hand-made
sequences; the loss's gradients against finite differences of `total`), the trainer's beta schedule, every refusal that needs no
device, the registry names, the two YAMLs, the header against the binding table, and a closed loop of the rule on the numpy restatement
of Nav2DRearr-v0 under its oracle."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import dagger_reference as D
import nav2d_rearr_oracle_reference as OR

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the mix rule -----------------------------------------------------------------------------------------------------------------
def mix(actions, expert, status, not_done, u, beta, coef=1.0, prev=None, agree=None, mask=None):
    n = len(actions)
    a = np.array(actions, np.int64)
    prev = np.full(n, -1, np.int64) if prev is None else prev
    agree = np.zeros(2, np.int64) if agree is None else agree
    w = np.full(n, np.nan, F)
    D.dagger_mix(a, np.array(expert, np.int64), np.array(status, np.int32), np.array(not_done, np.uint8), np.array(u, F), beta, coef, prev,
                 w, agree, mask)
    return a, w, prev, agree


def test_the_comparison_with_beta_is_strict():
    half = F(0.5)
    below, above = np.nextafter(half, F(0)), np.nextafter(half, F(1))
    a, *_ = mix([0, 0, 0], [3, 3, 3], [0, 0, 0], [1, 1, 1], [below, half, above], 0.5)
    assert a.tolist() == [3, 0, 0]                        # u == beta keeps the learner's action


def test_beta_zero_never_and_beta_one_always_takes_the_teacher():
    top = np.nextafter(F(1), F(0))                        # the largest u a generator of [0, 1) can give
    u = [0.0, 0.25, top]
    assert mix([0, 0, 0], [2, 2, 2], [0] * 3, [1] * 3, u, 0.0)[0].tolist() == [0, 0, 0]
    assert mix([0, 0, 0], [2, 2, 2], [0] * 3, [1] * 3, u, 1.0)[0].tolist() == [2, 2, 2]


def test_inflections_and_the_carry_across_a_rollout_boundary():
    """Env 0: the same label throughout, one episode start in the middle.  Env 1: the label changes at step 2.  The carry is handed from
    one "rollout" (steps 0-1) to the next (steps 2-3) and nothing else is."""
    expert = [[1, 1], [1, 1], [1, 2], [1, 2]]
    not_done = [[0, 0], [1, 1], [1, 1], [0, 1]]
    prev, agree, ws = np.full(2, -1, np.int64), np.zeros(2, np.int64), []
    for t in range(4):
        _, w, prev, agree = mix([1, 0], expert[t], [0, 0], not_done[t], [0.9, 0.9], 0.5, coef=3.0, prev=prev, agree=agree)
        ws.append(w.tolist())
    assert ws == [[3.0, 3.0], [1.0, 1.0], [1.0, 3.0], [3.0, 1.0]]
    assert prev.tolist() == [1, 2]
    assert agree.tolist() == [4, 8]                       # env 0 agreed at every step, env 1 never
    fresh = mix([1, 0], expert[2], [0, 0], not_done[2], [0.9, 0.9], 0.5, coef=3.0)[1]
    assert fresh.tolist() == [3.0, 3.0]                   # without the carry both steps would look like inflections


def test_gave_up_weighs_nothing_and_is_not_counted():
    status = [D.GO, D.ARRIVED, D.UNREACHABLE, D.STUCK, D.PICK, D.PLACE]
    a, w, prev, agree = mix([0] * 6, [0] * 6, status, [1] * 6, [0.0] * 6, 1.0, coef=2.0, prev=np.zeros(6, np.int64))
    assert w.tolist() == [1.0, 1.0, 0.0, 0.0, 1.0, 1.0]
    assert agree.tolist() == [4, 4]                       # all six agree, only the four with w > 0 are counted
    assert prev.tolist() == [0] * 6 and a.tolist() == [0] * 6
    assert mix([0], [0], [D.GO], [0], [0.0], 1.0, coef=0.0)[3].tolist() == [0, 0]   # an inflection weighed 0 is not counted either


def test_agreement_is_taken_before_the_mix_and_the_mask_leaves_an_env_alone():
    a, w, prev, agree = mix([5, 5, 5], [5, 4, 4], [0] * 3, [1] * 3, [0.0] * 3, 1.0, mask=np.array([1, 1, 0], np.uint8))
    assert a.tolist() == [5, 4, 5] and agree.tolist() == [1, 2]
    assert np.isnan(w[2]) and prev.tolist() == [5, 4, -1]


# ---- the loss ---------------------------------------------------------------------------------------------------------------------
def loss_inputs(B, seed, weights):
    r = np.random.default_rng(seed)
    logits = r.normal(size=(B, 6))
    logp = (logits - np.log(np.exp(logits).sum(1, keepdims=True)))[np.arange(B), r.integers(0, 6, B)]
    return dict(values=r.normal(size=B).astype(F), logp=logp.astype(F), entropy=r.uniform(0.2, 1.7, B).astype(F),
                weights=np.asarray(weights, F), returns=r.normal(size=B).astype(F), value_loss_coef=0.5, entropy_coef=0.01)


def test_loss_with_no_weight_at_all():
    d = loss_inputs(65, 0, np.zeros(65))
    r = D.bc_loss(**d)
    out = r["out"][0]
    assert out[1] == 0.0 and out[10] == 0.0 and out[11] == 65 and np.all(r["d_logp"][0] == 0.0)
    assert out[7] == np.inf and out[8] == 0.0 and out[9] == -np.inf
    assert np.isfinite(np.delete(out, [7, 9])).all() and np.isfinite(r["d_value"][0]).all()
    assert out[3] == pytest.approx(0.5 * out[0] - float(F(0.01)) * out[2], rel=1e-12)


def test_equal_weights_give_the_plain_mean_nll():
    for c in (1.0, 2.5):
        d = loss_inputs(63, 1, np.full(63, c))
        r = D.bc_loss(**d)
        assert r["out"][0][1] == pytest.approx(-d["logp"].astype(np.float64).mean(), rel=1e-12)
        assert np.allclose(r["d_logp"][0], -1.0 / 63, rtol=1e-12)
        p = np.exp(d["logp"].astype(np.float64))
        assert r["out"][0][7] == p.min() and r["out"][0][9] == p.max() and r["out"][0][8] == pytest.approx(p.mean(), rel=1e-12)


def test_gradients_are_the_finite_differences_of_total():
    r = np.random.default_rng(2)
    d = loss_inputs(17, 3, r.choice([0.0, 1.0, 3.2], 17))
    g = D.bc_loss(**d)
    x64 = {k: np.asarray(v, np.float64) for k, v in d.items()}
    h = 1e-6
    for name, grad in (("values", "d_value"), ("logp", "d_logp"), ("entropy", "d_entropy")):
        for i in range(17):
            up, dn = dict(x64), dict(x64)
            up[name], dn[name] = x64[name].copy(), x64[name].copy()
            up[name][i] += h
            dn[name][i] -= h
            fd = (D.bc_total(**up) - D.bc_total(**dn)) / (2 * h)
            assert fd == pytest.approx(g[grad][0][i], rel=1e-6, abs=1e-9), (name, i)
    assert g["out"][0][3] == pytest.approx(D.bc_total(**{**x64, "entropy_coef": float(F(0.01))}), rel=1e-12)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 4097])
def test_a_float32_evaluation_meets_half_of_the_allowance_and_the_wrong_normaliser_does_not(B):
    r = np.random.default_rng(B)
    for weights in (r.choice([0.0, 1.0, 3.2], B), np.zeros(B), np.eye(1, B, B // 2)[0] * 3.2):
        d = loss_inputs(B, B + 7, weights)
        ref, got, wrong = D.bc_loss(**d), D.bc_loss_f32(**d), D.bc_loss(**d, normalise_by_B=True)
        for k in ("d_value", "d_logp", "d_entropy", "out"):
            v, e = ref[k]
            fin = np.isfinite(v)
            assert np.array_equal(np.asarray(got[k], np.float64)[~fin], v[~fin])
            assert (np.abs(np.asarray(got[k], np.float64)[fin] - v[fin]) <= 0.5 * e[fin]).all(), (k, B)
        W = float(np.asarray(weights, F).astype(np.float64).sum())
        if W > 0 and max(W, 1.0) != B:   # dividing by B instead of max(W, 1) is seen wherever the two differ
            assert abs(wrong["out"][0][1] - ref["out"][0][1]) > ref["out"][1][1]
            on = np.asarray(weights) > 0
            assert (np.abs(wrong["d_logp"][0][on] - ref["d_logp"][0][on]) > ref["d_logp"][1][on]).all()


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def test_beta_schedule_and_its_resume_point():
    from habitat_amd.config.default import Config
    from habitat_amd.rl.ppo.ppo_trainer import imitation_beta
    im = Config(beta_start=1.0, beta_end=0.2, beta_decay_updates=40)
    assert [imitation_beta(im, n) for n in (0, 10, 20, 40, 41, 1000)] == pytest.approx([1.0, 0.8, 0.6, 0.2, 0.2, 0.2])
    for n in (0, 7, 39, 40, 400):
        assert imitation_beta(im, n) == D.beta_at(n, 1.0, 0.2, 40)
    # a run resumed after 25 updates draws its next rollout at the 25-update point of the same line, not at beta_start
    assert imitation_beta(im, 25) == pytest.approx(1.0 - 0.8 * 25 / 40)
    assert imitation_beta(Config(beta_start=0.5, beta_end=0.5, beta_decay_updates=100), 3) == 0.5
    assert imitation_beta(Config(beta_start=1.0, beta_end=0.0, beta_decay_updates=0), 0) == 0.0


def test_registry_names():
    from habitat_amd.common.baseline_registry import baseline_registry
    import habitat_amd.rl.ppo.ppo_trainer  # noqa: F401
    from habitat_amd.common.rollout_storage import ImitationRolloutStorage, RolloutStorage
    from habitat_amd.rl.ddppo.ddppo import DDDAgger, DecentralizedDistributedMixin
    from habitat_amd.rl.ppo.ppo import PPO, DAgger
    assert baseline_registry.get_updater("DAgger") is DAgger and issubclass(DAgger, PPO)
    assert baseline_registry.get_updater("DDDAgger") is DDDAgger
    assert DDDAgger.__mro__[1:3] == (DecentralizedDistributedMixin, DAgger)
    assert baseline_registry.get_storage("ImitationRolloutStorage") is ImitationRolloutStorage
    assert issubclass(ImitationRolloutStorage, RolloutStorage)


def test_both_yamls_load_and_the_defaults_leave_imitation_off():
    from habitat_amd.config.default import get_config
    from habitat_amd.rl.ppo.ppo_trainer import imitation_settings, refuse_imitation_config
    block = dict(enabled=False, beta_start=1.0, beta_end=0.0, beta_decay_updates=100, inflection_weight_coef=1.0)
    for sibling, mine, task in (("rearrange/ddppo_nav2d_rearrange_geodesic.yaml", "rearrange/dagger_nav2d_rearrange_geodesic.yaml", "Nav2DRearr-v0"),
                                ("pointnav/ppo_nav2d_geodesic.yaml", "pointnav/dagger_nav2d_geodesic.yaml", "Nav2D-v0")):
        base, cfg = get_config(sibling), get_config(mine)
        assert base.habitat_baselines.rl.imitation.to_dict() == block and imitation_settings(base) is None
        assert refuse_imitation_config(base) is None
        hb = cfg.habitat_baselines
        assert (hb.updater_name, hb.distrib_updater_name, hb.rollout_storage_name) == ("DAgger", "DDDAgger", "ImitationRolloutStorage")
        assert hb.rl.imitation.to_dict() == dict(block, enabled=True) and refuse_imitation_config(cfg) is hb.rl.imitation
        assert cfg.habitat.task.type == task and cfg.habitat.synthetic.distance_to_goal == "geodesic"
        a, b = base.to_dict(), cfg.to_dict()                 # every other key is the sibling's
        for k in ("updater_name", "distrib_updater_name", "rollout_storage_name"):
            b["habitat_baselines"][k] = a["habitat_baselines"][k]
        b["habitat_baselines"]["rl"]["imitation"] = a["habitat_baselines"]["rl"]["imitation"]
        assert a == b


def test_header_and_signature_table_agree():
    from habitat_amd import _lib
    text = open(os.path.join(ROOT, "include", "habitat_amd.h")).read()
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float}
    names = {"hab_dagger_mix": ["actions", "expert", "status", "not_done", "u", "mask", "beta", "inflection_coef", "prev_expert", "weights",
                                "agree", "N", "stream"],
             "hab_bc_loss": ["values", "logp", "entropy", "weights", "returns", "rows", "B", "value_loss_coef", "entropy_coef", "d_value",
                             "d_logp", "d_entropy", "out12", "stream"]}
    for entry, wanted in names.items():
        m = re.search(r"int %s\((.*?)\);" % entry, text, re.S)
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
        restype, argtypes = _lib.SIGNATURES[entry]
        assert restype is ctypes.c_int and len(params) == len(argtypes)
        for p, t in zip(params, argtypes):
            assert t is (ctypes.c_void_p if ("*" in p or p.startswith("hipStream_t")) else kinds[p.split()[0]]), (entry, p)
        assert [p.split()[-1].lstrip("*") for p in params] == wanted
        assert hasattr(_lib.lib(), entry)
    codes = {k: int(v) for k, v in re.findall(r"#define HAB_NAV2D_ORACLE_(\w+) +(\d+)", text)}
    assert codes == dict(GO=D.GO, ARRIVED=D.ARRIVED, UNREACHABLE=D.UNREACHABLE, STUCK=D.STUCK, PICK=D.PICK, PLACE=D.PLACE)
    follow = {k: int(v) for k, v in re.findall(r"#define HAB_NAV2D_FOLLOW_(\w+) +(\d+)", text)}
    assert follow == {k: codes[k] for k in ("GO", "ARRIVED", "UNREACHABLE", "STUCK")}      # the follower's four are the first four


def test_entry_points_refuse_bad_arguments_without_a_device():
    """The refusals come before any launch, so they can be seen without a GPU: every required pointer, N / B <= 0, beta outside [0, 1]
    or not finite, inflection_coef negative or not finite."""
    from habitat_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = [p, p, p, p, p, None, 0.5, 1.0, p, p, p, 1, None]
    for i in (0, 1, 2, 3, 4, 8, 9, 10):
        bad = list(good)
        bad[i] = None
        assert L.hab_dagger_mix(*bad) == -1, i
    for i, v in ((11, 0), (11, -3), (6, -0.01), (6, 1.01), (6, float("nan")), (6, float("inf")), (7, -1.0), (7, float("nan")),
                 (7, float("inf"))):
        bad = list(good)
        bad[i] = v
        assert L.hab_dagger_mix(*bad) == -1, (i, v)
    good = [p, p, p, p, p, None, 1, 0.5, 0.01, p, p, p, p, None]
    for i in (0, 1, 2, 3, 4, 9, 10, 11, 12):
        bad = list(good)
        bad[i] = None
        assert L.hab_bc_loss(*bad) == -1, i
    for b in (0, -1):
        bad = list(good)
        bad[6] = b
        assert L.hab_bc_loss(*bad) == -1


def test_teacher_interface_and_its_refusals():
    """expert_actions is follower_actions on Nav2D-v0 and oracle_actions on Nav2DRearr-v0; the four other tasks refuse by name in
    both distance modes, and the two that have a teacher refuse the Euclidean mode as their advisers do."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    called = []
    for cls, method in ((EF.Nav2DVectorEnv, "follower_actions"), (EF.Nav2DRearrVectorEnv, "oracle_actions")):
        env = cls.__new__(cls)
        setattr(env, method, lambda _m=method, **kw: called.append((_m, kw)) or "row")
        assert env.expert_actions(out=1, mask=2, next_d=3, status=4) == "row"
        assert called[-1] == (method, dict(out=1, mask=2, next_d=3, status=4))
        env = cls.__new__(cls)
        env.distance = "euclidean"
        with pytest.raises(_lib.HabError, match=cls._name + ":.*needs `distance_to_goal: geodesic`"):
            env.expert_actions()
    for cls in (EF.Nav2DVelVectorEnv, EF.Nav2DObjVectorEnv, EF.Nav2DRearrVelVectorEnv, EF.Nav2DSocialVectorEnv):
        for distance in EF.NAV2D_DISTANCES:
            env = cls.__new__(cls)
            env.distance = distance
            with pytest.raises(_lib.HabError, match=cls._name + ": the task has no discrete teacher"):
                env.expert_actions()


def test_storage_refuses_a_continuous_action_space():
    from habitat_amd import _lib
    from habitat_amd.common import spaces as S
    from habitat_amd.common.rollout_storage import ImitationRolloutStorage
    osp = S.Dict({"x": S.Box(-1.0, 1.0, (2,), np.float32)})
    pol = types.SimpleNamespace(num_recurrent_layers=1, recurrent_hidden_size=8)
    with pytest.raises(_lib.HabError, match="continuous action space"):
        ImitationRolloutStorage(4, 2, osp, S.Box(-1.0, 1.0, (2,), np.float32), pol, device="cpu")
    st = ImitationRolloutStorage(4, 2, osp, S.Discrete(6), pol, device="cpu")
    B = st.buffers
    assert B["expert_actions"].shape == B["actions"].shape and B["expert_actions"].dtype == B["actions"].dtype
    assert tuple(B["expert_weights"].shape) == (5, 2, 1) and str(B["expert_weights"].dtype) == "torch.float32"


def test_updater_refusals():
    from habitat_amd import _lib
    from habitat_amd.common import spaces as S
    from habitat_amd.common.rollout_storage import RolloutStorage
    from habitat_amd.rl.ppo.ppo import DAgger
    kw = dict(clip_param=0.2, ppo_epoch=1, num_mini_batch=1, value_loss_coef=0.5, entropy_coef=0.01, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    with pytest.raises(_lib.HabError, match="auxiliary-loss modules"):
        DAgger(types.SimpleNamespace(aux_loss_modules={"cpca": object()}), **kw)
    with pytest.raises(_lib.HabError, match="adaptive entropy penalty"):
        DAgger(types.SimpleNamespace(aux_loss_modules={}), **kw, use_adaptive_entropy_pen=True)
    with pytest.raises(_lib.HabError, match="adaptive entropy penalty"):      # and where it arrives by position
        DAgger(types.SimpleNamespace(aux_loss_modules={}), 0.2, 1, 1, 0.5, 0.01, 1e-3, 1e-5, 0.5, False, True, 0.0, True)
    st = RolloutStorage(4, 2, S.Dict({"x": S.Box(-1.0, 1.0, (2,), np.float32)}), S.Discrete(4),
                        types.SimpleNamespace(num_recurrent_layers=1, recurrent_hidden_size=8), device="cpu")
    with pytest.raises(_lib.HabError, match="no `expert_actions`"):
        DAgger.update(DAgger.__new__(DAgger), st)


def test_trainer_refusals():
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    from habitat_amd.common.baseline_registry import baseline_registry
    from habitat_amd.config.default import get_config
    from habitat_amd.rl.ppo.ppo_trainer import refuse_imitation_config, refuse_imitation_envs
    import habitat_amd.rl.ver.ver_trainer  # noqa: F401
    yaml = "rearrange/dagger_nav2d_rearrange_geodesic.yaml"
    with pytest.raises(_lib.HabError, match="VER trainer"):
        refuse_imitation_config(get_config(yaml), ver=True)
    with pytest.raises(_lib.HabError, match="VER trainer"):     # and the trainer itself, before it touches a device
        baseline_registry.get_trainer("ver")(get_config(yaml))._init_train()
    for ov, why in (("habitat_baselines.updater_name=PPO", "pair DAgger / ImitationRolloutStorage.*PPO / ImitationRolloutStorage"),
                    ("habitat_baselines.rollout_storage_name=RolloutStorage", "pair DAgger / ImitationRolloutStorage.*DAgger / RolloutStorage"),
                    ("habitat_baselines.rl.ppo.use_double_buffered_sampler=True", "use_double_buffered_sampler"),
                    ("habitat_baselines.rl.imitation.beta_start=1.5", "beta_start"),
                    ("habitat_baselines.rl.imitation.beta_end=-0.1", "beta_end"),
                    ("habitat_baselines.rl.imitation.inflection_weight_coef=-1.0", "inflection_weight_coef")):
        with pytest.raises(_lib.HabError, match=why):
            refuse_imitation_config(get_config(yaml, [ov]))
        with pytest.raises(_lib.HabError, match=why):
            baseline_registry.get_trainer("ppo")(get_config(yaml, [ov]))._init_train()
    with pytest.raises(_lib.HabError, match="distrib_updater_name DDDAgger"):
        refuse_imitation_config(get_config(yaml, ["habitat_baselines.distrib_updater_name=DDPPO"]), distributed=True)
    with pytest.raises(_lib.HabError, match="imitation.enabled=True"):      # the pair without the block: nothing would label the rollout
        refuse_imitation_config(get_config(yaml, ["habitat_baselines.rl.imitation.enabled=False"]))
    # the env's side of the contract is one method, expert_actions, which raises with its reason where it cannot teach; the
    # trainer makes one probing call and passes the reason on
    probed = []
    teaching = types.SimpleNamespace(expert_actions=lambda **kw: probed.append(kw))
    refuse_imitation_envs(teaching, True)
    assert probed == [{}]
    refuse_imitation_envs(teaching, True, probe=False)
    assert len(probed) == 1
    with pytest.raises(_lib.HabError, match="host rollout path"):
        refuse_imitation_envs(teaching, False)
    with pytest.raises(_lib.HabError, match="no expert_actions"):
        refuse_imitation_envs(object(), True)
    rearr = EF.Nav2DRearrVectorEnv.__new__(EF.Nav2DRearrVectorEnv)
    rearr.distance = "euclidean"
    with pytest.raises(_lib.HabError, match="imitation: Nav2DRearr:.*needs `distance_to_goal: geodesic`"):
        refuse_imitation_envs(rearr, True)
    nav = EF.Nav2DVectorEnv.__new__(EF.Nav2DVectorEnv)
    nav.distance = "euclidean"
    with pytest.raises(_lib.HabError, match="imitation: Nav2D:.*needs `distance_to_goal: geodesic`"):
        refuse_imitation_envs(nav, True)
    for cls in (EF.Nav2DVelVectorEnv, EF.Nav2DObjVectorEnv, EF.Nav2DRearrVelVectorEnv, EF.Nav2DSocialVectorEnv):
        for distance in EF.NAV2D_DISTANCES:
            env = cls.__new__(cls)
            env.distance = distance
            with pytest.raises(_lib.HabError, match="imitation: " + cls._name + ": the task has no discrete teacher"):
                refuse_imitation_envs(env, True)


# ---- a closed loop on the numpy envs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 100])
def test_closed_loop_on_the_restated_envs(seed):
    """Nav2DRearr-v0 in geodesic mode, K = 3, 10 degrees, 8 envs, episodes of at most 200 steps, 150 steps, beta = 1: a random
    "policy" samples, the oracle labels, the rule mixes.  Every executed action is the oracle's; the share of samples with w = 0 is at
    most 5 % (the condition that keeps the weighted tests from going empty); the weights are 0 exactly at the give-ups; the inflection
    weight sits exactly at episode starts and label changes.  Measured here: w = 0 on 0 of 1200 samples at seed 1 and on 0 of 1200 at
    seed 100 (the oracle's host tests count 4 give-ups in 384 episodes over all their configurations; none falls into these 150
    steps).  About 45 % of the samples are inflections at 10 degrees: the label changes between turning and going forward every few
    steps."""
    N, steps, coef = 8, 150, 3.2
    envs = OR.restated_envs(seed, N, 3, 10, False, max_steps=200)
    for e in envs:
        e.reset()
    rng = np.random.default_rng(seed)
    prev, agree, not_done = np.full(N, -1, np.int64), np.zeros(2, np.int64), np.zeros(N, np.uint8)
    zero = total = inflections = 0
    last_label = [None] * N
    for t in range(steps):
        decisions = [OR.oracle(e) for e in envs]
        expert = np.array([OR.action_of(d) for d in decisions], np.int64)
        status = np.array([d[0] for d in decisions], np.int32)
        actions, w = rng.integers(0, 6, N).astype(np.int64), np.full(N, np.nan, F)
        sampled = actions.copy()
        before = agree.copy()
        D.dagger_mix(actions, expert, status, not_done, rng.random(N, dtype=F), 1.0, coef, prev, w, agree)
        assert np.array_equal(actions, expert) and np.array_equal(prev, expert)
        for n in range(N):
            gave_up = status[n] in (OR.UNREACHABLE, OR.STUCK)
            inflection = not_done[n] == 0 or last_label[n] != expert[n]
            assert w[n] == (F(0) if gave_up else (F(coef) if inflection else F(1)))
            last_label[n] = expert[n]
            inflections += int(inflection and not gave_up)
        assert agree[1] - before[1] == (w > 0).sum() and agree[0] - before[0] == ((w > 0) & (sampled == expert)).sum()
        zero += int((w == 0).sum())
        total += N
        not_done = np.array([0 if e.step(int(a))[2] else 1 for e, a in zip(envs, actions)], np.uint8)
    print(f"dagger closed loop seed {seed}: w = 0 on {zero} of {total} samples, {inflections} inflections, agreement of the random "
          f"policy {agree[0]} / {agree[1]}")
    assert zero <= 0.05 * total
    assert inflections > N and agree[1] == total - zero
