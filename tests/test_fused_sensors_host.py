"""CPU: PointNavResNetPolicy on observation spaces with visual sensors under any name and raw 1-D sensors fused into the recurrent
encoder's input (`fuse_keys`; reference rl/ddppo/policy/resnet_policy.py:178-199,560-571,648-660).  The sensor resolution, the module's
parameters and the engine's parameter table (hab_policy_create needs no device) are checked against oracle.fixtures.resnet_param_shapes;
the refusals each carry a message."""
import numpy as np
import pytest
import torch

from oracle.fixtures import resnet_param_shapes

F32, U8 = np.float32, np.uint8
GOAL = "pointgoal_with_gps_compass"
HID = 64


def _S():
    from habitat_amd.common import spaces as S
    return S


def img(M, c, dtype=F32, hw=(64, 96), high=None):
    return M.Box(0, (255 if dtype == U8 else 1) if high is None else high, (hw[0], hw[1], c), dtype)


def vec(M, n, dtype=F32):
    return M.Box(-1e9, 1e9, (n,), dtype)


def rearrange_space(M, goal=True):
    d = {"head_depth": img(M, 1), "arm_depth": img(M, 1), "joint": vec(M, 7), "is_holding": vec(M, 1), "goal_to_agent_gps_compass": vec(M, 2)}
    if goal:
        d[GOAL] = vec(M, 2)
    return M.Dict(d)


def build(space, rnn_type="GRU", layers=1, **kw):
    from habitat_amd.rl.ddppo.policy import PointNavResNetPolicy
    return PointNavResNetPolicy(space, _S().Discrete(4), hidden_size=HID, rnn_type=rnn_type, num_recurrent_layers=layers, backbone="resnet18", **kw)


def engine_table(policy):
    """[(name, shape)] and offsets of the engine's flat arena for the policy's descriptor."""
    from habitat_amd.engine import policy_param_table
    tab = policy_param_table(**policy._engine_kwargs)
    return [(n, s) for n, s, _ in tab], [o for _, _, o in tab]


def check_names(policy, n_in, H, W, rnn_type, layers, blind=False, has_goal=True):
    names = [n for n, _ in resnet_param_shapes(max(n_in, 1), H or 64, W or 64, HID, 4, rnn_type, layers, "resnet18", 32, normalize=False,
                                               has_goal=has_goal)]
    if blind:
        names = [n for n in names if not n.startswith(("net.visual_encoder.", "net.visual_fc."))]
    sd = policy.state_dict()
    assert list(sd.keys()) == names
    tab, offs = engine_table(policy)
    assert [n for n, _ in tab] == names
    assert all(tuple(sd[n].shape) == s for n, s in tab)
    assert offs == sorted(offs)
    return sd


@pytest.mark.parametrize("rnn_type,layers,G", [("GRU", 1, 3), ("LSTM", 2, 4)])
def test_two_cameras_and_fused_sensors(rnn_type, layers, G):
    """head_depth + arm_depth -> a 2-channel encoder; joint(7) + is_holding(1) + goal_to_agent_gps_compass(2) -> 10 raw columns of
    weight_ih_l0 between visual_fc's output and the two embeddings; no parameter is added or renamed."""
    pol = build(rearrange_space(_S()), rnn_type, layers)
    sd = check_names(pol, 2, 64, 96, rnn_type, layers)
    assert sd["net.state_encoder.rnn.weight_ih_l0"].shape == (G * HID, HID + 10 + 64)
    assert sd["net.visual_encoder.backbone.conv1.0.weight"].shape == (32, 2, 7, 7)
    assert [v[0] for v in pol.visual_sensors] == ["head_depth", "arm_depth"]
    assert list(pol.fused_sensors) == [("joint", 7), ("is_holding", 1), ("goal_to_agent_gps_compass", 2)]
    assert not pol.is_blind


def test_eight_channels_blind_and_explicit_fuse_keys():
    S = _S()
    # u8x3, f32x1, u8x3, f32x1: 8 channels, uint8 sensors scaled by fp32(1 / high.max())
    d = {"head_rgb": img(S, 3, U8), "head_depth": img(S, 1), "arm_rgb": img(S, 3, U8, high=100), "arm_depth": img(S, 1), "joint": vec(S, 7),
         GOAL: vec(S, 2)}
    pol = build(S.Dict(d), normalize_visual_inputs=True)
    sd = pol.state_dict()
    assert sd["net.visual_encoder.backbone.conv1.0.weight"].shape == (32, 8, 7, 7)
    assert sd["net.visual_encoder.running_mean_and_var._mean"].shape == (1, 8, 1, 1)
    assert sd["net.state_encoder.rnn.weight_ih_l0"].shape == (3 * HID, HID + 7 + 64)
    tab, _ = engine_table(pol)
    assert [n for n, _ in tab] == list(sd.keys()) and all(tuple(sd[n].shape) == s for n, s in tab)
    scales = [v[3] for v in pol.visual_sensors]
    assert scales[0] == float(np.float32(1.0 / 255.0)) and scales[2] == float(np.float32(1.0 / 100.0)) and scales[1] == scales[3] == 1.0
    # blind: no rank-3 key -> no encoder, the 1-D sensors are fused all the same
    sp = S.Dict({"joint": vec(S, 7), "is_holding": vec(S, 1), "goal_to_agent_gps_compass": vec(S, 2), GOAL: vec(S, 2)})
    blind = build(sp)
    sdb = check_names(blind, 0, 0, 0, "GRU", 1, blind=True)
    assert blind.is_blind and sdb["net.state_encoder.rnn.weight_ih_l0"].shape == (3 * HID, 10 + 64)
    # force_blind_policy on the camera space gives the same net
    fb = build(rearrange_space(S), force_blind_policy=True)
    assert fb.is_blind and list(fb.state_dict().keys()) == list(sdb.keys())
    assert fb.state_dict()["net.state_encoder.rnn.weight_ih_l0"].shape == (3 * HID, 10 + 64)
    # explicit list: arm_depth dropped (stored by the rollout, not read), 1-D keys in the list's order
    ex = build(rearrange_space(S), fuse_keys=["is_holding", "head_depth", "joint"])
    sde = check_names(ex, 1, 64, 96, "GRU", 1)
    assert sde["net.visual_encoder.backbone.conv1.0.weight"].shape == (32, 1, 7, 7)
    assert [v[0] for v in ex.visual_sensors] == ["head_depth"] and list(ex.fused_sensors) == [("is_holding", 1), ("joint", 7)]
    assert sde["net.state_encoder.rnn.weight_ih_l0"].shape == (3 * HID, HID + 8 + 64)
    assert ex._engine_kwargs["fused_widths"] == (1, 7)


def test_refusals_carry_a_message():
    from habitat_amd._lib import HabError
    S = _S()
    base = {"joint": vec(S, 7), GOAL: vec(S, 2)}
    with pytest.raises(HabError, match="height x width"):
        build(S.Dict(dict(base, head_depth=img(S, 1), arm_depth=img(S, 1, hw=(64, 64)))))
    with pytest.raises(HabError, match="at most 8"):
        build(S.Dict(dict(base, a=img(S, 3, U8), b=img(S, 3, U8), c=img(S, 3, U8))))
    with pytest.raises(HabError, match="at most 4"):
        build(S.Dict(dict(base, a=img(S, 1), b=img(S, 1), c=img(S, 1), d=img(S, 1), e=img(S, 1))))
    with pytest.raises(HabError, match="float32"):
        build(S.Dict(dict(base, obj_id=vec(S, 1, np.int64))))
    with pytest.raises(HabError, match="fed twice"):
        build(S.Dict(dict(base, head_depth=img(S, 1))), fuse_keys=["head_depth", GOAL])
    with pytest.raises(HabError, match="heading"):
        build(S.Dict(dict(base, head_depth=img(S, 1), heading=vec(S, 1))))
    with pytest.raises(HabError, match="imagegoal"):
        build(S.Dict(dict(base, head_depth=img(S, 1), imagegoal=img(S, 3, U8))))
    with pytest.raises(KeyError):
        build(S.Dict(dict(base, head_depth=img(S, 1))), fuse_keys=["head_depth", "no_such_sensor"])


@pytest.mark.parametrize("order", [("rgb", "depth"), ("depth", "rgb")])
def test_space_accepted_before_keeps_its_parameter_table(order):
    """rgb + depth + goal: still described to the engine by the legacy flags; names, shapes and offsets are those of the table
    oracle.fixtures.resnet_param_shapes lists (what test_resnet_engine_vs_oracle compares against), packed in order."""
    S = _S()
    d = {k: (img(S, 3, U8) if k == "rgb" else img(S, 1)) for k in order}
    d[GOAL] = vec(S, 2)
    pol = build(S.Dict(d), "LSTM", 2, normalize_visual_inputs=True)
    kw = pol._engine_kwargs
    assert "visual_table" not in kw and "fused_widths" not in kw and kw["has_rgb"] and kw["has_depth"] and kw["visual_order"] == order
    want = resnet_param_shapes(4, 64, 96, HID, 4, "LSTM", 2, "resnet18", 32, normalize=True, with_buffers=True)
    tab, offs = engine_table(pol)
    assert tab == [(n, tuple(s)) for n, s in want]
    end = 0
    for (n, s), o in zip(tab, offs):  # the arena packs the entries in order, 16-byte aligned
        assert o == (end + 3) // 4 * 4, n
        end = o + int(np.prod(s))
    # the same sensors through the table form give the same table (one representation inside the engine)
    from habitat_amd.engine import policy_param_table
    from habitat_amd import _lib
    kw2 = dict(kw, has_rgb=False, has_depth=False, visual_order=(),
               visual_table=tuple((_lib.DTYPE_U8, 3, float(np.float32(1 / 255.0))) if k == "rgb" else (_lib.DTYPE_F32, 1, 1.0) for k in order))
    assert policy_param_table(**kw2) == policy_param_table(**kw)


def test_rearrange_host_env_matches_its_observation_space():
    from habitat_amd.core.host_env import make_rearrange_host_env
    env = make_rearrange_host_env(3, 32, 48, True, True, 4, 50)
    sp = env.observation_space.spaces
    assert list(sp.keys()) == ["head_depth", "arm_depth", "joint", "is_holding", "goal_to_agent_gps_compass"]
    o = env.reset()
    o2, r, done, info = env.step(1)
    for obs in (o, o2):
        assert list(obs.keys()) == list(sp.keys())
        for k, v in obs.items():
            assert v.shape == tuple(sp[k].shape) and v.dtype == sp[k].dtype, k
    pol = build(env.observation_space)
    assert pol.state_dict()["net.state_encoder.rnn.weight_ih_l0"].shape == (3 * HID, HID + 10 + 32)


def test_identical_to_live_reference():
    """state_dict names, shapes and seeded initial values equal the reference's policy on the same space with fuse_keys=None."""
    from oracle.ref_loader import load_reference, reference_available
    if not reference_available():
        pytest.skip("reference checkout not present")
    ns = load_reference()
    for goal in (True, False):
        torch.manual_seed(5)
        a = build(rearrange_space(_S(), goal)).state_dict()
        torch.manual_seed(5)
        b = ns.resnet_policy.PointNavResNetPolicy(rearrange_space(ns.spaces, goal), ns.spaces.Discrete(4), hidden_size=HID, backbone="resnet18").state_dict()
        assert list(a.keys()) == list(b.keys())
        assert all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in b)


# ------------------------------------------------------------------------------------------------------------------------------------
# The per-pixel arithmetic of the table-driven ingest kernel, run on the host (tests/hostcheck/hostcheck_ingest.hip executes the
# kernel's own `ingest_table_pixel`): bitwise F.avg_pool2d of the scaled, concatenated sensors
# ------------------------------------------------------------------------------------------------------------------------------------
U8c, F32c, I32c = 0, 1, 2  # HAB_DTYPE_*
INGEST_SETS = {"f1f1": [(F32c, 1, 1), (F32c, 1, 1)], "f1u3": [(F32c, 1, 1), (U8c, 3, 255)], "u3f1u3f1": [(U8c, 3, 255), (F32c, 1, 1), (U8c, 3, 255), (F32c, 1, 1)],
               "i1u3f1": [(I32c, 1, 1), (U8c, 3, 255), (F32c, 1, 1)], "u3high100_f1": [(U8c, 3, 100), (F32c, 1, 1)],
               "f2u4i1": [(F32c, 2, 1), (U8c, 4, 255), (I32c, 1, 1)]}


@pytest.mark.parametrize("H,W", [(20, 24), (21, 27)])
@pytest.mark.parametrize("name", list(INGEST_SETS))
def test_ingest_table_pixel_arithmetic_on_the_host(name, H, W):
    import ctypes as C
    import os
    import torch.nn.functional as F
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck", "libhab_hostcheck_ingest.so"))
    table = INGEST_SETS[name]
    rng = np.random.default_rng(3)
    nrows, rows = 7, np.array([3, 0, 3, 5], dtype=np.int32)
    sensors, parts, scales = [], [], []
    for dt, ch, high in table:
        if dt == U8c:
            a = rng.integers(0, high + 1, (nrows, H, W, ch), dtype=np.uint8)
            sc = np.float32(1.0 / high)
            parts.append(torch.from_numpy(a[rows]).permute(0, 3, 1, 2).float() * float(sc))
        elif dt == I32c:
            a, sc = rng.integers(0, 40, (nrows, H, W, ch)).astype(np.int32), np.float32(1.0)
            parts.append(torch.from_numpy(a[rows]).permute(0, 3, 1, 2).float())
        else:
            a, sc = rng.random((nrows, H, W, ch), dtype=np.float32), np.float32(1.0)
            parts.append(torch.from_numpy(a[rows]).permute(0, 3, 1, 2))
        sensors.append(np.ascontiguousarray(a))
        scales.append(float(sc))
    ref = F.avg_pool2d(torch.cat(parts, 1), 2).permute(0, 2, 3, 1).contiguous()
    n_in = ref.shape[-1]
    cpad = 4 if n_in <= 4 else 8
    n = len(table)
    y = np.full((4, H // 2, W // 2, cpad), np.nan, dtype=np.float32)
    vec = C.c_int(-1)
    rc = lib.hc_ingest_table((C.c_void_p * n)(*[s.ctypes.data for s in sensors]), (C.c_int * n)(*[t[0] for t in table]),
                             (C.c_int * n)(*[t[1] for t in table]), (C.c_float * n)(*scales), n, C.c_void_p(rows.ctypes.data),
                             C.c_void_p(y.ctypes.data), 4, H, W, cpad, C.byref(vec))
    assert rc == 0
    assert torch.equal(torch.from_numpy(y[..., :n_in]), ref), "scaling + 2x2 average must be bitwise the reference's arithmetic"
    assert n_in == cpad or float(np.abs(y[..., n_in:]).max()) == 0.0
    # even W: every uint8 x 3 / float32 x 1 sensor is read in paired-tap units; odd W: element loads only -- both forms are covered
    paired = sum(1 for dt, ch, _ in table if (dt, ch) in ((U8c, 3), (F32c, 1)))
    assert vec.value == (paired if W % 2 == 0 else 0)
