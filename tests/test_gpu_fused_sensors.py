"""Named visual sensors and raw-fused 1-D sensors of PointNavResNetPolicy on the GPU: the table-driven observation ingest (bitwise
against F.avg_pool2d on the scaled inputs), the fused gather, the engine with fused sensors blind and sighted (forward, backward, act),
PPO.update on such a space and the trainer end to end on the host env's `task="rearrange"` observation set.

The reference of the recurrent input is written here from the oracle's own pieces: the embeddings and torch.cat in the order
[visual_fc output | fused values | goal embeddings | previous-action embedding] (PointNavResNetNet.forward, resnet_policy.py:625-767 with
`fuse_keys`), then oracle.functional.rnn_forward and heads / gaussian_head.  With no fused sensor it must equal
oracle.functional.evaluate_actions (test_reference_without_fused_sensors_is_the_oracle, no GPU needed).  Bar: the project's 1e-4 relative
(max|got - ref| / max(floor, max|ref|), floor 1e-3 for outputs, 1e-4 for gradients)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import functional as O
from oracle.fixtures import det_params, resnet_param_shapes

GOAL = "pointgoal_with_gps_compass"
RN = "net.state_encoder.rnn."
U8, F32, I32 = 0, 1, 2  # HAB_DTYPE_*
GAUSS = dict(tanh=True, use_log_std=True, use_softplus=False, use_std_param=True, clamp_std=True, min_std=-5.0, max_std=2.0)  # raw (log) domain


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    from habitat_amd import _lib
    return _lib.lib()


def ck(code):
    from habitat_amd import _lib
    _lib.check(code)


def rel_err(got, ref, floor):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(floor, np.abs(ref).max()))


def rel_ok(got, ref, tol=1e-4, floor=1e-3):
    err = rel_err(got, ref, floor)
    print(f"    rel_err {err:.3e} (tol {tol:g})")
    return err <= tol


# ------------------------------------------------------------------------------------------------------------------------------------
# The reference: PointNavResNetNet.forward with fused sensors, from the oracle's pieces
# ------------------------------------------------------------------------------------------------------------------------------------
def ref_forward(p, spec, obs, fused_keys, h0, prev_actions, masks, training=False, taps=None, rmv_out=None):
    """(features, final hidden).  The parameters' dtype decides the precision (float64 for the blind cases); obs images stay what they are."""
    dt = p[RN + "weight_ih_l0"].dtype
    parts = []
    if spec.visual_keys:
        feats = O.resnet_encoder(p, "net.visual_encoder.", {k: obs[k] for k in spec.visual_keys}, spec.visual_keys, spec.backbone,
                                 spec.baseplanes, training, spec.normalize, taps, rmv_out)
        parts.append(F.relu(F.linear(feats.flatten(1), p["net.visual_fc.1.weight"], p["net.visual_fc.1.bias"])))
    parts += [obs[k].to(dt) for k in fused_keys]  # the raw values, behind visual_fc's output and in front of the embeddings
    if GOAL in obs:
        g = obs[GOAL].to(dt)
        g = torch.stack([g[:, 0], torch.cos(-g[:, 1]), torch.sin(-g[:, 1])], -1)
        parts.append(F.linear(g, p["net.tgt_embeding.weight"], p["net.tgt_embeding.bias"]))
    if spec.action_dist == "gaussian":
        parts.append(F.linear(masks.to(dt) * prev_actions.to(dt), p["net.prev_action_embedding.weight"], p["net.prev_action_embedding.bias"]))
    else:
        pa = prev_actions.squeeze(-1)
        pa = torch.where(masks.view(-1), pa + 1, torch.zeros_like(pa))
        parts.append(F.embedding(pa, p["net.prev_action_embedding.weight"]))
    x = torch.cat(parts, dim=1)
    if taps is not None:
        taps["rnn_in"] = x
    return O.rnn_forward(p, RN, spec.rnn_type, spec.num_layers, x, h0.to(dt), masks)


def ref_evaluate(p, spec, obs, fused_keys, h0, prev_actions, masks, action, training=True, taps=None, rmv_out=None):
    feats, hidden = ref_forward(p, spec, obs, fused_keys, h0, prev_actions, masks, training, taps, rmv_out)
    if spec.action_dist == "gaussian":
        mu, std, value = O.gaussian_head(p, spec, feats)
        return value, O.normal_log_prob(mu, std, action), O.normal_entropy(mu, std), hidden
    logits, probs, value = O.heads(p, feats)
    entropy = -(torch.clamp(logits, min=torch.finfo(logits.dtype).min) * probs).sum(-1, keepdim=True)
    return value, logits.gather(-1, action), entropy, hidden


def ref_act(p, spec, obs, fused_keys, h0, prev_actions, masks, noise):
    feats, hidden = ref_forward(p, spec, obs, fused_keys, h0, prev_actions, masks)
    if spec.action_dist == "gaussian":
        mu, std, value = O.gaussian_head(p, spec, feats)
        return value, mu + std * noise.to(mu.dtype), hidden
    logits, probs, value = O.heads(p, feats)
    return value, O.sample_actions(probs, noise), hidden


def blind_case(D, rnn_type, layers, gauss):
    widths = {0: (), 1: (1,), 10: (7, 1, 2), 16: (16,)}[D]
    return types.SimpleNamespace(D=D, widths=widths, rnn_type=rnn_type, layers=layers, gauss=gauss, hidden=64, T=4, n=3, A=3 if gauss else 4,
                                 Lh=layers * (2 if rnn_type == "LSTM" else 1))


def blind_shapes(c):
    """state_dict() names / shapes of the blind ResNet policy with the polar goal and c.D fused columns."""
    G = 3 if c.rnn_type == "GRU" else 4
    sh = [(k, s) for k, s in resnet_param_shapes(4, 64, 64, c.hidden, c.A, c.rnn_type, c.layers, normalize=False,
                                                 gauss=dict(use_std_param=True) if c.gauss else None)
          if not k.startswith(("net.visual_encoder.", "net.visual_fc."))]
    return [(k, (G * c.hidden, c.D + 64) if k == RN + "weight_ih_l0" else s) for k, s in sh]


def blind_inputs(c):
    T, n, B = c.T, c.n, c.T * c.n
    rng = np.random.default_rng(100 + 7 * c.D + c.layers)
    f32 = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    obs = {f"s{i}": f32(B, w) for i, w in enumerate(c.widths)}
    obs[GOAL] = torch.from_numpy(np.stack([rng.random(B) * 5, rng.uniform(-3.1, 3.1, B)], 1).astype(np.float32))
    masks = rng.random((T, n)) >= 0.3
    masks[1, 0] = masks[2, 1] = False  # episode starts inside the sequence
    masks[3, 0] = True
    inp = types.SimpleNamespace(obs=obs, fused_keys=[f"s{i}" for i in range(len(c.widths))], masks=torch.from_numpy(masks.reshape(B, 1)),
                                h0=f32(n, c.Lh, c.hidden), gouts=tuple(f32(B, 1) for _ in range(3)))
    if c.gauss:
        inp.actions, inp.prev_actions = f32(B, c.A), f32(B, c.A)
        inp.noise = f32(n, c.A)
    else:
        inp.actions, inp.prev_actions = torch.from_numpy(rng.integers(0, c.A, (B, 1))), torch.from_numpy(rng.integers(0, c.A, (B, 1)))
        inp.noise = torch.from_numpy(rng.exponential(1.0, (n, c.A)).astype(np.float32))
    return inp


def blind_spec(c):
    return O.NetSpec(kind="resnet", rnn_type=c.rnn_type, num_layers=c.layers, visual_keys=(), normalize=False, num_actions=c.A, hidden=c.hidden,
                     action_dist="gaussian" if c.gauss else "categorical", gauss=GAUSS if c.gauss else None)


@pytest.mark.parametrize("rnn_type,layers,gauss", [("GRU", 1, False), ("LSTM", 2, False), ("GRU", 1, True)])
def test_reference_without_fused_sensors_is_the_oracle(rnn_type, layers, gauss):
    """CPU: with D = 0 the reference above is oracle.functional.evaluate_actions (same operations in the same order, fp32)."""
    c = blind_case(0, rnn_type, layers, gauss)
    params, inp, spec = det_params(blind_shapes(c), 5), blind_inputs(c), blind_spec(c)
    with torch.no_grad():
        mine = ref_evaluate(params, spec, inp.obs, [], inp.h0, inp.prev_actions, inp.masks, inp.actions)
        ref = O.evaluate_actions(params, spec, inp.obs, inp.h0, inp.prev_actions, inp.masks, inp.actions)
    for a, b in zip(mine, ref):
        assert a.dtype == b.dtype and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. Ingest, bitwise
# ------------------------------------------------------------------------------------------------------------------------------------
SENSOR_SETS = {"f1f1": [(F32, 1), (F32, 1)], "f1u3": [(F32, 1), (U8, 3)], "u3f1u3f1": [(U8, 3), (F32, 1), (U8, 3), (F32, 1)],
               "i1u3f1": [(I32, 1), (U8, 3), (F32, 1)],
               # beside the sets above: an int32 sensor and a two-channel float32 sensor on the table-driven kernel
               "i1f1f1": [(I32, 1), (F32, 1), (F32, 1)], "f2u3": [(F32, 2), (U8, 3)]}


def make_sensor(rng, dt, ch, nrows, H, W, high=255):
    if dt == U8:
        return torch.from_numpy(rng.integers(0, high + 1, (nrows, H, W, ch), dtype=np.uint8))
    if dt == I32:
        return torch.from_numpy(rng.integers(0, 40, (nrows, H, W, ch)).astype(np.int32))
    return torch.from_numpy(rng.random((nrows, H, W, ch), dtype=np.float32))


def call_ingest(L, sensors, table, scales, rows, B, H, W, cpad, **kw):
    n = len(table)
    dev = [s.cuda() for s in sensors]
    ptrs = (C.c_void_p * n)(*[d.data_ptr() for d in dev])
    dts, chs, scs = (C.c_int32 * n)(*[t[0] for t in table]), (C.c_int32 * n)(*[t[1] for t in table]), (C.c_float * n)(*scales)
    y = torch.full((B, H // 2, W // 2, cpad), float("nan"), device="cuda")
    nb = C.c_int(0)
    ck(L.hab_obs_ingest_pool_sensors(ptrs, dts, chs, scs, n, P(rows.cuda()), P(y), B, H, W, cpad, P(kw.get("mean")), P(kw.get("var")),
                                     P(kw.get("pivot")), P(kw.get("partial")), C.byref(nb) if kw.get("partial") is not None else None, S()))
    torch.cuda.synchronize()
    return y.cpu(), nb.value


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(20, 24), (21, 27)])
@pytest.mark.parametrize("name", list(SENSOR_SETS))
def test_ingest_sensor_table_bitwise(L, name, H, W):
    """7 arena rows, 4 frames through rows[] with one row twice, even and odd sizes (the pool floors): the pooled tensor equals
    oracle.functional.resnet_input bit for bit, padding channels are zero; the evaluation-mode normalisation and the training-mode moments
    against float64 at the tolerances of test_gpu_kernels.py::test_ingest_and_running_mean_var."""
    table = SENSOR_SETS[name]
    rng = np.random.default_rng(3)
    nrows, B = 7, 4
    rows = torch.tensor([3, 0, 3, 5], dtype=torch.int32)
    sensors = [make_sensor(rng, dt, ch, nrows, H, W) for dt, ch in table]
    keys = [f"s{i}" for i in range(len(table))]
    x_ref = O.resnet_input({k: s[rows.long()] for k, s in zip(keys, sensors)}, keys)  # (B, C, H/2, W/2)
    n_in = x_ref.shape[1]
    cpad = 4 if n_in <= 4 else 8
    ref = x_ref.permute(0, 2, 3, 1).contiguous()
    scales = [float(np.float32(1.0 / 255.0)) if dt == U8 else 1.0 for dt, _ in table]
    y, _ = call_ingest(L, sensors, table, scales, rows, B, H, W, cpad)
    assert torch.equal(y[..., :n_in], ref), "scaling + 2x2 average must be bitwise the reference's arithmetic"
    assert n_in == cpad or float(y[..., n_in:].abs().max()) == 0.0
    # evaluation-mode RunningMeanAndVar fused into the pass
    mean, var = torch.rand(n_in), torch.rand(n_in) * 0.1
    yn, _ = call_ingest(L, sensors, table, scales, rows, B, H, W, cpad, mean=mean.cuda(), var=var.cuda())
    want = (ref.double() - mean.double()) * torch.rsqrt(torch.clamp(var.double(), min=1e-2))
    assert torch.allclose(yn[..., :n_in].double(), want, rtol=1e-5, atol=1e-5)
    assert n_in == cpad or float(yn[..., n_in:].abs().max()) == 0.0
    # training-mode moments about a pivot, accumulated by the same pass
    pivot = torch.rand(n_in)
    partial = torch.zeros(2048 * 16, dtype=torch.float64, device="cuda")
    ym, nb = call_ingest(L, sensors, table, scales, rows, B, H, W, cpad, pivot=pivot.cuda(), partial=partial)
    assert torch.equal(ym[..., :n_in], ref) and 1 <= nb <= 2048
    sums = partial.cpu().view(2048, 16)[:nb].sum(0)
    npix = B * (H // 2) * (W // 2)
    flat = ref.double().view(-1, n_in)
    b_mean = pivot.double() + sums[:n_in] / npix
    d = b_mean - pivot.double()
    b_var = (sums[8:8 + n_in] - 2 * d * sums[:n_in] + npix * d * d) / npix
    assert torch.allclose(b_mean, flat.mean(0), rtol=1e-5, atol=1e-6)
    assert torch.allclose(b_var, flat.var(0, unbiased=False), rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(20, 24), (21, 27)])
def test_ingest_uint8_scale_from_the_space(L, H, W):
    """A uint8 sensor whose high.max() is 100 is multiplied with fp32(1 / 100): bitwise F.avg_pool2d of the scaled values."""
    rng = np.random.default_rng(4)
    table = [(U8, 3), (F32, 1)]
    rows = torch.tensor([3, 0, 3, 5], dtype=torch.int32)
    sensors = [make_sensor(rng, U8, 3, 7, H, W, high=100), make_sensor(rng, F32, 1, 7, H, W)]
    sc = np.float32(1.0 / 100.0)
    x = torch.cat([sensors[0][rows.long()].permute(0, 3, 1, 2).float() * float(sc), sensors[1][rows.long()].permute(0, 3, 1, 2)], 1)
    ref = F.avg_pool2d(x, 2).permute(0, 2, 3, 1).contiguous()
    y, _ = call_ingest(L, sensors, table, [float(sc), 1.0], rows, 4, H, W, 4)
    assert torch.equal(y, ref)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. Fused gather
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("use_rows", [False, True])
@pytest.mark.parametrize("widths", [(1,), (7, 1, 2), (16,), (33, 3)])
def test_fused_gather(L, widths, use_rows):
    rng = np.random.default_rng(5)
    nrows, B, col0 = 300, 270, 64
    D = sum(widths)
    rnn_in = col0 + D + 32
    ld = (rnn_in + 15) & ~15
    srcs = [torch.from_numpy(rng.standard_normal((nrows, w)).astype(np.float32)) for w in widths]
    rows = torch.from_numpy(rng.permutation(nrows)[:B].astype(np.int32)) if use_rows else None
    dev = [s.cuda() for s in srcs]
    n = len(widths)
    dst = torch.full((B, ld), float("nan"), device="cuda")
    ck(L.hab_fused_gather((C.c_void_p * n)(*[d.data_ptr() for d in dev]), (C.c_int32 * n)(*widths), n, P(rows.cuda() if use_rows else None),
                          P(dst), ld, col0, rnn_in, ld - rnn_in, B, S()))
    got = dst.cpu()
    idx = rows.long() if use_rows else torch.arange(B)
    assert torch.equal(got[:, col0:col0 + D], torch.cat([s[idx] for s in srcs], 1))
    assert ld == rnn_in or float(got[:, rnn_in:].abs().max()) == 0.0  # padding columns exactly zero
    assert bool(torch.isnan(got[:, :col0]).all()) and bool(torch.isnan(got[:, col0 + D:rnn_in]).all()), "columns of other producers are untouched"


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. Blind ResNet engine with fused sensors
# ------------------------------------------------------------------------------------------------------------------------------------
BLIND_CASES = [blind_case(D, r, l, False) for D in (1, 10, 16) for r, l in (("GRU", 1), ("LSTM", 2))] + [blind_case(10, "GRU", 1, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("c", BLIND_CASES, ids=lambda c: f"D{c.D}-{c.rnn_type}{c.layers}" + ("-gauss" if c.gauss else ""))
def test_blind_engine_with_fused_sensors(c):
    from habitat_amd import _lib
    from habitat_amd.engine import DevicePackInfo, PolicyEngine
    T, n, B, hidden = c.T, c.n, c.T * c.n, c.hidden
    kw = dict(arch="resnet", rnn_type=c.rnn_type, rnn_layers=c.layers, hidden=hidden, num_actions=c.A, H=0, W=0, has_rgb=False, has_depth=False,
              goal_dim=2, max_frames=B, max_envs=n, visual_order=(), fused_widths=c.widths)
    if c.gauss:
        kw.update(action_dist="gaussian", gauss_flags=_lib.GAUSS_TANH_MU | _lib.GAUSS_USE_LOG_STD | _lib.GAUSS_CLAMP_STD | _lib.GAUSS_USE_STD_PARAM,
                  gauss_min_std=GAUSS["min_std"], gauss_max_std=GAUSS["max_std"])
    eng = PolicyEngine(**kw)
    shapes = blind_shapes(c)
    assert [(nm, shp) for nm, shp, _ in eng.specs] == [(k, tuple(s)) for k, s in shapes]
    params = det_params(shapes, 11)
    eng.load({k: v.cuda() for k, v in params.items()})
    inp, spec = blind_inputs(c), blind_spec(c)
    rnn_in = c.D + 64
    # float64 reference
    p = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    taps = {}
    v, lp, ent, hfin = ref_evaluate(p, spec, inp.obs, inp.fused_keys, inp.h0, inp.prev_actions, inp.masks,
                                    inp.actions.double() if c.gauss else inp.actions, taps=taps)
    gv, glp, gent = inp.gouts
    ((v * gv.double()).sum() + (lp.double() * glp.double()).sum() + (ent.double() * gent.double()).sum()).backward()
    # engine
    cu = lambda t: t.cuda()
    extra = {"fused": [cu(inp.obs[k]) for k in inp.fused_keys]}
    goal, masks, actions, prev, h0 = cu(inp.obs[GOAL]), cu(inp.masks), cu(inp.actions), cu(inp.prev_actions), cu(inp.h0)
    pack = DevicePackInfo(np.logical_not(inp.masks.view(T, n).numpy()), "cuda")
    dv, dl, de = (torch.full((B,), float("nan"), device="cuda") for _ in range(3))
    hf = torch.full((n, c.Lh, hidden), float("nan"), device="cuda")
    eng.evaluate(None, None, goal, None, h0, masks, actions, pack, B, n, value=dv, log_prob=dl, entropy=de, prev_actions=prev, extra=extra)
    eng.final_hidden(hf)
    x = eng.tap(3).view(B, -1).clone()  # HAB_TAP_RNN_IN
    eng.backward(None, None, goal, None, actions, pack, *(cu(g.view(-1).contiguous()) for g in inp.gouts), prev_actions=prev, extra=extra)
    torch.cuda.synchronize()
    assert x.shape[1] == (rnn_in + 15) // 16 * 16 and not bool(x[:, rnn_in:].any()), "padding columns of the recurrent input"
    assert torch.equal(x[:, :c.D].cpu(), torch.cat([inp.obs[k] for k in inp.fused_keys], 1)), "fused values are copied, not computed"
    bad = []
    for name, got, ref in (("rnn_in", x[:, :rnn_in], taps["rnn_in"]), ("value", dv, v.view(-1)), ("log_prob", dl, lp.view(-1)),
                           ("entropy", de, ent.view(-1)), ("final_hidden", hf, hfin)):
        e = rel_err(got.cpu().numpy(), ref.detach().numpy(), 1e-3)
        print(f"  {name}: {e:.3e}")
        if not e <= 1e-4:
            bad.append((name, e))
    for k, g in eng.grad_views.items():
        ref = p[k].grad.numpy()
        assert np.abs(ref).max() >= 1e-3, ("reference gradient too small for the floor: change the inputs", k)
        e = rel_err(g.cpu().numpy(), ref, 1e-4)
        print(f"  grad/{k}: {e:.3e}")
        if not e <= 1e-4:
            bad.append((k, e))
    assert not bad, bad
    # act on the first step's n frames
    o1 = {k: t[:n] for k, t in inp.obs.items()}
    pd = {k: t.detach() for k, t in p.items()}
    with torch.no_grad():
        rv, ra, rh = ref_act(pd, spec, o1, inp.fused_keys, inp.h0, inp.prev_actions[:n], inp.masks[:n], inp.noise)
    values = torch.full((n, 1), float("nan"), device="cuda")
    acts = torch.zeros((n, c.A), device="cuda") if c.gauss else torch.zeros((n, 1), dtype=torch.long, device="cuda")
    alp, hout = torch.zeros(n, 1, device="cuda"), torch.full((n, c.Lh, hidden), float("nan"), device="cuda")
    eng.act(None, None, goal[:n].contiguous(), h0, masks[:n].contiguous(), n, exp_noise=cu(inp.noise), values=values, actions=acts,
            action_log_probs=alp, hidden_out=hout, prev_actions=prev[:n].contiguous(), extra={"fused": [t[:n].contiguous() for t in extra["fused"]]})
    torch.cuda.synchronize()
    if c.gauss:
        assert rel_ok(acts.cpu().numpy(), ra.numpy())
    else:
        assert torch.equal(acts.cpu(), ra)
    assert rel_ok(values.cpu().numpy(), rv.numpy()) and rel_ok(hout.cpu().numpy(), rh.numpy())


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. Sighted
# ------------------------------------------------------------------------------------------------------------------------------------
def sighted_space(S_, cams, H, W):
    d = {}
    for k in cams:
        d[k] = S_.Box(0, 255, (H, W, 3), np.uint8) if k.endswith("rgb") else S_.Box(0.0, 1.0, (H, W, 1), np.float32)
    d["joint"] = S_.Box(-1e9, 1e9, (7,), np.float32)
    d["is_holding"] = S_.Box(0.0, 1.0, (1,), np.float32)
    d[GOAL] = S_.Box(-1e9, 1e9, (2,), np.float32)
    return S_.Dict(d)


def sighted_inputs(seed, cams, H, W, B, n, Lh, hidden):
    rng = np.random.default_rng(seed)
    obs = {}
    for k in cams:
        obs[k] = (torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)) if k.endswith("rgb")
                  else torch.from_numpy(rng.random((B, H, W, 1), dtype=np.float32)))
    obs["joint"] = torch.from_numpy(rng.uniform(-2, 2, (B, 7)).astype(np.float32))
    obs["is_holding"] = torch.from_numpy((rng.random((B, 1)) < 0.5).astype(np.float32))
    obs[GOAL] = torch.from_numpy(np.stack([rng.random(B) * 5, rng.uniform(-3.1, 3.1, B)], 1).astype(np.float32))
    masks = torch.from_numpy(rng.random((B, 1)) > 0.3)
    actions = torch.from_numpy(rng.integers(0, 4, (B, 1)))
    prev_actions = torch.from_numpy(rng.integers(0, 4, (B, 1)))
    h0 = torch.from_numpy(rng.standard_normal((n, Lh, hidden)).astype(np.float32))
    return rng, obs, masks, actions, prev_actions, h0


@pytest.fixture
def single_thread_oracle():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


TWO_DEPTH, FOUR_CAMS = ("head_depth", "arm_depth"), ("head_rgb", "head_depth", "arm_rgb", "arm_depth")
# (cameras, normalize_visual_inputs, rnn, layers, H, W, input seed): the seed is the first draw of 1..60 whose smallest oracle |pre-ReLU|
# exceeds 2e-5 with one oracle thread (the scheme of tests/test_gpu_policy.py::test_resnet_engine_vs_oracle), found on the CPU by
# sighted_seed_search below and recorded here
SIGHTED = [(TWO_DEPTH, True, "LSTM", 2, 64, 96, 31), (TWO_DEPTH, True, "LSTM", 2, 62, 30, 4),
           (FOUR_CAMS, False, "GRU", 1, 64, 96, 47), (FOUR_CAMS, False, "GRU", 1, 62, 30, 5)]


def sighted_setup(cams, normalize, rnn_type, layers, H, W):
    hidden, T, n = 64, 3, 2
    n_in = sum(3 if k.endswith("rgb") else 1 for k in cams)
    G = 3 if rnn_type == "GRU" else 4
    shapes = [(k, (G * hidden, hidden + 8 + 64) if k == RN + "weight_ih_l0" else s)
              for k, s in resnet_param_shapes(n_in, H, W, hidden, rnn_type=rnn_type, layers=layers)]
    params = det_params(shapes, 31)
    pre = "net.visual_encoder.running_mean_and_var."
    if normalize:
        params[pre + "_mean"], params[pre + "_var"], params[pre + "_count"] = (
            torch.full((1, n_in, 1, 1), 0.3), torch.full((1, n_in, 1, 1), 0.05), torch.tensor(6.0))
        order = [k for k, _ in resnet_param_shapes(n_in, H, W, hidden, rnn_type=rnn_type, layers=layers, normalize=True, with_buffers=True)]
        params = {k: params[k] for k in order}
    spec = O.NetSpec(kind="resnet", rnn_type=rnn_type, num_layers=layers, backbone="resnet18", baseplanes=32, visual_keys=cams,
                     normalize=normalize, hidden=hidden)
    return hidden, T, n, n_in, params, spec, layers * (2 if rnn_type == "LSTM" else 1)


def sighted_seed_search(cams, normalize, rnn_type, layers, H, W):
    """-> (seed, margin): first input draw of seeds 1..60 whose smallest |pre-ReLU| clears 2e-5, else the best one."""
    hidden, T, n, n_in, params, spec, Lh = sighted_setup(cams, normalize, rnn_type, layers, H, W)
    orig_relu, best = F.relu, None
    for seed in range(1, 61):
        rng, obs, masks, actions, prev_actions, h0 = sighted_inputs(seed, cams, H, W, T * n, n, Lh, hidden)
        margin = [np.inf]

        def relu_probe(x, inplace=False):
            margin[0] = min(margin[0], float(x.detach().abs().min()))
            return orig_relu(x)

        F.relu = relu_probe
        try:
            with torch.no_grad():
                ref_evaluate(params, spec, obs, ["joint", "is_holding"], h0, prev_actions, masks, actions, training=True)
        finally:
            F.relu = orig_relu
        if best is None or margin[0] > best[1]:
            best = (seed, margin[0])
        if margin[0] > 2e-5:
            break
    return best


@pytest.mark.gpu
@pytest.mark.parametrize("cams,normalize,rnn_type,layers,H,W,seed", SIGHTED,
                         ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_sighted_engine_with_named_cameras_and_fused_sensors(cams, normalize, rnn_type, layers, H, W, seed, single_thread_oracle):
    from habitat_amd.common import spaces as S_
    from habitat_amd.engine import DevicePackInfo
    from habitat_amd.rl.ppo import PointNavResNetPolicy
    hidden, T, n, n_in, params, spec, Lh = sighted_setup(cams, normalize, rnn_type, layers, H, W)
    B = T * n
    fused = ["joint", "is_holding"]
    pol = PointNavResNetPolicy(sighted_space(S_, cams, H, W), S_.Discrete(4), hidden_size=hidden, num_recurrent_layers=layers, rnn_type=rnn_type,
                               backbone="resnet18", normalize_visual_inputs=normalize, max_frames=B, max_envs=n)
    assert list(pol.state_dict().keys()) == list(params.keys())
    pol.load_state_dict(params)
    pol.to("cuda")
    pol.train()
    eng = pol.engine
    is_buffer = lambda k: "running_mean_and_var" in k
    rng, obs, masks, actions, prev_actions, h0 = sighted_inputs(seed, cams, H, W, B, n, Lh, hidden)
    p = {k: (v.clone().requires_grad_(True) if not is_buffer(k) else v.clone()) for k, v in params.items()}
    taps, rmv = {}, {}
    v, lp, ent, hfin = ref_evaluate(p, spec, obs, fused, h0, prev_actions, masks, actions, training=True, taps=taps, rmv_out=rmv)
    gv, glp, gent = (torch.from_numpy(rng.standard_normal((B, 1)).astype(np.float32)) for _ in range(3))
    ((v * gv).sum() + (lp * glp).sum() + (ent * gent).sum()).backward()
    pack = DevicePackInfo(np.logical_not(masks.view(T, n).numpy()), "cuda")
    dobs = {k: t.cuda() for k, t in obs.items()}
    rgb, depth, goal, extra = pol._obs_ptrs(dobs)
    assert rgb is None and depth is None and len(extra["visual"]) == len(cams) and len(extra["fused"]) == 2
    dv, dl, de = (torch.zeros(B, device="cuda") for _ in range(3))
    eng.evaluate(None, None, goal, None, h0.cuda(), masks.cuda(), actions.cuda(), pack, B, n, value=dv, log_prob=dl, entropy=de,
                 prev_actions=prev_actions.cuda(), extra=extra)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().numpy()
    cpad = 4 if n_in <= 4 else 8
    x0 = eng.tap(5).cpu().numpy().reshape(B, H // 2, W // 2, cpad)[..., :n_in]
    assert rel_ok(x0, nhwc(taps["enc_in"])), "encoder input (ingest + RunningMeanAndVar)"
    for tap_id, name in ((6, "stem"), (7, "pool"), (9, "layer1"), (10, "layer2"), (11, "layer3"), (12, "layer4"), (8, "compression")):
        ref = nhwc(taps[name])
        assert rel_ok(eng.tap(tap_id).cpu().numpy().reshape(ref.shape), ref), name
    rnn_in = hidden + 8 + 64
    xin = eng.tap(3).cpu().view(B, -1)
    assert xin.shape[1] == (rnn_in + 15) // 16 * 16 and not bool(xin[:, rnn_in:].any())
    assert rel_ok(xin[:, :rnn_in].numpy(), taps["rnn_in"].detach().numpy()), "rnn_in"
    assert rel_ok(dv.cpu().numpy(), v.detach().numpy().reshape(-1)) and rel_ok(dl.cpu().numpy(), lp.detach().numpy().reshape(-1))
    assert rel_ok(de.cpu().numpy(), ent.detach().numpy().reshape(-1))
    hf = torch.zeros(n, Lh, hidden, device="cuda")
    eng.final_hidden(hf)
    assert rel_ok(hf.cpu().numpy(), hfin.detach().numpy())
    pre = "net.visual_encoder.running_mean_and_var."
    if normalize:
        sd = pol.state_dict()
        for k in ("mean", "var", "count"):
            assert rel_ok(sd[pre + "_" + k].cpu().numpy(), rmv[k].numpy(), tol=1e-5), k
    eng.backward(None, None, goal, None, actions.cuda(), pack, gv.view(-1).cuda(), glp.view(-1).cuda(), gent.view(-1).cuda(),
                 prev_actions=prev_actions.cuda(), extra=extra)
    bad = [(k, float((g.cpu() - p[k].grad).abs().max()), float(p[k].grad.abs().max())) for k, g in eng.grad_views.items()
           if not is_buffer(k) and not rel_ok(g.cpu().numpy(), p[k].grad.numpy(), tol=1e-4, floor=1e-4)]
    assert not bad, bad
    # eval mode: act() on n envs equals the reference
    pol.eval()
    o1 = {k: t[:n].contiguous() for k, t in dobs.items()}
    noise = torch.from_numpy(rng.exponential(1.0, (n, 4)).astype(np.float32))
    ad = pol.act(o1, h0.cuda(), prev_actions[:n].cuda(), masks[:n].cuda(), exp_noise=noise.cuda())
    pp = {k: t.detach() for k, t in p.items()}
    pp.update({pre + "_" + k: val for k, val in rmv.items()})
    with torch.no_grad():
        rv, ra, rh = ref_act(pp, spec, {k: t[:n] for k, t in obs.items()}, fused, h0, prev_actions[:n], masks[:n], noise)
    assert torch.equal(ad.actions.cpu(), ra)
    assert rel_ok(ad.values.cpu().numpy(), rv.numpy()) and rel_ok(ad.rnn_hidden_states.cpu().numpy(), rh.numpy())


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. PPO.update
# ------------------------------------------------------------------------------------------------------------------------------------
def rearrange_space(S_, H, W):
    f = np.float32
    return S_.Dict({"head_depth": S_.Box(0.0, 1.0, (H, W, 1), f), "arm_depth": S_.Box(0.0, 1.0, (H, W, 1), f), "joint": S_.Box(-1e9, 1e9, (7,), f),
                    "is_holding": S_.Box(0.0, 1.0, (1,), f), "goal_to_agent_gps_compass": S_.Box(-1e9, 1e9, (2,), f)})


@pytest.mark.gpu
@pytest.mark.parametrize("gauss", [False, True], ids=["discrete", "gaussian"])
def test_ppo_update_rows_path_matches_autograd_bridge(gauss):
    """Storage filled through policy.act on the 2-camera + fused space (4 envs x 8 steps, 2 minibatches): the learner's rows-indirected
    evaluate / fused loss / backward and the autograd bridge (dense batch, torch loss, loss.backward()) give the same gradients to the
    bound of tests/test_gpu_policy.py::test_autograd_bridge_matches_fused_path (1e-4, floor 1e-4); then PPO.update itself runs."""
    from habitat_amd import _lib
    from habitat_amd.common import spaces as S_
    from habitat_amd.common.rollout_storage import RolloutStorage
    from habitat_amd.rl.ppo import PPO, PointNavResNetPolicy
    from oracle.ref_loader import make_config
    H = W = 64
    T, N, hidden = 8, 4, 64
    osp = rearrange_space(S_, H, W)
    asp = S_.Box(-1.0, 1.0, (3,), np.float32) if gauss else S_.Discrete(4)
    pcfg = None
    if gauss:
        pcfg = types.SimpleNamespace(action_distribution_type="gaussian",
                                     action_dist=dict(use_log_std=True, use_softplus=False, log_std_init=0.0, use_std_param=True, clamp_std=True,
                                                      min_std=1e-6, max_std=1, min_log_std=-5, max_log_std=2, action_activation="tanh"))
    torch.manual_seed(7)
    pol = PointNavResNetPolicy(osp, asp, hidden_size=hidden, backbone="resnet18", policy_config=pcfg, max_frames=T * N, max_envs=N)
    pol.to("cuda")
    st = RolloutStorage(T, N, osp, asp, pol, device="cuda", gae_variant="scan")
    rng = np.random.default_rng(9)

    def draw_obs():
        return {k: torch.from_numpy(rng.random((N, *sp.shape)).astype(np.float32)).cuda() for k, sp in osp.spaces.items()}

    st.insert_first_observations(draw_obs())
    pol.eval()
    for t in range(T):
        step = st.get_current_step(slice(0, N), 0)
        ad = pol.act(step["observations"], step["recurrent_hidden_states"], step["prev_actions"], step["masks"])
        st.insert(next_recurrent_hidden_states=ad.rnn_hidden_states, actions=ad.actions, action_log_probs=ad.action_log_probs,
                  value_preds=ad.values)
        st.insert(next_observations=draw_obs(), rewards=torch.from_numpy(rng.standard_normal((N, 1)).astype(np.float32)).cuda(),
                  next_masks=torch.from_numpy(rng.random((N, 1)) > 0.2).cuda())
        st.advance_rollout()
    last = st.get_last_step()
    st.compute_returns(pol.get_value(last["observations"], last["recurrent_hidden_states"], last["prev_actions"], last["masks"]), True, 0.99, 0.95)
    cfg = make_config(num_mini_batch=2, ppo_epoch=1, num_steps=T, hidden_size=hidden)
    pol.train()
    ppo = PPO.from_config(pol, cfg)
    adv = ppo.get_advantages(st)
    torch.manual_seed(3)
    batch = next(st.data_generator(adv, cfg.num_mini_batch))
    eng, Bf = pol.engine, st.buffers
    Bn = batch.T * batch.n
    # the learner's path: observations read in place through rows[]
    rgb, depth, goal, extra = pol._obs_ptrs(Bf["observations"])
    assert [t.data_ptr() for t in extra["visual"]] == [Bf["observations"][k].data_ptr() for k in ("head_depth", "arm_depth")]
    assert [t.data_ptr() for t in extra["fused"]] == [Bf["observations"][k].data_ptr() for k in ("joint", "is_holding", "goal_to_agent_gps_compass")]
    v, lp, ent, dv, dlp, dent = (torch.zeros(Bn, device="cuda") for _ in range(6))
    out = torch.zeros(24, device="cuda")
    eng.evaluate(rgb, depth, goal, batch.rows, Bf["recurrent_hidden_states"], Bf["masks"], Bf["actions"], batch.pack, Bn, batch.n, value=v,
                 log_prob=lp, entropy=ent, prev_actions=Bf["prev_actions"], extra=extra)
    _lib.check(_lib.lib().hab_ppo_loss(P(v), P(lp), P(ent), P(Bf["action_log_probs"]), P(adv), P(Bf["value_preds"]), P(Bf["returns"]),
                                       P(batch.rows), Bn, cfg.clip_param, cfg.value_loss_coef, cfg.entropy_coef,
                                       int(cfg.use_clipped_value_loss), P(dv), P(dlp), P(dent), P(out), _lib.stream_ptr()))
    eng.backward(rgb, depth, goal, batch.rows, Bf["actions"], batch.pack, dv, dlp, dent, prev_actions=Bf["prev_actions"], extra=extra)
    fused_grads = {k: g.clone() for k, g in eng.grad_views.items()}
    fused_losses = out[:4].cpu().numpy()
    # the bridge: dense gathered batch, torch loss, autograd
    bv, blp, bent, _, _ = pol.evaluate_actions(batch["observations"], batch["recurrent_hidden_states"], batch["prev_actions"], batch["masks"],
                                               batch["actions"], batch["rnn_build_seq_info"])
    b = {k: batch[k] for k in ("action_log_probs", "advantages", "value_preds", "returns")}
    total, vl, al, dent_, _ = O.ppo_loss(bv, blp, bent, b, cfg.clip_param, cfg.value_loss_coef, cfg.entropy_coef, cfg.use_clipped_value_loss)
    for p_ in pol.parameters():
        p_.grad = None
    total.backward()
    assert np.allclose(np.array([vl.item(), al.item(), dent_.item(), total.item()]), fused_losses, rtol=1e-4, atol=1e-6)
    for k, p_ in pol.named_parameters():
        assert rel_ok(p_.grad.cpu().numpy(), fused_grads[k].cpu().numpy(), tol=1e-4, floor=1e-4), k
    # and the updater end to end
    for k, p_ in pol.named_parameters():
        p_.grad = eng.grad_views[k]
    before = eng.params_flat.clone()
    losses = ppo.update(st)
    assert all(np.isfinite(x) for x in losses.values()), losses
    assert float((eng.params_flat - before).abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. Trainer
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_trainer_on_rearrange_host_env(tmp_path):
    """Two update cycles through the YAML entry point with worker processes running the host env's `task="rearrange"` observation set
    (64 x 64, hidden 64, 2 envs x 4 steps): finite losses, parameters move, a checkpoint round-trips."""
    from habitat_amd.config.default import get_config
    from habitat_amd.common.baseline_registry import baseline_registry
    import habitat_amd.rl.ppo.ppo_trainer  # noqa: F401
    N, T, size = 2, 4, 64
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=3",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          "habitat_baselines.rl.ppo.hidden_size=64", f"habitat_baselines.checkpoint_folder={tmp_path}",
          "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000", "habitat_baselines.rl.ddppo.backbone=resnet18",
          "habitat_baselines.rl.ppo.num_mini_batch=1",
          "habitat_baselines.vector_env_factory._target_=habitat_amd.common.env_factory.ProcessVectorEnvFactory",
          "habitat_baselines.vector_env_factory.make_env_fn=habitat_amd.core.host_env.make_rearrange_host_env"]
    for sname in ("rgb", "depth"):
        ov += [f"habitat.simulator.sensors.{sname}.height={size}", f"habitat.simulator.sensors.{sname}.width={size}"]
    cfg = get_config("pointnav/ddppo_pointnav.yaml", ov)
    cfg.habitat.simulator.sensors.pop("semantic", None)
    trainer = baseline_registry.get_trainer(cfg.habitat_baselines.trainer_name)(cfg)
    trainer._init_train()
    try:
        pol = trainer._agent.actor_critic
        assert [v[0] for v in pol.visual_sensors] == ["head_depth", "arm_depth"]
        assert [f[0] for f in pol.fused_sensors] == ["joint", "is_holding", "goal_to_agent_gps_compass"]
        assert pol.state_dict()["net.state_encoder.rnn.weight_ih_l0"].shape[1] == 64 + 10 + 32
        before = pol.engine.params_flat.clone()
        for _ in range(2):
            losses = trainer.run_update_cycle()
            assert all(np.isfinite(x) for x in losses.values()), losses
        assert trainer.num_steps_done == 2 * N * T and trainer.num_updates_done == 2
        assert float((pol.engine.params_flat - before).abs().max()) > 0
        trainer.save_checkpoint("ckpt.rearrange.pth")
        ckpt = trainer.load_checkpoint(os.path.join(str(tmp_path), "ckpt.rearrange.pth"), map_location="cpu")
        now = pol.state_dict()
        assert list(ckpt["state_dict"].keys()) == list(now.keys())
        assert all(torch.equal(ckpt["state_dict"][k], now[k].cpu()) for k in now)
        moved = {k: t + 1.0 for k, t in ckpt["state_dict"].items()}
        trainer._agent.load_ckpt_state_dict({"state_dict": moved})
        assert all(torch.equal(pol.state_dict()[k].cpu(), moved[k]) for k in moved)
    finally:
        trainer.envs.close()
