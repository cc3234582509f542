"""The recurrent encoder (csrc/rnn.hip, rnn_gates.h, rnn_persist.h) and the heads (csrc/heads.hip) against a plain float64 reference, at
the shapes no reference had seen: every hidden width of the 4-wave and 8-wave kernels (64 .. 1024: 1, 2, 3, 4, 5, 8 K-chunks per wave),
the layer wavefront at its last size (4) and the first layer count that falls back to layer by layer (5), one to sixteen row tiles with
ragged last ones (n = 256 = 16 tiles: the time-major form's fallback from the persistent kernel to step launches), T smaller than the
time-major chunk count, unbroken 128-step chains, every frame an episode start, saturated gates, the rollout step, the last action slots of
the padded heads (7, 8 actions; 1..4 Gaussian dimensions) and the refusals beside them.

The reference (ref_scan / ref_heads / ref_gauss_heads below) is ~80 lines of float64 torch with the semantics of the reference
implementation's rnn_state_encoder.py: the state entering step t is multiplied by masks[t]; no tiling, no packing.  Gradients are autograd
on it.  It is pinned on the CPU to oracle/functional.py (itself pinned to the live reference's goldens) to 1e-5, and four deliberately wrong
variants of it must each miss the tolerance by 10x or more under the same comparison function (test_wrong_reference_variants_are_caught):
that is the evidence that the comparison can fail.

Isolation: the reference is fed the ENGINE'S OWN recurrent input of the same evaluate (HAB_TAP_RNN_IN, cast to float64, padding columns
dropped), so recurrence + heads are compared alone; the gradients of net.state_encoder.rnn.*, action_distribution.* and critic.* given that
input are exactly the engine's.  Blind SimpleCNN engines (goal -> RNN -> heads: the packed form, the heads, act) have no other parameter,
so every gradient is compared there.  Blind ResNet engines (the only ones with a Gaussian head) also own embeddings in front of the
recurrence: those gradients are outside this file (tests/test_gpu_policy.py::test_blind_resnet_policy_vs_oracle).

Bar: the project's 1e-4 relative, measured as tests/test_gpu_policy.py::rel_ok does: max|got - ref| / max(floor, max|ref|) per tensor,
floor 1e-3 for outputs and 1e-4 for gradients.  No gradient tensor is skipped, and every compared gradient has max|ref| >= 10 x floor
(asserted), so the floor softens nothing -- except the tensors whose reference gradient is IDENTICALLY zero, which must be exactly zero in
the engine too: weight_hh when every frame starts an episode (the state entering every step is zero), and the actor of Discrete(1) (the
log-softmax of one logit is the constant 0).

Which time-major kernel ran (persistent at hidden 128 / 256 / 512 and <= 15 row tiles, step launches otherwise) cannot be asked of the
engine: RnnForm records chunks / wavefront only, and the HAB_PROBE_RNN_FWD bracket counts one event pair per layer and chunk in either
case.  The case ids name the kernel the dispatch code (rnn.hip: tm_persist_ok) selects; the one case that forces step launches does it
through matrix-path bit 12, as tests/test_gpu_rnn_persist.py does.

Largest error / tolerance per group measured on an MI355X (the run writes the per-test figures to parity_margins_rnn.json beside the other parity reports):
    widths 0.18, row tiles 0.15, layers 0.007, sequences (incl. saturated gates, p = 1) 0.008, act 0.015, heads 0.013
Layers, sequences, act and heads sit below 0.1 as whole groups (below 0.02).  The figures above 0.02 are all ONE tensor: critic.fc.bias,
whose gradient is the plain sum of the incoming value gradients -- at T = 13, n = 5 the test's 65 N(0, 1) draws sum to 0.022, so fp32
summation order shows at 1.8e-5 relative (four width cases share those draws and report the same figure); the fp32 CPU oracle in the
engine's place reads 0.02 .. 0.09 on the same cases.  Without that tensor every case is below 0.02.  The bar is not tightened here.
"""
import os
import types

import numpy as np
import pytest
import torch

from oracle import functional as O
from oracle.fixtures import baseline_param_shapes, det_params

GOAL = "pointgoal_with_gps_compass"
TOL, OUT_FLOOR, GRAD_FLOOR = 1e-4, 1e-3, 1e-4
STEP_LAUNCHES = 4096  # matrix-path bit 12
WIDTHS = [64, 128, 192, 256, 320, 384, 512, 640, 1024]
HEAD_PREFIXES = ("net.state_encoder.rnn.", "action_distribution.", "critic.")
GAUSS_OPTS = dict(tanh=True, use_log_std=True, use_softplus=False, clamp_std=True, min_std=-5.0, max_std=2.0)  # raw (log) domain

TENSOR_MARGINS = {}  # tensor name -> the same, over all tests
MARGINS = {}  # test id -> largest (error / tolerance) any comparison of that test saw; written to parity_margins_rnn.json (test_gpu_fullshape._report)


# ------------------------------------------------------------------------------------------------------------------------------------
# The float64 reference.  `wrong` selects one of four deliberate mistakes (test_wrong_reference_variants_are_caught), never used otherwise.
# ------------------------------------------------------------------------------------------------------------------------------------
def ref_gru_cell(x, h, w_ih, w_hh, b_ih, b_hh, wrong=None):
    H = h.shape[1]
    i_r, i_z, i_n = (x @ w_ih.T + b_ih).split(H, 1)
    h_r, h_z, h_n = (h @ w_hh.T).split(H, 1)
    b_r, b_z, b_n = b_hh.split(H)
    r = torch.sigmoid(i_r + h_r + b_r)
    z = torch.sigmoid(i_z + h_z + b_z)
    if wrong == "swap_rz":
        r, z = z, r
    if wrong == "bhn_outside":
        n = torch.tanh(i_n + r * h_n + b_n)
    else:
        n = torch.tanh(i_n + r * (h_n + b_n))
    return (1.0 - z) * n + z * h


def ref_lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    H = h.shape[1]
    i, f, g, o = (x @ w_ih.T + b_ih + h @ w_hh.T + b_hh).split(H, 1)
    c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c_new), c_new


def ref_scan(p, rnn_type, layers, x, h0, masks, wrong=None):
    """x (T, n, in), h0 (n, Lh, H) with the h layers first and then the c layers, masks (T, n) of 0 / 1: masks[t] multiplies the state that
    ENTERS step t.  Returns the last layer's output (T * n, H) in frame order and the final state (n, Lh, H)."""
    rn = "net.state_encoder.rnn."
    h = [h0[:, l] for l in range(layers)]
    c = [h0[:, layers + l] for l in range(layers)] if rnn_type == "LSTM" else []
    outs = []
    for t in range(x.shape[0]):
        m = masks[t].unsqueeze(1)
        inp = x[t]
        for l in range(layers):
            w = [p[f"{rn}{k}_l{l}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            h_in = h[l] if wrong == "mask_output" else h[l] * m
            if rnn_type == "GRU":
                h[l] = ref_gru_cell(inp, h_in, *w, wrong=wrong)
            else:
                c_in = c[l] if wrong in ("mask_output", "lstm_c_unmasked") else c[l] * m
                h[l], c[l] = ref_lstm_cell(inp, h_in, c_in, *w)
            if wrong == "mask_output":
                h[l] = h[l] * m
                if c:
                    c[l] = c[l] * m
            inp = h[l]
        outs.append(inp)
    return torch.cat(outs, 0), torch.stack(h + c, 1)


def ref_heads(p, feats, actions):
    """CriticHead + CategoricalNet: value, log-prob of `actions` (B, 1), entropy; each (B,)."""
    value = feats @ p["critic.fc.weight"].T + p["critic.fc.bias"]
    logits = feats @ p["action_distribution.linear.weight"].T + p["action_distribution.linear.bias"]
    logp_all = logits - torch.logsumexp(logits, 1, keepdim=True)
    entropy = -(logp_all.exp() * logp_all).sum(1)
    return value.view(-1), logp_all.gather(1, actions).view(-1), entropy, logp_all


def ref_gauss_heads(p, feats, actions, use_std_param):
    """GaussianNet with GAUSS_OPTS (tanh mean, clamped log-std) -> CustomNormal; actions (B, A) float64.  The distribution formulas are the
    oracle's own (normal_log_prob / normal_entropy keep the dtype they are given)."""
    value = feats @ p["critic.fc.weight"].T + p["critic.fc.bias"]
    out = feats @ p["action_distribution.mu_maybe_std.weight"].T + p["action_distribution.mu_maybe_std.bias"]
    mu, raw = (out, p["action_distribution.std"]) if use_std_param else out.chunk(2, 1)
    mu, std = torch.tanh(mu), torch.exp(torch.clamp(raw, GAUSS_OPTS["min_std"], GAUSS_OPTS["max_std"]))
    logp, entropy = O.normal_log_prob(mu, std, actions), O.normal_entropy(mu, std)
    assert logp.dtype == torch.float64 and entropy.dtype == torch.float64
    return value.view(-1), logp.view(-1), entropy.view(-1)


def reference(cfg, params, x, h0, masks, actions, gouts, wrong=None, keys=None):
    """Outputs and gradients of recurrence + heads in float64 on the recurrent input x (B, in).  params: fp32 (or fp64) tensors by name;
    keys: the parameters to differentiate (default: HEAD_PREFIXES).  -> (outputs dict, grads dict), numpy float64."""
    T, n = cfg.T, cfg.n
    keys = [k for k in params if k.startswith(HEAD_PREFIXES)] if keys is None else keys
    p = {k: params[k].detach().double().clone().requires_grad_(True) for k in keys}
    feats, hfin = ref_scan(p, cfg.rnn_type, cfg.layers, x.double().view(T, n, -1), h0.double(), masks.double().view(T, n), wrong)
    if cfg.gauss is None:
        v, lp, ent, _ = ref_heads(p, feats, actions.view(-1, 1))
    else:
        v, lp, ent = ref_gauss_heads(p, feats, actions.double(), cfg.gauss == "std_param")
    gv, glp, gent = (g.double().view(-1) for g in gouts)
    ((v * gv).sum() + (lp * glp).sum() + (ent * gent).sum()).backward()
    out = dict(value=v, log_prob=lp, entropy=ent, final_hidden=hfin)
    return {k: t.detach().numpy() for k, t in out.items()}, {k: t.grad.numpy() for k, t in p.items()}


# ------------------------------------------------------------------------------------------------------------------------------------
# The comparison
# ------------------------------------------------------------------------------------------------------------------------------------
def rel_err(got, ref, floor):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(floor, np.abs(ref).max()))


def compare(got_out, got_grads, ref_out, ref_grads, tol=TOL, record=True):
    """Every output (floor 1e-3) and every reference gradient (floor 1e-4; none skipped) -> (largest error / tol, failures).  A gradient
    whose reference is identically zero must be exactly zero; every other one must have max|ref| >= 10 x floor."""
    ratios, bad = {}, []
    for k, ref in ref_out.items():
        ratios[k] = rel_err(got_out[k], ref, OUT_FLOOR) / tol
    assert set(ref_grads) <= set(got_grads), sorted(set(ref_grads) - set(got_grads))
    for k, ref in ref_grads.items():
        if not np.any(ref):
            if np.any(np.asarray(got_grads[k])):
                bad.append((k, "reference gradient is identically zero", float(np.abs(got_grads[k]).max())))
            continue
        assert np.abs(ref).max() >= 10 * GRAD_FLOOR, ("reference gradient too small for the floor: change the inputs", k, np.abs(ref).max())
        ratios["grad/" + k] = rel_err(got_grads[k], ref, GRAD_FLOOR) / tol
    bad += [(k, r) for k, r in ratios.items() if not r <= 1.0]
    worst = float("nan") if any(r != r for r in ratios.values()) else max(ratios.values(), default=0.0)
    if record:
        tid = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
        MARGINS[tid] = max(MARGINS.get(tid, 0.0), worst) if worst == worst else worst
        for k, r in ratios.items():  # per tensor name over the whole run: which tensor carries a group's figure
            TENSOR_MARGINS[k] = max(TENSOR_MARGINS.get(k, 0.0), r) if r == r else r
    return worst, bad


GROUPS = ("widths", "layers", "row_tiles", "sequences", "act", "heads")  # test_<group>...: the groups of the per-group maxima


@pytest.fixture(scope="module", autouse=True)
def _dump_margins():
    yield
    if not MARGINS:  # (a run without a GPU records nothing)
        return
    groups = {g: max([r for tid, r in MARGINS.items() if tid.split("::")[-1].startswith("test_" + g)], default=None) for g in GROUPS}
    from test_gpu_fullshape import _report  # the suite's parity_<name>.json writer
    _report("margins_rnn", {"what": "largest observed error / tolerance against the float64 reference (1.0 = at the limit)", "groups": groups,
                            "tensors": TENSOR_MARGINS, "tests": MARGINS})


# ------------------------------------------------------------------------------------------------------------------------------------
# Cases: configuration -> parameters and inputs (all on the CPU, deterministic)
# ------------------------------------------------------------------------------------------------------------------------------------
def case(rnn_type, layers, hidden, T, n, p_start, form="packed", A=4, seed=0, hh_scale=1.0, mask_mode=None, gauss=None, arch="simple_cnn"):
    """form: "packed" (blind engine, dense frames) or "tm" (SimpleCNN at 44 x 44, frames gathered through identity rows: the time-major
    form).  mask_mode: None (episode starts with probability p_start), "first_zero" (additionally every env starts an episode at t = 0)."""
    return types.SimpleNamespace(rnn_type=rnn_type, layers=layers, hidden=hidden, T=T, n=n, p_start=p_start, form=form, A=A, seed=seed,
                                 hh_scale=hh_scale, mask_mode=mask_mode, gauss=gauss, arch=arch, HW=44 if form == "tm" else 0,
                                 Lh=layers * (2 if rnn_type == "LSTM" else 1))


def blind_param_shapes(hidden, A, rnn_type, layers, goal_dim=2):
    """state_dict() names / shapes of a blind SimpleCNN policy: no visual encoder, the recurrent input is the goal alone."""
    shapes = [(k, s) for k, s in baseline_param_shapes(4, 44, 44, hidden, num_actions=A, goal_dim=goal_dim, rnn_type=rnn_type, layers=layers)
              if "visual_encoder" not in k]
    return [(k, (s[0], goal_dim) if k.endswith("weight_ih_l0") else s) for k, s in shapes]


def make_params(cfg, shapes=None):
    if shapes is None:
        shapes = (baseline_param_shapes(4, cfg.HW, cfg.HW, cfg.hidden, num_actions=cfg.A, rnn_type=cfg.rnn_type, layers=cfg.layers)
                  if cfg.form == "tm" else blind_param_shapes(cfg.hidden, cfg.A, cfg.rnn_type, cfg.layers))
    params = det_params(shapes, 11 + cfg.seed)
    for k in params:
        if "weight_hh" in k:
            params[k] = params[k] * cfg.hh_scale
    return params


def make_inputs(cfg):
    T, n, B, HW = cfg.T, cfg.n, cfg.T * cfg.n, cfg.HW
    rng = np.random.default_rng(1000 * cfg.seed + 31 * T + n)
    f32 = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    inp = types.SimpleNamespace(rgb=None, depth=None)
    if cfg.form == "tm":
        inp.rgb = torch.from_numpy(rng.integers(0, 256, (B, HW, HW, 3), dtype=np.uint8))
        inp.depth = torch.from_numpy(rng.random((B, HW, HW, 1), dtype=np.float32))
    inp.goal = f32(B, 2)
    masks = rng.random((T, n)) >= cfg.p_start
    if cfg.mask_mode == "first_zero":
        masks[0] = False
    inp.masks = torch.from_numpy(masks.reshape(B, 1))
    if cfg.gauss is None:
        inp.actions = torch.from_numpy(rng.integers(0, cfg.A, (B, 1)))
        inp.prev_actions = None
    else:
        inp.actions, inp.prev_actions = f32(B, cfg.A), f32(B, cfg.A)
    inp.h0 = f32(n, cfg.Lh, cfg.hidden)
    inp.gouts = tuple(f32(B) for _ in range(3))
    return inp


def oracle_spec(cfg):
    return O.NetSpec(kind="baseline", rnn_type=cfg.rnn_type, num_layers=cfg.layers, hidden=cfg.hidden, num_actions=cfg.A)


def oracle_evaluate(cfg, params, inp):
    """The fp32 CPU oracle in the role of the engine: (outputs, gradients by name, its recurrent input)."""
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    obs = {GOAL: inp.goal}
    if inp.rgb is not None:
        obs.update(rgb=inp.rgb, depth=inp.depth)
    taps = {}
    B = cfg.T * cfg.n
    v, lp, ent, hfin = O.evaluate_actions(p, oracle_spec(cfg), obs, inp.h0, torch.zeros(B, 1, dtype=torch.long), inp.masks, inp.actions,
                                          taps=taps)
    gv, glp, gent = (g.view(B, 1) for g in inp.gouts)
    ((v * gv).sum() + (lp * glp).sum() + (ent * gent).sum()).backward()
    out = dict(value=v.view(-1), log_prob=lp.view(-1), entropy=ent.view(-1), final_hidden=hfin)
    return ({k: t.detach().numpy() for k, t in out.items()}, {k: t.grad.numpy() for k, t in p.items()}, taps["rnn_in"].detach())


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the reference against the oracle, and the comparison against wrong references
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [case("GRU", 1, 64, 9, 5, 0.25, form="tm"), case("LSTM", 2, 64, 9, 5, 0.25, form="tm"),
                                 case("GRU", 1, 128, 9, 5, 0.25, form="packed")], ids=["gru1", "lstm2", "blind"])
def test_reference_matches_oracle(cfg):
    """The float64 reference on the oracle's own recurrent input against oracle.functional.evaluate_actions in fp32: outputs and the
    gradients of recurrence + heads (blind: of every parameter) to 1e-5 relative."""
    params, inp = make_params(cfg), make_inputs(cfg)
    o_out, o_grads, x = oracle_evaluate(cfg, params, inp)
    r_out, r_grads = reference(cfg, params, x, inp.h0, inp.masks, inp.actions, inp.gouts)
    if cfg.form == "packed":
        assert set(r_grads) == set(params) and torch.equal(x, inp.goal)
    worst, bad = compare(o_out, o_grads, r_out, r_grads, tol=1e-5, record=False)
    assert not bad, (worst, bad)


@pytest.mark.parametrize("wrong,rnn_type", [("bhn_outside", "GRU"), ("swap_rz", "GRU"), ("mask_output", "GRU"), ("lstm_c_unmasked", "LSTM")])
def test_wrong_reference_variants_are_caught(wrong, rnn_type):
    """The comparison must be able to fail: b_hn moved outside the r * (.) product, the r and z gates swapped, the episode-start mask
    applied to the step's output instead of the incoming state, the LSTM cell state left unmasked -- each in place of the engine, against the
    right reference, on a T = 9, n = 5 case -- must exceed the tolerance by 10x or more."""
    cfg = case(rnn_type, 1, 64, 9, 5, 0.25)
    params, inp = make_params(cfg), make_inputs(cfg)
    assert 0 < int((~inp.masks).sum()) < cfg.T * cfg.n
    r_out, r_grads = reference(cfg, params, inp.goal, inp.h0, inp.masks, inp.actions, inp.gouts)
    w_out, w_grads = reference(cfg, params, inp.goal, inp.h0, inp.masks, inp.actions, inp.gouts, wrong=wrong)
    worst, bad = compare(w_out, w_grads, r_out, r_grads, record=False)
    assert worst >= 10.0 and bad, (wrong, worst)
    out_only, _ = compare(w_out, r_grads, r_out, r_grads, record=False)  # (visible in the forward outputs alone, too)
    assert out_only >= 10.0, (wrong, out_only)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the engine in the role of the oracle above
# ------------------------------------------------------------------------------------------------------------------------------------
def make_engine(cfg):
    from habitat_amd import _lib
    from habitat_amd.engine import PolicyEngine
    tm = cfg.form == "tm"
    kw = dict(arch=cfg.arch, rnn_type=cfg.rnn_type, rnn_layers=cfg.layers, hidden=cfg.hidden, num_actions=cfg.A, H=cfg.HW, W=cfg.HW,
              has_rgb=tm, has_depth=tm, goal_dim=2, max_frames=cfg.T * cfg.n, max_envs=cfg.n)
    if cfg.arch == "resnet":
        kw.update(visual_order=())
    if cfg.gauss is not None:
        flags = _lib.GAUSS_TANH_MU | _lib.GAUSS_USE_LOG_STD | _lib.GAUSS_CLAMP_STD | (_lib.GAUSS_USE_STD_PARAM if cfg.gauss == "std_param" else 0)
        kw.update(action_dist="gaussian", gauss_flags=flags, gauss_min_std=GAUSS_OPTS["min_std"], gauss_max_std=GAUSS_OPTS["max_std"])
    return PolicyEngine(**kw)


def engine_evaluate(cfg, params, inp):
    """evaluate + final_hidden + backward on the GPU -> (outputs, gradients by name, the engine's own recurrent input (B, rnn_in))."""
    from habitat_amd.engine import DevicePackInfo
    T, n, B = cfg.T, cfg.n, cfg.T * cfg.n
    eng = make_engine(cfg)
    if params is None:  # (engines whose parameter table the fixtures do not list: named by the engine itself)
        params = make_params(cfg, [(nm, shp) for nm, shp, _ in eng.specs])
    assert [s[0] for s in eng.specs] == list(params), "engine parameter table differs from the case's"
    eng.load({k: v.cuda() for k, v in params.items()})
    cu = lambda t: None if t is None else t.cuda()
    rgb, depth, goal, masks, actions, prev = cu(inp.rgb), cu(inp.depth), cu(inp.goal), cu(inp.masks), cu(inp.actions), cu(inp.prev_actions)
    pack = DevicePackInfo(np.logical_not(inp.masks.view(T, n).numpy()), "cuda")
    rows = torch.arange(B, dtype=torch.int32, device="cuda") if cfg.form == "tm" else None
    # NaN-filled outputs: a kernel that leaves a frame unwritten cannot pass
    dv, dl, de = (torch.full((B,), float("nan"), device="cuda") for _ in range(3))
    hf = torch.full((n, cfg.Lh, cfg.hidden), float("nan"), device="cuda")
    eng.evaluate(rgb, depth, goal, rows, cu(inp.h0), masks, actions, pack, B, n, value=dv, log_prob=dl, entropy=de, prev_actions=prev)
    eng.final_hidden(hf)
    x = eng.tap(3).view(B, -1).clone()  # HAB_TAP_RNN_IN
    eng.backward(rgb, depth, goal, rows, actions, pack, *(cu(g) for g in inp.gouts), prev_actions=prev)
    torch.cuda.synchronize()
    rnn_in = params["net.state_encoder.rnn.weight_ih_l0"].shape[1]
    assert x.shape[1] >= rnn_in and x.shape[1] % 16 == 0 and not bool(x[:, rnn_in:].any()), "padding columns of the recurrent input"
    out = dict(value=dv, log_prob=dl, entropy=de, final_hidden=hf)
    return ({k: t.cpu().numpy() for k, t in out.items()}, {k: g.cpu().numpy() for k, g in eng.grad_views.items()}, x[:, :rnn_in].cpu(), params)


def run_case(cfg, params="default"):
    """params: None = named and shaped by the engine's own parameter table."""
    params = make_params(cfg) if isinstance(params, str) else params
    inp = make_inputs(cfg)
    g_out, g_grads, x, params = engine_evaluate(cfg, params, inp)
    if cfg.form == "packed" and cfg.arch == "simple_cnn":
        assert torch.equal(x, inp.goal)  # blind: the recurrent input is the goal itself
    r_out, r_grads = reference(cfg, params, x, inp.h0, inp.masks, inp.actions, inp.gouts)
    if cfg.form == "packed" and cfg.arch == "simple_cnn":
        assert set(r_grads) == set(g_grads), "a blind policy has no parameter outside recurrence + heads"
    worst, bad = compare(g_out, g_grads, r_out, r_grads)
    assert not bad, (worst, bad)
    return r_grads, g_grads


def tm_kernel(hidden, n):
    return "persist" if hidden in (128, 256, 512) and (n + 15) // 16 <= 15 else "steps"


def cid(c):
    s = f"{c.form}-{c.rnn_type}{c.layers}x{c.hidden}-T{c.T}-n{c.n}"
    return s + ("-" + tm_kernel(c.hidden, c.n) if c.form == "tm" else "")


WIDTH_CASES = [case(r, l, h, 13, 5, 0.25, form=f) for f in ("packed", "tm") for r in ("GRU", "LSTM") for l in (1, 2) for h in WIDTHS]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", WIDTH_CASES, ids=cid)
def test_widths(cfg):
    """Every width class of launch_step / rnn_seq_layer_backward / the wavefront: 4 waves at hidden 64, 192, 320 (1, 3, 5 K-chunks per
    wave), 8 waves at 128 .. 1024 (1, 2, 3, 4, 5, 8), and both branches of the heads' loads (hidden % 256)."""
    run_case(cfg)


LAYER_CASES = [case(r, l, h, 11, 17, 0.25) for r in ("GRU", "LSTM") for h in (64, 384) for l in (3, 4, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", LAYER_CASES, ids=lambda c: cid(c) + ("-wavefront" if c.layers <= 4 else "-layer_by_layer"))
def test_layers(cfg):
    """3 and 4 layers run as one wavefront (4 = RNN_MAX_WAVE_LAYERS, the size of its argument struct), 5 fall back to layer by layer; two
    row tiles, the second with one row."""
    run_case(cfg)


TILE_N = [1, 15, 16, 17, 37, 64, 240, 256]
TILE_CASES = [case(r, l, 128, 6, n, 0.2, form=f) for f in ("packed", "tm") for r, l in (("LSTM", 2), ("GRU", 1)) for n in TILE_N]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", TILE_CASES, ids=lambda c: cid(c) + f"-{(c.n + 15) // 16}tiles")
def test_row_tiles(cfg):
    """1 .. 16 row tiles of 16 sequences, full and ragged; time-major: 240 = the persistent kernel's last size (15 tiles), 256 = its
    fallback to step launches."""
    run_case(cfg)


@pytest.mark.gpu
def test_row_tiles_step_launches_forced():
    """A persistent case of test_row_tiles (LSTM 2 x 128, n = 37: three tiles, ragged) with matrix-path bit 12 set: the step-per-launch
    time-major form against the reference at several tiles."""
    from habitat_amd import _lib
    L = _lib.lib()
    prev = L.hab_set_matrix_path(-1)
    try:
        L.hab_set_matrix_path(prev | STEP_LAUNCHES)
        run_case(case("LSTM", 2, 128, 6, 37, 0.2, form="tm"))
    finally:
        L.hab_set_matrix_path(prev)


SEQUENCE_CASES = {
    "c2_rollout-tm-GRU1x512-T128-n16-persist": case("GRU", 1, 512, 128, 16, 0.04, form="tm"),
    "c2_rollout-packed-GRU1x512-T128-n16": case("GRU", 1, 512, 128, 16, 0.04),
    "unbroken_chain-tm-LSTM2x512-T128-n4-persist": case("LSTM", 2, 512, 128, 4, 0.0, form="tm"),
    "unbroken_chain-packed-LSTM2x512-T128-n4": case("LSTM", 2, 512, 128, 4, 0.0),
    "fewer_steps_than_chunks-tm-GRU1x128-T2-n5-persist": case("GRU", 1, 128, 2, 5, 0.25, form="tm"),
    "fewer_steps_than_chunks-tm-LSTM2x256-T3-n5-persist": case("LSTM", 2, 256, 3, 5, 0.25, form="tm"),
    "fewer_steps_than_chunks-tm-GRU2x64-T3-n17-steps": case("GRU", 2, 64, 3, 17, 0.25, form="tm"),
    "h0_carried_in-tm-GRU2x128-T5-n5-persist": case("GRU", 2, 128, 5, 5, 0.0, form="tm"),
    "h0_carried_in-packed-LSTM1x192-T5-n5": case("LSTM", 1, 192, 5, 5, 0.0),
    "h0_ignored-tm-LSTM1x128-T5-n5-persist": case("LSTM", 1, 128, 5, 5, 0.1, form="tm", mask_mode="first_zero"),
    "h0_ignored-packed-GRU2x192-T5-n5": case("GRU", 2, 192, 5, 5, 0.1, mask_mode="first_zero"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SEQUENCE_CASES))
def test_sequences(name):
    """Sequence structure: the C2 rollout (T = 128, 16 envs, an episode start every ~25 steps), one unbroken 128-step chain, time-major
    with fewer steps than chunks (chunks = min(4, T)), an all-ones mask with a non-zero stored state (carried in), a mask whose first row is
    all zeros (the stored state must not matter: checked against the reference AND by running the engine again from another h0)."""
    cfg = SEQUENCE_CASES[name]
    inp = make_inputs(cfg)
    if name.startswith("h0_carried_in"):
        assert bool(inp.masks.all()) and float(inp.h0.abs().max()) > 1
    run_case(cfg)
    if name.startswith("h0_ignored"):
        assert not bool(inp.masks.view(cfg.T, cfg.n)[0].any())
        params = make_params(cfg)
        a = engine_evaluate(cfg, params, inp)
        inp.h0 = inp.h0 * -3.0 + 1.0
        b = engine_evaluate(cfg, params, inp)
        assert all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [case("LSTM", 2, 1024, 16, 5, 1.0), case("GRU", 2, 256, 16, 5, 1.0, form="tm"),
                                 case("GRU", 1, 320, 16, 20, 1.0)], ids=cid)
def test_sequences_every_frame_starts_an_episode(cfg):
    """p = 1: the state entering every step is zero, so the reference's weight_hh gradients are identically zero and the engine's must be
    EXACTLY zero (compare() asserts that for every identically-zero reference gradient); everything else to the usual bar."""
    r_grads, g_grads = run_case(cfg)
    hh = [k for k in r_grads if "weight_hh" in k]
    assert len(hh) == cfg.layers
    for k in hh:
        assert not np.any(r_grads[k]) and not np.any(g_grads[k]), k
    assert all(np.any(r_grads[k]) for k in r_grads if "weight_hh" not in k)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [case("GRU", 1, 512, 128, 16, 0.04, form="tm", hh_scale=2.0), case("GRU", 1, 512, 128, 16, 0.04, hh_scale=2.0),
                                 case("LSTM", 3, 128, 64, 37, 0.1, hh_scale=2.0)], ids=cid)
def test_sequences_saturated_gates(cfg):
    """Recurrent weight matrices scaled by 2: gate pre-activations several units wide, sigmoids and tanh near their rails over long
    chains.  (Not by 4: there plain fp32 arithmetic on the CPU is itself 8.7e-4 from float64 and the case cannot tell right from wrong.)"""
    run_case(cfg)


# ---- the rollout step ---------------------------------------------------------------------------------------------------------------
ACT_CASES = [case(r, l, h, 1, n, 0.3) for r, l in (("GRU", 1), ("LSTM", 2)) for h in WIDTHS for n in (1, 17, 64)]


def act_reference(cfg, params, inp):
    """One step: state * mask -> cells -> heads; the deterministic action is the arg-max.  -> value, log-probs (n, A), new state."""
    p = {k: v.double() for k, v in params.items()}
    with torch.no_grad():
        feats, hnew = ref_scan(p, cfg.rnn_type, cfg.layers, inp.goal.double().view(1, cfg.n, -1), inp.h0.double(), inp.masks.double().view(1, cfg.n))
        value, _, _, logp_all = ref_heads(p, feats, torch.zeros(cfg.n, 1, dtype=torch.long))
    return value.numpy(), logp_all.numpy(), hnew.numpy()


def act_decided_rows(logp_all):
    """Rows whose two largest reference probabilities differ by more than 1e-3 (the arg-max of the others may legitimately flip)."""
    pr = np.sort(np.exp(logp_all), axis=1)
    return (pr[:, -1] - pr[:, -2]) > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ACT_CASES, ids=lambda c: f"{c.rnn_type}{c.layers}x{c.hidden}-n{c.n}")
def test_act(cfg):
    """hab_policy_act in deterministic mode on a blind engine (rnn_step_layer_forward with the input projection fused into the step,
    1 / 2 / 4 row tiles): value, log-prob of the chosen action, new hidden state; the chosen action itself on the decided rows."""
    n = cfg.n
    for cfg.seed in range(16):  # the first seed whose inputs the REFERENCE decides on at least 98 % of the rows (nothing of the engine enters)
        params, inp = make_params(cfg), make_inputs(cfg)
        value, logp_all, hnew = act_reference(cfg, params, inp)
        decided = act_decided_rows(logp_all)
        if (~decided).sum() <= 0.02 * n:
            break
    assert (~decided).sum() <= 0.02 * n, "no seed gives the reference 98 % decided rows"
    eng = make_engine(cfg)
    eng.load({k: v.cuda() for k, v in params.items()})
    vals, lps = (torch.full((n, 1), float("nan"), device="cuda") for _ in range(2))
    acts = torch.full((n, 1), -1, dtype=torch.long, device="cuda")
    hout = torch.full((n, cfg.Lh, cfg.hidden), float("nan"), device="cuda")
    eng.act(None, None, inp.goal.cuda(), inp.h0.cuda(), inp.masks.cuda(), n, deterministic=True, values=vals, actions=acts,
            action_log_probs=lps, hidden_out=hout)
    torch.cuda.synchronize()
    a = acts.cpu().numpy().reshape(-1)
    assert ((a >= 0) & (a < cfg.A)).all()
    assert np.array_equal(a[decided], logp_all.argmax(1)[decided]), "deterministic action differs from the reference's arg-max"
    got = dict(value=vals.cpu().numpy().reshape(-1), log_prob=lps.cpu().numpy().reshape(-1), hidden=hout.cpu().numpy())
    ref = dict(value=value, log_prob=logp_all[np.arange(n), a], hidden=hnew)  # log-prob of the action the ENGINE chose
    worst, bad = compare(got, {}, ref, {})
    assert not bad, (worst, bad)


# ---- heads --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [64, 256, 384], ids=lambda h: f"hidden{h}")
@pytest.mark.parametrize("A", [1, 2, 3, 5, 7, 8], ids=lambda a: f"Discrete{a}")
def test_heads(A, hidden):
    """CategoricalNet + critic over Discrete(A) up to MAX_A = 8 (7, 8: the last slots of the padded [B][8] saves), both load branches
    (hidden % 256), B = 21 = 4 * 5 + 1 frames (four frames per workgroup: the last workgroup holds one).  Discrete(1): log-prob and entropy
    are the constant 0, so the actor's reference gradients are identically zero and the engine's must be exactly zero."""
    cfg = case("GRU", 1, hidden, 7, 3, 0.25, A=A)
    r_grads, g_grads = run_case(cfg)
    if A == 1:
        assert not np.any(r_grads["action_distribution.linear.weight"]) and not np.any(g_grads["action_distribution.linear.weight"])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["std_param", "two_A_outputs"])
@pytest.mark.parametrize("A", [1, 2, 3, 4], ids=lambda a: f"Box{a}")
def test_heads_gaussian(A, form):
    """GaussianNet up to GA = 4 action dimensions, with the state-independent std parameter and with 2A linear outputs, evaluate mode, on a
    blind ResNet engine (the only arch with a Gaussian head), B = 21 frames."""
    cfg = case("LSTM", 1, 64, 7, 3, 0.25, A=A, gauss=form, arch="resnet")
    r_grads, _ = run_case(cfg, params=None)
    assert ("action_distribution.std" in r_grads) == (form == "std_param")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
REFUSED = {
    "hidden96-packed": case("GRU", 1, 96, 4, 3, 0.25), "hidden96-tm": case("LSTM", 2, 96, 4, 3, 0.25, form="tm"),
    "discrete9": case("GRU", 1, 64, 4, 3, 0.25, A=9),
    "gaussian5-std_param": case("LSTM", 1, 64, 4, 3, 0.25, A=5, gauss="std_param", arch="resnet"),
    "gaussian5-two_A_outputs": case("LSTM", 1, 64, 4, 3, 0.25, A=5, gauss="two_A_outputs", arch="resnet"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(name):
    """Configurations outside the kernels' limits are refused by hab_policy_create (host-side checks at the top of engine.hip, before any
    workspace exists or any kernel is launched -- which is why this needs no GPU and can never be a way to make one fault): a hidden size
    that is not a multiple of 64 (96: the recurrent kernels' 16-wide K-chunks x 4 waves), Discrete(9) (MAX_A = 8), a 5-dimensional Gaussian
    head (GA = 4).  No engine exists afterwards, so nothing was written anywhere."""
    from habitat_amd._lib import HabError
    with pytest.raises(HabError, match="hab_policy_create"):
        make_engine(REFUSED[name])


@pytest.mark.gpu
def test_refusals_neighbours_inside_the_limits_are_accepted():
    make_engine(case("LSTM", 1, 64, 4, 3, 0.25, A=4, gauss="std_param", arch="resnet"))
    make_engine(case("GRU", 1, 64, 4, 3, 0.25, A=8))
    make_engine(case("GRU", 1, 128, 4, 3, 0.25, form="tm"))
