"""GPU: DAgger on the device.  hab_dagger_mix against tests/dagger_reference.py bit for bit; hab_bc_loss against its float64
definition within the allowance of a running error analysis of the kernel's float32 operations (dagger_reference.bc_loss, in the
manner of tests/test_gpu_learner_math.py); then the trainer from the two new YAMLs replayed through the numpy envs and their
restated teachers, the executed oracle (beta = 1) finishing episodes, the PPO path without the block, and the learning run.

Every kernel case: outputs pre-filled with NaN (a sentinel for integers) inside guard elements which must come back untouched, and the
loss is run twice on fresh copies and must reproduce its bits.

Worst error / allowance of hab_bc_loss seen on the MI355X (printed at the end of a run with -s):
  d_value 0.321, d_logp 0.042, d_entropy 0.305, out[0..3] 0.032, out[5] 0.012, out[7..9] 0.188, out[10] 0.030; value_pred min and
  max and B exact.  No case came above 0.5."""
import ctypes as C
import importlib.util
import math
import os
import time

import numpy as np
import pytest
import torch

import dagger_reference as D
import nav2d_follow_reference as FR
import nav2d_geo_reference as G
import nav2d_rearr_oracle_reference as OR
from test_gpu_nav2d import make_trainer

pytestmark = pytest.mark.gpu
F = np.float32
GUARD, ISENT, NAN = 4, -77, float("nan")
ERR_ARG = -1
WORST = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from habitat_amd import _lib
    yield _lib.lib()
    for k in sorted(WORST):
        print("worst error/allowance hab_bc_loss %-12s %.3f" % (k, WORST[k]))


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class Guarded:
    """A device array with GUARD elements of `fill` on each side of its body."""

    def __init__(self, body, fill):
        body = np.ascontiguousarray(body)
        self.n = body.size
        host = np.full(self.n + 2 * GUARD, fill, body.dtype)
        host[GUARD:GUARD + self.n] = body.reshape(-1)
        self.fill, self.t = fill, dev(host)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + GUARD * self.t.element_size())

    def read(self):
        """The body; asserts that the guards still hold their fill."""
        host = self.t.cpu().numpy()
        g = np.concatenate([host[:GUARD], host[GUARD + self.n:]])
        assert np.array_equal(g, np.full_like(g, self.fill), equal_nan=True), "a guard element was written"
        return host[GUARD:GUARD + self.n]


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ================================================================================================
# hab_dagger_mix
# ================================================================================================
def mix_case(N, beta, seed, steps=3):
    """`steps` successive steps of N envs: every status code, episode starts, labels that repeat and change, u == beta planted."""
    r = np.random.default_rng([N, int(beta * 8), seed])
    out = []
    for t in range(steps):
        expert = r.integers(0, 3, N).astype(np.int64) if t else np.full(N, 1, np.int64)   # repeats are common: both weights occur
        status = ((np.arange(N) + t) % 6).astype(np.int32)
        not_done = (r.random(N) > 0.3).astype(np.uint8)
        u = r.random(N, dtype=F)
        u[::3] = F(beta)                              # the strict comparison decides these
        u[1::7] = np.nextafter(F(beta), F(0)) if beta > 0 else F(0)
        out.append(dict(actions=r.integers(0, 6, N).astype(np.int64), expert=expert, status=status, not_done=not_done, u=u,
                        mask=(r.random(N) > 0.25).astype(np.uint8)))
    return out


@pytest.mark.parametrize("use_mask", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("N", [1, 64, 70])
@pytest.mark.parametrize("coef", [3.2, 0.0], ids=["coef3.2", "coef0"])   # at 0 an inflection weighs nothing and is not counted
def test_dagger_mix_bitwise(L, N, beta, use_mask, coef):
    prev_ref, agree_ref = np.full(N, -1, np.int64), np.array([5, 9], np.int64)       # the counters accumulate onto what they held
    prev, agree = Guarded(prev_ref, ISENT), Guarded(agree_ref, ISENT)
    for t, s in enumerate(mix_case(N, beta, 3)):
        mask = s["mask"] if use_mask else None
        a_ref, w_ref = s["actions"].copy(), np.full(N, NAN, F)
        D.dagger_mix(a_ref, s["expert"], s["status"], s["not_done"], s["u"], beta, coef, prev_ref, w_ref, agree_ref, mask)
        acts, w = Guarded(s["actions"], ISENT), Guarded(np.full(N, NAN, F), NAN)
        keep = [dev(s[k]) for k in ("expert", "status", "not_done", "u")] + [dev(mask) if use_mask else None]
        assert L.hab_dagger_mix(acts.ptr, P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), P(keep[4]), beta, coef, prev.ptr, w.ptr,
                                agree.ptr, N, S()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(acts.read(), a_ref), f"actions, step {t}"
        assert np.array_equal(w.read().view(np.int32), w_ref.view(np.int32)), f"weights, step {t}"      # NaN where masked out
        assert np.array_equal(prev.read(), prev_ref), f"prev_expert, step {t}"
        assert np.array_equal(agree.read(), agree_ref), f"agree, step {t}"
    assert agree_ref[1] > 9 or N == 1 or coef == 0


def test_dagger_mix_refusals(L):
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = P(t)
    good = [p, p, p, p, p, None, 0.5, 1.0, p, p, p, 4, S()]
    for i in (0, 1, 2, 3, 4, 8, 9, 10):
        bad = list(good)
        bad[i] = None
        assert L.hab_dagger_mix(*bad) == ERR_ARG, i
    for i, v in ((11, 0), (11, -1), (6, -0.5), (6, 1.5), (6, NAN), (6, math.inf), (7, -0.5), (7, NAN), (7, math.inf)):
        bad = list(good)
        bad[i] = v
        assert L.hab_dagger_mix(*bad) == ERR_ARG, (i, v)
    torch.cuda.synchronize()
    assert int(t.abs().sum()) == 0                    # a refused call wrote nothing


# ================================================================================================
# hab_bc_loss
# ================================================================================================
VC, EC, CW = 0.5, 0.01, 3.2


def loss_case(B, kind, seed=0):
    r = np.random.default_rng([B, seed, sum(map(ord, kind))])
    logits = r.normal(size=(B, 6)) * 2.0
    logp = (logits - np.log(np.exp(logits).sum(1, keepdims=True)))[np.arange(B), r.integers(0, 6, B)]
    w = {"mixed": r.choice([0.0, 1.0, CW], B), "zero": np.zeros(B), "single": np.eye(1, B, B // 2)[0] * CW}[kind]
    return dict(values=r.normal(size=B).astype(F), logp=logp.astype(F), entropy=r.uniform(0.2, 1.7, B).astype(F), weights=w.astype(F),
                returns=(r.normal(size=B) * 2).astype(F))


def run_loss(L, d, rows):
    """One call on fresh device copies; rows: None (dense) or the gather the storage buffers are read through."""
    B = len(d["values"])
    if rows is None:
        w_st, r_st = d["weights"], d["returns"]
    else:                                     # storage rows that no frame names hold NaN: reading one would poison the sums
        M = int(rows.max()) + 3
        w_st, r_st = np.full(M, NAN, F), np.full(M, NAN, F)
        w_st[rows], r_st[rows] = d["weights"], d["returns"]
    ins = [dev(d["values"]), dev(d["logp"]), dev(d["entropy"]), dev(w_st), dev(r_st), dev(rows) if rows is not None else None]
    outs = {k: Guarded(np.full(n, NAN, F), NAN) for k, n in (("d_value", B), ("d_logp", B), ("d_entropy", B), ("out", 12))}
    assert L.hab_bc_loss(P(ins[0]), P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), P(ins[5]), B, VC, EC, outs["d_value"].ptr,
                         outs["d_logp"].ptr, outs["d_entropy"].ptr, outs["out"].ptr, S()) == 0
    torch.cuda.synchronize()
    return {k: v.read() for k, v in outs.items()}


def ratio(got, ref):
    v, e = ref
    got = np.asarray(got, np.float64)
    fin = np.isfinite(v)
    if not np.array_equal(got[~fin], v[~fin]) or not np.isfinite(got[fin]).all():
        return np.full(v.shape, math.inf)
    out = np.zeros(v.shape)
    err = np.abs(got[fin] - v[fin])
    out[fin] = np.where(e[fin] > 0, err / np.where(e[fin] > 0, e[fin], 1.0), np.where(err == 0, 0.0, math.inf))
    return out


OUT_GROUPS = {"out[0..3]": [0, 1, 2, 3], "out[5]": [5], "out[7..9]": [7, 8, 9], "out[10]": [10], "out[4,6,11]": [4, 6, 11]}


@pytest.mark.parametrize("kind", ["mixed", "zero", "single"])
@pytest.mark.parametrize("layout", ["dense", "rows"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 4097])
def test_bc_loss(L, B, layout, kind):
    d = loss_case(B, kind)
    rows = None if layout == "dense" else np.random.default_rng(B).permutation(B + 37)[:B].astype(np.int32)
    a, b = run_loss(L, d, rows), run_loss(L, d, rows)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{k}: two runs on fresh copies differ"
    ref = D.bc_loss(**d, value_loss_coef=VC, entropy_coef=EC)
    for k in ("d_value", "d_logp", "d_entropy"):
        q = float(ratio(a[k], ref[k]).max())
        WORST[k] = max(WORST.get(k, 0.0), q)
        print(f"hab_bc_loss B {B} {layout} {kind}: {k} at {q:.3f} of the allowance")
        assert q <= 1.0, f"{k}: error is {q:.3g} x the allowance"
    q = ratio(a["out"], ref["out"])
    for name, idx in OUT_GROUPS.items():
        WORST[name] = max(WORST.get(name, 0.0), float(q[idx].max()))
    print(f"hab_bc_loss B {B} {layout} {kind}: out at", np.round(q, 3).tolist())
    assert (q[[4, 6, 11]] == 0).all(), "minima, maxima and B are exact"
    assert (q <= 1.0).all(), f"out: error / allowance {q}"
    if kind == "zero":
        assert a["out"][1] == 0 and a["out"][10] == 0 and (a["d_logp"] == 0).all() and not np.signbit(a["out"][1])
        assert a["out"][7] == math.inf and a["out"][8] == 0 and a["out"][9] == -math.inf and np.isfinite(a["out"][3])
    W = float(d["weights"].astype(np.float64).sum())
    if W > 0 and max(W, 1.0) != B:            # the wrong variant, the BC term normalised by B: outside the allowance
        wrong = D.bc_loss(**d, value_loss_coef=VC, entropy_coef=EC, normalise_by_B=True)
        on = d["weights"] > 0
        assert float(ratio(a["out"], wrong["out"])[1]) > 1.0 and (ratio(a["d_logp"], wrong["d_logp"])[on] > 1.0).all()


def test_bc_loss_refusals(L):
    t = torch.zeros(64, device="cuda")
    p = P(t)
    good = [p, p, p, p, p, None, 4, VC, EC, p, p, p, p, S()]
    for i in (0, 1, 2, 3, 4, 9, 10, 11, 12):
        bad = list(good)
        bad[i] = None
        assert L.hab_bc_loss(*bad) == ERR_ARG, i
    for B in (0, -5):
        bad = list(good)
        bad[6] = B
        assert L.hab_bc_loss(*bad) == ERR_ARG
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0


# ================================================================================================
# the trainer
# ================================================================================================
SIZE = 64


def dagger_config(yaml, tmp_path, N, T, beta=(0.5, 0.5), extra=()):
    from habitat_amd.config.default import get_config
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=1000",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          "habitat_baselines.rl.ppo.hidden_size=128", f"habitat_baselines.checkpoint_folder={tmp_path}", "habitat_baselines.log_interval=1000",
          f"habitat_baselines.tensorboard_dir={tmp_path}/tb", "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000",
          "habitat_baselines.trainer_name=ppo", f"habitat_baselines.rl.imitation.beta_start={beta[0]}",
          f"habitat_baselines.rl.imitation.beta_end={beta[1]}", "habitat_baselines.rl.imitation.inflection_weight_coef=3.2"]
    return get_config(yaml, ov + list(extra))


def snapshot(trainer):
    """The finished rollout right before the update (after_update copies row T over row 0), with the uniforms and beta of its mix."""
    snap, orig = {}, trainer._update_agent

    def update():
        B = trainer._agent.rollouts.buffers
        snap.update({k: B[k].clone() for k in ("actions", "prev_actions", "expert_actions", "expert_weights", "rewards", "masks")})
        snap.update(u=trainer._imitation["u"].clone(), beta=trainer._imitation["beta"])
        return orig()

    trainer._update_agent = update
    return snap


def replay(trainer, cfg, renvs, teacher, cycles, N, T):
    """`cycles` update cycles; the stored actions replayed through the restated envs `renvs`, whose teacher `teacher(env)` answers
    (action, status).  Returns the executed actions and the weights."""
    snap, coef = snapshot(trainer), F(cfg.habitat_baselines.rl.imitation.inflection_weight_coef)
    prev, nd, took, all_w = np.full(N, -1, np.int64), np.zeros(N, np.uint8), 0, []
    for cycle in range(cycles):
        losses = trainer.run_update_cycle()
        assert all(np.isfinite(v) for k, v in losses.items() if k != "expert_prob_min"), losses
        assert losses["imitation_beta"] == snap["beta"] == 0.5 and 0.0 <= losses["imitation_agreement"] <= 1.0
        assert {"value_loss", "action_loss", "dist_entropy", "expert_prob_min", "expert_prob_mean", "expert_prob_max", "imitation_weight_sum",
                "grad_norm"} <= set(losses) and "prob_ratio_mean" not in losses
        g = lambda k, rows: snap[k][:rows].cpu().numpy().reshape(rows, N)
        actions, expert, weights, rewards = g("actions", T), g("expert_actions", T), g("expert_weights", T), g("rewards", T)
        prev_actions, masks, u = g("prev_actions", T + 1), g("masks", T + 1), snap["u"].cpu().numpy()
        assert u.shape == (T, N) and u.dtype == F and (u >= 0).all() and (u < 1).all()
        assert np.array_equal(masks[0].astype(np.uint8), nd), "row 0 carries the last step's mask"
        low = high = counted = 0
        for t in range(T):
            for n, e in enumerate(renvs):
                a, status = teacher(e)
                assert expert[t, n] == a, f"cycle {cycle} step {t} env {n}: the label is not the restated teacher's"
                gave_up = status in (D.UNREACHABLE, D.STUCK)
                w = F(0) if gave_up else (coef if (nd[n] == 0 or prev[n] != a) else F(1))
                assert weights[t, n].view(np.int32) == w.view(np.int32), f"cycle {cycle} step {t} env {n}: weight"
                if u[t, n] < F(0.5):
                    assert actions[t, n] == a, f"cycle {cycle} step {t} env {n}: u < beta and the teacher's action was not executed"
                    took += 1
                    high += int(w > 0)
                else:                                  # the executed action is the policy's own sample: its agreement is known
                    low += int(w > 0 and actions[t, n] == a)
                    high += int(w > 0 and actions[t, n] == a)
                counted += int(w > 0)
                prev[n] = a
                assert prev_actions[t + 1, n] == actions[t, n]
                _, r, done, _ = e.step(int(actions[t, n]))
                assert rewards[t, n] == r, f"cycle {cycle} step {t} env {n}: reward"
                assert bool(masks[t + 1, n]) == (not done), f"cycle {cycle} step {t} env {n}: mask"
                nd[n] = 0 if done else 1
        agreed, total = trainer._imitation["counts"]
        assert total == counted and low <= agreed <= high, (agreed, total, low, high, counted)
        all_w.append(weights)
        assert np.array_equal(trainer._imitation["prev_expert"].cpu().numpy(), prev)
    assert 0.3 * cycles * T * N < took < 0.7 * cycles * T * N
    return np.concatenate(all_w)


def test_trainer_replay_rearrangement(tmp_path):
    """Two update cycles from dagger_nav2d_rearrange_geodesic.yaml (ResNet18 at 64 x 64, hidden 128, 8 envs x 16 steps, K = 3, 10
    degrees, beta 0.5 throughout, inflection weight 3.2).  The stored `actions` replayed through the numpy env from the same seed: at
    every step `expert_actions` is the oracle restatement's answer, `expert_weights` and the executed action follow the mix rule for
    the u drawn (carry across the rollout boundary included), prev_actions[t + 1] == actions[t], rewards and masks are the
    restatement's, and the agreement counters lie in the only range the stored data allow."""
    N, T = 8, 16
    cfg = dagger_config("rearrange/dagger_nav2d_rearrange_geodesic.yaml", tmp_path, N, T,
                        extra=[f"habitat.simulator.sensors.head_depth.height={SIZE}", f"habitat.simulator.sensors.head_depth.width={SIZE}"])
    trainer = make_trainer(cfg)
    ac = trainer._agent.actor_critic
    assert type(ac).__name__ == "PointNavResNetPolicy" and type(trainer._agent.updater).__name__ == "DAgger"
    assert type(trainer._agent.rollouts).__name__ == "ImitationRolloutStorage" and trainer._device_envs
    syn = cfg.habitat.synthetic
    assert (syn.num_obstacles, syn.turn_angle, syn.start_holding) == (3, 10, False)
    renvs = OR.restated_envs(cfg.habitat.seed, N, 3, 10, False, max_steps=cfg.habitat.environment.max_episode_steps)
    for e in renvs:
        e.reset()

    def teacher(e):
        d = OR.oracle(e)
        return OR.action_of(d), d[0]

    w = replay(trainer, cfg, renvs, teacher, 2, N, T)
    assert (w == F(3.2)).any() and (w == 1).any()
    trainer.envs.close()


def test_trainer_replay_nav2d(tmp_path):
    """The same from dagger_nav2d_geodesic.yaml with the blind PointNavBaselinePolicy (no image sensor, K = 8, 10 degrees): the
    teacher is the shortest-path follower's restatement."""
    N, T = 8, 16
    cfg = dagger_config("pointnav/dagger_nav2d_geodesic.yaml", tmp_path, N, T,
                        extra=["habitat_baselines.vector_env_factory.use_rgb=False", "habitat_baselines.vector_env_factory.use_depth=False"])
    trainer = make_trainer(cfg)
    assert type(trainer._agent.actor_critic).__name__ == "PointNavBaselinePolicy" and len(trainer.envs.observation_spaces[0].spaces) == 1
    hab = cfg.habitat
    renvs = [G.Nav2DGeoEnv(hab.seed, n, num_obstacles=hab.synthetic.num_obstacles, turn_angle=hab.synthetic.turn_angle,
                           max_episode_steps=hab.environment.max_episode_steps, use_rgb=False, use_depth=False) for n in range(N)]
    for e in renvs:
        e.reset()

    def teacher(e):
        d = FR.follow(e)
        return FR.discrete_action(d[0], d[1]), d[0]

    replay(trainer, cfg, renvs, teacher, 2, N, T)
    trainer.envs.close()


def test_the_executed_oracle_finishes_episodes(tmp_path):
    """beta = 1, one rollout of 200 steps, K = 3, 8 envs from the rearrangement YAML: every executed action is the label, and the
    window's success and did_pick_object are > 0 (the rate is printed; the oracle's own row is 0.9955 at K = 3 and 10 degrees).  No
    rearrangement run of the trainer recorded a success before this (tests/test_gpu_nav2d_rearr.py: "Success stayed 0.0"), and
    without the feature nothing reads the configuration's keys."""
    N, T = 8, 200
    cfg = dagger_config("rearrange/dagger_nav2d_rearrange_geodesic.yaml", tmp_path, N, T, beta=(1.0, 1.0),
                        extra=[f"habitat.simulator.sensors.head_depth.height={SIZE}", f"habitat.simulator.sensors.head_depth.width={SIZE}",
                               "habitat_baselines.rl.ppo.num_mini_batch=4"])
    trainer = make_trainer(cfg)
    snap = snapshot(trainer)
    losses = trainer.run_update_cycle()
    assert torch.equal(snap["actions"][:T], snap["expert_actions"][:T]) and losses["imitation_beta"] == 1.0
    stats = {k: float(v[-1].sum()) for k, v in trainer.window_episode_stats.items()}
    print("dagger beta = 1 window:", {k: round(v, 3) for k, v in stats.items()}, {k: round(v, 4) for k, v in losses.items()})
    assert stats["count"] > 0 and stats["success"] > 0 and stats["did_pick_object"] > 0
    trainer.envs.close()


def test_without_the_block_the_ppo_path_is_what_it_was(tmp_path):
    """No imitation: from ddppo_nav2d_rearrange_geodesic.yaml the trainer has no imitation state, the storage no expert rows, and two
    runs of two updates from one seed store the same actions, report the same losses and leave the CPU generator in the same state.
    The run's figures on the commit before the feature are held below exactly: the stored actions and all eleven losses of both
    updates, as hex floats (see DESIGN N18).  A change that moves them on purpose dumps them again."""
    from habitat_amd.config.default import get_config

    def run(folder):
        ov = ["habitat_baselines.num_environments=8", "habitat_baselines.rl.ppo.num_steps=16", "habitat_baselines.num_updates=1000",
              "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
              "habitat_baselines.rl.ppo.hidden_size=128", f"habitat_baselines.checkpoint_folder={folder}", "habitat_baselines.log_interval=1000",
              f"habitat_baselines.tensorboard_dir={folder}/tb", "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000",
              "habitat_baselines.trainer_name=ppo", f"habitat.simulator.sensors.head_depth.height={SIZE}",
              f"habitat.simulator.sensors.head_depth.width={SIZE}"]
        trainer = make_trainer(get_config("rearrange/ddppo_nav2d_rearrange_geodesic.yaml", ov))
        assert trainer._imitation is None and "expert_actions" not in trainer._agent.rollouts.buffers
        assert type(trainer._agent.updater).__name__ == "PPO"
        acts, losses, orig = [], [], trainer._update_agent

        def update():
            acts.append(trainer._agent.rollouts.buffers["actions"][:16].clone())
            return orig()

        trainer._update_agent = update
        for _ in range(2):
            losses.append(trainer.run_update_cycle())
        state = torch.random.get_rng_state()
        trainer.envs.close()
        return torch.stack(acts).cpu(), losses, state

    a, la, sa = run(tmp_path / "a")
    b, lb, sb = run(tmp_path / "b")
    print("ppo path, two updates: action checksum", int((a.flatten().double() * torch.arange(1, a.numel() + 1).double()).sum()),
          {k: float(np.float32(v)) for k, v in la[1].items()})
    assert torch.equal(a, b) and la == lb and torch.equal(sa, sb)
    assert "imitation_beta" not in la[0] and "prob_ratio_mean" in la[0]
    # what the commit before the feature stored and reported for this run on one MI355X (dumped from both trees in one session: the
    # 256 actions, all eleven losses of both updates and the CPU generator's state afterwards were equal bit for bit)
    assert a.flatten()[:24].tolist() == [3, 0, 1, 2, 0, 0, 1, 5, 2, 3, 0, 1, 5, 3, 2, 1, 2, 4, 4, 3, 4, 3, 3, 2]
    assert int((a.flatten().double() * torch.arange(1, a.numel() + 1).double()).sum()) == PARENT_ACTION_CHECKSUM
    for i, parent in enumerate(PARENT_LOSSES):
        assert set(la[i]) == set(parent), f"update {i}: the metric keys differ from the parent's"
        for k, v in parent.items():
            assert la[i][k] == float.fromhex(v), f"update {i}: {k} is {float(la[i][k]).hex()}, the parent reported {v}"


PARENT_ACTION_CHECKSUM = 79142
PARENT_LOSSES = (
    {"action_loss": "0x1.533b86p-6", "dist_entropy": "0x1.cab0a0p+0", "grad_norm": "0x1.06c5fcp-4", "ppo_fraction_clipped": "0x0.0p+0",
     "prob_ratio_max": "0x1.00a84ap+0", "prob_ratio_mean": "0x1.000f1ap+0", "prob_ratio_min": "0x1.fe97d6p-1", "value_loss": "0x1.07e208p-6",
     "value_pred_max": "0x1.0f762ap-5", "value_pred_mean": "-0x1.689484p-5", "value_pred_min": "-0x1.107094p-3"},
    {"action_loss": "0x1.5db26ep-5", "dist_entropy": "0x1.caafe2p+0", "grad_norm": "0x1.a474a0p-5", "ppo_fraction_clipped": "0x0.0p+0",
     "prob_ratio_max": "0x1.00ce54p+0", "prob_ratio_mean": "0x1.fffcb2p-1", "prob_ratio_min": "0x1.fe765cp-1", "value_loss": "0x1.28e994p-6",
     "value_pred_max": "0x1.0aa5bap-5", "value_pred_mean": "-0x1.7ad6fep-5", "value_pred_min": "-0x1.1f4af4p-3"})


LEARN_UPDATES = 60
SUCCESS_PPO_PARENT = 0.0


def test_the_policy_learns_to_agree_with_the_oracle(tmp_path):
    """tools/nav2d_rearr_dagger_learning.py, seed 100: the sizes of the geodesic leg of tools/nav2d_rearr_geo_learning.py (32 envs x
    32 steps at 64 x 64, ResNet18, hidden 128, start_holding, turn_angle 30, K = 3, episodes of 48, lr 5e-4, 4 epochs x 2 minibatches),
    beta 1 -> 0 over the first half of LEARN_UPDATES updates.  The family's criterion on `imitation_agreement`: the agree / total counts
    of the last 5 updates against the first 5, two-proportion z >= 5 with the agreement higher, and a lower action_loss.  Then a
    pure-policy window (beta = 0, no update, 4 rollouts): its success must be above the PPO run's of the same sizes, seed and update
    count on the commit before the feature, success_dagger > success_ppo_parent = 0.0 (tools/nav2d_rearr_learning.py, geodesic, K = 3:
    success of the last five updates 0.0 at seeds 100, 101 and 102, after 60 updates and after 100).
    Measured on one MI355X in one session: tests/test_gpu_nav2d.py::test_the_loop_learns 2.66 s, so the budget was 10.6 s; this test
    2.87 s.  Agreement 0.248 -> 0.490 (1267 / 5118 -> 2506 / 5120), z = 25.4, action_loss 1.48 -> 0.88; the window's success 0.087
    of 104 episodes (0.110 of 209 with 8 rollouts; 0.028 and 0.076 at seeds 101 and 102; after 100 updates 0.451, 0.216, 0.171; the
    oracle itself 0.945, 0.934, 0.926 in the same window)."""
    spec = importlib.util.spec_from_file_location("nav2d_rearr_dagger_learning", os.path.join(ROOT, "tools", "nav2d_rearr_dagger_learning.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    t0 = time.time()
    r = tool.learning_run(str(tmp_path), seed=100, updates=LEARN_UPDATES, window=4)
    print(f"nav2drearr dagger learning ({time.time() - t0:.1f} s):", {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
    assert r["z"] >= 5.0 and r["agreement_last"] > r["agreement_first"] and r["action_loss_last"] < r["action_loss_first"], r
    assert r["window_episodes"] > 0 and r["window_success"] > SUCCESS_PPO_PARENT, r
