"""GPU, world_size 2 on ONE device (gloo transport, 127.0.0.1): the DD-PPO updater with the REAL policy engine -- the method of the
reference's test/test_ddppo_reduce.py:28-132 (spawned ranks, real model, gradients equal across ranks) extended to what this
implementation adds on top of DistributedDataParallel:

  * the all-reduced gradient arena equals the sum of the ranks' local gradients (bitwise) and is identical on every rank;
  * parameters after full update cycles are bit-identical across ranks;
  * the early exchange of the arena tail through the engine's grad-ready callback (overlap with the conv stack's backward) gives
    bit-identical parameters to the single blocking all-reduce (HAB_NO_GRAD_OVERLAP=1);
  * one optimiser step equals clip + Adam (CPU oracle) applied to the AVERAGED gradient by a single process;
  * RunningMeanAndVar under DD-PPO (engine all-reduce callback): statistics after a training-mode forward equal the oracle's merge
    of the rank-averaged moments with the rank-summed frame count (rl/ddppo/policy/running_mean_and_var.py:38-71), also when the
    ranks hold DIFFERENT numbers of frames (preempted rollout), and stay identical across ranks.
The RCCL transport itself needs one GPU per rank and is exercised by the driver's multi-GPU bench; everything above the transport
(callbacks, ordering against the engine's stream, arena ranges, scaling) is what runs here."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def find_free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _cfg(workload, N, T):
    from habitat_amd.config.default import get_config
    if workload == "c2":
        path, size, extra = "pointnav/ppo_pointnav_habitat_iccv19.yaml", 64, ["habitat_baselines.trainer_name=ddppo"]
    else:
        path, size, extra = "pointnav/ddppo_pointnav.yaml", 128, ["habitat_baselines.rl.ddppo.backbone=resnet18"]
    ov = [f"habitat_baselines.num_environments={N}", f"habitat_baselines.rl.ppo.num_steps={T}", "habitat_baselines.num_updates=8",
          "habitat_baselines.total_num_steps=-1", "habitat_baselines.num_checkpoints=-1", "habitat_baselines.checkpoint_interval=1000000",
          "habitat_baselines.rl.ppo.hidden_size=64", "habitat_baselines.rl.ppo.num_mini_batch=2", "habitat_baselines.rl.ppo.ppo_epoch=2",
          "habitat_baselines.checkpoint_folder=/tmp/habitat_amd_test_dist_ckpt", "habitat_baselines.rl.ddppo.distrib_backend=GLOO",
          "habitat_baselines.rl.preemption.save_resume_state_interval=1000000000", "habitat_baselines.rl.ddppo.force_distributed=True"]
    for s in ("rgb", "depth"):
        ov += [f"habitat.simulator.sensors.{s}.height={size}", f"habitat.simulator.sensors.{s}.width={size}"]
    cfg = get_config(path, ov + extra)
    cfg.habitat.simulator.sensors.pop("semantic", None)
    return cfg


def _worker(rank, world, port, q, workload, overlap, short_rank1):
    for p in (ROOT, os.path.join(ROOT, "habitat-lab_amd")):
        sys.path.insert(0, p)
    os.environ.update(LOCAL_RANK=str(rank), RANK=str(rank), WORLD_SIZE=str(world), MAIN_ADDR="127.0.0.1", MAIN_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    os.environ.pop("MASTER_PORT", None)
    if not overlap:
        os.environ["HAB_NO_GRAD_OVERLAP"] = "1"
    else:
        os.environ.pop("HAB_NO_GRAD_OVERLAP", None)
    import torch.distributed as dist
    import habitat_amd.rl.ppo.ppo_trainer as tr
    from oracle import functional as O
    N, T = 4, 8
    cfg = _cfg(workload, N, T)
    trainer = tr.PPOTrainer(cfg)
    trainer._init_train()
    assert dist.get_world_size() == world and trainer._is_distributed
    agent = trainer._agent
    pol, upd, st = agent.actor_critic, agent.updater, agent.rollouts
    eng = pol.engine
    out = {"p_init": eng.params_flat.cpu().clone()}
    ppo_cfg = cfg.habitat_baselines.rl.ppo

    # ---- RunningMeanAndVar at world 2 against the oracle's pooled statistics (ResNet policy only) ----------------------------
    if workload == "c3":
        agent.eval()
        trainer.collect_rollout()
        T_eff = T // 2 if (short_rank1 and rank == 1) else T  # a preempted rank holds fewer frames (ppo_trainer.py:641-653)
        st.current_rollout_step_idxs = [T_eff]
        last = st.get_last_step()
        nv = pol.get_value({k: v.contiguous() for k, v in last["observations"].items()}, last["recurrent_hidden_states"],
                           last["prev_actions"], last["masks"])
        st.compute_returns(nv, True, 0.99, 0.95)
        agent.train()
        adv = upd.get_advantages(st)
        batch = next(st.data_generator(adv, ppo_cfg.num_mini_batch))
        Bn, Bf = batch.T * batch.n, st.buffers
        obs = Bf["observations"]
        pre = "net.visual_encoder.running_mean_and_var."
        sd0 = {k: v.cpu().clone() for k, v in pol.state_dict().items() if pre in k}
        eng.evaluate(obs.get("rgb"), obs.get("depth"), obs.get("pointgoal_with_gps_compass"), batch.rows, Bf["recurrent_hidden_states"],
                     Bf["masks"], Bf["actions"], batch.pack, Bn, batch.n, prev_actions=Bf["prev_actions"])
        torch.cuda.synchronize()
        got = {k: v.cpu().clone() for k, v in pol.state_dict().items() if pre in k}
        # oracle: local moments, then the reference's collective protocol on CPU tensors over the same process group
        cols = batch.inds
        x = O.resnet_input({k: obs[k][0:batch.T].index_select(1, cols.cuda()).flatten(0, 1).cpu() for k in ("rgb", "depth")}, ["rgb", "depth"])
        xc = x.transpose(1, 0).contiguous().view(x.size(1), -1)
        new_mean = xc.mean(-1, keepdim=True)
        new_count = torch.full((), float(x.size(0)))
        dist.all_reduce(new_mean)
        dist.all_reduce(new_count)
        new_mean /= world
        new_var = (xc - new_mean).pow(2).mean(dim=-1, keepdim=True)
        dist.all_reduce(new_var)
        new_var /= world
        var, mean, count = O.rmv_merge(sd0[pre + "_mean"], sd0[pre + "_var"], sd0[pre + "_count"], new_mean.view(1, -1, 1, 1),
                                       new_var.view(1, -1, 1, 1), new_count)
        out["rmv_err"] = max(float((got[pre + "_mean"] - mean).abs().max()), float((got[pre + "_var"] - var).abs().max()),
                             float((got[pre + "_count"] - count).abs().max()))
        out["rmv_count"] = float(got[pre + "_count"])
        out["rmv_frames"] = Bn
        out["rmv_state"] = torch.cat([got[pre + "_mean"].view(-1), got[pre + "_var"].view(-1), got[pre + "_count"].view(-1)])
        st.current_rollout_step_idxs = [T]
        st.after_update()

    # ---- first minibatch step instrumented: local gradient, reduced gradient, parameters / Adam state around the step ----------
    rec = {}
    orig_reduce, orig_step = upd._all_reduce_grads, upd.optimizer.step

    def reduce_hook():
        if "g_local" not in rec and not overlap:
            rec["g_local"] = eng.grads_flat.cpu().clone()
        orig_reduce()
        if "g_reduced" not in rec:
            torch.cuda.synchronize()
            rec["g_reduced"] = eng.grads_flat.cpu().clone()
            rec["p_before"] = eng.params_flat.cpu().clone()

    def step_hook(*a, **k):
        r = orig_step(*a, **k)
        if "p_after" not in rec:
            torch.cuda.synchronize()
            rec["p_after"] = eng.params_flat.cpu().clone()
            rec["step_kwargs"] = {kk: vv for kk, vv in k.items() if kk in ("max_grad_norm", "grad_scale")}
            rec["lr"] = upd.optimizer.param_groups[0]["lr"]
        return r

    upd._all_reduce_grads, upd.optimizer.step = reduce_hook, step_hook
    for _ in range(2):
        losses = trainer.run_update_cycle()
        assert all(np.isfinite(v) for v in losses.values()), losses
    torch.cuda.synchronize()
    out.update(rec)
    out["p_final"] = eng.params_flat.cpu().clone()
    out["steps_done"] = trainer.num_steps_done
    out["losses"] = losses
    # tensors go through the queue BY VALUE (numpy): torch's fd-passing of shared storage dies with the rank process
    q.put((rank, {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()}))
    dist.barrier()
    dist.destroy_process_group()
    trainer.envs.close()


def _run(workload, overlap, short_rank1=False):
    world, port = 2, find_free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, workload, overlap, short_rank1)) for r in range(world)]
    for p in procs:
        p.start()
    import queue
    import time
    res, t0 = {}, time.time()
    while len(res) < world:  # fail fast when a rank dies instead of sitting out the timeout on the GPU box
        try:
            r, o = q.get(timeout=2)
            res[r] = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in o.items()}
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or time.time() - t0 > 420:
                for p in procs:
                    p.kill()
                raise AssertionError(f"rank process failed / timed out (exit codes {[p.exitcode for p in procs]})")
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    return res[0], res[1]


@pytest.mark.parametrize("workload", ["c2", "c3"])
def test_ddppo_real_engine_world2(workload):
    from oracle import functional as O
    a, b = _run(workload, overlap=False)
    # rank 0's initial parameters were broadcast (DDP constructor, ddppo.py:128-140)
    assert torch.equal(a["p_init"], b["p_init"])
    # gradients: sum of the local ones, identical on both ranks (test_ddppo_reduce.py:100-116)
    assert torch.equal(a["g_reduced"], b["g_reduced"])
    assert torch.equal(a["g_reduced"], a["g_local"] + b["g_local"])
    assert float((a["g_local"] - b["g_local"]).abs().max()) > 0  # the ranks really saw different data
    # one step == clip + Adam of a single process on the averaged gradient (oracle arithmetic on the flat arena)
    g_avg = (a["g_local"] + b["g_local"]) / 2.0
    p = a["p_before"].clone()
    O.clip_grad_norm([g_avg], a["step_kwargs"]["max_grad_norm"])
    O.adam_step(p, g_avg, torch.zeros_like(p), torch.zeros_like(p), 1, a["lr"], 1e-5)
    upd_ref, upd_got = p - a["p_before"], a["p_after"] - a["p_before"]
    # (the update is read back as a difference of fp32 parameters: one ulp of the largest parameter is the floor)
    assert float((upd_got - upd_ref).abs().max()) <= 1e-4 * float(upd_ref.abs().max()) + 2.4e-7 * max(1.0, float(p.abs().max()))
    # parameters after 2 full cycles: bit-identical across ranks
    assert torch.equal(a["p_final"], b["p_final"])
    assert a["steps_done"] == b["steps_done"] == 2 * 2 * 4 * 8 and a["losses"] == b["losses"]
    if workload == "c3":
        assert a["rmv_err"] <= 1e-5 and b["rmv_err"] <= 1e-5, (a["rmv_err"], b["rmv_err"])
        assert torch.equal(a["rmv_state"], b["rmv_state"]) and a["rmv_count"] == 2 * a["rmv_frames"]
    # early exchange of the arena tail, overlapped with the conv stack's backward: same bits
    a2, b2 = _run(workload, overlap=True)
    assert torch.equal(a2["p_final"], b2["p_final"])
    assert torch.equal(a2["p_final"], a["p_final"]), float((a2["p_final"] - a["p_final"]).abs().max())
    assert torch.equal(a2["g_reduced"], a["g_reduced"])


def test_ddppo_running_mean_var_with_uneven_frame_counts():
    """A preempted rank evaluates fewer frames: the statistics must merge with the real all-reduced frame count and stay identical on
    every rank (round-1 advisor finding: a hard-coded B * world_size lets the buffers diverge for good)."""
    a, b = _run("c3", overlap=True, short_rank1=True)
    assert a["rmv_frames"] == 2 * b["rmv_frames"]
    assert a["rmv_count"] == b["rmv_count"] == a["rmv_frames"] + b["rmv_frames"]
    assert a["rmv_err"] <= 1e-5 and b["rmv_err"] <= 1e-5, (a["rmv_err"], b["rmv_err"])
    assert torch.equal(a["rmv_state"], b["rmv_state"])
    assert torch.equal(a["p_final"], b["p_final"])


def test_bench_py_launches_two_ranks_and_reports_whole_job_rate():
    """The driver's multi-GPU scaling run is the first time RCCL sees more than one rank; everything around the transport must not be
    able to fail there.  `bench.py --full --gpus 2` (the self-launching form: torchrun with --master-addr 127.0.0.1) on ONE GPU with the gloo
    transport (HAB_BENCH_DISTRIB_BACKEND=GLOO; both ranks wrap onto device 0): exactly one JSON line, n_gpus = ranks_seen = 2,
    parallelism dp2, all 2 x 64 x 128 x K env-steps counted, value = env-steps / max-over-ranks time; the `exchange` record and the
    `c4` sub-record (ResNet18 + LSTM on both ranks) are there."""
    import json
    import subprocess
    env = dict(os.environ, HAB_BENCH_DISTRIB_BACKEND="GLOO", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ranks_seen"] == 2 and out["config"]["parallelism"] == "dp2" and out["scaling"] == "weak"
    assert out["steps"] == 2 and out["warmup"] == 1
    steps = 2 * 64 * 128 * 2
    assert abs(out["value"] * out["ms_per_step"] * 2 / 1e3 - steps) <= 0.01 * steps  # whole-job aggregate over both ranks
    assert "cpu_baseline" not in out and "note" in out
    # the line says which exchange carried the gradients, and carries the DD-PPO ResNet18 + LSTM workload (BASELINE.json configs[3]) run by
    # both ranks through a SECOND trainer on the same process group
    assert out["exchange"] == {"comm": "torch-callbacks", "backend": "gloo", "rccl_ranks": None, "process_group_ranks": 2, "grad_overlap": True}
    c4 = out["c4"]
    assert c4["n_gpus"] == 2 and "ResNet18" in c4["workload"] and c4["steps"] == 5
    assert abs(c4["value"] * c4["ms_per_step"] * 5 / 1e3 - 2 * 64 * 128 * 5) <= 0.01 * 2 * 64 * 128 * 5
    # both gradient exchanges in one run: on a gloo group the native RCCL communicator is not wanted, so the second
    # trainer runs the callbacks as well -- two trainers from the same seeds must then end on bit-identical parameter arenas on both ranks
    ab = out["exchange_ab"]
    assert ab["bit_identical"] is True and ab["native_ran"] is False and ab["param_max_abs_diff"] == 0.0, ab
    for k in ("torch-callbacks", "rccl-native"):
        assert ab[k]["exchange_that_ran"] == "torch-callbacks" and ab[k]["value"] > 0 and ab[k]["steps"] == 3, ab


def _reduce_worker(rank, world, port, unused_params, q):
    """The body of the reference's own worker, test/test_ddppo_reduce.py:28-121, on this package's classes: blind
    PointNavBaselinePolicy (only `pointgoal_with_gps_compass`, Discrete(1)), DDPPO, RolloutStorage, one batch through the
    updater's `_evaluate_actions`, autograd backward, gradients compared across ranks."""
    for p in (ROOT, os.path.join(ROOT, "habitat-lab_amd")):
        sys.path.insert(0, p)
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    import torch.distributed as distrib
    from torch import nn
    from habitat_amd.common import spaces as S
    from habitat_amd.common.rollout_storage import RolloutStorage
    from habitat_amd.config.default import get_config
    from habitat_amd.rl.ddppo.ddppo import DDPPO
    from habitat_amd.rl.ppo import PointNavBaselinePolicy
    device = torch.device("cuda")
    store = distrib.TCPStore("127.0.0.1", port, world, rank == 0)
    distrib.init_process_group("gloo", store=store, rank=rank, world_size=world)
    config = get_config("pointnav/ppo_pointnav_example.yaml", ["habitat_baselines.rl.ppo.num_mini_batch=1", "habitat_baselines.rl.ppo.num_steps=16",
                                                               "habitat_baselines.rl.ppo.ppo_epoch=4", "habitat_baselines.rl.ppo.clip_param=0.1"])
    obs_space = S.Dict({"pointgoal_with_gps_compass": S.Box(np.finfo(np.float32).min, np.finfo(np.float32).max, (2,), np.float32)})
    action_space = S.Discrete(1)
    torch.manual_seed(100 + rank)  # different initial weights per rank: init_distributed must make them rank 0's
    actor_critic = PointNavBaselinePolicy.from_config(config, obs_space, action_space)
    if unused_params:
        actor_critic.unused = nn.Linear(64, 64)
    actor_critic.to(device=device)
    ppo_cfg = config.habitat_baselines.rl.ppo
    agent = DDPPO(actor_critic=actor_critic, clip_param=ppo_cfg.clip_param, ppo_epoch=ppo_cfg.ppo_epoch, num_mini_batch=ppo_cfg.num_mini_batch,
                  value_loss_coef=ppo_cfg.value_loss_coef, entropy_coef=ppo_cfg.entropy_coef, lr=ppo_cfg.lr, eps=ppo_cfg.eps,
                  max_grad_norm=ppo_cfg.max_grad_norm, use_normalized_advantage=ppo_cfg.use_normalized_advantage)
    agent.init_distributed(find_unused_params=unused_params)
    rollouts = RolloutStorage(ppo_cfg.num_steps, 2, obs_space, action_space, actor_critic, is_double_buffered=False)
    rollouts.to(device)
    torch.manual_seed(7 + rank)  # the ranks see different observations
    for k, v in rollouts.buffers["observations"].items():
        rollouts.buffers["observations"][k] = torch.randn_like(v)
    rollouts.advance_rollout()
    rollouts.advance_rollout()
    batch = next(rollouts.data_generator(rollouts.buffers["returns"], 1))
    value, action_log_probs, dist_entropy, _, _ = agent._evaluate_actions(batch["observations"], batch["recurrent_hidden_states"], batch["prev_actions"],
                                                                          batch["masks"], batch["actions"], batch["rnn_build_seq_info"])
    (value.mean() + action_log_probs.mean() + dist_entropy.mean()).backward()
    n_checked, local_norm = 0, 0.0
    for name, param in actor_critic.named_parameters():
        if param.grad is not None:
            mine = param.grad.detach().cpu().clone()
            grads = [torch.empty_like(mine) for _ in range(world)]
            distrib.all_gather(grads, mine)
            for i in range(world):
                assert torch.isclose(grads[i], grads[rank]).all(), name
            n_checked += 1
            local_norm += float(mine.abs().sum())
        else:
            assert name.startswith("unused."), name
    assert n_checked == 4 + 2 * 2, n_checked  # GRU (4) + the two heads (2 x 2): a blind policy has no visual encoder
    assert local_norm > 0
    # the full fused update on the same storage: parameters stay identical across ranks, foreign parameters untouched
    before = actor_critic.unused.weight.detach().clone() if unused_params else None
    agent.update(rollouts)
    flat = actor_critic.engine.params_flat.detach().cpu()
    both = [torch.empty_like(flat) for _ in range(world)]
    distrib.all_gather(both, flat)
    assert torch.equal(both[0], both[1])
    if unused_params:
        assert torch.equal(before, actor_critic.unused.weight) and actor_critic.unused.weight.is_cuda
    q.put(rank)
    distrib.barrier()
    distrib.destroy_process_group()


@pytest.mark.parametrize("unused_params", [True, False])
def test_ddppo_reduce_reference_configuration(unused_params):
    """test/test_ddppo_reduce.py:43-56,123-132 as the reference runs it."""
    world, port = 2, find_free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, unused_params, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0, [p.exitcode for p in procs]
    assert sorted(q.get(timeout=5) for _ in range(world)) == [0, 1]


def _native_comm_worker(port, q, native):
    """One rank on the `nccl` backend (RCCL with a single rank: the 1-GPU box cannot host two RCCL ranks), C3-small, two update cycles."""
    for p in (ROOT, os.path.join(ROOT, "habitat-lab_amd")):
        sys.path.insert(0, p)
    os.environ.update(LOCAL_RANK="0", RANK="0", WORLD_SIZE="1", MAIN_ADDR="127.0.0.1", MAIN_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0",
                      HAB_NATIVE_COMM="1" if native else "0", HAB_FORCE_GRAD_OVERLAP="1")
    os.environ.pop("MASTER_PORT", None)
    os.environ.pop("HAB_NO_GRAD_OVERLAP", None)
    import torch.distributed as dist
    import habitat_amd.rl.ppo.ppo_trainer as tr
    from habitat_amd.config.default import read_write
    torch.manual_seed(7)
    cfg = _cfg("c3", 4, 8)
    with read_write(cfg):
        cfg.habitat_baselines.rl.ddppo.distrib_backend = "NCCL"
    trainer = tr.PPOTrainer(cfg)
    trainer._init_train()
    upd, eng = trainer._agent.updater, trainer._agent.actor_critic.engine
    assert dist.get_backend() == "nccl" and (upd._native_comm is not None) == native
    if native:  # the communicator itself: in-place sum over the one rank = identity, on the current stream
        t = torch.arange(1000, device="cuda", dtype=torch.float32)
        assert torch.equal(upd._native_comm.all_reduce_sum_(t.clone()), t)
        assert upd._native_comm.world_size() == 1
        # 1000 rounds of the start-up self-test: the communicator's all-reduces on two side streams (the tails' and the moments' roles),
        # alternating with torch.distributed's own RCCL all-reduce on its stream -- event reuse and cross-stream ordering under load
        from habitat_amd.rl.ddppo.ddppo import _native_comm_selftest
        os.environ["HAB_NATIVE_COMM_SELFTEST"] = "1000"
        ok, detail = _native_comm_selftest(upd._native_comm, torch.device("cuda", torch.cuda.current_device()), 120.0)
        assert ok, detail
    for _ in range(2):
        losses = trainer.run_update_cycle()
        assert all(np.isfinite(v) for v in losses.values()), losses
    torch.cuda.synchronize()
    q.put({"p_final": eng.params_flat.cpu().numpy(), "rmv": np.concatenate([v.cpu().numpy().reshape(-1) for k, v in
                                                                             trainer._agent.actor_critic.state_dict().items() if "running_mean_and_var" in k]),
           "losses": {k: float(v) for k, v in losses.items()}})
    trainer.shutdown()
    dist.destroy_process_group()
    trainer.envs.close()


def test_device_side_exchange_on_rccl_matches_the_callback_form():
    """csrc/comm.hip: with HAB_NATIVE_COMM the library's own RCCL communicator carries the gradient exchange (tails enqueued by the
    engine inside backward, head + join in hab_policy_grad_sync) and the RunningMeanAndVar sums (inside the training forward).  On the
    `nccl` backend with one rank -- all this box can host -- two full update cycles of the ResNet18 policy must leave bit-identical
    parameters and statistics to the callback form through torch.distributed (every stream dependency and range of the exchange is
    exercised; the sums themselves are RCCL's)."""
    res = []
    for native in (True, False):
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        p = ctx.Process(target=_native_comm_worker, args=(find_free_port(), q, native))
        p.start()
        import queue
        import time
        t0, got = time.time(), None
        while got is None:
            try:
                got = q.get(timeout=2)
            except queue.Empty:
                if p.exitcode not in (None, 0) or time.time() - t0 > 420:
                    p.kill()
                    raise AssertionError(f"rank process failed / timed out (exit code {p.exitcode}, native={native})")
        p.join(120)
        assert p.exitcode == 0
        res.append(got)
    a, b = res
    assert np.array_equal(a["p_final"], b["p_final"]) and np.array_equal(a["rmv"], b["rmv"]) and a["losses"] == b["losses"]
