"""CPU: the shortest-path follower of Nav2D-v0 / Nav2DVel-v0 on its numpy restatement (tests/nav2d_follow_reference.py): what it
scores on generated worlds, the properties the rule promises, hand-made worlds, the velocity action's round trip through the env's
decoder, the header against the binding table, and the refusals of the Python layer."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import nav2d_follow_reference as FR
import nav2d_geo_reference as G
import nav2d_reference as R
import nav2d_vel_reference as V

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS, ENVS, EPISODES = (1, 100), 24, 5
VEL_SAMPLES = {"5/30/5": (dict(turn_angle=5, max_turn_angle=30, min_abs_ang_speed=5), 8, 4, 3),
               "1/10": (dict(turn_angle=1, max_turn_angle=10), 3, 2, 2)}


@functools.lru_cache(maxsize=None)
def discrete_run(seed, turn):
    """The first 5 episodes of envs 0..23 at 8 obstacles under the follower."""
    out = []
    for e in range(ENVS):
        env = G.Nav2DGeoEnv(seed, e, num_obstacles=8, turn_angle=turn, max_episode_steps=500, use_rgb=False, use_depth=False)
        out += [dict(ep, env=e, index=i) for i, ep in enumerate(FR.episodes(env, EPISODES))]
    return out


@functools.lru_cache(maxsize=None)
def velocity_run(name):
    kw, K, envs, count = VEL_SAMPLES[name]
    out = []
    for e in range(envs):
        env = G.Nav2DVelGeoEnv(3, e, num_obstacles=K, max_episode_steps=500, use_rgb=False, use_depth=False, **kw)
        out += FR.episodes(env, count)
    return out


def all_runs():
    return ([discrete_run(s, t) for s in SEEDS for t in (10, 30)]) + [velocity_run(k) for k in VEL_SAMPLES]


@pytest.mark.parametrize("seed", SEEDS)
def test_discrete_follower_on_generated_worlds(seed):
    """turn_angle = 10: every reachable episode succeeds, no collision, no STUCK, mean SPL >= 0.99 and lowest >= 0.95 (measured:
    120 / 120 at both seeds, means 0.9990 / 0.9980, minima 0.9789 / 0.9754).  An unreachable episode is given up at its first step."""
    eps = discrete_run(seed, 10)
    reach = [e for e in eps if e["reachable"]]
    spl = [e["spl"] for e in reach]
    print(f"nav2d follower seed {seed}: {sum(e['success'] for e in reach)} / {len(reach)} reachable of {len(eps)}, "
          f"SPL mean {np.mean(spl):.4f} min {min(spl):.4f}")
    assert len(eps) == ENVS * EPISODES and len(reach) >= 100
    assert all(e["success"] and e["end"] == FR.ARRIVED for e in reach)
    assert sum(e["collisions"] for e in eps) == 0 and not any(e["timeout"] for e in eps)
    assert np.mean(spl) >= 0.99 and min(spl) >= 0.95
    for e in eps:
        if not e["reachable"]:
            assert e["end"] == FR.UNREACHABLE and len(e["steps"]) == 1 and not e["success"]


@pytest.mark.parametrize("seed", SEEDS)
def test_coarse_headings_give_up_honestly(seed):
    """turn_angle = 30: no collision; every reachable episode ends ARRIVED with success, or STUCK; no timeout; STUCK in at most 5 %
    of the reachable episodes (measured 1 and 2 of 120)."""
    eps = discrete_run(seed, 30)
    reach = [e for e in eps if e["reachable"]]
    stuck = [e for e in reach if e["end"] == FR.STUCK]
    print(f"nav2d follower seed {seed}, 30 degrees: {len(stuck)} STUCK of {len(reach)}")
    assert sum(e["collisions"] for e in eps) == 0 and not any(e["timeout"] for e in eps)
    assert all((e["end"] == FR.ARRIVED and e["success"]) or (e["end"] == FR.STUCK and not e["success"]) for e in reach)
    assert 20 * len(stuck) <= len(reach)


@pytest.mark.parametrize("name", list(VEL_SAMPLES))
def test_velocity_follower(name):
    """Both parameter sets: every episode succeeds without a collision (measured 12 / 12 and 4 / 4)."""
    eps = velocity_run(name)
    _, _, envs, count = VEL_SAMPLES[name]
    assert len(eps) == envs * count and all(e["reachable"] for e in eps)
    assert all(e["success"] and e["end"] == FR.ARRIVED and e["collisions"] == 0 and not e["timeout"] for e in eps)
    kw = VEL_SAMPLES[name][0]
    M = kw["max_turn_angle"] // kw["turn_angle"]
    big = [s for e in eps for s in e["steps"] if s["status"] == FR.GO and abs(s["delta"]) > M]
    assert big and not any(s["moved"] for s in big)            # turns in place happen, and move nothing


def test_properties_on_those_runs():
    """d falls strictly at every forward; every forward the follower asks for is taken; the winner is constant between moves;
    next_d equals the d the env then reports."""
    forwards = turns = 0
    for eps in all_runs():
        for e in eps:
            winner = None
            for s in e["steps"]:
                if s["status"] != FR.GO:
                    assert s is e["steps"][-1]
                    continue
                if winner is not None:
                    assert s["winner"] == winner, "the winner changed while the agent only turned"
                if s["d_after"] is None:      # the step limit ended the episode: never here
                    continue
                if s["moved"]:
                    forwards += 1
                    assert s["d_after"] == s["next_d"] and s["d_after"] < s["d_prev"]
                    winner = None
                else:
                    turns += 1
                    assert s["delta"] != 0, "a forward was refused"
                    assert s["d_after"] == s["d_prev"]
                    winner = s["winner"]
    assert forwards > 1000 and turns > 1000      # the properties were looked at often


@pytest.mark.parametrize("case", FR.hand_made_cases(), ids=lambda c: c[0])
def test_hand_made_worlds(case):
    env = FR.hand_made_env(case)
    status, delta, next_d = FR.follow(env)
    assert (status, delta) == case[-1]
    assert FR.discrete_action(status, delta) == (R.STOP if status != FR.GO else
                                                 R.MOVE_FORWARD if delta == 0 else R.TURN_LEFT if delta > 0 else R.TURN_RIGHT)
    if status == FR.ARRIVED:
        assert next_d == env.d_prev
        _, _, done, info = env.step(R.STOP)
        assert done and info["success"] == 1.0
    elif status == FR.GO:
        assert next_d < env.d_prev
    else:
        assert np.isposinf(next_d)


def test_mirror_pair_is_a_tie_and_infinite_candidates_lose():
    """The premises of two hand-made cases: the two mirror candidates have bitwise one value, the lowest; inside the ring every
    candidate is free and sees nothing."""
    env = FR.hand_made_env(FR.hand_made_cases()[1])
    w = env.world
    free, v = FR.candidates(env.px, env.py, w.rects, w.gx, w.gy, env.D, env.dirs)
    assert free.all() and v[2] == v[4] == v.min() and (v == v.min()).sum() == 2
    env = FR.hand_made_env(FR.hand_made_cases()[-1])
    w = env.world
    free, v = FR.candidates(env.px, env.py, w.rects, w.gx, w.gy, env.D, env.dirs)
    assert free.all() and np.isposinf(v).all()


def test_stuck_state_is_the_run_s():
    """The STUCK world the reference keeps is the state at which the 30 degree run of seed 1 gave up."""
    stuck = [e for e in discrete_run(1, 30) if e["end"] == FR.STUCK]
    assert len(stuck) == 1 and (stuck[0]["env"], stuck[0]["index"]) == (6, 3)
    last = stuck[0]["steps"][-1]
    s = last["state"]
    assert s["rects"] == FR.STUCK_RECTS and (s["px"], s["py"]) == FR.STUCK_START and (s["gx"], s["gy"]) == FR.STUCK_GOAL
    assert s["h"] == FR.STUCK_HEADING and last["d_prev"] == FR.STUCK_D_PREV
    case = [c for c in FR.hand_made_cases() if c[-1][0] == FR.STUCK][0]
    assert FR.hand_made_env(case).d_prev == FR.STUCK_D_PREV


def test_a_ang_round_trip():
    """Every |delta| <= M <= 180: (1, fl(fl(delta) / fl(M))) decodes to l = 0.25 and dh = delta."""
    for M in range(1, 181):
        for delta in range(-M, M + 1):
            a = FR.velocity_action(FR.GO, delta, M)
            c_lin, c_ang, l, dh, _ = V.decode(a, M)
            assert l == R.FORWARD and dh == delta, (M, delta)
    assert FR.velocity_action(FR.GO, 11, 10) == (F(-1.0), F(1.0)) and FR.velocity_action(FR.GO, -11, 10) == (F(-1.0), F(-1.0))
    for a, M in ((FR.velocity_action(FR.GO, 11, 10), 10), (FR.velocity_action(FR.GO, -11, 10), 10)):
        _, _, l, dh, _ = V.decode(a, M)
        assert l == 0 and abs(dh) == M
    _, _, l, dh, _ = V.decode(FR.VEL_STOP, 10)
    assert l == 0 and dh == 0 and FR.velocity_action(FR.STUCK, 3, 10) == FR.VEL_STOP


def test_header_and_signature_table_agree():
    """The header's prototypes of the two entries and the ctypes table: the same number of arguments, pointers where the header has
    pointers, size_t and int in their places; the velocity entry is the discrete one with max_turn_steps before the stream; the
    status codes are the restatement's."""
    from habitat_amd import _lib
    text = open(os.path.join(ROOT, "include", "habitat_amd.h")).read()
    kinds = {"size_t": ctypes.c_size_t, "int": ctypes.c_int}

    def names(entry):
        m = re.search(r"int %s\((.*?)\);" % entry, text, re.S)
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
        restype, argtypes = _lib.SIGNATURES[entry]
        assert restype is ctypes.c_int and len(params) == len(argtypes), entry
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if ("*" in p or p.startswith("hipStream_t")) else kinds[p.split()[0]]
            assert t is want, (entry, p)
        return [p.split()[-1].lstrip("*") for p in params]

    plain, vel = names("hab_nav2d_follow"), names("hab_nav2d_vel_follow")
    assert plain == ["state", "state_stride_bytes", "geo", "dirs", "mask", "actions", "next_d", "status", "N", "num_obstacles",
                     "num_headings", "stream"]
    assert vel == plain[:-1] + ["max_turn_steps", "stream"]
    codes = {k: int(v) for k, v in re.findall(r"#define HAB_NAV2D_FOLLOW_(\w+) +(\d+)", text)}
    assert codes == dict(GO=FR.GO, ARRIVED=FR.ARRIVED, UNREACHABLE=FR.UNREACHABLE, STUCK=FR.STUCK)
    L = _lib.lib()
    assert hasattr(L, "hab_nav2d_follow") and hasattr(L, "hab_nav2d_vel_follow")


def test_python_refusals():
    """Without a GPU: the four tasks without a follower refuse by name, the two with one refuse the Euclidean mode; so does
    ShortestPathFollower."""
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as EF
    from habitat_amd.common.shortest_path_follower import ShortestPathFollower
    assert EF.Nav2DVectorEnv._follow_entry == "hab_nav2d_follow" and EF.Nav2DVelVectorEnv._follow_entry == "hab_nav2d_vel_follow"
    for cls, name in ((EF.Nav2DObjVectorEnv, "Nav2DObj"), (EF.Nav2DRearrVectorEnv, "Nav2DRearr"), (EF.Nav2DRearrVelVectorEnv, "Nav2DRearrVel"),
                      (EF.Nav2DSocialVectorEnv, "Nav2DSocial")):
        assert cls._follow_entry is None
        for distance in EF.NAV2D_DISTANCES:
            env = cls.__new__(cls)                # no device: the refusal comes before anything of the env is touched
            env.distance = distance
            with pytest.raises(_lib.HabError, match=name + ":.*no shortest-path follower"):
                env.follower_actions()
            with pytest.raises(_lib.HabError, match=name + ":"):
                ShortestPathFollower(env)
    for cls, name in ((EF.Nav2DVectorEnv, "Nav2D"), (EF.Nav2DVelVectorEnv, "Nav2DVel")):
        env = cls.__new__(cls)
        env.distance = "euclidean"
        with pytest.raises(_lib.HabError, match=name + ":.*needs `distance_to_goal: geodesic`"):
            env.follower_actions()
        with pytest.raises(_lib.HabError, match="geodesic"):
            ShortestPathFollower(env)
    with pytest.raises(_lib.HabError, match="no shortest-path follower"):
        ShortestPathFollower(object())
