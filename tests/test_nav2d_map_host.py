"""CPU: the restatement of the top-down map (tests/nav2d_map_reference.py) checked independently of itself -- in float64, on every
script and case of the six tasks -- and the host side of the feature: the keyword's refusals, the factory's pass-through, the header
against the binding and the colour tables, the frame's panel arithmetic, and the evaluator's video files on a stub env."""
import functools
import os
import re
import types

import numpy as np
import pytest

import nav2d_map_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOLUTIONS = (16, 40, 128)
MARGIN = 1e-4   # a cell whose centre is nearer than this to a boundary it is tested against may fall on either side in float32


@functools.lru_cache(maxsize=4)
def scripted_actions(task, kind, case):
    return M.TASKS[task].actions(kind, case)[0]


def centres64(S):
    cell = 8.0 / S
    x = (np.arange(S) + 0.5) * cell
    y = (S - 1 - np.arange(S) + 0.5) * cell
    return x[None, :], y[:, None]


def static64(v, S):
    """(codes, sure): the static layer's rules in float64 and the cells farther than MARGIN from every boundary tested."""
    X, Y = centres64(S)
    shape = (S, S)
    code, sure = np.ones(shape, np.int64), np.ones(shape, bool)
    for x0, y0, x1, y1 in ((float(a) for a in r) for r in v.rects):
        code[np.broadcast_to((X > x0) & (X < x1) & (Y > y0) & (Y < y1), shape)] = M.OCCUPIED
        for edge, Z in ((x0, X), (x1, X), (y0, Y), (y1, Y)):
            sure &= np.broadcast_to(np.abs(Z - edge) > MARGIN, shape)

    def disc(cx, cy, r):
        d = np.hypot(X - float(cx), Y - float(cy))
        return d <= r, np.abs(d - r) > MARGIN

    for pick in (M.OBJECT, M.TARGET):
        for x, y, r2, c in v.markers:
            if c == pick:
                inside, ok = disc(x, y, {float(M.GOAL_R2): 0.2, float(M.OBJ_R2): 0.3}[float(r2)])
                code[inside & (code != M.TARGET)] = c
                sure &= ok
    inside, ok = disc(v.px, v.py, 0.15)
    code[inside] = M.START
    return code, sure & ok


def separated64(px, py, X, Y, rects):
    """Per cell centre (1-D X, Y): whether the segment from (px, py) crosses the interior of a rectangle shrunk by MARGIN, float64,
    by clipping the segment's parameter interval against the two slabs."""
    px, py = float(px), float(py)
    out = np.zeros(X.shape, bool)
    for x0, y0, x1, y1 in ((float(a) for a in r) for r in rects):
        lo, hi = np.zeros(X.shape), np.ones(X.shape)
        for p, q, a, b in ((px, X, x0 + MARGIN, x1 - MARGIN), (py, Y, y0 + MARGIN, y1 - MARGIN)):
            d = q - p
            with np.errstate(divide="ignore", invalid="ignore"):
                t0, t1 = (a - p) / d, (b - p) / d
            par = d == 0
            lo = np.where(par, np.where((p > a) & (p < b), lo, np.inf), np.maximum(lo, np.minimum(t0, t1)))
            hi = np.where(par, hi, np.minimum(hi, np.maximum(t0, t1)))
        out |= lo < hi
    return out


def check_begin(run, n, S, unsure):
    v = M.view(run.task, run.envs[n])
    want, sure = static64(v, S)
    unsure[0] += int((~sure).sum())
    unsure[1] += sure.size
    static = M.static_layer(v, S)
    assert np.array_equal(static[sure], want[sure].astype(np.uint8)), "static layer against float64"
    drawn = run.map[n] != static
    assert (run.map[n][drawn] == M.TRAJECTORY).all() and not np.isin(static[drawn], (M.START, M.TARGET)).any()
    first = np.zeros((S, S), np.uint8)
    M.reveal(first, v, S, run.vis)
    assert np.array_equal(run.fog[n], first), "fog right after a clear is the first reveal alone"
    rec = run.rec[n]
    assert rec[M.W_EPISODE] == v.episode and (rec[5:] == 0).all()
    assert np.array_equal(rec[1:5].view(np.float32), np.array([v.px, v.py, v.px, v.py], np.float32))


def agent_cell(e, S):
    cell = 8.0 / S
    return S - 1 - int(float(e.py) / cell), int(float(e.px) / cell)


def check_run(task, kind, case, S, unsure):
    t = M.TASKS[task]
    run = M.MapRun(t.code, t.make_envs(kind, case), S)
    run.reset()
    X, Y = centres64(S)
    for n in range(len(run.envs)):
        check_begin(run, n, S, unsure)
    occupied = [M.occupied(*M.centres(S), e.world.rects) for e in run.envs]   # per env, of its running episode
    begins = 0
    for a in scripted_actions(task, kind, case):
        fog0 = run.fog.copy()
        before = [(e.px, e.py) for e in run.envs]
        run.step(a)
        for n, e in enumerate(run.envs):
            r, c = agent_cell(e, S)
            assert run.map[n, r, c] != M.OCCUPIED, "the agent's cell is never shown occupied"
            if run.dones[n]:
                begins += 1
                check_begin(run, n, S, unsure)
                occupied[n] = M.occupied(*M.centres(S), e.world.rects)
                new = run.fog[n] == 1
            else:
                assert (run.fog[n] >= fog0[n]).all(), "fog never falls within an episode"
                if (e.px, e.py) != before[n]:
                    assert run.map[n, r, c] in (M.TRAJECTORY, M.START, M.TARGET), "an accepted move lands on the trajectory"
                assert np.array_equal(run.rec[n, 3:5].view(np.float32), np.array([e.px, e.py], np.float32))
                new = (run.fog[n] == 1) & (fog0[n] == 0)
            rr, cc = np.nonzero(new)
            if rr.size:
                assert not separated64(e.px, e.py, X[0, cc], Y[rr, 0], e.world.rects).any(), "a seen cell is behind a rectangle"
                assert not occupied[n][new].any(), "occupied cells are never marked"
    assert begins > 0


def _runs():
    for name, t in M.TASKS.items():
        for kind in t.scripts:
            yield pytest.param(name, kind, id=f"{name}-{kind}")


@pytest.mark.parametrize("task,kind", list(_runs()))
def test_map_properties_on_every_script_and_case(task, kind):
    """Every script of the task over its SCRIPT_CASES at S = 16, 40 and 128: the properties of check_run and check_begin, and the
    cells that the float64 comparison leaves out for lying within 1e-4 m of a boundary are at most 2 % of the cells."""
    unsure = [0, 0]
    for case in M.TASKS[task].cases:
        for S in RESOLUTIONS:
            check_run(task, kind, case, S, unsure)
    assert unsure[0] <= 0.02 * unsure[1], unsure


# ---- frames ---------------------------------------------------------------------------------------------------------------------
def short_run(task="rearr", S=40, steps=20, H=0, W=0):
    t = M.TASKS[task]
    case = t.cases[-1]
    acts = scripted_actions(task, t.turning, case)[:steps]
    kw = dict(H=H, W=W) if H else {}
    run = M.MapRun(t.code, t.make_envs(t.turning, case, **kw), S)
    run.reset()
    for a in acts:
        run.step(a)
    return run


@pytest.mark.parametrize("draw_fog", [True, False])
def test_frame_colours_follow_the_fog(draw_fog):
    """At Hf = S a pixel is a cell: a free cell without an overlay shows the table's colour where it has been seen and, with
    draw_fog, each channel >> 1 where not; every other code shows the table's colour."""
    run = short_run()
    run.draw_fog = draw_fog
    S = run.S
    fr = run.frames(S)
    assert fr.shape == (len(run.envs), S, S, 3)
    for n, e in enumerate(run.envs):
        code = M.map_panel_codes(run.map[n], M.view(run.task, e), S)
        free, seen = code == M.FREE, run.fog[n] == 1
        assert free.any() and (free & seen).any() and (free & ~seen).any() and (code == M.AGENT).any()
        assert (fr[n][free & seen] == M.COLORS[M.FREE]).all()
        assert (fr[n][free & ~seen] == (M.COLORS[M.FREE] >> 1 if draw_fog else M.COLORS[M.FREE])).all()
        assert np.array_equal(fr[n][~free], M.COLORS[code[~free]])


@pytest.mark.parametrize("H,W", [(12, 20), (9, 18)])
@pytest.mark.parametrize("Hf", [24, 50])
def test_frame_panels(H, W, Hf):
    """Panel widths follow the helper (the library's and the restatement's), the image panels are nearest-neighbour picks of the
    observation and the grey of depth is (int)(d * 255)."""
    from habitat_amd import _lib
    run = short_run("rearr", 16, 6, H, W)
    Wp = (Hf * W) // H
    for rgb, depth in ((True, True), (False, True), (False, False)):
        want = Hf + (int(rgb) + int(depth)) * Wp
        assert M.frame_width(Hf, H, W, rgb, depth) == want == _lib.lib().hab_nav2d_map_frame_width(Hf, H, W, int(rgb), int(depth))
        fr = run.frames(Hf, "head_rgb" if rgb else None, "head_depth" if depth else None)
        assert fr.shape == (len(run.envs), Hf, want, 3)
        sr, sc = (np.arange(Hf) * H) // Hf, (np.arange(Wp) * W) // Wp
        for n in range(len(run.envs)):
            x = 0
            if rgb:
                assert np.array_equal(fr[n][:, :Wp], run.obs[n]["head_rgb"][sr][:, sc])
                x = Wp
            if depth:
                g = (run.obs[n]["head_depth"][..., 0][sr][:, sc].astype(np.float64) * 255.0).astype(np.int64)
                assert np.array_equal(fr[n][:, x:x + Wp], np.repeat(g[..., None], 3, 2))
    assert _lib.lib().hab_nav2d_map_frame_width(0, H, W, 1, 1) < 0 and _lib.lib().hab_nav2d_map_frame_width(Hf, 0, W, 1, 0) < 0


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
def _classes():
    from habitat_amd.common import env_factory as E
    return (E.Nav2DVectorEnv, E.Nav2DVelVectorEnv, E.Nav2DObjVectorEnv, E.Nav2DRearrVectorEnv, E.Nav2DRearrVelVectorEnv,
            E.Nav2DSocialVectorEnv)


@pytest.mark.parametrize("bad,word", [(dict(map_resolution=15), "map_resolution"), (dict(map_resolution=513), "map_resolution"),
                                      (dict(map_resolution=64.0), "map_resolution"), (dict(map_resolution=True), "map_resolution"),
                                      (dict(visibility_dist=0.0), "visibility_dist"), (dict(visibility_dist=-1.0), "visibility_dist"),
                                      (dict(visibility_dist=float("inf")), "visibility_dist"),
                                      (dict(visibility_dist=float("nan")), "visibility_dist"), (dict(visibility_dist="far"), "visibility_dist"),
                                      (dict(fov=79), "fov"), (dict(draw_fog=1), "draw_fog"), ("yes", "top_down_map")])
def test_keyword_refusals(bad, word):
    """Every class refuses by name, before it touches a device."""
    from habitat_amd._lib import HabError
    for cls in _classes():
        with pytest.raises(HabError, match=word) as err:
            cls(2, 16, 16, device="cpu", top_down_map=bad)
        assert cls._name + ":" in str(err.value)


def test_keyword_accepted_values():
    from habitat_amd.common.env_factory import nav2d_map_parameters
    assert nav2d_map_parameters(None) is None
    assert nav2d_map_parameters({}) == (128, 5.0, True)
    assert nav2d_map_parameters(dict(map_resolution=16, visibility_dist=2, draw_fog=False, fov=90.0, draw_source=True)) == (16, 2.0, False)
    assert nav2d_map_parameters(dict(map_resolution=np.int64(512))) == (512, 5.0, True)


@pytest.mark.parametrize("yaml", ["pointnav/ppo_nav2d.yaml", "pointnav/ppo_nav2d_vel.yaml", "objectnav/ddppo_nav2d_objectnav.yaml",
                                  "rearrange/ddppo_nav2d_rearrange.yaml", "rearrange/ddppo_nav2d_rearrange_vel.yaml",
                                  "social_nav/ddppo_nav2d_social.yaml"])
def test_factory_passes_the_measurement_through(yaml, monkeypatch):
    from habitat_amd.common import env_factory as E
    from habitat_amd.config.default import get_config
    seen = {}

    def recorder(name):
        def make(*a, **kw):
            seen.update(kw, cls=name)
            return name
        return make

    for cls in _classes():
        monkeypatch.setattr(E, cls.__name__, recorder(cls.__name__))
    fac = E.SyntheticVectorEnvFactory()
    fac.construct_envs(get_config(yaml), device="cpu")
    assert "top_down_map" not in seen, "without the measurement the keyword is not given"
    fac.construct_envs(get_config(yaml, ["habitat.task.measurements.top_down_map.map_resolution=40"]), device="cpu")
    assert seen["top_down_map"] == dict(map_resolution=40)
    fac.construct_envs(get_config(yaml, ["habitat.task.measurements.top_down_map.visibility_dist=2.5",
                                         "habitat.task.measurements.top_down_map.draw_fog=false",
                                         "habitat.task.measurements.top_down_map.fov=90"]), device="cpu")
    assert seen["top_down_map"] == dict(visibility_dist=2.5, draw_fog=False, fov=90)
    monkeypatch.undo()
    with pytest.raises(E._lib.HabError, match="map_resolution"):
        fac.construct_envs(get_config(yaml, ["habitat.task.measurements.top_down_map.map_resolution=8"]), device="cpu")


def header():
    src = open(os.path.join(ROOT, "include", "habitat_amd.h")).read()
    return src, {k: int(v, 0) for k, v in re.findall(r"#define (HAB_NAV2D_MAP_[A-Z0-9_]+) (-?(?:0x)?[0-9A-Fa-f]+)\b", src)}


def test_header_binding_and_tables_agree():
    from habitat_amd import _lib
    from habitat_amd.common import env_factory as E
    src, d = header()
    L = _lib.lib()
    for name in ("hab_nav2d_map_rec_bytes", "hab_nav2d_map_update", "hab_nav2d_map_frame_width", "hab_nav2d_map_frame"):
        decl = re.search(name + r"\((.*?)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S).group(1)
        count = 0 if decl.strip() == "void" else decl.count(",") + 1
        assert count == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name)
    assert L.hab_nav2d_map_rec_bytes() == d["HAB_NAV2D_MAP_REC_BYTES"] == 32 == 4 * M.REC_WORDS
    assert [d[f"HAB_NAV2D_MAP_W_{k}"] for k in ("EPISODE", "START_X", "START_Y", "PREV_X", "PREV_Y", "ZERO")] == [
        M.W_EPISODE, M.W_START_X, M.W_START_Y, M.W_PREV_X, M.W_PREV_Y, 5]
    assert (d["HAB_NAV2D_MAP_MIN_RESOLUTION"], d["HAB_NAV2D_MAP_MAX_RESOLUTION"]) == (M.MIN_RESOLUTION, M.MAX_RESOLUTION) == (
        E.NAV2D_MAP_MIN_RESOLUTION, E.NAV2D_MAP_MAX_RESOLUTION)
    tasks = [d[f"HAB_NAV2D_MAP_TASK_{k}"] for k in ("GOAL", "OBJ", "REARR", "SOCIAL")]
    assert tasks == [M.TASK_GOAL, M.TASK_OBJ, M.TASK_REARR, M.TASK_SOCIAL] == [E.NAV2D_MAP_TASK_GOAL, E.NAV2D_MAP_TASK_OBJ,
                                                                              E.NAV2D_MAP_TASK_REARR, E.NAV2D_MAP_TASK_SOCIAL]
    codes = dict(occupied=M.OCCUPIED, free=M.FREE, start=M.START, target=M.TARGET, trajectory=M.TRAJECTORY, object=M.OBJECT,
                 carried=M.CARRIED, person=M.PERSON, agent=M.AGENT, tick=M.TICK)
    assert codes == E.NAV2D_MAP_CODES == {k: d[f"HAB_NAV2D_MAP_{k.upper()}"] for k in codes}
    assert [M.OCCUPIED, M.FREE, M.START, M.TARGET] == [0, 1, 4, 6] and M.TRAJECTORY == 10   # habitat's values
    table = re.search(r"#define HAB_NAV2D_MAP_COLORS \{(.*?)\}", src, flags=re.S).group(1).replace("\\", "")
    words = [int(w, 16) for w in re.findall(r"0x[0-9A-Fa-f]+", table)]
    assert len(words) == 32
    rgb = np.array([[w & 255, (w >> 8) & 255, (w >> 16) & 255] for w in words], np.uint8)
    assert np.array_equal(rgb, M.COLORS) and np.array_equal(rgb, E.NAV2D_MAP_COLORS)


# ---- the evaluator on a stub env ------------------------------------------------------------------------------------------------
class StubEnvs:
    """Two envs whose episodes last 3 and 5 steps; frame t of env n is filled with a value that tells n, the episode and t."""
    num_envs, LENGTHS = 2, (3, 5)

    def __init__(self, with_frames=True):
        self.number_of_episodes = [1 << 30] * 2
        self.episode, self.t = [0, 0], [0, 0]
        if with_frames:
            self.render_frames = self._render_frames

    def reset(self):
        return [dict(x=np.zeros(1, np.float32)) for _ in range(2)]

    def post_step(self, obs):
        return obs

    def current_episodes(self):
        return [dict(scene_id="stub", episode_id=f"{n}:{self.episode[n]}") for n in range(2)]

    def step(self, actions):
        out = []
        for n in range(2):
            self.t[n] += 1
            done = self.t[n] == self.LENGTHS[n]
            info = dict(success=float(n), spl=0.125 * (self.episode[n] + 1)) if done else {}
            if done:
                self.episode[n], self.t[n] = self.episode[n] + 1, 0
            out.append((dict(x=np.zeros(1, np.float32)), 1.0, done, info))
        return out

    def _render_frames(self):
        import torch
        f = torch.zeros(2, 6, 8, 3, dtype=torch.uint8)
        for n in range(2):
            f[n] = 100 * n + 10 * self.episode[n] + self.t[n]
        return f

    def pause_at(self, i):
        raise AssertionError("never paused")


def stub_evaluation(tmp_path, video_option, with_frames=True, episodes=3):
    import torch
    from habitat_amd.common import spaces
    from habitat_amd.rl.ppo import evaluator as EV
    from habitat_amd.rl.ppo import ppo_trainer as PT

    class Policy:
        policy_action_space = spaces.Discrete(4)
        hidden_state_shape = (1, 4)

        def act(self, obs, h, prev, masks, deterministic=False):
            n = h.shape[0]
            a = torch.ones(n, 1, dtype=torch.long)
            return types.SimpleNamespace(should_inserts=None, rnn_hidden_states=h, actions=a, env_actions=a)

        def get_extra(self, action_data, infos, dones):
            return [{} for _ in infos]

        def on_envs_pause(self, ids):
            pass

    agent = types.SimpleNamespace(actor_critic=Policy(), masks_shape=(1,), eval=lambda: None)
    cfg = types.SimpleNamespace(habitat_baselines=types.SimpleNamespace(
        eval=types.SimpleNamespace(video_option=video_option, evals_per_ep=1), test_episode_count=episodes, video_dir=str(tmp_path / "v"),
        video_fps=10))
    writer = types.SimpleNamespace(add_scalar=lambda *a: None)
    ev = EV.HabitatEvaluator()
    orig = PT.batch_obs
    PT.batch_obs = lambda obs, device: {"x": torch.zeros(len(obs), 1)}
    try:
        ev.evaluate_agent(agent, StubEnvs(with_frames), cfg, 7, 0, writer, "cpu", [], None, set())
    finally:
        PT.batch_obs = orig
    return ev


def test_evaluator_writes_one_file_per_episode(tmp_path):
    from habitat_amd.rl.ppo.evaluator import read_episode_video
    ev = stub_evaluation(tmp_path, ["disk"])
    files = sorted(os.listdir(tmp_path / "v"))
    assert len(files) == len(ev.last_stats_episodes) == len(ev.last_video_files) >= 3
    for ((scene, episode_id), _), stats in ev.last_stats_episodes.items():
        n, episode = (int(x) for x in episode_id.split(":"))
        stem = f"episode={n}_{episode}-ckpt=7-success={stats['success']:.2f}-spl={stats['spl']:.2f}"
        match = [f for f in files if os.path.splitext(f)[0] == stem]
        assert len(match) == 1, (stem, files)
        frames = read_episode_video(str(tmp_path / "v" / match[0]))
        assert frames.shape == (StubEnvs.LENGTHS[n], 6, 8, 3) == (ev.last_episode_lengths[((scene, episode_id), 1)], 6, 8, 3)
        # the ending step's frame opens the next episode: frame t of this file is (n, episode, t)
        assert [int(f[0, 0, 0]) for f in frames] == [100 * n + 10 * episode + t for t in range(StubEnvs.LENGTHS[n])]


def test_evaluator_refusals_stay(tmp_path):
    from habitat_amd._lib import HabError
    text = "eval.video_option: video generation needs the simulator's renderer and is not part of this path"
    for option, with_frames in ((["tensorboard"], True), (["disk", "tensorboard"], True), (["disk"], False)):
        with pytest.raises(HabError) as err:
            stub_evaluation(tmp_path, option, with_frames)
        assert str(err.value) == text
    assert not os.path.exists(tmp_path / "v")
    assert len(stub_evaluation(tmp_path, [], False).last_stats_episodes) >= 3 and not os.path.exists(tmp_path / "v")
