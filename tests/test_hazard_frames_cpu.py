"""CPU: moving hazards (goal_rules.MovingHazards): the frame rule at its boundaries, the constructor's refusals, `circling`
against the reference's own gremlin motion (tests/golden/gremlin_cases.npz, made by tests/golden/make_gremlin_fixture.py), the
host waypoint loop with frames against a hand loop and split into calls, and the C ABI's new struct and symbols."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as rules
from mobrob_amd.envs.goal_rules import MovingHazards
from mobrob_amd.envs.wrapper import get_env
from mobrob_amd.waypoints import follow_waypoints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gremlin_cases.npz")


def _frames(F, M, S=None, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2, 2, ((F, M, 2) if S is None else (S, F, M, 2)))


@pytest.mark.parametrize("loop", [False, True], ids=["hold", "loop"])
def test_frame_index_and_rows_at_the_boundaries(loop):
    F, M, fs = 3, 5, 7
    loc = _frames(F, M)
    size = np.random.default_rng(1).uniform(0.1, 0.4, (1, F, M))
    hz = MovingHazards(loc, size, frame_steps=fs, loop=loop)
    assert hz.table.shape == (1, F, M, 3) and hz.table.dtype == np.float32
    assert (hz.n_scenes, hz.n_frames, hz.max_hazards, hz.frame_steps, hz.loop) == (1, F, M, fs, loop)
    want = {0: 0, fs - 1: 0, fs: 1, 2 * fs - 1: 1, 2 * fs: 2, F * fs - 1: F - 1, F * fs: 0 if loop else F - 1,
            F * fs + fs: 1 if loop else F - 1, 1000 * F * fs + fs + 1: 1 if loop else F - 1}
    for g, f in want.items():
        assert hz.frame_index(g) == f, (g, f)
        rows = hz.rows(0, g)
        assert rows.dtype == np.float64 and rows.shape == (M, 3)
        assert np.array_equal(rows[:, :2], loc[f].astype(np.float32)) and np.array_equal(rows[:, 2], size[0, f].astype(np.float32))
    assert np.array_equal(hz.rows(), hz.rows(0, 0))
    with pytest.raises(ValueError):
        hz.frame_index(-1)


def test_scenes_counts_and_size_shapes():
    S, F, M = 3, 2, 4
    loc = _frames(F, M, S)
    hz = MovingHazards(loc, np.arange(S * M).reshape(S, M) / 10.0, frame_steps=2, counts=[4, 2, 0], scene=[2, 0, 1, 1])
    assert hz.table.shape == (S, F, M, 3)
    assert hz.rows(0, 3).shape == (0, 3) and hz.rows(2, 0).shape == (2, 3) and hz.rows(1, 5).shape == (4, 3)
    assert np.array_equal(hz.rows(3, 2)[:, :2], loc[1, 1, :2].astype(np.float32))      # robot 3: scene 1, step 2: frame 1
    assert np.array_equal(hz.rows(3, 2)[:, 2], np.float32([0.4, 0.5]))                   # [S, M] sizes: the same in every frame
    for size in (0.25, np.full(M, 0.25), np.full((S, M), 0.25), np.full((S, F, M), 0.25)):
        assert np.all(MovingHazards(loc, size, scene=[0, 1, 2]).table[..., 2] == 0.25)
    hz.check_robots(4)
    with pytest.raises(ValueError):
        hz.check_robots(5)
    one = MovingHazards(loc[0])                                                       # [F, M, 2]: one scene
    assert one.table.shape == (1, F, M, 3) and one.scene is None and np.array_equal(one.counts, [M])


@pytest.mark.parametrize("kwargs", [
    dict(locations=np.zeros((4, 2))),                                         # no time axis
    dict(locations=np.zeros((2, 4, 3))),                                      # not [..., 2]
    dict(locations=np.zeros((0, 4, 2))),                                      # F = 0
    dict(locations=np.zeros((0, 2, 4, 2))),                                   # S = 0
    dict(locations=np.zeros((1, 1025, 2))),                                   # M > 1024
    dict(locations=np.zeros((2, 3, 2)), frame_steps=0),
    dict(locations=np.zeros((2, 3, 2)), frame_steps=-1),
    dict(locations=np.zeros((2, 3, 2)), frame_steps=2.5),
    dict(locations=np.zeros((2, 3, 2)), frame_steps=2 ** 31),
    dict(locations=np.full((2, 3, 2), np.nan)),
    dict(locations=np.zeros((2, 3, 2)), size=np.inf),
    dict(locations=np.zeros((2, 3, 2)), size=-0.1),
    dict(locations=np.zeros((2, 3, 2)), size=np.zeros(4)),                    # size of the wrong length
    dict(locations=np.zeros((2, 3, 2)), size=np.zeros((2, 2, 3))),            # S = 1 here: [S, F, M] is [1, 2, 3]
    dict(locations=np.zeros((2, 3, 2)), cost=-1.0),
    dict(locations=np.zeros((2, 3, 2)), cost=np.nan),
    dict(locations=np.zeros((2, 3, 2)), counts=[4]),                          # count > M
    dict(locations=np.zeros((2, 3, 2)), counts=[-1]),
    dict(locations=np.zeros((2, 3, 2)), counts=[[3, 3]]),                     # counts are per scene, not per frame
    dict(locations=np.zeros((2, 2, 3, 2))),                                   # S > 1 without scene
    dict(locations=np.zeros((2, 2, 3, 2)), scene=[0, 2]),
    dict(locations=np.zeros((2, 2, 3, 2)), scene=[0.5, 1.0]),
])
def test_moving_hazards_validation(kwargs):
    with pytest.raises(ValueError):
        MovingHazards(**kwargs)


def test_the_byte_cap_is_stated_and_checked_before_anything_is_built():
    assert rules.HAZARD_FRAMES_MAX_BYTES == 64 << 20
    F = rules.HAZARD_FRAMES_MAX_BYTES // (1024 * 12) + 1                      # one frame too many at M = 1024
    loc = np.broadcast_to(np.zeros(2), (F, 1024, 2))                          # a view: nothing of that size exists
    with pytest.raises(ValueError, match=r"cap of 67108864 bytes \(64 MiB\)"):
        MovingHazards(loc)


def test_circling_is_the_reference_gremlin_motion():
    """offset = travel * (sin phi, cos phi) at the frame's simulation time phi.  The fixture holds float64 values the reference's
    own set_mocaps produced; circling_offsets makes the same NumPy calls on the same float64 inputs, so equality is expected to be
    exact on a libm that agrees with the one the fixture was made on.  The bound asserted is what float64 allows if it does not:
    sin and cos of vendor libraries stay within 4 ulp (|value| <= 1, so 4 eps), times travel, plus one rounding of the
    product (eps / 2 * travel): 4.5 eps * travel with eps = finfo(fixture dtype).eps."""
    z = np.load(GOLDEN)
    assert z["offset"].dtype == np.float64 and np.all(z["same_for_all"])
    eps = np.finfo(z["offset"].dtype).eps
    C, F = z["time"].shape
    assert C >= 4 and F >= 8
    worst = 0.0
    for c in range(C):
        p0, dt, travel, size = (float(z[k][c]) for k in ("phase0", "dt", "travel", "size"))
        off = MovingHazards.circling_offsets(travel, F, dt, p0)
        worst = max(worst, float(np.max(np.abs(off - z["offset"][c])) / travel))
        assert np.all(np.abs(off - z["offset"][c]) <= 4.5 * eps * travel), c
        # the frames: centre + offset in float64, stored as float32; radius = size in every frame
        centres = np.random.default_rng(c).uniform(-2, 2, (3, 2))
        hz = MovingHazards.circling(centres, travel, size, F, dt, p0, frame_steps=2, loop=True)
        assert hz.table.shape == (1, F, 3, 3) and hz.frame_steps == 2 and hz.loop
        assert np.array_equal(hz.table[0, :, :, :2], (centres[None] + off[:, None]).astype(np.float32))
        assert np.all(hz.table[..., 2] == np.float32(size))
    print(f"circling: largest |offset - fixture| / travel = {worst:.3e} (0 = exact)")
    multi = MovingHazards.circling(np.zeros((2, 3, 2)), n_frames=4, scene=[0, 1])
    assert multi.table.shape == (2, 4, 3, 3)
    # a full turn in F frames comes back to the start (up to float32 of a float64 sum)
    turn = MovingHazards.circling(np.zeros((1, 2)), 1.0, 0.1, 9, 2 * np.pi / 8)
    assert np.allclose(turn.table[0, 8], turn.table[0, 0], atol=1e-6) and np.allclose(turn.table[0, 0, 0, :2], [0.0, 1.0])
    with pytest.raises(ValueError):
        MovingHazards.circling(np.zeros((3,)), n_frames=4)
    with pytest.raises(ValueError):
        MovingHazards.circling(np.zeros((3, 2)), n_frames=0)


class _Wander:
    """predict = towards the goal plus a term in the observation's noise features (the action depends on the step's noise)."""

    def __init__(self):
        self.A = np.linalg.pinv(get_env("point").env._mix)

    def predict(self, obs, deterministic=True):
        o = np.asarray(obs, np.float64)
        return np.clip(self.A @ o[:2] + 0.3 * o[6:6 + self.A.shape[0]], -1.0, 1.0), None


def _recording_env():
    """point's EnvWrapper (no time limit) whose step also logs the float64 position after the step"""
    from mobrob_amd.envs.wrapper import TimeLimit
    env = get_env("point", terminate_on_goal=False)
    while isinstance(env, TimeLimit):
        env = env.env
    log, step = [], env.step

    def logged(a):
        out = step(a)
        log.append(np.asarray(env.get_pos(), np.float64)[:2].copy())
        return out
    env.step = logged
    return env, log


def _job():
    """3 robots walking across hazards that circle around points on their way, 5 and (scene 1) 3 of them, 3 frames of 7 steps"""
    starts = np.array([[-1.0, -1.0], [1.0, -1.0], [0.0, 1.2]])
    wp = np.array([[[1.0, 1.0], [-1.0, 1.0]], [[-1.0, 1.0], [1.0, 1.0]], [[0.0, -1.2], [1.0, 0.0]]])
    centres = np.array([[[-0.5, -0.5], [0.0, 0.0], [0.6, 0.6], [0.5, -0.5], [0.0, 0.8]],
                        [[0.0, 0.6], [0.0, 0.0], [0.0, -0.6], [9.0, 9.0], [9.0, 9.0]]])
    return starts, wp, centres


@pytest.mark.parametrize("loop,fs", [(False, 7), (True, 4)], ids=["hold7", "loop4"])
@pytest.mark.parametrize("indicator", [False, True], ids=["shaped", "indicator"])
def test_host_follow_with_frames_equals_a_hand_loop_and_splits(loop, fs, indicator):
    starts, wp, centres = _job()
    hz = MovingHazards.circling(centres, 0.3, 0.35, 3, 0.8, frame_steps=fs, loop=loop, cost=1.5, indicator=indicator,
                                counts=[5, 3], scene=[0, 1, 0])
    pol, T = _Wander(), 40
    env, log = _recording_env()
    one = follow_waypoints(pol, env, starts, wp, max_steps=T, seed=5, hazards=hz)
    assert np.all(one["steps"] == T) and len(log) == 3 * T
    # hand loop: the float64 position after step g against the rows in force at g, summed in the loop's order: the same numbers
    for i in range(3):
        cost, first, count, clear = 0.0, -1, 0, np.inf
        for g in range(T):
            c, cl = rules.hazard_cost(log[i * T + g], hz.rows(i, g), hz.cost, hz.indicator)
            cost += float(c)
            count += c > 0
            first = g + 1 if c > 0 and first < 0 else first
            clear = min(clear, float(cl))
        assert one["violation_steps"][i] == count and one["first_violation"][i] == first, i
        assert one["cost_sum"][i] == cost and one["min_clearance"][i] == clear, (i, one["cost_sum"][i], cost)
    assert np.any(one["violation_steps"] > 0) and np.all(one["violation_steps"] < T)
    # the frames matter: the first frame held for the whole run gives other sums
    still = rules.Hazards(hz.table[:, 0, :, :2], hz.table[:, 0, :, 2], cost=1.5, indicator=indicator, counts=[5, 3], scene=[0, 1, 0])
    held = follow_waypoints(pol, "point", starts, wp, max_steps=T, seed=5, hazards=still)
    assert not np.array_equal(held["cost_sum"], one["cost_sum"]) and np.array_equal(held["reward_sum"], one["reward_sum"])
    # a run split 13 + 27 (no frame boundary at 13) ends with the carried arrays of one call of 40
    a = follow_waypoints(pol, "point", starts, wp, max_steps=13, seed=5, hazards=hz)
    b = follow_waypoints(pol, "point", max_steps=27, seed=5, hazards=hz, state=a["state"])
    s1, s2 = one["state"], b["state"]
    for k in ("state", "robot", "arrival", "leg_used", "status", "hazard"):
        assert np.array_equal(getattr(s1, k), getattr(s2, k), equal_nan=True), k
    assert s2.step0 == T
    for k in ("cost_sum", "violation_steps", "first_violation", "min_clearance"):
        assert np.array_equal(one[k], b[k]), k


def test_one_frame_is_the_static_scene_on_the_host():
    starts, wp, centres = _job()
    mv = MovingHazards(centres[0][None], 0.35, frame_steps=3, indicator=False)
    st = rules.Hazards(centres[0], 0.35, indicator=False)
    a = follow_waypoints(_Wander(), "point", starts, wp, max_steps=30, seed=2, hazards=mv)
    b = follow_waypoints(_Wander(), "point", starts, wp, max_steps=30, seed=2, hazards=st)
    for k in ("cost_sum", "violation_steps", "first_violation", "min_clearance", "reward_sum", "arrival"):
        assert np.array_equal(a[k], b[k]), k
    assert np.any(a["cost_sum"] > 0)


def test_frames_struct_layout_and_symbols(tmp_path):
    from mobrob_amd import _lib
    names = [n for n, _ in _lib.HazardFramesC._fields_]
    assert names == [n for n, _ in _lib.HazardsC._fields_] + ["n_frames", "frame_steps", "loop"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "mobrob_ppo.h"\nint main(void) {\n'
            '  printf("%zu\\n", sizeof(mobrob_hazard_frames_t));\n'
            + "".join(f'  printf("%zu\\n", offsetof(mobrob_hazard_frames_t, {n}));\n' for n in names)
            + '  printf("%zu\\n", (size_t)MOBROB_HAZARD_FRAMES_MAX_BYTES);\n  return 0;\n}\n')
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_lib.HazardFramesC) == 56
    assert out[1:-1] == [getattr(_lib.HazardFramesC, n).offset for n in names]
    assert out[-1] == rules.HAZARD_FRAMES_MAX_BYTES
    # the static struct is a prefix: same offsets
    assert all(getattr(_lib.HazardFramesC, n).offset == getattr(_lib.HazardsC, n).offset for n, _ in _lib.HazardsC._fields_)
    import __graft_entry__
    __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ("mobrob_ppo_evaluate_goal_env_hazard_frames", "mobrob_ppo_follow_waypoints_hazard_frames"):
        assert hasattr(lib, sym) and sym in _lib.SYMBOLS, sym
    assert len(_lib.SYMBOLS["mobrob_ppo_follow_waypoints_hazard_frames"][1]) == 13
    assert lib.mobrob_ppo_abi_version() == _lib.ABI_VERSION == 3


def test_cli_reads_frames(capsys, tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("follow_cli", os.path.join(ROOT, "examples", "follow.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    fr = MovingHazards.circling([[0.5, 0.5], [-0.5, 0.5]], 0.3, 0.3, 6, 0.6).table[0]          # [F][M][3]
    sq = np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 1.0]])
    cli.follow("point", "ppo", sq, 4, max_steps=60, host=True, seed=3, policy=_Wander(), hazard_frames=fr, frame_steps=5, hazard_loop=True)
    single = capsys.readouterr().out
    cli.follow("point", "ppo", sq, 4, max_steps=60, host=True, seed=3, policy=_Wander(), hazard_frames=fr, frame_steps=5, hazard_loop=True,
               horizon=17)
    assert capsys.readouterr().out == single and "mean hazard cost: " in single
    with pytest.raises(ValueError):
        cli.follow("point", "ppo", sq, 4, max_steps=60, host=True, policy=_Wander(), hazard_frames=fr[:, :, :2])
