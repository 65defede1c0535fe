"""GPU: run specifications on the device (k_spec_monitor through PPOEngine.spec_monitor and follow_waypoints(..., spec=)) against the
NumPy rule, bit for bit: integer views throughout, so -0.0 against +0.0 counts as different."""
import ctypes as C
import re

import numpy as np
import pytest

from mobrob_amd import _lib
from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import Regions, Spec, inside, outside, spec_fold, spec_result, spec_start
from mobrob_amd.waypoints import follow_waypoints, follow_with_replanning, monitor
from tests.util import _engine, _env, _go_to_goal_params, persistent_env  # noqa: F401

gpu = pytest.mark.gpu
INF = np.float32(np.inf)


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == bool else a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint64)


def assert_same_state(got, want, why=""):
    assert np.array_equal(bits(got.val), bits(want.val)), why
    assert np.array_equal(got.wit, want.wit), why


def assert_same_result(got, want, why=""):
    assert set(got) == set(want) == set(R.SPEC_RESULT_KEYS)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(bits(got[k]), bits(want[k])), (why, k)


# ---- the synthetic case: stated without a device, so its own conditions can be checked anywhere ---------------------------------------
ROWS = np.array([[0.0, 0.0, 0.5, 0.5], [2.0, 0.0, 0.5, 0.0], [0.0, 2.0, 0.0, 0.0], [2.0, 2.0, 0.0, 0.0], [-2.0, 0.0, 0.625, 0.625],
                 [-2.0, -2.0, 0.5, 0.0]], np.float32)    # box, circle, zero-size box, zero-radius circle, box, circle
KINDS = np.array([0, 1, 0, 1, 0, 1], np.int32)


def synthetic_spec(n, T, shared):
    if shared:
        reg = Regions(ROWS, KINDS)
    else:           # three scenes with unequal counts, one without regions; scene 1 is scene 0 moved a little
        reg = Regions(np.stack([ROWS, ROWS + np.float32([0.25, 0.0, 0.0, 0.0]), ROWS]), KINDS, counts=[6, 4, 0], scene=np.arange(n) % 3)
    return Spec(reg, [Spec.always(outside(2, 4)),                            # a union of the two zero-size regions, avoided
                      Spec.eventually(inside(0, 2), 0, T),                   # a union, reached
                      Spec.until(outside(4), inside(5)),                     # both signs, open window
                      Spec.always(inside(4), 0, min(2, T)),
                      Spec.eventually(outside(5), T, T)])                    # a == b


def synthetic_path(n, T, P, seed):
    """Seeded random walks around four kinds of starts (robot i: i % 4 -- inside box 0, inside circle 5, far from everything and
    standing still, inside box 4), every eighth robot standing still, and rows planted on region boundaries."""
    rng = np.random.default_rng(seed)
    starts = np.array([[0.0, 0.0], [-2.0, -2.0], [1.0, -1.5], [-2.0, 0.0]], np.float32)
    path = np.zeros((T + 1, n, P), np.float32)
    step = rng.normal(0.0, 0.03, (T + 1, n, 2)).astype(np.float32)
    step[0] = 0
    still = (np.arange(n) % 4 == 2) | (np.arange(n) % 8 == 0)
    step[:, still] = 0                                                       # equal margins at every pair of samples
    path[:, :, :2] = starts[np.arange(n) % 4][None] + np.cumsum(step, axis=0)
    if P == 3:
        path[:, :, 2] = rng.normal(0.0, 5.0, (T + 1, n))
    mid = (T + 1) // 2
    path[mid, 0, :2] = [0.5, 0.25]                                           # on a face of box 0: margin -0.0
    # (robots 12, 15 and 21 see scene 0 when the scenes are per robot: i % 3 == 0)
    for robot, record, xy in [(5, T, [-2.0, -1.5]), (21, T, [-2.0, -1.5]),   # on circle 5 at the last sample: margin +0.0
                              (12, mid, [0.0, 2.0]),                         # on the zero-size box: margin -0.0
                              (15, T, [2.0, 2.0])]:                          # on the zero-radius circle: margin +0.0
        if robot < n:
            path[record, robot, :2] = xy
    return path


def synthetic_conditions(n, T, spec, want, res):
    """What the test needs of its own case, asserted on the NumPy side before anything is compared."""
    assert np.any(want.wit == 0) and np.any(want.wit == T)
    if n >= 16:
        for c in range(spec.n_clauses):
            assert np.any(res["spec_rho"][:, c] > 0) and np.any(~(res["spec_rho"][:, c] > 0)), c
        assert np.any(res["spec_rho"] == 0)                                  # a planted boundary decided some clause


SHAPES = [(n, T, P) for n in (1, 16, 17, 70) for T in (1, 7, 60) for P in (2, 3)]


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", {})
    yield e
    e.close()


@gpu
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-robot"])
@pytest.mark.parametrize("n,T,P", SHAPES, ids=[f"n{n}-T{T}-P{P}" for n, T, P in SHAPES])
def test_synthetic_paths_bit_for_bit(engine, n, T, P, shared):
    spec = synthetic_spec(n, T, shared)
    path = synthetic_path(n, T, P, seed=100 * n + T)
    want = spec_fold(spec_start(n, spec), path, spec)
    res = spec_result(want, spec)
    synthetic_conditions(n, T, spec, want, res)
    got, got_res = engine.spec_monitor(spec, path)
    assert_same_state(got, want)
    assert_same_result(got_res, res)


def test_the_synthetic_case_meets_its_own_conditions_without_a_device():
    """(not gpu) the NumPy half of the test above at every shape: a case that stops meeting its conditions shows here first"""
    for n, T, P in SHAPES:
        for shared in (True, False):
            spec = synthetic_spec(n, T, shared)
            want = spec_fold(spec_start(n, spec), synthetic_path(n, T, P, seed=100 * n + T), spec)
            synthetic_conditions(n, T, spec, want, spec_result(want, spec))


@gpu
def test_every_two_way_split_on_the_device(engine):
    n, T = 17, 12
    spec = synthetic_spec(n, T, False)
    path = synthetic_path(n, T, 2, seed=5)
    want = spec_fold(spec_start(n, spec), path, spec)
    whole, res = engine.spec_monitor(spec, path)
    assert_same_state(whole, want)
    for cut in range(1, T):
        a, _ = engine.spec_monitor(spec, path[:cut + 1])
        b, res_b = engine.spec_monitor(spec, path[cut:], step0=cut, state=a)
        assert_same_state(b, whole, cut)
        assert_same_result(res_b, res, cut)
        assert_same_state(a, spec_fold(spec_start(n, spec), path[:cut + 1], spec), cut)


def limits_case():
    rng = np.random.default_rng(9)
    Rn, Cn, n, T = R.SPEC_REGIONS_MAX, R.SPEC_CLAUSES_MAX, 70, 7
    rows = np.concatenate([rng.uniform(-2, 2, (Rn, 2)), rng.uniform(0, 0.75, (Rn, 2))], axis=1)
    reg = Regions(rows, rng.integers(0, 2, Rn))
    clauses = []
    for c in range(Cn):
        lo = int(rng.integers(0, Rn))
        p1 = (inside, outside)[c % 2](lo, int(rng.integers(lo, Rn + 1)))
        lo2 = int(rng.integers(0, Rn))
        p2 = (outside, inside)[c % 2](lo2, int(rng.integers(lo2, Rn + 1)))
        a = int(rng.integers(0, T + 1))
        b = None if c % 5 == 0 else int(rng.integers(a, T + 3))
        clauses.append([Spec.always(p1, a, b), Spec.eventually(p1, a, b), Spec.until(p1, p2, a, b)][c % 3])
    clauses[0] = Spec.always(outside(0, Rn))                                 # the whole table as one union
    path = np.cumsum(rng.normal(0, 0.2, (T + 1, n, 2)), axis=0).astype(np.float32)
    return Spec(reg, clauses), path


@gpu
def test_the_limits_sixteen_clauses_over_sixty_four_regions(engine):
    spec, path = limits_case()
    want = spec_fold(spec_start(path.shape[1], spec), path, spec)
    got, res = engine.spec_monitor(spec, path)
    assert_same_state(got, want)
    assert_same_result(res, spec_result(want, spec))
    assert len(np.unique(want.wit)) > 4 and np.any(res["spec_rho"] > 0) and np.any(res["spec_rho"] < 0)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def raw_call(engine, spec, path, step0=0, change=None, n=None, T=None, P=None, null=()):
    """mobrob_ppo_spec_monitor called as a C caller would, with one thing wrong -> (return code, message, state untouched?)"""
    path = np.ascontiguousarray(path, np.float32)
    reg = spec.regions
    i32 = C.POINTER(C.c_int32)
    sp = _lib.SpecC()
    sp.n_scenes, sp.max_regions, sp.n_clauses = reg.n_scenes, reg.max_regions, spec.n_clauses
    kinds, counts = reg.kinds.copy(), reg.counts.copy()
    scene = None if reg.scene is None else reg.scene.copy()
    table = reg.table.copy()
    sp.regions, sp.kinds, sp.n_regions = table.ctypes.data_as(C.POINTER(C.c_float)), kinds.ctypes.data_as(i32), counts.ctypes.data_as(i32)
    sp.scene = None if scene is None else scene.ctypes.data_as(i32)
    for c, (op, a, b, p1, p2) in enumerate(spec.clauses):
        sp.op[c], sp.a[c], sp.b[c] = op, a, b
        sp.lo1[c], sp.hi1[c], sp.out1[c] = p1[0], p1[1], int(p1[2])
        sp.lo2[c], sp.hi2[c], sp.out2[c] = p2[0], p2[1], int(p2[2])
    if change is not None:
        change(sp, table, kinds, counts, scene)
    st = spec_start(path.shape[1], spec)
    before = (st.val.copy(), st.wit.copy())
    fp = C.POINTER(C.c_float)
    args = dict(spec=C.byref(sp), path=path.ctypes.data_as(fp), val=st.val.ctypes.data_as(fp), wit=st.wit.ctypes.data_as(i32))
    for k in null:
        args[k] = None
    rc = engine.lib.mobrob_ppo_spec_monitor(engine._h, args["spec"], args["path"], path.shape[1] if n is None else n,
                                            path.shape[0] - 1 if T is None else T, path.shape[2] if P is None else P, step0,
                                            args["val"], args["wit"])
    msg = engine.lib.mobrob_ppo_last_error().decode()
    untouched = np.array_equal(bits(st.val), bits(before[0])) and np.array_equal(st.wit, before[1])
    return rc, msg, untouched


def _set(field, c, v):
    def change(sp, *_):
        getattr(sp, field)[c] = v
    return change


def _attr(field, v):
    def change(sp, *_):
        setattr(sp, field, v)
    return change


@gpu
def test_refusals_return_the_error_and_launch_nothing(engine):
    n, T = 6, 4
    spec = synthetic_spec(n, T, False)
    path = synthetic_path(n, T, 2, seed=1)
    assert raw_call(engine, spec, path)[0] == _lib.OK                        # the call as it stands is taken

    def table_nan(sp, table, *_):
        table[0, 1, 2] = np.nan

    def kind_two(sp, table, kinds, *_):
        kinds[0, 3] = 2

    def count_over(sp, table, kinds, counts, scene):
        counts[1] = 7

    def scene_over(sp, table, kinds, counts, scene):
        scene[4] = 3

    nan_path = path.copy()
    nan_path[2, 3, 1] = np.inf
    cases = [(dict(null=("path",)), "null path"), (dict(null=("val",)), "null val"), (dict(null=("wit",)), "null wit"),
             (dict(null=("spec",)), "null spec"),
             (dict(n=0), "n must be >= 1"), (dict(T=0), "T must be >= 1"), (dict(P=4), "P must lie in 1 .. 3"), (dict(P=0), "P must lie"),
             (dict(change=_attr("n_clauses", 0)), "n_clauses"), (dict(change=_attr("n_clauses", 17)), "n_clauses"),
             (dict(change=_attr("max_regions", 65)), "max_regions"), (dict(change=_attr("n_scenes", 0)), "n_scenes"),
             (dict(change=count_over), r"n_regions\[1\] = 7"), (dict(change=scene_over), r"scene\[4\] = 3"),
             (dict(change=kind_two), "kind 2"), (dict(change=table_nan), "region 1 of scene 0"),
             (dict(change=_attr("scene", None)), "3 scenes need a scene index"),
             (dict(n=1 << 20, T=100, P=3), "path of .* bytes is above the limit"),
             (dict(step0=-1), "step0 must be >= 0"), (dict(step0=2 ** 31 - 3), "step0 \\+ T"),
             (dict(change=_set("a", 1, 5)), "window of clause 1"), (dict(change=_set("a", 0, -1)), "window of clause 0"),
             (dict(change=_set("op", 2, 3)), r"op\[2\] = 3"),
             (dict(change=_set("hi1", 0, 7)), r"region range \[2, 7\) of clause 0 outside 0 .. 6"),
             (dict(change=_set("lo1", 3, -1)), "region range"), (dict(change=_set("lo2", 2, 7)), "second region range"),
             (dict(change=_set("hi2", 2, 7)), "second region range")]
    for kw, msg in cases:
        rc, got, untouched = raw_call(engine, spec, path, **kw)
        assert rc == _lib.ERR_INVALID and untouched, (kw, got)
        assert re.search(msg, got), (kw, got)
    rc, got, untouched = raw_call(engine, spec, nan_path)
    assert rc == _lib.ERR_INVALID and untouched and "robot 3" in got and "record 2" in got
    with pytest.raises(ValueError, match="robot 3 in record 2"):
        engine.spec_monitor(spec, nan_path)
    with pytest.raises(ValueError, match="robots, clauses"):
        engine.spec_monitor(spec, path, state=spec_start(n + 1, spec))
    with pytest.raises(TypeError, match="Spec"):
        engine.spec_monitor(spec.regions, path)
    assert raw_call(engine, spec, path)[0] == _lib.OK                        # and the engine is as usable as before


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
N, S = 24, 60
CARRIED = ("state", "robot", "arrival", "leg_used", "status", "step0")


def e2e_inputs(P, seed=4):
    rng = np.random.default_rng(seed)
    start = rng.uniform(-1.5, 1.5, (N, P)).astype(np.float32)
    wp = rng.uniform(-1.5, 1.5, (N, 3, P)).astype(np.float32)
    return start, wp


def e2e_spec(plain):
    """From the call's own spec-free run: a circle of radius 0.1 around robot 0's final position and a box across robot 1's path, so
    that at least one robot satisfies and at least one violates each clause."""
    path = plain["path"]
    end0, mid1 = path[-1, 0, :2], path[S // 2, 1, :2]
    reg = Regions([[end0[0], end0[1], 0.1, 0.0], [mid1[0], mid1[1], 0.05, 0.05]], [1, 0])
    return Spec(reg, [Spec.eventually(inside(0), S // 2, S), Spec.always(outside(1)), Spec.until(outside(1), inside(0))])


def assert_same_call(a, b, why=""):
    """every key of the call without spec=, bit for bit (the FollowState by its carried arrays)"""
    for k in a:
        if k == "state":
            for f in CARRIED:
                x, y = getattr(a[k], f), getattr(b[k], f)
                assert np.array_equal(bits(np.asarray(x)), bits(np.asarray(y))), (why, k, f)
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (why, k)
        else:
            assert a[k] == b[k], (why, k)


def e2e(robot, kw=None, tile256=False):
    e, _ = _engine(robot, kw or {})
    env = _env(robot, N)
    _go_to_goal_params(e, env)
    if tile256:
        e.set_eval_tile256(True)
    P = env.pos_dim
    start, wp = e2e_inputs(P)
    run = dict(max_steps=S, seed=3, path_stride=1)
    plain = follow_waypoints(e, env, start, wp, **run)
    spec = e2e_spec(plain)
    r = follow_waypoints(e, env, start, wp, spec=spec, **run)
    assert set(r) - set(plain) == set(R.SPEC_RESULT_KEYS) and r["persistent"] == plain["persistent"]
    assert_same_call(plain, r, robot)
    want = spec_fold(spec_start(N, spec), r["path"], spec)
    assert_same_state(r["state"].spec, want)
    assert_same_result({k: r[k] for k in R.SPEC_RESULT_KEYS}, spec_result(want, spec))
    for c in range(spec.n_clauses):                                          # by construction: robot 0 reaches, robot 1 crosses
        assert np.any(r["spec_rho"][:, c] > 0) and np.any(~(r["spec_rho"][:, c] > 0)), c
    assert r["spec_rho"][0, 0] > 0 and r["spec_rho"][1, 1] < 0
    # one call of 60 steps equals three of 20 through `state`
    c = follow_waypoints(e, env, start, wp, spec=spec, **dict(run, max_steps=S // 3))
    for _ in range(2):
        c = follow_waypoints(e, env, spec=spec, state=c["state"], **dict(run, max_steps=S // 3))
    assert_same_state(c["state"].spec, want)
    assert_same_result({k: c[k] for k in R.SPEC_RESULT_KEYS}, spec_result(want, spec))
    # ... and the device fold equals the rule through monitor() either way
    assert_same_state(monitor(r["path"], spec, engine=e)[0], monitor(r["path"], spec)[0])
    return e, env, start, wp, spec, want, r


@gpu
@pytest.mark.parametrize("robot", ["point", "drone"])
def test_end_to_end_on_fused_engines(robot, persistent_env):
    persistent_env(None)
    e, env, start, wp, spec, want, r = e2e(robot)
    assert r["path"].shape == (S + 1, N, env.pos_dim)
    e.close()


@gpu
def test_end_to_end_through_follow_with_replanning(persistent_env):
    persistent_env(None)
    e, env, start, wp, spec, want, r = e2e("point")
    rr = follow_with_replanning(e, env, start, wp, lambda *a: {}, horizon=S // 3, rounds=3, seed=3, spec=spec, path_stride=1)
    assert_same_state(rr["state"].spec, want)
    assert_same_result({k: rr[k] for k in R.SPEC_RESULT_KEYS}, spec_result(want, spec))
    with pytest.raises(ValueError, match="spec=.*path_stride=1"):
        follow_waypoints(e, env, start, wp, max_steps=S, seed=3, path_stride=2, spec=spec)
    with pytest.raises(ValueError, match="spec=.*path_stride=1"):
        follow_with_replanning(e, env, start, wp, lambda *a: {}, horizon=S // 3, rounds=3, seed=3, spec=spec)
    e.close()


@gpu
def test_end_to_end_on_the_256_wide_tile(persistent_env):
    persistent_env(None)
    e, env, start, wp, spec, want, r = e2e("point", dict(pi=(256, 256), vf=(256, 256)), tile256=True)
    assert r["persistent"] is True                                           # the monitor does not care which tile ran
    e.close()


@gpu
def test_training_is_bit_identical_with_monitor_calls_in_between():
    spec, path = limits_case()
    params = []
    for with_monitor in (False, True):
        e, _ = _engine("point", {}, n_envs=16, seed=7)
        e.collect_synthetic()
        e.train(None)
        if with_monitor:
            st, _ = e.spec_monitor(spec, path)
            e.spec_monitor(spec, path[3:], step0=3, state=st)
        e.collect_synthetic()
        e.train(None)
        m, v, step = e.get_optimizer_state()
        params.append((e.get_flat_params().copy(), e.flatten(m).copy(), e.flatten(v).copy(), step))
        e.close()
    for a, b in zip(*params):
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))
