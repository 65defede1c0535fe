"""GPU: run specifications over things that move on the device (k_spec_monitor_moving through PPOEngine.spec_monitor and
follow_waypoints(..., spec=)) against the NumPy rule, bit for bit on val, wit, tail and the five result keys."""
import ctypes as C
import re

import numpy as np
import pytest

from mobrob_amd import _lib
from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import (MovingHazards, MovingRegions, Regions, Spec, Teams, apart, inside, outside, spec_fold, spec_result,
                                        spec_start, together)
from mobrob_amd.waypoints import follow_waypoints, monitor
from tests.test_spec_gpu import KINDS, ROWS, synthetic_path
from tests.test_spec_moving_cpu import split_case
from tests.test_spec_nested_cpu import assert_every_split_equals_the_whole, assert_same_result, assert_same_state, bits
from tests.test_spec_nested_gpu import _Counting, _attr, _set
from tests.util import _engine, _env, _go_to_goal_params, persistent_env  # noqa: F401

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", {})
    yield e
    e.close()


def regions(n, F, frame_steps, loop, shared, seed=0):
    """the synthetic scene of tests/test_spec_gpu.py, every region displaced anew in every frame; per robot: three scenes with
    unequal counts, one without regions"""
    rng = np.random.default_rng(seed)
    S = 1 if shared else 3
    t = np.tile(ROWS, (S, F, 1, 1))
    t[..., :2] += rng.normal(0.0, 0.1, (S, F, 6, 2)).astype(np.float32)
    t[:, 0] = ROWS                                                           # frame 0: the rows themselves, boundaries included
    if shared:
        return MovingRegions(t[0], KINDS, frame_steps=frame_steps, loop=loop)
    return MovingRegions(t, KINDS, frame_steps=frame_steps, loop=loop, counts=[6, 4, 0], scene=np.arange(n) % 3)


def mate_distances(size):
    """the synthetic path starts robot i at one of four places by i % 4, 2 .. 3.6 apart; mates of the same place are a few
    hundredths apart"""
    return (2.9, 3.2, 0.1) if size <= 4 else (0.1, 3.5, 0.05)


def case_spec(n, T, size, reg):
    d0, d1, d2 = mate_distances(size)
    return Spec(reg, [Spec.always(outside(2, 4)), Spec.eventually(inside(0, 2), 0, T), Spec.until(outside(4), inside(5)),
                      Spec.stay(inside(0, 2), 3), Spec.recur(outside(5), 5, 0, max(T - 5, 0)),
                      Spec.always(apart(d0), 1), Spec.eventually(together(d1), 0, T), Spec.until(apart(d2), inside(0, 2)),
                      Spec.stay(together(d1), 2, min(1, T)), Spec.recur(apart(d0), 6), Spec.until(inside(4), together(d1), 0, T // 2)],
                team_size=size)


# (n, team size, T, P, F, frame_steps, loop, shared, step0): every value of every axis at least once
CASES = [(1, 1, 1, 2, 1, 1, False, True, 0), (16, 16, 7, 3, 3, 7, True, True, 0), (48, 4, 60, 2, 5, 1, False, True, 5),
         (70, 2, 60, 3, 3, 7, False, False, 0), (70, 1, 7, 2, 5, 1, True, False, 5), (80, 16, 60, 2, 3, 7, False, False, 0),
         (80, 16, 60, 3, 5, 7, True, True, 5), (48, 4, 1, 3, 3, 1, True, False, 0), (70, 2, 60, 2, 5, 1, True, True, 0),
         (16, 16, 60, 2, 1, 7, True, False, 5), (1, 1, 60, 3, 5, 7, False, True, 0), (70, 1, 60, 2, 3, 1, False, False, 0),
         (48, 4, 7, 2, 5, 7, False, True, 0), (80, 16, 1, 2, 1, 1, False, True, 5)]


@gpu
@pytest.mark.parametrize("n,size,T,P,F,frame_steps,loop,shared,step0", CASES, ids=["-".join(str(int(v)) for v in c) for c in CASES])
def test_bit_for_bit_against_the_rule(engine, n, size, T, P, F, frame_steps, loop, shared, step0):
    path = synthetic_path(n, T, P, seed=100 * n + T)
    spec = case_spec(n, T, size, regions(n, F, frame_steps, loop, shared, seed=n + F))
    assert spec.dynamic and spec.nested
    want = spec_fold(spec_start(n, spec), path, spec, step0)
    got, res = engine.spec_monitor(spec, path, step0=step0)
    assert_same_state(got, want)
    assert_same_result(res, spec_result(want, spec))
    if T == 60 and n >= 16:                                                  # the case is not idle: both verdicts, for regions and mates
        rho = want.val[:, :, 0]
        for cols in ([0, 1, 2, 3, 4], [5, 6, 7, 8, 9]) if size > 1 else ([0, 1, 2, 3, 4],):
            v = rho[:, cols]
            assert np.any(np.isfinite(v) & (v > 0)) and np.any(np.isfinite(v) & (v < 0)), cols
    if size == 1:
        assert np.all(want.val[:, [5, 9], 0] == np.inf)


def mixed_spec(n, shared):
    """sixteen clauses: region and mate predicates, flat and nested with h in {0, 5, 60}, an until with a mate guard"""
    cl = [Spec.always(outside(2, 4)), Spec.always(apart(2.9), 1), Spec.eventually(inside(0, 2), 0, 50), Spec.eventually(together(3.2)),
          Spec.until(apart(0.1), inside(5)), Spec.until(outside(4), together(3.0), 2, 40), Spec.until(apart(2.5), apart(3.0)),
          Spec.stay(inside(0, 2), 0), Spec.stay(together(3.2), 0, 3), Spec.stay(inside(4, 6), 5), Spec.stay(apart(2.9), 5, 0, 30),
          Spec.stay(outside(0, 6), 60), Spec.stay(together(3.4), 60), Spec.recur(outside(5), 5), Spec.recur(together(3.1), 60),
          Spec.recur(apart(2.0), 0, 7)]
    return Spec(regions(n, 3, 7, True, shared, seed=5), cl, team_size=4)


@gpu
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-robot"])
def test_sixteen_mixed_clauses(engine, shared):
    n, T = 72, 60
    spec = mixed_spec(n, shared)
    assert spec.n_clauses == 16 and {cl[0] for cl in spec.clauses} == {0, 1, 2, 3, 4} and set(spec.holds) == {0, 5, 60}
    path = synthetic_path(n, T, 2, seed=21)
    want = spec_fold(spec_start(n, spec), path, spec)
    got, res = engine.spec_monitor(spec, path)
    assert_same_state(got, want)
    assert_same_result(res, spec_result(want, spec))
    assert len(np.unique(want.wit)) > 4 and np.any(res["spec_rho"] > 0) and np.any(np.isfinite(res["spec_rho"]) & (res["spec_rho"] < 0))


@gpu
def test_the_slot_cap_with_moving_regions_whole_and_in_three_calls(engine):
    """two holds of 255: 512 slots, the largest LDS block, with region frames and a mate clause"""
    n, T = 72, 300
    spec = Spec(regions(n, 5, 7, True, False, seed=9), [Spec.stay(inside(0, 2), 255), Spec.always(apart(2.9)),
                                                         Spec.recur(together(3.3), 255, 10, None), Spec.always(outside(2, 4))], team_size=4)
    assert sum(h + 1 for h in spec.holds if h) == R.SPEC_WINDOW_SLOTS
    path = synthetic_path(n, T, 2, seed=33)
    want = spec_fold(spec_start(n, spec), path, spec)
    got, res = engine.spec_monitor(spec, path)
    assert_same_state(got, want)
    assert_same_result(res, spec_result(want, spec))
    assert np.any(np.isfinite(want.val[:, [0, 2], 0])) and len(np.unique(want.wit[:, [0, 2]])) > 2
    st = None
    for k in range(3):
        st, res3 = engine.spec_monitor(spec, path[100 * k:100 * k + 101], step0=100 * k, state=st)
    assert_same_state(st, want)
    assert_same_result(res3, res)


@gpu
@pytest.mark.parametrize("frame_steps,loop", [(1, False), (4, True), (7, False), (7, True)])
def test_every_split_of_twelve_steps_on_the_device(engine, frame_steps, loop):
    spec, path = split_case(frame_steps, loop, n=20)
    n = path.shape[1]
    whole = assert_every_split_equals_the_whole(lambda p, step0, st: engine.spec_monitor(spec, p, step0=step0, state=st)[0], spec, path)
    assert_same_state(whole, spec_fold(spec_start(n, spec), path, spec))


@gpu
def test_one_frame_and_no_mates_equal_the_static_kernels(engine):
    n, T = 70, 60
    path = synthetic_path(n, T, 3, seed=8)
    cl = [Spec.always(outside(2, 4)), Spec.eventually(inside(0, 2), 0, T), Spec.until(outside(4), inside(5)), Spec.stay(inside(0, 2), 4)]
    static = Regions(np.stack([ROWS, ROWS + np.float32([0.25, 0, 0, 0]), ROWS]), KINDS, counts=[6, 4, 0], scene=np.arange(n) % 3)
    one = MovingRegions(static.table[:, None], KINDS, frame_steps=7, loop=True, counts=[6, 4, 0], scene=np.arange(n) % 3)
    a, ra = engine.spec_monitor(Spec(static, cl), path)
    b, rb = engine.spec_monitor(Spec(one, cl), path)
    assert_same_state(a, b)
    assert_same_result(ra, rb)


@gpu
def test_a_static_specification_still_takes_the_entry_point_it_took(engine):
    n, T = 16, 7
    path = synthetic_path(n, T, 2, seed=2)
    static = Regions(ROWS, KINDS)
    flat = Spec(static, [Spec.always(outside(2, 4)), Spec.eventually(inside(0, 2))])
    nested = Spec(static, [Spec.always(outside(2, 4)), Spec.stay(inside(0, 2), 0)])
    moving = Spec(regions(n, 1, 1, False, True), flat.clauses)
    mates = Spec(static, flat.clauses + (Spec.always(apart(0.1)),), team_size=4)
    assert not flat.dynamic and not nested.dynamic and moving.dynamic and mates.dynamic
    lib = engine.lib
    engine.lib = counting = _Counting(lib)
    try:
        a, _ = engine.spec_monitor(flat, path)
        assert counting.calls == {"mobrob_ppo_spec_monitor": 1}
        engine.spec_monitor(nested, path)
        assert counting.calls == {"mobrob_ppo_spec_monitor": 1, "mobrob_ppo_spec_monitor_nested": 1}
        b, _ = engine.spec_monitor(moving, path)
        c, _ = engine.spec_monitor(mates, path)
        assert counting.calls == {"mobrob_ppo_spec_monitor": 1, "mobrob_ppo_spec_monitor_nested": 1, "mobrob_ppo_spec_monitor_moving": 2}
    finally:
        engine.lib = lib
    assert np.array_equal(bits(a.val), bits(b.val)) and np.array_equal(a.wit, b.wit)       # frame 0 of `regions` is ROWS
    assert np.array_equal(bits(a.val), bits(c.val[:, :2])) and np.array_equal(a.wit, c.wit[:, :2])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def raw_call(engine, spec, path, step0=0, change=None, n=None, T=None, P=None, W=None, null=()):
    """mobrob_ppo_spec_monitor_moving called as a C caller would, with one thing wrong -> (return code, message, state untouched?)"""
    path = np.ascontiguousarray(path, np.float32)
    reg = spec.regions
    i32, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    sp = _lib.SpecMovingC()
    sp.n_scenes, sp.max_regions, sp.n_clauses = reg.n_scenes, reg.max_regions, spec.n_clauses
    kinds, counts, table = reg.kinds.copy(), reg.counts.copy(), reg.table.copy()
    scene = None if reg.scene is None else reg.scene.copy()
    sp.regions, sp.kinds, sp.n_regions = table.ctypes.data_as(fp), kinds.ctypes.data_as(i32), counts.ctypes.data_as(i32)
    sp.scene = None if scene is None else scene.ctypes.data_as(i32)
    for c, cl in enumerate(spec.clauses):
        op, a, b = cl[:3]
        w1, w2 = R.spec_predicate_words(cl[3]), R.spec_predicate_words(cl[4])
        sp.op[c], sp.a[c], sp.b[c], sp.hold[c] = op, a, b, spec.holds[c]
        sp.lo1[c], sp.hi1[c], sp.out1[c], sp.kind1[c], sp.rad1[c] = w1
        sp.lo2[c], sp.hi2[c], sp.out2[c], sp.kind2[c], sp.rad2[c] = w2
    sp.team_size, sp.n_frames, sp.frame_steps, sp.loop = spec.team_size, reg.n_frames, reg.frame_steps, int(reg.loop)
    if change is not None:
        change(sp, table, kinds, counts, scene)
    st = spec_start(path.shape[1], spec)
    before = st.copy()
    args = dict(spec=C.byref(sp), path=path.ctypes.data_as(fp), val=st.val.ctypes.data_as(fp), wit=st.wit.ctypes.data_as(i32),
                tail=st.tail.ctypes.data_as(fp))
    for k in null:
        args[k] = None
    rc = engine.lib.mobrob_ppo_spec_monitor_moving(engine._h, args["spec"], args["path"], path.shape[1] if n is None else n,
                                                   path.shape[0] - 1 if T is None else T, path.shape[2] if P is None else P, step0,
                                                   args["val"], args["wit"], args["tail"], spec.tail_width if W is None else W)
    msg = engine.lib.mobrob_ppo_last_error().decode()
    untouched = (np.array_equal(bits(st.val), bits(before.val)) and np.array_equal(st.wit, before.wit)
                 and np.array_equal(bits(st.tail), bits(before.tail)))
    return rc, msg, untouched


@gpu
def test_refusals_of_the_moving_entry_point(engine):
    n, T = 8, 4
    spec = Spec(regions(n, 3, 2, True, False), [Spec.always(outside(2, 4)), Spec.stay(inside(0, 2), 3), Spec.until(apart(0.1), inside(5)),
                                                Spec.recur(together(3.0), 250), Spec.eventually(outside(5), T, T)], team_size=4)
    path = synthetic_path(n, T, 2, seed=1)
    assert raw_call(engine, spec, path)[0] == _lib.OK                        # the call as it stands is taken

    def frame_nan(sp, table, *_):
        table[0, 2, 1, 2] = np.nan

    def frame_negative(sp, table, *_):
        table[1, 1, 0, 3] = -1.0                                             # a box's half extent, in the second frame

    def kind_two(sp, table, kinds, *_):
        kinds[0, 3] = 2

    def count_over(sp, table, kinds, counts, scene):
        counts[1] = 7

    def scene_over(sp, table, kinds, counts, scene):
        scene[4] = 3

    def cap(sp, *_):
        sp.op[0], sp.hold[0], sp.hold[1] = R.SPEC_STAY, 255, 5

    nan_path = path.copy()
    nan_path[2, 3, 1] = np.inf
    who = "^spec_monitor_moving: "
    cases = [  # everything the nested call refuses
             (dict(null=("path",)), "null path"), (dict(null=("val",)), "null val"), (dict(null=("wit",)), "null wit"),
             (dict(null=("spec",)), "null spec"), (dict(null=("tail",)), "null tail with W = 253"),
             (dict(n=0), "n must be >= 1"), (dict(T=0), "T must be >= 1"), (dict(P=4), "P must lie in 1 .. 3"), (dict(P=0), "P must lie"),
             (dict(change=_attr("n_clauses", 0)), "n_clauses"), (dict(change=_attr("n_clauses", 17)), "n_clauses"),
             (dict(change=_attr("max_regions", 65)), "max_regions"), (dict(change=_attr("n_scenes", 0)), "n_scenes"),
             (dict(change=count_over), r"n_regions\[1\] = 7"), (dict(change=scene_over), r"scene\[4\] = 3"),
             (dict(change=kind_two), "kind 2"), (dict(change=_attr("scene", None)), "3 scenes need a scene index"),
             (dict(n=1 << 20, T=100, P=3), "path of .* bytes is above the limit"),
             (dict(step0=-1), "step0 must be >= 0"), (dict(step0=2 ** 31 - 3), "step0 \\+ T"),
             (dict(change=_set("a", 4, 5)), "window of clause 4"), (dict(change=_set("a", 0, -1)), "window of clause 0"),
             (dict(change=_set("op", 2, 5)), r"op\[2\] = 5 outside 0 .. 4"), (dict(change=_set("op", 2, -1)), r"op\[2\] = -1"),
             (dict(change=_set("hi1", 0, 7)), r"region range \[2, 7\) of clause 0 outside 0 .. 6"),
             (dict(change=_set("lo1", 3, -1)), "region range"), (dict(change=_set("lo2", 2, 7)), "second region range"),
             (dict(change=_set("hi2", 2, 7)), "second region range"),
             (dict(change=_set("hold", 1, 256)), r"hold\[1\] = 256 outside 0 .. 255"), (dict(change=_set("hold", 3, -1)), r"hold\[3\] = -1"),
             (dict(change=_set("hold", 0, 1)), r"hold\[0\] = 1 on the flat op 0"), (dict(change=_set("hold", 2, 9)), r"hold\[2\] = 9 on the flat op 2"),
             (dict(change=cap, W=510), "take 513 slots .* above 512"),
             (dict(W=252), "W = 252 is not the sum of the holds, 253"), (dict(W=0), "W = 0 is not the sum"),
             # and what is its own
             (dict(change=_attr("team_size", 3)), "team_size must be 1, 2, 4, 8 or 16, got 3"),
             (dict(change=_attr("team_size", 0)), "team_size must be"), (dict(change=_attr("team_size", 32)), "team_size must be"),
             (dict(change=_attr("team_size", 16)), "8 robots do not split into teams of 16"),
             (dict(n=6), "6 robots do not split into teams of 4"),
             (dict(change=_set("kind1", 0, 3)), r"kind1\[0\] = 3 outside 0 .. 2"), (dict(change=_set("kind1", 3, -1)), r"kind1\[3\] = -1"),
             (dict(change=_set("kind2", 2, 3)), r"kind2\[2\] = 3 outside 0 .. 2"),
             (dict(change=_set("rad1", 2, -0.5)), r"rad1\[2\] is negative or not finite"),
             (dict(change=_set("rad1", 0, np.nan)), r"rad1\[0\]"), (dict(change=_set("rad1", 3, np.inf)), r"rad1\[3\]"),
             (dict(change=_set("rad2", 2, -1.0)), r"rad2\[2\] is negative or not finite"),
             (dict(change=_attr("n_frames", 0)), "n_frames must be >= 1, got 0"), (dict(change=_attr("n_frames", -2)), "n_frames must be"),
             (dict(change=_attr("frame_steps", 0)), "frame_steps must be >= 1, got 0"),
             (dict(change=_attr("loop", 2)), "loop must be 0 or 1, got 2"), (dict(change=_attr("loop", -1)), "loop must be"),
             (dict(change=_attr("n_frames", (64 << 20) // (3 * 6 * 16) + 1)), "region frames of .* bytes are above the limit of 67108864"),
             (dict(change=frame_nan), "region 1 of scene 0 is not finite or has a negative extent in frame 2"),
             (dict(change=frame_negative), "region 0 of scene 1 .* in frame 1")]
    for kw, msg in cases:
        rc, got, untouched = raw_call(engine, spec, path, **kw)
        assert rc == _lib.ERR_INVALID and untouched, (kw, got)
        assert re.search(who, got) and re.search(msg, got), (kw, got)
    rc, got, untouched = raw_call(engine, spec, nan_path)
    assert rc == _lib.ERR_INVALID and untouched and "robot 3" in got and "record 2" in got
    with pytest.raises(ValueError, match="robot 3 in record 2"):
        engine.spec_monitor(spec, nan_path)
    with pytest.raises(ValueError, match="teams of 4"):
        engine.spec_monitor(Spec(regions(6, 3, 2, True, True), spec.clauses, team_size=4), path[:, :6])   # (a shared scene: any n)
    # the flat and the nested entry points go on refusing what they refuse
    from tests.test_spec_gpu import raw_call as flat_call
    from tests.test_spec_nested_gpu import raw_call as nested_call
    static = Regions(np.stack([ROWS, ROWS, ROWS]), KINDS, counts=[6, 4, 0], scene=np.arange(n) % 3)
    rc, got, untouched = flat_call(engine, Spec(static, [Spec.always(outside(2, 4)), Spec.eventually(inside(0))]), path,
                                   change=_set("op", 1, R.SPEC_STAY))
    assert rc == _lib.ERR_INVALID and untouched and re.search(r"^spec_monitor: spec: op\[1\] = 3 outside 0 .. 2", got)
    rc, got, untouched = nested_call(engine, Spec(static, [Spec.always(outside(2, 4)), Spec.stay(inside(0), 2)]), path,
                                     change=_set("hold", 1, 256))
    assert rc == _lib.ERR_INVALID and untouched and re.search(r"^spec_monitor_nested: spec: hold\[1\] = 256", got)
    assert raw_call(engine, spec, path)[0] == _lib.OK                        # and the engine is as usable as before


@gpu
def test_training_is_bit_identical_with_moving_monitor_calls_in_between():
    spec = mixed_spec(72, False)
    path = synthetic_path(72, 60, 2, seed=21)
    params = []
    for with_monitor in (False, True):
        e, _ = _engine("point", {}, n_envs=16, seed=7)
        e.collect_synthetic()
        e.train(None)
        if with_monitor:
            st, _ = e.spec_monitor(spec, path[:31])
            e.spec_monitor(spec, path[30:], step0=30, state=st)
        e.collect_synthetic()
        e.train(None)
        m, v, step = e.get_optimizer_state()
        params.append((e.get_flat_params().copy(), e.flatten(m).copy(), e.flatten(v).copy(), step))
        e.close()
    for a, b in zip(*params):
        assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b)))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
S = 60


def e2e(n, kw=None, tile256=False):
    """`point` with circling hazards and teams of 4: the clause over the hazards and the clause over the mates against the run's own
    clearances.  The bounds are the issue's: the monitor samples idle robots too (<=), and the hazard kernel's root is not
    correctly rounded (1e-5: about twenty float32 ulps at the arena's extent)."""
    e, _ = _engine("point", kw or {})
    env = _env("point", n)
    _go_to_goal_params(e, env)
    if tile256:
        e.set_eval_tile256(True)
    rng = np.random.default_rng(4)
    start = rng.uniform(-1.5, 1.5, (n, env.pos_dim)).astype(np.float32)
    wp = rng.uniform(-1.5, 1.5, (n, 3, env.pos_dim)).astype(np.float32)
    hz = MovingHazards.circling(rng.uniform(-1.2, 1.2, (6, 2)), travel=0.3, size=0.2, n_frames=21, dt=0.3, frame_steps=2, loop=True,
                                indicator=False)
    teams = Teams(4, 0.3)
    spec = Spec(MovingRegions.from_hazards(hz), [Spec.always(outside(0, 6), a=1), Spec.always(apart(teams.separation), a=1)],
                team_size=4)
    run = dict(max_steps=S, seed=3, path_stride=1, hazards=hz, teams=teams)
    plain = follow_waypoints(e, env, start, wp, **run)
    r = follow_waypoints(e, env, start, wp, spec=spec, **run)
    assert r["persistent"] == plain["persistent"] and np.array_equal(bits(r["path"]), bits(plain["path"]))
    want = spec_fold(spec_start(n, spec), r["path"], spec)
    assert_same_state(r["state"].spec, want)
    assert_same_result({k: r[k] for k in R.SPEC_RESULT_KEYS}, spec_result(want, spec))
    every = r["steps"] == S
    assert np.any(every)
    for c, key in enumerate(("min_clearance", "min_team_clearance")):
        rho, clear = r["spec_rho"][:, c].astype(np.float64), r[key].astype(np.float64)
        print(key, "largest rho - clearance:", float(np.nanmax(rho - clear)), "on robots that stepped throughout:",
              float(np.max(np.abs(rho[every] - clear[every]))))
        moved = ~np.isnan(clear)
        assert np.all(rho[moved] <= clear[moved] + 1e-5), key
        assert np.all(np.abs(rho[every] - clear[every]) <= 1e-5), key
    c = follow_waypoints(e, env, start, wp, spec=spec, **dict(run, max_steps=S // 3))       # three calls of 20 steps
    for _ in range(2):
        c = follow_waypoints(e, env, spec=spec, state=c["state"], **dict(run, max_steps=S // 3))
    assert_same_state(c["state"].spec, want)
    assert_same_state(monitor(r["path"], spec, engine=e)[0], monitor(r["path"], spec)[0])
    with pytest.raises(ValueError, match="teams.size = 2 differs from spec.team_size = 4"):
        follow_waypoints(e, env, start, wp, spec=spec, **dict(run, teams=Teams(2, 0.3)))
    return e, r


@gpu
def test_end_to_end_hazards_and_mates(persistent_env):
    persistent_env(None)
    e, r = e2e(64)
    e.close()


@gpu
def test_end_to_end_on_the_256_wide_tile(persistent_env):
    persistent_env(None)
    e, r = e2e(16, dict(pi=(256, 256), vf=(256, 256)), tile256=True)
    e.close()
