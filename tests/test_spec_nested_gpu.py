"""GPU: nested run specifications on the device (k_spec_monitor_nested through PPOEngine.spec_monitor and follow_waypoints(...,
spec=)) against the NumPy rule, bit for bit on val, wit, tail and the five result keys."""
import ctypes as C
import re

import numpy as np
import pytest

from mobrob_amd import _lib
from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import Regions, Spec, inside, outside, spec_fold, spec_result, spec_start
from mobrob_amd.waypoints import follow_waypoints, monitor
from tests.test_spec_gpu import KINDS, ROWS, synthetic_path
from tests.test_spec_nested_cpu import (assert_every_split_equals_the_whole, assert_same_result, assert_same_state, bits, split_case,
                                        zero_cases, zero_spec)
from tests.util import _engine, _env, _go_to_goal_params, persistent_env  # noqa: F401

gpu = pytest.mark.gpu
HOLDS = (0, 1, 5, 59, 60, 255)


@pytest.fixture(scope="module")
def engine():
    e, _ = _engine("point", {})
    yield e
    e.close()


def regions(n, shared):
    if shared:
        return Regions(ROWS, KINDS)
    return Regions(np.stack([ROWS, ROWS + np.float32([0.25, 0.0, 0.0, 0.0]), ROWS]), KINDS, counts=[6, 4, 0], scene=np.arange(n) % 3)


def hold_spec(n, T, h, shared):
    """every op, the nested ones at hold h, with open, closed and single-sample windows (four nested clauses; two where four
    windows of h + 1 are above the slot cap)"""
    cl = [Spec.always(outside(2, 4)), Spec.stay(inside(0, 2), h), Spec.until(outside(4), inside(5)),
          Spec.recur(inside(4), h, 0, max(T - h, 0)), Spec.eventually(inside(0, 2), 0, T),
          Spec.stay(outside(5), h, min(1, T), None), Spec.recur(outside(0, 6), h, T // 2, T // 2)]
    return Spec(regions(n, shared), cl if 4 * (h + 1) <= R.SPEC_WINDOW_SLOTS else cl[:5])


SHAPES = [(n, T, P) for n in (1, 16, 17, 70) for T in (1, 7, 60) for P in (2, 3)]


@gpu
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-robot"])
@pytest.mark.parametrize("n,T,P", SHAPES, ids=[f"n{n}-T{T}-P{P}" for n, T, P in SHAPES])
def test_every_hold_at_every_shape_bit_for_bit(engine, n, T, P, shared):
    path = synthetic_path(n, T, P, seed=100 * n + T)
    finite = []
    for h in HOLDS:
        spec = hold_spec(n, T, h, shared)
        want = spec_fold(spec_start(n, spec), path, spec)
        got, res = engine.spec_monitor(spec, path)
        assert_same_state(got, want, h)
        assert_same_result(res, spec_result(want, spec), h)
        assert want.tail.shape == (n, (4 if h < 255 else 2) * h)
        rho = want.val[:, [c for c, k in enumerate(spec.holds) if spec.clauses[c][0] >= R.SPEC_STAY], 0]
        assert np.all(np.isinf(rho[:, :2])) if h > T else np.any(np.isfinite(rho[:, 0]))   # a hold the call does not outlast
        finite.append(rho[np.isfinite(rho)])
    finite = np.concatenate(finite)
    if n >= 16:
        assert np.any(finite > 0) and np.any(finite < 0)


def mixed_spec(n, shared):
    """sixteen clauses, all five ops, holds of every size"""
    cl = []
    for k, h in enumerate((0, 1, 2, 5, 11, 59, 60, 100)):
        cl.append(Spec.stay((inside, outside)[k % 2](k % 3, k % 3 + 2), h, k % 4, None if k % 3 else 40))
        cl.append([Spec.always(outside(2, 4), k), Spec.eventually(inside(0, 6), 0, 3 * k), Spec.until(outside(4), inside(5), k, 50),
                   Spec.recur(inside(4, 6), h, 0, 30)][k % 4])
    return Spec(regions(n, shared), cl)


@gpu
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per-robot"])
def test_sixteen_mixed_clauses(engine, shared):
    n, T = 70, 60
    spec = mixed_spec(n, shared)
    assert spec.n_clauses == 16 and {cl[0] for cl in spec.clauses} == {0, 1, 2, 3, 4}
    path = synthetic_path(n, T, 2, seed=21)
    want = spec_fold(spec_start(n, spec), path, spec)
    got, res = engine.spec_monitor(spec, path)
    assert_same_state(got, want)
    assert_same_result(res, spec_result(want, spec))
    assert len(np.unique(want.wit)) > 4 and np.any(res["spec_rho"] > 0) and np.any(np.isfinite(res["spec_rho"]) & (res["spec_rho"] < 0))


@gpu
def test_the_slot_cap_whole_and_in_three_calls(engine):
    """two holds of 255: 512 slots, the largest LDS block, and a tail of 510 values a robot through three calls"""
    n, T = 70, 300
    spec = Spec(regions(n, False), [Spec.stay(inside(0, 2), 255), Spec.always(outside(2, 4)), Spec.recur(inside(0, 6), 255, 10, None)])
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
        assert_same_state(st, spec_fold(spec_start(n, spec), path[:100 * k + 101], spec), k)
    assert_same_state(st, want)
    assert_same_result(res3, res)


@gpu
def test_every_split_and_the_one_step_chain_on_the_device(engine):
    spec, path = split_case(n=17)
    n = path.shape[1]
    whole = assert_every_split_equals_the_whole(lambda p, step0, st: engine.spec_monitor(spec, p, step0=step0, state=st)[0], spec, path)
    assert_same_state(whole, spec_fold(spec_start(n, spec), path, spec))


@gpu
def test_signed_zeros_on_the_device(engine):
    for path, h, stay, recur in zero_cases():
        spec = zero_spec(h)
        got, _ = engine.spec_monitor(spec, path)
        assert [int(x) for x in bits(got.val[0, :, 0])] == [stay, recur], (path[:, 0, 0], h)
        assert_same_state(got, spec_fold(spec_start(1, spec), path, spec))


@gpu
def test_flat_clauses_on_the_nested_kernel_equal_the_flat_kernel(engine):
    n, T = 70, 60
    path = synthetic_path(n, T, 3, seed=8)
    for shared in (True, False):
        flat = [Spec.always(outside(2, 4)), Spec.eventually(inside(0, 2), 0, T), Spec.until(outside(4), inside(5)),
                Spec.always(inside(4), 0, 2), Spec.eventually(outside(5), T, T)]
        both = Spec(regions(n, shared), flat[:2] + [Spec.stay(inside(0), 0)] + flat[2:])
        alone, _ = engine.spec_monitor(Spec(regions(n, shared), flat), path)
        got, _ = engine.spec_monitor(both, path)
        cols = [0, 1, 3, 4, 5]
        assert np.array_equal(bits(got.val[:, cols]), bits(alone.val)) and np.array_equal(got.wit[:, cols], alone.wit)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def raw_call(engine, spec, path, step0=0, change=None, n=None, T=None, P=None, W=None, null=()):
    """mobrob_ppo_spec_monitor_nested called as a C caller would, with one thing wrong -> (return code, message, state untouched?)"""
    path = np.ascontiguousarray(path, np.float32)
    reg = spec.regions
    i32, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    sp = _lib.SpecNestedC()
    sp.n_scenes, sp.max_regions, sp.n_clauses = reg.n_scenes, reg.max_regions, spec.n_clauses
    kinds, counts, table = reg.kinds.copy(), reg.counts.copy(), reg.table.copy()
    scene = None if reg.scene is None else reg.scene.copy()
    sp.regions, sp.kinds, sp.n_regions = table.ctypes.data_as(fp), kinds.ctypes.data_as(i32), counts.ctypes.data_as(i32)
    sp.scene = None if scene is None else scene.ctypes.data_as(i32)
    for c, cl in enumerate(spec.clauses):
        op, a, b, p1, p2 = cl[:5]
        sp.op[c], sp.a[c], sp.b[c], sp.hold[c] = op, a, b, spec.holds[c]
        sp.lo1[c], sp.hi1[c], sp.out1[c] = p1[0], p1[1], int(p1[2])
        sp.lo2[c], sp.hi2[c], sp.out2[c] = p2[0], p2[1], int(p2[2])
    if change is not None:
        change(sp, table, kinds, counts, scene)
    st = spec_start(path.shape[1], spec)
    if W is not None and W > spec.tail_width:                                # the tail the call is told of is the tail it gets
        st.tail = np.full((path.shape[1], W), np.inf, np.float32)
    before = st.copy()
    args = dict(spec=C.byref(sp), path=path.ctypes.data_as(fp), val=st.val.ctypes.data_as(fp), wit=st.wit.ctypes.data_as(i32),
                tail=st.tail.ctypes.data_as(fp))
    for k in null:
        args[k] = None
    rc = engine.lib.mobrob_ppo_spec_monitor_nested(engine._h, args["spec"], args["path"], path.shape[1] if n is None else n,
                                                   path.shape[0] - 1 if T is None else T, path.shape[2] if P is None else P, step0,
                                                   args["val"], args["wit"], args["tail"], spec.tail_width if W is None else W)
    msg = engine.lib.mobrob_ppo_last_error().decode()
    untouched = (np.array_equal(bits(st.val), bits(before.val)) and np.array_equal(st.wit, before.wit)
                 and np.array_equal(bits(st.tail), bits(before.tail)))
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
def test_refusals_of_the_nested_entry_point(engine):
    n, T = 6, 4
    spec = Spec(regions(n, False), [Spec.always(outside(2, 4)), Spec.stay(inside(0, 2), 3), Spec.until(outside(4), inside(5)),
                                    Spec.recur(inside(4), 250), Spec.eventually(outside(5), T, T)])
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

    def third_window(sp, *_):                                                # 4 + 251 + 256 = 511 slots is taken, one more is not
        sp.op[0], sp.hold[0] = R.SPEC_STAY, 255

    def cap(sp, *_):
        sp.op[0], sp.hold[0], sp.hold[1] = R.SPEC_STAY, 255, 5

    nan_path = path.copy()
    nan_path[2, 3, 1] = np.inf
    who = "^spec_monitor_nested: "
    cases = [(dict(null=("path",)), "null path"), (dict(null=("val",)), "null val"), (dict(null=("wit",)), "null wit"),
             (dict(null=("spec",)), "null spec"), (dict(null=("tail",)), "null tail with W = 253"),
             (dict(n=0), "n must be >= 1"), (dict(T=0), "T must be >= 1"), (dict(P=4), "P must lie in 1 .. 3"), (dict(P=0), "P must lie"),
             (dict(change=_attr("n_clauses", 0)), "n_clauses"), (dict(change=_attr("n_clauses", 17)), "n_clauses"),
             (dict(change=_attr("max_regions", 65)), "max_regions"), (dict(change=_attr("n_scenes", 0)), "n_scenes"),
             (dict(change=count_over), r"n_regions\[1\] = 7"), (dict(change=scene_over), r"scene\[4\] = 3"),
             (dict(change=kind_two), "kind 2"), (dict(change=table_nan), "region 1 of scene 0"),
             (dict(change=_attr("scene", None)), "3 scenes need a scene index"),
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
             (dict(change=_set("hold", 1, 4)), "W = 253 is not the sum of the holds, 254")]
    for kw, msg in cases:
        rc, got, untouched = raw_call(engine, spec, path, **kw)
        assert rc == _lib.ERR_INVALID and untouched, (kw, got)
        assert re.search(who, got) and re.search(msg, got), (kw, got)
    assert raw_call(engine, spec, path, change=third_window, W=508)[0] == _lib.OK
    rc, got, untouched = raw_call(engine, spec, nan_path)
    assert rc == _lib.ERR_INVALID and untouched and "robot 3" in got and "record 2" in got
    with pytest.raises(ValueError, match="robot 3 in record 2"):
        engine.spec_monitor(spec, nan_path)
    with pytest.raises(ValueError, match="tail of shape"):
        engine.spec_monitor(spec, path, state=R.SpecState(*[getattr(spec_start(n, spec), k) for k in ("val", "wit")]))
    # the flat entry point goes on refusing the nested ops
    from tests.test_spec_gpu import raw_call as flat_call
    flat = Spec(regions(n, False), [Spec.always(outside(2, 4)), Spec.eventually(inside(0))])
    rc, got, untouched = flat_call(engine, flat, path, change=_set("op", 1, R.SPEC_STAY))
    assert rc == _lib.ERR_INVALID and untouched and re.search(r"^spec_monitor: spec: op\[1\] = 3 outside 0 .. 2", got)
    assert raw_call(engine, spec, path)[0] == _lib.OK                        # and the engine is as usable as before


class _Counting:
    """the engine's library with its calls counted by name"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


@gpu
def test_a_flat_specification_still_takes_the_flat_entry_point(engine):
    n, T = 17, 7
    path = synthetic_path(n, T, 2, seed=2)
    flat = Spec(regions(n, True), [Spec.always(outside(2, 4)), Spec.eventually(inside(0, 2))])
    nested = Spec(regions(n, True), [Spec.always(outside(2, 4)), Spec.stay(inside(0, 2), 0)])
    lib = engine.lib
    engine.lib = counting = _Counting(lib)
    try:
        a, _ = engine.spec_monitor(flat, path)
        assert counting.calls == {"mobrob_ppo_spec_monitor": 1}
        b, _ = engine.spec_monitor(nested, path)
        assert counting.calls == {"mobrob_ppo_spec_monitor": 1, "mobrob_ppo_spec_monitor_nested": 1}
    finally:
        engine.lib = lib
    assert a.tail.shape == (n, 0) and np.array_equal(bits(a.val), bits(b.val)) and np.array_equal(a.wit, b.wit)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
S = 60


def e2e(n, kw=None, tile256=False):
    e, _ = _engine("point", kw or {})
    env = _env("point", n)
    _go_to_goal_params(e, env)
    if tile256:
        e.set_eval_tile256(True)
    rng = np.random.default_rng(4)
    start = rng.uniform(-1.5, 1.5, (n, env.pos_dim)).astype(np.float32)
    wp = rng.uniform(-1.5, 1.5, (n, 3, env.pos_dim)).astype(np.float32)
    run = dict(max_steps=S, seed=3, path_stride=1)
    plain = follow_waypoints(e, env, start, wp, **run)
    # from the call's own spec-free run: a circle that holds robot 0's last seven samples and a box that holds seven of robot 1's
    # around the middle of the run, so that stay(5) is satisfied by robot 0 and recur(3) violated by robot 1, whatever their speed
    xy = plain["path"][:, :, :2].astype(np.float64)
    end0, mid1 = xy[-1, 0], xy[S // 2, 1]
    radius = float(np.max(np.linalg.norm(xy[S - 6:, 0] - end0, axis=1))) + 1e-3
    half = float(np.max(np.abs(xy[S // 2 - 3:S // 2 + 4, 1] - mid1))) + 1e-3
    reg = Regions([[end0[0], end0[1], radius, 0.0], [mid1[0], mid1[1], half, half]], [1, 0])
    spec = Spec(reg, [Spec.stay(inside(0), 5, 0, None), Spec.recur(outside(1), 3), Spec.always(outside(1)), Spec.stay(inside(0), 100)])
    r = follow_waypoints(e, env, start, wp, spec=spec, **run)
    assert r["persistent"] == plain["persistent"] and np.array_equal(bits(r["path"]), bits(plain["path"]))
    want = spec_fold(spec_start(n, spec), r["path"], spec)
    assert_same_state(r["state"].spec, want)
    assert_same_result({k: r[k] for k in R.SPEC_RESULT_KEYS}, spec_result(want, spec))
    assert np.all(r["spec_rho"][:, 3] == -np.inf) and np.all(np.isfinite(r["spec_rho"][:, :3]))
    assert r["spec_rho"][1, 1] < 0 and np.any(r["spec_rho"][:, 1] > 0) and np.any(r["spec_rho"][:, 0] < 0)
    c = follow_waypoints(e, env, start, wp, spec=spec, **dict(run, max_steps=S // 3))       # three calls of 20 steps
    for _ in range(2):
        c = follow_waypoints(e, env, spec=spec, state=c["state"], **dict(run, max_steps=S // 3))
    assert_same_state(c["state"].spec, want)
    assert_same_result({k: c[k] for k in R.SPEC_RESULT_KEYS}, spec_result(want, spec))
    assert_same_state(monitor(r["path"], spec, engine=e)[0], monitor(r["path"], spec)[0])
    return e, r


@gpu
def test_end_to_end_stay_and_recur(persistent_env):
    persistent_env(None)
    e, r = e2e(64)
    assert r["spec_rho"][0, 0] > 0                                           # robot 0 ends in its circle and stays
    e.close()


@gpu
def test_end_to_end_on_the_256_wide_tile(persistent_env):
    persistent_env(None)
    e, r = e2e(16, dict(pi=(256, 256), vf=(256, 256)), tile256=True)
    assert r["persistent"] is True
    e.close()


@gpu
def test_training_is_bit_identical_with_nested_monitor_calls_in_between():
    spec = mixed_spec(70, False)
    path = synthetic_path(70, 60, 2, seed=21)
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
