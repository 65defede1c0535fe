"""CPU: nested run specifications -- Spec.stay (eventually-always) and Spec.recur (always-eventually) in the NumPy rule
(goal_rules.spec_fold), the carried tail, the host loop, and the C layout of mobrob_ppo_spec_monitor_nested."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import Regions, Spec, SpecState, inside, outside, spec_fold, spec_result, spec_start
from mobrob_amd.envs.wrapper import get_env
from mobrob_amd.waypoints import follow_waypoints, monitor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF = f32(np.inf)


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == bool else a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint64)


def assert_same_state(got, want, why=""):
    assert np.array_equal(bits(got.val), bits(want.val)), why
    assert np.array_equal(got.wit, want.wit), why
    assert got.tail.shape == want.tail.shape and np.array_equal(bits(got.tail), bits(want.tail)), why


def assert_same_result(got, want, why=""):
    assert set(got) == set(want) == set(R.SPEC_RESULT_KEYS)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(bits(got[k]), bits(want[k])), (why, k)


# ---- the brute-force statement: from the formula, sharing nothing with spec_fold -------------------------------------------------------
def brute_margin(p, row, kind):
    """the inside margin of one region at one position, float32 operation by operation"""
    dx, dy = f32(p[0]) - row[0], f32(p[1]) - row[1]
    if kind == 1:
        return row[2] - np.sqrt(f32(dx * dx) + f32(dy * dy))
    qx, qy = f32(abs(dx)) - row[2], f32(abs(dy)) - row[3]
    ox, oy = max(qx, f32(0)), max(qy, f32(0))
    return -f32(np.sqrt(f32(ox * ox) + f32(oy * oy)) + min(max(qx, qy), f32(0)))


def brute_value(p, regions, pred):
    lo, hi, out = pred
    u = max([f32(brute_margin(p, regions.table[0, r], regions.kinds[0, r])) for r in range(lo, hi)], default=-INF)
    return f32(-u) if out else f32(u)


def total_order(v):
    """float32 in the order of its bits: by value, and -0.0 before +0.0"""
    return (float(v), 0 if math.copysign(1.0, float(v)) < 0 else 1)


def brute_nested(path, regions, clause):
    """(rho, witness) per robot of one stay / recur clause over the samples tau = 0 .. T: for every t in [a, b] with t + h <= T the
    minimum (stay) or maximum (recur) of v(t .. t + h) in the total order, then the outer maximum (stay) or minimum (recur), the
    first attainment kept"""
    op, a, b, pred, _, h = clause
    T, n = path.shape[0] - 1, path.shape[1]
    rho = np.full(n, -INF if op == R.SPEC_STAY else INF, f32)
    wit = np.full(n, -1, np.int32)
    for i in range(n):
        v = [brute_value(path[t, i], regions, pred) for t in range(T + 1)]
        for t in range(a, min(b, T - h) + 1):
            win = v[t:t + h + 1]
            s = min(win, key=total_order) if op == R.SPEC_STAY else max(win, key=total_order)
            if (s > rho[i]) if op == R.SPEC_STAY else (s < rho[i]):
                rho[i], wit[i] = s, t
    return rho, wit


# ---- random walks ----------------------------------------------------------------------------------------------------------------------
WALK_REGIONS = Regions([[0.0, 0.0, 0.3, 0.3], [0.1, 0.0, 0.3, 0.0]], [0, 1])    # a box and a circle of half-width 0.3 around the centre
HOLDS = (0, 1, 5, 39, 40)


def walks(seed, n=5, samples=40):
    """n random walks in [-1, 1]^2: robot 0 loiters at the centre (inside both regions at every sample), robot 1 in a far corner
    (outside both at every sample), the others wander across the regions' boundaries"""
    rng = np.random.default_rng(seed)
    start = np.concatenate([[[0.05, 0.0], [0.9, 0.9]], rng.uniform(-0.4, 0.4, (n - 2, 2))])
    sigma = np.concatenate([[0.005, 0.005], np.full(n - 2, 0.1)])
    step = rng.normal(0.0, 1.0, (samples, n, 2)) * sigma[None, :, None]
    step[0] = 0
    return np.clip(start[None] + np.cumsum(step, axis=0), -1.0, 1.0).astype(f32)


def walk_clauses(a, b):
    out = []
    for k, h in enumerate(HOLDS):
        out.append(Spec.stay((inside, outside)[k % 2](0, 2 if k == 2 else None), h, a, b))
        out.append(Spec.recur((outside, inside)[k % 2](1), h, a, b))
    return out


@pytest.mark.parametrize("window", [(0, None), (3, 20), (0, 0), (34, 38), (39, None)], ids=str)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fold_against_brute_force_on_random_walks(seed, window):
    path = walks(seed)
    T, n = path.shape[0] - 1, path.shape[1]
    clauses = walk_clauses(*window)
    spec = Spec(WALK_REGIONS, clauses)
    got = spec_fold(spec_start(n, spec), path, spec)
    assert np.all(np.isposinf(got.val[:, :, 1]))                             # guard is not used
    some_finite = False
    for c, cl in enumerate(clauses):
        rho, wit = brute_nested(path, WALK_REGIONS, (cl[0], cl[1], min(cl[2], T), cl[3], cl[4], cl[5]))
        assert np.array_equal(bits(got.val[:, c, 0]), bits(rho)), (c, cl)
        assert np.array_equal(got.wit[:, c], wit), (c, cl)
        if cl[1] + cl[5] <= T:                                               # some window completes: finite, and both verdicts occur
            assert np.all(np.isfinite(rho)) and np.any(rho > 0) and np.any(rho < 0), (c, cl)
            some_finite = True
        else:                                                                # none does
            assert np.all(rho == (-INF if cl[0] == R.SPEC_STAY else INF)) and np.all(wit == -1)
    assert some_finite
    assert got.tail.shape == (n, 2 * sum(HOLDS))


def test_hold_zero_is_eventually_and_always_bit_for_bit():
    path = walks(7)
    for a, b in [(0, None), (5, 17), (39, 39), (45, None)]:
        nested = Spec(WALK_REGIONS, [Spec.stay(inside(0, 2), 0, a, b), Spec.recur(outside(1), 0, a, b)])
        flat = Spec(WALK_REGIONS, [Spec.eventually(inside(0, 2), a, b), Spec.always(outside(1), a, b)])
        x, y = spec_fold(spec_start(5, nested), path, nested), spec_fold(spec_start(5, flat), path, flat)
        assert np.array_equal(bits(x.val), bits(y.val)) and np.array_equal(x.wit, y.wit)
        assert x.tail.shape == (5, 0) and nested.nested and not flat.nested
        assert_same_result(spec_result(x, nested), spec_result(y, flat))


# ---- splits ----------------------------------------------------------------------------------------------------------------------------
SPLIT_HOLDS = (1, 3, 11, 12, 20)


def split_case(n=5, T=12, seed=11):
    path = walks(seed, n=n, samples=T + 1)
    clauses = [Spec.always(outside(1), 2, 9), Spec.until(outside(1), inside(0))]
    for k, h in enumerate(SPLIT_HOLDS):
        clauses += [Spec.stay(inside(0, 2), h, 0, None if k % 2 else 6), Spec.recur(inside(k % 2), h, k % 3)]
    return Spec(WALK_REGIONS, clauses), path


def assert_every_split_equals_the_whole(fold, spec, path):
    """fold(path, step0, state) -> SpecState: every two-way split and the chain of one-step calls end on the whole run's bits"""
    T = path.shape[0] - 1
    whole = fold(path, 0, None)
    for cut in range(1, T):
        first = fold(path[:cut + 1], 0, None)
        assert_same_state(fold(path[cut:], cut, first), whole, cut)
    st = fold(path[:2], 0, None)
    for t in range(1, T):
        st = fold(path[t:t + 2], t, st)
    assert_same_state(st, whole, "one step at a time")
    return whole


def test_every_split_of_twelve_steps_carries_the_tail():
    spec, path = split_case()
    n = path.shape[1]
    whole = assert_every_split_equals_the_whole(
        lambda p, step0, st: spec_fold(spec_start(n, spec) if st is None else st, p, spec, step0), spec, path)
    assert whole.tail.shape == (n, 2 * sum(SPLIT_HOLDS))
    rho = whole.val[:, 2:, 0]
    assert np.any(np.isfinite(rho) & (rho > 0)) and np.any(np.isfinite(rho) & (rho < 0))
    # a hold of 12 completes exactly one window on 13 samples, a hold of 20 none
    c12, c20 = 2 + 2 * SPLIT_HOLDS.index(12), 2 + 2 * SPLIT_HOLDS.index(20)
    assert np.all(whole.wit[:, c12] == 0) and np.all(whole.wit[:, c20] == -1) and np.all(np.isinf(whole.val[:, c20, 0]))
    # the tail is chronological: its last entry is the last sample's value, for every hold
    last = spec_fold(spec_start(n, spec), path[-2:], spec)                   # (any fold whose last sample is the run's last)
    for c, h in enumerate(spec.holds):
        if h:
            o = spec.tail_offsets[c]
            assert np.array_equal(bits(whole.tail[:, o + h - 1]), bits(last.tail[:, o + h - 1]))


# ---- signed zeros ----------------------------------------------------------------------------------------------------------------------
ZERO_REGIONS = Regions([[0.0, 0.0, 1.0, 1.0], [3.0, 0.0, 1.0, 0.0]], [0, 1])    # the box [-1, 1]^2 and the circle of radius 1 around (3, 0)
EDGE, RIM, IN = (1.0, 0.0), (2.0, 0.0), (0.5, 0.0)                             # union margin -0.0, +0.0 and 0.5
NEG0, POS0, HALF = 0x80000000, 0x00000000, 0x3F000000


def zero_cases():
    """(path of one robot, hold, the bits of rho for stay, for recur) with inside(0, 2) over the whole run"""
    def p(*pts):
        return np.array(pts, f32)[:, None, :]
    return [(p(EDGE, RIM, IN), 1, NEG0, POS0),       # windows {-0, +0}, {+0, .5}: minima -0, +0 (a tie for >), maxima +0, .5
            (p(RIM, EDGE, IN), 1, NEG0, POS0),       # the same window visited the other way round: same bits
            (p(EDGE, RIM, IN), 2, NEG0, HALF),
            (p(RIM, EDGE, IN), 2, NEG0, HALF),
            (p(IN, RIM, EDGE, RIM), 1, POS0, POS0),  # minima +0, -0, -0: the first is kept;  maxima .5, +0, +0
            (p(RIM, EDGE, RIM, EDGE, RIM), 3, NEG0, POS0)]


def zero_spec(h):
    return Spec(ZERO_REGIONS, [Spec.stay(inside(0, 2), h), Spec.recur(inside(0, 2), h)])


def test_signed_zeros_have_one_answer():
    margins = R.region_margins(np.array([EDGE, RIM], f32), np.broadcast_to(ZERO_REGIONS.table[0], (2, 2, 4)),
                               np.broadcast_to(ZERO_REGIONS.kinds[0], (2, 2)))
    assert bits(margins)[0, 0] == NEG0 and bits(margins)[1, 1] == POS0       # the case is what it says: a box edge, a circle's rim
    for path, h, stay, recur in zero_cases():
        spec = zero_spec(h)
        st = spec_fold(spec_start(1, spec), path, spec)
        assert [int(x) for x in bits(st.val[0, :, 0])] == [stay, recur], (path[:, 0, 0], h)
    assert np.array_equal(R.spec_key(np.array([-0.0, 0.0, -1.0, 1.0, -np.inf, np.inf], f32)).argsort(), [4, 2, 0, 1, 3, 5])


# ---- incomplete windows ----------------------------------------------------------------------------------------------------------------
def test_windows_the_run_does_not_complete_are_not_folded():
    path = walks(5, samples=11)                                              # tau = 0 .. 10
    n = path.shape[1]
    spec = Spec(WALK_REGIONS, [Spec.stay(inside(0), 11), Spec.recur(inside(0), 11), Spec.stay(inside(0), 255), Spec.recur(inside(1), 200),
                               Spec.stay(inside(0, 2), 3, 7), Spec.recur(inside(1), 3, 7), Spec.stay(inside(0), 3, 8), Spec.recur(inside(0), 3, 8, 9)])
    st = spec_fold(spec_start(n, spec), path, spec)
    assert np.array_equal(st.val[:, :4, 0], np.tile([-INF, INF, -INF, INF], (n, 1))) and np.all(st.wit[:, :4] == -1)
    for c in (4, 5):                                                         # b open, one start left: t = 7, the window 7 .. 10
        rho, wit = brute_nested(path, WALK_REGIONS, spec.clauses[c][:2] + (10,) + spec.clauses[c][3:])
        assert np.array_equal(bits(st.val[:, c, 0]), bits(rho)) and np.all(st.wit[:, c] == 7) and np.array_equal(wit, st.wit[:, c])
    assert np.all(np.isinf(st.val[:, 6:, 0])) and np.all(st.wit[:, 6:] == -1)   # a start at 8 would end at 11
    # ... and the next call completes them from the tail
    more = np.concatenate([path[-1:], path[-1:]])
    nxt = spec_fold(st, more, spec, step0=10)
    assert np.all(nxt.wit[:, 6:] == 8) and np.all(nxt.wit[:, :2] == 0) and np.all(nxt.wit[:, 2:4] == -1)
    # "stay until the end of the run": a = b = T - hold asks for the last hold + 1 samples
    end = Spec(WALK_REGIONS, [Spec.stay(inside(0), 4, 6, 6)])
    rho, wit = brute_nested(path, WALK_REGIONS, end.clauses[0])
    got = spec_fold(spec_start(n, end), path, end)
    assert np.array_equal(bits(got.val[:, 0, 0]), bits(rho)) and np.all(got.wit == 6)
    assert np.array_equal(got.val[:, 0, 0], np.min([[brute_value(path[t, i], WALK_REGIONS, inside(0)) for i in range(n)] for t in range(6, 11)], axis=0))


# ---- refusals and state ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_state():
    for bad in (-1, 256, 1.5, True, None):
        with pytest.raises(ValueError, match=r"stay: hold must be an integer in 0 \.\. SPEC_HOLD_MAX = 255"):
            Spec.stay(inside(0), bad)
        with pytest.raises(ValueError, match=r"recur: every must be an integer in 0 \.\. SPEC_HOLD_MAX = 255"):
            Spec.recur(inside(0), bad)
    with pytest.raises(ValueError, match="0 <= a <= b"):
        Spec.stay(inside(0), 3, 5, 4)
    with pytest.raises(TypeError, match="inside"):
        Spec.recur((0, 1), 3)
    assert Spec.stay(inside(0), 255)[0] == R.SPEC_STAY == 3 and Spec.recur(inside(0), 0)[0] == R.SPEC_RECUR == 4
    assert (R.SPEC_HOLD_MAX, R.SPEC_WINDOW_SLOTS) == (255, 512)
    full = Spec(WALK_REGIONS, [Spec.stay(inside(0), 255), Spec.recur(inside(1), 255), Spec.always(outside(0))])   # 512 slots: the cap
    assert full.tail_width == 510 and full.holds == (255, 255, 0) and full.tail_offsets == (0, 255, 510)
    with pytest.raises(ValueError, match=r"513 slots.*SPEC_WINDOW_SLOTS = 512"):
        Spec(WALK_REGIONS, [Spec.stay(inside(0), 255), Spec.recur(inside(1), 255), Spec.stay(inside(0), 0)])
    with pytest.raises(ValueError, match=r"clause 0: hold must be an integer in 0 \.\. SPEC_HOLD_MAX"):
        Spec(WALK_REGIONS, [(R.SPEC_STAY, 0, 5, inside(0), inside(0), 300)])
    with pytest.raises(ValueError, match=r"clause 1: region range \[1, 3\) outside 0 .. 2"):
        Spec(WALK_REGIONS, [Spec.always(inside(0)), Spec.stay(inside(1, 3), 2)])
    for cl in [(R.SPEC_EVENTUALLY, 0, 5, inside(0), inside(0), 3), (R.SPEC_STAY, 0, 5, inside(0), inside(0)), (5, 0, 5, inside(0), inside(0))]:
        with pytest.raises(TypeError, match="Spec.always"):                  # a hold on a flat op, a nested op without one, no op at all
            Spec(WALK_REGIONS, [cl])
    # the state: a tail-less SpecState is a flat specification's
    flat = Spec(WALK_REGIONS, [Spec.always(outside(0))])
    st = spec_start(4, flat)
    assert st.tail.shape == (4, 0) and st.tail.dtype == f32
    plain = SpecState(st.val, st.wit)
    assert plain.tail.shape == (4, 0) and plain.copy().tail.shape == (4, 0)
    R.spec_check_state(plain, 4, flat)
    nested = Spec(WALK_REGIONS, [Spec.stay(inside(0), 3), Spec.always(outside(0)), Spec.recur(inside(1), 2)])
    st = spec_start(4, nested)
    assert np.array_equal(st.tail, np.tile([INF, INF, INF, -INF, -INF], (4, 1)))
    assert np.array_equal(st.val[0], [[-INF, INF], [INF, INF], [INF, INF]]) and np.all(st.wit == -1)
    kept = st.copy()
    assert kept.tail is not st.tail and np.array_equal(kept.tail, st.tail)
    with pytest.raises(ValueError, match=r"tail of shape \(4, 0\), the nested clauses need \(4, 5\)"):
        spec_fold(SpecState(st.val, st.wit), walks(1, n=4, samples=3), nested)
    with pytest.raises(ValueError, match=r"tail is \[n\]\[W\]"):
        SpecState(st.val, st.wit, np.zeros((3, 5), f32))
    assert "nested" in Spec.__doc__ and "stay" in Spec.__doc__ and "Not built" in Spec.__doc__
    assert "nested operators" not in Spec.__doc__
    assert set(spec_result(st, nested)) == set(R.SPEC_RESULT_KEYS)


# ---- the host loop ---------------------------------------------------------------------------------------------------------------------
class _GoToGoal:
    def __init__(self):
        self.A = np.linalg.pinv(get_env("point").env._mix)

    def predict(self, obs, deterministic=True):
        return np.clip(self.A @ np.asarray(obs, np.float64)[:2], -1.0, 1.0), None


def test_host_loop_with_a_stay_clause_equals_monitor_on_its_path():
    reg = Regions([[1.0, 1.0, 0.3, 0.0], [0.5, 0.5, 0.2, 0.2]], [1, 0])
    spec = Spec(reg, [Spec.stay(inside(0), 10), Spec.recur(outside(1), 4, 0, 40), Spec.always(outside(1)), Spec.stay(inside(0), 100)])
    starts = np.array([[0.0, 0.0], [1.0, -0.5], [-1.0, 0.9]])
    wp = np.array([[1.0, 1.0]])                                              # the robots park at the circle's centre, if they get there
    r = follow_waypoints(_GoToGoal(), "point", starts, wp, max_steps=90, path_stride=1, spec=spec)
    want, res = monitor(r["path"], spec)
    assert_same_state(r["state"].spec, want)
    assert_same_result({k: r[k] for k in R.SPEC_RESULT_KEYS}, res)
    assert np.any(r["spec_rho"][:, 0] > 0) and r["spec_rho"][0, 2] < 0         # robot 0 parks in the circle, through the box
    assert np.all(r["spec_rho"][:, 3] == -INF)                               # a hold the run does not outlast
    # three calls of 30 steps through `state` (FollowState.copy copies the tail) end on the same bits
    c = follow_waypoints(_GoToGoal(), "point", starts, wp, max_steps=30, path_stride=1, spec=spec)
    kept = c["state"].copy()
    assert kept.spec.tail is not c["state"].spec.tail
    c = follow_waypoints(_GoToGoal(), "point", max_steps=30, path_stride=1, spec=spec, state=kept)
    c = follow_waypoints(_GoToGoal(), "point", max_steps=30, path_stride=1, spec=spec, state=c["state"])
    assert_same_state(c["state"].spec, want)
    assert_same_result({k: c[k] for k in R.SPEC_RESULT_KEYS}, res)


# ---- the C side ------------------------------------------------------------------------------------------------------------------------
def test_nested_symbol_and_struct_layout(tmp_path):
    """The entry point is declared, exported and bound, the ABI number is unchanged, and sizeof / offsetof of mobrob_spec_nested_t
    as gcc lays the header out are the ctypes mirror's (every field, by name); mobrob_spec_t is a prefix of it."""
    from mobrob_amd import _lib
    header = open(os.path.join(ROOT, "include", "mobrob_ppo.h")).read()
    assert "mobrob_ppo_spec_monitor_nested(" in header and "mobrob_ppo_spec_monitor_nested" in _lib.SYMBOLS
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mobrob_ppo_spec_monitor_nested") and lib.mobrob_ppo_abi_version() == _lib.ABI_VERSION == 3
    names = [n for n, _ in _lib.SpecNestedC._fields_]
    assert names[:-1] == [n for n, _ in _lib.SpecC._fields_] and names[-1] == "hold"
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "mobrob_ppo.h"\nint main(void) {\n'
            '  printf("%zu %zu\\n", sizeof(mobrob_spec_nested_t), sizeof(mobrob_spec_t));\n'
            + "".join(f'  printf("%zu\\n", offsetof(mobrob_spec_nested_t, {n}));\n' for n in names)
            + "".join(f'  printf("%zu\\n", offsetof(mobrob_spec_t, {n}));\n' for n in names[:-1])
            + '  printf("%d %d %d %d\\n", MOBROB_SPEC_STAY, MOBROB_SPEC_RECUR, MOBROB_SPEC_HOLD_MAX, MOBROB_SPEC_WINDOW_SLOTS);\n  return 0;\n}\n')
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    k = len(names)
    assert out[:2] == [ctypes.sizeof(_lib.SpecNestedC), ctypes.sizeof(_lib.SpecC)]
    assert out[2:2 + k] == [getattr(_lib.SpecNestedC, n).offset for n in names]
    assert out[2 + k:1 + 2 * k] == out[2:1 + k]                              # the flat struct is a prefix
    assert out[1 + 2 * k:] == [R.SPEC_STAY, R.SPEC_RECUR, R.SPEC_HOLD_MAX, R.SPEC_WINDOW_SLOTS]
    # the entry point refuses a null engine before it touches a device, and names it
    rc = lib.mobrob_ppo_spec_monitor_nested(None, None, None, 1, 1, 2, 0, None, None, None, 0)
    lib.mobrob_ppo_last_error.restype = ctypes.c_char_p
    assert rc == _lib.ERR_INVALID and b"spec_monitor_nested: null engine" in lib.mobrob_ppo_last_error()
