"""CPU: the plan from a specification from the middle of a run, the NumPy rule itself (goal_rules.spec_plan with state=, step0=,
partial=; spec_plan_clauses, spec_plan_done, spec_plan_tour_resume): the defaults bit for bit, a deletion oracle, a brute force over
every subset and order, the absolute time base, the closed loop with the monitor (spec_fold) without a policy, the hand-over of the
run's state in follow_with_replanning, every refusal by name, and the new C symbol."""
import itertools

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.planning import GridPlanner
from tests.plan_spec_scenes import EXTENT, deadline_scene, random_scene, run_rule

INF, NONE = R.PLAN_TOUR_INF, R.PLAN_ASSIGN_NONE


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def state_with(spec, done):
    """a SpecState in which exactly the stations `done` [n][M] read as satisfied"""
    st = R.spec_start(done.shape[0], spec)
    cl = R.spec_plan_clauses(spec)
    st.val[:, cl, 0] = np.where(done, np.float32(0.25), st.val[:, cl, 0])
    return st


def plan(sc, K=16, **kw):
    return R.spec_plan(sc["grid"], sc["walls"], None, sc["spec"], sc["start"], sc["goal"], K, sc["pace"], **kw)


@pytest.fixture(scope="module")
def scenes():
    """one scene and its plain plan per (M, goal), made once"""
    out = {}
    for M, goal in ((1, True), (4, True), (4, False), (8, False)):
        sc = random_scene(40 + M, M, n=4, windows=(M == 4), goal=goal)
        out[M, goal] = (sc, run_rule(sc))
    return out


def test_the_defaults_are_the_plan_as_it_was(scenes):
    for (M, goal), (sc, ref) in scenes.items():
        out = plan(sc, state=None, step0=0, partial=False)
        for k in R.SPEC_PLAN_KEYS:
            assert np.array_equal(bits(out[k]), bits(ref[k])), k
        planned = ref["status"] != R.UNREACHABLE
        assert np.array_equal(ref["tour_len"], np.where(planned, M, 0)) and not ref["done"].any() and ref["done"].shape == (4, M)
        assert np.array_equal(ref["dropped"], np.where(planned, 0, (1 << M) - 1))
        assert R.SPEC_REPLAN_KEYS == ("tour_len", "dropped", "done") and all(k in ref for k in R.SPEC_REPLAN_KEYS)
        fresh = plan(sc, state=R.spec_start(4, sc["spec"]))                 # the state before the first sample: nothing is done
        for k in R.SPEC_PLAN_KEYS + R.SPEC_REPLAN_KEYS:
            assert np.array_equal(bits(fresh[k]), bits(ref[k])), k


@pytest.mark.parametrize("M,goal,pattern", [(1, True, [1]), (4, True, [0, 1, 0, 1]), (4, False, [1, 0, 0, 0]), (4, True, [1, 1, 1, 1]),
                                            (4, False, [1, 1, 1, 1]), (8, False, [1, 0, 1, 1, 0, 1, 1, 0]), (8, False, [1] * 8)])
def test_done_stations_are_deleted_clauses(scenes, M, goal, pattern):
    sc, _ = scenes[M, goal]
    n, spec = 4, sc["spec"]
    done = np.tile(np.array(pattern, bool), (n, 1))
    out = plan(sc, state=state_with(spec, done))
    assert np.array_equal(out["done"], done)
    keep = np.flatnonzero(~done[0])
    if keep.size == 0:                                                      # all done: the goal leg alone, or nothing at all
        assert np.all(out["tour_len"] == 0) and np.all(out["dropped"] == 0) and np.all(out["tour_order"] == -1)
        assert not out["release"].any() and np.all(out["station_waypoint"] == -1)
        if sc["goal"] is None:
            assert np.all(out["status"] == R.PLANNED) and np.all(out["count"] == 0) and np.all(out["cost"] == 0) and not out["waypoints"].any()
        else:
            ref = R.grid_plan(sc["grid"], None, None, sc["start"], sc["goal"], 16, occupancy=out["occupancy"])
            for k in ("waypoints", "count", "status"):
                assert np.array_equal(bits(out[k]), bits(ref[k])), k
            assert np.array_equal(out["cost"], np.where(ref["status"] == R.UNREACHABLE, -1, ref["cost"]))
        return
    clause = R.spec_plan_clauses(spec)
    gone = set(int(c) for c in clause[done[0]])
    less = dict(sc, spec=R.Spec(spec.regions, [cl for c, cl in enumerate(spec.clauses) if c not in gone]))
    ref = run_rule(less)
    for k in ("waypoints", "n_waypoints", "count", "status", "cost", "release"):
        assert np.array_equal(bits(out[k]), bits(ref[k])), k
    L = keep.size
    assert np.array_equal(out["tour_len"], ref["tour_len"]) and np.all(out["tour_order"][:, L:] == -1)
    mapped = np.where(ref["tour_order"] >= 0, keep[np.maximum(ref["tour_order"], 0)], -1)
    assert np.array_equal(out["tour_order"][:, :L], mapped)
    assert np.array_equal(out["tour_eta"][:, :L], ref["tour_eta"]) and np.array_equal(out["station_waypoint"][:, :L], ref["station_waypoint"])
    assert np.array_equal(out["dropped"], np.where(ref["status"] == R.UNREACHABLE, (1 << M) - 1 & ~sum(1 << j for j in range(M) if pattern[j]), 0))


def brute(d0, D, E, e0, open_c, close_c, dwell_c, todo, t0, partial):
    """every subset of todo and every order, in plain Python -> (V, order, cost) or None.  best(V, j): the least departure over the
    orders of V that end in j; the order is read back with the rule's tie: the lowest predecessor of equal values."""
    def dep(j, arr):
        begin = max(arr, open_c[j])
        return begin + dwell_c[j] if begin <= close_c[j] else INF

    def run(order):
        now = t0
        for k, j in enumerate(order):
            leg = d0[j] if k == 0 else D[order[k - 1]][j]
            if leg >= NONE:
                return INF
            now = dep(j, now + leg)
            if now >= INF:
                return INF
        return now
    M = len(d0)
    members = lambda V: [j for j in range(M) if V >> j & 1]   # noqa: E731
    best = {}
    for V in range(1, 1 << M):
        if V & ~todo:
            continue
        for j in members(V):
            rest = [i for i in members(V) if i != j]
            best[V, j] = min(run(p + (j,)) for p in itertools.permutations(rest))
    entries = []
    have = bin(todo).count("1")
    if e0 < NONE and (partial or todo == 0):
        entries.append((have, t0 + e0, 0, -1))
    for (V, j), v in best.items():
        if v < INF and E[j] < NONE and (partial or V == todo):
            entries.append((have - bin(V).count("1"), v + E[j], V, j))
    if not entries:
        return None
    _, cost, V, j = min(entries)
    order = []
    while j >= 0:
        order.append(j)
        rest = V ^ (1 << j)
        nxt = -1
        for i in members(rest):
            if best[rest, i] < INF and D[i][j] < NONE and dep(j, best[rest, i] + D[i][j]) == best[V, j]:
                nxt = i
                break
        V, j = rest, nxt
    return sum(1 << q for q in order), order[::-1], cost


def costs_of(sc, out):
    """d0, D, E, e0 of every robot, from the fields made anew on the plan's map and anchors"""
    G, occ, cell = sc["grid"].cells, out["occupancy"][0], out["station_cell"][0]
    M, n = len(cell), len(sc["start"])
    real = lambda v: NONE if v < 0 else int(v)   # noqa: E731
    fields = [R.grid_field(occ, c).reshape(-1) if c >= 0 else np.full(G * G, -1) for c in cell]
    scell, gcell = R.plan_assign_cells(sc["grid"], sc["start"], sc["start"] if sc["goal"] is None else sc["goal"])
    D = [[real(fields[j][cell[i]]) if cell[i] >= 0 else NONE for j in range(M)] for i in range(M)]
    rows = []
    for r in range(n):
        gf = None if sc["goal"] is None else R.grid_field(occ, gcell[r]).reshape(-1)
        rows.append(([real(f[scell[r]]) for f in fields], D, [0 if gf is None else (real(gf[c]) if c >= 0 else NONE) for c in cell],
                     0 if gf is None else real(gf[scell[r]])))
    return rows


BRUTE = [(3, 5, True, 0), (4, 5, True, 150), (6, 4, False, 150), (9, 3, True, 40)]


def brute_case(seed, M, goal, step0):
    """-> how many robots, with partial on, dropped a station, kept all of a nonempty todo, ended with the empty tour"""
    n = 10
    sc = random_scene(seed, M, n=n, windows=True, goal=goal, walls=False)
    rng = np.random.default_rng(seed)
    todo = rng.integers(0, 1 << M, n)
    todo[0], todo[1], todo[2] = 0, (1 << M) - 1, (1 << M) - 1
    done = ((todo[:, None] >> np.arange(M)) & 1) == 0
    st = state_with(sc["spec"], done)
    seen = {"dropped": 0, "all": 0, "none": 0}
    for partial in (False, True):
        out = plan(sc, state=st, step0=step0, partial=partial)
        t0 = -((-5 * step0) // sc["pace"])
        assert out["t0"] == t0
        for r, (d0, D, E, e0) in enumerate(costs_of(sc, out)):
            want = brute(d0, D, E, e0, out["open_c"], out["close_c"], out["dwell_c"], int(todo[r]), t0, partial)
            if want is None:
                assert out["status"][r] == R.UNREACHABLE and out["cost"][r] == -1 and out["tour_len"][r] == 0, r
                assert out["dropped"][r] == todo[r] and np.all(out["tour_order"][r] == -1)
                continue
            V, order, cost = want
            L = len(order)
            assert out["status"][r] != R.UNREACHABLE and out["cost"][r] == cost and out["tour_len"][r] == L, (r, want, out["cost"][r])
            assert list(out["tour_order"][r, :L]) == order and np.all(out["tour_order"][r, L:] == -1), (r, want, out["tour_order"][r])
            assert out["dropped"][r] == todo[r] & ~V
            if partial:
                seen["dropped"] += out["dropped"][r] != 0
                seen["all"] += todo[r] != 0 and out["dropped"][r] == 0
                seen["none"] += todo[r] != 0 and L == 0
        if partial:
            full = plan(sc, state=st, step0=step0, partial=False)
            same = full["status"] != R.UNREACHABLE                         # where the full set is feasible, partial is the same answer
            for k in R.SPEC_PLAN_KEYS[:9] + ("tour_len", "dropped"):
                assert np.array_equal(bits(out[k][same]), bits(full[k][same])), k
    return seen


def test_brute_force_over_every_subset_and_order():
    """... and the seeds counted, so that the test cannot pass vacuously: some robot drops a station, some keeps all, some ends with
    the empty tour"""
    total = {"dropped": 0, "all": 0, "none": 0}
    for args in BRUTE:
        for k, v in brute_case(*args).items():
            total[k] += int(v)
    assert total["dropped"] > 0 and total["all"] > 0 and total["none"] > 0, total


def test_the_time_base_is_absolute():
    grid, spec, start, goal = deadline_scene()
    call = lambda sp, **kw: R.spec_plan(grid, None, None, sp, start, goal, 16, 2, **kw)   # noqa: E731
    base = call(spec())
    later = call(spec(), step0=100)                                         # t0 = 250 ticks: every time moves by it
    assert later["t0"] == 250 and later["cost"][0] == base["cost"][0] + 250
    assert np.array_equal(later["tour_eta"], base["tour_eta"] + 250) and np.array_equal(later["waypoints"], base["waypoints"])
    assert call(spec(), step0=3)["t0"] == 8                                 # 15 / 2, rounded up: step0 * 5 % pace != 0
    # a deadline on station 0 at step 60 (tick 150) has closed before t0 = 250: the tour is lost, or the station dropped
    lost = call(spec(deadline=60), step0=100)
    assert lost["status"][0] == R.UNREACHABLE and lost["dropped"][0] == 3 and lost["tour_len"][0] == 0
    kept = call(spec(deadline=60), step0=100, partial=True)
    assert kept["status"][0] == R.PLANNED and kept["dropped"][0] == 1 and kept["tour_len"][0] == 1 and list(kept["tour_order"][0]) == [1, -1]
    # begin == close: the robot arrives at station 0 exactly at the closing tick, and one tick too late
    direct = call(spec(deadline=60), partial=True)                          # forces 0 first; its arrival from the start
    arrive = int(direct["tour_eta"][0, 0])
    assert direct["tour_order"][0, 0] == 0 and arrive > 0
    exact = R.spec_plan(grid, None, None, spec(deadline=arrive), start, goal, 16, 5, partial=True)   # pace 5: a tick a step, close == arrival
    assert exact["close_c"][0] == arrive and exact["tour_eta"][0, 0] == arrive and exact["dropped"][0] == 0
    short = R.spec_plan(grid, None, None, spec(deadline=arrive - 1), start, goal, 16, 5, partial=True)
    assert short["dropped"][0] == 1
    # a window that opens after t0: the robot is held, and the release is the departure in steps
    held = call(spec(opens=400), step0=100)
    k = list(held["tour_order"][0]).index(1)
    depart = int(held["open_c"][1])
    assert held["tour_eta"][0, k] < depart
    slot = held["station_waypoint"][0, k] + 1
    assert held["release"][0, slot] == -(-depart * 2 // 5) == 400 and np.count_nonzero(held["release"]) == 1


def test_done_is_strictly_positive():
    reg = R.Regions([[0.0, 0.0, 0.5, 0.5], [1.0, 1.0, 0.5, 0.5]], [0, 0])
    spec = R.Spec(reg, [R.Spec.always(R.outside(1)), R.Spec.eventually(R.inside(0)), R.Spec.stay(R.inside(1), 3)])
    assert list(R.spec_plan_clauses(spec)) == [1, 2]
    st = R.spec_start(5, spec)
    st.val[:, 1, 0] = [0.0, -0.0, 0.0, -np.inf, np.inf]
    st.val[:, 2, 0] = [0.0, 1.0, 0.0, 0.0, -0.0]
    raw = st.val.view(np.int32)                                             # the smallest positive float32 and its negative, by their bits
    raw[2, 1, 0], raw[0, 2, 0], raw[2, 2, 0] = 1, 1, np.int32(-2 ** 31 + 1)
    st.tail[:] = 5.0                                                        # a dwell in progress is not read
    assert np.array_equal(R.spec_plan_done(spec, st), [[False, True], [False, True], [True, False], [False, False], [True, False]])
    with pytest.raises(TypeError, match="SpecState"):
        R.spec_plan_done(spec, st.val)
    with pytest.raises(ValueError, match="clauses"):
        R.spec_plan_done(spec, R.SpecState(st.val[:, :2], st.wit[:, :2]))


def line_scene():
    """three covered stations in a row east of the start and a keep-out box off to the side: the tour is 0, 1, 2 and no leg crosses a
    station that is not its end"""
    grid = R.GridSpec(EXTENT, 32)
    reg = R.Regions([[-1.2, 0.1, 0.45, 0.45], [0.3, 0.1, 0.45, 0.45], [1.8, 0.1, 0.45, 0.45], [0.3, 2.0, 0.3, 0.3]], [0, 0, 0, 0])
    spec = R.Spec(reg, [R.Spec.eventually(R.inside(0)), R.Spec.always(R.outside(3)), R.Spec.eventually(R.inside(1)), R.Spec.eventually(R.inside(2))])
    start = np.array([[-2.6, 0.1], [-2.6, 0.3]], np.float32)
    return grid, spec, start


def walk(start, waypoints, step=0.08):
    """[T + 1][n][2]: every robot along its waypoints in steps of at most `step`, then standing; all robots the same T"""
    rows = []
    for s, wps in zip(start, waypoints):
        pts, at = [np.asarray(s, np.float64)], np.asarray(s, np.float64)
        for w in wps:
            k = max(int(np.ceil(np.linalg.norm(w - at) / step)), 1)
            pts += [at + (w - at) * (q + 1) / k for q in range(k)]
            at = np.asarray(w, np.float64)
        rows.append(pts)
    T = max(len(p) for p in rows)
    return np.stack([np.stack(p + [p[-1]] * (T - len(p))) for p in rows], axis=1).astype(np.float32)


@pytest.mark.parametrize("k", [1, 2])
def test_closed_loop_with_the_monitor_and_no_policy(k):
    grid, spec, start = line_scene()
    first = R.spec_plan(grid, None, None, spec, start, None, 16, 2)
    assert np.all(first["status"] == R.PLANNED) and np.all(first["covered"]) and np.all(first["tour_order"] == [0, 1, 2])
    path = walk(start, [first["waypoints"][r, :first["station_waypoint"][r, k - 1] + 1] for r in range(2)])
    state = R.spec_fold(R.spec_start(2, spec), path, spec)
    T = path.shape[0] - 1
    again = R.spec_plan(grid, None, None, spec, path[-1], None, 16, 2, state=state, step0=T, partial=True)
    walked = np.arange(3) < k
    assert np.array_equal(again["done"], np.tile(walked, (2, 1)))
    assert np.all(again["status"] == R.PLANNED) and np.all(again["tour_len"] == 3 - k) and np.all(again["dropped"] == 0)
    assert np.array_equal(np.sort(again["tour_order"][:, :3 - k], axis=1), np.tile(np.flatnonzero(~walked), (2, 1)))
    assert np.all(again["tour_eta"][:, 0] >= again["t0"]) and again["t0"] == -(-5 * T // 2)
    more = walk(path[-1], [again["waypoints"][r, :again["count"][r]] for r in range(2)])
    end = R.spec_fold(state, more, spec, step0=T)
    assert np.all(end.val[:, R.spec_plan_clauses(spec), 0] > 0) and np.all(R.spec_result(end, spec)["satisfied"])
    assert np.all(R.spec_plan(grid, None, None, spec, more[-1], None, 16, 2, state=end, step0=T + more.shape[0] - 1)["count"] == 0)


def test_follow_with_replanning_hands_the_state_to_a_planner_that_wants_it():
    from mobrob_amd.waypoints import FollowState, follow_with_replanning
    from tests.test_follow_cpu import _GoToGoal
    grid, spec, start = line_scene()
    wp = np.tile(np.array([[[-1.2, 0.1]]]), (2, 1, 1))
    got = []

    def wants(positions, status, reached, state=None):
        got.append(state.copy())
        return {}
    wants.wants_state = True

    def plain(positions, status, reached):
        got.append("plain")
        return {}
    kw = dict(horizon=5, rounds=2, spec=spec, path_stride=1)
    follow_with_replanning(_GoToGoal(), "point", start, wp, wants, **kw)
    follow_with_replanning(_GoToGoal(), "point", start, wp, plain, **kw)
    assert isinstance(got[0], FollowState) and isinstance(got[0].spec, R.SpecState) and got[0].step0 == 5 and got[1] == "plain"
    planner = GridPlanner("point", cells=32, extent=EXTENT)
    a = planner.plan_spec(got[0].positions, spec, pace=2, state=got[0])
    b = planner.plan_spec(got[0].positions, spec, pace=2, state=got[0].spec, step0=5)
    assert a["t0"] == 13 and all(np.array_equal(bits(a[k]), bits(b[k])) for k in R.SPEC_PLAN_KEYS + R.SPEC_REPLAN_KEYS)
    with pytest.raises(ValueError, match="step0"):
        planner.plan_spec(got[0].positions, spec, pace=2, state=got[0], step0=7)
    with pytest.raises(ValueError, match="specification"):
        planner.plan_spec(start, spec, pace=2, state=FollowState(start, wp))

    def releases(positions, status, reached, state=None):
        return {0: (np.array([[0.3, 0.1]]), np.array([40]))}
    releases.wants_state = True
    with pytest.raises(ValueError, match="schedule"):
        follow_with_replanning(_GoToGoal(), "point", start, wp, releases, **kw)
    out = follow_with_replanning(_GoToGoal(), "point", start, wp, releases, schedule=R.Schedule(np.zeros((2, 1), np.int32), home=start), **kw)
    assert out["state"].release[0, 0] == 40
    cb = planner.spec_callback(spec, pace=2)
    assert cb.wants_state and cb.calls == 0 and cb.last is None
    from mobrob_amd.waypoints import GOING, STALLED
    assert cb(got[0].positions, np.array([GOING, GOING]), np.zeros(2), state=got[0]) == {} and cb.calls == 1 and cb.last is None
    rows = cb(got[0].positions, np.array([STALLED, GOING]), np.zeros(2), state=got[0])
    assert list(rows) == [0] and np.array_equal(rows[0][0], a["waypoints"][0, :a["count"][0]]) and cb.calls == 2
    assert sorted(planner.spec_callback(spec, pace=2, when="all")(got[0].positions, np.array([STALLED, GOING]), np.zeros(2), state=got[0])) == [0, 1]
    with pytest.raises(ValueError, match="when"):
        planner.spec_callback(spec, when="never")
    with pytest.raises(ValueError, match="state"):
        cb(got[0].positions, np.array([STALLED, GOING]), np.zeros(2))


def test_every_refusal_by_name():
    grid, spec, start = line_scene()
    call = lambda **kw: R.spec_plan(grid, None, None, spec, start, None, 8, kw.pop("pace", 2), **kw)   # noqa: E731
    for bad in (-1, 1.0, True, "3"):
        with pytest.raises(ValueError, match="step0"):
            call(step0=bad)
    with pytest.raises(ValueError, match="pace"):
        call(step0=5, pace=None)                                            # no window or dwell anywhere, but t0 is in ticks
    assert call(step0=0, pace=None)["t0"] == 0
    with pytest.raises(ValueError, match="PLAN_TOUR_TICKS_MAX"):
        call(step0=R.PLAN_TOUR_TICKS_MAX + 1, pace=5)
    with pytest.raises(ValueError, match="PLAN_TOUR_TICKS_MAX"):
        call(step0=(R.PLAN_TOUR_TICKS_MAX * 2) // 5 + 1)
    assert call(step0=R.PLAN_TOUR_TICKS_MAX, pace=5)["t0"] == R.PLAN_TOUR_TICKS_MAX
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="partial"):
            call(partial=bad)
    with pytest.raises(TypeError, match="SpecState"):
        call(state=np.zeros((2, 4, 2)))
    with pytest.raises(ValueError, match="state"):
        call(state=R.spec_start(3, spec))
    other = R.Spec(spec.regions, list(spec.clauses[:2]))
    with pytest.raises(ValueError, match="state"):
        call(state=R.spec_start(2, other))
    with pytest.raises(ValueError, match="until"):
        R.spec_plan_clauses(R.Spec(spec.regions, [R.Spec.until(R.inside(0), R.inside(1))]))


def test_the_new_symbol_is_declared_exported_and_bound():
    import ctypes
    import os
    import re
    from mobrob_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mobrob_ppo.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    name = "mobrob_ppo_spec_replan"
    decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert decl, f"{name} is not declared in include/mobrob_ppo.h"
    assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS[name][1]) == len(decl.group(1).split(",")) == len(_lib.SYMBOLS["mobrob_ppo_spec_plan"][1]) + 5 == 39
    assert lib.mobrob_ppo_abi_version() == _lib.ABI_VERSION == 3
    assert len([n for n in _lib.SYMBOLS if n.startswith("mobrob_ppo_plan_")]) == 10
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    assert fn(*([None] * 5), 1, None, None, 0, *([None] * 5), 1, *([None] * 6), 0, 0, *([None] * 16)) == _lib.ERR_INVALID


class _Wander:
    """a policy that needs no checkpoint: a fixed action"""

    def predict(self, obs, deterministic=True):
        return np.array([0.6, 0.3]), None


def test_the_follow_example_replans_its_specification(capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mod = importlib.util.spec_from_file_location("follow_cli", os.path.join(root, "examples", "follow.py"))
    cli = importlib.util.module_from_spec(mod)
    mod.loader.exec_module(cli)
    box = np.array([[0.0, 0.0, 0.05, 0.6]])
    kw = dict(max_steps=40, host=True, seed=3, policy=_Wander(), goal=[0.7, 0.7], plan_cells=64, check_spec=True)
    r = cli.follow("point", "ppo", None, 4, walls=box, arena=True, plan_spec=True, spec_hold=3, pace=4, replan_spec=True, partial=True,
                   horizon=10, leg_steps=5, **kw)
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("planned from the specification: ") and any(ln.startswith("specification satisfied: ") for ln in out)
    assert r["state"].step0 == 40 and r["state"].release is not None      # the run had a schedule from its first call
    with pytest.raises(ValueError, match="--replan-spec needs --plan-spec"):
        cli.follow("point", "ppo", None, 4, replan_spec=True, **kw)
    with pytest.raises(ValueError, match="--partial needs --plan-spec"):
        cli.follow("point", "ppo", None, 4, partial=True, **kw)
    flags = {a.dest for a in cli.build_parser()._actions}
    assert {"replan_spec", "partial"} <= flags
