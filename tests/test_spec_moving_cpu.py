"""CPU: run specifications over things that move -- MovingRegions (a frame axis on the region table) and the mate predicates
together() / apart() in the NumPy rule (goal_rules.spec_fold), the host loop, and the C layout of mobrob_ppo_spec_monitor_moving."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import (MovingHazards, MovingRegions, Regions, Spec, Teams, apart, inside, outside, spec_fold, spec_result,
                                        spec_start, together)
from mobrob_amd.waypoints import follow_waypoints, monitor
from tests.test_spec_nested_cpu import (_GoToGoal, assert_every_split_equals_the_whole, assert_same_result, assert_same_state, bits,
                                        brute_margin, total_order, walks)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF = f32(np.inf)
KINDS = np.array([0, 1, 1], np.int32)            # a box and two circles


def frames(F, seed=0, S=1):
    """[S][F][3][4]: a box and two circles that drift across the centre of the walks' arena, a new position in every frame"""
    rng = np.random.default_rng(seed)
    base = np.array([[0.0, 0.0, 0.3, 0.2], [0.1, 0.0, 0.3, 0.0], [-0.2, 0.2, 0.25, 0.0]])
    t = np.zeros((S, F, 3, 4))
    t[:] = base
    t[..., :2] += rng.uniform(-0.3, 0.3, (S, F, 3, 2))
    t[..., 2] += rng.uniform(0.0, 0.1, (S, F, 3))
    return t.astype(f32)


def moving(F, frame_steps=1, loop=False, seed=0):
    return MovingRegions(frames(F, seed)[0], KINDS, frame_steps=frame_steps, loop=loop)


# ---- the brute-force statement: per robot and sample, sharing nothing with spec_fold ----------------------------------------------------
def brute_frame(tau, F, frame_steps, loop):
    g = max(tau - 1, 0)
    k = g // frame_steps
    return k % F if loop else min(k, F - 1)


def brute_value(path, tau, i, spec, pred):
    """the value of one predicate for robot i at the sample tau of a whole run (record tau)"""
    reg = spec.regions
    p = [f32(path[tau, i, 0]), f32(path[tau, i, 1]) if path.shape[2] > 1 else f32(0)]
    if pred[0] == "mates":
        _, kind, d = pred
        size = spec.team_size
        g = []
        for m in range(size):
            j = (i // size) * size + m
            if j != i:
                q = [f32(path[tau, j, 0]), f32(path[tau, j, 1]) if path.shape[2] > 1 else f32(0)]
                dx, dy = p[0] - q[0], p[1] - q[1]
                g.append(f32(f32(d) - np.sqrt(f32(f32(dx * dx) + f32(dy * dy)))))
        if kind == R.SPEC_PRED_TOGETHER:
            return f32(min(g, default=INF))
        return f32(-max(g, default=-INF))
    lo, hi, out = pred
    s = 0 if reg.scene is None else int(reg.scene[i])
    table = reg.table[s, brute_frame(tau, reg.n_frames, reg.frame_steps, reg.loop)] if isinstance(reg, MovingRegions) else reg.table[s]
    u = max([f32(brute_margin(p, table[r], reg.kinds[s, r])) for r in range(lo, min(hi, reg.counts[s]))], default=-INF)
    return f32(-u) if out else f32(u)


def brute_clause(path, spec, c):
    """(rho, witness) per robot of clause c over the samples tau = 0 .. T"""
    cl = spec.clauses[c]
    op, a, b, p1, p2 = cl[:5]
    T, n = path.shape[0] - 1, path.shape[1]
    rho = np.full(n, INF if op in (R.SPEC_ALWAYS, R.SPEC_RECUR) else -INF, f32)
    wit = np.full(n, -1, np.int32)
    for i in range(n):
        v1 = [brute_value(path, t, i, spec, p1) for t in range(T + 1)]
        if op in (R.SPEC_STAY, R.SPEC_RECUR):
            h = cl[5]
            for t in range(a, min(b, T - h) + 1):
                w = v1[t:t + h + 1]
                s = min(w, key=total_order) if op == R.SPEC_STAY else max(w, key=total_order)
                if (s > rho[i]) if op == R.SPEC_STAY else (s < rho[i]):
                    rho[i], wit[i] = s, t
        elif op == R.SPEC_UNTIL:
            v2 = [brute_value(path, t, i, spec, p2) for t in range(T + 1)]
            for t in range(a, min(b, T) + 1):
                w = min([v2[t]] + v1[:t + 1])
                if w > rho[i]:
                    rho[i], wit[i] = w, t
        else:
            for t in range(a, min(b, T) + 1):
                if (v1[t] < rho[i]) if op == R.SPEC_ALWAYS else (v1[t] > rho[i]):
                    rho[i], wit[i] = v1[t], t
    return rho, wit


def five_kinds(a=0, b=None):
    """all five clause kinds over region and mate predicates"""
    return [Spec.always(outside(0, 3), a, b), Spec.eventually(inside(1, 3), a, b), Spec.until(outside(0), inside(2), a, b),
            Spec.stay(inside(0, 2), 3, a, b), Spec.recur(outside(2), 2, a, b),
            Spec.always(apart(0.2), a, b), Spec.eventually(together(0.5), a, b), Spec.until(apart(0.1), together(0.4), a, b),
            Spec.stay(together(0.8), 2, a, b), Spec.recur(apart(0.3), 4, a, b), Spec.until(outside(1), apart(0.5), a, b)]


@pytest.mark.parametrize("frame_steps,loop", [(1, False), (4, True), (7, False), (3, True)])
@pytest.mark.parametrize("size", [1, 2, 4])
def test_fold_against_brute_force(size, frame_steps, loop):
    path = walks(3 + size, n=8, samples=25)
    reg = moving(5, frame_steps, loop)
    assert [reg.frame_at(t) for t in range(3)] == [0, 0, brute_frame(2, 5, frame_steps, loop)]
    for a, b in [(0, None), (2, 17)]:
        spec = Spec(reg, five_kinds(a, b), team_size=size)
        assert spec.dynamic and spec.moving and spec.mates
        got = spec_fold(spec_start(8, spec), path, spec)
        for c in range(spec.n_clauses):
            rho, wit = brute_clause(path, spec, c)
            assert np.array_equal(bits(got.val[:, c, 0]), bits(rho)), (c, spec.clauses[c])
            assert np.array_equal(got.wit[:, c], wit), (c, spec.clauses[c])
        rho = got.val[:, :5, 0]
        assert np.any(rho > 0) and np.any(np.isfinite(rho) & (rho < 0))
        if size == 1:                                                        # a team of one reads +inf in every mate predicate
            assert np.all(got.val[:, [5, 6, 8, 9], 0] == INF) and np.all(got.wit[:, 5] == -1)
        else:
            assert np.all(np.isfinite(got.val[:, 5:10, 0]))


def test_the_frames_matter_and_one_dimension_reads_y_as_zero():
    path = walks(2, n=4, samples=25)
    a, b = (Spec(moving(5, 1, False, seed=s), five_kinds()[:5]) for s in (0, 1))
    assert not np.array_equal(spec_fold(spec_start(4, a), path, a).val, spec_fold(spec_start(4, b), path, b).val)
    line = Spec(moving(3, 2, True), five_kinds(), team_size=2)
    one, two = path[:, :, :1], np.concatenate([path[:, :, :1], np.zeros_like(path[:, :, :1])], axis=2)
    assert_same_state(spec_fold(spec_start(4, line), one, line), spec_fold(spec_start(4, line), two, line))


def test_one_frame_is_the_static_regions_bit_for_bit():
    path = walks(9, n=6, samples=30)
    table = frames(1, seed=4)[0, 0]
    clauses = five_kinds()[:5]
    static = Spec(Regions(table, KINDS), clauses)
    assert not static.dynamic and not static.moving and static.team_size == 1
    want = spec_fold(spec_start(6, static), path, static)
    for frame_steps, loop in [(1, False), (7, True)]:
        one = Spec(MovingRegions(table[None], KINDS, frame_steps=frame_steps, loop=loop), clauses)
        assert one.dynamic and one.tail_width == static.tail_width == 5
        got = spec_fold(spec_start(6, one), path, one)
        assert_same_state(got, want)
        assert_same_result(spec_result(got, one), spec_result(want, static))
    # per-robot scenes with counts, as Regions takes them
    scene = np.arange(6) % 2
    st2 = Spec(Regions(np.stack([table, table + f32([0.1, 0, 0, 0])]), KINDS, counts=[3, 2], scene=scene), clauses)
    mv2 = Spec(MovingRegions(np.stack([table, table + f32([0.1, 0, 0, 0])])[:, None], KINDS, counts=[3, 2], scene=scene), clauses)
    assert_same_state(spec_fold(spec_start(6, mv2), path, mv2), spec_fold(spec_start(6, st2), path, st2))


def test_from_hazards_and_join():
    rng = np.random.default_rng(0)
    hz = MovingHazards(rng.uniform(-1, 1, (2, 4, 3, 2)), rng.uniform(0.1, 0.3, (2, 4, 3)), frame_steps=3, loop=True, counts=[3, 2],
                       scene=[0, 1, 1, 0])
    mv = MovingRegions.from_hazards(hz)
    assert mv.table.shape == (2, 4, 3, 4) and mv.table.dtype == f32 and np.array_equal(mv.table[..., :3], hz.table)
    assert np.all(mv.table[..., 3] == 0) and np.all(mv.kinds == R.SPEC_CIRCLE)
    assert (mv.frame_steps, mv.loop, mv.n_frames, mv.n_scenes, mv.max_regions) == (3, True, 4, 2, 3)
    assert np.array_equal(mv.counts, hz.counts) and np.array_equal(mv.scene, hz.scene)
    assert [mv.frame_at(t) for t in (0, 1, 3, 4, 12, 13)] == [hz.frame_index(max(t - 1, 0)) for t in (0, 1, 3, 4, 12, 13)] == [0, 0, 0, 1, 3, 0]
    with pytest.raises(TypeError, match="takes a MovingHazards"):
        MovingRegions.from_hazards(R.Hazards(np.zeros((2, 2))))
    static = Regions(rng.uniform(-1, 1, (2, 2, 4)) * [1, 1, 0, 0] + [0, 0, 0.2, 0.1], [0, 1], scene=[0, 1, 1, 0])
    both = MovingRegions.join(static, mv)
    assert both.table.shape == (2, 4, 5, 4) and np.array_equal(both.counts, [5, 4]) and np.array_equal(both.scene, hz.scene)
    assert all(np.array_equal(both.table[:, f, :2], static.table) for f in range(4)) and np.array_equal(both.table[:, :, 2:], mv.table)
    assert np.array_equal(both.kinds, [[0, 1, 1, 1, 1]] * 2) and (both.frame_steps, both.loop) == (3, True)
    # a clause over the joined table reads what the two tables read apart
    path = walks(1, n=4, samples=20)
    j = Spec(both, [Spec.always(outside(0, 2)), Spec.always(outside(2, 5), a=1)])
    s, m = Spec(static, [Spec.always(outside(0, 2))]), Spec(mv, [Spec.always(outside(0, 3), a=1)])
    got = spec_fold(spec_start(4, j), path, j)
    assert np.array_equal(bits(got.val[:, 0]), bits(spec_fold(spec_start(4, s), path, s).val[:, 0]))
    assert np.array_equal(bits(got.val[:, 1]), bits(spec_fold(spec_start(4, m), path, m).val[:, 0]))
    with pytest.raises(ValueError, match="static counts must all equal the 2 static regions"):
        MovingRegions.join(Regions(static.table, [0, 1], counts=[2, 1], scene=[0, 1, 1, 0]), mv)
    with pytest.raises(ValueError, match="same scene index"):
        MovingRegions.join(Regions(static.table, [0, 1], scene=[0, 1, 0, 1]), mv)
    with pytest.raises(ValueError, match="1 scenes, the moving ones 2"):
        MovingRegions.join(Regions(static.table[0], [0, 1]), mv)
    with pytest.raises(ValueError, match="same scene index"):
        MovingRegions.join(Regions(static.table[0], [0, 1]), MovingRegions(mv.table[:1], mv.kinds[:1], scene=[0, 0]))
    with pytest.raises(TypeError, match="join takes"):
        MovingRegions.join(mv, mv)


# ---- splits ----------------------------------------------------------------------------------------------------------------------------
def split_case(frame_steps, loop, n=8, size=4):
    path = walks(11, n=n, samples=13)
    cl = [Spec.always(outside(0, 3), 2, 9), Spec.until(outside(1), inside(0)), Spec.stay(inside(0, 2), 3), Spec.recur(inside(2), 11, 1),
          Spec.always(apart(0.2)), Spec.stay(together(0.6), 5, 0, 6), Spec.recur(apart(0.15), 1), Spec.until(apart(0.05), inside(1, 3), 1)]
    return Spec(moving(3, frame_steps, loop), cl, team_size=size), path


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("frame_steps", [1, 4, 7])
def test_every_split_of_twelve_steps(frame_steps, loop):
    """cuts land on frame boundaries (4 | cut, cut = 7) and off them; the frame depends on the global tau only"""
    spec, path = split_case(frame_steps, loop)
    n = path.shape[1]
    whole = assert_every_split_equals_the_whole(
        lambda p, step0, st: spec_fold(spec_start(n, spec) if st is None else st, p, spec, step0), spec, path)
    for c in range(spec.n_clauses):
        rho, wit = brute_clause(path, spec, c)
        assert np.array_equal(bits(whole.val[:, c, 0]), bits(rho)) and np.array_equal(whole.wit[:, c], wit), c


# ---- signed zeros through a mate predicate ---------------------------------------------------------------------------------------------
def test_signed_zeros_through_a_mate_predicate_in_stay_and_recur():
    """two mates exactly d apart: together reads +0.0 and apart -0.0; the inner extremum is taken in the order of the bits"""
    NEG0, POS0 = 0x80000000, 0x00000000

    def run(*gaps):
        return np.array([[[0.0, 0.0], [g, 0.0]] for g in gaps], f32)
    for path, h in [(run(1.0, 1.0, 0.5), 1), (run(0.5, 1.0, 1.0, 0.5), 2)]:
        spec = Spec(Regions(np.zeros((0, 4)), []), [Spec.stay(together(1.0), h), Spec.recur(together(1.0), h), Spec.stay(apart(1.0), h),
                                                    Spec.recur(apart(1.0), h), Spec.always(together(1.0)), Spec.eventually(apart(1.0))],
                    team_size=2)
        st = spec_fold(spec_start(2, spec), path, spec)
        # together: values +0.0 and +0.5: the stay's best minimum is +0.0; the recur's worst maximum +0.0 (h = 1) or +0.5 (h = 2)
        # apart: values -0.0 and -0.5
        want = [POS0, POS0 if h == 1 else 0x3F000000, 0xBF000000 if h == 2 else NEG0, NEG0, POS0, NEG0]
        assert [int(x) for x in bits(st.val[0, :, 0])] == want, (h, st.val[0, :, 0])
        assert np.array_equal(bits(st.val[0]), bits(st.val[1]))              # the distance is symmetric
        for c in range(6):
            rho, wit = brute_clause(path, spec, c)
            assert np.array_equal(bits(st.val[:, c, 0]), bits(rho)) and np.array_equal(st.wit[:, c], wit)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    ok = frames(3)[0]
    for rows, msg in [(np.zeros((3, 4)), r"\[F, R, 4\] or \[S, F, R, 4\]"), (np.zeros((2, 3, 5)), r"\[F, R, 4\]"),
                      (np.zeros((0, 3, 4)), "at least one frame"), (np.zeros((0, 2, 3, 4)), "at least one scene"),
                      (np.zeros((2, 65, 4)), "at most 64 regions")]:
        with pytest.raises(ValueError, match=msg):
            MovingRegions(rows, np.zeros(rows.shape[-2], np.int32))
    assert R.SPEC_FRAMES_MAX_BYTES == 64 << 20
    with pytest.raises(ValueError, match=r"exceed the cap of 67108864 bytes \(64 MiB\)"):
        MovingRegions(np.broadcast_to(f32(0), (65537, 64, 4)), np.zeros(64, np.int32))
    for bad in (0, -1, 1.5, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="frame_steps must"):
            MovingRegions(ok, KINDS, frame_steps=bad)
    for f, r, k, v, msg in [(2, 1, 0, np.nan, "finite"), (1, 0, 1, np.inf, "finite"), (2, 0, 2, -0.1, ">= 0"), (1, 0, 3, -0.1, ">= 0"),
                            (2, 2, 2, -1.0, ">= 0")]:
        rows = ok.copy()
        rows[f, r, k] = v
        with pytest.raises(ValueError, match=msg):                           # Regions' checks, in a frame that is not the first
            MovingRegions(rows, KINDS)
    rows = ok.copy()
    rows[2, 1, 3] = -5.0                                                     # (a circle's fourth column is not an extent)
    MovingRegions(rows, KINDS)
    with pytest.raises(ValueError, match="kinds must be 0"):
        MovingRegions(ok, [0, 1, 2])
    with pytest.raises(ValueError, match="kinds must be"):
        MovingRegions(ok, [0, 1])
    with pytest.raises(ValueError, match="counts must be"):
        MovingRegions(ok, KINDS, counts=[4])
    with pytest.raises(ValueError, match="scene index per robot"):
        MovingRegions(frames(2, S=2), KINDS)
    with pytest.raises(ValueError, match="scene indices"):
        MovingRegions(frames(2, S=2), KINDS, scene=[0, 2])
    mv = MovingRegions(frames(2, S=2), KINDS, scene=[0, 1, 1])
    with pytest.raises(ValueError, match="3 entries|must have 4 entries"):
        mv.check_robots(4)
    # the mate predicates and the team size
    for bad in (-0.1, np.nan, np.inf, 1e39):
        for pred in (together, apart):
            with pytest.raises(ValueError, match="finite and >= 0"):
                pred(bad)
    assert together(0.1)[2] == float(f32(0.1)) != 0.1 and apart(0)[1:] == (R.SPEC_PRED_APART, 0.0)
    assert inside(1, 3) == (1, 3, False) and outside(2) == (2, 3, True)       # what they returned before
    for bad in (0, 3, 32, 2.0, True, None):
        with pytest.raises(ValueError, match=r"team_size must be one of \(1, 2, 4, 8, 16\)"):
            Spec(mv, [Spec.always(apart(0.1))], team_size=bad)
    with pytest.raises(TypeError, match="regions must be"):
        Spec(MovingHazards(np.zeros((1, 1, 2))), [Spec.always(apart(0.1))])
    with pytest.raises(TypeError, match="predicate"):
        Spec(mv, [(R.SPEC_ALWAYS, 0, 5, ("mates", 3, 0.5), ("mates", 3, 0.5))])
    with pytest.raises(ValueError, match=r"region range \[0, 4\) outside 0 .. 3"):
        Spec(mv, [Spec.always(apart(0.1)), Spec.always(inside(0, 4))])
    spec = Spec(Regions(ok[0], KINDS), [Spec.always(apart(0.1))], team_size=4)
    assert spec.dynamic and spec.mates and not spec.moving
    with pytest.raises(ValueError, match="6 robots do not split into the specification's teams of 4"):
        spec_fold(spec_start(6, spec), walks(1, n=6, samples=3), spec)
    with pytest.raises(ValueError, match="teams of 4"):
        spec.check_robots(6)
    spec.check_robots(8)
    # a mate predicate with team_size 1 is legal and reads +inf
    alone = Spec(Regions(ok[0], KINDS), [Spec.always(apart(0.1)), Spec.eventually(together(0.1)), Spec.stay(apart(0.3), 2)])
    st = spec_fold(spec_start(5, alone), walks(1, n=5, samples=6), alone)
    assert alone.dynamic and np.all(st.val[:, 0, 0] == INF) and np.all(st.val[:, 1:, 0] == INF) and np.all(st.wit[:, 0] == -1)
    # a specification without either is the object it was
    plain = Spec(Regions(ok[0], KINDS), [Spec.always(outside(0)), Spec.stay(inside(1), 2)])
    assert not plain.dynamic and plain.team_size == 1 and plain.nested and plain.clauses[0] == (0, 0, R.SPEC_OPEN, (0, 1, True), (0, 1, True))
    assert "Not built" in Spec.__doc__ and "team-mates" not in Spec.__doc__.split("Not built")[1] and "velocity" in Spec.__doc__


def test_follow_waypoints_refuses_teams_of_another_size():
    spec = Spec(Regions(np.zeros((0, 4)), []), [Spec.always(apart(0.1))], team_size=4)
    starts, wp = np.zeros((4, 2)), np.array([[1.0, 1.0]])
    with pytest.raises(ValueError, match=r"teams.size = 2 differs from spec.team_size = 4"):
        follow_waypoints(_GoToGoal(), "point", starts, wp, max_steps=3, path_stride=1, spec=spec, teams=Teams(2, 0.1))
    with pytest.raises(ValueError, match="teams of 4"):
        follow_waypoints(_GoToGoal(), "point", np.zeros((6, 2)), wp, max_steps=3, path_stride=1, spec=spec)


# ---- the host loop ---------------------------------------------------------------------------------------------------------------------
def test_host_loop_end_to_end():
    """circling hazards and teams of 2 through follow_waypoints: the verdict is monitor's on the call's own path, three calls end
    on the whole run's bits, and the clause over the hazards never reads above the run's own clearance"""
    hz = MovingHazards.circling([[0.5, 0.5], [-0.3, 0.6]], travel=0.3, size=0.1, n_frames=20, dt=0.3, frame_steps=2, loop=True,
                                indicator=False)
    teams = Teams(2, 0.3)
    reg = MovingRegions.join(Regions([[1.0, 1.0, 0.3, 0.0]], [1]), MovingRegions.from_hazards(hz))
    spec = Spec(reg, [Spec.eventually(inside(0)), Spec.always(outside(1, 3), a=1), Spec.always(apart(teams.separation), a=1),
                      Spec.stay(together(1.0), 4), Spec.until(apart(0.05), inside(0))], team_size=2)
    starts = np.array([[0.0, 0.0], [0.2, -0.4], [-1.0, 0.9], [-0.8, 0.9]])
    wp = np.array([[1.0, 1.0]])
    run = dict(path_stride=1, spec=spec, hazards=hz, teams=teams)
    r = follow_waypoints(_GoToGoal(), "point", starts, wp, max_steps=60, **run)
    want, res = monitor(r["path"], spec)
    assert_same_state(r["state"].spec, want)
    assert_same_result({k: r[k] for k in R.SPEC_RESULT_KEYS}, res)
    for c in range(spec.n_clauses):
        rho, wit = brute_clause(r["path"].astype(f32), spec, c)
        assert np.array_equal(bits(r["spec_rho"][:, c]), bits(rho)) and np.array_equal(r["spec_witness"][:, c], wit), c
    assert np.all(r["spec_rho"][:, 1] <= r["min_clearance"] + 1e-5) and np.all(r["spec_rho"][:, 2] <= r["min_team_clearance"] + 1e-5)
    c = follow_waypoints(_GoToGoal(), "point", starts, wp, max_steps=20, **run)
    for _ in range(2):
        c = follow_waypoints(_GoToGoal(), "point", max_steps=20, state=c["state"], **run)
    assert_same_state(c["state"].spec, want)
    assert_same_result({k: c[k] for k in R.SPEC_RESULT_KEYS}, res)


# ---- the C side ------------------------------------------------------------------------------------------------------------------------
def test_moving_symbol_and_struct_layout(tmp_path):
    """The entry point is declared, exported and bound, the ABI number is unchanged, and sizeof / offsetof of mobrob_spec_moving_t as
    gcc lays the header out are the ctypes mirror's (every field, by name); mobrob_spec_nested_t is a prefix of it."""
    from mobrob_amd import _lib
    header = open(os.path.join(ROOT, "include", "mobrob_ppo.h")).read()
    assert "mobrob_ppo_spec_monitor_moving(" in header and "mobrob_ppo_spec_monitor_moving" in _lib.SYMBOLS
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mobrob_ppo_spec_monitor_moving") and lib.mobrob_ppo_abi_version() == _lib.ABI_VERSION == 3
    names = [n for n, _ in _lib.SpecMovingC._fields_]
    nested = [n for n, _ in _lib.SpecNestedC._fields_]
    assert names[:len(nested)] == nested
    assert names[len(nested):] == ["kind1", "kind2", "rad1", "rad2", "team_size", "n_frames", "frame_steps", "loop"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "mobrob_ppo.h"\nint main(void) {\n'
            '  printf("%zu %zu\\n", sizeof(mobrob_spec_moving_t), sizeof(mobrob_spec_nested_t));\n'
            + "".join(f'  printf("%zu\\n", offsetof(mobrob_spec_moving_t, {n}));\n' for n in names)
            + "".join(f'  printf("%zu\\n", offsetof(mobrob_spec_nested_t, {n}));\n' for n in nested)
            + '  printf("%d %d %d %u\\n", MOBROB_SPEC_PRED_REGIONS, MOBROB_SPEC_PRED_TOGETHER, MOBROB_SPEC_PRED_APART, '
              'MOBROB_SPEC_FRAMES_MAX_BYTES);\n  return 0;\n}\n')
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    k, j = len(names), len(nested)
    assert out[:2] == [ctypes.sizeof(_lib.SpecMovingC), ctypes.sizeof(_lib.SpecNestedC)]
    assert out[2:2 + k] == [getattr(_lib.SpecMovingC, n).offset for n in names]
    assert out[2 + k:2 + k + j] == out[2:2 + j]                              # the nested struct is a prefix
    assert out[2 + k + j:] == [R.SPEC_PRED_REGIONS, R.SPEC_PRED_TOGETHER, R.SPEC_PRED_APART, R.SPEC_FRAMES_MAX_BYTES]
    rc = lib.mobrob_ppo_spec_monitor_moving(None, None, None, 1, 1, 2, 0, None, None, None, 0)
    lib.mobrob_ppo_last_error.restype = ctypes.c_char_p
    assert rc == _lib.ERR_INVALID and b"spec_monitor_moving: null engine" in lib.mobrob_ppo_last_error()
