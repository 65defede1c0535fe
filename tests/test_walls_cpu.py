"""CPU: the wall rule (goal_rules.Walls / wall_check / wall_fold) and walls on the host loop of mobrob_amd.waypoints.

wall_check is float32 in the device's order; the reference here is an independent float64 evaluation: the signed distance by cases
(outside: the distance to the nearest point of the box; inside: minus the depth), the crossing by clipping the segment against the
two slabs, with divisions.  Tolerances, for coordinates and extents below 4 (so every intermediate is below 8): a signed distance
takes at most 8 float32 roundings of relative size 2^-24 on quantities below 8, |error| <= 8 x 8 x 2^-24 < 4e-6, asserted as
4e-6 on the clearance; a step's cost is at most 9 such terms, each with one more rounding, summed in float32 (9 more) and scaled
once: |error| <= 9 x (9 + 9 + 1) x 8 x 2^-24 < 1e-4, asserted as 1e-4.  The three separating-axis quantities carry at most 6
roundings on products below 32: < 2e-5.  Samples are kept only when every decision (contact, crossing, which wall is nearest) is at
least 1e-4 from its boundary in float64, so the decisions are compared exactly."""
import os

import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import WALL_START, WALLS_MAX, Walls, wall_check, wall_fold
from mobrob_amd.envs.wrapper import get_env
from mobrob_amd.waypoints import FollowState, follow_waypoints, follow_with_replanning, wall_result

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wall_cases.npz")
COST_TOL, CLEAR_TOL, MARGIN = 1e-4, 4e-6, 1e-4


def test_enclosure_is_the_reference_arena():
    z = np.load(GOLDEN)
    assert len(z["length"]) >= 4
    for c in range(len(z["length"])):
        b = Walls.enclosure(z["length"][c], z["thick"][c])
        assert np.array_equal(b[:, :2], z["frame_positions"][c][:, :2]) and np.array_equal(b[:, 2:], z["half_extents"][c][:, :2])
        moved = Walls.enclosure(z["length"][c], z["thick"][c], centre=(0.5, -2.0))
        assert np.array_equal(moved[:, 2:], b[:, 2:]) and np.allclose(moved[:, :2] - b[:, :2], [0.5, -2.0], atol=1e-15)
    arena = Walls.enclosure()
    assert np.array_equal(arena[:, :2], z["frame_positions"][0][:, :2]) and np.array_equal(arena[:, 2:], z["half_extents"][0][:, :2])
    # the four bars cover the square ring: outer side `length`, the inside free
    L, t = z["length"][0], z["thick"][0]
    w = Walls(arena)
    for x, y, inside in ((0.0, 0.0, False), (L / 2 - t / 2, 0.0, True), (-L / 2 + t / 2, 0.3, True), (L / 2 - 1e-3, L / 2 - 1e-3, True),
                         (-L / 2 + 1e-3, L / 2 - 1e-3, True), (L / 2 + 0.01, 0.0, False), (0.2, -L / 2 + t / 2, True)):
        assert wall_check([x, y], [x, y], w.rows())[3] == inside, (x, y)


def _sdf64(p, b):
    dx, dy = abs(p[0] - b[0]) - b[2], abs(p[1] - b[1]) - b[3]
    if dx > 0 or dy > 0:
        return float(np.hypot(max(dx, 0.0), max(dy, 0.0)))
    return -min(-dx, -dy)


def _clip64(a, p, b):
    """the segment a p meets the closed box b: clip the parameter interval [0, 1] against the two slabs"""
    lo, hi = 0.0, 1.0
    for j in range(2):
        d, mn, mx = p[j] - a[j], b[j] - b[2 + j], b[j] + b[2 + j]
        if d == 0.0:
            if a[j] < mn or a[j] > mx:
                return False
            continue
        t0, t1 = sorted(((mn - a[j]) / d, (mx - a[j]) / d))
        lo, hi = max(lo, t0), min(hi, t1)
    return lo <= hi


def _sat_margins64(a, p, b):
    m, e = 0.5 * (a + p) - b[:2], 0.5 * (p - a)
    return np.array([abs(m[0]) - (b[2] + abs(e[0])), abs(m[1]) - (b[3] + abs(e[1])),
                     abs(m[0] * e[1] - m[1] * e[0]) - (b[2] * abs(e[1]) + b[3] * abs(e[0]))])


@pytest.mark.parametrize("M", [1, 4, 5, 9])
def test_wall_check_against_an_independent_float64_evaluation(M):
    rng = np.random.default_rng(100 + M)
    radius, coef = float(np.float32(0.25)), float(np.float32(1.7))
    kept = contacts = hits = clears = 0
    for trial in range(400):
        boxes = np.concatenate([rng.uniform(-2.5, 2.5, (M, 2)), rng.uniform(0.0, 1.0, (M, 2))], axis=1).astype(np.float32)
        if trial % 5 == 0:
            boxes[rng.integers(M), 2 + rng.integers(2)] = 1e-4                    # a thin wall
        a = rng.uniform(-3.0, 3.0, 2).astype(np.float32)
        p = (a + rng.uniform(-1.5, 1.5, 2) * (rng.random() < 0.8)).astype(np.float32)   # some segments are points
        b64, a64, p64 = boxes.astype(np.float64), a.astype(np.float64), p.astype(np.float64)
        sdf = np.array([_sdf64(p64, b) for b in b64])
        margins = np.array([_sat_margins64(a64, p64, b) for b in b64])
        # away from the decision boundaries: contact, the separating axes, and which wall is nearest.  A separating axis decides
        # only where it separates or where none does: the largest margin of a wall is the one that counts
        order = np.sort(sdf)
        if (np.min(np.abs(sdf - radius)) < MARGIN or np.min(np.abs(np.max(margins, axis=1))) < MARGIN
                or (M > 1 and order[1] - order[0] < MARGIN)):
            continue
        kept += 1
        want_cost = coef * np.sum(np.where(sdf <= radius, radius - sdf, 0.0))
        want_hit = any(_clip64(a64, p64, b) for b in b64)
        cost, clear, wall, hit = wall_check(a, p, boxes, radius, coef, indicator=False)
        assert cost.dtype == np.float32 and clear.dtype == np.float32
        assert abs(float(cost) - want_cost) <= COST_TOL, (trial, cost, want_cost)
        assert abs(float(clear) - (order[0] - radius)) <= CLEAR_TOL and wall == int(np.argmin(sdf))
        assert bool(hit) == want_hit, (trial, margins)
        assert wall_check(a, p, boxes, radius, coef, indicator=True)[0] == float(want_cost > 0)
        contacts, hits, clears = contacts + (want_cost > 0), hits + want_hit, clears + (want_cost == 0 and not want_hit)
    assert kept > 200 and contacts > 10 and hits > 10 and clears > 10


def test_exact_edge_cases():
    box = [[1.0, 0.0, 0.25, 0.5]]
    # sdf == radius: contributes exactly 0, no contact
    cost, clear, wall, hit = wall_check([0.0, 0.0], [0.5, 0.0], box, radius=0.25, coef=3.0, indicator=False)
    assert cost == 0 and clear == 0 and wall == 0 and not hit
    assert wall_check([0.0, 0.0], [0.5, 0.0], box, radius=0.25, coef=3.0, indicator=True)[0] == 0
    rec = wall_fold(np.tile(WALL_START, (1, 1)), [[[0.0, 0.0]]], [[[0.5, 0.0]]], [[True]], Walls(box, radius=0.25, cost=3.0))
    assert np.array_equal(rec, [[0, 0, -1, 0, 0, 0, -1]])
    inside = wall_check([0.0, 0.0], [0.625, 0.0], box, radius=0.25, coef=2.0, indicator=False)
    assert inside[0] == 0.25 and inside[1] == -0.125 and not inside[3]
    # a segment through a thin box with both ends clear
    thin = [[0.0, 0.0, 1e-4, 1.0]]
    cost, clear, wall, hit = wall_check([-0.5, 0.25], [0.5, -0.25], thin, radius=0.1)
    assert hit and cost == 0 and clear > 0.39
    assert not wall_check([-0.5, 0.25], [-0.25, -0.25], thin, radius=0.1)[3]
    # a segment touching a corner: the diagonal x + y = 1.5 meets the box [0, 1]^2 shifted ... in its corner (1, 0.5) only
    assert wall_check([0.5, 1.0], [1.5, 0.0], [[0.5, 0.0, 0.5, 0.5]])[3]
    assert not wall_check([0.5, 1.0 + 2.0 ** -10], [1.5, 2.0 ** -10], [[0.5, 0.0, 0.5, 0.5]])[3]
    assert wall_check([2.0, 0.5], [1.0, 0.5], [[0.5, 0.0, 0.5, 0.5]])[3]             # ends on the corner
    # a == p: a hit iff p is in the closed box
    for p, want in (([1.0, 0.0], True), ([1.25, 0.5], True), ([0.75, -0.5], True), ([1.25 + 2.0 ** -20, 0.0], False),
                    ([1.0, 0.5 + 2.0 ** -20], False), ([0.0, 0.0], False)):
        assert wall_check(p, p, box)[3] == want, p
    # no walls
    cost, clear, wall, hit = wall_check([0.0, 0.0], [1.0, 1.0], np.zeros((0, 4)), radius=0.3)
    assert cost == 0 and np.isposinf(clear) and wall == -1 and not hit
    rec = wall_fold(np.tile(WALL_START, (2, 1)), np.zeros((2, 2, 2)), np.ones((2, 2, 2)), [[True, False]] * 2, Walls(np.zeros((0, 4))))
    assert np.array_equal(rec[0], [0, 0, -1, np.inf, -1, 0, -1]) and np.array_equal(rec[1], WALL_START, equal_nan=True)
    # counts: walls past the scene's count do not exist
    two = np.array([[5.0, 5.0, 0.1, 0.1], [0.0, 0.0, 0.5, 0.5]])
    assert wall_check([0.0, 0.0], [0.0, 0.0], two)[3] and not wall_check([0.0, 0.0], [0.0, 0.0], two, counts=1)[3]


def test_equal_clearances_go_to_the_lowest_index():
    # walls 1 and 2 are mirror images about the robot, wall 0 and 3 further: the tie crosses quarters
    boxes = [[0.0, 5.0, 0.5, 0.5], [1.0, 0.0, 0.25, 0.25], [-1.0, 0.0, 0.25, 0.25], [0.0, -5.0, 0.5, 0.5]]
    assert wall_check([0.0, 0.0], [0.0, 0.0], boxes)[2] == 1
    assert wall_check([0.0, 0.0], [0.0, 0.0], boxes[::-1])[2] == 1
    eight = boxes + [[9.0, 9.0, 0.1, 0.1]] + [[1.0, 0.0, 0.25, 0.25]] + [[9.0, -9.0, 0.1, 0.1]] * 2      # walls 1 and 5: one quarter
    assert wall_check([0.0, 0.0], [0.0, 0.0], eight)[2] == 1


def test_the_sum_runs_over_quarters_in_order():
    """The robot stands on (1, 0) with radius 1; a wall (c, 0, 0, 1) is the line x = c, at the exact distance 1 - c.  `tiny` is
    2^-24 deep (half an ulp of 1), `big` is 1 deep, `far` is out of reach.  Quarter q sums walls q, q + 4, q + 8 in that order, and
    the quarters combine as (p0 + p1) + (p2 + p3): tiny + tiny + big = 1 + 2^-23, big + tiny + tiny = 1, and a tiny in another
    quarter than big's is lost as well."""
    f32 = np.float32
    tiny, big, far = [f32(2.0 ** -24), 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 1.0], [-5.0, 0.0, 0.0, 1.0]

    def total(layout):
        return wall_check([1.0, 0.0], [1.0, 0.0], np.array(layout, f32), radius=1.0, coef=1.0, indicator=False)[0]
    assert total([tiny, far, far, far, tiny, far, far, far, big]) == f32(1.0) + f32(2.0 ** -23)      # quarter 0: tiny, tiny, big
    assert total([big, far, far, far, tiny, far, far, far, tiny]) == f32(1.0)                        # the same set, big first
    assert total([tiny, far, far, far, far, tiny, far, far, big]) == f32(1.0)                        # wall 4 <-> 5: another quarter
    assert total([far, tiny, far, far, far, tiny, far, far, big]) == f32(1.0) + f32(2.0 ** -23)      # both in quarter 1: p0 + p1
    assert total([far, tiny, far, tiny, far, far, far, far, big]) == f32(1.0)                        # quarters 1 and 3: (p0 + p1) first


def test_wall_fold_over_a_split_sequence_equals_the_unsplit_one():
    rng = np.random.default_rng(7)
    T, n = 40, 6
    boxes = np.concatenate([rng.uniform(-2, 2, (2, 5, 2)), rng.uniform(0.05, 0.6, (2, 5, 2))], axis=-1)
    walls = Walls(boxes, counts=[5, 3], scene=rng.integers(0, 2, n), radius=0.2, cost=1.5, indicator=False)
    pts = np.cumsum(rng.uniform(-0.3, 0.3, (T + 1, n, 2)), axis=0).astype(np.float32)
    pre, post = pts[:-1], pts[1:]
    stepped = rng.random((T, n)) < 0.85
    stepped[:, 5] = False
    start = np.tile(WALL_START, (n, 1))
    one = wall_fold(start, pre, post, stepped, walls)
    assert np.any(one[:, 1] > 0) and np.any(one[:, 5] > 0) and np.array_equal(one[5], WALL_START, equal_nan=True)
    for cut in (1, 17, 39):
        two = wall_fold(wall_fold(start, pre[:cut], post[:cut], stepped[:cut], walls), pre[cut:], post[cut:], stepped[cut:], walls, step0=cut)
        assert np.array_equal(one, two, equal_nan=True), cut
    assert np.array_equal(start, np.tile(WALL_START, (n, 1)), equal_nan=True)       # the record given is left alone


class _GoToGoal:
    """predict = the command that heads for the goal at full speed, whatever the noise"""

    def __init__(self, env_name="point"):
        env = get_env(env_name)
        self.P = env.env.pos_dim
        self.A = np.linalg.pinv(env.env._mix)

    def predict(self, obs, deterministic=True):
        v = np.asarray(obs, np.float64)[:self.P]
        return np.clip(self.A @ (v / max(np.linalg.norm(v), 1e-9)), -1.0, 1.0), None


def _corridor():
    """Robot 0 drives through a thin wall on x = 0, robot 1 drives along it 0.15 away, robot 2 is far away, robot 3 is parked."""
    start = np.array([[-1.0, 0.05], [0.15, -1.0], [-1.0, 2.5], [0.0, 0.0]])
    wp = np.array([[[1.0, 0.05]], [[0.15, 1.0]], [[1.0, 2.5]], [[0.0, 0.0]]])
    return start, wp, np.array([1, 1, 1, 0]), Walls([[0.0, 0.0, 1e-3, 1.5]], radius=0.2, cost=2.0, indicator=False)


def test_the_host_loop_reports_a_crossing_and_a_contact_and_nothing_else_changes():
    start, wp, nw, walls = _corridor()
    r = follow_waypoints(_GoToGoal(), "point", start, wp, nw, max_steps=60, seed=1, walls=walls)
    assert r["crossing_steps"][0] >= 1 and r["first_crossing"][0] > 1 and r["contact_steps"][0] > 0
    assert r["crossing_steps"][1] == 0 and r["contact_steps"][1] > 0 and -0.06 < r["min_wall_clearance"][1] < -0.04
    assert r["crossing_steps"][2] == 0 and r["contact_steps"][2] == 0 and r["min_wall_clearance"][2] > 0.5 and r["first_contact"][2] == -1
    assert r["steps"][3] == 0 and np.isnan(r["min_wall_clearance"][3]) and r["closest_wall"][3] == -1
    assert np.array_equal(r["closest_wall"][:3], [0, 0, 0]) and np.array_equal(r["state"].wall[:, 0], r["wall_cost_sum"])
    plain = follow_waypoints(_GoToGoal(), "point", start, wp, nw, max_steps=60, seed=1)
    for k in plain:
        if k not in ("state", "trace", "persistent"):
            assert np.array_equal(plain[k], r[k], equal_nan=True), k
    assert np.array_equal(plain["state"].state, r["state"].state) and plain["state"].wall is None


@pytest.mark.parametrize("split", [(25, 35), (1, 59)])
def test_the_host_loop_carries_the_wall_record_across_calls(split):
    start, wp, nw, walls = _corridor()
    pol = _GoToGoal()
    one = follow_waypoints(pol, "point", start, wp, nw, max_steps=60, seed=1, walls=walls)
    r = None
    for i, steps in enumerate(split):
        r = follow_waypoints(pol, "point", start if i == 0 else None, wp if i == 0 else None, nw if i == 0 else None,
                             max_steps=steps, seed=1, walls=walls, state=None if i == 0 else r["state"])
    assert np.array_equal(one["state"].wall, r["state"].wall, equal_nan=True)
    for k in wall_result(one["state"]):
        assert np.array_equal(one[k], r[k], equal_nan=True), k
    assert one["crossing_steps"][0] >= 1


def test_replan_and_copy_keep_the_wall_record_and_the_loop_takes_walls():
    start, wp, nw, walls = _corridor()
    pol = _GoToGoal()
    st = follow_waypoints(pol, "point", start, wp, nw, max_steps=40, seed=1, walls=walls)["state"]
    kept = st.wall.copy()
    assert np.any(kept[:, 5] > 0) and st.copy().wall is not st.wall and np.array_equal(st.copy().wall, kept, equal_nan=True)
    st.replan([0], np.array([[-1.0, 0.05]]))
    assert np.array_equal(st.wall, kept, equal_nan=True)
    assert np.array_equal(FollowState(start, wp, nw, walls=True).wall, np.tile(WALL_START, (4, 1)), equal_nan=True)
    out = follow_with_replanning(pol, "point", start, wp, lambda pos, status, reached: {}, horizon=30, rounds=2, n_waypoints=nw,
                                 seed=1, walls=walls)
    one = follow_waypoints(pol, "point", start, wp, nw, max_steps=60, seed=1, walls=walls)
    assert np.array_equal(out["state"].wall, one["state"].wall, equal_nan=True)


def test_refusals():
    ok = [[0.0, 0.0, 0.5, 0.5]]
    for bad in ([[0.0, 0.0, -0.1, 0.5]], [[0.0, np.nan, 0.1, 0.5]], [[np.inf, 0.0, 0.1, 0.5]], np.zeros((3, 3)), np.zeros((2, 2, 2, 4)),
                np.zeros((WALLS_MAX + 1, 4))):
        with pytest.raises(ValueError):
            Walls(bad)
    Walls(np.zeros((WALLS_MAX, 4)))
    for kw in ({"radius": -0.1}, {"radius": np.nan}, {"cost": -1.0}, {"cost": np.inf}, {"counts": [2]}, {"counts": [0.5]},
               {"scene": [0, 1]}, {"scene": [-1]}, {"scene": [0.0]}):
        with pytest.raises(ValueError):
            Walls(ok, **kw)
    with pytest.raises(ValueError):
        Walls(np.zeros((2, 1, 4)))                                                  # two scenes need a scene index
    Walls(np.zeros((2, 1, 4)), scene=[0, 1, 1]).check_robots(3)
    with pytest.raises(ValueError):
        Walls(np.zeros((2, 1, 4)), scene=[0, 1, 1]).check_robots(4)
    with pytest.raises(ValueError):
        Walls.enclosure(1.0, 2.0)
    with pytest.raises(ValueError):
        wall_check(np.zeros(3), np.zeros(3), ok)
    with pytest.raises(ValueError):
        wall_fold(np.zeros((3, 5)), np.zeros((1, 3, 2)), np.zeros((1, 3, 2)), np.ones((1, 3), bool), Walls(ok))
    start, wp, nw, walls = _corridor()
    pol = _GoToGoal()
    with pytest.raises(TypeError):
        follow_waypoints(pol, "point", start, wp, nw, max_steps=5, walls=ok)
    with pytest.raises(ValueError):
        follow_waypoints(pol, "point", start, wp, nw, max_steps=5, walls=Walls(ok, scene=[0, 0]))
    plain = follow_waypoints(pol, "point", start, wp, nw, max_steps=5)
    with pytest.raises(ValueError):                                                 # a run has walls in every call or in none
        follow_waypoints(pol, "point", max_steps=5, state=plain["state"], walls=walls)
    walled = follow_waypoints(pol, "point", start, wp, nw, max_steps=5, walls=walls)
    with pytest.raises(ValueError):
        follow_waypoints(pol, "point", max_steps=5, state=walled["state"])
