"""CPU: the plan from a specification, the NumPy rule itself (goal_rules.spec_plan_parse, spec_plan): against an independent oracle
written here (a plain heap Dijkstra and every one of the M! orders), the stitched walk cell by cell, the single-station case against
grid_plan bit for bit, deadlines, opening times and releases, the tie rule, a walled-in station, the closed loop through spec_fold,
and every refusal by name.  G = 32 and a handful of robots throughout."""
import heapq
import itertools

import numpy as np
import pytest

from mobrob_amd.envs import goal_rules as R
from tests.plan_spec_scenes import deadline_scene, random_scene, run_rule, symmetric_scene, walled_in_scene


def dijkstra(occ, src):
    """cost from the cell src to every cell: 5 / 7 moves, no corner cutting; a dict of reached cells"""
    G = occ.shape[0]
    if occ[src // G, src % G]:
        return {}
    dist, heap = {src: 0}, [(0, src)]
    while heap:
        d, c = heapq.heappop(heap)
        if d > dist[c]:
            continue
        x, y = c % G, c // G
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                nx, ny = x + dx, y + dy
                if (dx == 0 and dy == 0) or not (0 <= nx < G and 0 <= ny < G) or occ[ny, nx]:
                    continue
                if dx and dy and (occ[y, nx] or occ[ny, x]):
                    continue
                nd = d + (7 if dx and dy else 5)
                if nd < dist.get(ny * G + nx, 1 << 60):
                    dist[ny * G + nx] = nd
                    heapq.heappush(heap, (nd, ny * G + nx))
    return dist


def ticks(spec, pace):
    """open, close, dwell per station, from the clauses, independently of spec_plan_ticks"""
    out = []
    for cl in spec.clauses:
        if cl[0] == R.SPEC_ALWAYS:
            continue
        a, b, hold = cl[1], cl[2], (cl[5] if len(cl) == 6 else 0)
        out.append((-(-5 * a // pace), (1 << 24) if b == R.SPEC_OPEN else min(5 * b // pace, 1 << 24), -(-5 * hold // pace)))
    return out


def oracle(sc, out):
    """per robot (best cost or None, the set of orders achieving it) over all M! orders; every station must have an anchor (the
    anchors and the blocked map themselves are held to a float64 restatement in test_the_blocked_map_and_the_anchors_...)"""
    grid, G = sc["grid"], sc["grid"].cells
    n, M = len(sc["start"]), sc["M"]
    tk = ticks(sc["spec"], out["pace"])
    scene = sc["spec"].regions.scene
    res, cache = [], {}
    for r in range(n):
        s = 0 if scene is None else int(scene[r])
        occ = out["occupancy"][s]
        anchors = [int(c) for c in out["station_cell"][s]]
        assert min(anchors) >= 0, "the oracle is for scenes in which every station has an anchor"
        sx, sy = grid.cell_of(sc["start"][r, :2])
        nodes = [int(sy) * G + int(sx)] + anchors
        for c in nodes:
            if c >= 0 and (s, c) not in cache:
                cache[(s, c)] = dijkstra(occ, c)
        gc = None
        if sc["goal"] is not None:
            gx, gy = grid.cell_of(sc["goal"][r, :2])
            gc = int(gy) * G + int(gx)
        best, orders = None, []
        for order in itertools.permutations(range(M)):
            t, at, ok = 0, nodes[0], True
            for j in order:
                d = cache[(s, at)].get(anchors[j])
                if d is None:
                    ok = False
                    break
                t = max(t + d, tk[j][0])
                if t > tk[j][1]:
                    ok = False
                    break
                t, at = t + tk[j][2], anchors[j]
            if ok and gc is not None:
                d = cache[(s, at)].get(gc)
                ok, t = d is not None, t + (d or 0)
            if ok and (best is None or t < best):
                best, orders = t, [order]
            elif ok and t == best:
                orders.append(order)
        res.append((best, orders))
    return res


def walk_cells(sc, out, r):
    """the cells of robot r's stitched walk from its waypoints: straight runs in one of the eight directions; asserts each move"""
    grid, G = sc["grid"], sc["grid"].cells
    scene = sc["spec"].regions.scene
    occ = out["occupancy"][0 if scene is None else int(scene[r])]
    x, y = (int(v) for v in grid.cell_of(sc["start"][r, :2]))
    cells = [(x, y)]
    assert not occ[y, x]
    for k in range(out["count"][r]):
        tx, ty = (int(v) for v in grid.cell_of(out["waypoints"][r, k, :2]))
        dx, dy = tx - x, ty - y
        assert dx == 0 or dy == 0 or abs(dx) == abs(dy), f"robot {r}: waypoint {k} is not on a straight run"
        ux, uy = int(np.sign(dx)), int(np.sign(dy))
        while (x, y) != (tx, ty):
            assert not occ[y + uy, x + ux], f"robot {r}: enters a blocked cell"
            assert not (ux and uy and (occ[y, x + ux] or occ[y + uy, x])), f"robot {r}: cuts a corner"
            x, y = x + ux, y + uy
            cells.append((x, y))
    return cells


# (M, seed, windows, goal): seeds at which every station has an anchor and most robots a tour; for every M without windows (all M!
# orders feasible: the discriminating case) and with them, with and without a goal
CASES = [(1, 1, False, True), (1, 1, True, True), (1, 3, True, False),
         (2, 0, False, True), (2, 1, True, True), (2, 8, True, False),
         (3, 3, False, True), (3, 5, True, True), (3, 1, True, False),
         (4, 4, False, True), (4, 6, False, False), (4, 1, True, True), (4, 6, True, False),
         (5, 1, False, True), (5, 2, False, False), (5, 1, True, True), (5, 2, True, False)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"M{c[0]}-seed{c[1]}{'-windows' if c[2] else ''}{'-goal' if c[3] else ''}")
def planned(request):
    M, seed, windows, goal = request.param
    sc = random_scene(100 * M + seed, M, n=5, windows=windows, goal=goal)
    out = run_rule(sc, K=64)
    assert np.all(out["station_cell"] >= 0) and np.sum(out["status"] == R.PLANNED) >= 4      # the case checks something
    return sc, out


def test_cost_is_the_best_of_all_orders(planned):
    sc, out = planned
    for r, (best, orders) in enumerate(oracle(sc, out)):
        if best is None:
            assert out["status"][r] == R.UNREACHABLE and out["count"][r] == 0 and np.all(out["tour_order"][r] == -1)
            assert not out["waypoints"][r].any() and out["cost"][r] == -1
        else:
            assert out["status"][r] == R.PLANNED and out["cost"][r] == best, (r, out["cost"][r], best)
            assert tuple(out["tour_order"][r]) in orders


def test_the_stitched_walk_is_a_walk(planned):
    sc, out = planned
    grid, G = sc["grid"], sc["grid"].cells
    scene = sc["spec"].regions.scene
    for r in np.nonzero(out["status"] == R.PLANNED)[0]:
        cells = walk_cells(sc, out, r)
        anchors = out["station_cell"][0 if scene is None else int(scene[r])]
        at = 0
        for k, j in enumerate(out["tour_order"][r]):
            a = (int(anchors[j]) % G, int(anchors[j]) // G)
            assert a in cells[at:], f"robot {r}: station {j} is not passed in tour order"
            at = at + cells[at:].index(a)
            w = out["waypoints"][r, out["station_waypoint"][r, k], :2]
            assert np.array_equal(w, np.array([grid.centre(a[0]), grid.centre(a[1])], np.float32))
        # the cost without the waits is the length of the walk
        moves = sum(7 if (a[0] != b[0] and a[1] != b[1]) else 5 for a, b in zip(cells, cells[1:]))
        waits = sum(int(d) for d in out["dwell_c"]) + sum(max(0, int(out["open_c"][j]) - int(e)) for j, e in zip(out["tour_order"][r], out["tour_eta"][r]))
        assert moves <= out["cost"][r] <= moves + waits


def margins64(grid, reg, s):
    """the inside margin of every region of scene s at every cell centre, restated in float64 -> [R][iy][ix]"""
    G = grid.cells
    c = -float(grid.extent) + (np.arange(G) + 0.5) * float(grid.h)
    px, py = np.meshgrid(c, c)
    out = []
    for (cx, cy, e2, e3), kind in zip(reg.table[s].astype(np.float64), reg.kinds[s]):
        dx, dy = px - cx, py - cy
        if kind == R.SPEC_CIRCLE:
            out.append(e2 - np.hypot(dx, dy))
        else:
            qx, qy = np.abs(dx) - e2, np.abs(dy) - e3
            out.append(-(np.hypot(np.maximum(qx, 0), np.maximum(qy, 0)) + np.minimum(np.maximum(qx, qy), 0)))
    return np.array(out)


def test_the_blocked_map_and_the_anchors_against_a_float64_restatement(planned):
    """what the oracle takes from the output -- occupancy, station_cell -- held to the issue's text on its own: a cell is blocked by
    an avoid region with m >= -inflate, the anchor is the free cell of the largest margin.  float64 against float32: cells within
    1e-5 of a threshold are not judged here (test_equality_blocks_... and test_of_equal_margins_... judge the exact cases)."""
    sc, out = planned
    grid, reg, tol = sc["grid"], sc["spec"].regions, 1e-5
    inflate = float(grid.inflate_for(sc["walls"]))
    walls = R.grid_occupancy(grid, sc["walls"], None)
    avoid = [cl[3][:2] for cl in sc["spec"].clauses if cl[0] == R.SPEC_ALWAYS]
    stations = [cl[3][:2] for cl in sc["spec"].clauses if cl[0] != R.SPEC_ALWAYS]
    for s in range(reg.n_scenes):
        m = margins64(grid, reg, s)
        blocked, near = walls[s].copy(), np.zeros_like(walls[s])
        for lo, hi in avoid:
            for r in range(lo, min(hi, int(reg.counts[s]))):
                blocked |= m[r] >= -inflate
                near |= np.abs(m[r] + inflate) < tol
        assert np.array_equal(out["occupancy"][s][~near], blocked[~near])
        free = ~out["occupancy"][s]
        for j, (lo, hi) in enumerate(stations):
            u = np.max(m[lo:min(hi, int(reg.counts[s]))], axis=0)
            best, cell = u[free].max(), int(out["station_cell"][s, j])
            assert abs(float(out["station_margin"][s, j]) - best) < tol and best > tol
            assert free.reshape(-1)[cell] and abs(u.reshape(-1)[cell] - best) < tol


def test_equality_blocks_a_cell_of_an_avoid_region():
    """G = 32 over [-3, 3]: h = 0.1875 and every centre is exact.  A box of half extent h / 2 on the centre of cell (16, 16): two cells
    away along an axis the margin is exactly -0.28125 (= 9 / 32, whose square and its root are exact).  inflate = 0.28125: blocked,
    equality blocks; the next float32 below it: free."""
    at = -3.0 + 16.5 * 0.1875
    reg = R.Regions([[at, at, 0.09375, 0.09375]], [0])
    on = R.spec_plan_occupancy(R.GridSpec(3.0, 32, inflate=0.28125), None, None, reg, [(0, 1)])[0]
    below = R.spec_plan_occupancy(R.GridSpec(3.0, 32, inflate=float(np.nextafter(np.float32(0.28125), np.float32(0)))), None, None, reg, [(0, 1)])[0]
    edge = [(16, 18), (16, 14), (18, 16), (14, 16)]                      # (iy, ix)
    assert all(on[c] for c in edge) and not any(below[c] for c in edge)
    assert on[16, 16] and on[17, 17] and below[17, 17] and not on[16, 19] and not on[18, 18]
    assert on.sum() == 13 and below.sum() == 9                           # the 3 x 3 block and the four edge cells
    assert not R.spec_plan_occupancy(R.GridSpec(3.0, 32, inflate=0.28125), None, None, reg, []).any()
    assert not R.spec_plan_occupancy(R.GridSpec(3.0, 32, inflate=0.28125), None, None, R.Regions([[at, at, 0.09375, 0.09375]], [0], np.array([0])),
                                     [(0, 1)]).any()                   # a region beyond the scene's count blocks nothing


def test_of_equal_margins_the_lowest_cell_is_the_anchor():
    """a station box centred on the edge between cells 15 and 16 of row 16: both have the margin 0.3 - h / 2, computed from the same
    |dx|; the anchor is the lower cell index, and with that cell blocked the other one"""
    grid = R.GridSpec(3.0, 32)
    reg = R.Regions([[0.0, -3.0 + 16.5 * 0.1875, 0.3, 0.3]], [0])
    stations = [(0, 1, 0, R.SPEC_OPEN, 0)]
    occ = np.zeros((1, 32, 32), bool)
    cell, margin = R.spec_plan_stations(grid, reg, stations, occ)
    assert cell[0, 0] == 16 * 32 + 15 and margin[0, 0] == np.float32(0.3) - np.float32(0.09375)
    occ[0, 16, 15] = True
    cell2, margin2 = R.spec_plan_stations(grid, reg, stations, occ)
    assert cell2[0, 0] == 16 * 32 + 16 and margin2[0, 0] == margin[0, 0]
    occ[0] = True
    cell3, margin3 = R.spec_plan_stations(grid, reg, stations, occ)
    assert cell3[0, 0] == -1 and margin3[0, 0] == -np.inf


def test_one_station_is_grid_plan_to_its_anchor_bit_for_bit():
    sc = random_scene(7, 1, n=5, n_avoid=0, goal=False, pos_dim=3)
    out = run_rule(sc, K=8)
    G = sc["grid"].cells
    c = int(out["station_cell"][0, 0])
    goal = sc["start"].copy()
    goal[:, 0], goal[:, 1] = sc["grid"].centre(c % G), sc["grid"].centre(c // G)
    ref = R.grid_plan(sc["grid"], sc["walls"], None, sc["start"], goal, 8)
    for k in ("waypoints", "count", "cost", "n_waypoints", "status"):
        assert np.array_equal(np.ascontiguousarray(out[k]).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)), k


def test_a_deadline_forces_the_longer_order_and_an_opening_time_a_release():
    grid, spec, start, goal = deadline_scene()
    free = R.spec_plan(grid, None, None, spec(), start, goal, 16, 2)
    assert list(free["tour_order"][0]) == [1, 0]
    eta0 = int(free["tour_eta"][0, 1])                                   # station 0 second: too late for a deadline below it
    late = ((eta0 - 1) * 2) // 5                                         # at pace 2 the window closes before that arrival
    forced = R.spec_plan(grid, None, None, spec(deadline=late), start, goal, 16, 2)
    assert forced["status"][0] == R.PLANNED and list(forced["tour_order"][0]) == [0, 1] and forced["cost"][0] > free["cost"][0]
    assert not forced["release"].any()
    opens = 400
    held = R.spec_plan(grid, None, None, spec(deadline=late, opens=opens), start, goal, 16, 2)
    assert list(held["tour_order"][0]) == [0, 1] and held["tour_eta"][0, 1] < 5 * opens // 2
    slot = held["station_waypoint"][0, 1] + 1
    want = np.zeros(16, np.int32)
    want[slot] = opens                                                    # ceil(open_c * pace / 5) with open_c = 5 * 400 / 2
    assert np.array_equal(held["release"][0], want)
    assert held["cost"][0] == 5 * opens // 2 + (forced["cost"][0] - forced["tour_eta"][0, 1])
    impossible = R.spec_plan(grid, None, None, spec(deadline=3), start, goal, 16, 2)
    assert impossible["status"][0] == R.UNREACHABLE and impossible["count"][0] == 0


def test_equal_costs_take_the_order_the_tie_rule_names():
    sc = symmetric_scene()
    out = run_rule(sc)
    assert out["matrix"][0, 0, 1] == out["matrix"][0, 1, 0]
    best, orders = oracle(sc, out)[0]
    assert sorted(orders) == [(0, 1), (1, 0)]                            # a genuine tie
    assert np.all(out["tour_order"] == [1, 0])                          # the end is the lowest j of equal totals


def test_a_walled_in_station_parks_its_scene_only():
    sc = walled_in_scene()
    out = run_rule(sc)
    scene = sc["spec"].regions.scene
    assert np.all(out["station_cell"] >= 0)
    assert np.all(out["matrix"][1, 0, 1] == -1) and out["matrix"][0, 0, 1] > 0
    assert np.array_equal(out["status"], np.where(scene == 1, R.UNREACHABLE, R.PLANNED))


def test_a_station_without_a_free_cell_inside_has_no_anchor():
    grid = R.GridSpec(3.0, 32)
    reg = R.Regions([[1.0, 1.0, 0.3, 0.3], [1.0, 1.0, 0.5, 0.5]], [0, 0])
    spec = R.Spec(reg, [R.Spec.eventually(R.inside(0)), R.Spec.always(R.outside(1))])
    out = R.spec_plan(grid, None, None, spec, np.zeros((2, 2)), None, 4)
    assert out["station_cell"][0, 0] == -1 and np.all(out["status"] == R.UNREACHABLE) and not out["covered"][0, 0]


def follow(sc, out, r, T):
    """a point moved along robot r's waypoints, one cell per `pace` steps, held at a waypoint until the next one's release"""
    grid, pace = sc["grid"], out["pace"]
    pos = sc["start"][r, :2].astype(np.float64)
    path, step = [pos.copy()], 0
    for k in range(out["n_waypoints"][r]):
        while step < out["release"][r, k]:
            path.append(pos.copy())
            step += 1
        w = out["waypoints"][r, k, :2].astype(np.float64)
        ax, ay = grid.cell_of(pos.astype(np.float32))
        bx, by = grid.cell_of(w.astype(np.float32))
        legs = max(abs(int(bx) - int(ax)), abs(int(by) - int(ay)), 1) * pace
        for q in range(1, legs + 1):
            path.append(pos + (w - pos) * q / legs)
        step += legs
        pos = w
    assert len(path) <= T + 1
    return np.array(path + [pos] * (T + 1 - len(path)), np.float32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_plan_followed_at_the_pace_satisfies_the_specification(seed):
    sc = random_scene(40 + seed, 3, n=5, windows=True, walls=False, goal=seed != 2)
    grid = sc["grid"]
    sc["start"][:, :2] = grid.centre(np.stack(grid.cell_of(sc["start"][:, :2]), axis=1))   # starts at cell centres
    out = run_rule(sc, K=64)
    assert np.all(out["station_margin"] > 0)
    ok = np.nonzero(out["status"] == R.PLANNED)[0]
    assert ok.size > 0
    T = 900
    path = np.stack([follow(sc, out, r, T) if r in ok else np.tile(sc["start"][r, :2], (T + 1, 1)) for r in range(len(sc["start"]))], axis=1)
    res = R.spec_result(R.spec_fold(R.spec_start(path.shape[1], sc["spec"]), path, sc["spec"]), sc["spec"])
    assert np.all(res["satisfied"][ok]), (res["robustness"], res["weakest"])


def test_refusals_name_the_clause_and_the_reason():
    reg = R.Regions([[0, 0, 0.3, 0.3], [1, 1, 0.3, 0.3]], [0, 0])
    visit = R.Spec.eventually(R.inside(0))
    for clause, word in ((R.Spec.until(R.outside(1), R.inside(0)), "until"), (R.Spec.recur(R.inside(0), 5), "recur"),
                         (R.Spec.always(R.outside(1), 0, 50), "window"), (R.Spec.always(R.outside(1), 1, None), "window"),
                         (R.Spec.always(R.inside(1)), "inside"), (R.Spec.eventually(R.outside(1)), "outside"),
                         (R.Spec.stay(R.outside(1), 3), "outside"), (R.Spec.eventually(R.together(1.0)), "mate")):
        with pytest.raises(ValueError, match=f"clause 1.*{word}"):
            R.spec_plan_parse(R.Spec(reg, [visit, clause]))
    with pytest.raises(ValueError, match="team_size"):
        R.spec_plan_parse(R.Spec(reg, [visit], team_size=2))
    with pytest.raises(ValueError, match="MovingRegions"):
        R.spec_plan_parse(R.Spec(R.MovingRegions(np.zeros((2, 1, 4)), [0]), [visit]))
    with pytest.raises(ValueError, match="no visit clause"):
        R.spec_plan_parse(R.Spec(reg, [R.Spec.always(R.outside(1))]))
    with pytest.raises(ValueError, match="9 stations"):
        R.spec_plan_parse(R.Spec(reg, [visit] * 9))
    assert R.spec_plan_parse(R.Spec(reg, [R.Spec.stay(R.inside(0, 2), 4, 1, 9), R.Spec.always(R.outside(1)), visit])) == \
        ([(1, 2)], [(0, 2, 1, 9, 4), (0, 1, 0, R.SPEC_OPEN, 0)])
    grid, start = R.GridSpec(3.0, 32), np.zeros((2, 2))
    timed = R.Spec(reg, [R.Spec.eventually(R.inside(0), 0, 50)])
    with pytest.raises(ValueError, match="pace"):
        R.spec_plan(grid, None, None, timed, start, None, 4)
    for pace in (0, 1.5, True):
        with pytest.raises(ValueError, match="pace"):
            R.spec_plan(grid, None, None, timed, start, None, 4, pace)
    with pytest.raises(ValueError, match="station 0.*no move boundary"):
        R.spec_plan(grid, None, None, R.Spec(reg, [R.Spec.eventually(R.inside(0), 1, 1)]), start, None, 4, 3)
    walls2 = R.Walls(np.zeros((2, 1, 4)), scene=np.array([0, 1], np.int32))
    with pytest.raises(ValueError, match="scenes"):
        R.spec_plan(grid, walls2, None, R.Spec(reg, [visit]), start, None, 4)
    reg2 = R.Regions(np.zeros((2, 1, 4)), [0], None, np.array([1, 0], np.int32))
    with pytest.raises(ValueError, match="scene index"):
        R.spec_plan(grid, walls2, None, R.Spec(reg2, [visit]), start, None, 4)
    with pytest.raises(ValueError, match="goal"):
        R.spec_plan(grid, None, None, R.Spec(reg, [visit]), start, np.zeros((3, 2)), 4)


def test_the_planner_refuses_what_a_specification_plan_does_not_take():
    from mobrob_amd.planning import GridPlanner
    reg = R.Regions([[1, 1, 0.4, 0.4]], [0])
    spec = R.Spec(reg, [R.Spec.eventually(R.inside(0), 0, 300)])
    start = np.zeros((2, 2), np.float32)
    for kw, word in ((dict(teams=R.Teams(2, 0.3), layer_steps=4), "teams="), (dict(clearance=(2, 2)), "clearance="), (dict(smooth=True), "smooth="),
                     (dict(hazards=R.MovingHazards(np.zeros((2, 1, 2))), layer_steps=4), "MovingHazards")):
        with pytest.raises(ValueError, match=word):
            GridPlanner("point", cells=32, **kw).plan_spec(start, spec, pace=2)
    planner = GridPlanner("point", cells=32)
    with pytest.raises(ValueError, match="pace"):
        planner.plan_spec(start, spec)
    plan = planner.plan_spec(start, R.Spec(reg, [R.Spec.eventually(R.inside(0), 300, None)]), goal=start, pace=2)
    assert np.all(plan["status"] == R.PLANNED) and isinstance(plan["schedule"], R.Schedule)
    assert planner.plan_spec(start, R.Spec(reg, [R.Spec.eventually(R.inside(0))]))["schedule"] is None


class _Wander:
    """a policy that needs no checkpoint: a fixed action"""

    def predict(self, obs, deterministic=True):
        return np.array([0.6, 0.3]), None


def test_the_follow_example_plans_its_specification(capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mod = importlib.util.spec_from_file_location("follow_cli", os.path.join(root, "examples", "follow.py"))
    cli = importlib.util.module_from_spec(mod)
    mod.loader.exec_module(cli)
    box = np.array([[0.0, 0.0, 0.05, 0.6]])
    kw = dict(max_steps=40, host=True, seed=3, policy=_Wander(), goal=[0.7, 0.7], plan_cells=64, check_spec=True)
    r = cli.follow("point", "ppo", None, 4, walls=box, arena=True, plan_spec=True, spec_hold=3, pace=4, **kw)
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("planned from the specification: ") and out[1].startswith("planned rate: ")
    assert any(ln.startswith("specification satisfied: ") for ln in out) and r["satisfied"].shape == (4,)
    nw = r["state"].n_waypoints
    assert np.any(nw >= 1)
    for i in np.nonzero(nw)[0]:                                          # the plan ends in the station's anchor, inside the reach circle
        assert np.hypot(*(r["state"].waypoints[i, nw[i] - 1, :2] - np.float32([0.7, 0.7]))) < R.REACH_RADIUS
    with pytest.raises(ValueError, match="pace"):                        # a dwell needs the pace
        cli.follow("point", "ppo", None, 4, plan_spec=True, spec_hold=3, **kw)
    with pytest.raises(ValueError, match="--plan-spec needs --check-spec"):
        cli.follow("point", "ppo", None, 4, plan_spec=True, **dict(kw, check_spec=False))
    with pytest.raises(ValueError, match="--pace needs --plan-spec"):
        cli.follow("point", "ppo", None, 4, pace=3, **kw)
