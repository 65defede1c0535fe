"""Scenes shared by tests/test_plan_assign_cpu.py and tests/test_plan_assign_gpu.py (no tests here), all at 32 cells.  A scene is a
dict: spec, walls, hazards, start, goal [n][P] float32, size, time (layer_steps / layers, {} in a static scene) and `check`, the
scene's own claim about the rule's result (called by the CPU tests with {objective: grid_assign's dict})."""
import itertools

import numpy as np

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, MovingHazards, Teams, Walls
from tests.plan_scenes import EXTENT, INFLATE, POCKET, SCENE0, arena, two_scenes

SPEC32 = GridSpec(EXTENT, 32, INFLATE)
SEP = 0.1                                     # Teams' separation here: the rule uses the size alone
NONE = R.PLAN_ASSIGN_NONE


def teams(size):
    return Teams(size, SEP)


def centres(cells):
    """cells [n][2] (ix, iy) -> their centres [n][2] float32"""
    cells = np.asarray(cells)
    return np.stack([SPEC32.centre(cells[:, 0]), SPEC32.centre(cells[:, 1])], axis=-1).astype(np.float32)


def scene(walls, hazards, start, goal, size, check, **time):
    return dict(spec=SPEC32, walls=walls, hazards=hazards, start=np.asarray(start, np.float32), goal=np.asarray(goal, np.float32), size=size,
                time=time, check=check)


def matrix(out):
    """assign_matrix with NONE put back, int64"""
    m = out["assign_matrix"].astype(np.int64)
    return np.where(m < 0, NONE, m)


def all_matchings(C):
    """every permutation of one team's matrix C [size][size] -> (perms [size!][size], totals, maxima), vectorised"""
    size = C.shape[0]
    perms = np.array(list(itertools.permutations(range(size))), np.int64)
    picked = C[np.arange(size)[None, :], perms]
    return perms, picked.sum(axis=1), picked.max(axis=1)


def optimum(C, objective):
    """-> (best key, the permutations that reach it): the key is the total, or (max, total) as one integer for the makespan"""
    perms, total, most = all_matchings(np.asarray(C, np.int64))
    key = total if objective == "sum" else most * (np.int64(1) << 32) + total
    return int(key.min()), perms[key == key.min()]


# a thin wall at x = 0 with a gap around y = 0
GAP_WALL = arena([[0.0, -0.95, 0.02, 0.65], [0.0, 0.95, 0.02, 0.65]])


def crossed():
    """Teams of 2, one start on either side of the wall with the gap, each goal on the OTHER member's side: the identity sends both
    through the gap, the matching swaps the goals.  Team 1 is the same team already swapped: it keeps the identity."""
    start = np.array([(-1.0, 0.8), (1.0, -0.8), (-1.0, 0.8), (1.0, -0.8)])
    goal = np.array([(1.0, -0.4), (-1.0, 0.4), (-1.0, 0.4), (1.0, -0.4)])

    def check(outs):
        for out in outs.values():
            assert out["assign"].tolist() == [1, 0, 2, 3] and out["assign_changed"].tolist() == [True, False]
            assert out["assign_identity_total"][0] > out["assign_total"][0] and out["assign_identity_total"][1] == out["assign_total"][1]
    return scene(Walls(GAP_WALL, radius=0.05), None, start, goal, 2, check)


def euclid_greedy(start, goal, size):
    """pairing by straight-line distance, greedily: the closest (member, goal) pair of a team first -> col [n_teams][size]"""
    d = np.linalg.norm(start.reshape(-1, size, 1, 2) - goal.reshape(-1, 1, size, 2), axis=-1)
    col = np.zeros(d.shape[:2], np.int64)
    for t, dt in enumerate(d.copy()):
        for _ in range(size):
            i, j = np.unravel_index(np.argmin(dt), dt.shape)
            col[t, i] = j
            dt[i, :], dt[:, j] = np.inf, np.inf
    return col


def walled():
    """Teams of 4 at a wall along x = 0 that is open only at its top end: the goals just across the wall are the nearest in a straight
    line and the farthest by path.  Greedy pairing by straight-line distance sends all four around the wall."""
    wall = arena([[0.0, -0.45, 0.02, 1.15]])
    start = np.array([(-0.3, -1.2), (-0.3, -0.6), (0.4, 1.3), (0.8, 1.3)])
    goal = np.array([(0.3, -1.2), (0.3, -0.6), (-1.0, -1.2), (-1.0, -0.6)])

    def check(outs):
        out = outs["sum"]
        C = matrix(out)[0]
        greedy = euclid_greedy(start, goal, 4)[0]
        assert int(C[np.arange(4), greedy].sum()) > int(out["assign_total"][0]) and out["assign_changed"][0]
    return scene(Walls(wall, radius=0.05), None, start, goal, 4, check)


def sealed():
    """Teams of 4 in plan_scenes' scene 0, one goal of each team inside the sealed pocket: that column is NONE in every row, so
    every pairing has exactly one pair without a path, and the matching minimises the rest."""
    start = np.array([(-1.3, -1.2), (-0.5, -1.0), (-1.3, 1.0), (-0.4, 0.9), (-1.2, -0.5), (-0.3, -0.3), (-1.4, 0.0), (-0.5, 1.3)])
    goal = np.array([(-0.4, -0.4), (-1.3, 0.9), POCKET, (-0.5, 1.3), POCKET, (-1.3, -1.3), (-0.3, 0.6), (-1.4, 0.6)])

    def check(outs):
        for out in outs.values():
            assert np.all((out["assign_matrix"] < 0).sum(axis=1) == [[0, 0, 4, 0], [4, 0, 0, 0]])
            assert np.all((out["assign_cost"].reshape(2, 4) < 0).sum(axis=1) == 1)
            assert np.all(out["assign_total"] >= NONE) and np.all(out["assign_total"] < 2 * NONE) and np.all(out["assign_max"] == NONE)
    return scene(Walls(SCENE0, radius=0.05), None, start, goal, 4, check)


def tied():
    """An empty arena, mirror-symmetric about its axes; a team of 4 whose starts all lie below all of its goals, ten columns to the
    side: with the chamfer costs every one of the 24 matchings has the same total, the identity among them (and the identity, the
    monotone one, has the least maximum).  The identity must come back.  Team 1 is its mirror image."""
    sy, gy = (10, 11, 13, 14), (16, 18, 19, 21)
    start = centres([(9, y) for y in sy] + [(22, 31 - y) for y in sy])
    goal = centres([(21, y) for y in gy] + [(10, 31 - y) for y in gy])

    def check(outs):
        for obj, out in outs.items():
            for C in matrix(out):
                _, best = optimum(C, obj)
                assert (len(best) == 24 or obj == "makespan") and list(range(4)) in best.tolist()
            assert out["assign"].tolist() == list(range(8)) and not out["assign_changed"].any()
    return scene(None, None, start, goal, 4, check)


TIED2_ASSIGN = {"sum": [2, 0, 1, 3], "makespan": [2, 0, 1, 3]}


def tied2():
    """tied's geometry with the goals handed out in another order: several matchings are optimal and the identity is not one of
    them, so which one comes back is the tie-break of goal_rules.plan_assign_match (the lowest column on equal slack).  The
    result is pinned here as a literal."""
    sy, gy = (12, 13, 15, 22), (17, 19, 10, 21)
    start, goal = centres([(9, y) for y in sy]), centres([(21, y) for y in gy])

    def check(outs):
        for obj, out in outs.items():
            _, best = optimum(matrix(out)[0], "sum")
            assert len(best) > 1 and list(range(4)) not in best.tolist()
            assert out["assign"].tolist() == TIED2_ASSIGN[obj], (obj, out["assign"].tolist(), best.tolist())
    return scene(None, None, start, goal, 4, check)


def same_cell():
    """Teams of 2 whose two goals lie in ONE cell (two equal columns: every matching ties).  Team 0 keeps the identity; in team 1 the
    two goals differ in z alone, three-column positions."""
    start = np.array([(-1.0, -1.0, 0.2), (1.0, 1.0, 0.4), (0.5, -1.0, 0.6), (-0.5, 1.2, 0.8)])
    goal = np.array([(0.03, 0.03, 0.5), (0.09, 0.06, 0.7), (-0.7, 0.3, 0.1), (-0.7, 0.3, 0.9)])

    def check(outs):
        for out in outs.values():
            m = out["assign_matrix"]
            assert np.array_equal(m[:, :, 0], m[:, :, 1]) and not out["assign_changed"].any() and out["goal"].shape == (4, 3)
    return scene(None, None, start, goal, 2, check)


def sixteen():
    """3 teams of 16 in plan_scenes' two wall scenes (teams 0 and 2 in scene 0, team 1 in scene 1, whose halves are separate: pairs
    without a path), seeded starts and goals."""
    rng = np.random.default_rng(41)
    sc = np.repeat([0, 1, 0], 16)
    start, goal = rng.uniform(-1.5, 1.5, (48, 2)), rng.uniform(-1.5, 1.5, (48, 2))

    def check(outs):
        assert outs["sum"]["assign_changed"].all() and np.any(outs["sum"]["assign_matrix"][1] < 0)
    return scene(two_scenes(sc), None, start, goal, 16, check)


def moving():
    """Teams of 4 in plan_scenes' scene 0 with two circling hazards, T = 4 layers of 3 steps: the tail blocks every cell a hazard
    ever covers, layer 0 only what its first frames cover -- the cost map is the tail."""
    hz = MovingHazards.circling(np.array([[-0.9, -0.8], [0.9, -0.1]]), travel=0.35, size=0.15, n_frames=24, dt=2 * np.pi / 24, frame_steps=3,
                                loop=True)
    rng = np.random.default_rng(43)
    start, goal = rng.uniform(-1.5, 1.5, (8, 2)), rng.uniform(-1.5, 1.5, (8, 2))
    time = dict(layer_steps=3, layers=4)

    def check(outs):
        occ = R.grid_occupancy_time(SPEC32, Walls(SCENE0, radius=0.05), hz, 0, 3, 4)
        assert np.any(occ[0, 4] & ~occ[0, 0])
    return scene(Walls(SCENE0, radius=0.05), hz, start, goal, 4, check, **time)


def spread():
    """A team of 4 in an empty arena, seeded, on which the two objectives part: the minimum total takes a larger largest member cost
    than the makespan matching, which pays for its smaller maximum with a larger total."""
    rng = np.random.default_rng(5)
    start, goal = rng.uniform(-1.5, 1.5, (4, 2)), rng.uniform(-1.5, 1.5, (4, 2))

    def check(outs):
        s, m = outs["sum"], outs["makespan"]
        assert s["assign"].tolist() != m["assign"].tolist()
        assert s["assign_total"][0] < m["assign_total"][0] and s["assign_max"][0] > m["assign_max"][0]
    return scene(None, None, start, goal, 4, check)


SCENES = dict(crossed=crossed, walled=walled, sealed=sealed, tied=tied, tied2=tied2, same_cell=same_cell, sixteen=sixteen, moving=moving,
              spread=spread)
OBJECTIVES = R.PLAN_ASSIGN_OBJECTIVES


def rule(sc, objective):
    return R.grid_assign(sc["spec"], sc["walls"], sc["hazards"], sc["start"], sc["goal"], teams(sc["size"]), objective, **sc["time"])


def same_assign(dev, ref):
    """every output array of an assignment, bit for bit (the float32 goals as uint32), the matrix and the potentials included"""
    for k in R.ASSIGN_KEYS + ("assign_matrix",):
        a, b = np.asarray(dev[k]), np.asarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), k
    for a, b in zip(dev["assign_potentials"], ref["assign_potentials"]):
        assert a.dtype == b.dtype == np.int64 and np.array_equal(a, b)


def certificate(out, objective):
    """the dual certificate of the returned potentials on C' (C, or for the makespan C with the entries above assign_max as FORBID):
    u[i] + v[j] <= C'[i][j] everywhere, equality on the matched pairs"""
    C = matrix(out)
    if objective == "makespan":
        C = np.where(C > out["assign_max"].astype(np.int64)[:, None, None], np.int64(R.PLAN_ASSIGN_FORBID), C)
    u, v = out["assign_potentials"]
    g, size = u.shape
    slack = C - u[:, :, None] - v[:, None, :]
    assert np.all(slack >= 0)
    col = out["assign"].reshape(g, size) - (np.arange(g) * size)[:, None]
    assert np.all(slack[np.arange(g)[:, None], np.arange(size)[None, :], col] == 0)
