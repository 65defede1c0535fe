"""Scenes for the plans from a specification (tests/test_plan_spec_cpu.py, tests/test_plan_spec_gpu.py): regions, specifications,
starts and goals, made once per parameter set and shared."""
import numpy as np

from mobrob_amd.envs import goal_rules as R

EXTENT = 3.0


def random_scene(seed, M, S=1, n=5, G=32, windows=False, n_avoid=2, walls=True, pos_dim=2, goal=True):
    """S scenes with M station regions (boxes and circles, different per scene), n_avoid keep-out boxes and with `walls` a few walls;
    with S > 1 the scenes use different counts (the last regions of the later scenes are unused).  windows: deadlines, opening times
    and dwells on some stations, pace 3.  -> dict(grid, walls, spec, start, goal, pace, M)"""
    rng = np.random.default_rng(seed)
    grid = R.GridSpec(EXTENT, G)
    Rn = M + n_avoid + (1 if S > 1 else 0)             # one spare region that only scene 0 counts
    rows, kinds = np.zeros((S, Rn, 4)), np.zeros((S, Rn), np.int32)
    for s in range(S):
        for r in range(Rn):
            c = rng.uniform(-2.4, 2.4, 2)
            if r < M:
                kinds[s, r] = rng.integers(0, 2)
                rows[s, r] = (c[0], c[1], rng.uniform(0.3, 0.6), rng.uniform(0.3, 0.6) if kinds[s, r] == 0 else 0.0)
            else:
                rows[s, r] = (c[0], c[1], rng.uniform(0.1, 0.5), rng.uniform(0.1, 0.5))
    counts = np.array([Rn if s == 0 else Rn - 1 for s in range(S)], np.int32) if S > 1 else None
    scene = (np.arange(n) % S).astype(np.int32) if S > 1 else None
    reg = R.Regions(rows if S > 1 else rows[0], kinds if S > 1 else kinds[0], counts, scene)
    clauses = []
    for j in range(M):
        a, b, hold = 0, None, 0
        if windows:
            kind = (j + seed) % 4
            if kind == 0:
                b = int(rng.integers(20, 120))
            elif kind == 1:
                a = int(rng.integers(10, 90))
            elif kind == 2:
                hold = int(rng.integers(1, 12))
        clauses.append(R.Spec.stay(R.inside(j), hold, a, b) if hold else R.Spec.eventually(R.inside(j), a, b))
    if n_avoid:
        clauses.append(R.Spec.always(R.outside(M, Rn)))
    spec = R.Spec(reg, clauses)
    W = None
    if walls:
        boxes = np.zeros((S, 3, 4))
        for s in range(S):
            for w in range(3):
                c = rng.uniform(-2.0, 2.0, 2)
                boxes[s, w] = (c[0], c[1], rng.uniform(0.05, 0.8), rng.uniform(0.05, 0.3))
        W = R.Walls(boxes if S > 1 else boxes[0], radius=0.05, scene=scene)
    start = rng.uniform(-2.8, 2.8, (n, pos_dim)).astype(np.float32)
    gl = rng.uniform(-2.8, 2.8, (n, pos_dim)).astype(np.float32) if goal else None
    return dict(grid=grid, walls=W, spec=spec, start=start, goal=gl, pace=3 if windows else None, M=M)


def run_rule(sc, K=16):
    return R.spec_plan(sc["grid"], sc["walls"], None, sc["spec"], sc["start"], sc["goal"], K, sc["pace"])


def symmetric_scene(n=3):
    """Two stations mirrored about the start: every cost is equal, so the (value, i) rule decides -- the tour 0, 1 and 1, 0 tie in the
    total with no goal (d0 equal, D symmetric), and the end is the lowest j of equal totals: the tour ends at station 0."""
    grid = R.GridSpec(EXTENT, 32)
    h = float(grid.h)
    reg = R.Regions([[-7.5 * h, 0.5 * h, 0.3, 0.3], [8.5 * h, 0.5 * h, 0.3, 0.3]], [0, 0])   # cell centres, 8 cells either side
    spec = R.Spec(reg, [R.Spec.eventually(R.inside(0)), R.Spec.eventually(R.inside(1))])
    start = np.tile(np.array([[0.5 * h, 0.5 * h]], np.float32), (n, 1))
    return dict(grid=grid, walls=None, spec=spec, start=start, goal=None, pace=None, M=2)


def walled_in_scene():
    """Two scenes; in scene 1 the station sits inside a ring of four avoid boxes: its anchor exists, nothing reaches it"""
    grid = R.GridSpec(EXTENT, 32)
    ring = [[1.5, 2.4, 0.9, 0.1], [1.5, 0.6, 0.9, 0.1], [0.6, 1.5, 0.1, 0.9], [2.4, 1.5, 0.1, 0.9]]
    far = [[-2.5, -2.5, 0.05, 0.05]] * 4
    rows = np.array([[[1.5, 1.5, 0.4, 0.4], [-1.5, -1.5, 0.4, 0.4]] + far, [[1.5, 1.5, 0.4, 0.4], [-1.5, -1.5, 0.4, 0.4]] + ring])
    scene = np.array([0, 1, 0, 1, 1], np.int32)
    reg = R.Regions(rows, np.zeros((2, 6), np.int32), None, scene)
    spec = R.Spec(reg, [R.Spec.eventually(R.inside(0)), R.Spec.eventually(R.inside(1)), R.Spec.always(R.outside(2, 6))])
    start = np.array([[0, 0], [0, 0], [-1, 2], [2.8, -2.8], [-2, 0]], np.float32)
    return dict(grid=grid, walls=None, spec=spec, start=start, goal=None, pace=None, M=2)


def deadline_scene():
    """Station 0 far and next to the goal, station 1 off to the side of the way there: the shortest tour is 1 then 0, a deadline on
    station 0 forces 0 then 1 and the way back; an opening time on station 1 later than the arrival there holds the robot (a
    release at the waypoint after it, on the goal leg)."""
    grid = R.GridSpec(EXTENT, 32)
    reg = R.Regions([[2.0, 0.1, 0.4, 0.4], [-1.5, 2.0, 0.4, 0.4]], [0, 0])
    start = np.array([[-2.5, 0.1]], np.float32)
    goal = np.array([[2.6, 0.1]], np.float32)

    def spec(deadline=None, opens=0):
        return R.Spec(reg, [R.Spec.eventually(R.inside(0), 0, deadline), R.Spec.eventually(R.inside(1), opens, None)])
    return grid, spec, start, goal
