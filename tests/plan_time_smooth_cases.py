"""Cases and helpers shared by tests/test_plan_time_smooth_cpu.py and tests/test_plan_time_smooth_gpu.py (no tests here)."""
import numpy as np

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import GridSpec, MovingHazards
from tests.plan_scenes import EXTENT, INFLATE, robots33, three_hazards, two_scenes
from tests.plan_time_scenes import FAR, circling33, gap_case, goal_sitter

SMOOTH_KEYS = ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "moves", "field_of",
               "field_goal_cell", "field_scene")


def scenes():
    """name -> (spec, walls, hazards, start, goal, layer_steps, layers): the scenes whose counts DESIGN 4.12.4 records"""
    spec, walls, hz, _, start, goal = circling33()
    gs, gw, gh, gstart, ggoal = gap_case()
    ss, sh, sstart, sgoal = goal_sitter()
    return {"circling33_3_64": (spec, walls, hz, start, goal, 3, 64), "circling33_10_32": (spec, walls, hz, start, goal, 10, 32),
            "gap_case": (gs, gw, gh, gstart, ggoal, 10, 16), "goal_sitter": (ss, None, sh, sstart, sgoal, 10, 16)}


def kept_and_cells(plan, spec, start, goal, i):
    """robot i of a smoothed rule plan with next_blocked -> (cells c[0 .. A], actions, kept action indices); ([], [], []) without a walk"""
    f = plan["field_of"][i]
    s = plan["field_scene"][f]
    cells, acts, status = R.grid_walk_time(plan["fields"][f], plan["occupancy"][s], spec, start[i], goal[i])
    if status == R.UNREACHABLE:
        return [], [], []
    return cells, acts, R.grid_smooth_time(cells, plan["next_blocked"][s])


def static_twin():
    """robots33 among three_hazards, static and as a MovingHazards of one frame -> (spec, walls, one frame, static hazards, start, goal)"""
    scene, start, goal = robots33()
    h3 = three_hazards(scene)
    one = MovingHazards(h3.table[:, None, :, :2].astype(np.float64), size=h3.table[:, :, 2].astype(np.float64), counts=h3.counts, scene=scene)
    return GridSpec(EXTENT, 32, INFLATE), two_scenes(scene), one, h3, start, goal


EDGE_ACTIONS = (63, 64, 65, 127, 128, 129)
EDGE_MOVES = (60, 60, 60, 110, 110, 110)


def window_edges_waiting():
    """G = 128, an empty arena, layer_steps 1: six robots, each straight above a goal of its own (row 10, columns 10, 30 .. 110),
    robot k EDGE_MOVES[k] cells above it.  Hazard k sits on goal k for the first L_k = EDGE_ACTIONS[k] - 2 steps and is parked at FAR
    afterwards (one frame a step, hold).  With size 0.02 and inflate h it blocks the 3 x 3 cells around the goal (the diagonal
    neighbour at 0.0442 <= 0.05125, two cells away at 0.0625 not).  A cell entered by action t must be free in layers t and t + 1, so
    that block is entered by action L_k at the earliest and the goal by action L_k + 1: EDGE_ACTIONS[k] actions at the least.  The
    straight column is the only cheapest path, and a wait (4) is the cheapest way to lose an action (a step aside and back costs 7
    more): every walk has exactly EDGE_MOVES[k] moves and EDGE_ACTIONS[k] - EDGE_MOVES[k] waits INSIDE it, at the edges of a window of 64
    candidates and of the ring of 128 -> (spec, hazards, start [6][2], goal [6][2], layer_steps 1, layers 132)"""
    spec = GridSpec(EXTENT, 128)
    cols = [10 + 20 * k for k in range(6)]
    goal = np.array([(spec.centre(x), spec.centre(10)) for x in cols], np.float32)
    start = np.array([(spec.centre(x), spec.centre(10 + m)) for x, m in zip(cols, EDGE_MOVES)], np.float32)
    frames = np.empty((128, 6, 2))
    frames[:] = FAR
    for k, a in enumerate(EDGE_ACTIONS):
        frames[:a - 2, k] = goal[k]
    return spec, MovingHazards(frames, size=0.02, frame_steps=1), start, goal, 1, 132


def cap_boundary():
    """G = 128, T = 256, 15 fields over 2 scenes: the time fields alone are 15 x 257 x 128 x 128 x 4 bytes = 240.9 MiB and fit
    PLAN_TIME_MAX_BYTES (256 MiB); with the next-blocked table of 2 x 257 x 128 x 128 x 2 bytes = 16.1 MiB they are 257.0 MiB and do not
    -> (spec, hazards of two scenes, start [15][2], goal [15][2] in 15 distinct cells, layer_steps 1, layers 256)"""
    spec = GridSpec(EXTENT, 128)
    scene = np.arange(15) % 2
    goal = np.array([(spec.centre(8 * i + 4), spec.centre(64)) for i in range(15)], np.float32)
    start = np.tile(np.array([[spec.centre(64), spec.centre(20)]], np.float32), (15, 1))
    hazards = MovingHazards(np.full((2, 1, 1, 2), FAR[0]), size=0.02, scene=scene)
    assert 15 * 257 * 128 * 128 * 4 <= R.PLAN_TIME_MAX_BYTES < (15 * 4 + 2 * 2) * 257 * 128 * 128
    return spec, hazards, start, goal, 1, 256
