"""Scenes shared by tests/test_plan_team_cpu.py and tests/test_plan_team_gpu.py (no tests here)."""
import numpy as np

from mobrob_amd.envs.goal_rules import GridSpec, MovingHazards, Teams, Walls
from tests.plan_scenes import EXTENT, INFLATE, two_scenes
from tests.plan_time_scenes import same_time

TEAM_KEYS = ("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "occupancy", "fields", "field_of",
             "field_goal_cell", "field_scene", "team_clearance", "team_crossings")
SPEC32 = GridSpec(EXTENT, 32, INFLATE)
SEP = 0.1                                     # Teams' separation here: the rule uses the size alone


def centres(spec, cells):
    """cells [n][2] (ix, iy) -> their centres [n][2] float32"""
    cells = np.asarray(cells)
    return np.stack([spec.centre(cells[:, 0]), spec.centre(cells[:, 1])], axis=-1).astype(np.float32)


def swap_case():
    """an empty arena at 32 cells, two mates that swap places along row 16: (8, 16) <-> (24, 16) -> (spec, start, goal)"""
    start = centres(SPEC32, [(8, 16), (24, 16)])
    return SPEC32, start, start[::-1].copy()


def lattice_case():
    """16 starts and 16 goals, 32 distinct cells drawn with default_rng(0) from the lattice [1::3, 1::3] of an empty arena at 32
    cells: one team of 16 -> (spec, start, goal)"""
    lat = np.stack(np.meshgrid(np.arange(32)[1::3], np.arange(32)[1::3]), axis=-1).reshape(-1, 2)
    cells = lat[np.random.default_rng(0).choice(len(lat), 32, replace=False)]
    return SPEC32, centres(SPEC32, cells[:16]), centres(SPEC32, cells[16:])


def circling32(n_frames=24, frame_steps=3, loop=True):
    """32 robots in the two scenes of plan_scenes, robots 0 .. 15 in scene 0 and 16 .. 31 in scene 1 (so that teams of up to 16 stay in
    one scene), with plan_time_scenes.circling33's hazards; starts include a blocked cell and the sealed pocket, goals are shared, so
    mates compete for them -> (spec, walls, hazards, start, goal)"""
    from tests.plan_scenes import IN_WALL, OPEN_LEFT, OPEN_RIGHT, POCKET
    rng = np.random.default_rng(23)
    scene = np.arange(32) // 16
    right, left = np.array([OPEN_RIGHT, (1.3, -0.2), (0.5, 0.25)]), np.array([OPEN_LEFT, (-0.3, 1.3), (-1.3, 0.9)])
    start = rng.uniform(-1.5, 1.5, (32, 2))
    goals = np.where((start[:, :1] > 0), right[np.arange(32) % 3], left[np.arange(32) % 3])   # the tail cuts both arenas at x = 0
    start[1], start[17] = IN_WALL, IN_WALL
    start[5], goals[5], goals[9] = (1.25, -1.25), POCKET, POCKET
    centres_ = np.array([[[-0.6, -0.8], [0.7, 0.4], [0.0, 0.45]], [[0.5, -0.5], [-0.7, 0.0], [0.0, 0.0]]])
    hazards = MovingHazards.circling(centres_, travel=0.3, size=0.1, n_frames=n_frames, dt=2 * np.pi / n_frames, frame_steps=frame_steps,
                                     loop=loop, counts=[3, 2], scene=scene)
    return SPEC32, two_scenes(scene), hazards, start.astype(np.float32), goals.astype(np.float32)


def crossing_goal_case():
    """an empty arena at 32 cells, two mates: member 0 walks row 16 from column 4 to column 28 and passes column 16 at action 12;
    member 1 starts three cells below its goal (16, 16) and could arrive at action 3 -> (spec, start, goal)"""
    return SPEC32, centres(SPEC32, [(4, 16), (16, 13)]), centres(SPEC32, [(28, 16), (16, 16)])


def sealed_case():
    """SCENE0-like arena at 32 cells whose lower right pocket is sealed: member 0's goal lies in the pocket (UNREACHABLE), it is parked
    on the straight line between member 1's start and goal -> (spec, walls, start, goal)"""
    from tests.plan_scenes import POCKET, SCENE0
    walls = Walls(SCENE0, radius=0.05)
    row = 24
    start = centres(SPEC32, [(9, row), (5, row)])
    goal = np.array([POCKET, centres(SPEC32, [(13, row)])[0]], np.float32)
    return SPEC32, walls, start, goal


def teams(size):
    return Teams(size, SEP)


def same_team(dev, ref, keys=TEAM_KEYS):
    same_time(dev, ref, keys)
