"""Scenes shared by tests/test_plan_cpu.py and tests/test_plan_gpu.py (no tests here)."""
import numpy as np

from mobrob_amd.envs.goal_rules import GridSpec, Hazards, MovingHazards, Walls

EXTENT = 2.0


def arena(extra):
    """the enclosure (inner faces at +-1.6) plus the boxes `extra`"""
    return np.concatenate([Walls.enclosure(3.6, 0.2), np.asarray(extra, np.float64).reshape(-1, 4)])


# scene 0: a thin wall at x = 0 with a gap of one cell, a pocket sealed into the lower right corner, a free-standing block;
# scene 1: the thin wall without a gap (the two halves of the arena are separate) and another block
SCENE0 = arena([[0.0, -0.65, 0.02, 0.95], [0.0, 1.1, 0.02, 0.5], [1.2, -1.0, 0.4, 0.02], [0.8, -1.3, 0.02, 0.3], [-0.9, 0.3, 0.25, 0.25]])
SCENE1 = arena([[0.0, 0.0, 0.02, 1.6], [0.9, 0.5, 0.3, 0.1]])
INFLATE = 0.07
POCKET, OPEN_LEFT, OPEN_RIGHT, IN_WALL = (1.2, -1.3), (-1.2, -1.2), (1.2, 1.2), (0.0, -0.5)


def two_scenes(scene):
    """Walls of the two scenes (9 and 6 boxes) with the scene index `scene` [n] per robot"""
    boxes = np.zeros((2, 9, 4))
    boxes[0], boxes[1, :6] = SCENE0, SCENE1
    return Walls(boxes, counts=[9, 6], scene=np.asarray(scene), radius=0.05)


def three_hazards(scene):
    return Hazards(np.array([[[-0.6, -0.8], [0.7, 0.4], [-1.0, 1.1]], [[0.5, -0.5], [-0.7, 0.0], [0.0, 0.0]]]), size=[[0.2, 0.3, 0.15], [0.25, 0.1, 0.0]],
                   counts=[3, 2], scene=np.asarray(scene))


def robots33():
    """33 robots in two scenes, 7 distinct goals shared among them; starts include a blocked cell, the goal's own cell, the sealed
    pocket -> (scene [33], start [33][2], goal [33][2])"""
    rng = np.random.default_rng(17)
    goals = np.array([OPEN_RIGHT, OPEN_LEFT, (-0.3, 1.3), (1.3, -0.2), POCKET, (-1.3, 0.9), (0.5, 0.25)])
    scene = np.arange(33) % 2
    which = np.arange(33) % 7
    start = rng.uniform(-1.5, 1.5, (33, 2))
    start[0], start[1] = IN_WALL, IN_WALL                          # a blocked start cell in both scenes
    start[2], start[3] = goals[which[2]] + 0.01, goals[which[3]] - 0.01   # the goal's own cell
    start[5], start[6] = POCKET, (1.3, -1.35)                      # out of the sealed pocket (scene 1 has none: robot 5 is free there)
    start[4] = (1.25, -1.25)                                       # robot 4 (scene 0) starts inside the pocket and has the pocket as goal
    return scene, start.astype(np.float32), goals[which].astype(np.float32)


def robots8_xyz():
    """8 robots with THREE-column starts and goals in scene 0 at 32 cells: starts left of the thin wall, goals right of it, so every
    path turns at the gap; a plan's waypoints all carry the goal's z.  With K = 4 some plans truncate.  As teams of 2, mates cross on the way to the gap;
    two hazards circle in the lower left and the right half, clear of the gap -> (spec, walls, moving hazards, start [8][3], goal [8][3])"""
    rng = np.random.default_rng(29)
    start = np.concatenate([rng.uniform(-1.5, -0.2, (8, 1)), rng.uniform(-1.5, 1.5, (8, 1)), rng.uniform(0.1, 0.9, (8, 1))], axis=1)
    goal = np.array([OPEN_RIGHT + (0.25,), (1.3, -0.2, 0.5), (0.5, 0.25, 0.75), (-0.3, 1.3, 1.0)])[np.arange(8) % 4]
    hz = MovingHazards.circling(np.array([[-0.9, -0.8], [0.9, -0.3]]), travel=0.3, size=0.1, n_frames=12, dt=2 * np.pi / 12, frame_steps=5, loop=True)
    return GridSpec(EXTENT, 32, INFLATE), Walls(SCENE0, radius=0.05), hz, start.astype(np.float32), goal.astype(np.float32)


def xyz_checked(plan, goal, K):
    """a three-column plan: some robot truncates at K, and every waypoint handed out carries its robot's goal z"""
    assert plan["waypoints"].shape == (len(goal), K, 3) and np.any(plan["status"] == 2) and np.any(plan["status"] == 0)
    for i, nw in enumerate(plan["n_waypoints"]):
        assert np.all(plan["waypoints"][i, :nw, 2] == goal[i, 2]) and not plan["waypoints"][i, nw:].any()
    return plan


def serpentine(cells=64, lanes=15):
    """Walls of a serpentine over the whole arena: `lanes` - 1 thin bars, alternately open at the right and at the left end, so the
    only way from the bottom lane to the top lane runs through every lane -> (GridSpec, Walls, start, goal)"""
    bars, pitch = [], 3.2 / lanes
    for j in range(1, lanes):
        y = -1.6 + j * pitch
        bars.append([-0.2 if j % 2 else 0.2, y, 1.4, 0.01])
    return (GridSpec(EXTENT, cells, 0.04), Walls(arena(bars), radius=0.0), np.array([[-1.5, -1.6 + pitch / 2]], np.float32),
            np.array([[1.5 if lanes % 2 else -1.5, 1.6 - pitch / 2]], np.float32))


def show(occ):
    return "\n".join("".join("#" if v else "." for v in row) for row in occ[::-1])
