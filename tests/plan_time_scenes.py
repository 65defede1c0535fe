"""Scenes shared by tests/test_plan_time_cpu.py and tests/test_plan_time_gpu.py (no tests here)."""
import numpy as np

from mobrob_amd.envs.goal_rules import GridSpec, MovingHazards, Walls
from tests.plan_scenes import EXTENT, INFLATE, SCENE0, robots33, two_scenes

FAR = (1.9, 1.9)   # outside the enclosure: a hazard parked there blocks nothing a robot can reach


def gap_case(stay=40):
    """SCENE0 at 32 cells; a hazard sits in the one-cell gap of the thin wall (row 19, columns 15 and 16) for `stay` steps and is
    parked at FAR afterwards (hold).  One robot in row 19 from column 12 to column 19: seven moves E, and a wait for the hazard
    -> (spec, walls, hazards, start [1][2], goal [1][2])"""
    spec = GridSpec(EXTENT, 32, INFLATE)
    walls = Walls(SCENE0, radius=0.05)
    y = float(spec.centre(19))
    hazards = MovingHazards(np.array([[[0.0, y]], [FAR]]), size=0.1, frame_steps=stay)
    start = np.array([[spec.centre(12), y]], np.float32)
    goal = np.array([[spec.centre(19), y]], np.float32)
    return spec, walls, hazards, start, goal


def circling33(n_frames=24, frame_steps=3, loop=True):
    """robots33 in the two scenes of plan_scenes with three circling hazards a scene -> (spec, walls, hazards, scene, start, goal)"""
    scene, start, goal = robots33()
    centres = np.array([[[-0.6, -0.8], [0.7, 0.4], [0.0, 0.45]], [[0.5, -0.5], [-0.7, 0.0], [0.0, 0.0]]])
    hazards = MovingHazards.circling(centres, travel=0.3, size=0.1, n_frames=n_frames, dt=2 * np.pi / n_frames, frame_steps=frame_steps,
                                     loop=loop, counts=[3, 2], scene=scene)
    return GridSpec(EXTENT, 32, INFLATE), two_scenes(scene), hazards, scene, start, goal


def goal_sitter(stay=40):
    """An empty arena at 32 cells; a hazard sits on the goal for `stay` steps, then is parked at FAR (hold)
    -> (spec, hazards, start, goal)"""
    spec = GridSpec(EXTENT, 32, INFLATE)
    goal = np.array([[spec.centre(20), spec.centre(16)]], np.float32)
    hazards = MovingHazards(np.array([[goal[0]], [FAR]], np.float64), size=0.1, frame_steps=stay)
    return spec, hazards, np.array([[spec.centre(10), spec.centre(16)]], np.float32), goal


def same_time(dev, ref, keys=("waypoints", "n_waypoints", "count", "status", "cost", "waits", "leave", "arrive", "release", "occupancy",
                              "fields", "field_of", "field_goal_cell", "field_scene")):
    """every key bit for bit; float32 waypoints as uint32"""
    for k in keys:
        a, b = np.ascontiguousarray(dev[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, a.shape, b.dtype, b.shape)
        if k == "waypoints":
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero(a.ravel() != b.ravel())
        assert bad.size == 0, f"{k}: {bad.size} of {a.size} entries differ, first at {bad[:5]}"
