"""Scenes shared by tests/test_plan_team_rounds_cpu.py and tests/test_plan_team_rounds_gpu.py (no tests here)."""
import numpy as np

from mobrob_amd.envs.goal_rules import TEAM_ROUND_KEYS, Walls
from tests.plan_team_scenes import SPEC32, TEAM_KEYS, centres

ROUNDS_KEYS = TEAM_KEYS + TEAM_ROUND_KEYS
CORRIDOR_TIME = dict(layer_steps=4, layers=64)
CORRIDOR_K = 16
# the corridor by order of the members, listed by robot: (status, cost at reserve 0, cost at reserve 1)
CORRIDOR_TABLE = {(0, 1, 2, 3): ([0, 1, 1, 0], [64, -1, -1, 10], [64, -1, -1, 10]),
                  (1, 2, 0, 3): ([0, 0, 1, 0], [70, 79, -1, 10], [74, 79, -1, 10]),
                  (2, 1, 0, 3): ([0, 0, 0, 0], [78, 85, 120, 10], [86, 90, 120, 10])}


def corridor_case(copies=1):
    """32 cells: two boxes leave row 16 as a corridor one cell wide through the columns 9 .. 22, the only passage between the two
    halves.  One team of 4: members 0 and 1 stop IN the corridor, member 2 has to pass through it, member 3 stays on its side.
    In index order members 1 and 2 are boxed in; with the parked first, twice, everybody has a walk.  copies: that many teams of
    the same robots -> (spec, walls, start, goal)"""
    walls = Walls([[0.0, 1.075, 0.75, 0.925], [0.0, -1.0125, 0.75, 0.9875]], radius=0.05)
    start = centres(SPEC32, [(6, 20), (6, 12), (4, 16), (28, 4)])
    goal = centres(SPEC32, [(16, 16), (19, 16), (28, 16), (28, 6)])
    return SPEC32, walls, np.tile(start, (copies, 1)), np.tile(goal, (copies, 1))


def hopeless_pair():
    """an empty arena at 32 cells, two mates on adjacent start cells: at reserve 1 whoever plans second finds its start cell
    reserved, in either order -> (spec, start, goal)"""
    return SPEC32, centres(SPEC32, [(8, 16), (9, 16)]), centres(SPEC32, [(24, 20), (24, 12)])


def permuted(arr, order, size):
    """rows of arr [n][...] so that position p of team g holds member order[g][p]"""
    n = len(arr)
    return arr[np.arange(n) // size * size + np.asarray(order).ravel()]
