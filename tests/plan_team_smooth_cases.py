"""Cases and helpers shared by tests/test_plan_team_smooth_cpu.py and tests/test_plan_team_smooth_gpu.py (no tests here)."""
import numpy as np

from mobrob_amd.envs import goal_rules as R
from mobrob_amd.envs.goal_rules import grid_leg_cells, grid_plan_team
from tests.plan_team_scenes import TEAM_KEYS, circling32, crossing_goal_case, lattice_case, same_team, sealed_case, swap_case, teams

SMOOTH_TEAM_KEYS = TEAM_KEYS + ("moves",)


def rule_scenes():
    """name -> (spec, walls, hazards, start, goal, size, layer_steps, layers): the scenes of plan_team_scenes as teams"""
    spec, walls, hz, start, goal = circling32()
    out = {f"circling32_{size}": (spec, walls, hz, start, goal, size, 10, 8) for size in (2, 4, 16)}
    out["swap"] = swap_case()[:1] + (None, None) + swap_case()[1:] + (2, 5, 48)
    out["lattice"] = lattice_case()[:1] + (None, None) + lattice_case()[1:] + (16, 10, 48)
    out["crossing_goal"] = crossing_goal_case()[:1] + (None, None) + crossing_goal_case()[1:] + (2, 10, 24)
    spec, walls, start, goal = sealed_case()
    out["sealed"] = (spec, walls, None, start, goal, 2, 10, 16)
    return out


def rule(case, K, reserve, margin, max_leg, step0=0, **kw):
    spec, walls, hz, start, goal, size, layer_steps, layers = case
    return grid_plan_team(spec, walls, hz, start, goal, K, teams(size), reserve, step0, layer_steps, layers, smooth=True, margin=margin,
                          max_leg=max_leg, **kw)


def where_by_leg_cells(walk, keep, T):
    """The cells a member can be in, a layer at a time, from grid_leg_cells alone and action by action (no use of grid_leg_layers
    or grid_reserve_legs) -> a list of T + 1 sets"""
    A = len(walk) - 1
    anchors = [0] + list(keep) + [A]

    def during(t):
        if t >= A:
            return {tuple(walk[A])}
        a, b = next((a, b) for a, b in zip(anchors[:-1], anchors[1:]) if a <= t < b)
        return {tuple(walk[a]), tuple(walk[b])} if b - a == 1 else set(grid_leg_cells(walk[a], walk[b]))
    sets = [during(t) for t in range(T)]
    tail = set()
    for t in range(min(T, A), A + 1):
        tail |= during(t)
    return sets + [tail]


def brute_clearance(plan, size, T):
    """-> (per team the smallest Chebyshev distance over the pairs of mates that both have a walk (PLAN_NO_PAIR: none), the same
    over the pairs of an earlier parked mate and a later mate with a walk, the number of pairs compared)"""
    n = len(plan["walks"])
    has = [int(s) not in (R.UNREACHABLE, R.UNCONVERGED) for s in plan["status"]]
    where = [where_by_leg_cells(plan["walks"][i], plan["keeps"][i] if has[i] else [], T) for i in range(n)]
    both, parked, pairs = np.full(n // size, R.PLAN_NO_PAIR, np.int64), np.full(n // size, R.PLAN_NO_PAIR, np.int64), 0
    for i in range(n):
        for j in range(i + 1, (i // size + 1) * size):
            if not has[j]:
                continue
            pairs += 1
            d = min(max(abs(p[0] - q[0]), abs(p[1] - q[1])) for t in range(T + 1) for p in where[i][t] for q in where[j][t])
            into = both if has[i] else parked
            into[i // size] = min(into[i // size], d)
    return both, parked, pairs


def smooth_both(engine, case, K, reserve, margin, max_leg, step0=0):
    """the device against the rule, bit for bit: every key of SMOOTH_TEAM_KEYS, keeps and walks"""
    spec, walls, hz, start, goal, size, layer_steps, layers = case
    ref = rule(case, K, reserve, margin, max_leg, step0)
    dev = engine.plan_smooth_team(spec, walls, hz, teams=teams(size), reserve=reserve, start=start, goal=goal, step0=step0, layer_steps=layer_steps,
                                  layers=layers, max_waypoints=K, margin=margin, max_leg=max_leg, want_occupancy=True, want_fields=True,
                                  want_walks=True)
    same_team(dev, ref, SMOOTH_TEAM_KEYS)
    assert dev["walks"] == ref["walks"] and dev["keeps"] == ref["keeps"]
    assert not np.any(dev["status"] == R.UNCONVERGED) and np.all(dev["sweeps"] >= 1) and not np.any(dev["waits"])
    return dev, ref
