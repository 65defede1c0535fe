#!/usr/bin/env python3
"""Generate tests/golden/hazard_cases.npz by executing the reference's own hazard rule (run in the BUILD container only).

Needs /root/reference (read-only).  The bodies of `Engine.cost` and `Engine.dist_xy` (src/mobrob/envs/mujoco_robots/robots/
engine.py) are read from the reference's source with `ast` at run time and executed on a stand-in `self`: `sim.forward` does
nothing, `data.ncon = 0` (the contact loop is empty), `constrain_hazards` is on and every other `constrain_*` flag off,
`world.robot_pos()` returns the case's position and `hazards_pos` the case's layout.  No MuJoCo call is reached on those lines.
Only arrays are written: nothing of the reference's text lands in the repository.

Arrays (C cases, M_max hazard slots; a case uses the first n_hazards[c] rows):
  pos [C, 3]            robot positions (float32 values; z != 0 for the 3-D cases)
  hazards [C, M_max, 2] layouts (float32 values);  n_hazards [C];  size [C] hazards_size;  coef [C] hazards_cost
  cost_shaped [C]       cost_hazards with constrain_indicator False (float64, the reference's arithmetic)
  cost_indicator [C]    cost_hazards with constrain_indicator True
  boundary [C]          the position lies exactly on one hazard's boundary (d == r in float64) and inside none
"""
import ast
import os
import types

import numpy as np

REF = "/root/reference/src/mobrob/envs/mujoco_robots/robots/engine.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hazard_cases.npz")


def reference_methods():
    tree = ast.parse(open(REF).read())
    eng = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Engine")
    keep = [f for f in eng.body if isinstance(f, ast.FunctionDef) and f.name in ("cost", "dist_xy")]
    for f in keep:
        f.decorator_list = []
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF, "exec"), ns)
    return ns["cost"], ns["dist_xy"]


def stand_in(pos, layout, size, coef, indicator, dist_xy):
    s = types.SimpleNamespace()
    s.sim = types.SimpleNamespace(forward=lambda: None)
    s.data = types.SimpleNamespace(ncon=0, contact=[])
    for k in ("vases", "pillars", "buttons", "gremlins"):
        setattr(s, f"constrain_{k}", False)
    s.constrain_vases_velocity = False
    s.constrain_vases_displace = False
    s.vases_velocity_cost = s.vases_displace_cost = 0.0
    s.buttons_timer = 0
    s.constrain_hazards = True
    s.constrain_indicator = indicator
    s.hazards_size, s.hazards_cost = size, coef
    s.hazards_pos = [np.array([h[0], h[1], 0.02]) for h in layout]   # sites carry a z; dist_xy drops it
    s.world = types.SimpleNamespace(robot_pos=lambda: np.asarray(pos, np.float64))
    s.dist_xy = types.MethodType(dist_xy, s)
    return s


def cases():
    f32 = lambda v: np.float32(v).item()   # noqa: E731
    rng = np.random.default_rng(20261016)
    out = []   # (pos[3], layout [[x, y]], size, coef)
    # inside / outside one hazard, 2-D
    out.append(([0.1, 0.05, 0.0], [[0.0, 0.0]], 0.3, 1.0))
    out.append(([1.0, 1.0, 0.0], [[0.0, 0.0]], 0.3, 1.0))
    # exactly on the boundary (dyadic values, so that d == r holds exactly in float32 and float64)
    out.append(([0.375, 0.5, 0.0], [[0.0, 0.0]], 0.625, 1.0))            # 0.375^2 + 0.5^2 = 0.625^2
    out.append(([1.0 + 0.75, -2.0, 0.0], [[1.0, -2.0]], 0.75, 2.0))      # along x
    out.append(([0.5, 0.5 + 0.25, 0.7], [[0.5, 0.5]], 0.25, 1.0))        # along y, z != 0
    # overlapping hazards
    out.append(([0.0, 0.0, 0.0], [[0.1, 0.0], [-0.1, 0.05], [0.0, 0.2], [2.0, 2.0]], 0.3, 1.0))
    out.append(([0.05, -0.02, 0.0], [[0.0, 0.0], [0.0, 0.0]], 0.3, 0.5))
    # 3-D positions with z != 0 (the drone): z plays no part
    out.append(([0.1, 0.1, 2.5], [[0.0, 0.0], [0.3, 0.3]], 0.3, 1.0))
    out.append(([-0.2, 0.15, -1.0], [[0.0, 0.0]], 0.3, 1.0))
    # an empty scene
    out.append(([0.0, 0.0, 0.0], [], 0.3, 1.0))
    # coefficient 0: shaped 0, indicator 0
    out.append(([0.0, 0.0, 0.0], [[0.0, 0.0]], 0.3, 0.0))
    # random scenes in the 6 x 6 arena, 16 hazards, some positions inside
    for i in range(12):
        lay = rng.uniform(-3, 3, (16, 2))
        p = lay[i % 16] + rng.uniform(-0.4, 0.4, 2) if i % 2 == 0 else rng.uniform(-3, 3, 2)
        out.append(([p[0], p[1], rng.uniform(-1, 1) if i % 3 == 0 else 0.0], lay.tolist(), 0.3, 1.0))
    return [([f32(v) for v in p], [[f32(x), f32(y)] for x, y in lay], f32(sz), f32(c)) for p, lay, sz, c in out]


def main():
    cost_fn, dist_xy = reference_methods()
    cs = cases()
    C, Mmax = len(cs), max(max(len(c[1]) for c in cs), 1)
    pos = np.zeros((C, 3), np.float32)
    hz = np.zeros((C, Mmax, 2), np.float32)
    nh, size, coef = np.zeros(C, np.int32), np.zeros(C, np.float32), np.zeros(C, np.float32)
    shaped, ind, boundary = np.zeros(C), np.zeros(C), np.zeros(C, bool)
    for i, (p, lay, sz, c) in enumerate(cs):
        pos[i], nh[i], size[i], coef[i] = p, len(lay), sz, c
        if lay:
            hz[i, : len(lay)] = lay
        shaped[i] = cost_fn(stand_in(p, lay, sz, c, False, dist_xy))["cost_hazards"]
        ind[i] = cost_fn(stand_in(p, lay, sz, c, True, dist_xy))["cost_hazards"]
        d = [np.hypot(p[0] - x, p[1] - y) for x, y in lay]
        boundary[i] = any(v == sz for v in d) and not any(v < sz for v in d)
    assert boundary.sum() == 3 and np.all(shaped[boundary] == 0) and np.all(ind[boundary] == 0)
    np.savez_compressed(OUT, pos=pos, hazards=hz, n_hazards=nh, size=size, coef=coef, cost_shaped=shaped,
                        cost_indicator=ind, boundary=boundary)
    print(f"{OUT}: {C} cases, {int((shaped > 0).sum())} with cost, {int(boundary.sum())} on a boundary")


if __name__ == "__main__":
    main()
