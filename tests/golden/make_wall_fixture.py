#!/usr/bin/env python3
"""Generate tests/golden/wall_cases.npz by executing the reference's own arena layout (run in the BUILD container only).

Needs /root/reference (read-only).  The function `wall_info` (src/mobrob/envs/pybullet_robots/worlds/turtlebot3.py) is read from
the reference's source with `ast` at run time and executed on its own: the module imports pybullet at top level, so it cannot be
imported, and `wall_info` itself calls nothing.  Only arrays are written: nothing of the reference's text lands in the repository.

The arena's own numbers are read from the same source: the keyword arguments of the `create_wall(...)` call in `World._build_world`
are evaluated (they are arithmetic on literals).

Arrays (C cases; case 0 is the reference's arena):
  length [C], thick [C], height [C]   float64 arguments of wall_info
  half_extents [C, 4, 3]              what it returns first  (float64, the reference's arithmetic)
  frame_positions [C, 4, 3]           what it returns second
"""
import ast
import os

import numpy as np

REF = "/root/reference/src/mobrob/envs/pybullet_robots/worlds/turtlebot3.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wall_cases.npz")


def reference_wall_info():
    """-> (wall_info, the arena's (length, thick, height))"""
    tree = ast.parse(open(REF).read())
    keep = [f for f in tree.body if isinstance(f, ast.FunctionDef) and f.name == "wall_info"]
    ns = {}
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF, "exec"), ns)
    call = next(n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "create_wall"
                and any(k.arg == "wall_length" for k in n.keywords))
    kw = {k.arg: eval(compile(ast.Expression(k.value), REF, "eval"), {}) for k in call.keywords if k.arg.startswith("wall_")}
    return ns["wall_info"], (kw["wall_length"], kw["wall_thick"], kw["wall_height"])


def cases(arena):
    """(length, thick, height)"""
    return [arena, (4.0, 0.5, 1.0), (1.0, 0.01, 0.3), (10.0, 2.5, 0.1), (3.3, 0.7, 2.0), (2.0, 2.0, 1.0)]


def main():
    wall_info, arena = reference_wall_info()
    cs = cases(arena)
    C = len(cs)
    length, thick, height = (np.array([c[k] for c in cs], np.float64) for k in range(3))
    half, frame = np.zeros((C, 4, 3)), np.zeros((C, 4, 3))
    for c, (L, t, h) in enumerate(cs):
        he, fp = wall_info(L, t, h)
        half[c], frame[c] = np.array(he, np.float64), np.array(fp, np.float64)
    assert np.all(half >= 0) and np.all(frame[:, :, 2] == 0)
    np.savez_compressed(OUT, length=length, thick=thick, height=height, half_extents=half, frame_positions=frame)
    print(f"{OUT}: {C} cases, arena {arena}")


if __name__ == "__main__":
    main()
