#!/usr/bin/env python3
"""Generate tests/golden/gremlin_cases.npz by executing the reference's own gremlin motion (run in the BUILD container only).

Needs /root/reference (read-only).  The body of `Engine.set_mocaps` (src/mobrob/envs/mujoco_robots/robots/engine.py) is read
from the reference's source with `ast` at run time and executed on a stand-in `self`: `data.time` is the case's simulation
time, `gremlins_num`, `gremlins_travel` and `gremlins_size` are the case's, and `data.set_mocap_pos` records what it is given.
No MuJoCo call is reached.  Only arrays are written: nothing of the reference's text lands in the repository.

The fixture pins the OFFSET rule only (where a gremlin sits relative to the centre of its circle at simulation time phi).
Adding a placement centre to it is MovingHazards.circling's own.

Arrays (C cases of F frames each; case c, frame j is taken at time phase0[c] + j * dt[c]):
  phase0 [C], dt [C], travel [C], size [C]   float64
  time [C, F]      the simulation time handed to the stand-in (phase0 + j * dt, computed here in float64)
  offset [C, F, 2] x, y of the mocap position the reference sets (float64, the reference's arithmetic)
  z [C, F]         its third component (= gremlins_size)
  same_for_all [C] every gremlin of the case (3 of them) was given the same position
"""
import ast
import os
import types

import numpy as np

REF = "/root/reference/src/mobrob/envs/mujoco_robots/robots/engine.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gremlin_cases.npz")
FRAMES = 16


def reference_set_mocaps():
    tree = ast.parse(open(REF).read())
    eng = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Engine")
    keep = [f for f in eng.body if isinstance(f, ast.FunctionDef) and f.name == "set_mocaps"]
    for f in keep:
        f.decorator_list = []
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF, "exec"), ns)
    return ns["set_mocaps"]


def stand_in(time, num, travel, size, record):
    s = types.SimpleNamespace()
    s.gremlins_num, s.gremlins_travel, s.gremlins_size = num, travel, size
    s.data = types.SimpleNamespace(time=time, set_mocap_pos=lambda name, pos: record.append((name, np.array(pos, np.float64))))
    return s


def cases():
    """(phase0, dt, travel, size)"""
    return [(0.0, 0.05, 0.3, 0.1),                    # the reference's defaults at the goal env's dt
            (0.0, 0.002, 0.3, 0.1),                   # MuJoCo's own time step
            (1.25, 0.1, 0.5, 0.2),
            (0.0, 2.0 * np.pi / FRAMES, 1.0, 0.3),    # one turn in FRAMES frames
            (100.0, 0.7, 0.25, 0.05),                 # a late start, coarse frames (several turns)
            (-3.0, 0.5, 0.3, 0.1)]                    # negative time


def main():
    set_mocaps = reference_set_mocaps()
    cs = cases()
    C = len(cs)
    phase0, dt, travel, size = (np.array([c[k] for c in cs], np.float64) for k in range(4))
    time, offset, z, same = np.zeros((C, FRAMES)), np.zeros((C, FRAMES, 2)), np.zeros((C, FRAMES)), np.ones(C, bool)
    for c, (p0, d, tr, sz) in enumerate(cs):
        for j in range(FRAMES):
            time[c, j] = p0 + j * d
            rec = []
            set_mocaps(stand_in(time[c, j], 3, tr, sz, rec))
            assert [n for n, _ in rec] == [f"gremlin{i}mocap" for i in range(3)]
            same[c] &= all(np.array_equal(rec[0][1], p) for _, p in rec)
            offset[c, j], z[c, j] = rec[0][1][:2], rec[0][1][2]
    rec = []
    set_mocaps(stand_in(1.0, 0, 0.3, 0.1, rec))       # no gremlins: nothing is set
    assert rec == [] and np.all(same) and np.allclose(np.hypot(offset[..., 0], offset[..., 1]), travel[:, None])
    np.savez_compressed(OUT, phase0=phase0, dt=dt, travel=travel, size=size, time=time, offset=offset, z=z, same_for_all=same)
    print(f"{OUT}: {C} cases x {FRAMES} frames")


if __name__ == "__main__":
    main()
