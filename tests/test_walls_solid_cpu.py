"""CPU: the rule of solid walls (goal_rules.wall_block, wall_block_velocity, wall_blocked_fold, goal_propose32): a step's proposed
position resolved against axis-aligned boxes inflated by the robot's radius -- stop and slide, no tunnelling, a start inside an
inflated box can leave it -- and its two guarantees against goal_rules.wall_check."""
import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import (BLOCKED_START, Walls, goal_propose32, wall_block, wall_block_velocity, wall_blocked_fold,
                                        wall_check)

F = np.float32
BOX = np.array([[1.0, 0.0, 0.1, 1.0]], F)                 # a wall across x = 1, faces at 0.9 and 1.1
RADIUS = 0.1                                              # inflated faces at 0.8 and 1.2


def _scalar_block(a, p, boxes, radius):
    """the rule once more, one float32 operation after the other in plain Python loops"""
    ax, ay, px, py = (F(v) for v in (*a, *p))
    rad, half = F(radius), F(0.5)
    holds, inside = [], False
    for cx, cy, hx, hy in np.asarray(boxes, F).reshape(-1, 4):
        Hx, Hy = F(hx + rad), F(hy + rad)
        if abs(F(ax - cx)) <= Hx and abs(F(ay - cy)) <= Hy:
            inside = True
        else:
            holds.append((cx, cy, Hx, Hy))

    def hit(qx, qy):
        ex, ey = F(half * F(qx - ax)), F(half * F(qy - ay))
        sx, sy = F(half * F(ax + qx)), F(half * F(ay + qy))
        for cx, cy, Hx, Hy in holds:
            mx, my = F(sx - cx), F(sy - cy)
            cross = abs(F(F(mx * ey) - F(my * ex)))
            reach = F(F(Hx * abs(ey)) + F(Hy * abs(ex)))
            if not (abs(mx) > F(Hx + abs(ex)) or abs(my) > F(Hy + abs(ey)) or cross > reach):
                return True
        return False
    for code, (qx, qy) in enumerate(((px, py), (px, ay), (ax, py))):
        if not hit(qx, qy):
            return (qx, qy), code, inside
    return (ax, ay), 3, inside


def test_no_walls_and_far_walls_leave_the_step_alone():
    rng = np.random.default_rng(0)
    a, p = rng.uniform(-2, 2, (50, 2)).astype(F), rng.uniform(-2, 2, (50, 2)).astype(F)
    for boxes in (np.zeros((0, 4)), [[50.0, 50.0, 1.0, 1.0], [-40.0, 30.0, 0.5, 2.0]]):
        q, code, inside = wall_block(a, p, boxes, RADIUS)
        assert q.dtype == F and np.array_equal(q.view(np.uint32), p.view(np.uint32)) and not code.any() and not inside.any()
    q, code, inside = wall_block(a, p, BOX, RADIUS, counts=0)   # a count of 0: the row is not in use
    assert np.array_equal(q, p) and not code.any() and not inside.any()


def test_head_on_move_is_blocked_on_that_axis():
    a, p = np.array([0.7, 0.2], F), np.array([0.85, 0.2], F)      # straight at the inflated face x = 0.8
    q, code, inside = wall_block(a, p, BOX, RADIUS)
    # c1 = (px, ay) is c0 itself (y carries no move) and hits as well; c2 = (ax, py) drops the x move and is clean
    assert code == 2 and not inside and np.array_equal(q, a)
    v = wall_block_velocity(np.array([3.0, -0.0], F), code)
    assert v[0] == 0 and not np.signbit(v[0]) and np.signbit(v[1])   # +0.0 on the dropped axis, the other untouched
    # the same move from the other side, and one that ends short of the inflated face
    q, code, _ = wall_block(np.array([1.3, 0.2], F), np.array([1.15, 0.2], F), BOX, RADIUS)
    assert code == 2 and q[0] == F(1.3)
    q, code, _ = wall_block(a, np.array([0.79, 0.2], F), BOX, RADIUS)
    assert code == 0 and q[0] == F(0.79)


def test_oblique_move_slides():
    a, p = np.array([0.7, 0.2], F), np.array([0.85, 0.3], F)
    q, code, inside = wall_block(a, p, BOX, RADIUS)
    assert code == 2 and not inside and q[0] == a[0] and q[1].view(np.uint32) == p[1].view(np.uint32)
    v = wall_block_velocity(np.array([3.0, 2.0, 1.0], F), code)
    assert v[0] == 0 and not np.signbit(v[0]) and v[1] == 2.0 and v[2] == 1.0
    # along a wall that lies across y: the y move is dropped, x is kept
    box = np.array([[0.0, 1.0, 1.0, 0.1]], F)
    a, p = np.array([0.2, 0.7], F), np.array([0.3, 0.85], F)
    q, code, inside = wall_block(a, p, box, RADIUS)
    assert code == 1 and q[1] == a[1] and q[0].view(np.uint32) == p[0].view(np.uint32)
    v = wall_block_velocity(np.array([3.0, -2.0], F), code)
    assert v[0] == 3.0 and v[1] == 0 and not np.signbit(v[1])


def test_thin_wall_is_not_tunnelled():
    box = np.array([[0.0, 0.0, 1e-4, 5.0]], F)                     # half-thickness 1e-4 across a step of 1e-2
    a, p = np.array([-0.005, 0.3], F), np.array([0.005, 0.3], F)
    q, code, inside = wall_block(a, p, box, 0.0)
    assert code in (2, 3) and q[0] == a[0] and not inside
    assert not wall_check(a, q, box)[3] and wall_check(a, p, box)[3]


def test_a_start_inside_an_inflated_box_leaves_it():
    a = np.array([0.85, 0.0], F)                                   # between the inflated face 0.8 and the wall's own face 0.9
    q, code, inside = wall_block(a, np.array([0.6, 0.0], F), BOX, RADIUS)
    assert inside and code == 0 and q[0] == F(0.6)                 # the wall does not hold: the robot moves out ...
    q2, code2, inside2 = wall_block(q, a, BOX, RADIUS)             # ... and is then held out by the same wall
    assert not inside2 and code2 != 0 and q2[0] == q[0]
    q3, code3, inside3 = wall_block(a, np.array([1.15, 0.0], F), BOX, RADIUS)   # it may even go through: nothing holds it
    assert inside3 and code3 == 0


def test_random_segments_are_never_crossed_and_keep_their_clearance():
    rng = np.random.default_rng(7)
    n, M = 4000, 12                                                # dense scenes and long steps: many blocked steps of every code
    a = rng.uniform(-2, 2, (n, 2)).astype(F)
    p = (a + rng.normal(0, 0.4, (n, 2))).astype(F)
    boxes = np.concatenate([rng.uniform(-2, 2, (n, M, 2)), rng.uniform(0, 0.6, (n, M, 2)) * (rng.random((n, M, 2)) > 0.2)], -1).astype(F)
    counts = rng.integers(0, M + 1, n)
    for radius in (0.0, 0.12):
        q, code, inside = wall_block(a, p, boxes, radius, counts)
        _, clear, _, hit = wall_check(a, q, boxes, radius, counts=counts)
        free = ~inside
        assert free.sum() > n // 4 and (code[free] != 0).sum() > 100 and (code == 3).any() and (code == 1).any() and (code == 2).any()
        assert not hit[free].any()
        assert np.all(clear[free] > -1e-6), clear[free].min()
        taken = np.where(((code == 0) | (code == 1))[:, None] & np.array([True, False]) | ((code == 0) | (code == 2))[:, None] & np.array([False, True]), p, a)
        assert np.array_equal(q.view(np.uint32), taken.view(np.uint32))


def test_agrees_with_a_scalar_restatement():
    rng = np.random.default_rng(3)
    n, M = 400, 5
    a = rng.uniform(-1, 1, (n, 2)).astype(F)
    p = (a + rng.normal(0, 0.2, (n, 2))).astype(F)
    boxes = np.concatenate([rng.uniform(-1, 1, (n, M, 2)), rng.uniform(0, 0.4, (n, M, 2))], -1).astype(F)
    q, code, inside = wall_block(a, p, boxes, 0.05)
    for i in range(n):
        (qx, qy), c, ins = _scalar_block(a[i], p[i], boxes[i], 0.05)
        assert (F(qx).view(np.uint32), F(qy).view(np.uint32), c, ins) == (q[i, 0].view(np.uint32), q[i, 1].view(np.uint32), code[i], inside[i]), i
    assert len(set(code.tolist())) == 4 and inside.any()


def test_blocked_fold():
    code = np.array([[0, 1, 3], [2, 0, 3], [0, 0, 0]])
    inside = np.array([[False, True, False], [False, False, False], [True, False, False]])
    stepped = np.array([[True, True, True], [True, True, False], [True, True, True]])
    rec = wall_blocked_fold(np.tile(BLOCKED_START, (3, 1)), code, inside, stepped, step0=10)
    assert rec.tolist() == [[1, 12, 0, 1], [1, 11, 0, 1], [1, 11, 1, 0]]
    again = wall_blocked_fold(rec, code[:1], inside[:1], stepped[:1], step0=13)
    assert again.tolist() == [[1, 12, 0, 1], [2, 11, 0, 2], [2, 11, 2, 0]]


def test_goal_propose32_is_the_device_s_update():
    from fractions import Fraction

    def fma(x, y, z):                                              # exact in rationals, rounded once
        return F(float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))))
    rng = np.random.default_rng(5)
    P, A, dt, extent = 3, 4, F(0.05), F(3.0)
    mix = np.zeros((3, 32), F)
    mix[:, :A] = rng.standard_normal((3, A)).astype(F)
    for pos, vel, act in ((rng.uniform(-3, 3, 3), rng.normal(0, 1, 3), rng.uniform(-1, 1, A)) for _ in range(6)):
        pos, vel, act = pos.astype(F), vel.astype(F), act.astype(F)
        got_p, got_v = goal_propose32(pos, vel, act, mix[:, :A], dt, extent, P)
        for j in range(P):
            cmd = F(0)
            for k in range(A):
                cmd = fma(mix[j, k], act[k], cmd)
            v = fma(F(0.8), vel[j], F(0.2) * cmd)
            x = min(max(fma(dt, v, pos[j]), -extent), extent)
            assert got_v[j].view(np.uint32) == v.view(np.uint32) and got_p[j].view(np.uint32) == F(x).view(np.uint32)
    p_hi, _ = goal_propose32(np.array([2.99, 0, 0], F), np.array([50.0, 0, 0], F), np.zeros(A, F), mix[:, :A], dt, extent, 2)
    assert p_hi.shape == (2,) and p_hi[0] == extent                # the clamp, and P = 2 of a wider row


def test_walls_keyword():
    w = Walls(BOX, radius=RADIUS)
    assert w.solid is False and Walls(BOX, radius=RADIUS, solid=True).solid is True
    arena = Walls.enclosure(2.0, 0.2, solid=True, radius=RADIUS)
    assert isinstance(arena, Walls) and arena.solid and arena.max_walls == 4
    assert np.array_equal(arena.table[0], Walls.enclosure(2.0, 0.2).astype(F))
    assert Walls.enclosure(2.0, 0.2, solid=False).solid is False
    with pytest.raises(TypeError, match="solid"):
        Walls.enclosure(2.0, 0.2, radius=RADIUS)


def test_host_loop_blocks_and_slides():
    """the host path applies the rule: a robot driven at a wall stops short of it, slides along it and is never across it"""
    from mobrob_amd.envs.wrapper import get_env
    from mobrob_amd.waypoints import follow_waypoints

    class Towards:                                                 # act = least-squares command along the goal direction
        def __init__(self, env):
            self.pinv, self.P = np.linalg.pinv(env.env._mix), env.env.pos_dim

        def predict(self, obs, deterministic=True):
            return np.clip(4.0 * self.pinv @ obs[:self.P], -1, 1), None
    env = get_env("point", terminate_on_goal=False)
    while hasattr(env, "env") and not hasattr(env, "get_pos"):
        env = env.env
    walls = Walls([[1.0, 0.0, 0.1, 3.0]], radius=RADIUS, solid=True)
    start, wp = np.array([[0.0, 0.0]]), np.array([[[2.0, 1.0]]])
    r = follow_waypoints(Towards(env), env, start, wp, max_steps=120, seed=1, walls=walls, path_stride=1)
    free = follow_waypoints(Towards(env), env, start, wp, max_steps=120, seed=1, walls=Walls(walls.table[0], radius=RADIUS), path_stride=1)
    assert free["reached"][0] == 1 and free["crossing_steps"][0] > 0 and "wall_blocked_steps" not in free
    assert r["reached"][0] == 0 and r["crossing_steps"][0] == 0 and r["min_wall_clearance"][0] > -1e-6
    assert r["wall_blocked_steps"][0] > 10 and r["wall_first_blocked"][0] > 1 and r["wall_inside_steps"][0] == 0
    assert r["path"][:, 0, 0].max() <= 0.8 + 1e-6 and r["path"][-1, 0, 1] > 0.5      # short of the inflated face, and it slid up
    assert np.array_equal(r["state"].blocked[0], [r["wall_blocked_steps"][0], r["wall_first_blocked"][0], r["wall_stopped_steps"][0], 0])
    # a run split in two ends where the single call ends
    a = follow_waypoints(Towards(env), env, start, wp, max_steps=50, seed=1, walls=walls)
    b = follow_waypoints(Towards(env), env, max_steps=70, seed=1, walls=walls, state=a["state"])
    assert np.array_equal(b["state"].blocked, r["state"].blocked) and np.array_equal(b["state"].state, r["state"].state)
