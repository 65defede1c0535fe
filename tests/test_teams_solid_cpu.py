"""Solid teams, the rule itself (goal_rules.team_block, team_block_step, team_block_fold): NumPy only.

A mate is one more box of wall_block's rule -- the closed square of half-width `separation` around where it stands --, the order is
serial inside a team, and a pair that was never inside each other keeps its distance.  The device is held to these functions bit
for bit by tests/test_teams_solid_gpu.py."""
import numpy as np
import pytest

from mobrob_amd.envs.goal_rules import (TEAM_BLOCKED_START, Teams, Walls, team_block, team_block_fold, team_block_scalar,
                                        team_block_step, wall_block, wall_blocked_fold, wall_check)

F32 = np.float32
SEP = 0.2


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def test_a_mate_is_wall_blocks_box():
    rng = np.random.default_rng(0)
    n, J = 4000, 5
    a = rng.uniform(-1, 1, (n, 2)).astype(F32)
    p = (a + rng.uniform(-2 * SEP, 2 * SEP, (n, 2))).astype(F32)
    mates = (a[:, None] + rng.uniform(-3 * SEP, 3 * SEP, (n, J, 2))).astype(F32)
    q, code, inside, by_mate, by_wall, wall_inside = team_block(a, p, mates, SEP)
    boxes = np.concatenate([mates, np.full((n, J, 2), F32(SEP))], -1)
    q2, code2, inside2 = wall_block(a, p, boxes, radius=0.0)
    assert np.array_equal(_bits(q), _bits(q2)) and np.array_equal(code, code2) and np.array_equal(inside, inside2)
    assert all(np.sum(code == c) > 20 for c in range(4)) and inside.sum() > 100
    assert np.array_equal(by_mate, code != 0) and not by_wall.any() and not wall_inside.any()
    # no mates: nothing holds
    q, code, inside, *_ = team_block(a, p, np.zeros((n, 0, 2)), SEP)
    assert np.array_equal(_bits(q), _bits(p)) and not code.any() and not inside.any()


def test_walls_and_mates_are_one_list():
    rng = np.random.default_rng(1)
    n, J, M, radius = 3000, 3, 4, 0.05
    a = rng.uniform(-1, 1, (n, 2)).astype(F32)
    p = (a + rng.uniform(-2 * SEP, 2 * SEP, (n, 2))).astype(F32)
    mates = (a[:, None] + rng.uniform(-3 * SEP, 3 * SEP, (n, J, 2))).astype(F32)
    walls = np.concatenate([a[:, None] + rng.uniform(-0.6, 0.6, (n, M, 2)), rng.uniform(0.01, 0.2, (n, M, 2))], -1).astype(F32)
    counts = rng.integers(0, M + 1, n)
    q, code, inside, by_mate, by_wall, wall_inside = team_block(a, p, mates, SEP, walls, radius, counts)
    # the union as ONE wall scene: a mate's square is the box (c, sep - radius) inflated by the radius where that sum is exact
    # -- instead the union is checked through the definition: wall_block on mates + walls gives code and position when the
    # mates' half-widths are handed down unrounded, i.e. with radius 0 and the walls pre-inflated
    infl = walls.copy()
    infl[..., 2:] = walls[..., 2:] + F32(radius)
    infl = np.where((np.arange(M)[None, :] < counts[:, None])[..., None], infl, F32([1e6, 1e6, 0, 0]))
    union = np.concatenate([np.concatenate([mates, np.full((n, J, 2), F32(SEP))], -1), infl], 1)
    q2, code2, inside2 = wall_block(a, p, union, radius=0.0)
    assert np.array_equal(_bits(q), _bits(q2)) and np.array_equal(code, code2) and np.array_equal(inside | wall_inside, inside2)
    assert np.array_equal(by_mate | by_wall, code != 0)
    assert np.sum(by_mate & ~by_wall) > 20 and np.sum(by_wall & ~by_mate) > 20 and np.sum(by_wall & by_mate) > 20
    # the walls alone / the mates alone block no less often than they do in the union's rejected candidates
    _, code_w, _ = wall_block(a, p, walls, radius, counts)
    assert np.all(code_w[by_wall & ~by_mate] != 0)
    _, code_m, *_ = team_block(a, p, mates, SEP)
    assert np.all(code_m[by_mate & ~by_wall] != 0)


def test_scalar_restatement():
    rng = np.random.default_rng(2)
    n, J = 600, 3
    a = rng.uniform(-1, 1, (n, 2)).astype(F32)
    p = (a + rng.uniform(-2 * SEP, 2 * SEP, (n, 2))).astype(F32)
    mates = (a[:, None] + rng.uniform(-2.5 * SEP, 2.5 * SEP, (n, J, 2))).astype(F32)
    q, code, inside, by_mate, *_ = team_block(a, p, mates, SEP)
    for i in range(n):
        (qx, qy), c, ins, bm = team_block_scalar(a[i], p[i], mates[i], SEP)
        assert (c, ins, bm) == (code[i], inside[i], by_mate[i]), i
        assert np.array_equal(_bits([qx, qy]), _bits(q[i])), i


def _serial_by_hand(stand, prop, stepped, G, sep):
    """team_block_step restated robot by robot with the scalar rule -> (positions, codes, pairs inside [n][n], boxes used)"""
    pos = np.array(stand, F32)
    n = len(pos)
    code, pair_inside, used = np.zeros(n, np.int64), np.zeros((n, n), bool), {}
    for i in range(n):                                    # ascending global index = ascending team-local index in every team
        if not stepped[i]:
            continue
        t0 = i - i % G
        mates = [j for j in range(t0, t0 + G) if j != i]
        cj = pos[mates].copy()                             # lower indices: already resolved; higher: still where they stood
        (qx, qy), code[i], _, _ = team_block_scalar(pos[i], prop[i], cj, sep)
        for j, c in zip(mates, cj):
            pair_inside[i, j] = abs(pos[i, 0] - c[0]) <= F32(sep) and abs(pos[i, 1] - c[1]) <= F32(sep)
        used[i] = (pos[i].copy(), mates, cj)
        pos[i] = (qx, qy)
    return pos, code, pair_inside, used


@pytest.mark.parametrize("G", [2, 4, 16])
def test_random_teams_keep_their_distance(G):
    rng = np.random.default_rng(10 + G)
    n, T = 32, 300
    teams = Teams(G, SEP, solid=True)
    # teams side by side, members on a jittered grid a little more than the separation apart
    side = int(np.ceil(np.sqrt(G)))
    local = np.stack([np.arange(G) % side, np.arange(G) // side], 1) * (1.3 * SEP)
    pos = (np.tile(local, (n // G, 1)) + rng.uniform(-0.02, 0.02, (n, 2))).astype(F32)
    ever_inside = np.zeros((n, n), bool)
    record = np.tile(TEAM_BLOCKED_START, (n, 1))
    codes = np.zeros(4, np.int64)
    for t in range(T):
        ang, length = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * SEP, n)
        pull = 0.05 * (local.mean(0)[None] - pos)         # keeps the team together, so the rule keeps biting
        prop = (pos + np.stack([np.cos(ang), np.sin(ang)], 1) * length[:, None] + pull).astype(F32)
        stepped = rng.random(n) < 0.9
        q, code, inside, by_mate, by_wall, wall_inside = team_block_step(pos, prop, stepped, teams)
        want, want_code, pair_inside, used = _serial_by_hand(pos, prop, stepped, G, SEP)
        assert np.array_equal(_bits(q), _bits(want)) and np.array_equal(code, want_code), t
        assert np.array_equal(inside, pair_inside.any(1)) and np.array_equal(by_mate, code != 0) and not by_wall.any()
        ever_inside |= pair_inside | pair_inside.T
        for i, (a, mates, cj) in used.items():                             # exact: the step's segment meets no square that held
            boxes = np.concatenate([cj, np.full((len(mates), 2), F32(SEP))], 1)
            for j, box in zip(mates, boxes):
                if not ever_inside[i, j]:
                    assert not wall_check(a, q[i], box[None], radius=0.0)[3], (t, i, j)
        cheb = np.abs(q[:, None].astype(np.float64) - q[None]).max(-1)
        same = (np.arange(n)[:, None] // G == np.arange(n)[None] // G) & ~np.eye(n, dtype=bool)
        assert np.all(cheb[same & ~ever_inside] > SEP - 1e-6), t
        record = team_block_fold(record, code[None], inside[None], by_mate[None], stepped[None], step0=t)
        codes += np.bincount(code[stepped], minlength=4)
        pos = q
    # (one square alone rarely rejects both slides, so a full stop is only demanded of teams with several mates)
    assert np.all(codes[1:3] > 0) and (G == 2 or codes[3] > 0), codes
    assert record[:, 0].sum() == codes[1:].sum() and record[:, 2].sum() == codes[3] and np.all(record[record[:, 0] > 0, 1] >= 1)
    assert np.sum(same & ~ever_inside) > 0


def _head_on():
    stand = np.array([[-0.25, 0.0], [0.25, 0.0]], F32)
    prop = np.array([[-0.05, 0.0], [0.05, 0.0]], F32)
    return stand, prop


def test_jacobi_counter_example():
    """two mates 0.5 apart step 0.2 towards each other, separation 0.2: tested against the other's PRE-step position both advance
    and end 0.1 apart -- inside each other, where the rule no longer holds them; in the serial order the second one stops"""
    stand, prop = _head_on()
    jac = np.stack([team_block(stand[i], prop[i], stand[None, 1 - i], SEP)[0] for i in range(2)])
    assert np.array_equal(jac, prop) and np.abs(jac[0] - jac[1]).max() <= SEP
    assert team_block(jac[0], jac[0], jac[None, 1], SEP)[2]                # ... so the pair is `inside` from now on
    q, code, inside, by_mate, *_ = team_block_step(stand, prop, np.ones(2, bool), Teams(2, SEP, solid=True))
    assert np.array_equal(q, np.array([[-0.05, 0.0], [0.25, 0.0]], F32)) and code.tolist() == [0, 2]
    assert not inside.any() and by_mate.tolist() == [False, True] and np.abs(q[0] - q[1]).max() > SEP
    assert not team_block(q[1], q[1], q[None, 0], SEP)[2]


def test_the_lower_index_goes_first():
    stand, prop = _head_on()
    teams = Teams(2, SEP, solid=True)
    q, code, *_ = team_block_step(stand, prop, np.ones(2, bool), teams)
    qs, codes, *_ = team_block_step(stand[::-1], prop[::-1], np.ones(2, bool), teams)      # the two members swap their indices
    assert code.tolist() == [0, 2] and codes.tolist() == [0, 2]
    assert np.array_equal(q[0], prop[0]) and np.array_equal(q[1], stand[1])                # the robot on the right yields
    assert np.array_equal(qs[0], prop[1]) and np.array_equal(qs[1], stand[0])              # now the robot on the left does
    # a mate that does not step counts where it stands, and teams never see each other
    q, code, *_ = team_block_step(stand, prop, np.array([False, True]), teams)
    assert np.array_equal(q, np.array([stand[0], prop[1]])) and not code.any()
    q, code, *_ = team_block_step(np.tile(stand, (2, 1)), np.tile(prop, (2, 1)), np.ones(4, bool), Teams(1, SEP, solid=True))
    assert np.array_equal(q, np.tile(prop, (2, 1))) and not code.any()


def test_an_overlapping_start_separates_and_then_holds():
    teams = Teams(4, SEP, solid=True)
    pos = np.array([[0.0, 0.0], [0.05, 0.02], [-0.03, 0.06], [0.04, -0.05]], F32)          # all four inside each other
    out = np.array([[-1.0, -1.0], [1.0, 0.3], [-0.4, 1.0], [0.7, -1.0]])
    out = (0.04 * out / np.linalg.norm(out, axis=1, keepdims=True)).astype(F32)
    inside_steps, apart_at = 0, None
    for t in range(40):                                   # apart: nobody holds anybody while they are inside each other
        q, code, inside, *_ = team_block_step(pos, pos + out, np.ones(4, bool), teams)
        cheb = np.abs(q[:, None] - q[None]).max(-1) + 10 * np.eye(4)
        inside_steps += int(inside.sum())
        pos = q
        if cheb.min() > SEP:
            apart_at = t
            break
    assert apart_at is not None and inside_steps > 0
    blocked = 0
    for t in range(40):                                   # ... and back towards the middle: now they hold each other
        q, code, inside, by_mate, *_ = team_block_step(pos, (pos - out).astype(F32), np.ones(4, bool), teams)
        assert not inside.any()
        cheb = np.abs(q[:, None].astype(np.float64) - q[None]).max(-1) + 10 * np.eye(4)
        assert cheb.min() > SEP - 1e-6, t
        blocked += int(by_mate.sum())
        pos = q
    assert blocked > 40


def test_fold_and_the_split_with_walls():
    teams = Teams(2, SEP, solid=True)
    walls = Walls([[0.0, 0.3, 1.0, 0.05]], radius=0.05, solid=True)        # a bar above the pair
    stand = np.array([[-0.25, 0.0], [0.25, 0.0]], F32)
    prop = np.array([[-0.05, 0.3], [0.05, 0.1]], F32)                     # 0 runs into the bar, 1 into 0's square
    q, code, inside, by_mate, by_wall, wall_inside = team_block_step(stand, prop, np.ones(2, bool), teams, walls)
    assert code.tolist() == [1, 2] and by_wall.tolist() == [True, False] and by_mate.tolist() == [False, True]
    assert np.array_equal(q, np.array([[-0.05, 0.0], [0.25, 0.1]], F32))
    rec_t = team_block_fold(np.tile(TEAM_BLOCKED_START, (2, 1)), code[None], inside[None], by_mate[None], np.ones((1, 2), bool), step0=6)
    rec_w = wall_blocked_fold(np.tile(TEAM_BLOCKED_START, (2, 1)), np.where(by_wall, code, 0)[None], wall_inside[None], np.ones((1, 2), bool), 6)
    assert rec_t.tolist() == [[0, -1, 0, 0], [1, 7, 0, 0]] and rec_w.tolist() == [[1, 7, 0, 0], [0, -1, 0, 0]]
    # a robot that does not step accounts nothing
    rec = team_block_fold(rec_t, code[None], inside[None], by_mate[None], np.zeros((1, 2), bool), step0=7)
    assert np.array_equal(rec, rec_t)


def test_teams_solid_flag_and_refusals():
    from mobrob_amd.envs.goal_rules import Hazards
    from mobrob_amd.waypoints import FollowState, follow_waypoints, team_blocked_result, team_solid_check
    assert Teams(4, 0.3).solid is False and Teams(4, 0.3, solid=True).solid is True
    start, wp = np.zeros((4, 2)), np.ones((4, 1, 2))
    solid = Teams(2, 0.3, solid=True)
    st = FollowState(start, wp, teams=solid)
    assert np.array_equal(st.team_blocked, np.tile(TEAM_BLOCKED_START, (4, 1))) and st.team_blocked.dtype == np.int32
    assert FollowState(start, wp, teams=True).team_blocked is None and FollowState(start, wp, teams=Teams(2, 0.3)).team_blocked is None
    assert list(team_blocked_result(st)) == ["team_blocked_steps", "team_first_blocked", "team_stopped_steps", "team_inside_steps"]
    assert team_solid_check(st, None, solid, None) and team_solid_check(st, None, solid, Walls(np.zeros((0, 4)), solid=True))
    with pytest.raises(ValueError, match="solid teams in every call or in none"):
        team_solid_check(FollowState(start, wp, teams=True), None, solid, None)
    with pytest.raises(ValueError, match="solid teams in every call or in none"):
        team_solid_check(st, None, Teams(2, 0.3), None)
    with pytest.raises(ValueError, match=r"Teams\(solid=True\) does not run with static hazards"):
        team_solid_check(st, Hazards(np.zeros((1, 2)), 0.1), solid, None)
    with pytest.raises(ValueError, match=r"Teams\(solid=True\) does not run with observational walls"):
        team_solid_check(st, None, solid, Walls(np.zeros((0, 4))))
    with pytest.raises(ValueError, match=r"Teams\(solid=True\) runs on the device engine only"):
        follow_waypoints(None, "point", start, wp, max_steps=3, teams=solid)
