"""NumPy restatement of the goal environment's step (kernels_env.h goal_advance) for the evaluation tests, in float32."""
import numpy as np

F32 = np.float32


def trace_fields(tr, D, A):
    """Split a trace [steps][robots][9 + D + A + 4] into its named parts."""
    return dict(pos=tr[..., 0:3], vel=tr[..., 3:6], goal=tr[..., 6:9], obs=tr[..., 9:9 + D], act=tr[..., 9 + D:9 + D + A],
                reward=tr[..., 9 + D + A], reached=tr[..., 10 + D + A] > 0, term=tr[..., 11 + D + A] > 0,
                tr=tr[..., 12 + D + A] > 0)


def goal_advance(pos, vel, goal, act, mix, P, dt, extent, reach=0.3, bonus=5.0, extra_bonus=0.0):
    """One step of robots [n] (pos / vel / goal [n][3], act [n][A] clipped) -> (pos', vel', reward, reached)."""
    pos, vel, goal = pos[:, :P].astype(F32), vel[:, :P].astype(F32), goal[:, :P].astype(F32)
    cmd = (act.astype(F32) @ np.asarray(mix, F32)[:P].T).astype(F32)
    d0 = np.sqrt(np.sum((goal - pos) ** 2, axis=1, dtype=F32)).astype(F32)
    vel2 = (F32(0.8) * vel + F32(0.2) * cmd).astype(F32)
    pos2 = np.clip(pos + F32(dt) * vel2, -F32(extent), F32(extent)).astype(F32)
    d1 = np.sqrt(np.sum((goal - pos2) ** 2, axis=1, dtype=F32)).astype(F32)
    reached = d1 < F32(reach)
    reward = (d0 - d1) + np.where(reached, F32(bonus) + F32(extra_bonus), F32(0))
    return pos2, vel2, reward.astype(F32), reached
