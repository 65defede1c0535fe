"""Bit-level comparison of two builds of libmobrob_ppo.so on the same inputs (refactoring check).
  training leg: three PPO iterations on three shapes, then parameters / Adam moments / step statistics must be identical.
  evaluation and follow legs: every array evaluate_goal_env / follow_waypoints return (reward sums, steps, episode records,
    arrivals, final distance, path, trace; raw bytes, so NaN payloads count) for one robot per DP instantiation of the tile kernel
    (point 16, car 32, turtlebot3 48, doggo 64, and drone: 16 with the two-block head) on both paths (default and
    MOBROB_EVAL_PERSISTENT=0), deterministic and sampled actions, obs_noise 0 and 0.1, 37 robots (not a multiple of 16), an
    episode quota under a time limit and the no-limit protocol, waypoint lists of which some finish early; plus a 2x256 doggo
    engine (per-step path only).
    python scratch/compare_builds.py /path/to/old.so /path/to/new.so   (the two children run one after the other)"""
import os, subprocess, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def digest(r):
    import hashlib
    import numpy as np
    h = hashlib.sha256()
    for k in sorted(r):
        if r[k] is not None:
            a = np.ascontiguousarray(r[k])
            h.update(k.encode() + str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()[:16] + (" tile" if r["persistent"] else " per-step")


def eval_follow_legs(out):
    import numpy as np
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    from mobrob_amd.envs.wrapper import ROBOT_DIMS
    N, S, K = 37, 150, 5
    for robot, H in [("point", 64), ("car", 64), ("turtlebot3", 64), ("doggo", 64), ("drone", 64), ("doggo", 256)]:
        D, A, P = ROBOT_DIMS[robot]
        e = PPOEngine(obs_dim=D, act_dim=A, n_envs=16, n_steps=16, batch_size=64, n_epochs=1, pi=(H, H), vf=(H, H), seed=3)
        rng = np.random.default_rng(7)
        p = e.get_params()
        for k, v in p.items():
            p[k] = (np.full_like(v, -0.5) if k == "log_std" else
                    (rng.standard_normal(v.shape) / np.sqrt(v.shape[1])).astype(np.float32) if v.ndim == 2 else
                    (0.1 * rng.standard_normal(v.shape)).astype(np.float32))
        e.set_params(p)
        env = DeviceGoalVecEnv.for_robot(robot, N, time_limit=30, seed=5)
        # every second robot: waypoints 2 cm apart (inside the reach radius: reached on consecutive steps, the robot finishes
        # early); the others: far waypoints behind two near ones; robot 3 has no waypoint, robot 4 a shorter list
        start = rng.uniform(-1.5, 1.5, (N, P)).astype(np.float32)
        u = rng.standard_normal((N, 1, P))
        u /= np.linalg.norm(u, axis=2, keepdims=True)
        near = start[:, None, :] + 0.02 * (np.arange(K)[None, :, None] + 1) * u
        far = rng.uniform(-2.0, 2.0, (N, K, P))
        far[:, :2] = near[:, :2]
        wp = np.where((np.arange(N) % 2 == 0)[:, None, None], near, far).astype(np.float32)
        nw = np.full(N, K, np.int32)
        nw[3], nw[4] = 0, 2
        for pe in ((None, "0") if H == 64 else (None,)):
            if pe is None:
                os.environ.pop("MOBROB_EVAL_PERSISTENT", None)
            else:
                os.environ["MOBROB_EVAL_PERSISTENT"] = pe
            for det in (True, False):
                for noise in (0.0, 0.1):
                    kw = dict(dt=env.dt, extent=env.extent, extra_bonus=env.extra_bonus, obs_noise=noise, deterministic=det, seed=11)
                    tag = f"{robot} 2x{H} {'per-step' if pe else 'default '} {'det ' if det else 'samp'} noise {noise}"
                    r = e.evaluate_goal_env(P, env.mix, 30, True, n_robots=N, max_steps=3 * 30, episodes=50, trace=(N, 90), **kw)
                    out[tag + " | evaluate quota"] = digest(r)
                    r = e.evaluate_goal_env(P, env.mix, 0, True, n_robots=N, max_steps=S, episodes=0, trace=(N, S), **kw)
                    out[tag + " | evaluate no-limit"] = digest(r)
                    r = e.follow_waypoints(P, env.mix, start=start, waypoints=wp, n_waypoints=nw, max_steps=S, path_stride=3,
                                           trace=(N, S), **kw)
                    assert 0 < int((r["reached"] == nw).sum()) < N and int(r["steps"].min()) == 0 and int(r["steps"].max()) == S
                    out[tag + " | follow"] = digest(r)
        os.environ.pop("MOBROB_EVAL_PERSISTENT", None)
        e.close()


if len(sys.argv) == 3 and sys.argv[1] == "--run":
    import numpy as np, hashlib
    from mobrob_amd import _lib
    _lib.LIB_PATH = sys.argv[2]
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.rl_control.init import orthogonal_policy_init
    out = {}
    for (D, A, H, N, T, B) in [(58, 12, 256, 512, 64, 4096), (14, 2, 64, 256, 64, 2048), (26, 2, 48, 64, 32, 256)]:
        e = PPOEngine(obs_dim=D, act_dim=A, n_envs=N, n_steps=T, batch_size=B, n_epochs=3, pi=(H, H), vf=(H, H), ent_coef=0.01, seed=5)
        e.set_params(orthogonal_policy_init(D, A, (H, H), (H, H), 0))
        for _ in range(3):
            e.collect_synthetic(p_term=0.02, time_limit=40)
            st = e.train(None)
        m, v, step = e.get_optimizer_state()
        h = hashlib.sha256(e.get_flat_params().tobytes())
        for k in sorted(m):
            h.update(m[k].tobytes()); h.update(v[k].tobytes())
        out[f"{D}x{A}x{H}"] = [h.hexdigest()[:16], step, repr(st["grad_norm"]), repr(st["loss"])]
        e.close()
    eval_follow_legs(out)
    print(json.dumps(out))
else:
    res = []
    for p in sys.argv[1:3]:   # one process at a time; a child that fails ends the comparison
        c = subprocess.run([sys.executable, __file__, "--run", p], capture_output=True, text=True)
        if c.returncode != 0:
            sys.exit(f"{p}: exit status {c.returncode}\n{c.stderr[-4000:]}")
        res.append(json.loads(c.stdout.strip().splitlines()[-1]))
    for k in res[0]:
        print(f"{k:<62}", "IDENTICAL" if res[0][k] == res[1][k] else "DIFFERENT", res[0][k], res[1][k])
    bad = [k for k in res[0] if res[0][k] != res[1][k]]
    print(f"{len(res[0]) - len(bad)} of {len(res[0])} identical")
    sys.exit(1 if bad else 0)
