"""Bit-level comparison of two builds of libmobrob_ppo.so on the same inputs (refactoring check).
  training leg: three PPO iterations on three shapes, then parameters / Adam moments / step statistics must be identical (the
    2x48 shape runs the generic chain, whose float atomics differ between two runs of one build: reported, not judged), and
    train_legs: every host path of the update -- 2x256 chain kernel (two Dp), MOBROB_NO_CHAIN, MOBROB_NO_X3, Dp 48, A > 16; 2x64
    epoch kernel, three launches, block kernel, pair kernel with the narrow and the wide reduce; on both widths target_kl (early
    stop asserted), clip_range_vf, normalize_advantage off, MOBROB_NO_NORM_RECORDS, caller permutations, a short last minibatch
    and the step-wise driver -- hashing parameters, moments, adam_step, statistics rows, update_mode and last_train_info.
  evaluation and follow legs: every array evaluate_goal_env / follow_waypoints return (reward sums, steps, episode records,
    arrivals, final distance, path, trace; raw bytes, so NaN payloads count) for one robot per DP instantiation of the tile kernel
    (point 16, car 32, turtlebot3 48, doggo 64, and drone: 16 with the two-block head) on both paths (default and
    MOBROB_EVAL_PERSISTENT=0), deterministic and sampled actions, obs_noise 0 and 0.1, 37 robots (not a multiple of 16), an
    episode quota under a time limit and the no-limit protocol, waypoint lists of which some finish early; plus a 2x256 doggo
    engine (per-step path only).
  rollout leg: the raw bytes of every rollout buffer (obs, actions, rewards, episode_starts, values, log_probs, advantages, returns,
    last_values, last_dones, clipped_actions; host rollouts also the caller's clipped actions) after one and after two consecutive
    collections, for every way a rollout is enqueued: device rollouts (synthetic source and goal env) on the 64-wide tile kernel
    without and with the overlapped value pass, the one-wave kernel (MOBROB_ROLLOUT64_TILE_MAX=0), the 256-wide kernel with and
    without overlap, n_steps that the chunk length does not divide, the per-step path eager and graph-replayed; host rollouts of
    the native C env served by the rollout kernel (both widths, one and two row ranges) and through the launch-per-step collector
    (MOBROB_COLLECT_SERVER=0); act / store with pinned and with ordinary buffers (truncations in every rollout).  A second child
    per library runs the 256-wide device rollouts with MOBROB_ROLLOUT_S8=0 (the four-wave kernel; read once per process).
    python scratch/compare_builds.py /path/to/old.so /path/to/new.so   (the children run one after the other)"""
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


ROLLOUT_KEYS = ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns", "last_values",
                "last_dones", "clipped_actions")


def rollout_digest(e, extra=None):
    import hashlib
    h = hashlib.sha256()
    for k in ROLLOUT_KEYS:
        h.update(e.read(k).tobytes())
    if extra is not None:
        h.update(extra.tobytes())
    return h.hexdigest()[:16]


def rollout_legs(out, s8_off):
    """s8_off: the child runs under MOBROB_ROLLOUT_S8=0 -- only the configurations that kernel choice touches (256-wide, persistent)."""
    import numpy as np
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs.native_env import NativeGoalVecEnv
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    from mobrob_amd.rl_control.init import orthogonal_policy_init
    from oracle import ppo_oracle as O
    tag0 = "rollout S8=0 | " if s8_off else "rollout | "

    def engine(robot, H, N, T, **kw):
        D, A, _ = ROBOT_DIMS[robot]
        e = PPOEngine(obs_dim=D, act_dim=A, n_envs=N, n_steps=T, batch_size=N, n_epochs=1, pi=(H, H), vf=(H, H), seed=5, **kw)
        e.set_params(orthogonal_policy_init(D, A, (H, H), (H, H), 0))
        return e

    from mobrob_amd.envs.wrapper import ROBOT_DIMS
    # ---- device rollouts: (name, robot, H, N, T, environment at engine_create, engine keywords)
    dev = [("256 S8 overlap", "doggo", 256, 512, 64, {}, {}),
           ("256 overlap, chunk does not divide T", "doggo", 256, 512, 72, {}, {}),
           ("256 no overlap (193 tiles)", "car", 256, 193 * 32, 8, {}, {}),
           ("256 Dp 48 (x3 packs rebuilt per rollout)", "turtlebot3", 256, 128, 40, {}, {}),
           ("256 Dp 16 one chunk", "point", 256, 64, 12, {}, {})]
    if not s8_off:
        dev += [("64 tile no overlap", "point", 64, 256, 64, {}, {}),
                ("64 tile overlap", "point", 64, 1024, 256, {}, {}),
                ("64 tile overlap, chunk does not divide T", "turtlebot3", 64, 1024, 260, {}, {}),
                ("64 one-wave kernel", "car", 64, 256, 64, {"MOBROB_ROLLOUT64_TILE_MAX": "0"}, {}),
                ("64 per-step graph", "point", 64, 64, 16, {}, dict(rollout_persistent=False)),
                ("64 per-step eager", "point", 64, 64, 16, {}, dict(rollout_persistent=False, rollout_graph=False)),
                ("256 per-step graph", "doggo", 256, 64, 16, {}, dict(rollout_persistent=False)),
                ("256 per-step eager", "doggo", 256, 64, 16, {}, dict(rollout_persistent=False, rollout_graph=False)),
                ("48 generic per-step graph", "car", 48, 64, 16, {}, {}),
                ("48 generic per-step eager", "car", 48, 64, 16, {}, dict(rollout_graph=False))]
    for name, robot, H, N, T, env_vars, kw in dev:
        for source in ("synthetic", "goal"):
            os.environ.update(env_vars)
            try:
                e = engine(robot, H, N, T, **kw)
            finally:
                for k in env_vars:
                    os.environ.pop(k, None)
            genv = DeviceGoalVecEnv.for_robot(robot, N, time_limit=30, seed=5)
            for i in (1, 2):
                if source == "synthetic":
                    e.collect_synthetic(p_term=0.02, time_limit=40)
                else:
                    genv.collect(e)
                e.synchronize()
                out[f"{tag0}{name} | {source} | after {i}"] = rollout_digest(e)
            e.close()
    if s8_off:   # (the served collector exists for the eight-wave kernel only)
        return
    # ---- host rollouts of the native C env: served by the rollout kernel (2: or fail) and launch-per-step (0)
    host = [("256", "doggo", 256, 128, 37, 1), ("256", "doggo", 256, 128, 37, 2), ("256 Dp 48", "turtlebot3", 256, 192, 40, 2),
            ("64", "doggo", 64, 128, 37, 1), ("64", "point", 64, 128, 37, 2), ("64 overlap", "point", 64, 1024, 256, 2)]
    for name, robot, H, N, T, parts in host:
        for mode in ("2", "0"):
            e = engine(robot, H, N, T)
            D, A = e.D, e.A
            env = NativeGoalVecEnv.for_robot(robot, N, time_limit=5, seed=7)
            b = dict(obs=e.pinned((N, D)), clip=e.pinned((N, A)), rew=e.pinned((N,)), done=e.pinned((N,), np.uint8),
                     trunc=e.pinned((N,), np.uint8), term=e.pinned((N, D)))
            env.use_buffers(obs=b["obs"], rewards=b["rew"], dones=b["done"], truncated=b["trunc"], terminal_obs=b["term"])
            env.reset()
            os.environ["MOBROB_COLLECT_SERVER"] = mode
            os.environ["MOBROB_SERVER_TIMEOUT_S"] = "10"
            try:
                for i in (1, 2):
                    e.rollout_begin()
                    e.part_pipeline(parts, b["obs"], b["clip"], b["rew"], b["done"], b["trunc"], b["term"]).collect(env.step_range_fn, env.handle)
                    out[f"{tag0}host {name} {robot} {parts} range(s) | {'served' if mode == '2' else 'launch-per-step'} | after {i}"] = rollout_digest(e, b["clip"])
            finally:
                os.environ.pop("MOBROB_COLLECT_SERVER", None)
                os.environ.pop("MOBROB_SERVER_TIMEOUT_S", None)
            env.close()
            e.close()
    # ---- act / store per step, pinned and ordinary buffers, a time limit of 5 steps (truncated rows with a bootstrap)
    for H in (64, 256):
        for pinned in (True, False):
            D, A, N, T = 14, 2, 6, 12
            e = engine("point", H, N, T)
            env = O.NumpySyntheticVecEnv(N, D, A, p_term=0.1, time_limit=5, seed=3)
            mk = e.pinned if pinned else (lambda shape, dtype=np.float32: np.zeros(shape, dtype))
            b = dict(obs=mk((N, D)), clip=mk((N, A)), rew=mk((N,)), done=mk((N,), np.uint8), trunc=mk((N,), np.uint8), term=mk((N, D)))
            b["obs"][:] = env.reset()
            saw_trunc = False
            for i in (1, 2):
                e.rollout_begin()
                for t in range(T):
                    e.act(b["obs"], None, out_clipped=b["clip"], want_all=False)
                    obs, rew, done, trunc, term = env.step(b["clip"].copy())
                    b["obs"][:], b["rew"][:], b["done"][:], b["trunc"][:], b["term"][:] = obs, rew, done, trunc, term
                    saw_trunc |= bool(trunc.any())
                    e.store(b["rew"], b["done"], b["trunc"], b["term"])
                e.finish_rollout(b["obs"], b["done"])
                assert saw_trunc
                out[f"{tag0}act/store 2x{H} {'pinned' if pinned else 'ordinary'} buffers | after {i}"] = rollout_digest(e, b["clip"])
            e.close()


def train_legs(out):
    """Every host path of the optimizer update.  Per case: two collect_synthetic + train iterations of three epochs, then the raw
    bytes of parameters, both Adam moments, adam_step, the step-statistics rows, update_mode and last_train_info.  Environment
    switches are set before the engine is created and removed afterwards (they are read at creation or once per train())."""
    import ctypes as C
    import hashlib
    import numpy as np
    from mobrob_amd._lib import check
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.rl_control.init import orthogonal_policy_init
    W256 = dict(D=58, A=12, H=256, N=128, T=32, B=1024)   # chain kernel, Dp 64
    W64 = dict(D=14, A=2, H=64, N=64, T=32, B=512)        # split kernel (16 tiles), three launches per step or k_epoch64
    REF = dict(D=58, A=12, H=64, N=16, T=125, B=100)      # reference-YAML-like: batch 100 = four tiles -> k_epoch64
    cases = [("256 chain Dp 64", W256, dict(x3=7)),
             ("256 chain Dp 32", dict(W256, D=26, A=2), dict(x3=7)),
             ("256 MOBROB_NO_CHAIN", W256, dict(env={"MOBROB_NO_CHAIN": "1"}, x3=3)),
             ("256 MOBROB_NO_X3", W256, dict(env={"MOBROB_NO_X3": "1"}, x3=0)),
             ("256 Dp 48", dict(W256, D=40, A=2), dict(x3=1)),
             ("256 A 20", dict(W256, A=20), dict(x3=1)),
             ("64 epoch kernel", REF, dict(mode=1)),
             ("64 epoch_kernel=0", REF, dict(hyper=dict(epoch_kernel=0), mode=0)),
             ("64 block kernel", dict(W64, N=256, T=64, B=2048), dict(env={"MOBROB_SPLIT64_MAX_TILES": "0"}, mode=0, kernel="block")),
             ("64 pair, narrow reduce", dict(W64, N=512, T=32, B=4096), dict(mode=0, kernel="pair")),
             ("64 pair, wide reduce (256 slabs per network)", dict(W64, N=1024, T=32, B=16384), dict(mode=0, kernel="wide"))]
    for w, base in (("256", W256), ("64", W64), ("64 ref", REF)):
        cases += [(f"{w} target_kl early stop", base, dict(hyper=dict(target_kl=1e-5), stop=True)),
                  (f"{w} clip_range_vf", base, dict(hyper=dict(clip_range_vf=0.2))),
                  (f"{w} normalize_advantage off", base, dict(kw=dict(normalize_advantage=False))),
                  (f"{w} MOBROB_NO_NORM_RECORDS", base, dict(env={"MOBROB_NO_NORM_RECORDS": "1"}, mode=0)),
                  (f"{w} caller permutations", base, dict(perms=True)),
                  (f"{w} short last minibatch", dict(base, B=base["B"] * 3 // 5), {}),
                  (f"{w} step-wise driver", base, dict(stepwise=True))]
    for name, s, o in cases:
        if "kernel" in o:   # the engine's rule (grad64_plan; defaults: split up to 64 tiles, pair from 65, 4 pairs x 256 CUs / 2 sequences)
            ntiles = -(-s["B"] // 32)
            nbseq = (min(ntiles, 512) + 1) // 2
            split = "MOBROB_SPLIT64_MAX_TILES" not in o.get("env", {}) and ntiles <= 64
            want = "split" if split else "block" if ntiles < 65 else "wide" if nbseq > 128 else "pair"
            assert want == o["kernel"], (name, want)
        env_vars = o.get("env", {})
        os.environ.update(env_vars)
        try:
            e = PPOEngine(obs_dim=s["D"], act_dim=s["A"], n_envs=s["N"], n_steps=s["T"], batch_size=s["B"], n_epochs=3,
                          pi=(s["H"], s["H"]), vf=(s["H"], s["H"]), ent_coef=0.01, seed=5, **o.get("kw", {}))
            e.set_params(orthogonal_policy_init(s["D"], s["A"], (s["H"], s["H"]), (s["H"], s["H"]), 0))
            e.set_hyper(**o.get("hyper", {}))
            if "x3" in o:
                assert e.x3_mode() == o["x3"], (name, e.x3_mode())
            total, rng = s["N"] * s["T"], np.random.default_rng(11)
            assert (total % s["B"] != 0) == ("short" in name)
            h = hashlib.sha256()
            for _ in range(2):
                e.collect_synthetic(p_term=0.02, time_limit=40)
                if o.get("stepwise"):
                    for _ep in range(3):
                        e.epoch_begin()
                        for mb in range(e.n_minibatches):
                            e.minibatch_grad(mb)
                            e.minibatch_apply()
                else:
                    perms = np.stack([rng.permutation(total) for _ in range(3)]).astype(np.int64) if o.get("perms") else None
                    check(e.lib.mobrob_ppo_train(e._h, perms.ctypes.data_as(C.POINTER(C.c_int64)) if perms is not None else None, None))
                h.update(e.fetch_step_stats().tobytes())   # (train() with a statistics struct would have consumed the rows)
                if "mode" in o:
                    assert e.update_mode() == o["mode"], (name, e.update_mode())
            info = e.last_train_info()
            if o.get("stop"):
                assert info[1], (name, info)
            m, v, step = e.get_optimizer_state()
            h.update(e.get_flat_params().tobytes())
            for k in sorted(m):
                h.update(m[k].tobytes()); h.update(v[k].tobytes())
            h.update(repr((step, e.update_mode(), info)).encode())
            out[f"train | {name}"] = [h.hexdigest()[:16], step, e.update_mode(), list(info)]
            e.close()
        finally:
            for k in env_vars:
                os.environ.pop(k, None)


if len(sys.argv) >= 3 and sys.argv[1] == "--run-s8off":
    from mobrob_amd import _lib
    _lib.LIB_PATH = sys.argv[2]
    out = {}
    rollout_legs(out, True)
    print(json.dumps(out))
elif len(sys.argv) == 3 and sys.argv[1] == "--run":
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
    train_legs(out)
    rollout_legs(out, False)
    eval_follow_legs(out)
    print(json.dumps(out))
else:
    res = []
    for p in sys.argv[1:3]:   # one process at a time; a child that fails ends the comparison
        r = {}
        for leg, env in (("--run", {}), ("--run-s8off", {"MOBROB_ROLLOUT_S8": "0"})):
            c = subprocess.run([sys.executable, __file__, leg, p], capture_output=True, text=True, env={**os.environ, **env})
            if c.returncode != 0:
                sys.exit(f"{p} ({leg}): exit status {c.returncode}\n{c.stderr[-4000:]}")
            r.update(json.loads(c.stdout.strip().splitlines()[-1]))
        res.append(r)
    # the generic chain (float atomics in its minibatch sums) differs between two runs of ONE build: reported, not judged
    unjudged = ("26x2x48",)
    for k in res[0]:
        print(f"{k:<86}", "IDENTICAL" if res[0][k] == res[1][k] else "DIFFERENT", res[0][k], res[1][k], "(not judged)" if k in unjudged else "")
    bad = [k for k in res[0] if res[0][k] != res[1][k] and k not in unjudged]
    print(f"{len(res[0]) - len(unjudged) - len(bad)} of {len(res[0]) - len(unjudged)} judged rows identical")
    sys.exit(1 if bad else 0)
