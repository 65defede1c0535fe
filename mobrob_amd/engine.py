"""NumPy-facing wrapper of the C ABI: one `PPOEngine` per GPU (one per process in data-parallel runs)."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import BUF, Config, DroneParams, EpisodeStats, EvalSpec, FollowSpec, GoalEnv, HazardFramesC, HazardsC, TrainStats, check

F32 = np.float32
STAT_KEYS = ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "grad_norm")


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _u8(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))


def _f32c(a, shape=None):
    a = np.ascontiguousarray(a, dtype=F32)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
    return a


MAX_HIDDEN = 8   # kMaxHidden (csrc/device_utils.h): hidden layers per network

# policy_kwargs `activation_fn`: lower-cased torch.nn class name -> (MOBROB_ACT_* code, torch.nn class name).  The parameter-free
# element-wise modules with torch's default arguments; tanh is SB3's default for MlpPolicy (every reference YAML).
ACTIVATIONS = OrderedDict([("tanh", (0, "Tanh")), ("relu", (1, "ReLU")), ("elu", (2, "ELU")), ("leakyrelu", (3, "LeakyReLU")),
                           ("sigmoid", (4, "Sigmoid")), ("softplus", (5, "Softplus")), ("softsign", (6, "Softsign")),
                           ("hardtanh", (7, "Hardtanh")), ("relu6", (8, "ReLU6")), ("silu", (9, "SiLU")), ("gelu", (10, "GELU")),
                           ("mish", (11, "Mish"))])


def activation_name(act) -> str:
    """`activation_fn` as a torch.nn class, its name or None (SB3's default, Tanh) -> key of ACTIVATIONS; anything else raises
    NotImplementedError by name."""
    if act is None:
        return "tanh"
    name = getattr(act, "__name__", None) or str(act)
    if name.startswith("<class "):   # the readable side of a checkpoint blob: "<class 'torch.nn.modules.activation.ELU'>"
        name = name.split("'")[1]
    name = name.rsplit(".", 1)[-1].replace("_", "").lower()
    if name not in ACTIVATIONS:
        raise NotImplementedError(f"activation_fn {act!r}: implemented are {', '.join(v[1] for v in ACTIVATIONS.values())} "
                                  "(parameter-free element-wise modules, torch's default arguments)")
    return name


def param_shapes(obs_dim, act_dim, pi, vf, use_sde=False, full_std=True):
    """SB3 `policy.state_dict()` key order and shapes (include/mobrob_ppo.h 'Conventions'); one to eight hidden layers per
    network (`nn.Sequential` indices 0, 2, 4 ...: every Linear is followed by its activation module)."""
    s = OrderedDict()
    # gSDE: one row per unit of the policy's last hidden layer (one column without full_std)
    s["log_std"] = (pi[-1], act_dim if full_std else 1) if use_sde else (act_dim,)
    for net, widths in (("policy_net", pi), ("value_net", vf)):
        prev = obs_dim
        for i, w in enumerate(widths):
            s[f"mlp_extractor.{net}.{2 * i}.weight"] = (w, prev)
            s[f"mlp_extractor.{net}.{2 * i}.bias"] = (w,)
            prev = w
    s["action_net.weight"] = (act_dim, pi[-1])
    s["action_net.bias"] = (act_dim,)
    s["value_net.weight"] = (1, vf[-1])
    s["value_net.bias"] = (1,)
    return s


class _PinnedBlock:
    """Owner of one hipHostMalloc allocation.  NumPy arrays made from it keep it alive through `.base`, and the memory
    is returned to the driver when the LAST such array dies -- not when the engine closes: the rollout collector, the
    environment (`use_buffers`) and `PPO._last_obs` all hold views that outlive `PPOEngine.close()`."""

    def __init__(self, lib, nbytes, shape, dtype):
        self._lib, self.ptr = lib, lib.mobrob_ppo_host_alloc(max(int(nbytes), 1))
        if not self.ptr:
            raise MemoryError("hipHostMalloc failed")
        C.memset(self.ptr, 0, max(int(nbytes), 1))
        self.__array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(dtype).str, "data": (self.ptr, False),
                                    "version": 3}

    def __del__(self):
        ptr, self.ptr = getattr(self, "ptr", None), None
        if ptr:
            try:
                self._lib.mobrob_ppo_host_free(C.c_void_p(ptr))
            except Exception:  # noqa: BLE001 - interpreter shutdown
                pass


class PartPipeline:
    """The N envs cut into `nparts` contiguous row ranges: while the host simulator steps range p, the GPU runs the
    policy for the other ranges.  Results equal act()/store() over all rows (same noise per env and step).  The
    ctypes pointers of the pinned arrays are taken once: the loop below is the per-step hot path of a host-env rollout.

        pipe = engine.part_pipeline(2, obs, clip, rew, done, trunc, term); engine.rollout_begin()
        for p in range(2): pipe.act(p)
        for t in range(T):
            for p in range(2):
                pipe.wait(p); n_trunc = env.step_range(*pipe.bounds[p], clip); pipe.store(p, n_trunc > 0)
                if t + 1 < T: pipe.act(p)
        engine.finish_rollout(obs, done)

    or, for an environment stepped by a C function, the same loop without Python: pipe.collect(fn, handle).
    """

    def __init__(self, engine, nparts, obs, clipped, rewards, dones, truncated, terminal_obs):
        e, n = engine, int(nparts)
        want = dict(obs=((e.N, e.D), F32), clipped=((e.N, e.A), F32), rewards=((e.N,), F32), dones=((e.N,), np.uint8),
                    truncated=((e.N,), np.uint8), terminal_obs=((e.N, e.D), F32))
        for name, arr in dict(obs=obs, clipped=clipped, rewards=rewards, dones=dones, truncated=truncated,
                              terminal_obs=terminal_obs).items():
            shape, dt = want[name]
            if arr.shape != shape or arr.dtype != dt or not arr.flags.c_contiguous:
                raise ValueError(f"{name} must be a C-contiguous {np.dtype(dt).name}{shape} array from engine.pinned()")
        self._keep = (obs, clipped, rewards, dones, truncated, terminal_obs)
        self.nparts, self._h, self._lib = n, engine._h, engine.lib
        self.bounds = [(e.N * p // n, e.N * (p + 1) // n) for p in range(n)]
        self._obs, self._clip, self._rew = _fp(obs), _fp(clipped), _fp(rewards)
        self._done, self._trunc, self._term = _u8(dones), _u8(truncated), _fp(terminal_obs)

    def act(self, part):
        check(self._lib.mobrob_ppo_act_part(self._h, part, self.nparts, self._obs, self._clip))

    def wait(self, part):
        check(self._lib.mobrob_ppo_wait_part(self._h, part))

    def store(self, part, any_truncated=True, pull_next_obs=True):
        """pull_next_obs: the same launch also moves the part's next observations (already in `obs`: the env wrote
        them) into the next rollout slot, so the following act() launches the policy kernel only."""
        check(self._lib.mobrob_ppo_store_part(self._h, part, self.nparts, self._rew, self._done,
                                              self._trunc if any_truncated else None,
                                              self._term if any_truncated else None,
                                              self._obs if pull_next_obs else None))

    def collect(self, step_range_fn, env_handle):
        """The whole rollout (rollout_begin ... finish_rollout) in one native call: mobrob_ppo_collect_host drives the
        environment through `step_range_fn` (address of a C function with mobrob_env_step_range_fn's signature, e.g.
        NativeGoalVecEnv.step_range_fn) -- no Python frame per step."""
        check(self._lib.mobrob_ppo_collect_host(self._h, step_range_fn, env_handle, self.nparts, self._obs, self._clip,
                                                self._rew, self._done, self._trunc, self._term))


class PPOEngine:
    @staticmethod
    def make_config(obs_dim, act_dim, n_envs, n_steps, batch_size=64, n_epochs=10, pi=(64, 64), vf=(64, 64),
                    gamma=0.99, gae_lambda=0.95, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                    learning_rate=3e-4, adam_betas=(0.9, 0.999), adam_eps=1e-5, normalize_advantage=True,
                    action_low=-1.0, action_high=1.0, seed=0, device_id=0, rank=0, world_size=1, fast_kernels=True,
                    rollout_graph=True, rollout_persistent=True, activation="tanh", forward_x3=True, use_sde=False,
                    sde_sample_freq=-1, sde_full_std=True, sde_use_expln=False) -> Config:
        """PPO(...) keyword arguments -> `mobrob_ppo_config_t` (SB3 defaults, Appendix A.1)."""
        if not (1 <= len(pi) <= MAX_HIDDEN and 1 <= len(vf) <= MAX_HIDDEN):
            raise ValueError(f"net_arch: one to {MAX_HIDDEN} hidden layers per network (pi=[h1, ...], vf=[h1, ...])")
        cfg = Config()
        _lib.load().mobrob_ppo_default_config(C.byref(cfg))
        cfg.obs_dim, cfg.act_dim = int(obs_dim), int(act_dim)
        pw, vw = (list(map(int, pi)) + [0] * MAX_HIDDEN)[:MAX_HIDDEN], (list(map(int, vf)) + [0] * MAX_HIDDEN)[:MAX_HIDDEN]   # 0 ends the list
        cfg.pi_hidden[0], cfg.pi_hidden[1], cfg.pi_hidden3 = pw[:3]
        cfg.vf_hidden[0], cfg.vf_hidden[1], cfg.vf_hidden3 = vw[:3]
        for i in range(3, MAX_HIDDEN):
            cfg.pi_hidden_ext[i - 3], cfg.vf_hidden_ext[i - 3] = pw[i], vw[i]
        cfg.n_envs, cfg.n_steps, cfg.batch_size, cfg.n_epochs = int(n_envs), int(n_steps), int(batch_size), int(n_epochs)
        cfg.gamma, cfg.gae_lambda, cfg.clip_range = float(gamma), float(gae_lambda), float(clip_range)
        cfg.ent_coef, cfg.vf_coef, cfg.max_grad_norm = float(ent_coef), float(vf_coef), float(max_grad_norm)
        cfg.learning_rate = float(learning_rate)
        cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps = float(adam_betas[0]), float(adam_betas[1]), float(adam_eps)
        cfg.action_low, cfg.action_high = float(action_low), float(action_high)
        cfg.normalize_advantage = int(bool(normalize_advantage))
        cfg.seed, cfg.device_id, cfg.rank, cfg.world_size = int(seed), int(device_id), int(rank), int(world_size)
        cfg.fast_kernels = int(bool(fast_kernels))
        cfg.rollout_graph = int(bool(rollout_graph))
        cfg.rollout_persistent = int(bool(rollout_persistent))
        cfg.activation = ACTIVATIONS[activation_name(activation)][0]
        cfg.forward_x3 = int(bool(forward_x3))
        cfg.use_sde, cfg.sde_sample_freq = int(bool(use_sde)), int(sde_sample_freq)
        cfg.sde_full_std, cfg.sde_use_expln = int(bool(sde_full_std)), int(bool(sde_use_expln))
        return cfg

    @staticmethod
    def device_bytes(**kwargs) -> int:
        """Device bytes an engine with these arguments occupies (host-only sizing pass, no GPU needed)."""
        cfg = PPOEngine.make_config(**kwargs)
        n = C.c_size_t(0)
        check(_lib.load().mobrob_ppo_device_bytes(C.byref(cfg), C.byref(n)))
        return int(n.value)

    def __init__(self, obs_dim, act_dim, n_envs, n_steps, *, arena=None, **kwargs):
        """arena: optional (device_pointer, bytes) -- build the engine inside caller-owned device memory
        (mobrob_ppo_create_in_arena; the fleet packs several engines into one allocation this way)."""
        self.lib = _lib.load()
        cfg = self.make_config(obs_dim, act_dim, n_envs, n_steps, **kwargs)
        pi = tuple(w for w in (cfg.pi_hidden[0], cfg.pi_hidden[1], cfg.pi_hidden3, *cfg.pi_hidden_ext) if w > 0)
        vf = tuple(w for w in (cfg.vf_hidden[0], cfg.vf_hidden[1], cfg.vf_hidden3, *cfg.vf_hidden_ext) if w > 0)
        self.cfg = cfg
        self.D, self.A, self.N, self.T = int(obs_dim), int(act_dim), int(n_envs), int(n_steps)
        self.shapes = param_shapes(self.D, self.A, pi, vf, bool(cfg.use_sde), bool(cfg.sde_full_std))
        self.use_sde, self.HL = bool(cfg.use_sde), int(pi[-1])
        self._h = C.c_void_p()
        if arena is None:
            check(self.lib.mobrob_ppo_create(C.byref(cfg), C.byref(self._h)))
        else:
            check(self.lib.mobrob_ppo_create_in_arena(C.byref(cfg), C.c_void_p(int(arena[0])), C.c_size_t(int(arena[1])),
                                                      C.byref(self._h)))
        self.P = int(self.lib.mobrob_ppo_param_count(self._h))
        assert self.P == sum(int(np.prod(s)) for s in self.shapes.values())
        self.n_minibatches = int(self.lib.mobrob_ppo_num_minibatches(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.mobrob_ppo_destroy(self._h)
            self._h = C.c_void_p()
            for addr in list(getattr(self, "_registered", [])):
                self.unregister_host(addr)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters ---------------------------------------------------------------------------
    def get_flat_params(self):
        out = np.empty(self.P, F32)
        check(self.lib.mobrob_ppo_get_params(self._h, _fp(out), self.P))
        return out

    def set_flat_params(self, flat):
        flat = _f32c(flat, (self.P,))
        check(self.lib.mobrob_ppo_set_params(self._h, _fp(flat), self.P))

    def unflatten(self, flat):
        out, o = OrderedDict(), 0
        for k, s in self.shapes.items():
            n = int(np.prod(s))
            out[k] = np.array(flat[o:o + n], F32).reshape(s)
            o += n
        return out

    def flatten(self, d):
        parts = []
        for k, s in self.shapes.items():
            a = np.asarray(d[k], F32)
            if a.shape != tuple(s):
                raise ValueError(f"size mismatch for {k}: expected {tuple(s)}, got {a.shape}")
            parts.append(a.ravel())
        return np.concatenate(parts)

    def get_params(self):
        return self.unflatten(self.get_flat_params())

    def set_params(self, d):
        self.set_flat_params(self.flatten(d))

    def get_optimizer_state(self):
        m, v, step = np.empty(self.P, F32), np.empty(self.P, F32), C.c_int64()
        check(self.lib.mobrob_ppo_get_optimizer_state(self._h, _fp(m), _fp(v), self.P, C.byref(step)))
        return self.unflatten(m), self.unflatten(v), int(step.value)

    def set_optimizer_state(self, exp_avg, exp_avg_sq, step):
        m, v = _f32c(self.flatten(exp_avg)), _f32c(self.flatten(exp_avg_sq))
        check(self.lib.mobrob_ppo_set_optimizer_state(self._h, _fp(m), _fp(v), self.P, int(step)))

    # ---- rollout ------------------------------------------------------------------------------
    # ---- gSDE ---------------------------------------------------------------------------------
    def sde_reset_noise(self):
        """policy.reset_noise(n_envs): new exploration matrices from the current log_std."""
        check(self.lib.mobrob_ppo_sde_reset_noise(self._h))

    def sde_set_noise(self, z):
        """Exploration matrices as an input: z ~ N(0, 1) of shape [n_envs, HL, A] (None: the engine's own draws again)."""
        if z is None:
            check(self.lib.mobrob_ppo_sde_set_noise(self._h, None))
            return
        z = _f32c(z, (self.N, self.HL, self.A))
        check(self.lib.mobrob_ppo_sde_set_noise(self._h, _fp(z)))

    def rollout_begin(self):
        check(self.lib.mobrob_ppo_rollout_begin(self._h))

    def act(self, obs, eps=None, out_clipped=None, want_all=True):
        """-> (raw actions, clipped actions, values, log_probs).  With want_all=False only the clipped actions the
        env needs are copied back (raw actions / values / log-probs stay in the device rollout buffer);
        out_clipped may be a pinned array (engine.pinned) to skip the staging copy."""
        obs = _f32c(obs, (self.N, self.D))
        eps = None if eps is None else _f32c(eps, (self.N, self.A))
        a_clip = np.empty((self.N, self.A), F32) if out_clipped is None else out_clipped
        if not want_all:
            check(self.lib.mobrob_ppo_act(self._h, _fp(obs), _fp(eps), None, _fp(a_clip), None, None))
            return None, a_clip, None, None
        a_raw = np.empty((self.N, self.A), F32)
        val, lp = np.empty(self.N, F32), np.empty(self.N, F32)
        check(self.lib.mobrob_ppo_act(self._h, _fp(obs), _fp(eps), _fp(a_raw), _fp(a_clip), _fp(val), _fp(lp)))
        return a_raw, a_clip, val, lp

    def store(self, rewards, dones, truncated=None, terminal_obs=None):
        rewards = _f32c(rewards, (self.N,))
        dones = np.ascontiguousarray(dones, dtype=np.uint8)
        tr = None if truncated is None else np.ascontiguousarray(truncated, dtype=np.uint8)
        to = None if terminal_obs is None else _f32c(terminal_obs, (self.N, self.D))
        check(self.lib.mobrob_ppo_store(self._h, _fp(rewards), _u8(dones), _u8(tr), _fp(to)))

    def part_pipeline(self, nparts, obs, clipped, rewards, dones, truncated, terminal_obs):
        """Driver of the pipelined host-env rollout (mobrob_ppo_act_part / wait_part / store_part) over FULL [N][...]
        pinned arrays (`engine.pinned`); see PartPipeline."""
        return PartPipeline(self, nparts, obs, clipped, rewards, dones, truncated, terminal_obs)

    def finish_rollout(self, last_obs, dones):
        last_obs = _f32c(last_obs, (self.N, self.D))
        dones = np.ascontiguousarray(dones, dtype=np.uint8)
        check(self.lib.mobrob_ppo_finish_rollout(self._h, _fp(last_obs), _u8(dones)))

    def collect_synthetic(self, p_term=1.0 / 107.0, time_limit=1000):
        check(self.lib.mobrob_ppo_collect_synthetic(self._h, float(p_term), int(time_limit)))

    def collect_goal_env(self, pos_dim, mix, time_limit, terminate_on_goal=True, dt=0.05, extent=3.0, reach_radius=0.3,
                         goal_bonus=5.0, extra_bonus=0.0, obs_noise=0.1):
        """Whole rollout + GAE against the device-resident goal environment (mobrob_ppo_collect_goal_env).
        mix: [pos_dim, act_dim] action -> velocity command read-out."""
        g = GoalEnv()
        g.pos_dim, g.terminate_on_goal, g.time_limit = int(pos_dim), int(bool(terminate_on_goal)), int(time_limit)
        g.dt, g.extent, g.reach_radius = float(dt), float(extent), float(reach_radius)
        g.goal_bonus, g.extra_bonus, g.obs_noise = float(goal_bonus), float(extra_bonus), float(obs_noise)
        mix = np.asarray(mix, F32)
        if mix.shape != (int(pos_dim), self.A):
            raise ValueError(f"mix must be [{int(pos_dim)}, {self.A}], got {mix.shape}")
        for j in range(mix.shape[0]):
            for k in range(mix.shape[1]):
                g.mix[j][k] = float(mix[j, k])
        check(self.lib.mobrob_ppo_collect_goal_env(self._h, C.byref(g)))

    def _goal_env_struct(self, pos_dim, mix, time_limit, terminate_on_goal, dt, extent, reach_radius, goal_bonus, extra_bonus,
                         obs_noise):
        g = GoalEnv()
        g.pos_dim, g.terminate_on_goal, g.time_limit = int(pos_dim), int(bool(terminate_on_goal)), int(time_limit)
        g.dt, g.extent, g.reach_radius = float(dt), float(extent), float(reach_radius)
        g.goal_bonus, g.extra_bonus, g.obs_noise = float(goal_bonus), float(extra_bonus), float(obs_noise)
        mix = np.asarray(mix, F32)
        if mix.shape != (int(pos_dim), self.A):
            raise ValueError(f"mix must be [{int(pos_dim)}, {self.A}], got {mix.shape}")
        for j in range(mix.shape[0]):
            for k in range(mix.shape[1]):
                g.mix[j][k] = float(mix[j, k])
        return g

    @staticmethod
    def _hazards_struct(hazards, n):
        """mobrob_hazards_t of a goal_rules.Hazards (mobrob_hazard_frames_t of a goal_rules.MovingHazards) for n robots, and the
        arrays it points into (kept alive by the caller)."""
        from .envs.goal_rules import Hazards, MovingHazards
        if not isinstance(hazards, (Hazards, MovingHazards)):
            raise TypeError(f"hazards must be a mobrob_amd.envs.goal_rules.Hazards or MovingHazards, not {type(hazards).__name__}")
        hazards.check_robots(n)
        keep = (hazards.table, hazards.counts, hazards.scene)
        if isinstance(hazards, MovingHazards):
            h = HazardFramesC()
            h.n_frames, h.frame_steps, h.loop = hazards.n_frames, hazards.frame_steps, int(hazards.loop)
        else:
            h = HazardsC()
        h.n_scenes, h.max_hazards = hazards.n_scenes, hazards.max_hazards
        h.hazards, h.n_hazards = _fp(hazards.table), hazards.counts.ctypes.data_as(C.POINTER(C.c_int32))
        h.scene = None if hazards.scene is None else hazards.scene.ctypes.data_as(C.POINTER(C.c_int32))
        h.cost, h.indicator = hazards.cost, int(hazards.indicator)
        return h, keep

    @staticmethod
    def _hazard_result(hz):
        """The keys hazard_out adds to both calls' dicts."""
        return {"cost_sum": hz[:, 0], "violation_steps": hz[:, 1].astype(np.int64), "first_violation": hz[:, 2].astype(np.int64),
                "min_clearance": hz[:, 3]}

    def _eval_spec_common(self, what, sp, max_steps, deterministic, seed, trace, trace_extra=0):
        """What evaluate_goal_env and follow_waypoints fill alike in their spec (max_steps, deterministic, seed, trace sizes), after
        refusing sampled actions of a gSDE policy.  Returns the trace buffer, or None without a trace."""
        if self.use_sde and not deterministic:
            raise ValueError(f"{what}: stochastic actions of a use_sde (gSDE) policy are not supported; use deterministic=True")
        sp.max_steps, sp.deterministic, sp.seed = int(max_steps), int(bool(deterministic)), int(seed) & (2 ** 64 - 1)
        sp.trace_robots, sp.trace_steps = (0, 0) if trace is None else (int(trace[0]), int(trace[1]))
        if trace is None:
            return None
        return np.zeros((max(sp.trace_steps, 1), max(sp.trace_robots, 1), 9 + self.D + self.A + 4 + trace_extra), F32)

    @staticmethod
    def _eval_result(robot, r):
        """The keys both calls return from robot_out's first two columns and the C call's return value."""
        return {"reward_sum": robot[:, 0], "steps": robot[:, 1].astype(np.int64), "persistent": bool(r == 1)}

    def evaluate_goal_env(self, pos_dim, mix, time_limit=0, terminate_on_goal=True, dt=0.05, extent=3.0, reach_radius=0.3,
                          goal_bonus=5.0, extra_bonus=0.0, obs_noise=0.1, *, n_robots, max_steps=1000, episodes=0, quota=None,
                          deterministic=True, seed=0, trace=None, hazards=None, walls=None):
        """The current policy on `n_robots` fresh robots of the device goal environment (mobrob_ppo_evaluate_goal_env).
        time_limit 0: no limit (examples/control.py).  episodes > 0: SB3 evaluate_policy's quota of finished episodes, split
        (episodes + i) // n_robots unless `quota` ([n_robots] ints) is given.  trace = (robots, steps): teacher-forcing trace.
        Returns a dict of NumPy arrays: reward_sum, steps, episodes, goals ([n_robots]); episode_returns, episode_lengths,
        episode_success ([n_robots][max quota], NaN past an unfinished quota); trace ([steps][robots][9 + D + A + 4]) and
        `persistent` (which kernel path ran).  hazards: a goal_rules.Hazards -> mobrob_ppo_evaluate_goal_env_hazards, adding
        cost_sum, violation_steps, first_violation, min_clearance ([n_robots]) and episode_cost ([n_robots][max quota], NaN
        past an unfinished quota); trace rows then end in the step's cost and clearance.  A goal_rules.MovingHazards ->
        mobrob_ppo_evaluate_goal_env_hazard_frames: the same keys, the check after the call's step t on frame f(t).
        walls: refused (ValueError) -- an evaluation resets robots by teleporting them, and a swept segment across a reset has
        no meaning; walls belong to waypoint-following runs (follow_waypoints(walls=))."""
        if walls is not None:
            raise ValueError("evaluate: walls: an evaluation takes no walls (resets teleport robots); use follow_waypoints(walls=)")
        n = int(n_robots)
        sp = EvalSpec()
        tr = self._eval_spec_common("evaluate_goal_env", sp, max_steps, deterministic, seed, trace, 0 if hazards is None else 2)
        g = self._goal_env_struct(pos_dim, mix, time_limit, terminate_on_goal, dt, extent, reach_radius, goal_bonus, extra_bonus,
                                  obs_noise)
        sp.n_robots, sp.episodes = n, int(episodes)
        if quota is not None:
            q = np.ascontiguousarray(quota, dtype=np.int32)
            if q.shape != (max(n, 0),):
                raise ValueError(f"quota must have shape ({n},), got {q.shape}")
        elif int(episodes) > 0 and n > 0:
            q = ((int(episodes) + np.arange(n)) // n).astype(np.int32)
        else:
            q = np.zeros(max(n, 0), np.int32)
        maxq = int(q.max()) if q.size else 0
        robot = np.zeros((max(n, 1), 4), np.float64)
        ep = np.zeros((max(n, 1), max(maxq, 1), 3), np.float64)
        dp = C.POINTER(C.c_double)
        if hazards is None:
            r = check(self.lib.mobrob_ppo_evaluate_goal_env(self._h, C.byref(g), C.byref(sp), q.ctypes.data_as(C.POINTER(C.c_int32)),
                                                             robot.ctypes.data_as(dp), ep.ctypes.data_as(dp), _fp(tr)))
        else:
            h, _keep = self._hazards_struct(hazards, n)
            hz = np.zeros((max(n, 1), 4), np.float64)
            ec = np.zeros((max(n, 1), max(maxq, 1)), np.float64)
            call = (self.lib.mobrob_ppo_evaluate_goal_env_hazard_frames if isinstance(h, HazardFramesC)
                    else self.lib.mobrob_ppo_evaluate_goal_env_hazards)
            r = check(call(
                self._h, C.byref(g), C.byref(sp), C.byref(h), q.ctypes.data_as(C.POINTER(C.c_int32)), robot.ctypes.data_as(dp),
                ep.ctypes.data_as(dp), hz.ctypes.data_as(dp), ec.ctypes.data_as(dp), _fp(tr)))
        ep = ep[:, :maxq]
        done = np.arange(maxq)[None, :] < np.minimum(robot[:, 2:3], q[:, None])
        out = self._eval_result(robot, r)
        out.update({"episodes": robot[:, 2].astype(np.int64), "goals": robot[:, 3].astype(np.int64), "quota": q,
                    "episode_returns": np.where(done, ep[:, :, 0], np.nan), "episode_lengths": np.where(done, ep[:, :, 1], np.nan),
                    "episode_success": np.where(done, ep[:, :, 2], np.nan)})
        if hazards is not None:
            out.update(self._hazard_result(hz))
            out["episode_cost"] = np.where(done, ec[:, :maxq], np.nan)
        if tr is not None:
            out["trace"] = tr
        return out

    def follow_waypoints(self, pos_dim, mix, dt=0.05, extent=3.0, reach_radius=0.3, goal_bonus=5.0, extra_bonus=0.0,
                         obs_noise=0.1, *, start=None, waypoints=None, n_waypoints=None, max_steps=1000, deterministic=True, seed=0,
                         path_stride=0, trace=None, hazards=None, resume=None, leg_steps=0, teams=None, schedule=None,
                         walls=None):
        """The current policy as a tracker of given goal sequences (mobrob_ppo_follow_waypoints): robot i starts at rest on
        start[i] ([n][P]) and follows waypoints[i][:n_waypoints[i]] (waypoints [n][K][P], or [K][P] for all robots; n_waypoints
        None = K each), no time limit, no reset.  path_stride > 0 records positions; trace = (robots, steps): teacher-forcing
        trace.  Returns the dict of mobrob_amd.waypoints (arrival, reached, steps, reward_sum, final_distance, path, trace,
        persistent).  hazards: a goal_rules.Hazards -> mobrob_ppo_follow_waypoints_hazards, adding cost_sum, violation_steps,
        first_violation, min_clearance; trace rows then end in the step's cost and clearance.  A goal_rules.MovingHazards ->
        mobrob_ppo_follow_waypoints_hazard_frames (with or without `resume`): the check after global step g on frame f(g).
        resume: a waypoints.FollowState -> mobrob_ppo_follow_waypoints_resume, one call of the run the state is in (start,
        waypoints and n_waypoints must be None: the state holds them); leg_steps: step budget per waypoint (0: none).  With
        `leg_steps` alone the call starts a run.  Such a call adds `state` (the FollowState after the call; the one given is left
        as it was) and `status` [n] to the dict; steps, reached, reward_sum and the hazard sums are the run's, path and trace the
        call's.  teams: a goal_rules.Teams -> mobrob_ppo_follow_waypoints_teams (always a call of a run; without `resume` its
        first), adding team_cost_sum, conflict_steps, first_conflict, min_team_clearance, closest_partner and `state.team`.
        schedule: a goal_rules.Schedule -> mobrob_ppo_follow_waypoints_scheduled (always a call of a run; without `resume` its
        first: the state then takes release and home from it; with `resume` the state's are in force), adding hold_steps,
        hold_drift, lateness and `state.sched`; trace rows of hold steps carry the flags 0, 0.
        walls: a goal_rules.Walls -> mobrob_ppo_follow_waypoints_walls (always a call of a run; without `resume` its first),
        adding the keys of waypoints.wall_result (wall_cost_sum, contact_steps, first_contact, min_wall_clearance, closest_wall,
        crossing_steps, first_crossing) and `state.wall`; nothing else the call returns changes.  With walls.solid the walls
        block (mobrob_ppo_follow_waypoints_solid; goal_rules.wall_block states the rule): robots stop and slide at them, the
        dict gains the keys of waypoints.blocked_result (wall_blocked_steps, wall_first_blocked, wall_stopped_steps,
        wall_inside_steps) and `state.blocked`.  Solid walls with a MovingHazards are refused (ValueError naming `solid`).
        With teams.solid the mates block each other (mobrob_ppo_follow_waypoints_teams_solid; goal_rules.team_block_step states
        the rule), alone or with solid walls, with or without a schedule: the dict gains the keys of waypoints.team_blocked_result
        (team_blocked_steps, team_first_blocked, team_stopped_steps, team_inside_steps) and `state.team_blocked`.  Solid teams with
        hazards of either kind or with observational walls are refused (ValueError naming `Teams(solid=True)`)."""
        from .waypoints import FollowState, follow_inputs
        if resume is not None or int(leg_steps) != 0 or teams is not None or schedule is not None or walls is not None:
            if resume is None:
                resume = FollowState(start, waypoints, n_waypoints, hazards is not None, pos_dim, teams if teams is not None else False, schedule,
                                     walls if walls is not None else False)
            elif not (start is None and waypoints is None and n_waypoints is None):
                raise ValueError("follow_waypoints: a resumed call takes its robots and waypoints from `resume`")
            return self._follow_resume(pos_dim, mix, dt, extent, reach_radius, goal_bonus, extra_bonus, obs_noise, resume,
                                       int(leg_steps), max_steps, deterministic, seed, path_stride, trace, hazards, teams, schedule,
                                       walls)
        if start is None or waypoints is None:
            raise ValueError("follow_waypoints: start and waypoints are needed unless `resume` continues a run")
        s, wp, nw = follow_inputs(start, waypoints, n_waypoints, pos_dim)
        n, K, P = wp.shape
        sp = FollowSpec()
        tr = self._eval_spec_common("follow_waypoints", sp, max_steps, deterministic, seed, trace, 0 if hazards is None else 2)
        g = self._goal_env_struct(pos_dim, mix, 0, False, dt, extent, reach_radius, goal_bonus, extra_bonus, obs_noise)
        sp.n_robots, sp.max_waypoints, sp.path_stride = n, K, int(path_stride)
        arrival = np.empty((n, K), np.int32)
        robot = np.zeros((n, 4), np.float64)
        path = np.zeros((int(max_steps) // int(path_stride) + 1, n, P), F32) if int(path_stride) > 0 and int(max_steps) > 0 else None
        i32, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        if hazards is None:
            r = check(self.lib.mobrob_ppo_follow_waypoints(self._h, C.byref(g), C.byref(sp), _fp(s), _fp(wp), nw.ctypes.data_as(i32),
                                                            arrival.ctypes.data_as(i32), robot.ctypes.data_as(dp), _fp(path), _fp(tr)))
        else:
            h, _keep = self._hazards_struct(hazards, n)
            hz = np.zeros((n, 4), np.float64)
            tail = (_fp(s), _fp(wp), nw.ctypes.data_as(i32), arrival.ctypes.data_as(i32), robot.ctypes.data_as(dp),
                    hz.ctypes.data_as(dp), _fp(path), _fp(tr))
            if isinstance(h, HazardFramesC):
                r = check(self.lib.mobrob_ppo_follow_waypoints_hazard_frames(self._h, C.byref(g), C.byref(sp), C.byref(h), None, *tail))
            else:
                r = check(self.lib.mobrob_ppo_follow_waypoints_hazards(self._h, C.byref(g), C.byref(sp), C.byref(h), *tail))
        out = self._eval_result(robot, r)
        out.update({"arrival": arrival.astype(np.int64), "reached": robot[:, 2].astype(np.int64), "final_distance": robot[:, 3],
                    "trace": tr})
        if hazards is not None:
            out.update(self._hazard_result(hz))
        if path is not None:
            out["path"] = path
        return out

    def _follow_resume(self, pos_dim, mix, dt, extent, reach_radius, goal_bonus, extra_bonus, obs_noise, state, leg_steps,
                       max_steps, deterministic, seed, path_stride, trace, hazards, teams=None, schedule=None, walls=None):
        """One call of a run (mobrob_ppo_follow_waypoints_resume; with a MovingHazards mobrob_ppo_follow_waypoints_hazard_frames;
        with teams mobrob_ppo_follow_waypoints_teams; with a schedule mobrob_ppo_follow_waypoints_scheduled; with walls
        mobrob_ppo_follow_waypoints_walls) on a copy of `state`."""
        from ._lib import FollowResume, FollowScheduleC, TeamsC, WallsC
        from .envs.goal_rules import Schedule, Teams, Walls
        from .envs.goal_rules import MovingHazards
        from .waypoints import (FollowState, blocked_result, schedule_result, team_blocked_result, team_result, team_solid_check,
                                wall_result)
        if not isinstance(state, FollowState):
            raise TypeError(f"follow_waypoints: resume must be a FollowState, not {type(state).__name__}")
        if (state.hazard is None) != (hazards is None):
            raise ValueError("follow_waypoints: a run has hazards in every call or in none (FollowState(..., hazards=True))")
        if (getattr(state, "team", None) is None) != (teams is None):
            raise ValueError("follow_waypoints: a run has teams in every call or in none (FollowState(..., teams=True))")
        if teams is not None:
            if not isinstance(teams, Teams):
                raise TypeError(f"teams must be a mobrob_amd.envs.goal_rules.Teams, not {type(teams).__name__}")
            teams.check_robots(state.n_robots)
        tsolid = team_solid_check(state, hazards, teams, walls)
        if (getattr(state, "release", None) is None) != (schedule is None):
            raise ValueError("follow_waypoints: a run has a schedule in every call or in none (FollowState(..., schedule=Schedule))")
        if schedule is not None and not isinstance(schedule, Schedule):
            raise TypeError(f"schedule must be a mobrob_amd.envs.goal_rules.Schedule, not {type(schedule).__name__}")
        if (getattr(state, "wall", None) is None) != (walls is None):
            raise ValueError("follow_waypoints: a run has walls in every call or in none (FollowState(..., walls=True))")
        if walls is not None:
            if not isinstance(walls, Walls):
                raise TypeError(f"walls must be a mobrob_amd.envs.goal_rules.Walls, not {type(walls).__name__}")
            walls.check_robots(state.n_robots)
        solid = walls is not None and bool(getattr(walls, "solid", False))
        if (getattr(state, "blocked", None) is None) == solid:
            raise ValueError("follow_waypoints: a run has solid walls in every call or in none (FollowState(..., walls=Walls(..., solid=True)))")
        if solid and isinstance(hazards, MovingHazards):
            raise ValueError("follow_waypoints: solid=True does not run with MovingHazards yet (static hazards, teams and schedules do)")
        st = state.copy()
        n, K, P = st.waypoints.shape
        if P != int(pos_dim):
            raise ValueError(f"follow_waypoints: the state has {P} position dimensions, the environment {int(pos_dim)}")
        st.state, st.waypoints = np.ascontiguousarray(st.state, F32), np.ascontiguousarray(st.waypoints, F32)
        st.robot = np.ascontiguousarray(st.robot, np.float64)
        st.arrival, st.n_waypoints, st.leg_used, st.status = (np.ascontiguousarray(x, np.int32) for x in
                                                             (st.arrival, st.n_waypoints, st.leg_used, st.status))
        if st.hazard is not None:
            st.hazard = np.ascontiguousarray(st.hazard, np.float64)
        if teams is not None:
            st.team = np.ascontiguousarray(st.team, np.float64)
            if st.team.shape != (n, 5):
                raise ValueError("follow_waypoints: the arrays of `resume` do not fit its waypoints")
        if schedule is not None:
            st.release, st.home = np.ascontiguousarray(st.release, np.int32), np.ascontiguousarray(st.home, F32)
            st.sched = np.ascontiguousarray(st.sched, np.float64)
            if st.release.shape != (n, K) or st.home.shape != (n, P) or st.sched.shape != (n, 2):
                raise ValueError("follow_waypoints: the arrays of `resume` do not fit its waypoints")
        if walls is not None:
            st.wall = np.ascontiguousarray(st.wall, np.float64)
            if st.wall.shape != (n, 7):
                raise ValueError("follow_waypoints: the arrays of `resume` do not fit its waypoints")
        if solid:
            st.blocked = np.ascontiguousarray(st.blocked, np.int32)
            if st.blocked.shape != (n, 4):
                raise ValueError("follow_waypoints: the arrays of `resume` do not fit its waypoints")
        if tsolid:
            st.team_blocked = np.ascontiguousarray(st.team_blocked, np.int32)
        if st.state.shape != (n, 6) or st.robot.shape != (n, 4) or st.arrival.shape != (n, K) or st.leg_used.shape != (n,):
            raise ValueError("follow_waypoints: the arrays of `resume` do not fit its waypoints")
        sp = FollowSpec()
        tr = self._eval_spec_common("follow_waypoints", sp, max_steps, deterministic, seed, trace, 0 if hazards is None else 2)
        g = self._goal_env_struct(pos_dim, mix, 0, False, dt, extent, reach_radius, goal_bonus, extra_bonus, obs_noise)
        sp.n_robots, sp.max_waypoints, sp.path_stride = n, K, int(path_stride)
        path = np.zeros((int(max_steps) // int(path_stride) + 1, n, P), F32) if int(path_stride) > 0 and int(max_steps) > 0 else None
        i32, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        rs = FollowResume()
        if not (-2 ** 31 <= int(st.step0) < 2 ** 31 and -2 ** 31 <= int(leg_steps) < 2 ** 31):
            raise ValueError("follow_waypoints: step0 and leg_steps must fit an int32")
        rs.step0, rs.leg_steps = int(st.step0), int(leg_steps)
        rs.state, rs.leg_used, rs.status = _fp(st.state), st.leg_used.ctypes.data_as(i32), st.status.ctypes.data_as(i32)
        h, _keep = (None, None) if hazards is None else self._hazards_struct(hazards, n)
        tail = (_fp(st.waypoints), st.n_waypoints.ctypes.data_as(i32), st.arrival.ctypes.data_as(i32), st.robot.ctypes.data_as(dp),
                None if h is None else st.hazard.ctypes.data_as(dp), _fp(path), _fp(tr))
        tm = None
        if teams is not None:
            tm = TeamsC()
            tm.team_size, tm.separation, tm.cost, tm.indicator = teams.size, teams.separation, teams.cost, int(teams.indicator)
        frames = isinstance(h, HazardFramesC)
        sc = None
        if schedule is not None:
            sc = FollowScheduleC()
            sc.release, sc.home = st.release.ctypes.data_as(i32), _fp(st.home)
        if tsolid:
            wl = None
            if walls is not None:
                wl = WallsC()
                wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
                wl.boxes, wl.n_walls = _fp(walls.table), walls.counts.ctypes.data_as(i32)
                wl.scene = None if walls.scene is None else walls.scene.ctypes.data_as(i32)
                wl.radius, wl.cost, wl.indicator = walls.radius, walls.cost, int(walls.indicator)
            r = check(self.lib.mobrob_ppo_follow_waypoints_teams_solid(
                self._h, C.byref(g), C.byref(sp), None, None, C.byref(rs), C.byref(tm), None if sc is None else C.byref(sc),
                None if wl is None else C.byref(wl), *tail[:5], st.team.ctypes.data_as(dp),
                None if sc is None else st.sched.ctypes.data_as(dp), None if wl is None else st.wall.ctypes.data_as(dp),
                None if wl is None else st.blocked.ctypes.data_as(i32), st.team_blocked.ctypes.data_as(i32), *tail[5:]))
        elif walls is not None:
            wl = WallsC()
            wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
            wl.boxes, wl.n_walls = _fp(walls.table), walls.counts.ctypes.data_as(i32)
            wl.scene = None if walls.scene is None else walls.scene.ctypes.data_as(i32)
            wl.radius, wl.cost, wl.indicator = walls.radius, walls.cost, int(walls.indicator)
            head = (self._h, C.byref(g), C.byref(sp), None if h is None or frames else C.byref(h), C.byref(h) if frames else None,
                    C.byref(rs), None if tm is None else C.byref(tm), None if sc is None else C.byref(sc), C.byref(wl), *tail[:5],
                    None if tm is None else st.team.ctypes.data_as(dp), None if sc is None else st.sched.ctypes.data_as(dp),
                    st.wall.ctypes.data_as(dp))
            if solid:
                r = check(self.lib.mobrob_ppo_follow_waypoints_solid(*head, st.blocked.ctypes.data_as(i32), *tail[5:]))
            else:
                r = check(self.lib.mobrob_ppo_follow_waypoints_walls(*head, *tail[5:]))
        elif schedule is not None:
            r = check(self.lib.mobrob_ppo_follow_waypoints_scheduled(
                self._h, C.byref(g), C.byref(sp), None if h is None or frames else C.byref(h), C.byref(h) if frames else None,
                C.byref(rs), None if tm is None else C.byref(tm), C.byref(sc), *tail[:5],
                None if tm is None else st.team.ctypes.data_as(dp), st.sched.ctypes.data_as(dp), *tail[5:]))
        elif teams is not None:
            r = check(self.lib.mobrob_ppo_follow_waypoints_teams(
                self._h, C.byref(g), C.byref(sp), None if h is None or frames else C.byref(h), C.byref(h) if frames else None,
                C.byref(rs), C.byref(tm), *tail[:5], st.team.ctypes.data_as(dp), *tail[5:]))
        elif isinstance(h, HazardFramesC):
            r = check(self.lib.mobrob_ppo_follow_waypoints_hazard_frames(self._h, C.byref(g), C.byref(sp), C.byref(h), C.byref(rs),
                                                                         None, *tail))
        else:
            r = check(self.lib.mobrob_ppo_follow_waypoints_resume(self._h, C.byref(g), C.byref(sp), None if h is None else C.byref(h),
                                                                  C.byref(rs), *tail))
        st.step0 += int(max_steps)
        out = self._eval_result(st.robot.copy(), r)
        out.update({"arrival": st.arrival.astype(np.int64), "reached": st.reached, "final_distance": st.robot[:, 3].copy(),
                    "trace": tr, "state": st, "status": st.status.copy()})
        if hazards is not None:
            out.update(self._hazard_result(st.hazard.copy()))
        if teams is not None:
            out.update(team_result(st.team))
        if schedule is not None:
            out.update(schedule_result(st))
        if walls is not None:
            out.update(wall_result(st))
        if solid:
            out.update(blocked_result(st))
        if tsolid:
            out.update(team_blocked_result(st))
        if path is not None:
            out["path"] = path
        return out

    def spec_monitor(self, spec, path, step0=0, state=None):
        """A specification folded over the positions of one call of a run (mobrob_ppo_spec_monitor; the rule: goal_rules.spec_fold,
        reproduced bit for bit).  spec: a goal_rules.Spec; path [T + 1][n][P] as follow_waypoints returns it with path_stride=1;
        step0: the run's global step at the call's entry; state: the goal_rules.SpecState the previous call returned (None:
        spec_start).  Returns (the new SpecState, goal_rules.spec_result of it).  A specification with a nested clause (Spec.stay /
        Spec.recur) goes through mobrob_ppo_spec_monitor_nested, which also carries the state's tail; one without takes
        mobrob_ppo_spec_monitor as before.  A `dynamic` specification -- moving regions or a mate predicate -- goes through
        mobrob_ppo_spec_monitor_moving, flat and nested clauses alike; one that is not takes the call it took."""
        from ._lib import SpecC, SpecMovingC, SpecNestedC
        from .envs.goal_rules import SPEC_UNTIL, Spec, SpecState, spec_check_state, spec_predicate_words, spec_result, spec_start
        if not isinstance(spec, Spec):
            raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.Spec, not {type(spec).__name__}")
        path = np.ascontiguousarray(path, F32)
        if path.ndim != 3:
            raise ValueError(f"spec_monitor: path must be [T + 1][n][P], got shape {path.shape}")
        T, n, P = path.shape[0] - 1, path.shape[1], path.shape[2]
        reg = spec.regions
        spec.check_robots(n)
        if state is None:
            state = spec_start(n, spec)
        spec_check_state(state, n, spec)
        if not -2 ** 31 <= int(step0) < 2 ** 31:
            raise ValueError("spec_monitor: step0 must fit an int32")
        new = state.copy()
        i32 = C.POINTER(C.c_int32)
        sp = SpecMovingC() if spec.dynamic else SpecNestedC() if spec.nested else SpecC()
        sp.n_scenes, sp.max_regions, sp.n_clauses = reg.n_scenes, reg.max_regions, spec.n_clauses
        sp.regions, sp.kinds, sp.n_regions = _fp(reg.table), reg.kinds.ctypes.data_as(i32), reg.counts.ctypes.data_as(i32)
        sp.scene = None if reg.scene is None else reg.scene.ctypes.data_as(i32)
        for c, (op, a, b, p1, p2) in enumerate(cl[:5] for cl in spec.clauses):
            sp.op[c], sp.a[c], sp.b[c] = op, a, b
            w1, w2 = spec_predicate_words(p1), spec_predicate_words(p2)
            sp.lo1[c], sp.hi1[c], sp.out1[c] = w1[:3]
            if op == SPEC_UNTIL:
                sp.lo2[c], sp.hi2[c], sp.out2[c] = w2[:3]
            if spec.dynamic:
                sp.kind1[c], sp.rad1[c] = w1[3:]
                if op == SPEC_UNTIL:
                    sp.kind2[c], sp.rad2[c] = w2[3:]
        if spec.dynamic:
            for c, h in enumerate(spec.holds):
                sp.hold[c] = h
            sp.team_size = spec.team_size
            # a static table [S][R][4] is the one frame of [S][1][R][4]
            sp.n_frames, sp.frame_steps, sp.loop = (reg.n_frames, reg.frame_steps, int(reg.loop)) if spec.moving else (1, 1, 0)
            W = spec.tail_width
            check(self.lib.mobrob_ppo_spec_monitor_moving(self._h, C.byref(sp), _fp(path), n, T, P, int(step0), _fp(new.val),
                                                          new.wit.ctypes.data_as(i32), _fp(new.tail) if W else None, W))
        elif spec.nested:
            for c, h in enumerate(spec.holds):
                sp.hold[c] = h
            W = spec.tail_width
            check(self.lib.mobrob_ppo_spec_monitor_nested(self._h, C.byref(sp), _fp(path), n, T, P, int(step0), _fp(new.val),
                                                          new.wit.ctypes.data_as(i32), _fp(new.tail) if W else None, W))
        else:
            check(self.lib.mobrob_ppo_spec_monitor(self._h, C.byref(sp), _fp(path), n, T, P, int(step0), _fp(new.val),
                                                   new.wit.ctypes.data_as(i32)))
        return new, spec_result(new, spec)

    def plan_grid(self, spec, walls=None, hazards=None, *, start, goal, max_waypoints=16, want_occupancy=False, want_fields=False,
                  reuse=None):
        """Waypoints for every robot from a grid over the scene (mobrob_ppo_plan_grid; the rule: goal_rules.grid_occupancy /
        grid_field / grid_path, reproduced bit for bit).  spec: a goal_rules.GridSpec; walls / hazards: a goal_rules.Walls /
        Hazards or None; start, goal [n][P] (P = 2 or 3).  Robots that share a scene and a goal cell share a field (deduplicated
        here with NumPy).  Returns a dict: waypoints [n][K][P] float32, n_waypoints, count, status (goal_rules.PLANNED,
        UNREACHABLE, TRUNCATED, UNCONVERGED), cost [n] int32, field_of [n], field_goal_cell [F], field_scene [F], sweeps [F] (the
        relaxation sweeps of each field; None on a reused call), fields_id, and on request occupancy bool [S][G][G] and fields int32
        [F][G][G].  reuse: the dict a previous call returned -- its fields are still on the device (same scene, same goal cells:
        ValueError otherwise) and only the paths are walked again."""
        from ._lib import PlanSpec, WallsC
        from .envs.goal_rules import GridSpec, plan_fields, plan_scene
        if not isinstance(spec, GridSpec):
            raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.GridSpec, not {type(spec).__name__}")
        start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
        if goal.ndim != 2 or goal.shape[0] < 1 or goal.shape[1] not in (2, 3) or start.shape != goal.shape:
            raise ValueError(f"plan: start and goal must both be [n_robots, 2 or 3], got shapes {start.shape} and {goal.shape}")
        if not (np.all(np.isfinite(start)) and np.all(np.isfinite(goal))):
            raise ValueError("plan: start and goal must be finite")
        n, P = goal.shape
        K = int(max_waypoints)
        if K < 1:
            raise ValueError("plan: max_waypoints must be >= 1")
        S, scene = plan_scene(walls, hazards)
        for sc in (walls, hazards):
            if sc is not None:
                sc.check_robots(n)
        start, goal = np.ascontiguousarray(start, F32), np.ascontiguousarray(goal, F32)
        field_of, fcell, fscene = plan_fields(spec, None, scene, goal)
        if reuse is not None and not (np.array_equal(reuse["field_goal_cell"], fcell) and np.array_equal(reuse["field_scene"], fscene)):
            raise ValueError("plan: reuse: the goal cells or scenes are not those of the fields to reuse")
        Fn, G = len(fcell), spec.cells
        i32 = C.POINTER(C.c_int32)
        sp = PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n, P, G, K, S, Fn
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), float(spec.inflate_for(walls))
        sp.reuse_id = 0 if reuse is None else int(reuse["fields_id"])
        wl = None
        if walls is not None:
            wl = WallsC()
            wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
            wl.boxes, wl.n_walls = _fp(walls.table), walls.counts.ctypes.data_as(i32)
            wl.scene = None if walls.scene is None else walls.scene.ctypes.data_as(i32)
            wl.radius, wl.cost, wl.indicator = walls.radius, walls.cost, int(walls.indicator)
        h, _keep = (None, None) if hazards is None else self._hazards_struct(hazards, n)
        wp = np.zeros((n, K, P), F32)
        nwp, count, status, cost = (np.zeros(n, np.int32) for _ in range(4))
        occ = np.zeros((S, G, G), np.uint8) if want_occupancy else None
        fields = np.zeros((Fn, G, G), np.int32) if want_fields else None
        sweeps = np.zeros(Fn, np.int32) if reuse is None else None
        fid = C.c_int64(0)
        check(self.lib.mobrob_ppo_plan_grid(
            self._h, C.byref(sp), None if wl is None else C.byref(wl), None if h is None else C.byref(h), _fp(start), _fp(goal),
            field_of.ctypes.data_as(i32), fcell.ctypes.data_as(i32), fscene.ctypes.data_as(i32), _fp(wp), nwp.ctypes.data_as(i32),
            count.ctypes.data_as(i32), status.ctypes.data_as(i32), cost.ctypes.data_as(i32),
            None if occ is None else occ.ctypes.data_as(C.POINTER(C.c_uint8)), None if fields is None else fields.ctypes.data_as(i32),
            None if sweeps is None else sweeps.ctypes.data_as(i32), C.byref(fid)))
        out = {"waypoints": wp, "n_waypoints": nwp, "count": count, "status": status, "cost": cost, "field_of": field_of,
               "field_goal_cell": fcell, "field_scene": fscene, "sweeps": sweeps, "fields_id": int(fid.value), "n_scenes": int(S)}
        if occ is not None:
            out["occupancy"] = occ.astype(bool)
        if fields is not None:
            out["fields"] = fields
        return out

    def plan_smooth(self, spec, *, reuse, start, goal, scene=None, max_waypoints=16, margin=1):
        """Line-of-sight smoothed waypoints on the fields a plan_grid call left on the device (mobrob_ppo_plan_smooth; the rule:
        goal_rules.grid_los / grid_smooth / grid_path_smooth, reproduced bit for bit).  reuse: the dict that plan_grid call
        returned (the same scenes and goal cells: ValueError otherwise; fields no longer resident: EngineError); scene [n] or
        None: the scene index per robot (the walls' / hazards' own); margin: 0 or 1, the clearance of the line-of-sight test in
        cells.  Returns waypoints [n][K][P] float32, n_waypoints, count, status, cost as plan_grid does, moves [n] int32 (the
        moves of each walk) and field_of, field_goal_cell, field_scene, fields_id."""
        from ._lib import PlanSpec
        from .envs.goal_rules import GridSpec, plan_fields
        if not isinstance(spec, GridSpec):
            raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.GridSpec, not {type(spec).__name__}")
        start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
        if goal.ndim != 2 or goal.shape[0] < 1 or goal.shape[1] not in (2, 3) or start.shape != goal.shape:
            raise ValueError(f"plan_smooth: start and goal must both be [n_robots, 2 or 3], got shapes {start.shape} and {goal.shape}")
        if not (np.all(np.isfinite(start)) and np.all(np.isfinite(goal))):
            raise ValueError("plan_smooth: start and goal must be finite")
        n, P = goal.shape
        K = int(max_waypoints)
        if K < 1:
            raise ValueError("plan_smooth: max_waypoints must be >= 1")
        if scene is not None:
            scene = np.ascontiguousarray(scene, np.int32)
            if scene.shape != (n,):
                raise ValueError(f"plan_smooth: scene must be [n_robots = {n}], got shape {scene.shape}")
        start, goal = np.ascontiguousarray(start, F32), np.ascontiguousarray(goal, F32)
        field_of, fcell, fscene = plan_fields(spec, None, scene, goal)
        if not (np.array_equal(reuse["field_goal_cell"], fcell) and np.array_equal(reuse["field_scene"], fscene)):
            raise ValueError("plan_smooth: the goal cells or scenes are not those of the resident fields")
        i32 = C.POINTER(C.c_int32)
        sp = PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_fields = n, P, spec.cells, K, len(fcell)
        sp.n_scenes = int(reuse.get("n_scenes", int(fscene.max()) + 1))
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), 0.0
        sp.reuse_id = int(reuse["fields_id"])
        wp = np.zeros((n, K, P), F32)
        nwp, count, status, cost, moves = (np.zeros(n, np.int32) for _ in range(5))
        check(self.lib.mobrob_ppo_plan_smooth(
            self._h, C.byref(sp), int(margin), _fp(start), _fp(goal), field_of.ctypes.data_as(i32),
            None if scene is None else scene.ctypes.data_as(i32), _fp(wp), nwp.ctypes.data_as(i32), count.ctypes.data_as(i32),
            status.ctypes.data_as(i32), cost.ctypes.data_as(i32), moves.ctypes.data_as(i32)))
        return {"waypoints": wp, "n_waypoints": nwp, "count": count, "status": status, "cost": cost, "moves": moves,
                "field_of": field_of, "field_goal_cell": fcell, "field_scene": fscene, "fields_id": int(reuse["fields_id"]),
                "n_scenes": int(sp.n_scenes)}

    def plan_grid_clear(self, spec, walls=None, hazards=None, *, clearance, start, goal, max_waypoints=16, want_occupancy=False,
                        want_fields=False, want_surcharge=False, reuse=None):
        """plan_grid with a surcharge on cells near blocked ones (mobrob_ppo_plan_grid_clear; the rule: goal_rules.grid_plan(...,
        clearance=(reach, weight)), reproduced bit for bit).  clearance: (reach 1 .. 8, weight 1 .. 16).  Returns plan_grid's dict
        -- `fields` are the cost fields with the surcharges in them, `cost` includes the surcharges paid -- and clearance_min [n]
        int32, `clearance` itself, on request surcharge uint8 [S][G][G].  reuse: the dict a previous plan_grid_clear call returned
        (a plan_grid dict names fields of the other family: EngineError)."""
        from ._lib import PlanSpec, WallsC
        from .envs.goal_rules import GridSpec, plan_clearance_check, plan_fields, plan_scene
        if not isinstance(spec, GridSpec):
            raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.GridSpec, not {type(spec).__name__}")
        reach, weight = plan_clearance_check(clearance)
        start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
        if goal.ndim != 2 or goal.shape[0] < 1 or goal.shape[1] not in (2, 3) or start.shape != goal.shape:
            raise ValueError(f"plan_grid_clear: start and goal must both be [n_robots, 2 or 3], got shapes {start.shape} and {goal.shape}")
        if not (np.all(np.isfinite(start)) and np.all(np.isfinite(goal))):
            raise ValueError("plan_grid_clear: start and goal must be finite")
        n, P = goal.shape
        K = int(max_waypoints)
        if K < 1:
            raise ValueError("plan_grid_clear: max_waypoints must be >= 1")
        S, scene = plan_scene(walls, hazards)
        for sc in (walls, hazards):
            if sc is not None:
                sc.check_robots(n)
        start, goal = np.ascontiguousarray(start, F32), np.ascontiguousarray(goal, F32)
        field_of, fcell, fscene = plan_fields(spec, None, scene, goal)
        if reuse is not None and not (np.array_equal(reuse["field_goal_cell"], fcell) and np.array_equal(reuse["field_scene"], fscene)):
            raise ValueError("plan_grid_clear: reuse: the goal cells or scenes are not those of the fields to reuse")
        Fn, G = len(fcell), spec.cells
        i32, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        sp = PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n, P, G, K, S, Fn
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), float(spec.inflate_for(walls))
        sp.reuse_id = 0 if reuse is None else int(reuse["fields_id"])
        wl = None
        if walls is not None:
            wl = WallsC()
            wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
            wl.boxes, wl.n_walls = _fp(walls.table), walls.counts.ctypes.data_as(i32)
            wl.scene = None if walls.scene is None else walls.scene.ctypes.data_as(i32)
            wl.radius, wl.cost, wl.indicator = walls.radius, walls.cost, int(walls.indicator)
        h, _keep = (None, None) if hazards is None else self._hazards_struct(hazards, n)
        wp = np.zeros((n, K, P), F32)
        nwp, count, status, cost, cmin = (np.zeros(n, np.int32) for _ in range(5))
        occ = np.zeros((S, G, G), np.uint8) if want_occupancy else None
        pen = np.zeros((S, G, G), np.uint8) if want_surcharge else None
        fields = np.zeros((Fn, G, G), np.int32) if want_fields else None
        sweeps = np.zeros(Fn, np.int32) if reuse is None else None
        fid = C.c_int64(0)
        check(self.lib.mobrob_ppo_plan_grid_clear(
            self._h, C.byref(sp), None if wl is None else C.byref(wl), None if h is None else C.byref(h), reach, weight, _fp(start),
            _fp(goal), field_of.ctypes.data_as(i32), fcell.ctypes.data_as(i32), fscene.ctypes.data_as(i32), _fp(wp),
            nwp.ctypes.data_as(i32), count.ctypes.data_as(i32), status.ctypes.data_as(i32), cost.ctypes.data_as(i32),
            cmin.ctypes.data_as(i32), None if occ is None else occ.ctypes.data_as(u8),
            None if fields is None else fields.ctypes.data_as(i32), None if sweeps is None else sweeps.ctypes.data_as(i32),
            None if pen is None else pen.ctypes.data_as(u8), C.byref(fid)))
        out = {"waypoints": wp, "n_waypoints": nwp, "count": count, "status": status, "cost": cost, "clearance_min": cmin,
               "field_of": field_of, "field_goal_cell": fcell, "field_scene": fscene, "sweeps": sweeps, "fields_id": int(fid.value),
               "n_scenes": int(S), "clearance": (reach, weight)}
        if occ is not None:
            out["occupancy"] = occ.astype(bool)
        if pen is not None:
            out["surcharge"] = pen
        if fields is not None:
            out["fields"] = fields
        return out

    def plan_smooth_clear(self, spec, *, reuse, start, goal, scene=None, max_waypoints=16, margin=1):
        """plan_smooth on the fields a plan_grid_clear call left on the device (mobrob_ppo_plan_smooth_clear): the clearance-aware
        walk, smoothed by the same line-of-sight rule (goal_rules.grid_plan(..., smooth=True, clearance=)), bit for bit.  reuse:
        the dict that plan_grid_clear call returned.  Returns plan_smooth's dict and clearance_min [n] int32."""
        from ._lib import PlanSpec
        from .envs.goal_rules import GridSpec, plan_fields
        if not isinstance(spec, GridSpec):
            raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.GridSpec, not {type(spec).__name__}")
        start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
        if goal.ndim != 2 or goal.shape[0] < 1 or goal.shape[1] not in (2, 3) or start.shape != goal.shape:
            raise ValueError(f"plan_smooth_clear: start and goal must both be [n_robots, 2 or 3], got shapes {start.shape} and {goal.shape}")
        if not (np.all(np.isfinite(start)) and np.all(np.isfinite(goal))):
            raise ValueError("plan_smooth_clear: start and goal must be finite")
        n, P = goal.shape
        K = int(max_waypoints)
        if K < 1:
            raise ValueError("plan_smooth_clear: max_waypoints must be >= 1")
        if scene is not None:
            scene = np.ascontiguousarray(scene, np.int32)
            if scene.shape != (n,):
                raise ValueError(f"plan_smooth_clear: scene must be [n_robots = {n}], got shape {scene.shape}")
        start, goal = np.ascontiguousarray(start, F32), np.ascontiguousarray(goal, F32)
        field_of, fcell, fscene = plan_fields(spec, None, scene, goal)
        if not (np.array_equal(reuse["field_goal_cell"], fcell) and np.array_equal(reuse["field_scene"], fscene)):
            raise ValueError("plan_smooth_clear: the goal cells or scenes are not those of the resident fields")
        i32 = C.POINTER(C.c_int32)
        sp = PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_fields = n, P, spec.cells, K, len(fcell)
        sp.n_scenes = int(reuse.get("n_scenes", int(fscene.max()) + 1))
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), 0.0
        sp.reuse_id = int(reuse["fields_id"])
        wp = np.zeros((n, K, P), F32)
        nwp, count, status, cost, moves, cmin = (np.zeros(n, np.int32) for _ in range(6))
        check(self.lib.mobrob_ppo_plan_smooth_clear(
            self._h, C.byref(sp), int(margin), _fp(start), _fp(goal), field_of.ctypes.data_as(i32),
            None if scene is None else scene.ctypes.data_as(i32), _fp(wp), nwp.ctypes.data_as(i32), count.ctypes.data_as(i32),
            status.ctypes.data_as(i32), cost.ctypes.data_as(i32), moves.ctypes.data_as(i32), cmin.ctypes.data_as(i32)))
        return {"waypoints": wp, "n_waypoints": nwp, "count": count, "status": status, "cost": cost, "moves": moves,
                "clearance_min": cmin, "field_of": field_of, "field_goal_cell": fcell, "field_scene": fscene,
                "fields_id": int(reuse["fields_id"]), "n_scenes": int(sp.n_scenes)}

    def plan_grid_time(self, spec, walls=None, hazards=None, *, start, goal, step0=0, layer_steps, layers=64, max_waypoints=16,
                       want_occupancy=False, want_fields=False):
        """Waypoints and release steps for every robot among hazards that move (mobrob_ppo_plan_grid_time; the rule:
        goal_rules.grid_plan_time, reproduced bit for bit).  hazards: a goal_rules.MovingHazards; step0: the global step at
        which the plan starts; layer_steps: the steps a robot is given for one move or wait; layers: T, the actions planned in
        time before the conservative tail.  Returns plan_grid's dict (sweeps: the tail's; no fields_id -- every call computes
        and keeps nothing resident, fields a plan_grid call left resident stay valid) plus waits, leave [n][K] int32, arrive
        [n] int32 and release [n][K] int32 (goal_rules.grid_release: Schedule's release steps), and on request occupancy bool
        [S][T + 1][G][G] and fields int32 [F][T + 1][G][G]."""
        return self._plan_time(spec, walls, hazards, start, goal, step0, layer_steps, layers, max_waypoints, want_occupancy, want_fields)

    def _plan_time(self, spec, walls, hazards, start, goal, step0, layer_steps, layers, max_waypoints, want_occupancy, want_fields,
                   smooth=None, want_next_blocked=False):
        """plan_grid_time's call (smooth None) or plan_smooth_time's (smooth: the margin): the checks and the arrays of both"""
        from ._lib import PlanSpec, PlanTime, WallsC
        from .envs import goal_rules as R
        if not isinstance(spec, R.GridSpec):
            raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.GridSpec, not {type(spec).__name__}")
        start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
        if goal.ndim != 2 or goal.shape[0] < 1 or goal.shape[1] not in (2, 3) or start.shape != goal.shape:
            raise ValueError(f"plan_time: start and goal must both be [n_robots, 2 or 3], got shapes {start.shape} and {goal.shape}")
        if not (np.all(np.isfinite(start)) and np.all(np.isfinite(goal))):
            raise ValueError("plan_time: start and goal must be finite")
        n, P = goal.shape
        K = int(max_waypoints)
        if K < 1:
            raise ValueError("plan_time: max_waypoints must be >= 1")
        S, scene = R.plan_scene_time(walls, hazards)
        step0, layer_steps, T = R.plan_time_check(step0, layer_steps, layers)
        for sc in (walls, hazards):
            if sc is not None:
                sc.check_robots(n)
        start, goal = np.ascontiguousarray(start, F32), np.ascontiguousarray(goal, F32)
        field_of, fcell, fscene = R.plan_fields(spec, None, scene, goal)
        Fn, G = len(fcell), spec.cells
        i32 = C.POINTER(C.c_int32)
        sp = PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n, P, G, K, S, Fn
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), float(spec.inflate_for(walls))
        sp.reuse_id = 0
        tm = PlanTime()
        tm.step0, tm.layer_steps, tm.layers = step0, layer_steps, T
        wl = None
        if walls is not None:
            wl = WallsC()
            wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
            wl.boxes, wl.n_walls = _fp(walls.table), walls.counts.ctypes.data_as(i32)
            wl.scene = None if walls.scene is None else walls.scene.ctypes.data_as(i32)
            wl.radius, wl.cost, wl.indicator = walls.radius, walls.cost, int(walls.indicator)
        h, _keep = self._hazards_struct(hazards, n)
        if smooth is not None:
            R.plan_time_smooth_check(Fn, S, T, G, smooth)
        big = Fn * (T + 1) * G * G * 4 > R.PLAN_TIME_MAX_BYTES            # refused by name below; nothing that large is allocated here
        wp = np.zeros((n, K, P), F32)
        waits, leave = np.zeros((n, K), np.int32), np.zeros((n, K), np.int32)
        nwp, count, status, cost, arrive = (np.zeros(n, np.int32) for _ in range(5))
        occ = np.zeros((S, T + 1, G, G), np.uint8) if want_occupancy and not big else None
        fields = np.zeros((Fn, T + 1, G, G), np.int32) if want_fields and not big else None
        sweeps = np.zeros(Fn, np.int32)
        head = (self._h, C.byref(sp), None if wl is None else C.byref(wl), C.byref(h), C.byref(tm))
        robots = (_fp(start), _fp(goal), field_of.ctypes.data_as(i32), fcell.ctypes.data_as(i32), fscene.ctypes.data_as(i32), _fp(wp),
                  nwp.ctypes.data_as(i32), count.ctypes.data_as(i32), status.ctypes.data_as(i32), cost.ctypes.data_as(i32),
                  waits.ctypes.data_as(i32), leave.ctypes.data_as(i32), arrive.ctypes.data_as(i32))
        copies = (None if occ is None else occ.ctypes.data_as(C.POINTER(C.c_uint8)), None if fields is None else fields.ctypes.data_as(i32),
                  sweeps.ctypes.data_as(i32))
        if smooth is None:
            check(self.lib.mobrob_ppo_plan_grid_time(*head, *robots, *copies))
            release = R.grid_release(waits, leave, step0, layer_steps)
        else:
            moves = np.zeros(n, np.int32)
            nb = np.zeros((S, T + 1, G, G), np.int16) if want_next_blocked else None
            check(self.lib.mobrob_ppo_plan_grid_time_smooth(*head, int(smooth), *robots, moves.ctypes.data_as(i32), *copies,
                                                            None if nb is None else nb.ctypes.data_as(C.POINTER(C.c_int16))))
            release = R.grid_release_smooth(leave, step0, layer_steps)
        out = {"waypoints": wp, "n_waypoints": nwp, "count": count, "status": status, "cost": cost, "waits": waits, "leave": leave,
               "arrive": arrive, "release": release, "field_of": field_of,
               "field_goal_cell": fcell, "field_scene": fscene, "sweeps": sweeps, "n_scenes": int(S)}
        if smooth is not None:
            out["moves"] = moves
            if nb is not None:
                out["next_blocked"] = nb
        if occ is not None:
            out["occupancy"] = occ.astype(bool)
        if fields is not None:
            out["fields"] = fields
        return out

    def plan_smooth_time(self, spec, walls=None, hazards=None, *, start, goal, step0=0, layer_steps, layers=64, max_waypoints=16, margin=1,
                         want_occupancy=False, want_fields=False, want_next_blocked=False):
        """plan_grid_time with line-of-sight smoothing over time (mobrob_ppo_plan_grid_time_smooth; the rule:
        goal_rules.grid_plan_time(smooth=True), reproduced bit for bit): a straight leg is kept only where it is clear, at
        `margin` (0 or 1) cells, in every layer it spans.  Returns plan_grid_time's dict with the smoothed waypoints,
        n_waypoints, count and status; leave [n][K]: the action index of each waypoint's anchor; release [n][K]
        (goal_rules.grid_release_smooth: a hold at every anchor but the start); waits all zero; moves [n] int32, the moves of
        each walk; and on request next_blocked int16 [S][T + 1][G][G] (goal_rules.grid_next_blocked)."""
        if isinstance(margin, bool) or margin not in (0, 1):
            raise ValueError(f"line-of-sight margin must be 0 or 1, got {margin!r}")
        return self._plan_time(spec, walls, hazards, start, goal, step0, layer_steps, layers, max_waypoints, want_occupancy, want_fields,
                               smooth=int(margin), want_next_blocked=want_next_blocked)

    def plan_grid_team(self, spec, walls=None, hazards=None, *, teams, reserve, start, goal, step0=0, layer_steps, layers, max_waypoints=16,
                       want_occupancy=False, want_fields=False, want_walks=False, clearance=True):
        """Waypoints and release steps for robots in teams, planned around each other (mobrob_ppo_plan_grid_team; the rule:
        goal_rules.grid_plan_team, reproduced bit for bit): inside a team the members plan in index order and every member's walk is
        reserved, `reserve` cells wide, in the layers of the members after it.  hazards: None, a goal_rules.Hazards (a static scene
        is handed down as one frame) or a MovingHazards; teams: a goal_rules.Teams (its size is used).  Returns plan_grid_time's
        dict per robot (field_of is the identity, sweeps [n]; nothing stays resident) plus team_clearance and team_crossings
        [n_teams] int32 (goal_rules.grid_team_clearance_cells of the walks the device reports, all pairs and teams at once;
        clearance=False leaves both out, and the call is then the device call alone), workgroups (the workgroups k_plan_team was
        launched with), and on request walks (per robot the cells of its walk, as lists), occupancy bool [S][T + 1][G][G] (the base
        layers) and fields int32 [n][T + 1][G][G].  The walks come back in T + 1 + 2 G cells a robot; only where a walk is longer
        (a maze) is the call made a second time with room for the longest."""
        return self._plan_team(spec, walls, hazards, teams, reserve, start, goal, step0, layer_steps, layers, max_waypoints, want_occupancy,
                               want_fields, want_walks, clearance)

    def plan_grid_team_rounds(self, spec, walls=None, hazards=None, *, teams, reserve, retries, start, goal, step0=0, layer_steps, layers,
                              max_waypoints=16, want_occupancy=False, want_fields=False, want_walks=False, clearance=True, smooth=False):
        """plan_grid_team with up to `retries` (0 .. 8) reordering rounds inside the device call (mobrob_ppo_plan_grid_team_rounds:
        k_plan_team_rounds; the rule: goal_rules.grid_plan_team_rounds, reproduced bit for bit): a team whose plan leaves members
        parked (UNREACHABLE or UNCONVERGED) is planned again with those members first, and the result is the round with the fewest
        parked members.  Returns plan_grid_team's dict of that round, indexed by robot, plus team_order int32 [n_teams][size] (the
        result's order), team_rounds [n_teams] (rounds planned, >= 1), team_parked and team_parked_first [n_teams] (parked members
        of the result and of round 0).  What rounds do not repair: goal_rules.grid_plan_team_rounds.  smooth=True is
        refused by name: rounds of smoothed team plans are not built."""
        from .envs import goal_rules as R
        retries = R.plan_retries_check(retries)
        if smooth:
            raise ValueError("plan_team: retries with smooth=True is not supported (reordering rounds plan unsmoothed team plans only)")
        return self._plan_team(spec, walls, hazards, teams, reserve, start, goal, step0, layer_steps, layers, max_waypoints, want_occupancy,
                               want_fields, want_walks, clearance, retries=retries)

    def plan_smooth_team(self, spec, walls=None, hazards=None, *, teams, reserve, start, goal, step0=0, layer_steps, layers, max_waypoints=16,
                         margin=1, max_leg=8, want_occupancy=False, want_fields=False, want_walks=False, clearance=True):
        """plan_grid_team with line-of-sight smoothing (mobrob_ppo_plan_grid_team_smooth; the rule:
        goal_rules.grid_plan_team(smooth=True), reproduced bit for bit): a leg is kept where it is clear at `margin` (0 or 1) cells in
        every layer it spans on the member's own map and at most `max_leg` actions long (None: no cap), and it is reserved for the
        later members as a swept region -- all of its cells in every layer of its span.  Returns plan_grid_team's dict with the
        smoothed waypoints, n_waypoints, count and status; leave, release and waits as plan_smooth_time's; moves [n] int32; keeps
        (per robot the kept indices in full; a call is repeated with more room where a robot keeps more than T + 1 + 2 G);
        team_clearance is goal_rules.grid_team_clearance_legs's (the guarantee: > reserve), team_crossings the walks' count."""
        from .envs import goal_rules as R
        if isinstance(margin, bool) or margin not in (0, 1):
            raise ValueError(f"line-of-sight margin must be 0 or 1, got {margin!r}")
        cap = 2 ** 31 - 1 if max_leg is None else R.plan_max_leg_check(max_leg)
        return self._plan_team(spec, walls, hazards, teams, reserve, start, goal, step0, layer_steps, layers, max_waypoints, want_occupancy,
                               want_fields, want_walks, clearance, smooth=(int(margin), cap))

    def _plan_team(self, spec, walls, hazards, teams, reserve, start, goal, step0, layer_steps, layers, max_waypoints, want_occupancy,
                   want_fields, want_walks, clearance, smooth=None, retries=None):
        """plan_grid_team's call (smooth and retries None), plan_smooth_team's (smooth: (margin, max_leg)) or plan_grid_team_rounds's
        (retries: an int): the checks and the arrays of all three"""
        from ._lib import PlanSpec, PlanTime, WallsC
        from .envs import goal_rules as R
        if not isinstance(spec, R.GridSpec):
            raise TypeError(f"spec must be a mobrob_amd.envs.goal_rules.GridSpec, not {type(spec).__name__}")
        start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
        if goal.ndim != 2 or goal.shape[0] < 1 or goal.shape[1] not in (2, 3) or start.shape != goal.shape:
            raise ValueError(f"plan_team: start and goal must both be [n_robots, 2 or 3], got shapes {start.shape} and {goal.shape}")
        if not (np.all(np.isfinite(start)) and np.all(np.isfinite(goal))):
            raise ValueError("plan_team: start and goal must be finite")
        n, P = goal.shape
        K = int(max_waypoints)
        if K < 1:
            raise ValueError("plan_team: max_waypoints must be >= 1")
        moving = isinstance(hazards, R.MovingHazards)
        S, scene = R.plan_scene_time(walls, hazards) if moving else R.plan_scene(walls, hazards)
        step0, layer_steps, T = R.plan_time_check(step0, layer_steps, layers)
        for sc in (walls, hazards):
            if sc is not None:
                sc.check_robots(n)
        size, r = R.plan_team_check(teams, reserve, n, scene)
        if hazards is not None and not moving:                             # a static scene: its own single frame
            hazards = R.MovingHazards(hazards.table[:, None, :, :2].astype(np.float64), size=hazards.table[:, :, 2].astype(np.float64),
                                      cost=hazards.cost, indicator=hazards.indicator, counts=hazards.counts, scene=hazards.scene)
        start, goal = np.ascontiguousarray(start, F32), np.ascontiguousarray(goal, F32)
        G = spec.cells
        i32 = C.POINTER(C.c_int32)
        sp = PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n, P, G, K, S, n
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), float(spec.inflate_for(walls))
        sp.reuse_id = 0
        tm = PlanTime()
        tm.step0, tm.layer_steps, tm.layers = step0, layer_steps, T
        wl = None
        if walls is not None:
            wl = WallsC()
            wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
            wl.boxes, wl.n_walls = _fp(walls.table), walls.counts.ctypes.data_as(i32)
            wl.scene = None if walls.scene is None else walls.scene.ctypes.data_as(i32)
            wl.radius, wl.cost, wl.indicator = walls.radius, walls.cost, int(walls.indicator)
        h, _keep = self._hazards_struct(hazards, n) if hazards is not None else (None, None)
        one = (T + 1) * G * G * 4
        big = one > R.PLAN_TIME_MAX_BYTES or n * one > R.PLAN_TIME_MAX_BYTES     # refused by name below; nothing that large is allocated here
        fields = np.zeros((n, T + 1, G, G) if not big else (1,), np.int32) if want_fields else None
        occ = np.zeros((S, T + 1, G, G), np.uint8) if want_occupancy else None
        walk_cap = keep_cap = T + 1 + 2 * G
        if smooth is not None and R.plan_team_smooth_bytes(G, T) > R.PLAN_TIME_MAX_BYTES:
            raise ValueError(f"plan_team: one team's field, next-blocked table and reservation of {T + 1} x {G} x {G} x 7 bytes exceed the cap "
                             f"of {R.PLAN_TIME_MAX_BYTES} bytes ({R.PLAN_TIME_MAX_BYTES >> 20} MiB)")
        u16 = C.POINTER(C.c_uint16)
        while True:                                                        # a second call only where a walk is longer than walk_cap
            wp = np.zeros((n, K, P), F32)
            waits, leave = np.zeros((n, K), np.int32), np.zeros((n, K), np.int32)
            nwp, count, status, cost, arrive, sweeps, moves = (np.zeros(n, np.int32) for _ in range(7))
            walk = np.zeros((n, walk_cap), np.uint16)
            wgs = C.c_int32(0)
            head = (self._h, C.byref(sp), None if wl is None else C.byref(wl), None if h is None else C.byref(h), C.byref(tm), size, r)
            robots = (_fp(start), _fp(goal), _fp(wp), nwp.ctypes.data_as(i32), count.ctypes.data_as(i32), status.ctypes.data_as(i32),
                      cost.ctypes.data_as(i32), waits.ctypes.data_as(i32), leave.ctypes.data_as(i32), arrive.ctypes.data_as(i32))
            copies = (None if occ is None else occ.ctypes.data_as(C.POINTER(C.c_uint8)), None if fields is None else fields.ctypes.data_as(i32),
                      C.byref(wgs))
            if retries is not None:
                order = np.zeros((n // size, size), np.int32)
                rounds, parked, parked_first = (np.zeros(n // size, np.int32) for _ in range(3))
                check(self.lib.mobrob_ppo_plan_grid_team_rounds(*head, retries, *robots, sweeps.ctypes.data_as(i32), walk.ctypes.data_as(u16),
                                                                walk_cap, *copies, order.ctypes.data_as(i32), rounds.ctypes.data_as(i32),
                                                                parked.ctypes.data_as(i32), parked_first.ctypes.data_as(i32)))
                if int(arrive.max()) + 1 <= walk_cap:
                    break
            elif smooth is None:
                check(self.lib.mobrob_ppo_plan_grid_team(*head, *robots, sweeps.ctypes.data_as(i32), walk.ctypes.data_as(u16), walk_cap, *copies))
                if int(arrive.max()) + 1 <= walk_cap:
                    break
            else:
                keep = np.zeros((n, keep_cap), np.int32)
                check(self.lib.mobrob_ppo_plan_grid_team_smooth(*head, smooth[0], smooth[1], *robots, moves.ctypes.data_as(i32),
                                                                sweeps.ctypes.data_as(i32), walk.ctypes.data_as(u16), walk_cap,
                                                                keep.ctypes.data_as(i32), keep_cap, *copies))
                if int(arrive.max()) + 1 <= walk_cap and int(count.max()) - 1 <= keep_cap:
                    break
                keep_cap = max(keep_cap, int(count.max()) - 1)
            walk_cap = max(walk_cap, int(arrive.max()) + 1)
        cells = np.stack([walk & 127, walk >> 7], axis=-1)
        out = {"waypoints": wp, "n_waypoints": nwp, "count": count, "status": status, "cost": cost, "waits": waits, "leave": leave,
               "arrive": arrive, "release": R.grid_release(waits, leave, step0, layer_steps), "field_of": np.arange(n, dtype=np.int32),
               "field_goal_cell": (lambda gx, gy: (gy * G + gx).astype(np.int32))(*spec.cell_of(goal[:, :2])),
               "field_scene": np.zeros(n, np.int32) if scene is None else np.asarray(scene, np.int32).copy(), "sweeps": sweeps,
               "n_scenes": int(S), "workgroups": int(wgs.value)}
        walks = [[(int(x), int(y)) for x, y in cells[i, :int(arrive[i]) + 1]] for i in range(n)] if want_walks or (smooth is not None and clearance) else None
        if retries is not None:
            out.update(team_order=order, team_rounds=rounds, team_parked=parked, team_parked_first=parked_first)
        if smooth is not None:
            out["release"], out["moves"] = R.grid_release_smooth(leave, step0, layer_steps), moves
            out["keeps"] = [keep[i, :max(int(count[i]) - 1, 0)].tolist() for i in range(n)]
        if clearance:
            out["team_clearance"], out["team_crossings"] = R.grid_team_clearance_cells(cells, arrive.astype(np.int64) + 1, size, T)
            if smooth is not None:
                out["team_clearance"] = R.grid_team_clearance_legs(walks, R.plan_team_keeps_with_walks(out["keeps"], status), size, T)
        if want_walks:
            out["walks"] = walks
        if occ is not None:
            out["occupancy"] = occ.astype(bool)
        if fields is not None:
            out["fields"] = fields
        return out

    def plan_assign(self, spec, walls=None, hazards=None, *, teams, start, goal, objective="sum", step0=0, layer_steps=None, layers=None,
                    want_matrix=False):
        """Who takes which goal inside every team: a minimum-cost perfect matching per team on the device (mobrob_ppo_plan_assign:
        the base map, k_plan_assign_cost, k_plan_assign; the rule: goal_rules.grid_assign, reproduced bit for bit, the potentials
        included).  The costs are each robot's own static cost-to-go on the scene's map (with a goal_rules.MovingHazards the
        conservative tail of its layers: layer_steps and layers are required then, and only then); objective "sum" or "makespan".
        Returns grid_assign's dict: assign [n] (whose input goal robot i is given), goal [n][P] = goal[assign], assign_cost [n],
        assign_total, assign_max, assign_identity_total, assign_identity_max, assign_changed, assign_status [n_teams] (UNCONVERGED:
        a field hit its sweep bound; that team keeps the identity), assign_potentials (u, v), sweeps [n], and with want_matrix
        assign_matrix int32 [n_teams][size][size].  Nothing stays resident and nothing of a plan or of training is touched."""
        from ._lib import PlanSpec, PlanTime, WallsC
        from .envs import goal_rules as R
        start, goal, size, obj, step0, layer_steps, T = R.plan_assign_check(spec, walls, hazards, start, goal, teams, objective, step0,
                                                                           layer_steps, layers)
        moving = isinstance(hazards, R.MovingHazards)
        S, _ = R.plan_scene_time(walls, hazards) if moving else R.plan_scene(walls, hazards)
        start, goal = np.ascontiguousarray(start, F32), np.ascontiguousarray(goal, F32)
        n, P = goal.shape
        g = n // size
        i32 = C.POINTER(C.c_int32)
        i64 = C.POINTER(C.c_int64)
        sp = PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n, P, spec.cells, 1, S, n
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(spec.extent), float(spec.h), float(spec.inv_h), float(spec.inflate_for(walls))
        sp.reuse_id = 0
        tm = None
        if moving:
            tm = PlanTime()
            tm.step0, tm.layer_steps, tm.layers = step0, layer_steps, T
        wl = None
        if walls is not None:
            wl = WallsC()
            wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
            wl.boxes, wl.n_walls = _fp(walls.table), walls.counts.ctypes.data_as(i32)
            wl.scene = None if walls.scene is None else walls.scene.ctypes.data_as(i32)
            wl.radius, wl.cost, wl.indicator = walls.radius, walls.cost, int(walls.indicator)
        h, _keep = self._hazards_struct(hazards, n) if hazards is not None else (None, None)
        assign, cost, sweeps = (np.zeros(n, np.int32) for _ in range(3))
        goal_out = np.zeros((n, P), F32)
        total, team = np.zeros((2, g), np.int64), np.zeros((4, g), np.int32)
        u, v = np.zeros((g, size), np.int64), np.zeros((g, size), np.int64)
        matrix = np.zeros((g, size, size), np.int32) if want_matrix else None
        check(self.lib.mobrob_ppo_plan_assign(
            self._h, C.byref(sp), None if wl is None else C.byref(wl), None if h is None or moving else C.byref(h),
            C.byref(h) if moving else None, None if tm is None else C.byref(tm), size, obj, _fp(start), _fp(goal), assign.ctypes.data_as(i32),
            _fp(goal_out), cost.ctypes.data_as(i32), total.ctypes.data_as(i64), team.ctypes.data_as(i32), u.ctypes.data_as(i64),
            v.ctypes.data_as(i64), None if matrix is None else matrix.ctypes.data_as(i32), sweeps.ctypes.data_as(i32)))
        out = {"assign": assign, "goal": goal_out, "assign_cost": cost, "assign_total": total[0].copy(), "assign_max": team[0].copy(),
               "assign_identity_total": total[1].copy(), "assign_identity_max": team[1].copy(), "assign_changed": team[2] != 0,
               "assign_status": team[3].copy(), "assign_potentials": (u, v), "sweeps": sweeps}
        if matrix is not None:
            out["assign_matrix"] = matrix
        return out

    def plan_spec(self, grid, walls=None, hazards=None, *, spec, start, goal=None, pace=None, max_waypoints=16, want_occupancy=False,
                  state=None, step0=0, partial=False, share=None, objective="makespan"):
        """A plan from a specification on the device (mobrob_ppo_spec_plan; the rule: goal_rules.spec_plan, reproduced bit for bit):
        the avoid clauses of `spec` become obstacles, its reach clauses stations, and per robot the order of the stations and the
        stitched waypoints are computed in one call.  grid: a goal_rules.GridSpec; walls / hazards: static, or None; spec: a
        goal_rules.Spec of the plannable fragment (spec_plan_parse); start [n][P]; goal [n][P] or None; pace: spec_plan_pace's.
        Returns spec_plan's dict (occupancy only with want_occupancy) and `sweeps`, the relaxation sweeps of each field.  Nothing
        stays resident and plan_grid's resident fields stay valid.
        state (a goal_rules.SpecState), step0, partial: the plan from the middle of a run, spec_plan's keywords.  With all three at
        their defaults the call is mobrob_ppo_spec_plan; otherwise mobrob_ppo_spec_replan (k_plan_tour_resume,
        k_plan_tour_path_legs), with todo made here from the state.  Either way the dict holds SPEC_REPLAN_KEYS and t0.
        share (a team size), objective ("makespan" / "sum"): the team's stations are shared among its members, spec_plan's
        keywords; the call is then mobrob_ppo_spec_plan_share (k_plan_tour_best, k_plan_team_share, k_plan_team_void) and the dict
        also holds SPEC_SHARE_KEYS.  share=None takes the path it took."""
        from ._lib import PlanSpec, SpecC, WallsC
        from .envs import goal_rules as R
        raw_pace = pace
        avoid, stations, (open_c, close_c, dwell_c), S, scene, start, goal, K, pace = R.spec_plan_check(grid, walls, hazards, spec, start,
                                                                                                     goal, max_waypoints, pace)
        done, todo, t0 = R.spec_plan_resume_check(spec, start.shape[0], None if raw_pace is None else pace, state, step0, partial)
        resume = state is not None or step0 != 0 or bool(partial)
        if share is not None:
            share, objective = R.spec_plan_share_check(start.shape[0], share, objective)
        reg = spec.regions
        n, P = start.shape
        G, M = grid.cells, len(stations)
        start = np.ascontiguousarray(start, F32)
        i32 = C.POINTER(C.c_int32)
        ip = lambda a: a.ctypes.data_as(i32)   # noqa: E731
        if goal is not None:
            goal = np.ascontiguousarray(goal, F32)
            field_of, fcell, fscene = R.plan_fields(grid, None, scene, goal)
        Fg = 0 if goal is None else len(fcell)
        sp = PlanSpec()
        sp.n_robots, sp.pos_dim, sp.cells, sp.max_waypoints, sp.n_scenes, sp.n_fields = n, P, G, K, S, Fg
        sp.extent, sp.h, sp.inv_h, sp.inflate = float(grid.extent), float(grid.h), float(grid.inv_h), float(grid.inflate_for(walls))
        sp.reuse_id = 0
        wl = None
        if walls is not None:
            wl = WallsC()
            wl.n_scenes, wl.max_walls = walls.n_scenes, walls.max_walls
            wl.boxes, wl.n_walls = _fp(walls.table), ip(walls.counts)
            wl.scene = None if walls.scene is None else ip(walls.scene)
            wl.radius, wl.cost, wl.indicator = walls.radius, walls.cost, int(walls.indicator)
        h, _keep = (None, None) if hazards is None else self._hazards_struct(hazards, n)
        rg = SpecC()
        rg.n_scenes, rg.max_regions, rg.n_clauses = reg.n_scenes, reg.max_regions, 0
        rg.regions, rg.kinds, rg.n_regions = _fp(reg.table), ip(reg.kinds), ip(reg.counts)
        rg.scene = None if reg.scene is None else ip(reg.scene)
        st_lo, st_hi = (np.array([s[k] for s in stations], np.int32) for k in (0, 1))
        av_lo, av_hi = (np.array([a[k] for a in avoid], np.int32) for k in (0, 1))
        wp = np.zeros((n, K, P), F32)
        nwp, count, status, cost = (np.zeros(n, np.int32) for _ in range(4))
        order, eta, swp = (np.zeros((n, M), np.int32) for _ in range(3))
        release = np.zeros((n, K), np.int32)
        cell, margin, matrix = np.zeros((S, M), np.int32), np.zeros((S, M), F32), np.zeros((S, M, M), np.int32)
        occ = np.zeros((S, G, G), np.uint8) if want_occupancy else None
        sweeps = np.zeros(S * M + Fg, np.int32)
        ins = (self._h, C.byref(sp), None if wl is None else C.byref(wl), None if h is None else C.byref(h), C.byref(rg), M, ip(st_lo),
               ip(st_hi), len(avoid), ip(av_lo) if avoid else None, ip(av_hi) if avoid else None, ip(open_c), ip(close_c), ip(dwell_c), pace,
               _fp(start), None if goal is None else _fp(goal), None if goal is None else ip(field_of), None if goal is None else ip(fcell),
               None if goal is None else ip(fscene))
        outs = (_fp(wp), ip(nwp), ip(count), ip(status), ip(cost), ip(order), ip(eta), ip(swp), ip(release), ip(cell), _fp(margin),
                ip(matrix), None if occ is None else occ.ctypes.data_as(C.POINTER(C.c_uint8)), ip(sweeps))
        shared = {}
        if share is not None:
            todo = np.ascontiguousarray(todo, np.int32)
            tour_len, dropped, mine = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
            cover, lost, makespan = (np.zeros(n // share, np.int32) for _ in range(3))
            total = np.zeros(n // share, np.int64)
            check(self.lib.mobrob_ppo_spec_plan_share(*ins, ip(todo), t0, int(bool(partial)), share, R.SPEC_SHARE_OBJECTIVES.index(objective),
                                                      *outs, ip(tour_len), ip(dropped), ip(mine), ip(cover), ip(lost), ip(makespan),
                                                      total.ctypes.data_as(C.POINTER(C.c_int64))))
            shared = {"share": mine, "team_cover": cover, "team_dropped": lost, "team_makespan": makespan, "team_total": total,
                      "team_done": done.reshape(n // share, share, M).any(axis=1), "team_feasible": makespan >= 0}
        elif resume:
            todo = np.ascontiguousarray(todo, np.int32)
            tour_len, dropped = np.zeros(n, np.int32), np.zeros(n, np.int32)
            check(self.lib.mobrob_ppo_spec_replan(*ins, ip(todo), t0, int(bool(partial)), *outs, ip(tour_len), ip(dropped)))
        else:
            check(self.lib.mobrob_ppo_spec_plan(*ins, *outs))
            tour_len, dropped = np.where(order[:, 0] >= 0, M, 0).astype(np.int32), np.where(order[:, 0] >= 0, 0, todo).astype(np.int32)
        out = {"waypoints": wp, "n_waypoints": nwp, "count": count, "status": status, "cost": cost, "tour_order": order, "tour_eta": eta,
               "station_waypoint": swp, "release": release, "station_cell": cell, "station_margin": margin,
               "covered": margin >= np.float32(R.REACH_RADIUS), "matrix": matrix, "open_c": open_c, "close_c": close_c, "dwell_c": dwell_c,
               "pace": pace, "sweeps": sweeps, "tour_len": tour_len, "dropped": dropped, "done": done, "t0": t0, **shared}
        if occ is not None:
            out["occupancy"] = occ.astype(bool)
        return out

    def episode_stats(self, reset=True):
        """Episodes finished by the goal environment since the counters were last reset."""
        st = EpisodeStats()
        check(self.lib.mobrob_ppo_episode_stats(self._h, C.byref(st), int(bool(reset))))
        n = int(st.episodes)
        return {"episodes": n, "goals": int(st.goals), "ep_rew_mean": st.return_sum / n if n else float("nan"),
                "ep_len_mean": st.length_sum / n if n else float("nan")}

    def episode_records(self, max_records=100):
        """Monitor records [{r, l}] of the episodes the device goal environment finished since the last call
        (oldest first, the newest `max_records` at most)."""
        out = np.zeros((int(max_records), 2), F32)
        n = check(self.lib.mobrob_ppo_episode_records(self._h, _fp(out), int(max_records)))
        return [{"r": float(r), "l": int(l)} for r, l in out[:n]]

    # ---- env-side controllers (batched on the device, csrc/robot_ctrl.h) ---------------------------
    def ctrl_turtlebot3(self, pos, theta, goal, gain_changes):
        """Turtlebot3's proportional controller for n robots: -> twist [n, 2] = (v, w)."""
        pos, goal, gc = _f32c(pos), _f32c(goal), _f32c(gain_changes)
        theta = _f32c(theta)
        n = theta.shape[0]
        if pos.shape != (n, 2) or goal.shape != (n, 2) or gc.shape != (n, 2):
            raise ValueError("pos, goal, gain_changes must be [n, 2] and theta [n]")
        twist = np.empty((n, 2), F32)
        check(self.lib.mobrob_ctrl_turtlebot3(self._h, n, 0, _fp(pos), _fp(theta), _fp(goal), _fp(gc), _fp(twist)))
        return twist

    def ctrl_drone_pid(self, pos, rpy, goal, action, ctrl_state, mass, max_thrust, max_xy_torque, max_z_torque, g=9.8,
                       dt=1.0 / 50.0, max_roll_pitch=np.pi / 6, tune_fac=0.3):
        """The drone's cascaded PID for n robots; `ctrl_state` [n, 12] is updated in place -> [n, 4] thrust, torques."""
        pos, rpy, goal, action = _f32c(pos), _f32c(rpy), _f32c(goal), _f32c(action)
        n = pos.shape[0]
        if pos.shape != (n, 3) or rpy.shape != (n, 3) or goal.shape != (n, 3) or action.shape != (n, 18):
            raise ValueError("pos, rpy, goal must be [n, 3] and action [n, 18]")
        if ctrl_state.shape != (n, 12) or ctrl_state.dtype != F32 or not ctrl_state.flags.c_contiguous:
            raise ValueError("ctrl_state must be a C-contiguous float32 [n, 12] array")
        prm = DroneParams(mass, g, dt, max_thrust, max_xy_torque, max_z_torque, max_roll_pitch, tune_fac)
        out = np.empty((n, 4), F32)
        check(self.lib.mobrob_ctrl_drone_pid(self._h, n, 0, C.byref(prm), _fp(pos), _fp(rpy), _fp(goal), _fp(action),
                                             _fp(ctrl_state), _fp(out)))
        return out

    def compute_gae(self):
        check(self.lib.mobrob_ppo_compute_gae(self._h))

    def x3_mode(self):
        """Bit 0: rollout / value forward on the bf16 pipe with split float32 operands; bit 1: the gradient kernel's forward too."""
        return int(self.lib.mobrob_ppo_x3_mode(self._h))

    def update_mode(self):
        """Bit 0: the latest train() ran every epoch as one co-operative launch (k_epoch64) instead of three launches per step."""
        return int(self.lib.mobrob_ppo_update_mode(self._h))

    def set_eval_tile256(self, on):
        """Switch the one-launch evaluation / following kernel of fused 2x256 tanh engines (k_goal256_tile) on or off for this
        engine: evaluate_goal_env and follow_waypoints calls without hazards, teams or walls then report `persistent` True.  Off
        unless told (or MOBROB_EVAL_TILE256=1 for engines never told).  ValueError naming tile256 on any other engine."""
        if not isinstance(on, (bool, np.bool_)):
            raise TypeError(f"eval_tile256 must be a bool, got {type(on).__name__}")
        check(self.lib.mobrob_ppo_set_eval_tile256(self._h, int(bool(on))))
        self._eval_tile256 = bool(on)

    @property
    def eval_tile256(self):
        """What set_eval_tile256 was told last (False: never told)."""
        return bool(getattr(self, "_eval_tile256", False))

    def set_eval_tile256_wide(self, on):
        """The same kernel for calls WITH static or moving hazards: a switch of its own, off unless told (or
        MOBROB_EVAL_TILE256_WIDE=1 for engines never told).  Such a call reports `persistent` True only when tile256 is in force as
        well (set_eval_tile256); calls with walls or teams, resumed runs with static hazards and scheduled runs with moving hazards
        are not served and run the per-step path as before.  ValueError naming tile256 on an engine that is not fused 2x256 tanh."""
        if not isinstance(on, (bool, np.bool_)):
            raise TypeError(f"eval_tile256_wide must be a bool, got {type(on).__name__}")
        check(self.lib.mobrob_ppo_set_eval_tile256_wide(self._h, int(bool(on))))
        self._eval_tile256_wide = bool(on)

    @property
    def eval_tile256_wide(self):
        """What set_eval_tile256_wide was told last (False: never told)."""
        return bool(getattr(self, "_eval_tile256_wide", False))

    def explained_variance(self):
        """1 - Var[returns - values] / Var[returns] over the rollout in the buffer (SB3's train/explained_variance)."""
        out = C.c_double()
        check(self.lib.mobrob_ppo_explained_variance(self._h, C.byref(out)))
        return float(out.value)

    def mark_rollout_ready(self):
        check(self.lib.mobrob_ppo_mark_rollout_ready(self._h))

    # ---- update -------------------------------------------------------------------------------
    def train(self, perms=None):
        """Whole PPO.train().  perms: [n_epochs, T*N] int64 env-major permutations or None."""
        p = None
        if perms is not None:
            perms = np.ascontiguousarray(perms, dtype=np.int64)
            if perms.shape != (self.cfg.n_epochs, self.N * self.T):
                raise ValueError(f"perms must be [{self.cfg.n_epochs}, {self.N * self.T}]")
            p = perms.ctypes.data_as(C.POINTER(C.c_int64))
        st = TrainStats()
        check(self.lib.mobrob_ppo_train(self._h, p, C.byref(st)))
        return {k: float(getattr(st, k)) for k in STAT_KEYS} | {"n_minibatches": int(st.n_minibatches)}

    def comm_prepare(self):
        """Local, non-collective half of comm_init (RCCL loadable, device selectable, no communicator yet): ranks agree
        on its outcome before any of them enters the blocking collective."""
        check(self.lib.mobrob_ppo_comm_prepare(self._h))

    def comm_init(self, unique_id=None, rank=None, nranks=None):
        """Collective over the ranks of the job: build the engine's RCCL communicator.  Rank 0 calls
        `PPOEngine.comm_unique_id()` and ships the 128 bytes to the others (parallel.py uses torch.distributed).
        rank / nranks: position in the process (sub)group the communicator spans (default: the engine's config)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        if rank is None and nranks is None:
            check(self.lib.mobrob_ppo_comm_init(self._h, buf))
        else:
            check(self.lib.mobrob_ppo_comm_init_rank(self._h, buf, int(rank), int(nranks)))

    def comm_info(self):
        """(ncclCommCount, ncclCommUserRank) of the engine's communicator; (0, -1) without one."""
        n, r = C.c_int32(), C.c_int32()
        check(self.lib.mobrob_ppo_comm_info(self._h, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    def oneshot_export(self) -> bytes:
        """IPC handle of this rank's exchange buffer of the one-shot all-reduce (mobrob_ppo_oneshot_export)."""
        buf = (C.c_uint8 * 64)()
        check(self.lib.mobrob_ppo_oneshot_export(self._h, buf))
        return bytes(buf)

    def oneshot_open(self, handles, rank, nranks):
        """handles: the ranks' export handles in rank order; afterwards train_dp() exchanges through peer-mapped memory."""
        blob = b"".join(bytes(h) for h in handles)
        if len(blob) != 64 * int(nranks):
            raise ValueError(f"expected {nranks} handles of 64 bytes")
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        check(self.lib.mobrob_ppo_oneshot_open(self._h, buf, int(rank), int(nranks)))

    def oneshot_close(self):
        check(self.lib.mobrob_ppo_oneshot_close(self._h))

    def exchange_selfcheck(self, which):
        """A known vector through the engine's RCCL communicator (which = "rccl") or its one-shot exchange ("oneshot"), compared
        with the rank-ordered sum (collective).  -> number of message elements that are not bit-equal to it (0 = sound)."""
        bad = C.c_int32(-1)
        check(self.lib.mobrob_ppo_exchange_selfcheck(self._h, {"rccl": 0, "oneshot": 1}[which], C.byref(bad)))
        return int(bad.value)

    def allreduce_counters(self, reset=False):
        """(calls, payload bytes) of the all-reduces train_dp issued since the last reset."""
        c, b = C.c_int64(), C.c_int64()
        check(self.lib.mobrob_ppo_allreduce_counters(self._h, C.byref(c), C.byref(b), int(bool(reset))))
        return int(c.value), int(b.value)

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        check(_lib.load().mobrob_ppo_comm_unique_id(buf))
        return bytes(buf)

    def train_dp(self, perms=None, allreduce=None):
        """PPO.train() across the ranks, the whole loop in C (mobrob_ppo_train_dp): one all-reduce of the gradient per
        optimizer step on the engine's stream.  allreduce: None -> RCCL on the communicator of comm_init; or a Python
        callable (device_ptr, count, dtype_code, hip_stream) -> None that sums in place (tests)."""
        p = None
        if perms is not None:
            perms = np.ascontiguousarray(perms, dtype=np.int64)
            if perms.shape != (self.cfg.n_epochs, self.N * self.T):
                raise ValueError(f"perms must be [{self.cfg.n_epochs}, {self.N * self.T}]")
            p = perms.ctypes.data_as(C.POINTER(C.c_int64))
        if allreduce is None:
            check(self.lib.mobrob_ppo_train_dp(self._h, p, None, None))
            return
        failure = []

        def trampoline(_ctx, buf, count, dtype, stream):
            try:
                allreduce(int(buf), int(count), int(dtype), int(stream or 0))
                return 0
            except BaseException as ex:  # noqa: BLE001 - must not propagate through the C frame
                failure.append(ex)
                return 1

        cb = _lib.ALLREDUCE_FN(trampoline)
        rc = self.lib.mobrob_ppo_train_dp(self._h, p, C.cast(cb, C.c_void_p), None)
        if failure:
            raise failure[0]
        check(rc)

    def set_hyper(self, **values):
        """learning_rate / clip_range (schedule values for the coming train()), clip_range_vf (None = off), target_kl
        (None = off), ent_coef, vf_coef -> mobrob_ppo_set_hyper."""
        for name, v in values.items():
            if name not in _lib.HYPER:
                raise ValueError(f"unknown hyper-parameter {name!r} (known: {sorted(_lib.HYPER)})")
            check(self.lib.mobrob_ppo_set_hyper(self._h, _lib.HYPER[name], -1.0 if v is None else float(v)))

    def last_train_info(self):
        """(epochs started, stopped early by target_kl, optimizer steps applied) of the latest train()."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        check(self.lib.mobrob_ppo_last_train_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), bool(b.value), int(c.value)

    def train_enqueue(self):
        """PPO.train() enqueued on the engine's stream without waiting (device-drawn permutations)."""
        check(self.lib.mobrob_ppo_train_enqueue(self._h, None))

    def train_stats(self):
        """Means over the last epoch's minibatches of the most recent update (waits for the stream)."""
        rows = self.fetch_step_stats(self.n_minibatches)
        m = np.zeros(7)
        if len(rows):
            r = rows.astype(np.float64)
            m = r.mean(axis=0)
            ok = ~np.isnan(r[:, 6])  # a step dropped by target_kl has no gradient norm
            m[6] = r[ok, 6].mean() if ok.any() else 0.0
        return {k: float(m[i]) for i, k in enumerate(STAT_KEYS)}

    def epoch_begin(self, perm=None):
        p = None
        if perm is not None:
            perm = np.ascontiguousarray(perm, dtype=np.int64)
            if perm.shape != (self.N * self.T,):
                raise ValueError("perm must have T*N entries")
            p = perm.ctypes.data_as(C.POINTER(C.c_int64))
        check(self.lib.mobrob_ppo_epoch_begin(self._h, p))

    def minibatch_grad(self, mb):
        check(self.lib.mobrob_ppo_minibatch_grad(self._h, int(mb)))

    def minibatch_apply(self):
        check(self.lib.mobrob_ppo_minibatch_apply(self._h))

    def minibatch_apply_checked(self):
        """minibatch_apply behind SB3's target_kl check -> True when the step was DROPPED (the driver ends train())."""
        stopped = C.c_int32()
        check(self.lib.mobrob_ppo_minibatch_apply_checked(self._h, C.byref(stopped)))
        return bool(stopped.value)

    def fetch_step_stats(self, max_rows=None):
        max_rows = int(max_rows or (self.n_minibatches * self.cfg.n_epochs))
        out = np.zeros((max_rows, 8), F32)
        n = check(self.lib.mobrob_ppo_fetch_step_stats(self._h, _fp(out), max_rows))
        return out[:n, :7]

    # ---- inference ----------------------------------------------------------------------------
    def predict(self, obs, deterministic=True, eps=None, want_values=False):
        obs = np.asarray(obs)
        single = obs.ndim == 1
        x = _f32c(obs[None] if single else obs)
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError(f"Unexpected observation shape {obs.shape} for Box environment with shape ({self.D},)")
        n = x.shape[0]
        act = np.empty((n, self.A), F32)
        val = np.empty(n, F32) if want_values else None
        eps = None if eps is None else _f32c(eps, (n, self.A))
        check(self.lib.mobrob_ppo_predict(self._h, _fp(x), n, int(bool(deterministic)), _fp(eps), _fp(act), _fp(val)))
        act = act[0] if single else act
        return (act, val) if want_values else act

    # ---- buffers ------------------------------------------------------------------------------
    def _buf_shape(self, name):
        T, N = self.T, self.N
        return {"obs": ((T + 1, N, self.D), F32), "actions": ((T, N, self.A), F32), "rewards": ((T, N), F32),
                "episode_starts": ((T, N), F32), "values": ((T, N), F32), "log_probs": ((T, N), F32),
                "advantages": ((T, N), F32), "returns": ((T, N), F32), "params": ((self.P,), F32),
                "grads": ((self.P,), F32), "advstat": ((self.n_minibatches, 4), np.float64),
                "last_values": ((N,), F32), "last_dones": ((N,), F32), "clipped_actions": ((N, self.A), F32), "episode_start_state": ((N,), F32),
                "terminal_obs": ((N, 16 * ((self.D + 15) // 16) if self.D <= 64 else 8 * ((self.D + 7) // 8)), F32), "terminal_values": ((N,), F32),
                "truncated": ((N,), np.uint8), "env_state": ((N, 12), F32), "grad_exchange": ((self.P + 8,), F32),
                "sde_noise": ((N, getattr(self, "HL", 0), self.A), F32)}[name]

    def read(self, name):
        shape, dt = self._buf_shape(name)
        out = np.empty(shape, dt)
        check(self.lib.mobrob_ppo_read_buffer(self._h, BUF[name], out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def write(self, name, arr):
        shape, dt = self._buf_shape(name)
        a = np.ascontiguousarray(arr, dtype=dt)
        if a.shape != shape:
            raise ValueError(f"{name}: expected {shape}, got {a.shape}")
        check(self.lib.mobrob_ppo_write_buffer(self._h, BUF[name], a.ctypes.data_as(C.c_void_p), a.nbytes))

    def device_buffer(self, name):
        """(device pointer, bytes) -- e.g. to wrap grads/advstat for a collective."""
        p, b = C.c_void_p(), C.c_size_t()
        check(self.lib.mobrob_ppo_buffer_info(self._h, BUF[name], C.byref(p), C.byref(b)))
        return int(p.value), int(b.value)

    def load_rollout(self, buf, last_values, dones):
        """Inject a complete rollout (tests): dict of [T,N,..] arrays as in the oracle."""
        obs = np.zeros((self.T + 1, self.N, self.D), F32)
        obs[:self.T] = buf["obs"]
        self.write("obs", obs)
        for k in ("actions", "rewards", "episode_starts", "values", "log_probs"):
            self.write(k, buf[k])
        self.write("last_values", last_values)
        self.write("last_dones", np.asarray(dones, F32))
        if "advantages" in buf:
            self.write("advantages", buf["advantages"])
            self.write("returns", buf["returns"])
            self.mark_rollout_ready()

    def feistel_permutation(self, n, key):
        out = np.empty(int(n), np.int64)
        check(self.lib.mobrob_ppo_feistel_permutation(self._h, int(n), int(key) & (2 ** 64 - 1),
                                                      out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def pinned(self, shape, dtype=np.float32):
        """Zero-filled NumPy array backed by pinned, device-visible host memory (mobrob_ppo_host_alloc): the kernels
        read / write such buffers in place (no staging copy).  The allocation lives as long as any view of the
        array does (see _PinnedBlock), also past close()."""
        dtype = np.dtype(dtype)
        shape = tuple(int(s) for s in np.atleast_1d(shape)) if not isinstance(shape, tuple) else shape
        block = _PinnedBlock(self.lib, int(np.prod(shape)) * dtype.itemsize, shape, dtype)
        return np.asarray(block)

    def register_host(self, address, nbytes):
        """Pin + map caller-owned host memory in place (mobrob_ppo_host_register), e.g. the shared block of
        `ShmVecEnv`; unregistered by unregister_host() or close()."""
        check(self.lib.mobrob_ppo_host_register(C.c_void_p(int(address)), C.c_size_t(int(nbytes))))
        self._registered = getattr(self, "_registered", [])
        self._registered.append(int(address))

    def unregister_host(self, address):
        if int(address) in getattr(self, "_registered", []):
            self._registered.remove(int(address))
            check(self.lib.mobrob_ppo_host_unregister(C.c_void_p(int(address))))

    def set_stream(self, stream_handle):
        check(self.lib.mobrob_ppo_set_stream(self._h, C.c_void_p(stream_handle)))

    def synchronize(self):
        check(self.lib.mobrob_ppo_synchronize(self._h))

    def profile(self, on=True, only=None):
        """HIP-event bracketing of the engine's phases.  only: names from _lib.KERNEL_IDS to restrict it to (each
        bracketed launch costs a few microseconds of GPU time)."""
        v = int(bool(on))
        if on and only is not None:
            v = sum(1 << (_lib.KERNEL_IDS[k] + 1) for k in only)
        check(self.lib.mobrob_ppo_profile_enable(self._h, v))

    def profile_read(self):
        n = len(_lib.KERNEL_IDS)  # MOBROB_K_COUNT
        ms, calls = (C.c_double * n)(), (C.c_int64 * n)()
        check(self.lib.mobrob_ppo_profile_read(self._h, ms, calls))
        return {k: (float(ms[i]), int(calls[i])) for k, i in _lib.KERNEL_IDS.items()}
