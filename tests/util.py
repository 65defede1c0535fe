"""Shared helpers for the parity tests (fixtures -> oracle structures)."""
import os
from collections import OrderedDict

import numpy as np
import pytest

from oracle import ppo_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENVS = ["point", "car", "doggo", "drone", "turtlebot3"]


def load_golden(env):
    return np.load(os.path.join(GOLDEN, f"{env}.npz"))


def golden_params(g, prefix="p/"):
    keys = O.param_keys()
    return OrderedDict((k, g[prefix + k].astype(np.float32).copy()) for k in keys)


def golden_adam(g, m="m/", v="v/", step_key="adam_step"):
    keys = O.param_keys()
    return O.AdamState(OrderedDict((k, g[m + k].copy()) for k in keys),
                       OrderedDict((k, g[v + k].copy()) for k in keys), int(g[step_key]))


def golden_hyper(g):
    return O.Hyper(gamma=float(g["hyper/gamma"]), gae_lambda=float(g["hyper/gae_lambda"]),
                   clip_range=float(g["hyper/clip_range"]), ent_coef=float(g["hyper/ent_coef"]),
                   vf_coef=float(g["hyper/vf_coef"]), max_grad_norm=float(g["hyper/max_grad_norm"]),
                   learning_rate=float(g["hyper/learning_rate"]), beta1=float(g["hyper/beta1"]),
                   beta2=float(g["hyper/beta2"]), adam_eps=float(g["hyper/adam_eps"]),
                   n_epochs=int(g["hyper/n_epochs"]), batch_size=int(g["hyper/batch_size"]))


def golden_minibatch(g):
    return (g["mb/obs"], g["mb/actions"], g["mb/old_values"], g["mb/old_log_prob"], g["mb/advantages"],
            g["mb/returns"])


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / (1e-6 + np.maximum(np.abs(a), np.abs(b))))) if a.size else 0.0


def scaled_err(a, b):
    """max |a-b| relative to the largest magnitude in the reference array (robust to cancellation)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-12, float(np.max(np.abs(b))))) if a.size else 0.0


def synthetic_rollout(T, N, D, A, seed=0, p_done=0.02):
    """A random rollout buffer with episode boundaries, for GAE / train parity."""
    rng = np.random.default_rng(seed)
    f = np.float32
    buf = dict(obs=rng.standard_normal((T, N, D)).astype(f), actions=rng.standard_normal((T, N, A)).astype(f),
               rewards=(0.03 + 0.5 * rng.standard_normal((T, N))).astype(f),
               episode_starts=(rng.random((T, N)) < p_done).astype(f),
               values=rng.standard_normal((T, N)).astype(f), log_probs=(-A + rng.standard_normal((T, N))).astype(f))
    last_values = rng.standard_normal(N).astype(f)
    dones = rng.random(N) < 0.3
    return buf, last_values, dones


# ---- tests/golden/arch_cases.npz (make_arch_fixture.py): other activations and depths through torch's own modules ----
_ARCH = None


def arch_cases():
    """-> list of case names"""
    global _ARCH
    if _ARCH is None:
        _ARCH = np.load(os.path.join(GOLDEN, "arch_cases.npz"))
    return [str(c) for c in _ARCH["cases"]]


ARCH_CASES = ["act_tanh", "act_relu", "act_elu", "act_leakyrelu", "act_sigmoid", "act_softplus", "act_softsign", "act_hardtanh",
              "act_relu6", "depth4_tanh", "depth5_3_elu", "depth8_relu", "depth1_6_tanh", "act_silu", "act_gelu", "act_mish"]


def arch_case(name):
    """-> (case dict of arrays without the name prefix, activation, pi widths, vf widths, params, Hyper)"""
    arch_cases()
    pre = name + "/"
    c = {k[len(pre):]: _ARCH[k] for k in _ARCH.files if k.startswith(pre)}
    act, pi, vf = str(c["activation"]), tuple(int(w) for w in c["pi"]), tuple(int(w) for w in c["vf"])
    keys = O.param_keys(len(pi), len(vf))
    p = OrderedDict((k, c["p/" + k].astype(np.float32).copy()) for k in keys)
    lr, clip, ent, vfc, mgn, eps = (float(x) for x in _ARCH["hyper"])
    h = O.Hyper(clip_range=clip, ent_coef=ent, vf_coef=vfc, max_grad_norm=mgn, learning_rate=lr, adam_eps=eps, activation=act,
                batch_size=100, n_epochs=1)
    return c, act, pi, vf, p, h


# ---- tests/golden/sde_cases.npz (make_sde_fixture.py): PPO(use_sde=True) through torch's own ops ----
SDE_CASES = ["sde_tanh_2x2", "sde_relu_1_3", "sde_elu_4", "sde_expln", "sde_shared_std", "sde_shared_expln"]
_SDE = None


def sde_case(name):
    """-> (case dict, activation, pi, vf, params, Hyper(use_sde=True, sde_use_expln=...)); c["full_std"] / c["use_expln"]: the options"""
    global _SDE
    if _SDE is None:
        _SDE = np.load(os.path.join(GOLDEN, "sde_cases.npz"))
    assert [str(c) for c in _SDE["cases"]] == SDE_CASES
    pre = name + "/"
    c = {k[len(pre):]: _SDE[k] for k in _SDE.files if k.startswith(pre)}
    act, pi, vf = str(c["activation"]), tuple(int(w) for w in c["pi"]), tuple(int(w) for w in c["vf"])
    p = OrderedDict((k, c["p/" + k].astype(np.float32).copy()) for k in O.param_keys(len(pi), len(vf)))
    lr, clip, ent, vfc, mgn, eps = (float(x) for x in _SDE["hyper"])
    h = O.Hyper(clip_range=clip, ent_coef=ent, vf_coef=vfc, max_grad_norm=mgn, learning_rate=lr, adam_eps=eps, activation=act,
                batch_size=100, n_epochs=1, use_sde=True, sde_use_expln=bool(c["use_expln"]))
    return c, act, pi, vf, p, h


# ---- GPU tests of the evaluation family (test_eval_gpu.py, test_follow_gpu.py) ----
# (name, robot, engine kwargs, MOBROB_EVAL_PERSISTENT, persistent path expected)
EVAL_CASES = [
    ("doggo64", "doggo", dict(pi=(64, 64), vf=(64, 64)), None, True),
    ("point64", "point", dict(pi=(64, 64), vf=(64, 64)), None, True),
    ("doggo256", "doggo", dict(pi=(256, 256), vf=(256, 256)), None, False),
    ("elu3x32", "point", dict(pi=(32, 32, 32), vf=(32, 32, 32), activation="elu"), None, False),
    ("sde64", "point", dict(pi=(64, 64), vf=(64, 64), use_sde=True), None, False),
    ("doggo64_perstep", "doggo", dict(pi=(64, 64), vf=(64, 64)), "0", False),
]
EVAL_IDS = [c[0] for c in EVAL_CASES]


@pytest.fixture
def persistent_env(monkeypatch):
    def set_(v):
        if v is None:
            monkeypatch.delenv("MOBROB_EVAL_PERSISTENT", raising=False)
        else:
            monkeypatch.setenv("MOBROB_EVAL_PERSISTENT", v)
    return set_


def _engine(robot, kw, n_envs=16, seed=3, scale=1.0):
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs.wrapper import ROBOT_DIMS
    D, A, _ = ROBOT_DIMS[robot]
    e = PPOEngine(obs_dim=D, act_dim=A, n_envs=n_envs, n_steps=16, batch_size=64, n_epochs=2, seed=seed, **kw)
    rng = np.random.default_rng(seed)
    p = e.get_params()
    for k, v in p.items():
        if k == "log_std":
            p[k] = np.full_like(v, -0.5)
        elif v.ndim == 2:
            p[k] = (scale * rng.standard_normal(v.shape) / np.sqrt(v.shape[1])).astype(np.float32)
        else:
            p[k] = (0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    e.set_params(p)
    return e, p


def _env(robot, n, tl=0, seed=5):
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    return DeviceGoalVecEnv.for_robot(robot, n, time_limit=tl, seed=seed)


def _snapshot(e, stats=True):
    s = {k: e.read(k) for k in ("obs", "actions", "rewards", "values", "log_probs", "episode_starts")}
    m, v, step = e.get_optimizer_state()
    s["params"], s["m"], s["v"], s["step"] = e.get_flat_params(), e.flatten(m), e.flatten(v), step
    if stats:
        st = e.episode_stats(reset=False)
        s["stats_counts"] = np.array([st["episodes"], st["goals"]])
        s["stats_means"] = np.array([st["ep_rew_mean"], st["ep_len_mean"]])
    s["env_state"] = e.read("env_state")
    return s


def _go_to_goal_params(e, env, zero=False):
    """A near-linear tanh actor: h1 = tanh(s * unit), h2 = tanh(h1), mean = pinv(mix) . unit (times a gain)."""
    p = e.get_params()
    for k in p:
        p[k] = np.zeros_like(p[k])
    P = env.pos_dim
    s = 0.1
    W1 = np.zeros_like(p["mlp_extractor.policy_net.0.weight"])
    W2 = np.zeros_like(p["mlp_extractor.policy_net.2.weight"])
    for j in range(P):
        W1[j, j] = s
        W2[j, j] = 1.0
    p["mlp_extractor.policy_net.0.weight"] = W1
    p["mlp_extractor.policy_net.2.weight"] = W2
    Wa = np.zeros_like(p["action_net.weight"])
    if not zero:   # command mix . a = unit vector to the goal (speed 1)
        gain = 1.0 / np.tanh(np.tanh(s))
        Wa[:, :P] = (gain * np.linalg.pinv(env.mix.astype(np.float64))).astype(np.float32)
    p["action_net.weight"] = Wa
    p["log_std"] = np.full_like(p["log_std"], -1.0)
    e.set_params(p)


def _write_checkpoint(data_dir, robot):
    """data/policies/<robot>-ppo.zip with the reference checkpoint's weights (tests/golden/<robot>.npz)."""
    from mobrob_amd.rl_control.ppo import PPO
    model = PPO(env=_env(robot, 16, tl=1000), n_steps=16, batch_size=64, seed=0)
    model.engine.set_params(golden_params(load_golden(robot)))
    os.makedirs(os.path.join(data_dir, "policies"), exist_ok=True)
    model.save(os.path.join(data_dir, "policies", f"{robot}-ppo.zip"))
