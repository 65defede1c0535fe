"""GPU: batched on-device policy evaluation (mobrob_ppo_evaluate_goal_env, evaluate_policy, EvalCallback, control.py --robots)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ppo_oracle as O
from tests.eval_model import goal_advance, trace_fields
from tests.util import EVAL_CASES as CASES, EVAL_IDS as IDS, _engine, _env, _go_to_goal_params, _snapshot, _write_checkpoint, persistent_env  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_teacher_forced_trace(case, persistent_env):
    name, robot, kw, pe, expect_persistent = case
    persistent_env(pe)
    e, p = _engine(robot, kw)
    env = _env(robot, 8, tl=40)
    D, A, P = e.D, e.A, env.pos_dim
    S, R = 120, 8
    r = env.evaluate(e, n_robots=R, max_steps=S, episodes=0, quota=np.full(R, 50, np.int32), trace=(R, S), seed=9)
    assert r["persistent"] == expect_persistent
    f = trace_fields(r["trace"], D, A)
    act = kw.get("activation", "tanh")
    mean, _ = O.policy_outputs(p, f["obs"].reshape(-1, D).astype(np.float32), activation=act)
    want = np.clip(mean, -1.0, 1.0).reshape(S, R, A)
    assert np.max(np.abs(f["act"] - want)) <= 1e-5 * max(1.0, float(np.max(np.abs(want))))
    # transitions
    for t in range(S):
        pos2, vel2, rew, reached = goal_advance(f["pos"][t], f["vel"][t], f["goal"][t], f["act"][t], env.mix, P, env.dt,
                                                env.extent, extra_bonus=env.extra_bonus)
        assert np.max(np.abs(f["reward"][t] - rew)) <= 2e-6
        assert np.array_equal(f["reached"][t], reached)
        if t + 1 == S:
            break
        done = f["term"][t] | f["tr"][t]
        cont = ~done
        assert np.allclose(f["pos"][t + 1][cont, :P], pos2[cont], atol=1e-6)
        assert np.allclose(f["vel"][t + 1][cont, :P], vel2[cont], atol=1e-6)
        assert np.array_equal(f["goal"][t + 1][cont], f["goal"][t][cont])
        rch = f["term"][t]   # lazy reset: pose kept, new goal in [-extent, extent]
        assert np.allclose(f["pos"][t + 1][rch, :P], pos2[rch], atol=1e-6)
        assert np.all(np.abs(f["goal"][t + 1][rch, :P]) <= env.extent)
        trc = f["tr"][t]     # truncation: fresh pose in [-extent/2, extent/2], zero velocity
        assert np.all(np.abs(f["pos"][t + 1][trc, :P]) <= env.extent / 2)
        assert np.all(f["vel"][t + 1][trc] == 0.0)
    assert f["tr"].any(), "the run should truncate some episodes (time_limit 40 < 120 steps)"
    # robot_out / episode_out against float64 sums over the trace
    rew64 = f["reward"].astype(np.float64)
    for i in range(R):
        assert r["reward_sum"][i] == sum(float(x) for x in rew64[:, i])
        assert r["steps"][i] == S
        ends = np.nonzero(f["term"][:, i] | f["tr"][:, i])[0]
        assert r["episodes"][i] == len(ends)
        assert r["goals"][i] == int(f["reached"][:, i].sum())
        start = 0
        for k, end in enumerate(ends):
            ret = 0.0
            for x in rew64[start:end + 1, i]:
                ret += float(x)
            assert r["episode_returns"][i, k] == ret
            assert r["episode_lengths"][i, k] == end + 1 - start
            assert r["episode_success"][i, k] == float(f["reached"][end, i])
            start = end + 1
    e.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_quota_bookkeeping_and_invalid_specs(case, persistent_env):
    name, robot, kw, pe, expect_persistent = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    TL, n, total = 30, 10, 25
    env = _env(robot, n, tl=TL)
    q = (total + np.arange(n)) // n
    S = int(q.max()) * TL                              # the default max_steps of a quota run
    r = env.evaluate(e, episodes=total, seed=2, trace=(n, S))
    f = trace_fields(r["trace"], e.D, e.A)
    assert np.array_equal(r["quota"], q) and r["episode_returns"].shape == (n, q.max())
    assert np.array_equal(r["episodes"], q)           # every robot met its quota, then idled
    for i in range(n):
        L = r["episode_lengths"][i, :q[i]].astype(int)
        assert np.all(L <= TL) and np.all(L >= 1)
        assert r["steps"][i] == L.sum()                # no step after the quota
        if q[i] < q.max():
            assert r["steps"][i] < S
        last = np.cumsum(L) - 1                        # trace rows of the episodes' last steps
        bonus = f["reward"][last, i] > 4.0             # the goal bonus (+5) dominates a one-step progress of <= 0.1
        assert np.array_equal(r["episode_success"][i, :q[i]] == 1.0, bonus)
        assert not np.any(f["obs"][r["steps"][i]:, i])   # idle rows of the trace stay zero
    with pytest.raises(ValueError):
        env.evaluate(e, n_robots=0)
    with pytest.raises(ValueError):
        e.evaluate_goal_env(env.pos_dim, env.mix, 0, n_robots=4, max_steps=10, episodes=4)
    if kw.get("use_sde"):
        with pytest.raises(ValueError, match="gSDE"):
            env.evaluate(e, episodes=4, deterministic=False)
    e.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_determinism(case, persistent_env):
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    e, _ = _engine(robot, kw)
    env = _env(robot, 64, tl=50)
    outs = [env.evaluate(e, n_robots=64, max_steps=200, deterministic=True, seed=s) for s in (1, 1, 2)]
    stoch = [env.evaluate(e, n_robots=64, max_steps=200, deterministic=False, seed=s) for s in (1, 1, 2)] if not kw.get("use_sde") else []
    for k in ("reward_sum", "steps", "episodes", "goals"):
        assert np.array_equal(outs[0][k], outs[1][k])
        if stoch:
            assert np.array_equal(stoch[0][k], stoch[1][k])
    assert not np.array_equal(outs[0]["reward_sum"], outs[2]["reward_sum"])
    if stoch:
        assert not np.array_equal(stoch[0]["reward_sum"], stoch[2]["reward_sum"])
        assert not np.array_equal(stoch[0]["reward_sum"], outs[0]["reward_sum"])
    e.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[4], CASES[2]], ids=["fused64", "generic_elu", "generic_sde", "x3_256"])
def test_evaluation_does_not_interfere_with_training(case, persistent_env):
    name, robot, kw, pe, _ = case
    persistent_env(pe)
    env_a, env_b = _env(robot, 16, tl=40), _env(robot, 16, tl=40)
    ea, _ = _engine(robot, kw, seed=7)
    eb, _ = _engine(robot, kw, seed=7)
    for it in range(3):
        env_a.collect(ea)
        env_b.collect(eb)
        env_b.evaluate(eb, n_robots=33, max_steps=60, seed=it)
        env_b.evaluate(eb, n_robots=5, episodes=7, seed=it + 10)
        sa, sb = _snapshot(ea), _snapshot(eb)
        # the Monitor statistics are float64 atomics and the record ring's slot order is the order of those atomics across
        # workgroups (kernels_env.h): equal as multisets and up to the summation order, with or without an evaluation
        for k in sa:
            if k == "stats_means":
                assert np.allclose(sa[k], sb[k], rtol=1e-12, atol=0, equal_nan=True), f"iteration {it}: {k}"
            else:
                assert np.array_equal(sa[k], sb[k]), f"iteration {it}: {k} differs after collect"
        recs = [sorted((r["r"], r["l"]) for r in x.episode_records(100)) for x in (ea, eb)]
        assert recs[0] == recs[1]
        ea.train()
        eb.train()
        env_b.evaluate(eb, n_robots=17, max_steps=30, seed=99)
        assert np.array_equal(ea.get_flat_params(), eb.get_flat_params())
    env_a.collect(ea)
    env_b.collect(eb)
    sa, sb = _snapshot(ea), _snapshot(eb)
    for k in ("obs", "actions", "rewards", "params", "m", "v"):
        assert np.array_equal(sa[k], sb[k]), k
    ea.close()
    eb.close()


def test_persistent_and_per_step_paths_agree(persistent_env):
    """Not bit-identical: the persistent kernel runs the actor on the 16x16x4 MFMA with its own tanh, the per-step path the fused
    forward's 32x32x2 order -- the two agree statistically."""
    e, _ = _engine("doggo", dict(pi=(64, 64), vf=(64, 64)), scale=1.0)
    env = _env("doggo", 4096, tl=100)
    persistent_env(None)
    a = env.evaluate(e, n_robots=4096, max_steps=300, episodes=0, quota=np.ones(4096, np.int32), seed=4)
    persistent_env("0")
    b = env.evaluate(e, n_robots=4096, max_steps=300, episodes=0, quota=np.ones(4096, np.int32), seed=4)
    assert a["persistent"] and not b["persistent"]
    for k in ("reward_sum",):
        se = np.sqrt(a[k].var() / 4096 + b[k].var() / 4096)
        assert abs(a[k].mean() - b[k].mean()) <= 3 * se + 1e-9
    sa, sb = np.nan_to_num(a["episode_success"][:, 0]), np.nan_to_num(b["episode_success"][:, 0])
    assert abs(sa.mean() - sb.mean()) <= 3 * np.sqrt((sa.var() + sb.var()) / 4096) + 1e-9
    assert np.mean(a["episodes"] == b["episodes"]) >= 0.95
    e.close()


def test_a_policy_that_solves_the_task_scores_as_one():
    from mobrob_amd.evaluation import evaluate_episodes, evaluate_policy
    from mobrob_amd.envs.vec_env import HostVecEnv, make_vec_env
    from mobrob_amd.envs.wrapper import get_env
    from mobrob_amd.rl_control.ppo import PPO
    env = _env("point", 16, tl=200)
    model = PPO(env=env, n_steps=16, batch_size=64, seed=1)
    _go_to_goal_params(model.engine, env)
    rew, lens, succ = evaluate_episodes(model, env, n_eval_episodes=256)
    assert len(rew) == 256 and np.mean(succ) >= 0.9, np.mean(succ)
    zero_model = PPO(env=env, n_steps=16, batch_size=64, seed=1)
    _go_to_goal_params(zero_model.engine, env, zero=True)
    _, _, succ0 = evaluate_episodes(zero_model, env, n_eval_episodes=256)
    assert np.mean(succ0) < np.mean(succ) - 0.3
    mean_d, std_d = evaluate_policy(model, env, n_eval_episodes=256)
    host = make_vec_env(get_env, 8, env_kwargs=dict(env_name="point", terminate_on_goal=True, time_limit=200), vec_env_cls=HostVecEnv,
                        seed=3)
    hr, hl, hs = evaluate_episodes(model, host, n_eval_episodes=96)
    se_r = np.sqrt(np.var(rew) / len(rew) + np.var(hr) / len(hr))
    assert abs(np.mean(rew) - np.mean(hr)) <= 3 * se_r + 1e-9, (np.mean(rew), np.mean(hr))
    se_s = np.sqrt(np.var(succ) / len(succ) + np.var(hs) / len(hs))
    assert abs(np.mean(succ) - np.mean(hs)) <= max(3 * se_s, 0.02)
    assert mean_d == pytest.approx(np.mean(rew))


def test_eval_callback_end_to_end(tmp_path):
    from mobrob_amd.evaluation import evaluate_policy
    from mobrob_amd.rl_control.ppo import PPO, EvalCallback, StopTrainingOnRewardThreshold
    from mobrob_amd import tb_events as tb
    env = _env("point", 16, tl=100)
    eval_env = _env("point", 8, tl=100, seed=21)
    model = PPO(env=env, n_steps=32, batch_size=128, n_epochs=2, seed=1, tensorboard_log=str(tmp_path / "tb"), verbose=1)
    stop = StopTrainingOnRewardThreshold(reward_threshold=-1e9)   # the first evaluation already crosses it
    cb = EvalCallback(eval_env, n_eval_episodes=8, eval_freq=32, log_path=str(tmp_path / "logs"),
                      best_model_save_path=str(tmp_path / "best"), verbose=1)
    model.learn(total_timesteps=16 * 32 * 3, callback=cb)
    d = np.load(tmp_path / "logs" / "evaluations.npz")
    assert sorted(d.files) == ["ep_lengths", "results", "successes", "timesteps"]
    assert d["results"].shape == (3, 8) and d["ep_lengths"].shape == (3, 8) and d["timesteps"].tolist() == [512, 1024, 1536]
    best = PPO.load(str(tmp_path / "best" / "best_model.zip"))
    mean, _ = evaluate_policy(best, eval_env, n_eval_episodes=8)
    assert mean == pytest.approx(cb.best_mean_reward, abs=1e-9)
    run = os.path.join(str(tmp_path / "tb"), "PPO_1")
    ev = tb.read_events(os.path.join(run, os.listdir(run)[0]))
    for k in ("eval/mean_reward", "eval/mean_ep_length", "eval/success_rate"):
        assert all(k in e["scalars"] for e in ev[1:]), k
    # StopTrainingOnRewardThreshold ends learn() early
    model2 = PPO(env=env, n_steps=32, batch_size=128, n_epochs=2, seed=1)
    cb2 = EvalCallback(eval_env, callback_on_new_best=stop, n_eval_episodes=4, eval_freq=32, verbose=0)
    model2.learn(total_timesteps=16 * 32 * 10, callback=cb2)
    assert model2.num_timesteps == 16 * 32 < 16 * 32 * 10


def test_control_cli_robots(tmp_path):
    _write_checkpoint(str(tmp_path), "point")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "control.py"), "--env-name", "point", "--robots", "64"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, MOBROB_DATA_DIR=str(tmp_path)))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert lines[0].startswith("average reward: ") and lines[1].startswith("reward stds: ") and lines[2].startswith("rewards: [")
    rewards = eval(lines[2][len("rewards: "):])
    assert len(rewards) == 64
    assert float(lines[0].split(": ")[1]) == pytest.approx(np.mean(rewards))
