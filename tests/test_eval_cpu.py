"""CPU: evaluate_policy's host path (SB3 2.0 semantics) and EvalCallback's bookkeeping, with stub models and environments."""
import os

import numpy as np
import pytest

from mobrob_amd.evaluation import evaluate_policy
from mobrob_amd.rl_control.ppo import EvalCallback, StopTrainingOnRewardThreshold


class _CountdownVecEnv:
    """n envs; env i ends its episodes after lengths[i] steps; reward 1 per step (episode return == length)."""

    def __init__(self, lengths):
        self.lengths = list(lengths)
        self.num_envs = len(self.lengths)
        self.t = np.zeros(self.num_envs, int)
        self.steps_seen = np.zeros(self.num_envs, int)

    def reset(self):
        self.t[:] = 0
        return np.zeros((self.num_envs, 3), np.float32)

    def step(self, actions):
        assert actions.shape == (self.num_envs, 2)
        self.t += 1
        self.steps_seen += 1
        dones = self.t >= np.array(self.lengths)
        infos = [{"is_success": bool(i % 2 == 0)} if d else {} for i, d in enumerate(dones)]
        self.t[dones] = 0
        return np.zeros((self.num_envs, 3), np.float32), np.ones(self.num_envs, np.float32), dones, infos


class _StubModel:
    def __init__(self):
        self.calls = []

    def predict(self, obs, state=None, episode_start=None, deterministic=False):
        self.calls.append(deterministic)
        return np.zeros((obs.shape[0], 2), np.float32), None


def test_host_evaluate_policy_follows_the_sb3_episode_split():
    env = _CountdownVecEnv([2, 3, 5])
    m = _StubModel()
    rewards, lengths = evaluate_policy(m, env, n_eval_episodes=7, return_episode_rewards=True)
    # SB3: episode_count_targets = [(7 + i) // 3] = [2, 2, 3]
    assert sorted(lengths) == sorted([2, 2, 3, 3, 5, 5, 5])
    assert rewards == [float(x) for x in lengths]
    assert all(m.calls)                       # deterministic=True by default
    mean, std = evaluate_policy(m, env, n_eval_episodes=7)
    assert mean == pytest.approx(np.mean([2, 2, 3, 3, 5, 5, 5])) and std == pytest.approx(np.std([2, 2, 3, 3, 5, 5, 5]))


def test_host_evaluate_policy_reward_threshold_and_single_env():
    class One:
        def __init__(self):
            self.t = 0

        def reset(self):
            self.t = 0
            return np.zeros(3, np.float32), {}

        def step(self, a):
            self.t += 1
            return np.zeros(3, np.float32), 0.5, self.t % 4 == 0, False, {}

    mean, _ = evaluate_policy(_StubModel(), One(), n_eval_episodes=3)
    assert mean == pytest.approx(2.0)
    with pytest.raises(AssertionError):
        evaluate_policy(_StubModel(), One(), n_eval_episodes=2, reward_threshold=5.0)


class _StubPPO:
    world_size = 1

    def __init__(self, tmp):
        self.num_timesteps, self.saved, self.records, self.tmp = 0, [], {}, tmp

    def save(self, path):
        self.saved.append(path)
        open(path + ".zip", "wb").close()

    def _record(self, k, v):
        self.records[k] = v


def test_eval_callback_file_format_best_model_and_stop(tmp_path):
    means = iter([1.0, 3.0, 2.0, 9.0])

    def fake_eval(model, env, n, deterministic):
        m = next(means)
        return [m - 0.5, m + 0.5], [10, 12], [True, False]

    stop = StopTrainingOnRewardThreshold(reward_threshold=8.0)
    cb = EvalCallback(object(), callback_on_new_best=stop, n_eval_episodes=2, eval_freq=3, log_path=str(tmp_path / "logs"),
                      best_model_save_path=str(tmp_path / "best"), verbose=0)
    cb.evaluate_fn = fake_eval
    model = _StubPPO(tmp_path)
    cb.init_callback(model)
    go = []
    for k in range(12):
        model.num_timesteps = 8 * (k + 1)
        go.append(cb.on_step())
    assert go == [True] * 11 + [False]        # the fourth evaluation (mean 9) crosses the threshold
    d = np.load(tmp_path / "logs" / "evaluations.npz")
    assert sorted(d.files) == ["ep_lengths", "results", "successes", "timesteps"]
    assert d["timesteps"].tolist() == [24, 48, 72, 96]
    assert d["results"].shape == (4, 2) and d["ep_lengths"].shape == (4, 2) and d["successes"].shape == (4, 2)
    assert cb.best_mean_reward == 9.0 and cb.last_mean_reward == 9.0
    assert len(model.saved) == 3 and all(p.endswith(os.path.join("best", "best_model")) for p in model.saved)
    assert model.records["eval/mean_reward"] == 9.0 and model.records["eval/mean_ep_length"] == 11.0
    assert model.records["eval/success_rate"] == 0.5


def test_eval_callback_refuses_data_parallel():
    m = _StubPPO(None)
    m.world_size = 2
    with pytest.raises(ValueError, match="data-parallel"):
        EvalCallback(object(), eval_freq=1).init_callback(m)
