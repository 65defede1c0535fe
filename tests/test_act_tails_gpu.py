"""GPU: per-unit activation probes (tests/act_probe.py) on the generic chain and on the fused tanh families: every hidden activation's f(z) and f'(z) read back
unit by unit on the tails and kinks, against float64 closed forms, with the bounds tests/test_act_tails_cpu.py measures:

  |got - ref64| <= BOUND[act][dir] * max(1, |ref64|),   BOUND = max(2^-22, ~2 x the oracle's float32 formula's own error)
  (all on the floor 2^-22 except the silu / mish backwards, 1.9 x 7.45e-7 and 1.9 x 8.18e-7);
  softplus backward for -80 <= z <= -5 RELATIVE, 4 ulp = 4.77e-7 (the corrected formula measures 1.41e-7 on the CPU): with the
  cancelling 1 - exp(-h) the kernel returned exactly 0 from z = -17 on, and this test failed.

Measured on the MI355X, worst forward / backward in units of 2^-22: tanh 0.17 / 0.29, relu 0 / 0.13, elu 0.17 / 0.32, leakyrelu
0.15 / 0.10, sigmoid 0.34 / 0.34, softplus 0.24 / 0.31, softsign 0.15 / 0.47, hardtanh 0 / 0.17, relu6 0 / 0.10, silu 0.32 / 3.22, gelu
0.37 / 0.43, mish 0.32 / 1.96; softplus backward relative on [-80, -5]: 1.07e-7 (parent: 74 of 120 probed units exactly 0).

The 64- and 256-wide tanh families (fast_tanh / fast_tanh_scaled) are held to the code's own claim, 2e-7 absolute, to 4e-7 + 2^-23 for
the 1 - h^2 of the backward, to h == +-1 exactly from |z| = 20 on and to finite values up to 1e30.  Measured, every forward family
(k_fused64_act, k_rollout64_tile, k_rollout64_persistent, k_fused_act, k_rollout_persistent x3 and f32): 1.42e-7 at z = -0.999;
backward k_split64_train, k_fused64_train, k_pair64_train, k_epoch64: 2.40e-7; k_chain_train, k_fused_train x3 and f32: 2.44e-7, at
the same point.  The claim holds.  Layer 2 of the generic chain stays inside layer 1's figures (worst mish backward 1.96).

The two one-launch evaluation tiles came later and build their own observations, so no selector row reaches them: their layer 2 is
probed through a bias-saturated layer 1 (tests/act_probe.py tile_probe) and read back as the traced action of a one-step evaluation.
Every layer-2 unit, every point of TANH_POS in both signs, every column of W2 (all k-quarters of the fragment; on the 256 tile the
register-resident slice, a quarter of it in AGPRs).  Measured: k_goal64_tile<16>, <32>, <48>, <64> (point, car, turtlebot3, doggo),
<16> with two head blocks (drone), k_goal256_tile with one and two head blocks (doggo, drone): 1.42e-7 at z = -0.999 each, exactly
+-1 from |z| = 20 on, finite with 1e30 in W2.  Layer 1 of the tiles is exercised as the saturated selector only: there is no
per-unit probe of their layer 1 here.

Hidden widths 72 and 40 are no multiples of the 32-wide fragment, so clamped lanes are in play; the probed units sit on both sides of
every fragment edge and at the last column.
"""
import numpy as np
import pytest

from tests import act_probe as P

pytestmark = pytest.mark.gpu
WPI, WVF, A1, D1, N1 = 72, 40, 8, 9, 64


def _engine(D, A, N, T, pi, vf, **kw):
    from mobrob_amd.engine import PPOEngine
    return PPOEngine(obs_dim=D, act_dim=A, n_envs=N, n_steps=T, pi=pi, vf=vf, action_low=-1e38, action_high=1e38, **kw)


def _check(act, direction, got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), (act, what, "not finite")
    e = P.err(got, ref)
    print(f"{act} {what}: worst {float(e.max()) / P.FLOOR:.3f} x 2^-22 (bound {P.BOUND[act][direction] / P.FLOOR:.3f})")
    bad = e > P.BOUND[act][direction]
    assert not bad.any(), (act, what, got[bad][:4], ref[bad][:4], float(e.max()))


@pytest.mark.parametrize("act", P.ACTS)
def test_layer1_forward_per_unit(act):
    """z = obs through act() with eps = 0, predict(), and the per-row value evaluator of a time-limit bootstrap (gamma = 1, reward 0:
    the stored reward is V(terminal_obs))."""
    e = _engine(D1, A1, N1, 1, (WPI,), (WVF,), batch_size=N1, n_epochs=1, activation=act, gamma=1.0)
    zero = np.zeros((N1, A1), np.float32)
    linear = 0
    for k in range(-(-len(P.GRID) // N1)):
        p, obs, units, uv = P.layer1_forward(D1, A1, WPI, WVF, P.GRID, N1, k)
        e.set_params(p)
        zpi, zvf = obs[:, [u % D1 for u in units]], obs[:, uv % D1]
        ref_m, ref_v = P.f(act, zpi), P.f(act, zvf)
        e.rollout_begin()
        a_raw, a_clip, val, _ = e.act(obs, zero)
        e.store(np.zeros(N1, np.float32), np.ones(N1, bool), np.ones(N1, bool), obs)
        boot = e.read("rewards")[0]
        e.finish_rollout(obs, np.ones(N1, bool))
        pm, pv = e.predict(obs, deterministic=True, want_values=True)
        for what, got, ref in (("act mean", a_raw, ref_m), ("act value", val, ref_v), ("predict mean", pm, ref_m), ("predict value", pv, ref_v),
                               ("bootstrap value", boot, ref_v)):
            _check(act, 0, got, ref, what)
            if act == "softplus":      # linear above the threshold: f(z) == z
                lin = (zpi if ref is ref_m else zvf) > 20.0
                assert np.array_equal(np.asarray(got)[lin], (zpi if ref is ref_m else zvf)[lin]), what
                linear += int(lin.sum())
        assert np.array_equal(a_clip, a_raw)
    assert act != "softplus" or linear > 0
    e.close()


B_ROWS = 32


def _layer1_backward(act, all_rows=False):
    """-> per network: (z, f'(z) as read off the bias gradient, raw gradient, factor, minibatch index) over all minibatches."""
    B, A = B_ROWS, 2
    nmb = -(-len(P.GRID) // WVF)
    flats, facts = [], []
    for k in range(nmb):
        p, row = P.layer1_backward(WPI, WVF, A, P.GRID, k)
        mb, fpi, fvf, zpi, zvf = P.backward_minibatch(p, row, act, B, active=None if all_rows else (5 * k) % B)
        flats.append(mb)
        facts.append((fpi, fvf, zpi, zvf))
    flat = {k: np.concatenate([m[k] for m in flats]) for k in flats[0]}
    e = _engine(WPI, A, B, nmb, (WPI,), (WVF,), batch_size=B, n_epochs=1, activation=act, normalize_advantage=False, vf_coef=P.VF_COEF)
    e.set_params(p)
    e.load_rollout(P.as_rollout(flat, nmb, B), np.zeros(B, np.float32), np.zeros(B, bool))
    e.epoch_begin(np.arange(nmb * B))
    out = {P.PI: [], P.VF: []}
    for k in range(nmb):
        e.minibatch_grad(k)
        g = e.unflatten(e.read("grads"))
        fpi, fvf, zpi, zvf = facts[k]
        for prefix, fac, z in ((P.PI, fpi, zpi), (P.VF, fvf, zvf)):
            raw = g[P.hidden_bias_key(prefix, 0)].astype(np.float64)
            assert np.all(np.abs(fac) > 0.5)
            out[prefix].append((z, raw / fac, raw, fac, np.full(len(z), k)))
    e.close()
    return {k: tuple(np.concatenate([t[i] for t in v]) for i in range(5)) for k, v in out.items()}


def _check_kinks(act, prefix, ref, raw, fac, mb):
    """Kinked activations: the derivative is exactly 0, or every unit of one slope carries the same float, 0.01f of it on the leaky
    side, and that float is float32(factor).  For the value net exactly: its factor is 2 vf_coef w (v - return) / B with powers of
    two around one rounding of v - return.  For the policy net to 2 ulp: its factor carries ratio = expf(log-prob - old log-prob), 1
    up to the rounding of a log-prob of magnitude 1.8 (half an ulp of 2^-23 relative to 1) and expf's own ulp."""
    assert np.all(raw[ref == 0.0] == 0.0), (act, prefix)
    for k in np.unique(mb):      # (the factor is one float per minibatch)
        one, leak = raw[(mb == k) & (ref == 1.0)], raw[(mb == k) & (ref == 0.01)]
        assert len(set(one.tolist())) <= 1 and len(set(leak.tolist())) <= 1, (act, prefix, k, one[:4], leak[:4])
        if len(one) and len(leak):
            assert np.float32(leak[0]) == np.float32(0.01) * np.float32(one[0]), (act, prefix, k, leak[0], one[0])
        if len(one):
            f32 = np.float32(fac[(mb == k) & (ref == 1.0)][0])
            ulps = abs(float(np.float32(one[0])) - float(f32)) / float(np.spacing(np.abs(f32)))
            assert ulps <= (0 if prefix == P.VF else 2), (act, prefix, k, one[0], f32, ulps)


@pytest.mark.parametrize("act", P.ACTS)
def test_layer1_backward_per_unit(act):
    """f'(z) = bias gradient / factor over minibatches of identical rows, one of which carries the loss (the row moves with the
    minibatch); then with every row carrying it, where the float32 column sum of B equal terms rounds up to B - 1 times, 2^-24 of the
    sum each: bound + (B - 1) 2^-24."""
    for all_rows in (False, True):
        res = _layer1_backward(act, all_rows)
        for prefix, (z, d, raw, fac, mb) in res.items():
            ref = P.df(act, z)
            if all_rows:
                e = P.err(d, ref)
                print(f"{act} {prefix} f' (all rows): worst {float(e.max()) / P.FLOOR:.3f} x 2^-22")
                assert np.isfinite(d).all() and np.all(e <= P.BOUND[act][1] + (B_ROWS - 1) * 2.0 ** -24), (act, prefix, float(e.max()))
                continue
            _check(act, 1, d, ref, f"{prefix} f'")
            if act in P.KINKED:
                _check_kinks(act, prefix, ref, raw, fac, mb)


# ------------------------------------------------------------------------------------------------
# a deeper layer: z2 through the second layer's bias (both GEMMs of the chain, the stored-z path of silu / gelu / mish at layer 2,
# the backward epilogue behind a hidden weight matrix; widths 40 and 24 clamp fragment lanes of the second GEMM)
# ------------------------------------------------------------------------------------------------
PI2, VF2, A2 = (72, 40), (40, 24), 20


@pytest.mark.parametrize("act", P.ACTS)
def test_layer2_forward_per_unit(act):
    N = 8
    e = _engine(D1, A2, N, 1, PI2, VF2, batch_size=N, n_epochs=1, activation=act)
    obs, zero = np.zeros((N, D1), np.float32), np.zeros((N, A2), np.float32)
    for k in range(-(-len(P.GRID) // A2)):
        p, units, uv = P.layer2_bias(D1, A2, PI2, VF2, P.GRID, k, act)
        e.set_params(p)
        mean, value, zpi, zvf = P.forward64(p, obs, act)
        a_raw, _, val, _ = e.act(obs, zero)
        pm, pv = e.predict(obs, deterministic=True, want_values=True)
        for what, got, ref in (("act mean", a_raw, mean), ("act value", val, value), ("predict mean", pm, mean), ("predict value", pv, value)):
            _check(act, 0, got, ref, "layer 2 " + what)
    e.close()


@pytest.mark.parametrize("act", P.ACTS)
def test_layer2_backward_per_unit(act):
    B, A = B_ROWS, 2
    e = _engine(D1, A, B, 1, PI2, VF2, batch_size=B, n_epochs=1, activation=act, normalize_advantage=False, vf_coef=P.VF_COEF)
    for k in range(-(-len(P.GRID) // min(PI2[1], VF2[1]))):
        p, _, _ = P.layer2_bias(D1, A, PI2, VF2, P.GRID, k, act, heads="uniform")
        mb, fpi, fvf, zpi, zvf = P.backward_minibatch(p, np.zeros(D1, np.float32), act, B, active=(5 * k) % B)
        e.set_params(p)
        e.load_rollout(P.as_rollout(mb, 1, B), np.zeros(B, np.float32), np.zeros(B, bool))
        e.epoch_begin(np.arange(B))
        e.minibatch_grad(0)
        g = e.unflatten(e.read("grads"))
        for prefix, fac, z in ((P.PI, fpi, zpi), (P.VF, fvf, zvf)):
            raw = g[P.hidden_bias_key(prefix, 1)].astype(np.float64)
            ref = P.df(act, z)
            _check(act, 1, raw / fac, ref, f"layer 2 {prefix} f'")
            if act in P.KINKED:
                _check_kinks(act, prefix, ref, raw, fac, np.zeros(len(z)))
    e.close()


def test_softplus_backward_relative_in_the_left_tail():
    """-80 <= z <= -5: relative error of f'(z) = sigmoid(z) ~ e^z, bound 4 ulp (tests/act_probe.py SOFTPLUS_REL)."""
    res = _layer1_backward("softplus")
    for prefix, (z, d, raw, fac, _) in res.items():
        sel = (z >= -80.0) & (z <= -5.0)
        assert sel.sum() >= len(P.SOFTPLUS_TAIL)
        ref = P.df("softplus", z[sel])
        rel = np.abs(d[sel] - ref) / ref
        print(f"softplus backward {prefix}: worst relative error {float(rel.max()):.3e} (bound {P.SOFTPLUS_REL:.3e}); zeros: {int((d[sel] == 0).sum())}")
        assert np.all(rel <= P.SOFTPLUS_REL), (prefix, z[sel][rel > P.SOFTPLUS_REL][:6], d[sel][rel > P.SOFTPLUS_REL][:6], float(rel.max()))


# ------------------------------------------------------------------------------------------------
# the 64- and 256-wide tanh families (fast_tanh / fast_tanh_scaled, csrc/kernels_fused.h): layer 2 through a column of W2 that a
# saturated layer 1 selects per row (tests/act_probe.py tanh_layer2)
# ------------------------------------------------------------------------------------------------
def _tanh_engine(H, N, monkeypatch, env, **kw):
    from mobrob_amd.engine import PPOEngine
    for name in ("MOBROB_ROLLOUT64_TILE_MAX", "MOBROB_SPLIT64_MAX_TILES", "MOBROB_PAIR64_MIN_TILES", "MOBROB_EPOCH_KERNEL", "MOBROB_NO_CHAIN",
                 "MOBROB_NO_TRAIN_X3"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    return PPOEngine(obs_dim=P.NSEL, act_dim=kw.pop("A"), n_envs=N, n_steps=1, batch_size=N, n_epochs=1, pi=(H, H), vf=(H, H),
                     action_low=-1e38, action_high=1e38, **kw)


def _check_tanh_forward(name, got, z):
    got, z = np.asarray(got, np.float64), np.asarray(z, np.float64)
    assert np.isfinite(got).all(), (name, "not finite", z[~np.isfinite(got)][:4])
    e = np.abs(got - np.tanh(z))
    sat = np.abs(z) >= 20.0
    assert np.array_equal(got[sat], np.sign(z[sat])), (name, "saturation", z[sat][got[sat] != np.sign(z[sat])][:4])
    return float(e.max()), float(z.ravel()[int(np.argmax(e))]), int(sat.sum())


# (family, hidden width, forward_x3, environment, how the forward is reached)
TANH_FORWARD = [("k_fused64_act", 64, True, {}, "act"), ("k_rollout64_tile", 64, True, {}, "rollout"),
                ("k_rollout64_persistent", 64, True, {"MOBROB_ROLLOUT64_TILE_MAX": "0"}, "rollout"),
                ("k_fused_act", 256, True, {}, "act"), ("k_rollout_persistent x3", 256, True, {}, "rollout"),
                ("k_rollout_persistent f32", 256, False, {}, "rollout")]


@pytest.mark.parametrize("name,H,x3,env,how", TANH_FORWARD, ids=[c[0].replace(" ", "_") for c in TANH_FORWARD])
def test_tanh_family_forward(name, H, x3, env, how, monkeypatch):
    """tanh(z2) behind the action head (16 units over the width) and the value head against float64: the code's own claim, 2e-7
    absolute; exactly +-1 from |z| = 20 on; finite up to 1e30 (layer 1 sees +-1e30 in every row).  The rollout kernels draw their
    own noise: log_std = -60 makes the stored action the mean."""
    A, N = 16, 2 * P.NSEL
    rows = P.selector_rows()
    e = _tanh_engine(H, N, monkeypatch, env, A=A, forward_x3=x3)
    assert H == 64 or (e.x3_mode() & 1) == int(x3)
    worst, saturated = (0.0, 0.0), 0
    for off in range(0, 6 * P.NSEL, P.NSEL):
        p, units, uv = P.tanh_layer2(H, A, P.TANH_POS, off)
        mean, value, zpi, zvf = P.forward64(p, rows, "tanh")
        if how == "act":
            e.set_params(p)
            got_m, _, got_v, _ = e.act(rows, np.zeros((N, A), np.float32))
        else:
            p["log_std"][:] = -60.0
            e.set_params(p)
            e.collect_synthetic()                  # starts the device env; its last observation is slot T of `obs`
            e.synchronize()
            slots = e.read("obs")
            slots[1] = rows                        # the next rollout's first observation
            e.write("obs", slots)
            e.collect_synthetic()
            e.synchronize()
            assert np.array_equal(e.read("obs")[0], rows)
            got_m, got_v = e.read("actions")[0], e.read("values")[0]
        for got, z in ((got_m, zpi[:, units]), (got_v, zvf[:, uv])):
            w = _check_tanh_forward(name, got, z)
            worst, saturated = max(worst, w[:2]), saturated + w[2]
    e.close()
    assert saturated > 0
    print(f"{name}: fast_tanh worst absolute error {worst[0]:.3e} at z = {worst[1]:.4g} (claim {P.TANH_FWD_ABS:.1e})")
    assert worst[0] <= P.TANH_FWD_ABS, (name, worst)


# (family, hidden width, forward_x3, environment, rows, "grad": epoch_begin / minibatch_grad, "train": one train() = k_epoch64)
TANH_BACKWARD = [("k_split64_train", 64, True, {}, 32, "grad"), ("k_fused64_train", 64, True, {"MOBROB_SPLIT64_MAX_TILES": "0"}, 32, "grad"),
                 ("k_pair64_train", 64, True, {}, 65 * 32, "grad"), ("k_epoch64", 64, True, {}, 32, "train"),
                 ("k_chain_train", 256, True, {}, 32, "grad"), ("k_fused_train x3", 256, True, {"MOBROB_NO_CHAIN": "1"}, 32, "grad"),
                 ("k_fused_train f32", 256, False, {}, 32, "grad")]


@pytest.mark.parametrize("name,H,x3,env,B,how", TANH_BACKWARD, ids=[c[0].replace(" ", "_") for c in TANH_BACKWARD])
def test_tanh_family_backward(name, H, x3, env, B, how, monkeypatch):
    """1 - h^2 of layer 2 read off its bias gradient: |d(1 - h^2)| <= 2 |h| 2e-7 plus one rounding = 4e-7 + 2^-23 absolute; exactly 0
    from |z| = 20 on.  Points up to 100 and selector rows of +-64 (the far tail is the forward test's: with 1e30 in W2 and in the
    observations the FIRST layer's weight gradient overflows, which is no business of tanh).  One table shows every point to the 64 / 256 units; one minibatch per selector row, one row of it carrying the
    loss.  Learning rate 0 and no gradient clipping, so that the one-launch epoch kernel can be asked too: its gradient is read
    after train()."""
    A = 2
    rows, pts = P.selector_rows(64.0), P.TANH_POS[P.TANH_POS <= 100.0]
    e = _tanh_engine(H, B, monkeypatch, env, A=A, forward_x3=x3, normalize_advantage=False, vf_coef=P.VF_COEF, learning_rate=0.0,
                     max_grad_norm=1e30)
    if H == 256:
        assert e.x3_mode() & 3 == (3 if x3 else 0)
    p, _, _ = P.tanh_layer2(H, A, pts, 0, heads="uniform")
    e.set_params(p)
    worst, seen = (0.0, 0.0), set()
    for r in range(len(rows)):
        mb, fpi, fvf, zpi, zvf = P.backward_minibatch(p, rows[r], "tanh", B, active=(5 * r) % B)
        e.load_rollout(P.as_rollout(mb, 1, B), np.zeros(B, np.float32), np.zeros(B, bool))
        if how == "train":
            e.train(np.arange(B)[None])
            assert e.update_mode() == 1
        else:
            e.epoch_begin(np.arange(B))
            e.minibatch_grad(0)
        g = e.unflatten(e.read("grads"))
        for prefix, fac, z in ((P.PI, fpi, zpi), (P.VF, fvf, zvf)):
            raw = g[P.hidden_bias_key(prefix, 1)].astype(np.float64)
            assert np.isfinite(raw).all(), (name, prefix, r)
            sat = np.abs(z) >= 20.0
            assert np.all(raw[sat] == 0.0), (name, prefix, z[sat][raw[sat] != 0][:4])
            err = np.abs(raw / fac - P.df("tanh", z))
            worst = max(worst, (float(err.max()), float(z[int(np.argmax(err))])))
            seen |= set(np.abs(z).tolist())
    e.close()
    assert seen == set(pts.astype(np.float64).tolist())
    print(f"{name}: 1 - h^2 worst absolute error {worst[0]:.3e} at z = {worst[1]:.4g} (bound {P.TANH_BWD_ABS:.3e})")
    assert worst[0] <= P.TANH_BWD_ABS, (name, worst)


# ------------------------------------------------------------------------------------------------
# the one-launch evaluation tiles (k_goal64_tile at its four observation widths, k_goal256_tile): they build their own observations,
# so layer 2 is reached through a bias-saturated layer 1 (tests/act_probe.py tile_probe) and read back as the traced action of a
# one-step evaluation of 16 robots
# ------------------------------------------------------------------------------------------------
# (kernel, robot: its D picks the tile width and its A the head blocks, hidden width)
TILE_ACTORS = [("k_goal64_tile<16>", "point", 64), ("k_goal64_tile<32>", "car", 64), ("k_goal64_tile<48>", "turtlebot3", 64),
               ("k_goal64_tile<64>", "doggo", 64), ("k_goal64_tile<16> two head blocks", "drone", 64),
               ("k_goal256_tile", "doggo", 256), ("k_goal256_tile two head blocks", "drone", 256)]


@pytest.mark.parametrize("name,robot,H", TILE_ACTORS, ids=[f"{c[1]}{c[2]}" for c in TILE_ACTORS])
def test_tile_actor_forward(name, robot, H, monkeypatch):
    """fast_tanh of layer 2 in both tile actors, the assertions of test_tanh_family_forward: 2e-7 absolute against float64, exactly
    +-1 from |z| = 20 on, finite with 1e30 in W2.  Every layer-2 unit is probed, each with a point of |z| >= 20 and one of |z| < 1;
    every point of TANH_POS is seen in both signs; the chosen column k of W2 walks through every k-step and k-quarter (on the 256
    tile: through the register-resident fragment; the probed units cover all four waves' head slices).  Layer 1 is exercised as
    the saturated selector only."""
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs.vec_env import DeviceGoalVecEnv
    from mobrob_amd.envs.wrapper import ROBOT_DIMS
    monkeypatch.delenv("MOBROB_EVAL_PERSISTENT", raising=False)
    D, A, _ = ROBOT_DIMS[robot]
    R = 16
    e = PPOEngine(obs_dim=D, act_dim=A, n_envs=R, n_steps=16, batch_size=64, n_epochs=1, pi=(H, H), vf=(H, H))   # action bounds +-1
    if H == 256:
        e.set_eval_tile256(True)
    env = DeviceGoalVecEnv.for_robot(robot, R, time_limit=0, seed=1)
    worst, saturated = (0.0, 0.0), 0
    big, small, cols, seen = np.zeros(H, bool), np.zeros(H, bool), set(), set()
    for i in range(P.tile_launches(A, H)):
        p, units, ks, z = P.tile_probe(D, A, H, i)
        e.set_params(p)
        r = env.evaluate(e, n_robots=R, max_steps=1, trace=(R, 1), seed=i)
        assert r["persistent"] is True
        act = r["trace"][0, :, 9 + D:9 + D + A]
        assert np.array_equal(act, np.broadcast_to(act[0], act.shape)), (name, i, "the robots of a tile differ")
        w = _check_tanh_forward(name, act, np.broadcast_to(z, act.shape))
        worst, saturated = max(worst, w[:2]), saturated + w[2]
        big[units[np.abs(z) >= 20.0]] = True
        small[units[np.abs(z) < 1.0]] = True
        cols |= set(ks.tolist())
        seen |= {(float(abs(v)), bool(np.signbit(v))) for v in z}
    e.close()
    assert big.all() and small.all(), (name, "units without a tail point or a small one", np.flatnonzero(~(big & small)))
    assert cols == set(range(H)), (name, "columns of W2 never chosen")
    assert seen == {(float(v), s) for v in P.TANH_POS for s in (False, True)}
    assert saturated > 0
    print(f"{name}: fast_tanh worst absolute error {worst[0]:.3e} at z = {worst[1]:.4g} (claim {P.TANH_FWD_ABS:.1e})")
    assert worst[0] <= P.TANH_FWD_ABS, (name, worst)
