"""CPU: the activation probe's own footing (tests/act_probe.py), before tests/test_act_tails_gpu.py holds the kernels to it.

(a) the float64 closed forms against torch's float64 autograd of the torch.nn modules, on the whole grid: 1e-12 relative or 1e-300
    absolute.  Where torch's own float64 backward formula cancels and the closed form here does not (TORCH_CANCELS: 1 - tanh^2 is
    exactly 0 at z = -100, where the derivative is 5.5e-87; s (1 - s)), and only at the points of
    those activations where the two differ by more than 1e-12 relative, the derivative is held to 4 float64 epsilons of the O(1) terms
    that cancel, and the test shows that torch's value there is the cancelling formula's, evaluated in float64;
(b) the oracle's float32 restatements against the closed forms -- which also MEASURES the table of bounds the GPU test uses:
    BOUND[act][dir] = max(2^-22, 2 x worst |err| / max(1, |ref|)) of the oracle's float32 formula on the grid.  The committed table
    must lie between the measurement and twice the measurement (or sit on the floor), so it can neither drift loose nor be set by hand.
    The factor 2: each formula makes at most two transcendental calls, whose device versions may differ from NumPy's by 1 - 2 ulp;
(c) the probe builders: the float64 forward of a built network hands the grid back, and the backward factor is far from 0.
"""
import numpy as np
import pytest

from oracle import ppo_oracle as O
from tests import act_probe as P


# torch's float64 backward formulas that lose the tail to cancellation, restated: the test checks that torch's gradient IS this
TORCH_CANCELS = {"tanh": lambda z: 1.0 - np.tanh(z) ** 2,
                 "sigmoid": lambda z: (1.0 / (1.0 + np.exp(-z))) * (1.0 - 1.0 / (1.0 + np.exp(-z)))}


@pytest.mark.parametrize("act", P.ACTS)
def test_closed_forms_match_torch_float64_autograd(act):
    import torch
    mod = {"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU, "elu": torch.nn.ELU, "leakyrelu": torch.nn.LeakyReLU, "sigmoid": torch.nn.Sigmoid,
           "softplus": torch.nn.Softplus, "softsign": torch.nn.Softsign, "hardtanh": torch.nn.Hardtanh, "relu6": torch.nn.ReLU6,
           "silu": torch.nn.SiLU, "gelu": torch.nn.GELU, "mish": torch.nn.Mish}[act]()
    pts = np.concatenate([P.GRID, P.TANH_POS, -P.TANH_POS]) if act == "tanh" else P.GRID
    z = torch.tensor(pts.astype(np.float64), requires_grad=True)
    y = mod(z)
    y.sum().backward()
    for name, got, ref in (("f", P.f(act, pts), y.detach().numpy()), ("df", P.df(act, pts), z.grad.numpy())):
        bad = np.abs(got - ref) > np.maximum(1e-12 * np.abs(ref), 1e-300)
        if name == "df" and act in TORCH_CANCELS and bad.any():
            zb = pts[bad].astype(np.float64)
            cancelling = TORCH_CANCELS[act](zb)
            assert np.all(np.abs(cancelling - ref[bad]) <= 4 * np.finfo(np.float64).eps), (act, "torch is not the cancelling formula", zb[:5])
            assert np.all(np.abs(got[bad] - ref[bad]) <= 4 * np.finfo(np.float64).eps), (act, zb[:5], got[bad][:5], ref[bad][:5])
            print(f"{act}: torch float64 backward cancels at {int(bad.sum())} of {len(pts)} points, first {zb[:3]}")
            bad[:] = False
        assert not bad.any(), (act, name, pts[bad][:5], got[bad][:5], ref[bad][:5])


def oracle_errors(act):
    """Worst |err| / max(1, |ref|) of the oracle's float32 forward and backward on the grid."""
    z = P.GRID
    h = O._activate(z, act)
    one = np.ones_like(z)
    d = O._activation_grad_pre(z, one, act) if act in O.NEEDS_PRE_ACTIVATION else O._activation_grad(h, one, act)
    assert h.dtype == np.float32 and d.dtype == np.float32
    return float(P.err(h, P.f(act, z)).max()), float(P.err(d, P.df(act, z)).max())


@pytest.mark.parametrize("act", P.ACTS)
def test_bound_table_is_the_oracles_measured_error(act):
    fwd, bwd = oracle_errors(act)
    print(f"{act}: measured fwd {fwd / P.FLOOR:.3f} bwd {bwd / P.FLOOR:.3f} (units of 2^-22); BOUND {P.BOUND[act][0] / P.FLOOR:.3f} {P.BOUND[act][1] / P.FLOOR:.3f}")
    for name, measured, bound in (("fwd", fwd, P.BOUND[act][0]), ("bwd", bwd, P.BOUND[act][1])):
        assert bound >= measured, (act, name, measured, bound)
        assert bound == P.FLOOR or measured <= bound <= 2.0 * measured, (act, name, measured, bound)
        assert (bound == P.FLOOR) == (2.0 * measured <= P.FLOOR), (act, name, measured, bound)


def test_softplus_backward_keeps_its_relative_precision_in_the_left_tail():
    """The corrected formula, -expm1(-h): relative error on the probe points in [-80, -5] (the cancelling form returned exactly 0 from
    z = -17 on).  The GPU test's relative bound is twice this measurement, floor 4 ulp."""
    z = P.SOFTPLUS_TAIL
    assert len(z) >= 20 and z.min() <= -60 and z.max() <= -5
    d = O._activation_grad(O._activate(z, "softplus"), np.ones_like(z), "softplus")
    ref = P.df("softplus", z)
    rel = float(np.max(np.abs(d - ref) / ref))
    print(f"softplus backward, -80 <= z <= -5: worst relative error {rel:.3e} = {rel * 2 ** 23:.2f} ulp; bound {P.SOFTPLUS_REL:.3e}")
    assert np.all(d > 0)
    assert 0.8 <= rel / P.SOFTPLUS_REL_MEASURED <= 1.25, (rel, P.SOFTPLUS_REL_MEASURED)
    assert P.SOFTPLUS_REL == max(4 * 2.0 ** -23, 2.0 * P.SOFTPLUS_REL_MEASURED)


@pytest.mark.parametrize("act", ["tanh", "softplus", "relu6", "gelu"])
def test_layer1_builder_hands_the_grid_back(act):
    D, A, wpi, wvf, N = 9, 8, 72, 40, 64
    n_pass = -(-len(P.GRID) // N)
    seen_pi, seen_vf = set(), set()
    for k in range(n_pass):
        p, obs, units, uv = P.layer1_forward(D, A, wpi, wvf, P.GRID, N, k)
        mean, value, zpi, zvf = P.forward64(p, obs, act)
        assert np.array_equal(zpi[:, units], obs[:, [u % D for u in units]]) and np.array_equal(zvf[:, uv], obs[:, uv % D])
        assert np.array_equal(mean, P.f(act, zpi[:, units])) and np.array_equal(value, P.f(act, zvf[:, uv]))
        seen_pi |= set(zpi[:, units].ravel().tolist())
        seen_vf |= set(zvf[:, uv].tolist())
    assert seen_pi == seen_vf == set(P.GRID.astype(np.float64).tolist())
    assert max(units) == wpi - 1 and 31 in units and 32 in units


@pytest.mark.parametrize("act", ["elu", "sigmoid", "mish"])
def test_layer2_bias_builder_lands_near_the_grid(act):
    D, A, pi, vf = 9, 20, (72, 40), (40, 24)
    n = len(P.GRID)
    seen_pi, seen_pi_all, seen_vf_all = set(), set(), set()
    for k in range(-(-n // A)):
        p, units, uv = P.layer2_bias(D, A, pi, vf, P.GRID, k, act)
        mean, value, zpi, zvf = P.forward64(p, np.zeros((4, D), np.float32), act)
        want = P.GRID[(A * k + np.arange(A)) % n]
        assert np.max(np.abs(zpi[0, units] - want)) <= 2.0 ** -8 * abs(float(P.f(act, 0.0))) + 1e-12
        assert abs(zvf[0, uv] - want[0]) <= 2.0 ** -8 * abs(float(P.f(act, 0.0))) + 1e-12
        assert np.array_equal(mean[0], P.f(act, zpi[0, units])) and value[0] == P.f(act, zvf[0, uv])
        seen_pi |= set(want.tolist())
    assert seen_pi == set(P.GRID.tolist())
    for k in range(-(-n // 24)):
        p, _, _ = P.layer2_bias(D, 2, pi, vf, P.GRID, k, act, heads="uniform")
        seen_pi_all |= set(p[P.PI + ".2.bias"].tolist())
        seen_vf_all |= set(p[P.VF + ".2.bias"].tolist())
    assert seen_pi_all == seen_vf_all == set(P.GRID.tolist())


def test_tanh_selector_builder_and_the_backward_factor():
    H, A = 64, 16
    rows = P.selector_rows()
    seen = set()
    for off in range(0, len(P.TANH_POS), 16):
        p, units, uv = P.tanh_layer2(H, A, P.TANH_POS, off)
        mean, value, zpi, zvf = P.forward64(p, rows, "tanh")
        table = P.tanh_table(H, P.TANH_POS, off).astype(np.float64)
        assert np.array_equal(zpi[:P.NSEL], table.T) and np.array_equal(zpi[P.NSEL:], -table.T) and np.array_equal(zvf, zpi)
        assert np.array_equal(mean, np.tanh(zpi[:, units])) and np.array_equal(value, np.tanh(zvf[:, uv]))
        seen |= set(np.abs(zvf[:, uv]).tolist())
    assert seen == set(P.TANH_POS.astype(np.float64).tolist())       # even the single value unit meets every point
    # backward: identical rows, factor = 1 per action for the policy net and 1 for the value net, up to the rounding of the inputs
    p, _, _ = P.tanh_layer2(H, 2, P.TANH_POS, 0, heads="uniform")
    mb, fpi, fvf, zpi, zvf = P.backward_minibatch(p, rows[3], "tanh", 32)
    assert np.all(np.abs(fpi + 2.0) < 1e-5) and np.all(np.abs(fvf - 1.0) < 1e-5), (fpi[:3], fvf[:3])
    assert np.array_equal(zpi, P.tanh_table(H, P.TANH_POS, 0)[:, 3].astype(np.float64))
    assert np.all(np.abs(mb["actions"] - 0.5) < 2.0 ** -8) and np.all(mb["returns"] <= mb["values"]) and mb["returns"][0] < mb["values"][0] - 1
    ro = P.as_rollout(mb, 8, 4)
    assert ro["obs"].shape == (8, 4, P.NSEL) and ro["actions"].shape == (8, 4, 2)
