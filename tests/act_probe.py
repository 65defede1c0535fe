"""Per-unit activation probes: float64 closed forms of the twelve hidden activations and their derivatives, a grid of pre-activations
that sits on the tails and kinks, and builders of networks whose heads hand single hidden units back.

Pure NumPy / float64; imports neither the oracle nor the engine, so it is an independent witness for both (tests/test_act_tails_cpu.py
pins the closed forms to torch's float64 autograd).

How a probe works.  A first-layer weight matrix with a single 1.0 per row makes z = obs exactly on every product path (the other
products are 0 * finite).  A head row with a single 1.0 returns one unit's f(z) as an action mean (eps = 0) or as the value.  For
the derivative every row of a minibatch is the same, one of them carries the loss, advantages are not normalised, and the heads weigh
every unit of the last hidden layer alike: the bias gradient of unit j is then f'(z_j) times a factor the float64 reference computes, with no cancellation.
A deeper layer gets its z from its bias (generic chain: the layers in front see zeros) or, for tanh, from a column of W2 that a
saturated first layer (tanh(+-1e30) = +-1, tanh(0) = 0) selects per row.
"""
import math
from collections import OrderedDict

import numpy as np

F32 = np.float32
ACTS = ("tanh", "relu", "elu", "leakyrelu", "sigmoid", "softplus", "softsign", "hardtanh", "relu6", "silu", "gelu", "mish")
KINKED = ("relu", "leakyrelu", "hardtanh", "relu6")     # derivative is one of 0 / 0.01 / 1 everywhere
FLOOR = 2.0 ** -22


def _erf(x):
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _softplus(z):
    """torch Softplus(beta 1, threshold 20): z above 20, log1p(exp(z)) below."""
    return np.where(z > 20.0, z, np.log1p(np.exp(np.minimum(z, 20.0))))


def f(act, z):
    """f(z) in float64 with torch.nn's default arguments."""
    z = np.asarray(z, np.float64)
    if act == "tanh":
        return np.tanh(z)
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "elu":
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))
    if act == "leakyrelu":
        return np.where(z > 0, z, 0.01 * z)
    if act == "sigmoid":
        return _sigmoid(z)
    if act == "softplus":
        return _softplus(z)
    if act == "softsign":
        return z / (1.0 + np.abs(z))
    if act == "hardtanh":
        return np.clip(z, -1.0, 1.0)
    if act == "relu6":
        return np.clip(z, 0.0, 6.0)
    if act == "silu":
        return z * _sigmoid(z)
    if act == "gelu":
        return 0.5 * z * (1.0 + _erf(z / math.sqrt(2.0)))
    if act == "mish":
        return z * np.tanh(_softplus(z))
    raise ValueError(act)


def df(act, z):
    """f'(z) in float64 with torch's sub-gradient conventions at the kinks (relu 0 at 0; leaky slope at z <= 0; hardtanh / relu6 0 at
    the clamp points; softplus 1 above its threshold)."""
    z = np.asarray(z, np.float64)
    if act == "tanh":
        return 1.0 / np.cosh(np.minimum(np.abs(z), 350.0)) ** 2
    if act == "relu":
        return (z > 0).astype(np.float64)
    if act == "elu":
        return np.where(z > 0, 1.0, np.exp(np.minimum(z, 0.0)))
    if act == "leakyrelu":
        return np.where(z > 0, 1.0, 0.01)
    if act == "sigmoid":
        s = _sigmoid(z)
        return s * _sigmoid(-z)
    if act == "softplus":
        return np.where(z > 20.0, 1.0, _sigmoid(z))
    if act == "softsign":
        return 1.0 / (1.0 + np.abs(z)) ** 2
    if act == "hardtanh":
        return ((z > -1.0) & (z < 1.0)).astype(np.float64)
    if act == "relu6":
        return ((z > 0.0) & (z < 6.0)).astype(np.float64)
    if act == "silu":
        s = _sigmoid(z)
        return s * (1.0 + z * _sigmoid(-z))
    if act == "gelu":
        return 0.5 * (1.0 + _erf(z / math.sqrt(2.0))) + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    if act == "mish":
        sp = _softplus(z)
        t = np.tanh(sp)
        dsp = np.where(z > 20.0, 1.0, _sigmoid(z))
        return t + z * dsp / np.cosh(np.minimum(sp, 350.0)) ** 2
    raise ValueError(act)


def _grid():
    pos = [0.0, 1e-30, 1e-8, 1e-4, 1e-3, 0.01, 0.1, 0.5, 0.999, 1.0, 1.001, 2.0, 3.0, 5.0, 5.999, 6.0, 6.001]
    pos += [float(v) for v in range(8, 20)] + [19.999, 20.0, 20.001, 25.0, 40.0, 60.0, 87.0, 89.0, 100.0]
    pts = [F32(s * v) for v in pos for s in (1.0, -1.0)]
    pts += [F32(v) for v in np.linspace(-30.0, 30.0, 97)]
    for k in (0.0, 1.0, -1.0, 6.0, 20.0, -20.0):      # one float32 either side of every kink and threshold
        pts += [np.nextafter(F32(k), F32(np.inf)), np.nextafter(F32(k), F32(-np.inf))]
    return np.unique(np.array(pts, F32))     # 173 points: the listed and the linear ones share 0, +-5, +-10 .. +-25 and more, and -0 == 0


GRID = _grid()                                        # the generic chain's probe points (|z| <= 100)
# the tanh families also take the far tail: saturation must be exact and nothing may turn into a NaN
TANH_POS = np.unique(np.concatenate([np.abs(GRID), np.array([21.0, 30.0, 50.0, 1e3, 1e6, 1e10, 1e20, 1e30], F32)])).astype(F32)


def err(got, ref):
    """|got - ref| / max(1, |ref|) per element: the measure BOUND is stated in."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


# ------------------------------------------------------------------------------------------------
# parameters (SB3 state-dict keys and order) and a float64 forward of the same float32 numbers
# ------------------------------------------------------------------------------------------------
PI, VF = "mlp_extractor.policy_net", "mlp_extractor.value_net"


def zero_params(D, A, pi, vf):
    p = OrderedDict()
    p["log_std"] = np.zeros(A, F32)
    for prefix, widths in ((PI, pi), (VF, vf)):
        last = D
        for i, w in enumerate(widths):
            p[f"{prefix}.{2 * i}.weight"] = np.zeros((w, last), F32)
            p[f"{prefix}.{2 * i}.bias"] = np.zeros(w, F32)
            last = w
    p["action_net.weight"], p["action_net.bias"] = np.zeros((A, pi[-1]), F32), np.zeros(A, F32)
    p["value_net.weight"], p["value_net.bias"] = np.zeros((1, vf[-1]), F32), np.zeros(1, F32)
    return p


def forward64(p, obs, act):
    """-> (mean [N, A], value [N], last-layer pre-activations of the policy net [N, w], of the value net), all float64."""
    out = {}
    for prefix in (PI, VF):
        x = np.asarray(obs, np.float64)
        i = 0
        while f"{prefix}.{2 * i}.weight" in p:
            w, b = p[f"{prefix}.{2 * i}.weight"].astype(np.float64), p[f"{prefix}.{2 * i}.bias"].astype(np.float64)
            z = x @ w.T + b
            x = f(act, z)
            i += 1
        out[prefix] = (x, z)
    mean = out[PI][0] @ p["action_net.weight"].astype(np.float64).T + p["action_net.bias"]
    value = (out[VF][0] @ p["value_net.weight"].astype(np.float64).T + p["value_net.bias"])[:, 0]
    return mean, value, out[PI][1], out[VF][1]


def select(w, rows, cols):
    """One 1.0 per row: unit u reads input column u % cols."""
    for u in range(rows):
        w[u, u % cols] = 1.0
    return w


def spread_units(width, k):
    """k distinct units over the width: the first, the last, and both sides of every 32-lane fragment edge first."""
    first = [0, width - 1] + [u for e in range(32, width, 32) for u in (e - 1, e)]
    rest = [int(u) for u in np.linspace(1, width - 2, 4 * k).round()]
    out = []
    for u in first + rest:
        if 0 <= u < width and u not in out:
            out.append(u)
    assert len(out) >= k, (width, k)
    return out[:k]


def one_hot_heads(p, units_pi, unit_vf):
    p["action_net.weight"][:] = 0
    p["value_net.weight"][:] = 0
    for a, u in enumerate(units_pi):
        p["action_net.weight"][a, u] = 1.0
    p["value_net.weight"][0, unit_vf] = 1.0
    return p


HEAD_W = 2.0 ** -21      # uniform head weights of the backward probes: the means stay below 2^-8, far under sigma / 2 and the return gap


def uniform_heads(p):
    p["action_net.weight"][:] = HEAD_W
    p["value_net.weight"][:] = HEAD_W
    return p


# ---- layer 1 -------------------------------------------------------------------------------------
def layer1_forward(D, A, wpi, wvf, pts, n_rows, p_idx):
    """One hidden layer per network, z = obs.  Pass p_idx of ceil(len(pts) / n_rows): the rows walk through the points, so that
    over the passes every unit behind a head has seen all of them.  -> (params, obs, units_pi, unit_vf)."""
    p = zero_params(D, A, (wpi,), (wvf,))
    select(p[f"{PI}.0.weight"], wpi, D)
    select(p[f"{VF}.0.weight"], wvf, D)
    units = spread_units(wpi, A)
    uv = spread_units(wvf, 8)[p_idx % 8]
    one_hot_heads(p, units, uv)
    r, c = np.meshgrid(np.arange(n_rows), np.arange(D), indexing="ij")
    obs = pts[(p_idx * n_rows + r + 0 * c) % len(pts)].astype(F32)      # row r: one point in every column
    return p, obs, units, uv


def layer1_backward(wpi, wvf, A, pts, k):
    """z = obs with D = wpi observation columns; minibatch k's row.  -> (params, obs row [D])."""
    D = wpi
    p = zero_params(D, A, (wpi,), (wvf,))
    select(p[f"{PI}.0.weight"], wpi, D)
    select(p[f"{VF}.0.weight"], wvf, D)
    uniform_heads(p)
    return p, pts[(wvf * k + np.arange(D)) % len(pts)].astype(F32)


# ---- a deeper layer through its bias (any activation) ----------------------------------------------
def layer2_bias(D, A, pi, vf, pts, k, act, heads="one_hot"):
    """Two hidden layers per network, observations all zero: h1 = f(0), z2 = 2^-8 h1 + b2 with b2 walking through the points.
    One-hot heads (forward): pass k of ceil(len(pts) / A) puts points A k .. A k + A - 1 on the A units behind the action head and the
    first of them on the value head's unit too.  Uniform heads (backward): pass k of ceil(len(pts) / min(pi[1], vf[1])), unit u of
    either network gets point min(..) k + u.  -> (params, units_pi, unit_vf)."""
    p = zero_params(D, A, pi, vf)
    units, uv = spread_units(pi[1], A), spread_units(vf[1], 8)[k % 8]
    stride = A if heads == "one_hot" else min(pi[1], vf[1])
    for prefix, w, first in ((PI, pi, units), (VF, vf, [uv])):
        select(p[f"{prefix}.0.weight"], w[0], D)
        for u in range(w[1]):
            p[f"{prefix}.2.weight"][u, u % w[0]] = 2.0 ** -8
        order = (list(first) + [u for u in range(w[1]) if u not in first]) if heads == "one_hot" else list(range(w[1]))
        p[f"{prefix}.2.bias"][order] = pts[(stride * k + np.arange(w[1])) % len(pts)]
    if heads == "one_hot":
        one_hot_heads(p, units, uv)
    else:
        uniform_heads(p)
    return p, units, uv


# ---- tanh: layer 2 through a column of W2 that a saturated layer 1 selects ------------------------------------
NSEL = 16


def tanh_table(H, pts_pos, off):
    """W2[u, j] for the NSEL selector units j: non-negative point off + NSEL (u % 6) + j.  Six neighbouring units hold 6 NSEL = 96
    consecutive points between them, so one table shows every point to the uniform heads, and six tables (off = 0, NSEL, ..) show
    every point to any single unit."""
    u, j = np.meshgrid(np.arange(H), np.arange(NSEL), indexing="ij")
    return pts_pos[(off + NSEL * (u % 6) + j) % len(pts_pos)].astype(F32)


def tanh_layer2(H, A, pts_pos, off, heads="one_hot"):
    """2 x H tanh networks over NSEL observation columns.  Row `s * e_j * 1e30` (s = +-1) saturates unit j of layer 1 to s and leaves
    the others at tanh(0) = 0, so z2[u] = s * W2[u, j].  -> (params, units_pi, unit_vf)."""
    p = zero_params(NSEL, A, (H, H), (H, H))
    for prefix in (PI, VF):
        for j in range(NSEL):
            p[f"{prefix}.0.weight"][j, j] = 1.0
        p[f"{prefix}.2.weight"][:, :NSEL] = tanh_table(H, pts_pos, off)
    units = spread_units(H, A)
    uv = H - 1
    if heads == "one_hot":
        one_hot_heads(p, units, uv)
    else:
        uniform_heads(p)
    return p, units, uv


def selector_rows(mag=1e30):
    """[2 NSEL, NSEL]: +mag e_j for j < NSEL, then -mag e_j.  (mag = 64 saturates as well -- exp(128) is past float32 -- and keeps
    the first layer's weight gradients, which carry the observation as a factor, finite.)"""
    obs = np.zeros((2 * NSEL, NSEL), F32)
    for j in range(NSEL):
        obs[j, j], obs[NSEL + j, j] = mag, -mag
    return obs


# ---- tanh: layer 2 of the evaluation tiles (k_goal64_tile, k_goal256_tile) through a bias-saturated layer 1 ----------------
# The tiles build their own observations, so no selector row reaches them.  Instead W1 = 0 and b1 = +TILE_B1 make every h1[k] the
# saturated 1, whatever the observation; W2[u, k] = z for ONE k per probed unit u (all else 0, b2 = 0) gives z2[u] = z exactly, through
# the layer-2 MFMA and, on the 256 tile, the register-resident fragment element (u, k); W3[a, u_a] = 1 (b3 = 0) hands tanh(z2[u_a]) back
# as action a -- the head, and the 256 tile's fixed-order sum of four partials, add only zeros.  Layer 1 is the saturated selector here
# and nothing more: this is no per-unit probe of layer 1.
TILE_B1 = 30.0


def tile_points(pts_pos=None):
    """every probe point in both signs (-0.0 included)"""
    pos = TANH_POS if pts_pos is None else pts_pos
    return np.concatenate([pos, -pos]).astype(F32)


def _tile_probe(j, H, pts):
    """probe j -> (unit, k, z): unit j % H, so that any A <= H consecutive probes sit on distinct units; the first H probes show every
    unit a point with |z| >= 20, the next H one with |z| < 1, the rest walk through all points; k = (5 j + 3) % H walks through every
    column of W2 (5 is coprime to H = 64 and 256), so through all four k-quarters l >> 4 of every fragment k-step."""
    big, small = pts[np.abs(pts) >= 20.0], pts[np.abs(pts) < 1.0]
    z = big[j % len(big)] if j < H else small[j % len(small)] if j < 2 * H else pts[(j - 2 * H) % len(pts)]
    return j % H, (5 * j + 3) % H, F32(z)


def tile_launches(A, H, pts_pos=None):
    """launches of A probes each that cover tile_points on top of the two per-unit passes"""
    return -(-(2 * H + len(tile_points(pts_pos))) // A)


def tile_probe(D, A, H, launch, pts_pos=None):
    """-> (params of a 2 x H tanh network over D observation features, units [A], columns k [A], points z [A]) of one launch"""
    assert A <= H
    pts = tile_points(pts_pos)
    p = zero_params(D, A, (H, H), (H, H))
    p[f"{PI}.0.bias"][:] = TILE_B1
    units, ks, zs = [], [], []
    for a in range(A):
        u, k, z = _tile_probe(launch * A + a, H, pts)
        p[f"{PI}.2.weight"][u, k] = z
        p["action_net.weight"][a, u] = 1.0
        units.append(u), ks.append(k), zs.append(z)
    assert len(set(units)) == A
    return p, np.array(units), np.array(ks), np.array(zs, F32)


# ---- the backward probe's minibatch and its float64 factor ------------------------------------------
ADV, RET_GAP = 2.0 ** 22, 1.0
VF_COEF = 2.0 ** 20      # with HEAD_W = 2^-21 and the gap of 1: the value net's factor is 2 * 2^20 * 2^-21 = 1, the policy net's 2^22 * 0.5 * 2^-21 = 1 per action


def backward_minibatch(p, row, act, B, active=0):   # active=None: every row carries the loss (ADV, RET_GAP each)
    """B copies of one observation row: actions at mean + sigma / 2 (sigma = exp(0) = 1), old log-prob = log-prob.  ONE row carries
    the loss -- advantage B * ADV > 0 and return = value - B * RET_GAP -- and the others none (advantage 0, return = value to the
    rounding of the value, 2^-32 of the active row's gap): a float32 sum over B equal terms would round B - 1 times, which is the
    summation's error and not the activation's.  -> (dict of flat [B, ...] float32 arrays, factor_pi [w], factor_vf [w], z_pi [w],
    z_vf [w]): the bias gradient of the last hidden layer's unit j is factor[j] * f'(z[j]) with PPO's loss at vf_coef = VF_COEF, no
    advantage normalisation, ratio inside the clip range."""
    obs = np.repeat(np.asarray(row, F32)[None], B, axis=0)
    mean, value, zpi, zvf = forward64(p, obs, act)
    actions = (mean + 0.5).astype(F32)
    d = actions.astype(np.float64) - mean
    lp = np.sum(-(d * d) / 2.0 - 0.5 * math.log(2.0 * math.pi), axis=1)
    old_lp = lp.astype(F32)
    if active is None:
        adv, gap = np.full(B, ADV), np.full(B, RET_GAP)
    else:
        adv, gap = np.zeros(B), np.zeros(B)
        adv[active], gap[active] = B * ADV, B * RET_GAP
    ret = (value - gap).astype(F32)
    ratio = np.exp(lp - old_lp)
    assert np.all(np.abs(ratio - 1.0) < 1e-3)
    g_mean = (-(adv * ratio) / B)[:, None] * d                                 # d loss / d mean, sigma = 1
    g_val = VF_COEF * 2.0 * (value - ret.astype(np.float64)) / B
    fpi = (g_mean @ p["action_net.weight"].astype(np.float64)).sum(axis=0)
    fvf = (g_val[:, None] @ p["value_net.weight"].astype(np.float64)).sum(axis=0)
    mb = dict(obs=obs, actions=actions, values=value.astype(F32), log_probs=old_lp, advantages=adv.astype(F32), returns=ret,
              rewards=np.zeros(B, F32), episode_starts=np.zeros(B, F32))
    return mb, fpi, fvf, zpi[0], zvf[0]


def as_rollout(flat, T, N):
    """Flat minibatch-ordered arrays [T * N, ...] -> the engine's [T, N, ...] buffers (the flatten is env-major: flat = n * T + t)."""
    return {k: np.ascontiguousarray(np.swapaxes(v.reshape((N, T) + v.shape[1:]), 0, 1)) for k, v in flat.items()}


def hidden_bias_key(prefix, layer):
    return f"{prefix}.{2 * layer}.bias"


# ------------------------------------------------------------------------------------------------
# bounds (measured by tests/test_act_tails_cpu.py, which also holds this table to its own measurement)
# ------------------------------------------------------------------------------------------------
SOFTPLUS_TAIL = GRID[(GRID >= -80.0) & (GRID <= -5.0)]
# (forward, backward) per activation: max(2^-22, ~2 x the oracle's float32 formula's worst |err| / max(1, |ref|) on GRID).  Measured, in
# units of 2^-22: tanh 0.19 / 0.38, elu 0.20 / 0.20, leakyrelu 0.15 / 0.00, sigmoid 0.34 / 0.34, softplus 0.31 / 0.27,
# softsign 0.15 / 0.29, silu 0.32 / 3.12, gelu 0.14 / 0.23, mish 0.37 / 3.43, relu / hardtanh / relu6 0 / 0.  Only the silu and mish
# backwards leave the floor (their formula s (1 + z (1 - s)) cancels near z = -1.28, in torch's float32 as well); they are committed
# at 1.9 x so that an ulp of difference in another NumPy's exp does not push the table out of its [1 x, 2 x] window.
BOUND = {a: (FLOOR, FLOOR) for a in ACTS}
BOUND["silu"] = (FLOOR, 1.9 * 7.447e-07)
BOUND["mish"] = (FLOOR, 1.9 * 8.176e-07)
# softplus backward on SOFTPLUS_TAIL, RELATIVE: the corrected formula -expm1(-h) measures 1.41e-7 (1.18 ulp); twice that is under the floor of 4 ulp
SOFTPLUS_REL_MEASURED = 1.408e-07
SOFTPLUS_REL = max(4 * 2.0 ** -23, 2.0 * SOFTPLUS_REL_MEASURED)
# fast_tanh / fast_tanh_scaled (csrc/kernels_fused.h): the code's own claim, absolute; 1 - h^2 follows with |h| <= 1 and one rounding
TANH_FWD_ABS = 2e-7
TANH_BWD_ABS = 4e-7 + 2.0 ** -23
