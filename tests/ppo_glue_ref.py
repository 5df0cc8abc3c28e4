"""fp64 references, bars and case tables of the PPO glue kernels (csrc/bez_ppo.hip, csrc/bez_ppo_loss.h) for
tests/test_gpu_ppo_glue_envelope.py; tests/test_ppo_glue_ref_cpu.py checks this module against the torch formulation it restates
(bez_isaacgym_amd/ppo/a2c_continuous.py), without a GPU.  numpy only.

Every operation is one function written from the rl_games formulation, with the arithmetic's type as a parameter: `dt=np.float64` is the
reference, `dt=np.float32` the YARDSTICK -- the same statements in numpy float32 on the same inputs (sums added one term after the other).

Bars.  For an output block: 3 x the yardstick's worst error against the reference + 2 ulps (fp32; fp16 for an fp16 output) of the block's
largest |reference| (bar()).  Computed from the reference alone; no typed-in tolerance.  Exact comparison where the arithmetic is exact
(integer-valued data with sums below 2^24, copies, fp16 casts); fp64 sums of fp32 data at rows * 2^-53 * sum |x|; the fp64 running
statistics at 16 * 2^-53 of the largest intermediate of their eight-operation chain (rms_apply_bars()).

Branch boundaries.  The loss and the clamps are piecewise.  A row whose reference lies within the yardstick's bar of a switch
(|ratio - (1 +- e_clip)|, ||v - old_v| - e_clip|, the tie of the two value losses, ||mu| - 1.1|) is left out of the gradient
comparison -- its statistics still count -- and at most 1 % of a case's rows may be (LOSS_EXCLUDE_CAP; the seeds below keep every case
under it, tests/test_ppo_glue_ref_cpu.py asserts that).  elu_bwd's fp16 output: the kernel rounds the product to fp32, then to fp16; an
element whose exact product lies within one fp32 ulp of an fp16 rounding midpoint gets one fp16 ulp, at most 0.1 % of a case's elements
(ELU_MIDPOINT_CAP)."""
import functools
import itertools
import math
import zlib

import numpy as np
import torch

F16, F32, F64 = np.float16, np.float32, np.float64
EPS64 = 2.0 ** -53
FLT_MAX = 3.4028234663852886e38
LOG_2PI = math.log(2.0 * math.pi)
LOSS_EXCLUDE_CAP = 0.01
ELU_MIDPOINT_CAP = 0.001


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def ulp32(x):
    return float(np.spacing(F32(abs(float(x)))))


def ulp16(x):
    return float(np.spacing(F16(abs(float(x)))))


def bar(r64, r32, half=False):
    """3 x the yardstick's worst error + 2 ulps of the block's largest |reference|"""
    r64 = np.asarray(r64, F64)
    top = float(np.abs(r64).max()) if r64.size else 0.0
    return 3.0 * float(np.abs(np.asarray(r32, F64) - r64).max()) + 2.0 * (ulp16(top) if half else ulp32(top))


def _sum(x, axis, dt):
    """fp64: numpy's sum; fp32: one term after the other (the plainest fp32 statement of a sum)"""
    if dt is F32:
        return np.take(np.cumsum(x, axis=axis, dtype=F32), -1, axis=axis)
    return np.sum(x, axis=axis, dtype=F64)


def both(fn, *a, **k):
    """(reference, yardstick) of one operation"""
    return fn(*a, dt=F64, **k), fn(*a, dt=F32, **k)


# ---- running mean / std
def moments(x):
    """([column sums | sums of squares | rows], their fp64 bars) of fp32 data"""
    xd = np.asarray(x, F64)
    rows = xd.shape[0]
    s1, s2 = xd.sum(0), (xd * xd).sum(0)
    b1, b2 = rows * EPS64 * np.abs(xd).sum(0), rows * EPS64 * (xd * xd).sum(0)
    return np.concatenate([s1, s2, [float(rows)]]), np.concatenate([b1, b2, [0.0]])


def rms_apply(mean, var, count, mom):
    """RunningMeanStd.update_from_moments in fp64 (the statistics are fp64 buffers): (mean, var, count)"""
    d = mean.size
    s1, s2, n = mom[:d], mom[d:2 * d], float(mom[2 * d])
    b_mean = s1 / n
    b_var = np.maximum(s2 / n - b_mean * b_mean, 0.0) * (n / max(n - 1.0, 1.0))
    delta, tot = b_mean - mean, count + n
    m2 = var * count + b_var * n + delta * delta * count * n / tot
    return mean + delta * n / tot, m2 / tot, tot


def rms_apply_bars(mean, var, count, mom):
    """the chain has eight fp64 operations, none on a number larger than the ones below (s2 / n - b_mean^2 cancels: its error is relative
    to s2 / n, and the factors behind it, n / (n - 1) * n / tot, are at most 2): 16 x 2^-53 x that"""
    d = mean.size
    n = float(mom[2 * d])
    b_mean = mom[:d] / n
    top_m = max(float(np.abs(b_mean).max()), float(np.abs(mean).max()), 1e-300)
    top_v = max(float((mom[d:2 * d] / n).max()), float(np.abs(var).max()), float(((b_mean - mean) ** 2).max()), 1e-300)
    return 16 * EPS64 * top_m, 16 * EPS64 * top_v


def _sd(var, eps, dt):
    """sqrt(var + eps) on the statistics read as fp32 (running_var.float())"""
    return np.sqrt(np.asarray(var, F64).astype(F32).astype(dt) + dt(F32(eps)))


def normalize(x, mean, var, eps, dt=F64):
    """RunningMeanStd.forward (eval): the fp64 statistics are read as fp32 (.float()), then (x - mean) / sqrt(var + eps), clamp +-5"""
    m = np.asarray(mean, F64).astype(F32).astype(dt)
    with np.errstate(all="ignore"):
        y = (np.asarray(x).astype(dt) - m) / _sd(var, eps, dt)
        return np.clip(y, dt(-5.0), dt(5.0))     # (np.clip keeps a NaN, as torch.clamp does)


def unnormalize(x, mean, var, eps, dt=F64):
    """RunningMeanStd.forward(unnorm=True): sqrt(var + eps) * clamp(x, +-5) + mean"""
    m = np.asarray(mean, F64).astype(F32).astype(dt)
    return _sd(var, eps, dt) * np.clip(np.asarray(x).astype(dt), dt(-5.0), dt(5.0)) + m


# ---- sampling, rollout bookkeeping
def neglogp(x, mean, std, logstd, dt=F64):
    """ModelA2CContinuousLogStd.neglogp"""
    q = (x - mean) / std
    return dt(0.5) * _sum(q * q, -1, dt) + dt(0.5 * LOG_2PI) * dt(x.shape[-1]) + _sum(np.broadcast_to(logstd, x.shape), -1, dt)


def sample(mu, logstd, noise, dt=F64):
    """action = mu + exp(logstd) noise, its clamp to +-1 for the env, sigma, neglogp(action)"""
    mu, logstd, noise = np.asarray(mu).astype(dt), np.asarray(logstd).astype(dt), np.asarray(noise).astype(dt)
    s = np.exp(logstd)
    act = mu + s * noise
    sigma = np.broadcast_to(s, mu.shape).copy()
    return dict(act=act, env_act=np.clip(act, dt(-1.0), dt(1.0)), sigma=sigma, neglogp=neglogp(act, mu, sigma, logstd, dt))


def rollout_post(rew, dones, timeouts, values, reward_scale, gamma, bootstrap, cur_rew, cur_len, dt=F64):
    """_rollout_impl's bookkeeping of one env step; stats = what is ADDED to [episodes, sum of returns, sum of lengths]"""
    rew, values, cur_rew, cur_len = (np.asarray(a).astype(dt).reshape(-1) for a in (rew, values, cur_rew, cur_len))
    d, t = np.asarray(dones).astype(dt), np.asarray(timeouts).astype(dt)
    shaped = rew * dt(F32(reward_scale))
    if bootstrap:
        shaped = shaped + dt(F32(gamma)) * values * t
    cr, cl = cur_rew + rew, cur_len + dt(1.0)
    stats = np.array([d.sum(dtype=F64), (cr * d).sum(dtype=F64), (cl * d).sum(dtype=F64)])
    return dict(shaped=shaped, dones_f=d, cur_rew=cr * (dt(1.0) - d), cur_len=cl * (dt(1.0) - d), stats=stats)


def fold(parts):
    """the per-slot fold: (what is added to ep_stats, the slots afterwards)"""
    p = np.asarray(parts, F64).reshape(-1, 4)
    after = p.copy()
    after[:, :3] = 0.0
    return p[:, :3].sum(0), after


# ---- the PPO loss
def loss(d, cfg, dt=F64):
    """a2c_continuous' loss of one minibatch in closed form: the five statistics as SUMS over the rows, d loss / d mu, d value, d log-sigma
    of loss = mean(a) + 0.5 critic_coef mean(c) - entropy_coef mean(entropy) + bounds_coef mean(b), times the loss scale; torch.max splits
    a tie evenly and clamp passes the gradient on its limits; b_loss is reported as 0 when bounds_coef is 0 (as the agent does).
    `switch`: the quantities whose sign decides a branch."""
    g = lambda k: np.asarray(d[k]).astype(dt)
    mu, logstd, value, act, old_logp, adv = g("mu"), g("logstd"), g("value").reshape(-1), g("actions"), g("old_logp"), g("advantages")
    ov, rt, om, os_ = g("old_values").reshape(-1), g("returns").reshape(-1), g("old_mu"), g("old_sigma")
    e, cc, ec, bc = (dt(F32(cfg[k])) for k in ("e_clip", "critic_coef", "entropy_coef", "bounds_coef"))
    S = dt(F32(cfg["scale"])) if cfg["scale"] is not None else dt(1.0)
    B, A = mu.shape
    one, half, two = dt(1.0), dt(0.5), dt(2.0)
    s = np.exp(logstd)
    z = (act - mu) / s
    nlp = half * _sum(z * z, 1, dt) + dt(0.5 * LOG_2PI) * dt(A) + _sum(logstd, 0, dt)
    ent_row = _sum(half + dt(0.5 * LOG_2PI) + logstd, 0, dt)
    ratio = np.exp(old_logp - nlp)
    lo_r, hi_r = one - e, one + e
    rc = np.clip(ratio, lo_r, hi_r)
    l1, l2 = -adv * ratio, -adv * rc
    a_l = np.maximum(l1, l2)
    through = np.where((ratio >= lo_r) & (ratio <= hi_r), -adv, dt(0.0))      # d l2 / d ratio
    g_ratio = np.where(l1 > l2, -adv, np.where(l1 < l2, through, half * (-adv) + half * through))
    g_nlp = -ratio * g_ratio
    if cfg["clip_value"]:
        dv = value - ov
        vc = ov + np.clip(dv, -e, e)
        q1, q2 = (value - rt) ** 2, (vc - rt) ** 2
        c_l = np.maximum(q1, q2)
        g1 = two * (value - rt)
        g2 = np.where((dv >= -e) & (dv <= e), two * (vc - rt), dt(0.0))
        g_v = np.where(q1 > q2, g1, np.where(q1 < q2, g2, half * (g1 + g2)))
        sw_v = [np.abs(dv) - e, q1 - q2]
    else:
        c_l = (rt - value) ** 2
        g_v = two * (value - rt)
        sw_v = []
    soft = dt(1.1)
    hi, lo = np.maximum(mu - soft, dt(0.0)), np.minimum(mu + soft, dt(0.0))
    b_l = _sum(hi * hi + lo * lo, 1, dt) if bc > 0 else np.zeros(B, dt)
    dm = om - mu
    kl = _sum(np.log(os_ / s + dt(1e-5)) + (s * s + dm * dm) / (two * (os_ * os_ + dt(1e-5))) - half, 1, dt)
    invB = one / dt(B)
    g_b = bc * two * (hi + lo) if bc > 0 else np.zeros_like(mu)
    gmu = (g_nlp[:, None] * (-z / s) + g_b) * invB * S
    glog_rows = (g_nlp[:, None] * (one - z * z) - ec) * invB * S
    gval = half * cc * g_v * invB * S
    stats = np.array([_sum(a_l, 0, dt), _sum(c_l, 0, dt), _sum(b_l, 0, dt), _sum(kl, 0, dt), ent_row * dt(B)])
    jump = np.abs(ratio * adv)[:, None] * np.abs(one - z * z) * invB * S      # what a row's d / d log-sigma changes by across a ratio switch
    return dict(stats=stats, gmu=gmu, gval=gval, glog=_sum(glog_rows, 0, dt), glog_jump=jump, ratio=ratio, a_rows=a_l, c_rows=c_l, g_ratio=g_ratio, g_v=g_v,
                switch_pi=[ratio - lo_r, ratio - hi_r] + ([np.abs(mu) - soft] if bc > 0 else []), switch_v=sw_v,
                new_sigma=np.broadcast_to(s, mu.shape).copy())


def loss_excluded(r64, r32, adv):
    """(rows left out of the gmu / glog comparison, rows left out of the gval comparison): a switch quantity within its own bar of 0 (an exact
    0 is a tie or a limit that both precisions see alike, and stays in); a ratio switch does not matter where the advantage is 0"""
    def near(q64, q32):
        b = bar(q64, q32)
        m = (np.abs(q64) <= b) & (q64 != 0.0)
        return m if m.ndim == 1 else m.any(1)
    n = r64["gval"].shape[0]
    pi, v = np.zeros(n, bool), np.zeros(n, bool)
    for k, (a, b) in enumerate(zip(r64["switch_pi"], r32["switch_pi"])):
        pi |= near(a, b) & ((np.asarray(adv) != 0) | (k >= 2))
    for a, b in zip(r64["switch_v"], r32["switch_v"]):
        v |= near(a, b)
    return pi, v


LOSS_KEYS = ("mu", "logstd", "value", "actions", "old_logp", "advantages", "old_values", "returns", "old_mu", "old_sigma")
PLANTS = ("clip_hi_adv+", "clip_hi_adv-", "clip_lo_adv+", "clip_lo_adv-", "adv0", "dv_above", "dv_below", "dv_zero", "mu_above", "mu_below", "value_tie")


def loss_cfg(idx):
    """the switches of loss case idx, cycling with periods of 2 to 7 (tests/test_ppo_glue_ref_cpu.py holds that each value of each is met)"""
    return dict(clip_value=idx % 2 == 0, bounds_coef=0.5 if (idx // 2) % 2 == 0 else 0.0, entropy_coef=0.01 if idx % 3 == 0 else 0.0,
                scale=1024.0 if idx % 5 < 3 else None, e_clip=0.25 if idx % 4 < 2 else 0.2, critic_coef=2.0, accumulate=idx % 3 == 1,
                update_mu_sigma=idx % 7 == 0)


def loss_cases():
    """(rows, width, index): every template width at 65 rows (a full tile and a one-row tile); six widths at 1, 63, 64 and 130 rows"""
    c = [(65, a) for a in range(1, 33)] + [(n, a) for a in (1, 4, 5, 18, 31, 32) for n in (1, 63, 64, 130)]
    return [(n, a, i) for i, (n, a) in enumerate(c)]


def loss_data(n, a, idx):
    """fp32 inputs of a loss case: random rows, with the designed rows planted among them (as many of PLANTS as there are rows).
    Returns (inputs, cfg, {plant: row})."""
    rng = np.random.default_rng(seed_of("loss", n, a, idx))
    cfg = loss_cfg(idx)
    e = float(F32(cfg["e_clip"]))
    f = lambda x: np.ascontiguousarray(x, F32)
    mu, logstd = f(rng.normal(size=(n, a)) * 0.8), f(rng.normal(size=a) * 0.3 - 1.0)
    old_sigma = f(np.broadcast_to(np.exp(logstd.astype(F64) + 0.05 * rng.normal(size=a)), (n, a)))
    old_mu = f(mu + 0.05 * rng.normal(size=(n, a)))
    act = f(old_mu + old_sigma * rng.normal(size=(n, a)))
    value, ov, rt, adv = f(rng.normal(size=n)), f(rng.normal(size=n)), f(rng.normal(size=n)), f(rng.normal(size=n))
    adv[adv == 0] = 1.0
    rows = {}
    order = rng.permutation(n)
    for p, r in zip(PLANTS, order):
        rows[p] = int(r)
    target = np.exp(0.3 * rng.normal(size=n))           # the ratio each row is given
    for p, t in (("clip_hi_adv+", 1.5), ("clip_hi_adv-", 1.5), ("clip_lo_adv+", 0.5), ("clip_lo_adv-", 0.5)):
        if p in rows:
            target[rows[p]] = t
            adv[rows[p]] = 1.0 if p.endswith("+") else -1.0
    if "adv0" in rows:
        adv[rows["adv0"]] = 0.0
    for p, dv in (("dv_above", 0.5), ("dv_below", -0.5), ("dv_zero", 0.0)):
        if p in rows:
            ov[rows[p]] = 0.25
            value[rows[p]] = 0.25 + dv
    # |mu| beyond 1.1: the action and the old mean move with the mean, as in a rollout -- the action stays a draw around mu.  (Left where they
    # were, (action - mu) / sigma is about -12 and neglogp about 72: exp() then turns every fp32 ulp of neglogp, 7.6e-6, into that much RELATIVE
    # error of the ratio, in the yardstick and in any kernel alike, and the one row decides the whole block's bar by a single draw.)
    for p, c, to in (("mu_above", 0, 1.5), ("mu_below", a - 1, -1.75)):
        if p in rows:
            r = rows[p]
            shift = F32(to) - mu[r, c]
            mu[r, c], old_mu[r, c], act[r, c] = to, old_mu[r, c] + shift, act[r, c] + shift
    if "value_tie" in rows and e == 0.25:   # v - old_v = 0.75 > e_clip: the clipped value 0.25 and v = 0.75 are equally far from the return 0.5
        r = rows["value_tie"]
        ov[r], value[r], rt[r] = 0.0, 0.75, 0.5
    else:
        rows.pop("value_tie", None)
    d = dict(mu=mu, logstd=logstd, value=value, actions=act, advantages=adv, old_values=ov, returns=rt, old_mu=old_mu, old_sigma=old_sigma)
    s = np.exp(logstd.astype(F64))
    zz = (act.astype(F64) - mu.astype(F64)) / s
    nlp = 0.5 * (zz * zz).sum(1) + 0.5 * LOG_2PI * a + logstd.astype(F64).sum()
    d["old_logp"] = f(nlp + np.log(target))
    return d, cfg, rows


@functools.lru_cache(maxsize=None)
def loss_ref(n, a, idx):
    """(inputs, cfg, planted rows, reference, bars per block, rows kept for gmu / glog, rows kept for gval) of a loss case, computed once"""
    d, cfg, rows = loss_data(n, a, idx)
    r64, r32 = both(loss, d, cfg)
    ex_pi, ex_v = loss_excluded(r64, r32, d["advantages"])
    kp, kv = ~ex_pi, ~ex_v
    bars = dict(stats=bar(r64["stats"], r32["stats"]), gmu=bar(r64["gmu"][kp], r32["gmu"][kp]), gval=bar(r64["gval"][kv], r32["gval"][kv]),
                glog=bar(r64["glog"], r32["glog"]) + float(r64["glog_jump"][ex_pi].sum(0).max() if ex_pi.any() else 0.0),
                new_sigma=bar(r64["new_sigma"], r32["new_sigma"]))
    return d, cfg, rows, r64, bars, kp, kv


# ---- gradient reductions of the fp16 linear layers
def wgrad_sum(part, base=None, dt=F64):
    """sum over the splits of fp16 partial products (S, n), added to `base`"""
    s = _sum(np.asarray(part, F16).astype(dt), 0, dt)
    return s if base is None else s + np.asarray(base).astype(dt)


def colsum(y, base=None, dt=F64):
    s = _sum(np.asarray(y).astype(dt), 0, dt)
    return s if base is None else s + np.asarray(base).astype(dt)


def elu_bwd(gy, y):
    """gz = gy elu'(y) from the ELU's output (alpha 1: y > 0 ? 1 : y + 1) as an fp16 number: (gz, elements within one fp32 ulp of an fp16
    rounding midpoint).  y + 1 is exact in fp32 (a multiple of 2^-24 in [0, 1]) and the product of an 11-bit and a 24-bit number is exact
    in fp64, so the only freedom is fp32-then-fp16 against fp16 directly."""
    g, v = np.asarray(gy, F16).astype(F64), np.asarray(y, F16).astype(F64)
    p = g * np.where(v > 0, 1.0, v + 1.0)
    h = p.astype(F16)
    with np.errstate(all="ignore"):
        toward = np.where(p > h.astype(F64), np.inf, -np.inf).astype(F16)
        mid = 0.5 * (h.astype(F64) + np.nextafter(h, toward).astype(F64))
        near = (p != h.astype(F64)) & (np.abs(p - mid) <= np.spacing(np.abs(p).astype(F32)).astype(F64))
    return h, near


def head_grads(gmu, gval):
    """the fp16 casts of d loss / d mu, d loss / d value (exact roundings)"""
    return np.asarray(gmu, F32).astype(F16), np.asarray(gval, F32).astype(F16).reshape(-1)


# ---- GAE
def gae(rew, val, mb_dones, dones, last_values, gamma, tau, unnorm=None, dt=F64):
    """a2c_common.discount_values on (H, N) arrays; unnorm = (mean, var, eps): the bootstrap values are de-normalised first.
    Returns (advantages, returns = advantages + values)."""
    rew, val, mbd = (np.asarray(a).astype(dt) for a in (rew, val, mb_dones))
    nv = np.asarray(last_values).astype(dt).reshape(-1)
    if unnorm is not None:
        nv = unnormalize(nv, *unnorm, dt=dt)
    g, t_ = dt(F32(gamma)), dt(F32(tau))
    nnt = dt(1.0) - np.asarray(dones).astype(dt).reshape(-1)
    H = rew.shape[0]
    advs, last = np.zeros_like(rew), np.zeros_like(nv)
    for t in reversed(range(H)):
        delta = rew[t] + g * nv * nnt - val[t]
        last = delta + g * t_ * nnt * last
        advs[t] = last
        nnt, nv = dt(1.0) - mbd[t], val[t]
    return advs, advs + val


# ---- prepare_dataset
def dataset_prep(values, returns, vrms, normalize_adv, dt=F64):
    """a2c_continuous.prepare_dataset behind GAE: the value normaliser absorbs the values' moments, normalises the values, absorbs the returns'
    moments, normalises the returns (its statistics stay fp64 in either precision); both transposed (H, N) -> env-major; advantage =
    return - value, normalised with torch's unbiased std.  vrms = (mean, var, count, eps) or None.
    Returns dict(old_values, returns, advantages, vrms=(mean, var, count) afterwards, val_mom, ret_mom)."""
    v = np.asarray(values, F32).T.reshape(-1)
    r = np.asarray(returns, F32).T.reshape(-1)
    val_mom, _ = moments(v.reshape(-1, 1))
    ret_mom, _ = moments(r.reshape(-1, 1))
    v, r = v.astype(dt), r.astype(dt)
    after = None
    if vrms is not None:
        m, var, cnt, eps = vrms
        s = rms_apply(np.array([m], F64), np.array([var], F64), float(cnt), val_mom)
        v = normalize(v, s[0], s[1], eps, dt)
        s = rms_apply(s[0], s[1], s[2], ret_mom)
        r = normalize(r, s[0], s[1], eps, dt)
        after = (float(s[0][0]), float(s[1][0]), float(s[2]))
    adv = r - v
    if normalize_adv:
        n = adv.size
        mean = _sum(adv, 0, dt) / dt(n)
        c = adv - mean
        std = np.sqrt(_sum(c * c, 0, dt) / dt(max(n - 1, 1)))
        adv = c / (std + dt(1e-8))
    return dict(old_values=v, returns=r, advantages=adv, vrms=after, val_mom=val_mom, ret_mom=ret_mom)


def prep_scratch_doubles(h, n, mbrows, nmb):
    """what bez_ppo_dataset_prep asks of its scratch (include/bez_sim.h): (tasks) x workgroups x 128 + 2 per 256 rows"""
    maxrows = max(h * n // 64, mbrows if nmb > 0 else 0)
    g = min((maxrows + 127) // 128, 256)
    return (nmb + 2) * g * 128 + 2 * ((h * n + 255) // 256)


# (H, N, minibatches, observations, minibatch rows, value normaliser, normalise advantages, constant advantages)
PREP_CASES = [
    (1, 64, 0, 1, 1, False, True, False), (1, 64, 1, 1, 1, True, True, False), (1, 64, 8, 64, 3, True, False, False),
    (64, 1, 1, 64, 4, False, True, False), (64, 1, 8, 1, 5, True, True, False), (64, 1, 0, 64, 129, True, True, False),
    (2, 32, 8, 64, 1, True, True, False), (2, 32, 1, 1, 129, False, False, False), (2, 32, 1, 64, 3, False, True, True),
    (3, 64, 8, 1, 4, True, True, False), (3, 64, 1, 64, 5, False, True, False), (3, 64, 0, 1, 1, False, False, True),
    (5, 320, 8, 64, 129, True, True, False), (5, 320, 1, 1, 3, True, False, False), (5, 320, 8, 1, 4, False, True, False),
    (5, 320, 1, 64, 1, True, True, False), (5, 320, 8, 64, 5, False, True, True),
]
# (what, H, N, minibatches, observations, scratch shortfall, code)
PREP_REFUSED = [("rows", 5, 20, 1, 1, 0, -3), ("minibatches", 1, 64, 9, 1, 0, -1), ("observations", 1, 64, 1, 65, 0, -1), ("scratch", 1, 64, 1, 1, 1, -1)]


def prep_data(case):
    h, n, nmb, d, mbrows, norm_v, norm_a, const = case
    rng = np.random.default_rng(seed_of("prep", *case))
    values = (rng.normal(size=(h, n)) * 3.0 + 1.0).astype(F32)
    returns = (values + 0.5).astype(F32) if const else (rng.normal(size=(h, n)) * 3.0 + 2.0).astype(F32)
    if const:      # dyadic values: return - value is 0.5 exactly in every row
        values = np.round(values * 4) / 4
        values, returns = values.astype(F32), (values + 0.5).astype(F32)
    obs = (rng.normal(size=(max(nmb, 1) * mbrows, d)) + 100.0).astype(F32)
    vrms = (0.3, 2.5, 7.0, 1e-5) if norm_v else None
    return values, returns, obs, vrms


# ---- gradient norm, optimiser step
def norm_parts(g):
    """bez_ppo_grad_norm_parts' shares: workgroup b owns units [1024 b, 1024 (b + 1)); a unit = a float4 of the gradient, then one unit for
    each of the last n % 4 elements -- so a workgroup's elements are one contiguous range.  Returns (sum g^2 per workgroup in fp64, the same
    added in fp32 one term after the other, non-finite count per workgroup); a non-finite element counts and adds nothing."""
    g = np.asarray(g, F32)
    n = g.size
    n4, tail = n // 4, n % 4
    nb = (n4 + tail + 1023) // 1024
    owner = np.concatenate([np.repeat(np.arange(n4), 4), n4 + np.arange(tail)]) // 1024
    starts = np.searchsorted(owner, np.arange(nb + 1))
    fin = np.isfinite(g)
    with np.errstate(all="ignore"):
        clean = np.where(fin, g, F32(0.0))
        pad = np.zeros((nb, 4096), F32)
        for b in range(nb):
            pad[b, :starts[b + 1] - starts[b]] = clean[starts[b]:starts[b + 1]]
        s64 = (pad.astype(F64) ** 2).sum(1)
        s32 = np.cumsum(pad * pad, axis=1, dtype=F32)[:, -1].astype(F64)
    return s64, s32, np.bincount(owner, ~fin, nb)


def adam(st, g, hp, dt=F64):
    """GradScaler.unscale_ + clip_grad_norm_ + torch.optim.Adam (L2 weight decay, no amsgrad) + GradScaler.update + the step counters, the
    tail sums and AdaptiveScheduler's rule, on flat buffers.  st: p, m, v, step, lr, scale (None: no loss scaling), tracker.
    hp: betas, eps, weight_decay, max_norm, grad_div, growth, backoff, interval, tail [(dst, src, scale)], adapt (kl, thr, min, max) or None,
    overflow_skips (the share / meeting-point norm modes skip a step whose squared norm exceeds fp32; the in-launch mode clips it to
    nothing, as torch does).  Returns the new state (skipped: True / False)."""
    p, m, v, gg = (np.asarray(a).astype(dt) for a in (st["p"], st["m"], st["v"], g))
    scale = st["scale"]
    sc = dt(F32(scale)) if scale is not None else dt(1.0)
    div = dt(F32(hp["grad_div"]))
    b1, b2, eps, wd, mx = (dt(F32(hp[k])) for k in ("beta1", "beta2", "eps", "weight_decay", "max_norm"))
    lr, step = dt(F32(st["lr"])), dt(F32(st["step"]))
    with np.errstate(all="ignore"):
        inv = dt(1.0) / (sc * div if div > 1 else sc)
        u = gg * inv
        bad = int((~np.isfinite(u)).sum())
        norm2 = float(_sum(np.where(np.isfinite(u), u, 0) ** 2, 0, dt))
        over = norm2 > FLT_MAX
        if over and hp.get("overflow_skips"):
            bad += 1
        skip = scale is not None and bad > 0
        out = dict(st)
        out["skipped"] = skip
        out["norm"] = math.sqrt(norm2)
        if not skip:
            coef = dt(0.0) if (over and mx > 0) else (min(mx / (np.sqrt(dt(norm2)) + dt(1e-6)), dt(1.0)) if mx > 0 else dt(1.0))
            t = step + dt(1.0)
            bc1, bc2 = dt(1.0) - b1 ** t, dt(1.0) - b2 ** t
            x = u * coef
            if wd != 0:
                x = x + wd * p
            m = b1 * m + (dt(1.0) - b1) * x
            v = b2 * v + (dt(1.0) - b2) * x * x
            p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
            out.update(p=p, m=m, v=v, step=float(t))
        if scale is not None:
            if skip:
                out.update(scale=float(sc * dt(F32(hp["backoff"]))), tracker=0)
            elif st["tracker"] + 1 == hp["interval"]:
                out.update(scale=float(sc * dt(F32(hp["growth"]))), tracker=0)
            else:
                out["tracker"] = st["tracker"] + 1
    out["tail"] = [dt(F32(dst)) + dt(F32(src)) * dt(F32(a)) for dst, src, a in hp.get("tail", [])]
    if hp.get("adapt") is not None:
        out["lr"] = float(adaptive_lr(st["lr"], *hp["adapt"], dt=dt))
    return out


def adaptive_lr(lr, kl, thr, min_lr, max_lr, dt=F64):
    """AdaptiveScheduler.update"""
    lr, kl, thr = dt(F32(lr)), dt(F32(kl)), dt(F32(thr))
    if kl > dt(2.0) * thr:
        lr = max(lr / dt(1.5), dt(F32(min_lr)))
    if kl < dt(0.5) * thr:
        lr = min(lr * dt(1.5), dt(F32(max_lr)))
    return lr


ADAM_N = (1, 2, 3, 4, 5, 4 * 1023 + 3, 4097, 16383, 16385, 524288, 524289, 524288 + 3 * 1024 + 1)
ADAM_MODES = ("launch", "shares", "grid")


def adam_hp(idx):
    """the optimiser's switches of case idx = 3 k + j (k: the place of n in ADAM_N, j: the norm mode).  max_norm and the tail sums turn with
    k + j, so each of their values meets every norm mode (four of the twelve n each); the others with idx, whose residues mod 2, 4 and 5 run
    through every mode as k does"""
    k, j = divmod(idx, 3)
    return dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01 if idx % 2 else 0.0, max_norm=0.0 if (k + j) % 3 == 2 else 1.0,
                grad_div=2.0 if idx % 4 == 1 else 1.0, growth=2.0, backoff=0.5, interval=2 if idx % 5 == 0 else 2000, nsteps=64 if idx % 2 else 1,
                ntail=4 if (k + j) % 3 == 0 else 0)


def adam_bad_positions(n):
    """where a skipped step's inf / NaN is planted, one launch each: the first element, the last (for n % 4 != 0 one of the norm pass's tail
    elements), the middle, and for n > 2 x 256 x 1024 an element that only the capped grid's loop reaches"""
    pos = [0, n - 1, n // 2]
    if n > 524288 + 1:
        pos.append(524288 + (n - 524288) // 2)
    return sorted(set(pos))


def adam_cases():
    return [(n, mode, i * 3 + j) for i, n in enumerate(ADAM_N) for j, mode in enumerate(ADAM_MODES)]


def adam_data(n, idx):
    """(p, g, m, v) of a case: a (loss-scaled) gradient whose norm is far above max_norm = 1 whatever n"""
    rng = np.random.default_rng(seed_of("adam", n, idx))
    p = rng.normal(size=n).astype(F32)
    g = ((1.0 + np.abs(rng.normal(size=n))) * rng.choice([-1.0, 1.0], n) * 1024.0 * 3.0).astype(F32)
    m = (rng.normal(size=n) * 0.1).astype(F32)
    v = (rng.random(size=n) * 0.01).astype(F32)
    return p, g, m, v


# ---- the other case tables
RMS_COLS = (1, 31, 32, 33, 54, 63, 64)
RMS_ROWS = (1, 3, 4, 5, 127, 128, 129, 513)
RMS_CAPPED = (131072 + 130, 3)
NORMALIZE_CASES = [(1, 1), (3, 54), (4, 64), (13, 200), (257, 1), (37, 54)]      # (rows, cols): totals 1, 162, 256, 2600, 257, 1998
SAMPLE_N = (1, 255, 256, 257)
SAMPLE_A = (1, 18, 32)
SAMPLE_D = (1, 54, 64)
SAMPLE_BIG = (4097, 18, 64)
POST_N = (1, 64, 65, 257)
POST_PATTERNS = ("none", "all", "timeouts-bootstrap", "timeouts-plain")
FOLD_SLOTS = (1, 63, 257)
WSUM_SPLITS = (1, 3, 4, 5, 8, 64)
WSUM_N = (1, 2, 63, 127, 128, 129)
COLSUM_ROWS = (1, 3, 4, 7, 8, 9, 255, 256, 257, 513)
COLSUM_COLS = (1, 2, 19, 127, 128, 129, 130, 257)
HEAD_A = (1, 7, 18, 32, 100, 255, 256)
HEAD_ROWS = (1, 255, 256, 257, 600)
GAE_H = (1, 7, 8, 9, 16, 17)
GAE_N = (1, 255, 257)
GAE_PATTERNS = ("none", "all", "last")
GAE_UNNORM = (0.3, 2.5, 1e-5)      # (mean, var, eps) of the value normaliser where the bootstrap values are de-normalised


def rms_data(rows, cols):
    """unit noise on a common offset of about 10^3: an fp32 accumulation anywhere fails the fp64 bar"""
    rng = np.random.default_rng(seed_of("rms", rows, cols))
    return (rng.normal(size=(rows, cols)) + 1000.0 + 10.0 * np.arange(cols)).astype(F32)


def elu_data(rows, cols):
    """fp16 (gy, y) with y = 0, -0.0, just above -1 and positive values among the random ELU outputs"""
    rng = np.random.default_rng(seed_of("elu", rows, cols))
    gy = rng.normal(size=(rows, cols)).astype(F16)
    z = rng.normal(size=(rows, cols))
    y = np.where(z > 0, z, np.expm1(z)).astype(F16)
    flat = y.reshape(-1)
    special = np.array([0.0, -0.0, -1.0 + 2.0 ** -11, -1.0 + 2.0 ** -10, 2.0, -(2.0 ** -24)], F16)
    k = min(flat.size, special.size)
    flat[rng.permutation(flat.size)[:k]] = special[:k]
    y = flat.reshape(rows, cols)
    near = elu_bwd(gy, y)[1]
    if near.sum() > ELU_MIDPOINT_CAP * near.size:      # a small case may hold none: those elements get a gradient of 0
        gy[near] = 0.0
    return gy, y


def product(*a):
    return list(itertools.product(*a))


def normalize_data(rows, cols):
    """(x, mean, var, eps).  From 9 rows on: eps = 1 and a column with var = 3 (sqrt(var + eps) = 2 exactly) that holds values exactly on
    and beyond +-5, a column with var = 0, and a NaN and both infinities among the inputs."""
    rng = np.random.default_rng(seed_of("normalize", rows, cols))
    mean, var = rng.normal(size=cols) * 0.5, rng.random(size=cols) + 0.5
    x = (rng.normal(size=(rows, cols)) * 2.0 + mean).astype(F32)
    if rows < 9:
        return x, mean, var, 1e-5
    c, z = cols // 2, 0
    mean[c], var[c], var[z] = 2.0, 3.0, 0.0
    if c == z:       # one column: it is the exact one
        var[z] = 3.0
    x[:6, c] = [12.0, -8.0, 14.0, -10.0, 2.0, 11.99]      # (x - 2) / 2 = 5, -5, 6, -6, 0, 4.995
    x[-1, c], x[-2, c], x[-3, c] = np.nan, np.inf, -np.inf
    if c != z:
        x[0, z] = mean[z] + 7.0
        x[1, z] = mean[z] - 7.0
    return x, mean, var, 1.0


def post_data(n, pattern):
    """one env step's inputs: integer-valued rewards, returns and lengths (their fp32 and fp64 sums are exact)"""
    rng = np.random.default_rng(seed_of("post", n, pattern))
    dones = np.zeros(n, np.int64)
    timeouts = np.zeros(n, np.int64)
    if pattern == "all":
        dones[:] = 1
    elif pattern.startswith("timeouts"):
        dones = (rng.random(n) < 0.4).astype(np.int64)
        dones[0] = 1
        timeouts = dones * (rng.random(n) < 0.5)
        timeouts[0] = 1
    return dict(rew=rng.integers(-5, 6, n).astype(F32), values=rng.normal(size=n).astype(F32), dones=dones, timeouts=timeouts.astype(np.int64),
                cur_rew=rng.integers(-40, 40, n).astype(F32), cur_len=rng.integers(0, 50, n).astype(F32), bootstrap=pattern != "timeouts-plain")


def fold_data(slots):
    """(slots, 4) fp64: episode count, return sum, length sum (integers; nothing where the count is 0) and a fourth word that is nobody's"""
    rng = np.random.default_rng(seed_of("fold", slots))
    c = rng.integers(0, 4, slots).astype(F64)
    c[0] = 2.0
    return np.stack([c, rng.integers(-90, 90, slots) * (c > 0), rng.integers(1, 400, slots) * (c > 0), 123.25 + np.arange(slots)], 1).astype(F64)


def wsum_data(splits, n):
    rng = np.random.default_rng(seed_of("wsum", splits, n))
    return rng.normal(size=(splits, n)).astype(F16), rng.normal(size=n).astype(F32)


def head_data(rows, a):
    rng = np.random.default_rng(seed_of("head", rows, a))
    return (rng.normal(size=(rows, a)) * 0.01).astype(F32), (rng.normal(size=(rows, 1)) * 0.01).astype(F32)


def gae_data(h, n, pattern):
    rng = np.random.default_rng(seed_of("gae", h, n, pattern))
    mbd = np.zeros((h, n), F32)
    dones = np.zeros(n, F32)
    if pattern == "all":
        mbd[:], dones[:] = 1.0, 1.0
    elif pattern == "last":
        mbd[h - 1] = 1.0
        dones = (rng.random(n) < 0.5).astype(F32)
    last = (rng.normal(size=n) * 4.0).astype(F32)
    last[0] = 7.5
    last[-1] = -6.25 if n > 1 else 7.5
    return dict(rew=rng.normal(size=(h, n)).astype(F32), val=(rng.normal(size=(h, n)) * 2.0).astype(F32), mb_dones=mbd, dones=dones, last=last)


def _torch_loss(mu, logstd, value, mb, e, critic_coef, entropy_coef, bounds_coef, clip_value):
    from bez_isaacgym_amd.ppo.a2c_continuous import ModelA2CContinuousLogStd, policy_kl
    sigma = torch.exp(logstd).unsqueeze(0).expand_as(mu)
    neglogp = ModelA2CContinuousLogStd.neglogp(mb["actions"], mu, sigma, logstd.unsqueeze(0).expand_as(mu))
    entropy = (0.5 + 0.5 * math.log(2 * math.pi) + logstd.unsqueeze(0).expand_as(mu)).sum(-1)
    ratio = torch.exp(mb["old_logp"] - neglogp)
    a_loss = torch.max(-mb["advantages"] * ratio, -mb["advantages"] * torch.clamp(ratio, 1 - e, 1 + e))
    if clip_value:
        vclip = mb["old_values"] + (value - mb["old_values"]).clamp(-e, e)
        c_loss = torch.max((value - mb["returns"]) ** 2, (vclip - mb["returns"]) ** 2)
    else:
        c_loss = (mb["returns"] - value) ** 2
    b_loss = (torch.clamp_min(mu - 1.1, 0.0) ** 2 + torch.clamp_max(mu + 1.1, 0.0) ** 2).sum(-1)
    loss = a_loss.mean() + 0.5 * c_loss.mean() * critic_coef - entropy.mean() * entropy_coef + b_loss.mean() * bounds_coef
    kl = policy_kl(mu.detach(), sigma.detach(), mb["mu"], mb["sigma"])
    return loss, a_loss.mean(), c_loss.mean(), b_loss.mean(), kl, entropy.mean()
