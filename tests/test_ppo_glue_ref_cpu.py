"""tests/ppo_glue_ref.py on its own, without a GPU: every reference against the torch formulation it restates
(bez_isaacgym_amd/ppo/a2c_continuous.py) run on the CPU in float64 -- agreement to fp64 rounding --, the exclusion rule's caps for every
case from the reference alone, the designed rows on the branches they claim, and finite non-zero bars for every block of every case."""
import math

import numpy as np
import pytest
import torch

from tests import ppo_glue_ref as R

F32, F64 = np.float32, np.float64
T = lambda a: torch.from_numpy(np.ascontiguousarray(a, F64))


def _close(got, want, ops=64):
    """agreement to fp64 rounding: `ops` roundings of the block's largest number"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    tol = ops * R.EPS64 * max(float(np.abs(want).max()), 1e-300)
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= tol, (float(np.abs(got - want).max()), tol)


def _bars_ok(*bars):
    for b in bars:
        b = np.asarray(b, F64)
        assert np.isfinite(b).all() and (b > 0).all(), b


@pytest.mark.parametrize("cols", [1, 54])
def test_running_mean_std(cols):
    from bez_isaacgym_amd.ppo.a2c_continuous import RunningMeanStd
    rms = RunningMeanStd((cols,))
    rms.count.fill_(1e-4)
    rms.train()
    mean, var, count = np.zeros(cols), np.ones(cols), 1e-4
    seen = []
    for rows in (5, 1, 129):
        x = R.rms_data(rows, cols)
        x[:, 0] = 1000.0 if rows == 5 else x[:, 0]      # a constant column: the negative-variance clamp
        seen.append(x)
        rms.update(T(x))
        mom, mbar = R.moments(x)
        assert np.isfinite(mbar).all() and (mbar[:-1] > 0).all()
        bm, bv = R.rms_apply_bars(mean, var, count, mom)
        mean, var, count = R.rms_apply(mean, var, count, mom)
        assert np.abs(rms.running_mean.numpy() - mean).max() <= bm and np.abs(rms.running_var.numpy() - var).max() <= bv and float(rms.count) == count
    # (nearly) the mean of everything seen: the initial count of 1e-4 weighs 1e-4 / 135
    allx = np.concatenate(seen).astype(F64)
    assert np.abs(mean - allx.mean(0)).max() < 1e-3 * np.abs(allx.mean(0)).max()
    # forward / unnorm: torch keeps sqrt(var + eps) an fp32 number whatever the input's type, so the agreement to fp64 rounding is checked
    # where that root is exact (var + eps = 4, 9, 16, 1); on arbitrary statistics the two differ by that root's fp32 rounding
    rms.eval()
    rms.epsilon = 1.0
    rms.running_var.copy_(T(np.resize([3.0, 8.0, 15.0, 0.0], cols))); rms.running_mean.copy_(T(np.round(mean * 8) / 8))
    x = R.rms_data(7, cols) + (rms.running_mean.numpy() - 1000.0 - 10.0 * np.arange(cols)).astype(F32)
    _close(R.normalize(x, rms.running_mean.numpy(), rms.running_var.numpy(), 1.0), rms(T(x)).numpy())
    if cols == 1:
        u = (R.rms_data(7, cols) - 1000.0) * 6
        _close(R.unnormalize(u, rms.running_mean.numpy(), rms.running_var.numpy(), 1.0), rms(T(u), unnorm=True).numpy())
        assert (np.abs(u) > 5).any() and (np.abs(u) < 5).any()
    # the combination rule against the concatenated data: with unbiased batch variances, var_new * tot = SS_all + var_a + var_b exactly
    a, b = R.rms_data(40, cols).astype(F64), R.rms_data(9, cols).astype(F64) * 1.5
    ma, va = a.mean(0), a.var(0, ddof=1)
    m2, v2, tot = R.rms_apply(ma, va, 40.0, R.moments(b.astype(F32))[0])
    b = b.astype(F32).astype(F64)
    cat = np.concatenate([a, b])
    _close(m2, cat.mean(0), 1 << 20)     # (the moments' cancellation at an offset of 10^3: 10^6 x 2^-53 relative to a variance of 1)
    np.testing.assert_allclose(v2 * tot, ((cat - cat.mean(0)) ** 2).sum(0) + va + b.var(0, ddof=1), rtol=1e-8)


def test_sampling_and_neglogp():
    from bez_isaacgym_amd.ppo.a2c_continuous import ModelA2CContinuousLogStd
    for n, a in R.product(R.SAMPLE_N, R.SAMPLE_A):
        rng = np.random.default_rng(R.seed_of("sample", n, a))
        mu, logstd, noise = rng.normal(size=(n, a)).astype(F32), (rng.normal(size=a) * 0.3 - 0.5).astype(F32), rng.normal(size=(n, a)).astype(F32)
        r64, r32 = R.both(R.sample, mu, logstd, noise)
        sig = torch.exp(T(logstd))
        act = T(mu) + sig * T(noise)
        _close(r64["act"], act.numpy())
        _close(r64["env_act"], act.clamp(-1, 1).numpy())
        _close(r64["neglogp"], ModelA2CContinuousLogStd.neglogp(act, T(mu), sig.expand(n, a), T(logstd).expand(n, a)).numpy())
        _bars_ok(*[R.bar(r64[k], r32[k]) for k in r64])


def test_rollout_bookkeeping_and_fold():
    for n, pat in R.product(R.POST_N, R.POST_PATTERNS):
        d = R.post_data(n, pat)
        r64, r32 = R.both(R.rollout_post, d["rew"], d["dones"], d["timeouts"], d["values"], 0.01, 0.99, d["bootstrap"], d["cur_rew"], d["cur_len"])
        rew, val, dn, tm = T(d["rew"]), T(d["values"]), T(d["dones"]), T(d["timeouts"])
        shaped = rew * float(F32(0.01)) + (float(F32(0.99)) * val * tm if d["bootstrap"] else 0.0)    # _rollout_impl
        cr, cl = T(d["cur_rew"]) + rew, T(d["cur_len"]) + 1.0
        _close(r64["shaped"], shaped.numpy())
        assert np.array_equal(r64["cur_rew"], (cr * (1 - dn)).numpy()) and np.array_equal(r64["cur_len"], (cl * (1 - dn)).numpy())
        assert np.array_equal(r64["stats"], [float(dn.sum()), float((cr * dn).sum()), float((cl * dn).sum())])
        # integer-valued: the yardstick is exact too, and every sum stays below 2^24
        for k in ("cur_rew", "cur_len", "stats", "dones_f"):
            assert np.array_equal(np.asarray(r32[k], F64), r64[k]) and np.abs(r64[k]).max(initial=0) < 2 ** 24, k
        assert (r64["stats"][0] == 0) == (pat == "none")
        _bars_ok(R.bar(r64["shaped"], r32["shaped"]))
    for slots in R.FOLD_SLOTS:
        parts = R.fold_data(slots)
        add, after = R.fold(parts)
        assert np.array_equal(add, parts[:, :3].sum(0)) and np.array_equal(after[:, 3], parts[:, 3]) and not after[:, :3].any() and add.max() < 2 ** 24


def _torch_loss64(d, cfg):
    from tests.ppo_glue_ref import _torch_loss
    t = {k: T(d[k]) for k in R.LOSS_KEYS}
    mu, logstd, value = t["mu"].requires_grad_(), t["logstd"].requires_grad_(), t["value"].reshape(-1, 1).requires_grad_()
    mb = dict(actions=t["actions"], old_logp=t["old_logp"], advantages=t["advantages"], old_values=t["old_values"].reshape(-1, 1),
              returns=t["returns"].reshape(-1, 1), mu=t["old_mu"], sigma=t["old_sigma"])
    f = lambda k: float(F32(cfg[k]))
    # (_torch_loss broadcasts (B,) against (B, 1) nowhere: a_loss is (B,), c_loss (B, 1))
    out = _torch_loss(mu, logstd, value, mb, f("e_clip"), f("critic_coef"), f("entropy_coef"), f("bounds_coef"), cfg["clip_value"])
    (out[0] * (f("scale") if cfg["scale"] is not None else 1.0)).backward()
    return [float(o.detach()) for o in out[1:]], mu.grad.numpy(), value.grad.numpy().reshape(-1), logstd.grad.numpy()


@pytest.mark.parametrize("case", R.loss_cases(), ids=lambda c: "n%d-a%d-%d" % c)
def test_loss_reference_against_autograd(case):
    n, a, idx = case
    d, cfg, rows, r64, bars, kp, kv = R.loss_ref(*case)
    (a_l, c_l, b_l, kl, ent), gmu, gval, glog = _torch_loss64(d, cfg)
    want = np.array([a_l, c_l, b_l if cfg["bounds_coef"] > 0 else 0.0, kl, ent]) * n
    ops = 64 * (a + 8)
    _close(r64["stats"], want, ops)
    _close(r64["gmu"], gmu, ops)
    _close(r64["gval"], gval, ops)
    _close(r64["glog"], glog, ops * n)
    # the exclusion rule's cap, from the reference alone
    assert (~kp | ~kv).sum() <= R.LOSS_EXCLUDE_CAP * n, ((~kp).sum(), (~kv).sum())
    _bars_ok(*bars.values())
    # the designed rows sit on the branch they claim
    e = float(F32(cfg["e_clip"]))
    adv, ratio = d["advantages"].astype(F64), r64["ratio"]
    for p, r in rows.items():
        assert kp[r] and kv[r], p
        if p.startswith("clip_hi"):
            assert ratio[r] > 1 + e + 0.1 and adv[r] == (1.0 if p.endswith("+") else -1.0)
            assert r64["g_ratio"][r] == (0.0 if adv[r] > 0 else 1.0)          # a positive advantage at a ratio clipped high: no gradient
        if p.startswith("clip_lo"):
            assert ratio[r] < 1 - e - 0.1 and r64["g_ratio"][r] == (-1.0 if adv[r] > 0 else 0.0)
        if p == "adv0":
            assert adv[r] == 0 and r64["g_ratio"][r] == 0
        if cfg["clip_value"] and p in ("dv_above", "dv_below"):
            assert abs(float(d["value"][r]) - float(d["old_values"][r])) == 0.5 > e
        if p == "dv_zero":
            assert d["value"][r] == d["old_values"][r]
        if p == "mu_above":
            assert d["mu"][r, 0] == 1.5 and (cfg["bounds_coef"] == 0 or r64["stats"][2] > 0)
        if p == "mu_below":
            assert d["mu"][r, a - 1] == -1.75
        if p == "value_tie" and cfg["clip_value"]:
            assert e == 0.25 and r64["c_rows"][r] == 0.0625 and r64["g_v"][r] == 0.5 * (2 * 0.25 + 0.0)      # half of d q1 / d v, nothing from the clipped branch


def test_loss_cases_reach_every_mode():
    cfgs = [R.loss_cfg(i) for _, _, i in R.loss_cases()]
    for k, vals in (("clip_value", (True, False)), ("bounds_coef", (0.0, 0.5)), ("entropy_coef", (0.0, 0.01)), ("scale", (None, 1024.0)),
                    ("accumulate", (True, False)), ("update_mu_sigma", (True, False)), ("e_clip", (0.2, 0.25))):
        assert {c[k] for c in cfgs} == set(vals), k
    assert sorted({a for n, a, _ in R.loss_cases() if n == 65}) == list(range(1, 33))
    ties = [c for c in R.loss_cases() if "value_tie" in R.loss_ref(*c)[2] and R.loss_ref(*c)[1]["clip_value"]]
    assert len(ties) >= 6


def test_gradient_reductions():
    for s, n in R.product(R.WSUM_SPLITS, R.WSUM_N):
        part, base = R.wsum_data(s, n)
        r64, r32 = R.both(R.wgrad_sum, part, base)
        _close(r64, (T(base) + T(part.astype(F64)).sum(0)).numpy())
        _bars_ok(R.bar(r64, r32))
    worst = 0.0
    for rows, cols in R.product(R.COLSUM_ROWS, R.COLSUM_COLS):
        gy, y = R.elu_data(rows, cols)
        gz, near = R.elu_bwd(gy, y)
        # elu'(x) from the output y = elu(x): 1 for y > 0, y + 1 otherwise
        want = (T(gy.astype(F64)) * torch.where(T(y.astype(F64)) > 0, torch.ones(()).double(), T(y.astype(F64)) + 1.0)).numpy()
        assert np.array_equal(gz, want.astype(np.float16))
        assert near.sum() <= R.ELU_MIDPOINT_CAP * near.size, (rows, cols, int(near.sum()))
        worst = max(worst, near.mean())
        r64, r32 = R.both(R.colsum, gz)
        _close(r64, T(gz.astype(F64)).sum(0).numpy())
        _bars_ok(R.bar(r64, r32))
        if rows * cols >= 6:
            assert (y == 0).any() and np.signbit(y[y == 0]).any() and (y.astype(F64) == -1 + 2.0 ** -11).any() and (y > 1).any()
    for a, rows in R.product(R.HEAD_A, R.HEAD_ROWS):
        gmu, gval = R.head_data(rows, a)
        h_mu, h_v = R.head_grads(gmu, gval)
        assert np.array_equal(h_mu, torch.from_numpy(gmu).half().numpy()) and np.array_equal(h_v, torch.from_numpy(gval).half().numpy().reshape(-1))
        _bars_ok(R.bar(*R.both(R.colsum, h_mu)), R.bar(*R.both(R.colsum, h_v.reshape(-1, 1))))


def test_gae():
    from bez_isaacgym_amd.ppo.a2c_continuous import RunningMeanStd, discount_values
    for h, n, pat in R.product(R.GAE_H, R.GAE_N, R.GAE_PATTERNS):
        d = R.gae_data(h, n, pat)
        for unnorm in (None, (0.25, 3.0, 1.0)):      # (sqrt(var + eps) = 2: torch keeps that root in fp32)
            (adv, ret), (adv32, ret32) = R.both(R.gae, d["rew"], d["val"], d["mb_dones"], d["dones"], d["last"], 0.99, 0.95, unnorm=unnorm)
            last = T(d["last"]).reshape(n, 1)
            if unnorm is not None:
                rms = RunningMeanStd((1,), epsilon=unnorm[2])
                rms.running_mean.fill_(unnorm[0]); rms.running_var.fill_(unnorm[1])
                rms.eval()
                last = rms(last, unnorm=True)
                assert (np.abs(d["last"]) > 5).any() or n == 1
            want = discount_values(float(F32(0.99)), float(F32(0.95)), T(d["dones"]), last, T(d["mb_dones"]), T(d["val"]).reshape(h, n, 1),
                                   T(d["rew"]).reshape(h, n, 1)).reshape(h, n)
            _close(adv, want.numpy(), 64 * h)
            _close(ret, (want + T(d["val"])).numpy(), 64 * h)
            _bars_ok(R.bar(adv, adv32), R.bar(ret, ret32))


@pytest.mark.parametrize("case", R.PREP_CASES, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_prepare_dataset(case):
    from bez_isaacgym_amd.ppo.a2c_continuous import RunningMeanStd, swap_and_flatten01
    h, n, nmb, dcols, mbrows, norm_v, norm_a, const = case
    values, returns, obs, vrms = R.prep_data(case)
    r64, r32 = R.both(R.dataset_prep, values, returns, vrms, norm_a)
    v, r = swap_and_flatten01(T(values).reshape(h, n, 1)), swap_and_flatten01(T(returns).reshape(h, n, 1))
    assert v.shape == (h * n, 1) and float(v[min(1, h * n - 1), 0]) == float(values[1 % h, 1 // h])     # env-major: row j = env j // H, step j % H
    if norm_v:
        rms = RunningMeanStd((1,), epsilon=vrms[3])
        rms.running_mean.fill_(vrms[0]); rms.running_var.fill_(vrms[1]); rms.count.fill_(vrms[2])
        vm, rm = rms.moments(v), rms.moments(r)
        _close(vm.numpy(), r64["val_mom"])
        rms.eval()
        # torch keeps sqrt(var + eps) an fp32 number; with that one factor put back the two agree to fp64 rounding (where the clamp is idle)
        for name, mom, x in (("old_values", vm, v), ("returns", rm, r)):
            rms.update_from_moments(mom)
            y = rms(x)
            root32 = float(torch.sqrt(rms.running_var.float() + rms.epsilon))
            root64 = float(R._sd(rms.running_var.numpy(), rms.epsilon, F64)[0])
            idle = np.abs(r64[name]) < 4.99
            assert idle.sum() > 0.8 * idle.size
            _close(r64[name][idle] * root64, y.reshape(-1).numpy()[idle] * root32, 1 << 12)
            if name == "old_values":
                v = y
            else:
                r = y
        _close([float(rms.running_mean), float(rms.running_var), float(rms.count)], r64["vrms"], 1 << 12)
    adv = (r - v).sum(dim=1)
    if norm_a:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    # (with the value normaliser: torch's sqrt(var + eps) is an fp32 number, the reference's an fp64 one -- two fp32 roundings, add and root)
    ops = (1 << 31) if norm_v else (1 << 12)
    _close(r64["old_values"], v.reshape(-1).numpy(), ops)
    _close(r64["returns"], r.reshape(-1).numpy(), ops)
    if norm_v and norm_a:
        ops *= 8      # (advantage = the difference of two such numbers, divided by a std below 1)
    if const and not norm_v:
        assert not r64["advantages"].any() if norm_a else (r64["advantages"] == 0.5).all()
        assert np.array_equal(adv.numpy(), r64["advantages"])
    else:
        _close(r64["advantages"], adv.numpy(), ops)
    _bars_ok(*[R.bar(r64[k], r32[k]) for k in ("old_values", "returns", "advantages")])
    if nmb:
        mom, mbar = R.moments(obs[:mbrows])
        _close(mom, RunningMeanStd((dcols,)).moments(T(obs[:mbrows])).numpy())
    assert R.prep_scratch_doubles(h, n, mbrows, nmb) > 0


def test_prepare_dataset_refusals_are_what_the_header_says():
    for what, h, n, nmb, d, short, code in R.PREP_REFUSED:
        assert (code == -3) == ((h * n) % 64 != 0)
        assert what != "minibatches" or nmb > 8
        assert what != "observations" or d > 64


@pytest.mark.parametrize("n", [1, 5, 4097])
def test_adam_against_torch(n):
    for idx in range(6):
        hp = R.adam_hp(idx)
        p, g, m, v = R.adam_data(n, idx)
        for scale in (None, 1024.0):
            st = dict(p=p, m=m, v=v, step=0.0, lr=3e-4, scale=scale, tracker=0)
            w = torch.nn.Parameter(T(p))
            opt = torch.optim.Adam([w], lr=float(F32(3e-4)), betas=(float(F32(0.9)), float(F32(0.999))), eps=float(F32(1e-8)), weight_decay=float(F32(hp["weight_decay"])))
            opt.state[w] = dict(step=torch.tensor(0.0), exp_avg=T(m), exp_avg_sq=T(v))
            for k in range(2):
                out = R.adam(st, g, hp)
                inv = 1.0 / ((float(scale) if scale else 1.0) * (hp["grad_div"] if hp["grad_div"] > 1 else 1.0))
                w.grad = T(g) * inv
                norm = float(w.grad.norm())
                if hp["max_norm"] > 0:
                    torch.nn.utils.clip_grad_norm_([w], hp["max_norm"])
                opt.step()
                assert not out["skipped"] and abs(out["norm"] - norm) <= 1e-12 * norm and norm > 1.0
                _close(out["p"], w.detach().numpy(), 4096)
                _close(out["m"], opt.state[w]["exp_avg"].numpy(), 4096)
                _close(out["v"], opt.state[w]["exp_avg_sq"].numpy(), 4096)
                assert out["step"] == k + 1.0
                st = {kk: out[kk] for kk in st}
            r64, r32 = R.adam(dict(st, step=0.0), g, hp), R.adam(dict(st, step=0.0), g, hp, dt=F32)
            _bars_ok(*[R.bar(r64[k], r32[k]) for k in ("p", "m", "v")])


def test_adam_skips_and_schedules():
    hp = dict(R.adam_hp(0), interval=2, tail=[(1.0, 2.0, 0.5)], adapt=(0.1, 0.008, 1e-6, 1e-2))
    p, g, m, v = R.adam_data(9, 0)
    st = dict(p=p, m=m, v=v, step=3.0, lr=3e-4, scale=1024.0, tracker=0)
    for bad in (np.inf, np.nan):
        gb = g.copy(); gb[-1] = bad
        out = R.adam(st, gb, hp)
        assert out["skipped"] and out["scale"] == 512.0 and out["tracker"] == 0 and out["step"] == 3.0 and out["p"] is p
        assert out["tail"] == [2.0] and abs(out["lr"] - float(F32(3e-4)) / 1.5) < 1e-12      # the tail sums and the lr rule run on a skipped step too
        assert R.adam(dict(st, scale=None), gb, hp)["skipped"] is False                    # GradScaler skips; without one the step is taken
    out = R.adam(dict(st, tracker=1), g, hp)
    assert not out["skipped"] and out["scale"] == 2048.0 and out["tracker"] == 0
    assert R.adam(st, g, hp)["tracker"] == 1
    # finite, but the squared norm is beyond fp32
    big = np.full(9, 1e30, F32)
    assert R.adam(st, big, dict(hp, overflow_skips=True))["skipped"]
    out = R.adam(st, big, dict(hp, overflow_skips=False))
    assert not out["skipped"] and np.array_equal(out["m"], F64(F32(0.9)) * m.astype(F64))      # torch: coef = max_norm / inf = 0
    from bez_isaacgym_amd.ppo.a2c_continuous import AdaptiveScheduler
    s = AdaptiveScheduler(0.008)
    for lr, kl in ((3e-4, 0.1), (3e-4, 0.001), (3e-4, 0.008), (1e-6, 0.1), (1e-2, 0.0)):
        assert abs(float(R.adaptive_lr(lr, kl, 0.008, 1e-6, 1e-2)) - s.update(float(F32(lr)), float(F32(kl)))) <= 2.0 ** -23 * lr      # (the limits reach the kernel as fp32)


def test_adam_cases_reach_every_switch_in_every_norm_mode():
    for mode in R.ADAM_MODES:
        hps = [R.adam_hp(i) for n, m, i in R.adam_cases() if m == mode]
        for k, vals in (("max_norm", {0.0, 1.0}), ("ntail", {0, 4}), ("weight_decay", {0.0, 0.01}), ("grad_div", {1.0, 2.0}), ("nsteps", {1, 64}), ("interval", {2, 2000})):
            assert {h[k] for h in hps} == vals, (mode, k)
    for n in R.ADAM_N:
        pos = R.adam_bad_positions(n)
        assert pos[0] == 0 and pos[-1] == n - 1 and all(0 <= q < n for q in pos)
        assert n <= 524289 or any(524288 <= q < n - 1 for q in pos)
    assert 524288 in R.adam_bad_positions(524289)      # n - 1 there: the one element behind the grid's two passes


def test_norm_parts_layout():
    for n in R.ADAM_N:
        g = R.adam_data(n, 0)[1]
        s64, s32, bad = R.norm_parts(g)
        units = n // 4 + n % 4
        assert len(s64) == (units + 1023) // 1024 and not bad.any()
        _close(s64.sum(), (g.astype(F64) ** 2).sum(), 4096)
        _bars_ok(R.bar(s64, s32))
        gb = g.copy(); gb[-1] = np.inf
        assert R.norm_parts(gb)[2].tolist() == [0] * (len(s64) - 1) + [1]
    # n / 4 one short of a multiple of 1024: the n % 4 tail spills into a workgroup of its own
    assert len(R.norm_parts(np.ones(4 * 1023 + 3, F32))[0]) == 2 and R.norm_parts(np.ones(4 * 1023 + 3, F32))[0].tolist() == [4093.0, 2.0]


def test_normalize_cases():
    for rows, cols in R.NORMALIZE_CASES:
        x, mean, var, eps = R.normalize_data(rows, cols)
        r64, r32 = R.both(R.normalize, x, mean, var, eps)
        fin = np.isfinite(x)
        assert np.abs(r64[fin]).max() <= 5.0
        _bars_ok(R.bar(r64[fin], r32[fin]), R.bar(r64[fin], r32[fin], half=True))
        if rows >= 9:
            assert (r64 == 5.0).any() and (r64 == -5.0).any() and np.isnan(r64).any() and ((var == 0).any() or cols == 1)
            # exactly on the limit without the clamp's help: (x - mean) / sqrt(var + eps) = +-5 in exact arithmetic
            assert eps == 1.0
            c = int(np.argmax(var == 3.0))
            on = (x[:, c].astype(F64) - mean[c]) / 2.0
            assert (on == 5.0).any() and (on == -5.0).any() and (np.abs(on) > 5).any()
