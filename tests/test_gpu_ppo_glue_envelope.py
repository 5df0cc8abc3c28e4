"""The PPO glue kernels (csrc/bez_ppo.hip, csrc/bez_ppo_loss.h: every bez_ppo_* entry point defined there) across the shapes their host gates
accept, against the fp64 references of tests/ppo_glue_ref.py.  Bars come from the reference alone (3 x the fp32 yardstick's worst error + 2
ulps of the block's largest |reference|; exact where the arithmetic is exact or the output is a copy); every output is allocated with
sentinel rows behind it -- and in front, for the buffers a kernel updates in place -- which must be untouched after every call; refused
shapes are declined by the host gate with every output untouched.  The case tables, the bars and the exclusion rule are those of
tests/ppo_glue_ref.py; DESIGN.md 6 states the envelope.

BEZ_ENVELOPE_REPORT=<file>: the worst observed error / bar of every case is APPENDED there, as the policy envelope's file does with the same
variable: for profiles/ppo_glue_envelope_errors.txt remove the file first and run this test file alone."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import ppo_glue_ref as R
from tests.gpu_util import DEV, GUARD, Guarded, SENT

pytestmark = pytest.mark.gpu
F16, F32, F64 = np.float16, np.float32, np.float64
FRONT = 4       # sentinel rows in front of a banded buffer (4: a flat fp32 buffer stays 16-byte aligned, as the optimiser's float4 loads ask)
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("BEZ_ENVELOPE_REPORT")
    if path and REPORT:
        with open(path, "a") as f:
            for key in sorted(REPORT):
                f.write("%-44s %s\n" % (key, "  ".join("%s=%s" % kv for kv in REPORT[key].items())))


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_error():
    """a test that leaves the device in an error state ends the session: nothing more is launched on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error, nothing more is launched: %s" % e, returncode=3)


class Banded(Guarded):
    """Guarded with FRONT sentinel rows in front as well: for flat buffers and for what a kernel updates in place"""

    def __init__(self, n, cols=None, dtype=torch.float32, init=None):
        self.n = n
        self.full = torch.full((n + FRONT + GUARD,) if cols is None else (n + FRONT + GUARD, cols), SENT, device=DEV, dtype=dtype)
        self.t = self.full[FRONT:FRONT + n]
        if init is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(init)).reshape(self.t.shape))

    def band_untouched(self):
        return bool((self.full[:FRONT] == SENT).all()) and bool((self.full[FRONT + self.n:] == SENT).all())


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def P(t):
    return None if t is None else C.c_void_p((t.t if isinstance(t, Guarded) else t).data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def lib():
    from bez_isaacgym_amd.ppo import fused as F
    return F.lib()


def host(t):
    return (t.t if isinstance(t, Guarded) else t).double().cpu().numpy()


def check(key, name, got, ref, bar, keep=None):
    """|got - ref| <= bar everywhere (bar: a number or an array; 0 = equal); the worst ratio is printed before it is asserted and kept for the report"""
    ref = np.asarray(ref, F64)
    got = host(got).reshape(ref.shape) if not isinstance(got, np.ndarray) else got.reshape(ref.shape)
    diff = np.abs(got - ref)
    diff[(got == ref)] = 0.0       # (equal infinities)
    bar = np.broadcast_to(np.asarray(bar, F64), ref.shape)
    if keep is not None:
        diff, bar = diff[keep], bar[keep]
    ratio = np.where(diff == 0, 0.0, diff / np.maximum(bar, 1e-300))
    worst = float(ratio.max()) if ratio.size else 0.0
    REPORT.setdefault(key, {})[name] = "%.3f" % worst if np.isfinite(worst) else "FAIL"
    print("%s %s: worst |error| / bar = %.3f (max |error| %.3e)" % (key, name, worst, float(diff.max()) if diff.size else 0.0))
    assert worst <= 1.0 and not np.isnan(diff).any(), (key, name, worst, np.argwhere(~(ratio <= 1.0))[:4].tolist())


def exact(key, name, got, ref):
    ref = np.asarray(ref)
    got = host(got).reshape(ref.shape) if not isinstance(got, np.ndarray) else got.reshape(ref.shape)
    bad = np.argwhere(got != ref.astype(F64))
    assert bad.size == 0, "%s %s: %d mismatches, first at %s: got %s, want %s" % (key, name, len(bad), bad[:4].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
    REPORT.setdefault(key, {})[name] = "exact"


def bands(key, *bufs):
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert b.band_untouched(), (key, i)


# ---------------------------------------------------------------------------------------------------------------- running mean / std
@pytest.mark.parametrize("rows,cols", R.product(R.RMS_ROWS, R.RMS_COLS) + [R.RMS_CAPPED], ids=lambda v: str(v))
def test_rms_moments(rows, cols):
    """bez_ppo_rms_moments with float atomics (scratch NULL) and in a fixed order (three calls: the same bits): fp64 sums of data at an offset
    of 10^3, at rows * 2^-53 * sum |x| -- an fp32 accumulation anywhere is 10^8 times that"""
    key = "rms_moments r%d-c%d" % (rows, cols)
    x = R.rms_data(rows, cols)
    ref, bars = R.moments(x)
    xd = dev(x)
    g = min((rows + 127) // 128, 1024)
    for path in ("atomics", "fixed"):
        out = Banded(2 * cols + 1, dtype=torch.float64)
        scratch = None if path == "atomics" else Banded(1 + g * 2 * cols, dtype=torch.float64, init=np.zeros(1 + g * 2 * cols))
        seen = []
        for _ in range(1 if path == "atomics" else 3):
            assert lib().bez_ppo_rms_moments(P(xd), rows, cols, P(out), P(scratch), stream()) == 0
            seen.append(out.t.clone())
        assert all(torch.equal(seen[0], s) for s in seen[1:]), key
        check(key, path, out, ref, bars)
        bands(key, out, *([scratch] if scratch else []))


def _rms_cases(cols):
    """(name, mean, var, count, batch): a first update from count 1e-4, a batch of one row (the n - 1 clamp), a constant column (the
    negative-variance clamp), and statistics that ARE a batch's, so that the result can be held against the concatenated data"""
    a = R.rms_data(40, cols).astype(F64)
    const = R.rms_data(5, cols)
    const[:, 0] = 1000.0
    return [("first", np.zeros(cols), np.ones(cols), 1e-4, R.rms_data(5, cols)), ("one-row", np.full(cols, 999.0), np.full(cols, 2.0), 37.0, R.rms_data(1, cols)),
            ("constant", np.full(cols, 1001.0), np.full(cols, 0.5), 12.0, const), ("concat", a.mean(0), a.var(0, ddof=1), 40.0, R.rms_data(9, cols) * F32(1.5))]


@pytest.mark.parametrize("via", ["rms_apply", "adam_step"])
@pytest.mark.parametrize("cols", [1, 64])
def test_rms_apply(cols, via):
    """bez_ppo_rms_apply, and the same update restated inside the optimiser launch (adam_step(next_rms=)), against the formula in fp64 and
    against mean / variance of the concatenated data"""
    from bez_isaacgym_amd.ppo import fused as F
    for name, mean, var, count, x in _rms_cases(cols):
        key = "%s c%d-%s" % (via, cols, name)
        mom = R.moments(x)[0]
        m, v, c = (Banded(k, dtype=torch.float64, init=a) for k, a in ((cols, mean), (cols, var), (1, [count])))
        md = dev(mom)
        if via == "rms_apply":
            assert lib().bez_ppo_rms_apply(P(md), cols, P(m), P(v), P(c), stream()) == 0
        else:
            rms = types.SimpleNamespace(running_mean=m.t, running_var=v.t, count=c.t)
            z = lambda k, val=0.0: Banded(k, init=np.full(k, val, F32))
            p, g, ea, es, steps, lr, work = z(4, 1.0), z(4, 0.5), z(4), z(4), z(1), z(1, 1e-3), z(F.ADAM_WORK_FLOATS)
            F.adam_step(p.t, g.t, ea.t, es.t, steps.t, lr.t, (0.9, 0.999), 1e-8, 0.0, 1.0, None, None, 2.0, 0.5, 2000, work.t,
                        next_rms=(types.SimpleNamespace(rms=rms, d=cols), md))
            bands(key, p, g, ea, es, steps, lr, work)
            assert not work.t.any() and float(steps.t[0]) == 1.0
        rm, rv, rc = R.rms_apply(mean, var, count, mom)
        bm, bv = R.rms_apply_bars(mean, var, count, mom)
        check(key, "mean", m, rm, bm)
        check(key, "var", v, rv, bv)
        exact(key, "count", c, [rc])
        bands(key, m, v, c)
        if name == "concat":     # var_new * tot = SS of everything + var_a + var_b (unbiased batch variances, rl_games' rule), mean_new = its mean
            cat = np.concatenate([R.rms_data(40, cols).astype(F64), x.astype(F64)])
            slack = cat.shape[0] * R.EPS64 * (cat * cat).sum(0).max()      # the moments' own rounding: rows * 2^-53 * sum x^2
            check(key, "mean-of-all", m, cat.mean(0), bm + slack / cat.shape[0])
            check(key, "var-of-all", host(v) * rc, ((cat - cat.mean(0)) ** 2).sum(0) + var + x.astype(F64).var(0, ddof=1), rc * bv + 4 * slack)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("rows,cols", R.NORMALIZE_CASES, ids=lambda v: str(v))
def test_rms_normalize(rows, cols, half):
    """bez_ppo_rms_normalize.  Non-finite inputs: the kernel's fminf / fmaxf return the other operand for a NaN, so a NaN observation becomes -5
    where RunningMeanStd.forward (torch.clamp) hands the NaN on; +-inf become +-5 in both."""
    key = "rms_normalize r%d-c%d-%s" % (rows, cols, "f16" if half else "f32")
    x, mean, var, eps = R.normalize_data(rows, cols)
    r64, r32 = R.both(R.normalize, x, mean, var, eps)
    y = Banded(rows, cols, torch.float16 if half else torch.float32)
    xd, md, vd = dev(x), dev(mean), dev(var)
    assert lib().bez_ppo_rms_normalize(P(xd), rows, cols, P(md), P(vd), C.c_float(eps), P(y), 1 if half else 0, stream()) == 0
    fin = np.isfinite(x)
    check(key, "y", y, np.where(fin, r64, 0.0), R.bar(r64[fin], r32[fin], half), keep=fin)
    got = host(y)
    assert np.abs(got).max() <= 5.0
    if not fin.all():
        assert np.isnan(r64[np.isnan(x)]).all()                                      # torch.clamp: NaN
        assert (got[np.isnan(x)] == -5.0).all(), got[np.isnan(x)]                     # the kernel: -5
        assert (got[x == np.inf] == 5.0).all() and (got[x == -np.inf] == -5.0).all() and (r64[x == np.inf] == 5.0).all()
        on = np.abs((x.astype(F64) - mean) / 2.0) == 5.0
        assert on.any() and (np.abs(got[on & (var == 3.0)]) == 5.0).all()
    bands(key, y)


# ---------------------------------------------------------------------------------------------------------------- sampling, rollout
def _sample_inputs(n, a, d):
    rng = np.random.default_rng(R.seed_of("sample", n, a, d))
    f = lambda *s: rng.normal(size=s).astype(F32)
    return dict(mu=f(n, a) * F32(0.7), value=f(n, 1) * F32(4.0), logstd=f(a) * F32(0.3) - F32(0.5), noise=f(n, a), obs=f(n, d), dones=(rng.random(n) < 0.3).astype(F32))


def _check_sampling(key, tag, out, mu32, logstd, noise):
    r64, r32 = R.both(R.sample, mu32, logstd, noise)
    for k in ("act", "env_act", "sigma", "neglogp"):
        check(key, tag + k, out[k], r64[k], R.bar(r64[k], r32[k]))
    assert np.abs(host(out["env_act"])).max() <= 1.0


@pytest.mark.parametrize("n,a,d", R.product(R.SAMPLE_N, R.SAMPLE_A, R.SAMPLE_D) + [R.SAMPLE_BIG], ids=lambda v: str(v))
def test_sample_and_rollout_pre(n, a, d):
    """bez_ppo_sample, and bez_ppo_rollout_pre with fp16 and fp32 network outputs, with and without the value normaliser: the rollout-buffer rows are
    copies (bit for bit), the de-normalised value and the sampling within their bars"""
    from bez_isaacgym_amd.ppo import fused as F
    key = "sample n%d-a%d-d%d" % (n, a, d)
    i = _sample_inputs(n, a, d)
    t = {k: dev(v) for k, v in i.items()}
    out = dict(act=Guarded(n, a), env_act=Guarded(n, a), neglogp=Banded(n), sigma=Guarded(n, a))
    F.sample(t["mu"], t["logstd"], t["noise"], out["act"].t, out["env_act"].t, out["neglogp"].t, out["sigma"].t)
    _check_sampling(key, "", out, i["mu"], i["logstd"], i["noise"])
    bands(key, *out.values())
    vstat = types.SimpleNamespace(running_mean=dev(np.array([0.3])), running_var=dev(np.array([2.5])), epsilon=1e-5)
    big = (n, a, d) == R.SAMPLE_BIG
    for half, rms in ((False, vstat),) if big else ((False, None), (False, vstat), (True, None), (True, vstat)):
        k2 = "rollout_pre n%d-a%d-d%d-%s-%s" % (n, a, d, "f16" if half else "f32", "vnorm" if rms else "plain")
        mu_in, v_in = (t["mu"].half(), t["value"].half()) if half else (t["mu"], t["value"])
        mu32, v32 = mu_in.float().cpu().numpy(), v_in.float().cpu().numpy()
        o = dict(mb_obs=Guarded(n, d), mb_dones=Banded(n), mb_mu=Guarded(n, a), mb_val=Guarded(n, 1), act=Guarded(n, a), env_act=Guarded(n, a), neglogp=Banded(n),
                 sigma=Guarded(n, a))
        F.rollout_pre(mu_in, v_in, t["logstd"], t["noise"], t["obs"], t["dones"], rms, *[o[k].t for k in ("mb_obs", "mb_dones", "mb_mu", "mb_val", "act", "env_act", "neglogp", "sigma")])
        exact(k2, "mb_obs", o["mb_obs"], i["obs"])
        exact(k2, "mb_dones", o["mb_dones"], i["dones"])
        exact(k2, "mb_mu", o["mb_mu"], mu32)
        if rms is None:
            exact(k2, "mb_val", o["mb_val"], v32)
        else:
            r64, r32 = R.both(R.unnormalize, v32, [0.3], [2.5], 1e-5)
            check(k2, "mb_val", o["mb_val"], r64, R.bar(r64, r32))
            assert n == 1 or (np.abs(v32) > 5).any()
        _check_sampling(k2, "", o, mu32, i["logstd"], i["noise"])
        bands(k2, *o.values())


def _post_buffers(n, d):
    return dict(shaped=Banded(n), dones_f=Banded(n), cur_rew=Banded(n, init=d["cur_rew"]), cur_len=Banded(n, init=d["cur_len"]),
                stats=Banded(3, dtype=torch.float64, init=[5.0, -7.0, 11.0]))


def _check_post(key, o, d, extra=0.0):
    r64, r32 = R.both(R.rollout_post, d["rew"], d["dones"], d["timeouts"], d["values"], 0.01, 0.99, d["bootstrap"], d["cur_rew"], d["cur_len"])
    check(key, "shaped", o["shaped"], r64["shaped"], R.bar(r64["shaped"], r32["shaped"]))
    for k in ("dones_f", "cur_rew", "cur_len"):
        exact(key, k, o[k], r64[k])
    exact(key, "stats", o["stats"], np.array([5.0, -7.0, 11.0]) + r64["stats"] + extra)      # integer-valued: exact in fp64 whatever the order
    bands(key, *o.values())
    return r64


@pytest.mark.parametrize("pattern", R.POST_PATTERNS)
@pytest.mark.parametrize("n", R.POST_N)
def test_rollout_post(n, pattern):
    """bez_ppo_rollout_post: no env done (the statistics untouched), every env done, time-outs with and without the value bootstrap"""
    from bez_isaacgym_amd.ppo import fused as F
    key = "rollout_post n%d-%s" % (n, pattern)
    d = R.post_data(n, pattern)
    o = _post_buffers(n, d)
    F.rollout_post(dev(d["rew"]), dev(d["dones"]), dev(d["timeouts"]), dev(d["values"]), 0.01, 0.99, d["bootstrap"], o["shaped"].t, o["dones_f"].t, o["cur_rew"].t,
                   o["cur_len"].t, o["stats"].t)
    r64 = _check_post(key, o, d)
    assert (pattern == "none") == (not r64["stats"].any())


@pytest.mark.parametrize("slots", R.FOLD_SLOTS)
@pytest.mark.parametrize("n", R.POST_N)
def test_rollout_post_fold(n, slots):
    """bez_ppo_rollout_post_fold: the env step's bookkeeping as above, and one more workgroup that adds words 0..2 of every slot to the statistics
    and clears them; word 3 of every slot is nobody's"""
    from bez_isaacgym_amd.ppo import fused as F
    key = "rollout_post_fold n%d-s%d" % (n, slots)
    d = R.post_data(n, "timeouts-bootstrap" if slots != 63 else "none")
    parts = R.fold_data(slots)
    add, after = R.fold(parts)
    o = _post_buffers(n, d)
    pb = Banded(4 * slots, dtype=torch.float64, init=parts.reshape(-1))
    F.rollout_post(dev(d["rew"]), dev(d["dones"]), dev(d["timeouts"]), dev(d["values"]), 0.01, 0.99, d["bootstrap"], o["shaped"].t, o["dones_f"].t, o["cur_rew"].t,
                   o["cur_len"].t, o["stats"].t, ep_parts=pb.t)
    _check_post(key, o, d, extra=add)
    exact(key, "slots", pb, after.reshape(-1))
    bands(key, pb)


# ---------------------------------------------------------------------------------------------------------------- the loss
def _loss_call(t, n, a, cfg, flags, scale, gmu, gval, glog, stats, scratch):
    f = lambda k: C.c_float(float(F32(cfg[k])))
    return lib().bez_ppo_loss(P(t["mu"]), P(t["logstd"]), P(t["value"]), P(t["actions"]), P(t["old_logp"]), P(t["advantages"]), P(t["old_values"]), P(t["returns"]),
                              P(t["old_mu"]), P(t["old_sigma"]), n, a, f("e_clip"), f("critic_coef"), f("entropy_coef"), f("bounds_coef"), flags, P(scale), P(gmu), P(gval),
                              P(glog), P(stats), P(scratch), stream())


def _loss_inputs(d, n, a):
    t = {k: dev(d[k]) for k in R.LOSS_KEYS if k not in ("old_mu", "old_sigma")}
    t["old_mu"], t["old_sigma"] = Banded(n, a, init=d["old_mu"]), Banded(n, a, init=d["old_sigma"])     # (update_mu_sigma writes them)
    return t


@pytest.mark.parametrize("case", R.loss_cases(), ids=lambda c: "n%d-a%d-%d" % c)
def test_loss(case):
    """bez_ppo_loss at every template width: float atomics, the fixed-order sums (three calls: the same bits), the deferred partials (whose
    columns sum to the same values); value clipping, the bounds and entropy terms, the loss scale, the accumulate bits onto non-zero bases and
    update_mu_sigma cycle over the cases (ppo_glue_ref.loss_cfg).  What is compared is the block the kernel writes: where the accumulate bits are
    set that block carries the base, reference and yardstick add it, and the bar's 2-ulp term is that of base + gradient -- so the bare log-sigma
    gradient of an accumulating case is held less tightly than that of an overwriting one (n65-a5-4: 1.6 x the bar of the gradient alone, inside
    the bar of its block; expf(logstd) one ulp off acts on all rows alike).  The deferred launch is the fixed-order launch without its second stage:
    its partials must be the same bits, and their sums are held to that call's output, not to the reference a second time."""
    n, a, idx = case
    key = "loss n%d-a%d-%d" % case
    d, cfg, rows, r64, bars, kp, kv = R.loss_ref(*case)
    scale = None if cfg["scale"] is None else dev(np.array([cfg["scale"]], F32))
    rng = np.random.default_rng(idx)
    base_g, base_s = (rng.integers(-8, 9, a) / 8.0, rng.integers(-8, 9, 5) / 8.0) if cfg["accumulate"] else (np.zeros(a), np.zeros(5))
    flags = (1 if cfg["clip_value"] else 0) | (6 if cfg["accumulate"] else 0) | (8 if cfg["update_mu_sigma"] else 0)
    # the output blocks carry the base: reference and yardstick add it, each in its own arithmetic (excluded rows: their jump stays in the bar)
    want_g, want_s = r64["glog"] + base_g, r64["stats"] + base_s
    r32 = R.loss(d, cfg, dt=F32)
    bar_g = R.bar(want_g, r32["glog"].astype(F32) + base_g.astype(F32)) + float(r64["glog_jump"][~kp].sum(0).max() if (~kp).any() else 0.0)
    bar_s = R.bar(want_s, r32["stats"].astype(F32) + base_s.astype(F32))
    nb = (n + 63) // 64

    def run(tag, scratch, fl):
        t = _loss_inputs(d, n, a)
        gmu, gval, glog, stats = Guarded(n, a), Guarded(n, 1), Banded(a, init=base_g), Banded(5, init=base_s)
        assert _loss_call(t, n, a, cfg, fl, scale, gmu, gval, glog, stats, scratch) == 0
        check(key, tag + "gmu", gmu, r64["gmu"], bars["gmu"], keep=kp)
        check(key, tag + "gval", gval, r64["gval"], bars["gval"], keep=kv)
        if cfg["update_mu_sigma"]:
            exact(key, tag + "new_mu", t["old_mu"], d["mu"])
            check(key, tag + "new_sigma", t["old_sigma"], r64["new_sigma"], bars["new_sigma"])
        else:
            exact(key, tag + "old_mu", t["old_mu"], d["old_mu"])
            exact(key, tag + "old_sigma", t["old_sigma"], d["old_sigma"])
        bands(key, gmu, gval, glog, stats, t["old_mu"], t["old_sigma"])
        return gmu, gval, glog, stats

    _, _, glog, stats = run("atomic-", None, flags)
    check(key, "atomic-glog", glog, want_g, bar_g)
    check(key, "atomic-stats", stats, want_s, bar_s)
    scratch = Banded(2 + nb * (a + 5), init=np.zeros(2 + nb * (a + 5)))
    outs = [run("fixed-", scratch, flags) for _ in range(3)]
    for o in outs[1:]:
        assert all(torch.equal(x.t, y.t) for x, y in zip(outs[0], o)), key
    check(key, "fixed-glog", outs[0][2], want_g, bar_g)
    check(key, "fixed-stats", outs[0][3], want_s, bar_s)
    fresh = Banded(2 + nb * (a + 5), init=np.full(2 + nb * (a + 5), SENT))      # (no partial is a seven: every slot must be written)
    _, _, glog, stats = run("deferred-", fresh, flags | 16)
    assert host(glog).tolist() == base_g.tolist() and host(stats).tolist() == base_s.tolist()    # the partials only
    assert torch.equal(fresh.t[2:], scratch.t[2:]) and not bool((fresh.t[2:] == SENT).any()), key      # the same launch: the same bits
    # ... whose columns sum to what the fixed-order call returned: its second stage adds the same nb partials and the base in fp32, each addition
    # within 2^-24 of a running sum that is at most sum |partials| + |base|
    parts = fresh.t[2:2 + nb * (a + 5)].double().cpu().numpy().reshape(a + 5, nb)
    total, mag = parts.sum(1) + np.concatenate([base_g, base_s]), np.abs(parts).sum(1) + np.abs(np.concatenate([base_g, base_s]))
    check(key, "deferred-sums", total, np.concatenate([host(outs[0][2]), host(outs[0][3])]), (nb + 1) * 2.0 ** -24 * mag)
    bands(key, fresh)
    bands(key, scratch)


def test_loss_refusals():
    """33 actions, and the deferred partials without a scratch: -1 from the host gate, nothing written"""
    n = 65
    for a, flags, with_scratch in ((33, 1, True), (18, 17, False)):
        d, cfg, _ = R.loss_data(n, a, 0)
        t = _loss_inputs(d, n, a)
        gmu, gval, glog, stats = Guarded(n, a), Guarded(n, 1), Banded(a), Banded(5)
        scratch = Banded(2 + 2 * (a + 5)) if with_scratch else None
        assert _loss_call(t, n, a, cfg, flags, None, gmu, gval, glog, stats, scratch) == -1
        torch.cuda.synchronize()
        assert all(g.untouched() for g in (gmu, gval, glog, stats) + ((scratch,) if scratch else ())), a
        exact("loss refused a%d" % a, "old_mu", t["old_mu"], d["old_mu"])


# ---------------------------------------------------------------------------------------------------------------- gradient reductions
@pytest.mark.parametrize("splits,n", R.product(R.WSUM_SPLITS, R.WSUM_N), ids=lambda v: str(v))
def test_wgrad_sum(splits, n):
    from bez_isaacgym_amd.ppo import fused as F
    key = "wgrad_sum s%d-n%d" % (splits, n)
    part, base = R.wsum_data(splits, n)
    out = Banded(n, init=base)
    pd = dev(part)
    F.wgrad_sum(pd, out.t, accumulate=True)
    r64, r32 = R.both(R.wgrad_sum, part, base)
    check(key, "accumulate", out, r64, R.bar(r64, r32))
    F.wgrad_sum(pd, out.t, accumulate=False)
    r64, r32 = R.both(R.wgrad_sum, part)
    check(key, "overwrite", out, r64, R.bar(r64, r32))
    bands(key, out)


@pytest.mark.parametrize("rows,cols", R.product(R.COLSUM_ROWS, R.COLSUM_COLS), ids=lambda v: str(v))
def test_colsum_and_elu_backward(rows, cols):
    """bez_ppo_colsum_f16 and bez_ppo_elu_bwd_colsum_f16, accumulating onto a base and overwriting.  gz = fp16(gy elu'(y)) bit for bit, one fp16 ulp
    where the exact product sits within an fp32 ulp of an fp16 midpoint (the kernel rounds to fp32 first); the bias gradient = the column sums of
    the gz the kernel stored"""
    from bez_isaacgym_amd.ppo import fused as F
    key = "colsum r%d-c%d" % (rows, cols)
    gy, y = R.elu_data(rows, cols)
    base = (np.random.default_rng(rows * 1000 + cols).integers(-8, 9, cols) / 8.0).astype(F32)
    gyd, yd = dev(gy), dev(y)
    for acc in (True, False):
        tag = "accumulate" if acc else "overwrite"
        out = Banded(cols, init=base)
        F.colsum_f16(gyd, out.t, accumulate=acc)
        r64, r32 = R.both(R.colsum, gy, base if acc else None)
        check(key, tag, out, r64, R.bar(r64, r32))
        bands(key, out)
        k2 = key.replace("colsum", "elu_bwd")
        gz, bias = Guarded(rows, cols, torch.float16), Banded(cols, init=base)
        F.elu_bwd_colsum_f16(gyd, yd, gz.t, bias.t, accumulate=acc)
        want, near = R.elu_bwd(gy, y)
        assert near.sum() <= R.ELU_MIDPOINT_CAP * near.size
        got = gz.t.cpu().numpy()
        exact(k2, tag + "-gz", got.astype(F64)[~near], want.astype(F64)[~near])
        assert (np.abs(got.astype(F64)[near] - want.astype(F64)[near]) <= np.spacing(np.abs(want[near])).astype(F64)).all(), k2
        r64, r32 = R.both(R.colsum, got, base if acc else None)
        check(k2, tag + "-bias", bias, r64, R.bar(r64, r32))
        bands(k2, gz, bias)


@pytest.mark.parametrize("a,rows", R.product(R.HEAD_A, R.HEAD_ROWS), ids=lambda v: str(v))
def test_head_grads(a, rows):
    """bez_ppo_head_grads_f16 up to 256 actions (idle threads where 256 % A != 0): the fp16 casts bit for bit, their column sums added to the bias gradients"""
    from bez_isaacgym_amd.ppo import fused as F
    key = "head_grads a%d-r%d" % (a, rows)
    gmu, gval = R.head_data(rows, a)
    h_mu, h_v = R.head_grads(gmu, gval)
    base = (np.random.default_rng(a).integers(-8, 9, a + 1) / 64.0).astype(F32)
    o = dict(gmu16=Guarded(rows, a, torch.float16), gv16=Guarded(rows, 1, torch.float16), bmu=Banded(a, init=base[:a]), bv=Banded(1, init=base[a:]))
    F.head_grads_f16(dev(gmu), dev(gval), o["gmu16"].t, o["gv16"].t, o["bmu"].t, o["bv"].t)
    exact(key, "gmu16", o["gmu16"], h_mu.astype(F64))
    exact(key, "gv16", o["gv16"], h_v.astype(F64))
    r64, r32 = R.both(R.colsum, h_mu, base[:a])
    check(key, "bmu", o["bmu"], r64, R.bar(r64, r32))
    r64, r32 = R.both(R.colsum, h_v.reshape(-1, 1), base[a:])
    check(key, "bv", o["bv"], r64, R.bar(r64, r32))
    bands(key, *o.values())


def test_head_grads_refuses_257_actions():
    rows, a = 4, 257
    o = [Guarded(rows, a, torch.float16), Guarded(rows, 1, torch.float16), Banded(a), Banded(1)]
    z = torch.zeros(rows, a, device=DEV)
    assert lib().bez_ppo_head_grads_f16(P(z), P(z[:, :1].contiguous()), rows, a, P(o[0]), P(o[1]), P(o[2]), P(o[3]), stream()) == -1
    torch.cuda.synchronize()
    assert all(g.untouched() for g in o)


# ---------------------------------------------------------------------------------------------------------------- GAE, dataset preparation
@pytest.mark.parametrize("h,n", R.product(R.GAE_H, R.GAE_N), ids=lambda v: str(v))
def test_gae(h, n):
    """bez_ppo_gae around its chunks of eight steps: no done, all done, done only at t = H - 1; returns NULL and given; bootstrap values beyond +-5
    through the value normaliser"""
    from bez_isaacgym_amd.ppo import fused as F
    m, v, e = R.GAE_UNNORM
    vstat = types.SimpleNamespace(running_mean=dev(np.array([m])), running_var=dev(np.array([v])), epsilon=e)
    for k, pattern in enumerate(R.GAE_PATTERNS):
        d = R.gae_data(h, n, pattern)
        t = {q: dev(a) for q, a in d.items()}
        for unnorm in (None, R.GAE_UNNORM):
            for with_ret in (True, False) if unnorm is None else (k % 2 == 0,):
                key = "gae h%d-n%d-%s-%s-%s" % (h, n, pattern, "unnorm" if unnorm else "plain", "ret" if with_ret else "noret")
                adv, ret = Guarded(h, n), Guarded(h, n)
                F.gae(t["rew"], t["val"], t["mb_dones"], t["dones"], t["last"], 0.99, 0.95, adv.t, ret.t if with_ret else None, vstat if unnorm else None)
                (a64, r64), (a32, r32) = R.both(R.gae, d["rew"], d["val"], d["mb_dones"], d["dones"], d["last"], 0.99, 0.95, unnorm=unnorm)
                check(key, "adv", adv, a64, R.bar(a64, a32))
                if with_ret:
                    check(key, "returns", ret, r64, R.bar(r64, r32))
                else:
                    assert ret.untouched(), key
                bands(key, adv, ret)


def _prep_call(case, values, returns, obs, vrms, o, scratch, staged):
    from bez_isaacgym_amd.ppo import fused as F
    h, n, nmb, d, mbrows, norm_v, norm_a, _ = case
    if staged:
        rms = None if vrms is None else types.SimpleNamespace(running_mean=o["vmean"].t, running_var=o["vvar"].t, count=o["vcount"].t, epsilon=vrms[3])
        ok = F.dataset_prep(obs if nmb else None, mbrows, nmb, o["obs_mom"].t if nmb else None, values, returns, rms, o["val_mom"].t, o["ret_mom"].t, o["old_values"].t,
                            o["ds_returns"].t, o["advantages"].t, norm_a, scratch.t)
        return 0 if ok else -3
    return lib().bez_ppo_dataset_prep(P(obs) if nmb else None, mbrows, nmb, d, P(o["obs_mom"]) if nmb else None, P(values), P(returns), h, n,
                                      P(o["vmean"]) if vrms else None, P(o["vvar"]) if vrms else None, P(o["vcount"]) if vrms else None,
                                      C.c_float(vrms[3] if vrms else 0.0), P(o["val_mom"]), P(o["ret_mom"]), P(o["old_values"]), P(o["ds_returns"]), P(o["advantages"]),
                                      1 if norm_a else 0, P(scratch), scratch.n, stream())


def _prep_buffers(h, n, nmb, d, vrms):
    f64 = torch.float64
    m, v, c = (vrms[0], vrms[1], vrms[2]) if vrms else (SENT, SENT, SENT)
    return dict(obs_mom=Banded(max(nmb, 1) * (2 * d + 1), dtype=f64), val_mom=Banded(3, dtype=f64), ret_mom=Banded(3, dtype=f64), old_values=Banded(h * n),
                ds_returns=Banded(h * n), advantages=Banded(h * n), vmean=Banded(1, dtype=f64, init=[m]), vvar=Banded(1, dtype=f64, init=[v]),
                vcount=Banded(1, dtype=f64, init=[c]))


@pytest.mark.parametrize("case", R.PREP_CASES, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_dataset_prep(case):
    """bez_ppo_dataset_prep (and the staged entry point behind fused.dataset_prep: the same bits) on the smallest and most lopsided shapes: the
    (H, N) -> env-major transposition, the per-minibatch observation moments, both value-normaliser updates, the advantage normalisation"""
    h, n, nmb, d, mbrows, norm_v, norm_a, const = case
    key = "dataset_prep " + "-".join(str(int(x)) for x in case)
    values, returns, obs, vrms = R.prep_data(case)
    r64, r32 = R.both(R.dataset_prep, values, returns, vrms, norm_a)
    vd, rd, od = dev(values), dev(returns), dev(obs)
    need = R.prep_scratch_doubles(h, n, mbrows, nmb)
    seen = []
    for staged in (False, True):
        o = _prep_buffers(h, n, nmb, d, vrms)
        scratch = Banded(need, dtype=torch.float64, init=np.zeros(need))
        assert _prep_call(case, vd, rd, od, vrms, o, scratch, staged) == 0
        bands(key, scratch, *o.values())
        seen.append({k: b.t.clone() for k, b in o.items()})
    assert all(torch.equal(seen[0][k], seen[1][k]) for k in seen[0]), key
    for i in range(nmb):
        mom, mbar = R.moments(obs[i * mbrows:(i + 1) * mbrows])
        check(key, "obs_mom%d" % i, o["obs_mom"].t[i * (2 * d + 1):(i + 1) * (2 * d + 1)], mom, mbar)
    if not nmb:
        assert o["obs_mom"].untouched()
    for name, src in (("val_mom", values), ("ret_mom", returns)):
        mom, mbar = R.moments(src.reshape(-1, 1))
        check(key, name, o[name], mom, mbar)
    if vrms is None:
        exact(key, "old_values", o["old_values"], values.T.reshape(-1))      # copies, transposed
        exact(key, "ds_returns", o["ds_returns"], returns.T.reshape(-1))
        assert all(o[k].untouched() for k in ("vmean", "vvar", "vcount"))
    else:
        check(key, "old_values", o["old_values"], r64["old_values"], R.bar(r64["old_values"], r32["old_values"]))
        check(key, "ds_returns", o["ds_returns"], r64["returns"], R.bar(r64["returns"], r32["returns"]))
        one = lambda x: np.array([x], F64)
        bm1, bv1 = R.rms_apply_bars(one(vrms[0]), one(vrms[1]), vrms[2], r64["val_mom"])
        mid = R.rms_apply(one(vrms[0]), one(vrms[1]), vrms[2], r64["val_mom"])
        bm2, bv2 = R.rms_apply_bars(mid[0], mid[1], mid[2], r64["ret_mom"])
        check(key, "vmean", o["vmean"], [r64["vrms"][0]], bm1 + bm2)
        check(key, "vvar", o["vvar"], [r64["vrms"][1]], bv1 + bv2)
        exact(key, "vcount", o["vcount"], [r64["vrms"][2]])
    if const and vrms is None:
        exact(key, "advantages", o["advantages"], r64["advantages"])          # 0.5 in every row; normalised: (0.5 - 0.5) / (0 + 1e-8) = 0
    else:
        check(key, "advantages", o["advantages"], r64["advantages"], R.bar(r64["advantages"], r32["advantages"]))


@pytest.mark.parametrize("what,h,n,nmb,d,short,code", R.PREP_REFUSED, ids=[r[0] for r in R.PREP_REFUSED])
def test_dataset_prep_refusals(what, h, n, nmb, d, short, code):
    """H N = 100 rows: -3; 9 minibatches, 65 observations, a scratch one double short: -1; every output untouched"""
    case = (h, n, nmb, d, 4, True, True, False)
    values, returns, obs, vrms = R.prep_data(case)
    o = _prep_buffers(h, n, nmb, d, vrms)
    need = R.prep_scratch_doubles(h, n, 4, nmb) - short
    scratch = Banded(need, dtype=torch.float64)
    assert _prep_call(case, dev(values), dev(returns), dev(obs), vrms, o, scratch, False) == code
    torch.cuda.synchronize()
    assert scratch.untouched() and all(o[k].untouched() for k in ("obs_mom", "val_mom", "ret_mom", "old_values", "ds_returns", "advantages"))
    assert [float(o[k].t[0]) for k in ("vmean", "vvar", "vcount")] == list(vrms[:3]) and all(o[k].band_untouched() for k in ("vmean", "vvar", "vcount"))


# ---------------------------------------------------------------------------------------------------------------- gradient norm, optimiser
def _adam_launch(b, hp, mode, tails, adapt):
    """one bez_ppo_adam_step on the buffers `b` in the norm mode `mode`; returns the shares tensor (mode 'shares')"""
    from bez_isaacgym_amd.ppo import fused as F
    n = b["p"].n
    kw, shares = {}, None
    if mode == "shares":
        units = n // 4 + n % 4
        shares = Guarded((units + 1023) // 1024, 2)
        view = F.grad_norm_parts(b["g"].t, shares.t)
        assert view.shape[0] == shares.n
        kw["norm_parts"] = view
    elif mode == "grid":
        kw["grid_norm"] = b["grid"].t
    packed = None if b["packed"] is None else types.SimpleNamespace(hflat=b["p16"].t, map_a=b["map_a"], map_b=b["map_b"], flat=b["packed"].t)
    F.adam_step(b["p"].t, b["g"].t, b["m"].t, b["v"].t, b["steps"].t, b["lr"].t, (hp["beta1"], hp["beta2"]), hp["eps"], hp["weight_decay"], hp["max_norm"],
                b["scale"].t, b["tracker"].t, hp["growth"], hp["backoff"], hp["interval"], b["work"].t, params_f16=b["p16"].t,
                tail=[(d.t, s.t, a) for (d, s), a in zip(b["tails"], tails)], adapt=None if adapt is None else (b["kl"].t,) + tuple(adapt), packed=packed,
                grad_div=hp["grad_div"], **kw)
    torch.cuda.synchronize()
    assert not b["work"].t.any() and (mode != "grid" or int(b["grid"].t[512:513].view(torch.int32)) == 0)      # the ticket and the arrival counter are back at 0
    return shares


@pytest.mark.parametrize("case", R.adam_cases(), ids=lambda c: "n%d-%s-%d" % c)
def test_grad_norm_parts_and_adam_step(case):
    """bez_ppo_grad_norm_parts and bez_ppo_adam_step in its three norm modes (in-launch, shares, the grid meeting point where adam_grid_fits says it may
    run): a clean step with the norm above max_norm, then one launch for each place an inf / a NaN is planted at -- the first element, the last, the
    middle and, for n > 2 x 256 x 1024, one that only the capped grid's loop reaches -- each skipped: p, m, v, the fp16 copy, the packed copies and the
    step counters bit-unchanged, the scale backed off, the tracker cleared.  The switches (ppo_glue_ref.adam_hp) turn independently of the norm mode."""
    from bez_isaacgym_amd.ppo import fused as F
    n, mode, idx = case
    key = "adam n%d-%s-%d" % case
    if mode == "grid" and not F.adam_grid_fits(n):
        pytest.skip("the launch's workgroups are not all resident on this device: bez_ppo_adam_step would refuse the meeting point with -6")
    hp = dict(R.adam_hp(idx), overflow_skips=mode != "launch")
    p, g, m, v = R.adam_data(n, idx)
    tails = [0.5, 2.0, -1.0, 0.25][:hp["ntail"]]
    tail_vals = [(1.0 + i, 3.0 - i) for i in range(hp["ntail"])]
    adapt = (0.008, 1e-6, 1e-2) if idx % 2 == 0 else None
    kl = 0.1 if idx % 4 == 0 else 0.001
    with_packed = idx % 2 == 0
    rng = np.random.default_rng(idx)
    ma, mb = rng.permutation(n).astype(np.int32), (n + rng.permutation(n)).astype(np.int32)
    ma[::7], mb[::5] = -1, -1
    ma[-1] = -1        # (for n > 524288: an index only the capped loop reaches)
    b = dict(p=Banded(n, init=p), g=Banded(n, init=g), m=Banded(n, init=m), v=Banded(n, init=v), p16=Banded(n, dtype=torch.float16, init=p.astype(F16)),
             steps=Banded(hp["nsteps"], init=np.full(hp["nsteps"], 3.0, F32)), lr=Banded(1, init=[3e-4]), scale=Banded(1, init=[1024.0]),
             tracker=Banded(1, dtype=torch.int32, init=np.array([1], np.int32)), work=Banded(F.ADAM_WORK_FLOATS, init=np.zeros(F.ADAM_WORK_FLOATS)),
             grid=Banded(F.ADAM_GRIDNORM_FLOATS, init=np.zeros(F.ADAM_GRIDNORM_FLOATS)), kl=Banded(1, init=[kl]),
             tails=[(Banded(1, init=[d]), Banded(1, init=[s])) for d, s in tail_vals],
             packed=Banded(2 * n, dtype=torch.float16, init=np.full(2 * n, 3.0, F16)) if with_packed else None, map_a=dev(ma), map_b=dev(mb))
    st = dict(p=p, m=m, v=v, step=3.0, lr=3e-4, scale=1024.0, tracker=1)
    hp["tail"] = [(d, s, a) for (d, s), a in zip(tail_vals, tails)]
    hp["adapt"] = None if adapt is None else (kl,) + adapt

    def all_bands():
        bands(key, *[x for x in b.values() if isinstance(x, Guarded)], *[y for pair in b["tails"] for y in pair])

    # ---- a clean step
    shares = _adam_launch(b, hp, mode, tails, adapt)
    if shares is not None:
        s64, s32, bad = R.norm_parts(g)
        got = host(shares)
        check(key, "shares", got[:, 0], s64, R.bar(s64, s32))
        exact(key, "shares-nonfinite", got[:, 1], bad.astype(F64))
        bands(key, shares)
    r64, r32 = R.adam(st, g, hp), R.adam(st, g, hp, dt=F32)
    assert not r64["skipped"] and r64["norm"] > 1.0
    for k in ("p", "m", "v"):
        check(key, k, b[k], r64[k], R.bar(r64[k], r32[k]))

    def check_copies(tag):
        p16 = b["p16"].t.cpu().numpy()
        exact(key, tag + "p16", p16.astype(F64), b["p"].t.half().cpu().numpy().astype(F64))       # the fp16 cast of the parameter the launch stored
        if with_packed:
            want = np.full(2 * n, 3.0, F16)
            want[ma[ma >= 0]] = p16[ma >= 0]
            want[mb[mb >= 0]] = p16[mb >= 0]
            exact(key, tag + "packed", b["packed"], want.astype(F64))
    check_copies("")
    exact(key, "steps", b["steps"], np.full(hp["nsteps"], 4.0))
    exact(key, "scale", b["scale"], [r64["scale"]])
    assert int(b["tracker"].t[0]) == r64["tracker"]
    check(key, "lr", b["lr"], [r64["lr"]], R.bar([r64["lr"]], [r32["lr"]]))
    for i, (dst, src) in enumerate(b["tails"]):
        check(key, "tail%d" % i, dst, [r64["tail"][i]], R.bar([r64["tail"][i]], [r32["tail"][i]]))
        exact(key, "tail-src%d" % i, src, [tail_vals[i][1]])
    all_bands()

    # ---- a non-finite gradient: the step is skipped, wherever the element sits (one launch per position, inf and NaN in turn)
    before = {k: b[k].t.clone() for k in ("p", "m", "v", "p16", "steps")}
    packed_before = b["packed"].t.clone() if with_packed else None
    st2 = {k: r64[k] for k in st}
    st2.update(p=host(b["p"]), m=host(b["m"]), v=host(b["v"]))
    for q, pos in enumerate(R.adam_bad_positions(n)):
        tag = "skip@%d-" % pos
        g2 = g.copy()
        g2[pos] = np.inf if (idx + q) % 2 else np.nan
        b["g"].t.copy_(dev(g2))
        st2.update(lr=float(b["lr"].t[0]), scale=float(b["scale"].t[0]), tracker=int(b["tracker"].t[0]))
        hp["tail"] = [(float(dst.t[0]), s, a) for (dst, _), (_, s), a in zip(b["tails"], tail_vals, tails)]
        shares = _adam_launch(b, hp, mode, tails, adapt)
        if shares is not None:
            exact(key, tag + "shares-nonfinite", host(shares)[:, 1], R.norm_parts(g2)[2].astype(F64))
        q64, q32 = R.adam(st2, g2, hp), R.adam(st2, g2, hp, dt=F32)
        assert q64["skipped"]
        for k, t in before.items():
            assert torch.equal(b[k].t, t), (key, pos, "skipped step changed", k)
        assert packed_before is None or torch.equal(b["packed"].t, packed_before), (key, pos)
        exact(key, tag + "scale", b["scale"], [q64["scale"]])
        assert float(b["scale"].t[0]) == st2["scale"] * 0.5 and int(b["tracker"].t[0]) == 0 and q64["tracker"] == 0, (key, pos)
        check(key, tag + "lr", b["lr"], [q64["lr"]], R.bar([q64["lr"]], [q32["lr"]]))
        for i, (dst, _) in enumerate(b["tails"]):
            check(key, tag + "tail%d" % i, dst, [q64["tail"][i]], R.bar([q64["tail"][i]], [q32["tail"][i]]))
        all_bands()
    REPORT[key]["skipped"] = "bit-unchanged"


@pytest.mark.parametrize("mode", R.ADAM_MODES)
def test_adam_step_norm_beyond_fp32(mode):
    """a finite gradient whose squared norm overflows fp32: the share and meeting-point modes skip the step (the kernel's comment: 'a share that
    overflowed'); the in-launch mode does what torch does with an infinite norm -- the clip coefficient is 0, the step is taken with no gradient"""
    from bez_isaacgym_amd.ppo import fused as F
    n = 9
    if mode == "grid" and not F.adam_grid_fits(n):
        pytest.skip("the launch's workgroups are not all resident on this device")
    key = "adam overflow-%s" % mode
    hp = dict(R.adam_hp(0), overflow_skips=mode != "launch", ntail=0, tail=[], adapt=None)
    p, _, m, v = R.adam_data(n, 0)
    g = np.full(n, 1e30, F32)
    b = dict(p=Banded(n, init=p), g=Banded(n, init=g), m=Banded(n, init=m), v=Banded(n, init=v), p16=Banded(n, dtype=torch.float16, init=p.astype(F16)),
             steps=Banded(1, init=[3.0]), lr=Banded(1, init=[3e-4]), scale=Banded(1, init=[1.0]), tracker=Banded(1, dtype=torch.int32, init=np.array([0], np.int32)),
             work=Banded(F.ADAM_WORK_FLOATS, init=np.zeros(F.ADAM_WORK_FLOATS)), grid=Banded(F.ADAM_GRIDNORM_FLOATS, init=np.zeros(F.ADAM_GRIDNORM_FLOATS)),
             kl=Banded(1), tails=[], packed=None, map_a=None, map_b=None)
    _adam_launch(b, hp, mode, [], None)
    st = dict(p=p, m=m, v=v, step=3.0, lr=3e-4, scale=1.0, tracker=0)
    r64, r32 = R.adam(st, g, hp), R.adam(st, g, hp, dt=F32)
    assert r64["skipped"] == (mode != "launch")
    for k in ("p", "m", "v"):
        if r64["skipped"]:
            exact(key, k, b[k], st[k])
        else:
            check(key, k, b[k], r64[k], R.bar(r64[k], r32[k]))
    exact(key, "steps", b["steps"], [3.0 if r64["skipped"] else 4.0])
    exact(key, "scale", b["scale"], [r64["scale"]])
    bands(key, *[x for x in b.values() if isinstance(x, Guarded)])


def test_adaptive_lr_and_abi():
    """bez_ppo_adaptive_lr on both sides of both thresholds and at both limits; bez_ppo_abi_version is the binding's"""
    from bez_isaacgym_amd.ppo import fused as F
    assert int(lib().bez_ppo_abi_version()) == F.PPO_ABI_VERSION
    for lr, kl in ((3e-4, 0.1), (3e-4, 0.001), (3e-4, 0.008), (3e-4, 0.016), (3e-4, 0.004), (1e-6, 0.1), (1e-2, 0.0), (1.2e-6, 0.1), (9e-3, 0.0)):
        key = "adaptive_lr lr%g-kl%g" % (lr, kl)
        l, k = Banded(1, init=[lr]), Banded(1, init=[kl])
        F.adaptive_lr(l.t, k.t, 0.008, 1e-6, 1e-2)
        r64, r32 = R.both(R.adaptive_lr, lr, kl, 0.008, 1e-6, 1e-2)
        check(key, "lr", l, [r64], R.bar([r64], [r32]))
        bands(key, l, k)
