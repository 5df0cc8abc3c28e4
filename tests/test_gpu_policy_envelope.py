"""The MFMA policy kernels (csrc/bez_policy.hip policy_forward_kernel / policy_backward_kernel, csrc/bez_wgrad.hip wgrad_kernel and the
second-stage reductions) across the shape range their host gates accept, against the fp64 references of tests/policy_ref.py: integer data
bit for bit, random data within bounds derived from the case's own weights and data (never a chosen tolerance, no excluded element).
Every output is allocated with a band of sentinel rows behind row n, so a tail overrun shows as a wrong number.  The networks, the kernel
template each selects and the row counts are the tables of tests/policy_ref.py; DESIGN.md 4.4 states the envelope.

BEZ_ENVELOPE_REPORT=<file>: the worst observed error / derived bound of every case is written there (profiles/policy_envelope_errors.txt)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import policy_ref as R
from tests.gpu_util import DEV, GUARD, Guarded, SENT

pytestmark = pytest.mark.gpu
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("BEZ_ENVELOPE_REPORT")
    if path and REPORT:
        with open(path, "a") as f:
            for key in sorted(REPORT):
                f.write("%-44s %s\n" % (key, "  ".join("%s=%s" % kv for kv in REPORT[key].items())))


def _check(key, name, got, ref, bound, mode):
    """integer: equal; random: |got - ref| <= bound everywhere; the worst ratio is printed before it is asserted and kept for the report"""
    got = (got.np() if isinstance(got, Guarded) else got.double().cpu().numpy()).reshape(ref.shape)
    rec = REPORT.setdefault(key, {})
    if mode == "integer":
        bad = np.argwhere(got != ref)
        assert bad.size == 0, "%s %s: %d mismatches, first at %s: got %s, want %s" % (key, name, len(bad), bad[:4].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
        rec[name] = "exact"
        return
    diff = np.abs(got - ref)
    bound = np.broadcast_to(bound, ref.shape)
    ratio = float((diff / np.maximum(bound, 1e-300)).max()) if diff.max() > 0 else 0.0
    rec[name] = "%.3f" % ratio
    print("%s %s: worst |error| / bound = %.3f (max |error| %.3e)" % (key, name, ratio, diff.max()))
    assert (diff <= bound).all(), (key, name, ratio, np.argwhere(diff > bound)[:4].tolist())


@functools.lru_cache(maxsize=None)
def _net(net, mode):
    """the case's flat fp16 working copy on the device, its views, both weight layouts' launchers"""
    from bez_isaacgym_amd.ppo import fused as F
    dat = R.data(net, mode)
    d, units, a = R.NETS[net]
    lay, _ = R.flat_layout(net)
    hflat = torch.from_numpy(dat["flat"].copy()).to(DEV)
    views = [(hflat[wo:wo + o * k].view(o, k), hflat[bo:bo + o]) for wo, o, k, bo in lay]
    layout = [(wo, o, k) for wo, o, k, _ in lay]
    nh = len(units)
    packed = F.PackedWeights(hflat, layout, a)
    ns = types.SimpleNamespace(dat=dat, d=d, units=units, a=a, nh=nh, hflat=hflat, views=views, layout=layout, packed=packed, fwd={}, bwd={})
    for pk in (None, packed):
        ns.fwd[pk is not None] = F.PolicyForward(views[:nh], views[nh], views[nh + 1], None, pk)
        ns.bwd[pk is not None] = F.PolicyBackward(hflat, layout, a, pk)
        ns.bwd[pk is not None].refresh()
    ns.obs = torch.from_numpy(dat["obs"].copy()).to(DEV)
    ns.gmu = torch.from_numpy(dat["gmu"].copy()).to(DEV)
    ns.gval = torch.from_numpy(dat["gval"].copy()).to(DEV)
    torch.cuda.synchronize()
    return ns


@functools.lru_cache(maxsize=None)
def _ref_forward(net, mode, n):
    return R.forward(R.data(net, mode), n)


def _check_forward(key, ref, mode, mu, val, acts=None, x0=None):
    _check(key, "mu", mu, ref["mu"], ref["mu_bound"], mode)
    _check(key, "value", val, ref["value"], ref["value_bound"], mode)
    if x0 is not None:
        assert np.array_equal(x0.np(), ref["x0"]), (key, "x0")     # the fp16 rounding of the fp32 input: no freedom in either mode
        for L, a in enumerate(acts):
            _check(key, "act%d" % L, a, ref["y"][L], ref["err"][L], mode)
    for g in [mu, val] + ([x0] + list(acts) if x0 is not None else []):
        assert g.band_untouched(), key


@pytest.mark.parametrize("case", R.cases(R.FWD_ROWS), ids=R.case_id)
def test_forward_and_rollout_step(case):
    """bez_ppo_policy_forward against the reference, and bez_ppo_policy_rollout_step = that forward + bez_ppo_rollout_pre: the same mu / value /
    action / sigma / observation rows bit for bit; neglogp within the order of its fp32 sum of A + 2 terms."""
    from bez_isaacgym_amd.ppo import fused as F
    net, n, pk, mode = case
    key = "fwd " + R.case_id(case)
    N = _net(net, mode)
    ref = _ref_forward(net, mode, n)
    obs = N.obs[:n].contiguous()
    pf = N.fwd[pk]
    mu, val = Guarded(n, N.a), Guarded(n, 1)
    pf(obs, mu.t, val.t)
    torch.cuda.synchronize()
    _check_forward(key, ref, mode, mu, val)
    g = torch.Generator(device=DEV); g.manual_seed(100 + n)
    logstd = torch.randn(N.a, device=DEV, generator=g) * 0.3 - 0.5
    noise = torch.randn(n, N.a, device=DEV, generator=g)
    dones = (torch.rand(n, device=DEV, generator=g) < 0.3).float()
    shapes = dict(mb_obs=(n, N.d), mb_dones=(n,), mb_mu=(n, N.a), mb_val=(n, 1), act=(n, N.a), env_act=(n, N.a), neglogp=(n,), sigma=(n, N.a))
    want, got = ({k: Guarded(*s) for k, s in shapes.items()} for _ in range(2))
    order = ("mb_obs", "mb_dones", "mb_mu", "mb_val", "act", "env_act", "neglogp", "sigma")
    F.rollout_pre(mu.t, val.t, logstd, noise, obs, dones, None, *[want[k].t for k in order])
    pf.rollout_step(obs, logstd, noise, dones, None, *[got[k].t for k in order])
    torch.cuda.synchronize()
    for k in order:
        assert got[k].band_untouched() and want[k].band_untouched(), (key, k)
        if k != "neglogp":
            assert torch.equal(got[k].t, want[k].t), (key, k)
    assert torch.equal(got["mb_mu"].t, mu.t) and torch.equal(got["mb_val"].t, val.t) and torch.equal(got["mb_obs"].t, obs)
    # neglogp = 0.5 sum q^2 + 0.5 log(2 pi) A + sum log sigma: A + 2 terms (and the halving), summed in fp32 in either launch's order
    q = ((want["act"].t - want["mb_mu"].t) / want["sigma"].t).double()
    mag = 0.5 * (q * q).sum(1) + 0.5 * np.log(2 * np.pi) * N.a + float(logstd.double().abs().sum())
    diff = (got["neglogp"].t.double() - want["neglogp"].t.double()).abs()
    bound = (N.a + 3) * R.EPS32 * mag
    print("%s neglogp: worst |difference| / bound = %.3f" % (key, float((diff / bound).max())))
    assert bool((diff <= bound).all()), key


def _loss_partials(n, a, seed):
    """a real bez_ppo_loss(defer_reduce) on n rows: (scratch with the per-workgroup partials, fp64 sums of its columns, their bounds)"""
    from bez_isaacgym_amd.ppo import fused as F
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    mu, logstd, value = rn(n, a) * 0.8, rn(a) * 0.3 - 1.0, rn(n, 1)
    old_sigma = torch.exp(logstd + 0.05 * rn(a)).expand(n, a).contiguous()
    old_mu = (mu + 0.05 * rn(n, a)).contiguous()
    mb = dict(actions=(old_mu + old_sigma * rn(n, a)).contiguous(), old_logp=rn(n) + 10.0, advantages=rn(n), old_values=rn(n, 1), returns=rn(n, 1),
              mu=old_mu, sigma=old_sigma)
    scratch = F.loss_scratch(n, a, DEV)
    gmu, gval = torch.empty(n, a, device=DEV), torch.empty(n, 1, device=DEV)
    glog, stats = Guarded(a), Guarded(5)
    F.loss(mu, logstd, value, mb, 0.2, 2.0, 0.01, 0.001, True, None, gmu, gval, glog.t, stats.t, scratch=scratch, defer_reduce=True)
    torch.cuda.synchronize()
    assert glog.untouched() and stats.untouched()     # deferred: the partials only
    nb = (n + 63) // 64
    parts = scratch[2:2 + nb * (a + 5)].double().cpu().numpy().reshape(a + 5, nb)
    assert np.abs(parts).max() > 0
    return scratch, parts.sum(1), nb * R.EPS32 * np.abs(parts).sum(1)


@functools.lru_cache(maxsize=None)
def _tiny_wgrad():
    """a one-block weight-gradient plan whose partial images ride along where a test is about grad_reduce_all's other parts"""
    from bez_isaacgym_amd.ppo import fused as F
    (dy, x, _), = R.wgrad_data("w416", 64, "integer")
    dy, x = torch.from_numpy(dy[:, :32].copy()).to(DEV), torch.from_numpy(x[:, :32].copy()).to(DEV)
    grad = Guarded(32, 32)
    wg = F.WgradMfma([dy], [x], [grad.t])
    assert wg.ok
    return wg, grad, dy.double().cpu().numpy().T @ x.double().cpu().numpy()


@pytest.mark.parametrize("case", R.cases(R.TRAIN_ROWS), ids=R.case_id)
def test_train_forward_and_backward(case):
    """bez_ppo_policy_forward_train (mu, value, x0 and every stored activation) and bez_ppo_policy_backward, plain and deferred +
    bez_ppo_grad_reduce_all: every gz, gmu16, gv16 and every bias gradient against the reference chain started from the activations the
    backward was given (random mode: the forward's own, so forward rounding does not leak into the backward bounds)."""
    from bez_isaacgym_amd.ppo import fused as F
    net, n, pk, mode = case
    key = "train " + R.case_id(case)
    N = _net(net, mode)
    dat = N.dat
    obs = N.obs[:n].contiguous()
    x0 = Guarded(n, N.d, torch.float16)
    acts = [Guarded(n, w, torch.float16) for w in N.units]
    mu, val = Guarded(n, N.a), Guarded(n, 1)
    N.fwd[pk].train_forward(obs, x0.t, [a.t for a in acts], mu.t, val.t)
    torch.cuda.synchronize()
    _check_forward(key, _ref_forward(net, mode, n), mode, mu, val, acts, x0)

    acts_np = [a[:n] for a in dat["acts"]] if mode == "integer" else [a.np() for a in acts]
    acts_dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV).half() for a in acts_np]
    gmu, gval = N.gmu[:n].contiguous(), N.gval[:n].contiguous()
    ref = R.backward(dat, acts_np, dat["gmu"], dat["gval"])
    pb = N.bwd[pk]

    def run(defer):
        o = dict(gz=[Guarded(n, w, torch.float16) for w in N.units], gmu16=Guarded(n, N.a, torch.float16), gv16=Guarded(n, 1, torch.float16),
                 bias=[Guarded(w) for w in N.units], bmu=Guarded(N.a), bv=Guarded(1))
        if not defer:   # the plain call ADDS the column sums to the bias gradients
            for b in o["bias"] + [o["bmu"], o["bv"]]:
                b.t.zero_()
        pb(gmu, gval, acts_dev, [z.t for z in o["gz"]], o["gmu16"].t, o["gv16"].t, [b.t for b in o["bias"]], o["bmu"].t, o["bv"].t, defer_reduce=defer)
        return o
    plain = run(False)
    torch.cuda.synchronize()
    deferred = run(True)
    torch.cuda.synchronize()
    assert all(b.untouched() for b in deferred["bias"] + [deferred["bmu"], deferred["bv"]]), key      # deferred: the partials only
    wg, wgrad, wref = _tiny_wgrad()
    assert wg(reduce=False)
    scratch, lsum, lbound = _loss_partials(n, N.a, 7 * n + N.a)
    glog, stats = Guarded(N.a), Guarded(5)
    wgrad.full.fill_(SENT)
    F.grad_reduce_all(wg, pb, [b.t for b in deferred["bias"]], deferred["bmu"].t, deferred["bv"].t, n, scratch, glog.t, stats.t, accumulate=False)
    torch.cuda.synchronize()
    for tag, o in (("", plain), ("deferred ", deferred)):
        k2 = key if not tag else key.replace("train ", "train-deferred ")
        assert np.array_equal(o["gmu16"].np(), ref["gmu16"]) and np.array_equal(o["gv16"].np(), ref["gv16"]), k2   # exact roundings of the inputs
        for L in range(N.nh):
            _check(k2, "gz%d" % L, o["gz"][L], ref["gz"][L], ref["gz_bound"][L], mode)
            # bias gradient = column sums of the gz the kernel stored
            s, bound = R.colsum(o["gz"][L].np())
            _check(k2, "bias%d" % L, o["bias"][L], s, bound, mode)
            if mode == "integer":
                assert np.array_equal(o["bias"][L].np(), ref["gz"][L].sum(0)), (k2, L)
        for name, src in (("bmu", "gmu16"), ("bv", "gv16")):
            s, bound = R.colsum(ref[src])
            _check(k2, name, o[name], s, bound, mode)
        for g in o["gz"] + [o["gmu16"], o["gv16"]] + o["bias"] + [o["bmu"], o["bv"]]:
            assert g.band_untouched(), k2
    for a, b in zip(plain["gz"], deferred["gz"]):     # the same launch: the same bits in either mode
        assert torch.equal(a.t, b.t), key
    # the other two parts of the one-launch reduction: the loss kernel's partials (fp64 sum of the scratch's own numbers) and the split-K images
    got = np.concatenate([glog.np(), stats.np()])
    diff = np.abs(got - lsum)
    print("%s loss sums: worst |error| / bound = %.3f" % (key, float((diff / np.maximum(lbound, 1e-300)).max())))
    assert (diff <= lbound).all() and glog.band_untouched() and stats.band_untouched(), key
    assert np.array_equal(wgrad.np(), wref) and wgrad.band_untouched(), key


@functools.lru_cache(maxsize=None)
def _reduce_partner():
    """net F's deferred backward and a deferred loss at 64 rows: the bias and loss parts grad_reduce_all needs beside a weight-gradient plan"""
    N = _net("F", "integer")
    n, pb = 64, N.bwd[True]
    acts = [torch.from_numpy(a[:n].copy()).to(DEV).half() for a in N.dat["acts"]]
    gz = [torch.empty(n, w, device=DEV, dtype=torch.float16) for w in N.units]
    bias = [torch.zeros(w, device=DEV) for w in N.units]
    bmu, bv = torch.zeros(N.a, device=DEV), torch.zeros(1, device=DEV)
    pb(N.gmu[:n].contiguous(), N.gval[:n].contiguous(), acts, gz, torch.empty(n, N.a, device=DEV, dtype=torch.float16),
       torch.empty(n, 1, device=DEV, dtype=torch.float16), bias, bmu, bv, defer_reduce=True)
    scratch, _, _ = _loss_partials(n, N.a, 5)
    want = [R.backward(N.dat, [a[:n] for a in N.dat["acts"]], N.dat["gmu"], N.dat["gval"])["gz"][L].sum(0) for L in range(N.nh)]
    return pb, n, bias, bmu, bv, scratch, want


@pytest.mark.parametrize("rows", R.WGRAD_ROWS)
@pytest.mark.parametrize("name", sorted(R.WGRAD_SETS))
def test_wgrad_short_reductions(name, rows):
    """wgrad_kernel with 1, 2, 3, 5 and 7 reduction stages (the planner clips the splits to the stage count; ragged and single-stage splits):
    accumulate onto a base, overwrite (twice: the same bits) and partial images + bez_ppo_grad_reduce_all, each against the fp64 product."""
    from bez_isaacgym_amd.ppo import fused as F
    pb, prow, pbias, pbmu, pbv, pscratch, pwant = _reduce_partner()
    for mode in ("integer", "random"):
        key = "wgrad %s-rows%d-%s" % (name, rows, mode)
        layers = R.wgrad_data(name, rows, mode)
        dys = [torch.from_numpy(dy.copy()).to(DEV) for dy, _, _ in layers]
        xs = [torch.from_numpy(x.copy()).to(DEV) for _, x, _ in layers]
        grads = [Guarded(*base.shape) for _, _, base in layers]
        for g, (_, _, base) in zip(grads, layers):
            g.t.copy_(torch.from_numpy(base.copy()))
        wg = F.WgradMfma(dys, xs, [g.t for g in grads])
        assert wg.ok, key
        assert wg(accumulate=True)
        torch.cuda.synchronize()
        for L, (g, (dy, x, base)) in enumerate(zip(grads, layers)):
            _check(key, "acc%d" % L, g, *R.wgrad_ref(dy, x, base), mode)
        refs = [R.wgrad_ref(dy, x) for dy, x, _ in layers]
        outs = []
        for _ in range(2):
            for g in grads:
                g.full.fill_(SENT)
            assert wg(accumulate=False)
            torch.cuda.synchronize()
            outs.append([g.t.clone() for g in grads])
        assert all(torch.equal(a, b) for a, b in zip(*outs)), key
        for L, (g, (ref, bound)) in enumerate(zip(grads, refs)):
            _check(key, "write%d" % L, g, ref, bound, mode)
        for g in grads:
            g.full.fill_(SENT)
        assert wg(reduce=False)
        torch.cuda.synchronize()
        assert all(g.untouched() for g in grads), key      # the partial images only
        glog, stats = Guarded(pb.A), Guarded(5)
        F.grad_reduce_all(wg, pb, pbias, pbmu, pbv, prow, pscratch, glog.t, stats.t, accumulate=False)
        torch.cuda.synchronize()
        for L, (g, (ref, bound)) in enumerate(zip(grads, refs)):
            _check(key, "reduce_all%d" % L, g, ref, bound, mode)
            assert torch.equal(g.t, outs[0][L]) or mode == "random", key
            assert g.band_untouched(), key
        assert all(np.array_equal(b.double().cpu().numpy(), w) for b, w in zip(pbias, pwant)), key


def _refused(call):
    with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
        call()


def test_refused_shapes_are_declined_before_any_launch():
    """What the host gates decline (-1 / -3 / False, before any launch): outputs stay untouched, and the agent's gate
    (a2c_continuous.policy_kernel_gate) declines the same shapes."""
    from bez_isaacgym_amd.ppo import fused as F
    from bez_isaacgym_amd.ppo.a2c_continuous import policy_kernel_gate
    n = 64
    h16 = lambda *s: torch.zeros(*s, device=DEV, dtype=torch.float16)

    def net(d, units, a):
        dims = [d] + list(units)
        hidden = [(h16(dims[i + 1], dims[i]), h16(dims[i + 1])) for i in range(len(units))]
        return F.PolicyForward(hidden, (h16(a, dims[-1]), h16(a)), (h16(1, dims[-1]), h16(1)), None)
    for what, d, units, a in R.REFUSED:
        assert policy_kernel_gate(d, units, a)[what] is False, (what, d, units, a)
        obs = torch.zeros(n, d, device=DEV)
        outs = [Guarded(n, a), Guarded(n, 1)]
        if what == "forward":
            pf = net(d, units, a)
            _refused(lambda: pf(obs, outs[0].t, outs[1].t))
            # the other two entry points share the gate
            roll = [Guarded(n, d), Guarded(n), Guarded(n, a), Guarded(n, 1), Guarded(n, a), Guarded(n, a), Guarded(n), Guarded(n, a)]
            _refused(lambda: pf.rollout_step(obs, torch.zeros(a, device=DEV), torch.zeros(n, a, device=DEV), torch.zeros(n, device=DEV), None, *[g.t for g in roll]))
            outs += roll
        if what in ("forward", "train_forward"):
            pf = net(d, units, a)
            tr = [Guarded(n, d, torch.float16)] + [Guarded(n, w, torch.float16) for w in units]
            _refused(lambda: pf.train_forward(obs, tr[0].t, [g.t for g in tr[1:]], outs[0].t, outs[1].t))
            outs += tr
        if what == "backward":
            # (the Python constructor asserts the same widths: built on a width the kernel takes, then handed the refused one)
            ok = (64, 32)
            lay, total = R.flat_layout((d, ok, a))
            pb = F.PolicyBackward(h16(total), [(wo, o, k) for wo, o, k, _ in lay], a)
            pb.widths = list(units)
            pb.c_widths = (type(pb.c_widths))(*units)
            o = [Guarded(n, w, torch.float16) for w in units] + [Guarded(n, a, torch.float16), Guarded(n, 1, torch.float16)] + [Guarded(w) for w in units] + \
                [Guarded(a), Guarded(1)]
            nh = len(units)
            _refused(lambda: pb(torch.zeros(n, a, device=DEV), torch.zeros(n, 1, device=DEV), [h16(n, w) for w in units], [g.t for g in o[:nh]], o[nh].t,
                                o[nh + 1].t, [g.t for g in o[nh + 2:2 * nh + 2]], o[-2].t, o[-1].t))
            outs += o
        torch.cuda.synchronize()
        assert all(g.untouched() for g in outs), (what, d, units, a)
    # 32 actions: the loss kernel takes them, the policy kernels and the one-launch reduction do not -- the agent's gate follows the policy kernels
    assert policy_kernel_gate(54, (64, 64), 32)["forward"] is False and policy_kernel_gate(54, (64, 64), 31)["forward"] is True

    # the fused loss + backward launch exists for 18 actions on the narrow fragment-major tiles only: -3, the wrapper says False
    for d, units, a in ((54, (400, 200, 100), 7), R.NETS["D"]):
        lay, total = R.flat_layout((d, units, a))
        layout = [(wo, o, k) for wo, o, k, _ in lay]
        hflat = h16(total)
        pb = F.PolicyBackward(hflat, layout, a, F.PackedWeights(hflat, layout, a))
        z = lambda *s: torch.zeros(*s, device=DEV)
        mb = dict(actions=z(n, a), old_logp=z(n), advantages=z(n), old_values=z(n, 1), returns=z(n, 1), mu=z(n, a), sigma=torch.ones(n, a, device=DEV))
        ops = F.LossOperands.of(z(n, a), z(a), z(n, 1), mb, 0.2, 2.0, 0.0, 0.001, True, None, False, F.loss_scratch(n, a, DEV))
        o = [Guarded(n, w, torch.float16) for w in units] + [Guarded(n, a, torch.float16), Guarded(n, 1, torch.float16)] + [Guarded(w) for w in units] + \
            [Guarded(a), Guarded(1)]
        nh = len(units)
        assert pb.with_loss(ops, [h16(n, w) for w in units], [g.t for g in o[:nh]], o[nh].t, o[nh + 1].t, [g.t for g in o[nh + 2:2 * nh + 2]], o[-2].t,
                            o[-1].t) is False
        torch.cuda.synchronize()
        assert all(g.untouched() for g in o), (d, units, a)

    # weight gradients: whole 64-row stages only
    grad = Guarded(32, 32)
    wg = F.WgradMfma([h16(100, 32)], [h16(100, 32)], [grad.t])
    assert not wg.ok and wg(accumulate=False) is False
    torch.cuda.synchronize()
    assert grad.untouched()
