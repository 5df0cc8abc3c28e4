"""The references, bounds and data of tests/policy_ref.py checked on their own (no GPU): every integer-mode case is exactly representable at
every rounding point, a plain fp32 numpy evaluation of every random case stays inside the derived bounds, and the agent's kernel gate
declines the shapes the C entry points decline."""
import numpy as np
import pytest

from tests import policy_ref as R


@pytest.mark.parametrize("net", sorted(R.NETS))
def test_integer_data_is_exact_at_every_rounding_point(net):
    dat = R.data(net, "integer")
    fwd = R.forward(dat, R.N_MAX)
    assert R.inexact_points(fwd) == []
    assert all(float(z.min()) >= 1.0 for z in fwd["z"])                    # ELU is the identity, and no bias is zero
    assert all(np.array_equal(z, y) for z, y in zip(fwd["z"], fwd["y"]))
    bwd = R.backward(dat, dat["acts"], dat["gmu"], dat["gval"])
    assert R.inexact_points(bwd) == []
    # the data exercises what it is meant to: both ELU branches backwards, non-trivial gradients in every layer, fp32-exact column sums
    assert all(float((np.asarray(a) < 0).mean()) > 0.1 and float((np.asarray(a) > 0).mean()) > 0.1 for a in dat["acts"])
    assert all(float(np.abs(g).max()) > 0 for g in bwd["gz"]) and float(np.abs(fwd["mu"]).max()) > 0
    for g in bwd["gz"] + [bwd["gmu16"], bwd["gv16"]]:
        s, _ = R.colsum(g)
        assert np.array_equal(s, g.astype(np.float32).sum(0, dtype=np.float32).astype(np.float64))
    # the flat working copy holds the same numbers
    lay, total = R.flat_layout(net)
    assert dat["flat"].size == total
    for (wo, o, k, bo), w, b in zip(lay, dat["W"], dat["b"]):
        assert np.array_equal(dat["flat"][wo:wo + o * k].reshape(o, k).astype(np.float64), w)
        assert np.array_equal(dat["flat"][bo:bo + o].astype(np.float64), b)


@pytest.mark.parametrize("net", sorted(R.NETS))
def test_fp32_evaluation_of_the_random_data_stays_inside_the_derived_bounds(net):
    dat = R.data(net, "random")
    n = R.N_MAX
    ref = R.forward(dat, n)
    x0, ys, mu, val = R.forward_fp32(dat, n)
    assert np.array_equal(x0.astype(np.float64), ref["x0"])
    for L, y in enumerate(ys):
        assert (np.abs(y - ref["y"][L]) <= ref["err"][L]).all(), L
    assert (np.abs(mu - ref["mu"]) <= ref["mu_bound"]).all() and (np.abs(val - ref["value"]) <= ref["value_bound"]).all()
    assert float(min((y < 0).mean() for y in ys)) > 0.2           # the negative ELU branch is covered
    # worst-case bounds grow with every layer they pass; where the chains start they are far below the size of the numbers
    assert float(ref["err"][0].max()) < 0.01 * float(np.abs(ref["y"][0]).max())
    bwd = R.backward(dat, ys, dat["gmu"], dat["gval"])
    gmu16, gv16, gz = R.backward_fp32(dat, ys, dat["gmu"], dat["gval"])
    assert np.array_equal(gmu16, bwd["gmu16"]) and np.array_equal(gv16, bwd["gv16"])
    assert float(bwd["gz_bound"][-1].max()) < 0.01 * float(np.abs(bwd["gz"][-1]).max())
    for L, g in enumerate(gz):
        assert (np.abs(g - bwd["gz"][L]) <= bwd["gz_bound"][L]).all(), L
        s, bound = R.colsum(g)
        assert (np.abs(g.sum(0, dtype=np.float32) - s) <= bound).all()


@pytest.mark.parametrize("name", sorted(R.WGRAD_SETS))
def test_wgrad_data_and_bound(name):
    for rows in R.WGRAD_ROWS:
        for dy, x, base in R.wgrad_data(name, rows, "integer"):
            ref, _ = R.wgrad_ref(dy, x, base)
            assert float(np.abs(ref).max()) < 2 ** 24 and np.array_equal(ref, np.round(ref))    # exact in fp32 in any order
        for dy, x, base in R.wgrad_data(name, rows, "random"):
            ref, bound = R.wgrad_ref(dy, x, base)
            got = base + dy.astype(np.float32).T @ x.astype(np.float32)
            assert (np.abs(got - ref) <= bound).all()
            assert float(bound.max()) < 1e-3 * float(np.abs(ref).max())


def test_case_table():
    for rows in (R.TRAIN_ROWS, R.FWD_ROWS):
        cs = R.cases(rows)
        assert len(set(cs)) == len(cs) and {c[0] for c in cs} == set(R.NETS)
        for net in R.FULL:
            assert sum(c[0] == net for c in cs) == len(rows) * 4
        assert all(c[1] <= R.N_MAX for c in cs)
    assert max(R.WGRAD_ROWS) <= 448 and all(r % 64 == 0 for r in R.WGRAD_ROWS)


def test_agent_gate_declines_what_the_kernels_decline():
    from bez_isaacgym_amd.ppo.a2c_continuous import policy_kernel_gate
    for d, units, a in R.NETS.values():
        assert policy_kernel_gate(d, units, a) == dict(forward=True, train_forward=True, backward=True)
    for what, d, units, a in R.REFUSED:
        assert policy_kernel_gate(d, units, a)[what] is False, (what, d, units, a)
    assert policy_kernel_gate(54, (64, 30), 18) == dict(forward=True, train_forward=True, backward=False)
    assert policy_kernel_gate(53, (64, 33), 18) == dict(forward=True, train_forward=False, backward=False)
