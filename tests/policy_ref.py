"""fp64 references, derived error bounds and test data of the MFMA policy kernels (csrc/bez_policy.hip, csrc/bez_wgrad.hip) for
tests/test_gpu_policy_envelope.py; tests/test_policy_ref_cpu.py checks this module and its data without a GPU.  numpy only.

The reference applies the kernels' rounding points to an fp64 evaluation and nothing else: fp16 input tile, exact fp16 x fp16 products
summed in fp64, fp16 rounding of every pre-activation and of every ELU output, fp16 head outputs read as fp32; backwards
gz_L = fp16(g_L elu'(y_L)), g_(L-1) = fp16(gz_L W_L), head input g = fp16(gmu16 W_mu + gv16 W_v).

Two kinds of data.  INTEGER: sparse {-1, 0, 1} weights, small integer inputs, biases that keep every pre-activation >= 0, backward
activations from {-0.5, 0, 1, 2}: every intermediate is an fp16 number and every fp32 partial sum is exact, so a kernel must match
the reference bit for bit whatever its summation order.  RANDOM: Gaussian weights and data; what separates a kernel from the
reference is then (i) the order of an fp32 sum of K terms, at most K 2^-24 sum |terms|, (ii) the flip of an fp16 rounding that
follows from it, one fp16 ulp, and (iii) what the next layer makes of both: forwards the carried error times the layer's row-sum
norm, backwards times its column-sum norm (|elu'| <= 1 adds no gain).  Every bound is computed from the case's own weights and data."""
import numpy as np

# (num_obs, units, actions); which kernel template each selects follows the host rule of csrc/bez_policy.hip:
#   tile 0 holds the input and the outputs of the odd layers (forward) / the head tile and d/d h_L for L = nhid - 2, nhid - 4, ... (backward);
#   w0 = its widest tenant, narrow = pad16(w0) + 8 <= 216 -> strides <216, 424>, two workgroups per CU; otherwise <424, 424>.
#   Plain forward / rollout_step at n <= 8192 rows: <MODE, 424, 424, packed, 32 rows> (small_batch), row-major: <MODE, 424, 424, false, 64 rows>.
NETS = {
    "A": (54, (400, 200, 100), 18),            # fwd w0 = max(54, 200) = 200, bwd w0 = max(32, 200) = 200: narrow <216, 424>; the yaml shape
    "B": (54, (400, 208, 100), 18),            # w0 = 208: pad16 = 208, 208 + 8 = 216: the last narrow width <216, 424>
    "C": (54, (400, 210, 100), 18),            # w0 = 210: pad16 = 224: the first wide width <424, 424>; 210 % 4 = 2: the backward's column-pair path
    "D": (54, (256, 256, 128), 18),            # w0 = 256: wide <424, 424> forward and backward
    "E": (54, (416,), 31),                     # one layer: fwd w0 = 54, bwd w0 = 32: narrow <216, 424>, tile 1 holds the 416 columns; value = head column 31
    "F": (6, (32, 32, 32, 32, 32, 32), 1),     # six layers of the backward's minimum width: w0 = 32, narrow <216, 424>
    "G": (416, (64, 34), 18),                  # fwd w0 = max(416, 34) = 416: wide <424, 424> because of the input; bwd w0 = max(32, 64) = 64: narrow; 34 is even only
    "H": (54, (400, 400, 200, 100), 18),       # fwd w0 = max(54, 400, 100) = 400, bwd w0 = max(32, 400, 400) = 400: wide <424, 424>
}
N_MAX = 130                                    # rows of every case's data; a test of n rows takes the first n
TRAIN_ROWS = (1, 63, 64, 65, 130)
FWD_ROWS = (1, 33, 130)
FULL = ("C", "D", "E")                         # full cross product of rows x weight layout x data mode; the others: see cases()

WGRAD_ROWS = (64, 128, 192, 320, 448)
WGRAD_SETS = {                                 # [(out, in)] of the Linears whose weight gradients one launch forms
    "w416": [(416, 416)],
    "w32": [(32, 32), (31, 32), (1, 32)],
    "yaml": [(400, 54), (200, 400), (100, 200), (18, 100), (1, 100)],
    "w34": [(34, 416), (64, 34)],
}

ULP16 = 2.0 ** -10     # relative spacing of fp16
EPS32 = 2.0 ** -24     # unit roundoff of fp32
TINY16 = 2.0 ** -14    # smallest normal fp16: below it the spacing is 2^-24 = ULP16 * TINY16


def cases(rows):
    """[(net, n, packed, mode)]: nets C, D, E at every row count, layout and mode; the others with fragment-major weights at n = 1
    and 65 in both modes plus one row-major case."""
    out = []
    for net in NETS:
        if net in FULL:
            out += [(net, n, pk, mode) for n in rows for pk in (False, True) for mode in ("integer", "random")]
        else:
            edge = (1, 65) if 65 in rows else (rows[0], rows[-1])
            out += [(net, n, True, mode) for n in edge for mode in ("integer", "random")]
            out.append((net, rows[-1], False, "random"))
    return out


def case_id(c):
    return "%s-n%d-%s-%s" % (c[0], c[1], "packed" if c[2] else "rowmajor", c[3])


def _ulp(mag):
    """upper estimate of the fp16 spacing at magnitudes `mag`: 2^-10 |v| (>= the true 2^(floor(log2 |v|) - 10)), 2^-24 below the normal range.
    Two numbers that differ by d round to fp16 numbers that differ by at most d + this."""
    return ULP16 * np.maximum(mag, TINY16)


def f16(x):
    """round to fp16, back as fp64"""
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def shapes_of(net):
    d, units, a = NETS[net] if isinstance(net, str) else net
    dims = [d] + list(units)
    return [(dims[i + 1], dims[i]) for i in range(len(units))] + [(a, dims[-1]), (1, dims[-1])]


def flat_layout(net):
    """[(weight offset, out, in, bias offset)] of the Linears in the flat fp16 working copy (hidden layers, mu head, value head: weight then
    bias, nothing in between -- the agent's own layout, so a head's weight may start on an odd element), and its size"""
    off, lay = 0, []
    for o, k in shapes_of(net):
        lay.append((off, o, k, off + o * k))
        off += o * k + o
    return lay, off


def _sparse(rng, o, k, nnz):
    """(o, k) matrix with min(nnz, k) entries of +-1 per row"""
    nnz = min(nnz, k)
    cols = np.argsort(rng.random((o, k)), axis=1)[:, :nnz]
    w = np.zeros((o, k))
    np.put_along_axis(w, cols, rng.choice([-1.0, 1.0], size=(o, nnz)), axis=1)
    return w


_DATA = {}


def data(net, mode):
    """The case's weights and inputs (made once, never modified): W / b = fp64 copies of the fp16 weights / biases in network order, flat = the
    fp16 working copy, obs (N_MAX, d) fp32, gmu (N_MAX, A) / gval (N_MAX, 1) fp32, acts = fp16-valued activations for the backward chain
    (integer mode: supplied directly; random mode: None -- the backward starts from the activations the forward under test stored)."""
    key = (net, mode)
    if key not in _DATA:
        _DATA[key] = _make_integer(net) if mode == "integer" else _make_random(net)
    return _DATA[key]


def _pack(net, W, b, **kw):
    lay, total = flat_layout(net)
    flat = np.zeros(total, dtype=np.float16)
    for (wo, o, k, bo), w, bb in zip(lay, W, b):
        flat[wo:wo + o * k] = w.reshape(-1)
        flat[bo:bo + o] = bb
    W = [f16(w) for w in W]
    b = [f16(x) for x in b]
    for a in W + b + [flat] + [v for v in kw.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return dict(net=net, W=W, b=b, flat=flat, **kw)


def _make_random(net):
    d, units, a = NETS[net]
    rng = np.random.default_rng(1000 + sorted(NETS).index(net))
    W = [rng.standard_normal((o, k)) / np.sqrt(k) for o, k in shapes_of(net)]
    b = [rng.standard_normal(o) * 0.1 for o, _ in shapes_of(net)]
    obs = (rng.standard_normal((N_MAX, d)) * 1.5).astype(np.float32)
    gmu = (rng.standard_normal((N_MAX, a)) * 1e-2).astype(np.float32)
    gval = (rng.standard_normal((N_MAX, 1)) * 1e-2).astype(np.float32)
    return _pack(net, W, b, obs=obs, gmu=gmu, gval=gval, acts=None)


def _make_integer(net):
    """Sparse +-1 weights with the most entries per row (4, 3, 2, 1) at which every intermediate of the forward AND of the backward chain is an
    fp16 number; the biases of the hidden layers are 1 - (the smallest pre-activation of the column), so every pre-activation is >= 1 (ELU is
    the identity) and a dropped bias shows."""
    d, units, a = NETS[net]
    nh = len(units)
    for nnz in (4, 3, 2, 1):
        rng = np.random.default_rng(2000 + 10 * sorted(NETS).index(net) + nnz)
        W = [_sparse(rng, o, k, nnz) for o, k in shapes_of(net)]
        obs = rng.integers(-2, 3, (N_MAX, d)).astype(np.float32)
        b, h = [], obs.astype(np.float64)
        for L in range(nh):
            z = h @ W[L].T
            b.append(1.0 - z.min(0))
            h = z + b[-1]
        b += [rng.integers(-3, 4, a).astype(np.float64), rng.integers(-3, 4, 1).astype(np.float64)]
        gmu = rng.integers(-2, 3, (N_MAX, a)).astype(np.float32)
        gval = rng.integers(-2, 3, (N_MAX, 1)).astype(np.float32)
        acts = [rng.choice([-0.5, 0.0, 1.0, 2.0], size=(N_MAX, w)) for w in units]
        dat = _pack(net, W, b, obs=obs, gmu=gmu, gval=gval, acts=acts, nnz=nnz)
        if not inexact_points(forward(dat, N_MAX)) and not inexact_points(backward(dat, acts, gmu, gval)):
            return dat
    return dat   # (tests/test_policy_ref_cpu.py fails on it and names the rounding point)


def forward(dat, n, x16=None):
    """fp64 forward of the first n rows with the kernels' rounding points.  x0: the fp16 input tile; z[L] / y[L]: pre-activation and ELU output,
    both as rounded to fp16; mu, value: the heads' fp16 outputs; raw: (name, value before its rounding, value after) of every rounding point;
    err[L] (n, width): bound on |kernel - reference| of layer L's stored activations; mu_bound / value_bound: of the head outputs."""
    W, b = dat["W"], dat["b"]
    nh = len(W) - 2
    x0 = f16(dat["obs"][:n]) if x16 is None else np.asarray(x16, dtype=np.float64)
    raw = [("x0", dat["obs"][:n].astype(np.float64), x0)] if x16 is None else []
    h, zs, ys, errs = x0, [], [], []
    err = np.zeros_like(x0)                        # bound on |kernel - reference| of the layer's input, per element
    for L in range(nh):
        zr = h @ W[L].T + b[L]                     # exact products, fp64 sums
        z = f16(zr)
        er = np.where(z > 0, z, np.expm1(z))
        y = f16(er)
        raw += [("z%d" % L, zr, z), ("y%d" % L, er, y)]
        k = W[L].shape[1]
        # (i) the order of the fp32 sum of k products and the bias, on the kernel's own inputs (|h| + err); (iii) the carried error through |W|
        # (element by element: never more than the largest carried error times the row-sum norm)
        dz = err @ np.abs(W[L]).T + (k + 1) * EPS32 * ((np.abs(h) + err) @ np.abs(W[L]).T + np.abs(b[L]))
        dz = dz + _ulp(np.abs(zr) + dz)            # (ii) the fp16 rounding of the pre-activation
        # ELU is convex and increasing: over [z - dz, z + dz] its slope is at most the slope at the right end; then the fp16 rounding of its
        # output, and 2^-22 for the kernel's fp32 exp (v_exp_f32 on z log2(e), 1 - that: absolute errors of a few 2^-24 below |y| <= 1)
        slope = np.exp(np.minimum(z + dz, 0.0))
        err = slope * dz + _ulp(np.abs(y) + slope * dz) + 2.0 ** -22
        zs.append(z); ys.append(y); errs.append(err)
        h = y
    out = dict(x0=x0, z=zs, y=ys, err=errs, raw=raw)
    for name, i in (("mu", nh), ("value", nh + 1)):
        zr = h @ W[i].T + b[i]
        v = f16(zr)
        raw.append((name, zr, v))
        k = W[i].shape[1]
        dz = err @ np.abs(W[i]).T + (k + 2) * EPS32 * ((np.abs(h) + err) @ np.abs(W[i]).T + np.abs(b[i]))   # (the bias is added to the fp32 sum: one more rounding)
        out[name] = v
        out[name + "_bound"] = dz + _ulp(np.abs(zr) + dz)
    return out


def backward(dat, acts, gmu, gval):
    """fp64 backward chain of the rows of `acts` (fp16-valued activations, the kernel's own in the GPU tests) from gmu / gval (fp32).
    gmu16 / gv16: the fp16 head gradients (exact roundings of the inputs: no bound, they must be equal); gz[L]: d loss / d pre-activation of
    layer L as stored; gz_bound[L] (n, width); raw as forward()."""
    W = dat["W"]
    nh = len(W) - 2
    acts = [np.asarray(a, dtype=np.float64) for a in acts]
    n = acts[0].shape[0]
    gmu16, gv16 = f16(gmu[:n]), f16(gval[:n]).reshape(n, 1)
    raw = [("gmu16", np.asarray(gmu[:n], dtype=np.float64), gmu16), ("gv16", np.asarray(gval[:n], dtype=np.float64).reshape(n, 1), gv16)]
    gr = gmu16 @ W[nh] + gv16 @ W[nh + 1]
    g = f16(gr)
    raw.append(("g%d" % (nh - 1), gr, g))
    # the head product runs over the 32 padded head columns
    e = 32 * EPS32 * (np.abs(gmu16) @ np.abs(W[nh]) + np.abs(gv16) @ np.abs(W[nh + 1]))
    e = e + _ulp(np.abs(gr) + e)
    gz, bounds = [None] * nh, [None] * nh
    for L in range(nh - 1, -1, -1):
        y = acts[L]
        d = np.where(y > 0, 1.0, y + 1.0)
        zr = g * d
        gz[L] = f16(zr)
        raw.append(("gz%d" % L, zr, gz[L]))
        e = e * np.abs(d)                              # |elu'| <= 1: no gain (the activations are the kernel's own: no error in d)
        e = e + _ulp(np.abs(zr) + e)                   # one ulp for the rounding of the stored gz
        bounds[L] = e
        if L > 0:
            gr = gz[L] @ W[L]
            g = f16(gr)
            raw.append(("g%d" % (L - 1), gr, g))
            k = W[L].shape[0]
            # the carried error through |W| down the columns (never more than the largest one times the column-sum norm) + the fp32 sum's order
            e = e @ np.abs(W[L]) + k * EPS32 * ((np.abs(gz[L]) + e) @ np.abs(W[L]))
            e = e + _ulp(np.abs(gr) + e)
    return dict(gmu16=gmu16, gv16=gv16, gz=gz, gz_bound=bounds, raw=raw)


def colsum(x16):
    """(fp64 column sums, bound of an fp32 sum of the same rows in any order) of fp16-valued rows"""
    x = np.asarray(x16, dtype=np.float64)
    return x.sum(0), x.shape[0] * EPS32 * np.abs(x).sum(0)


def inexact_points(ref):
    """names of the rounding points of a reference at which rounding changed a value (integer mode: none)"""
    return [name for name, before, after in ref["raw"] if not np.array_equal(before, after)]


def forward_fp32(dat, n):
    """plain fp32 numpy evaluation of the forward with the same rounding points: (x0, [y_L], mu, value)"""
    W, b = [w.astype(np.float32) for w in dat["W"]], [x.astype(np.float32) for x in dat["b"]]
    nh = len(W) - 2
    r16 = lambda v: v.astype(np.float16).astype(np.float32)
    h = r16(dat["obs"][:n])
    x0, ys = h, []
    for L in range(nh):
        z = r16(h @ W[L].T + b[L])
        h = r16(np.where(z > 0, z, np.expm1(z)))
        ys.append(h)
    return x0, ys, r16(h @ W[nh].T + b[nh]), r16(h @ W[nh + 1].T + b[nh + 1])


def backward_fp32(dat, acts, gmu, gval):
    """plain fp32 numpy evaluation of the backward chain: (gmu16, gv16, [gz_L])"""
    W = [w.astype(np.float32) for w in dat["W"]]
    nh = len(W) - 2
    n = acts[0].shape[0]
    r16 = lambda v: v.astype(np.float16).astype(np.float32)
    gmu16, gv16 = r16(gmu[:n]), r16(gval[:n]).reshape(n, 1)
    g = r16(gmu16 @ W[nh] + gv16 @ W[nh + 1])
    gz = [None] * nh
    for L in range(nh - 1, -1, -1):
        y = np.asarray(acts[L], dtype=np.float32)
        gz[L] = r16(g * np.where(y > 0, np.float32(1), y + np.float32(1)))
        if L > 0:
            g = r16(gz[L] @ W[L])
    return gmu16, gv16, gz


# ---- weight gradients: dW_L = base_L + dY_L^T X_L

_WDATA = {}


def wgrad_data(name, rows, mode):
    """[(dy (rows, out) fp16, x (rows, in) fp16, base (out, in) fp32)] per layer of the set; integer mode: small integers (the construction of
    test_wgrad_mfma_matches_fp32_reference), so base + product is exact in fp32 in any order"""
    key = (name, rows, mode)
    if key not in _WDATA:
        rng = np.random.default_rng(3000 + 100 * sorted(WGRAD_SETS).index(name) + rows + (mode == "integer"))
        out = []
        for o, i in WGRAD_SETS[name]:
            if mode == "integer":
                dy = rng.integers(-2, 3, (rows, o)).astype(np.float16)
                x = (rng.integers(-2, 3, (rows, i)) + (np.arange(i) % 3 == 0)).astype(np.float16)
                base = rng.integers(-8, 9, (o, i)).astype(np.float32)
            else:
                dy = (rng.standard_normal((rows, o)) * 1e-2).astype(np.float16)
                x = rng.standard_normal((rows, i)).astype(np.float16)
                base = rng.standard_normal((o, i)).astype(np.float32)
            for a in (dy, x, base):
                a.setflags(write=False)
            out.append((dy, x, base))
        _WDATA[key] = out
    return _WDATA[key]


def wgrad_ref(dy, x, base=None):
    """(fp64 dY^T X (+ base), bound of an fp32 sum of the same rows' products (and the base) in any order: terms x 2^-24 x sum |terms|)"""
    dy, x = dy.astype(np.float64), x.astype(np.float64)
    ref, mag, terms = dy.T @ x, np.abs(dy).T @ np.abs(x), dy.shape[0]
    if base is not None:
        ref, mag, terms = ref + base.astype(np.float64), mag + np.abs(base.astype(np.float64)), terms + 1
    return ref, terms * EPS32 * mag


# ---- what the kernels refuse: (what, num_obs, units, actions) for the policy entry points

REFUSED = [
    ("forward", 54, (418, 100), 18),                      # a width past the LDS tiles
    ("forward", 54, (64,) * 7, 18),                       # seven hidden layers
    ("forward", 54, (64, 64), 32),                        # no padded head column left for the value
    ("train_forward", 54, (64, 33), 18),                  # an odd width: the stored activations leave as half2
    ("train_forward", 53, (64, 64), 18),                  # an odd observation width: x0 leaves as half2
    ("backward", 54, (64, 30), 18),                       # fewer than 32 columns of K for the 16-byte fragment reads
]
