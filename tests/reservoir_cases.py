"""Shared builders of the reservoir edge tests (tests/test_gpu_reservoir_edges.py on the device, tests/test_oracle_reservoir.py
for the checker and the inputs themselves): models with non-square layouts, per-variable z sizes, mask dtypes and directly
supplied sparse structure; the restatement's increment with scipy's stored-entry semantics or a dense product, chosen
explicitly; and the checker that compares the class of every element (NaN, +Inf, -Inf, finite) before the finite values.

The arithmetic stays ``reservoir_np``'s: numpy in the real dtypes of the sources and masks, so float32 * float32 rounds to
float32 and anything with a float64 operand does not, by numpy's own promotion.
"""
import zlib

import numpy as np

import reservoir_np as R

STATE_GATE = 1e-13       # the state, absolute
OUTPUT_GATE_F64 = 1e-12  # float64 outputs, times max|y|; float32 outputs: one ulp of the expected value

NON_FINITE = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}

# the suite's 2304-input shape (test_large_shapes_match_restatement) couples with 0.05; larger inputs scale it by
# 1 / sqrt(n_in), which keeps the spread of a row's sum, and so the meaning of the state gate, where it is there
COUPLING_AT_2304 = 0.05


def coupling_for(n_in):
    return COUPLING_AT_2304 * np.sqrt(2304.0 / n_in) if n_in > 2304 else COUPLING_AT_2304


# ---------------------------------------------------------------------------------------------
# sparse structure
# ---------------------------------------------------------------------------------------------


def dense_of(csr):
    """The dense matrix of (indptr, indices, data, shape), duplicates summed."""
    indptr, idx, val, shape = csr
    w = np.zeros(shape)
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    np.add.at(w, (rows, idx), val)
    return w


def stored_of(csr):
    """[row, col] True where an entry is stored (an explicit zero included)."""
    indptr, idx, _, shape = csr
    stored = np.zeros(shape, bool)
    stored[np.repeat(np.arange(shape[0]), np.diff(indptr)), idx] = True
    return stored


def csr_from_coo(rows, cols, vals, shape):
    """CSR in the given order of the entries within each row (stable), duplicates kept."""
    rows, cols, vals = np.asarray(rows), np.asarray(cols), np.asarray(vals, np.float64)
    order = np.argsort(rows, kind="stable")
    indptr = np.zeros(shape[0] + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=shape[0]), out=indptr[1:])
    return indptr, cols[order].astype(np.int32), vals[order], tuple(shape)


def bounded_w_res(rng, size, density):
    """A random W_res whose rows sum to at most 0.9 in magnitude (spectral radius <= 0.9) without a dense eigenproblem."""
    indptr, idx, val, shape = R.random_csr(rng, size, size, density, 1.0)
    rows = np.repeat(np.arange(size), np.diff(indptr))
    row_sum = np.bincount(rows, weights=np.abs(val), minlength=size).max() if val.size else 0.0
    return indptr, idx, val * (0.9 / row_sum if row_sum > 0 else 1.0), shape


def with_empty_rows(csr, rows):
    """The matrix with the stored entries of ``rows`` removed."""
    indptr, idx, val, shape = csr
    r = np.repeat(np.arange(shape[0]), np.diff(indptr))
    keep = ~np.isin(r, rows)
    return csr_from_coo(r[keep], idx[keep], val[keep], shape)


def with_unsorted_columns(rng, csr):
    """The same matrix with the entries of every row in a random order."""
    indptr, idx, val, shape = csr
    idx, val = idx.copy(), val.copy()
    for i in range(shape[0]):
        p = rng.permutation(indptr[i + 1] - indptr[i]) + indptr[i]
        idx[indptr[i]:indptr[i + 1]], val[indptr[i]:indptr[i + 1]] = idx[p], val[p]
    return indptr, idx, val, shape


def with_exact_nnz(rng, rows, cols, nnz, scale):
    """``nnz`` stored entries at random places of a [rows, cols] matrix."""
    flat = np.sort(rng.choice(rows * cols, nnz, replace=False))
    return csr_from_coo(flat // cols, flat % cols, rng.uniform(-scale, scale, nnz), (rows, cols))


def coo_with_duplicates(rng, rows, cols, density, scale, n_dup):
    """(COO arrays with ``n_dup`` of the entries stored twice, in a shuffled order; the CSR of the summed matrix)."""
    indptr, idx, val, shape = R.random_csr(rng, rows, cols, density, scale)
    r = np.repeat(np.arange(rows), np.diff(indptr))
    dup = rng.choice(val.size, n_dup, replace=False)
    extra = rng.uniform(-scale, scale, n_dup)
    summed = val.copy()
    summed[dup] += extra
    order = rng.permutation(val.size + n_dup)
    coo = {"row": np.concatenate([r, r[dup]])[order].astype(np.int32),
           "col": np.concatenate([idx, idx[dup]])[order].astype(np.int32),
           "data": np.concatenate([val, extra])[order], "format": np.array(b"coo"), "shape": np.array(shape, np.int64)}
    return coo, (indptr, idx, summed, shape)


# ---------------------------------------------------------------------------------------------
# the restatement, with the semantics of the W_in product chosen by the caller
# ---------------------------------------------------------------------------------------------


def product(v, csr, entries):
    """``v @ W.T`` in float64.  ``entries="stored"``: scipy's sparse product, which touches stored entries only -- a
    non-finite ``v[s, k]`` reaches row ``i`` only where ``W[i, k]`` is stored (an explicit zero then gives NaN).
    ``entries="dense"``: the product with the zero-filled matrix, where it reaches every row.  Written with numpy alone,
    so the result does not depend on whether scipy imports (tests/test_oracle_reservoir.py compares it with scipy's)."""
    if entries not in ("stored", "dense"):
        raise ValueError(f"entries must be 'stored' or 'dense', got {entries!r}")
    v = np.asarray(v)
    v = v.astype(np.result_type(v.dtype, np.float64), copy=False)
    w = dense_of(csr)
    with np.errstate(invalid="ignore", over="ignore"):
        if entries == "dense":
            return v @ w.T
        bad = ~np.isfinite(v)
        if not bad.any():
            return v @ w.T
        x = np.where(bad, 0.0, v) @ w.T
        stored = stored_of(csr)
        for s, k in np.argwhere(bad):
            i = np.nonzero(stored[:, k])[0]
            x[s, i] += v[s, k] * w[i, k]
        return x


def masked_input(m, arrays):
    """The encoding times the masks, [subdomain, input], in the dtype numpy's own promotion gives it."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = R.blocks(R.encode(m["input"], arrays), m["layout"], m["overlap"])
        if m.get("input_mask") is not None:
            u = u * m["input_mask"]
    return u


def pre_activation(m, state, arrays, w_in="stored"):
    """(u @ W_in.T, state @ W_res.T)."""
    return product(masked_input(m, arrays), m["w_in"], w_in), product(state, m["w_res"], "stored")


def increment(m, state, arrays, w_in="stored"):
    """``reservoir_np.increment`` with the W_in product's semantics explicit; W_res is always walked as stored (the
    kernels keep it in CSR)."""
    a, b = pre_activation(m, state, arrays, w_in)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.tanh(a + b)


def predict(m, state, hybrid_arrays=None):
    """``reservoir_np.predict`` without numpy's warnings about the non-finite values passing through."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return R.predict(m, state, hybrid_arrays)


# ---------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------


def classes(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN per element."""
    a = np.asarray(a)
    return (np.isposinf(a) * 1 + np.isneginf(a) * 2 + np.isnan(a) * 3).astype(np.int8)


def check(got, want, gate, name=""):
    """(a) the map of {finite, +Inf, -Inf, NaN} of ``got`` equals ``want``'s, element for element; (b) where ``want`` is
    finite, |got - want| <= gate (a scalar or an array of want's shape).  A failure says how many elements differ and
    where the first one is.  Returns the worst |got - want| / gate."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    cg, cw = classes(got), classes(want)
    differ = np.argwhere(cg != cw)
    if differ.size:
        first = tuple(int(i) for i in differ[0])
        raise AssertionError(f"{name}: {len(differ)} of {want.size} elements differ in class (0 finite, 1 +Inf, 2 -Inf, "
                             f"3 NaN); first at {first}: got {cg[first]} ({got[first]}), want {cw[first]} ({want[first]})")
    finite = cw == 0
    gate = np.broadcast_to(np.asarray(gate, np.float64), want.shape)
    err = np.zeros(want.shape)
    err[finite] = np.abs(got[finite].astype(np.float64) - want[finite].astype(np.float64))
    over = np.argwhere(finite & ~(err <= gate))
    if over.size:
        first = tuple(int(i) for i in over[0])
        worst = tuple(int(i) for i in np.unravel_index(np.argmax(np.where(finite, err - gate, -np.inf)), want.shape))
        raise AssertionError(f"{name}: {len(over)} of {want.size} elements are outside the gate; first at {first}: got "
                             f"{got[first]!r}, want {want[first]!r}, |difference| {err[first]:.3e} > {gate[first]:.3e}; "
                             f"worst at {worst}: {err[worst]:.3e}")
    if not finite.any():
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / gate, 0.0)
    return float(ratio[finite].max())


def output_gate(want):
    """The gate of one decoded output: 1e-12 * max|y| over its finite part (float64), one ulp per element (float32)."""
    want = np.asarray(want)
    finite = np.isfinite(want)
    if want.dtype == np.float32:
        return np.where(finite, np.spacing(np.abs(np.where(finite, want, 0)).astype(np.float32)), 0).astype(np.float64)
    return OUTPUT_GATE_F64 * (np.abs(want[finite]).max() if finite.any() else 0.0)


def check_outputs(got, want, name=""):
    """``check`` over each decoded output with its own gate; dtypes and shapes must agree.  Returns the worst ratio."""
    assert len(got) == len(want), (name, len(got), len(want))
    worst = 0.0
    for v, (g, w) in enumerate(zip(got, want)):
        g = np.asarray(g)
        assert g.dtype == w.dtype, (name, v, g.dtype, w.dtype)
        worst = max(worst, check(g, w, output_gate(w), f"{name} output {v}"))
    return worst


# ---------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------


def _mask(rng, shape, dtype):
    """A mask with fractional values (a 0 / 1 mask multiplies exactly, which would hide a missing float32 rounding) and
    some zeros."""
    if dtype is None:
        return None
    m = rng.uniform(0.25, 1.75, shape)
    m[rng.random_sample(shape) < 0.1] = 0.0
    return m.astype(dtype)


def make_transformer(kind, rng, sizes, extent, mask_dtype=None):
    """``sizes``: the z size of each variable (equal for scale-spatial); ``mask_dtype``: None, np.float32 or np.float64."""
    sizes = [int(v) for v in sizes]
    if kind == "do-nothing":
        return {"kind": kind, "sizes": sizes}
    assert len(set(sizes)) == 1, "scale-spatial variables share one z size"
    n_var, nz = len(sizes), sizes[0]
    n = n_var * extent[0] * extent[1] * nz
    return {"kind": kind, "sizes": sizes, "spatial_features": (extent[0], extent[1], nz), "num_variables": n_var,
            "center": rng.randn(n).astype(np.float32), "scale": rng.uniform(0.5, 2.0, n).astype(np.float32),
            "mask": _mask(rng, (extent[0], extent[1], nz * n_var), mask_dtype)}


def make_model(rng, layout, sub, overlap=0, state_size=41, in_sizes=(1,), out_sizes=(1,), hybrid_sizes=None,
               in_kind="do-nothing", out_kind="do-nothing", hybrid_kind="do-nothing", in_tf_mask=None, out_tf_mask=None,
               hybrid_tf_mask=None, input_mask=None, hybrid_mask=None, square=False, w_in=None, w_res=None,
               w_in_density=1.0, w_res_density=0.2, coupling=None):
    """A restatement model.  ``layout`` and ``sub`` (cells per subdomain without overlap) may be non-square; the ``*_sizes``
    are per-variable z sizes; the ``*_mask`` arguments are dtypes (None: no mask); ``w_in`` / ``w_res`` may be given as
    (indptr, indices, data, shape)."""
    rank = (layout[0] * sub[0], layout[1] * sub[1])
    ov_ext = (rank[0] + 2 * overlap, rank[1] + 2 * overlap)
    ns = layout[0] * layout[1]
    m = {"layout": tuple(layout), "overlap": overlap, "rank": rank, "square": square,
         "input": make_transformer(in_kind, rng, in_sizes, ov_ext, in_tf_mask),
         "output": make_transformer(out_kind, rng, out_sizes, rank, out_tf_mask)}
    n_in = (sub[0] + 2 * overlap) * (sub[1] + 2 * overlap) * sum(in_sizes)
    scale = coupling_for(n_in) if coupling is None else coupling
    m["w_in"] = R.random_csr(rng, state_size, n_in, w_in_density, scale) if w_in is None else w_in
    m["w_res"] = bounded_w_res(rng, state_size, w_res_density) if w_res is None else w_res
    assert m["w_in"][3] == (state_size, n_in) and m["w_res"][3] == (state_size, state_size)
    m["input_mask"] = _mask(rng, (ns, n_in), input_mask)
    n_h = 0
    m["hybrid"], m["hybrid_mask"] = None, None
    if hybrid_sizes is not None:
        m["hybrid"] = make_transformer(hybrid_kind, rng, hybrid_sizes, rank, hybrid_tf_mask)
        n_h = sub[0] * sub[1] * sum(hybrid_sizes)
        m["hybrid_mask"] = _mask(rng, (ns, n_h), hybrid_mask)
    n_out = sub[0] * sub[1] * sum(out_sizes)
    m["coefficients"] = rng.randn(ns, state_size + n_h, n_out) / np.sqrt(state_size + n_h)
    m["intercepts"] = rng.randn(ns, n_out)
    return m


def n_in_of(m):
    return m["w_in"][3][1]


def ov_extent(m):
    return m["rank"][0] + 2 * m["overlap"], m["rank"][1] + 2 * m["overlap"]


def make_arrays(rng, sizes, extent, dtypes=np.float64, views="plain"):
    """One (x, y, z) array per variable.  ``dtypes``: one dtype, or one per variable; ``views``: "plain", "transposed" (an
    (x, y, z) view of a (z, y, x) array) or "strided" (every second y and all but the last z of a larger array), or one per
    variable."""
    n = len(sizes)
    dtypes = list(dtypes) if isinstance(dtypes, (list, tuple)) else [dtypes] * n
    views = list(views) if isinstance(views, (list, tuple)) else [views] * n
    out = []
    for nz, dtype, view in zip(sizes, dtypes, views):
        a = rng.randn(extent[0], extent[1], nz).astype(dtype)
        if view == "transposed":
            a = np.ascontiguousarray(a.transpose(2, 1, 0)).transpose(2, 1, 0)
        elif view == "strided":
            big = np.zeros((extent[0], 2 * extent[1], nz + 1), dtype)
            big[:, ::2, :nz] = a
            a = big[:, ::2, :nz]
        out.append(a)
    return out


def source_dtypes(kind, n):
    """"f32", "f64" or "mixed" (alternating, float32 first) for ``n`` variables."""
    return {"f32": [np.float32] * n, "f64": [np.float64] * n,
            "mixed": [np.float32 if v % 2 == 0 else np.float64 for v in range(n)]}[kind]


def package_model(m, state=None, storage=0, w_in=None, w_res=None):
    """The package's model of a restatement model (no files).  ``w_in`` / ``w_res``: a ``SparseMatrix`` to upload in place of
    the model's CSR arrays (COO with duplicates, say)."""
    from fv3net_amd.fit.reservoir import (HybridReservoirComputingModel, Reservoir, ReservoirComputingModel,
                                          ReservoirComputingReadout, TransformerGroup)
    from fv3net_amd.reservoir import DoNothingTransformer, RankXYDivider, ScaleSpatialConcatZTransformer, SparseMatrix

    def tf(t):
        if t["kind"] == "do-nothing":
            return DoNothingTransformer(t["sizes"])
        return ScaleSpatialConcatZTransformer(t["center"], t["scale"], t["spatial_features"], t["num_variables"], t.get("mask"))

    names = lambda t, p: [f"{p}{v}" for v in range(len(t["sizes"]))]  # noqa: E731
    divider = RankXYDivider(tuple(m["layout"]), m["overlap"], rank_extent=tuple(m["rank"]),
                            z_feature_size=sum(m["input"]["sizes"]))
    size = m["w_res"][3][0]
    res = Reservoir({"state_size": size}, m["w_in"][3][1], w_in or SparseMatrix.from_csr(*m["w_in"]),
                    w_res or SparseMatrix.from_csr(*m["w_res"]), input_mask_array=m.get("input_mask"), state=state)
    readout = ReservoirComputingReadout(m["coefficients"], m["intercepts"])
    hyb = m["hybrid"] if m["hybrid"] is not None else m["input"]
    tfs = TransformerGroup(tf(m["input"]), tf(m["output"]), tf(hyb))
    if m["hybrid"] is not None:
        return HybridReservoirComputingModel(names(m["input"], "i"), names(m["hybrid"], "h"), names(m["output"], "o"), res,
                                             readout, divider, tfs, square_half_hidden_state=m["square"],
                                             hybrid_input_mask=m.get("hybrid_mask"), w_in_storage=storage)
    return ReservoirComputingModel(names(m["input"], "i"), names(m["output"], "o"), res, readout, divider, tfs,
                                   square_half_hidden_state=m["square"], w_in_storage=storage)


# ---------------------------------------------------------------------------------------------
# the increment shapes of the device tests; tests/test_oracle_reservoir.py checks each one's summation-order condition
# ---------------------------------------------------------------------------------------------

# layout -> the subdomains per wave the plan must report (1, 2, <= 4, <= 8, <= 16, else 32); the groups of
# 3, 6, 9, 12, 33 and 36 subdomains are partial
LAYOUTS = {(1, 2): 2, (2, 1): 2, (3, 1): 4, (2, 3): 8, (3, 2): 8, (3, 3): 16, (3, 4): 16, (3, 11): 32, (6, 6): 32}
STATE_SIZES = (1, 2, 63, 127, 128, 129, 257)

# id -> z sizes of 16 do-nothing variables over 8 x 8 cells (sub 2 x 2, overlap 3) on a 16 x 16 layout, state 1000:
# 97 levels are 97 steps of 64 input rows, 50 levels 50 steps
MULTI_STEP = {"chunk192_short_last": [6] * 15 + [7], "chunk128_equal": [3] * 14 + [4] * 2}


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


def layout_case(layout, overlap):
    """Non-square rank (2 x 3 cells per subdomain), three do-nothing variables of z sizes 2, 1 and 3, a hybrid pair of z
    sizes 1 and 2, two outputs of z sizes 2 and 1: (model, state, inputs, hybrid inputs)."""
    rng = np.random.RandomState(_seed("layout", layout, overlap))
    m = make_model(rng, layout, (2, 3), overlap=overlap, state_size=41, in_sizes=(2, 1, 3), out_sizes=(2, 1),
                   hybrid_sizes=(1, 2), input_mask=np.float64, hybrid_mask=np.float64)
    ns = layout[0] * layout[1]
    state = rng.uniform(-1, 1, (ns, 41))
    return m, state, make_arrays(rng, (2, 1, 3), ov_extent(m)), make_arrays(rng, (1, 2), m["rank"])


def state_size_case(size):
    """Three subdomains (a partial group of four), 3 x 2 cells each with overlap 1, scale-spatial inputs."""
    rng = np.random.RandomState(_seed("state", size))
    m = make_model(rng, (3, 1), (3, 2), overlap=1, state_size=size, in_sizes=(2, 2), in_kind="scale-spatial",
                   in_tf_mask=np.float64, w_res_density=0.5)
    state = rng.uniform(-1, 1, (3, size))
    return m, state, make_arrays(rng, (2, 2), ov_extent(m), np.float32)


def multi_step_case(name):
    """The multi-step slices of the dense input product: 256 subdomains, 16 variables, state 1000, one output level."""
    sizes = MULTI_STEP[name]
    rng = np.random.RandomState(_seed("multi", name))
    m = make_model(rng, (16, 16), (2, 2), overlap=3, state_size=1000, in_sizes=sizes, out_sizes=(1,), w_res_density=0.003)
    state = rng.uniform(-1, 1, (256, 1000))
    return m, state, make_arrays(rng, sizes, ov_extent(m))


_CACHE = {}


def cached(build, *key):
    """A case and whatever was computed from it, built once per session and shared read-only."""
    k = (build.__name__,) + key
    if k not in _CACHE:
        _CACHE[k] = build(*key)
    return _CACHE[k]


# ---------------------------------------------------------------------------------------------
# dtypes: sources x transformer x mask
# ---------------------------------------------------------------------------------------------

SOURCES = ("f32", "f64", "mixed")
TRANSFORMERS = {"do-nothing": ("do-nothing", None), "scale-none": ("scale-spatial", None),
                "scale-f32": ("scale-spatial", np.float32), "scale-f64": ("scale-spatial", np.float64)}
MASKS = {"none": None, "f32": np.float32, "f64": np.float64}
VIEWS = ("plain", "transposed", "strided")


def dtype_case(sources, transformer, mask, hybrid):
    """Two by three subdomains of 2 x 3 cells, three variables of two levels; the dtypes under test on the input side
    (``hybrid`` False: overlap 1) or on the hybrid side.  (model, state, inputs, hybrid inputs or None); each variable of
    the side under test comes as another kind of view."""
    kind, tf_mask = TRANSFORMERS[transformer]
    rng = np.random.RandomState(_seed("dtype", sources, transformer, mask, hybrid))
    sizes = (2, 2, 2)
    if hybrid:
        m = make_model(rng, (2, 3), (2, 3), overlap=1, state_size=41, in_sizes=(1,), out_sizes=(1, 2), hybrid_sizes=sizes,
                       hybrid_kind=kind, hybrid_tf_mask=tf_mask, hybrid_mask=MASKS[mask], square=True)
    else:
        m = make_model(rng, (2, 3), (2, 3), overlap=1, state_size=41, in_sizes=sizes, in_kind=kind, in_tf_mask=tf_mask,
                       input_mask=MASKS[mask])
    state = rng.uniform(-1, 1, (6, 41))
    side = make_arrays(rng, sizes, m["rank"] if hybrid else ov_extent(m), source_dtypes(sources, 3), list(VIEWS))
    if hybrid:
        return m, state, make_arrays(rng, (1,), ov_extent(m)), side
    return m, state, side, None


# ---------------------------------------------------------------------------------------------
# non-finite values
# ---------------------------------------------------------------------------------------------

NF_LAYOUT, NF_SUB = (3, 4), (2, 3)       # 12 subdomains of 2 x 3 cells, overlap 1: the inputs cover 8 x 14 cells
NF_SHARED_CELL = (2, 3)                  # in the overlap of subdomains 0, 1, 3 and 4
NF_SHARED_BY = (0, 1, 3, 4)


def nf_model(rng, in_kind="do-nothing", in_tf_mask=None, input_mask=None, out_kind="do-nothing", w_in_density=1.0):
    return make_model(rng, NF_LAYOUT, NF_SUB, overlap=1, state_size=41, in_sizes=(2, 2), out_sizes=(2, 2),
                      hybrid_sizes=(1, 1), in_kind=in_kind, in_tf_mask=in_tf_mask, input_mask=input_mask, out_kind=out_kind,
                      out_tf_mask=np.float64 if out_kind != "do-nothing" else None, w_in_density=w_in_density)


def _flat_ids(m):
    """[subdomain, input] -> the (x, y, latent z) cell of the overlapped rank extent, flattened."""
    ext = ov_extent(m)
    zl = sum(m["input"]["sizes"])
    return R.blocks(np.arange(ext[0] * ext[1] * zl).reshape(ext[0], ext[1], zl), m["layout"], m["overlap"])


def input_cases():
    """id -> (model, state, clean inputs, planted inputs): non-finite values in the inputs of an increment, W_in fully
    stored (dense and CSR storage then agree with scipy's product)."""
    out = {}
    x, y = NF_SHARED_CELL
    for name, value in NON_FINITE.items():
        for where in ("overlap", "corner"):
            rng = np.random.RandomState(_seed("nf-input", where))
            m = nf_model(rng)
            state = rng.uniform(-1, 1, (12, 41))
            clean = make_arrays(rng, (2, 2), ov_extent(m))
            planted = [a.copy() for a in clean]
            if where == "overlap":
                planted[0][x, y, 1] = value
            else:
                planted[1][0, 0, 0] = value
            out[f"{where}-{name}"] = (m, state, clean, planted)
    # +Inf and -Inf meet in the rows of subdomain 0 whose two weights have the same sign
    rng = np.random.RandomState(_seed("nf-meet"))
    m = nf_model(rng)
    state = rng.uniform(-1, 1, (12, 41))
    clean = make_arrays(rng, (2, 2), ov_extent(m))
    planted = [a.copy() for a in clean]
    planted[0][0, 0, 0], planted[0][0, 1, 0] = np.inf, -np.inf
    out["inf-meets-inf"] = (m, state, clean, planted)
    # a mask of 0 on a NaN cell: 0 * NaN is NaN in numpy
    for which in ("input-mask", "transformer-mask"):
        rng = np.random.RandomState(_seed("nf-masked", which))
        m = nf_model(rng, in_kind="scale-spatial" if which == "transformer-mask" else "do-nothing",
                      in_tf_mask=np.float64 if which == "transformer-mask" else None,
                      input_mask=np.float64 if which == "input-mask" else None)
        state = rng.uniform(-1, 1, (12, 41))
        clean = make_arrays(rng, (2, 2), ov_extent(m))
        planted = [a.copy() for a in clean]
        planted[0][x, y, 1] = np.nan
        if which == "input-mask":
            cell = (x * ov_extent(m)[1] + y) * 4 + 1
            m["input_mask"][_flat_ids(m) == cell] = 0.0
        else:
            m["input"]["mask"][x, y, 1] = 0.0
        out[f"{which}-zero-on-nan"] = (m, state, clean, planted)
    # scale-spatial: float64 sources beyond float32's range become +-Inf in the float32 cast
    rng = np.random.RandomState(_seed("nf-range"))
    m = nf_model(rng, in_kind="scale-spatial", in_tf_mask=np.float64)
    state = rng.uniform(-1, 1, (12, 41))
    clean = make_arrays(rng, (2, 2), ov_extent(m))
    planted = [a.copy() for a in clean]
    m["input"]["mask"][x, y, 1] = 1.0
    m["input"]["mask"][7, 13, 2] = 1.0
    planted[0][x, y, 1] = 1.0e39
    planted[1][7, 13, 0] = -1.0e39
    out["beyond-float32"] = (m, state, clean, planted)
    # scale-spatial: a scale of exactly -1e-7f makes the denominator 0: +-Inf, and 0 / 0 where the source is the center
    rng = np.random.RandomState(_seed("nf-denominator"))
    m = nf_model(rng, in_kind="scale-spatial")
    state = rng.uniform(-1, 1, (12, 41))
    clean = make_arrays(rng, (2, 2), ov_extent(m))
    ext = ov_extent(m)
    feature = lambda v, i, j, z: ((v * ext[0] + i) * ext[1] + j) * 2 + z  # noqa: E731
    m["input"]["scale"][feature(0, x, y, 1)] = np.float32(-1.0e-7)
    m["input"]["scale"][feature(1, 0, 0, 0)] = np.float32(-1.0e-7)
    planted = [a.copy() for a in clean]
    planted[1][0, 0, 0] = np.float64(m["input"]["center"][feature(1, 0, 0, 0)])  # 0 / 0
    out["zero-denominator"] = (m, state, planted, planted)
    return out


def state_cases():
    """id -> (model, state with non-finite entries, inputs): W_res walks stored entries, so the value reaches only the rows
    with a weight in its column; +-Inf there saturates tanh to exactly +-1, and +Inf meeting -Inf gives NaN."""
    out = {}
    plants = {name: [((1, 5), v)] for name, v in NON_FINITE.items()}
    plants["inf-meets-inf"] = [((1, 5), np.inf), ((1, 6), -np.inf), ((7, 0), -np.inf)]
    for name, plant in plants.items():
        rng = np.random.RandomState(_seed("nf-state"))
        m = nf_model(rng)
        m["w_res"] = bounded_w_res(rng, 41, 0.5)
        state = rng.uniform(-1, 1, (12, 41))
        for at, v in plant:
            state[at] = v
        out[name] = (m, state, make_arrays(rng, (2, 2), ov_extent(m)))
    return out


def dense_difference_case():
    """The documented difference of dense W_in storage: 2 x 2 layout, overlap 1, state 41, 90 % of W_in stored, one NaN
    cell.  scipy's product makes NaN only the rows with a stored weight in the cell's column; a dense product makes NaN
    every row of the subdomains that hold the cell."""
    rng = np.random.RandomState(_seed("dense-difference"))
    m = make_model(rng, (2, 2), (4, 4), overlap=1, state_size=41, in_sizes=(1, 1), w_in_density=0.9)
    state = rng.uniform(-1, 1, (4, 41))
    arrays = make_arrays(rng, (1, 1), ov_extent(m))
    arrays[0][4, 4, 0] = np.nan  # in the overlap of all four subdomains
    return m, state, arrays


# ---------------------------------------------------------------------------------------------
# sparse structure
# ---------------------------------------------------------------------------------------------


def sparse_cases():
    """id -> (model, state, inputs, SparseMatrix arrays to upload as W_in or None, expected dense storage under AUTO or
    None).  3 x 2 subdomains of 2 x 2 cells, overlap 1: 32 inputs, state 41; one input cell is NaN in the cases where stored
    zeros and unstored entries must be told apart."""
    out = {}

    def base(key, **kw):
        rng = np.random.RandomState(_seed("sparse", key))
        m = make_model(rng, (3, 2), (2, 2), overlap=1, state_size=41, in_sizes=(1, 1), **kw)
        return rng, m, rng.uniform(-1, 1, (6, 41)), make_arrays(rng, (1, 1), ov_extent(m))

    rng, m, state, x = base("empty-rows", w_in_density=0.6, w_res_density=0.3)
    m["w_in"] = with_empty_rows(m["w_in"], [0, 7, 40])
    m["w_res"] = with_empty_rows(m["w_res"], [0, 8, 39, 40])
    out["empty-rows"] = (m, state, x, None, None)

    rng, m, state, x = base("empty-w-in")
    m["w_in"] = csr_from_coo(np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0), (41, 32))
    out["empty-w-in"] = (m, state, x, None, False)

    rng, m, state, x = base("stored-zeros", w_in_density=0.6)
    m["w_in"][2][rng.random_sample(m["w_in"][2].size) < 0.3] = 0.0
    m["w_res"][2][::3] = 0.0
    x[0][1, 1, 0] = np.nan
    state[2, 3] = np.inf
    out["stored-zeros"] = (m, state, x, None, None)

    rng, m, state, x = base("duplicates")
    coo, summed = coo_with_duplicates(rng, 41, 32, 0.7, COUPLING_AT_2304, 60)
    m["w_in"] = summed
    out["coo-duplicates"] = (m, state, x, coo, None)

    rng, m, state, x = base("unsorted", w_in_density=0.6)
    m["w_in"] = with_unsorted_columns(rng, m["w_in"])
    m["w_res"] = with_unsorted_columns(rng, m["w_res"])
    out["unsorted-columns"] = (m, state, x, None, None)

    for name, nnz, dense in (("just-below-half", 41 * 32 // 2 - 1, False), ("just-at-half", 41 * 32 // 2, True),
                             ("just-above-half", 41 * 32 // 2 + 1, True)):
        rng, m, state, x = base(name)
        m["w_in"] = with_exact_nnz(rng, 41, 32, nnz, COUPLING_AT_2304)
        out[name] = (m, state, x, None, dense)
    return out


# ---------------------------------------------------------------------------------------------
# readout tails
# ---------------------------------------------------------------------------------------------

# id -> (layout, cells per subdomain, state size, hybrid z sizes or None, output z sizes); H = cells * sum(hybrid sizes)
READOUTS = {
    "S60_H12": ((2, 3), (2, 3), 60, (1, 1), (2, 1)),    # the state / hybrid boundary inside a 64-row step and an 8-row group
    "S64_H0": ((3, 2), (1, 3), 64, None, (1, 2)),       # one whole step; n_out 9 (odd)
    "S65_H0": ((2, 1), (1, 1), 65, None, (1,)),         # one row past a step; n_out 1
    "S33_H96": ((2, 3), (2, 3), 33, (5, 11), (3,)),     # J = 129: three slices, the last one row long
    "S7_H1": ((2, 3), (1, 1), 7, (1,), (1,)),           # less than one 8-row group; n_out 1
}


def readout_case(name, square, out_kind):
    """(model, state, hybrid inputs or None).  A scale-spatial output transformer needs equal z sizes: it takes the first
    size for every output variable."""
    layout, sub, size, hybrid_sizes, out_sizes = READOUTS[name]
    if out_kind == "scale-spatial":
        out_sizes = (out_sizes[0],) * len(out_sizes)
    rng = np.random.RandomState(_seed("readout", name, square, out_kind))
    m = make_model(rng, layout, sub, overlap=1, state_size=size, in_sizes=(1,), out_sizes=out_sizes,
                   hybrid_sizes=hybrid_sizes, hybrid_mask=np.float64 if hybrid_sizes else None, out_kind=out_kind,
                   out_tf_mask=np.float64 if out_kind == "scale-spatial" else None, square=square)
    state = rng.uniform(-1, 1, (layout[0] * layout[1], size))
    return m, state, make_arrays(rng, hybrid_sizes, m["rank"]) if hybrid_sizes else None


def long_readout_case():
    """One subdomain of 64 x 128 cells (n_out 8192), state 8200, no weights into the state: the readout rows come in slices
    of more than one 64-row step.  C (537 MB) is a cheap deterministic pattern of 257 values spread over [-1, 1] / sqrt(J)."""
    size, n_out = 8200, 8192
    rng = np.random.RandomState(_seed("long-readout"))
    empty = lambda n: csr_from_coo(np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0), (size, n))  # noqa: E731
    j = np.arange(size, dtype=np.int32)[:, None]
    k = np.arange(n_out, dtype=np.int32)[None, :]
    c = (((j * 31 + k * 17) % 257 - 128).astype(np.float64) * (1.0 / (128 * np.sqrt(size))))[None]
    tf = {"kind": "do-nothing", "sizes": [1]}
    m = {"layout": (1, 1), "overlap": 0, "rank": (64, 128), "square": False, "input": tf, "output": tf, "hybrid": None,
         "hybrid_mask": None, "input_mask": None, "w_in": empty(n_out), "w_res": empty(size), "coefficients": c,
         "intercepts": rng.randn(1, n_out)}
    return m, rng.uniform(-1, 1, (1, size))
