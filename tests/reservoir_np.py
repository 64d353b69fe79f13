"""A float64 numpy/scipy restatement of fv3fit's reservoir step, the checker of the GPU path, and builders of test models.

Written from the reference's semantics (reservoir.py, readout.py, model.py, domain2.py, transformers/transformer.py):
  - subdomain s of a (layout_x, layout_y) layout covers x block s % layout_x, y block s // layout_x; each subdomain is
    flattened in (x, y, z) order;
  - "do-nothing" concatenates the variables along z; "scale-spatial-concat-z" computes (x - center) / (scale + 1e-7) in
    float32 per (variable, x, y, z) feature, concatenates along z and multiplies by its mask; decoding multiplies by the
    mask, then x * scale + center in float32;
  - increment: state = tanh(u * input_mask @ W_in.T + state @ W_res.T);
  - readout: square_even_terms (axis 0 for the pure model, -1 for the hybrid one), then [state, hybrid] @ C[s] + b[s].
"""
import os

import numpy as np

try:
    import scipy.sparse as _sp
except ImportError:  # dense products instead
    _sp = None


def blocks(arr, layout, overlap):
    """[subdomain, flat] of an (x, y, z) array covering the overlapped rank extent."""
    lx, ly = layout
    bx = (arr.shape[0] - 2 * overlap) // lx
    by = (arr.shape[1] - 2 * overlap) // ly
    out = []
    for s in range(lx * ly):
        x0, y0 = (s % lx) * bx, (s // lx) * by
        out.append(arr[x0:x0 + bx + 2 * overlap, y0:y0 + by + 2 * overlap].reshape(-1))
    return np.stack(out)


def merge(flat, layout, extent, nz):
    lx, ly = layout
    bx, by = extent[0] // lx, extent[1] // ly
    out = np.empty((extent[0], extent[1], nz), flat.dtype)
    for s in range(lx * ly):
        x0, y0 = (s % lx) * bx, (s // lx) * by
        out[x0:x0 + bx, y0:y0 + by] = flat[s].reshape(bx, by, nz)
    return out


def encode(tf, arrays):
    arrays = [np.asarray(a) for a in arrays]
    if tf["kind"] == "do-nothing":
        return np.concatenate(arrays, axis=-1)
    x, y, z = tf["spatial_features"]
    n = len(arrays)
    stacked = np.concatenate([a.reshape(-1) for a in arrays]).astype(np.float32)
    c = np.asarray(tf["center"], np.float32).reshape(-1)
    s = np.asarray(tf["scale"], np.float32).reshape(-1)
    norm = (stacked - c) / (s + np.float32(1.0e-7))
    parts = np.split(norm, n)
    out = np.concatenate([p.reshape(x, y, z) for p in parts], axis=-1)
    if tf.get("mask") is not None:
        out = out * tf["mask"]
    return out


def decode(tf, merged):
    if tf["kind"] == "do-nothing":
        return np.split(merged, np.cumsum(tf["sizes"])[:-1], axis=-1)
    x, y, z = tf["spatial_features"]
    if tf.get("mask") is not None:
        merged = merged * tf["mask"]
    n = merged.shape[-1] // z
    stacked = np.concatenate([p.reshape(-1) for p in np.split(merged, n, axis=-1)]).astype(np.float32)
    out = stacked * np.asarray(tf["scale"], np.float32).reshape(-1) + np.asarray(tf["center"], np.float32).reshape(-1)
    return [p.reshape(x, y, z) for p in np.split(out, n)]


def _matmul_t(dense, csr):
    """dense @ W.T for W given as (indptr, indices, data, shape)."""
    indptr, idx, val, shape = csr
    if _sp is not None:
        w = _sp.csc_matrix(_sp.csr_matrix((val, idx, indptr), shape=shape))
        return dense @ w.T
    w = np.zeros(shape)
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    np.add.at(w, (rows, idx), val)
    return dense @ w.T


def increment(m, state, arrays):
    u = blocks(encode(m["input"], arrays), m["layout"], m["overlap"])
    if m.get("input_mask") is not None:
        u = u * m["input_mask"]
    return np.tanh(_matmul_t(u, m["w_in"]) + _matmul_t(state, m["w_res"]))


def square_even_terms(v, axis):
    out = np.array(v, copy=True)
    idx = [slice(None)] * out.ndim
    idx[axis] = slice(0, None, 2)
    out[tuple(idx)] = out[tuple(idx)] ** 2
    return out


def predict(m, state, hybrid_arrays=None):
    r = state
    if m["square"]:
        r = square_even_terms(r, axis=-1 if m["hybrid"] is not None else 0)
    if m["hybrid"] is not None:
        h = blocks(encode(m["hybrid"], hybrid_arrays), m["layout"], 0)
        if m.get("hybrid_mask") is not None:
            h = h * m["hybrid_mask"]
        r = np.concatenate([r, h], axis=-1)
    y = np.einsum("ij,ijk->ik", r, m["coefficients"]) + m["intercepts"]
    nz = m["coefficients"].shape[-1] // (m["rank"][0] // m["layout"][0] * m["rank"][1] // m["layout"][1])
    return decode(m["output"], merge(y, m["layout"], m["rank"], nz))


# ---------------------------------------------------------------------------------------------
# test models
# ---------------------------------------------------------------------------------------------


def random_csr(rng, m, n, density, scale=1.0):
    mask = rng.random_sample((m, n)) < density
    rows, cols = np.nonzero(mask)
    vals = rng.uniform(-scale, scale, rows.size)
    indptr = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=m), out=indptr[1:])
    return indptr, cols.astype(np.int32), vals, (m, n)


def scale_to_radius(csr, radius, rng):
    """W_res scaled to a spectral radius estimate (power iteration on |W|, an upper bound)."""
    indptr, idx, val, shape = csr
    w = np.zeros(shape)
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    np.add.at(w, (rows, idx), val)
    ev = np.max(np.abs(np.linalg.eigvals(w))) if shape[0] <= 600 else None
    if ev is None:
        v = rng.random_sample(shape[0])
        a = np.abs(w)
        for _ in range(50):
            v = a @ v
            v /= np.linalg.norm(v)
        ev = float(v @ (a @ v))
    return indptr, idx, val * (radius / ev), shape


def make_transformer(kind, rng, n_var, nz, extent, mask=False, mask_dtype=np.float64):
    if kind == "do-nothing":
        return {"kind": kind, "sizes": [nz] * n_var}
    n = n_var * extent[0] * extent[1] * nz
    t = {"kind": kind, "spatial_features": (extent[0], extent[1], nz), "num_variables": n_var,
         "center": rng.randn(n).astype(np.float32), "scale": rng.uniform(0.5, 2.0, n).astype(np.float32), "mask": None}
    if mask:
        t["mask"] = (rng.random_sample((extent[0], extent[1], nz * n_var)) > 0.2).astype(mask_dtype)
    return t


def make_model(rng, layout=(2, 2), overlap=0, rank=(8, 8), n_var=2, nz=1, state_size=40, in_kind="do-nothing",
               out_kind="do-nothing", hybrid_kind=None, n_out_var=1, square=False, input_mask=False, hybrid_mask=False,
               w_in_density=1.0, w_res_density=0.2, radius=0.99, coupling=0.1):
    ov_ext = (rank[0] + 2 * overlap, rank[1] + 2 * overlap)
    ns = layout[0] * layout[1]
    sub = (rank[0] // layout[0], rank[1] // layout[1])
    m = {"layout": layout, "overlap": overlap, "rank": rank, "square": square, "n_var": n_var, "nz": nz,
         "input": make_transformer(in_kind, rng, n_var, nz, ov_ext),
         "output": make_transformer(out_kind, rng, n_out_var, nz, rank, mask=out_kind != "do-nothing")}
    if in_kind != "do-nothing":
        m["input"]["mask"] = (rng.random_sample((ov_ext[0], ov_ext[1], nz * n_var)) > 0.2).astype(np.float64)
    n_in = (sub[0] + 2 * overlap) * (sub[1] + 2 * overlap) * nz * n_var
    m["w_in"] = random_csr(rng, state_size, n_in, w_in_density, coupling)
    m["w_res"] = scale_to_radius(random_csr(rng, state_size, state_size, w_res_density, 1.0), radius, rng)
    m["input_mask"] = (rng.random_sample((ns, n_in)) > 0.1).astype(np.float64) if input_mask else None
    n_h = 0
    m["hybrid"] = None
    if hybrid_kind:
        m["hybrid"] = make_transformer(hybrid_kind, rng, n_var, nz, rank)
        n_h = sub[0] * sub[1] * nz * n_var
        m["hybrid_mask"] = (rng.random_sample((ns, n_h)) > 0.3).astype(np.float64) if hybrid_mask else None
    n_out = sub[0] * sub[1] * nz * n_out_var
    m["coefficients"] = rng.randn(ns, state_size + n_h, n_out) / np.sqrt(state_size)
    m["intercepts"] = rng.randn(ns, n_out)
    return m


def _dump_transformer(t, path):
    os.makedirs(path, exist_ok=True)
    import yaml
    if t["kind"] == "do-nothing":
        with open(os.path.join(path, "mock_transformer.yaml"), "w") as f:
            yaml.safe_dump({"original_feature_sizes": list(t["sizes"])}, f)
        return
    with open(os.path.join(path, "scale_spatial_concat_z_transformer.yaml"), "w") as f:
        # yaml.dump of the tuple .shape[-3:], as the reference writes it
        f.write(yaml.dump({"num_variables": t["num_variables"], "spatial_features": tuple(t["spatial_features"])}))
    np.save(os.path.join(path, "scale.npy"), t["scale"])
    np.save(os.path.join(path, "center.npy"), t["center"])
    if t.get("mask") is not None:
        np.save(os.path.join(path, "mask.npy"), t["mask"])


def _save_sparse(path, csr, fmt):
    indptr, idx, val, shape = csr
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    if fmt == "csr":
        arrays = {"indices": idx, "indptr": indptr, "format": np.array(b"csr"), "shape": np.array(shape), "data": val}
    elif fmt == "csc":
        order = np.lexsort((rows, idx))
        cptr = np.zeros(shape[1] + 1, np.int64)
        np.cumsum(np.bincount(idx, minlength=shape[1]), out=cptr[1:])
        arrays = {"indices": rows[order].astype(np.int32), "indptr": cptr, "format": np.array(b"csc"),
                  "shape": np.array(shape), "data": val[order]}
    else:
        arrays = {"row": rows.astype(np.int32), "col": idx, "format": np.array(b"coo"), "shape": np.array(shape),
                  "data": val}
    with open(path, "wb") as f:
        np.savez_compressed(f, **arrays)


def write_reference_layout(m, path, name=None, fmt="csc", state=None, square=None, variables=("a", "b"),
                           out_variables=None, hybrid_variables=None):
    """A model directory as fv3fit.dump writes it (reservoir/model.py, adapters.py)."""
    import yaml
    inner = path
    if name is not None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "name"), "w") as f:
            f.write(name)
        if name.endswith("adapter"):
            inner = os.path.join(path, "hybrid_reservoir_model" if name.startswith("hybrid") else "reservoir_model")
    res = os.path.join(inner, "reservoir")
    os.makedirs(res, exist_ok=True)
    _save_sparse(os.path.join(res, "reservoir_W_in.npz"), m["w_in"], fmt)
    _save_sparse(os.path.join(res, "reservoir_W_res.npz"), m["w_res"], fmt)
    hp = {"state_size": m["w_res"][3][0], "adjacency_matrix_sparsity": 0.8, "spectral_radius": 0.99, "seed": 0,
          "input_coupling_sparsity": 0.0, "input_coupling_scaling": 0.1}
    with open(os.path.join(res, "metadata.bin"), "w") as f:
        f.write(yaml.safe_dump({"reservoir_hyperparameters": hp, "input_size": m["w_in"][3][1]}))
    if m.get("input_mask") is not None:
        np.save(os.path.join(res, "input_mask.npy"), m["input_mask"])
    if state is not None:
        np.save(os.path.join(res, "state.npy"), state)
    ro = os.path.join(inner, "readout")
    os.makedirs(ro, exist_ok=True)
    with open(os.path.join(ro, "coefficients.npz"), "wb") as f:
        np.save(f, m["coefficients"])
    np.save(os.path.join(ro, "intercepts.npy"), m["intercepts"])
    out_variables = list(out_variables or variables)
    with open(os.path.join(inner, "metadata.yaml"), "w") as f:
        f.write(yaml.dump({"square_half_hidden_state": bool(m["square"] if square is None else square),
                           "input_variables": tuple(variables), "output_variables": tuple(out_variables)}))
    nz_in = sum(m["input"]["sizes"]) if m["input"]["kind"] == "do-nothing" else m["input"]["spatial_features"][2] * \
        m["input"]["num_variables"]
    with open(os.path.join(inner, "rank_divider.yaml"), "w") as f:
        f.write(yaml.dump({"subdomain_layout": tuple(m["layout"]), "overlap": m["overlap"], "rank_extent": tuple(m["rank"]),
                           "z_feature_size": nz_in}))
    tdir = os.path.join(inner, "transformers")
    _dump_transformer(m["input"], os.path.join(tdir, "input_transformer"))
    _dump_transformer(m["output"], os.path.join(tdir, "output_transformer"))
    _dump_transformer(m["hybrid"] if m["hybrid"] is not None else m["input"], os.path.join(tdir, "hybrid_transformer"))
    if m["hybrid"] is not None:
        with open(os.path.join(inner, "hybrid_variables.yaml"), "w") as f:
            f.write(yaml.dump({"hybrid_variables": list(hybrid_variables or variables)}))
        if m.get("hybrid_mask") is not None:
            np.save(os.path.join(inner, "hybrid_input_mask.npy"), m["hybrid_mask"])
    return path


def regtest_model(hybrid):
    """get_8x8_overlapped_model (tests/reservoir/test_model_adapter.py): 2x2 layout, overlap 2, 8x8 with overlap, z 6
    (two do-nothing variables of 3), state 25, RandomState(0) readout.  W_in / W_res do not matter at zero state."""
    rng = np.random.RandomState(0)
    ns, n_flat = 4, 2 * 2 * 6
    n_in_feat = 25 + (n_flat if hybrid else 0)
    coefficients = rng.randn(ns, n_in_feat, n_flat)
    intercepts = rng.randn(ns, n_flat)
    other = np.random.RandomState(1)
    tf = {"kind": "do-nothing", "sizes": [3, 3]}
    return {"layout": (2, 2), "overlap": 2, "rank": (4, 4), "square": False, "input": tf, "output": tf,
            "hybrid": tf if hybrid else None, "hybrid_mask": np.ones((ns, n_flat)) if hybrid else None,
            "w_in": random_csr(other, 25, 6 * 6 * 6, 1.0, 1.0),
            "w_res": scale_to_radius(random_csr(other, 25, 25, 1.0, 1.0), 1.0, other), "input_mask": None,
            "coefficients": coefficients, "intercepts": intercepts}


def regtest_data(overlap=True):
    rng = np.random.RandomState(0)
    n = 8 if overlap else 4
    return rng.randn(n, n, 3), rng.randn(n, n, 3)
