"""Case builders of the column codec tests (tests/test_host_codec.py on the CPU, tests/test_gpu_codec.py and
tests/test_gpu_reservoir_codec.py on the device).

Every shape case is built once over ``N_COLUMNS`` = 257 columns (a 1 x 257 extent) and shared read-only; the smaller column
counts of the device tests are its leading columns.  The builders assert on the CPU what the gates rely on: no latent unit
of a dense case is dead (each is positive for some columns and zero for others, so no level of the oracle is identically
zero), and an affine case summed in a permuted order stays within a quarter of its float64 gate.
"""
import zlib

import numpy as np

import codec_np as N

N_COLUMNS = 257
COLUMN_COUNTS = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 257: (1, 257)}  # count -> (nx, ny)
AFFINE_GATE = 1e-12  # times max|want| per latent unit / output level (DESIGN section 12's float64 gate)

# name -> (z sizes, hidden widths of either side, n_latent).  Together: K 1, 3, 7, 63, 64, 65, 316 and the cap 1024;
# widths 1, 20, 33 and 256; 0, 1, 2 and 3 hidden layers per side; n_latent 1, 10, 40 and the cap 256.  "wide" and "cap" hold
# layers too large to stage in LDS beside the tile, the others are staged whole.
DENSE = {
    "default": ((79, 79, 79, 79), (20, 20), 10),
    "k1": ((1,), (), 1),
    "k3_width1": ((1, 1, 1), (1,), 1),
    "k7": ((5, 1, 1), (33,), 10),
    "k63_three": ((63,), (20, 33, 20), 40),
    "k64": ((32, 32), (256,), 40),
    "k65_none": ((64, 1), (), 10),
    "wide": ((79, 79, 79, 79), (256, 256), 40),
    "cap": ((64,) * 16, (256,), 256),
}
SCALE_ONLY = {"s316": (79, 79, 79, 79), "s7": (5, 1, 1), "s1": (1,), "s65": (64, 1)}
# name -> (z sizes, n_latent, whiten, with_mean, with_std, enforce_positive)
AFFINE = {
    "default": ((79, 79, 79, 79), 10, False, True, True, False),
    "whiten40": ((79, 79, 79, 79), 40, True, True, True, True),
    "k1": ((1,), 1, False, True, True, False),
    "k3": ((1, 1, 1), 1, True, False, True, False),
    "k7": ((5, 1, 1), 1, False, True, False, True),
    "k63": ((63,), 10, True, True, True, False),
    "k64": ((32, 32), 40, False, False, False, False),
    "k65": ((64, 1), 10, True, True, False, False),
}


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 31)


_CACHE = {}


def cached(build, *key):
    k = (build.__name__,) + key
    if k not in _CACHE:
        _CACHE[k] = build(*key)
    return _CACHE[k]


def _layers(rng, widths):
    """He-scaled kernels (the activations keep their spread through the ReLUs) and small biases."""
    return [((rng.randn(a, b) * np.sqrt(2.0 / a)).astype(np.float32), (0.1 * rng.randn(b)).astype(np.float32))
            for a, b in zip(widths[:-1], widths[1:])]


def columns(rng, sizes, center, scale, n=N_COLUMNS):
    """One [n, z] float64 array per variable: center + scale * N(0, 1), so that the normalised column is of order one."""
    out, k0 = [], 0
    for nz in sizes:
        out.append(center[k0:k0 + nz].astype(np.float64) + scale[k0:k0 + nz] * rng.randn(n, nz))
        k0 += nz
    return out


def dense_spec(rng, sizes, hidden, n_latent, limits=True):
    k = sum(sizes)
    center = rng.randn(k).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, k).astype(np.float32)
    spec = {"sizes": list(sizes), "center": center, "scale": scale,
            "enc": _layers(rng, [k, *hidden, n_latent]), "dec": _layers(rng, [n_latent, *hidden])}
    width = hidden[-1] if hidden else n_latent
    spec["heads"] = [((rng.randn(width, nz) / np.sqrt(width)).astype(np.float32), (0.1 * rng.randn(nz)).astype(np.float32))
                     for nz in sizes]
    # limits away from zero on the first and the last variable (a limit of exactly 0 would make a level of the oracle
    # identically zero, which the per-level gate then wants exactly zero on both sides of a rounding)
    spec["min"] = [None] * len(sizes)
    spec["max"] = [None] * len(sizes)
    if limits:
        spec["min"][0] = float(center[0] - 0.75 * scale[0]) or 0.5
        spec["max"][-1] = float(center[-1] + 0.75 * scale[-1]) or 0.5
        if len(sizes) == 1:
            spec["max"][0] = spec["min"][0] + 1.5 * float(scale[0])
    return spec


def dense_case(name):
    """(spec, inputs [257, z] per variable float64, latent float32 for the decode tests)."""
    sizes, hidden, n_latent = DENSE[name]
    for attempt in range(20):
        rng = np.random.RandomState(_seed("dense", name, attempt))
        spec = dense_spec(rng, sizes, hidden, n_latent, limits=False)
        x = columns(rng, sizes, spec["center"], spec["scale"])
        z = N.dense_encode(spec, x, np.float64)
        if np.all((z > 0).any(axis=0) & (z == 0).any(axis=0)):
            break
    else:
        raise AssertionError(f"dense case {name}: a latent unit is dead in every attempt")
    # the decode tests start from a latent of their own: non-negative as a ReLU's, float32
    latent = np.maximum(rng.randn(N_COLUMNS, n_latent), 0).astype(np.float32)
    # limits that cut the lowest 2 % of the first variable and the highest 2 % of the last: every level keeps most of its
    # columns unlimited, so the float32 yardstick of the per-level gate is not an accident of a few columns
    free = N.dense_decode(spec, latent, np.float64)
    spec["min"][0] = float(np.float32(np.percentile(free[0], 2)))
    spec["max"][-1] = float(np.float32(np.percentile(free[-1], 98)))
    assert spec["min"][0] != 0 and spec["max"][-1] != 0 and (len(sizes) > 1 or spec["max"][0] > spec["min"][0])
    truth = N.dense_decode(spec, latent, np.float64)
    assert all(np.all(np.abs(t).max(axis=0) > 0) for t in truth), f"dense case {name}: an output level is identically zero"
    return spec, x, latent


def scale_only_case(name):
    sizes = SCALE_ONLY[name]
    rng = np.random.RandomState(_seed("scale-only", name))
    spec = dense_spec(rng, sizes, (), sum(sizes), limits=False)
    spec["enc"], spec["dec"], spec["heads"] = [], [], []
    x = columns(rng, sizes, spec["center"], spec["scale"])
    return spec, x, rng.randn(N_COLUMNS, sum(sizes)).astype(np.float32)


def affine_spec(rng, sizes, n_latent, whiten, with_mean, with_std, positive):
    k = sum(sizes)
    q, _ = np.linalg.qr(rng.randn(k, n_latent))
    return {"sizes": list(sizes), "mean": rng.randn(k) if with_mean else None,
            "std": rng.uniform(0.5, 2.0, k) if with_std else None, "pca_mean": 0.1 * rng.randn(k),
            "components": np.ascontiguousarray(q.T), "ev": rng.uniform(0.5, 4.0, n_latent) if whiten else None,
            "positive": bool(positive)}


def affine_gate(want):
    """1e-12 x max|want| per latent unit / output level (the last axis), over the finite part."""
    w = np.where(np.isfinite(want), np.abs(want), 0.0)
    return AFFINE_GATE * w.reshape(-1, w.shape[-1]).max(axis=0)


def affine_case(name):
    """(spec, inputs [257, z] per variable float64, latent float64, expected encoding, expected decoding)."""
    sizes, n_latent, whiten, with_mean, with_std, positive = AFFINE[name]
    for attempt in range(20):
        rng = np.random.RandomState(_seed("affine", name, attempt))
        spec = affine_spec(rng, sizes, n_latent, whiten, with_mean, with_std, positive)
        k = sum(sizes)
        center = spec["mean"] if with_mean else np.zeros(k)
        x = columns(rng, sizes, center, spec["std"] if with_std else np.ones(k))
        latent = rng.randn(N_COLUMNS, n_latent)
        z, y = N.affine_encode(spec, x), N.affine_decode(spec, latent)
        order_k, order_l = rng.permutation(k), rng.permutation(n_latent)
        dz = np.abs(N.affine_encode(spec, x, order_k) - z).max(axis=0)
        dy = np.abs(np.concatenate(N.affine_decode(spec, latent, order_l), -1) - np.concatenate(y, -1)).max(axis=0)
        if np.all(dz <= 0.25 * affine_gate(z)) and np.all(dy <= 0.25 * affine_gate(np.concatenate(y, -1))):
            return spec, x, latent, z, y
    raise AssertionError(f"affine case {name}: a permuted summation order leaves a quarter of the gate in every attempt")


# ---------------------------------------------------------------------------------------------
# the package's objects
# ---------------------------------------------------------------------------------------------


def dense_codec(spec):
    from fv3net_amd.reservoir import DenseAutoencoder

    unzip = lambda layers, i: [layer[i] for layer in layers]  # noqa: E731
    return DenseAutoencoder(spec["center"], spec["scale"], spec["sizes"], unzip(spec["enc"], 0), unzip(spec["enc"], 1),
                            unzip(spec["dec"], 0), unzip(spec["dec"], 1), unzip(spec["heads"], 0), unzip(spec["heads"], 1),
                            output_min=spec.get("min"), output_max=spec.get("max"))


def affine_codec(spec):
    from fv3net_amd.reservoir import SkTransformer

    return SkTransformer(spec["components"], spec["pca_mean"], spec["sizes"], explained_variance=spec["ev"],
                         scaler_mean=spec["mean"], scaler_scale=spec["std"], enforce_positive_outputs=spec["positive"])


def as_extent(arrays, count):
    """The leading ``count`` columns of [257, z] arrays as (nx, ny, z) arrays."""
    nx, ny = COLUMN_COUNTS[count]
    return [np.ascontiguousarray(a[:count]).reshape(nx, ny, a.shape[-1]) for a in arrays]


SOURCES = ("f32", "f64", "mixed")
VIEWS = ("plain", "transposed", "strided")


def source_dtypes(kind, n):
    return {"f32": [np.float32] * n, "f64": [np.float64] * n,
            "mixed": [np.float32 if v % 2 == 0 else np.float64 for v in range(n)]}[kind]
