"""Shared builders of the convolution tests: random networks, inputs of the kind real fields have, and the
``torch.nn.functional.conv2d`` chain on the CPU (float64: a second opinion on ``conv_np``; float32: the reference arithmetic
the GPU result is compared with)."""
import numpy as np
import torch

import tolerances
from fv3net_amd.conv import ConvInput, ConvOutput, ConvSpec


def make_spec(rng, channels, filters, depth, k, heads, activation="relu", bias=True, unit_inputs=False):
    """``channels`` / ``heads``: name -> channel count.  Weights N(0, 1 / sqrt(fan_in)); output scales fall over decades."""
    inputs = []
    for name, nf in channels.items():
        center = np.zeros(nf, np.float32) if unit_inputs else rng.normal(0, 1, nf).astype(np.float32) * 10
        scale = np.ones(nf, np.float32) if unit_inputs else rng.uniform(0.5, 2, nf).astype(np.float32)
        inputs.append(ConvInput(name, nf, center, scale))
    c_in = sum(channels.values())
    kernels, biases = [], []
    for _ in range(depth - 1):
        kernels.append((rng.normal(0, 1, (k, k, c_in, filters)) / np.sqrt(k * k * c_in)).astype(np.float32))
        biases.append(rng.normal(0, 0.1, filters).astype(np.float32))
        c_in = filters
    outputs = []
    for name, nf in heads.items():
        outputs.append(ConvOutput(name, nf, (rng.normal(0, 1, (filters, nf)) / np.sqrt(filters)).astype(np.float32),
                                  rng.normal(0, 0.1, nf).astype(np.float32), tolerances.decades(rng, nf),
                                  (rng.normal(0, 1, nf) * tolerances.decades(rng, nf)).astype(np.float32)))
    return ConvSpec(inputs, kernels, biases if bias else None, outputs, activation=activation)


def make_inputs(rng, spec, lead, nx, ny, dtype=np.float32):
    """name -> ``lead + (x, y, z)``: standard normal scaled and shifted per channel to the variable's own mean and spread."""
    out = {}
    for i in spec.inputs:
        a = rng.normal(0, 1, tuple(lead) + (nx, ny, i.nfeat))
        out[i.source] = (a * np.asarray(i.scale, np.float64) + np.asarray(i.center, np.float64)).astype(dtype)
    return out


def torch_chain(spec, inputs, dtype=torch.float32):
    """``inputs``: name -> [sample, x, y, z] with the halo.  The same graph through ``conv2d`` on the CPU in ``dtype``."""
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dtype)
    cols = [(tt(inputs[i.source]) - tt(i.center)) / tt(i.scale) for i in spec.inputs]
    x = torch.cat(cols, dim=-1).permute(0, 3, 1, 2)  # [s, c, x, y]
    act = {"relu": torch.relu, "tanh": torch.tanh, "linear": lambda v: v}[spec.activation]
    for l, w in enumerate(spec.hidden_kernels):
        b = None if spec.hidden_biases is None else tt(spec.hidden_biases[l])
        x = act(torch.nn.functional.conv2d(x, tt(w).permute(3, 2, 0, 1), b))
    out = {}
    for o in spec.outputs:
        y = torch.nn.functional.conv2d(x, tt(o.kernel).t()[:, :, None, None], tt(o.bias))
        y = y.permute(0, 2, 3, 1) * tt(o.scale) + tt(o.center)
        out[o.name] = y.numpy()
    return out


# ---------------------------------------------------------------------------------------------------------
# edge cases: tests/test_gpu_conv_edges.py on the device, tests/test_oracle_conv.py for the checkers themselves
# ---------------------------------------------------------------------------------------------------------
# interior extents (nx, ny) around the 16 x 16 tile: one cell, below / at / past one tile and two, x and y crossing a tile
# multiple differently.  With a batch of 2: 2 * 1938 = 3876 pixels per network.
EDGE_EXTENTS = [(1, 1), (2, 5), (3, 3), (15, 16), (16, 17), (17, 15), (31, 2), (33, 33)]

# id -> (input channels, filters, depth, k, heads, activation).  More than 64 filters: gridDim.z > 1 in the hidden layers, a
# partly (65, 67) or almost wholly (130) padded last N block; channel counts that are no multiple of the K chunk (4 channels
# for k = 5, 2 for k = 7) in the first layer (7, 9, 3, 5) and in the later ones (5, 33, 3, 67); k = 1: no halo at all.
EDGE_NETWORKS = {
    "k1": ({"T": 7, "lat": 1}, 5, 3, 1, {"dQ1": 7, "rain": 1}, "relu"),
    "k3_f65": ({"T": 7, "lat": 1}, 65, 3, 3, {"dQ1": 7, "rain": 1}, "relu"),
    "k3_f130_tanh": ({"T": 9}, 130, 2, 3, {"dQ1": 33}, "tanh"),
    "k5_c7_f5": ({"T": 6, "lat": 1}, 5, 3, 5, {"dQ1": 6, "rain": 1}, "tanh"),
    "k5_c9_f33": ({"T": 9}, 33, 2, 5, {"dQ1": 9}, "relu"),
    "k7_c3_f3": ({"T": 3}, 3, 2, 7, {"dQ1": 3}, "relu"),
    "k7_c5_f67": ({"T": 5}, 67, 2, 7, {"dQ1": 5}, "linear"),
}

# id -> (network as above, face sizes n): n == h (the halo is the neighbour's whole face), n just above it, n past one tile
CUBE_NETWORKS = {
    "cube_k3_depth3": (({"T": 7, "lat": 1}, 33, 3, 3, {"dQ1": 7, "rain": 1}, "relu"), (2, 3, 17)),
    "cube_k7_depth2": (({"T": 3}, 3, 2, 7, {"dQ1": 3}, "tanh"), (3, 16)),
    "cube_k1": (({"T": 7, "lat": 1}, 5, 3, 1, {"dQ1": 7, "rain": 1}, "relu"), (5,)),
}

NON_FINITE = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
ACTIVATION_NAMES = ("relu", "tanh", "linear")
NON_FINITE_NETWORK = ({"T": 7, "lat": 1}, 5, 3, 3, {"dQ1": 7, "rain": 1})
NON_FINITE_EXTENT = (20, 9)
NON_FINITE_HIT = (9, 4, 3)  # interior cell (x, y) and the channel of T, sample 0; lat's halo corner [0, 0] of sample 1 too


def pad_cube(fields, h):
    """name -> [6, x, y, z] -> name -> [6, x + 2 h, y + 2 h, z] by the oracle's own halo fill."""
    import conv_np

    return {k: np.moveaxis(conv_np.append_halos(np.moveaxis(v, -1, 1), h), 1, -1) for k, v in fields.items()}


def reference(spec, padded):
    """(float64 oracle, float32 CPU chain) of inputs that carry their halo, both evaluated on the inputs rounded to float32
    (what the device is given); non-finite values pass through without numpy's warnings."""
    import conv_np

    f32 = {k: np.asarray(v).astype(np.float32) for k, v in padded.items()}
    with np.errstate(invalid="ignore", over="ignore"):
        return conv_np.forward(spec, f32), torch_chain(spec, f32, torch.float32)


_CACHE = {}


def _cached(key, build):
    """Inputs and references are computed once per session and shared (read-only) by the tests that need them."""
    if key not in _CACHE:
        _CACHE[key] = build()
        for part in _CACHE[key][1]:
            for d in part[1:]:
                for a in d.values():
                    a.setflags(write=False)
    return _CACHE[key]


def sweep_case(name):
    """``EDGE_NETWORKS[name]`` over ``EDGE_EXTENTS``: (spec, [((nx, ny), inputs with the halo [2, x, y, z], truth, cpu32)])."""
    def build():
        channels, filters, depth, k, heads, activation = EDGE_NETWORKS[name]
        rng = np.random.default_rng(100 + list(EDGE_NETWORKS).index(name))
        spec = make_spec(rng, channels, filters, depth, k, heads, activation=activation)
        h = spec.halos_required
        parts = []
        for nx, ny in EDGE_EXTENTS:
            fields = make_inputs(rng, spec, (2,), nx + 2 * h, ny + 2 * h)
            parts.append(((nx, ny), fields) + reference(spec, fields))
        return spec, parts
    return _cached(("sweep", name), build)


def cube_case(name):
    """``CUBE_NETWORKS[name]``: (spec, [(n, six faces [6, n, n, z] without halo, truth, cpu32)]), the references from the
    oracle's own ``append_halos``."""
    def build():
        (channels, filters, depth, k, heads, activation), sizes = CUBE_NETWORKS[name]
        rng = np.random.default_rng(200 + list(CUBE_NETWORKS).index(name))
        spec = make_spec(rng, channels, filters, depth, k, heads, activation=activation)
        parts = []
        for n in sizes:
            cube = make_inputs(rng, spec, (6,), n, n)
            parts.append((n, cube) + reference(spec, pad_cube(cube, spec.halos_required)))
        return spec, parts
    return _cached(("cube", name), build)


def non_finite_case(activation, value):
    """The network of ``NON_FINITE_NETWORK`` on a 20 x 9 interior field, batch of 2, and the same field with ``value`` planted
    in one interior cell of one ``T`` channel of sample 0 and in the halo corner ``[0, 0]`` of ``lat`` in sample 1:
    (spec, [("clean", inputs, truth, cpu32), ("planted", inputs, truth, cpu32)])."""
    def build():
        channels, filters, depth, k, heads = NON_FINITE_NETWORK
        rng = np.random.default_rng(300 + sorted(ACTIVATION_NAMES).index(activation))
        spec = make_spec(rng, channels, filters, depth, k, heads, activation=activation)
        h = spec.halos_required
        clean = make_inputs(rng, spec, (2,), NON_FINITE_EXTENT[0] + 2 * h, NON_FINITE_EXTENT[1] + 2 * h)
        planted = {k_: v.copy() for k_, v in clean.items()}
        x, y, c = NON_FINITE_HIT
        planted["T"][0, h + x, h + y, c] = value
        planted["lat"][1, 0, 0, 0] = value
        return spec, [("clean", clean) + reference(spec, clean), ("planted", planted) + reference(spec, planted)]
    return _cached(("non_finite", activation, repr(value)), build)


def footprint_mask(spec, nx, ny):
    """[x, y] True where an output's window holds the interior cell ``NON_FINITE_HIT`` (5 x 5 cells for k = 3, depth 3)."""
    h, (x, y, _) = spec.halos_required, NON_FINITE_HIT
    m = np.zeros((nx, ny), bool)
    m[max(x - h, 0):x + h + 1, max(y - h, 0):y + h + 1] = True
    return m


def assert_close_pooled(parts, name=""):
    """``parts``: [(label, got, truth, cpu32)], arrays [..., level].  The pixels of all parts pooled into ONE call of
    ``tolerances.assert_close_per_level`` -- a level's scale is then a statistic over all of them, not over the two pixels of
    a 1 x 1 field -- and a failure names the part that holds the worst error / scale.  Returns the worst ratio."""
    flat = lambda a: np.asarray(a, np.float64).reshape(-1, np.shape(a)[-1])  # noqa: E731
    got, truth, cpu32 = (np.concatenate([flat(p[i]) for p in parts]) for i in (1, 2, 3))
    scale = np.max(np.abs(truth), axis=0)
    safe = np.where(scale == 0, 1, scale)
    ratios = [float(np.max(np.where(scale == 0, 0, np.abs(flat(p[1]) - flat(p[2])) / safe))) for p in parts]
    worst = int(np.argmax(ratios))
    try:
        return tolerances.assert_close_per_level(got, truth, cpu32=cpu32, name=name)
    except AssertionError as e:
        raise AssertionError(f"{name}: worst error / level scale {ratios[worst]:.2e} in part {parts[worst][0]}; {e}") from None


def classes(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN per element."""
    a = np.asarray(a)
    return (np.isposinf(a) * 1 + np.isneginf(a) * 2 + np.isnan(a) * 3).astype(np.int8)


def assert_close_with_non_finite(got, truth, cpu32, name="", cap=0.10):
    """``got``, ``truth``, ``cpu32``: [..., level] of one head.  (a) the map of {finite, +Inf, -Inf, NaN} of ``got`` equals the
    oracle's, element for element (an exact condition: the float32 chain meets it); (c) at most ``cap`` of the pixels hold a
    non-finite level, so that (b) the usual gate judges the rest, the non-finite elements of all three set to 0.
    Returns the number of pixels that hold a non-finite level."""
    got, truth, cpu32 = (np.array(a, np.float64) for a in (got, truth, cpu32))
    assert got.shape == truth.shape == cpu32.shape, (name, got.shape, truth.shape, cpu32.shape)
    cg, ct = classes(got), classes(truth)
    differ = [tuple(int(i) for i in d) for d in np.argwhere(cg != ct)]
    assert not differ, (name, f"{len(differ)} elements differ in class (0 finite, 1 +Inf, 2 -Inf, 3 NaN) from the oracle; "
                              f"first at {differ[0]}: got {cg[differ[0]]}, oracle {ct[differ[0]]}")
    bad = ct != 0
    n_pixels = int(np.prod(truth.shape[:-1]))
    n_bad = int(np.count_nonzero(bad.any(axis=-1)))
    assert n_bad <= cap * n_pixels, (name, f"{n_bad} of {n_pixels} pixels are non-finite in the oracle: nothing left to judge")
    got[bad], truth[bad] = 0.0, 0.0
    cpu32[bad | ~np.isfinite(cpu32)] = 0.0
    nf = truth.shape[-1]
    tolerances.assert_close_per_level(got.reshape(-1, nf), truth.reshape(-1, nf), cpu32=cpu32.reshape(-1, nf), name=name)
    return n_bad
