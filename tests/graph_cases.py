"""Specs and inputs of the graph autoregressor tests: weights drawn as N(0, 1 / fan_in), the state as N(0, 1)."""
import functools

import numpy as np
import torch


def sage_layer(rng, c_in, c_out, bias=True):
    """A SAGE layer whose fan-in is the 2 c_in rows of [W_self; W_neigh]."""
    from fv3net_amd.graph import SageLayer

    draw = lambda: (rng.normal(0, 1, (c_in, c_out)) / np.sqrt(2 * c_in)).astype(np.float32)
    return SageLayer(draw(), draw(), (rng.normal(0, 0.1, c_out) if bias else np.zeros(c_out)).astype(np.float32))


def up_layer(rng, c_in, c_out):
    from fv3net_amd.graph import UpLayer

    return UpLayer((rng.normal(0, 1, (c_in, 2, 2, c_out)) / np.sqrt(c_in)).astype(np.float32),
                   rng.normal(0, 0.1, c_out).astype(np.float32))


def make_spec(rng, variables, depth=1, min_filters=4, activation="relu"):
    """``variables``: name -> feature count.  Means and stds as a temperature-like and a humidity-like field have them."""
    from fv3net_amd.graph import GraphUNetSpec, GraphVariable, layer_plan

    vs = [GraphVariable(name, nf, rng.normal(0, 10, nf), rng.uniform(0.5, 2, nf) * 10.0 ** rng.integers(-3, 2)) for name, nf in
          variables.items()]
    layers = {name: sage_layer(rng, ci, co) if kind == "sage" else up_layer(rng, ci, co)
              for name, kind, ci, co, _ in layer_plan(depth, sum(variables.values()), min_filters)}
    return GraphUNetSpec(vs, depth, min_filters, activation, layers)


def make_state(rng, n_samples, n, n_features):
    return rng.normal(0, 1, (n_samples, 6, n, n, n_features)).astype(np.float32)


def make_dataset(rng, spec, n_times, n, dtype=np.float64, order=("time", "tile", "x", "y", "z")):
    """name -> (dims, array) of raw (denormalised) fields ``[time, tile, x, y(, z)]`` stored in the dim order ``order``; a
    one-feature variable has no ``z``."""
    out = {}
    for v in spec.variables:
        a = rng.normal(0, 1, (n_times, 6, n, n, v.nfeat)) * v.std + v.mean
        dims = list(order)
        if v.nfeat == 1:
            a, dims = a[..., 0], [d for d in order if d != "z"]
        canon = [d for d in ("time", "tile", "x", "y", "z") if d in dims]
        out[v.name] = (tuple(dims), np.ascontiguousarray(np.transpose(a.astype(dtype), [canon.index(d) for d in dims])))
    return out


def canonical(dataset):
    """``make_dataset``'s result as name -> ``[time, tile, x, y(, z)]`` arrays, for the oracle."""
    out = {}
    for name, (dims, a) in dataset.items():
        canon = [d for d in ("time", "tile", "x", "y", "z") if d in dims]
        out[name] = np.transpose(a, [dims.index(d) for d in canon])
    return out


def twin_step(spec, dtype=torch.float32):
    """The plain-torch twin on the CPU as a function state -> next state (numpy in and out)."""
    from fv3net_amd.fit.graph import twin_from_spec

    twin = twin_from_spec(spec, dtype)

    def step(state):
        with torch.no_grad():
            return twin(torch.from_numpy(np.ascontiguousarray(state)).to(dtype)).numpy()

    return step


def worst_ratio(got, truth):
    """Worst per-level error / level scale over ``[..., level]`` arrays."""
    got, truth = np.asarray(got, np.float64).reshape(-1, got.shape[-1]), np.asarray(truth, np.float64).reshape(-1, truth.shape[-1])
    scale = np.max(np.abs(truth), axis=0)
    return float(np.max(np.max(np.abs(got - truth), axis=0) / np.where(scale == 0, 1, scale)))


# -- the reference's own known answer (graph/test_graph.py:64-103) ----------------------------------
def flip_series(rng, n_samples, n_batch, n_time, nx, nz):
    """Batches ``a`` [batch, time, 6, nx, nx, nz] and ``b`` [batch, time, 6, nx, nx]: every time is the negation of the one
    before it."""
    sign = (-1.0) ** np.arange(n_time)
    out = []
    for _ in range(n_samples):
        a = rng.uniform(-1, 1, (n_batch, 1, 6, nx, nx, nz)) * sign[None, :, None, None, None, None]
        b = rng.uniform(-1, 1, (n_batch, 1, 6, nx, nx)) * sign[None, :, None, None, None]
        out.append({"a": a, "b": b})
    return out


@functools.lru_cache(maxsize=1)
def trained_flip_model():
    """``GraphUNetConfig`` defaults, 30 epochs, AdamW with lr 0.005, on 20 + 3 batches of 2 samples of the sign-flipping series
    at nx = 6, nz = 2, trained on the CPU with seed 2 (test_host_graph.py says why); and one continuous test series of 100 times.
    Returns (predictor, test arrays).  ``tests/golden/graph_flip_model`` is this predictor, written by ``fit.dump``."""
    from fv3net_amd.fit.graph import GraphHyperparameters, train_graph_model

    rng = np.random.default_rng(0)
    train, valid = flip_series(rng, 20, 2, 2, 6, 2), flip_series(rng, 3, 2, 2, 6, 2)
    test = flip_series(rng, 1, 1, 100, 6, 2)[0]
    hp = GraphHyperparameters(state_variables=["a", "b"], n_epoch=30, optimizer_kwargs={"lr": 0.005}, seed=2)
    predictor = train_graph_model(hp, train, valid, device="cpu")
    return predictor, {"a": test["a"][0], "b": test["b"][0]}


def check_flip_skill(predicted, reference):
    """After one step |mean bias| < 0.1 and rmse < 0.1 for every variable."""
    for name in ("a", "b"):
        bias = np.asarray(predicted[name])[:, 1] - np.asarray(reference[name])[:, 1]
        mean_bias, rmse = float(np.mean(bias)), float(np.sqrt(np.mean(bias ** 2)))
        print(f"flip series, {name}: mean bias {mean_bias:+.4f}, rmse {rmse:.4f}")
        assert abs(mean_bias) < 0.1, (name, mean_bias)
        assert rmse < 0.1, (name, rmse)


# -- single layers on the device and in float32 on the CPU -------------------------------------------
def device_layer(device, kind, h, layer=None, activation="linear", c_out=None, dst=None, dst_off=0, src_off=0, src_width=None):
    """One ``fv3hip_graph_*`` launch on ``h`` ``[S, 6, n, n, c]`` (numpy).  ``src_off`` / ``src_width``: ``h`` is placed at that
    channel offset of a wider NaN-filled buffer; ``dst``: a ``[S, 6, n_out, n_out, ld]`` device tensor to write into at channel
    ``dst_off`` (else a fresh exact-width one).  Returns the destination tensor."""
    import ctypes

    from fv3net_amd import _lib
    from fv3net_amd.graph import ACTIVATIONS
    from fv3net_amd.ops import _stream

    S, _, n, _, c = h.shape
    wide = np.full((S, 6, n, n, src_width or c + src_off), np.nan, np.float32)
    wide[..., src_off:src_off + c] = h
    src = torch.from_numpy(wide).to(device)
    n_out = {"sage": n, "pool2": n // 2, "up2": 2 * n}[kind]
    c_out = c_out or (c if kind == "pool2" else np.asarray(layer.bias).shape[0])
    if dst is None:
        dst = torch.full((S, 6, n_out, n_out, c_out + dst_off), -7.0, dtype=torch.float32, device=device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    st = _stream(device)
    if kind == "sage":
        ws, wn, b = up(layer.w_self), up(layer.w_neigh), up(layer.bias)
        _lib.call_on(device, "fv3hip_graph_sage", src.data_ptr(), src.shape[-1], src_off, 0, ws.data_ptr(), wn.data_ptr(), b.data_ptr(),
                     dst.data_ptr(), dst.shape[-1], dst_off, 0, S, n, c, c_out, ACTIVATIONS[activation], st)
    elif kind == "pool2":
        _lib.call_on(device, "fv3hip_graph_pool2", src.data_ptr(), src.shape[-1], src_off, dst.data_ptr(), dst.shape[-1], dst_off, S, n,
                     c, st)
    else:
        w, b = up(layer.weight), up(layer.bias)
        _lib.call_on(device, "fv3hip_graph_up2", src.data_ptr(), src.shape[-1], src_off, w.data_ptr(), b.data_ptr(), dst.data_ptr(),
                     dst.shape[-1], dst_off, S, n, c, c_out, st)
    torch.cuda.synchronize(device)
    return dst


def twin_sage(layer, h, activation="linear", dtype=torch.float32):
    """One SAGE layer of the plain-torch twin on the CPU."""
    from fv3net_amd.fit.graph import _TORCH_ACTIVATIONS, _SageMean

    c_in, c_out = np.asarray(layer.w_self).shape
    op = _SageMean(c_in, c_out)
    op.load_state_dict({"fc_self.weight": torch.from_numpy(np.ascontiguousarray(layer.w_self.T)),
                        "fc_neigh.weight": torch.from_numpy(np.ascontiguousarray(layer.w_neigh.T)), "bias": torch.from_numpy(np.array(layer.bias))})
    with torch.no_grad():
        return _TORCH_ACTIVATIONS[activation]()(op.to(dtype)(torch.from_numpy(np.ascontiguousarray(h)).to(dtype))).numpy()


def twin_up2(layer, h, dtype=torch.float32):
    """``ConvTranspose2d(c_in, c_out, 2, stride 2)`` per tile in torch on the CPU."""
    S, _, n, _, c = h.shape
    w = torch.from_numpy(np.ascontiguousarray(layer.weight.transpose(0, 3, 1, 2))).to(dtype)      # [c_in, c_out, kx, ky]
    x = torch.from_numpy(np.ascontiguousarray(h)).to(dtype).permute(0, 1, 4, 2, 3).reshape(S * 6, c, n, n)
    y = torch.nn.functional.conv_transpose2d(x, w, torch.from_numpy(np.array(layer.bias)).to(dtype), stride=2)
    return y.reshape(S, 6, -1, 2 * n, 2 * n).permute(0, 1, 3, 4, 2).numpy()
