"""The random-forest kernels at their edges on the MI355X, bit for bit: inputs next to every threshold (float32, and
float64 whose rounding decides), inputs sklearn refuses, layouts and strides, the sum kernel's unrolled body, tail and
both vector widths, single-leaf and chain trees, special values, the limits of the node code word, non-finite model
values, more trees than one launch holds, and one handle at many sizes.

The reference is sklearn's own ``apply`` / ``predict`` wherever sklearn accepts the input, else ``forest_np`` (proved
against sklearn, and shown to discriminate on these very inputs, in ``test_host_forest.py``).  No tolerances."""
import numpy as np
import pytest
import torch

from fv3net_amd import _lib
from fv3net_amd.forest import ForestInput, ForestModel, ForestOutput, ForestSpec, tree_arrays

import forest_np

pytestmark = pytest.mark.gpu


def _sklearn_forest(kind):
    pytest.importorskip("sklearn.ensemble")
    return forest_np.sklearn_forest(kind)


def _to(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _scaler(n_out, seed=0):
    rng = np.random.default_rng(seed)
    return rng.normal(size=n_out), rng.uniform(0.5, 2.0, n_out)


def _model(trees, n_in, device, mean=None, std=None):
    n_out = trees["leaf_values"].shape[1]
    spec = ForestSpec([ForestInput("x", n_in)], [ForestOutput("y", n_out)], trees,
                      np.zeros(n_out) if mean is None else mean, np.ones(n_out) if std is None else std)
    return ForestModel(spec, device=device)


def _run(model, X, device):
    """(leaf ids [tree, sample], outputs [sample, n_out]) of inputs [sample, feature]."""
    xt = _to(X.T, device)
    return model.apply({"x": xt}).cpu().numpy(), model.predict({"x": xt})["y"].cpu().numpy().T


def _check_against_forest_np(trees, X, device, mean=None, std=None, name=""):
    n_out = trees["leaf_values"].shape[1]
    mean, std = (np.zeros(n_out), np.ones(n_out)) if mean is None else (mean, std)
    leaves, y = _run(_model(trees, X.shape[1], device, mean, std), X, device)
    want = forest_np.walk_stumps(trees, X) if forest_np.is_stumps(trees) else forest_np.walk(trees, X)
    np.testing.assert_array_equal(leaves, want, err_msg=name)
    forest_np.assert_same_bits(y, forest_np.denormalize(forest_np.forest_sum(trees, want), mean, std), name)
    return want


# ---- a. threshold neighbours -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", forest_np.SKLEARN_KINDS)
def test_threshold_neighbours_match_sklearn(device, kind, dtype):
    forest, X_train = _sklearn_forest(kind)
    if dtype == np.float32:
        X = forest_np.probe_inputs(forest, X_train, np.random.default_rng(1))
    else:  # every row decides by how a float64 rounds to float32; then the training rows, NaNs included
        X = np.concatenate([forest_np.float64_probes(forest, np.nan_to_num(X_train), np.random.default_rng(2)),
                            X_train.astype(np.float64)])
    assert X.dtype == dtype and 300 <= X.shape[0] < 10000
    mean, std = _scaler(forest.n_outputs_)
    leaves, y = _run(_model(tree_arrays(forest), 6, device, mean, std), X, device)
    np.testing.assert_array_equal(leaves.T, forest.apply(X))
    forest_np.assert_same_bits(y, forest_np.sklearn_predict(forest, X, mean, std))


# ---- b. inputs sklearn refuses -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32_inf", "f64_beyond_f32"])
@pytest.mark.parametrize("kind", ["rf_nan_depth8", "rf_depth13"])
def test_inputs_sklearn_refuses(device, kind, dtype):
    forest, X_train = _sklearn_forest(kind)
    X = forest_np.unrepresentable_inputs(forest, X_train, np.random.default_rng(3), dtype)
    mean, std = _scaler(forest.n_outputs_)
    _check_against_forest_np(tree_arrays(forest), X, device, mean, std)


# ---- c. layouts and strides --------------------------------------------------------------------------------------
def _step2(t, axis):
    """``t`` as every second element along ``axis`` of an array twice as long (NaN in between)."""
    shape = list(t.shape)
    shape[axis] *= 2
    big = torch.full(shape, float("nan"), dtype=t.dtype, device=t.device)
    idx = [slice(None)] * t.dim()
    idx[axis] = slice(None, None, 2)
    big[tuple(idx)] = t
    view = big[tuple(idx)]
    assert view.shape == t.shape and view.stride(axis) == 2 * t.stride(axis)
    return view


@pytest.fixture(scope="module")
def layout_case(device):
    """Three sources (float32 clipped to start=3, float64, 1-D float32) -> outputs of 5 and 2 features."""
    sklearn_ensemble = pytest.importorskip("sklearn.ensemble")
    rng = np.random.default_rng(21)
    X_train = rng.normal(size=(300, 8)).astype(np.float32)
    y = np.stack([np.sin(X_train[:, i] * (1 + i % 5)) + 0.1 * rng.normal(size=300) for i in range(7)], axis=1)
    X_train[rng.uniform(size=X_train.shape) < 0.1] = np.nan
    forest = sklearn_ensemble.RandomForestRegressor(n_estimators=7, max_depth=8, random_state=0, n_jobs=1).fit(X_train, y)
    X = forest_np.probe_inputs(forest, X_train, rng)
    mean, std = _scaler(7, seed=22)
    spec = ForestSpec([ForestInput("a", 4, start=3), ForestInput("b", 3), ForestInput("c", 1)],
                      [ForestOutput("p", 5), ForestOutput("q", 2)], tree_arrays(forest), mean, std)
    model = ForestModel(spec, device=device)
    n = X.shape[0]
    a = np.full((7, n), np.nan, np.float32)  # (the rows below the clip start are never read)
    a[3:] = X[:, :4].T
    src = {"a": _to(a, device), "b": _to(X[:, 4:7].T.astype(np.float64), device), "c": _to(X[:, 7], device)}
    return forest, model, X, src, mean, std


def _both(model, src, layout):
    """(leaf ids [tree, sample], outputs [7, sample]) whatever the layout."""
    leaves = model.apply(src, layout=layout).cpu().numpy()
    out = model.predict(src, layout=layout)
    for name, nf in (("p", 5), ("q", 2)):
        assert out[name].is_contiguous() and out[name].dtype == torch.float64
        assert out[name].shape == ((nf, leaves.shape[1]) if layout == "feature_sample" else (leaves.shape[1], nf))
    y = torch.cat([out["p"], out["q"]], dim=0 if layout == "feature_sample" else 1).cpu().numpy()
    return leaves, y if layout == "feature_sample" else y.T


def _transposed(src):
    return {k: v.T.contiguous() if v.dim() == 2 else v for k, v in src.items()}


def test_layouts_contiguous_match_sklearn(layout_case):
    forest, model, X, src, mean, std = layout_case
    leaves, y = _both(model, src, "feature_sample")
    np.testing.assert_array_equal(leaves.T, forest.apply(X))
    forest_np.assert_same_bits(y.T, forest_np.sklearn_predict(forest, X, mean, std))
    leaves_sf, y_sf = _both(model, _transposed(src), "sample_feature")
    np.testing.assert_array_equal(leaves_sf, leaves)
    forest_np.assert_same_bits(y_sf, y)


@pytest.mark.parametrize("layout", ["feature_sample", "sample_feature"])
@pytest.mark.parametrize("variant", ["step2_samples", "step2_features", "transposed_view", "more_features"])
def test_layouts_strided_equal_contiguous(layout_case, layout, variant):
    forest, model, X, src, mean, std = layout_case
    want_leaves, want = _both(model, src, "feature_sample")
    fs = layout == "feature_sample"
    s = src if fs else _transposed(src)
    sample_axis = 1 if fs else 0
    if variant == "step2_samples":
        s = {k: _step2(v, sample_axis if v.dim() == 2 else 0) for k, v in s.items()}
    elif variant == "step2_features":  # (the 1-D source as the 2-D array it stands for)
        s = {k: _step2(v if v.dim() == 2 else v.unsqueeze(1 - sample_axis), 1 - sample_axis) for k, v in s.items()}
    elif variant == "transposed_view":  # the other layout's memory, seen through .T
        s = {k: v.T if v.dim() == 2 else v for k, v in (_transposed(src) if fs else src).items()}
        assert not s["a"].is_contiguous()
    else:
        nan = {k: torch.full_like(v, float("nan")) for k, v in s.items()}
        s = {"a": torch.cat([s["a"], nan["a"][:3] if fs else nan["a"][:, :3]], 1 - sample_axis),
             "b": torch.cat([s["b"], nan["b"]], 1 - sample_axis), "c": s["c"]}
        assert s["a"].shape[1 - sample_axis] == 10 and s["b"].shape[1 - sample_axis] == 6
    leaves, y = _both(model, s, layout)
    np.testing.assert_array_equal(leaves, want_leaves)
    forest_np.assert_same_bits(y, want)


@pytest.mark.parametrize("layout", ["feature_sample", "sample_feature"])
def test_layouts_zero_stride_source(layout_case, layout):
    """One column of the float32 source broadcast over the samples (``expand``: sample stride 0)."""
    forest, model, X, src, mean, std = layout_case
    n = X.shape[0]
    column = src["a"][:, 5:6].contiguous()
    if layout == "feature_sample":
        s = {"a": column.expand(7, n), "b": src["b"], "c": src["c"]}
        assert s["a"].stride() == (1, 0)
    else:
        s = {"a": column.T.expand(n, 7), "b": src["b"].T.contiguous(), "c": src["c"]}
        assert s["a"].stride() == (0, 1)
    want_leaves, want = _both(model, {"a": column.repeat(1, n), "b": src["b"], "c": src["c"]}, "feature_sample")
    leaves, y = _both(model, s, layout)
    np.testing.assert_array_equal(leaves, want_leaves)
    forest_np.assert_same_bits(y, want)
    Xb = X.copy()
    Xb[:, :4] = X[5, :4]
    np.testing.assert_array_equal(leaves.T, forest.apply(Xb))
    forest_np.assert_same_bits(y.T, forest_np.sklearn_predict(forest, Xb, mean, std))


# ---- d. the sum kernel's shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", forest_np.SUM_N_OUT)
@pytest.mark.parametrize("T", forest_np.SUM_T)
def test_sum_kernel_shapes(device, T, n_out):
    """Eight trees per unrolled step, then a tail; one output per lane (n_out == 1) or two, the odd row padded."""
    trees, X, mean, std = forest_np.sum_case(T, n_out)
    _check_against_forest_np(trees, X, device, mean, std)


# ---- e. tree shapes ------------------------------------------------------------------------------------------------
def test_single_leaf_forest(device):
    rng = np.random.default_rng(40)
    X = rng.normal(size=(100, 2)).astype(np.float32)
    X[::7, 0] = np.nan
    trees = forest_np.single_leaf(1, value=[0.1])
    leaves = _check_against_forest_np(trees, X, device, np.asarray([0.3]), np.asarray([3.0]))
    assert (leaves == 0).all()
    seven = forest_np.concat_forests(*[forest_np.single_leaf(3, value=rng.normal(size=3)) for _ in range(7)])
    _check_against_forest_np(seven, X, device, *_scaler(3))


def test_single_leaf_trees_among_stumps(device):
    rng = np.random.default_rng(41)
    leaf = [forest_np.single_leaf(2, value=rng.normal(size=2)) for _ in range(3)]
    trees = forest_np.concat_forests(leaf[0], forest_np.stumps(5, 3, 2, rng), leaf[1], forest_np.stumps(4, 3, 2, rng), leaf[2])
    X = rng.normal(size=(500, 3)).astype(np.float32)
    X[rng.uniform(size=X.shape) < 0.1] = np.nan
    leaves = _check_against_forest_np(trees, X, device, *_scaler(2))
    assert (leaves[[0, 6, 11]] == 0).all() and (leaves[1:6] > 0).all()


@pytest.mark.parametrize("side", ["left", "right"])
def test_chain_ends_at_every_depth(device, side):
    depth = 200
    rng = np.random.default_rng(4)
    trees = forest_np.chain(depth, side, 3, 2, rng)
    X = forest_np.chain_inputs(depth, 3, rng)
    leaves = _check_against_forest_np(trees, X, device, *_scaler(2))
    assert {2 * depth - 1, 2 * depth} <= set(leaves[0].tolist())  # the pair of leaves at exactly `depth`
    assert set(leaves[0].tolist()) == set(np.flatnonzero(trees["children_left"] == -1).tolist())


# ---- f. special values -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_special_thresholds_and_inputs(device, dtype):
    """Thresholds +inf, +-0, the smallest subnormal, 1e-40 and +-max against themselves, their float32 neighbours, +-0,
    NaN and +-inf; as float64 also 1e39, 1e-40, 1e-46 and values just beyond the largest float32."""
    trees, X = forest_np.special_value_case(dtype)
    assert X.dtype == dtype
    _check_against_forest_np(trees, X, device, *_scaler(2))


# ---- g. the node code word ---------------------------------------------------------------------------------------
def test_thirty_two_sources(device):
    trees, X, starts = forest_np.packing_case()
    mean, std = _scaler(3)
    inputs = [ForestInput(f"s{i}", 1, start=int(starts[i])) for i in range(forest_np.PACK_N)]
    model = ForestModel(ForestSpec(inputs, [ForestOutput("y", 3)], trees, mean, std), device=device)
    src = {}
    for i in range(forest_np.PACK_N):
        a = np.full((starts[i] + 1, X.shape[0]), np.nan, np.float64 if i % 2 else np.float32)
        a[starts[i]] = X[:, i]
        src[f"s{i}"] = _to(a, device)
    want = forest_np.walk_stumps(trees, X)
    np.testing.assert_array_equal(model.apply(src).cpu().numpy(), want)
    got = model.predict(src)["y"].cpu().numpy().T
    forest_np.assert_same_bits(got, forest_np.denormalize(forest_np.forest_sum(trees, want), mean, std))


def test_thirty_two_outputs(device):
    rng = np.random.default_rng(32)
    trees = forest_np.stumps(9, 4, 32, rng)
    X = rng.normal(size=(300, 4)).astype(np.float32)
    mean, std = _scaler(32)
    outputs = [ForestOutput(f"o{j}", 1) for j in range(32)]
    model = ForestModel(ForestSpec([ForestInput("x", 4)], outputs, trees, mean, std), device=device)
    want = forest_np.predict(trees, X, mean, std)
    for layout in ("feature_sample", "sample_feature"):
        out = model.predict({"x": _to(X.T if layout == "feature_sample" else X, device)}, layout=layout)
        assert list(out) == [f"o{j}" for j in range(32)]
        got = np.concatenate([out[f"o{j}"].cpu().numpy().reshape(-1, 1) for j in range(32)], axis=1)
        forest_np.assert_same_bits(got, want, layout)


@pytest.mark.parametrize("which, message", [("sources", "n_sources must be in [1, 32], got 33"),
                                            ("outputs", "n_outputs must be in [1, 32], got 33")])
def test_thirty_three_are_refused(device, which, message):
    rng = np.random.default_rng(33)
    n_in, n_out = (33, 2) if which == "sources" else (2, 33)
    trees = forest_np.stumps(3, n_in, n_out, rng)
    spec = ForestSpec([ForestInput(f"s{i}", 1) for i in range(n_in)], [ForestOutput(f"o{j}", 1) for j in range(n_out)],
                      trees, np.zeros(n_out), np.ones(n_out))
    with pytest.raises(_lib.Fv3HipError) as err:
        ForestModel(spec, device=device)
    assert err.value.code == _lib.EINVAL
    assert message in str(err.value)


# ---- h. non-finite model values ------------------------------------------------------------------------------------
def test_non_finite_leaf_values_mean_and_std(device):
    trees, X = forest_np.non_finite_model_case()
    ordinary = np.asarray([0.5, -1.5, 2.0, 1.0, -0.25])
    for k, (mean, std) in enumerate([(ordinary, np.abs(ordinary))] + forest_np.non_finite_scalers()):
        _check_against_forest_np(trees, X, device, mean, std, name=f"scaler {k}")
    finite = {k: v for k, v in trees.items()}
    finite["leaf_values"] = np.random.default_rng(12).normal(size=trees["leaf_values"].shape)
    for k, (mean, std) in enumerate(forest_np.non_finite_scalers()):
        _check_against_forest_np(finite, X, device, mean, std, name=f"finite leaves, scaler {k}")


# ---- i. more trees than one launch -----------------------------------------------------------------------------------
def test_more_trees_than_one_launch(device):
    """65540 stumps: the walk takes two launches per slab (65535 trees, then 5), and 1100 samples take three slabs."""
    T, n = 65535 + 5, 1100
    slab = (128 << 20) // (4 * T)  # kLeafScratchBytes / (T * sizeof(int32_t)) in csrc/forest.hip
    assert n > 2 * slab
    rng = np.random.default_rng(65)
    trees = forest_np.stumps(T, 4, 3, rng)
    X = rng.normal(size=(n, 4)).astype(np.float32)
    X[rng.uniform(size=X.shape) < 0.05] = np.nan
    mean, std = _scaler(3)
    want_leaves = forest_np.walk_stumps(trees, X)
    want = forest_np.denormalize(forest_np.forest_sum(trees, want_leaves), mean, std)
    model = _model(trees, 4, device, mean, std)
    fs, sf = _to(X.T, device), _to(X, device)
    leaves = model.apply({"x": fs})
    assert leaves.dtype == torch.int32 and torch.equal(leaves, _to(want_leaves, device))  # (compared where they lie: 288 MB)
    assert torch.equal(model.apply({"x": sf}, layout="sample_feature"), leaves)
    full = model.predict({"x": fs})["y"].cpu().numpy().T
    forest_np.assert_same_bits(full, want)
    forest_np.assert_same_bits(model.predict({"x": sf}, layout="sample_feature")["y"].cpu().numpy(), want)
    # the bits depend on neither the slab nor the grid: the first and the last hundred samples alone
    for part in (slice(0, 100), slice(n - 100, n)):
        alone = model.predict({"x": fs[:, part].contiguous()})["y"].cpu().numpy().T
        forest_np.assert_same_bits(alone, full[part])


# ---- j. one handle, many sizes -------------------------------------------------------------------------------------
def test_one_handle_small_large_small_empty_large(device):
    rng = np.random.default_rng(50)
    trees = forest_np.stumps(33, 5, 3, rng)
    mean, std = _scaler(3)
    model = _model(trees, 5, device, mean, std)
    for n in (1, 5000, 63, 0, 5000):
        X = rng.normal(size=(n, 5)).astype(np.float32)
        X[rng.uniform(size=X.shape) < 0.1] = np.nan
        leaves, y = _run(model, X, device)
        assert leaves.shape == (33, n) and leaves.dtype == np.int32 and y.shape == (n, 3)
        want = forest_np.walk_stumps(trees, X)
        np.testing.assert_array_equal(leaves, want, err_msg=f"n = {n}")
        forest_np.assert_same_bits(y, forest_np.denormalize(forest_np.forest_sum(trees, want), mean, std), f"n = {n}")
    empty = model.predict({"x": torch.empty((0, 5), dtype=torch.float64, device=device)}, layout="sample_feature")["y"]
    assert empty.shape == (0, 3) and empty.dtype == torch.float64
