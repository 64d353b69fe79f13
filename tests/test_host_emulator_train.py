"""The host side of the emulator training, without a GPU: the configuration layer, the normalisation
fits, the restatement tests/emulator_train_np.py against float64 autograd of the torch backend's loss expression, its gates
against a float32 evaluation (and against three wrong ones), and the torch backend of ``fit.train_transformed_model`` on the CPU."""
import copy

import numpy as np
import pytest
import torch

import emulator_train_cases as C
import emulator_train_np as E
import train_np as T
from fv3net_amd import fit
from fv3net_amd.emulation.models import HipEmulator, HipLocalEmulator, load_emulator
from fv3net_amd.emulation.transforms import Difference, LogTransform, TransformedVariableConfig
from fv3net_amd.fit import emulator_train as fe
from oracle import mlp_np

NZ = 5


def dense_yaml():
    """A mapping of the shape of projects/microphysics/train/dense.yaml, cut to 5 levels (the level count is the data's)."""
    return {
        "use_wandb": True, "wandb": {"wandb_project": "microphysics-emulation"}, "batch_size": 512, "epochs": 25, "nfiles_valid": 100,
        "valid_freq": 2, "out_url": "gs://bucket/dense", "train_url": "gs://bucket/train", "test_url": "gs://bucket/test",
        "tensor_transform": [
            {"to": "log_cloud_input", "source": "cloud_water_mixing_ratio_input", "transform": {"epsilon": 1e-10}},
            {"to": "log_humidity_input", "source": "specific_humidity_input", "transform": {"epsilon": 1e-8}},
            {"to": "log_humidity_after_last_gscond", "source": "specific_humidity_after_last_gscond", "transform": {"epsilon": 1e-8}},
            {"to": "temperature_gscond_difference", "before": "air_temperature_input", "after": "air_temperature_after_gscond"},
            {"to": "humidity_gscond_difference", "before": "specific_humidity_input", "after": "specific_humidity_after_gscond"},
            {"to": "cloud_precpd_difference", "before": "cloud_water_mixing_ratio_input", "after": "cloud_water_mixing_ratio_after_precpd"},
            {"to": "temperature_precpd_difference", "before": "air_temperature_input", "after": "air_temperature_after_precpd"},
            {"to": "humidity_precpd_difference", "before": "specific_humidity_input", "after": "specific_humidity_after_precpd"},
        ],
        "loss": {
            "optimizer": {"kwargs": {"learning_rate": 0.0001}, "name": "Adam"},
            "metric_variables": ["air_temperature_after_gscond", "specific_humidity_after_gscond", "air_temperature_after_precpd",
                                 "specific_humidity_after_precpd", "cloud_water_mixing_ratio_after_precpd"],
            "loss_variables": ["total_precipitation", "cloud_precpd_difference", "temperature_precpd_difference",
                               "humidity_precpd_difference", "temperature_gscond_difference", "humidity_gscond_difference"],
            "weights": {"total_precipitation": 1.0, "cloud_precpd_difference": 1.0, "temperature_precpd_difference": 1.0,
                        "humidity_precpd_difference": 1.0, "temperature_gscond_difference": 1.0, "humidity_gscond_difference": 1.0},
        },
        "model": {
            "architecture": {"kwargs": {"width": 256, "depth": 2}, "name": "dense"},
            "input_variables": ["air_temperature_input", "specific_humidity_input", "cloud_water_mixing_ratio_input", "log_cloud_input",
                                "log_humidity_input", "pressure_thickness_of_atmospheric_layer", "air_temperature_after_last_gscond",
                                "specific_humidity_after_last_gscond", "log_humidity_after_last_gscond"],
            "direct_out_variables": ["total_precipitation", "cloud_precpd_difference", "temperature_precpd_difference",
                                     "humidity_precpd_difference", "temperature_gscond_difference", "humidity_gscond_difference"],
            "normalize_default": {"center": "per_feature", "scale": "all"},
            "selection_map": {},
            "timestep_increment_sec": 900,
        },
        "transform": {"antarctic_only": False, "derived_microphys_timestep": 900, "use_tensors": True, "vertical_subselections": None},
    }


def classifier_yaml():
    """The shape of gscond-classifier.yaml's ``config`` without its class and humidity transforms."""
    d = dense_yaml()
    d["tensor_transform"] = d["tensor_transform"][:3]
    d["loss"] = {"optimizer": {"kwargs": {"learning_rate": 0.001}, "name": "Adam"}, "metric_variables": [],
                 "logit_variables": ["gscond_classes"], "weights": {"gscond_classes": 1.0}}
    d["model"] = {
        "architecture": {"kwargs": {"width": 256, "depth": 2}, "name": "dense-local", "output_channels": {"gscond_classes": 4}},
        "input_variables": d["model"]["input_variables"] + ["air_pressure", "surface_air_pressure", "surface_air_pressure_after_last_gscond"],
        "unscaled_outputs": ["gscond_classes"],
        "normalize_default": {"center": "per_feature", "scale": "all"},
        "normalize_map": {"air_pressure": {"center": "all", "scale": "all_center_all"}},
        "selection_map": {}, "timestep_increment_sec": 900,
    }
    return d


# ---- the configuration layer ------------------------------------------------------------------------------------------------------
def test_from_dict_reads_the_dense_configuration():
    hp = fit.TransformedParameters.from_dict(dense_yaml())
    assert (hp.batch_size, hp.epochs, hp.valid_freq, hp.seed, hp.use_wandb, hp.out_url) == (512, 25, 2, 0, True, "gs://bucket/dense")
    assert hp.shuffle_buffer_size == 13824 and hp.checkpoint_model is True and hp.verbose == 2     # the reference's defaults
    assert [type(t) for t in hp.tensor_transform] == [TransformedVariableConfig] * 3 + [Difference] * 5
    assert isinstance(hp.tensor_transform[0].transform, LogTransform) and hp.tensor_transform[0].transform.epsilon == 1e-10
    assert hp.model.architecture == fit.ArchitectureConfig("dense", {"width": 256, "depth": 2})
    assert hp.model.normalize_default == fit.NormFactory(scale="all", center="per_feature")
    assert hp.loss.optimizer == fit.OptimizerConfig("Adam", {"learning_rate": 0.0001})
    assert len(hp.loss.loss_variables) == 6 and len(hp.loss.metric_variables) == 5 and hp.loss.logit_variables == []
    assert hp.loss.normalization == fit.NormFactory("all", "per_feature")


def test_from_dict_reads_the_classifier_configuration():
    hp = fit.TransformedParameters.from_dict(classifier_yaml())
    assert hp.model.architecture.name == "dense-local" and hp.model.architecture.output_channels == {"gscond_classes": 4}
    assert hp.model.unscaled_outputs == ["gscond_classes"] and hp.model.direct_out_variables == []
    assert hp.model.normalize_map == {"air_pressure": fit.NormFactory("all_center_all", "all")}
    assert hp.loss.logit_variables == ["gscond_classes"] and hp.loss.loss_variables == []


def test_defaults_are_the_references():
    hp = fit.TransformedParameters()
    assert (hp.epochs, hp.batch_size, hp.valid_freq, hp.shuffle_buffer_size, hp.checkpoint_interval, hp.seed) == (1, 128, 5, 13824, 1, 0)
    assert fit.MicrophysicsConfig().architecture.name == "linear" and fit.MicrophysicsConfig().timestep_increment_sec == 900
    assert fit.CustomLoss().optimizer.name == "Adam" and fit.CustomLoss().normalization == fit.NormFactory("all", "per_feature")
    assert fit.SliceConfig(1, 4).slice == slice(1, 4, None)


@pytest.mark.parametrize("where", ["top", "model", "loss", "architecture", "optimizer", "norm"])
def test_an_unknown_key_raises(where):
    d = dense_yaml()
    target = {"top": d, "model": d["model"], "loss": d["loss"], "architecture": d["model"]["architecture"],
              "optimizer": d["loss"]["optimizer"], "norm": d["model"]["normalize_default"]}[where]
    target["no_such_key"] = 1
    with pytest.raises(ValueError, match="no_such_key"):
        fit.TransformedParameters.from_dict(d)


def _with(path, value):
    d = dense_yaml()
    node = d
    for key in path[:-1]:
        node = node[key]
    node[path[-1]] = value
    return d


REFUSED = {
    "rnn": (_with(("model", "architecture"), {"name": "rnn"}), "rnn"),
    "rnn-v1": (_with(("model", "architecture"), {"name": "rnn-v1"}), "rnn-v1"),
    "rnn-v1-shared-weights": (_with(("model", "architecture"), {"name": "rnn-v1-shared-weights"}), "rnn-v1-shared-weights"),
    "ZhaoCarrLoss": (_with(("loss",), {"zhao_carr_loss": True, "masked_weight": 2.0}), "ZhaoCarrLoss"),
    "bias_metric_variables": (_with(("loss", "bias_metric_variables"), ["total_precipitation"]), "bias_metric_variables"),
    "kernel_regularizer": (_with(("model", "architecture"), {"name": "dense", "kernel_regularizer": {"name": "l2", "kwargs": {"l2": 1e-4}}}),
                           "kernel_regularizer 'l2'"),
    "filters": (_with(("filters",), [{"high_antarctic_only": True}]), "filters"),
    "ConditionallyScaled": (_with(("tensor_transform",), [{"to": "a", "condition_on": "b", "source": "c", "bins": 50}]), "ConditionallyScaled"),
    "CloudWaterDiffPrecpd": (_with(("tensor_transform",), [{"to": "a", "sphum_source": "b", "cloud_input": "c", "cloud_after_precpd": "d"}]),
                             "CloudWaterDiffPrecpd"),
    "classes": (_with(("tensor_transform",), [{"cloud_in": "cloud_water_mixing_ratio_input", "to": "gscond_classes"}]),
                "MicrophysicsClassesV1OneHot"),
    "GscondRoute": (_with(("tensor_transform",), [{"gscond_route": True}]), "GscondRoute"),
    "RelativeHumidity": (_with(("tensor_transform",), [{"relative_humidity": "relative_humidity"}]), "RelativeHumidity"),
    "LimitValueTransform": (_with(("tensor_transform",), [{"source": "a", "transform": {"lower": 0.0}}]), "LimitValueTransform"),
    "optimizer": (_with(("loss", "optimizer"), {"name": "SGD"}), "SGD"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_each_refused_feature_raises_naming_it(name):
    d, word = REFUSED[name]
    with pytest.raises(NotImplementedError, match=word):
        fit.TransformedParameters.from_dict(d)


def test_refusal_comes_before_the_data_is_touched():
    hp = fit.TransformedParameters.from_dict(C.dense_config())
    hp.model.architecture = fit.ArchitectureConfig("rnn-v1-shared-weights")

    class Untouchable:
        def __iter__(self):
            raise AssertionError("the batches were read")

    with pytest.raises(NotImplementedError, match="rnn-v1-shared-weights"):
        fit.train_transformed_model(hp, Untouchable())
    with pytest.raises(ValueError, match="backend"):
        fit.train_transformed_model(fit.TransformedParameters.from_dict(C.dense_config()), Untouchable(), backend="tensorflow")


def test_required_variables_follow_the_references_set_logic():
    """Difference transforms whose ``after`` fields are loss variables: ``before`` and ``after`` are required, ``to`` is not."""
    hp = fit.TransformedParameters(
        tensor_transform=[TransformedVariableConfig("qc", LogTransform(1e-10), to="log_qc"), Difference("dT", "T_in", "T_after"),
                          Difference("dq", "q_in", "q_after")],
        model=fit.MicrophysicsConfig(input_variables=["T_in", "log_qc"], direct_out_variables=["dT", "dq"],
                                     architecture=fit.ArchitectureConfig("dense")),
        loss=fit.CustomLoss(loss_variables=["T_after", "q_after"]))
    assert hp.input_variables == {"T_in", "qc", "q_in"}
    assert hp.model_variables == {"T_in", "qc", "q_in", "T_after", "q_after"}
    hp.loss = fit.CustomLoss(loss_variables=["dT", "precip"])
    assert hp.model_variables == {"T_in", "qc", "q_in", "T_after", "q_after", "precip"}


# ---- normalisation ------------------------------------------------------------------------------------------------------------------
def test_every_normalisation_method_against_its_definition():
    rng = np.random.default_rng(3)
    x = (rng.normal(0, 1, (7, 3)) * [1.0, 10.0, 0.1] + [250.0, 0.0, -3.0]).astype(np.float32)
    x64 = x.astype(np.float64)
    mean_pf = x64.mean(axis=0)
    std_pf = np.sqrt(((x64 - mean_pf) ** 2).mean(axis=0))
    want_scale = {
        "per_feature": std_pf.astype(np.float32),
        "all": np.float32(np.sqrt(((x64 - mean_pf.astype(np.float32).astype(np.float64)) ** 2).mean())),
        "all_center_all": np.float32(np.sqrt(((x64 - x64.mean()) ** 2).mean())),
        "max": np.float32(std_pf.max()), "mean": np.float32(std_pf.mean()), "none": np.float32(1.0),
    }
    want_center = {"per_feature": mean_pf.astype(np.float32), "all": np.float32(x64.mean()), "none": np.float32(0.0)}
    assert set(want_scale) == set(fe.STD_DEV_METHODS) and set(want_center) == set(fe.MEAN_METHODS)
    for method, want in want_scale.items():
        got = fe.fit_scale(x, method)
        assert got.dtype == np.float32 and np.array_equal(got, want), method
    for method, want in want_center.items():
        got = fe.fit_center(x, method)
        assert got.dtype == np.float32 and np.array_equal(got, want), method
    center, scale, forward = fit.NormFactory("max", "all", epsilon=1e-3).build(x)
    assert np.array_equal(forward, (want_scale["max"] + np.float32(1e-3)).astype(np.float32)) and np.array_equal(scale, want_scale["max"])
    with pytest.raises(ValueError):
        fit.NormFactory("all_all")


# ---- the restatement against autograd, its gates against float32 evaluations ------------------------------------------------------
def _case(kind, seed=11):
    rng = np.random.default_rng(seed)
    if kind == "dense":
        heads, f = C.dense_loss_case(rng, rows=5, nfeat=3)
        levels, n = 1, 5
    else:
        heads, f = C.local_loss_case(rng, rows=3, levels=4)
        levels, n = 4, 3
    yhat = rng.normal(0, 1, (n * levels, f)).astype(np.float32)
    return heads, levels, n, yhat


def _autograd64(heads, levels, n, yhat):
    y = torch.tensor(yhat.astype(np.float64), requires_grad=True)
    loss, values = fe.emulator_loss_torch(y, fe.heads_to_torch(heads, "cpu", torch.float64), torch.arange(n), levels)
    loss.backward()
    return y.grad.numpy(), np.array([float(v.detach()) for v in values]), float(loss.detach())


@pytest.mark.parametrize("kind", ["dense", "local"])
def test_restatement_is_the_gradient_of_the_torch_backends_loss(kind, monkeypatch):
    heads, levels, n, yhat = _case(kind)
    want_dy, want_values, want_loss = _autograd64(heads, levels, n, yhat)
    # (torch.mean divides by the count; the kernel multiplies by the float32 value of weight / count, which is part of its
    # definition: compared unrounded here, and the rounding checked to be no more than that)
    monkeypatch.setattr(E, "EXACT_WGRAD", True)
    dy, values, loss, _, _, _ = E.loss_grad(yhat, heads, levels)
    assert np.max(np.abs(dy - want_dy)) <= 1e-12 * np.max(np.abs(want_dy))
    assert np.max(np.abs(values - want_values) / np.abs(want_values)) <= 1e-12 and abs(loss - want_loss) <= 1e-12 * abs(want_loss)
    monkeypatch.setattr(E, "EXACT_WGRAD", False)
    rounded = E.loss_grad(yhat, heads, levels)[0]
    assert np.max(np.abs(rounded - dy)) <= 2 * T.U * np.max(np.abs(dy)) and not np.array_equal(rounded, dy)
    term_less = [h for h in heads if h.slot is None and h.slot_after is None]
    for h in term_less:
        assert not dy[:, h.col0:h.col0 + h.ncol].any()
    if kind == "local":
        single = heads[1]
        assert single.single_level and not dy.reshape(n, levels, -1)[:, 1:, single.col0].any() and dy.reshape(n, levels, -1)[:, 0, single.col0].all()


def test_a_nan_metric_target_stays_out_of_the_gradient_as_in_the_torch_backend():
    heads, levels, n, yhat = _case("dense")
    metric = heads[4]
    assert metric.slot is not None and not metric.is_loss
    metric.target[1, 0] = np.nan
    heads[1].target_after[2, 1] = np.nan      # the metric-only after term beside a direct loss term
    want_dy, want_values, want_loss = _autograd64(heads, levels, n, yhat)
    dy, values, loss, _, _, _ = E.loss_grad(yhat, heads, levels)
    dy32, values32, loss32 = E.loss_grad32(yhat, heads, levels)
    assert np.isfinite(want_dy).all() and np.isfinite(dy).all() and np.isfinite(dy32).all() and np.isfinite(loss) and np.isfinite(loss32)
    assert not dy[:, metric.col0:metric.col0 + metric.ncol].any()
    nan = np.isnan(values)
    assert nan.sum() == 2 and nan[metric.slot] and nan[heads[1].slot_after] and np.array_equal(np.isnan(want_values), nan)
    assert np.array_equal(np.isnan(values32), nan)


def _worst(got, want, gate):
    ok = gate > 0
    return float(np.max(np.abs(got - want)[ok] / gate[ok])) if ok.any() else 0.0


@pytest.mark.parametrize("kind", ["dense", "local"])
def test_float32_evaluation_stays_inside_the_gates(kind):
    heads, levels, n, yhat = _case(kind)
    dy, values, loss, gate, vgate, lgate = E.loss_grad(yhat, heads, levels)
    dy32, values32, loss32 = E.loss_grad32(yhat, heads, levels)
    assert np.all(np.abs(dy32 - dy) <= gate)
    assert np.all(np.abs(values32 - values) <= vgate) and abs(loss32 - loss) <= lgate
    assert np.all(gate[dy != 0] <= 1e-3 * np.max(np.abs(dy)))   # (a gate as wide as the gradient would hold nothing)


@pytest.mark.parametrize("kind,variant", [("dense", "drop_after_grad"), ("dense", "count_n"), ("local", "st_one"), ("local", "drop_after_grad")])
def test_the_gates_catch_the_three_mistakes(kind, variant):
    heads, levels, n, yhat = _case(kind)
    if kind == "local" and variant == "drop_after_grad":   # (the case's after term is a metric: make it a loss term)
        heads = copy.deepcopy(heads)
        heads[0].is_loss_after = True
    dy, values, _, gate, vgate, _ = E.loss_grad(yhat, heads, levels)
    wrong, wrong_values, _ = E.loss_grad32(yhat, heads, levels, variant=variant)
    if variant == "drop_after_grad":
        h = next(h for h in heads if h.slot_after is not None and h.is_loss_after)
        affected = np.zeros(dy.shape, bool)
        affected[:, h.col0:h.col0 + h.ncol] = True
    elif variant == "count_n":
        affected = np.zeros(dy.shape, bool)
        for h in heads:
            if h.ncol > 1 and ((h.slot is not None and h.is_loss) or (h.slot_after is not None and h.is_loss_after)):
                affected[:, h.col0:h.col0 + h.ncol] = True
        slots = [s for h in heads if h.ncol > 1 for s in (h.slot, h.slot_after) if s is not None]
        assert np.all(np.abs(wrong_values - values)[slots] > vgate[slots])
    else:   # st = 1 is wrong wherever the truth does not add up to one: the soft row's rounding aside, the all-zero row
        h = heads[2]
        affected = np.zeros((n, levels, dy.shape[1]), bool)
        affected[2, :, h.col0:h.col0 + h.ncol] = True
        affected = affected.reshape(dy.shape)
    assert affected.any() and np.all((np.abs(wrong - dy) > gate)[affected])
    assert np.all((np.abs(wrong - dy) <= gate)[~affected])


def test_cross_entropy_of_extreme_logits_is_finite():
    rng = np.random.default_rng(5)
    heads, f = C.make_heads(rng, 3, 2, [("xent", 4, dict(direct=("loss", 1.0)))])
    heads[0].target[:] = np.eye(4, dtype=np.float32)[[[1, 1], [2, 3], [1, 1]]]
    yhat = np.array([[1e4, -1e4, 0, 3], [-1e4, 1e4, 1e4, -1e4], [88.8, 0, -88.8, 1], [0, 88.8, 88.8, 88.8], [1e4, 1e4, 1e4, 1e4],
                     [-1e4, -1e4, -1e4, -1e4]], np.float32)
    dy, values, loss, gate, vgate, _ = E.loss_grad(yhat, heads, 2)
    dy32, values32, loss32 = E.loss_grad32(yhat, heads, 2)
    assert np.isfinite(dy32).all() and np.isfinite(values32).all() and np.isfinite(loss32)
    assert np.all(np.abs(dy32 - dy) <= gate) and np.all(np.abs(values32 - values) <= vgate)
    by_hand = (2e4 + np.log(2) + (np.float32(88.8) * 2 + np.log1p(np.exp(-87.8))) + np.log(3) + 2 * np.log(4)) / 6
    assert abs(values[0] - by_hand) <= 1e-9 * by_hand   # (the first point puts its mass on a class 2e4 below the maximum)


# ---- the torch backend on the CPU -------------------------------------------------------------------------------------------------
ROWS, VALID = 256, 64
CONFIGS = {"dense": lambda **kw: C.dense_config(batch_size=64, **kw), "local": lambda **kw: C.local_config(batch_size=32, **kw)}


def _train(kind, **kw):
    hp = fit.TransformedParameters.from_dict(CONFIGS[kind](**kw))
    return hp, fit.train_transformed_model(hp, C.batches(ROWS, NZ), C.batches(VALID, NZ, seed=1), device="cpu")


@pytest.fixture(scope="module")
def trained():
    return {kind: _train(kind) for kind in CONFIGS}


def _arrays(emulator):
    return emulator.spec.to_arrays()


def _same_spec(a, b):
    (ma, aa), (mb, ab) = _arrays(a), _arrays(b)
    return ma == mb and aa.keys() == ab.keys() and all(np.array_equal(aa[k], ab[k]) and aa[k].dtype == ab[k].dtype for k in aa)


@pytest.mark.parametrize("kind", sorted(CONFIGS))
def test_zero_epochs_return_the_initial_weights(kind):
    hp, result = _train(kind, epochs=0)
    prep = fe._prepare(hp, C.batches(ROWS, NZ), None)
    spec = result.emulator.spec
    for got, want in zip(list(spec.hidden_kernels) + [spec.out_kernel], prep.kernels):
        assert np.array_equal(got, want)
    assert not np.concatenate([b for b in spec.hidden_biases] + [spec.out_bias]).any()
    limit = np.sqrt(6.0 / (prep.kernels[0].shape[0] + prep.kernels[0].shape[1]))   # glorot_uniform
    assert np.abs(prep.kernels[0]).max() <= limit and np.abs(prep.kernels[0]).max() > 0.5 * limit
    assert all(v == [] for v in result.history.values())


@pytest.mark.parametrize("kind", sorted(CONFIGS))
def test_three_epochs_lower_the_loss_and_fill_the_history(kind, trained):
    hp, result = trained[kind]
    h = result.history
    names = hp.loss.loss_variables + hp.loss.logit_variables + hp.loss.metric_variables
    want = {"loss"} | {f"{n}_loss" for n in names}
    assert set(h) == want | {f"val_{k}" for k in want}
    assert all(len(h[k]) == 3 for k in want) and all(len(h[f"val_{k}"]) == 1 for k in want)    # valid_freq 2: epoch 2 only
    assert h["loss"][2] < h["loss"][0] and np.isfinite(h["val_loss"][0])
    weights = hp.loss.weights
    recomputed = sum(weights.get(n, 1.0) * h[f"{n}_loss"][1] for n in hp.loss.loss_variables + hp.loss.logit_variables)
    assert abs(recomputed - h["loss"][1]) <= 1e-5 * h["loss"][1]
    assert isinstance(result.emulator, HipEmulator if kind == "dense" else HipLocalEmulator)
    assert [type(t) for t in result.transform.transforms] == [type(t) for t in hp.tensor_transform]


@pytest.mark.parametrize("kind", sorted(CONFIGS))
def test_the_same_seed_gives_the_same_model_bitwise(kind, trained):
    _, again = _train(kind)
    assert _same_spec(trained[kind][1].emulator, again.emulator) and again.history == trained[kind][1].history
    _, other = _train(kind, seed=1)
    assert not _same_spec(trained[kind][1].emulator, other.emulator)


@pytest.mark.parametrize("kind", sorted(CONFIGS))
def test_the_emulator_survives_dump_and_load_bitwise(kind, trained, tmp_path):
    emulator = trained[kind][1].emulator
    emulator.dump(str(tmp_path / kind))
    loaded = load_emulator(str(tmp_path / kind))
    assert type(loaded) is type(emulator) and _same_spec(loaded, emulator)


@pytest.mark.parametrize("kind", sorted(CONFIGS))
def test_the_spec_reproduces_the_torch_models_outputs(kind, trained):
    """The exported spec through the numpy oracle of the predict graph (float64, from the untransformed state) against the
    training graph's own float32 outputs on 8 rows, ``after`` fields included.  The gate is the restatement's: the bound of
    the resident input (``_spec_input``) carried through the layers by ``train_np._contract``; an output adds
    2 U (|y s| + |c|), an ``after`` field U (|before| + |p|); doubled."""
    hp, result = trained[kind]
    spec = result.emulator.spec
    state = {k: v[:8] for k, v in C.state(ROWS, NZ).items()}
    want = (mlp_np.forward_local if kind == "local" else mlp_np.forward)(spec, {k: state[k] for k in spec.sources}, dtype=np.float64)
    L = NZ
    x32, e = _spec_input(spec, state, kind)
    h, x = torch.from_numpy(x32), x32.astype(np.float64)
    kernels, biases = list(spec.hidden_kernels) + [spec.out_kernel], list(spec.hidden_biases) + [spec.out_bias]
    for l, (w, b) in enumerate(zip(kernels, biases)):
        e = T._contract(x, e, w.astype(np.float64), np.zeros(w.shape), w.shape[0] + 1, np.abs(b.astype(np.float64)))
        h = h @ torch.from_numpy(w) + torch.from_numpy(b)
        x = x @ w.astype(np.float64) + b.astype(np.float64)
        if l + 1 < len(kernels):
            h, x = torch.relu(h), np.maximum(x, 0)
    yhat, c0 = h.numpy(), 0
    assert yhat.dtype == np.float32
    checked = 0
    for o in spec.outputs:
        ncol = o.channels if kind == "local" else o.nfeat
        y, ey = yhat[:, c0:c0 + ncol], e[:, c0:c0 + ncol]
        c0 += ncol
        if kind == "local":
            y, ey = (y.reshape(8, L, ncol), ey.reshape(8, L, ncol)) if ncol > 1 else (y.reshape(8, L), ey.reshape(8, L))
        if o.scale is not None:
            s, c = np.atleast_1d(o.scale).astype(np.float32), np.atleast_1d(o.center).astype(np.float32)
            p = y * s + c
            ep = 2 * T.U * (np.abs(y * s) + np.abs(c)) + ey * np.abs(s)
        else:
            p, ep = y, ey
        assert p.dtype == np.float32 and np.all(np.abs(p - want[o.name]) <= 2 * ep + 1e-37), o.name
        checked += 1
        before = getattr(o, "before", None) or next((r.source for r in getattr(spec, "residuals", []) if r.output == o.name), None)
        if before is not None:
            after_name = getattr(o, "after", None) or next(r.name for r in spec.residuals if r.output == o.name)
            b32 = np.asarray(state[before], np.float32)
            after = b32 + p
            ea = ep + T.U * (np.abs(b32) + np.abs(p))
            assert after.dtype == np.float32 and np.all(np.abs(after - want[after_name]) <= 2 * ea), after_name
            assert np.max(2 * ea) < 1e-4 * np.max(np.abs(after))
            checked += 1
    assert checked == len(spec.output_names)


def _spec_input(spec, state, kind):
    """The network input of the spec on ``state`` in float32, the arithmetic of the shared preparation, ``(x - center) / scale``,
    and its bound: 2 U |x| for the difference and the quotient, 3 ulp of ``|log a|`` through ``1 / scale`` for a log input;
    doubled."""
    cols, errs = [], []
    for i in spec.inputs:
        a = np.asarray(state[i.source], np.float32)
        a = a[:, None] if a.ndim == 1 else a
        if kind == "dense":
            a = a[:, i.start:i.start + i.nfeat]
        e = np.zeros(a.shape)
        if i.transform == "log":
            a = np.log(np.maximum(a, np.float32(i.eps)))
            e = 3 * T.U * np.abs(a.astype(np.float64))
        if i.center is not None:
            c, sc = np.asarray(i.center, np.float32), np.asarray(i.scale, np.float32)
            e = (e + T.U * (np.abs(a) + np.abs(c))) / np.abs(sc)
            a = ((a - c) / sc).astype(np.float32)
            e = e + T.U * np.abs(a)
        cols.append(a)
        errs.append(2 * e)
    if kind == "dense":
        return np.ascontiguousarray(np.concatenate(cols, axis=1), np.float32), np.concatenate(errs, axis=1)
    nz = max(c.shape[1] for c in cols)
    stack = lambda vs, dt: np.ascontiguousarray(np.stack([np.broadcast_to(c, (c.shape[0], nz)) for c in vs], axis=2).reshape(-1, len(vs)), dt)  # noqa: E731
    return stack(cols, np.float32), stack(errs, np.float64)
