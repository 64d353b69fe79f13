"""The random-forest predictor: ``fv3fit.sklearn.RandomForest`` (registered ``"sklearn"``,
external/fv3fit/fv3fit/sklearn/_random_forest.py:65-377), predicting on the MI355X.

``train_random_forest`` (the reference's ``"sklearn_random_forest"`` training function, _random_forest.py:39-62) grows the trees
on the device (``fv3net_amd.forest_train``, csrc/forest_train.hip): the trees of sklearn's ``RandomForestRegressor`` with the
same hyperparameters and ``random_state`` -- the same partition of the training samples into leaves, leaf values equal to
rounding.  ``from_sklearn`` exports a forest that sklearn fitted (``RandomForestRegressor`` / ``ExtraTreesRegressor``) to the same
plain arrays (``fv3net_amd.forest.tree_arrays``); ``predict`` runs ``fv3hip_forest_predict`` and returns what
``SklearnWrapper.predict`` returns, bit for bit.  The artifact is ``name`` ("sklearn") + ``forest.npz`` + ``metadata.yaml``,
nothing executable.  ``load`` also reads a directory in the reference's own layout (``sklearn.pkl`` + ``scaler.bin`` +
``metadata.bin``) where sklearn and joblib import, converting it on the way.
"""
import dataclasses
import io as _bytes_io
import os
from typing import Dict, Hashable, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import yaml

from ..cubedsphere._device import compute_device, download_all
from ..forest import TREE_ARRAYS, TREE_STATS, ForestInput, ForestModel, ForestOutput, ForestSpec, tree_arrays
from ..xr_compat import DataArray, Dataset, from_compat, to_compat
from . import io
from .input_sensitivity import InputSensitivity, RandomForestInputSensitivity
from .novelty import Clip, _slice
from .predictor import Predictor
from .stacking import column_sources, match_prediction_to_input_coords

_FOREST_ESTIMATORS = ("RandomForestRegressor", "ExtraTreesRegressor")


def _is_forest(regressor) -> bool:
    try:
        import sklearn.ensemble as ens
    except ImportError:  # the class name is all there is to go by
        return type(regressor).__name__ in _FOREST_ESTIMATORS
    return isinstance(regressor, tuple(getattr(ens, n) for n in _FOREST_ESTIMATORS))


@io.register("sklearn")
class RandomForest(Predictor):
    """A fitted tree ensemble over packed column inputs, denormalised by the target scaler's ``mean`` / ``std``."""

    _ARRAYS_NAME = "forest.npz"
    _METADATA_NAME = "metadata.yaml"
    # the reference's own layout (SklearnWrapper, _random_forest.py:187-189)
    _PICKLE_NAME = "sklearn.pkl"
    _SCALER_NAME = "scaler.bin"
    _REF_METADATA_NAME = "metadata.bin"

    def __init__(self, input_variables: Sequence[Hashable], output_variables: Sequence[Hashable],
                 output_features: Sequence[int], trees: Mapping[str, np.ndarray], n_features_in: int, mean: np.ndarray,
                 std: np.ndarray, clip: Optional[Clip] = None, predict_columns: bool = True):
        """``trees``: ``fv3net_amd.forest.TREE_ARRAYS``; ``output_features``: the features of each output variable
        (``PackingInfo.features``); ``n_features_in``: the packed input features the forest was fitted on."""
        super().__init__(list(input_variables), list(output_variables))
        self.output_features = [int(f) for f in output_features]
        if len(self.output_features) != len(self.output_variables):
            raise ValueError("output_features needs one feature count per output variable")
        self.trees = {k: np.asarray(trees[k]) for k in TREE_ARRAYS}
        if all(k in trees for k in TREE_STATS):  # (a forest exported before the statistics were kept has none)
            self.trees.update({k: np.asarray(trees[k]) for k in TREE_STATS})
        self.n_features_in = int(n_features_in)
        self.mean = np.asarray(mean, np.float64).reshape(-1)
        self.std = np.asarray(std, np.float64).reshape(-1)
        n_out = sum(self.output_features)
        if self.trees["leaf_values"].shape[1:] != (n_out,) or self.mean.shape != (n_out,) or self.std.shape != (n_out,):
            raise ValueError(f"leaf values {self.trees['leaf_values'].shape}, mean {self.mean.shape} and std {self.std.shape} "
                             f"do not match the {n_out} output features")
        self.clip = {k: dict(v) for k, v in (clip or {}).items()}
        for name in self.clip:
            if name in self.output_variables:
                raise NotImplementedError("Clipping for ML outputs is not implemented.")
            if _slice(self.clip, name).step not in (None, 1):
                raise NotImplementedError(f"clip of {name!r} has a step; only contiguous level ranges are supported")
        self.predict_columns = bool(predict_columns)
        self._models: Dict[Tuple, ForestModel] = {}  # by the inputs' feature ranges; created on first predict

    @property
    def n_trees(self) -> int:
        return int(self.trees["node_offset"].shape[0]) - 1

    # -- export ------------------------------------------------------------------------------
    @classmethod
    def from_sklearn(cls, regressor, input_variables, output_variables, output_features, mean, std,
                     clip: Optional[Clip] = None, predict_columns: bool = True) -> "RandomForest":
        """A fitted ``RandomForestRegressor`` or ``ExtraTreesRegressor`` (the reference's ``SklearnWrapper.model``) with
        its target scaler's ``mean`` / ``std`` and the wrapper's ``output_features_.features``."""
        if not _is_forest(regressor):
            raise NotImplementedError(f"{type(regressor).__name__} is not a tree ensemble this package can run; "
                                      f"supported: {', '.join(_FOREST_ESTIMATORS)}")
        return cls(input_variables, output_variables, output_features, tree_arrays(regressor), regressor.n_features_in_,
                   mean, std, clip=clip, predict_columns=predict_columns)

    # -- prediction --------------------------------------------------------------------------
    def _spec(self, nfeat: Mapping[Hashable, int]) -> ForestSpec:
        inputs = []
        for name in self.input_variables:
            levels = range(nfeat[name])[_slice(self.clip, name)]
            inputs.append(ForestInput(str(name), len(levels), levels.start if len(levels) else 0))
        total = sum(i.nfeat for i in inputs)
        if total != self.n_features_in or any(i.nfeat == 0 for i in inputs):
            raise ValueError(f"X has {total} features, but the forest is expecting {self.n_features_in} features as input")
        outputs = [ForestOutput(str(n), f) for n, f in zip(self.output_variables, self.output_features)]
        return ForestSpec(inputs, outputs, self.trees, self.mean, self.std)

    def _model(self, spec: ForestSpec) -> ForestModel:
        key = tuple((i.start, i.nfeat) for i in spec.inputs)
        if key not in self._models:
            self._models[key] = ForestModel(spec, device=compute_device())
        return self._models[key]

    def predict(self, X):
        """Predict an output dataset from an input dataset (SklearnWrapper.predict, _random_forest.py:261-271).  Does not
        mutate ``X``; host data in, host data out; device data in, device data out."""
        x = to_compat(X)
        unstacked = ["z"] if self.predict_columns else []
        sources, sample_dims, sizes, _, host_input = column_sources(x, self.input_variables, unstacked)
        spec = self._spec({name: int(t.shape[0]) for name, t in sources.items()})
        outs = self._model(spec).predict({str(k): v for k, v in sources.items()}, layout="feature_sample")
        shaped, dims_of = {}, {}
        for name, nf in zip(self.output_variables, self.output_features):
            t = outs[str(name)]
            if nf == 1:  # unpack -> to_unstacked_dataset drops a one-feature dim
                shaped[name], dims_of[name] = t.reshape([sizes[d] for d in sample_dims]), tuple(sample_dims)
            else:
                shaped[name] = t.reshape([nf] + [sizes[d] for d in sample_dims])
                dims_of[name] = ("z",) + tuple(sample_dims)
        if not (isinstance(host_input, torch.Tensor) and host_input.is_cuda):
            shaped = download_all(shaped)
        result = Dataset()
        for name in self.output_variables:
            result[name] = DataArray(shaped[name], dims=dims_of[name])
        return from_compat(match_prediction_to_input_coords(x, result), X)

    # -- sensitivity -------------------------------------------------------------------------
    def feature_importances(self) -> np.ndarray:
        """[tree, packed input feature]: sklearn's ``feature_importances_`` of every tree."""
        from ..forest_train import feature_importances

        if not all(k in self.trees for k in TREE_STATS):
            raise NotImplementedError("this forest carries no impurity statistics (" + ", ".join(TREE_STATS) + "): it was exported "
                                      "before they were kept; export it again from the fitted estimator, or train it here")
        return feature_importances(self.trees, self.n_features_in)

    def input_sensitivity(self, stacked_sample) -> InputSensitivity:
        """Mean and standard deviation over the trees of sklearn's feature importances, grouped by input variable
        (_random_forest.py:127-172).  ``stacked_sample`` holds the inputs as ``[sample, feature]`` (``[sample]``: a scalar, whose
        index is NaN); it is read for its feature counts only."""
        importances = self.feature_importances()
        mean, std = importances.mean(axis=0), importances.std(axis=0)
        sample = to_compat(stacked_sample)
        out, col = {}, 0
        for name in self.input_variables:
            values = sample[name].values
            if values.ndim == 1:
                indices: List = [float("nan")]
            else:
                indices = list(range(len(range(values.shape[-1])[_slice(self.clip, name)])))
            nf = len(indices)
            out[name] = RandomForestInputSensitivity(mean_importances=mean[col:col + nf].tolist(),
                                                     std_importances=std[col:col + nf].tolist(), indices=indices)
            col += nf
        if col != self.n_features_in:
            raise ValueError(f"the sample has {col} input features, but the forest was fitted on {self.n_features_in}")
        return InputSensitivity(rf_feature_importances=out)

    # -- serialisation -----------------------------------------------------------------------
    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        np.savez(os.path.join(path, self._ARRAYS_NAME), mean=self.mean, std=self.std, **self.trees)
        with open(os.path.join(path, self._METADATA_NAME), "w") as f:
            yaml.safe_dump({
                "input_variables": [str(v) for v in self.input_variables],
                "output_variables": [str(v) for v in self.output_variables],
                "output_features": {"names": [str(v) for v in self.output_variables], "features": self.output_features},
                "n_features_in": self.n_features_in,
                "clip": self.clip,
                "predict_columns": self.predict_columns,
            }, f)

    @classmethod
    def load(cls, path: str) -> "RandomForest":
        if os.path.exists(os.path.join(path, cls._ARRAYS_NAME)):
            with open(os.path.join(path, cls._METADATA_NAME)) as f:
                meta = yaml.safe_load(f)
            with np.load(os.path.join(path, cls._ARRAYS_NAME), allow_pickle=False) as z:
                arrays = {k: z[k] for k in z.files}
            return cls(meta["input_variables"], meta["output_variables"], meta["output_features"]["features"], arrays,
                       meta["n_features_in"], arrays["mean"], arrays["std"], clip=meta.get("clip"),
                       predict_columns=meta.get("predict_columns", True))
        if os.path.exists(os.path.join(path, cls._PICKLE_NAME)):
            return cls._load_reference(path)
        raise ValueError(f"{path} holds neither {cls._ARRAYS_NAME} nor the reference's {cls._PICKLE_NAME}")

    @classmethod
    def _load_reference(cls, path: str) -> "RandomForest":
        """SklearnWrapper.load (_random_forest.py:316-377): unpickle the regressor with joblib, read the target scaler
        and the metadata, and export the arrays."""
        try:
            import joblib
            import sklearn  # noqa: F401
        except ImportError as missing:
            raise ValueError(
                f"{path} is a random forest pickled by the reference (sklearn + joblib), which are not importable here; "
                "export it with fv3net_amd.fit.RandomForest.load(path).dump(new_path) where they are") from missing
        with open(os.path.join(path, cls._PICKLE_NAME), "rb") as f:
            components = joblib.load(_bytes_io.BytesIO(f.read()))
        regressor = components["regressors"]
        if isinstance(regressor, list):  # backward compatibility: one batch regressor saved as a list
            if len(regressor) != 1:
                raise ValueError("Cannot load older models that saved multiple batch regressors.")
            regressor = regressor[0]
        scaler_path = os.path.join(path, cls._SCALER_NAME)
        if not os.path.exists(scaler_path):
            raise ValueError("Target scaler not present.")
        with open(scaler_path, "rb") as f:
            mean, std = _read_standard_scaler(f.read())
        with open(os.path.join(path, cls._REF_METADATA_NAME), "rb") as f:
            meta = yaml.safe_load(f.read())
        clip = {name: {k: c.get(k) for k in ("start", "stop", "step")}
                for name, c in ((meta.get("packer_config") or {}).get("clip") or {}).items()}
        of = meta["output_features"]
        if list(of["names"]) != list(meta["output_variables"]):
            raise ValueError(f"output features {of['names']} do not follow the output variables {meta['output_variables']}")
        return cls.from_sklearn(regressor, meta["input_variables"], meta["output_variables"], of["features"], mean, std,
                                clip=clip, predict_columns=meta.get("predict_columns", True))


def _read_standard_scaler(blob: bytes):
    """``scaler.dumps`` (_shared/scaler.py:155-171): YAML of (kind, bytes of an ``np.savez`` of mean and std)."""
    try:
        kind, data = yaml.safe_load(blob)
    except (yaml.YAMLError, TypeError, ValueError):  # a bare np.savez
        kind, data = "standard", blob
    if kind != "standard":
        raise NotImplementedError(f"Cannot load {kind} scaler")
    with np.load(_bytes_io.BytesIO(data), allow_pickle=False) as z:
        if "mean" not in z.files or "std" not in z.files:
            raise ValueError("Target scaler not present.")
        return np.asarray(z["mean"], np.float64), np.asarray(z["std"], np.float64)


# ---------------------------------------------------------------------------------------------
# training (csrc/forest_train.hip)
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class RandomForestHyperparameters:
    """fv3fit's ``RandomForestHyperparameters`` (training_config.py:280-332), same fields and defaults.  ``packer_config`` is
    ``{"clip": {name: {"start", "stop", "step"}}}``.  ``n_jobs`` is accepted and ignored: the trees grow on the device."""

    input_variables: List[str]
    output_variables: List[str]
    scaler_type: str = "standard"
    scaler_kwargs: Optional[Mapping] = None
    n_jobs: int = 8
    random_state: int = 0
    n_estimators: int = 100
    max_depth: Optional[int] = None
    min_samples_split: Union[int, float] = 2
    min_samples_leaf: Union[int, float] = 1
    max_features: Union[str, int, float, None] = "auto"
    max_samples: Optional[Union[int, float]] = None
    bootstrap: bool = True
    packer_config: Mapping = dataclasses.field(default_factory=lambda: {"clip": {}})
    predict_columns: bool = True

    @property
    def clip(self) -> Dict:
        pc = self.packer_config
        clip = pc.get("clip") if isinstance(pc, Mapping) else getattr(pc, "clip", None)
        return {name: dict(c) if isinstance(c, Mapping) else {"start": c.start, "stop": c.stop, "step": c.step}
                for name, c in (clip or {}).items()}


def _pack_batches(batches, names, clip) -> Tuple[np.ndarray, List[int]]:
    """``pack_tfdataset`` over the concatenated batches: every variable ``[sample]`` or ``[sample, feature]`` (ensure_nd(2)),
    float64 cast to float32 (tfdataset.float64_to_float32), clipped along the feature dimension, side by side."""
    cols: List[List[np.ndarray]] = [[] for _ in names]
    for batch in batches:
        batch = to_compat(batch) if not isinstance(batch, Mapping) else batch
        for i, name in enumerate(names):
            a = batch[name]
            a = np.asarray(a.values if hasattr(a, "values") else a)
            if a.ndim == 1:
                a = a[:, None]
            if a.ndim != 2:
                raise ValueError(f"{name!r} has shape {a.shape}: batches must be stacked with at most one non-sample dimension")
            if a.dtype == np.float64:
                a = a.astype(np.float32)
            cols[i].append(a[:, _slice(clip, name)])
    if not cols or not cols[0]:
        raise ValueError("no training batches")
    packed = [np.concatenate(c, axis=0) for c in cols]
    return np.concatenate(packed, axis=1), [int(p.shape[1]) for p in packed]


def train_random_forest(hyperparameters: RandomForestHyperparameters, train_batches, validation_batches=None) -> RandomForest:
    """The reference's ``train_random_forest`` (_random_forest.py:39-62, SklearnWrapper.fit :232-257) with the trees grown on the
    device: all batches in one, float64 cast to float32, the inputs clipped by ``packer_config``, the targets normalised by a
    ``StandardScaler`` fitted on them, then ``n_estimators`` trees seeded and bootstrapped as ``RandomForestRegressor`` seeds and
    bootstraps them.  ``validation_batches`` is ignored, as there."""
    from ..forest_train import check_max_features, forest_arrays, grow_forest

    hp = hyperparameters
    if hp.scaler_type != "standard":
        raise NotImplementedError("only 'standard' scaler_type is implemented")
    clip = hp.clip
    for name in clip:
        if name in hp.output_variables:
            raise NotImplementedError("Clipping for ML outputs is not implemented.")
        if _slice(clip, name).step not in (None, 1):  # (what the predictor could not run is refused before it is trained)
            raise NotImplementedError(f"clip of {name!r} has a step; only contiguous level ranges are supported")
    X, _ = _pack_batches(train_batches, [str(v) for v in hp.input_variables], clip)
    y, output_features = _pack_batches(train_batches, [str(v) for v in hp.output_variables], {})
    check_max_features(hp.max_features, X.shape[1])
    if not np.isfinite(X).all() or not np.isfinite(y).all():
        raise ValueError("the training inputs and targets must be finite")
    # StandardScaler.fit / normalize (_shared/scaler.py:56-68): statistics in the data's dtype, then float64
    mean = np.mean(y, axis=0).astype(np.float64)
    std = np.std(y, axis=0).astype(np.float64) + 1e-12  # (the wrapper builds its scaler without scaler_kwargs)
    y_norm = (y - mean) / std
    trees = grow_forest(X.astype(np.float32), y_norm, n_estimators=hp.n_estimators, random_state=hp.random_state,
                        max_depth=hp.max_depth, min_samples_split=hp.min_samples_split, min_samples_leaf=hp.min_samples_leaf,
                        max_features=hp.max_features, max_samples=hp.max_samples, bootstrap=hp.bootstrap,
                        device=torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu")
    return RandomForest(hp.input_variables, hp.output_variables, output_features, forest_arrays(trees), X.shape[1], mean, std,
                        clip=clip, predict_columns=hp.predict_columns)
