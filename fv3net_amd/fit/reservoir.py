"""Reservoir computing models: fv3fit's ``"pure-reservoir"`` / ``"hybrid-reservoir"`` (reservoir/model.py:36-337) and
their dataset adapters ``"reservoir-adapter"`` / ``"hybrid-reservoir-adapter"`` (reservoir/adapters.py:92-301), stepping
on the MI355X.

The artifact is the reference's own layout, read and written with numpy and YAML only: ``reservoir/`` (W_in and W_res as
``scipy.sparse.save_npz`` files, ``metadata.bin``, optional ``input_mask.npy`` and ``state.npy``), ``readout/``
(``coefficients.npz``, which ``np.save`` writes despite its name, and ``intercepts.npy``), ``metadata.yaml``,
``rank_divider.yaml`` and ``transformers/{input,output,hybrid}_transformer/``.  ``train_reservoir_model`` makes one
(DESIGN.md section 20): the reservoir steps over the training series, the per-subdomain Gram sums of the readout's ridge
regression (``csrc/gram.hip``) and its solve all run on the device; fitting the reference's default normalising transformer
is out of scope, so the transformers are given.

Two behaviours of the reference are kept on purpose: the pure model squares the even *subdomains*
of the state when ``square_half_hidden_state`` is set (``square_even_terms(state, axis=0)``, model.py:225) where the hybrid
model squares even state elements (axis -1, model.py:122); and a ``scale-spatial-concat-z`` transformer rejects inputs
whose (x, y, z) extent differs from its own.  ``get_model_from_subdomain`` gives the sub-model a copy of the parent's
state row instead of sharing the parent's reservoir object.  Where a transformer is a column codec (``DenseAutoencoder`` /
``SkTransformer``) the device handle holds a one-variable do-nothing transformer of the latent size in
its place: ``increment_state`` encodes the inputs into a latent buffer kept with the model and increments from it, ``predict``
reads out into a float64 latent buffer and decodes it, and hybrid inputs are encoded over the extent without overlap.
``w_in_storage`` (``reservoir.WIN_AUTO`` / ``WIN_DENSE`` / ``WIN_CSR``): dense storage, which AUTO picks from half the entries of ``W_in`` stored up, spreads a non-finite input over every
state row of its subdomain where scipy's product reaches only the rows with a stored weight.
"""
import dataclasses
import os
from typing import Hashable, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
import yaml

from ..cubedsphere._device import compute_device
from ..reservoir import (SQUARE_ELEMENTS, SQUARE_NONE, SQUARE_SUBDOMAINS, WIN_AUTO, DenseAutoencoder, DoNothingTransformer,
                         GramAccumulator, RankXYDivider, ReservoirModel, SkTransformer, SparseMatrix, _yaml_load, is_column_codec,
                         load_transformer)
from ..xr_compat import DataArray, Dataset, from_compat, to_compat
from . import io
from .predictor import Predictor


class Reservoir:
    """The reservoir's arrays (reservoir.py:33-200): W_in [state, input_size], W_res [state, state], optional input mask
    and saved state, and the hyperparameters as written (training only needs them)."""

    INPUT_WEIGHTS_NAME = "reservoir_W_in.npz"
    RESERVOIR_WEIGHTS_NAME = "reservoir_W_res.npz"
    METADATA_NAME = "metadata.bin"
    INPUT_MASK_NAME = "input_mask.npy"
    STATE_NAME = "state.npy"

    def __init__(self, hyperparameters: dict, input_size: int, W_in: SparseMatrix, W_res: SparseMatrix,
                 input_mask_array: Optional[np.ndarray] = None, state: Optional[np.ndarray] = None):
        self.hyperparameters = dict(hyperparameters)
        self.input_size = int(input_size)
        self.W_in, self.W_res = W_in, W_res
        self.input_mask_array = input_mask_array
        self.state = state
        if W_in.shape != (self.state_size, self.input_size) or W_res.shape != (self.state_size, self.state_size):
            raise ValueError(f"W_in {W_in.shape} / W_res {W_res.shape} do not match state_size {self.state_size} and "
                             f"input_size {self.input_size}")

    @property
    def state_size(self) -> int:
        return int(self.hyperparameters["state_size"])

    @classmethod
    def generate(cls, hyperparameters: "ReservoirHyperparameters", input_size: int,
                 input_mask_array: Optional[np.ndarray] = None) -> "Reservoir":
        """Random weights as the reference draws them (reservoir.py:23-138), on the host with scipy: ``W_in`` column by
        column, so that every input has the same number of stored entries, uniform in +-``input_coupling_scaling``;
        ``W_res`` uniform in [0, 1) at density ``1 - adjacency_matrix_sparsity``, scaled so that its largest-magnitude
        eigenvalue has modulus ``spectral_radius``.  Seeded by ``hyperparameters.seed`` through a generator of its own (the
        reference seeds numpy's global one): a restatement, not the reference's random stream."""
        import scipy.sparse
        import scipy.sparse.linalg

        hp = hyperparameters
        size, rs = int(hp.state_size), np.random.RandomState(hp.seed)

        def uniform_sparse(m, n, sparsity, lo, hi):
            return scipy.sparse.random(m, n, density=1.0 - sparsity, format="csc", random_state=rs,
                                       data_rvs=lambda d: rs.uniform(lo, hi, size=d))

        scale = hp.input_coupling_scaling
        w_in = scipy.sparse.hstack([uniform_sparse(size, 1, hp.input_coupling_sparsity, -scale, scale)
                                    for _ in range(int(input_size))], format="csc")
        w_res = uniform_sparse(size, size, hp.adjacency_matrix_sparsity, 0.0, 1.0)
        if size > 3:  # ARPACK needs k < n - 1
            largest = scipy.sparse.linalg.eigs(w_res, return_eigenvectors=False, k=1, which="LM",
                                               v0=rs.uniform(size=size)).item()
        else:
            largest = max(np.linalg.eigvals(w_res.toarray()), key=abs)
        if abs(largest) == 0:
            raise ValueError("W_res has no nonzero eigenvalue to scale to the spectral radius; lower "
                             "adjacency_matrix_sparsity or raise state_size")
        w_res = (hp.spectral_radius / abs(largest)) * w_res

        def sparse_matrix(m):
            m = m.tocsc()
            return SparseMatrix("csc", m.shape, {"indices": m.indices, "indptr": m.indptr, "format": np.array(b"csc"),
                                                 "shape": np.asarray(m.shape, np.int64), "data": m.data})

        return cls(dataclasses.asdict(hp), input_size, sparse_matrix(w_in), sparse_matrix(w_res),
                   input_mask_array=input_mask_array)

    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        self.W_in.dump(os.path.join(path, self.INPUT_WEIGHTS_NAME))
        self.W_res.dump(os.path.join(path, self.RESERVOIR_WEIGHTS_NAME))
        if self.input_mask_array is not None:
            np.save(os.path.join(path, self.INPUT_MASK_NAME), self.input_mask_array, allow_pickle=False)
        if self.state is not None:
            np.save(os.path.join(path, self.STATE_NAME), self.state, allow_pickle=False)
        with open(os.path.join(path, self.METADATA_NAME), "w") as f:
            yaml.safe_dump({"reservoir_hyperparameters": self.hyperparameters, "input_size": self.input_size}, f)

    @classmethod
    def load(cls, path: str) -> "Reservoir":
        with open(os.path.join(path, cls.METADATA_NAME)) as f:
            meta = _yaml_load(f.read())

        def optional(name):
            p = os.path.join(path, name)
            return np.load(p, allow_pickle=False) if os.path.exists(p) else None

        return cls(meta["reservoir_hyperparameters"], meta["input_size"],
                   SparseMatrix.load(os.path.join(path, cls.INPUT_WEIGHTS_NAME)),
                   SparseMatrix.load(os.path.join(path, cls.RESERVOIR_WEIGHTS_NAME)),
                   input_mask_array=optional(cls.INPUT_MASK_NAME), state=optional(cls.STATE_NAME))


class ReservoirComputingReadout:
    """coefficients [(subdomain), in, out] and intercepts [(subdomain), out] (readout.py:75-147)."""

    COEFFICIENTS_NAME = "coefficients.npz"
    INTERCEPTS_NAME = "intercepts.npy"

    def __init__(self, coefficients: np.ndarray, intercepts: np.ndarray):
        if coefficients.ndim not in (2, 3):
            raise ValueError(f"Coefficients must be a 2D or 3D array. Got coefficients with shape {coefficients.shape}")
        self.coefficients, self.intercepts = coefficients, intercepts

    def get_subdomain_readout(self, subdomain: int) -> "ReservoirComputingReadout":
        if self.coefficients.ndim == 2 and self.intercepts.ndim == 1:
            raise ValueError("Cannot get subdomain readout from single domain readout")
        return ReservoirComputingReadout(self.coefficients[subdomain], self.intercepts[subdomain])

    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, self.COEFFICIENTS_NAME), "wb") as f:
            np.save(f, self.coefficients, allow_pickle=False)
        np.save(os.path.join(path, self.INTERCEPTS_NAME), self.intercepts, allow_pickle=False)

    @classmethod
    def load(cls, path: str) -> "ReservoirComputingReadout":
        with open(os.path.join(path, cls.COEFFICIENTS_NAME), "rb") as f:
            coefficients = np.load(f, allow_pickle=False)
        return cls(coefficients, np.load(os.path.join(path, cls.INTERCEPTS_NAME), allow_pickle=False))


class TransformerGroup:
    INPUT_DIR, OUTPUT_DIR, HYBRID_DIR = "input_transformer", "output_transformer", "hybrid_transformer"

    def __init__(self, input, output, hybrid):
        self.input, self.output, self.hybrid = input, output, hybrid

    def dump(self, path: str) -> None:
        self.input.dump(os.path.join(path, self.INPUT_DIR))
        self.output.dump(os.path.join(path, self.OUTPUT_DIR))
        self.hybrid.dump(os.path.join(path, self.HYBRID_DIR))

    @classmethod
    def load(cls, path: str) -> "TransformerGroup":
        return cls(*(load_transformer(os.path.join(path, d)) for d in (cls.INPUT_DIR, cls.OUTPUT_DIR, cls.HYBRID_DIR)))


def _to_device(arr, dev) -> torch.Tensor:
    t = arr if isinstance(arr, torch.Tensor) else torch.from_numpy(np.asarray(arr))
    return t.to(dev)


def _as_xyz(arr):
    """(x, y) -> (x, y, 1) view; anything else as it is."""
    if arr.ndim == 2:
        return arr[:, :, None]
    return arr


def _is_device(arrays) -> bool:
    return any(isinstance(a, torch.Tensor) and a.is_cuda for a in arrays)


@io.register("pure-reservoir")
class ReservoirComputingModel(Predictor):
    RESERVOIR_SUBDIR = "reservoir"
    READOUT_SUBDIR = "readout"
    METADATA_NAME = "metadata.yaml"
    RANK_DIVIDER_NAME = "rank_divider.yaml"
    TRANSFORMERS_SUBDIR = "transformers"
    _SQUARE = SQUARE_SUBDOMAINS

    def __init__(self, input_variables: Sequence[Hashable], output_variables: Sequence[Hashable], reservoir: Reservoir,
                 readout: ReservoirComputingReadout, rank_divider: RankXYDivider, transformers: TransformerGroup,
                 square_half_hidden_state: bool = False, w_in_storage: int = WIN_AUTO):
        super().__init__(list(input_variables), list(output_variables))
        self.reservoir, self.readout = reservoir, readout
        self.rank_divider, self.transformers = rank_divider, transformers
        self.square_half_hidden_state = bool(square_half_hidden_state)
        self.w_in_storage = w_in_storage
        self._output_rank_divider = rank_divider.get_no_overlap_rank_divider().get_new_zdim_rank_divider(
            transformers.output.n_latent_dims)
        self._device_model: Optional[ReservoirModel] = None

    # -- device ------------------------------------------------------------------------------
    _n_hybrid = 0
    _hybrid_mask = None

    @staticmethod
    def _device_transformer(tf):
        """What the device handle holds for ``tf``: a column codec runs outside it, on its latent."""
        return DoNothingTransformer([tf.n_latent_dims]) if is_column_codec(tf) else tf

    def _latent(self, name: str, extent, n_latent: int, dtype, device) -> torch.Tensor:
        """The latent buffer ``name`` of the model, allocated once (a captured graph replays into the same address)."""
        buffers = self.__dict__.setdefault("_latent_buffers", {})
        shape = (*extent, n_latent)
        t = buffers.get(name)
        if t is None or tuple(t.shape) != shape or t.dtype != dtype or t.device != device:
            t = buffers[name] = torch.empty(shape, dtype=dtype, device=device)
        return t

    def _encoded(self, name: str, tf, arrays, extent, device):
        """The device inputs of the handle: the arrays, or a codec's latent of them."""
        tensors = [_to_device(a, device) for a in arrays]
        if not is_column_codec(tf):
            return tensors
        return [tf.encode_device(tensors, out=self._latent(name, extent, tf.n_latent_dims, tf.latent_dtype, device))]

    def _readout(self, m: ReservoirModel, hybrid=None) -> List[torch.Tensor]:
        tf = self.transformers.output
        if not is_column_codec(tf):
            return m.predict(hybrid)
        latent = self._latent("output", self.rank_divider.rank_extent, tf.n_latent_dims, torch.float64, m.device)
        m.predict(hybrid, outs=[latent])
        return tf.decode_device(latent)

    def _model(self) -> ReservoirModel:
        if self._device_model is None:
            ns = self.rank_divider.n_subdomains
            c = self.readout.coefficients
            b = self.readout.intercepts
            state = self.reservoir.state
            mask = self.reservoir.input_mask_array
            self._device_model = ReservoirModel(
                self.rank_divider, self._device_transformer(self.transformers.input),
                self._device_transformer(self.transformers.output), self.reservoir.W_in,
                self.reservoir.W_res, c.reshape((ns,) + c.shape[-2:]), b.reshape(ns, b.shape[-1]),
                square=self._SQUARE if self.square_half_hidden_state else SQUARE_NONE,
                input_mask=None if mask is None else np.asarray(mask).reshape(-1, self.reservoir.input_size)[-ns:],
                hybrid_transformer=self._device_transformer(self.transformers.hybrid), n_hybrid=self._n_hybrid,
                hybrid_mask=self._hybrid_mask,
                state=None if state is None else np.asarray(state).reshape(ns, -1), w_in_storage=self.w_in_storage,
                device=compute_device())
        return self._device_model

    def _check_inputs(self, arrays, tf, extent):
        tf.check_inputs([tuple(a.shape) for a in arrays])
        for i, (a, nz) in enumerate(zip(arrays, tf.original_feature_sizes)):
            if tuple(a.shape) != (*extent, nz):
                raise ValueError(f"input array {i} has shape {tuple(a.shape)}, expected {(*extent, nz)}")

    def get_state(self) -> np.ndarray:
        """The reservoir state [subdomain, state_size] (a host copy)."""
        return self._model().get_state().cpu().numpy()

    def set_state(self, state) -> None:
        self._model().set_state(state)

    # -- the reference's surface -------------------------------------------------------------
    def reset_state(self):
        self._model().reset_state()

    def increment_state(self, prediction_with_overlap: Sequence) -> None:
        arrays = [_as_xyz(a) for a in prediction_with_overlap]
        self._check_inputs(arrays, self.transformers.input, self.rank_divider.overlap_rank_extent)
        m = self._model()
        m.increment(self._encoded("input", self.transformers.input, arrays, self.rank_divider.overlap_rank_extent, m.device))

    def synchronize(self, synchronization_time_series: Sequence) -> None:
        """Reset, then one increment per time step of the [time, x, y, z] arrays."""
        series = list(synchronization_time_series)
        n_t = int(series[0].shape[0])
        self.reset_state()
        for t in range(n_t):
            self.increment_state([a[t] for a in series])

    def _outputs(self, outs: List[torch.Tensor], device_out: bool):
        return outs if device_out else [t.cpu().numpy() for t in outs]

    def predict(self, device_output: bool = False):
        """The decoded readout of the current state: one (x, y, z) array per output variable (numpy unless
        ``device_output``)."""
        return self._outputs(self._readout(self._model()), device_output)

    def get_model_from_subdomain(self, subdomain_index: int) -> "ReservoirComputingModel":
        """A model of subdomain ``subdomain_index`` alone, starting from that subdomain's current state."""
        if self.rank_divider.n_subdomains == 1:
            raise ValueError("Model must have multiple subdomains to split.")
        divider = RankXYDivider((1, 1), self.rank_divider.overlap, overlap_rank_extent=self.rank_divider.subdomain_extent,
                                z_feature_size=self.rank_divider.z_feature_size)
        mask = self.reservoir.input_mask_array
        if mask is not None and np.ndim(mask) == 2 and np.shape(mask)[0] == self.rank_divider.n_subdomains:
            mask = np.asarray(mask)[subdomain_index]
        state = self.get_state()[subdomain_index][None] if self._device_model is not None else (
            None if self.reservoir.state is None else np.asarray(self.reservoir.state).reshape(
                self.rank_divider.n_subdomains, -1)[subdomain_index][None])
        reservoir = Reservoir(self.reservoir.hyperparameters, self.reservoir.input_size, self.reservoir.W_in,
                              self.reservoir.W_res, input_mask_array=mask, state=state)
        return self._sub_model(reservoir, self.readout.get_subdomain_readout(subdomain_index), divider, subdomain_index)

    def _sub_model(self, reservoir, readout, divider, subdomain_index):
        return ReservoirComputingModel(self.input_variables, self.output_variables, reservoir, readout, divider,
                                       self.transformers, self.square_half_hidden_state, self.w_in_storage)

    # -- serialisation -----------------------------------------------------------------------
    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        self.reservoir.dump(os.path.join(path, self.RESERVOIR_SUBDIR))
        self.readout.dump(os.path.join(path, self.READOUT_SUBDIR))
        with open(os.path.join(path, self.METADATA_NAME), "w") as f:
            yaml.safe_dump({"square_half_hidden_state": self.square_half_hidden_state,
                            "input_variables": [str(v) for v in self.input_variables],
                            "output_variables": [str(v) for v in self.output_variables]}, f)
        self.rank_divider.dump(os.path.join(path, self.RANK_DIVIDER_NAME))
        self.transformers.dump(os.path.join(path, self.TRANSFORMERS_SUBDIR))

    @classmethod
    def _load_parts(cls, path: str):
        with open(os.path.join(path, cls.METADATA_NAME)) as f:
            meta = _yaml_load(f.read())
        return dict(input_variables=meta["input_variables"], output_variables=meta["output_variables"],
                    reservoir=Reservoir.load(os.path.join(path, cls.RESERVOIR_SUBDIR)),
                    readout=ReservoirComputingReadout.load(os.path.join(path, cls.READOUT_SUBDIR)),
                    rank_divider=RankXYDivider.load(os.path.join(path, cls.RANK_DIVIDER_NAME)),
                    transformers=TransformerGroup.load(os.path.join(path, cls.TRANSFORMERS_SUBDIR)),
                    square_half_hidden_state=meta["square_half_hidden_state"])

    @classmethod
    def load(cls, path: str) -> "ReservoirComputingModel":
        return cls(**cls._load_parts(path))


@io.register("hybrid-reservoir")
class HybridReservoirComputingModel(ReservoirComputingModel):
    HYBRID_VARIABLES_NAME = "hybrid_variables.yaml"
    HYBRID_MASK_NAME = "hybrid_input_mask.npy"
    _SQUARE = SQUARE_ELEMENTS

    def __init__(self, input_variables, hybrid_variables, output_variables, reservoir, readout, rank_divider,
                 transformers, square_half_hidden_state: bool = False, hybrid_input_mask: Optional[np.ndarray] = None,
                 w_in_storage: int = WIN_AUTO):
        super().__init__(input_variables, output_variables, reservoir, readout, rank_divider, transformers,
                         square_half_hidden_state, w_in_storage)
        self.hybrid_variables = list(hybrid_variables)
        self._hybrid_input_mask = hybrid_input_mask
        self._hybrid_mask = hybrid_input_mask
        no_overlap = rank_divider.get_no_overlap_rank_divider()
        self._hybrid_rank_divider = no_overlap.get_new_zdim_rank_divider(transformers.hybrid.n_latent_dims)
        self._n_hybrid = self._hybrid_rank_divider.flat_subdomain_len

    def predict(self, hybrid_input: Sequence, device_output: Optional[bool] = None):
        """The readout of the current state and the hybrid inputs (x, y, z arrays without overlap)."""
        arrays = [_as_xyz(a) for a in hybrid_input]
        self._check_inputs(arrays, self.transformers.hybrid, self.rank_divider.rank_extent)
        m = self._model()
        outs = self._readout(m, self._encoded("hybrid", self.transformers.hybrid, arrays, self.rank_divider.rank_extent,
                                              m.device))
        return self._outputs(outs, _is_device(arrays) if device_output is None else device_output)

    def _sub_model(self, reservoir, readout, divider, subdomain_index):
        mask = self._hybrid_input_mask
        if mask is not None and np.ndim(mask) == 2 and np.shape(mask)[0] == self.rank_divider.n_subdomains:
            mask = np.asarray(mask)[subdomain_index]
        return HybridReservoirComputingModel(self.input_variables, self.hybrid_variables, self.output_variables, reservoir,
                                             readout, divider, self.transformers, self.square_half_hidden_state,
                                             hybrid_input_mask=mask, w_in_storage=self.w_in_storage)

    def dump(self, path: str) -> None:
        super().dump(path)
        with open(os.path.join(path, self.HYBRID_VARIABLES_NAME), "w") as f:
            yaml.safe_dump({"hybrid_variables": [str(v) for v in self.hybrid_variables]}, f)
        if self._hybrid_input_mask is not None:
            np.save(os.path.join(path, self.HYBRID_MASK_NAME), self._hybrid_input_mask, allow_pickle=False)

    @classmethod
    def load(cls, path: str) -> "HybridReservoirComputingModel":
        parts = cls._load_parts(path)
        with open(os.path.join(path, cls.HYBRID_VARIABLES_NAME)) as f:
            hybrid_variables = _yaml_load(f.read())["hybrid_variables"]
        mask_path = os.path.join(path, cls.HYBRID_MASK_NAME)
        mask = np.load(mask_path, allow_pickle=False) if os.path.exists(mask_path) else None
        return cls(parts.pop("input_variables"), hybrid_variables, parts.pop("output_variables"), **parts,
                   hybrid_input_mask=mask)


# ---------------------------------------------------------------------------------------------
# dataset adapters (adapters.py)
# ---------------------------------------------------------------------------------------------

_DIM_ORDER = ("x", "y", "z")


def _input_arrays(ds: Dataset, variables) -> list:
    """Each variable as an (x, y, z) array view (a missing z is a 1-level field); the dataset is not modified."""
    out = []
    for v in variables:
        da = ds[v]
        if any(d not in _DIM_ORDER for d in da.dims) or "x" not in da.dims or "y" not in da.dims:
            raise ValueError(f"variable {v!r} must have dims x, y and optionally z, got {da.dims}")
        order = [da.dims.index(d) for d in _DIM_ORDER if d in da.dims]
        data = da.data.permute(*order) if isinstance(da.data, torch.Tensor) else np.transpose(np.asarray(da.data), order)
        out.append(data if "z" in da.dims else data[:, :, None])
    return out


def _output_dataset(variables, arrays, output_dims) -> Dataset:
    """DatasetAdapter.output_array_to_ds: a trailing z of 1 is squeezed, then dims follow ``output_dims``."""
    ds = Dataset()
    for name, arr in zip(variables, arrays):
        if arr.shape[-1] == 1:
            ds[name] = DataArray(arr[:, :, 0], dims=("x", "y"))
        else:
            ds[name] = DataArray(arr, dims=_DIM_ORDER)
    order = [d for d in (output_dims or _DIM_ORDER) if d in ds.dims]
    return ds.transpose(*order)


@io.register("reservoir-adapter")
class ReservoirDatasetAdapter(Predictor):
    MODEL_DIR = "reservoir_model"

    def __init__(self, model: ReservoirComputingModel, input_variables=None, output_variables=None):
        super().__init__(model.input_variables, model.output_variables)
        self.model = model
        self.nonhybrid_input_variables = model.input_variables

    @property
    def input_overlap(self) -> int:
        return self.model.rank_divider.overlap

    @property
    def is_hybrid(self) -> bool:
        return False

    def predict(self, inputs):
        x = to_compat(inputs) if inputs is not None else None
        dims = list(x.dims) if x is not None and len(x) else None
        device_out = x is not None and _is_device([da.data for da in x.values()])
        result = _output_dataset(self.output_variables, self.model.predict(device_output=device_out), dims)
        return from_compat(result, inputs)

    def increment_state(self, inputs):
        self.model.increment_state(_input_arrays(to_compat(inputs), self.model.input_variables))

    def reset_state(self):
        self.model.reset_state()

    def get_model_from_subdomain(self, subdomain_index: int) -> "ReservoirDatasetAdapter":
        return type(self)(self.model.get_model_from_subdomain(subdomain_index))

    def dump(self, path: str) -> None:
        self.model.dump(os.path.join(path, self.MODEL_DIR))

    @classmethod
    def load(cls, path: str) -> "ReservoirDatasetAdapter":
        return cls(ReservoirComputingModel.load(os.path.join(path, cls.MODEL_DIR)))


@io.register("hybrid-reservoir-adapter")
class HybridReservoirDatasetAdapter(ReservoirDatasetAdapter):
    MODEL_DIR = "hybrid_reservoir_model"

    def __init__(self, model: HybridReservoirComputingModel, input_variables=None, output_variables=None):
        super().__init__(model)
        self.input_variables = list(dict.fromkeys(list(model.input_variables) + list(model.hybrid_variables)))
        self.hybrid_variables = model.hybrid_variables

    @property
    def is_hybrid(self) -> bool:
        return True

    def predict(self, inputs):
        x = to_compat(inputs)
        arrays = _input_arrays(x, self.model.hybrid_variables)
        result = _output_dataset(self.output_variables, self.model.predict(arrays), list(x.dims))
        return from_compat(result, inputs)

    @classmethod
    def load(cls, path: str) -> "HybridReservoirDatasetAdapter":
        return cls(HybridReservoirComputingModel.load(os.path.join(path, cls.MODEL_DIR)))


def split_multi_subdomain_model(model) -> list:
    """One single-subdomain model per subdomain (adapters.py:240-255)."""
    divider = model.model.rank_divider if isinstance(model, ReservoirDatasetAdapter) else model.rank_divider
    return [model.get_model_from_subdomain(i) for i in range(divider.n_subdomains)]


# ---------------------------------------------------------------------------------------------
# the column codecs as artifacts of their own; their predict is the round trip (SkTransformer.predict, and the
# DatasetPredictor that the reference's train_dense_autoencoder returns)
# ---------------------------------------------------------------------------------------------

io.register("hip-dense-autoencoder")(DenseAutoencoder)
io.register("hip-sk-transformer")(SkTransformer)


@dataclasses.dataclass
class DenseAutoencoderHyperparameters:
    """The fields of fv3fit's ``DenseAutoencoderHyperparameters`` (autoencoder.py:95-127) that shape the graph and its
    training; ``output_limits`` maps a variable to its (min, max), either of them None."""

    state_variables: Sequence[str]
    latent_dim_size: int = 10
    units: int = 20
    n_dense_layers: int = 2
    epochs: int = 10
    batch_size: int = 512
    learning_rate: float = 1e-3
    normalization_fit_samples: int = 500_000
    output_limits: dict = dataclasses.field(default_factory=dict)
    seed: int = 0


def train_dense_autoencoder(hyperparameters: DenseAutoencoderHyperparameters, arrays: Sequence[np.ndarray],
                            device: Optional[str] = None) -> DenseAutoencoder:
    """The counterpart of the reference's ``"dense_autoencoder"`` training function (autoencoder.py:179-275), offline in plain
    torch: ``arrays`` holds one [sample, z] array per state variable.  The normalisation constants are the per-feature mean
    and standard deviation of up to ``normalization_fit_samples`` samples, in float32; the graph is ``n_dense_layers``
    ReLU layers of ``units`` and a ReLU latent layer of ``latent_dim_size``, the same number of ReLU layers back and one
    linear head per variable (glorot-uniform kernels, zero biases, as Keras initialises a Dense layer); the loss is the MSE
    of the standardised outputs summed over the variables, minimised by Adam from ``seed``.  The output limits are applied
    at prediction only.  The callbacks and validation batches of the reference are out of scope."""
    hp = hyperparameters
    arrays = [np.asarray(a, np.float32) for a in arrays]
    if len(arrays) != len(hp.state_variables) or any(a.ndim != 2 or a.shape[0] != arrays[0].shape[0] for a in arrays):
        raise ValueError("arrays must hold one [sample, z] array per state variable, with a common sample count")
    torch.manual_seed(hp.seed)
    dev = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
    sizes = [a.shape[1] for a in arrays]
    x = np.concatenate(arrays, axis=1)
    nfit = hp.normalization_fit_samples
    center = x[:nfit].mean(axis=0, dtype=np.float32)
    scale = x[:nfit].std(axis=0, dtype=np.float32)
    xn = torch.from_numpy((x - center) / (scale + np.float32(1e-7))).to(dev)

    def dense(fan_in, fan_out):
        lin = torch.nn.Linear(fan_in, fan_out)
        torch.nn.init.xavier_uniform_(lin.weight)
        torch.nn.init.zeros_(lin.bias)
        return lin

    widths = [hp.units] * hp.n_dense_layers
    enc, fan = [], x.shape[1]
    for w in widths + [hp.latent_dim_size]:
        enc.append(dense(fan, w))
        fan = w
    dec = []
    for w in widths:
        dec.append(dense(fan, w))
        fan = w
    heads = [dense(fan, nz) for nz in sizes]
    modules = torch.nn.ModuleList(enc + dec + heads).to(dev)

    def forward(batch):
        h = batch
        for lin in enc + dec:
            h = torch.relu(lin(h))
        return torch.cat([head(h) for head in heads], dim=1)

    opt = torch.optim.Adam(modules.parameters(), lr=hp.learning_rate)
    n = xn.shape[0]
    gen = torch.Generator().manual_seed(hp.seed)
    for _ in range(hp.epochs):
        order = torch.randperm(n, generator=gen).to(dev)
        for start in range(0, n, hp.batch_size):
            batch = xn[order[start:start + hp.batch_size]]
            # the heads give standardised values, so the std-scaled MSE of each variable is its plain MSE here
            err = (forward(batch) - batch) ** 2
            loss = sum(part.mean() for part in torch.split(err, sizes, dim=1))
            opt.zero_grad()
            loss.backward()
            opt.step()

    kernel = lambda lin: lin.weight.detach().cpu().numpy().T.copy()  # noqa: E731  ([in, out] as Keras stores it)
    bias = lambda lin: lin.bias.detach().cpu().numpy().copy()  # noqa: E731
    limits = [hp.output_limits.get(v, (None, None)) for v in hp.state_variables]
    return DenseAutoencoder(center, scale, sizes, [kernel(m) for m in enc], [bias(m) for m in enc],
                            [kernel(m) for m in dec], [bias(m) for m in dec], [kernel(m) for m in heads],
                            [bias(m) for m in heads], output_min=[lo for lo, _ in limits],
                            output_max=[hi for _, hi in limits])


# ---------------------------------------------------------------------------------------------
# training (reservoir/config.py, readout.py:14-70, utils.py:40-75, train.py:165-396)
# ---------------------------------------------------------------------------------------------


@dataclasses.dataclass
class CubedsphereSubdomainConfig:
    layout: Tuple[int, int]
    overlap: int
    rank_dims: Sequence[str]


@dataclasses.dataclass
class ReservoirHyperparameters:
    """``state_size``: W_res is [state_size, state_size]; ``adjacency_matrix_sparsity``: fraction of W_res that is zero;
    ``spectral_radius``: modulus of W_res' largest eigenvalue; ``input_coupling_sparsity``: fraction of each input's
    column of W_in that is zero; ``input_coupling_scaling``: W_in is uniform in +- this."""

    state_size: int
    adjacency_matrix_sparsity: float
    spectral_radius: float
    seed: int = 0
    input_coupling_sparsity: float = 0.0
    input_coupling_scaling: float = 1.0


@dataclasses.dataclass
class BatchLinearRegressorHyperparameters:
    """``l2``: ridge coefficient; ``add_bias_term``: append a constant feature for the intercept;
    ``use_least_squares_solve``: ``np.linalg.lstsq`` on the host, for small underdetermined cases."""

    l2: float
    add_bias_term: bool = True
    use_least_squares_solve: bool = False


@dataclasses.dataclass
class TransformerConfig:
    input: Optional[str] = None
    output: Optional[str] = None
    hybrid: Optional[str] = None


def _from_dict(cls, data, casts=True):
    """A dataclass from a mapping, strictly (unknown or missing keys are errors), scalars cast to the annotated type."""
    if isinstance(data, cls):
        return data
    fields = {f.name: f for f in dataclasses.fields(cls)}
    unknown = set(data) - set(fields)
    if unknown:
        raise ValueError(f"{cls.__name__} has no field(s) {sorted(unknown)}")
    missing = [n for n, f in fields.items() if n not in data and f.default is dataclasses.MISSING
               and f.default_factory is dataclasses.MISSING]
    if missing:
        raise ValueError(f"{cls.__name__} is missing field(s) {missing}")
    kwargs = {}
    for name, value in data.items():
        kind = fields[name].type
        if casts and value is not None and kind in (int, float, bool, str):
            value = kind(value)
        elif casts and value is not None and kind == Tuple[int, int]:
            value = tuple(int(v) for v in value)
        kwargs[name] = value
    return cls(**kwargs)


@dataclasses.dataclass
class ReservoirTrainingConfig:
    """The reference's training configuration, field for field.  ``n_jobs`` and ``validate_sst_only`` are kept for parity
    and unused: the subdomains update in one launch, and validation is the caller's.  ``transformers`` names artifacts by
    path in the reference; ``train_reservoir_model`` takes the loaded ``TransformerGroup`` as an argument instead."""

    input_variables: Sequence[str]
    output_variables: Sequence[str]
    subdomain: CubedsphereSubdomainConfig
    reservoir_hyperparameters: ReservoirHyperparameters
    readout_hyperparameters: BatchLinearRegressorHyperparameters
    n_timesteps_synchronize: int
    input_noise: float
    seed: int = 0
    transformers: Optional[TransformerConfig] = None
    n_jobs: Optional[int] = 1
    square_half_hidden_state: bool = False
    hybrid_variables: Optional[Sequence[str]] = None
    mask_reservoir_inputs: bool = False
    mask_hybrid_inputs: bool = False
    mask_variable: Optional[str] = None
    validate_sst_only: bool = False

    def __post_init__(self):
        if self.hybrid_variables is not None:
            if set(self.hybrid_variables).intersection(self.input_variables):
                raise ValueError(f"Hybrid variables {self.hybrid_variables} cannot overlap with input variables "
                                 f"{self.input_variables}.")
        if (self.mask_reservoir_inputs or self.mask_hybrid_inputs) and self.mask_variable is None:
            raise ValueError("mask_variable must be specified if masking is enabled")

    @property
    def variables(self) -> set:
        extra = list(self.hybrid_variables or []) + ([] if self.mask_variable is None else [self.mask_variable])
        return set(list(self.input_variables) + list(self.output_variables) + extra)

    @classmethod
    def from_dict(cls, kwargs) -> "ReservoirTrainingConfig":
        kwargs = {**kwargs}
        for name, kind in (("reservoir_hyperparameters", ReservoirHyperparameters),
                           ("readout_hyperparameters", BatchLinearRegressorHyperparameters),
                           ("subdomain", CubedsphereSubdomainConfig), ("transformers", TransformerConfig)):
            kwargs[name] = _from_dict(kind, kwargs.get(name) or {})
        return _from_dict(cls, kwargs, casts=False)


class NotFittedError(Exception):
    pass


class BatchLinearRegressor:
    """Solves ``(A + l2 I) W = B`` with ``A = X.T X`` and ``B = X.T y`` summed over batches (readout.py:19-70), for every
    subdomain at once and on the device: the sums are ``GramAccumulator``'s, the solve ``torch.linalg.solve`` in float64,
    one subdomain at a time so that the workspace stays one matrix.

    ``batch_update(X, y)`` takes [time, subdomain, feature] arrays (numpy or device tensors; strided device views are
    used as they are), or the reference's [time, feature], which is one subdomain.  ``get_weights()`` returns
    ``(coefficients, intercepts)`` as numpy, [subdomain, feature, out] and [subdomain, out] (without the subdomain
    dimension after [time, feature] updates)."""

    def __init__(self, hyperparameters: BatchLinearRegressorHyperparameters, device=None):
        self.hyperparameters = hyperparameters
        self._device = device
        self._acc: Optional[GramAccumulator] = None
        self._squeeze = False

    def _as_device(self, a) -> torch.Tensor:
        dev = torch.device(self._device) if self._device is not None else compute_device()
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, np.float64))
        return t.to(dev, torch.float64)

    def batch_update(self, X, y) -> None:
        X, y = self._as_device(X), self._as_device(y)
        if X.dim() == 2:
            X, y, self._squeeze = X[:, None, :], y[:, None, :], True
        if X.dim() != 3 or y.dim() != 3 or X.shape[:2] != y.shape[:2]:
            raise ValueError(f"X and y must be [time, subdomain, feature] arrays with common leading dimensions, got "
                             f"{tuple(X.shape)} and {tuple(y.shape)}")
        if not self.hyperparameters.add_bias_term:
            last = X[:, :, -1]
            if not torch.allclose(last, torch.ones_like(last)):
                raise ValueError("Last column of X array must all be ones if add_bias_term is False.")
        if self._acc is None:
            self._acc = GramAccumulator(X.shape[1], X.shape[2], y.shape[2], add_bias=self.hyperparameters.add_bias_term,
                                        device=X.device)
        self._acc.update(X, y)

    def sums(self, subdomain: Optional[int] = None):
        """(A, B) as device tensors: of one subdomain, or of all with a leading subdomain dimension."""
        if self._acc is None:
            raise NotFittedError("At least one call of batch_update on data must be done before solving for weights.")
        return self._acc.get(subdomain)

    def get_weights(self):
        if self._acc is None:
            raise NotFittedError("At least one call of batch_update on data must be done before solving for weights.")
        acc, hp = self._acc, self.hyperparameters
        weights = np.empty((acc.n_subdomains, acc.n_rows, acc.n_outputs))
        for s in range(acc.n_subdomains):
            a, b = acc.get(s)
            a.diagonal().add_(hp.l2)
            if hp.use_least_squares_solve:
                weights[s] = np.linalg.lstsq(a.cpu().numpy(), b.cpu().numpy(), rcond=None)[0]
            else:
                weights[s] = torch.linalg.solve(a, b).cpu().numpy()
        coefficients, intercepts = weights[:, :-1, :], weights[:, -1, :]
        return (coefficients[0], intercepts[0]) if self._squeeze else (coefficients, intercepts)


class SynchronizationTracker:
    """The reference's ``SynchronziationTracker`` (utils.py:40-75), counting as it counts: synchronization is complete only
    once *more than* ``n_synchronize`` steps have been counted, and the trim keeps the last ``steps_past_sync`` samples of
    the array it is given, however many of them the current batch contributed."""

    def __init__(self, n_synchronize: int):
        self.n_synchronize = n_synchronize
        self.n_steps_synchronized = 0

    @property
    def completed_synchronization(self) -> bool:
        return self.n_steps_synchronized > self.n_synchronize

    def count_synchronization_steps(self, n_samples: int) -> None:
        self.n_steps_synchronized += n_samples

    def trim_synchronization_samples_if_needed(self, arr):
        if not self.completed_synchronization:
            return arr[:0]
        steps_past_sync = self.n_steps_synchronized - self.n_synchronize
        return arr if steps_past_sync > len(arr) else arr[-steps_past_sync:]


def _txyz(arr):
    """assure_txyz_dims (utils.py:18-37): [t, x, y] gains a feature dimension, [x, y] a time dimension too."""
    if arr.ndim == 4:
        return arr
    if arr.ndim == 3:
        return arr[..., None]
    if arr.ndim == 2:
        return arr[None, :, :, None]
    raise ValueError(f"Tensor data has {arr.ndim} dims, must either have either 4 dims (t, x, y, z) or 3 dims (t, x, y) "
                     "or 2 dims (x, y).")


def _host(arr) -> np.ndarray:
    return arr.cpu().numpy() if isinstance(arr, torch.Tensor) else np.asarray(arr)


def _mask_array(mask_variable: str, batch: Mapping, divider: RankXYDivider, trim_halo: bool = False) -> np.ndarray:
    """_get_input_mask_array (train.py:92-118): the mask variable's first time step over every latent feature, per subdomain
    and flat; its values must be 0 and 1."""
    if mask_variable not in batch:
        raise KeyError(f"'{mask_variable}' must be included in training data if the mask_variable is specified in training "
                       "configuration.")
    mask = _txyz(_host(batch[mask_variable]))
    mask = mask * np.ones((*divider.overlap_rank_extent, divider.z_feature_size))
    if trim_halo:
        mask = divider.trim_halo_from_rank_data(mask)
        divider = divider.get_no_overlap_rank_divider()
    mask = divider.get_all_subdomains_with_flat_feature(mask[0])
    if set(np.unique(mask)) != {0, 1}:
        raise ValueError(f"Mask variable values in field {mask_variable} are not all in {{0, 1}}.")
    return mask


def _series_inputs(tf, arrays, extent, device) -> List[torch.Tensor]:
    """[t, x, y, z] arrays as the device handle's series inputs; a column codec encodes each time step into a latent
    series first (the existing per-step path)."""
    tensors = [_to_device(a, device) for a in arrays]
    tf.check_inputs([tuple(t.shape) for t in tensors])
    if not is_column_codec(tf):
        return tensors
    latent = torch.empty((tensors[0].shape[0], *extent, tf.n_latent_dims), dtype=tf.latent_dtype, device=device)
    for t in range(latent.shape[0]):
        tf.encode_device([a[t] for a in tensors], out=latent[t])
    return [latent]


def train_reservoir_model(hyperparameters: ReservoirTrainingConfig, train_batches, transformers: TransformerGroup):
    """The reference's ``"reservoir"`` training function (train.py:165-362) on the device.

    ``train_batches``: a sequence of batches, each a mapping from variable name to a [t, x, y(, z)] array (numpy or device
    tensor) over the rank extent with its overlap, or a sequence of such sequences; the reservoir state is reset at the
    first batch of each sequence and synchronized over its first ``n_timesteps_synchronize`` steps, which do not enter the
    regression.  ``transformers``: the ``TransformerGroup`` to encode with (any transformers the model classes accept);
    fitting the reference's default normalising transformer when none is configured is out of scope.

    Per batch the handle steps the reservoir over the series (``input_noise`` > 0 adds
    ``RandomState(hyperparameters.seed).normal`` draws of shape [t, subdomain, input], made on the host, to the encoded
    inputs), the targets are encoded without their halo, ``X = states[:-1] (|| hybrid[:-1])`` and ``Y = targets[1:]`` are
    trimmed by the tracker and summed into the Gram accumulators; one ridge solve per subdomain gives the readout.  Returns
    a ``ReservoirDatasetAdapter`` or ``HybridReservoirDatasetAdapter`` whose ``dump`` is the reference's layout.

    One deliberate narrowing: the hybrid input mask is taken from the first batch, and a later batch whose mask differs is
    an error (the reference recomputes it per batch and keeps the last one)."""
    hp = hyperparameters
    if transformers is None or any(getattr(transformers, side, None) is None for side in ("input", "output", "hybrid")):
        raise ValueError("train_reservoir_model needs the input, output and hybrid transformers: fitting the reference's "
                         "default normalising transformer when none is configured is out of scope")
    sequences = list(train_batches)
    if not sequences:
        raise ValueError("train_batches is empty")
    if isinstance(sequences[0], Mapping):
        sequences = [sequences]
    sequences = [list(seq) for seq in sequences]
    sample = sequences[0][0]
    hybrid = hp.hybrid_variables is not None
    overlap_extent = tuple(_txyz(sample[hp.input_variables[0]]).shape[1:-1])
    divider = RankXYDivider(tuple(hp.subdomain.layout), hp.subdomain.overlap, overlap_rank_extent=overlap_extent,
                            z_feature_size=transformers.input.n_latent_dims)
    input_mask = _mask_array(hp.mask_variable, sample, divider) if hp.mask_reservoir_inputs else None
    reservoir = Reservoir.generate(hp.reservoir_hyperparameters, divider.flat_subdomain_len, input_mask)

    no_overlap = divider.get_no_overlap_rank_divider()
    n_out = no_overlap.get_new_zdim_rank_divider(transformers.output.n_latent_dims).flat_subdomain_len
    hybrid_divider = divider.get_new_zdim_rank_divider(transformers.hybrid.n_latent_dims) if hybrid else None
    hybrid_mask = _mask_array(hp.mask_variable, sample, hybrid_divider, trim_halo=True) \
        if hybrid and hp.mask_hybrid_inputs else None
    n_hybrid = hybrid_divider.get_no_overlap_rank_divider().flat_subdomain_len if hybrid else 0
    size, ns = reservoir.state_size, divider.n_subdomains
    # the model with an empty readout: its device handle steps the reservoir and encodes; the readout follows
    readout = ReservoirComputingReadout(np.zeros((ns, size + n_hybrid, n_out)), np.zeros((ns, n_out)))
    if hybrid:
        model = HybridReservoirComputingModel(hp.input_variables, hp.hybrid_variables, hp.output_variables, reservoir, readout,
                                              divider, transformers, hp.square_half_hidden_state,
                                              hybrid_input_mask=hybrid_mask)
    else:
        model = ReservoirComputingModel(hp.input_variables, hp.output_variables, reservoir, readout, divider, transformers,
                                        hp.square_half_hidden_state)
    handle = model._model()
    dev = handle.device
    regressor = BatchLinearRegressor(hp.readout_hyperparameters, device=dev)
    noise_rs = np.random.RandomState(hp.seed)
    o = divider.overlap
    trim = (lambda a: a[:, o:a.shape[1] - o, o:a.shape[2] - o]) if o else (lambda a: a)

    for batches in sequences:
        tracker = SynchronizationTracker(hp.n_timesteps_synchronize)
        for b, batch in enumerate(batches):
            inputs = _series_inputs(transformers.input, [_txyz(batch[v]) for v in hp.input_variables],
                                    divider.overlap_rank_extent, dev)
            n_t = int(inputs[0].shape[0])
            if b == 0:
                handle.reset_state()
            targets = _series_inputs(transformers.output,
                                     [trim(_txyz(batch[v])) for v in hp.output_variables], divider.rank_extent, dev)
            hybrid_inputs = None
            if hybrid:
                hybrid_inputs = _series_inputs(transformers.hybrid,
                                               [trim(_txyz(batch[v])) for v in hp.hybrid_variables], divider.rank_extent, dev)
                if hp.mask_hybrid_inputs and not np.array_equal(
                        _mask_array(hp.mask_variable, batch, hybrid_divider, trim_halo=True), hybrid_mask):
                    raise ValueError(f"the hybrid input mask of field {hp.mask_variable} differs between batches; one mask "
                                     "per training run is supported")
            noise = None
            if hp.input_noise > 0:
                noise = torch.from_numpy(noise_rs.normal(0.0, hp.input_noise, (n_t, ns, reservoir.input_size))).to(dev)
            states = handle.train_series(inputs, hybrid_inputs, noise=noise,
                                         square_even_elements=hp.square_half_hidden_state)
            encoded_targets = handle.encode_targets(targets)
            tracker.count_synchronization_steps(n_t)
            if tracker.completed_synchronization:
                regressor.batch_update(tracker.trim_synchronization_samples_if_needed(states[:-1]),
                                       tracker.trim_synchronization_samples_if_needed(encoded_targets[1:]))

    coefficients, intercepts = regressor.get_weights()
    model.readout = ReservoirComputingReadout(coefficients, intercepts)
    # the state after the last training step goes with the model, as the reference's reservoir keeps it; the next call
    # uploads it with the trained readout
    model.reservoir.state = handle.get_state().cpu().numpy()
    model._device_model = None
    return HybridReservoirDatasetAdapter(model) if hybrid else ReservoirDatasetAdapter(model)
