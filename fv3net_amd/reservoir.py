"""Reservoir computing: the rank divider, the transformers, the sparse weight files and the device handle.

``RankXYDivider`` is the subdomain index arithmetic of fv3fit's ``reservoir/domain2.py`` (numpy only; pace's
``TilePartitioner`` is replaced by its closed form: subdomain ``s`` covers x block ``s % layout_x`` and y block
``s // layout_x``).  ``DoNothingTransformer`` and ``ScaleSpatialConcatZTransformer`` read and write the reference's
transformer directories.  ``SparseMatrix`` reads and writes ``scipy.sparse.save_npz`` files with numpy alone.
``ReservoirModel`` uploads a model once (``fv3hip_reservoir_create``) and runs its steps on the GPU: the increment and the
readout are HIP kernels (``csrc/reservoir.hip``); there is no host path.
"""
import ctypes
import os
from typing import List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
import yaml

from . import _lib
from .ops import _require_device, _stream

# ---------------------------------------------------------------------------------------------
# rank divider (domain2.py:22-390)
# ---------------------------------------------------------------------------------------------


def _check_feature_dims_consistent(data_shape, feature_shape):
    n = len(feature_shape)
    got = tuple(data_shape[-n:]) if n else ()
    if n == 0 or got != tuple(feature_shape):
        raise ValueError(f"Feature dimensions of data {got} are not consistent with expected: {tuple(feature_shape)}")


class RankXYDivider:
    """Subdomains of one rank's (x, y[, z]) arrays; trailing dims are x, y and optionally a feature dim z."""

    def __init__(self, subdomain_layout: Tuple[int, int], overlap: int, rank_extent: Optional[Tuple[int, int]] = None,
                 overlap_rank_extent: Optional[Tuple[int, int]] = None, z_feature_size: Optional[int] = None):
        if len(subdomain_layout) != 2:
            raise ValueError("Rank divider only handles 2D subdomain layouts")
        if overlap < 0:
            raise ValueError("Overlap must be non-negative")
        self.overlap = int(overlap)
        self.subdomain_layout = tuple(int(v) for v in subdomain_layout)
        self.n_subdomains = self.subdomain_layout[0] * self.subdomain_layout[1]
        if (rank_extent is None) == (overlap_rank_extent is None):
            raise ValueError("Specify exactly one of rank_extent and overlap_rank_extent")
        ext = rank_extent if rank_extent is not None else overlap_rank_extent
        if len(ext) != 2:
            raise ValueError("Rank divider only handles 2D rank extents")
        if rank_extent is not None:
            self.rank_extent = tuple(int(v) for v in rank_extent)
        else:
            self.rank_extent = tuple(int(v) - 2 * self.overlap for v in overlap_rank_extent)
        self.overlap_rank_extent = tuple(v + 2 * self.overlap for v in self.rank_extent)
        self._z_feature_size = None if z_feature_size is None else int(z_feature_size)
        for d in range(2):
            if self.rank_extent[d] % self.subdomain_layout[d] != 0:
                raise ValueError(f"{'XY'[d]} rank extent {self.rank_extent[d]} is not divisible by subdomain layout "
                                 f"{self.subdomain_layout[d]}")
        self._block = tuple(self.rank_extent[d] // self.subdomain_layout[d] for d in range(2))

    def __eq__(self, other):
        return (isinstance(other, RankXYDivider) and self.subdomain_layout == other.subdomain_layout
                and self.rank_extent == other.rank_extent and self._z_feature_size == other._z_feature_size)

    @property
    def z_feature_size(self) -> Optional[int]:
        return self._z_feature_size

    @property
    def subdomain_extent(self) -> Tuple[int, int]:
        return self._block[0] + 2 * self.overlap, self._block[1] + 2 * self.overlap

    def _with_z(self, values, z):
        return [*values] + ([] if self._z_feature_size is None else [z])

    @property
    def _subdomain_shape(self):
        return self._with_z(self.subdomain_extent, self._z_feature_size)

    @property
    def flat_subdomain_len(self) -> int:
        return int(np.prod(self._subdomain_shape))

    @property
    def subdomain_axis(self) -> int:
        return -(len(self._subdomain_shape) + 1)

    def get_new_zdim_rank_divider(self, z_feature_size: int) -> "RankXYDivider":
        return RankXYDivider(self.subdomain_layout, self.overlap, rank_extent=self.rank_extent, z_feature_size=z_feature_size)

    def get_no_overlap_rank_divider(self) -> "RankXYDivider":
        if self.overlap == 0:
            return self
        return RankXYDivider(self.subdomain_layout, 0, rank_extent=self.rank_extent, z_feature_size=self._z_feature_size)

    def subdomain_origin(self, i: int) -> Tuple[int, int]:
        """(x, y) of subdomain ``i``'s first point in the overlapped rank array (pace's subtile order: x fastest)."""
        return (i % self.subdomain_layout[0]) * self._block[0], (i // self.subdomain_layout[0]) * self._block[1]

    def _slices(self, i):
        x0, y0 = self.subdomain_origin(i)
        sx, sy = self.subdomain_extent
        return self._with_z([slice(x0, x0 + sx), slice(y0, y0 + sy)], slice(None))

    def get_subdomain(self, data: np.ndarray, subdomain_index: int) -> np.ndarray:
        if subdomain_index < 0 or subdomain_index >= self.n_subdomains:
            raise ValueError(f"Subdomain index {subdomain_index} out of range [0, {self.n_subdomains})")
        _check_feature_dims_consistent(data.shape, self._with_z(self.overlap_rank_extent, self._z_feature_size))
        return data[(Ellipsis, *self._slices(subdomain_index))]

    def get_all_subdomains(self, data: np.ndarray) -> np.ndarray:
        return np.stack([self.get_subdomain(data, i) for i in range(self.n_subdomains)], axis=self.subdomain_axis)

    def flatten_subdomain_features(self, data: np.ndarray) -> np.ndarray:
        _check_feature_dims_consistent(data.shape, self._subdomain_shape)
        return data.reshape(list(data.shape[:-len(self._subdomain_shape)]) + [-1])

    def reshape_flat_subdomain_features(self, data: np.ndarray) -> np.ndarray:
        _check_feature_dims_consistent(data.shape, [self.flat_subdomain_len])
        return data.reshape(list(data.shape[:-1]) + self._subdomain_shape)

    def merge_all_subdomains(self, data: np.ndarray) -> np.ndarray:
        if self.overlap > 0:
            raise ValueError("Cannot merge subdomains with overlap")
        _check_feature_dims_consistent(data.shape, [self.n_subdomains] + self._subdomain_shape)
        ax = self.subdomain_axis
        merged = np.empty(list(data.shape[:ax]) + self._with_z(self.rank_extent, self._z_feature_size), dtype=data.dtype)
        for i in range(self.n_subdomains):
            merged[(Ellipsis, *self._slices(i))] = np.take(data, i, axis=ax)
        return merged

    def get_all_subdomains_with_flat_feature(self, data: np.ndarray) -> np.ndarray:
        return self.flatten_subdomain_features(self.get_all_subdomains(data))

    def merge_all_flat_feature_subdomains(self, data: np.ndarray) -> np.ndarray:
        return self.merge_all_subdomains(self.reshape_flat_subdomain_features(data))

    def trim_halo_from_rank_data(self, data: np.ndarray) -> np.ndarray:
        _check_feature_dims_consistent(data.shape, self._with_z(self.overlap_rank_extent, self._z_feature_size))
        if self.overlap == 0:
            return data
        sl = slice(self.overlap, -self.overlap)
        return data[(Ellipsis, *self._with_z([sl, sl], slice(None)))]

    def dump(self, path: str) -> None:
        with open(path, "w") as f:
            yaml.safe_dump({"subdomain_layout": list(self.subdomain_layout), "overlap": self.overlap,
                            "rank_extent": list(self.rank_extent), "z_feature_size": self._z_feature_size}, f)

    @classmethod
    def load(cls, path: str) -> "RankXYDivider":
        with open(path) as f:
            meta = _yaml_load(f.read())
        return cls(tuple(meta["subdomain_layout"]), meta["overlap"], rank_extent=tuple(meta["rank_extent"]),
                   z_feature_size=meta.get("z_feature_size"))


class _TupleLoader(yaml.SafeLoader):
    """SafeLoader that also reads the ``!!python/tuple`` tag ``yaml.dump`` writes for tuples (as a list)."""


_TupleLoader.add_constructor("tag:yaml.org,2002:python/tuple", lambda loader, node: loader.construct_sequence(node))


def _yaml_load(text):
    return yaml.load(text, Loader=_TupleLoader)


# ---------------------------------------------------------------------------------------------
# transformers (reservoir/transformers/transformer.py)
# ---------------------------------------------------------------------------------------------


class DoNothingTransformer:
    """``"do-nothing-transformer"``: the variables concatenated along z, float64 (``mock_transformer.yaml``)."""

    CONFIG_NAME = "mock_transformer.yaml"
    kind = 0

    def __init__(self, original_feature_sizes: Sequence[int]):
        self.original_feature_sizes = [int(v) for v in original_feature_sizes]

    @property
    def n_latent_dims(self) -> int:
        return sum(self.original_feature_sizes)

    @property
    def n_variables(self) -> int:
        return len(self.original_feature_sizes)

    def check_inputs(self, shapes: Sequence[Tuple[int, ...]]):
        if len(shapes) != self.n_variables:
            raise ValueError(f"Expected {self.n_variables} input arrays but got {len(shapes)}")

    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, self.CONFIG_NAME), "w") as f:
            yaml.safe_dump({"original_feature_sizes": self.original_feature_sizes}, f)

    @classmethod
    def load(cls, path: str) -> "DoNothingTransformer":
        with open(os.path.join(path, cls.CONFIG_NAME)) as f:
            return cls(_yaml_load(f.read())["original_feature_sizes"])


class ScaleSpatialConcatZTransformer:
    """``"scale-spatial-concat-z-transformer"``: per-(x, y, z) ``(x - center) / (scale + 1e-7)`` in float32 (NormLayer casts
    center and scale to float32), the variables concatenated along z, times the optional ``mask`` [x, y, z * n_var]."""

    CONFIG_NAME = "scale_spatial_concat_z_transformer.yaml"
    kind = 1

    def __init__(self, center: np.ndarray, scale: np.ndarray, spatial_features: Sequence[int], num_variables: int,
                 mask: Optional[np.ndarray] = None):
        self.center = np.asarray(center)
        self.scale = np.asarray(scale)
        self.spatial_features = tuple(int(v) for v in spatial_features)
        self.num_variables = int(num_variables)
        self.mask = None if mask is None else np.asarray(mask)
        if len(self.spatial_features) != 3:
            raise ValueError(f"spatial_features must be (x, y, z), got {self.spatial_features}")
        n = self.num_variables * int(np.prod(self.spatial_features))
        if self.center.size != n or self.scale.size != n:
            raise ValueError(f"center and scale need {n} values (num_variables * x * y * z), got {self.center.size} "
                             f"and {self.scale.size}")
        x, y, z = self.spatial_features
        if self.mask is not None and self.mask.size != x * y * z * self.num_variables:
            raise ValueError(f"mask needs shape {(x, y, z * self.num_variables)}, got {self.mask.shape}")

    @property
    def n_latent_dims(self) -> int:
        return self.num_variables * self.spatial_features[-1]

    @property
    def n_variables(self) -> int:
        return self.num_variables

    @property
    def original_feature_sizes(self) -> List[int]:
        return [self.spatial_features[-1]] * self.num_variables

    def check_inputs(self, shapes: Sequence[Tuple[int, ...]]):
        """_check_consistent_xyz (transformer.py:128-141), with its messages."""
        if len(shapes) != self.num_variables:
            raise ValueError(f"Expected {self.num_variables} input arrays but got {len(shapes)}")
        for i, shape in enumerate(shapes):
            if tuple(shape[-3:]) != self.spatial_features:
                raise ValueError("All arrays must have the same x,y,z features. "
                                 f"Expected {self.spatial_features} but got {tuple(shape[-3:])} for array {i}.")

    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, self.CONFIG_NAME), "w") as f:
            yaml.safe_dump({"num_variables": self.num_variables, "spatial_features": list(self.spatial_features)}, f)
        np.save(os.path.join(path, "scale.npy"), self.scale)
        np.save(os.path.join(path, "center.npy"), self.center)
        if self.mask is not None:
            np.save(os.path.join(path, "mask.npy"), self.mask)

    @classmethod
    def load(cls, path: str) -> "ScaleSpatialConcatZTransformer":
        with open(os.path.join(path, cls.CONFIG_NAME)) as f:
            config = _yaml_load(f.read())
        mask_path = os.path.join(path, "mask.npy")
        mask = np.load(mask_path, allow_pickle=False) if os.path.exists(mask_path) else None
        return cls(np.load(os.path.join(path, "center.npy"), allow_pickle=False),
                   np.load(os.path.join(path, "scale.npy"), allow_pickle=False), config["spatial_features"],
                   config["num_variables"], mask=mask)


# the reference's other transformer types, by a file each writes; they need TensorFlow or pickled code
_FOREIGN_TRANSFORMERS = (("encoder.tf", "dense-autoencoder"), ("decoder.tf", "dense-autoencoder"),
                         ("sk_transformer.pkl", "sk-transformer"), ("sk_scaler.pkl", "sk-transformer"))


def load_transformer(path: str):
    """A transformer directory of ``TransformerGroup.dump`` (which writes no ``name`` file), read by its files."""
    if os.path.exists(os.path.join(path, DoNothingTransformer.CONFIG_NAME)):
        return DoNothingTransformer.load(path)
    if os.path.exists(os.path.join(path, ScaleSpatialConcatZTransformer.CONFIG_NAME)):
        return ScaleSpatialConcatZTransformer.load(path)
    name = None
    if os.path.exists(os.path.join(path, "name")):
        with open(os.path.join(path, "name")) as f:
            name = f.read().strip()
    for leaf, kind in _FOREIGN_TRANSFORMERS:
        if name is None and os.path.exists(os.path.join(path, leaf)):
            name = kind
    if name is not None:
        raise ValueError(f"transformer of type '{name}' in {path} is not supported: it needs the reference's "
                         "TensorFlow/sklearn stack; supported: do-nothing-transformer, scale-spatial-concat-z-transformer")
    raise ValueError(f"{path} holds no transformer this package can read")


# ---------------------------------------------------------------------------------------------
# sparse matrices in scipy.sparse.save_npz files
# ---------------------------------------------------------------------------------------------


class SparseMatrix:
    """The arrays of a ``save_npz`` file (``format`` csc / csr / coo), kept as read so that a dump writes them back."""

    def __init__(self, fmt: str, shape: Tuple[int, int], arrays: Mapping[str, np.ndarray]):
        if fmt not in ("csc", "csr", "coo"):
            raise ValueError(f"sparse format {fmt!r} is not supported (csc, csr, coo)")
        self.format = fmt
        self.shape = (int(shape[0]), int(shape[1]))
        self.arrays = dict(arrays)

    @classmethod
    def load(cls, path: str) -> "SparseMatrix":
        with np.load(path, allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        fmt = arrays["format"].item()
        fmt = fmt.decode("ascii") if isinstance(fmt, bytes) else str(fmt)
        return cls(fmt, tuple(arrays["shape"]), arrays)

    @classmethod
    def from_csr(cls, indptr, indices, data, shape) -> "SparseMatrix":
        return cls("csr", shape, {"indices": np.asarray(indices), "indptr": np.asarray(indptr), "format": np.array(b"csr"),
                                  "shape": np.asarray(shape, np.int64), "data": np.asarray(data)})

    def dump(self, path: str) -> None:
        with open(path, "wb") as f:
            np.savez_compressed(f, **self.arrays)

    @property
    def nnz(self) -> int:
        return int(self.arrays["data"].shape[0])

    def csr(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(indptr int64, indices int32, data float64) with columns ascending within each row (stable: duplicates in
        stored order)."""
        a, (m, n) = self.arrays, self.shape
        data = np.asarray(a["data"], np.float64)
        if self.format == "csr":
            ptr = np.asarray(a["indptr"], np.int64)
            row = np.repeat(np.arange(m, dtype=np.int64), np.diff(ptr))
            col = np.asarray(a["indices"], np.int64)
        elif self.format == "csc":
            ptr = np.asarray(a["indptr"], np.int64)
            col = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
            row = np.asarray(a["indices"], np.int64)
        else:
            row, col = np.asarray(a["row"], np.int64), np.asarray(a["col"], np.int64)
        if row.shape != data.shape or col.shape != data.shape:
            raise ValueError("sparse matrix arrays disagree in length")
        if data.size and (row.min() < 0 or row.max() >= m or col.min() < 0 or col.max() >= n):
            raise ValueError(f"sparse matrix index outside its shape {self.shape}")
        order = np.lexsort((col, row))
        indptr = np.zeros(m + 1, np.int64)
        np.cumsum(np.bincount(row, minlength=m), out=indptr[1:])
        return indptr, col[order].astype(np.int32), np.ascontiguousarray(data[order])

    def toarray(self) -> np.ndarray:
        out = np.zeros(self.shape, np.float64)
        indptr, idx, val = self.csr()
        rows = np.repeat(np.arange(self.shape[0]), np.diff(indptr))
        np.add.at(out, (rows, idx), val)
        return out


# ---------------------------------------------------------------------------------------------
# device model
# ---------------------------------------------------------------------------------------------

SQUARE_NONE, SQUARE_SUBDOMAINS, SQUARE_ELEMENTS = 0, 1, 2
WIN_AUTO, WIN_DENSE, WIN_CSR = 0, 1, 2


def _ptr(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def _fill_transformer(td, tf, keep: list):
    if tf is None:
        return
    td.kind = tf.kind
    td.n_variables = tf.n_variables
    nz = np.asarray(tf.original_feature_sizes, np.intc)
    keep.append(nz)
    td.var_nz = _ptr(nz, ctypes.c_int)
    if tf.kind == 1:
        td.nx, td.ny = tf.spatial_features[0], tf.spatial_features[1]
        c = np.ascontiguousarray(np.asarray(tf.center).reshape(-1), np.float32)
        s = np.ascontiguousarray(np.asarray(tf.scale).reshape(-1), np.float32)
        keep += [c, s]
        td.center, td.scale = _ptr(c, ctypes.c_float), _ptr(s, ctypes.c_float)
        if tf.mask is not None:
            m = np.ascontiguousarray(np.asarray(tf.mask).reshape(-1), np.float64)
            keep.append(m)
            td.mask = _ptr(m, ctypes.c_double)
            td.mask_f32 = int(np.asarray(tf.mask).dtype == np.float32)


def _expand_mask(mask, n_sub, n):
    m = np.asarray(mask)
    out = np.ascontiguousarray(np.broadcast_to(m.astype(np.float64), (n_sub, n)))
    return out, int(m.dtype == np.float32)


class ReservoirModel:
    """Device handle of a reservoir model (``fv3hip_reservoir_t``): state, weights and readout on one GPU.

    ``divider``: the input rank divider (with overlap); ``w_in`` [state, input_size] and ``w_res`` [state, state] as
    ``SparseMatrix``; ``coefficients`` [subdomain, state + n_hybrid, n_out] and ``intercepts`` [subdomain, n_out].

    ``w_in_storage``: ``WIN_CSR`` walks the stored entries of ``W_in`` as scipy's product does; ``WIN_DENSE`` multiplies the
    zero-padded matrix, so a non-finite input makes every state row of its subdomain NaN, not only the rows with a stored
    weight in that column.  ``WIN_AUTO`` picks dense storage from half the entries stored up and
    inherits this difference."""

    def __init__(self, divider: RankXYDivider, input_transformer, output_transformer, w_in: SparseMatrix,
                 w_res: SparseMatrix, coefficients: np.ndarray, intercepts: np.ndarray, square: int = SQUARE_NONE,
                 input_mask: Optional[np.ndarray] = None, hybrid_transformer=None, n_hybrid: int = 0,
                 hybrid_mask: Optional[np.ndarray] = None, state: Optional[np.ndarray] = None, w_in_storage: int = WIN_AUTO,
                 device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ReservoirModel needs a 'cuda' (ROCm) device; there is no CPU fallback")
        self.divider = divider
        self.n_subdomains = divider.n_subdomains
        self.state_size = int(w_res.shape[0])
        self.input_transformer, self.output_transformer, self.hybrid_transformer = (input_transformer, output_transformer,
                                                                                    hybrid_transformer)
        self.n_hybrid = int(n_hybrid)
        keep = []
        d = _lib.ReservoirDesc()
        d.layout_x, d.layout_y = divider.subdomain_layout
        d.overlap = divider.overlap
        d.rank_x, d.rank_y = divider.rank_extent
        d.state_size = self.state_size
        d.input_size = int(w_in.shape[1])
        if w_in.shape[0] != self.state_size or w_res.shape != (self.state_size, self.state_size):
            raise ValueError(f"W_in {w_in.shape} and W_res {w_res.shape} disagree on the state size")
        _fill_transformer(d.input, input_transformer, keep)
        _fill_transformer(d.output, output_transformer, keep)
        _fill_transformer(d.hybrid, hybrid_transformer if self.n_hybrid else None, keep)
        for prefix, mat in (("w_in", w_in), ("w_res", w_res)):
            ptr, idx, val = mat.csr()
            keep += [ptr, idx, val]
            setattr(d, prefix + "_indptr", _ptr(ptr, ctypes.c_int64))
            setattr(d, prefix + "_indices", _ptr(idx, ctypes.c_int32))
            setattr(d, prefix + "_data", _ptr(val, ctypes.c_double))
        d.w_in_storage = int(w_in_storage)
        if input_mask is not None:
            m, d.input_mask_f32 = _expand_mask(input_mask, self.n_subdomains, d.input_size)
            keep.append(m)
            d.input_mask = _ptr(m, ctypes.c_double)
        d.square = int(square)
        d.n_hybrid = self.n_hybrid
        if hybrid_mask is not None and self.n_hybrid:
            m, d.hybrid_mask_f32 = _expand_mask(hybrid_mask, self.n_subdomains, self.n_hybrid)
            keep.append(m)
            d.hybrid_mask = _ptr(m, ctypes.c_double)
        c = np.ascontiguousarray(coefficients, np.float64)
        b = np.ascontiguousarray(intercepts, np.float64)
        n_out = output_transformer.n_latent_dims * int(np.prod(divider.get_no_overlap_rank_divider().subdomain_extent))
        if c.shape != (self.n_subdomains, self.state_size + self.n_hybrid, n_out) or b.shape != (self.n_subdomains, n_out):
            raise ValueError(f"readout coefficients {c.shape} / intercepts {b.shape} do not match "
                             f"({self.n_subdomains}, {self.state_size + self.n_hybrid}, {n_out})")
        keep += [c, b]
        d.coefficients, d.intercepts = _ptr(c, ctypes.c_double), _ptr(b, ctypes.c_double)
        if state is not None:
            st = np.ascontiguousarray(np.broadcast_to(np.asarray(state, np.float64),
                                                      (self.n_subdomains, self.state_size)))
            keep.append(st)
            d.state = _ptr(st, ctypes.c_double)
        self.n_out = n_out
        with torch.cuda.device(self.device):
            _require_device(torch.empty(1, device=self.device))
            h = ctypes.c_void_p()
            _lib.call("fv3hip_reservoir_create", ctypes.byref(d), ctypes.byref(h))
            self._handle = h

    @staticmethod
    def _sources(tensors: Sequence[torch.Tensor]):
        n = len(tensors)
        strides = []
        for t in tensors:
            if t.dim() != 3:
                raise ValueError(f"inputs must be (x, y, z) arrays, got shape {tuple(t.shape)}")
            if t.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"inputs must be float32 or float64, got {t.dtype}")
            strides += list(t.stride())
        return ((ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors]),
                (ctypes.c_int * n)(*[_lib.F64 if t.dtype == torch.float64 else _lib.F32 for t in tensors]),
                (ctypes.c_int64 * (3 * n))(*strides))

    _PLAN_FIELDS = ("dense", "in_sb", "in_chunk", "in_split", "out_chunk", "out_split", "ldw", "ldc")

    def plan(self) -> dict:
        """The launch plan the library chose at creation (read-only): whether ``W_in`` is dense, the subdomains per wave,
        rows per slice and slice count of the dense input product, rows per slice and slice count of the readout, and the
        padded ``W_in`` row count and readout row length."""
        out = (ctypes.c_int64 * 8)()
        _lib.call("fv3hip_reservoir_plan", self._handle, out)
        return dict(zip(self._PLAN_FIELDS, (int(v) for v in out)))

    def increment(self, inputs: Sequence[torch.Tensor]) -> None:
        """One ``increment_state`` from device (x, y, z) arrays over the overlapped rank extent (shapes checked by the
        caller)."""
        dev = _require_device(*inputs)
        _lib.call_on(dev, "fv3hip_reservoir_increment", self._handle, *self._sources(inputs), _stream(dev))

    def predict(self, hybrid_inputs: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
        """The readout decoded into one (x, y, z) device array per output variable (float32 for a scale-spatial output
        transformer, float64 otherwise)."""
        rx, ry = self.divider.rank_extent
        dtype = torch.float32 if self.output_transformer.kind == 1 else torch.float64
        outs = [torch.empty((rx, ry, nz), dtype=dtype, device=self.device)
                for nz in self.output_transformer.original_feature_sizes]
        k = len(outs)
        out_args = ((ctypes.c_void_p * k)(*[t.data_ptr() for t in outs]),
                    (ctypes.c_int64 * (3 * k))(*[s for t in outs for s in t.stride()]))
        if self.n_hybrid:
            _require_device(*hybrid_inputs)
            src = self._sources(hybrid_inputs)
        else:
            src = (None, None, None)
        _lib.call_on(self.device, "fv3hip_reservoir_predict", self._handle, *src, *out_args, _stream(self.device))
        return outs

    def get_state(self) -> torch.Tensor:
        out = torch.empty((self.n_subdomains, self.state_size), dtype=torch.float64, device=self.device)
        _lib.call_on(self.device, "fv3hip_reservoir_get_state", self._handle, out.data_ptr(), _stream(self.device))
        return out

    def set_state(self, state) -> None:
        t = torch.as_tensor(state, dtype=torch.float64).to(self.device)
        if tuple(t.shape) != (self.n_subdomains, self.state_size):
            raise ValueError("Provided state does not match reservoir state shape")
        t = t.contiguous()
        _lib.call_on(self.device, "fv3hip_reservoir_set_state", self._handle, t.data_ptr(), _stream(self.device))
        self._keep = t  # alive until the copy on the stream has run

    def reset_state(self) -> None:
        _lib.call_on(self.device, "fv3hip_reservoir_reset_state", self._handle, _stream(self.device))

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            try:
                _lib.load().fv3hip_reservoir_destroy(h)
            except Exception:
                pass
