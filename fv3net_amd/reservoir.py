"""Reservoir computing: the rank divider, the transformers, the sparse weight files and the device handle.

``DenseAutoencoder`` and ``SkTransformer`` are the two transformers that reduce the dimension of a column, on the GPU
(``csrc/codec.hip``).  ``RankXYDivider`` is the subdomain index arithmetic of fv3fit's ``reservoir/domain2.py`` (numpy only; pace's
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
from .cube import cuda_device
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


# ---------------------------------------------------------------------------------------------
# column codecs: the transformers that reduce the dimension of a column (csrc/codec.hip)
# ---------------------------------------------------------------------------------------------


def _ptr(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def _fill_variables(d, sizes, keep: list):
    """``n_variables`` and ``var_nz`` of a transformer or codec descriptor."""
    nz = np.asarray(sizes, np.intc)
    keep.append(nz)
    d.n_variables, d.var_nz = len(nz), _ptr(nz, ctypes.c_int)


def _xyz_args(tensors: Sequence[torch.Tensor], ndim: int, what: str):
    """(pointer table, dtype codes, strides) of device arrays as the library's entry points take their sources: (x, y, z)
    arrays (``ndim`` 3) or [t, x, y, z] series (``ndim`` 4), float32 or float64, strided as they come."""
    n = len(tensors)
    strides = []
    for t in tensors:
        if t.dim() != ndim:
            dims = "(x, y, z)" if ndim == 3 else "(t, x, y, z)"
            raise ValueError(f"{what} must be {dims} arrays, got shape {tuple(t.shape)}")
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{what} must be float32 or float64, got {t.dtype}")
        strides += list(t.stride())
    return ((ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors]),
            (ctypes.c_int * n)(*[_lib.F64 if t.dtype == torch.float64 else _lib.F32 for t in tensors]),
            (ctypes.c_int64 * (ndim * n))(*strides))


def _out_args(tensors: Sequence[torch.Tensor]):
    """(pointer table, strides) of (x, y, z) device arrays as the entry points take their outputs."""
    n = len(tensors)
    return ((ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors]),
            (ctypes.c_int64 * (3 * n))(*[s for t in tensors for s in t.stride()]))


def _create(fn: str, device, *args):
    """A handle of ``fn`` (which takes ``args``, then the address of the handle), created on ``device``."""
    h = ctypes.c_void_p()
    with torch.cuda.device(device):
        _require_device(torch.empty(1, device=device))
        _lib.call(fn, *args, ctypes.byref(h))
    return h


def _destroy(fn: str, handle) -> None:
    if handle:
        try:
            getattr(_lib.load(), fn)(handle)
        except Exception:
            pass


def _npz_load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


class _ColumnCodec:
    """What the two column codecs share: the device handle (``fv3hip_codec_t``, created on first use) and the four entry
    points.  ``encode`` / ``decode`` take arrays whose last dimension is the feature dimension, ``encode_unstacked_xyz`` /
    ``decode_unstacked_xyz`` take (x, y, z) arrays; all four return numpy for numpy and device tensors for device tensors.
    There is no host path: the arithmetic runs in the HIP kernels."""

    is_column_codec = True
    kind = None  # not a transformer the reservoir handle knows: the model classes put a do-nothing transformer in its place
    latent_dtype = torch.float32
    output_dtype = torch.float32
    original_feature_sizes: List[int]

    @property
    def n_variables(self) -> int:
        return len(self.original_feature_sizes)

    @property
    def n_features(self) -> int:
        return sum(self.original_feature_sizes)

    def check_inputs(self, shapes: Sequence[Tuple[int, ...]]):
        if len(shapes) != self.n_variables:
            raise ValueError(f"Expected {self.n_variables} input arrays but got {len(shapes)}")
        for i, (shape, nz) in enumerate(zip(shapes, self.original_feature_sizes)):
            if len(shape) == 0 or shape[-1] != nz:
                raise ValueError(f"input array {i} has shape {tuple(shape)}, its feature dimension must be {nz}")

    # -- device ----------------------------------------------------------------------------------
    def _fill(self, d, keep):
        raise NotImplementedError

    def _handle_on(self, device):
        device = cuda_device(device, type(self).__name__)
        handles = self.__dict__.setdefault("_handles", {})
        if device.index not in handles:
            keep = []
            d = _lib.CodecDesc()
            _fill_variables(d, self.original_feature_sizes, keep)
            d.n_latent = self.n_latent_dims
            self._fill(d, keep)
            handles[device.index] = _create("fv3hip_codec_create", device, ctypes.byref(d))
        return handles[device.index]

    def encode_device(self, tensors: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(x, y, z) device arrays, float32 or float64 and strided as they come, to the latent [x, y, n_latent] (written
        into ``out`` when given: contiguous, of ``latent_dtype``).  One launch; nothing is allocated beside ``out``."""
        self.check_inputs([tuple(t.shape) for t in tensors])
        dev = _require_device(*tensors)
        nx, ny = int(tensors[0].shape[0]), int(tensors[0].shape[1])
        for i, t in enumerate(tensors):
            if t.dim() != 3 or tuple(t.shape[:2]) != (nx, ny):
                raise ValueError(f"input array {i} has shape {tuple(t.shape)}, expected ({nx}, {ny}, z)")
        if out is None:
            out = torch.empty((nx, ny, self.n_latent_dims), dtype=self.latent_dtype, device=dev)
        elif (tuple(out.shape) != (nx, ny, self.n_latent_dims) or out.dtype != self.latent_dtype
              or not out.is_contiguous()):
            raise ValueError(f"the latent buffer must be a contiguous {self.latent_dtype} array of shape "
                             f"{(nx, ny, self.n_latent_dims)}")
        _lib.call_on(dev, "fv3hip_codec_encode", self._handle_on(dev), *_xyz_args(tensors, 3, "inputs"), nx, ny,
                     out.data_ptr(), _stream(dev))
        return out

    def decode_device(self, latent: torch.Tensor, outs: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
        """The latent [x, y, n_latent] (float32 or float64, contiguous) to one (x, y, z) array of ``output_dtype`` per variable
        (written into ``outs`` when given, strided as they come)."""
        dev = _require_device(latent)
        if latent.dim() != 3 or latent.shape[-1] != self.n_latent_dims:
            raise ValueError(f"the latent must have shape (x, y, {self.n_latent_dims}), got {tuple(latent.shape)}")
        if latent.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"the latent must be float32 or float64, got {latent.dtype}")
        latent = latent.contiguous()
        nx, ny = int(latent.shape[0]), int(latent.shape[1])
        if outs is None:
            outs = [torch.empty((nx, ny, nz), dtype=self.output_dtype, device=dev) for nz in self.original_feature_sizes]
        for i, (t, nz) in enumerate(zip(outs, self.original_feature_sizes)):
            if tuple(t.shape) != (nx, ny, nz) or t.dtype != self.output_dtype:
                raise ValueError(f"output array {i} must be {self.output_dtype} of shape {(nx, ny, nz)}")
        _require_device(*outs)
        _lib.call_on(dev, "fv3hip_codec_decode", self._handle_on(dev), latent.data_ptr(),
                     _lib.F64 if latent.dtype == torch.float64 else _lib.F32, nx, ny, *_out_args(outs), _stream(dev))
        return list(outs)

    @staticmethod
    def _default_device():
        from .cubedsphere._device import compute_device

        return compute_device()

    def encode_unstacked_xyz(self, arrays: Sequence):
        if all(isinstance(a, torch.Tensor) and a.is_cuda for a in arrays):
            return self.encode_device(list(arrays))
        dev = self._default_device()
        return self.encode_device([torch.as_tensor(np.asarray(a)).to(dev) for a in arrays]).cpu().numpy()

    def decode_unstacked_xyz(self, latent):
        if isinstance(latent, torch.Tensor) and latent.is_cuda:
            return self.decode_device(latent)
        return [t.cpu().numpy() for t in self.decode_device(torch.as_tensor(np.asarray(latent)).to(self._default_device()))]

    def encode(self, arrays: Sequence):
        """Arrays [..., z_v] with the same leading dimensions to the latent [..., n_latent]."""
        self.check_inputs([tuple(a.shape) for a in arrays])
        lead = tuple(arrays[0].shape[:-1])
        out = self.encode_unstacked_xyz([a.reshape(-1, 1, a.shape[-1]) for a in arrays])
        return out.reshape(lead + (self.n_latent_dims,))

    def decode(self, latent):
        lead = tuple(latent.shape[:-1])
        outs = self.decode_unstacked_xyz(latent.reshape(-1, 1, latent.shape[-1]))
        return [o.reshape(lead + (o.shape[-1],)) for o in outs]

    def predict(self, arrays: Sequence):
        """The round trip ``decode(encode(arrays))``, as the reference's ``SkTransformer.predict``: what the codec loses."""
        return self.decode(self.encode(arrays))

    def __del__(self):
        for h in self.__dict__.get("_handles", {}).values():
            _destroy("fv3hip_codec_destroy", h)


def _f32_list(arrays, what):
    out = [np.ascontiguousarray(a, np.float32) for a in arrays]
    for a in out:
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{what} must be finite")
    return out


class DenseAutoencoder(_ColumnCodec):
    """fv3fit's ``"dense-autoencoder"`` transformer as plain arrays (``dense_autoencoder.yaml`` + ``weights.npz``), float32
    throughout as Keras computes it.

    encode: ``(x - center) / (scale + 1e-7)`` per feature of the concatenated column, then ``relu(h @ W + b)`` per encoder
    layer (kernels [in, out] as Keras stores them); the last encoder layer is the latent layer and is a ReLU too.  decode:
    the decoder's ReLU layers, one linear head per variable, ``y * scale + center`` and the optional output limits
    (``output_min`` / ``output_max`` per variable, None: no limit; below min -> min, at or above max -> max, NaN stays).
    Without encoder layers it is the reference's "concat and scale only" form (no decoder layers, no heads).

    There is no ``from_keras``: a TF SavedModel cannot be read without TensorFlow, and the normalisation constants are graph
    constants that ``get_weights()`` does not return.  INTEGRATION.md shows the export."""

    CONFIG_NAME = "dense_autoencoder.yaml"
    WEIGHTS_NAME = "weights.npz"
    latent_dtype = torch.float32
    output_dtype = torch.float32
    MAX_VARIABLES, MAX_FEATURES, MAX_WIDTH, MAX_LAYERS = 16, 1024, 256, 8

    def __init__(self, center, scale, original_feature_sizes: Sequence[int], encoder_kernels=(), encoder_biases=(),
                 decoder_kernels=(), decoder_biases=(), head_kernels=(), head_biases=(), output_min=None, output_max=None):
        self.original_feature_sizes = [int(v) for v in original_feature_sizes]
        k = self.n_features
        self.center = np.ascontiguousarray(np.asarray(center).reshape(-1), np.float32)
        self.scale = np.ascontiguousarray(np.asarray(scale).reshape(-1), np.float32)
        if self.center.size != k or self.scale.size != k:
            raise ValueError(f"center and scale need {k} values (the sum of original_feature_sizes), got "
                             f"{self.center.size} and {self.scale.size}")
        self.encoder_kernels = _f32_list(encoder_kernels, "encoder kernels")
        self.encoder_biases = _f32_list(encoder_biases, "encoder biases")
        self.decoder_kernels = _f32_list(decoder_kernels, "decoder kernels")
        self.decoder_biases = _f32_list(decoder_biases, "decoder biases")
        self.head_kernels = _f32_list(head_kernels, "head kernels")
        self.head_biases = _f32_list(head_biases, "head biases")
        n = self.n_variables
        self.output_min = [None] * n if output_min is None else [None if v is None else float(v) for v in output_min]
        self.output_max = [None] * n if output_max is None else [None if v is None else float(v) for v in output_max]
        if len(self.output_min) != n or len(self.output_max) != n:
            raise ValueError(f"output_min and output_max need one entry per variable ({n})")
        for lo, hi in zip(self.output_min, self.output_max):
            if lo is not None and hi is not None and hi <= lo:
                raise ValueError(f"max value ({hi}) must be greater than min value ({lo}).")
        self._check_chain()

    def _check_chain(self):
        k = self.n_features
        if not self.encoder_kernels:
            if self.decoder_kernels or self.head_kernels:
                raise ValueError("an autoencoder without encoder layers (concat and scale only) has no decoder layers or heads")
            return

        def chain(side, width, kernels, biases):
            if len(kernels) != len(biases):
                raise ValueError(f"{side}: {len(kernels)} kernels but {len(biases)} biases")
            for i, (w, b) in enumerate(zip(kernels, biases)):
                if w.ndim != 2 or w.shape[0] != width or b.shape != (w.shape[1],):
                    raise ValueError(f"{side} layer {i}: kernel {w.shape} / bias {b.shape} do not follow an input of "
                                     f"width {width}")
                width = w.shape[1]
            return width

        latent = chain("encoder", k, self.encoder_kernels, self.encoder_biases)
        width = chain("decoder", latent, self.decoder_kernels, self.decoder_biases)
        if len(self.head_kernels) != self.n_variables or len(self.head_biases) != self.n_variables:
            raise ValueError(f"need one head per variable ({self.n_variables}), got {len(self.head_kernels)} kernels and "
                             f"{len(self.head_biases)} biases")
        for v, (w, b, nz) in enumerate(zip(self.head_kernels, self.head_biases, self.original_feature_sizes)):
            if w.shape != (width, nz) or b.shape != (nz,):
                raise ValueError(f"head {v}: kernel {w.shape} / bias {b.shape}, expected {(width, nz)} / {(nz,)}")

    @property
    def n_latent_dims(self) -> int:
        return int(self.encoder_kernels[-1].shape[1]) if self.encoder_kernels else self.n_features

    def _fill(self, d, keep):
        d.kind = _lib.CODEC_DENSE
        d.center, d.scale = _ptr(self.center, ctypes.c_float), _ptr(self.scale, ctypes.c_float)

        def pointers(arrays):
            arr = (ctypes.POINTER(ctypes.c_float) * max(len(arrays), 1))(*[_ptr(a, ctypes.c_float) for a in arrays])
            keep.append(arr)
            return arr

        def units(kernels):
            u = np.asarray([w.shape[1] for w in kernels], np.intc)
            keep.append(u)
            return _ptr(u, ctypes.c_int)

        d.n_enc, d.n_dec = len(self.encoder_kernels), len(self.decoder_kernels)
        if d.n_enc:
            d.enc_units, d.enc_kernels, d.enc_biases = (units(self.encoder_kernels), pointers(self.encoder_kernels),
                                                        pointers(self.encoder_biases))
            d.head_kernels, d.head_biases = pointers(self.head_kernels), pointers(self.head_biases)
        if d.n_dec:
            d.dec_units, d.dec_kernels, d.dec_biases = (units(self.decoder_kernels), pointers(self.decoder_kernels),
                                                        pointers(self.decoder_biases))
        for name, bounds in (("out_min", self.output_min), ("out_max", self.output_max)):
            if any(v is not None for v in bounds):
                a = np.asarray([np.nan if v is None else v for v in bounds], np.float32)
                keep.append(a)
                setattr(d, name, _ptr(a, ctypes.c_float))

    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, self.CONFIG_NAME), "w") as f:
            yaml.safe_dump({"original_feature_sizes": self.original_feature_sizes,
                            "n_encoder_layers": len(self.encoder_kernels), "n_decoder_layers": len(self.decoder_kernels),
                            "output_min": self.output_min, "output_max": self.output_max}, f)
        arrays = {"center": self.center, "scale": self.scale}
        for prefix, ws, bs in (("encoder", self.encoder_kernels, self.encoder_biases),
                               ("decoder", self.decoder_kernels, self.decoder_biases),
                               ("head", self.head_kernels, self.head_biases)):
            for i, (w, b) in enumerate(zip(ws, bs)):
                arrays[f"{prefix}_kernel_{i}"], arrays[f"{prefix}_bias_{i}"] = w, b
        with open(os.path.join(path, self.WEIGHTS_NAME), "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path: str) -> "DenseAutoencoder":
        with open(os.path.join(path, cls.CONFIG_NAME)) as f:
            config = _yaml_load(f.read())
        z = _npz_load(os.path.join(path, cls.WEIGHTS_NAME))
        n_enc, n_dec = config["n_encoder_layers"], config["n_decoder_layers"]
        n_head = len(config["original_feature_sizes"]) if n_enc else 0
        pick = lambda prefix, what, n: [z[f"{prefix}_{what}_{i}"] for i in range(n)]  # noqa: E731
        return cls(z["center"], z["scale"], config["original_feature_sizes"], pick("encoder", "kernel", n_enc),
                   pick("encoder", "bias", n_enc), pick("decoder", "kernel", n_dec), pick("decoder", "bias", n_dec),
                   pick("head", "kernel", n_head), pick("head", "bias", n_head), config.get("output_min"),
                   config.get("output_max"))


class SkTransformer(_ColumnCodec):
    """fv3fit's ``"sk-transformer"`` (``StandardScaler`` + ``PCA``) as plain arrays (``sk_transformer.yaml`` +
    ``arrays.npz``), float64 throughout.

    encode: ``z = (((x - scaler_mean) / scaler_scale) - pca_mean) @ components.T``, divided by
    ``sqrt(explained_variance)`` when the PCA whitens.  decode: ``z @ components`` (row j times
    ``sqrt(explained_variance[j])`` when it whitens) ``+ pca_mean``, times ``scaler_scale`` plus ``scaler_mean``; with
    ``enforce_positive_outputs`` then ``np.where(decoded >= 0, decoded, 0.0)``, which turns a NaN into 0.0 as the
    reference's does.  ``scaler_mean`` / ``scaler_scale`` of None are ``with_mean=False`` / ``with_std=False``.

    Two deliberate differences from the reference: sklearn keeps an all-float32 pack in float32 where this codec always
    computes in float64 (float32 sources are widened first, the outputs are float64); and ``original_feature_sizes`` is
    required here, where the reference sets it on the first ``encode``, because ``decode`` and the reservoir's rank divider
    need it before any data has been seen."""

    CONFIG_NAME = "sk_transformer.yaml"
    ARRAYS_NAME = "arrays.npz"
    latent_dtype = torch.float64
    output_dtype = torch.float64

    def __init__(self, components, pca_mean, original_feature_sizes: Sequence[int], explained_variance=None,
                 scaler_mean=None, scaler_scale=None, enforce_positive_outputs: bool = False):
        if original_feature_sizes is None:
            raise ValueError("original_feature_sizes is required (the reference sets it on the first encode)")
        self.original_feature_sizes = [int(v) for v in original_feature_sizes]
        k = self.n_features
        f64 = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)  # noqa: E731
        self.components, self.pca_mean = f64(components), f64(pca_mean).reshape(-1)
        self.explained_variance = f64(explained_variance)
        self.scaler_mean, self.scaler_scale = f64(scaler_mean), f64(scaler_scale)
        self.enforce_positive_outputs = bool(enforce_positive_outputs)
        if self.components.ndim != 2 or self.components.shape[1] != k or self.pca_mean.shape != (k,):
            raise ValueError(f"components {self.components.shape} / pca_mean {self.pca_mean.shape} do not match the "
                             f"{k} features of original_feature_sizes")
        for name, a, n in (("explained_variance", self.explained_variance, self.components.shape[0]),
                           ("scaler_mean", self.scaler_mean, k), ("scaler_scale", self.scaler_scale, k)):
            if a is not None and a.shape != (n,):
                raise ValueError(f"{name} needs shape {(n,)}, got {a.shape}")

    @property
    def n_latent_dims(self) -> int:
        return int(self.components.shape[0])

    @classmethod
    def from_sklearn(cls, transformer, scaler, enforce_positive_outputs: bool = False,
                     original_feature_sizes: Optional[Sequence[int]] = None) -> "SkTransformer":
        """From a fitted ``sklearn.decomposition.PCA`` (whitened or not) and ``StandardScaler``, by their attributes alone
        (sklearn is not imported).  Any other transformer is refused by its type."""
        if type(transformer).__name__ != "PCA" or not hasattr(transformer, "components_"):
            raise ValueError(f"transformer of type '{type(transformer).__name__}' is not supported: only a fitted "
                             "sklearn.decomposition.PCA is")
        if type(scaler).__name__ != "StandardScaler" or not hasattr(scaler, "n_features_in_"):
            raise ValueError(f"scaler of type '{type(scaler).__name__}' is not supported: only a fitted "
                             "sklearn.preprocessing.StandardScaler is")
        if original_feature_sizes is None:
            raise ValueError("original_feature_sizes is required (the reference sets it on the first encode)")
        return cls(transformer.components_, transformer.mean_, original_feature_sizes,
                   explained_variance=transformer.explained_variance_ if transformer.whiten else None,
                   scaler_mean=scaler.mean_ if scaler.with_mean else None,
                   scaler_scale=scaler.scale_ if scaler.with_std else None,
                   enforce_positive_outputs=enforce_positive_outputs)

    def _fill(self, d, keep):
        d.kind = _lib.CODEC_AFFINE
        d.pca_mean, d.components = _ptr(self.pca_mean, ctypes.c_double), _ptr(self.components, ctypes.c_double)
        for name, a in (("mean", self.scaler_mean), ("std", self.scaler_scale),
                        ("explained_variance", self.explained_variance)):
            if a is not None:
                setattr(d, name, _ptr(a, ctypes.c_double))
        d.enforce_positive = int(self.enforce_positive_outputs)

    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, self.CONFIG_NAME), "w") as f:
            yaml.safe_dump({"original_feature_sizes": self.original_feature_sizes,
                            "enforce_positive_outputs": self.enforce_positive_outputs}, f)
        arrays = {"components": self.components, "pca_mean": self.pca_mean}
        for name in ("explained_variance", "scaler_mean", "scaler_scale"):
            if getattr(self, name) is not None:
                arrays[name] = getattr(self, name)
        with open(os.path.join(path, self.ARRAYS_NAME), "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path: str) -> "SkTransformer":
        with open(os.path.join(path, cls.CONFIG_NAME)) as f:
            config = _yaml_load(f.read())
        z = _npz_load(os.path.join(path, cls.ARRAYS_NAME))
        return cls(z["components"], z["pca_mean"], config["original_feature_sizes"],
                   explained_variance=z.get("explained_variance"), scaler_mean=z.get("scaler_mean"),
                   scaler_scale=z.get("scaler_scale"), enforce_positive_outputs=config["enforce_positive_outputs"])


def is_column_codec(tf) -> bool:
    return bool(getattr(tf, "is_column_codec", False))


# the reference's own files of those two types; they need TensorFlow or pickled code
_FOREIGN_TRANSFORMERS = (("encoder.tf", "dense-autoencoder"), ("decoder.tf", "dense-autoencoder"),
                         ("sk_transformer.pkl", "sk-transformer"), ("sk_scaler.pkl", "sk-transformer"))


def load_transformer(path: str):
    """A transformer directory of ``TransformerGroup.dump`` (which writes no ``name`` file), read by its files."""
    if os.path.exists(os.path.join(path, DoNothingTransformer.CONFIG_NAME)):
        return DoNothingTransformer.load(path)
    if os.path.exists(os.path.join(path, ScaleSpatialConcatZTransformer.CONFIG_NAME)):
        return ScaleSpatialConcatZTransformer.load(path)
    for codec in (DenseAutoencoder, SkTransformer):
        if os.path.exists(os.path.join(path, codec.CONFIG_NAME)):
            return codec.load(path)
    name = None
    if os.path.exists(os.path.join(path, "name")):
        with open(os.path.join(path, "name")) as f:
            name = f.read().strip()
    for leaf, kind in _FOREIGN_TRANSFORMERS:
        if name is None and os.path.exists(os.path.join(path, leaf)):
            name = kind
    if name is not None:
        raise ValueError(f"transformer of type '{name}' in {path} is not supported: it needs the reference's "
                         "TensorFlow/sklearn stack; supported: do-nothing-transformer, scale-spatial-concat-z-transformer, "
                         "and the array exports of the other two (DenseAutoencoder / SkTransformer.from_sklearn, "
                         "INTEGRATION.md)")
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


def _fill_transformer(td, tf, keep: list):
    if tf is None:
        return
    td.kind = tf.kind
    _fill_variables(td, tf.original_feature_sizes, keep)
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
        self._handle = _create("fv3hip_reservoir_create", self.device, ctypes.byref(d))

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
        _lib.call_on(dev, "fv3hip_reservoir_increment", self._handle, *_xyz_args(inputs, 3, "inputs"), _stream(dev))

    def predict(self, hybrid_inputs: Optional[Sequence[torch.Tensor]] = None,
                outs: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
        """The readout decoded into one (x, y, z) device array per output variable (float32 for a scale-spatial output
        transformer, float64 otherwise); written into ``outs`` when given."""
        rx, ry = self.divider.rank_extent
        dtype = torch.float32 if self.output_transformer.kind == 1 else torch.float64
        sizes = self.output_transformer.original_feature_sizes
        if outs is None:
            outs = [torch.empty((rx, ry, nz), dtype=dtype, device=self.device) for nz in sizes]
        else:
            outs = list(outs)
            _require_device(*outs)
            if len(outs) != len(sizes) or any(tuple(t.shape) != (rx, ry, nz) or t.dtype != dtype
                                              for t, nz in zip(outs, sizes)):
                raise ValueError(f"outs must be {dtype} arrays of shapes {[(rx, ry, nz) for nz in sizes]}")
        if self.n_hybrid:
            _require_device(*hybrid_inputs)
            src = _xyz_args(hybrid_inputs, 3, "inputs")
        else:
            src = (None, None, None)
        _lib.call_on(self.device, "fv3hip_reservoir_predict", self._handle, *src, *_out_args(outs), _stream(self.device))
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

    # -- training --------------------------------------------------------------
    @staticmethod
    def _series_sources(tensors: Sequence[torch.Tensor], extent, sizes, n_times: int, what: str):
        """[t, x, y, z] device arrays as the series entry points take them; every shape is checked here, since the kernels
        index by the model's extents alone."""
        if len(tensors) != len(sizes):
            raise ValueError(f"Expected {len(sizes)} {what} arrays but got {len(tensors)}")
        for i, (t, nz) in enumerate(zip(tensors, sizes)):
            if tuple(t.shape) != (n_times, *extent, nz):
                raise ValueError(f"{what} array {i} has shape {tuple(t.shape)}, expected {(n_times, *extent, nz)}")
        return _xyz_args(tensors, 4, f"{what} arrays")

    def train_series(self, inputs: Sequence[torch.Tensor], hybrid_inputs: Optional[Sequence[torch.Tensor]] = None,
                     noise: Optional[torch.Tensor] = None, square_even_elements: bool = False) -> torch.Tensor:
        """One increment per time step of the [t, x, y, z] device arrays (over the overlapped rank extent) and the readout
        inputs after each: X [t, subdomain, state_size + n_hybrid] float64, the state with its even elements squared when
        asked, then the encoded, masked hybrid inputs ([t, x, y, z] over the rank extent) of the same time step.  ``noise``
        [t, subdomain, input_size] float64 is added to the encoded inputs, times the input mask."""
        dev = _require_device(*inputs)
        n_t = int(inputs[0].shape[0])
        src = self._series_sources(inputs, self.divider.overlap_rank_extent, self.input_transformer.original_feature_sizes,
                                   n_t, "input")
        if self.n_hybrid:
            _require_device(*hybrid_inputs)
            hyb = self._series_sources(hybrid_inputs, self.divider.rank_extent, self.hybrid_transformer.original_feature_sizes,
                                       n_t, "hybrid")
        else:
            hyb = (None, None, None)
        n_in = self.divider.flat_subdomain_len
        if noise is not None:
            _require_device(noise)
            if tuple(noise.shape) != (n_t, self.n_subdomains, n_in) or noise.dtype != torch.float64:
                raise ValueError(f"noise must be a float64 array of shape {(n_t, self.n_subdomains, n_in)}")
            noise = noise.contiguous()
        out = torch.empty((n_t, self.n_subdomains, self.state_size + self.n_hybrid), dtype=torch.float64, device=self.device)
        _lib.call_on(dev, "fv3hip_reservoir_train_series", self._handle, *src, None if noise is None else noise.data_ptr(),
                     *hyb, n_t, int(bool(square_even_elements)), out.data_ptr(), _stream(dev))
        self._keep = noise  # alive until the launches on the stream have run
        return out

    def encode_targets(self, outputs: Sequence[torch.Tensor]) -> torch.Tensor:
        """The output transformer's encoding of [t, x, y, z] device arrays over the rank extent without overlap, per
        subdomain: Y [t, subdomain, n_out] float64."""
        dev = _require_device(*outputs)
        n_t = int(outputs[0].shape[0])
        src = self._series_sources(outputs, self.divider.rank_extent, self.output_transformer.original_feature_sizes, n_t,
                                   "output")
        out = torch.empty((n_t, self.n_subdomains, self.n_out), dtype=torch.float64, device=self.device)
        _lib.call_on(dev, "fv3hip_reservoir_encode_targets", self._handle, *src, n_t, out.data_ptr(), _stream(dev))
        return out

    def __del__(self):
        _destroy("fv3hip_reservoir_destroy", getattr(self, "_handle", None))


class GramAccumulator:
    """Device handle of the readout regression's sums (``fv3hip_gram_t``, ``csrc/gram.hip``): per subdomain
    ``A += X.T @ X`` [J1, J1] and ``B += X.T @ Y`` [J1, n_out] in float64, J1 = J + 1 with ``add_bias`` (a column of ones
    that is never materialised).  The bits depend on the shapes only and every ``A[s]`` is bitwise symmetric."""

    K_STEP = 4  # time steps per MFMA: two updates equal one bit for bit when the first has a multiple of this many

    def __init__(self, n_subdomains: int, n_features: int, n_outputs: int, add_bias: bool = True, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GramAccumulator needs a 'cuda' (ROCm) device; there is no CPU fallback")
        self.n_subdomains, self.n_features, self.n_outputs = int(n_subdomains), int(n_features), int(n_outputs)
        self.add_bias = bool(add_bias)
        self.n_rows = self.n_features + int(self.add_bias)
        self._handle = _create("fv3hip_gram_create", self.device, self.n_subdomains, self.n_features, self.n_outputs,
                               int(self.add_bias))

    def reset(self) -> None:
        _lib.call_on(self.device, "fv3hip_gram_reset", self._handle, _stream(self.device))

    def update(self, X: torch.Tensor, Y: torch.Tensor) -> None:
        """``X`` [t, subdomain, J] and ``Y`` [t, subdomain, n_out]: float64 device arrays, strided views allowed in the
        time and subdomain dimensions (the feature dimension must be contiguous)."""
        _require_device(X, Y)
        n_t = int(X.shape[0]) if X.dim() == 3 else -1
        if X.dim() != 3 or tuple(X.shape[1:]) != (self.n_subdomains, self.n_features):
            raise ValueError(f"X must have shape (t, {self.n_subdomains}, {self.n_features}), got {tuple(X.shape)}")
        if tuple(Y.shape) != (n_t, self.n_subdomains, self.n_outputs):
            raise ValueError(f"y must have shape ({n_t}, {self.n_subdomains}, {self.n_outputs}), got {tuple(Y.shape)}")
        if X.dtype != torch.float64 or Y.dtype != torch.float64:
            raise TypeError("X and y must be float64")
        if n_t == 0:
            return
        fix = lambda a: a if (a.shape[2] == 1 or a.stride(2) == 1) and a.stride(0) >= 0 and a.stride(1) >= 0 \
            else a.contiguous()  # noqa: E731
        X, Y = fix(X), fix(Y)
        _lib.call_on(self.device, "fv3hip_gram_update", self._handle, X.data_ptr(), X.stride(0), X.stride(1), Y.data_ptr(),
                     Y.stride(0), Y.stride(1), n_t, _stream(self.device))
        self._keep = (X, Y)  # alive until the launch on the stream has run

    def get(self, subdomain: Optional[int] = None):
        """(A, B) of one subdomain ([J1, J1], [J1, n_out]), or of all of them with a leading subdomain dimension."""
        lead = (self.n_subdomains,) if subdomain is None else ()
        if subdomain is not None and not 0 <= subdomain < self.n_subdomains:
            raise ValueError(f"subdomain {subdomain} is outside [0, {self.n_subdomains})")
        a = torch.empty(lead + (self.n_rows, self.n_rows), dtype=torch.float64, device=self.device)
        b = torch.empty(lead + (self.n_rows, self.n_outputs), dtype=torch.float64, device=self.device)
        _lib.call_on(self.device, "fv3hip_gram_get", self._handle, -1 if subdomain is None else int(subdomain), a.data_ptr(),
                     b.data_ptr(), _stream(self.device))
        return a, b

    def __del__(self):
        _destroy("fv3hip_gram_destroy", getattr(self, "_handle", None))
