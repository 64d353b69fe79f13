"""Convolutional network: the arrays of fv3fit's ``"convolutional"`` model and its device handle.

``ConvSpec`` holds what ``ConvolutionalNetworkConfig.build`` + ``build_model`` produce
(external/fv3fit/fv3fit/keras/_models/shared/convolutional_network.py:103-195, convolutional.py:153-210) as plain arrays:
per input variable the normalisation, ``depth - 1`` hidden ``Conv2D`` kernels ``[k, k, c_in, filters]`` (Keras layout: first
kernel axis along ``x``, cross-correlation, ``padding="valid"``) with optional biases, and one 1 x 1 head per output with its
de-normalisation.  ``ConvModel`` uploads it once (``fv3hip_conv_create``) and runs ``fv3hip_conv_predict`` on device arrays
read through their strides; the halo of ``halos_required`` cells comes with the input, from strip buffers, or from the
neighbouring faces of a resident six-tile cube.
"""
import ctypes
import dataclasses
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .ops import _require_device, _stream

ACTIVATIONS = {"linear": _lib.ACT_LINEAR, "relu": _lib.ACT_RELU, "tanh": _lib.ACT_TANH}
HALO_MODES = {"input": _lib.CONV_HALO_INPUT, "strips": _lib.CONV_HALO_STRIPS, "cube": _lib.CONV_HALO_CUBE}


def halos_required(kernel_size: int, depth: int) -> int:
    """``ConvolutionalNetwork.halos_required`` (convolutional_network.py:103-134) with the configuration's checks."""
    if depth < 1:
        raise ValueError("depth must be at least 1, so we can have an output layer")
    if kernel_size % 2 == 0:
        raise ValueError("kernel_size must be odd")
    return (kernel_size - 1) // 2 * (depth - 1)


@dataclasses.dataclass
class ConvInput:
    """One input variable: ``nfeat`` channels normalised as ``(x - center) / scale`` (scale = std + epsilon, float32)."""

    source: str
    nfeat: int
    center: np.ndarray
    scale: np.ndarray


@dataclasses.dataclass
class ConvOutput:
    """One head: 1 x 1 kernel ``[filters, nfeat]``, bias, then ``y * scale + center``."""

    name: str
    nfeat: int
    kernel: np.ndarray
    bias: np.ndarray
    scale: np.ndarray
    center: np.ndarray


@dataclasses.dataclass
class ConvSpec:
    inputs: List[ConvInput]
    hidden_kernels: List[np.ndarray]            # depth - 1 arrays [k, k, c_in, filters]
    hidden_biases: Optional[List[np.ndarray]]   # None: no biases (a ``diffusive`` network)
    outputs: List[ConvOutput]
    activation: str = "relu"

    def __post_init__(self):
        self.validate()

    @property
    def depth(self) -> int:
        return len(self.hidden_kernels) + 1

    @property
    def kernel_size(self) -> int:
        return int(self.hidden_kernels[0].shape[0])

    @property
    def filters(self) -> int:
        return int(self.hidden_kernels[0].shape[3])

    @property
    def n_in_channels(self) -> int:
        return sum(i.nfeat for i in self.inputs)

    @property
    def halos_required(self) -> int:
        return halos_required(self.kernel_size, self.depth)

    @property
    def sources(self) -> List[str]:
        return [i.source for i in self.inputs]

    @property
    def output_names(self) -> List[str]:
        return [o.name for o in self.outputs]

    @property
    def flops_per_pixel(self) -> int:
        k2, f = self.kernel_size ** 2, self.filters
        return 2 * k2 * self.n_in_channels * f + (self.depth - 2) * 2 * k2 * f * f + 2 * f * sum(o.nfeat for o in self.outputs)

    def validate(self):
        if self.activation not in ACTIVATIONS:
            raise ValueError(f"activation {self.activation!r} is not supported; supported: {sorted(ACTIVATIONS)} -- a model "
                             "must not run with another activation than it was saved with")
        if len(self.hidden_kernels) < 1:
            raise ValueError("depth must be at least 2: the reference's convolutional model takes its outputs from the last "
                             "hidden layer and fails without one (depth = 1)")
        if not self.inputs or not self.outputs:
            raise ValueError("a convolutional model needs at least one input and one output")
        if len(set(self.sources)) != len(self.inputs):
            raise ValueError(f"an input variable is named twice: {self.sources}")
        k0 = np.asarray(self.hidden_kernels[0])
        if k0.ndim != 4 or k0.shape[0] != k0.shape[1]:
            raise ValueError(f"hidden kernels must be [k, k, c_in, filters], got {k0.shape}")
        k, f = int(k0.shape[0]), int(k0.shape[3])
        if k % 2 == 0:
            raise ValueError("kernel_size must be odd")
        if f == 0:
            raise ValueError("filters=0 causes a floating point exception, and we haven't written a workaround")
        c_in = self.n_in_channels
        for l, w in enumerate(self.hidden_kernels):
            if tuple(np.asarray(w).shape) != (k, k, c_in, f):
                raise ValueError(f"hidden kernel {l} has shape {np.asarray(w).shape}, expected {(k, k, c_in, f)}")
            c_in = f
        if self.hidden_biases is not None:
            if len(self.hidden_biases) != len(self.hidden_kernels):
                raise ValueError("hidden_biases needs one array per hidden kernel (or None for no biases)")
            for l, b in enumerate(self.hidden_biases):
                if tuple(np.asarray(b).shape) != (f,):
                    raise ValueError(f"hidden bias {l} has shape {np.asarray(b).shape}, expected ({f},)")
        for i in self.inputs:
            if i.nfeat < 1 or np.asarray(i.center).shape != (i.nfeat,) or np.asarray(i.scale).shape != (i.nfeat,):
                raise ValueError(f"input {i.source!r}: center and scale must have shape ({i.nfeat},)")
        for o in self.outputs:
            if o.nfeat < 1 or np.asarray(o.kernel).shape != (f, o.nfeat):
                raise ValueError(f"output {o.name!r}: kernel has shape {np.asarray(o.kernel).shape}, expected {(f, o.nfeat)}")
            for a in (o.bias, o.scale, o.center):
                if np.asarray(a).shape != (o.nfeat,):
                    raise ValueError(f"output {o.name!r}: bias, scale and center must have shape ({o.nfeat},)")
        halos_required(k, self.depth)

    # -- serialisation: (yaml-able metadata, arrays for one npz) -------------------------------------
    def to_arrays(self):
        meta = {
            "activation": self.activation,
            "depth": self.depth,
            "kernel_size": self.kernel_size,
            "filters": self.filters,
            "hidden_bias": self.hidden_biases is not None,
            "inputs": [{"source": str(i.source), "nfeat": int(i.nfeat)} for i in self.inputs],
            "outputs": [{"name": str(o.name), "nfeat": int(o.nfeat)} for o in self.outputs],
        }
        arrays = {}
        for n, i in enumerate(self.inputs):
            arrays[f"in{n}_center"] = np.asarray(i.center, np.float32)
            arrays[f"in{n}_scale"] = np.asarray(i.scale, np.float32)
        for l, w in enumerate(self.hidden_kernels):
            arrays[f"hidden{l}_kernel"] = np.asarray(w, np.float32)
            if self.hidden_biases is not None:
                arrays[f"hidden{l}_bias"] = np.asarray(self.hidden_biases[l], np.float32)
        for n, o in enumerate(self.outputs):
            for key in ("kernel", "bias", "scale", "center"):
                arrays[f"out{n}_{key}"] = np.asarray(getattr(o, key), np.float32)
        return meta, arrays

    @classmethod
    def from_arrays(cls, meta: Mapping, arrays: Mapping[str, np.ndarray]) -> "ConvSpec":
        if meta.get("activation") not in ACTIVATIONS:
            raise ValueError(f"activation {meta.get('activation')!r} is not supported; supported: {sorted(ACTIVATIONS)}")
        n_hidden = int(meta["depth"]) - 1
        inputs = [ConvInput(i["source"], int(i["nfeat"]), np.asarray(arrays[f"in{n}_center"], np.float32),
                            np.asarray(arrays[f"in{n}_scale"], np.float32)) for n, i in enumerate(meta["inputs"])]
        kernels = [np.asarray(arrays[f"hidden{l}_kernel"], np.float32) for l in range(n_hidden)]
        biases = [np.asarray(arrays[f"hidden{l}_bias"], np.float32) for l in range(n_hidden)] if meta["hidden_bias"] else None
        outputs = [ConvOutput(o["name"], int(o["nfeat"]), *[np.asarray(arrays[f"out{n}_{key}"], np.float32)
                                                              for key in ("kernel", "bias", "scale", "center")])
                   for n, o in enumerate(meta["outputs"])]
        return cls(inputs, kernels, biases, outputs, activation=meta["activation"])


class ConvModel:
    """Device handle of a convolutional network (``fv3hip_conv_t``)."""

    def __init__(self, spec: ConvSpec, device="cuda"):
        spec.validate()
        self.spec = spec
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ConvModel needs a 'cuda' (ROCm) device; there is no CPU fallback")
        with torch.cuda.device(self.device):
            _require_device(torch.empty(1, device=self.device))
            self._handle = create_handle(spec)

    def predict(self, sources: Mapping[str, torch.Tensor], halo: str = "input", strips: Optional[torch.Tensor] = None,
                channels_last: bool = False) -> Dict[str, torch.Tensor]:
        """``sources``: name -> device array ``[..., z, y, x]`` (or ``[..., x, y, z]`` with ``channels_last``), float32 or
        float64, any strides, the leading dims alike for all.  A single-channel variable may omit ``z`` next to a multi-channel one
        (or when it is 2-D); otherwise it carries a ``z`` axis of length 1.  The arrays are read in place through their
        strides; the one exception: the kernel takes one batch stride, so an array whose leading dims cannot be merged into
        (batch, tile) as a view (two or more batch dims stored in another order) is copied once by ``reshape``.

        ``halo='input'``: the arrays carry the ``halos_required`` cells on every side; ``'cube'``: the last leading dim holds
        the six tiles and the halo is read from the neighbouring faces; ``'strips'``: ``strips`` ``[..., 4, h, C, n]`` holds
        it (side x-low, x-high, y-low, y-high; line 0 next to the tile; all input channels concatenated).
        Returns name -> float32 array in the layout of the inputs, without the halo."""
        if halo not in HALO_MODES:
            raise ValueError(f"halo must be one of {sorted(HALO_MODES)}, got {halo!r}")
        spec = self.spec
        h = spec.halos_required
        # the number of leading dims comes from a multi-channel source (its dims minus z, y, x); a single-channel source with
        # one dim fewer is then taken to omit z.  With single-channel sources only, one may omit z only if it is 2-D.
        n_lead = next((sources[i.source].dim() - 3 for i in spec.inputs if i.nfeat > 1), None)
        tensors, lead = [], None
        for i in spec.inputs:
            t = sources[i.source]
            if t.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"source {i.source!r} must be float32 or float64, got {t.dtype}")
            if i.nfeat == 1 and (t.dim() == n_lead + 2 if n_lead is not None else t.dim() == 2):
                t = t.unsqueeze(-1) if channels_last else t.unsqueeze(-3)
            if t.dim() < 3:
                raise ValueError(f"source {i.source!r} must be at least 3-D, got shape {tuple(t.shape)}")
            t = t if channels_last else t.permute(*range(t.dim() - 3), t.dim() - 1, t.dim() - 2, t.dim() - 3)  # [..., x, y, z]
            if t.shape[-1] != i.nfeat:
                raise ValueError(f"source {i.source!r} has {t.shape[-1]} channels, the network needs {i.nfeat}")
            if lead is None:
                lead, ext = tuple(t.shape[:-3]), tuple(t.shape[-3:-1])
            elif tuple(t.shape[:-3]) != lead or tuple(t.shape[-3:-1]) != ext:
                raise ValueError("sources differ in their leading or horizontal dims")
            tensors.append(t)
        dev = _require_device(*tensors)
        pad = 2 * h if halo == "input" else 0
        nx, ny = ext[0] - pad, ext[1] - pad
        if nx < 1 or ny < 1:
            raise ValueError(f"inputs of extent {ext} do not hold a halo of {h} cells")
        n_tiles = 1
        batch = lead
        if halo == "cube":
            if not lead or lead[-1] != 6:
                raise ValueError("halo='cube' needs the six tiles in the dim before [z, y, x]")
            n_tiles, batch = 6, lead[:-1]
        n_batch = int(np.prod(batch)) if batch else 1

        def five(t):  # (batch, tile, x, y, channel) element strides of a [*lead, x, y, z] view
            t = t.reshape((n_batch, n_tiles) + tuple(t.shape[-3:]))  # (a view where the leading dims merge, else a copy: see the docstring)
            return t, list(t.stride())

        views, strides = zip(*[five(t) for t in tensors])
        s_dtype = _lib.F32
        if halo == "strips" and h > 0:
            if strips is None:
                raise ValueError("halo='strips' needs the strips")
            want = lead + (4, h, spec.n_in_channels, nx)
            if tuple(strips.shape) != want or nx != ny:
                raise ValueError(f"strips have shape {tuple(strips.shape)}, expected {want} (square tiles)")
            if strips.dtype not in (torch.float32, torch.float64):
                raise TypeError("strips must be float32 or float64")
            strips = strips.contiguous()
            _require_device(strips)
            s_dtype = _lib.F64 if strips.dtype == torch.float64 else _lib.F32
        outs, oviews = {}, []
        for o in spec.outputs:
            shape = lead + ((nx, ny, o.nfeat) if channels_last else (o.nfeat, ny, nx))
            t = torch.empty(shape, dtype=torch.float32, device=dev)
            outs[o.name] = t
            v = t if channels_last else t.permute(*range(t.dim() - 3), t.dim() - 1, t.dim() - 2, t.dim() - 3)
            oviews.append(v.reshape((n_batch, n_tiles, nx, ny, o.nfeat)))
        for v, t in zip(oviews, outs.values()):
            assert v.data_ptr() == t.data_ptr()
        lib = _lib.load()
        nbytes = int(lib.fv3hip_conv_workspace_bytes(self._handle, n_batch, n_tiles, nx, ny))
        work = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=dev)
        n, k = len(views), len(oviews)
        _lib.call_on(dev, "fv3hip_conv_predict", self._handle,
                     (ctypes.c_void_p * n)(*[v.data_ptr() for v in views]),
                     (ctypes.c_int * n)(*[_lib.F64 if v.dtype == torch.float64 else _lib.F32 for v in views]),
                     (ctypes.c_int64 * (5 * n))(*[s for st in strides for s in st]),
                     n_batch, n_tiles, nx, ny, HALO_MODES[halo], strips.data_ptr() if (halo == "strips" and h > 0) else None,
                     s_dtype, (ctypes.c_void_p * k)(*[v.data_ptr() for v in oviews]),
                     (ctypes.c_int64 * (5 * k))(*[s for v in oviews for s in v.stride()]),
                     work.data_ptr(), nbytes, _stream(dev))
        return outs

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            try:
                _lib.load().fv3hip_conv_destroy(h)
            except Exception:
                pass


def create_handle(spec: ConvSpec):
    """``fv3hip_conv_create`` on the current device (the library validates the arrays before any HIP call)."""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    nfeat = np.asarray([i.nfeat for i in spec.inputs], np.intc)
    center = f32(np.concatenate([np.asarray(i.center, np.float32) for i in spec.inputs]))
    scale = f32(np.concatenate([np.asarray(i.scale, np.float32) for i in spec.inputs]))
    kernels = [f32(w) for w in spec.hidden_kernels]
    biases = None if spec.hidden_biases is None else [f32(b) for b in spec.hidden_biases]
    onf = np.asarray([o.nfeat for o in spec.outputs], np.intc)
    cat = lambda key: f32(np.concatenate([np.asarray(getattr(o, key), np.float32) for o in spec.outputs], axis=-1))
    ok, ob, os_, oc = cat("kernel"), cat("bias"), cat("scale"), cat("center")

    def ptr(a, ct=ctypes.c_float):
        return a.ctypes.data_as(ctypes.POINTER(ct))

    fp = ctypes.POINTER(ctypes.c_float)
    d = _lib.ConvDesc()
    d.n_inputs = len(spec.inputs)
    d.in_nfeat = ptr(nfeat, ctypes.c_int)
    d.in_center = ptr(center)
    d.in_scale = ptr(scale)
    d.n_hidden = len(kernels)
    d.kernel_size = spec.kernel_size
    d.filters = spec.filters
    d.activation = ACTIVATIONS[spec.activation]
    d.hidden_kernels = (fp * len(kernels))(*[ptr(w) for w in kernels])
    d.hidden_biases = None if biases is None else (fp * len(biases))(*[ptr(b) for b in biases])
    d.n_outputs = len(spec.outputs)
    d.out_nfeat = ptr(onf, ctypes.c_int)
    d.out_kernel = ptr(ok)
    d.out_bias = ptr(ob)
    d.out_scale = ptr(os_)
    d.out_center = ptr(oc)
    handle = ctypes.c_void_p()
    _lib.call("fv3hip_conv_create", ctypes.byref(d), ctypes.byref(handle))
    return handle
