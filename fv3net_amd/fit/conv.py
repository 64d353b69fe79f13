"""The convolutional predictor: ``fv3fit``'s ``"convolutional"`` training function returns a ``PureKerasModel`` with
``unstacked_dims=("x", "y", "z")`` and ``n_halo = halos_required`` (external/fv3fit/fv3fit/keras/_models/convolutional.py:141-149);
``predict_on_dataset`` pads every tile with halos from its neighbours before the network runs
(_shared/xr_prediction.py:120-129).  ``HipConvolutionalModel`` is that predictor on the MI355X: the network runs in
``fv3hip_conv_predict``, which reads the dataset's arrays in place and takes the halo cells from the neighbouring faces of a
resident cube, or -- with the cube sharded by tile over ``torch.distributed`` ranks -- from strips exchanged in one
all-gather (``parallel.exchange_edge_strips``).  Training stays offline; the artifact is ``name`` ("hip-convolutional") +
``config.yaml`` (the reference's four keys) + ``spec.yaml`` + ``weights.npz``.
"""
import os
from typing import Hashable, Iterable, Optional, Sequence

import numpy as np
import torch
import yaml

from ..conv import ConvInput, ConvModel, ConvOutput, ConvSpec
from ..cubedsphere._device import compute_device, download_all, on_device
from ..xr_compat import DataArray, Dataset, from_compat, to_compat
from . import io
from .predictor import Predictor
from .stacking import match_prediction_to_input_coords


@io.register("hip-convolutional")
class HipConvolutionalModel(Predictor):
    """Convolutional network over ``[x, y, z]`` fields with cube halos, running on the MI355X."""

    _CONFIG_FILENAME = "config.yaml"
    _SPEC_FILENAME = "spec.yaml"
    _WEIGHTS_FILENAME = "weights.npz"

    def __init__(self, input_variables: Iterable[Hashable], output_variables: Iterable[Hashable], model: ConvSpec,
                 unstacked_dims: Sequence[str] = ("x", "y", "z"), n_halo: Optional[int] = None):
        super().__init__(list(input_variables), list(output_variables))
        self.spec = model
        if n_halo is not None and int(n_halo) != model.halos_required:
            raise ValueError(f"n_halo = {n_halo}, but a network of depth {model.depth} with {model.kernel_size} x "
                             f"{model.kernel_size} kernels needs {model.halos_required} halo cells")
        self._n_halo = model.halos_required
        self._unstacked_dims = list(unstacked_dims)
        if len(self._unstacked_dims) != 3:
            raise ValueError(f"a convolutional model's unstacked_dims are (x, y, z), got {self._unstacked_dims}")
        if list(model.sources) != [str(v) for v in self.input_variables]:
            raise ValueError(f"input variables {self.input_variables} differ from the network's inputs {model.sources}")
        missing = [v for v in self.output_variables if v not in model.output_names]
        if missing:
            raise ValueError(f"output variables {missing} are not produced by the network ({model.output_names})")
        self._model: Optional[ConvModel] = None  # created on first predict (needs the GPU)

    @property
    def n_halo(self) -> int:
        return self._n_halo

    @property
    def model(self) -> ConvModel:
        if self._model is None:
            self._model = ConvModel(self.spec, device=compute_device())
        return self._model

    # -- prediction -------------------------------------------------------------------------
    def _halo_route(self, n_tile_dim: Optional[int], tile_coord):
        """('input' | 'cube' | 'exchange', this rank's tiles): where the halo cells come from."""
        from ..parallel import tiles_of_rank, world

        if self._n_halo == 0:
            return "input", None
        rank, size = world()
        if n_tile_dim is None:
            if size == 6:
                return "exchange", [rank]
            if size > 6 and size % 6 == 0:
                raise ValueError(f"{size} ranks: a tile split over several ranks (layout > 1) is out of scope of this "
                                 "predictor; run one rank per tile or give the whole cube")
            raise ValueError("either dataset must have tile dimension or MPI must be present")
        mine = list(range(6)) if (size == 1 or n_tile_dim == 6) else tiles_of_rank(size, rank)
        if n_tile_dim != len(mine) or not mine:
            raise ValueError(f"dataset must have exactly six tiles to append halos (or, sharded by tile, this rank's tiles "
                             f"{mine}), got {n_tile_dim}")
        if tile_coord is not None and np.asarray(tile_coord).tolist() != mine:
            raise ValueError(f"`tile` coordinate must be {mine}, in this order")
        return ("cube" if len(mine) == 6 else "exchange"), mine

    def predict(self, X):
        """Predict an output dataset from an input dataset whose variables have ``x`` and ``y`` (and, unless single-level,
        ``z``) dimensions, a ``tile`` dimension unless every rank holds one tile, and any batch dimensions, in any order.
        Does not mutate ``X``; host data in, host data out; device data in, device data out."""
        from ..cubedsphere.halos import edge_strips, halo_strips
        from ..parallel import exchange_edge_strips

        x = to_compat(X)
        xd, yd, zd = self._unstacked_dims
        arrays = {name: x[name] for name in self.input_variables}  # KeyError for a missing variable
        batch, sizes = [], {}
        for name, da in arrays.items():
            for dim in (xd, yd):
                if dim not in da.dims:
                    raise ValueError(f"variable {name!r} has no {dim!r} dimension")
            for dim, n in da.sizes.items():
                if sizes.setdefault(dim, n) != n:
                    raise ValueError(f"conflicting sizes for dimension {dim!r}")
                if dim not in (xd, yd, zd, "tile") and dim not in batch:
                    batch.append(dim)
        has_tile = "tile" in sizes
        route, mine = self._halo_route(sizes.get("tile"), x.coords.get("tile") if has_tile else None)
        lead = batch + (["tile"] if has_tile else [])
        host_input, sources = None, {}
        for i, (name, da) in zip(self.spec.inputs, arrays.items()):
            if set(da.dims) - {zd} != set(lead) | {xd, yd}:
                raise ValueError(f"variable {name!r} has dims {da.dims}, expected {lead + [xd, yd]} (and {zd!r})")
            if host_input is None:
                host_input = da.data
            t = on_device(da.data)
            names = list(da.dims)
            if zd not in names:
                t, names = t.unsqueeze(0), [zd] + names
            t = t.permute(*[names.index(dim) for dim in lead + [zd, yd, xd]])  # a view: the kernel reads through strides
            if route == "exchange" and not has_tile:
                t = t.unsqueeze(-4)
            sources[i.source] = t
        if route == "exchange":  # the one exchange step: the edge strips of this rank's tiles against everybody's
            h, nb = self._n_halo, len(batch)
            ts = list(sources.values())
            if any(t.dtype != ts[0].dtype for t in ts):
                ts = [t.to(torch.float64) for t in ts]
            # [batch.., tile, z, y, x] -> [tile, batch.., z, x, y] -> edges [tile, 4, h, batch.., z, n]
            edges = torch.cat([edge_strips(t.movedim(nb, 0).transpose(-1, -2), h) for t in ts], dim=-2)
            table = exchange_edge_strips(edges.contiguous())
            strips = halo_strips(table, mine)                                   # [tile, 4, h, batch.., C, n]
            strips = strips.permute(*range(3, 3 + nb), 0, 1, 2, 3 + nb, 4 + nb)   # [batch.., tile, 4, h, C, n]
            outs = self.model.predict(sources, halo="strips", strips=strips)
        else:
            outs = self.model.predict(sources, halo=route)

        shaped, dims_of = {}, {}
        nfeat = {o.name: o.nfeat for o in self.spec.outputs}
        for name in self.output_variables:
            t = outs[str(name)]
            if route == "exchange" and not has_tile:
                t = t.squeeze(-4)
            if nfeat[str(name)] == 1:
                shaped[name], dims_of[name] = t.squeeze(-3), tuple(lead + [yd, xd])
            else:
                shaped[name], dims_of[name] = t, tuple(lead + [zd, yd, xd])
        if not (isinstance(host_input, torch.Tensor) and host_input.is_cuda):
            shaped = download_all(shaped)  # host data in -> host data out, one copy for all outputs
        result = Dataset()
        for name in self.output_variables:
            result[name] = DataArray(shaped[name], dims=dims_of[name])
        return from_compat(match_prediction_to_input_coords(x, result), X)

    # -- serialisation ----------------------------------------------------------------------
    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        meta, arrays = self.spec.to_arrays()
        np.savez(os.path.join(path, self._WEIGHTS_FILENAME), **arrays)
        with open(os.path.join(path, self._SPEC_FILENAME), "w") as f:
            yaml.safe_dump(meta, f)
        with open(os.path.join(path, self._CONFIG_FILENAME), "w") as f:
            yaml.safe_dump(
                {"input_variables": list(self.input_variables), "output_variables": list(self.output_variables),
                 "unstacked_dims": list(self._unstacked_dims), "n_halo": self._n_halo}, f)

    @classmethod
    def load(cls, path: str) -> "HipConvolutionalModel":
        with open(os.path.join(path, cls._CONFIG_FILENAME)) as f:
            config = yaml.safe_load(f)
        with open(os.path.join(path, cls._SPEC_FILENAME)) as f:
            meta = yaml.safe_load(f)
        with np.load(os.path.join(path, cls._WEIGHTS_FILENAME), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        return cls(config["input_variables"], config["output_variables"], ConvSpec.from_arrays(meta, arrays),
                   unstacked_dims=config.get("unstacked_dims", ("x", "y", "z")), n_halo=config.get("n_halo"))


def conv_spec_from_arrays(
    input_variables: Sequence[str],
    input_means: Sequence[np.ndarray],
    input_stds: Sequence[np.ndarray],
    hidden_kernels: Sequence[np.ndarray],
    hidden_biases: Optional[Sequence[np.ndarray]],
    output_variables: Sequence[str],
    output_kernels: Sequence[np.ndarray],
    output_biases: Sequence[np.ndarray],
    output_means: Sequence[np.ndarray],
    output_stds: Sequence[np.ndarray],
    activation: str = "relu",
    epsilon: float = 1e-7,
) -> ConvSpec:
    """Assemble the predict graph of convolutional.py:153-210 from its weights, Keras layouts: hidden kernels
    ``[k, k, c_in, filters]``, head kernels ``[1, 1, filters, z]`` (or ``[filters, z]``).  ``input_stds`` are the fitted standard
    deviations; the forward scale is ``std + epsilon`` in float32.  ``hidden_biases=None``: a network without them."""
    inputs = []
    for name, mean, std in zip(input_variables, input_means, input_stds):
        mean, std = np.atleast_1d(np.asarray(mean, np.float32)), np.atleast_1d(np.asarray(std, np.float32))
        inputs.append(ConvInput(str(name), int(mean.shape[0]), mean, std + np.float32(epsilon)))
    outputs = []
    for name, kern, bias, mean, std in zip(output_variables, output_kernels, output_biases, output_means, output_stds):
        kern = np.asarray(kern, np.float32)
        kern = kern.reshape(kern.shape[-2:])
        nf = int(kern.shape[1])
        outputs.append(ConvOutput(str(name), nf, kern, np.asarray(bias, np.float32).reshape(nf),
                                  np.broadcast_to(np.asarray(std, np.float32), (nf,)).copy(),
                                  np.broadcast_to(np.asarray(mean, np.float32), (nf,)).copy()))
    return ConvSpec(inputs, [np.asarray(k, np.float32) for k in hidden_kernels],
                    None if hidden_biases is None else [np.asarray(b, np.float32) for b in hidden_biases], outputs,
                    activation=activation)
