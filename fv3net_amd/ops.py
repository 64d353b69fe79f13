"""Array-level entry points: torch device tensors in, torch device tensors out.

Every function here is a thin shape/dtype check around one C-ABI call into ``libfv3hip.so``
(``include/fv3hip.h``), enqueued on torch's current HIP stream.  PyTorch only supplies device
memory and the stream; no torch kernel does any of the arithmetic.  There is no CPU path:
tensors must live on a ``cuda`` (ROCm) device.
"""
import ctypes
import dataclasses
import os
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

_DTYPE_CODE = {
    torch.float32: _lib.F32,
    torch.float64: _lib.F64,
    torch.int32: _lib.I32,
    torch.int64: _lib.I64,
}

_OPS = {
    "sum": _lib.OP_SUM,
    "mean": _lib.OP_MEAN,
    "min": _lib.OP_MIN,
    "max": _lib.OP_MAX,
    "median": _lib.OP_MEDIAN,
    "mode": _lib.OP_MODE,
}

_initialised_devices = set()


def _require_device(*tensors):
    dev = None
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(t)}")
        if not t.is_cuda:
            raise RuntimeError(
                "fv3net_amd.ops works on device tensors only (there is no CPU fallback); "
                "move the input to a 'cuda' (ROCm) device first"
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors live on different devices: {dev} and {t.device}")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _initialised_devices:
        _lib.call("fv3hip_init", idx)
        _initialised_devices.add(idx)
    return dev


def _code(t: torch.Tensor) -> int:
    try:
        return _DTYPE_CODE[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}") from None


def _float_code(t: torch.Tensor) -> int:
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"expected float32 or float64, got {t.dtype}")
    return _DTYPE_CODE[t.dtype]


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


try:  # the raw handle of torch's current stream without building a Stream object (several microseconds per launch)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover
    _raw_stream = None


def _stream(dev) -> ctypes.c_void_p:
    if _raw_stream is not None:
        idx = None if dev is None else torch.device(dev).index
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device() if idx is None else idx))
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _prod(xs) -> int:
    return int(math.prod(int(x) for x in xs))


def _weights_repeat(obj: torch.Tensor, weights: torch.Tensor):
    """Return (weights_contiguous, w_repeat) such that weight slice ``o // w_repeat`` applies to
    outer slice ``o`` of ``obj`` (both viewed as [n_outer, ny, nx])."""
    if weights.shape[-2:] != obj.shape[-2:]:
        raise ValueError(
            f"horizontal shape of weights {tuple(weights.shape[-2:])} does not match "
            f"the field's {tuple(obj.shape[-2:])}"
        )
    o_outer, w_outer = tuple(obj.shape[:-2]), tuple(weights.shape[:-2])
    if w_outer == o_outer:
        return weights.contiguous(), 1
    # weights' outer dims are a prefix of the field's: shared by the trailing outer dims
    if len(w_outer) <= len(o_outer) and o_outer[: len(w_outer)] == w_outer:
        return weights.contiguous(), max(_prod(o_outer[len(w_outer):]), 1)
    # anything else: materialise the broadcast (numpy broadcasting rules)
    expanded = torch.broadcast_to(weights, obj.shape).contiguous()
    return expanded, 1


def _promoted(a: torch.Tensor, b: torch.Tensor) -> torch.dtype:
    return torch.float64 if torch.float64 in (a.dtype, b.dtype) else torch.float32


def _weighted_operands(obj: torch.Tensor, weights: torch.Tensor, factor: Optional[int] = None):
    """What the weighted averages of a contiguous ``obj`` [.., ny, nx] hand to the library: (weights made contiguous,
    w_repeat, n_outer, ny, nx) and, given a block ``factor`` (checked here), the shape of the block means as well."""
    weights, w_repeat = _weights_repeat(obj, weights)
    ny, nx = int(obj.shape[-2]), int(obj.shape[-1])
    operands = (weights, w_repeat, _prod(obj.shape[:-2]), ny, nx)
    if factor is None:
        return operands
    if factor < 1 or ny % factor or nx % factor:
        raise ValueError(f"horizontal extents ({ny}, {nx}) are not multiples of the coarsening factor {factor}")
    return operands + (tuple(obj.shape[:-2]) + (ny // factor, nx // factor),)


def weighted_block_average(obj: torch.Tensor, weights: torch.Tensor, factor: int) -> torch.Tensor:
    """``nansum(obj*w)/nansum(w)`` over factor x factor blocks of the last two dims
    (vcm.cubedsphere.weighted_block_average, coarsen.py:183-218)."""
    dev = _require_device(obj, weights)
    factor = int(factor)
    if obj.dim() < 2:
        raise ValueError("field must have at least two (horizontal) dimensions")
    obj = obj.contiguous()
    weights, w_repeat, n_outer, ny, nx, oshape = _weighted_operands(obj, weights, factor)
    out = torch.empty(oshape, dtype=_promoted(obj, weights), device=dev)
    _lib.call_on(dev,
        "fv3hip_weighted_block_average", _ptr(obj), _float_code(obj), _ptr(weights), _float_code(weights),
        n_outer, ny, nx, w_repeat, factor, _ptr(out), _stream(dev),
    )
    return out


def weighted_block_average_multi(fields: Sequence[torch.Tensor], weights: torch.Tensor, factor: int) -> list:
    """``weighted_block_average(field, weights, factor)`` for several fields of one shape and dtype that share their weights
    (2-D, or the fields' shape): four fields per launch read the weights once.  Same results as the single-field call when
    fields and weights have one dtype (the surface-data arithmetic does)."""
    fields = [f.contiguous() for f in fields]
    if not fields:
        return []
    f0 = fields[0]
    if len(fields) == 1 or any(f.shape != f0.shape or f.dtype != f0.dtype for f in fields) or weights.dtype != f0.dtype:
        return [weighted_block_average(f, weights, factor) for f in fields]
    dev = _require_device(weights, *fields)
    factor = int(factor)
    w, w_repeat, n_outer, ny, nx, oshape = _weighted_operands(f0, weights, factor)
    outs = [torch.empty(oshape, dtype=f0.dtype, device=dev) for _ in fields]
    try:
        _lib.call_on(dev, "fv3hip_mass_weighted_block_average", _ptr_array(fields), len(fields), _float_code(f0), None, _ptr(w),
                     _float_code(w), n_outer, ny, nx, w_repeat, factor, _ptr_array(outs), _stream(dev))
    except _lib.Fv3HipError as err:
        if err.code != _lib.EUNSUPPORTED:
            raise
        return [weighted_block_average(f, weights, factor) for f in fields]
    return outs


def mass_weighted_block_average(fields: Sequence[torch.Tensor], delp: torch.Tensor, area: torch.Tensor, factor: int) -> list:
    """``weighted_block_average(field, delp * area, factor)`` for several fields that share ``delp`` [.., ny, nx] (the
    fields' shape and dtype) and ``area`` (2-D weights shared by trailing outer dims, as in ``weighted_block_average``): the
    product is formed in registers and read once per four fields (coarsen_restarts.py:335-427, 856-900).  Falls back to the
    product + ``weighted_block_average`` kernels for shapes the fused kernel does not take."""
    fields = [f.contiguous() for f in fields]
    if not fields:
        return []
    dev = _require_device(delp, area, *fields)
    factor = int(factor)
    f0 = fields[0]
    if any(f.shape != f0.shape or f.dtype != f0.dtype for f in fields) or delp.shape != f0.shape:
        raise ValueError("fields and delp must share one shape and dtype")
    delp = cast(delp, f0.dtype).contiguous()
    area_b, a_repeat, n_outer, ny, nx, oshape = _weighted_operands(f0, area, factor)
    out_dtype = _promoted(f0, area_b)
    outs = [torch.empty(oshape, dtype=out_dtype, device=dev) for _ in fields]
    try:
        _lib.call_on(dev, "fv3hip_mass_weighted_block_average", _ptr_array(fields), len(fields), _float_code(f0), _ptr(delp),
                     _ptr(area_b), _float_code(area_b), n_outer, ny, nx, a_repeat, factor, _ptr_array(outs), _stream(dev))
    except _lib.Fv3HipError as err:
        if err.code != _lib.EUNSUPPORTED:
            raise
        # the same result from the product kernel and the single-field average
        lead = area_b.dim() - 2
        if a_repeat > 1:
            w = ew("mul", delp.reshape(tuple(delp.shape[:lead]) + (-1, ny, nx)), area_b).reshape(delp.shape)
        else:
            w = ew("mul", delp, area_b)
        if w.dtype != out_dtype:
            w = w.to(out_dtype)
        return [weighted_block_average(f, w, factor) for f in fields]
    return outs


def edge_weighted_block_average(
    obj: torch.Tensor, spacing: torch.Tensor, factor: int, edge: str = "x"
) -> torch.Tensor:
    """Weighted mean over ``factor`` cells along one horizontal dim, every factor-th line kept
    along the other (vcm.cubedsphere.edge_weighted_block_average, coarsen.py:221-273).
    The last two dims are (y, x)."""
    if edge not in ("x", "y"):
        raise ValueError(f"'edge' most be either 'x' or 'y'; got {edge}.")
    dev = _require_device(obj, spacing)
    factor = int(factor)
    obj = obj.contiguous()
    spacing, w_repeat, n_outer, ny, nx = _weighted_operands(obj, spacing)
    if edge == "x":
        if nx % factor:
            raise ValueError(f"x extent {nx} is not a multiple of the coarsening factor {factor}")
        oshape = (-(-ny // factor), nx // factor)
    else:
        if ny % factor:
            raise ValueError(f"y extent {ny} is not a multiple of the coarsening factor {factor}")
        oshape = (ny // factor, -(-nx // factor))
    out = torch.empty(tuple(obj.shape[:-2]) + oshape, dtype=_promoted(obj, spacing), device=dev)
    _lib.call_on(dev,
        "fv3hip_edge_weighted_block_average", _ptr(obj), _float_code(obj), _ptr(spacing),
        _float_code(spacing), n_outer, ny, nx, w_repeat, factor, 0 if edge == "x" else 1,
        _ptr(out), _stream(dev),
    )
    return out


def weighted_window_average(obj: torch.Tensor, weights: torch.Tensor, window: Sequence[int], stride: Sequence[int]) -> torch.Tensor:
    """``sum(obj * weights) / sum(weights)`` over windows (by, bx) every (sy, sx) cells of the last two dims -- the general
    form of ``weighted_block_average`` (f, f / f, f) and ``edge_weighted_block_average`` ('x': (1, f) / (f, f)); on fields
    already reduced to the lines the edge-weighted mean keeps: (1, f) / (1, f)."""
    dev = _require_device(obj, weights)
    by, bx = (int(v) for v in window)
    sy, sx = (int(v) for v in stride)
    obj = obj.contiguous()
    weights, w_repeat, n_outer, ny, nx = _weighted_operands(obj, weights)
    if ny < by or nx < bx:
        raise ValueError(f"window ({by}, {bx}) is larger than the field ({ny}, {nx})")
    out = torch.empty(tuple(obj.shape[:-2]) + ((ny - by) // sy + 1, (nx - bx) // sx + 1), dtype=_promoted(obj, weights), device=dev)
    _lib.call_on(dev, "fv3hip_weighted_window_average", _ptr(obj), _float_code(obj), _ptr(weights), _float_code(weights),
                 n_outer, ny, nx, w_repeat, by, bx, sy, sx, _ptr(out), _stream(dev))
    return out


def take_lines(x: torch.Tensor, step: int, axis: int) -> torch.Tensor:
    """Every ``step``-th line of the last (``axis`` = 0, x) or second-to-last (``axis`` = 1, y) dim, starting with the
    first: ``x.isel(dim=slice(None, None, step))`` as a device gather (coarsen.py:265-271 keeps these lines)."""
    window, stride = (1, 1), ((1, int(step)) if axis == 0 else (int(step), 1))
    return block_reduce(x, window, stride, op="max", nan_policy="propagate")


def repeat(x: torch.Tensor, fy: int, fx: int) -> torch.Tensor:
    """Repeat each value ``fy`` times along the second-to-last and ``fx`` times along the last dim
    (``xarray_utils.repeat``, vcm/xarray_utils.py:37-82, a count per horizontal dim)."""
    fy, fx = int(fy), int(fx)
    return _upsampled(x, "fv3hip_repeat", lambda ny, nx: (ny * fy, nx * fx), fy, fx)


def _upsampled(x: torch.Tensor, entry: str, out_hw, *factors) -> torch.Tensor:
    """``repeat`` and ``block_upsample``: words of 4 or 8 bytes copied by ``entry`` to a fresh [.., *out_hw(ny, nx)] tensor."""
    dev = _require_device(x)
    x = x.contiguous()
    if x.element_size() not in (4, 8):
        raise TypeError(f"unsupported dtype {x.dtype}")
    ny, nx = int(x.shape[-2]), int(x.shape[-1])
    out = torch.empty(tuple(x.shape[:-2]) + out_hw(ny, nx), dtype=x.dtype, device=dev)
    _lib.call_on(dev, entry, _ptr(x), x.element_size(), _prod(x.shape[:-2]), ny, nx, *factors, _ptr(out), _stream(dev))
    return out


def block_reduce(
    x: torch.Tensor,
    window: Sequence[int],
    stride: Optional[Sequence[int]] = None,
    op: str = "sum",
    nan_policy: str = "skip",
) -> torch.Tensor:
    """Windowed reduction over the last two dims: window (by, bx), stride (sy, sx) (default =
    window).  ops: sum, mean, min, max (NaN-skipping like xarray's coarsen), median (numpy.median),
    mode (scipy.stats.mode 1.7.3, ``nan_policy`` 'propagate' or 'omit')."""
    dev = _require_device(x)
    by, bx = (int(v) for v in window)
    sy, sx = (by, bx) if stride is None else (int(v) for v in stride)
    if op not in _OPS:
        raise ValueError(f"unknown block reduction {op!r}")
    policy = {"skip": _lib.NAN_SKIP, "propagate": _lib.NAN_PROPAGATE, "omit": _lib.NAN_OMIT}[nan_policy]
    x = x.contiguous()
    ny, nx = int(x.shape[-2]), int(x.shape[-1])
    if ny < by or nx < bx:
        raise ValueError(f"window ({by}, {bx}) is larger than the field ({ny}, {nx})")
    nyo, nxo = (ny - by) // sy + 1, (nx - bx) // sx + 1
    out = torch.empty(tuple(x.shape[:-2]) + (nyo, nxo), dtype=x.dtype, device=dev)
    _lib.call_on(dev,
        "fv3hip_block_reduce", _ptr(x), _code(x), _prod(x.shape[:-2]), ny, nx, by, bx, sy, sx, _OPS[op],
        policy, _ptr(out), _stream(dev),
    )
    return out


def block_upsample(x: torch.Tensor, factor: int) -> torch.Tensor:
    """Repeat each value ``factor`` times along the last two dims; a dim of odd size is treated
    as staggered and its last point is not repeated (coarsen.py:843-897)."""
    factor = int(factor)
    size = lambda n: (n - 1) * factor + 1 if n % 2 == 1 else n * factor
    return _upsampled(x, "fv3hip_block_upsample", lambda ny, nx: (size(ny), size(nx)), factor)


def _column_view(x: torch.Tensor, z_axis: int):
    z_axis = z_axis % x.dim()
    return z_axis, _prod(x.shape[:z_axis]), int(x.shape[z_axis]), _prod(x.shape[z_axis + 1:])


def column_sum(x: torch.Tensor, z_axis: int, addend: float = 0.0) -> torch.Tensor:
    """``x.sum(z_axis) + addend`` (surface_pressure_from_delp, vertically_dependent.py:189-208)."""
    dev = _require_device(x)
    code = _float_code(x)
    x = x.contiguous()
    z_axis, nb, nz, ni = _column_view(x, z_axis)
    out = torch.empty(tuple(x.shape[:z_axis]) + tuple(x.shape[z_axis + 1:]), dtype=x.dtype, device=dev)
    _lib.call_on(dev, "fv3hip_column_sum", _ptr(x), code, nb, nz, ni, float(addend), _ptr(out), _stream(dev))
    return out


def blend_weights(blending_pressure: torch.Tensor, ps_coarse: torch.Tensor, pfull_coarse: torch.Tensor, z_axis: int) -> torch.Tensor:
    """``(ps - p) / (ps - pb)`` where ``p > pb`` else 1 (coarsen_restarts.py:559-576); ``pfull_coarse`` has
    the z axis, the other two the same shape without it."""
    dev = _require_device(blending_pressure, ps_coarse, pfull_coarse)
    code = _float_code(pfull_coarse)
    p = pfull_coarse.contiguous()
    z_axis, nb, nz, ni = _column_view(p, z_axis)
    pb, ps = blending_pressure.to(p.dtype).contiguous(), ps_coarse.to(p.dtype).contiguous()
    want = tuple(p.shape[:z_axis]) + tuple(p.shape[z_axis + 1:])
    if tuple(pb.shape) != want or tuple(ps.shape) != want:
        raise ValueError(f"blending and surface pressures must have shape {want}")
    out = torch.empty_like(p)
    _lib.call_on(dev, "fv3hip_blend_weights", _ptr(pb), _ptr(ps), _ptr(p), code, nb, nz, ni, _ptr(out), _stream(dev))
    return out


def hydrostatic_balance(dz: torch.Tensor, phis: torch.Tensor, t: torch.Tensor, q: torch.Tensor, delp: torch.Tensor,
                        toa_pressure: float, z_axis: int):
    """Hydrostatic layer thicknesses and the surface geopotential that keeps the model-top height
    (coarsen_restarts.py:990-1017).  Returns (dz, phis)."""
    dev = _require_device(dz, phis, t, q, delp)
    dt = torch.float64 if any(a.dtype == torch.float64 for a in (dz, phis, t, q, delp)) else torch.float32
    dz, phis, t, q, delp = (a.to(dt).contiguous() for a in (dz, phis, t, q, delp))
    z_axis, nb, nz, ni = _column_view(dz, z_axis)
    for a in (t, q, delp):
        if tuple(a.shape) != tuple(dz.shape):
            raise ValueError("DZ, T, sphum and delp must have the same shape")
    if tuple(phis.shape) != tuple(dz.shape[:z_axis]) + tuple(dz.shape[z_axis + 1:]):
        raise ValueError("phis must have DZ's shape without the vertical axis")
    dz_out, phis_out = torch.empty_like(dz), torch.empty_like(phis)
    _lib.call_on(dev, "fv3hip_hydrostatic_balance", _ptr(dz), _ptr(phis), _ptr(t), _ptr(q), _ptr(delp), _DTYPE_CODE[dt], nb, nz, ni,
              float(toa_pressure), _ptr(dz_out), _ptr(phis_out), _stream(dev))
    return dz_out, phis_out


def level_scale(x: torch.Tensor, scale: torch.Tensor, z_axis: int) -> torch.Tensor:
    """``scale[z] * x`` along ``z_axis`` in float64 (TaperConfig.apply, _shared/config.py:11-24)."""
    dev = _require_device(x, scale)
    code = _float_code(x)
    x = x.contiguous()
    z_axis, nb, nz, ni = _column_view(x, z_axis)
    scale = scale.to(torch.float64).contiguous()
    if tuple(scale.shape) != (nz,):
        raise ValueError(f"scale must have shape ({nz},), got {tuple(scale.shape)}")
    out = torch.empty(x.shape, dtype=torch.float64, device=dev)
    _lib.call_on(dev, "fv3hip_level_scale", _ptr(x), code, _ptr(scale), nb, nz, ni, _ptr(out), _stream(dev))
    return out


def _flux_operands(arrays, surface, z_axis: int):
    """Column arrays and [columns-without-z] surface arrays in one float dtype (numpy's promotion), contiguous."""
    dt = torch.float64 if any(t is not None and t.dtype == torch.float64 for t in list(arrays) + list(surface)) else torch.float32
    arrays = [cast(t, dt).contiguous() for t in arrays]
    shape = tuple(arrays[0].shape)
    for t in arrays[1:]:
        if tuple(t.shape) != shape:
            raise ValueError(f"column arrays differ in shape: {tuple(t.shape)} and {shape}")
    z_axis, nb, nz, ni = _column_view(arrays[0], z_axis)
    flat = shape[:z_axis] + shape[z_axis + 1:]
    out_surface = []
    for t in surface:
        if t is not None:
            t = cast(t, dt).contiguous()
            if tuple(t.shape) != flat:
                raise ValueError(f"surface array has shape {tuple(t.shape)}, the columns have {flat}")
        out_surface.append(t)
    return dt, arrays, out_surface, (nb, nz, ni), flat


def tendency_to_flux(tendency: torch.Tensor, delp: torch.Tensor, toa_net_flux: Optional[torch.Tensor],
                     surface_upward_flux: torch.Tensor, z_axis: int, rectify: bool = True, closure_only: bool = False):
    """``vcm.calc.flux_form._tendency_to_flux`` (flux_form.py:7-46): (net flux at the interface above each cell, surface
    downward flux); ``closure_only``: ``_tendency_to_implied_surface_downward_flux`` (:49-75), (None, downward flux)."""
    dev = _require_device(tendency, delp, surface_upward_flux)
    dt, (tend, dp), (toa, up), (nb, nz, ni), flat = _flux_operands([tendency, delp], [toa_net_flux, surface_upward_flux], z_axis)
    flux = None if closure_only else torch.empty_like(tend)
    down = torch.empty(flat, dtype=dt, device=dev)
    _lib.call_on(dev, "fv3hip_tendency_to_flux", _ptr(tend), _ptr(dp), _ptr(toa), _ptr(up), _float_code(tend), nb, nz, ni,
                 int(bool(rectify)), int(bool(closure_only)), _ptr(flux), _ptr(down), _stream(dev))
    return flux, down


def flux_to_tendency(net_flux: torch.Tensor, surface_downward_flux: torch.Tensor, surface_upward_flux: torch.Tensor,
                     delp: torch.Tensor, z_axis: int) -> torch.Tensor:
    """``vcm.calc.flux_form._flux_to_tendency`` (flux_form.py:78-104)."""
    dev = _require_device(net_flux, delp)
    dt, (flux, dp), (down, up), (nb, nz, ni), _ = _flux_operands([net_flux, delp], [surface_downward_flux, surface_upward_flux], z_axis)
    out = torch.empty_like(flux)
    _lib.call_on(dev, "fv3hip_flux_to_tendency", _ptr(flux), _ptr(down), _ptr(up), _ptr(dp), _float_code(flux), nb, nz, ni, _ptr(out),
                 _stream(dev))
    return out


def minmax_score(variables: Sequence[torch.Tensor], scales: Sequence[torch.Tensor], offsets: Sequence[torch.Tensor]) -> torch.Tensor:
    """MinMaxNoveltyDetector's score (fv3fit/sklearn/_min_max_novelty_detector.py:94-121) of ``[feature, sample]`` arrays
    (any strides) scaled as ``MinMaxScaler.transform`` does: ``max(max_f - 1, 0) + max(-min_f, 0)``, float64 ``[sample]``."""
    if len(variables) == 0:  # (no launch would ever write the score)
        raise ValueError("minmax_score needs at least one variable")
    if not len(variables) == len(scales) == len(offsets):
        raise ValueError("minmax_score needs one scale and one offset array per variable")
    dev = _require_device(*variables)
    n = int(variables[0].shape[1])
    run_max = torch.empty(n, dtype=torch.float64, device=dev)
    run_min = torch.empty(n, dtype=torch.float64, device=dev)
    score = torch.empty(n, dtype=torch.float64, device=dev)
    for k, (t, sc, off) in enumerate(zip(variables, scales, offsets)):
        if t.dim() != 2 or int(t.shape[1]) != n or tuple(sc.shape) != (t.shape[0],) or tuple(off.shape) != (t.shape[0],):
            raise ValueError("variables must be [feature, sample] arrays over the same samples with [feature] scales and offsets")
        _lib.call_on(dev, "fv3hip_minmax_score", _ptr(t), _float_code(t), int(t.stride(0)), int(t.stride(1)), int(t.shape[0]),
                     _ptr(sc.to(torch.float64).contiguous()), _ptr(off.to(torch.float64).contiguous()), n, int(k == 0),
                     int(k == len(variables) - 1), _ptr(run_max), _ptr(run_min), _ptr(score), _stream(dev))
    return score


def ocsvm_score(x: torch.Tensor, mean: torch.Tensor, scale: torch.Tensor, support_vectors: torch.Tensor, dual_coef: torch.Tensor,
                gamma: float) -> torch.Tensor:
    """``-Pipeline(StandardScaler, OneClassSVM(rbf)).score_samples`` of the packed float64 ``x`` [feature, sample]
    (fv3fit/sklearn/_ocsvm_novelty_detector.py:124-160)."""
    dev = _require_device(x, mean, scale, support_vectors, dual_coef)
    x = x.to(torch.float64).contiguous()
    nf, n = int(x.shape[0]), int(x.shape[1])
    sv = support_vectors.to(torch.float64).contiguous()
    if tuple(sv.shape[1:]) != (nf,) or tuple(dual_coef.shape) != (sv.shape[0],) or tuple(mean.shape) != (nf,) or tuple(scale.shape) != (nf,):
        raise ValueError("support vectors [n_sv, feature], dual_coef [n_sv], mean / scale [feature] do not fit x [feature, sample]")
    out = torch.empty(n, dtype=torch.float64, device=dev)
    _lib.call_on(dev, "fv3hip_ocsvm_score", _ptr(x), nf, n, _ptr(mean.to(torch.float64).contiguous()), _ptr(scale.to(torch.float64).contiguous()),
                 _ptr(sv), _ptr(dual_coef.to(torch.float64).contiguous()), int(sv.shape[0]), float(gamma), _ptr(out), _stream(dev))
    return out


def precip_closure(t_res: Optional[torch.Tensor], q_res: Optional[torch.Tensor], col_precip: torch.Tensor, delp: torch.Tensor,
                   physics_precip: torch.Tensor, couple: bool = True, in_place: bool = False):
    """The column water budget of fv3fit's precipitative model (keras/_models/precipitative.py:239-253) on the network's
    three denormalised heads, contiguous float32 ``[nz, n]``: returns ``(dQ1, dQ2, total_precipitation_rate [n])``.
    ``delp`` ``[nz, n]`` and ``physics_precip`` ``[n]`` (or ``[1, n]``) are read as they lie, float32 or float64, any strides.
    ``couple``: ``dQ1 = t_res + c_heat * col_precip``, ``dQ2 = q_res + col_precip`` -- written over ``t_res`` / ``q_res``
    when ``in_place``; without it the residual heads are returned as they are (and may be None)."""
    nz, n = int(col_precip.shape[0]), int(col_precip.shape[1])
    heads = [col_precip] + ([t_res, q_res] if couple else [])
    dev = _require_device(*heads, delp, physics_precip)
    for t in heads:
        if t.dtype != torch.float32 or tuple(t.shape) != (nz, n) or not t.is_contiguous():
            raise ValueError(f"the heads must be contiguous float32 [{nz}, {n}] arrays")
    if tuple(delp.shape) != (nz, n):
        raise ValueError(f"delp has shape {tuple(delp.shape)}, the heads have {(nz, n)}")
    pp = physics_precip.reshape(-1) if physics_precip.dim() != 1 and physics_precip.shape[0] == 1 else physics_precip
    if tuple(pp.shape) != (n,):
        raise ValueError(f"physics_precip has shape {tuple(physics_precip.shape)}, expected ({n},)")
    dq1, dq2 = t_res, q_res
    if couple and not in_place:
        dq1, dq2 = torch.empty_like(t_res), torch.empty_like(q_res)
    precip = torch.empty(n, dtype=torch.float32, device=dev)
    on = lambda t: _ptr(t if couple else None)
    _lib.call_on(dev, "fv3hip_precip_closure", on(t_res), on(q_res), _ptr(col_precip), _ptr(delp), _float_code(delp),
                 int(delp.stride(0)), int(delp.stride(1)), _ptr(pp), _float_code(pp), int(pp.stride(0)), nz, n, int(bool(couple)),
                 on(dq1), on(dq2), _ptr(precip), _stream(dev))
    return dq1, dq2, precip


def member_reduce(members: Sequence[torch.Tensor], op: str) -> torch.Tensor:
    """NaN-skipping ``mean`` / ``median`` over same-shaped member arrays (EnsembleModel.predict, models.py:253-260)."""
    dev = _require_device(*members)
    dt = torch.float64 if any(m.dtype == torch.float64 for m in members) else torch.float32
    ms = [m.to(dt).contiguous() for m in members]
    if any(tuple(m.shape) != tuple(ms[0].shape) for m in ms):
        raise ValueError("ensemble members differ in shape")
    if op not in ("mean", "median"):
        raise NotImplementedError(f"Got reduction {op}: only mean, median supported")
    out = torch.empty_like(ms[0])
    ptrs = (ctypes.c_void_p * len(ms))(*[m.data_ptr() for m in ms])
    _lib.call_on(dev, "fv3hip_member_reduce", ptrs, len(ms), _DTYPE_CODE[dt], _OPS[op], out.numel(), _ptr(out), _stream(dev))
    return out


def interpolate_2d(xp: torch.Tensor, x: torch.Tensor, y: torch.Tensor, fill_value: float = float("nan"),
                   z_axis: int = -1) -> torch.Tensor:
    """``mappm.interpolate_2d`` (interpolate_2d.f90:1-28): linear interpolation of ``y(x)`` onto ``xp``
    along ``z_axis`` (x, y: n_in points there, xp: n_out), ``fill_value`` outside each column's range.
    Arrays share all other dims; computed and returned in float64."""
    dev = _require_device(xp, x, y)
    z_axis = z_axis % x.dim()
    if tuple(x.shape) != tuple(y.shape):
        raise ValueError("x and y must have the same shape")
    rest = lambda t: tuple(t.shape[:z_axis]) + tuple(t.shape[z_axis + 1:])
    if rest(xp) != rest(x):
        raise ValueError("xp must match x in every dimension but the interpolated one")
    xp, x, y = (t.to(torch.float64).contiguous() for t in (xp, x, y))
    n_in, n_out = int(x.shape[z_axis]), int(xp.shape[z_axis])
    n_batch, n_inner = _prod(x.shape[:z_axis]), _prod(x.shape[z_axis + 1:])
    layout = _lib.LAYOUT_LEVEL_COL if n_inner > 1 else _lib.LAYOUT_COL_LEVEL
    out = torch.empty_like(xp)
    _lib.call_on(dev, "fv3hip_interpolate_2d", _ptr(xp), _ptr(x), _ptr(y), n_batch, n_inner, n_in, n_out, float(fill_value), layout,
              _ptr(out), _stream(dev))
    return out


EW_OPS = {"mul": 0, "isclose": 1, "isclose_s": 2, "where_nan": 3, "select": 4, "select_s": 5, "gt_s": 6, "lt_s": 7,
          "fillna_s": 8, "and": 9, "min_s": 10, "blend": 11, "mul_s": 12, "where_s": 13, "add": 14, "add_s": 15,
          "sub": 16, "log_floor_s": 17, "exp": 18, "relu_threshold_s": 19, "below_s": 20, "div_s": 21, "incloud_to_gridcell": 22,
          "clip01": 23, "pow_base_s": 24, "minimum_s": 25, "div": 26, "where_pos_s": 27, "sign": 28, "abs": 29, "rsub_s": 30,
          "rdiv_s": 31, "where_gt_s": 32, "le_s": 33, "sin": 34, "cos": 35}


def ew(op: str, a: torch.Tensor, b: Optional[torch.Tensor] = None, c: Optional[torch.Tensor] = None,
       scalar: float = 0.0) -> torch.Tensor:
    """One step of the surface-data mask arithmetic (coarsen_restarts.py:1140-1470), see
    ``fv3hip_ew``: ``b`` / ``c`` have ``a``'s shape, or are [.., y, x] fields shared by the extra
    (level) axis of ``a`` [.., level, y, x]."""
    dev = _require_device(a)
    code = _float_code(a)
    a = a.contiguous()
    inner = int(a.shape[-1] * a.shape[-2]) if a.dim() >= 2 else max(int(a.numel()), 1)

    def operand(t):
        if t is None:
            return None, 1
        t = cast(t, a.dtype).contiguous()
        if tuple(t.shape) == tuple(a.shape):
            return t, 1
        if a.dim() >= 3 and tuple(t.shape) == tuple(a.shape[:-3]) + tuple(a.shape[-2:]):
            return t, int(a.shape[-3])
        raise ValueError(f"operand shape {tuple(t.shape)} does not match {tuple(a.shape)}")

    b, b_rep = operand(b)
    c, c_rep = operand(c)
    out = torch.empty_like(a)
    _lib.call_on(dev, "fv3hip_ew", EW_OPS[op], _ptr(a), _ptr(b), _ptr(c), float(scalar), code, a.numel(), inner, b_rep, c_rep,
              _ptr(out), _stream(dev))
    return out


_CAST_IN = {torch.float32: _lib.F32, torch.float64: _lib.F64, torch.int32: _lib.I32, torch.int64: _lib.I64}


def cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """``x`` in ``dtype`` (float32 / float64): the tensor itself when it already is, else one pass of ``cast_kernel``."""
    if x.dtype == dtype:
        return x
    if x.dtype not in _CAST_IN or dtype not in (torch.float32, torch.float64):
        return x.to(dtype)  # (bool / half etc.: not on the restart path)
    dev = _require_device(x)
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=dev)
    _lib.call_on(dev, "fv3hip_cast", _ptr(x), _CAST_IN[x.dtype], _ptr(out), _CAST_IN[dtype], x.numel(), _stream(dev))
    return out


def cast_many(tensors: Sequence[torch.Tensor], dtype: torch.dtype) -> list:
    """``cast`` of several tensors with one launch for all that need converting (``fv3hip_cast_many``)."""
    tensors = list(tensors)
    todo = [i for i, t in enumerate(tensors) if t.dtype != dtype and t.dtype in _CAST_IN]
    if dtype not in (torch.float32, torch.float64) or len(todo) < 2:
        return [cast(t, dtype) for t in tensors]
    dev = _require_device(*[tensors[i] for i in todo])
    src = [tensors[i].contiguous() for i in todo]
    dst = [torch.empty(t.shape, dtype=dtype, device=dev) for t in src]
    n = len(src)
    _lib.call_on(dev, "fv3hip_cast_many", (ctypes.c_void_p * n)(*[t.data_ptr() for t in src]),
                 (ctypes.c_int * n)(*[_CAST_IN[t.dtype] for t in src]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in dst]),
                 _CAST_IN[dtype], (ctypes.c_int64 * n)(*[t.numel() for t in src]), n, _stream(dev))
    out = list(tensors)
    for i, d in zip(todo, dst):
        out[i] = d
    return [t if t.dtype == dtype else cast(t, dtype) for t in out]  # (anything left: exotic dtypes, one by one)


def halo_pick(rows: torch.Tensor, nbr, row, flip) -> torch.Tensor:
    """(lo, hi) stacked as [2, n_local, ..., n] from the boundary-vector table ``rows`` [6, 4, ..., n] (``cube_edge_rows``):
    entry ``side * n_local + i`` of the host lists names the neighbour tile, which of its four vectors, and whether it is
    read reversed (cubedsphere/grid.py holds the connectivity)."""
    dev = _require_device(rows)
    rows = rows.contiguous()
    n_local = len(nbr) // 2
    # refused here, before anything is allocated or launched: the kernel indexes ``rows`` with these entries
    if rows.dim() < 3 or rows.shape[1] != 4 or rows.element_size() not in (4, 8):
        raise ValueError(f"rows must be [tile, 4, ..., n] of 4- or 8-byte words, got {tuple(rows.shape)} of {rows.dtype}")
    if len(nbr) != 2 * n_local or len(row) != len(nbr) or len(flip) != len(nbr) or n_local > 6:
        raise ValueError(f"nbr, row and flip must hold one entry per side of at most 6 local tiles, got {len(nbr)}, {len(row)}, {len(flip)}")
    if any(not 0 <= int(v) < min(int(rows.shape[0]), 6) for v in nbr) or any(not 0 <= int(v) < 4 for v in row):
        raise ValueError(f"neighbour tiles must lie in [0, {min(int(rows.shape[0]), 6)}) and their vectors in [0, 4), got {list(nbr)}, {list(row)}")
    n = int(rows.shape[-1])
    mid = tuple(rows.shape[2:-1])
    out = torch.empty((2, n_local) + mid + (n,), dtype=rows.dtype, device=dev)
    arr = lambda v: (ctypes.c_int * len(v))(*[int(x) for x in v])
    _lib.call_on(dev, "fv3hip_halo_pick", _ptr(rows), rows.element_size(), n_local, _prod(mid), n, arr(nbr), arr(row), arr(flip),
                 _ptr(out), _stream(dev))
    return out


def cube_edge_rows(x: torch.Tensor) -> torch.Tensor:
    """The four boundary vectors of every square tile of ``x`` [tile, ..., n, n] ->
    [tile, 4, ..., n]: 0: x = 0, 1: x = n-1 (indexed by y), 2: y = 0, 3: y = n-1 (indexed by x).
    The one-cell halo the neighbouring cube faces need (xgcm.py:7-34)."""
    dev = _require_device(x)
    x = x.contiguous()
    if x.element_size() not in (4, 8):
        raise TypeError(f"unsupported dtype {x.dtype}")
    if x.dim() < 3 or x.shape[-1] != x.shape[-2]:
        raise ValueError(f"cube faces must be square [tile, ..., n, n], got {tuple(x.shape)}")
    n_tiles, n = int(x.shape[0]), int(x.shape[-1])
    mid = tuple(x.shape[1:-2])
    rows = torch.empty((n_tiles, 4) + mid + (n,), dtype=x.dtype, device=dev)
    _lib.call_on(dev, "fv3hip_cube_edge_rows", _ptr(x), x.element_size(), n_tiles, _prod(mid), n, _ptr(rows), _stream(dev))
    return rows


def interp_center_to_outer(x: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, axis: int, step: int = 1) -> torch.Tensor:
    """``0.5 * (left + right)`` from cell centres to the n+1 cell edges along the last (``axis`` = 0,
    x) or second-to-last (``axis`` = 1, y) dim; ``lo`` / ``hi`` [..., n_edge] hold the neighbours
    beyond the two ends (regridz.py:123-135).  ``step`` > 1: only every step-th edge (n / step + 1 of them)."""
    dev = _require_device(x)
    code = _float_code(x)
    x = x.contiguous()
    lo = cast(lo, x.dtype).contiguous()
    hi = cast(hi, x.dtype).contiguous()
    ny, nx = int(x.shape[-2]), int(x.shape[-1])
    want = tuple(x.shape[:-2]) + ((ny,) if axis == 0 else (nx,))
    if tuple(lo.shape) != want or tuple(hi.shape) != want:
        raise ValueError(f"halo shape must be {want}, got {tuple(lo.shape)} and {tuple(hi.shape)}")
    step = int(step)
    if step < 1 or (nx if axis == 0 else ny) % step:
        raise ValueError(f"the extent along the axis must be a multiple of step={step}")
    oshape = (ny // step + 1 if axis == 1 else ny, nx // step + 1 if axis == 0 else nx)
    out = torch.empty(tuple(x.shape[:-2]) + oshape, dtype=x.dtype, device=dev)
    _lib.call_on(dev, "fv3hip_interp_center_to_outer_lines", _ptr(x), code, _prod(x.shape[:-2]), ny, nx, int(axis), step,
              _ptr(lo), _ptr(hi), _ptr(out), _stream(dev))
    return out


def pressure_at_interface(delp: torch.Tensor, toa_pressure: float, z_axis: int) -> torch.Tensor:
    """``p[0] = toa; p[k+1] = p[k] + delp[k]`` along ``z_axis`` (size nz -> nz + 1), accumulated
    sequentially in delp's dtype (vertically_dependent.py:41-66)."""
    dev = _require_device(delp)
    delp = delp.contiguous()
    z_axis = z_axis % delp.dim()
    nz = int(delp.shape[z_axis])
    n_batch, n_inner = _prod(delp.shape[:z_axis]), _prod(delp.shape[z_axis + 1:])
    shape = list(delp.shape)
    shape[z_axis] = nz + 1
    out = torch.empty(shape, dtype=delp.dtype, device=dev)
    _lib.call_on(dev,
        "fv3hip_pressure_at_interface", _ptr(delp), _float_code(delp), n_batch, nz, n_inner,
        float(toa_pressure), _ptr(out), _stream(dev),
    )
    return out


def pressure_at_midpoint_log(delp: torch.Tensor, toa_pressure: float, z_axis: int) -> torch.Tensor:
    """``delp / diff(log(p_interface))`` along ``z_axis`` (vertically_dependent.py:153-179)."""
    dev = _require_device(delp)
    delp = delp.contiguous()
    z_axis = z_axis % delp.dim()
    nz = int(delp.shape[z_axis])
    n_batch, n_inner = _prod(delp.shape[:z_axis]), _prod(delp.shape[z_axis + 1:])
    out = torch.empty_like(delp)
    _lib.call_on(dev,
        "fv3hip_pressure_at_midpoint_log", _ptr(delp), _float_code(delp), n_batch, nz, n_inner,
        float(toa_pressure), _ptr(out), _stream(dev),
    )
    return out


def mask_weights(
    weights: torch.Tensor, p_coarse: torch.Tensor, p_fine: torch.Tensor, z_axis: int, extrapolate: bool = False,
    coarse_factor: Optional[int] = None,
) -> torch.Tensor:
    """``weights where p_level < p_fine[surface] else 0`` (regridz.py:200-220).
    ``extrapolate=False``: ``p_coarse`` holds the nz+1 coarse interface pressures and level k is
    compared through its bottom interface; ``extrapolate=True``: ``p_coarse`` holds the nz coarse
    midpoint pressures.  ``p_fine`` has nz+1 levels along ``z_axis``; ``weights`` has the pressure
    shape without the z axis.  ``coarse_factor``: ``p_coarse`` is still on its horizontally coarser grid (last two dims;
    the z axis third from last) and is read through (y // factor, x // factor) instead of an upsampled copy."""
    if coarse_factor is not None and int(coarse_factor) > 1:
        if z_axis % p_fine.dim() != p_fine.dim() - 3:
            return mask_weights(weights, block_upsample(p_coarse, int(coarse_factor)), p_fine, z_axis, extrapolate)
        dev = _require_device(weights, p_coarse, p_fine)
        if p_coarse.dtype != p_fine.dtype:
            raise ValueError("p_coarse and p_fine must have the same dtype")
        p_coarse, p_fine, weights = p_coarse.contiguous(), p_fine.contiguous(), weights.contiguous()
        nz, ny, nx = int(p_fine.shape[-3]) - 1, int(p_fine.shape[-2]), int(p_fine.shape[-1])
        cmp_levels, cmp_offset = (nz, 0) if extrapolate else (nz + 1, 1)
        batch_shape = tuple(p_fine.shape[:-3])
        if tuple(weights.shape) != batch_shape + (ny, nx) or int(p_coarse.shape[-3]) != cmp_levels:
            raise ValueError("weights / p_coarse do not match the fine pressures' shape")
        # the C entry point indexes p_coarse through (y // f) * nxc + x // f and cannot see its size
        f_ = int(coarse_factor)
        coarse_extent = lambda n: (n - 1) // f_ + 1 if n % 2 else n // f_  # (an odd, staggered extent keeps its last point)
        want_c = batch_shape + (cmp_levels, coarse_extent(ny), coarse_extent(nx))
        if tuple(p_coarse.shape) != want_c:
            raise ValueError(f"p_coarse has shape {tuple(p_coarse.shape)}, expected {want_c} for fine pressures "
                             f"{tuple(p_fine.shape)} coarsened by {f_}")
        out = torch.empty(batch_shape + (nz, ny, nx), dtype=weights.dtype, device=dev)
        try:
            _lib.call_on(dev, "fv3hip_mask_weights_coarse", _ptr(weights), _float_code(weights), _ptr(p_coarse), cmp_levels, cmp_offset,
                         _ptr(p_fine), _float_code(p_fine), _prod(batch_shape), nz, ny, nx, int(coarse_factor), 1, _ptr(out), _stream(dev))
        except _lib.Fv3HipError as err:
            if err.code != _lib.EUNSUPPORTED:
                raise
            return mask_weights(weights, block_upsample(p_coarse, int(coarse_factor)), p_fine, z_axis, extrapolate)
        return out
    dev = _require_device(weights, p_coarse, p_fine)
    if p_coarse.dtype != p_fine.dtype:
        raise ValueError("p_coarse and p_fine must have the same dtype")
    p_coarse, p_fine, weights = p_coarse.contiguous(), p_fine.contiguous(), weights.contiguous()
    z_axis = z_axis % p_fine.dim()
    nz = int(p_fine.shape[z_axis]) - 1
    cmp_levels, cmp_offset = (nz, 0) if extrapolate else (nz + 1, 1)
    expect = list(p_fine.shape)
    expect[z_axis] = cmp_levels
    if list(p_coarse.shape) != expect:
        raise ValueError(f"p_coarse has shape {tuple(p_coarse.shape)}, expected {tuple(expect)}")
    batch_shape, inner_shape = tuple(p_fine.shape[:z_axis]), tuple(p_fine.shape[z_axis + 1:])
    n_batch, n_inner = _prod(batch_shape), _prod(inner_shape)
    if tuple(weights.shape) != batch_shape + inner_shape:
        raise ValueError(
            f"weights shape {tuple(weights.shape)} must be the pressure shape without its z axis "
            f"{batch_shape + inner_shape}"
        )
    out = torch.empty(batch_shape + (nz,) + inner_shape, dtype=weights.dtype, device=dev)
    _lib.call_on(dev,
        "fv3hip_mask_weights", _ptr(weights), _float_code(weights), _ptr(p_coarse), cmp_levels, cmp_offset,
        _ptr(p_fine), _float_code(p_fine), n_batch, nz, n_inner, 1, _ptr(out), _stream(dev),
    )
    return out


_workspaces = {}


def _workspace(dev, nbytes: int) -> torch.Tensor:
    """Scratch of the remap, one per (device, HIP stream): it holds a call's list of columns to redo and the fallback
    planes, so calls on different streams must not share it.  A grown workspace replaces the old tensor only for its own
    stream, whose earlier launches are ordered before the new ones."""
    key = (dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _workspaces[key] = ws
    return ws


# Arithmetic of the remap when a call does not say: "exact" -- bit-identical to the compiled reference Fortran, the
# library's contract.  "fast" (reciprocal-multiply, fused multiply-adds and hardware minima in the sweep kernel: a few ulp
# from the reference on every level, except that the reference's limiter is discontinuous where a slope cancels to exactly
# zero -- such a level may take the other, equally monotone profile) is an opt-in: per call (``arith="fast"``), per process
# (``ops.MAPPM_ARITHMETIC = "fast"``) or per environment (``FV3NET_AMD_MAPPM_ARITH=fast``).  bench.py times both.
MAPPM_ARITHMETIC = os.environ.get("FV3NET_AMD_MAPPM_ARITH", "exact")


def _arith_code(arith: Optional[str]) -> int:
    mode = MAPPM_ARITHMETIC if arith is None else arith
    if mode not in ("exact", "fast"):
        raise ValueError(f"arith must be 'exact' or 'fast', got {mode!r}")
    return _lib.ARITH_FAST if mode == "fast" else _lib.ARITH_EXACT


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _remap_inputs(pe1: torch.Tensor, pe2: torch.Tensor, fields):
    """The remap's arrays in one float dtype (float64 if any of them is) and contiguous."""
    dtypes = {t.dtype for t in (pe1, pe2, *fields)}
    if len(dtypes) > 1:
        common = torch.float64 if torch.float64 in dtypes else torch.float32
        pe1, pe2, fields = pe1.to(common), pe2.to(common), [q.to(common) for q in fields]
    return pe1.contiguous(), pe2.contiguous(), [q.contiguous() for q in fields]


def mappm(
    pe1: torch.Tensor,
    q1: torch.Tensor,
    pe2: torch.Tensor,
    iv: int = 1,
    kord: int = 1,
    z_axis: int = -1,
    arith: Optional[str] = None,
) -> torch.Tensor:
    """PPM vertical remap of ``q1`` from interface pressures ``pe1`` to ``pe2`` (mappm.f90).
    ``arith``: "exact" | "fast" (default: ``ops.MAPPM_ARITHMETIC``), see ``FV3HIP_ARITH_*`` in include/fv3hip.h.
    ``z_axis`` is the level axis of all three arrays (km+1, km, kn+1 levels); the other dims
    must match.  ``z_axis=-1`` is the [column, level] layout f2py callers use; any other
    position is handled in place as the native [.., level, .. columns ..] layout.
    Returns float32 with kn levels along ``z_axis``."""
    return mappm_multi(pe1, [q1], pe2, iv=iv, kord=kord, z_axis=z_axis, arith=arith)[0]


def mappm_multi(pe1: torch.Tensor, fields: Sequence[torch.Tensor], pe2: torch.Tensor, iv: int = 1, kord: int = 1,
                z_axis: int = -1, arith: Optional[str] = None) -> list:
    """``mappm`` of several fields that share ``pe1`` and ``pe2`` (every variable of a dataset in
    regridz.py:163-185): one sweep per four fields computes the control flow and the pressure-only terms
    once.  Each result is bit-identical to ``mappm`` on that field in the same arithmetic mode (``arith``: see ``mappm``;
    the default "exact" is bit-identical to the compiled reference)."""
    fields = list(fields)
    if not fields:
        return []
    dev = _require_device(pe1, pe2, *fields)
    pe1, pe2, fields = _remap_inputs(pe1, pe2, fields)
    q1 = fields[0]
    nd = q1.dim()
    z_axis = z_axis % nd
    km, kn = int(q1.shape[z_axis]), int(pe2.shape[z_axis]) - 1
    if int(pe1.shape[z_axis]) != km + 1:
        raise ValueError("f_in must have a vertical dimension one shorter than p_in")

    def others(t):
        return tuple(t.shape[:z_axis]) + tuple(t.shape[z_axis + 1:])

    if any(tuple(q.shape) != tuple(q1.shape) for q in fields) or not (others(pe1) == others(q1) == others(pe2)):
        raise ValueError("All dimensions except vertical must be same size for p_in, f_in and p_out")
    n_batch, n_inner = _prod(q1.shape[:z_axis]), _prod(q1.shape[z_axis + 1:])
    if z_axis == nd - 1:
        layout, nb, ni = _lib.LAYOUT_COL_LEVEL, n_batch, 1
    else:
        layout, nb, ni = _lib.LAYOUT_LEVEL_COL, n_batch, n_inner
    shape = list(q1.shape)
    shape[z_axis] = kn
    outs = [torch.empty(shape, dtype=torch.float32, device=dev) for _ in fields]
    ws = _workspace(dev, int(_lib.load().fv3hip_mappm_workspace_bytes(nb * ni, km)))
    _lib.call_on(dev, "fv3hip_mappm_multi", _ptr(pe1), _ptr_array(fields), _ptr(pe2), _float_code(q1), _ptr_array(outs), len(fields),
                 nb, ni, km, kn, int(iv), int(kord), layout, _arith_code(arith), _ptr(ws), ws.numel(), _stream(dev))
    return outs


def mappm_multi_coarse_target(pe1: torch.Tensor, fields: Sequence[torch.Tensor], pe2_coarse: torch.Tensor, factor: int, iv: int = 1,
                              kord: int = 1, z_axis: int = -3, arith: Optional[str] = None) -> list:
    """``mappm_multi(pe1, fields, block_upsample(pe2_coarse, factor), ...)`` without the upsampled copy: the target interfaces
    stay on their coarse grid ``[..., z, ny_c, nx_c]`` and fine column (y, x) reads coarse column (y // factor, x // factor)
    (regridz.py:119-185; a staggered dim's last point maps to the last coarse point, as ``block_upsample`` repeats it).  The
    vertical axis must be third from last; shapes the fused kernel does not take go through the upsampled copy.  Same results."""
    fields = list(fields)
    if not fields:
        return []
    factor = int(factor)
    q1 = fields[0]
    nd = q1.dim()

    def fallback():
        return mappm_multi(pe1, fields, block_upsample(pe2_coarse, factor), iv=iv, kord=kord, z_axis=z_axis, arith=arith)

    if nd < 3 or z_axis % nd != nd - 3 or factor < 2:
        return fallback()
    dev = _require_device(pe1, pe2_coarse, *fields)
    pe1, pe2_coarse, fields = _remap_inputs(pe1, pe2_coarse, fields)
    q1 = fields[0]
    km, kn = int(q1.shape[-3]), int(pe2_coarse.shape[-3]) - 1
    ny, nx = int(q1.shape[-2]), int(q1.shape[-1])
    if int(pe1.shape[-3]) != km + 1:
        raise ValueError("f_in must have a vertical dimension one shorter than p_in")
    coarse = lambda n: (n - 1) // factor + 1 if n % 2 == 1 else n // factor
    if (any(tuple(q.shape) != tuple(q1.shape) for q in fields) or tuple(pe1.shape[:-3]) != tuple(q1.shape[:-3])
            or tuple(pe1.shape[-2:]) != (ny, nx) or tuple(pe2_coarse.shape[:-3]) != tuple(q1.shape[:-3])
            or tuple(pe2_coarse.shape[-2:]) != (coarse(ny), coarse(nx))):
        raise ValueError("All dimensions except vertical must be same size for p_in, f_in and (the upsampled) p_out")
    nb = _prod(q1.shape[:-3])
    outs = [torch.empty(tuple(q1.shape[:-3]) + (kn, ny, nx), dtype=torch.float32, device=dev) for _ in fields]
    ws = _workspace(dev, int(_lib.load().fv3hip_mappm_workspace_bytes(nb * ny * nx, km)))
    try:
        _lib.call_on(dev, "fv3hip_mappm_multi_coarse_target", _ptr(pe1), _ptr_array(fields), _ptr(pe2_coarse), _float_code(q1),
                     _ptr_array(outs), len(fields), nb, ny, nx, factor, km, kn, int(iv), int(kord), _arith_code(arith), _ptr(ws),
                     ws.numel(), _stream(dev))
    except _lib.Fv3HipError as err:
        if err.code != _lib.EUNSUPPORTED:
            raise
        return fallback()
    return outs


def mappm_block_mean(pe1: torch.Tensor, fields: Sequence[torch.Tensor], pe2_coarse: torch.Tensor, area: torch.Tensor,
                     level_coarse: Optional[torch.Tensor] = None, factor: int = 8, iv: int = 1, kord: int = 1,
                     arith: Optional[str] = None, counters: Optional[torch.Tensor] = None) -> Optional[list]:
    """``weighted_block_average(mappm_multi_coarse_target(pe1, fields, pe2_coarse, factor), mask_weights(area, level, pe1, ...,
    coarse_factor=factor), factor)`` in one kernel (regridz.py:149-220 followed by coarsen.py:183-218, as the pressure-level
    restart pipelines call them): a wavefront owns one 8 x 8 block, sums its remapped, masked values in LDS and writes the
    coarse means -- the fine remapped fields and the masked weights never exist.  ``level_coarse``: the coarse midpoint
    pressures [.., kn, ny/8, nx/8] (``extrapolate=True``); None compares each layer's bottom interface (``pe2_coarse``).
    ``area`` [.., ny, nx] float32 with leading dims that lead the fields' (shared by the rest).  Arrays in [.., z, y, x] order.
    Bit-identical to the three calls above in the same ``arith``.  Returns None where the kernel does not apply (factor != 8,
    extents not multiples of 8, a non-float32 area, kord > 3, ...): the caller takes the three calls.
    ``counters``: a pinned int32 host tensor of 4 elements that receives, asynchronously on the current stream, the call's
    last [columns listed for the sequential routine, blocks redone, blocks whose waves gave up summing, 0] -- what an adaptive
    caller looks at before it chooses the route of its next call (``regridz.area_weighted_pressure_means``)."""
    fields = list(fields)
    if not fields:
        return []
    q1 = fields[0]
    nd = q1.dim()
    if int(factor) != 8 or nd < 3 or area.dtype != torch.float32:
        return None
    dev = _require_device(pe1, pe2_coarse, area, *fields)
    lvl, cmp_offset = (pe2_coarse, 1) if level_coarse is None else (level_coarse, 0)
    dtypes = {t.dtype for t in (pe1, pe2_coarse, lvl, *fields)}
    if len(dtypes) > 1:
        return None
    km, kn = int(q1.shape[-3]), int(pe2_coarse.shape[-3]) - 1
    ny, nx = int(q1.shape[-2]), int(q1.shape[-1])
    batch = tuple(q1.shape[:-3])
    if ny % 8 or nx % 8 or int(kord) > 3 or km < 8 or kn < 1 or kn + 1 > 128:
        return None
    if int(pe1.shape[-3]) != km + 1:
        raise ValueError("f_in must have a vertical dimension one shorter than p_in")
    coarse_hw = (ny // 8, nx // 8)
    if (any(tuple(q.shape) != tuple(q1.shape) for q in fields) or tuple(pe1.shape) != batch + (km + 1, ny, nx)
            or tuple(pe2_coarse.shape) != batch + (kn + 1,) + coarse_hw
            or tuple(lvl.shape) != batch + (kn + cmp_offset,) + coarse_hw):
        raise ValueError("All dimensions except vertical must be same size for p_in, f_in and (the upsampled) p_out")
    lead = tuple(area.shape[:-2])
    if tuple(area.shape[-2:]) != (ny, nx) or lead != batch[: len(lead)]:
        raise ValueError(f"area of shape {tuple(area.shape)} does not lead the fields' {tuple(q1.shape)}")
    nb = _prod(batch)
    if min(len(fields), 4) * nb * kn * ny * nx * 4 > _BLOCK_MEAN_SCRATCH_LIMIT:
        return None   # (the scratch rows are fine-size: 71 GB for a whole C3072 cube -- such calls take the three launches)
    area_repeat = nb // max(_prod(lead), 1)
    pe1, pe2_coarse, lvl, area = pe1.contiguous(), pe2_coarse.contiguous(), lvl.contiguous(), area.contiguous()
    fields = [q.contiguous() for q in fields]
    n = len(fields)
    lib = _lib.load()
    ws = _workspace(dev, int(lib.fv3hip_mappm_block_mean_workspace_bytes(nb * ny * nx, km)))
    # fine-size rows that only evicted values and redone blocks pass through: one allocation, kept per (device, stream, size)
    scratch = _scratch_rows(dev, n, nb * kn * ny * nx)
    outs = [torch.empty(batch + (kn,) + coarse_hw, dtype=torch.float32, device=dev) for _ in fields]
    s_ptrs = _ptr_array([scratch[i % len(scratch)] for i in range(n)])  # (a sweep takes four fields)
    try:
        _lib.call_on(dev, "fv3hip_mappm_block_mean", _ptr(pe1), _ptr_array(fields), _ptr(pe2_coarse), _ptr(lvl), kn + cmp_offset, cmp_offset,
                     _float_code(q1), _ptr(area), area_repeat, s_ptrs, _ptr_array(outs), n, nb, ny, nx, 8, km, kn, int(iv), int(kord),
                     _arith_code(arith), _ptr(ws), ws.numel(), _stream(dev))
    except _lib.Fv3HipError as err:
        if err.code != _lib.EUNSUPPORTED:
            raise
        return None
    if counters is not None:
        counters.copy_(ws[:16].view(torch.int32), non_blocking=True)
    return outs


_scratch = {}
_BLOCK_MEAN_SCRATCH_LIMIT = 24 << 30   # bytes of scratch the fused remap + block mean may hold per (device, stream)


def _scratch_rows(dev, n: int, numel: int) -> list:
    """``n`` float32 scratch arrays of ``numel`` elements for the fused remap + block mean, one set per (device, HIP stream)
    like the remap's workspace: a sweep's four fields use the first four, the next sweep of the same call reuses them in
    stream order."""
    n = min(n, 4)
    key = (dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream)
    have = _scratch.get(key)
    if have is None or have.numel() < n * numel:
        have = _scratch[key] = torch.empty(n * numel, dtype=torch.float32, device=dev)
    return [have[i * numel:(i + 1) * numel] for i in range(n)]


class GroupPlan:
    """Which cells ``group_sums`` adds into which group: ``order`` (int32 cell ids ``batch * n_inner + i``, sorted by group
    with a stable sort), ``start`` (int64 [n_groups + 1]) and the work items the groups are cut into (at most
    ``group_sums_chunk()`` cells each) -- all on the device; ``counts`` (cells per group) is a host array."""

    __slots__ = ("n_batch", "n_inner", "n_groups", "n_items", "order", "start", "item_group", "item_chunk", "group_item", "counts")

    def __init__(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, v)


def group_sums_chunk() -> int:
    """Cells per work item of ``group_sums`` (``fv3hip_group_sums_chunk``)."""
    return int(_lib.load().fv3hip_group_sums_chunk())


def group_plan(group_id: torch.Tensor, n_groups: int) -> GroupPlan:
    """The plan of ``group_sums`` for the integer group ids ``group_id`` [n_batch, n_inner]; an id < 0 or >= ``n_groups``
    leaves the cell in no group.  The sort is torch's stable device sort (index plumbing, no field arithmetic); the cells
    per group come to the host once, to cut the groups into work items."""
    dev = _require_device(group_id)
    if group_id.dim() != 2 or group_id.dtype not in (torch.int32, torch.int64):
        raise ValueError("group_id must be an int32 / int64 tensor [n_batch, n_inner]")
    n_groups = int(n_groups)
    n_batch, n_inner = int(group_id.shape[0]), int(group_id.shape[1])
    if n_groups < 0 or n_batch * n_inner > 0x7FFFFFFF:
        raise ValueError("n_groups must not be negative, and cell ids must fit int32")
    gid = group_id.reshape(-1).to(torch.int64)
    key = torch.where((gid >= 0) & (gid < n_groups), gid, torch.full_like(gid, n_groups))
    _, idx = torch.sort(key, stable=True)
    counts = torch.bincount(key, minlength=n_groups + 1)[:n_groups].cpu().numpy().astype(np.int64)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    chunk = group_sums_chunk()
    per_group = -(-counts // chunk)
    group_item = np.concatenate([[0], np.cumsum(per_group)]).astype(np.int64)
    n_items = int(group_item[-1])
    item_group = np.repeat(np.arange(n_groups, dtype=np.int32), per_group)
    item_chunk = (np.arange(n_items, dtype=np.int64) - group_item[:-1][item_group]).astype(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return GroupPlan(n_batch=n_batch, n_inner=n_inner, n_groups=n_groups, n_items=n_items,
                     order=idx[:int(start[-1])].to(torch.int32).contiguous(), start=up(start), item_group=up(item_group),
                     item_chunk=up(item_chunk), group_item=up(group_item), counts=counts)


def group_sums(a: torch.Tensor, b: Optional[torch.Tensor], weights: Optional[torch.Tensor], plan: GroupPlan,
               z_axis: Optional[int] = None) -> torch.Tensor:
    """float64 [10, n_groups, nz] sums over the cells of each group of ``plan`` (``fv3hip_group_sums``): with ``d = a - b``,
    0: sum w, 1: sum w where a is not NaN, 2: sum w a, 3: sum (w a) a, 4-6: the same for ``b``, 7-9: for ``d``; NaN terms
    are skipped (``nansum``), ``b`` None leaves 4-9 zero, ``weights`` None is 1.  ``a`` (and ``b``) view as
    [n_batch, nz, n_inner] around ``z_axis`` (None: no level axis, nz = 1); ``weights`` as [n_batch, n_inner].  Bitwise
    identical from run to run."""
    tensors = [t for t in (a, b, weights) if t is not None]
    dev = _require_device(plan.order, *tensors)
    code = _float_code(a)
    a = a.contiguous()
    if z_axis is None:
        nb, nz, ni = plan.n_batch, 1, plan.n_inner
        if a.numel() != nb * ni:
            raise ValueError(f"the field has {a.numel()} cells, the plan {nb} x {ni}")
    else:
        _, nb, nz, ni = _column_view(a, z_axis)
        if (nb, ni) != (plan.n_batch, plan.n_inner):
            raise ValueError(f"the field views as [{nb}, {nz}, {ni}], the plan is for [{plan.n_batch}, {plan.n_inner}] cells")
    if b is not None:
        if tuple(b.shape) != tuple(a.shape):
            raise ValueError("a and b must have the same shape")
        b = cast(b, a.dtype).contiguous()
    w_code = _lib.F64
    if weights is not None:
        w_code = _float_code(weights)
        weights = weights.contiguous()
        if weights.numel() != nb * ni:
            raise ValueError(f"weights have {weights.numel()} cells, the plan {nb} x {ni}")
    out = torch.empty((10, plan.n_groups, nz), dtype=torch.float64, device=dev)
    nbytes = int(_lib.load().fv3hip_group_sums_workspace_bytes(plan.n_items, nz))
    ws = _workspace(dev, nbytes)
    _lib.call_on(dev, "fv3hip_group_sums", _ptr(a), _ptr(b), code, _ptr(weights), w_code, nb, nz, ni, _ptr(plan.order),
                 plan.order.numel(), _ptr(plan.start), plan.n_groups, _ptr(plan.item_group), _ptr(plan.item_chunk), plan.n_items,
                 _ptr(plan.group_item), _ptr(out), _ptr(ws), ws.numel(), _stream(dev))
    return out


def _edges(edges: torch.Tensor, dev) -> torch.Tensor:
    if edges.dim() != 1 or edges.numel() < 2:
        raise ValueError("bin edges must be a 1-D array of at least two values")
    return cast(edges.to(dev), torch.float64).contiguous()


def histogram_counts(x: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """``np.histogram(x, bins=edges)[0]`` for explicit edges (a device tensor), int64 [len(edges) - 1]: bins are
    ``edges[i] <= x < edges[i + 1]``, the last one closed; NaN and values outside are dropped.  Up to 4096 bins."""
    dev = _require_device(x, edges)
    x = _as_float(x).contiguous()
    edges = _edges(edges, dev)
    n_bins = int(edges.numel()) - 1
    if n_bins > 4096:
        raise ValueError(f"at most 4096 bins, got {n_bins}")
    counts = torch.empty(n_bins, dtype=torch.int64, device=dev)
    _lib.call_on(dev, "fv3hip_histogram", _ptr(x), _float_code(x), x.numel(), _ptr(edges), n_bins, _ptr(counts), _stream(dev))
    return counts


def histogram2d_counts(x: torch.Tensor, y: torch.Tensor, xedges: torch.Tensor, yedges: torch.Tensor) -> torch.Tensor:
    """``np.histogram2d(x.ravel(), y.ravel(), bins=[xedges, yedges])[0]`` as int64 [nx, ny]; a pair is dropped if either
    member is NaN or outside its edges.  Up to 128 x 128 bins."""
    dev = _require_device(x, y, xedges, yedges)
    if x.numel() != y.numel():
        raise ValueError("x and y must have the same number of values")
    x, y = _as_float(x), _as_float(y)
    dt = _promoted(x, y)
    x, y = cast(x, dt).contiguous(), cast(y, dt).contiguous()
    xedges, yedges = _edges(xedges, dev), _edges(yedges, dev)
    nx, ny = int(xedges.numel()) - 1, int(yedges.numel()) - 1
    if nx > 128 or ny > 128:
        raise ValueError(f"at most 128 x 128 bins, got {nx} x {ny}")
    counts = torch.empty((nx, ny), dtype=torch.int64, device=dev)
    _lib.call_on(dev, "fv3hip_histogram2d", _ptr(x), _ptr(y), _float_code(x), x.numel(), _ptr(xedges), nx, _ptr(yedges), ny,
                 _ptr(counts), _stream(dev))
    return counts


def _as_float(t: torch.Tensor) -> torch.Tensor:
    """Integer data as float64 (what numpy's comparison against float64 edges sees); float data as it is."""
    return t if t.dtype in (torch.float32, torch.float64) else cast(t, torch.float64)


# ---------------------------------------------------------------------------------------------
# training the dense column network (csrc/mlp_train.hip): the caller owns every tensor, nothing is allocated or synchronised
# ---------------------------------------------------------------------------------------------
def train_chunk_rows() -> int:
    """Rows per chunk of ``train_linear_backward_weight``: a longer batch needs its workspace."""
    return int(_lib.load().fv3hip_train_chunk_rows())


def train_backward_weight_workspace_floats(n: int, k: int, o: int) -> int:
    return int(_lib.load().fv3hip_train_backward_weight_workspace_bytes(int(n), int(k), int(o))) // 4


def train_loss_workspace_doubles() -> int:
    return int(_lib.load().fv3hip_train_loss_workspace_doubles())


def _rows_f32(t: torch.Tensor, what: str, features: Optional[int] = None):
    """(rows, features, ld) of a float32 [rows, features] tensor or view whose features are contiguous."""
    if t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError(f"{what} must be a 2-D float32 tensor, got {t.dtype} with {t.dim()} dimensions")
    rows, feats = int(t.shape[0]), int(t.shape[1])
    if feats > 1 and t.stride(1) != 1:
        raise ValueError(f"{what}: the features must be contiguous")
    ld = int(t.stride(0)) if rows > 1 else max(int(t.stride(0)), feats)
    if ld < feats:
        raise ValueError(f"{what}: row stride {ld} is shorter than its {feats} features")
    if features is not None and feats != features:
        raise ValueError(f"{what} has {feats} features, expected {features}")
    return rows, feats, ld


def _vec(t: Optional[torch.Tensor], what: str, n: int, dtype=torch.float32):
    if t is None:
        return None
    if t.dtype != dtype or t.dim() != 1 or int(t.shape[0]) != n or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} vector of {n} values")
    return t


def _batch_rows(idx: Optional[torch.Tensor], table_rows: int) -> int:
    if idx is None:
        return table_rows
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
        raise TypeError("idx must be a contiguous 1-D int64 tensor")
    return int(idx.shape[0])


def train_linear_forward(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor,
                         idx: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """``out[n] = act(a[row(n)] @ w + bias)`` with ``row(n) = idx[n]`` (int64, on the device) or ``n``."""
    dev = _require_device(*(t for t in (a, w, bias, out, idx) if t is not None))
    a_rows, k, lda = _rows_f32(a, "a")
    _, o, ldw = _rows_f32(w, "w")
    if int(w.shape[0]) != k:
        raise ValueError(f"w has {w.shape[0]} rows, a has {k} features")
    n = _batch_rows(idx, a_rows)
    h_rows, _, ldh = _rows_f32(out, "out", o)
    if h_rows < n:
        raise ValueError(f"out has {h_rows} rows, the batch {n}")
    _lib.call_on(dev, "fv3hip_train_linear_forward", _ptr(a), lda, a_rows, _ptr(idx), _ptr(w), ldw, _ptr(_vec(bias, "bias", o)), _ptr(out),
                 ldh, n, k, o, _lib.ACT_RELU if relu else _lib.ACT_LINEAR, _stream(dev))
    return out


def train_linear_backward_data(dh: torch.Tensor, w: torch.Tensor, p: Optional[torch.Tensor], out: torch.Tensor,
                               shared_p: bool = False) -> torch.Tensor:
    """``out[n] = (dh[n] @ w.T) * (p[n] > 0)``; ``p`` None: no mask; ``shared_p``: every row is masked by ``p[0]``."""
    dev = _require_device(*(t for t in (dh, w, p, out) if t is not None))
    n, o, lddh = _rows_f32(dh, "dh")
    k, _, ldw = _rows_f32(w, "w", o)
    a_rows, _, ldda = _rows_f32(out, "out", k)
    if a_rows < n:
        raise ValueError(f"out has {a_rows} rows, the batch {n}")
    ldp = 0
    if p is not None:
        p_rows, _, ldp = _rows_f32(p, "p", k)
        if p_rows < (1 if shared_p else n):
            raise ValueError(f"p has {p_rows} rows, the batch {n}")
    _lib.call_on(dev, "fv3hip_train_linear_backward_data", _ptr(dh), lddh, _ptr(w), ldw, _ptr(p), ldp, 0 if shared_p else 1, _ptr(out),
                 ldda, n, k, o, _stream(dev))
    return out


def _caller_workspace(workspace: Optional[torch.Tensor]):
    if workspace is None:
        return None, 0
    if workspace.dtype != torch.float32 or not workspace.is_contiguous():
        raise TypeError("workspace must be a contiguous float32 tensor")
    return workspace, workspace.numel() * 4


def train_linear_backward_weight(a: torch.Tensor, dh: torch.Tensor, dw: torch.Tensor, db: torch.Tensor,
                                 idx: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """``dw = a[rows].T @ dh``, ``db = dh.sum(0)``; a batch longer than ``train_chunk_rows()`` needs a float32 ``workspace`` of
    ``train_backward_weight_workspace_floats(n, k, o)`` values."""
    dev = _require_device(*(t for t in (a, dh, dw, db, idx, workspace) if t is not None))
    a_rows, k, lda = _rows_f32(a, "a")
    n = _batch_rows(idx, a_rows)
    dh_rows, o, lddh = _rows_f32(dh, "dh")
    if dh_rows < n:
        raise ValueError(f"dh has {dh_rows} rows, the batch {n}")
    w_rows, _, lddw = _rows_f32(dw, "dw", o)
    if w_rows != k:
        raise ValueError(f"dw has {w_rows} rows, a has {k} features")
    workspace, ws_bytes = _caller_workspace(workspace)
    _lib.call_on(dev, "fv3hip_train_linear_backward_weight", _ptr(a), lda, a_rows, _ptr(idx), _ptr(dh), lddh, _ptr(dw), lddw,
                 _ptr(_vec(db, "db", o)), _ptr(workspace), ws_bytes, n, k, o, _stream(dev))
    return dw, db


def train_mse_grad(yhat: torch.Tensor, scale, center, inv_cstd2, lo, hi, keep, wnorm, targets: torch.Tensor, dy: torch.Tensor,
                   loss: torch.Tensor, loss_workspace: torch.Tensor, idx: Optional[torch.Tensor] = None, n: Optional[int] = None):
    """The std-scaled MSE of the clamped, clipped heads (see ``fv3hip_train_mse_grad``): writes ``dy`` and the float64
    ``loss[0]``.  The seven per-feature arrays are float32 ``[F_out]``; ``targets`` is read through ``idx``."""
    dev = _require_device(*(t for t in (yhat, scale, center, inv_cstd2, lo, hi, keep, wnorm, targets, dy, loss, loss_workspace, idx)
                            if t is not None))
    y_rows, f, ldy = _rows_f32(yhat, "yhat")
    t_rows, _, ldt = _rows_f32(targets, "targets", f)
    n = int(n) if n is not None else _batch_rows(idx, y_rows)
    _batch_rows(idx, 0)
    d_rows, _, lddy = _rows_f32(dy, "dy", f)
    if y_rows < n or d_rows < n or (idx is not None and int(idx.shape[0]) < n) or (idx is None and t_rows < n):
        raise ValueError(f"the batch has {n} rows; yhat {y_rows}, dy {d_rows}")
    if loss.dtype != torch.float64 or loss.numel() < 1 or loss_workspace.dtype != torch.float64 or \
            loss_workspace.numel() < train_loss_workspace_doubles() or not loss_workspace.is_contiguous():
        raise ValueError(f"loss must be float64 and loss_workspace {train_loss_workspace_doubles()} contiguous float64 values")
    vecs = [_vec(t, name, f) for t, name in ((scale, "scale"), (center, "center"), (inv_cstd2, "inv_cstd2"), (lo, "lo"), (hi, "hi"),
                                            (keep, "keep"), (wnorm, "wnorm"))]
    _lib.call_on(dev, "fv3hip_train_mse_grad", _ptr(yhat), ldy, *(_ptr(v) for v in vecs), _ptr(targets), ldt, t_rows, _ptr(idx), _ptr(dy),
                 lddy, _ptr(loss), _ptr(loss_workspace), n, f, _stream(dev))
    return dy, loss


def train_precip_loss_grad(yhat: torch.Tensor, scale1, center1, scale2, center2, inv_cstd2_1, inv_cstd2_2, inv_cstd2_3: float,
                           delp: torch.Tensor, physics_precip: torch.Tensor, t1: torch.Tensor, t2: torch.Tensor, t3: torch.Tensor,
                           dy: torch.Tensor, loss: torch.Tensor, loss_workspace: torch.Tensor, idx: Optional[torch.Tensor] = None,
                           couple: bool = True, has_dead: bool = False, l1: float = 0.0, l2: float = 0.0,
                           dq1: Optional[torch.Tensor] = None, dq2: Optional[torch.Tensor] = None,
                           precip: Optional[torch.Tensor] = None, n: Optional[int] = None):
    """The loss behind the closure of the precipitative model and its gradient (see ``fv3hip_train_precip_loss_grad``): writes
    ``dy`` and the float64 ``loss[0]``.  ``yhat`` / ``dy``: ``[n, 3 nz + has_dead]`` laid out ``t | q | dead | cp``; the six
    per-level arrays are float32 ``[nz]``; ``delp``, ``t1``, ``t2`` ``[rows, nz]`` (``t1`` and ``t2`` with one row stride) and
    ``physics_precip``, ``t3`` ``[rows]`` are read through ``idx``.  ``dq1``, ``dq2`` (contiguous ``[n, nz]``) and ``precip``
    (``[n]``) receive the predictions where given."""
    tensors = (yhat, scale1, center1, scale2, center2, inv_cstd2_1, inv_cstd2_2, delp, physics_precip, t1, t2, t3, dy, loss,
               loss_workspace, idx, dq1, dq2, precip)
    dev = _require_device(*(t for t in tensors if t is not None))
    has_dead = bool(has_dead)
    y_rows, f, ldy = _rows_f32(yhat, "yhat")
    nz, rem = divmod(f - int(has_dead), 3)
    if rem or nz < 1:
        raise ValueError(f"yhat has {f} features: not three blocks of levels{' and the dead head' if has_dead else ''}")
    rows, _, ldd = _rows_f32(delp, "delp", nz)
    t_rows, _, ldt = _rows_f32(t1, "t1", nz)
    t2_rows, _, ldt2 = _rows_f32(t2, "t2", nz)
    if ldt2 != ldt or t_rows != rows or t2_rows != rows:
        raise ValueError("delp, t1 and t2 must have the same rows, t1 and t2 one row stride")
    _vec(physics_precip, "physics_precip", rows)
    _vec(t3, "t3", rows)
    n = int(n) if n is not None else _batch_rows(idx, y_rows)
    _batch_rows(idx, 0)
    d_rows, _, lddy = _rows_f32(dy, "dy", f)
    if y_rows < n or d_rows < n or (idx is not None and int(idx.shape[0]) < n) or (idx is None and rows < n):
        raise ValueError(f"the batch has {n} rows; yhat {y_rows}, dy {d_rows}")
    if loss.dtype != torch.float64 or loss.numel() < 1 or loss_workspace.dtype != torch.float64 or \
            loss_workspace.numel() < train_loss_workspace_doubles() or not loss_workspace.is_contiguous():
        raise ValueError(f"loss must be float64 and loss_workspace {train_loss_workspace_doubles()} contiguous float64 values")
    for t, name in ((dq1, "dq1"), (dq2, "dq2")):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (n, nz) or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 [{n}, {nz}] tensor")
    _vec(precip, "precip", n)
    vecs = [_vec(t, name, nz) for t, name in ((scale1, "scale1"), (center1, "center1"), (scale2, "scale2"), (center2, "center2"),
                                             (inv_cstd2_1, "inv_cstd2_1"), (inv_cstd2_2, "inv_cstd2_2"))]
    _lib.call_on(dev, "fv3hip_train_precip_loss_grad", _ptr(yhat), ldy, *(_ptr(v) for v in vecs), float(inv_cstd2_3), _ptr(delp), ldd,
                 _ptr(physics_precip), _ptr(t1), _ptr(t2), ldt, _ptr(t3), rows, _ptr(idx), int(bool(couple)), int(has_dead), float(l1),
                 float(l2), _ptr(dy), lddy, _ptr(loss), _ptr(loss_workspace), _ptr(dq1), _ptr(dq2), _ptr(precip), n, nz, _stream(dev))
    return dy, loss


def train_emulator_loss_workspace_doubles() -> int:
    return int(_lib.load().fv3hip_train_emulator_loss_workspace_doubles())


@dataclasses.dataclass
class EmulatorHead:
    """One head of ``train_emulator_loss_grad`` (``fv3hip_emulator_head_t``).  ``kind``: ``"mse"`` (dense: ``ncol`` features,
    tables ``[ncol]``, target rows ``[rows, ncol]``), ``"mse_local"`` (one column; tables ``[levels]``, target rows
    ``[rows, levels]``, or ``[rows]`` / ``[rows, 1]`` with ``single_level``) or ``"xent"`` (``ncol`` channels, target
    ``[rows, levels, ncol]``).  The direct term exists where ``slot`` is given, the after term where ``slot_after`` is; a term
    with ``is_loss`` false is a metric."""

    kind: str
    col0: int
    ncol: int = 1
    single_level: bool = False
    scale: Optional[torch.Tensor] = None
    center: Optional[torch.Tensor] = None
    slot: Optional[int] = None
    target: Optional[torch.Tensor] = None
    inv: Optional[torch.Tensor] = None
    weight: float = 1.0
    is_loss: bool = True
    slot_after: Optional[int] = None
    before: Optional[torch.Tensor] = None
    target_after: Optional[torch.Tensor] = None
    inv_after: Optional[torch.Tensor] = None
    weight_after: float = 1.0
    is_loss_after: bool = True


_EMULATOR_KINDS = {"mse": _lib.EMULATOR_HEAD_MSE_DENSE, "mse_local": _lib.EMULATOR_HEAD_MSE_LOCAL, "xent": _lib.EMULATOR_HEAD_XENT}


class EmulatorHeadTable:
    """The head table of ``train_emulator_loss_grad`` in the library's form, built once: the descriptors as a host array (it goes
    to the kernel by value), the tensors they point into kept alive, their common device and row count."""

    def __init__(self, heads: Sequence[EmulatorHead], levels: int = 1):
        self.heads, self.levels = list(heads), int(levels)
        self.array = (_lib.EmulatorHead * max(len(self.heads), 1))()
        self.n_slots = sum((h.slot is not None) + (h.slot_after is not None) for h in self.heads)
        self.f = sum(int(h.ncol) for h in self.heads)
        tensors, rows = [], set()

        def resident(t, what, inner):
            """(pointer, row stride) of a float32 array [rows, *inner] (or [rows] for one value a row) with contiguous rows."""
            if t is None:
                return None, 0
            if t.dtype != torch.float32 or (t.dim() == 1 and _prod(inner) != 1) or (t.dim() > 1 and tuple(t.shape[1:]) != tuple(inner)):
                raise ValueError(f"{what} must be a float32 [rows, {', '.join(str(i) for i in inner)}] tensor, got {t.dtype} "
                                 f"{tuple(t.shape)}")
            if t.dim() > 1 and not t[0].is_contiguous():
                raise ValueError(f"{what}: the values of a row must be contiguous")
            tensors.append(t)
            rows.add(int(t.shape[0]))
            return t.data_ptr(), max(int(t.stride(0)), _prod(inner)) if t.shape[0] > 1 else _prod(inner)

        for d, h in zip(self.array, self.heads):
            if h.kind not in _EMULATOR_KINDS:
                raise ValueError(f"head kind must be one of {sorted(_EMULATOR_KINDS)}, got {h.kind!r}")
            d.kind, d.col0, d.ncol, d.single_level = _EMULATOR_KINDS[h.kind], int(h.col0), int(h.ncol), int(bool(h.single_level))
            d.slot = -1 if h.slot is None else int(h.slot)
            d.slot_after = -1 if h.slot_after is None else int(h.slot_after)
            d.is_loss, d.is_loss_after = int(bool(h.is_loss)), int(bool(h.is_loss_after))
            d.weight, d.weight_after = float(h.weight), float(h.weight_after)
            nt = int(h.ncol) if h.kind == "mse" else self.levels   # the tables' length
            inner = (self.levels, int(h.ncol)) if h.kind == "xent" else (1,) if h.single_level else (nt,)
            for key in ("scale", "center", "inv", "inv_after"):
                t = _vec(getattr(h, key), key, nt)
                if t is not None:
                    tensors.append(t)
                setattr(d, key, None if t is None else t.data_ptr())
            d.target, d.ld_target = resident(h.target, "target", inner)
            d.before, d.ld_before = resident(h.before, "before", inner)
            d.target_after, d.ld_target_after = resident(h.target_after, "target_after", inner)
        if len(rows) > 1:
            raise ValueError(f"the resident arrays differ in their rows: {sorted(rows)}")
        self.rows = rows.pop() if rows else None   # (no resident array: any batch fits)
        self.tensors = tensors
        self.device = _require_device(*tensors) if tensors else None


def train_emulator_loss_grad(yhat: torch.Tensor, table: EmulatorHeadTable, dy: Optional[torch.Tensor], values: torch.Tensor,
                             loss: torch.Tensor, workspace: torch.Tensor, idx: Optional[torch.Tensor] = None,
                             accum: Optional[torch.Tensor] = None, n: Optional[int] = None):
    """The multi-variable loss of the microphysics emulators and its gradient (see ``fv3hip_train_emulator_loss_grad``).
    ``yhat`` / ``dy``: ``[n * levels, >= f]`` network rows (``dy`` None: loss only); ``values`` float64 ``[n_slots]``, ``loss``
    float64 ``[1]``, ``accum`` float64 ``[1 + n_slots]`` or None, ``workspace`` ``train_emulator_loss_workspace_doubles()``
    float64 values; ``idx`` the row table of the ``n`` batch rows."""
    dev = _require_device(*(t for t in (yhat, dy, values, loss, workspace, idx, accum) if t is not None))
    if table.device is not None and table.device != dev:
        raise RuntimeError(f"the head table lives on {table.device}, the call on {dev}")
    y_rows, y_feats, ldy = _rows_f32(yhat, "yhat")
    levels = table.levels
    _batch_rows(idx, 0)
    n = int(n) if n is not None else (int(idx.shape[0]) if idx is not None else y_rows // levels)
    if n < 1 or y_rows < n * levels or y_feats < table.f or (idx is not None and int(idx.shape[0]) < n):
        raise ValueError(f"the batch has {n} rows of {levels} levels and {table.f} head features; yhat is {tuple(yhat.shape)}")
    lddy = 0
    if dy is not None:
        d_rows, d_feats, lddy = _rows_f32(dy, "dy")
        if d_rows < n * levels or d_feats < table.f:
            raise ValueError(f"dy is {tuple(dy.shape)}, the batch needs [{n * levels}, {table.f}]")
    for t, name, count in ((values, "values", table.n_slots), (loss, "loss", 1), (workspace, "workspace", train_emulator_loss_workspace_doubles()),
                           (accum, "accum", 1 + table.n_slots)):
        if t is not None and (t.dtype != torch.float64 or t.numel() < count or not t.is_contiguous()):
            raise ValueError(f"{name} must hold {count} contiguous float64 values")
    _lib.call_on(dev, "fv3hip_train_emulator_loss_grad", _ptr(yhat), ldy, n, levels, table.f, table.array, len(table.heads), table.n_slots,
                 n if table.rows is None else table.rows, _ptr(idx), _ptr(dy), lddy, _ptr(values), _ptr(loss), _ptr(accum), _ptr(workspace), _stream(dev))
    return dy, loss


def _optimizer_state(params: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: torch.Tensor):
    """(device, count) of the flat float32 buffers of ``train_adam`` / ``train_adamw`` and their int64 step counter, checked."""
    dev = _require_device(params, grad, m, v, step)
    count = int(params.numel())
    for t, name in ((params, "params"), (grad, "grad"), (m, "m"), (v, "v")):
        _vec(t, name, count)
    if step.dtype != torch.int64 or step.numel() != 1:
        raise TypeError("step must be an int64 tensor of one element")
    return dev, count


def train_adam(params: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: torch.Tensor, lr: float = 1e-3,
               beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8) -> None:
    """``torch.optim.Adam``'s default update of one flat float32 buffer; ``step`` is an int64 device scalar holding the number of
    steps taken so far, advanced on the device."""
    dev, count = _optimizer_state(params, grad, m, v, step)
    _lib.call_on(dev, "fv3hip_train_adam", _ptr(params), _ptr(grad), _ptr(m), _ptr(v), count, _ptr(step), float(lr), float(beta1),
                 float(beta2), float(eps), _stream(dev))


# ---------------------------------------------------------------------------------------------
# training the convolutional network (csrc/conv_train.hip): the caller owns every tensor, nothing is allocated or synchronised
# ---------------------------------------------------------------------------------------------
def train_conv_chunk_pixels() -> int:
    """Output pixels per chunk of ``train_conv_backward_weight``: a larger batch needs its workspace."""
    return int(_lib.load().fv3hip_train_conv_chunk_pixels())


def train_conv_backward_weight_workspace_floats(n: int, x: int, y: int, k: int, c: int, f: int) -> int:
    """For ``n`` samples of a layer INPUT of ``x`` by ``y`` cells."""
    return int(_lib.load().fv3hip_train_conv_backward_weight_workspace_bytes(int(n), int(x), int(y), int(k), int(c), int(f))) // 4


def _cells_f32(t: torch.Tensor, what: str, channels: Optional[int] = None):
    """((samples, x, y, channels), (sample, x, y strides)) of a float32 [sample, x, y, channel] tensor or view whose channels are
    contiguous."""
    if t.dtype != torch.float32 or t.dim() != 4:
        raise TypeError(f"{what} must be a 4-D float32 tensor [sample, x, y, channel], got {t.dtype} with {t.dim()} dimensions")
    shape = tuple(int(v) for v in t.shape)
    if min(shape) < 1:
        raise ValueError(f"{what} is empty: {shape}")
    if shape[3] > 1 and t.stride(3) != 1:
        raise ValueError(f"{what}: the channels must be contiguous")
    # (the stride of an axis of length 1 is never multiplied by anything but 0: any valid value does)
    strides = [int(t.stride(d)) if shape[d] > 1 else 0 for d in range(3)]
    strides[2] = max(strides[2], shape[3])
    if min(strides) < 0 or (shape[2] > 1 and int(t.stride(2)) < shape[3]):
        raise ValueError(f"{what}: strides {tuple(t.stride())} do not hold {shape[3]} contiguous channels")
    if channels is not None and shape[3] != channels:
        raise ValueError(f"{what} has {shape[3]} channels, expected {channels}")
    return shape, strides


def _conv_kernel_f32(w: torch.Tensor, what: str):
    """(k, c, f, ld) of a float32 kernel [k, k, c_in, f] (Keras layout) that is a matrix [k k c_in][f] with a leading dimension."""
    if w.dtype != torch.float32 or w.dim() != 4 or w.shape[0] != w.shape[1]:
        raise TypeError(f"{what} must be a float32 kernel [k, k, c_in, f], got {w.dtype} {tuple(w.shape)}")
    k, _, c, f = (int(v) for v in w.shape)
    if min(k, c, f) < 1:
        raise ValueError(f"{what} is empty: {tuple(w.shape)}")
    if f > 1 and w.stride(3) != 1:
        raise ValueError(f"{what}: the filters must be contiguous")
    ld = int(w.stride(2)) if c > 1 else (int(w.stride(1)) if k > 1 else f)
    want = (k * c * ld, c * ld, ld)
    if ld < f or any(int(w.shape[d]) > 1 and int(w.stride(d)) != want[d] for d in range(3)):
        raise ValueError(f"{what}: strides {tuple(w.stride())} are not those of a matrix [k k c_in][f] with one leading dimension")
    return k, c, f, ld


def train_conv_forward(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor,
                       idx: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """``out[s, x, y] = act(sum_{i,j} a[sample(s), x + i, y + j] @ w[i, j] + bias)`` ("valid"), ``sample(s) = idx[s]`` (int64, on
    the device) or ``s``; ``a`` ``[samples, X, Y, c]``, ``out`` ``[>= batch, X - k + 1, Y - k + 1, f]``, views with padding allowed."""
    dev = _require_device(*(t for t in (a, w, bias, out, idx) if t is not None))
    k, c, f, ldw = _conv_kernel_f32(w, "w")
    (a_samples, X, Y, _), sa = _cells_f32(a, "a", c)
    n = _batch_rows(idx, a_samples)
    (h_samples, ox, oy, _), sh = _cells_f32(out, "out", f)
    if h_samples < n or (ox, oy) != (X - k + 1, Y - k + 1):
        raise ValueError(f"out is {tuple(out.shape)}; a batch of {n} samples of {X} x {Y} cells under a {k} x {k} kernel gives "
                         f"{(n, X - k + 1, Y - k + 1, f)}")
    _lib.call_on(dev, "fv3hip_train_conv_forward", _ptr(a), *sa, a_samples, _ptr(idx), _ptr(w), ldw, _ptr(_vec(bias, "bias", f)),
                 _ptr(out), *sh, n, X, Y, k, c, f, _lib.ACT_RELU if relu else _lib.ACT_LINEAR, _stream(dev))
    return out


def train_conv_backward_data(dh: torch.Tensor, w: torch.Tensor, p: Optional[torch.Tensor], out: torch.Tensor) -> torch.Tensor:
    """``out`` = the gradient with respect to the layer's input ``[n, X, Y, c]`` from ``dh`` ``[n, X - k + 1, Y - k + 1, f]``,
    an exact 0 where ``p > 0`` is false (``p``: the post-ReLU input of the layer, of ``out``'s extent; None: no mask)."""
    dev = _require_device(*(t for t in (dh, w, p, out) if t is not None))
    k, c, f, ldw = _conv_kernel_f32(w, "w")
    (n, ox, oy, _), sdh = _cells_f32(dh, "dh", f)
    (a_samples, X, Y, _), sda = _cells_f32(out, "out", c)
    if a_samples < n or (ox, oy) != (X - k + 1, Y - k + 1):
        raise ValueError(f"out is {tuple(out.shape)}, dh {tuple(dh.shape)}: not the input and output of a {k} x {k} kernel")
    sp = [0, 0, 0]
    if p is not None:
        (p_samples, px, py, _), sp = _cells_f32(p, "p", c)
        if p_samples < n or (px, py) != (X, Y):
            raise ValueError(f"p is {tuple(p.shape)}, out {tuple(out.shape)}")
    _lib.call_on(dev, "fv3hip_train_conv_backward_data", _ptr(dh), *sdh, _ptr(w), ldw, _ptr(p), *sp, _ptr(out), *sda, n, X, Y, k, c, f,
                 _stream(dev))
    return out


def train_conv_backward_weight(a: torch.Tensor, dh: torch.Tensor, dw: torch.Tensor, db: Optional[torch.Tensor],
                               idx: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """``dw[i, j] = sum_{s,x,y} a[sample(s), x + i, y + j].T @ dh[s, x, y]``, ``db = dh.sum((0, 1, 2))`` (None: skipped); a batch
    of more than ``train_conv_chunk_pixels()`` output pixels needs a float32 ``workspace`` of
    ``train_conv_backward_weight_workspace_floats(n, X, Y, k, c, f)`` values."""
    dev = _require_device(*(t for t in (a, dh, dw, db, idx, workspace) if t is not None))
    k, c, f, lddw = _conv_kernel_f32(dw, "dw")
    (a_samples, X, Y, _), sa = _cells_f32(a, "a", c)
    n = _batch_rows(idx, a_samples)
    (dh_samples, ox, oy, _), sdh = _cells_f32(dh, "dh", f)
    if dh_samples < n or (ox, oy) != (X - k + 1, Y - k + 1):
        raise ValueError(f"dh is {tuple(dh.shape)}; a batch of {n} samples of {X} x {Y} cells under a {k} x {k} kernel gives "
                         f"{(n, X - k + 1, Y - k + 1, f)}")
    workspace, ws_bytes = _caller_workspace(workspace)
    _lib.call_on(dev, "fv3hip_train_conv_backward_weight", _ptr(a), *sa, a_samples, _ptr(idx), _ptr(dh), *sdh, _ptr(dw), lddw,
                 _ptr(_vec(db, "db", f)), _ptr(workspace), ws_bytes, n, X, Y, k, c, f, _stream(dev))
    return dw, db


def train_conv_constrain(w: torch.Tensor) -> torch.Tensor:
    """``w <- 0.5 * (w + w.transpose(0, 1))`` in place (the reference's ``TransposeInvariant``), bitwise symmetric."""
    dev = _require_device(w)
    k, c, f, ldw = _conv_kernel_f32(w, "w")
    _lib.call_on(dev, "fv3hip_train_conv_constrain", _ptr(w), ldw, k, c, f, _stream(dev))
    return w


# ---------------------------------------------------------------------------------------------
# training the graph U-Net (csrc/graph_train.hip): the caller owns every tensor, nothing is allocated or synchronised.  A cube
# buffer is passed as a slice (``cube._Slice``: tensor, ld, channel offset, sample stride; stride 0: densely packed cubes).
# ---------------------------------------------------------------------------------------------
def graph_train_chunk_cells() -> int:
    """Cells per chunk of the graph weight gradients: a larger batch needs their workspace."""
    return int(_lib.load().fv3hip_graph_train_chunk_cells())


def graph_sage_backward_weight_workspace_floats(n_samples: int, n: int, c_in: int, c_out: int) -> int:
    return int(_lib.load().fv3hip_graph_sage_backward_weight_workspace_bytes(int(n_samples), int(n), int(c_in), int(c_out))) // 4


def graph_up2_backward_weight_workspace_floats(n_samples: int, n: int, c_in: int, c_out: int) -> int:
    """For ``n_samples`` cubes of a layer INPUT (``low``) of ``n`` cells per edge."""
    return int(_lib.load().fv3hip_graph_up2_backward_weight_workspace_bytes(int(n_samples), int(n), int(c_in), int(c_out))) // 4


def _cube_slice(sl, what: str, n_samples: int, n: int, c: int):
    """(pointer, ld, off, stride) of a slice, checked against its tensor: ``c`` channels of ``n_samples`` cubes must fit."""
    t = sl.tensor
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    if sl.off < 0 or sl.off + c > sl.ld:
        raise ValueError(f"{what}: channels [{sl.off}, {sl.off + c}) do not fit a row of {sl.ld}")
    cube = 6 * n * n * sl.ld
    stride = sl.stride or cube
    if stride < cube or (t.is_contiguous() and n_samples and (n_samples - 1) * stride + cube > t.numel()):
        raise ValueError(f"{what}: {n_samples} cubes of {n} x {n} cells and {sl.ld} channels do not fit a tensor of shape {tuple(t.shape)}")
    return ctypes.c_void_p(sl.ptr), sl.ld, sl.off, sl.stride


def _dense_weight(t: torch.Tensor, what: str, shape) -> torch.Tensor:
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t


def graph_sage_backward_data(dh, w_self: torch.Tensor, w_neigh: torch.Tensor, p, p_act: int, dst, n_samples: int, n: int,
                             c_in: int, c_out: int, accumulate: bool = False) -> None:
    """``dst = (dh W_self^T + mean5(dh) W_neigh^T) act'(p)`` (``p``: a slice or None); ``accumulate``: added to ``dst``."""
    dev = _require_device(dh.tensor, w_self, w_neigh, dst.tensor, *([p.tensor] if p is not None else []))
    _dense_weight(w_self, "w_self", (c_in, c_out)), _dense_weight(w_neigh, "w_neigh", (c_in, c_out))
    ps = _cube_slice(p, "p", n_samples, n, c_in) if p is not None else (None, 0, 0, 0)
    _lib.call_on(dev, "fv3hip_graph_sage_backward_data", *_cube_slice(dh, "dh", n_samples, n, c_out), _ptr(w_self), _ptr(w_neigh),
                 *ps, int(p_act), *_cube_slice(dst, "dst", n_samples, n, c_in), int(bool(accumulate)), n_samples, n, c_in, c_out,
                 _stream(dev))


def graph_sage_backward_weight(x, g, dw_self: torch.Tensor, dw_neigh: torch.Tensor, db: Optional[torch.Tensor], n_samples: int,
                               n: int, c_in: int, c_out: int, workspace: Optional[torch.Tensor] = None,
                               accumulate: bool = False) -> None:
    """``dw_self = x^T g``, ``dw_neigh = mean5(x)^T g``, ``db = sum g`` over the cells of the batch; ``accumulate``: added."""
    dev = _require_device(x.tensor, g.tensor, dw_self, dw_neigh, *(t for t in (db, workspace) if t is not None))
    _dense_weight(dw_self, "dw_self", (c_in, c_out)), _dense_weight(dw_neigh, "dw_neigh", (c_in, c_out))
    ws, ws_bytes = _caller_workspace(workspace)
    _lib.call_on(dev, "fv3hip_graph_sage_backward_weight", *_cube_slice(x, "x", n_samples, n, c_in),
                 *_cube_slice(g, "g", n_samples, n, c_out), _ptr(dw_self), _ptr(dw_neigh), _ptr(_vec(db, "db", c_out)),
                 int(bool(accumulate)), _ptr(ws), ws_bytes, n_samples, n, c_in, c_out, _stream(dev))


def graph_up2_backward_data(dcat, w: torch.Tensor, p, p_act: int, dst, n_samples: int, n: int, c_in: int, c_out: int) -> None:
    """``dst[i][j][ci] = (sum dcat[2i+di][2j+dj][co] w[ci][di][dj][co]) act'(p)``; ``n``: the edge of ``dst``."""
    dev = _require_device(dcat.tensor, w, dst.tensor, *([p.tensor] if p is not None else []))
    _dense_weight(w, "w", (c_in, 2, 2, c_out))
    ps = _cube_slice(p, "p", n_samples, n, c_in)[:3] if p is not None else (None, 0, 0)
    _lib.call_on(dev, "fv3hip_graph_up2_backward_data", *_cube_slice(dcat, "dcat", n_samples, 2 * n, c_out)[:3], _ptr(w), *ps,
                 int(p_act), *_cube_slice(dst, "dst", n_samples, n, c_in)[:3], n_samples, n, c_in, c_out, _stream(dev))


def graph_up2_backward_weight(low, dcat, dw: torch.Tensor, db: Optional[torch.Tensor], n_samples: int, n: int, c_in: int,
                              c_out: int, workspace: torch.Tensor, accumulate: bool = False) -> None:
    """``dw[ci][di][dj][co] = sum low[i][j][ci] dcat[2i+di][2j+dj][co]``, ``db = sum dcat``; ``n``: the edge of ``low``."""
    dev = _require_device(low.tensor, dcat.tensor, dw, workspace, *([db] if db is not None else []))
    _dense_weight(dw, "dw", (c_in, 2, 2, c_out))
    ws, ws_bytes = _caller_workspace(workspace)
    _lib.call_on(dev, "fv3hip_graph_up2_backward_weight", *_cube_slice(low, "low", n_samples, n, c_in)[:3],
                 *_cube_slice(dcat, "dcat", n_samples, 2 * n, c_out)[:3], _ptr(dw), _ptr(_vec(db, "db", c_out)),
                 int(bool(accumulate)), _ptr(ws), ws_bytes, n_samples, n, c_in, c_out, _stream(dev))


def graph_pool2_backward(dpool, p, p_act: int, dst, n_samples: int, n: int, c: int) -> None:
    """``dst = (dst + 0.25 dpool[x / 2][y / 2]) act'(p)`` in place; ``n``: the edge of ``dst``."""
    dev = _require_device(dpool.tensor, dst.tensor, *([p.tensor] if p is not None else []))
    ps = _cube_slice(p, "p", n_samples, n, c)[:3] if p is not None else (None, 0, 0)
    _lib.call_on(dev, "fv3hip_graph_pool2_backward", *_cube_slice(dpool, "dpool", n_samples, n // 2, c)[:3], *ps, int(p_act),
                 *_cube_slice(dst, "dst", n_samples, n, c)[:3], n_samples, n, c, _stream(dev))


def train_adamw(params: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: torch.Tensor, lr: float = 1e-3,
                beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 1e-2) -> None:
    """``torch.optim.AdamW``'s default update of one flat float32 buffer: ``p *= 1 - lr weight_decay``, then ``train_adam``."""
    dev, count = _optimizer_state(params, grad, m, v, step)
    _lib.call_on(dev, "fv3hip_train_adamw", _ptr(params), _ptr(grad), _ptr(m), _ptr(v), count, _ptr(step), float(lr), float(beta1),
                 float(beta2), float(eps), float(weight_decay), _stream(dev))


# ---------------------------------------------------------------------------------------------
# training the CycleGAN (csrc/cyclegan_train.hip): the caller owns every tensor, nothing is allocated or
# synchronised.  Cube buffers are ``cube._Slice``s; ``n`` is the edge of the layer input ``x``; ``kind`` is a key of
# ``cyclegan.KINDS``; ``halo``: cube halos (True) or zero padding.
# ---------------------------------------------------------------------------------------------
def _cyclegan_geometry(kind: str, n: int, halo: bool):
    """(kind code, halo code, edge of dy)."""
    codes = {"regular": (_lib.CYCLEGAN_CONV_REGULAR, n), "strided": (_lib.CYCLEGAN_CONV_STRIDED, n // 2),
             "transposed": (_lib.CYCLEGAN_CONV_TRANSPOSED, 2 * n)}
    if kind not in codes:
        raise ValueError(f"unknown convolution kind {kind!r}: {sorted(codes)} are built")
    return codes[kind][0], _lib.CYCLEGAN_HALO_CUBE if halo else _lib.CYCLEGAN_HALO_ZEROS, codes[kind][1]


def _cyclegan_weight(t: torch.Tensor, what: str, kind: str, k: int, c_in: int, c_out: int) -> torch.Tensor:
    shape = (2, 2, 2, 2, c_in, c_out) if kind == "transposed" else (k, k, c_in, c_out)
    return _dense_weight(t, what, shape)


def cyclegan_train_chunk_cells() -> int:
    """Rows per partial of the CycleGAN weight gradients."""
    return int(_lib.load().fv3hip_cyclegan_train_chunk_cells())


def cyclegan_train_backward_data_workspace_floats(n_samples: int, n: int, c_in: int, kind: str, k: int, halo: bool) -> int:
    code, mode, _ = _cyclegan_geometry(kind, n, halo)
    return int(_lib.load().fv3hip_cyclegan_train_backward_data_workspace_bytes(int(n_samples), int(n), int(c_in), code, int(k), mode)) // 4


def cyclegan_train_backward_weight_workspace_floats(n_samples: int, n: int, c_in: int, c_out: int, kind: str, k: int) -> int:
    code, _, _ = _cyclegan_geometry(kind, n, True)
    return int(_lib.load().fv3hip_cyclegan_train_backward_weight_workspace_bytes(int(n_samples), int(n), int(c_in), int(c_out), code,
                                                                                 int(k))) // 4


def cyclegan_train_conv(x, w: torch.Tensor, bias: Optional[torch.Tensor], y, n_samples: int, n: int, c_in: int, c_out: int, kind: str,
                        k: int, halo: bool) -> None:
    """``y = conv(x~, w) + bias``: ``fv3hip_cyclegan_conv`` without the loader's transform, plus the 3 x 3 strided kind."""
    dev = _require_device(x.tensor, w, y.tensor, *([bias] if bias is not None else []))
    code, mode, n_out = _cyclegan_geometry(kind, n, halo)
    _cyclegan_weight(w, "w", kind, k, c_in, c_out)
    _lib.call_on(dev, "fv3hip_cyclegan_train_conv", *_cube_slice(x, "x", n_samples, n, c_in), _ptr(w), _ptr(_vec(bias, "bias", c_out)),
                 *_cube_slice(y, "y", n_samples, n_out, c_out), n_samples, n, c_in, c_out, code, int(k), mode, _stream(dev))


def cyclegan_train_backward_data(dy, w: torch.Tensor, dx, n_samples: int, n: int, c_in: int, c_out: int, kind: str, k: int, halo: bool,
                                 workspace: Optional[torch.Tensor] = None) -> None:
    """``dx`` = the adjoint of the convolution in its input, across the seams; cube halos need ``workspace``."""
    dev = _require_device(dy.tensor, w, dx.tensor, *([workspace] if workspace is not None else []))
    code, mode, n_out = _cyclegan_geometry(kind, n, halo)
    _cyclegan_weight(w, "w", kind, k, c_in, c_out)
    ws, ws_bytes = _caller_workspace(workspace)
    _lib.call_on(dev, "fv3hip_cyclegan_train_backward_data", *_cube_slice(dy, "dy", n_samples, n_out, c_out), _ptr(w),
                 *_cube_slice(dx, "dx", n_samples, n, c_in), _ptr(ws), ws_bytes, n_samples, n, c_in, c_out, code, int(k), mode,
                 _stream(dev))


def cyclegan_train_backward_weight(x, dy, dw: torch.Tensor, db: Optional[torch.Tensor], n_samples: int, n: int, c_in: int, c_out: int,
                                   kind: str, k: int, halo: bool, workspace: torch.Tensor) -> None:
    """``dw`` in the forward's weight layout and ``db = sum dy`` (or None), both overwritten."""
    dev = _require_device(x.tensor, dy.tensor, dw, workspace, *([db] if db is not None else []))
    code, mode, n_out = _cyclegan_geometry(kind, n, halo)
    _cyclegan_weight(dw, "dw", kind, k, c_in, c_out)
    ws, ws_bytes = _caller_workspace(workspace)
    _lib.call_on(dev, "fv3hip_cyclegan_train_backward_weight", *_cube_slice(x, "x", n_samples, n, c_in),
                 *_cube_slice(dy, "dy", n_samples, n_out, c_out), _ptr(dw), _ptr(_vec(db, "db", c_out)), _ptr(ws), ws_bytes, n_samples, n,
                 c_in, c_out, code, int(k), mode, _stream(dev))


def cyclegan_train_norm_backward(dy, x, mean: torch.Tensor, rstd: torch.Tensor, bias: Optional[torch.Tensor], slope: float, dx,
                                 dbias: Optional[torch.Tensor], n_samples: int, n: int, c: int) -> None:
    """The adjoint of ``act((x - mean) * rstd + bias)`` (leaky ReLU of ``slope``; 1: none) in ``x``; ``dbias``: in the bias."""
    dev = _require_device(dy.tensor, x.tensor, mean, rstd, dx.tensor, *(t for t in (bias, dbias) if t is not None))
    _dense_weight(mean, "mean", (n_samples, 6, c)), _dense_weight(rstd, "rstd", (n_samples, 6, c))
    for t, what in ((bias, "bias"), (dbias, "dbias")):
        if t is not None:
            _dense_weight(t, what, (6, n, n, c))
    _lib.call_on(dev, "fv3hip_cyclegan_train_norm_backward", *_cube_slice(dy, "dy", n_samples, n, c), *_cube_slice(x, "x", n_samples, n, c),
                 _ptr(mean), _ptr(rstd), _ptr(bias), float(slope), *_cube_slice(dx, "dx", n_samples, n, c), _ptr(dbias), n_samples, n, c,
                 _stream(dev))


# ---------------------------------------------------------------------------------------------
# training the FMR recurrent generator (csrc/cyclegan_train.hip): a regular convolution with context
# channels -- ``ctx_cell`` ``[6, n, n, c_cell]`` and ``ctx_uniform`` ``[c_uni]`` (either may be None) -- whose weights are the
# source rows ``w`` ``[k, k, c_in, c_out]`` and the context rows ``w_ctx`` ``[k, k, c_cell + c_uni, c_out]``; and the window loss.
# ---------------------------------------------------------------------------------------------
def _context(ctx_cell: Optional[torch.Tensor], ctx_uniform: Optional[torch.Tensor], n: int):
    """(c_cell, c_uni) of a checked context."""
    c_cell = c_uni = 0
    if ctx_cell is not None:
        c_cell = int(ctx_cell.shape[-1]) if ctx_cell.dim() == 4 else 0
        _dense_weight(ctx_cell, "ctx_cell", (6, n, n, max(c_cell, 1)))
    if ctx_uniform is not None:
        c_uni = int(ctx_uniform.numel())
        _vec(ctx_uniform, "ctx_uniform", max(c_uni, 1))
    return c_cell, c_uni


def cyclegan_train_conv_context(x, w: torch.Tensor, w_ctx: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                                ctx_cell: Optional[torch.Tensor], ctx_uniform: Optional[torch.Tensor], y, n_samples: int, n: int,
                                c_in: int, c_out: int, k: int, halo: bool) -> None:
    """``y = conv(x~ || ctx~, w || w_ctx) + bias``: ``fv3hip_cyclegan_conv_context`` without a loader transform."""
    tensors = [t for t in (w_ctx, bias, ctx_cell, ctx_uniform) if t is not None]
    dev = _require_device(x.tensor, w, y.tensor, *tensors)
    code, mode, _ = _cyclegan_geometry("regular", n, halo)
    c_cell, c_uni = _context(ctx_cell, ctx_uniform, n)
    _cyclegan_weight(w, "w", "regular", k, c_in, c_out)
    if w_ctx is not None:
        _cyclegan_weight(w_ctx, "w_ctx", "regular", k, c_cell + c_uni, c_out)
    _lib.call_on(dev, "fv3hip_cyclegan_conv_context", *_cube_slice(x, "x", n_samples, n, c_in), None, None, None, 0, _ptr(w),
                 _ptr(_vec(bias, "bias", c_out)), None, *_cube_slice(y, "y", n_samples, n, c_out), n_samples, n, c_in, c_out, code, int(k),
                 mode, _ptr(ctx_cell), c_cell, _ptr(ctx_uniform), c_uni, _ptr(w_ctx), _stream(dev))


def cyclegan_train_backward_weight_context_workspace_floats(n_samples: int, n: int, c_in: int, c_cell: int, c_uni: int, c_out: int,
                                                            k: int) -> int:
    return int(_lib.load().fv3hip_cyclegan_train_backward_weight_context_workspace_bytes(int(n_samples), int(n), int(c_in), int(c_cell),
                                                                                         int(c_uni), int(c_out), int(k))) // 4


def cyclegan_train_backward_weight_context(x, dy, ctx_cell: Optional[torch.Tensor], ctx_uniform: Optional[torch.Tensor], dw: torch.Tensor,
                                           dw_ctx: Optional[torch.Tensor], db: Optional[torch.Tensor], n_samples: int, n: int, c_in: int,
                                           c_out: int, k: int, halo: bool, workspace: torch.Tensor, kind: str = "regular") -> None:
    """``dw`` and ``dw_ctx`` (the context rows, None without a context) in the forward's layouts and ``db = sum dy`` (or None),
    all overwritten.  Only the regular ``kind`` takes a context."""
    tensors = [t for t in (ctx_cell, ctx_uniform, dw_ctx, db) if t is not None]
    dev = _require_device(x.tensor, dy.tensor, dw, workspace, *tensors)
    code, mode, n_out = _cyclegan_geometry(kind, n, halo)
    c_cell, c_uni = _context(ctx_cell, ctx_uniform, n)
    _cyclegan_weight(dw, "dw", kind, k, c_in, c_out)
    if dw_ctx is not None:
        _dense_weight(dw_ctx, "dw_ctx", (dw.shape[0], dw.shape[1], c_cell + c_uni, c_out))
    ws, ws_bytes = _caller_workspace(workspace)
    _lib.call_on(dev, "fv3hip_cyclegan_train_backward_weight_context", *_cube_slice(x, "x", n_samples, n, c_in),
                 *_cube_slice(dy, "dy", n_samples, n_out, c_out), _ptr(ctx_cell), c_cell, _ptr(ctx_uniform), c_uni, _ptr(dw), _ptr(dw_ctx),
                 _ptr(_vec(db, "db", c_out)), _ptr(ws), ws_bytes, n_samples, n, c_in, c_out, code, int(k), mode, _stream(dev))


FMR_LOSS_KINDS = {"mse": _lib.FMR_LOSS_MSE, "mae": _lib.FMR_LOSS_MAE}


def fmr_loss_grad(fake: torch.Tensor, real: torch.Tensor, dgan: Optional[torch.Tensor], dfake: Optional[torch.Tensor],
                  identity_kind: str, identity_weight: float, target_kind: str, target_weight: float,
                  values: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The window loss of the recurrent generator and its gradient in one launch (``fv3hip_fmr_loss_grad``).  ``fake`` and
    ``real``: float32 ``[window, time, ...]`` tensors or permuted views of ``[time, window, ...]`` ones whose states (the
    trailing dimensions) are contiguous; ``dgan`` (or None) and ``dfake`` (None: the values only) with ``fake``'s shape and
    strides.  Returns ``values``, two float64 on the device: the weighted identity loss (time 0) and target loss (times 1 ...)."""
    tensors = [t for t in (dgan, dfake, values, workspace) if t is not None]
    dev = _require_device(fake, real, *tensors)
    if fake.dim() < 3 or fake.shape != real.shape:
        raise ValueError(f"fake and real must be [window, time, ...] of one shape, got {tuple(fake.shape)} and {tuple(real.shape)}")
    W, T, E = int(fake.shape[0]), int(fake.shape[1]), _prod(fake.shape[2:])
    for t, what in ((fake, "fake"), (real, "real"), (dgan, "dgan"), (dfake, "dfake")):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.shape != fake.shape or not (t[0, 0].is_contiguous() if W and T else True):
            raise ValueError(f"{what} must be float32 of shape {tuple(fake.shape)} with contiguous states")
        if what.startswith("d") and t.stride()[:2] != fake.stride()[:2]:
            raise ValueError(f"{what} must have fake's strides {fake.stride()[:2]}, got {t.stride()[:2]}")
    for kind in (identity_kind, target_kind):
        if kind not in FMR_LOSS_KINDS:
            raise ValueError(f"unknown loss kind {kind!r}: 'mse' and 'mae' are built")
    need = int(_lib.load().fv3hip_fmr_loss_grad_workspace_bytes(W, T, E)) // 8
    if values is None:
        values = torch.empty(2, dtype=torch.float64, device=dev)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.float64, device=dev)
    for t, what, count in ((values, "values", 2), (workspace, "workspace", None)):
        if t.dtype != torch.float64 or not t.is_contiguous() or (count is not None and t.numel() != count):
            raise ValueError(f"{what} must be a contiguous float64 tensor" + (f" of {count} values" if count else ""))
    _lib.call_on(dev, "fv3hip_fmr_loss_grad", _ptr(fake), fake.stride(0), fake.stride(1), _ptr(real), real.stride(0), real.stride(1),
                 _ptr(dgan), _ptr(dfake), W, T, E, FMR_LOSS_KINDS[identity_kind], float(identity_weight), FMR_LOSS_KINDS[target_kind],
                 float(target_weight), _ptr(values), _ptr(workspace), workspace.numel() * 8, _stream(dev))
    return values


class HipTimer:
    """HIP events recorded on torch's current stream (used by bench.py)."""

    def __init__(self):
        self._h = ctypes.c_void_p()
        _lib.call("fv3hip_timer_create", ctypes.byref(self._h))

    def start(self, dev=None):
        _lib.call_on(dev, "fv3hip_timer_start", self._h, _stream(dev))

    def stop(self, dev=None):
        _lib.call_on(dev, "fv3hip_timer_stop", self._h, _stream(dev))

    def elapsed_ms(self) -> float:
        ms = ctypes.c_float()
        _lib.call("fv3hip_timer_elapsed_ms", self._h, ctypes.byref(ms))
        return float(ms.value)

    def __del__(self):
        try:
            _lib.load().fv3hip_timer_destroy(self._h)
        except Exception:
            pass


def device_info() -> dict:
    info = _lib.DeviceInfo()
    _lib.call("fv3hip_device_info", ctypes.byref(info))
    return {
        "name": info.name.decode(),
        "arch": info.arch.decode(),
        "compute_units": info.compute_units,
        "wavefront_size": info.wavefront_size,
        "lds_bytes_per_cu": info.lds_bytes_per_cu,
        "clock_mhz": info.clock_mhz,
        "hbm_bytes": int(info.hbm_bytes),
    }


def as_numpy(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy()
