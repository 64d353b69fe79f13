"""Specs, inputs and CPU evaluations of the CycleGAN tests: weights drawn as N(0, 1 / fan_in), the state as N(0, 1).

The float64 truth of a whole generator is ``GeneratorTwin`` converted with ``.double()`` (``lon`` and ``xyz`` too), fed the
float32 seconds as float64; the float32 chain is the same twin as it is.  Single layers are torch's ``conv2d`` /
``conv_transpose2d`` (+ crop) on ``append_halos_tensor``-padded or zero-padded input.
"""
import numpy as np
import torch

F = torch.nn.functional


def synthetic_grid(nx):
    """Cell centres of an equidistant gnomonic cube: ``lon`` ``[6, nx, nx]`` and unit vectors ``xyz`` ``[6, 3, nx, nx]``, float32."""
    a = (np.arange(nx) + 0.5) / nx * 2 - 1
    u, v = np.meshgrid(a, a, indexing="ij")
    one = np.ones_like(u)
    faces = [(one, u, v), (-u, one, v), (-u, v, one), (-one, v, -u), (-v, -one, -u), (-v, u, -one)]
    xyz = np.stack([np.stack(f, axis=0) for f in faces])
    xyz = xyz / np.linalg.norm(xyz, axis=1, keepdims=True)
    return np.mod(np.arctan2(xyz[:, 1], xyz[:, 0]), 2 * np.pi).astype(np.float32), xyz.astype(np.float32)


def make_generator(rng, channels, nx, n_convolutions, n_resnet, max_filters, kernel_size=3, bias=True, features=True, embedded=False):
    from fv3net_amd.cyclegan import GeneratorSpec, layer_plan, weight_shape

    weights, biases = {}, {}
    for name, kind, ci, co, k, _ in layer_plan(channels, n_convolutions, n_resnet, kernel_size, max_filters, features):
        taps = 4 if kind == "transposed" else k * k
        weights[name] = (rng.normal(0, 1, weight_shape(kind, ci, co, k)) / np.sqrt(ci * taps)).astype(np.float32)
        biases[name] = rng.normal(0, 0.1, co).astype(np.float32)
    m = int(max_filters / 2 ** n_convolutions)
    geo = lambda c: rng.normal(0, 0.3, (6, c, nx, nx)).astype(np.float32)
    lon, xyz = synthetic_grid(nx) if features else (None, None)
    return GeneratorSpec(channels, nx, weights, biases, n_convolutions, n_resnet, kernel_size, 4, max_filters,
                         geo(channels) if bias else None, geo(channels) if bias else None, geo(m) if embedded else None, lon, xyz)


def make_spec(rng, variables, nx, n_convolutions, n_resnet, max_filters, convolution_type="halo_conv2d", **flags):
    """``variables``: name -> feature count.  Both generators, and scalers as a temperature-like and a humidity-like field."""
    from fv3net_amd.cyclegan import CycleGanSpec

    channels = sum(variables.values())
    gens = [make_generator(rng, channels, nx, n_convolutions, n_resnet, max_filters, **flags) for _ in range(2)]
    scalers = {f"{d}_{name}": (rng.normal(0, 10, nf), rng.uniform(0.5, 2, nf) * 10.0 ** rng.integers(-3, 2))
               for d in "ab" for name, nf in variables.items()}
    return CycleGanSpec(gens[0], gens[1], list(variables.items()), scalers, convolution_type)


def make_dataset(rng, spec, n_times, dtype=np.float64, order=("time", "tile", "x", "y", "z"), domain="a"):
    """name -> (dims, array) of raw fields stored in the dim order ``order`` (a one-feature variable has no ``z``), and the
    times as float64 seconds since 1970, some hours apart."""
    n, out = spec.generator_a_to_b.nx, {}
    for name, nf in spec.variables:
        mean, std = spec.scalers[f"{domain}_{name}"]
        a = rng.normal(0, 1, (n_times, 6, n, n, nf)) * std + mean
        dims = list(order)
        if nf == 1:
            a, dims = a[..., 0], [d for d in order if d != "z"]
        canon = [d for d in ("time", "tile", "x", "y", "z") if d in dims]
        out[name] = (tuple(dims), np.ascontiguousarray(np.transpose(a.astype(dtype), [canon.index(d) for d in dims])))
    return out, 1.7e9 + 977 + 7 * 3600.0 * np.arange(n_times)


def canonical(dataset):
    out = {}
    for name, (dims, a) in dataset.items():
        canon = [d for d in ("time", "tile", "x", "y", "z") if d in dims]
        out[name] = np.transpose(a, [dims.index(d) for d in canon])
    return out


def pack(spec, arrays, domain="a"):
    """numpy's ``pack_to_tensor``: ``float32((x - mean) / std)`` in float64, ``[time, 6, n, n, F]``."""
    cols = []
    for name, nf in spec.variables:
        a = np.asarray(arrays[name], np.float64)
        mean, std = spec.scalers[f"{domain}_{name}"]
        cols.append((a if a.ndim == 5 else a[..., None]) - mean)
        cols[-1] = cols[-1] / std
    return np.concatenate(cols, axis=-1).astype(np.float32)


def unpack(spec, state, domain="b"):
    """numpy's ``unpack_tensor``: ``float64(state) * std + mean`` per variable (no ``z`` for a one-feature variable)."""
    out, f0 = {}, 0
    for name, nf in spec.variables:
        mean, std = spec.scalers[f"{domain}_{name}"]
        a = np.asarray(state[..., f0:f0 + nf], np.float64) * std + mean
        out[name] = a[..., 0] if nf == 1 else a
        f0 += nf
    return out


def twin_forward(generator, convolution_type, state, seconds, dtype=torch.float32):
    """The plain-torch twin on the CPU: ``state`` ``[S, 6, n, n, C]`` float32 (numpy) and float32 seconds -> ``[S, 6, n, n, C]``."""
    from fv3net_amd.fit.cyclegan import twin_from_spec

    twin = twin_from_spec(generator, convolution_type, dtype)
    x = torch.from_numpy(np.ascontiguousarray(state)).to(dtype).permute(0, 1, 4, 2, 3)
    t = torch.from_numpy(np.asarray(seconds, np.float32)).to(dtype)
    with torch.no_grad():
        return twin(t, x).permute(0, 1, 3, 4, 2).contiguous().numpy()


def worst_ratio(got, truth):
    got, truth = np.asarray(got, np.float64).reshape(-1, got.shape[-1]), np.asarray(truth, np.float64).reshape(-1, truth.shape[-1])
    scale = np.max(np.abs(truth), axis=0)
    return float(np.max(np.max(np.abs(got - truth), axis=0) / np.where(scale == 0, 1, scale)))


# -- single layers ---------------------------------------------------------------------------------
def pad(t, h, halo):
    """``[S, 6, c, n, n]`` padded by ``h`` cells from the neighbouring faces (``halo``) or with zeros."""
    from fv3net_amd.cubedsphere.halos import append_halos_tensor

    return append_halos_tensor(t.movedim(1, 0), h).movedim(0, 1) if halo else F.pad(t, (h, h, h, h))


def torch_layer(kind, k, halo, x, w, bias, transform=None, dtype=torch.float32):
    """One layer on the CPU.  ``x`` ``[S, 6, n, n, c]`` numpy, ``w`` in torch's layout; ``transform`` = (mean ``[S, 6, c]``,
    rstd, bias ``[6, n, n, c]`` or None, relu), applied before padding.  Returns ``[S, 6, n_out, n_out, c_out]``."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    if transform is not None:
        mean, rstd, cell_bias, relu = transform
        t = (t - torch.from_numpy(mean).to(dtype)[:, :, None, None]) * torch.from_numpy(rstd).to(dtype)[:, :, None, None]
        if cell_bias is not None:
            t = t + torch.from_numpy(cell_bias).to(dtype)
        if relu:
            t = torch.relu(t)
    S, _, n, _, c = t.shape
    h = 1 if k == 4 else (k - 1) // 2
    p = pad(t.permute(0, 1, 4, 2, 3), h, halo).reshape(S * 6, c, n + 2 * h, n + 2 * h)
    w, b = torch.from_numpy(np.ascontiguousarray(w)).to(dtype), None if bias is None else torch.from_numpy(bias).to(dtype)
    if kind == "transposed":
        y = F.conv_transpose2d(p, w, b, stride=2)[..., 3:-3, 3:-3]
    else:
        y = F.conv2d(p, w, b, stride=2 if kind == "strided" else 1)
    return y.reshape(S, 6, y.shape[1], y.shape[2], y.shape[3]).permute(0, 1, 3, 4, 2).contiguous().numpy()


SENTINEL = -7.0   # what every destination buffer is filled with before a launch


def gapped(x, off=0, width=None, gap=0, lead=0, fill=np.nan):
    """``x`` ``[S, 6, n, n, c]`` laid out for a launch: a flat float32 buffer filled with ``fill`` in which sample ``s``'s cube
    starts at ``lead + s * (cube + gap)`` and ``x`` sits at channel ``off`` of rows ``width`` wide.  Returns (buffer, ld, stride)."""
    S, _, n, _, c = x.shape
    ld = width or c + off
    cube = 6 * n * n * ld
    buf = np.full(lead + S * (cube + gap), fill, np.float32)
    buf[lead:].reshape(S, cube + gap)[:, :cube].reshape(S, 6, n, n, ld)[..., off:off + c] = x
    return buf, ld, cube + gap


def split(buf, S, n, ld, gap=0, lead=0):
    """The inverse of ``gapped``: (the cubes ``[S, 6, n, n, ld]``, everything outside them as one flat array)."""
    buf = np.asarray(buf).reshape(-1)
    cube = 6 * n * n * ld
    inside = np.zeros(buf.size, bool)
    for s in range(S):
        inside[lead + s * (cube + gap):lead + s * (cube + gap) + cube] = True
    return buf[inside].reshape(S, 6, n, n, ld), buf[~inside]


def untouched(a, fill=SENTINEL):
    """Every element of ``a`` still holds the bits of ``fill``."""
    return bool(np.all(np.ascontiguousarray(a, np.float32).view(np.uint32) == np.float32(fill).view(np.uint32)))


def _up(device, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def _ptr(t, lead=0):
    return None if t is None else t.data_ptr() + 4 * lead


def device_layer(device, kind, k, halo, x, w, bias, transform=None, out_bias=None, src_off=0, src_width=None, dst_off=0, dst_width=None,
                 src_gap=0, dst_gap=0, src_lead=0, dst_lead=0, into=None):
    """One ``fv3hip_cyclegan_conv`` launch.  ``x`` sits at channel ``src_off`` of a NaN-filled buffer ``src_width`` wide, the
    result goes to channel ``dst_off`` of a buffer ``dst_width`` wide filled with the sentinel -7.  Returns that buffer (numpy).

    ``src_gap`` / ``dst_gap``: extra floats between consecutive samples (NaN on the source side, the sentinel on the destination
    side), ``src_lead`` / ``dst_lead``: floats in front of the first sample; the sample stride passed is then ``cube + gap``
    (0, for "contiguous", when there is neither a gap nor a lead) and the whole flat destination buffer is returned, to be taken
    apart with ``split``.  ``into``: a flat device tensor to write to in place of a fresh sentinel buffer."""
    from fv3net_amd import _lib
    from fv3net_amd.cyclegan import KINDS, split_transposed_weight
    from fv3net_amd.ops import _stream

    S, _, n, _, c = x.shape
    c_out = w.shape[1] if kind == "transposed" else w.shape[0]
    n_out = {"regular": n, "strided": n // 2, "transposed": 2 * n}[kind]
    wide, src_ld, src_ss = gapped(x, src_off, src_width, src_gap, src_lead)
    flat, dst_ld, dst_ss = gapped(np.full((S, 6, n_out, n_out, c_out), SENTINEL, np.float32), dst_off, dst_width, dst_gap, dst_lead, SENTINEL)
    src, dst = _up(device, wide), _up(device, flat) if into is None else into
    wk = _up(device, split_transposed_weight(w) if kind == "transposed" else np.asarray(w).transpose(2, 3, 1, 0))
    mean, rstd, cell_bias, relu = transform or (None, None, None, False)
    held = [_up(device, a) for a in (mean, rstd, cell_bias, bias, out_bias)]
    plain = lambda gap, lead, t: t is None and gap == 0 and lead == 0
    _lib.call_on(device, "fv3hip_cyclegan_conv", _ptr(src, src_lead), src_ld, src_off, 0 if plain(src_gap, src_lead, None) else src_ss,
                 _ptr(held[0]), _ptr(held[1]), _ptr(held[2]), int(relu), wk.data_ptr(), _ptr(held[3]), _ptr(held[4]), _ptr(dst, dst_lead),
                 dst_ld, dst_off, 0 if plain(dst_gap, dst_lead, into) else dst_ss, S, n, c, c_out, KINDS[kind], k,
                 _lib.CYCLEGAN_HALO_CUBE if halo else _lib.CYCLEGAN_HALO_ZEROS, _stream(device))
    torch.cuda.synchronize(device)
    out = dst.cpu().numpy()
    return out.reshape(S, 6, n_out, n_out, dst_ld) if plain(dst_gap, dst_lead, into) else out


def device_stats(device, x, eps=1e-5, src_off=0, src_width=None, src_gap=0):
    """``fv3hip_cyclegan_stats`` on ``x`` ``[S, 6, n, n, c]`` -> (mean, rstd) ``[S, 6, c]`` numpy.  ``x`` sits at channel
    ``src_off`` of a NaN-filled buffer ``src_width`` wide with ``src_gap`` NaNs between the samples."""
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    S, _, n, _, c = x.shape
    wide, ld, ss = gapped(x, src_off, src_width, src_gap)
    src = _up(device, wide)
    st = torch.full((2, S, 6, c), SENTINEL, dtype=torch.float32, device=device)
    _lib.call_on(device, "fv3hip_cyclegan_stats", src.data_ptr(), ld, src_off, ss if src_gap else 0, st[0].data_ptr(), st[1].data_ptr(), S, n,
                 c, eps, _stream(device))
    torch.cuda.synchronize(device)
    return st[0].cpu().numpy(), st[1].cpu().numpy()


def apply_np(x, mean=None, rstd=None, bias=None, relu=False, res=None, dtype=np.float32):
    """``fv3hip_cyclegan_apply``'s expression in numpy, every step rounded to ``dtype``, in the kernel's order:
    ``(v - mean) * rstd``, ``+ bias``, ReLU (``v < 0 ? 0 : v``: a NaN stays), ``+ res``.  ``x``, ``res`` ``[S, 6, n, n, c]``,
    ``mean``, ``rstd`` ``[S, 6, c]``, ``bias`` ``[6, n, n, c]``."""
    v = np.asarray(x, dtype)
    if mean is not None:
        v = (v - np.asarray(mean, dtype)[:, :, None, None]) * np.asarray(rstd, dtype)[:, :, None, None]
    if bias is not None:
        v = v + np.asarray(bias, dtype)
    if relu:
        v = np.where(v < 0, dtype(0), v)
    if res is not None:
        v = v + np.asarray(res, dtype)
    assert v.dtype == dtype
    return v


def device_apply(device, x, mean=None, rstd=None, bias=None, relu=False, res=None, src_off=0, src_width=None, src_gap=0, res_off=0,
                 res_width=None, res_gap=0, dst_off=0, dst_width=None, dst_gap=0, in_place=False, res_is_dst=False):
    """One ``fv3hip_cyclegan_apply`` launch.  ``x`` and ``res`` ``[S, 6, n, n, c]`` sit in NaN-filled buffers of their own
    (offset, width, gap as in ``device_layer``); the destination is a sentinel-filled one.  ``in_place``: the destination is the
    source slice itself (the ``dst_*`` arguments are ignored; what surrounds the slice is NaN).  ``res_is_dst``: the residual is
    what the destination slice holds before the launch (the ``res_*`` arguments are ignored; with ``in_place`` the residual is
    ``x`` itself and ``res`` is ignored too).  Returns ``split`` of the destination: (cubes ``[S, 6, n, n, ld]``, the gaps)."""
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    S, _, n, _, c = x.shape
    wide, src_ld, src_ss = gapped(x, src_off, src_width, src_gap)
    src = _up(device, wide)
    if in_place:
        dst, dst_ld, dst_off, dst_ss, dst_gap = src, src_ld, src_off, src_ss, src_gap
    else:
        first = res if res_is_dst else np.full(x.shape, SENTINEL, np.float32)
        flat, dst_ld, dst_ss = gapped(first, dst_off, dst_width, dst_gap, fill=SENTINEL)
        dst = _up(device, flat)
    if res_is_dst:
        rbuf, res_ld, res_off, res_ss, res_gap = dst, dst_ld, dst_off, dst_ss, dst_gap
    elif res is not None:
        flat, res_ld, res_ss = gapped(res, res_off, res_width, res_gap)
        rbuf = _up(device, flat)
    else:
        rbuf, res_ld, res_off, res_ss, res_gap = None, 0, 0, 0, 0
    held = [_up(device, a) for a in (mean, rstd, bias)]
    _lib.call_on(device, "fv3hip_cyclegan_apply", src.data_ptr(), src_ld, src_off, src_ss if src_gap else 0, _ptr(held[0]), _ptr(held[1]),
                 _ptr(held[2]), int(relu), _ptr(rbuf), res_ld, res_off, res_ss if res_gap else 0, dst.data_ptr(), dst_ld, dst_off,
                 dst_ss if dst_gap else 0, S, n, c, _stream(device))
    torch.cuda.synchronize(device)
    return split(dst.cpu().numpy(), S, n, dst_ld, dst_gap)


def device_input(device, x, bias=None, lon=None, xyz=None, theta=None, src_off=0, src_width=None, src_gap=0, dst_off=0, dst_width=None,
                 dst_gap=0):
    """One ``fv3hip_cyclegan_input`` launch.  The state ``x`` ``[S, 6, n, n, c]`` sits in a NaN-filled buffer, the ``c`` (with
    ``lon`` ``[6, n, n]``, ``xyz`` ``[6, n, n, 3]`` and ``theta`` ``[S]``: ``c + 5``) output channels go to channel ``dst_off`` of
    a sentinel-filled one.  Returns ``split`` of the destination: (cubes ``[S, 6, n, n, ld]``, the gaps)."""
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    S, _, n, _, c = x.shape
    wide, src_ld, src_ss = gapped(x, src_off, src_width, src_gap)
    c_out = c + (0 if lon is None else 5)
    flat, dst_ld, dst_ss = gapped(np.full((S, 6, n, n, c_out), SENTINEL, np.float32), dst_off, dst_width, dst_gap, fill=SENTINEL)
    src, dst = _up(device, wide), _up(device, flat)
    held = [_up(device, a) for a in (bias, lon, xyz, theta)]
    _lib.call_on(device, "fv3hip_cyclegan_input", src.data_ptr(), src_ld, src_off, src_ss if src_gap else 0, _ptr(held[0]), _ptr(held[1]),
                 _ptr(held[2]), _ptr(held[3]), dst.data_ptr(), dst_ld, dst_off, dst_ss if dst_gap else 0, S, n, c, _stream(device))
    torch.cuda.synchronize(device)
    return split(dst.cpu().numpy(), S, n, dst_ld, dst_gap)


def device_instance_norm(device, x, relu=False, residual=None, in_place=False):
    """Statistics + apply on the device: ``[S, 6, n, n, c]`` numpy -> the normalised array."""
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    S, _, n, _, c = x.shape
    src = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(device)
    st = torch.empty((2, S, 6, c), dtype=torch.float32, device=device)
    res = None if residual is None else torch.from_numpy(np.ascontiguousarray(residual, np.float32)).to(device)
    dst = src if in_place else torch.full_like(src, -7.0)
    stream = _stream(device)
    _lib.call_on(device, "fv3hip_cyclegan_stats", src.data_ptr(), c, 0, 0, st[0].data_ptr(), st[1].data_ptr(), S, n, c, 1e-5, stream)
    _lib.call_on(device, "fv3hip_cyclegan_apply", src.data_ptr(), c, 0, 0, st[0].data_ptr(), st[1].data_ptr(), None, int(relu),
                 None if res is None else res.data_ptr(), c, 0, 0, dst.data_ptr(), c, 0, 0, S, n, c, stream)
    torch.cuda.synchronize(device)
    return dst.cpu().numpy()


def torch_instance_norm(x, dtype=torch.float32):
    """``nn.InstanceNorm2d`` on the CPU, ``[S, 6, n, n, c]`` -> the same shape."""
    S, _, n, _, c = x.shape
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).permute(0, 1, 4, 2, 3).reshape(S * 6, c, n, n)
    y = torch.nn.InstanceNorm2d(c)(t)
    return y.reshape(S, 6, c, n, n).permute(0, 1, 3, 4, 2).contiguous().numpy()
