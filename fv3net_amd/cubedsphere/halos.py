"""n-cell halos of the cube faces: ``fv3fit._shared.halos.append_halos`` (external/fv3fit/fv3fit/_shared/halos.py:135-160),
the step that makes a convolutional model's prediction depend on the neighbouring faces.

Every tile is padded by ``n_halo`` cells on both sides of ``x`` and ``y``; the four edge strips are filled from the
neighbours and the four ``n_halo x n_halo`` corners stay zero.  Strip line ``d`` (0 next to the tile, growing outward) on
the low / high side of an axis is the neighbour's line ``d`` counted inward from the shared edge -- its last lines for the low
side, its first for the high side -- oriented along the edge as ``grid.halos_from_rows`` orients line 0: reversed when the
neighbour is joined through its other axis; neighbours as in ``grid.FV3_FACE_CONNECTIONS``.  The reference exchanges through
``pace.util``; its torch-only twin ``AppendHalos`` (fv3fit/pytorch/cyclegan/modules.py:425-543), which the reference's tests
hold equal to it, wrote ``tests/golden/append_halos_reference.npz``, and that fixture pins this rule.

Arrays here are ``[tile, ..., x, y]`` (the layout of the reference's ``[sample, x, y, z]`` networks; ``grid.py`` keeps
``[..., y, x]``).  Everything is array indexing, on whatever device the data lives: these are strips, ``4 h / n`` of the data.
The convolution kernel itself never sees a padded copy (``fv3hip_conv_predict`` reads the neighbours or the strips in place).
"""
import numpy as np
import torch

from ..xr_compat import DataArray, Dataset, from_compat, to_compat
from .grid import _ROW, FV3_FACE_CONNECTIONS

SIDES = (("x", 0), ("x", 1), ("y", 0), ("y", 1))  # strip order: x-low, x-high, y-low, y-high


def edge_strips(field: torch.Tensor, n_halo: int) -> torch.Tensor:
    """``[T, ..., n, n]`` (x, y last) -> ``[T, 4, n_halo, ..., n]``: the ``n_halo`` lines next to each of a tile's own four
    edges, in the order of ``ops.cube_edge_rows`` (x first, x last, y first, y last), line ``d`` counted inward from the edge,
    each running along the other axis.  This is what a rank contributes to ``parallel.exchange_edge_strips``."""
    n = field.shape[-1]
    if field.shape[-2] != n:
        raise ValueError(f"cube tiles are square, got {tuple(field.shape[-2:])}")
    if not 0 < n_halo <= n:
        raise ValueError(f"n_halo must be in [1, {n}], got {n_halo}")
    d = torch.arange(n_halo, device=field.device)
    rows = [field.index_select(-2, d), field.index_select(-2, n - 1 - d),
            field.index_select(-1, d).transpose(-1, -2), field.index_select(-1, n - 1 - d).transpose(-1, -2)]  # [T, ..., h, n]
    return torch.stack([r.movedim(-2, 1) for r in rows], dim=1)


def halo_strips(edges: torch.Tensor, tiles) -> torch.Tensor:
    """The halo of ``tiles`` picked from the edge strips of ALL six tiles (``edges`` ``[6, 4, h, ..., n]``):
    ``[len(tiles), 4, h, ..., n]``, side x-low, x-high, y-low, y-high, line 0 next to the tile, running along the tile's own
    other axis."""
    if edges.shape[0] != 6 or edges.shape[1] != 4:
        raise ValueError(f"edge strips of the six tiles are [6, 4, h, ..., n], got {tuple(edges.shape)}")
    out = []
    for t in tiles:
        sides = []
        for axis, high in SIDES:
            nbr, nbr_axis = FV3_FACE_CONNECTIONS[int(t)][axis][high]
            v = edges[nbr, _ROW[(nbr_axis, "first" if high else "last")]]
            sides.append(v if nbr_axis == axis else v.flip(-1))
        out.append(torch.stack(sides))
    return torch.stack(out)


def fill_halos(field: torch.Tensor, strips: torch.Tensor) -> torch.Tensor:
    """``field`` ``[T, ..., n, n]`` padded by the ``h`` lines of ``strips`` ``[T, 4, h, ..., n]``; corners zero."""
    h, n = strips.shape[2], field.shape[-1]
    out = torch.zeros(tuple(field.shape[:-2]) + (n + 2 * h, n + 2 * h), dtype=field.dtype, device=field.device)
    out[..., h:h + n, h:h + n] = field
    for d in range(h):
        out[..., h - 1 - d, h:h + n] = strips[:, 0, d]
        out[..., h + n + d, h:h + n] = strips[:, 1, d]
        out[..., h:h + n, h - 1 - d] = strips[:, 2, d]
        out[..., h:h + n, h + n + d] = strips[:, 3, d]
    return out


def append_halos_tensor(field: torch.Tensor, n_halo: int) -> torch.Tensor:
    """``[6, ..., n, n]`` (x, y last) -> ``[6, ..., n + 2 n_halo, n + 2 n_halo]``."""
    if field.shape[0] != 6:
        raise ValueError(f"the leading dimension must hold the six tiles of the cube, got {field.shape[0]}")
    if n_halo == 0:
        return field
    return fill_halos(field, halo_strips(edge_strips(field, n_halo), range(6)))


class _PaddedTile(torch.autograd.Function):
    """One tile of ``append_halos_tensor`` as an autograd node of its own: forward ``[6, ..., n, n] -> [..., n + 2 h, n + 2 h]``
    for tile ``t``; backward the tile's own cells and the four neighbours' strips it shows, zero elsewhere.  The tiles are
    dimension ``tile_dim`` of the input as it is given, so that the node hangs on the caller's tensor itself."""

    @staticmethod
    def forward(ctx, field, n_halo, t, tile_dim):
        field = field.movedim(tile_dim, 0)
        ctx.n_halo, ctx.t, ctx.tile_dim, ctx.meta = n_halo, t, tile_dim, (field.shape, field.dtype, field.device)
        return fill_halos(field[t:t + 1], halo_strips(edge_strips(field, n_halo), [t]))[0]

    @staticmethod
    def backward(ctx, d):
        h, t = ctx.n_halo, ctx.t
        shape, dtype, device = ctx.meta
        n = shape[-1]
        mid = slice(h, h + n)
        g = torch.zeros(shape, dtype=dtype, device=device)
        g[t] = d[..., mid, mid]
        lines = lambda pick: torch.stack([pick(dl) for dl in range(h)], dim=-2)   # noqa: E731  [..., h, n], line 0 next to the tile
        shown = [lines(lambda dl: d[..., h - 1 - dl, mid]), lines(lambda dl: d[..., h + n + dl, mid]),
                 lines(lambda dl: d[..., mid, h - 1 - dl]), lines(lambda dl: d[..., mid, h + n + dl])]
        for side, (axis, high) in enumerate(SIDES):
            nbr, nbr_axis = FV3_FACE_CONNECTIONS[t][axis][high]
            rows = shown[side] if nbr_axis == axis else shown[side].flip(-1)
            k = _ROW[(nbr_axis, "first" if high else "last")]    # the neighbour's edge strip (edge_strips): line d inward
            if k == 0:
                g[nbr][..., 0:h, :] = rows
            elif k == 1:
                g[nbr][..., n - h:n, :] = rows.flip(-2)
            elif k == 2:
                g[nbr][..., :, 0:h] = rows.transpose(-1, -2)
            else:
                g[nbr][..., :, n - h:n] = rows.flip(-2).transpose(-1, -2)
        return g.movedim(0, ctx.tile_dim), None, None, None


def append_halos_tensor_reference_order(field: torch.Tensor, n_halo: int, tile_dim: int = 0) -> torch.Tensor:
    """``append_halos_tensor`` (the same values; the tiles are dimension ``tile_dim`` of ``field`` and of the result) whose
    gradient reaches ``field`` as the reference's torch module ``AppendHalos`` (modules.py:425-543) sends it.

    A cell within ``n_halo`` of two edges is shown three times -- itself and once in the halo of each of two neighbours -- and a
    sum of three floats depends on which two are added first; a tensor that something else reads as well (the input of a
    residual block) gets a further term.  ``append_halos_tensor`` is a few batched gathers, so autograd adds a cell's own term,
    then the y sides', then the x sides', and hands the sum over as one term.  The reference builds tile after tile from
    slices of its input, so autograd adds, one by one and after whatever was created later, the terms of the tiles that show
    the cell (the cell's own tile for its own position) by descending tile number.  Here every padded tile is an autograd node
    of its own, created in tile order, which gives that order; the plain-torch twins pad with this function, and a float64
    training step of theirs then repeats the reference's bit for bit."""
    if field.shape[tile_dim] != 6:
        raise ValueError(f"dimension {tile_dim} must hold the six tiles of the cube, got {field.shape[tile_dim]}")
    if n_halo == 0:
        return field
    return torch.stack([_PaddedTile.apply(field, n_halo, t, tile_dim) for t in range(6)], dim=tile_dim)


def append_halos(ds, n_halo: int, x_dim: str = "x", y_dim: str = "y"):
    """``fv3fit._shared.halos.append_halos``: a dataset (or data array) with ``tile``, ``x`` and ``y`` dimensions and exactly six
    tiles, padded by ``n_halo`` along ``x`` and ``y``; coordinates are dropped; ``n_halo = 0`` returns the input.  A bare
    numpy array or torch tensor is taken as ``[6, ..., x, y]``."""
    if n_halo < 0:
        raise ValueError(f"n_halo must not be negative, got {n_halo}")
    if isinstance(ds, torch.Tensor):
        return append_halos_tensor(ds, n_halo)
    if isinstance(ds, np.ndarray):
        return append_halos_tensor(torch.from_numpy(np.ascontiguousarray(ds)), n_halo).numpy()
    if n_halo == 0:
        return ds
    d = to_compat(ds)
    single = isinstance(d, DataArray)
    arrays = {"__array__": d} if single else {name: d[name] for name in d}
    padded = {}
    for name, da in arrays.items():
        for dim in ("tile", x_dim, y_dim):
            if dim not in da.dims:
                raise ValueError(f"variable {name!r} must have tile, {x_dim} and {y_dim} dimensions to append halos")
        if da.sizes["tile"] != 6:
            raise ValueError(f"dataset must have exactly six tiles to append halos, got {da.sizes['tile']}")
        rest = [dim for dim in da.dims if dim not in ("tile", x_dim, y_dim)]
        order = ["tile"] + rest + [x_dim, y_dim]
        data = da.transpose(*order).data
        host = not isinstance(data, torch.Tensor)
        t = torch.from_numpy(np.ascontiguousarray(data)) if host else data
        res = append_halos_tensor(t, n_halo)
        out = DataArray(res.numpy() if host else res, dims=order, attrs=da.attrs, name=da.name)
        padded[name] = out.transpose(*da.dims)
    if single:
        return from_compat(padded["__array__"], ds)
    return from_compat(Dataset(padded, attrs=d.attrs), ds)
