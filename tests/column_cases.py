"""Inputs shared by tests/test_host_columns.py (which pins the numpy references of tests/column_np.py on them) and
tests/test_gpu_column_edges.py (which runs the column kernels of csrc/vertical.hip on them): pressures on the surface pressure
and one float next to it, NaN, +-inf and +-0 in every operand of a comparison, the sizes around one 256-thread block and shapes
past the 16384-block cap of the grid-stride loops."""
import functools
import math

import numpy as np

import column_np
from glue_cases import COLUMNS, PAST_THE_CAP_SHAPE as PAST_THE_CAP_TOTAL_SHAPE  # (3, 7, 199741): > 16384 * 256 elements

TOA = 300.0
NZS = (1, 2, 79)
PAST_THE_CAP_COLUMNS_SHAPE = (3, 2, 1398187)   # 4194561 columns > 16384 blocks of 256; z in the middle
PAST_THE_CAP_MASK_SHAPE = (1, 3, 1398187)      # (n_batch, nz, n_inner): 4194561 mask cells, n_inner % 4 != 0
assert 3 * 1398187 > 256 * 64 * 256 and 1398187 % 4 != 0

PS_SPECIALS = (101325.0, 0.0, -0.0, np.nan, np.inf)
WEIGHT_SPECIALS = (0.75, np.nan, np.inf, -0.0, 0.0)
N_LEVEL_KINDS = 8   # of _around
N_BLEND_P_KINDS = 9


def layouts(nz):
    """(shape, z_axis): z in the middle (outer and inner extents both > 1), then z first and z last with column counts
    around one 256-thread block and several blocks."""
    return [((3, nz, 5, 7), 1)] + [((nz, cols), 0) for cols in COLUMNS] + [((cols, nz), 1) for cols in COLUMNS]


def _around(ps):
    """The 8 levels to compare with ``ps``: on it, one float above and below it, NaN, +-inf, +-0."""
    T = ps.dtype.type
    full = lambda v: np.full(ps.shape, v, ps.dtype)
    return [ps, np.nextafter(ps, T(np.inf)), np.nextafter(ps, T(-np.inf)), full(np.nan), full(np.inf), full(-np.inf), full(0.0),
            full(-0.0)]


def n_special_columns(nz, kinds=N_LEVEL_KINDS):
    """Columns it takes until every (level kind, pair of the 5 x 5 per-column specials) has occurred, nz kinds per column."""
    return 25 * math.ceil(kinds / nz)


def mask_case(tw, tp, n_batch, nz, n_inner, extrapolate, w_repeat=1):
    """(weights [n_batch / w_repeat, n_inner], p_cmp [n_batch, cmp_levels, n_inner], p_fine [n_batch, nz + 1, n_inner],
    cmp_offset).  Column j = b * n_inner + c takes surface pressure ``PS_SPECIALS[j // 5 % 5]``, weight
    ``WEIGHT_SPECIALS[j % 5]`` and, at level k, kind ``(j // 25 * nz + k + j % 25) % 8`` of ``_around``: with
    ``w_repeat == 1`` every (level, ps, weight) triple occurs within the first ``n_special_columns(nz)`` columns.  The columns
    after those are random with pressures on either side of their surface pressure.  The levels that the kernels must not read
    hold other values."""
    assert n_batch % w_repeat == 0
    rng = np.random.default_rng(13 * nz + n_inner + 1000 * n_batch)
    cmp_levels, off = (nz, 0) if extrapolate else (nz + 1, 1)
    n_special = n_special_columns(nz)
    j = np.arange(n_batch * n_inner).reshape(n_batch, n_inner)
    special = j < n_special
    ps = np.where(special, np.array(PS_SPECIALS, tp)[j // 5 % 5], rng.uniform(9e4, 1.05e5, j.shape).astype(tp))
    p_fine = rng.uniform(100, 9e4, (n_batch, nz + 1, n_inner)).astype(tp)
    p_fine[:, nz] = ps
    kind = (j[:, None, :] // 25 * nz + np.arange(nz)[None, :, None] + j[:, None, :] % 25) % N_LEVEL_KINDS
    ps3 = np.ascontiguousarray(np.broadcast_to(ps[:, None, :], kind.shape))
    level = np.where(special[:, None, :], np.choose(kind, _around(ps3)), rng.uniform(8e4, 1.1e5, kind.shape).astype(tp))
    p_cmp = rng.uniform(8e4, 1.1e5, (n_batch, cmp_levels, n_inner)).astype(tp)
    p_cmp[:, off:off + nz] = level
    jw = np.arange(n_batch // w_repeat * n_inner).reshape(n_batch // w_repeat, n_inner)
    weights = np.where(jw < n_special, np.array(WEIGHT_SPECIALS, tw)[jw % 5], rng.uniform(0.5, 1, jw.shape).astype(tw))
    return np.ascontiguousarray(weights.astype(tw)), p_cmp, p_fine, off


def mask_triples(n_batch, nz, n_inner):
    """The (level kind, ps index, weight index) triples that ``mask_case`` (w_repeat == 1) lays out: 8 x 5 x 5 = 200 once it
    has ``n_special_columns(nz)`` columns."""
    n = min(n_batch * n_inner, n_special_columns(nz))
    return {((j // 25 * nz + k + j % 25) % N_LEVEL_KINDS, j // 5 % 5, j % 5) for j in range(n) for k in range(nz)}


GENERIC_INNER, ROWS_INNER = (1, 3, 1030), (4, 1020, 1024, 1028)   # n_inner % 4 != 0 (or one column) / whole quads
# (n_batch, nz, n_inner) with enough columns for every triple: nz = 3 at every n_inner, then nz = 1 on either kernel
MASK_TABLE_SHAPES = [(max(2, math.ceil(n_special_columns(3) / n)), 3, n) for n in GENERIC_INNER + ROWS_INNER] + [(67, 1, 3), (50, 1, 4)]
CONSTANT_PAIRS, CONSTANT_NZ, CONSTANT_Q_MAX = 1000, 8, (1.0, 0.03)

COARSE_SHAPES = [  # (ny, nx, factor)
    (8, 8, 2),      # plain kernel: factor < 4
    (8, 8, 4),      # quads, each inside one coarse column
    (12, 12, 6),    # quads that straddle two coarse columns at offsets 4 and 2
    (10, 20, 5),    # ... at every offset 1..4
    (24, 48, 12),   # quads over two workgroups in x (1152 columns)
    (9, 12, 4),     # staggered y with quads
    (8, 9, 4),      # staggered x: plain kernel
    (5, 5, 2),      # both staggered
]


def coarse_extent(n, f):
    return (n - 1) // f + 1 if n % 2 else n // f


def coarse_mask_case(tw, tp, n_batch, nz, ny, nx, f, extrapolate, w_repeat=1):
    """(weights [n_batch / w_repeat, ny, nx], p_cmp_coarse [n_batch, cmp_levels, nyc, nxc], p_fine [n_batch, nz + 1, ny, nx],
    cmp_offset).  The coarse levels cycle through PS_SPECIALS so that neighbouring coarse columns and levels differ; fine cell
    i takes as its surface pressure kind ``i % 9`` of (``_around`` + one ordinary pressure) of level ``i // 9 % nz`` of ITS
    coarse column: ties, neighbours and NaNs sit next to cells of the neighbouring coarse column that relate differently to
    theirs."""
    assert n_batch % w_repeat == 0
    rng = np.random.default_rng(ny * nx + f)
    cmp_levels, off = (nz, 0) if extrapolate else (nz + 1, 1)
    nyc, nxc = coarse_extent(ny, f), coarse_extent(nx, f)
    jc = np.arange(n_batch * cmp_levels * nyc * nxc).reshape(n_batch, cmp_levels, nyc, nxc)
    xc = jc % nxc
    p_cmp = np.array(PS_SPECIALS + (98000.0, 101000.0), tp)[(jc // nxc + 3 * xc + jc // (nyc * nxc)) % 7]
    p_cmp = np.where(rng.random(jc.shape) < 0.2, rng.uniform(9e4, 1.1e5, jc.shape), p_cmp).astype(tp)
    cy, cx = np.minimum(np.arange(ny) // f, nyc - 1), np.minimum(np.arange(nx) // f, nxc - 1)
    mine = p_cmp[:, off:off + nz][:, :, cy][:, :, :, cx]                    # [n_batch, nz, ny, nx]: the levels of each cell's column
    i = np.arange(n_batch * ny * nx).reshape(n_batch, ny, nx)
    base = np.take_along_axis(mine, (i // 9 % nz)[:, None], axis=1)[:, 0]
    ps = np.choose(i % 9, _around(np.ascontiguousarray(base)) + [np.full(base.shape, 100500.0, tp)])
    p_fine = rng.uniform(100, 9e4, (n_batch, nz + 1, ny, nx)).astype(tp)
    p_fine[:, nz] = ps
    iw = np.arange(n_batch // w_repeat * ny * nx).reshape(n_batch // w_repeat, ny, nx)
    weights = np.where(iw % 7 < 5, np.array(WEIGHT_SPECIALS, tw)[iw % 5], rng.uniform(0.5, 1, iw.shape).astype(tw)).astype(tw)
    return np.ascontiguousarray(weights), np.ascontiguousarray(p_cmp), p_fine, off


def blend_case(dtype, shape, z_axis):
    """(blending_pressure, ps_coarse, pfull_coarse).  Column j takes ``pb = PB[j % 5]`` and ``ps = PS[j // 5 % 5]`` -- an
    ordinary pair, ``ps == pb`` (a zero denominator), NaN and +-inf in either -- and, at level k, ``p`` of kind
    ``(j // 25 * nz + k + j % 25) % 9``: on ``pb``, one float above and below it, on ``ps`` (a zero numerator), an ordinary
    pressure in between, NaN, +-inf and -0 (against ``pb = +0``).  Later columns are ordinary with ``p`` on either side of
    ``pb``."""
    T = np.dtype(dtype).type
    nz = shape[z_axis]
    flat = shape[:z_axis] + shape[z_axis + 1:]
    ncol = int(np.prod(flat))
    rng = np.random.default_rng(31 * nz + ncol)
    j = np.arange(ncol)
    special = j < n_special_columns(nz, N_BLEND_P_KINDS)
    ps_r = rng.uniform(9.5e4, 1.03e5, ncol)
    pb = np.where(special, np.array([91192.5, np.nan, np.inf, -np.inf, 0.0], dtype)[j % 5], (0.9 * ps_r).astype(dtype)).astype(dtype)
    ps = np.where(special, np.array([101325.0, 91192.5, np.nan, np.inf, -np.inf], dtype)[j // 5 % 5], ps_r.astype(dtype)).astype(dtype)
    kind = (j[None, :] // 25 * nz + np.arange(nz)[:, None] + j[None, :] % 25) % N_BLEND_P_KINDS
    pb2, ps2 = (np.ascontiguousarray(np.broadcast_to(a, kind.shape)) for a in (pb, ps))
    full = lambda v: np.full(kind.shape, v, dtype)
    table = [pb2, np.nextafter(pb2, T(np.inf)), np.nextafter(pb2, T(-np.inf)), ps2, full(95000.0), full(np.nan), full(np.inf),
             full(-np.inf), full(-0.0)]
    p = np.where(special[None, :], np.choose(kind, table), rng.uniform(300, 1.03e5, kind.shape).astype(dtype)).astype(dtype)
    back = lambda x: np.ascontiguousarray(np.moveaxis(x.reshape((nz,) + flat), 0, z_axis))
    return pb.reshape(flat), ps.reshape(flat), back(p)


NAN_COLUMN, INF_COLUMN = 1, 2   # (where a case has at least 3 columns)


def column_fields(dtype, shape, z_axis, thin=False):
    """dict of delp, t, q, dz [shape] and phis [shape without z].  ``delp`` in U(300, 1500) under a 300 Pa top -- ``thin``:
    U(1, 50), the first layer 9e4 Pa -- and, where there are 3 columns, column 1 with a NaN and column 2 with an
    infinity at level nz // 2."""
    nz = shape[z_axis]
    flat = shape[:z_axis] + shape[z_axis + 1:]
    ncol = int(np.prod(flat))
    rng = np.random.default_rng(17 * nz + ncol)
    delp = rng.uniform(1, 50, (nz, ncol)) if thin else rng.uniform(300, 1500, (nz, ncol))
    if thin:
        delp[0] = 9e4
    if ncol >= 3:
        delp[nz // 2, NAN_COLUMN], delp[nz // 2, INF_COLUMN] = np.nan, np.inf
    back = lambda x: np.ascontiguousarray(np.moveaxis(x.reshape((nz,) + flat), 0, z_axis).astype(dtype))
    return dict(delp=back(delp), t=back(rng.uniform(200, 320, (nz, ncol))), q=back(rng.uniform(0, 0.025, (nz, ncol))),
                dz=back(rng.uniform(-2000, -50, (nz, ncol))), phis=rng.uniform(0, 3e4, flat).astype(dtype))


def as_columns(x, z_axis):
    """[nz, ncol] view-or-copy of an array with its z axis at ``z_axis``."""
    x = np.moveaxis(np.asarray(x), z_axis, 0)
    return x.reshape(x.shape[0], -1)


@functools.lru_cache(maxsize=None)
def past_the_cap_delp():
    """float32 delp of PAST_THE_CAP_COLUMNS_SHAPE (34 MB), built once; treat as read-only."""
    rng = np.random.default_rng(5)
    x = rng.uniform(300, 1500, PAST_THE_CAP_COLUMNS_SHAPE).astype(np.float32)
    x.setflags(write=False)
    return x


def virtual_constant_pairs(n_pairs, nz, q_max):
    """float32 (t, q, delp) [nz, 2 * n_pairs] for the differential test of the virtual-temperature constant: column 2i has
    ``q`` in U(0, q_max); column 2i + 1 shares its delp and has ``t' = float32(t * (1 + float32(Rv / Rd - 1) * q))``, ``q' = 0``,
    so that a kernel with the reference's constant gives both columns the same virtual temperature, bit for bit.  Also the
    number of pairs in which the float32 quotient ``float32(Rv) / float32(Rd) - 1`` gives another virtual temperature."""
    f = np.float32
    rng = np.random.default_rng(n_pairs + int(1000 * q_max))
    t = rng.uniform(200, 320, (nz, n_pairs)).astype(f)
    q = rng.uniform(0, q_max, (nz, n_pairs)).astype(f)
    dp = rng.uniform(300, 1500, (nz, n_pairs)).astype(f)
    tv = column_np.virtual_temperature(t, q)
    tv_quotient = t * (f(1) + (f(column_np.RVGAS) / f(column_np.RDGAS) - f(1)) * q)
    assert tv.dtype == f and tv_quotient.dtype == f
    pair = lambda a, b: np.ascontiguousarray(np.stack([a, b], axis=2).reshape(nz, 2 * n_pairs))
    return pair(t, tv), pair(q, np.zeros_like(q)), pair(dp, dp), int(np.count_nonzero((tv != tv_quotient).any(axis=0)))
