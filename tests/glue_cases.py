"""Inputs shared by tests/test_host_glue.py (which pins the numpy references on them) and tests/test_gpu_glue_edges.py
(which runs the kernels on them): special values crossed with each other, the sizes around one 256-thread block and one
size past the 16384-block cap of the grid-stride loops."""
import numpy as np

SIZES = (1, 255, 256, 257)
PAST_THE_CAP = 256 * 64 * 256 + 257   # = 3 * 7 * 199741: more elements than 16384 blocks of 256 threads hold
PAST_THE_CAP_SHAPE = (3, 7, 199741)
COLUMNS = (1, 255, 256, 257, 1000)
SCALARS = (0.0, -1.5, 0.1, 1.0)       # zero, a negative one, one that float32 does not represent, the base of 1 ** nan


def specials(dtype, s):
    """NaN, +-inf, +-0, +-denormal, +-1, the scalar and its neighbours, both isclose tolerances around the scalar, the two
    cloud-fraction thresholds of incloud_to_gridcell and their neighbours."""
    T = np.dtype(dtype).type
    inf, tiny, s = T(np.inf), np.finfo(dtype).smallest_subnormal, T(s)
    vals = [T(np.nan), inf, -inf, T(0.0), T(-0.0), tiny, -tiny, T(1), T(-1), T(0.5), T(2), T(-3),
            s, np.nextafter(s, inf), np.nextafter(s, -inf)]
    tol = T(1e-8) + T(1e-5) * abs(s)
    for edge in (s + tol, s - tol, T(1e-3), T(5e-2)):
        vals += [edge, np.nextafter(edge, inf), np.nextafter(edge, -inf)]
    return np.array(vals, dtype)


def isclose_pairs(dtype):
    """(a, b) on both sides of ``atol + rtol |b|`` for a few b."""
    T = np.dtype(dtype).type
    a, b = [], []
    for y in (T(1), T(-3), T(1e-8), T(0), T(-0.0), T(1e5), T(np.pi)):
        tol = T(1e-8) + T(1e-5) * abs(y)
        for edge in (y + tol, y - tol):
            for x in (edge, np.nextafter(edge, T(np.inf)), np.nextafter(edge, T(-np.inf))):
                a.append(x)
                b.append(y)
    return np.array(a, dtype), np.array(b, dtype)


def ew_operands(dtype, s, seed=0):
    """1-D (a, b, c): the specials of ``a`` crossed with special ``b`` and ``c``, the isclose pairs, then a few hundred
    random values of several magnitudes."""
    rng = np.random.default_rng(seed)
    T = np.dtype(dtype).type
    tiny = np.finfo(dtype).smallest_subnormal
    av = specials(dtype, s)
    bv = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1, -1, 0.5, 2, tiny, 1e-2], dtype)
    cv = np.array([np.nan, np.inf, 0.0, -0.0, 1, -2.5], dtype)
    a, b, c = (g.reshape(-1) for g in np.meshgrid(av, bv, cv, indexing="ij"))
    pa, pb = isclose_pairs(dtype)
    n = 400
    ra = np.concatenate([rng.normal(0, 1, n // 4), rng.normal(0, 100, n // 4), 10.0 ** rng.uniform(-6, 3, n // 4), rng.uniform(0, 1, n // 4)])
    rb = np.where(rng.random(n) < 0.3, 0.0, rng.normal(0, 2, n))
    rc = np.where(rng.random(n) < 0.5, 0.0, rng.normal(0, 2, n))
    a = np.concatenate([a, pa, ra.astype(dtype)])
    b = np.concatenate([b, pb, rb.astype(dtype)])
    c = np.concatenate([c, np.ones(pa.size, dtype), rc.astype(dtype)])
    return a.astype(dtype), b.astype(dtype), c.astype(dtype)


def field(rng, shape, dtype, special_fraction=0.1):
    """Random values with NaN, +-inf, +-0 sprinkled in."""
    x = rng.normal(0, 2, shape)
    pick = rng.random(shape)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0)):
        x = np.where((pick >= k * special_fraction / 5) & (pick < (k + 1) * special_fraction / 5), v, x)
    return np.ascontiguousarray(x.astype(dtype))


EW_SHAPES = [  # (a, b, c): b / c either have a's shape or are [.., y, x] fields shared over a's level axis
    ((2, 3, 5, 7), (2, 3, 5, 7), (2, 5, 7)),
    ((2, 3, 5, 7), (2, 5, 7), (2, 3, 5, 7)),
    ((2, 3, 5, 7), (2, 5, 7), (2, 5, 7)),
    ((3, 5, 7), (5, 7), (3, 5, 7)),
    ((41,), (41,), (41,)),
]

# ------------------------------------------------------------------------------------------------
# member_reduce
# ------------------------------------------------------------------------------------------------
MEMBER_COUNTS = (1, 2, 3, 4, 31, 32)
MEMBER_DTYPES = ("float32", "float64", "mixed")


def member_dtypes(kind, count):
    if kind == "mixed":
        return [np.float32 if k % 2 == 0 else np.float64 for k in range(count)] if count > 1 else [np.float64]
    return [np.dtype(kind).type] * count


def members(kind, count, n, seed=0):
    """``count`` member arrays of ``n`` cells.  The first cells hold the patterns (as far as ``n`` reaches), the rest random
    values with random NaNs.  Values are small multiples of 1/8 so that every order of summation gives the same mean -- the
    reference adds in member order, numpy's nanmean in its own -- except where a pattern is about infinities or overflow."""
    rng = np.random.default_rng(seed + 1000 * count + n)
    m = rng.integers(-64, 65, (count, n)).astype(np.float64) / 8.0
    m[rng.random((count, n)) < 0.2] = np.nan
    big = 3.0e38  # twice this overflows float32; in a float64 reduction the same pattern uses 1.5e308
    if any(d == np.float64 for d in member_dtypes(kind, count)):
        big = 1.5e308
    if count < 2:
        big = 1.0  # (one member: nothing to add)
    k = np.arange(count)
    patterns = [
        k * 0.25 - 1.0,                                            # no NaN, ascending
        np.full(count, np.nan),                                    # all NaN
        np.where(k == count // 2, 2.5, np.nan),                    # all but one NaN
        np.where(k % 2 == 0, k * 0.5, np.nan),                     # alternating NaN, an even member first
        np.where(k % 2 == 1, -k * 0.5, np.nan),                    # alternating NaN, a NaN first
        (count - k) * 0.25,                                        # descending
        np.full(count, 1.75),                                      # all equal
        np.where(k % 3 == 0, 1.0, np.where(k % 3 == 1, -2.0, 1.0)),  # ties
        np.where(k % 2 == 0, 0.0, -0.0),                           # +-0
        np.full(count, -0.0),                                      # all -0
        np.where(k == 0, np.inf, np.where(k == count - 1, -np.inf, k * 1.0)),                     # inf and -inf in one cell
        np.where(k == 0, np.inf, np.where(k == count - 1, -np.inf, np.where(k == 1, np.nan, k * 1.0))),  # ... the other parity kept
        np.where(k == 0, -np.inf, np.where(k == 1, np.inf, np.nan)),                              # only the two infinities (or one)
        np.where(k < 2, big, np.nan),                              # two values whose sum overflows (an even kept count)
        np.where(k < 2, -big, np.nan),
    ]
    for col, p in enumerate(patterns[:n]):
        m[:, col] = p
    with np.errstate(over="ignore"):  # (the float32 members of a mixed ensemble hold inf where float64 ones hold 1.5e308)
        return [np.ascontiguousarray(m[j].astype(d)) for j, d in enumerate(member_dtypes(kind, count))]


# ------------------------------------------------------------------------------------------------
# the column kernels: tendency_to_flux, flux_to_tendency
# ------------------------------------------------------------------------------------------------
def column_layouts(nz):
    """(shape, z_axis): the production [tile, z, y, x] layout (outer and inner extents both > 1), then z first and z last
    with column counts around one 256-thread block and several blocks."""
    return [((3, nz, 5, 7), 1)] + [((nz, cols), 0) for cols in COLUMNS] + [((cols, nz), 1) for cols in COLUMNS]


def column_dtypes(kind):
    """dtypes of (tendency / net flux, delp, toa, upward)."""
    return {"float32": (np.float32,) * 4, "float64": (np.float64,) * 4,
            "mixed": (np.float32, np.float64, np.float32, np.float32)}[kind]


def columns(kind, shape, z_axis, seed=0, finite=False):
    """(tendency, delp, toa_net_flux, surface_upward_flux, net_flux, surface_downward_flux) with, unless ``finite``, a NaN
    or an infinity at the top, a middle and the bottom level of chosen columns and some zero pressure thicknesses."""
    nz = shape[z_axis]
    flat = shape[:z_axis] + shape[z_axis + 1:]
    rng = np.random.default_rng(seed + 7 * nz + int(np.prod(shape)))
    # [nz, columns...]; tendencies of either sign and a bounded range of magnitudes, so that a round trip through the
    # cumulative fluxes keeps its relative accuracy
    tend = np.moveaxis(rng.choice([-1.0, 1.0], shape) * rng.uniform(0.2e-4, 2e-4, shape), z_axis, 0).copy()
    flux = np.moveaxis(rng.normal(0, 50, shape), z_axis, 0).copy()
    delp = np.moveaxis(rng.uniform(300, 1500, shape), z_axis, 0).copy()
    toa, up, down = rng.normal(100, 30, flat), rng.uniform(0, 80, flat), rng.uniform(0, 80, flat)
    if not finite:
        ncol = int(np.prod(flat))
        t2, f2, d2 = (x.reshape(nz, ncol) for x in (tend, flux, delp))
        levels = sorted({0, nz // 2, nz - 1})
        for j, bad in enumerate((np.nan, np.inf, -np.inf)):
            for i, lev in enumerate(levels):
                col = (3 * j + i) * 5 + 1
                if col < ncol:
                    t2[lev, col] = f2[lev, col] = bad
        for col in range(3, ncol, 11):
            d2[rng.integers(0, nz), col] = 0.0                          # delp = 0: a division by zero in flux_to_tendency
        if ncol > 2:
            toa.reshape(-1)[2], up.reshape(-1)[ncol - 1], down.reshape(-1)[ncol // 2] = np.nan, np.inf, -np.inf
    dt = column_dtypes(kind)
    back = lambda x: np.ascontiguousarray(np.moveaxis(x, 0, z_axis))
    return (back(tend).astype(dt[0]), back(delp).astype(dt[1]), toa.astype(dt[2]), up.astype(dt[3]),
            back(flux).astype(dt[0]), down.astype(dt[3]))


# ------------------------------------------------------------------------------------------------
# minmax_score, ocsvm_score
# ------------------------------------------------------------------------------------------------
def minmax_case(n_vars, n_feat, n, dtype, plant, seed=0):
    """[feature, sample] variables with scales / offsets that map most of them into [0, 1], and one planted value in the
    first, a middle or the last variable (``plant`` = (which, value) or None)."""
    rng = np.random.default_rng(seed + 100 * n_vars + 10 * n_feat + n)
    variables = [np.ascontiguousarray(rng.normal(1e5, 1e3, (n_feat, n)).astype(dtype)) for _ in range(n_vars)]
    lo = [rng.normal(1e5 - 2.5e3, 100, n_feat) for _ in range(n_vars)]
    scales = [1.0 / rng.uniform(4e3, 6e3, n_feat) for _ in range(n_vars)]
    offsets = [-l * s for l, s in zip(lo, scales)]
    if plant is not None:
        which, value = plant
        v = variables[{"first": 0, "middle": n_vars // 2, "last": n_vars - 1}[which]]
        v[n_feat // 2, n // 2] = value
        v[n_feat - 1, 0] = value
    return variables, scales, offsets


def ocsvm_case(n_feat, n, n_sv, seed=0):
    rng = np.random.default_rng(seed + 1000 * n_feat + 10 * n + n_sv)
    mean, scale = rng.normal(0, 3, n_feat), rng.uniform(0.5, 2, n_feat)
    x = mean[:, None] + scale[:, None] * rng.normal(0, 1, (n_feat, n))
    sv = rng.normal(0, 1, (n_sv, n_feat))
    coef = rng.uniform(0.1, 1, n_sv)
    gamma = 1.0 / (4 * n_feat)
    if n >= 3:
        x[n_feat // 2, 1] = np.nan      # one sample with a NaN feature, one with an infinite one: their neighbours in the
        x[n_feat - 1, n - 2] = np.inf   # same workgroup must not notice
    return x, mean, scale, sv, coef, gamma
