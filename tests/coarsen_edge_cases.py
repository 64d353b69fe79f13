"""Inputs shared by tests/test_host_coarsen_edges.py (which pins the numpy restatements of tests/coarsen_edge_np.py on them)
and tests/test_gpu_coarsen_edges.py (which runs the kernels of csrc/coarsen.hip on them)."""
import numpy as np

import glue_cases

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
WORD_DTYPES = (F32, F64, I32, I64)
FLOAT_PAIRS = [(F32, F32), (F32, F64), (F64, F32), (F64, F64)]   # (obj, weights)

# ------------------------------------------------------------------------------------------------
# cast, cast_many
# ------------------------------------------------------------------------------------------------
CAST_PAIRS = [(i, o) for i in WORD_DTYPES for o in (F32, F64) if i != o]
CAST_SIZES = glue_cases.SIZES + (glue_cases.PAST_THE_CAP,)
CAST_MANY_COUNTS = (2, 48, 49, 97)       # the kernel's table holds 48
CAST_MANY_LONG = 4096 * 256 + 257        # more elements than the 4096 x 256 threads of one table row


def conversion_values(dtype, seed=0):
    """1-D values of ``dtype`` whose conversion to float32 / float64 must round, overflow or keep a sign:

    float32: +-0, +-inf, NaN, +-subnormals (the smallest and the largest), the smallest normal, FLT_MAX, random values.
    float64: the same as doubles, then for float64 -> float32: the overflow halfway point ``FLT_MAX + 2^103`` (a tie whose
      even neighbour is infinity) with the doubles just below (-> FLT_MAX) and just above it (-> inf), DBL_MAX (-> inf);
      ``1 + 2^-24`` (a tie, -> 1) with its two neighbours, ``1 + 3 * 2^-24`` (a tie, -> 1 + 2^-22); doubles that round to
      float32 subnormals (``1.5 * 2^-149`` and ``2.5 * 2^-149``, both ties to ``2 * 2^-149``; ``2^-127``; the double just below
      ``2^-126``) and to zero (``2^-150``, a tie to zero, with the double just above it -> ``2^-149``; ``2^-151``; a double
      subnormal), each of these with both signs.
    int32: 0, +-1, ``2^24 - 1`` (exact), ``2^24 + 1`` (a tie, -> 2^24), ``2^24 + 3`` (a tie, -> 2^24 + 4) and their
      negatives, INT32_MIN, INT32_MAX, random values of every magnitude.
    int64: those, then ``2^53 - 1`` (exact in float64), ``2^53 + 1`` (a tie, -> 2^53), ``2^53 + 3`` (a tie, -> 2^53 + 4) and
      their negatives, INT64_MIN, INT64_MAX, and around the float32 halfway points ``2^40 + 2^16`` (a tie, -> 2^40) and
      ``2^40 + 3 * 2^16`` (a tie, -> 2^40 + 2^18): the integers one below, on and one above.
    """
    rng = np.random.default_rng(seed + 17)
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        fi = np.finfo(np.float32)
        sub_max = np.nextafter(fi.tiny, F32(0))
        v = [0.0, -0.0, np.inf, -np.inf, np.nan, fi.smallest_subnormal, -fi.smallest_subnormal, sub_max, -sub_max, fi.tiny, -fi.tiny,
             fi.max, -fi.max, 1.0, -1.0, np.nextafter(F32(1), F32(2)), F32(0.1)]
        rnd = np.concatenate([rng.normal(0, 1, 150), 10.0 ** rng.uniform(-44, 38, 150) * rng.choice([-1, 1], 150)])
        return np.concatenate([np.array(v, F32), rnd.astype(F32)])
    if dtype == np.float64:
        fi, di = np.finfo(np.float32), np.finfo(np.float64)
        up, dn = (lambda x: np.nextafter(F64(x), F64(np.inf))), (lambda x: np.nextafter(F64(x), F64(-np.inf)))
        half_over = F64(fi.max) + F64(2.0) ** 103
        tie1, tie3 = F64(1) + F64(2.0) ** -24, F64(1) + 3 * F64(2.0) ** -24
        s = F64(2.0) ** -149
        pos = [half_over, dn(half_over), up(half_over), di.max, F64(fi.max), tie1, dn(tie1), up(tie1), tie3,
               1.5 * s, 2.5 * s, F64(2.0) ** -127, dn(F64(2.0) ** -126), F64(2.0) ** -126, s, F64(fi.tiny) - s,
               F64(2.0) ** -150, up(F64(2.0) ** -150), dn(F64(2.0) ** -150), F64(2.0) ** -151, di.smallest_subnormal, di.tiny,
               1.0, 0.1, F64(2.0) ** 24 + 1, F64(2.0) ** 25 + 1]
        v = [0.0, -0.0, np.inf, -np.inf, np.nan] + pos + [-p for p in pos]
        rnd = np.concatenate([rng.normal(0, 1, 150), 10.0 ** rng.uniform(-50, 40, 150) * rng.choice([-1, 1], 150)])
        return np.concatenate([np.array(v, F64), rnd])
    small = [0, 1, -1, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 - 1), -(2 ** 24 + 1), -(2 ** 24 + 3), 2 ** 24, 2 ** 25 + 2, 2 ** 25 + 6]
    if dtype == np.int32:
        ii = np.iinfo(np.int32)
        rnd = np.concatenate([rng.integers(ii.min, ii.max, 200, dtype=np.int64), rng.integers(-2 ** 26, 2 ** 26, 100, dtype=np.int64)])
        return np.concatenate([np.array(small + [ii.min, ii.max, ii.max - 64, ii.max - 63], np.int64), rnd]).astype(np.int32)
    assert dtype == np.int64
    ii = np.iinfo(np.int64)
    h1, h3 = 2 ** 40 + 2 ** 16, 2 ** 40 + 3 * 2 ** 16
    big = [2 ** 53 - 1, 2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53 - 1), -(2 ** 53 + 1), -(2 ** 53 + 3), 2 ** 53, ii.min, ii.max, ii.max - 2 ** 9,
           ii.max - 2 ** 38, h1 - 1, h1, h1 + 1, h3 - 1, h3, h3 + 1, -(h1 - 1), -h1, -(h1 + 1), -h3, 2 ** 31, -(2 ** 31) - 1, 2 ** 32 + 1]
    rnd = np.concatenate([rng.integers(ii.min, ii.max, 150, dtype=np.int64), rng.integers(-2 ** 56, 2 ** 56, 100, dtype=np.int64),
                          rng.integers(-2 ** 30, 2 ** 30, 50, dtype=np.int64)])
    return np.concatenate([np.array(small + big, np.int64), rnd])


def conversion_input(dtype, size):
    """``size`` elements that walk through ``conversion_values(dtype)`` again and again."""
    return np.resize(conversion_values(dtype), size)


def cast_many_tensors(count, out_dtype):
    """1-D arrays of which ``count`` need converting to ``out_dtype`` -- the entries of the kernel's table, their dtypes in a
    fixed rotation, sizes 1, 257 and a few others -- with one array that already has ``out_dtype`` after every seventh of
    them.  The third to convert (if there is one) is empty and, from 48 up, entry ``count - 2`` holds CAST_MANY_LONG elements
    while its table neighbours are short."""
    rot = [d for d in WORD_DTYPES if d != out_dtype]
    sizes = (1, 257, 5, 256, 33, 1000, 64)
    out = []
    for k in range(count):
        dtype, n = rot[k % 3], sizes[k % len(sizes)]
        if k == 2:
            n = 0
        if count >= 48 and k == count - 2:
            n = CAST_MANY_LONG
        out.append(np.roll(conversion_input(dtype, n), k))
        if k % 7 == 6:
            out.append(np.roll(conversion_input(out_dtype, sizes[k % 5]), k))
    return out


# ------------------------------------------------------------------------------------------------
# words: cube_edge_rows, halo_pick, repeat, block_upsample, take_lines
# ------------------------------------------------------------------------------------------------
def words(shape, dtype, seed=0):
    """Random words of ``dtype``: for the float types every bit pattern, so NaNs with payloads, infinities, subnormals and
    -0.0 among them (a -0.0 and a signalling NaN are planted in any case)."""
    rng = np.random.default_rng(seed + int(np.prod(shape)) + np.dtype(dtype).itemsize)
    it = {4: np.int32, 8: np.int64}[np.dtype(dtype).itemsize]
    ii = np.iinfo(it)
    bits = rng.integers(ii.min, ii.max, shape, dtype=it, endpoint=True)
    flat = bits.reshape(-1)
    if np.issubdtype(np.dtype(dtype), np.floating) and flat.size >= 2:
        flat[flat.size // 2] = ii.min                                                   # -0.0
        flat[-1] = {4: 0x7F800001, 8: 0x7FF0000000000001}[np.dtype(dtype).itemsize]   # a signalling NaN with payload 1
    return bits.view(dtype)


CUBE_SHAPES = [(6, n, n) for n in (1, 2, 12)] + [(6, 5, n, n) for n in (1, 2, 12)] + [(6, 2, 3, n, n) for n in (1, 2, 12)]
TILE_LISTS = [list(range(6)), [2, 5], [3], [5, 0, 3]]
INTERP_STEPS = (1, 2, 3, 4, 6, 12)   # of n = 12; at 12 both outputs are halo edges

# (nx_in, fx) -> nx_out on both sides of `nx_out % VEC == 0 && nx_out >= 256` for 4-byte (VEC = 4) and 8-byte (VEC = 2) words
REPEAT_X = [(36, 7), (84, 3), (126, 2), (256, 1), (128, 2), (86, 3), (129, 2), (258, 1), (52, 5), (130, 2), (514, 2), (1028, 1),
            (37, 7), (148, 7)]
REPEAT_YX = [(3, 1), (1, 4), (2, 5)]


def float_field(shape, dtype, seed=0):
    """Normal values with NaN and +-inf sprinkled in (glue_cases.field)."""
    return glue_cases.field(np.random.default_rng(seed + int(np.prod(shape))), shape, dtype)


def interp_rect(dtype, outer=(2, 4), ny=5, nx=8, seed=0):
    """(x [.., ny, nx], {axis: (lo, hi)}) with NaN and +-inf in interior cells and in halo cells and, next to each
    other, two values of 3e38 (1.5e308 in float64) whose sum overflows (in the interior and across a halo)."""
    rng = np.random.default_rng(seed + 5)
    x = rng.normal(0, 2, outer + (ny, nx)).astype(dtype)
    halos = {0: [rng.normal(0, 2, outer + (ny,)).astype(dtype) for _ in range(2)],
             1: [rng.normal(0, 2, outer + (nx,)).astype(dtype) for _ in range(2)]}
    big = np.dtype(dtype).type(3e38 if np.dtype(dtype) == np.float32 else 1.5e308)
    x[0, 0, 2, 3], x[0, 1, 1, 1], x[1, 0, 3, 6], x[1, 2, 0, 0] = np.nan, np.inf, -np.inf, np.nan
    x[0, 2, 2, 4], x[0, 2, 2, 5], x[0, 2, 3, 4] = big, big, big            # neighbours along x and along y
    x[1, 3, 4, 7], x[1, 3, 0, 7], x[1, 3, 4, 0] = -big, big, big           # at the edges, next to the planted halo cells
    for axis, n in ((0, ny), (1, nx)):
        lo, hi = halos[axis]
        lo[0, 0, 1], hi[0, 0, n - 1], lo[1, 1, 0], hi[1, 1, 2] = np.nan, np.inf, -np.inf, np.nan
    halos[0][0][1, 3, 4], halos[0][1][1, 3, 4] = big, -big     # beside x[1, 3, 4, 0] and x[1, 3, 4, 7]
    halos[1][0][1, 3, 7], halos[1][1][1, 3, 7] = big, -big     # below x[1, 3, 0, 7] and above x[1, 3, 4, 7]
    return x, halos


# ------------------------------------------------------------------------------------------------
# weighted_window_average
# ------------------------------------------------------------------------------------------------
WAVG_WINDOWS = [  # (shape, window, stride)
    ((2, 3, 5, 12), (1, 4), (1, 4)),     # as regridz uses it on the kept lines
    ((2, 3, 5, 12), (3, 2), (1, 1)),     # overlapping
    ((2, 3, 7, 11), (2, 2), (3, 3)),     # gaps
    ((2, 3, 7, 11), (2, 3), (2, 3)),     # a remainder in both dims
    ((2, 3, 5, 12), (5, 12), (5, 12)),   # the window is the field
    ((2, 20, 9, 13), (2, 2), (1, 1)),    # 3840 outputs: more than one block
]


def wavg_inputs(shape, obj_dtype, w_dtype, shared, window, plant=True, seed=0):
    """(obj, weights): normal values and weights from U(0.5, 1.5); ``shared``: 2-D weights per leading index, shared over the
    level dim.  ``plant``: a NaN in ``obj``, an infinity in the first window of the first slice, a NaN weight, the first
    window of the last slice with only NaN weights and the last ``window`` cells of the first slice with only zero weights
    (where the window is the field, the zero weights swallow the infinity)."""
    rng = np.random.default_rng(seed + int(np.prod(shape)) + 3 * window[0] + window[1])
    obj = rng.normal(0, 2, shape).astype(obj_dtype)
    w = rng.uniform(0.5, 1.5, (shape[0],) + shape[-2:] if shared else shape).astype(w_dtype)
    if plant:
        by, bx = window
        ny, nx = shape[-2:]
        obj[0, 1, ny // 2, nx // 2] = np.nan
        obj[0, -1, 0, 0] = np.inf
        w[0, ..., ny // 2, 0] = np.nan
        w[-1, ..., :by, :bx] = np.nan
        w[0, ..., ny - by:, nx - bx:] = 0.0
    return obj, w


FAST_FACTORS = (2, 4, 8, 16, 32)


def fast_shape(factor):
    return (2, 3, 2 * factor, max(2 * factor, 16))


# ------------------------------------------------------------------------------------------------
# block_reduce over strided windows, take_lines
# ------------------------------------------------------------------------------------------------
REDUCE_WINDOWS = [  # (shape, window, stride)
    ((2, 3, 6, 8), (1, 2), (2, 2)),
    ((2, 3, 6, 8), (3, 2), (1, 1)),
    ((2, 3, 7, 11), (2, 2), (3, 3)),
    ((2, 19, 17), (9, 8), (9, 8)),       # 72 values: the serial rank kernel; a remainder in both dims
    ((3, 5, 9, 12), (3, 2), (1, 1)),     # 1155 windows: more than the four waves of one block, many times over
]
REDUCE_OPS = ("sum", "mean", "min", "max", "median", "mode")
TAKE_STEPS = (1, 4, 17, 40)   # of 17 lines


def small_integers(shape, dtype, window, seed=0):
    """Integers in [-4, 4] (sums and means of two middle values are exact; many ties for the mode); for float types a NaN in
    about one value of eight, the first window of the first slice all NaN, the last ``window`` cells of the last slice without any."""
    rng = np.random.default_rng(seed + int(np.prod(shape)) + 5 * window[0] + window[1])
    a = rng.integers(-4, 5, shape).astype(dtype)
    if np.issubdtype(np.dtype(dtype), np.floating):
        a[rng.random(shape) < 0.125] = np.nan
        by, bx = window
        a.reshape((-1,) + shape[-2:])[0, :by, :bx] = np.nan
        a.reshape((-1,) + shape[-2:])[-1, -by:, -bx:] = rng.integers(-2, 3, (by, bx))
    return a
