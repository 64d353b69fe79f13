/*
 * fv3hip.h -- C ABI of libfv3hip.so, the MI355X (gfx950) implementation of fv3net's
 * column-wise ML tendency inference and cubed-sphere coarse-graining hot path.
 *
 * The reference has no native ABI for this path except the f2py-generated `mappm.mappm`
 * module; everything else is Python on top of TensorFlow / xarray / numpy.  Each entry point
 * below therefore cites the reference *Python or Fortran interface* it replaces (paths are
 * relative to the reference checkout).  INTEGRATION.md shows the ctypes stub a maintainer
 * of the reference would add for each one.
 *
 * Conventions
 *   - every function returns 0 on success or a negative FV3HIP_E* code; the message for the
 *     calling thread's last failure is returned by fv3hip_last_error();
 *   - all data pointers are DEVICE pointers (hipMalloc / torch.cuda tensors), caller-owned,
 *     never freed or retained by the library beyond the call (model handles copy their
 *     weights at create time);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call only
 *     enqueues work on that stream and never synchronises, so calls can be captured in a
 *     hipGraph;
 *   - arrays are dense, row-major, "x fastest": horizontal fields are [n_outer][ny][nx].
 */
#ifndef FV3HIP_H
#define FV3HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FV3HIP_ABI_VERSION 3

/* status codes */
#define FV3HIP_OK 0
#define FV3HIP_EINVAL -1      /* bad argument (shape, dtype, factor ...)            */
#define FV3HIP_EUNSUPPORTED -2 /* valid in the reference but not implemented here    */
#define FV3HIP_EHIP -3        /* a HIP runtime call failed                           */
#define FV3HIP_ENOMEM -4

/* element types */
#define FV3HIP_F32 0
#define FV3HIP_F64 1
#define FV3HIP_I32 2
#define FV3HIP_I64 3

/* block reductions (fv3hip_block_reduce) */
#define FV3HIP_OP_SUM 0
#define FV3HIP_OP_MEAN 1
#define FV3HIP_OP_MIN 2
#define FV3HIP_OP_MAX 3
#define FV3HIP_OP_MEDIAN 4
#define FV3HIP_OP_MODE 5

/* NaN handling for fv3hip_block_reduce */
#define FV3HIP_NAN_SKIP 0      /* xarray coarsen().sum()/min()/max()/mean() default (skipna) */
#define FV3HIP_NAN_PROPAGATE 1 /* numpy.sum/mean/min/max/median (NaN if any NaN in the window);
                                  scipy.stats.mode(nan_policy="propagate")                   */
#define FV3HIP_NAN_OMIT 2      /* scipy.stats.mode(nan_policy="omit")                        */

/* arithmetic of the remap (fv3hip_mappm, fv3hip_mappm_multi) */
#define FV3HIP_ARITH_EXACT 0 /* IEEE division, the Fortran's association order: bit-identical to the compiled reference */
#define FV3HIP_ARITH_FAST 1  /* a / b = a * v_rcp_f32(b) with shared reciprocals where the sweep kernel applies (LEVEL_COL,
                                kord <= 3, km >= 8, n_inner % 64 == 0); a few ulp from EXACT; elsewhere the same as EXACT */

/* column layouts (fv3hip_mappm, fv3hip_pressure_at_interface) */
#define FV3HIP_LAYOUT_COL_LEVEL 0 /* [column][level]: level fastest (what f2py callers pass)  */
#define FV3HIP_LAYOUT_LEVEL_COL 1 /* [batch][level][inner]: column fastest (native [z,y,x])   */

const char *fv3hip_last_error(void);
int fv3hip_abi_version(void);

/* Check that `device` exists and is a gfx950 part.  The calling thread's current device is NOT changed.
 * DEVICE RULE for every other entry point: kernels are launched on, and scratch memory is allocated on, the CURRENT
 * HIP device, which must be the device of the pointers passed (callers holding several GPUs make it current around
 * the call; fv3hip_mlp_predict returns FV3HIP_EINVAL when the model was created on another device). */
int fv3hip_init(int device);

typedef struct {
    char name[128];
    char arch[64];
    int compute_units;
    int wavefront_size;
    int lds_bytes_per_cu;
    int clock_mhz;
    size_t hbm_bytes;
} fv3hip_device_info_t;
int fv3hip_device_info(fv3hip_device_info_t *out);

/* ------------------------------------------------------------------------------------------
 * Horizontal coarse-graining
 * ------------------------------------------------------------------------------------------ */

/*
 * Replaces vcm.cubedsphere.weighted_block_average
 * (external/vcm/vcm/cubedsphere/coarsen.py:183-218):
 *     out = nansum_block(obj * w) / nansum_block(w)      over factor x factor blocks
 * obj: [n_outer][ny][nx]; weights: [n_outer / w_repeat][ny][nx], each weight slice shared by
 * w_repeat consecutive outer slices (w_repeat = 1: same shape as obj; w_repeat = nz: 2-D
 * area weights of a [tile][z][y][x] field).  out: [n_outer][ny/factor][nx/factor] in the
 * promoted type (F64 if either input is F64, else F32).  NaN products/weights are skipped as
 * xarray's skipna sums do; an all-zero denominator gives NaN (0/0) as in the reference.
 */
int fv3hip_weighted_block_average(const void *obj, int obj_dtype, const void *weights,
                                  int w_dtype, int64_t n_outer, int ny, int nx,
                                  int64_t w_repeat, int factor, void *out, void *stream);

/*
 * The mass-weighted means of the restart pipelines (external/vcm/vcm/cubedsphere/coarsen_restarts.py:335-427, 856-900:
 * weighted_block_average(ds[mass_weighted_vars], delp * area, ...)) for n_fields fields that share their weights:
 *     out_f[o][Y][X] = nansum_block(field_f * (delp * area)) / nansum_block(delp * area)
 * with the product delp * area formed in registers (never written) and read once per four fields.  `fields` / `outs` are
 * HOST arrays of device pointers; fields and delp [n_outer][ny][nx] in `dtype`, area [n_outer / a_repeat][ny][nx] in
 * `area_dtype`, outputs [n_outer][ny / f][nx / f] in the promoted type (F64 unless both are F32).  `delp` may be NULL: the
 * weights are then `area` alone, shared by the fields (the area-weighted means of the surface data,
 * coarsen_restarts.py:1163-1230, four fields per launch).  factor in
 * {2, 4, 8, 16} with 16-byte aligned rows; anything else returns FV3HIP_EUNSUPPORTED (callers then form the product with
 * fv3hip_ew and use fv3hip_weighted_block_average).
 */
int fv3hip_mass_weighted_block_average(const void *const *fields, int n_fields, int dtype, const void *delp,
                                       const void *area, int area_dtype, int64_t n_outer, int ny, int nx,
                                       int64_t a_repeat, int factor, void *const *outs, void *stream);

/*
 * Replaces vcm.cubedsphere.edge_weighted_block_average
 * (external/vcm/vcm/cubedsphere/coarsen.py:221-273).  edge = 0 ('x'): weighted mean over
 * `factor` cells along x, every factor-th row kept along y (out [n_outer][ceil(ny/f)][nx/f]);
 * edge = 1 ('y'): the transpose of that (out [n_outer][ny/f][ceil(nx/f)]).
 */
/* The general form of the two weighted means above: windows of by x bx cells every (sy, sx) cells,
 * out [n_outer][(ny - by) / sy + 1][(nx - bx) / sx + 1] (weights as in fv3hip_weighted_block_average; ABI v3).
 * weighted_block_average = (f, f, f, f); edge_weighted 'x' = (1, f, f, f); on fields already reduced to the kept lines: (1, f, 1, f). */
int fv3hip_weighted_window_average(const void *obj, int obj_dtype, const void *weights, int w_dtype,
                                   int64_t n_outer, int ny, int nx, int64_t w_repeat, int by, int bx,
                                   int sy, int sx, void *out, void *stream);
int fv3hip_edge_weighted_block_average(const void *obj, int obj_dtype, const void *spacing,
                                       int w_dtype, int64_t n_outer, int ny, int nx,
                                       int64_t w_repeat, int factor, int edge, void *out,
                                       void *stream);

/*
 * Replaces vcm.cubedsphere.block_coarsen / block_median / _block_mode / block_edge_coarsen
 * (external/vcm/vcm/cubedsphere/coarsen.py:795-840, 557-588, 750-786, 629-683) and the
 * vendored block_reduce they sit on (external/vcm/vcm/cubedsphere/_skimage.py:125-202):
 *     out[o][Y][X] = op over in[o][Y*sy .. Y*sy+by-1][X*sx .. X*sx+bx-1]
 * with ny_out = (ny - by)/sy + 1, nx_out = (nx - bx)/sx + 1.  Full blocks: by=bx=sy=sx=f;
 * edge 'x' coarsening: by=1, bx=f, sy=sx=f.  The output has the input's dtype except MEAN /
 * MEDIAN of integers, which is not supported (the reference only applies them to floats).
 */
int fv3hip_block_reduce(const void *in, int dtype, int64_t n_outer, int ny, int nx, int by,
                        int bx, int sy, int sx, int op, int nan_policy, void *out,
                        void *stream);

/*
 * Replaces vcm.cubedsphere.block_upsample / block_upsample_like
 * (external/vcm/vcm/cubedsphere/coarsen.py:869-938): out[o][y][x] = in[o][y/f][x/f], where a
 * coarse dimension of odd size is a staggered one whose last point is not repeated
 * (ny_out = (ny_in-1)*f+1) and an even one is repeated uniformly (ny_out = ny_in*f).
 * elem_size is 4 or 8 bytes.
 */
/* out[o][y][x] = in[o][y / fy][x / fx], out is [n_outer][ny_in * fy][nx_in * fx] (xarray_utils.repeat, vcm/xarray_utils.py:37-82,
 * with a count per horizontal dim; ABI v3) */
int fv3hip_repeat(const void *in, int elem_size, int64_t n_outer, int ny_in, int nx_in, int fy,
                  int fx, void *out, void *stream);
int fv3hip_block_upsample(const void *in, int elem_size, int64_t n_outer, int ny_in, int nx_in,
                          int factor, void *out, void *stream);

/*
 * The mask arithmetic of the 'complex' surface-data coarse-graining
 * (external/vcm/vcm/cubedsphere/coarsen_restarts.py:1140-1470), one elementwise launch per step.
 * a, out: n values; b, c: n values, or 2-D fields of `inner` values shared by b_rep / c_rep consecutive
 * outer slices of a (a = [.., level, y, x], b = [.., y, x]).  Masks are 0 / 1 in the fields' dtype.
 */
#define FV3HIP_EW_MUL 0        /* a * b                                              */
#define FV3HIP_EW_ISCLOSE 1    /* np.isclose(a, b) (rtol 1e-5, atol 1e-8)            */
#define FV3HIP_EW_ISCLOSE_S 2  /* np.isclose(a, scalar)                              */
#define FV3HIP_EW_WHERE_NAN 3  /* a.where(b): a where the mask b holds, else NaN     */
#define FV3HIP_EW_SELECT 4     /* xr.where(c, a, b)                                  */
#define FV3HIP_EW_SELECT_S 5   /* xr.where(b, scalar, a)                             */
#define FV3HIP_EW_GT_S 6       /* a > scalar                                         */
#define FV3HIP_EW_LT_S 7       /* a < scalar                                         */
#define FV3HIP_EW_FILLNA_S 8   /* a.fillna(scalar)                                   */
#define FV3HIP_EW_AND 9        /* a & b                                              */
#define FV3HIP_EW_MIN_S 10     /* a.where(a < scalar, other=scalar)                  */
#define FV3HIP_EW_BLEND 11     /* coarsen_restarts.blend: a * b + (1 - a) * c         */
#define FV3HIP_EW_MUL_S 12     /* scalar * a                                          */
#define FV3HIP_EW_WHERE_S 13   /* a.where(mask b, other=scalar)                       */
#define FV3HIP_EW_ADD 14       /* a + b                                               */
#define FV3HIP_EW_ADD_S 15     /* a + scalar                                          */
/* the emulators' tensor transforms (fv3fit/emulation/transforms/transforms.py:17-158; ABI v3) */
#define FV3HIP_EW_SUB 16               /* a - b                                (Difference.forward)               */
#define FV3HIP_EW_LOG_FLOOR_S 17       /* log(max(a, scalar))                  (LogTransform.forward)             */
#define FV3HIP_EW_EXP 18               /* exp(a)                               (LogTransform.backward)            */
#define FV3HIP_EW_RELU_THRESHOLD_S 19  /* a where a > scalar (strict) else 0, NaN stays  (LimitValueTransform, lower bound) */
#define FV3HIP_EW_BELOW_S 20           /* a where a < scalar else 0 * a (NaN for NaN, +inf) (LimitValueTransform, upper bound) */
#define FV3HIP_EW_DIV_S 21             /* a / scalar                           (vcm temperature_tendency, thermo/local.py:340-358) */
#define FV3HIP_EW_INCLOUD_TO_GRIDCELL 22 /* b where a <= 1e-3 else b * max-like(a, 5e-2): in-cloud -> gridcell condensate by cloud
                                          fraction a (vcm/calc/clouds.py:40-66) */
#define FV3HIP_EW_CLIP01 23            /* np.clip(a, 0, 1), a NaN stays        (taper_ramp, fv3fit/_shared/taper_function.py:41-51) */
#define FV3HIP_EW_POW_BASE_S 24        /* scalar ** a                          (taper_decay, taper_function.py:54-64) */
#define FV3HIP_EW_MINIMUM_S 25         /* np.minimum(a, scalar), a NaN stays   (taper_decay) */
/* ... and of the derived variables of vcm.DerivedMapping (external/vcm/vcm/derived_mapping.py) */
#define FV3HIP_EW_DIV 26               /* a / b                                (flux fractions, transmissivity :247-262) */
#define FV3HIP_EW_WHERE_POS_S 27       /* a where b > 0 else scalar            (_limit_sw_positive :243-244) */
#define FV3HIP_EW_SIGN 28              /* np.sign(a)                           (tendencies parallel to the wind :167-176) */
#define FV3HIP_EW_ABS 29               /* |a| */
#define FV3HIP_EW_RSUB_S 30            /* scalar - a                           (1 - fraction :293-295) */
#define FV3HIP_EW_RDIV_S 31            /* scalar / a                           (gridcell_to_incloud_condensate, calc/clouds.py:33) */
#define FV3HIP_EW_WHERE_GT_S 32        /* a.where(a > scalar, other=scalar)    (calc/clouds.py:33) */
#define FV3HIP_EW_LE_S 33              /* a <= scalar                          (calc/clouds.py:34-36) */
#define FV3HIP_EW_SIN 34               /* sin(a)                               (cos_zenith_angle, calc/_zenith_angle.py:226-242) */
#define FV3HIP_EW_COS 35               /* cos(a) */
int fv3hip_ew(int op, const void *a, const void *b, const void *c, double scalar, int dtype,
              int64_t n, int64_t inner, int64_t b_rep, int64_t c_rep, void *out, void *stream);

/*
 * Pick and orient the halo vectors of `n_local` tiles from the boundary-vector table of all six tiles (fv3hip_cube_edge_rows,
 * [6][4][n_mid][n]): out[side][i][o][j] = rows[nbr[side * n_local + i]][row[...]][o][flip[...] ? n - 1 - j : j], side 0 = the
 * neighbour below the first cell, 1 = beyond the last.  The connectivity of external/vcm/vcm/cubedsphere/xgcm.py:7-34
 * is the caller's (fv3net_amd/cubedsphere/grid.py); nbr / row / flip are HOST arrays of 2 * n_local ints.
 */
int fv3hip_halo_pick(const void *rows, int elem_size, int n_local, int64_t n_mid, int n, const int *nbr, const int *row,
                     const int *flip, void *out, void *stream);

/* out[i] = (out_dtype) in[i]: F32 / F64 / I32 / I64 -> F32 / F64 (the surface-data arithmetic of
 * coarsen_restarts.py:1140-1470 runs in one dtype; restart files mix them). */
int fv3hip_cast(const void *in, int in_dtype, void *out, int out_dtype, int64_t n, void *stream);
/* The same for `count` arrays in one launch (the 35 surface fields of a restart set): HOST arrays of device pointers,
 * input dtypes and lengths. */
int fv3hip_cast_many(const void *const *in, const int *in_dtype, void *const *out, int out_dtype, const int64_t *n, int count,
                     void *stream);

/*
 * Cell centres -> cell edges across the faces of the cube: the device half of what
 * xgcm.Grid.interp(delp, axis) does for vcm.cubedsphere.regridz.regrid_to_edge_weighted_pressure and
 * coarsen_restarts.compute_edge_delp (external/vcm/vcm/cubedsphere/regridz.py:123-135,
 * coarsen_restarts.py:825-853, connectivity table xgcm.py:7-34).
 *
 * fv3hip_cube_edge_rows: in [n_tiles][n_mid][n][n] -> rows [n_tiles][4][n_mid][n], the four
 * boundary vectors of every (square) tile indexed along the edge: 0: x = 0, 1: x = n-1 (index = y),
 * 2: y = 0, 3: y = n-1 (index = x).  These are what neighbouring tiles -- on this or another
 * GPU -- need as their one-cell halo (the only exchange step of the coarse-graining path).
 * elem_size is 4 or 8 bytes.
 *
 * fv3hip_interp_center_to_outer: out = 0.5 * (left + right) along axis (0 = x: [n_outer][ny][nx+1],
 * 1 = y: [n_outer][ny+1][nx]); at the two ends the outside neighbour comes from lo / hi
 * [n_outer][ny] (axis 0) or [n_outer][nx] (axis 1), already oriented along this tile's edge.
 */
int fv3hip_cube_edge_rows(const void *in, int elem_size, int n_tiles, int64_t n_mid, int n,
                          void *rows, void *stream);
int fv3hip_interp_center_to_outer(const void *in, int dtype, int64_t n_outer, int ny, int nx,
                                  int axis, const void *lo, const void *hi, void *out,
                                  void *stream);
/* ... only every step-th edge along the axis (n / step + 1 points; point j' is edge j' * step): the lines
 * vcm.cubedsphere.edge_weighted_block_average (coarsen.py:221-273) keeps -- the pressure-level D-grid wind path
 * (regridz.py:81-146, coarsen_restarts.py:497-556) needs the edge pressures on those lines only (ABI v3). */
int fv3hip_interp_center_to_outer_lines(const void *in, int dtype, int64_t n_outer, int ny, int nx,
                                        int axis, int step, const void *lo, const void *hi,
                                        void *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Vertical: interface pressures and the PPM remap
 * ------------------------------------------------------------------------------------------ */

/*
 * Replaces vcm.pressure_at_interface
 * (external/vcm/vcm/calc/thermo/vertically_dependent.py:41-66): p[0] = toa,
 * p[k+1] = p[k] + delp[k], accumulated sequentially in the array's own dtype (as
 * numpy.cumsum does).  delp: [n_batch][nz][n_inner] -> out: [n_batch][nz+1][n_inner]
 * (LEVEL_COL) or [ncol][nz] -> [ncol][nz+1] (COL_LEVEL, n_batch = ncol, n_inner = 1).
 * nz == 0: out is the toa plane and delp, an empty array, may be null.
 */
int fv3hip_pressure_at_interface(const void *delp, int dtype, int64_t n_batch, int nz,
                                 int64_t n_inner, double toa_pressure, void *out, void *stream);

/*
 * Replaces vcm.pressure_at_midpoint_log
 * (external/vcm/vcm/calc/thermo/vertically_dependent.py:153-179): delp / diff(log(p_interface)).
 * Same layout and dtype rules as fv3hip_pressure_at_interface; out has nz levels.
 */
int fv3hip_pressure_at_midpoint_log(const void *delp, int dtype, int64_t n_batch, int nz,
                                    int64_t n_inner, double toa_pressure, void *out, void *stream);

/*
 * Replaces vcm.cubedsphere.regridz._mask_weights
 * (external/vcm/vcm/cubedsphere/regridz.py:200-220):
 *     out[b][k][c] = weights[b / w_repeat][c]  if p_cmp[b][k + cmp_offset][c] < p_fine[b][nz][c] else 0
 * extrapolate=False: p_cmp = coarse interface pressures (nz+1 levels), cmp_offset = 1 (bottom
 * interface of layer k); extrapolate=True: p_cmp = coarse midpoint pressures (nz levels),
 * cmp_offset = 0.  p_cmp is [n_batch][cmp_levels][n_inner], p_fine [n_batch][nz+1][n_inner],
 * both in p_dtype; weights [n_batch / w_repeat][n_inner] and out [n_batch][nz][n_inner] in w_dtype.
 */
int fv3hip_mask_weights(const void *weights, int w_dtype, const void *p_cmp, int cmp_levels,
                        int cmp_offset, const void *p_fine, int p_dtype, int64_t n_batch, int nz,
                        int64_t n_inner, int64_t w_repeat, void *out, void *stream);

/* fv3hip_mask_weights with p_cmp on a horizontally coarser grid, [n_batch][cmp_levels][ny / factor][nx / factor]: column (y, x)
 * compares the level of coarse column (y / factor, x / factor) -- regridz.py:119-121 upsamples it first; this does not.
 * Any nx (an odd, staggered extent keeps its last point).  FV3HIP_EUNSUPPORTED only where n_batch * nz > 65535 (the grid's row
 * limit) or ny * nx >= 2^31 (upsample and call fv3hip_mask_weights then). */
int fv3hip_mask_weights_coarse(const void *weights, int w_dtype, const void *p_cmp_coarse, int cmp_levels, int cmp_offset,
                               const void *p_fine, int p_dtype, int64_t n_batch, int nz, int ny, int nx, int factor,
                               int64_t w_repeat, void *out, void *stream);

/*
 * Replaces the f2py module function mappm.mappm(p_in, f_in, p_out, i1, i2, iv, kord, ptop)
 * (external/mappm/mappm/mappm.f90:10-126 with ppm_profile :614-851 and ppm_limiters
 * :854-931; caller external/vcm/vcm/cubedsphere/regridz.py:304-338).  Single precision
 * inside, as in the Fortran (default REAL); inputs may be F32 or F64 (F64 is rounded to F32
 * on load, which is what f2py's argument conversion does).  q2 is always F32.
 *   COL_LEVEL: pe1 [ncol][km+1], q1 [ncol][km], pe2 [ncol][kn+1], q2 [ncol][kn]
 *              (n_batch = ncol, n_inner = 1)
 *   LEVEL_COL: pe1 [n_batch][km+1][n_inner], ... ; ncol = n_batch * n_inner
 * Every kord: ppm_profile (kord <= 7) and cs_profile / cs_limiters (kord > 7, mappm.f90:132-611: schemes 8 .. 16 and the linear
 * one above); kord > 7 with iv = -2 returns FV3HIP_EUNSUPPORTED (cs_profile would read the array qs that mappm never sets).
 * `arith`: FV3HIP_ARITH_EXACT or FV3HIP_ARITH_FAST (see above).
 * `workspace` must hold fv3hip_mappm_workspace_bytes(...) bytes of device memory; it carries the call's
 * list of columns to redo, so concurrent calls (other streams) need workspaces of their own.
 */
size_t fv3hip_mappm_workspace_bytes(int64_t ncol, int km);
int fv3hip_mappm(const void *pe1, const void *q1, const void *pe2, int in_dtype, float *q2,
                 int64_t n_batch, int64_t n_inner, int km, int kn, int iv, int kord, int layout, int arith,
                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same remap for n_fields fields that share pe1 and pe2 (regridz.py:163-185 remaps every variable of a
 * dataset between the same two pressure grids): q1 / q2 are HOST arrays of n_fields device pointers.  Fields are
 * processed four at a time in one sweep that computes the control flow and every pressure-only term once;
 * each field's result is bit-identical to fv3hip_mappm on that field.  Same workspace as fv3hip_mappm.
 */
int fv3hip_mappm_multi(const void *pe1, const void *const *q1, const void *pe2, int in_dtype,
                       float *const *q2, int n_fields, int64_t n_batch, int64_t n_inner, int km,
                       int kn, int iv, int kord, int layout, int arith, void *workspace,
                       size_t workspace_bytes, void *stream);

/*
 * fv3hip_mappm_multi with the target interfaces on a horizontally coarser grid: pe2_coarse is [n_batch][kn + 1][ny / factor]
 * [nx / factor], the fields and pe1 [n_batch][level][ny][nx]; fine column (y, x) is remapped to the interfaces of coarse column
 * (y / factor, x / factor).  regridz.py:119-185 reaches the same result through an upsampled copy of the coarse pressures
 * (block_upsample_like); here that copy is never made and the 64 columns of a wave share 64 / factor target columns.  Results are
 * identical to upsampling and calling fv3hip_mappm_multi.  FV3HIP_EUNSUPPORTED unless factor >= 2, nx % 64 == 0 and the shape is
 * one the sweep kernel takes (kord <= 3, km >= 8, ny * nx % 64 == 0); same workspace as fv3hip_mappm for n_batch * ny * nx columns.
 */
int fv3hip_mappm_multi_coarse_target(const void *pe1, const void *const *q1, const void *pe2_coarse, int in_dtype, float *const *q2,
                                     int n_fields, int64_t n_batch, int ny, int nx, int factor, int km, int kn, int iv, int kord,
                                     int arith, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Vertical remap to the coarse grid's pressure levels and the masked 8 x 8 block mean of the result in one pass -- what the
 * pressure-level restart pipelines do with every cell-centred field (coarsen_restarts.py:483-495, 940-961:
 * weighted_block_average(*regrid_to_area_weighted_pressure(ds, delp, area, ...)); regridz.py:149-220):
 *   mean[f][b][k][Y][X] = sum_block(q2 * w) / sum_block(w),   q2 = mappm of q1[f] onto the interfaces pe2_coarse[b][.][Y][X],
 *   w[y][x] = area[b / area_repeat][y][x]  where  level_coarse[b][k + cmp_offset][Y][X] < pe1[b][km][y][x] (the fine surface), else 0
 * (cmp_offset 1 with level_coarse = pe2_coarse, cmp_levels = kn + 1: the layer's bottom interface, extrapolate=False;
 * cmp_offset 0 with the coarse midpoint pressures, cmp_levels = kn: extrapolate=True).  pe1 / q1[f] are [n_batch][km(+1)][ny][nx],
 * pe2_coarse / level_coarse [n_batch][levels][ny / 8][nx / 8] in the input dtype, area float32.  One wavefront owns one block;
 * the remapped values are summed in LDS in the order of fv3hip_weighted_block_average and never written: the means are
 * bit-identical to fv3hip_mappm_multi_coarse_target + fv3hip_mask_weights_coarse + fv3hip_weighted_block_average in the same
 * `arith` (blocks with an ill-formed column -- NaN or non-monotone pressures -- are redone through the sequential routine, i.e.
 * in EXACT arithmetic).  scratch[f]: [n_batch][kn][ny][nx] float32 each, touched only by values a lane has to park outside
 * LDS and by redone blocks.  q1 / scratch / mean are HOST arrays of n_fields device pointers.
 * FV3HIP_EUNSUPPORTED unless factor == 8, ny % 8 == 0, nx % 8 == 0, kord <= 3, km >= 8, kn + 1 <= 128.
 */
size_t fv3hip_mappm_block_mean_workspace_bytes(int64_t ncol, int km);
int fv3hip_mappm_block_mean(const void *pe1, const void *const *q1, const void *pe2_coarse, const void *level_coarse,
                            int cmp_levels, int cmp_offset, int in_dtype, const float *area, int64_t area_repeat,
                            float *const *scratch, float *const *mean, int n_fields, int64_t n_batch, int ny, int nx, int factor,
                            int km, int kn, int iv, int kord, int arith, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Column MLP (fv3fit dense model / Zhao-Carr microphysics emulator)
 * ------------------------------------------------------------------------------------------ */

#define FV3HIP_TRANSFORM_NONE 0
#define FV3HIP_TRANSFORM_LOG 1 /* log(max(x, eps)) : fv3fit/emulation/transforms/transforms.py:111-129 */

#define FV3HIP_ACT_LINEAR 0
#define FV3HIP_ACT_RELU 1
#define FV3HIP_ACT_TANH 2   /* convolutional models only */

/*
 * Description of the fused predict graph of
 *   fv3fit.keras._models.dense.build_model (external/fv3fit/fv3fit/keras/_models/dense.py:239-310)
 *   fv3fit.emulation MicrophysicsConfig.build with the "dense" architecture
 *     (external/fv3fit/fv3fit/emulation/models/microphysics.py:123-139,
 *      layers/architecture.py:27-50,228-282,304-343, layers/fields.py:33-66)
 * i.e.  x_i -> (optional log) -> clip slice -> (x - center) / scale -> concat ->
 *       [Dense + activation] * n_hidden -> Dense per output -> y * out_scale + out_center ->
 *       limit to [out_min, out_max] -> multiply by 0/1 level mask
 *       -> optional residual outputs  after = before + difference.
 * All arrays are HOST pointers, copied (and re-laid-out for the MFMA kernel) at create time.
 */
typedef struct {
    /* inputs */
    int n_sources;           /* number of distinct arrays the caller passes to predict()     */
    int n_inputs;            /* network input variables, concatenated in this order          */
    const int *in_source;    /* [n_inputs] which source array feeds input i                  */
    const int *in_feat_start;/* [n_inputs] first feature (level) of the source that is used  */
    const int *in_nfeat;     /* [n_inputs] number of features used (K = sum)                 */
    const int *in_transform; /* [n_inputs] FV3HIP_TRANSFORM_*                                */
    const float *in_eps;     /* [n_inputs] epsilon of the log transform                      */
    const float *in_center;  /* [K] subtracted                                               */
    const float *in_scale;   /* [K] divided by (the reference's scale + epsilon, in f32)     */
    /* hidden layers: n_hidden dense layers of `width` units, Keras kernels [in][out]        */
    int n_hidden;
    int width;
    int hidden_activation;   /* FV3HIP_ACT_* */
    const float *const *hidden_kernels; /* [n_hidden] -> [in][width] row-major               */
    const float *const *hidden_biases;  /* [n_hidden] -> [width]                             */
    /* output heads, concatenated: F = sum(out_nfeat) */
    int n_outputs;
    const int *out_nfeat;    /* [n_outputs] */
    const float *out_kernel; /* [width (or K if n_hidden == 0)][F] row-major                 */
    const float *out_bias;   /* [F] */
    const float *out_scale;  /* [F] y = yhat * scale + center                                */
    const float *out_center; /* [F] */
    const float *out_min;    /* [F] or NULL; -inf = no lower limit                           */
    const float *out_max;    /* [F] or NULL; +inf = no upper limit                           */
    const float *out_mask;   /* [F] of 0/1 or NULL (ClipConfig.zero_mask_clipped_layer)      */
    /* residual outputs: derived d = source[res_source[d]] + output[res_output[d]]           */
    int n_residual;
    const int *res_source;   /* [n_residual] */
    const int *res_output;   /* [n_residual] */
    /* 1: the activations of the last hidden layer ([width] features) are an output of their own, stored
     * to the array passed after the outputs and the residual outputs (n_outputs may then be 0).  The
     * cell of a recurrent layer -- tf.keras.layers.SimpleRNN, relu([x_t, h_{t-1}] [W; U] + b)
     * (external/fv3fit/fv3fit/emulation/layers/architecture.py:186-191) -- is such a model. */
    int hidden_output;
} fv3hip_mlp_desc_t;

typedef struct fv3hip_mlp *fv3hip_mlp_t;

int fv3hip_mlp_create(const fv3hip_mlp_desc_t *desc, fv3hip_mlp_t *out);
int fv3hip_mlp_destroy(fv3hip_mlp_t model);

/*
 * Replaces the Keras call inside fv3fit._shared.xr_prediction._predict
 * (external/fv3fit/fv3fit/_shared/xr_prediction.py:75-108: `model(inputs)`) and inside
 * emulation.models.ModelWithClassifier.__call__ (external/emulation/emulation/models.py:37-53:
 * `model.predict(inputs, batch_size=...)`).
 *   sources[s]: device pointer to source array s, dtype src_dtype[s] (F32/F64), element
 *               (feature f, sample n) at  f * src_feat_stride[s] + n * src_sample_stride[s]
 *               (so both [feature][sample] and [sample][feature] are accepted without a copy);
 *   outputs[j]: n_outputs + n_residual device pointers, dtype out_dtype (F32 or F64),
 *               element (f, n) at f * out_feat_stride[j] + n * out_sample_stride[j].
 */
int fv3hip_mlp_predict(fv3hip_mlp_t model, const void *const *sources, const int *src_dtype,
                       const int64_t *src_feat_stride, const int64_t *src_sample_stride,
                       int64_t n_samples, void *const *outputs, int out_dtype,
                       const int64_t *out_feat_stride, const int64_t *out_sample_stride,
                       void *stream);

/* FLOPs of the dense contraction per sample (2 * sum(in * out)), for roofline accounting. */
int64_t fv3hip_mlp_flops_per_sample(fv3hip_mlp_t model);
/* Calls of at most max_samples samples go to the feature-split kernel for small sample counts (mlp_small_kernel: 32 samples
 * per workgroup, a layer's output features split over its waves -- four times the CUs of the 128-sample tiles, a quarter
 * of their latency; same graph and arithmetic class, contraction in plain feature order).  -1 (default): while one round of
 * such workgroups covers the call (32 x CUs samples; FV3HIP_MLP_SMALL_MAX_SAMPLES overrides per process); 0: never.
 * Results of the two kernels agree to float32 rounding, not bit for bit: pin the limit where runs on different domain
 * decompositions must reproduce each other exactly (ABI v3). */
int fv3hip_mlp_set_small_limit(fv3hip_mlp_t model, int64_t max_samples);

/* Diagnostic: the kernel instantiation the model's last fv3hip_mlp_predict launched and the epilogue its full
 * sample tiles took, e.g. "mlp_fused_kernel<8,false,true,false,false,false> epilogue=residual" (the name rocprofv3
 * reports, so that tests and bench.py can tell which code path a result came from).  "" before the first call.
 * The string lives in the model handle. */
const char *fv3hip_mlp_last_variant(fv3hip_mlp_t model);

/*
 * EXPERIMENTAL: the same predict graph with the contraction on the bf16 matrix cores, every fp32 operand split into three
 * bf16 pieces and six cross products accumulated in fp32 (fv3net_amd/csrc/mlp_bf16x3.hip).  Same
 * descriptor as fv3hip_mlp_create (hidden_output included: it is the last entry of `outputs`, and n_outputs may then be 0);
 * restrictions: hidden width 256, ReLU, no limits / masks, log epsilons >= FLT_MIN, 1 / 3 / 5 / 13 output tiles of 32, at most
 * 64 layer-1 k-steps of 16 input features (every input padded to 16), at least two k-steps per sample tile, tables within
 * 160 KiB of LDS.  Sources and outputs are float32 [feature][sample] with unit sample stride (element (f, n) at
 * f * feat_stride + n; feat_stride >= n_samples for every source an input reads and for the hidden output).  Not a
 * replacement of fv3hip_mlp_predict: the fp32 kernel is the product path.
 */
typedef struct fv3hip_mlp3 *fv3hip_mlp3_t;
int fv3hip_mlp3_create(const fv3hip_mlp_desc_t *desc, fv3hip_mlp3_t *out);
int fv3hip_mlp3_destroy(fv3hip_mlp3_t model);
int64_t fv3hip_mlp3_flops_per_sample(fv3hip_mlp3_t model);
int fv3hip_mlp3_predict(fv3hip_mlp3_t model, const void *const *sources, const int64_t *src_feat_stride, int64_t n_samples,
                        void *const *outputs, const int64_t *out_feat_stride, void *stream);
/* Diagnostic (additive to ABI v3): the instantiation the model's last fv3hip_mlp3_predict launched and the run-time facts
 * that choose code inside it, e.g.
 *   "mlp3_kernel<13,true,true> out=mfma hout=0 layer1=block ks1=16/5 hidden=2 xwrap=0"
 * <output tiles, residual outputs, 16-byte epilogue>; out: the output layer on the matrix cores (mfma), on the vector ALU
 * with F outputs (valu<F>) or absent (none); hout: a hidden output is stored; layer1: how layer 1 requests its weight chunks
 * (block: inside the k-step's assembly block; builtin: a single hidden layer in front of an output layer on the matrix
 * cores); ks1: layer-1 k-steps / those of log inputs; hidden: hidden layers; xwrap: 16 feature rows of a source span 4 GiB or
 * more.  "" before the first call that launches (a call of 0 samples launches nothing and leaves the string).  The string
 * lives in the model handle. */
const char *fv3hip_mlp3_last_variant(fv3hip_mlp3_t model);

/*
 * Random forest: fv3fit.sklearn.RandomForest (registered "sklearn", external/fv3fit/fv3fit/sklearn/_random_forest.py:65-377),
 * i.e. sklearn's RandomForestRegressor / ExtraTreesRegressor .predict on the packed inputs followed by the target scaler's
 * denormalize (_random_forest.py:247-259, _shared/scaler.py:65-73).  Bit-identical to sklearn:
 *   - inputs are cast to float32 (numpy astype); at an internal node NaN goes left iff missing_go_to_left, any other x
 *     goes left iff x <= threshold, where `threshold` is the largest float32 <= sklearn's float64 threshold;
 *   - y = sum over trees, in tree order, of the leaf's float64 values; y /= n_trees; y = y * std + mean.
 * Nodes are sklearn's tree_ arrays, concatenated: tree t owns nodes [node_offset[t], node_offset[t+1]) with tree-local ids.
 * fv3hip_forest_create validates everything on the host before any HIP call (FV3HIP_EINVAL): n_trees >= 1; every internal
 * node's children have larger ids than the node (so every walk ends); feature indices are inside the packed inputs; leaf
 * rows are inside leaf_values.
 */
typedef struct {
    int n_trees;
    const int64_t *node_offset;        /* [n_trees + 1], node_offset[0] = 0 */
    const int32_t *children_left;      /* [n_nodes] tree-local ids; -1 marks a leaf (sklearn's TREE_LEAF) */
    const int32_t *children_right;     /* [n_nodes] */
    const int32_t *feature;            /* [n_nodes] packed input feature of an internal node */
    const float *threshold;            /* [n_nodes] largest float32 <= tree_.threshold */
    const uint8_t *missing_go_to_left; /* [n_nodes] */
    const int32_t *leaf_row;           /* [n_nodes] a leaf's row of leaf_values (ignored for internal nodes) */
    int64_t n_leaf_rows;
    const double *leaf_values;         /* [n_leaf_rows][n_out] (tree_.value[:, :, 0]) */
    /* the packed inputs: features [src_feat_start[s], src_feat_start[s] + src_nfeat[s]) of each source in turn (the
     * packer's clip, _shared/packer.py:113-169) */
    int n_sources;                     /* <= 32 */
    const int *src_feat_start;
    const int *src_nfeat;
    int n_outputs;                     /* <= 32 */
    const int *out_nfeat;              /* n_out = sum(out_nfeat) */
    const double *mean;                /* [n_out] target scaler */
    const double *std;                 /* [n_out] */
} fv3hip_forest_desc_t;

typedef struct fv3hip_forest *fv3hip_forest_t;

int fv3hip_forest_create(const fv3hip_forest_desc_t *desc, fv3hip_forest_t *out);
int fv3hip_forest_destroy(fv3hip_forest_t forest);
/* SklearnWrapper._predict_on_stacked_data (_random_forest.py:247-259: pack, model.predict, denormalize, unpack).
 *   sources[s]: as in fv3hip_mlp_predict -- dtype src_dtype[s] (F32/F64, may differ between sources), element (feature f,
 *               sample n) at f * src_feat_stride[s] + n * src_sample_stride[s];
 *   outputs[j]: float64, element (f, n) at f * out_feat_stride[j] + n * out_sample_stride[j].
 * Keeps a [tree][sample] scratch of leaf rows with the forest (grown on demand: warm up before capturing a graph). */
int fv3hip_forest_predict(fv3hip_forest_t forest, const void *const *sources, const int *src_dtype,
                          const int64_t *src_feat_stride, const int64_t *src_sample_stride, int64_t n_samples,
                          double *const *outputs, const int64_t *out_feat_stride, const int64_t *out_sample_stride,
                          void *stream);
/* RandomForestRegressor.apply on the packed inputs: leaf_node[t * n_samples + n] = the tree-local id of the leaf sample n
 * reaches in tree t (sklearn's forest.apply(X).T). */
int fv3hip_forest_apply(fv3hip_forest_t forest, const void *const *sources, const int *src_dtype,
                        const int64_t *src_feat_stride, const int64_t *src_sample_stride, int64_t n_samples,
                        int32_t *leaf_node, void *stream);

/*
 * Convolutional network: fv3fit's "convolutional" model (external/fv3fit/fv3fit/keras/_models/convolutional.py:141-210,
 * shared/convolutional_network.py:136-195).  Per sample, on [x, y, channel] fields:
 *   x^ = (x - in_center) / in_scale per channel, the variables concatenated along the channel axis (C channels);
 *   n_hidden = depth - 1 layers of k x k "valid" cross-correlation to `filters` channels (kernel [k][k][c_in][filters], first
 *   kernel axis along x), + bias (a null entry: none), activation; each shrinks x and y by k - 1;
 *   one 1 x 1 linear head per output on the last hidden layer (out_kernel [filters][sum of out_nfeat], the outputs'
 *   channels concatenated), then y * out_scale + out_center.
 * The input is the field with a halo of h = (k - 1) / 2 * n_hidden cells on every side; halo_mode says where it comes from.
 * fv3hip_conv_create validates everything on the host before any HIP call (FV3HIP_EINVAL; k > 7: FV3HIP_EUNSUPPORTED).
 */
#define FV3HIP_CONV_HALO_INPUT 0   /* the sources carry the halo: extent (nx + 2 h, ny + 2 h) */
#define FV3HIP_CONV_HALO_STRIPS 1  /* strips[sample][side][line][channel][n]: side 0..3 = x-low, x-high, y-low, y-high, line 0
                                    * next to the tile, n along the tile's other axis, C channels concatenated; nx == ny */
#define FV3HIP_CONV_HALO_CUBE 2    /* n_tiles == 6: read from the neighbouring faces (append_halos, halos.py:135-160) */
typedef struct {
    int n_inputs;                 /* input variables, at most 8 */
    const int *in_nfeat;          /* [n_inputs] channels of each */
    const float *in_center;       /* [C] */
    const float *in_scale;        /* [C] std + epsilon, not zero */
    int n_hidden;                 /* depth - 1 >= 1 */
    int kernel_size;              /* odd */
    int filters;
    int activation;               /* FV3HIP_ACT_* of the hidden layers */
    const float *const *hidden_kernels;
    const float *const *hidden_biases;   /* null, or [n_hidden] with null entries: no bias */
    int n_outputs;                /* at most 8 */
    const int *out_nfeat;
    const float *out_kernel;
    const float *out_bias;
    const float *out_scale;
    const float *out_center;
} fv3hip_conv_desc_t;

typedef struct fv3hip_conv *fv3hip_conv_t;

int fv3hip_conv_create(const fv3hip_conv_desc_t *desc, fv3hip_conv_t *out);
int fv3hip_conv_destroy(fv3hip_conv_t model);
/* Bytes of the hidden layers' outputs ([sample][x][y][filters] float32, two buffers when n_hidden > 1). */
size_t fv3hip_conv_workspace_bytes(fv3hip_conv_t model, int64_t n_batch, int n_tiles, int nx, int ny);
/* Sample (b, t), b < n_batch, t < n_tiles.  sources[i]: dtype src_dtype[i] (F32 / F64), element (b, t, x, y, channel c) at
 * b * s[0] + t * s[1] + x * s[2] + y * s[3] + c * s[4] with s = src_strides + 5 i.  outputs[j]: float32 [.., nx, ny, out_nfeat[j]]
 * addressed the same way through out_strides + 5 j.  strips: dtype strips_dtype, read in mode STRIPS only.  The caller owns
 * every buffer, the workspace included; nothing is allocated or synchronised. */
int fv3hip_conv_predict(fv3hip_conv_t model, const void *const *sources, const int *src_dtype, const int64_t *src_strides,
                        int64_t n_batch, int n_tiles, int nx, int ny, int halo_mode, const void *strips, int strips_dtype,
                        float *const *outputs, const int64_t *out_strides, void *workspace, size_t workspace_bytes,
                        void *stream);

/*
 * Reservoir computing: fv3fit.reservoir's ReservoirComputingModel / HybridReservoirComputingModel (registered
 * "pure-reservoir" / "hybrid-reservoir", external/fv3fit/fv3fit/reservoir/model.py:36-337), per step:
 *   increment  state[s] = tanh(u[s] * input_mask[s] @ W_in.T + state[s] @ W_res.T)      (reservoir.py:68-82)
 *              u[s] = the input transformer's encoding of the inputs, subdomain s of the rank divider, flattened;
 *   predict    y[s] = f(state[s]) @ C[s][:S] (+ hybrid[s] @ C[s][S:]) + b[s]               (readout.py:98-99)
 *              merged over the no-overlap subdomains and decoded by the output transformer into each output array.
 * Subdomain s covers x block s % layout_x and y block s / layout_x (pace's TilePartitioner); a subdomain's flat feature
 * index is (x * sub_y + y) * z_latent + z.  Sums are float64; the state is double-buffered in device memory.
 * fv3hip_reservoir_create validates everything on the host before any HIP call (FV3HIP_EINVAL).
 */
#define FV3HIP_RESERVOIR_DO_NOTHING 0    /* "do-nothing-transformer": concatenation along z, float64 */
#define FV3HIP_RESERVOIR_SCALE_SPATIAL 1 /* "scale-spatial-concat-z-transformer": float32 (x - c) / (s + 1e-7f) */
#define FV3HIP_RESERVOIR_SQUARE_NONE 0
#define FV3HIP_RESERVOIR_SQUARE_SUBDOMAINS 1 /* square_even_terms(state, axis=0): even subdomains (model.py:225) */
#define FV3HIP_RESERVOIR_SQUARE_ELEMENTS 2   /* square_even_terms(state, axis=-1): even state elements (model.py:122) */
#define FV3HIP_RESERVOIR_WIN_AUTO 0          /* dense when nnz / (state_size * input_size) >= 0.5 */
#define FV3HIP_RESERVOIR_WIN_DENSE 1
#define FV3HIP_RESERVOIR_WIN_CSR 2
typedef struct {
    int kind;                 /* FV3HIP_RESERVOIR_DO_NOTHING / _SCALE_SPATIAL */
    int n_variables;          /* <= 16 */
    const int *var_nz;        /* [n_variables] z size of each variable (scale-spatial: all equal) */
    int nx, ny;               /* scale-spatial: the x, y of its spatial features (must equal the extent it encodes) */
    const float *center;      /* scale-spatial: [n_variables * nx * ny * nz] */
    const float *scale;
    const double *mask;       /* scale-spatial, optional: [nx][ny][n_variables * nz] */
    int mask_f32;             /* the mask was float32 (a float32 product is rounded to float32) */
} fv3hip_reservoir_transformer_t;

typedef struct {
    int layout_x, layout_y;   /* subdomain layout */
    int overlap;
    int rank_x, rank_y;       /* rank extent without the overlap */
    int state_size;
    int input_size;           /* sub_x * sub_y * input latent z, sub = rank / layout + 2 * overlap */
    fv3hip_reservoir_transformer_t input, output, hybrid;
    /* W_in [state_size][input_size] and W_res [state_size][state_size] as CSR (column indices need not be sorted) */
    const int64_t *w_in_indptr;
    const int32_t *w_in_indices;
    const double *w_in_data;
    int w_in_storage;         /* FV3HIP_RESERVOIR_WIN_* */
    const int64_t *w_res_indptr;
    const int32_t *w_res_indices;
    const double *w_res_data;
    const double *input_mask; /* optional [n_subdomains][input_size] */
    int input_mask_f32;
    int square;               /* FV3HIP_RESERVOIR_SQUARE_* */
    int n_hybrid;             /* hybrid features per subdomain (0: pure model): sub_x' * sub_y' * hybrid latent z, no overlap */
    const double *hybrid_mask; /* optional [n_subdomains][n_hybrid] */
    int hybrid_mask_f32;
    const double *coefficients; /* [n_subdomains][state_size + n_hybrid][n_out], n_out = (rank_x / layout_x) *
                                   (rank_y / layout_y) * output latent z */
    const double *intercepts;   /* [n_subdomains][n_out] */
    const double *state;        /* optional initial state [n_subdomains][state_size] (else zeros) */
} fv3hip_reservoir_desc_t;

typedef struct fv3hip_reservoir *fv3hip_reservoir_t;

int fv3hip_reservoir_create(const fv3hip_reservoir_desc_t *desc, fv3hip_reservoir_t *out);
int fv3hip_reservoir_destroy(fv3hip_reservoir_t model);
/* The launch plan chosen at creation, read-only (host values, no HIP call): out = {dense W_in storage (0 / 1), subdomains
 * per wave of the dense product, input rows per slice, input slices, readout rows per slice, readout slices, padded W_in
 * row count, padded readout row length}.  With CSR storage the four W_in entries are 1, 0, 1 and 0. */
int fv3hip_reservoir_plan(fv3hip_reservoir_t model, int64_t out[8]);
/* One reservoir step.  sources[v]: input variable v, dtype src_dtype[v] (F32/F64), element (x, y, z) of the overlapped
 * rank extent at x * strides[3v] + y * strides[3v+1] + z * strides[3v+2].  No host synchronisation. */
int fv3hip_reservoir_increment(fv3hip_reservoir_t model, const void *const *sources, const int *src_dtype,
                               const int64_t *strides, void *stream);
/* The readout of the current state.  hybrid_sources: as sources above over the rank extent without overlap (NULL for a
 * pure model).  outputs[v]: output variable v, float32 (scale-spatial output transformer) or float64 (do-nothing),
 * element (x, y, z) at x * out_strides[3v] + y * out_strides[3v+1] + z * out_strides[3v+2]. */
int fv3hip_reservoir_predict(fv3hip_reservoir_t model, const void *const *hybrid_sources, const int *hybrid_dtype,
                             const int64_t *hybrid_strides, void *const *outputs, const int64_t *out_strides, void *stream);
/* state: [n_subdomains][state_size] float64 device arrays, ordered on `stream`. */
int fv3hip_reservoir_get_state(fv3hip_reservoir_t model, double *state, void *stream);
int fv3hip_reservoir_set_state(fv3hip_reservoir_t model, const double *state, void *stream);
int fv3hip_reservoir_reset_state(fv3hip_reservoir_t model, void *stream);

/*
 * Training series of a reservoir model (fv3fit.reservoir train.py:211-282): n_times reservoir steps
 * from [t, x, y, z] arrays, each one the launches of the increment entry above, and row t of the readout inputs after step
 * t.  sources[v]: input variable v over the overlapped rank extent, element (t, x, y, z) at t * strides[4v] +
 * x * strides[4v+1] + y * strides[4v+2] + z * strides[4v+3].  noise: optional [n_times][n_subdomains][input_size] float64,
 * added to the encoded input as u += noise[t] * input_mask (for a 0/1 mask the reference's (u + noise) * mask).
 * hybrid_sources: as sources over the rank extent without overlap (NULL for a pure model).  X: [n_times][n_subdomains]
 * [state_size + n_hybrid] float64, contiguous: the new state, its even elements squared when square_even_elements is set
 * (axis -1, the training rule of train.py:389, whatever the model's own square mode), then the hybrid transformer's
 * encoding of time t times hybrid_mask.  The model's state afterwards is that of n_times increments.
 */
int fv3hip_reservoir_train_series(fv3hip_reservoir_t model, const void *const *sources, const int *src_dtype,
                                  const int64_t *strides, const double *noise, const void *const *hybrid_sources,
                                  const int *hybrid_dtype, const int64_t *hybrid_strides, int64_t n_times,
                                  int square_even_elements, double *X, void *stream);
/* The readout targets of a training series: the output transformer's encoding of the output variables over the rank extent
 * without overlap (sources and strides as above), per no-overlap subdomain, Y [n_times][n_subdomains][n_out] float64. */
int fv3hip_reservoir_encode_targets(fv3hip_reservoir_t model, const void *const *sources, const int *src_dtype,
                                    const int64_t *strides, int64_t n_times, double *Y, void *stream);

/*
 * Gram sums of the readout's ridge regression (readout.py:39-52): per subdomain s,
 * A[s] [J1][J1] += X_s^T X_s and B[s] [J1][n_outputs] += X_s^T Y_s in float64, J1 = n_features + 1 with add_bias (a column of
 * ones after the features, never materialised) and n_features otherwise.  X element (t, s, j) is at t * x_time_stride +
 * s * x_sub_stride + j, Y likewise; both float64 device arrays.  One MFMA chain per element in ascending time, no atomics:
 * the bits depend on the shapes only, and A[s] is bitwise symmetric.  The accumulators start at zero.
 * Reading back copies subdomain `subdomain` (A [J1][J1], B [J1][n_outputs]), or every subdomain for -1, into device arrays;
 * either destination may be NULL.
 */
typedef struct fv3hip_gram *fv3hip_gram_t;

int fv3hip_gram_create(int n_subdomains, int n_features, int n_outputs, int add_bias, fv3hip_gram_t *out);
int fv3hip_gram_destroy(fv3hip_gram_t acc);
int fv3hip_gram_reset(fv3hip_gram_t acc, void *stream);
int fv3hip_gram_update(fv3hip_gram_t acc, const double *X, int64_t x_time_stride, int64_t x_sub_stride, const double *Y,
                       int64_t y_time_stride, int64_t y_sub_stride, int64_t n_times, void *stream);
int fv3hip_gram_get(fv3hip_gram_t acc, int subdomain, double *A, double *B, void *stream);

/*
 * Column codecs of the reservoir models: fv3fit.reservoir's "dense-autoencoder" (transformers/autoencoder.py:48-247) and
 * "sk-transformer" (transformers/sk_transformer.py:17-134, StandardScaler + PCA), DESIGN.md section 19.  A codec maps the
 * K = sum(var_nz) values of a column, the variables concatenated along z, to n_latent values and back; it runs once per
 * reservoir step before fv3hip_reservoir_increment and after fv3hip_reservoir_predict, one launch per direction.
 *
 * FV3HIP_CODEC_DENSE, float32 throughout as Keras computes it:
 *   encode  h = (float(x) - center) / (scale + 1e-7f) (IEEE subtraction and division), then n_enc layers
 *           h = relu(h . W + b), W [in][out]; the last one is the latent layer (enc_units[n_enc - 1] == n_latent);
 *   decode  float(latent), n_dec layers relu(h . W + b), one linear head per variable, y * scale + center (two roundings),
 *           then per variable: y < out_min -> out_min, y >= out_max -> out_max (a NaN bound: no bound; NaN y stays NaN).
 *   n_enc == 0 is the "concat and scale only" form: no layers, no heads, n_dec == 0 and n_latent == K.
 * FV3HIP_CODEC_AFFINE, float64 throughout:
 *   encode  z = (((x - mean) / std) - pca_mean) . components^T, divided by sqrt(explained_variance) when that is given;
 *   decode  xh = z . (components, row j times sqrt(explained_variance[j]) when given) + pca_mean, x = xh * std + mean,
 *           then with enforce_positive x >= 0 ? x : 0.0 (a NaN becomes 0.0, as np.where does).
 * Every dot product is an fma chain in ascending input index from 0, the bias added after the sum; no atomics: the bits
 * depend on the shapes only.
 * Caps, checked by fv3hip_codec_create on the host before any HIP call (FV3HIP_EINVAL): n_variables <= 16, K <= 1024,
 * every layer width and n_latent <= 256, n_enc <= 8 and n_dec <= 8.
 */
#define FV3HIP_CODEC_DENSE 0
#define FV3HIP_CODEC_AFFINE 1
#define FV3HIP_CODEC_MAX_VARIABLES 16
#define FV3HIP_CODEC_MAX_FEATURES 1024
#define FV3HIP_CODEC_MAX_WIDTH 256
#define FV3HIP_CODEC_MAX_LAYERS 8
typedef struct {
    int kind;                          /* FV3HIP_CODEC_DENSE / _AFFINE */
    int n_variables;
    const int *var_nz;                 /* [n_variables] z size of each variable */
    int n_latent;
    /* dense */
    const float *center;               /* [K] */
    const float *scale;                /* [K] */
    int n_enc;                         /* encoder layers, the latent layer included (0: scale only) */
    const int *enc_units;              /* [n_enc] */
    const float *const *enc_kernels;   /* [n_enc] each [in][out] */
    const float *const *enc_biases;    /* [n_enc] each [out] */
    int n_dec;                         /* decoder layers before the heads */
    const int *dec_units;              /* [n_dec] */
    const float *const *dec_kernels;
    const float *const *dec_biases;
    const float *const *head_kernels;  /* [n_variables] each [in][var_nz[v]] (n_enc > 0) */
    const float *const *head_biases;   /* [n_variables] each [var_nz[v]] */
    const float *out_min;              /* optional [n_variables], NaN: no lower bound */
    const float *out_max;              /* optional [n_variables], NaN: no upper bound */
    /* affine */
    const double *mean;                /* optional [K] (StandardScaler with_mean) */
    const double *std;                 /* optional [K] (StandardScaler with_std: scale_) */
    const double *pca_mean;            /* [K] */
    const double *components;          /* [n_latent][K] */
    const double *explained_variance;  /* [n_latent] when the PCA whitens, else NULL */
    int enforce_positive;
} fv3hip_codec_desc_t;

typedef struct fv3hip_codec *fv3hip_codec_t;

int fv3hip_codec_create(const fv3hip_codec_desc_t *desc, fv3hip_codec_t *out);
int fv3hip_codec_destroy(fv3hip_codec_t codec);
/* sources[v]: variable v, dtype src_dtype[v] (F32/F64), element (x, y, z) at x * strides[3v] + y * strides[3v+1] +
 * z * strides[3v+2], over nx x ny columns.  latent: contiguous [nx][ny][n_latent], float32 (dense) or float64 (affine).
 * No host synchronisation and no allocation. */
int fv3hip_codec_encode(fv3hip_codec_t codec, const void *const *sources, const int *src_dtype, const int64_t *strides,
                        int nx, int ny, void *latent, void *stream);
/* latent: contiguous [nx][ny][n_latent] of latent_dtype (F32/F64), cast to the codec's own precision.  outputs[v]: float32
 * (dense) or float64 (affine), addressed through out_strides as the sources above. */
int fv3hip_codec_decode(fv3hip_codec_t codec, const void *latent, int latent_dtype, int nx, int ny, void *const *outputs,
                        const int64_t *out_strides, void *stream);

/* `n_workgroups` idle wavefronts of `microseconds` (<= 100000) each on `stream`: the host layer times a small one beside a large one
 * on another stream to learn which streams the runtime lets run side by side (cubedsphere/_device.py: the pipelines' side streams). */
int fv3hip_spin(int64_t microseconds, int n_workgroups, void *stream);

/* ------------------------------------------------------------------------------------------
 * Timing helper: HIP events on the caller's stream (bench.py measures kernels with these
 * because torch.cuda.Event only sees torch's current stream).
 * ------------------------------------------------------------------------------------------ */
typedef struct fv3hip_timer *fv3hip_timer_t;
int fv3hip_timer_create(fv3hip_timer_t *out);
int fv3hip_timer_start(fv3hip_timer_t t, void *stream);
int fv3hip_timer_stop(fv3hip_timer_t t, void *stream);
int fv3hip_timer_elapsed_ms(fv3hip_timer_t t, float *ms); /* synchronises on the stop event */
int fv3hip_timer_destroy(fv3hip_timer_t t);

/*
 * Column helpers of the restart pipelines coarsen_restarts_on_pressure / _via_blended_method
 * (external/vcm/vcm/cubedsphere/coarsen_restarts.py:559-676, 990-1017).  Arrays are
 * [n_batch][nz][n_inner]; per-column results [n_batch][n_inner].
 *   fv3hip_column_sum          surface_pressure_from_delp (vertically_dependent.py:189-208): sum_k x + addend
 *   fv3hip_blend_weights       compute_blending_weights (coarsen_restarts.py:559-576)
 *   fv3hip_hydrostatic_balance _impose_hydrostatic_balance (coarsen_restarts.py:990-1017 with
 *                              height_at_interface, hydrostatic_dz, dz_and_top_to_phis,
 *                              vertically_dependent.py:69-99, 182-186, 211-235)
 * Columns without levels (nz == 0) still get their per-column result -- the addend, g * (phis / g) -- and the
 * [n_batch][nz][n_inner] arrays, being empty, may be null.
 */
int fv3hip_column_sum(const void *x, int dtype, int64_t n_batch, int nz, int64_t n_inner,
                      double addend, void *out, void *stream);
int fv3hip_blend_weights(const void *blending_pressure, const void *ps_coarse,
                         const void *pfull_coarse, int dtype, int64_t n_batch, int nz,
                         int64_t n_inner, void *out, void *stream);
int fv3hip_hydrostatic_balance(const void *dz, const void *phis, const void *t, const void *q,
                               const void *delp, int dtype, int64_t n_batch, int nz,
                               int64_t n_inner, double toa_pressure, void *dz_out,
                               void *phis_out, void *stream);

/*
 * Pre- and post-passes of the "dense-local" emulators (one MLP shared by all levels, a (level, column)
 * point is one sample of fv3hip_mlp_predict on the packed [n_inputs][nz * ncol] array) and the
 * classifier decode of emulation.models.ModelWithClassifier.  State arrays are [nz][ncol]
 * (call_py_fort's [feature, sample]) or, with has_levels = 0, [ncol]; tables are DEVICE float arrays.
 *   fv3hip_local_pack      one network input row: (t(x) - center[z]) / scale[z], t = identity or
 *                          log(max(x, eps)); float64 sources are cast to float32 first, as Keras does
 *                          (fv3fit/emulation/layers/architecture.py:53-75 combine_sequence_inputs,
 *                          layers/fields.py:6-41 FieldInput, transforms/transforms.py:111-129)
 *   fv3hip_local_unpack    one network output channel (layers/fields.py:44-66 FieldOutput, then the
 *                          backward transforms in the reference's order, transforms.py:219-224, 55-58):
 *                            direct   = yhat * scale[z] + center[z]            (scale/center NULL = 1/0)
 *                            unscaled = direct * max(cs_scale[b], min_scale) + cs_center[b],
 *                                       b = max(upper_bound(edges[0..n_bins), cond_on) - 1, 0)
 *                                       (keras/math.py:5-23 piecewise)          (cond_on NULL = skipped)
 *                            LimitValueTransform.backward (transforms.py:131-158) on the last of these:
 *                                       x <= value_lower -> 0, a NaN stays (limit_flags bit 0); x >= value_upper -> 0 * x,
 *                                       NaN for NaN and +inf (bit 1); the table: oracle/mlp_np.py:limit_value_backward
 *                            after    = before + that value, limited likewise with after_lower / after_upper
 *                                       (bits 2, 3)                             (before NULL = skipped)
 *                          level z of yhat starts at yhat + z * yhat_level_stride; any of out_direct /
 *                          out_unscaled / out_after may be NULL
 *   fv3hip_classify_onehot logits [n_class][n] -> onehot [n_class][n] (logits == max over classes,
 *                          ties all hot) and any_of [n] = onehot[cls_a] | onehot[cls_b]
 *                          (emulation/zhao_carr.py:193-198 _get_classify_output); any_of may be NULL
 */
int fv3hip_local_pack(const void *x, int dtype, int has_levels, int transform, double eps,
                      const float *center, const float *scale, int nz, int64_t ncol, float *out,
                      void *stream);
int fv3hip_local_unpack(const float *yhat, int64_t yhat_level_stride, const float *scale,
                        const float *center, const void *cond_on, int cond_dtype,
                        const float *edges, const float *cs_scale, const float *cs_center,
                        int n_bins, double min_scale, const void *before, int before_dtype,
                        int limit_flags, double value_lower, double value_upper,
                        double after_lower, double after_upper, int nz, int64_t ncol,
                        float *out_direct, float *out_unscaled, float *out_after, void *stream);
int fv3hip_classify_onehot(const void *logits, int dtype, int n_class, int64_t n,
                           uint8_t *onehot, uint8_t *any_of, int cls_a, int cls_b, void *stream);

/*
 * Predict-side glue of the fv3fit composite models (external/fv3fit/fv3fit/_shared/models.py:65-107, 223-276,
 * 442-483), on the prediction arrays right after the network.
 *   fv3hip_level_scale    TaperConfig.apply (_shared/config.py:11-24 with vcm/calc/calc.py:52-56): x [n_outer][nz][n_inner]
 *                         of `dtype` times the DEVICE float64 factors scale[nz]; the product is float64, as
 *                         numpy's float64 * float32 is
 *   fv3hip_member_reduce  EnsembleModel.predict (models.py:253-260): NaN-skipping mean / median (FV3HIP_OP_MEAN /
 *                         FV3HIP_OP_MEDIAN) over up to 32 member arrays of n values; `members` is a HOST array of
 *                         device pointers
 * SquashedOutputConfig.squash (_shared/config.py:135-142) is fv3hip_ew GT_S followed by WHERE_S.
 */
int fv3hip_level_scale(const void *x, int dtype, const double *scale, int64_t n_outer, int nz,
                       int64_t n_inner, double *out, void *stream);
int fv3hip_member_reduce(const void *const *members, int n_members, int dtype, int op, int64_t n,
                         void *out, void *stream);

/*
 * The flux-form output transforms of TransformedPredictor (external/fv3fit/fv3fit/_shared/models.py:279-337 applying
 * external/vcm/vcm/data_transform.py:140-300), replacing external/vcm/vcm/calc/flux_form.py on xarray:
 *   fv3hip_tendency_to_flux  _tendency_to_flux (flux_form.py:7-46): net_flux [n_outer][nz][n_inner] = flux at the interface
 *                            ABOVE each cell = toa_net_flux - cumsum(tendency * delp / g) of the cells above, and
 *                            surface_downward_flux [n_outer][n_inner] = the flux below the last cell + surface_upward_flux,
 *                            zero where negative if `rectify`.  closure = 1: _tendency_to_implied_surface_downward_flux
 *                            (:49-75), toa + upward - sum(tendency * delp / g); net_flux is not written (may be null).
 *                            toa_net_flux may be null (zero).  All arrays share `dtype` and are computed in it, operation by
 *                            operation as numpy does (a running sum: bit-identical for closure = 0).
 *   fv3hip_flux_to_tendency  _flux_to_tendency (:78-104): -(g * diff(concat(net_flux, down - up)) / delp).
 */
int fv3hip_tendency_to_flux(const void *tendency, const void *delp, const void *toa_net_flux,
                            const void *surface_upward_flux, int dtype, int64_t n_outer, int nz, int64_t n_inner,
                            int rectify, int closure, void *net_flux, void *surface_downward_flux, void *stream);
int fv3hip_flux_to_tendency(const void *net_flux, const void *surface_downward_flux, const void *surface_upward_flux,
                            const void *delp, int dtype, int64_t n_outer, int nz, int64_t n_inner, void *tendency,
                            void *stream);

/*
 * The novelty detectors OutOfSampleModel consults every timestep (external/fv3fit/fv3fit/_shared/models.py:340-440),
 * replacing sklearn on the host:
 *   fv3hip_minmax_score  MinMaxNoveltyDetector.predict (fv3fit/sklearn/_min_max_novelty_detector.py:94-121): one call per
 *                        packed variable x (feature f of sample i at x[f * feat_stride + i * sample_stride], `dtype`) folds
 *                        MinMaxScaler.transform's x * scale[f] + offset[f] (float64) into run_max / run_min [n]
 *                        (`first` != 0 starts them); `finish` != 0 writes score = max(max - 1, 0) + max(-min, 0).
 *   fv3hip_ocsvm_score   OCSVMNoveltyDetector.predict (_ocsvm_novelty_detector.py:124-160): score[i] = -sum_v dual_coef[v]
 *                        exp(-gamma |z_i - support_vectors[v]|^2), z = (x - mean) / scale; x [n_feat][n] float64 packed,
 *                        support_vectors [n_sv][n_feat] (already in the scaler's space, as sklearn stores them).
 */
int fv3hip_minmax_score(const void *x, int dtype, int64_t feat_stride, int64_t sample_stride, int n_feat,
                        const double *scale, const double *offset, int64_t n, int first, int finish, double *run_max,
                        double *run_min, double *score, void *stream);
int fv3hip_ocsvm_score(const double *x, int n_feat, int64_t n, const double *mean, const double *scale,
                       const double *support_vectors, const double *dual_coef, int n_sv, double gamma, double *score,
                       void *stream);

/*
 * The column water budget that closes fv3fit's "precipitative" model (external/fv3fit/fv3fit/keras/_models/
 * precipitative.py:239-253 with the layers of :35-66), on the three denormalised heads right after the network:
 *   fv3hip_precip_closure  t_res, q_res, col_precip [nz][n] float32 contiguous (what fv3hip_mlp_predict leaves in the
 *                          feature_sample layout); delp level k of sample i at delp[k * delp_feat_stride + i *
 *                          delp_sample_stride] (`delp_dtype`; the RAW thickness over all nz levels, :246, not the clipped
 *                          network input), physics_precip sample i at physics_precip[i * pp_stride] (`pp_dtype`).  Strides
 *                          count elements and are >= 0.  All arithmetic is float32 (Keras casts float64 inputs first), with
 *                          c_heat = (float)(-2.5e6 / 1004.6) and c_g = (float)(-1.0 / 9.80665):
 *                              precip[i] = (float)physics_precip[i] + c_g * sum_k(col_precip[k][i] * (float)delp[k][i])
 *                              couple != 0:  dq1 = t_res + c_heat * col_precip,  dq2 = q_res + col_precip   ([nz][n])
 *                          Every product is rounded before it is added; the sum runs in a float32 accumulator from +0.0f
 *                          over ascending k (TensorFlow leaves reduce_sum's order open; this fixes it, so that a numpy
 *                          float32 loop over the levels is bit-identical).  dq1 may be t_res and dq2 may be q_res (each
 *                          element is read before it is written); no other two arrays may overlap.  couple == 0 writes
 *                          precip only: t_res, q_res, dq1, dq2 are not read and may be null.  nz == 0: the sum is empty,
 *                          the [nz][n] arrays may be null.
 */
int fv3hip_precip_closure(const float *t_res, const float *q_res, const float *col_precip, const void *delp, int delp_dtype,
                          int64_t delp_feat_stride, int64_t delp_sample_stride, const void *physics_precip, int pp_dtype,
                          int64_t pp_stride, int nz, int64_t n, int couple, float *dq1, float *dq2, float *precip,
                          void *stream);

/*
 * Replaces mappm.interpolate_2d (external/mappm/mappm/interpolate_2d.f90:1-28; called from
 * external/vcm/vcm/interpolate.py:165-169): per column, linear interpolation of y(x) (n_in points,
 * x increasing) onto xp (n_out points); outside the column's range the result is fill_value.
 * float64.  Layouts as for fv3hip_mappm: COL_LEVEL [ncol][n] (n_batch = ncol, n_inner = 1) or
 * LEVEL_COL [n_batch][n][n_inner].  Bit-identical to the compiled Fortran.
 */
int fv3hip_interpolate_2d(const void *xp, const void *x, const void *y, int64_t n_batch,
                          int64_t n_inner, int n_in, int n_out, double fill_value, int layout,
                          void *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Zhao-Carr emulator post-processing (masks and conservation fixes on the emulator outputs)
 * ------------------------------------------------------------------------------------------
 * Replace the numpy / numba functions of external/emulation/emulation/masks.py:23-76 and
 * external/emulation/emulation/zhao_carr.py:60-344 that ModelConfig._build_masks composes
 * (external/emulation/emulation/config.py:175-221).  Arrays are contiguous [n0][n1] = [level][sample]
 * (the Fortran hook's layout) or flat (n); every array carries a dtype code (FV3HIP_F32/F64);
 * arithmetic and outputs use out_dtype = F64 if any operand is float64 (numpy's promotion), else F32.
 * NaN in gives NaN out wherever numpy gives it: the maxima / minima propagate a NaN from either operand
 * (np.maximum / np.minimum), the selects drop it where np.where does, and a column of logits with a NaN
 * has no hot class (logits == np.max(logits)).  Comparisons with a constant (bound, 273.16, -15, 1e-15,
 * 1e-20) are made in the compared array's own dtype, as numpy makes them.  An auxiliary array that only
 * decides (aux, logits) is compared as float64 and is not part of out_dtype.
 */
#define FV3HIP_ZC_NO_MASK 0            /* enforce_conservative_*: the emulator's cloud as is          */
#define FV3HIP_ZC_FORTRAN_VANISHES 1   /* mask_where_fortran_cloud_vanishes_gscond: aux = state cloud after gscond */
#define FV3HIP_ZC_FORTRAN_IDENTICAL 2  /* mask_where_fortran_cloud_identical: aux = state cloud after gscond       */
#define FV3HIP_ZC_CLASS_ZERO_CLOUD 3   /* mask_zero_cloud_classifier: aux = logits [n_class][n0][n1]               */
#define FV3HIP_ZC_CLASS_ZERO_TEND 4    /* mask_zero_tend_classifier:  aux = logits [n_class][n0][n1]               */

/* squash_gscond / squash_precpd (zhao_carr.py:60-86): cloud < bound -> 0, the removed water goes to qv.
 * cloud_out keeps cloud's dtype; qv_out has out_dtype. */
int fv3hip_zc_squash(const void *cloud, int cloud_dtype, const void *humidity, int hum_dtype,
                     int64_t n, double bound, int out_dtype, void *cloud_out, void *qv_out,
                     void *stream);
/* infer_gscond_cloud_from_conservation (zhao_carr.py:80-84). */
int fv3hip_zc_infer_cloud(const void *cloud_in, const void *qv_in, int state_dtype,
                          const void *qv_emul, int emul_dtype, int64_t n, int out_dtype,
                          void *cloud_out, void *stream);
/* The gscond masks + _update_with_net_condensation (zhao_carr.py:97-246): choose the cloud (mode),
 * limit the net condensation by the available vapour / liquid, apply it with the liquid latent heat
 * or (phase_dependent) the ice/water-flag scan along the last axis (zhao_carr.py:114-151). */
int fv3hip_zc_gscond_conserve(const void *cloud_in, const void *qv_in, const void *t_in,
                              int state_dtype, const void *cloud_emul, int emul_dtype, int mode,
                              const void *aux, int aux_dtype, int n_class, int cls, int64_t n0,
                              int64_t n1, int phase_dependent, int out_dtype, void *cloud_out,
                              void *qv_out, void *t_out, void *stream);
/* enforce_conservative_precpd (zhao_carr.py:249-323): strict TOA (last level) to surface budget.
 * n0 == 0: precip_out[n1] is zero (the other arrays are empty and may be NULL); likewise below. */
int fv3hip_zc_precpd_conserve(const void *cloud_g, const void *qv_g, const void *t_g,
                              const void *delp, int state_dtype, const void *cloud_p,
                              const void *qv_p, int emul_dtype, int64_t n0, int64_t n1,
                              int out_dtype, void *cloud_out, void *qv_out, void *t_out,
                              void *precip_out, void *stream);
/* conservative_precip_simple (zhao_carr.py:326-344): precip[n1] from the column water budget. */
int fv3hip_zc_precip_simple(const void *cloud_g, const void *qv_g, const void *delp,
                            int state_dtype, const void *cloud_p, const void *qv_p,
                            int emul_dtype, int64_t n0, int64_t n1, int out_dtype,
                            void *precip_out, void *stream);
/* mask_zero_cloud_classifier_precpd (zhao_carr.py:230-237): x -> 0 where class `cls` is hot. */
int fv3hip_zc_class_zero(const void *x, int dtype, const void *logits, int logits_dtype,
                         int n_class, int cls, int64_t n, void *out, void *stream);
/*
 * Replaces vcm.non_negative_sphum and vcm.non_negative_sphum_mse_conserving
 * (external/vcm/vcm/calc/thermo/non_negative_sphum.py:6-45), applied to the ML tendencies every
 * timestep (workflows/prognostic_c48_run/runtime/steppers/machine_learning.py:226-237).
 * mse_conserving = 0: where sphum + dQ2 dt < 0 both tendencies are scaled by -sphum / (dt dQ2);
 * mse_conserving = 1: dQ2 -> -sphum / dt there, and dQ1 is re-derived so that the moist static
 * energy tendency (cp - Rd) dQ1 + Lv dQ2 is unchanged.  q1 / q1_out may be NULL.  All arrays: n values
 * of `dtype` (FV3HIP_F32 / FV3HIP_F64).
 */
int fv3hip_non_negative_sphum(const void *sphum, const void *q1, const void *q2, int dtype,
                              int64_t n, double dt, int mse_conserving, void *q1_out,
                              void *q2_out, void *stream);
/* RangeMask (masks.py:23-41): np.maximum(x, lo) / np.minimum(x, hi), NaN-propagating. */
int fv3hip_clamp(const void *x, int dtype, int64_t n, double lo, double hi, int has_lo,
                 int has_hi, void *out, void *stream);
/* LevelMask (masks.py:44-76): float64 copy of the emulator field with levels [start, stop) taken from
 * src (or fill_value when src is NULL). */
int fv3hip_level_fill(const void *emul, int emul_dtype, const void *src, int src_dtype,
                      double fill_value, int64_t n0, int64_t n1, int64_t start, int64_t stop,
                      void *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Reductions of the offline diagnostics (additive to ABI v3)
 * ------------------------------------------------------------------------------------------ */

/*
 * Sums per (group, level) over an indexed cell list: the domain means, zonal / meridional bins and the diurnal cycle of
 * workflows/diagnostics/fv3net/diagnostics/offline/compute_diagnostics.py (with _shared/transform.py:288-318 and
 * vcm/select.py:18-77).
 *   a, b      [n_batch][nz][n_inner] of `dtype` (b may be NULL); weights [n_batch][n_inner] of `w_dtype` (NULL: 1)
 *   order     [n_order] int32 cell ids batch * n_inner + i, sorted by group (stable); start [n_groups + 1]: group g owns
 *             order[start[g] : start[g + 1]); cells in no group are absent
 *   items     work item k reduces cells [start[g] + c * CHUNK, min(that + CHUNK, start[g + 1])) of g = item_group[k],
 *             c = item_chunk[k] (CHUNK = fv3hip_group_sums_chunk()); the items of a group are consecutive, in chunk
 *             order: group g owns items [group_item[g], group_item[g + 1])
 *   sums      double [10][n_groups][nz]; in float64 with d = a - b and every product rounded once:
 *             0: sum w   1: sum w over a not NaN   2: sum w a   3: sum (w a) a   4-6: as 1-3 for b   7-9: as 1-3 for d
 *             A term enters its sum unless it is NaN (an infinity stays); with b NULL 4-9 are 0.
 *   workspace at least fv3hip_group_sums_workspace_bytes(n_items, nz) bytes
 * All index arrays are device memory.  One workgroup per (item, level) with a fixed reduction tree, a second kernel adds
 * a group's items in order: no floating-point atomics, results are bitwise identical from run to run.
 */
int fv3hip_group_sums_chunk(void);
size_t fv3hip_group_sums_workspace_bytes(int64_t n_items, int nz);
int fv3hip_group_sums(const void *a, const void *b, int dtype, const void *weights, int w_dtype,
                      int64_t n_batch, int nz, int64_t n_inner, const int32_t *order,
                      int64_t n_order, const int64_t *start, int64_t n_groups,
                      const int32_t *item_group, const int32_t *item_chunk, int64_t n_items,
                      const int64_t *group_item, double *sums, void *workspace,
                      size_t workspace_bytes, void *stream);
/*
 * np.histogram / np.histogram2d with array bins (vcm/calc/histogram.py): x (and y) [n] of `dtype`, converted to double;
 * DEVICE float64 edges [n_bins + 1]; bin i holds edges[i] <= v < edges[i + 1], the last bin also v == edges[n_bins]; NaN
 * and values outside are dropped (in 2-D the pair).  counts: int64 [n_bins] / [nx_bins][ny_bins], zeroed by the call.
 * Up to 4096 bins, in 2-D 128 x 128; more is FV3HIP_EINVAL.
 */
int fv3hip_histogram(const void *x, int dtype, int64_t n, const double *edges, int n_bins,
                     int64_t *counts, void *stream);
int fv3hip_histogram2d(const void *x, const void *y, int dtype, int64_t n, const double *xedges,
                       int nx_bins, const double *yedges, int ny_bins, int64_t *counts,
                       void *stream);

/*
 * fv3fit's graph U-Net autoregressor (external/fv3fit/fv3fit/pytorch/graph/unet.py:216-261, pytorch/predict.py:136-250):
 * stateless layer kernels on the resident six-tile cube.  Activations are float32, channel-last: cell (sample s, tile t, x, y)
 * of an array with row length `ld` and channel offset `off` holds its channels at
 *     base[s * sample_stride + ((t * n + x) * n + y) * ld + off + c],        x the first spatial axis,
 * so a layer reads one channel slice and writes another (the U-Net's concatenation is two layers writing the halves of one
 * buffer).  A sample stride of 0 means contiguous cubes (6 n n ld).  The caller owns every buffer; nothing is allocated or
 * synchronised; all arguments are checked on the host before any HIP call.  A layer must not read what it writes: slices of
 * one buffer (same base and ld) must be disjoint in channels, different buffers must not overlap (FV3HIP_EINVAL).
 *
 *   fv3hip_graph_sage   dgl's SAGEConv(c_in, c_out, "mean") on the graph of graph_builder.py:12-49 (every cell, its x-low,
 *                       x-high, y-low, y-high neighbours, across the cube seams as the one-cell halo of append_halos shows
 *                       them): dst = act(src W_self + mean5(src) W_neigh + bias), w_self / w_neigh [c_in][c_out] (the
 *                       transpose of torch's Linear weight), bias [c_out] or null, act one of FV3HIP_ACT_* (another code:
 *                       FV3HIP_EUNSUPPORTED).  mean5 = ((((self + x-low) + x-high) + y-low) + y-high) / 5 in float32, formed
 *                       while the tile is staged: no gathered or averaged copy is written to memory.  Exact-f32 MFMA over
 *                       K = 2 c_in in chunks of 8 channels (their 8 self rows, then their 8 mean rows).  ReLU keeps NaN.
 *   fv3hip_graph_pool2  AvgPool2d(2, 2) per tile, n even: ((a[2i][2j] + a[2i][2j+1]) + a[2i+1][2j]) + a[2i+1][2j+1], times 0.25.
 *   fv3hip_graph_up2    ConvTranspose2d(c_in, c_out, 2, stride 2) per tile: dst[2i+di][2j+dj][co] = bias[co] + sum over ci of
 *                       src[i][j][ci] w[ci][di][dj][co]  (w: torch's [c_in][c_out][kx][ky] moved to [c_in][kx][ky][c_out]);
 *                       dst has 2 n cells per edge.  The same MFMA kernel with K = c_in and N = 4 c_out.
 *   fv3hip_graph_pack   state[w][t][tile][x][y][f] float32 = (float)((x - mean[f]) / std[f]) computed in float64, from time
 *                       w * timesteps + t of variable v (f = its first feature + level): sources[v] of src_dtype[v] (F32 / F64),
 *                       element strides src_strides + 5 v for (time, tile, x, y, level); nfeat[v] levels; mean / std DEVICE
 *                       float64 [F], F = sum of nfeat; at most 16 variables.  sources / src_dtype / src_strides / nfeat are HOST arrays.
 *   fv3hip_graph_unpack outputs[v][row][tile][x][y][level] float64 contiguous = (double)state * std[f] + mean[f], the product
 *                       rounded before the sum; state [n_rows][6][n][n][F] contiguous.
 */
int fv3hip_graph_sage(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride, const float *w_self,
                      const float *w_neigh, const float *bias, float *dst, int64_t dst_ld, int64_t dst_off,
                      int64_t dst_sample_stride, int64_t n_samples, int n, int c_in, int c_out, int act, void *stream);
int fv3hip_graph_pool2(const float *src, int64_t src_ld, int64_t src_off, float *dst, int64_t dst_ld, int64_t dst_off,
                       int64_t n_samples, int n, int c, void *stream);
int fv3hip_graph_up2(const float *src, int64_t src_ld, int64_t src_off, const float *w, const float *bias, float *dst,
                     int64_t dst_ld, int64_t dst_off, int64_t n_samples, int n, int c_in, int c_out, void *stream);
int fv3hip_graph_pack(const void *const *sources, const int *src_dtype, const int64_t *src_strides, int n_vars, const int *nfeat,
                      const double *mean, const double *std, int64_t n_windows, int n_times, int timesteps, int n, float *state,
                      void *stream);
int fv3hip_graph_unpack(const float *state, int64_t n_rows, int n, int n_vars, const int *nfeat, const double *mean,
                        const double *std, double *const *outputs, void *stream);

/*
 * fv3fit's CycleGAN generators (external/fv3fit/fv3fit/pytorch/cyclegan/generator.py:19-270, modules.py): stateless layer
 * kernels on channel-last float32 slices of the resident six-tile cube, addressed as the fv3hip_graph_* layers address them
 * (row length, channel offset, sample stride; 0 = contiguous cubes).  The caller owns every buffer; nothing is allocated or
 * synchronised; all arguments are checked on the host before any HIP call.  Pack and unpack are fv3hip_graph_pack / _unpack.
 *
 *   fv3hip_cyclegan_conv   one convolution as an implicit GEMM on the exact-f32 MFMA, rows = output cells flattened over
 *                          (sample, tile, x, y).  `n` is the INPUT's cells per edge.  kind / k:
 *                            _REGULAR     k in {3, 5, 7}, stride 1, halo (k - 1) / 2, w [k][k][c_in][c_out]; output n
 *                            _STRIDED     k = 4, stride 2, halo 1: output (x, y) reads cells 2 x - 1 ... 2 x + 2, same in y;
 *                                         w [4][4][c_in][c_out]; n even, output n / 2
 *                            _TRANSPOSED  k = 4: ConvTranspose2d(4, stride 2) of the input padded by one halo line, cropped by
 *                                         3.  Per axis output 2 m takes tap 1 of cell m and tap 3 of cell m - 1, output
 *                                         2 m + 1 tap 0 of cell m + 1 and tap 2 of cell m.  w [px][py][a][b][c_in][c_out]:
 *                                         parity (px, py) of the output cell, then its 2 x 2 taps, a / b = 0 the first-named
 *                                         tap of the axis (torch's w[ci][co][kx][ky] with kx = 1 + 2 a for px = 0, 2 a for
 *                                         px = 1); output 2 n
 *                            any other k: FV3HIP_EUNSUPPORTED.
 *                          halo_mode: _HALO_CUBE takes cells off the face from the neighbouring faces as AppendHalos does
 *                          (corners zero), _HALO_ZEROS pads with zeros.  The halo must not be wider than the face.
 *                          While loading, a source value v becomes relu((v - in_mean) * in_rstd + in_bias): in_mean / in_rstd
 *                          [sample][6][c_in] (both or neither), in_bias [6][n][n][c_in] or null, in_relu 0 / 1 -- with the
 *                          statistics and the bias cell of the face the value lies on; padding zeros stay zero.  Products are
 *                          rounded separately.  The result is acc + bias[c_out] (or null) + out_bias [6][n_out][n_out][c_out]
 *                          (or null), in this order.  ReLU keeps NaN.  Source and destination must not overlap.
 *   fv3hip_cyclegan_conv_context  fv3hip_cyclegan_conv with context channels (the step layers of the recurrent generator,
 *                          recurrent/generator.py:127-182): the convolution of the channel-wise concatenation
 *                          [ T(src) | ctx_cell | ctx_uniform ] with the concatenated weight, where T is the loader's transform
 *                          above and touches the c_in source channels only.  ctx_cell [6][n][n][c_cell] (or null with
 *                          c_cell = 0): per-cell values at the INPUT's resolution; ctx_uniform DEVICE [c_uni] (or null with
 *                          c_uni = 0): one value per channel, the same on every cell of every sample; w_ctx
 *                          [taps][c_cell + c_uni][c_out]: the weight rows of the context channels, cell channels first.  A tap
 *                          off the face is resolved as for the source: with _HALO_CUBE the cell context is that of the
 *                          neighbouring face's cell and the uniform value is present, both are zero at the corners; with
 *                          _HALO_ZEROS both are zero everywhere off the face.  The taps x c_in source rows are summed first,
 *                          exactly as fv3hip_cyclegan_conv sums them, then the taps x (c_cell + c_uni) context rows (tap
 *                          slowest).  _REGULAR only: _STRIDED / _TRANSPOSED with a context return FV3HIP_EUNSUPPORTED.  With
 *                          c_cell = c_uni = 0 (w_ctx null) it is fv3hip_cyclegan_conv, bit for bit.
 *   fv3hip_cyclegan_stats  nn.InstanceNorm2d's statistics: per (sample, tile, channel) the mean over the face and
 *                          rstd = 1 / sqrt(biased variance + eps), the variance taken about the mean in a second pass, both
 *                          accumulated in float64 in a fixed order (no atomics); mean / rstd [sample][6][c] float32.
 *   fv3hip_cyclegan_apply  dst = relu((src - mean) * rstd + bias) + res with every part optional (mean / rstd null: no norm;
 *                          bias [6][n][n][c] or null; relu 0 / 1; res a slice or null).  dst may be src or res itself.
 *   fv3hip_cyclegan_input  dst[..., :c] = state + bias ([6][n][n][c] or null); with lon [6][n][n], xyz [6][n][n][3] and theta
 *                          [n_samples] (DEVICE; all three or none) dst[..., c:c+5] = sin(lon + theta_s), cos(lon + theta_s), x, y, z.
 */
#define FV3HIP_CYCLEGAN_CONV_REGULAR 0
#define FV3HIP_CYCLEGAN_CONV_STRIDED 1
#define FV3HIP_CYCLEGAN_CONV_TRANSPOSED 2
#define FV3HIP_CYCLEGAN_HALO_ZEROS 0
#define FV3HIP_CYCLEGAN_HALO_CUBE 1
int fv3hip_cyclegan_conv(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride, const float *in_mean,
                         const float *in_rstd, const float *in_bias, int in_relu, const float *w, const float *bias,
                         const float *out_bias, float *dst, int64_t dst_ld, int64_t dst_off, int64_t dst_sample_stride,
                         int64_t n_samples, int n, int c_in, int c_out, int kind, int k, int halo_mode, void *stream);
int fv3hip_cyclegan_conv_context(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride, const float *in_mean,
                                 const float *in_rstd, const float *in_bias, int in_relu, const float *w, const float *bias,
                                 const float *out_bias, float *dst, int64_t dst_ld, int64_t dst_off, int64_t dst_sample_stride,
                                 int64_t n_samples, int n, int c_in, int c_out, int kind, int k, int halo_mode,
                                 const float *ctx_cell, int c_cell, const float *ctx_uniform, int c_uni, const float *w_ctx,
                                 void *stream);
int fv3hip_cyclegan_stats(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride, float *mean, float *rstd,
                          int64_t n_samples, int n, int c, double eps, void *stream);
int fv3hip_cyclegan_apply(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride, const float *mean,
                          const float *rstd, const float *bias, int relu, const float *res, int64_t res_ld, int64_t res_off,
                          int64_t res_sample_stride, float *dst, int64_t dst_ld, int64_t dst_off, int64_t dst_sample_stride,
                          int64_t n_samples, int n, int c, void *stream);
int fv3hip_cyclegan_input(const float *state, int64_t state_ld, int64_t state_off, int64_t state_sample_stride, const float *bias,
                          const float *lon, const float *xyz, const float *theta, float *dst, int64_t dst_ld, int64_t dst_off,
                          int64_t dst_sample_stride, int64_t n_samples, int n, int c, void *stream);

/* ---- training the dense column network (fv3fit's "dense" training function, keras/_models/dense.py:165-310) and its Jacobian.
 * Stateless like the fv3hip_graph_* layers: the caller owns every DEVICE pointer, nothing is allocated or synchronised, all
 * arguments are checked on the host before any HIP call.  Activations are float32 row-major [row][feature] with a leading
 * dimension ld >= features; weights are [in][out] (Keras Dense: h = x W + b) with their own ld.  Every contraction runs on the
 * exact-float32 MFMA in a fixed order; there are no atomics, so results are bitwise reproducible and depend on the shapes
 * only.  A whole optimiser step (forwards, loss gradient, backward weight / data per layer, Adam) on one stream can be captured
 * in a HIP graph.
 *   idx (int64, DEVICE, or null): row n of the batch is row idx[n] of A (of the targets); an index outside [0, a_rows) reads
 *   as a row of zeros (a target row of NaN).
 *   fv3hip_train_linear_forward          H[n][o] = act(sum_k A[row(n)][k] W[k][o] + b[o]); act FV3HIP_ACT_LINEAR or _RELU; bias
 *                                        may be null.
 *   fv3hip_train_linear_backward_data    dA[n][k] = sum_o dH[n][o] W[k][o] where P[n * p_stride][k] > 0, else 0 (relu'(0) = 0 as
 *                                        in torch; a NaN activation masks too).  P: the post-ReLU activation that fed the layer,
 *                                        or null for no mask; p_stride 1, or 0 when every row shares the activation row P[0]
 *                                        (the Jacobian: dH holds one-hot cotangent rows).
 *   fv3hip_train_linear_backward_weight  dW[k][o] = sum_n A[row(n)][k] dH[n][o], db[o] = sum_n dH[n][o].  The batch is cut into
 *                                        chunks of fv3hip_train_chunk_rows() (512) rows: a batch of one chunk writes dW and db
 *                                        directly; a longer one writes each chunk's partial to `workspace` (at least
 *                                        fv3hip_train_backward_weight_workspace_bytes(n, k, o) bytes) and a second kernel adds
 *                                        the partials in ascending chunk order.
 *   fv3hip_train_mse_grad                per element, with p = yhat * scale + center and pc = p clamped to [lo, hi] (+-inf: no
 *                                        limit): dY = keep * [lo <= p <= hi] * 2 (pc - t) * inv_cstd2 * scale * wnorm (the
 *                                        products taken left to right in float32; torch.clamp's gradient, bounds inclusive),
 *                                        and loss[0] (float64) = sum over the kept elements of (pc - t)^2 inv_cstd2 wnorm,
 *                                        accumulated in float64: per-block partials in loss_workspace (at least
 *                                        fv3hip_train_loss_workspace_doubles() doubles), then one block adds them in order.
 *                                        wnorm[j] = 1 / (n * kept features of j's output) makes it the sum over outputs of
 *                                        mean(((p - t) / cstd)^2).  keep[j] == 0: the element gives an exact 0 and is not read.
 *   fv3hip_train_adam                    torch.optim.Adam's default update of one flat buffer at step t = step[0] + 1:
 *                                        m = b1 m + (1 - b1) g, taken as torch's lerp takes it: fma(1 - b1, g - m, m);
 *                                        v = b2 v + ((1 - b2) g) g;
 *                                        p -= (float)(lr / (1 - b1^t)) * m / (sqrt(v) / (float)sqrt(1 - b2^t) + eps), every
 *                                        product rounded; then step[0] += 1 on the device (int64), so a captured step replays.
 *   fv3hip_train_precip_loss_grad        the loss behind the closure of fv3fit's "precipitative" model (keras/_models/
 *                                        precipitative.py:181-279) and its gradient.  yhat [n][ldy] is the
 *                                        raw output of the concatenated head layer, [ t (nz) | q (nz) | dead (1, only with
 *                                        has_dead) | cp (nz) ]; dY [n][lddy] has the same layout.  scale1 / center1, scale2 /
 *                                        center2, inv_cstd2_1, inv_cstd2_2 are [nz]; the cp block is denormalised with scale2 /
 *                                        center2.  delp [rows][ldd] (the raw thickness), physics_precip [rows], T1 / T2
 *                                        [rows][ldt] and T3 [rows] are the resident arrays, read through idx: a row outside
 *                                        [0, rows) reads delp and physics_precip as 0 and its targets as NaN.  Per batch row,
 *                                        every product and sum rounded to float32, c_heat = (float)(-2.5e6 / 1004.6), c_g =
 *                                        (float)(-1 / 9.80665), w12 = (float)(1 / (n nz)), w3 = (float)(1 / n):
 *                                          t = t^ scale1 + center1, q = q^ scale2 + center2, cp = cp^ scale2 + center2
 *                                          dq1 = couple ? t + c_heat cp : t,  dq2 = couple ? q + cp : q
 *                                          acc = +0; for k ascending: acc = acc + cp[k] delp[k];  precip = pp + c_g acc
 *                                            (fv3hip_precip_closure's order: the same bits on the same heads)
 *                                          e1 = dq1 - T1, e2 = dq2 - T2, e3 = precip - T3
 *                                          g1 = 2 e1 inv1 w12, g2 = 2 e2 inv2 w12, g3 = 2 e3 inv3 w3   (left to right)
 *                                          dt^ = g1 scale1 + r(t^), dq^ = g2 scale2 + r(q^), ddead = r(dead)
 *                                          dcp^ = ((couple ? c_heat g1 + g2 : 0) + (c_g delp) g3) scale2
 *                                          r(x) = (l1 sign(x) + 2 l2 x) / n, sign(0) = 0; with l1 = l2 = 0 no r is added and
 *                                          ddead = 0
 *                                        loss[0] (float64) = sum of e1^2 inv1 w12, e2^2 inv2 w12, e3^2 inv3 w3 and
 *                                        (l1 |x| + l2 x^2) / n over t^, q^ and dead, accumulated in float64: per-block partials
 *                                        in loss_workspace (fv3hip_train_loss_workspace_doubles() doubles), then one block adds
 *                                        them in order.  couple, has_dead 0 / 1; l1, l2 >= 0.  dq1, dq2 [n][nz] and precip [n]
 *                                        (each may be null) receive the predictions.  nz >= 1.  Two launches.
 */
int fv3hip_train_chunk_rows(void);
size_t fv3hip_train_backward_weight_workspace_bytes(int64_t n, int k, int o);
int fv3hip_train_loss_workspace_doubles(void);
int fv3hip_train_linear_forward(const float *A, int64_t lda, int64_t a_rows, const int64_t *idx, const float *W, int64_t ldw,
                                const float *bias, float *H, int64_t ldh, int64_t n, int k, int o, int act, void *stream);
int fv3hip_train_linear_backward_data(const float *dH, int64_t lddh, const float *W, int64_t ldw, const float *P, int64_t ldp,
                                      int p_stride, float *dA, int64_t ldda, int64_t n, int k, int o, void *stream);
int fv3hip_train_linear_backward_weight(const float *A, int64_t lda, int64_t a_rows, const int64_t *idx, const float *dH,
                                        int64_t lddh, float *dW, int64_t lddw, float *db, float *workspace, size_t workspace_bytes,
                                        int64_t n, int k, int o, void *stream);
int fv3hip_train_mse_grad(const float *yhat, int64_t ldy, const float *scale, const float *center, const float *inv_cstd2,
                          const float *lo, const float *hi, const float *keep, const float *wnorm, const float *targets, int64_t ldt,
                          int64_t t_rows, const int64_t *idx, float *dY, int64_t lddy, double *loss, double *loss_workspace,
                          int64_t n, int f, void *stream);
int fv3hip_train_adam(float *params, const float *grad, float *m, float *v, int64_t count, int64_t *step, double lr, double beta1,
                      double beta2, double eps, void *stream);
int fv3hip_train_precip_loss_grad(const float *yhat, int64_t ldy, const float *scale1, const float *center1, const float *scale2,
                                  const float *center2, const float *inv_cstd2_1, const float *inv_cstd2_2, float inv_cstd2_3,
                                  const float *delp, int64_t ldd, const float *physics_precip, const float *T1, const float *T2,
                                  int64_t ldt, const float *T3, int64_t rows, const int64_t *idx, int couple, int has_dead, float l1,
                                  float l2, float *dY, int64_t lddy, double *loss, double *loss_workspace, float *dq1, float *dq2,
                                  float *precip, int64_t n, int nz, void *stream);

/* ---- the multi-variable loss of the microphysics emulators (fv3fit's "transformed" training function, train_microphysics.py:
 * 451-521; CustomLoss / _MultiVariableLoss, emulation/losses.py:33-146) and its gradient with respect to
 * the raw output of the concatenated head layer.  Stateless like the other fv3hip_train_* entries: the caller owns every DEVICE
 * pointer, nothing is allocated, copied or synchronised, every argument is checked on the host before any HIP call, and the two
 * launches can be captured.  The head table is a HOST array; it goes to the kernel by value.
 *
 *   yhat [n * levels][ldy]   network row m = b * levels + z of batch row b and level z; levels = 1 for the "dense" and "linear"
 *                            architectures, nz for "dense-local".
 *   idx                      the row table of the n batch rows (int64, DEVICE) or null: batch row b is row idx[b] of the resident
 *                            arrays; an index outside [0, rows) reads its targets as NaN and `before` as 0.
 *   dY [n * levels][lddy]    null: loss only.  Else it receives the gradient of `loss` for every column < f (0 for a head
 *                            without a loss term); columns >= f are never written.
 *   heads                    n_heads <= FV3HIP_EMULATOR_MAX_HEADS descriptors in ascending column order that tile [0, f) exactly.
 *
 * A head owns columns [col0, col0 + ncol) and is one of
 *   FV3HIP_EMULATOR_HEAD_MSE_DENSE  (levels == 1) ncol features; its tables (scale, center, inv, inv_after) and target rows are
 *                                   indexed by the feature j.
 *   FV3HIP_EMULATOR_HEAD_MSE_LOCAL  (ncol == 1)   tables and target rows are indexed by the level z.  single_level: only z = 0
 *                                   carries the terms (RNNOutput.call reads rnn_outputs[..., 0:1, :]), the count is n, target
 *                                   rows hold one value, and dY is 0 at the other levels.
 *   FV3HIP_EMULATOR_HEAD_XENT       (2 <= ncol <= 32 channels) softmax cross-entropy per (row, level) point against
 *                                   target [rows][ld_target] holding [levels][ncol] per row; direct term only, no tables.
 * An MSE head has an optional direct term (slot >= 0: target, inv) and an optional after term (slot_after >= 0: before,
 * target_after, inv_after), Difference.backward's after = before + difference.  weight must be finite and >= 0; is_loss 0 makes
 * the term a metric: it is reported and adds nothing to dY (its g term below is skipped, so a NaN of a metric target stays out
 * of dY).  With count = n ncol (dense), n levels (local, cross-entropy) or n (single level), wgrad = (float)(weight / count) and
 * wval = 1 / count, per element in float32, every product and sum rounded and taken left to right (t: the table index, r: the
 * resident row):
 *     p  = scale ? yhat * scale[t] + center[t] : yhat
 *     d  = p - target[r][t]                        value_d += d^2 inv[t];         g  = 2 d inv[t] wgrad
 *     a  = before[r][t] + p;  e = a - target_after[r][t]
 *                                                  value_a += e^2 inv_after[t];   g  = g + 2 e inv_after[t] wgrad_after
 *     dY = scale ? g * scale[t] : g
 * and per cross-entropy point with logits x_c and truth t_c (c ascending):
 *     mx = max_c x_c;  s = sum_c expf(x_c - mx);  lse = mx + logf(s);  st = sum_c t_c
 *     value += t_c (lse - x_c) for every c;        dY_c = (expf(x_c - lse) st - t_c) wgrad
 * The values are float64 sums of these float32 terms: per lane, then the block's fixed tree, one partial per block and term in
 * `workspace` (fv3hip_train_emulator_loss_workspace_doubles() doubles); the second launch adds each slot's partials in ascending
 * block order and writes values[slot] = sum * wval and loss[0] = the sum over the loss slots, in slot order, of weight *
 * values[slot].  The slots of the table must be 0 .. n_slots - 1, each used once.  accum (DEVICE, 1 + n_slots doubles, or null):
 * loss and every value are added into it by one thread in that order, so an epoch's means need no read-back per step.  No
 * atomics: the result depends on the shapes only.  A NaN or inf in one element reaches dY in that element only (in that point's
 * channels for cross-entropy) and its own slot only.
 * Bounds: 1 <= n, levels and n * levels <= 2^24; 1 <= f <= 2^20; ldy, lddy >= f; ld_target, ld_target_after, ld_before at least
 * the extent of a row (ncol; levels; 1 for a single level; levels * ncol for cross-entropy); rows >= 1, and rows >= n without a
 * row table. */
#define FV3HIP_EMULATOR_MAX_HEADS 16
#define FV3HIP_EMULATOR_HEAD_MSE_DENSE 0
#define FV3HIP_EMULATOR_HEAD_MSE_LOCAL 1
#define FV3HIP_EMULATOR_HEAD_XENT 2
typedef struct {
    int kind, col0, ncol, single_level;
    int slot, slot_after;             /* -1: no such term */
    int is_loss, is_loss_after;
    double weight, weight_after;
    const float *scale, *center;      /* both or neither */
    const float *target, *inv;
    const float *before, *target_after, *inv_after;
    int64_t ld_target, ld_before, ld_target_after;
} fv3hip_emulator_head_t;
int fv3hip_train_emulator_loss_workspace_doubles(void);
int fv3hip_train_emulator_loss_grad(const float *yhat, int64_t ldy, int64_t n, int levels, int f, const fv3hip_emulator_head_t *heads,
                                    int n_heads, int n_slots, int64_t rows, const int64_t *idx, float *dY, int64_t lddy,
                                    double *values, double *loss, double *accum, double *workspace, void *stream);

/* ---- training the convolutional network (fv3fit's "convolutional" training function, keras/_models/convolutional.py:101-210,
 * shared/convolutional_network.py:59-195).  Stateless like fv3hip_train_linear_*: the caller owns every
 * DEVICE pointer, the workspace included; nothing is allocated or synchronised; all arguments are checked on the host before any
 * HIP call.  Activations are float32, channel-last [sample][x][y][channel], each buffer with its element strides for sample, x
 * and y (_ss, _sx, _sy; the channel stride is 1, sy >= channels), so padded views work.  Kernels are [a][b][c_in][f] (Keras
 * Conv2D: first kernel axis along x, cross-correlation, "valid") with a leading dimension ldw >= f on the last axis.  X, Y are
 * the extents of the layer's INPUT; its output has X - k + 1 by Y - k + 1 cells; k is odd.  Every contraction is an implicit
 * GEMM on the exact-float32 MFMA in a fixed order (no im2col buffer, no atomics): results are bitwise reproducible and depend
 * on the shapes only.  Each entry is one launch (backward_weight: two with more than one chunk) on `stream`, so a whole step
 * captures as a chain.
 *   idx (int64, DEVICE, or null): sample s of the batch is sample idx[s] of A; an index outside [0, a_samples) reads as a sample
 *   of zeros.
 *   fv3hip_train_conv_forward          H[s][x][y][f] = act(sum_{a,b,c} A[row(s)][x + a][y + b][c] W[a][b][c][f] + bias[f]); act
 *                                      FV3HIP_ACT_LINEAR or _RELU (v < 0 ? 0 : v: a NaN stays); bias may be null.
 *   fv3hip_train_conv_backward_data    dA[s][x][y][c] = sum_{a,b,f} dH[s][x - a][y - b][f] W[a][b][c][f] over the terms whose dH
 *                                      cell exists, and an exact 0 where P[s][x][y][c] > 0 is false (relu'(0) = 0 as in torch; a
 *                                      NaN activation masks too).  P: the post-ReLU activation that fed the layer (the extent of
 *                                      dA), or null for no mask.
 *   fv3hip_train_conv_backward_weight  dW[a][b][c][f] = sum_{s,x,y} A[row(s)][x + a][y + b][c] dH[s][x][y][f]; db[f] =
 *                                      sum_{s,x,y} dH[s][x][y][f] (null: skipped).  The batch's output pixels (s, x, y) are cut
 *                                      into chunks of fv3hip_train_conv_chunk_pixels() (512): one chunk writes dW and db
 *                                      directly; more write each chunk's partial to `workspace` (at least
 *                                      fv3hip_train_conv_backward_weight_workspace_bytes(n, X, Y, k, c, f) bytes) and a second
 *                                      kernel adds the partials in ascending chunk order.
 *   fv3hip_train_conv_constrain        TransposeInvariant in place: w[a][b] and w[b][a] both become 0.5f * (w[a][b] + w[b][a])
 *                                      for every (c, f) -- bitwise symmetric, and bitwise 0.5 * (w + w.transpose(0, 1)).
 */
int fv3hip_train_conv_chunk_pixels(void);
size_t fv3hip_train_conv_backward_weight_workspace_bytes(int64_t n, int X, int Y, int k, int c, int f);
int fv3hip_train_conv_forward(const float *A, int64_t a_ss, int64_t a_sx, int64_t a_sy, int64_t a_samples, const int64_t *idx,
                              const float *W, int64_t ldw, const float *bias, float *H, int64_t h_ss, int64_t h_sx, int64_t h_sy,
                              int64_t n, int X, int Y, int k, int c, int f, int act, void *stream);
int fv3hip_train_conv_backward_data(const float *dH, int64_t dh_ss, int64_t dh_sx, int64_t dh_sy, const float *W, int64_t ldw,
                                    const float *P, int64_t p_ss, int64_t p_sx, int64_t p_sy, float *dA, int64_t da_ss, int64_t da_sx,
                                    int64_t da_sy, int64_t n, int X, int Y, int k, int c, int f, void *stream);
int fv3hip_train_conv_backward_weight(const float *A, int64_t a_ss, int64_t a_sx, int64_t a_sy, int64_t a_samples, const int64_t *idx,
                                      const float *dH, int64_t dh_ss, int64_t dh_sx, int64_t dh_sy, float *dW, int64_t lddw, float *db,
                                      float *workspace, size_t workspace_bytes, int64_t n, int X, int Y, int k, int c, int f,
                                      void *stream);
int fv3hip_train_conv_constrain(float *W, int64_t ldw, int k, int c, int f, void *stream);

/* ---- training the graph U-Net (fv3fit's "graph" training function, pytorch/graph/train.py:65-119, training_loop.py:75-198;
 * DESIGN.md section 24): the backward of fv3hip_graph_sage / _up2 / _pool2 and AdamW.  Stateless like fv3hip_graph_* and
 * fv3hip_train_*: the caller owns every DEVICE pointer, the workspace included; nothing is allocated or synchronised; all
 * arguments are checked on the host before any HIP call; a layer that would read what it writes gives FV3HIP_EINVAL, an unknown
 * activation code FV3HIP_EUNSUPPORTED.  Activations and their gradients are float32, channel-last, addressed as (base, ld,
 * channel offset, sample stride; 0: densely packed cubes) as in fv3hip_graph_sage; weights and their gradients are dense
 * [c_in][c_out] (up2: [c_in][2][2][c_out]).  Every contraction runs on the exact-float32 MFMA in a fixed order; there are no
 * atomics, so results are bitwise reproducible and depend on the shapes only.  n is the edge of the layer's INPUT cube (up2: of
 * `low`; its output and dcat have 2 n).  act'(P) is taken from the stored post-activation P that fed the layer, with its
 * activation code p_act: relu [P > 0] (relu'(0) = 0 as in torch; a NaN masks too), tanh 1 - P^2, linear 1; P null: no mask.
 *   fv3hip_graph_sage_backward_data    dst = (dH W_self^T + mean5(dH) W_neigh^T) act'(P), mean5 as the forward takes it (the
 *                                      five-point graph is symmetric, so mean5 is its own adjoint); dH is the masked gradient
 *                                      of the layer's output.  accumulate != 0: dst = dst + that (the rollout's state gradient).
 *   fv3hip_graph_sage_backward_weight  dW_self = X^T G, dW_neigh = mean5(X)^T G, db = sum over the cells of G (null: skipped),
 *                                      summed over the S 6 n^2 cells of the batch in memory order, cut into chunks of
 *                                      fv3hip_graph_train_chunk_cells() (512): one chunk writes the results directly; more
 *                                      write each chunk's partial to `workspace` (at least
 *                                      fv3hip_graph_sage_backward_weight_workspace_bytes(S, n, c_in, c_out) bytes) and a second
 *                                      kernel adds the partials in ascending chunk order.  accumulate != 0: every result is
 *                                      old + sum (the steps of a multistep rollout, in the order of the calls).
 *                                      The three results and the workspace must not overlap x, g or each other.
 *   fv3hip_graph_up2_backward_data     dst[i][j][ci] = (sum_{di,dj,co} dcat[2i+di][2j+dj][co] w[ci][di][dj][co]) act'(P)
 *   fv3hip_graph_up2_backward_weight   dW[ci][di][dj][co] = sum_{s,t,i,j} low[i][j][ci] dcat[2i+di][2j+dj][co]; db[co] = sum of
 *                                      dcat = the four (di, dj) column sums added in order.  Always through `workspace`
 *                                      (fv3hip_graph_up2_backward_weight_workspace_bytes) and the second kernel.
 *   fv3hip_graph_pool2_backward        dst = (dst + 0.25f dpool[x / 2][y / 2]) act'(P), in place: the skip connection's part is
 *                                      in dst first, the pool's is added second.
 *   fv3hip_train_adamw                 torch.optim.AdamW's default update: p = p * (float)(1 - lr weight_decay), then
 *                                      fv3hip_train_adam's update with the same device step counter.
 */
int fv3hip_graph_train_chunk_cells(void);
size_t fv3hip_graph_sage_backward_weight_workspace_bytes(int64_t n_samples, int n, int c_in, int c_out);
size_t fv3hip_graph_up2_backward_weight_workspace_bytes(int64_t n_samples, int n, int c_in, int c_out);
int fv3hip_graph_sage_backward_data(const float *dh, int64_t dh_ld, int64_t dh_off, int64_t dh_sample_stride, const float *w_self,
                                    const float *w_neigh, const float *p, int64_t p_ld, int64_t p_off, int64_t p_sample_stride,
                                    int p_act, float *dst, int64_t dst_ld, int64_t dst_off, int64_t dst_sample_stride,
                                    int accumulate, int64_t n_samples, int n, int c_in, int c_out, void *stream);
int fv3hip_graph_sage_backward_weight(const float *x, int64_t x_ld, int64_t x_off, int64_t x_sample_stride, const float *g,
                                      int64_t g_ld, int64_t g_off, int64_t g_sample_stride, float *dw_self, float *dw_neigh,
                                      float *db, int accumulate, float *workspace, size_t workspace_bytes, int64_t n_samples,
                                      int n, int c_in, int c_out, void *stream);
int fv3hip_graph_up2_backward_data(const float *dcat, int64_t dcat_ld, int64_t dcat_off, const float *w, const float *p,
                                   int64_t p_ld, int64_t p_off, int p_act, float *dst, int64_t dst_ld, int64_t dst_off,
                                   int64_t n_samples, int n, int c_in, int c_out, void *stream);
int fv3hip_graph_up2_backward_weight(const float *low, int64_t low_ld, int64_t low_off, const float *dcat, int64_t dcat_ld,
                                     int64_t dcat_off, float *dw, float *db, int accumulate, float *workspace,
                                     size_t workspace_bytes, int64_t n_samples, int n, int c_in, int c_out, void *stream);
int fv3hip_graph_pool2_backward(const float *dpool, int64_t dpool_ld, int64_t dpool_off, const float *p, int64_t p_ld,
                                int64_t p_off, int p_act, float *dst, int64_t dst_ld, int64_t dst_off, int64_t n_samples, int n,
                                int c, void *stream);
int fv3hip_train_adamw(float *params, const float *grad, float *m, float *v, int64_t count, int64_t *step, double lr, double beta1,
                       double beta2, double eps, double weight_decay, void *stream);

/* ---- training fv3fit's CycleGAN (pytorch/cyclegan/train_cyclegan.py, cyclegan_trainer.py): the adjoints of the fv3hip_cyclegan_*
 * layers, with their conventions: channel-last float32 slices (pointer, ld, channel offset, sample stride; 0 = contiguous
 * cubes), the caller owns every DEVICE buffer, all arguments are checked on the host before any HIP call, nothing is allocated
 * or synchronised.  Every contraction runs on the exact-float32 MFMA with separately rounded products in a fixed order; there
 * are no atomics, so results are bitwise reproducible and a sample's results do not depend on the batch it is in.  `n` is the
 * edge of the layer INPUT x; dy has the forward's output edge (n, n / 2 or 2 n).  kind / k / halo_mode / weight layout as
 * fv3hip_cyclegan_conv, plus _STRIDED k = 3 (halo 1: output (x, y) reads cells 2 x - 1 ... 2 x + 1; w [3][3][c_in][c_out]; the
 * discriminator's default).  Write x~ for the halo-extended face and T(o, t) for the padded position tap t of output o reads.
 *   fv3hip_cyclegan_train_conv            the forward: fv3hip_cyclegan_conv without the loader's transform and the per-cell
 *                                         output bias, bit for bit, plus _STRIDED k = 3.
 *   fv3hip_cyclegan_train_backward_data   dx[s,g,q] = sum over the padded positions (f, p) that show cell (g, q) -- its own, and
 *                                         with _HALO_CUBE one halo position on the neighbouring face across every edge the cell
 *                                         lies within the halo width of (none at halo corners) -- of
 *                                         sum_{(o,t): T(o,t) = p} W_t dy[s,f,o].  One writer per element: the terms of one
 *                                         position are summed tap by tap, channel fastest; the positions are added in the order
 *                                         own, x-low, x-high, y-low, y-high.  _HALO_CUBE needs a workspace of
 *                                         fv3hip_cyclegan_train_backward_data_workspace_bytes(...) bytes (the gradient of the
 *                                         padded field); _HALO_ZEROS needs none.  The weights are read in the forward's layout.
 *   fv3hip_cyclegan_train_backward_weight dw_t[ci][co] = sum_{s,f,o} x~[s,f,T(o,t)][ci] dy[s,f,o][co] in the forward's weight
 *                                         layout (the parity split of _TRANSPOSED included) and db[co] = sum dy in float64, rounded once (db null: not
 *                                         wanted).  The rows (sample, tile, x, y) are cut into chunks of
 *                                         fv3hip_cyclegan_train_chunk_cells() whose partials, in the workspace of
 *                                         fv3hip_cyclegan_train_backward_weight_workspace_bytes(...) bytes, are added in
 *                                         ascending order.  dw and db are overwritten.
 *   fv3hip_cyclegan_train_norm_backward   the adjoint of y = act(x^ + bias), x^ = (x - mean) * rstd, act a leaky ReLU of `slope`
 *                                         in [0, 1] (0: ReLU, 1: none): g = dy act'(x^ + bias) with the mask taken from the
 *                                         float32 pre-activation as fv3hip_cyclegan_apply forms it (positive: 1, else slope);
 *                                         dx = rstd ((g - mean_face(g)) - x^ mean_face(g x^)) in float64, rounded once, the two face means accumulated in
 *                                         float64 in the fixed order of fv3hip_cyclegan_stats.  mean / rstd [sample][6][c];
 *                                         bias [6][n][n][c] or null; dbias [6][n][n][c] or null: sum of g over the samples in
 *                                         ascending order.  dx must not overlap dy or x.
 */
int fv3hip_cyclegan_train_chunk_cells(void);
size_t fv3hip_cyclegan_train_backward_data_workspace_bytes(int64_t n_samples, int n, int c_in, int kind, int k, int halo_mode);
size_t fv3hip_cyclegan_train_backward_weight_workspace_bytes(int64_t n_samples, int n, int c_in, int c_out, int kind, int k);
int fv3hip_cyclegan_train_conv(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride, const float *w,
                               const float *bias, float *dst, int64_t dst_ld, int64_t dst_off, int64_t dst_sample_stride,
                               int64_t n_samples, int n, int c_in, int c_out, int kind, int k, int halo_mode, void *stream);
int fv3hip_cyclegan_train_backward_data(const float *dy, int64_t dy_ld, int64_t dy_off, int64_t dy_sample_stride, const float *w,
                                        float *dx, int64_t dx_ld, int64_t dx_off, int64_t dx_sample_stride, float *workspace,
                                        size_t workspace_bytes, int64_t n_samples, int n, int c_in, int c_out, int kind, int k,
                                        int halo_mode, void *stream);
int fv3hip_cyclegan_train_backward_weight(const float *x, int64_t x_ld, int64_t x_off, int64_t x_sample_stride, const float *dy,
                                          int64_t dy_ld, int64_t dy_off, int64_t dy_sample_stride, float *dw, float *db,
                                          float *workspace, size_t workspace_bytes, int64_t n_samples, int n, int c_in, int c_out,
                                          int kind, int k, int halo_mode, void *stream);
int fv3hip_cyclegan_train_norm_backward(const float *dy, int64_t dy_ld, int64_t dy_off, int64_t dy_sample_stride, const float *x,
                                        int64_t x_ld, int64_t x_off, int64_t x_sample_stride, const float *mean, const float *rstd,
                                        const float *bias, float slope, float *dx, int64_t dx_ld, int64_t dx_off,
                                        int64_t dx_sample_stride, float *dbias, int64_t n_samples, int n, int c, void *stream);

/* ---- training fv3fit's FMR recurrent generator (pytorch/recurrent/train_fmr.py), with the conventions of the CycleGAN training
 * entry points above.  The forward of a layer with context channels is fv3hip_cyclegan_conv_context without a loader transform;
 * the context has no gradient, so its backward-data is fv3hip_cyclegan_train_backward_data on the source rows w.
 *   fv3hip_cyclegan_train_backward_weight_context
 *       fv3hip_cyclegan_train_backward_weight plus the gradient of the context rows, in fv3hip_cyclegan_conv_context's layout
 *       [taps][c_cell + c_uni][c_out] (cell channels first):
 *           dw_ctx[t][j][co] = sum_{s,f,o} ctx~[s,f,T(o,t)][j] dy[s,f,o][co]
 *       with ctx~ resolved as the forward resolves it: with _HALO_CUBE the neighbouring face's cell context and the uniform
 *       value, both zero at corners; with _HALO_ZEROS both zero off the face.  _REGULAR only (k = 3, 5, 7); a context with another
 *       kind is FV3HIP_EUNSUPPORTED.  The same chunks in the same order, the same float64 db, no atomics; dw, dw_ctx and db are
 *       overwritten.  With c_cell = c_uni = 0 (ctx_cell, ctx_uniform, dw_ctx null) it is fv3hip_cyclegan_train_backward_weight
 *       bit for bit.  Workspace: fv3hip_cyclegan_train_backward_weight_context_workspace_bytes(...).
 *   fv3hip_fmr_loss_grad
 *       the window loss and its gradient.  fake and real are float32 windows [n_windows][n_times][n_elements] whose states
 *       (n_elements floats) are contiguous; the window and time strides, in floats, may put either outside (time-major or
 *       window-major).  dgan (null: zero) and dfake (null: the values only) have fake's strides; dgan may be dfake itself.
 *           values[0] = identity_weight / N0 * sum over time 0 of l(f - r),       N0 = n_windows * n_elements
 *           values[1] = target_weight / N1 * sum over times >= 1 of l(f - r),     N1 = n_windows * (n_times - 1) * n_elements
 *           l = |d| (FV3HIP_FMR_LOSS_MAE) or d^2 (FV3HIP_FMR_LOSS_MSE), every term formed in float64
 *           dfake = dgan + weight / N * sign(f - r)  (mae; sign(0) = 0)   or   dgan + 2 weight / N * (f - r)  (mse),
 *                   evaluated in float64 and rounded once, one writer per element
 *       The sums are float64 partials of blocks of consecutive elements, added in ascending order by one wave: no atomics, the
 *       result is bitwise reproducible.  values: two DEVICE doubles.  n_times < 2 is refused (the target would be a mean over
 *       no element).  Workspace: fv3hip_fmr_loss_grad_workspace_bytes(...) bytes of DEVICE memory, 8-byte aligned.
 */
#define FV3HIP_FMR_LOSS_MSE 0
#define FV3HIP_FMR_LOSS_MAE 1
size_t fv3hip_cyclegan_train_backward_weight_context_workspace_bytes(int64_t n_samples, int n, int c_in, int c_cell, int c_uni,
                                                                     int c_out, int k);
int fv3hip_cyclegan_train_backward_weight_context(const float *x, int64_t x_ld, int64_t x_off, int64_t x_sample_stride,
                                                  const float *dy, int64_t dy_ld, int64_t dy_off, int64_t dy_sample_stride,
                                                  const float *ctx_cell, int c_cell, const float *ctx_uniform, int c_uni, float *dw,
                                                  float *dw_ctx, float *db, float *workspace, size_t workspace_bytes,
                                                  int64_t n_samples, int n, int c_in, int c_out, int kind, int k, int halo_mode,
                                                  void *stream);
size_t fv3hip_fmr_loss_grad_workspace_bytes(int64_t n_windows, int64_t n_times, int64_t n_elements);
int fv3hip_fmr_loss_grad(const float *fake, int64_t fake_window_stride, int64_t fake_time_stride, const float *real,
                         int64_t real_window_stride, int64_t real_time_stride, const float *dgan, float *dfake, int64_t n_windows,
                         int64_t n_times, int64_t n_elements, int identity_kind, double identity_weight, int target_kind,
                         double target_weight, double *values, double *workspace, size_t workspace_bytes, void *stream);

/* ---- training random forests (fv3fit's "sklearn_random_forest"; sklearn's RandomForestRegressor.fit: squared error, exact
 * best split, all features).  Stateless like fv3hip_train_*: the caller owns every DEVICE buffer below, nothing is allocated or
 * synchronised, the arguments are checked on the host before any HIP call.  One tree grows level by level:
 *   fv3hip_forest_train_begin   compacts every row of `order` to the samples with weight > 0 (list_a; n_inbag of them) and makes
 *                               them the root's segment; level = {1, n_inbag, 1, 0}.
 *   fv3hip_forest_train_level   one level of the tree over n_open open nodes that cover n_positions list positions, the tree
 *                               holding n_nodes nodes so far (all three as `level` reported them); parity 0 reads list_a / seg_a /
 *                               node_a and writes the b set, parity 1 the reverse.  Writes the records of the level's nodes and
 *                               level = {open nodes of the next level, their positions, nodes so far, 0}.  The caller reads
 *                               `level` back, stops at level[0] == 0 and otherwise calls again with depth + 1 and the other
 *                               parity.  max_depth < 0: unlimited.
 * A node is a leaf at depth >= max_depth, with fewer than min_samples_split or 2 min_samples_leaf samples, with impurity <=
 * DBL_EPSILON or without an admissible position; positions p | p + 1 of a feature's sorted segment are admissible where
 * x[p + 1] > x[p] + 1e-7f (float32) and both sides hold min_samples_leaf samples.  The greatest proxy
 * sum_k SL_k^2 / WL + sum_k (S_k - SL_k)^2 / WR wins, then the lowest feature, then the lowest position.  Children are numbered
 * level by level (left, right, in node order); the caller renumbers.  Every sum has a fixed order; there are no atomics on
 * floating-point values.
 * Buffer sizes, with C = fv3hip_forest_train_chunk() and chunks = ceil(n / C): k_cap >= the most open nodes of a level (at most
 * min(n_inbag, 2^max_depth)), node_cap >= the nodes of the tree (at most min(2 n_inbag - 1, 2^(max_depth + 1) - 1)).
 * Limits, checked by both entry points before any launch (FV3HIP_EINVAL, nothing written): n < 2^31, F <= 65535 and
 * O <= 3821 -- one row of the scan's LDS tile, O + 2 doubles, has to fit 64 KB beside the chunk's ids and weights.
 * A level writes its whole `level` record, the fourth entry included (1: a buffer was too small for the children), and reads
 * nothing but the inputs, the a / b set of its parity and the tree records it wrote itself: no buffer needs to be zeroed. */
typedef struct {
    int64_t n;               /* samples */
    int F, O;                /* features, outputs */
    const float *xt;         /* [F][n] inputs, feature-major */
    const double *y;         /* [n][O] targets */
    const double *ysq;       /* [n] sum_k y[i][k]^2 */
    const int32_t *order;    /* [F][n] stable argsort of each feature */
    const int32_t *weight;   /* [n] bootstrap counts of this tree */
    int32_t *list_a, *list_b;   /* [F][n] */
    uint8_t *side;           /* [n] */
    int32_t *pos_node;       /* [n] */
    int64_t *seg_a, *seg_b;  /* [k_cap + 1] (at least 2) */
    int32_t *node_a, *node_b;   /* [k_cap] */
    double *stats;           /* [k_cap][O + 2] */
    double *carry;           /* [F][chunks][O + 2] */
    int32_t *count;          /* [F][chunks] */
    double *proxy;           /* [F][n] */
    double *best_proxy;      /* [k_cap][F]; -inf where no position of the node is admissible in the feature */
    int64_t *best_pos;       /* [k_cap][F]; INT64_MAX there */
    int64_t *n_left, *dst_left, *dst_right;   /* [k_cap] */
    int64_t k_cap, node_cap;
    /* the tree, [node_cap] each (value: [node_cap][O]) */
    int32_t *left, *right, *feature;
    double *threshold;
    uint8_t *missing_left;
    double *value, *impurity, *weighted_n;
    int32_t *n_samples;
    int64_t *level;          /* [4] */
} fv3hip_forest_train_t;

/* the phases of a level, in the order they must run (FV3HIP_FOREST_TRAIN_ALL in one call, or one call each to time them):
 * the chunk sums and node statistics; the scan and the best position per (node, feature); the split records, the children and
 * the partition of the lists */
#define FV3HIP_FOREST_TRAIN_SUMS 1
#define FV3HIP_FOREST_TRAIN_SCAN 2
#define FV3HIP_FOREST_TRAIN_SPLIT 4
#define FV3HIP_FOREST_TRAIN_ALL 7

int fv3hip_forest_train_chunk(void);
int fv3hip_forest_train_begin(const fv3hip_forest_train_t *ws, int64_t n_inbag, void *stream);
int fv3hip_forest_train_level(const fv3hip_forest_train_t *ws, int parity, int64_t n_open, int64_t n_positions, int64_t n_nodes,
                              int depth, int max_depth, int64_t min_samples_split, int64_t min_samples_leaf, int phases,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FV3HIP_H */
