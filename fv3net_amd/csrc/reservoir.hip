// Reservoir computing (fv3fit.reservoir, model.py / reservoir.py / readout.py): one increment_state and one predict per
// reservoir step, for every subdomain of a rank at once.
//
// increment (three launches):
//   res_encode_kernel     the input transformer's encoding, gathered into subdomains straight from the caller's strided
//                         (x, y, z) arrays, times input_mask: u [k][subdomain] float64.  Thread 0 also flips the parity of
//                         the double-buffered state, so a captured graph replays correctly.
//   res_in_dense_kernel   (dense W_in) partial sums of u @ W_in.T over slices of k: one wave per 128 state rows x SB
//                         subdomains, W_in column-major in 16-byte loads, u broadcast from LDS, float64 FMA in ascending k.
//   res_finish_kernel     adds the slices in order (or walks the CSR W_in row), adds state @ W_res.T (CSR row), tanh.
// predict (two launches, three for a hybrid model):
//   res_encode_kernel     (hybrid) the hybrid transformer's encoding over the no-overlap subdomains times hybrid_input_mask.
//   res_readout_kernel    partial readouts over slices of the readout input j: f(state) (square_even_terms) then the
//                         hybrid inputs, staged in LDS; C in 16-byte loads, k contiguous.
//   res_epilogue_kernel   adds the slices in order, + intercept, merges the subdomains and decodes into the output arrays.
// training series (fv3hip_reservoir_train_series): per time step the increment's launches as they are,
//   res_add_noise_kernel  (noise given) u += noise[t] * input_mask, between the encoding and the input product;
//   res_pack_kernel       row t of the readout inputs: the new state (even elements squared when asked), then the hybrid
//                         encoding of time t.
// No atomics anywhere: the bits depend on the shapes only.
//
// Each rule once: locate() (with FEATURE_INDEX / MASK_INDEX) places a flat subdomain element for the encode and the
// epilogue kernel; readout_input() is a row of the readout input for the readout and the pack kernel; on the host
// encode_args() builds the three encodings' launch arguments and encode() is their one launch, slice_plan() cuts both
// reductions, and columns.h (shared with codec.hip) turns the caller's pointer, dtype and stride tables into kernel
// arguments and owns the device buffers.
#include <vector>

#include "columns.h"

using namespace fv3hip;

namespace {

constexpr int kMaxVars = 16;
constexpr int kBlock = 256;
constexpr int kInKT = 64;          // k rows of u staged per step of res_in_dense_kernel
constexpr int kInAhead = 4;        // W_in rows in flight per lane of res_in_dense_kernel
constexpr int kReadRows = 64;      // readout input rows staged per step of res_readout_kernel
constexpr int kTargetBlocks = 1024;
constexpr int kInTargetWaves = 3072;  // about three waves per SIMD: res_in_dense_kernel holds ~160 registers per lane
constexpr double kDenseDensity = 0.5;  // FV3HIP_RESERVOIR_WIN_AUTO: dense W_in from this fraction of nonzeros up

// a transformer as the kernels see it
struct Tf {
    int kind, n_var, zlat, nx, ny, nz0, mask_f32;
    int zoff[kMaxVars + 1];
    const float *center, *scale;
    const double *mask;
};

// How the subdomains are cut from an (x, y) extent: lx of them side by side in x, one of sub_x by sub_y cells every
// (step_x, step_y) cells; the subdomains overlap where the step is shorter than the extent.  locate() needs no sub_x (x is
// the slowest index of a subdomain); the field keeps the kernel's argument offsets where they were.
struct Divider {
    int lx, sub_x, sub_y, step_x, step_y;
};

struct EncArgs {
    Tf tf;
    XyzSrc src[kMaxVars];
    Divider div;
    int64_t n_flat, n_sub;
    const double *pmask;                   // per-subdomain mask [s][k] or null
    int pmask_f32, src_all_f32;
    double *out;
    int64_t out_ls, out_lk;                // out[s * out_ls + k * out_lk]
    int *parity;                           // flipped by thread 0 when not null
};

// Where flat element k of subdomain s lies: the cell (X, Y) of the extent the subdomains were cut from, the latent level
// zl, and the variable v with the level zz within it.  locate() takes the divider's numbers by reference and fills a point
// it is handed, and the two index sums below are macros: in this form res_encode_kernel and res_epilogue_kernel compile to
// the instructions they had with the sums written out in each; as value-returning functions they are simplified before
// they are inlined and res_encode_kernel gets another schedule, which showed as a slow mode of back-to-back encodings.
struct SubPoint {
    int64_t X, Y;
    int zl, v, zz;
};

__device__ __forceinline__ void locate(const Tf &tf, const int &lx, const int &step_x, const int &step_y, const int &sub_y,
                                       int64_t s, int64_t k, SubPoint &p)
{
    p.zl = (int)(k % tf.zlat);
    const int64_t t = k / tf.zlat;
    const int yi = (int)(t % sub_y), xi = (int)(t / sub_y);
    p.X = (s % lx) * step_x + xi;
    p.Y = (s / lx) * step_y + yi;
    p.v = var_of(tf.zoff, tf.n_var, p.zl);
    p.zz = p.zl - tf.zoff[p.v];
}

// scale-spatial: the point's element of center and scale [variable][x][y][z] / of mask [x][y][latent level]
#define FEATURE_INDEX(tf, p) ((int64_t)(p).v * (tf).nx * (tf).ny * (tf).nz0 + ((p).X * (tf).ny + (p).Y) * (tf).nz0 + (p).zz)
#define MASK_INDEX(tf, p) (((p).X * (tf).ny + (p).Y) * (tf).zlat + (p).zl)

__global__ __launch_bounds__(kBlock) void res_encode_kernel(EncArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (a.parity && e == 0) *a.parity ^= 1;
    if (e >= a.n_sub * a.n_flat) return;
    const int64_t s = e / a.n_flat;
    const int64_t k = e - s * a.n_flat;
    SubPoint p;
    locate(a.tf, a.div.lx, a.div.step_x, a.div.step_y, a.div.sub_y, s, k, p);
    const double raw = load_xyz<double>(a.src[p.v], p.X, p.Y, p.zz);
    double val;
    bool f32;
    if (a.tf.kind == FV3HIP_RESERVOIR_SCALE_SPATIAL) {
        // NormLayer.forward in float32: (x - center) / (scale + 1e-7), IEEE subtraction and division
        const int64_t fi = FEATURE_INDEX(a.tf, p);
        const float den = __fadd_rn(a.tf.scale[fi], 1.0e-7f);
        const float enc = __fdiv_rn(__fsub_rn((float)raw, a.tf.center[fi]), den);
        val = (double)enc;
        f32 = true;
        if (a.tf.mask) {  // float32 * float64 is float64 in numpy; float32 * float32 rounds to float32
            val = val * a.tf.mask[MASK_INDEX(a.tf, p)];
            f32 = a.tf.mask_f32 != 0;
            if (f32) val = (double)(float)val;
        }
    } else {
        val = raw;  // np.concatenate: float32 only when every variable is
        f32 = a.src_all_f32 != 0;
    }
    if (a.pmask) {
        val = val * a.pmask[s * a.n_flat + k];
        if (f32 && a.pmask_f32) val = (double)(float)val;
    }
    a.out[s * a.out_ls + k * a.out_lk] = val;
}

// part[ks][s][i] = sum over k of slice ks of W_in[i][k] * u[k][s]; W is [kpad][ldw] (column-major W_in, zero padded)
template <int SB>
__global__ __launch_bounds__(64) void res_in_dense_kernel(const double *__restrict__ W, const double *__restrict__ u,
                                                          double *__restrict__ part, int64_t ldw, int S, int n_sub,
                                                          int k_chunk, int n_in, int kpad)
{
    __shared__ double us[kInKT * SB];
    const int lane = threadIdx.x;
    const int64_t i2 = (int64_t)blockIdx.x * 64 + lane;  // pair of state rows
    const int64_t n2 = ldw / 2;
    const int64_t i2c = i2 < n2 ? i2 : n2 - 1;
    const int s0 = blockIdx.z * SB;
    const int k_begin = blockIdx.y * k_chunk;
    const int k_end = min(k_begin + k_chunk, kpad);
    const double2 *W2 = reinterpret_cast<const double2 *>(W) + i2c;
    double a0[SB], a1[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) a0[s] = a1[s] = 0.0;
    // W rows kInAhead ahead of the FMAs, in registers across the LDS steps: the loads' latency is hidden by the FMAs
    double2 wq[kInAhead];
#pragma unroll
    for (int q = 0; q < kInAhead; ++q) wq[q] = W2[(int64_t)(k_begin + q) * n2];
    for (int k0 = k_begin; k0 < k_end; k0 += kInKT) {
        __syncthreads();
        for (int e = lane; e < kInKT * SB; e += 64) {
            const int kk = e / SB, s = e - kk * SB;
            const int k = k0 + kk;
            us[e] = (k < n_in && s0 + s < n_sub) ? u[(int64_t)k * n_sub + s0 + s] : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < kInKT; kk += kInAhead) {
#pragma unroll
            for (int q = 0; q < kInAhead; ++q) {
                const double *ur = us + (kk + q) * SB;
#pragma unroll
                for (int s = 0; s < SB; ++s) {
                    a0[s] = __fma_rn(wq[q].x, ur[s], a0[s]);
                    a1[s] = __fma_rn(wq[q].y, ur[s], a1[s]);
                }
                // then the slot's next row (into the same registers), clamped inside the slice: a clamped one is unused
                const int kn = min(k0 + kk + q + kInAhead, k_end - 1);
                wq[q] = W2[(int64_t)kn * n2];
                __builtin_amdgcn_sched_barrier(0);  // keep one row's u in registers at a time
            }
        }
    }
    if (i2 >= n2) return;
    const int64_t i = 2 * i2;
#pragma unroll
    for (int s = 0; s < SB; ++s) {
        if (s0 + s < n_sub) {
            double *p = part + ((int64_t)blockIdx.y * n_sub + s0 + s) * S;
            if (i < S) p[i] = a0[s];
            if (i + 1 < S) p[i + 1] = a1[s];
        }
    }
}

struct FinishArgs {
    const double *part;                // dense W_in: [n_split][s][i]
    int n_split;
    const int64_t *in_ptr;             // CSR W_in (when part is null)
    const int32_t *in_idx;
    const double *in_val;
    const double *u;                   // [k][s]
    const int64_t *res_ptr;
    const int32_t *res_idx;
    const double *res_val;
    double *state;                     // [2][s][i]
    const int *parity;
    int S, n_sub;
};

__global__ __launch_bounds__(kBlock) void res_finish_kernel(FinishArgs a)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= a.S) return;
    const int p = *a.parity;
    const int64_t plane = (int64_t)a.n_sub * a.S;
    const double *src = a.state + (p ? 0 : plane) + (int64_t)s * a.S;
    double *dst = a.state + (p ? plane : 0) + (int64_t)s * a.S;
    double x = 0.0;  // masked_input @ W_in.T
    if (a.part) {
        for (int q = 0; q < a.n_split; ++q) x += a.part[((int64_t)q * a.n_sub + s) * a.S + i];
    } else {
        for (int64_t n = a.in_ptr[i]; n < a.in_ptr[i + 1]; ++n) x = __fma_rn(a.in_val[n], a.u[(int64_t)a.in_idx[n] * a.n_sub + s], x);
    }
    double r = 0.0;  // state @ W_res.T
    for (int64_t n = a.res_ptr[i]; n < a.res_ptr[i + 1]; ++n) r = __fma_rn(a.res_val[n], src[a.res_idx[n]], r);
    dst[i] = tanh(x + r);
}

struct ReadArgs {
    const double *C;      // [s][S + H][ldc]
    const double *state;  // [2][s][S]
    const int *parity;
    const double *hyb;    // [s][H]
    double *part;         // [n_split][s][ldc]
    int64_t ldc;
    int S, H, n_sub, j_chunk, square;
};

// Row j of the readout input of subdomain s: the state, squared by square_even_terms in the even subdomains (pure model,
// axis 0) or in its even elements (hybrid model and train.py:389, axis -1), then the hybrid encoding.
__device__ __forceinline__ double readout_input(const double *state_row, const double *hyb_row, int s, int j, int S, int square)
{
    if (j >= S) return hyb_row[j - S];
    const double v = state_row[j];
    const bool sq = square == FV3HIP_RESERVOIR_SQUARE_SUBDOMAINS ? (s % 2 == 0)
                    : square == FV3HIP_RESERVOIR_SQUARE_ELEMENTS ? (j % 2 == 0)
                                                                    : false;
    return sq ? v * v : v;
}

__global__ __launch_bounds__(kBlock) void res_readout_kernel(ReadArgs a)
{
    __shared__ double vin[kReadRows];
    const int s = blockIdx.z;
    const int64_t k2 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t n2 = a.ldc / 2;
    const int64_t k2c = k2 < n2 ? k2 : n2 - 1;
    const int J = a.S + a.H;
    const int j_begin = blockIdx.y * a.j_chunk;
    const int j_end = min(j_begin + a.j_chunk, J);
    const double *st = a.state + (*a.parity ? (int64_t)a.n_sub * a.S : 0) + (int64_t)s * a.S;
    const double2 *C2 = reinterpret_cast<const double2 *>(a.C + (int64_t)s * J * a.ldc) + k2c;
    double acc0 = 0.0, acc1 = 0.0;
    for (int j0 = j_begin; j0 < j_end; j0 += kReadRows) {
        const int nj = min(kReadRows, j_end - j0);
        __syncthreads();
        if (threadIdx.x < nj)
            vin[threadIdx.x] = readout_input(st, a.hyb + (int64_t)s * a.H, s, j0 + threadIdx.x, a.S, a.square);
        __syncthreads();
        const double2 *row = C2 + (int64_t)j0 * n2;
        int jj = 0;
        for (; jj + 8 <= nj; jj += 8) {
            double2 c[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) c[q] = row[(int64_t)(jj + q) * n2];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                acc0 = __fma_rn(vin[jj + q], c[q].x, acc0);
                acc1 = __fma_rn(vin[jj + q], c[q].y, acc1);
            }
        }
        for (; jj < nj; ++jj) {
            const double2 c = row[(int64_t)jj * n2];
            acc0 = __fma_rn(vin[jj], c.x, acc0);
            acc1 = __fma_rn(vin[jj], c.y, acc1);
        }
    }
    if (k2 >= n2) return;
    double2 *out = reinterpret_cast<double2 *>(a.part + ((int64_t)blockIdx.y * a.n_sub + s) * a.ldc) + k2;
    *out = make_double2(acc0, acc1);
}

struct EpiArgs {
    const double *part;
    const double *bias;   // [s][n_out]
    int n_split;
    int64_t ldc, n_out, n_sub;
    Tf tf;
    int lx, sub_x, sub_y;
    void *out[kMaxVars];
    int64_t ox[kMaxVars], oy[kMaxVars], oz[kMaxVars];
};

__global__ __launch_bounds__(kBlock) void res_epilogue_kernel(EpiArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= a.n_sub * a.n_out) return;
    const int64_t s = e / a.n_out;
    const int64_t k = e - s * a.n_out;
    double y = 0.0;
    for (int q = 0; q < a.n_split; ++q) y += a.part[((int64_t)q * a.n_sub + s) * a.ldc + k];
    y = y + a.bias[s * a.n_out + k];
    SubPoint p;
    locate(a.tf, a.lx, a.sub_x, a.sub_y, a.sub_y, s, k, p);  // no overlap: the step is the extent
    const int64_t off = p.X * a.ox[p.v] + p.Y * a.oy[p.v] + p.zz * a.oz[p.v];
    if (a.tf.kind == FV3HIP_RESERVOIR_SCALE_SPATIAL) {
        if (a.tf.mask) y = y * a.tf.mask[MASK_INDEX(a.tf, p)];
        // NormLayer.backward in float32: x * scale + center, two roundings
        const int64_t fi = FEATURE_INDEX(a.tf, p);
        static_cast<float *>(a.out[p.v])[off] = __fadd_rn(__fmul_rn((float)y, a.tf.scale[fi]), a.tf.center[fi]);
    } else {
        static_cast<double *>(a.out[p.v])[off] = y;
    }
}

__global__ void res_get_state_kernel(const double *state, const int *parity, double *out, int64_t n)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < n) out[e] = state[(*parity ? n : 0) + e];
}

// u [k][s] += noise [s][k] * mask [s][k]: for a 0/1 mask the reference's (u + noise) * mask, u being masked already
__global__ __launch_bounds__(kBlock) void res_add_noise_kernel(double *u, const double *noise, const double *mask, int64_t n_in,
                                                               int64_t n_sub)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_sub * n_in) return;
    const int64_t s = e / n_in;
    const int64_t k = e - s * n_in;
    double v = noise[e];
    if (mask) v = v * mask[e];
    u[k * n_sub + s] = u[k * n_sub + s] + v;
}

struct PackArgs {
    const double *state;  // [2][s][S]
    const int *parity;
    const double *hyb;    // [s][H]
    double *row;          // [s][S + H]
    int S, H, n_sub, square;
};

__global__ __launch_bounds__(kBlock) void res_pack_kernel(PackArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int J = a.S + a.H;
    if (e >= (int64_t)a.n_sub * J) return;
    const int64_t s = e / J;
    const double *st = a.state + (*a.parity ? (int64_t)a.n_sub * a.S : 0) + s * a.S;
    a.row[e] = readout_input(st, a.hyb + s * a.H, (int)s, (int)(e - s * J), a.S, a.square);
}

struct HostTf {
    Tf t{};
    std::vector<float> center, scale;
    std::vector<double> mask;
};

}  // namespace

struct fv3hip_reservoir {
    int device = 0;
    int lx = 1, ly = 1, ov = 0, rx = 0, ry = 0, S = 0, n_in = 0, n_sub = 0, H = 0, square = 0;
    int64_t n_out = 0, ldc = 0, ldw = 0, kpad = 0;
    bool dense = false;
    HostTf in, out, hyb;
    double *d_state = nullptr;  // [2][n_sub][S]
    int *d_parity = nullptr;
    double *d_u = nullptr;      // [n_in][n_sub]
    double *d_w = nullptr;      // dense W_in [kpad][ldw]
    int64_t *d_in_ptr = nullptr;
    int32_t *d_in_idx = nullptr;
    double *d_in_val = nullptr;
    int64_t *d_res_ptr = nullptr;
    int32_t *d_res_idx = nullptr;
    double *d_res_val = nullptr;
    double *d_pmask = nullptr;
    double *d_hmask = nullptr;
    double *d_C = nullptr;      // [n_sub][S + H][ldc]
    double *d_bias = nullptr;
    double *d_hyb = nullptr;    // [n_sub][H]
    double *d_in_part = nullptr;
    double *d_out_part = nullptr;
    int pmask_f32 = 0, hmask_f32 = 0, in_split = 1, in_chunk = 0, in_sb = 1, out_split = 1, out_chunk = 0;
    DeviceAllocs mem;
};

namespace {

// `which`: "input transformer", ...
int check_tf(const fv3hip_reservoir_transformer_t &d, const char *which, int nx, int ny, HostTf &h)
{
    FV3HIP_REQUIRE(d.kind == FV3HIP_RESERVOIR_DO_NOTHING || d.kind == FV3HIP_RESERVOIR_SCALE_SPATIAL,
                   "%s: unknown kind %d", which, d.kind);
    Tf &t = h.t;
    const int rc = fill_zoff(d.var_nz, d.n_variables, kMaxVars, which, t.zoff);
    if (rc) return rc;
    t.kind = d.kind;
    t.n_var = d.n_variables;
    t.zlat = t.zoff[d.n_variables];
    t.nz0 = d.var_nz[0];
    if (d.kind == FV3HIP_RESERVOIR_SCALE_SPATIAL) {
        for (int v = 1; v < d.n_variables; ++v)
            FV3HIP_REQUIRE(d.var_nz[v] == d.var_nz[0], "%s: scale-spatial variables must share one z size", which);
        FV3HIP_REQUIRE(d.nx == nx && d.ny == ny, "%s: its spatial features (%d, %d) differ from the extent it "
                       "transforms (%d, %d)", which, d.nx, d.ny, nx, ny);
        FV3HIP_REQUIRE(d.center && d.scale, "%s: null center or scale", which);
        const size_t n = (size_t)d.n_variables * nx * ny * d.var_nz[0];
        h.center.assign(d.center, d.center + n);
        h.scale.assign(d.scale, d.scale + n);
        if (d.mask) h.mask.assign(d.mask, d.mask + (size_t)nx * ny * t.zlat);
        t.nx = nx;
        t.ny = ny;
        t.mask_f32 = d.mask_f32 ? 1 : 0;
    }
    return FV3HIP_OK;
}

int check_csr(const int64_t *ptr, const int32_t *idx, const double *val, int rows, int cols, const char *which)
{
    FV3HIP_REQUIRE(ptr, "%s: null indptr", which);
    FV3HIP_REQUIRE(ptr[0] == 0, "%s: indptr[0] must be 0", which);
    for (int r = 0; r < rows; ++r)
        FV3HIP_REQUIRE(ptr[r + 1] >= ptr[r], "%s: indptr decreases at row %d", which, r);
    const int64_t nnz = ptr[rows];
    FV3HIP_REQUIRE(nnz == 0 || (idx && val), "%s: null indices or data", which);
    for (int64_t n = 0; n < nnz; ++n)
        FV3HIP_REQUIRE(idx[n] >= 0 && idx[n] < cols, "%s: column index %d is outside [0, %d)", which, idx[n], cols);
    return FV3HIP_OK;
}

int build(const fv3hip_reservoir_desc_t *d, fv3hip_reservoir *m)
{
    FV3HIP_REQUIRE(d, "null descriptor");
    FV3HIP_REQUIRE(d->layout_x >= 1 && d->layout_y >= 1, "subdomain layout must be positive, got (%d, %d)", d->layout_x,
                   d->layout_y);
    FV3HIP_REQUIRE(d->overlap >= 0, "overlap must be non-negative, got %d", d->overlap);
    FV3HIP_REQUIRE(d->rank_x >= 1 && d->rank_y >= 1 && d->rank_x < (1 << 16) && d->rank_y < (1 << 16),
                   "bad rank extent (%d, %d)", d->rank_x, d->rank_y);
    FV3HIP_REQUIRE(d->rank_x % d->layout_x == 0 && d->rank_y % d->layout_y == 0,
                   "rank extent (%d, %d) is not divisible by the subdomain layout (%d, %d)", d->rank_x, d->rank_y,
                   d->layout_x, d->layout_y);
    FV3HIP_REQUIRE(d->state_size >= 1 && d->state_size < (1 << 24), "bad state_size %d", d->state_size);
    FV3HIP_REQUIRE(d->square >= 0 && d->square <= 2, "bad square mode %d", d->square);
    FV3HIP_REQUIRE(d->w_in_storage >= 0 && d->w_in_storage <= 2, "bad w_in_storage %d", d->w_in_storage);
    FV3HIP_REQUIRE(d->n_hybrid >= 0, "bad n_hybrid %d", d->n_hybrid);
    FV3HIP_REQUIRE(d->coefficients && d->intercepts, "null coefficients or intercepts");
    m->lx = d->layout_x;
    m->ly = d->layout_y;
    m->ov = d->overlap;
    m->rx = d->rank_x;
    m->ry = d->rank_y;
    m->S = d->state_size;
    m->n_sub = d->layout_x * d->layout_y;
    m->square = d->square;
    const int bx = d->rank_x / d->layout_x, by = d->rank_y / d->layout_y;
    int rc;
    if ((rc = check_tf(d->input, "input transformer", d->rank_x + 2 * d->overlap, d->rank_y + 2 * d->overlap, m->in))) return rc;
    if ((rc = check_tf(d->output, "output transformer", d->rank_x, d->rank_y, m->out))) return rc;
    const int64_t n_in = (int64_t)(bx + 2 * d->overlap) * (by + 2 * d->overlap) * m->in.t.zlat;
    FV3HIP_REQUIRE(d->input_size == n_in && n_in < (1 << 30), "input_size %d does not match the subdomain extent (%d, %d) "
                   "times the input transformer's %d latent levels", d->input_size, bx + 2 * d->overlap,
                   by + 2 * d->overlap, m->in.t.zlat);
    m->n_in = d->input_size;
    m->n_out = (int64_t)bx * by * m->out.t.zlat;
    if (d->n_hybrid > 0) {
        if ((rc = check_tf(d->hybrid, "hybrid transformer", d->rank_x, d->rank_y, m->hyb))) return rc;
        FV3HIP_REQUIRE((int64_t)d->n_hybrid == (int64_t)bx * by * m->hyb.t.zlat, "n_hybrid %d does not match the subdomain "
                       "extent (%d, %d) times the hybrid transformer's %d latent levels", d->n_hybrid, bx, by, m->hyb.t.zlat);
        m->H = d->n_hybrid;
    }
    if ((rc = check_csr(d->w_in_indptr, d->w_in_indices, d->w_in_data, m->S, m->n_in, "W_in"))) return rc;
    if ((rc = check_csr(d->w_res_indptr, d->w_res_indices, d->w_res_data, m->S, m->S, "W_res"))) return rc;
    const double density = (double)d->w_in_indptr[m->S] / ((double)m->S * m->n_in);
    m->dense = d->w_in_storage == FV3HIP_RESERVOIR_WIN_DENSE ||
               (d->w_in_storage == FV3HIP_RESERVOIR_WIN_AUTO && density >= kDenseDensity);
    m->pmask_f32 = d->input_mask_f32 ? 1 : 0;
    m->hmask_f32 = d->hybrid_mask_f32 ? 1 : 0;
    return FV3HIP_OK;
}

int upload_tf(fv3hip_reservoir *m, HostTf &h)
{
    int rc;
    float *c = nullptr, *s = nullptr;
    double *mk = nullptr;
    if (h.t.kind != FV3HIP_RESERVOIR_SCALE_SPATIAL) return FV3HIP_OK;
    if ((rc = m->mem.upload(&c, h.center.data(), h.center.size())) || (rc = m->mem.upload(&s, h.scale.data(), h.scale.size())))
        return rc;
    if (!h.mask.empty() && (rc = m->mem.upload(&mk, h.mask.data(), h.mask.size()))) return rc;
    h.t.center = c;
    h.t.scale = s;
    h.t.mask = mk;
    return FV3HIP_OK;
}

// a CSR matrix of `rows` rows as the finish kernel walks it
int upload_csr(fv3hip_reservoir *m, const int64_t *ptr, const int32_t *idx, const double *val, int64_t rows, int64_t **d_ptr,
               int32_t **d_idx, double **d_val)
{
    int rc;
    const size_t nnz = (size_t)ptr[rows];
    if ((rc = m->mem.upload(d_ptr, ptr, (size_t)(rows + 1))) || (rc = m->mem.upload(d_idx, idx, nnz))) return rc;
    return m->mem.upload(d_val, val, nnz);
}

// How a sum over `total` rows, taken in steps of `unit` rows, is cut into slices of whole steps: as many slices as bring a
// launch of `base` blocks per slice to `target` blocks, at most one per step.  The slices are added in order afterwards, so
// the bits of a model follow this plan.
struct Slices {
    int chunk, n;  // rows per slice, slices
};

Slices slice_plan(int64_t total, int unit, int64_t base, int64_t target)
{
    const int64_t steps = ceil_div(total, unit);
    int64_t split = ceil_div(target, base);
    split = split < 1 ? 1 : split > steps ? steps : split;
    const int64_t chunk = ceil_div(steps, split) * unit;
    return Slices{(int)chunk, (int)ceil_div(total, chunk)};
}

int upload_all(const fv3hip_reservoir_desc_t *d, fv3hip_reservoir *m)
{
    int rc;
    FV3HIP_CHECK_HIP(hipGetDevice(&m->device));
    if ((rc = upload_tf(m, m->in)) || (rc = upload_tf(m, m->out)) || (rc = upload_tf(m, m->hyb))) return rc;
    const int64_t S = m->S, NS = m->n_sub, N = m->n_in;
    // state: both buffers hold the initial state, parity 0
    if ((rc = m->mem.alloc(&m->d_state, (size_t)(2 * NS * S))) || (rc = m->mem.alloc(&m->d_parity, 1))) return rc;
    FV3HIP_CHECK_HIP(hipMemset(m->d_parity, 0, sizeof(int)));
    if (d->state) {
        FV3HIP_CHECK_HIP(hipMemcpy(m->d_state, d->state, NS * S * sizeof(double), hipMemcpyHostToDevice));
        FV3HIP_CHECK_HIP(hipMemcpy(m->d_state + NS * S, d->state, NS * S * sizeof(double), hipMemcpyHostToDevice));
    } else {
        FV3HIP_CHECK_HIP(hipMemset(m->d_state, 0, 2 * NS * S * sizeof(double)));
    }
    if ((rc = m->mem.alloc(&m->d_u, (size_t)(N * NS)))) return rc;
    if (m->dense) {
        // column-major W_in, rows padded to an even count (16-byte pairs), k padded to whole LDS steps; duplicates summed
        m->ldw = (S + 1) / 2 * 2;
        m->kpad = (N + kInKT - 1) / kInKT * kInKT;
        std::vector<double> w((size_t)(m->kpad * m->ldw), 0.0);
        for (int64_t i = 0; i < S; ++i)
            for (int64_t n = d->w_in_indptr[i]; n < d->w_in_indptr[i + 1]; ++n)
                w[(size_t)d->w_in_indices[n] * m->ldw + i] += d->w_in_data[n];
        if ((rc = m->mem.upload(&m->d_w, w.data(), w.size()))) return rc;
        // slices of k: enough waves to fill the chip, whole LDS steps each
        m->in_sb = NS >= 32 ? 32 : NS > 8 ? 16 : NS > 4 ? 8 : NS > 2 ? 4 : NS;
        const Slices in = slice_plan(m->kpad, kInKT, ceil_div(m->ldw / 2, 64) * ceil_div(NS, m->in_sb), kInTargetWaves);
        m->in_chunk = in.chunk;
        m->in_split = in.n;
        if ((rc = m->mem.alloc(&m->d_in_part, (size_t)(m->in_split * NS * S)))) return rc;
    } else if ((rc = upload_csr(m, d->w_in_indptr, d->w_in_indices, d->w_in_data, S, &m->d_in_ptr, &m->d_in_idx, &m->d_in_val))) {
        return rc;
    }
    if ((rc = upload_csr(m, d->w_res_indptr, d->w_res_indices, d->w_res_data, S, &m->d_res_ptr, &m->d_res_idx, &m->d_res_val)))
        return rc;
    if (d->input_mask && (rc = m->mem.upload(&m->d_pmask, d->input_mask, (size_t)(NS * N)))) return rc;
    const int64_t H = m->H, J = S + H;
    if (H > 0) {
        if ((rc = m->mem.alloc(&m->d_hyb, (size_t)(NS * H)))) return rc;
        if (d->hybrid_mask && (rc = m->mem.upload(&m->d_hmask, d->hybrid_mask, (size_t)(NS * H)))) return rc;
    }
    // readout: C rows padded to an even length for 16-byte loads
    m->ldc = (m->n_out + 1) / 2 * 2;
    if (m->ldc == m->n_out) {
        if ((rc = m->mem.upload(&m->d_C, d->coefficients, (size_t)(NS * J * m->ldc)))) return rc;
    } else {
        std::vector<double> c((size_t)(NS * J * m->ldc), 0.0);
        for (int64_t r = 0; r < NS * J; ++r)
            memcpy(&c[(size_t)(r * m->ldc)], d->coefficients + r * m->n_out, m->n_out * sizeof(double));
        if ((rc = m->mem.upload(&m->d_C, c.data(), c.size()))) return rc;
    }
    if ((rc = m->mem.upload(&m->d_bias, d->intercepts, (size_t)(NS * m->n_out)))) return rc;
    // slices of j from the row length alone (not the subdomain count), so a single-subdomain model split off a larger
    // one adds in the same order
    const Slices out = slice_plan(J, kReadRows, ceil_div(m->ldc / 2, kBlock), 2 * kTargetBlocks);
    m->out_chunk = out.chunk;
    m->out_split = out.n;
    return m->mem.alloc(&m->d_out_part, (size_t)(m->out_split * NS * m->ldc));
}

int check_device(fv3hip_reservoir_t m)
{
    FV3HIP_REQUIRE(m, "null reservoir handle");
    return check_handle_device(m->device, "reservoir");
}

// The three encodings.  The input's: over the subdomains with their overlap, times input_mask, u [k][s], and it flips the
// state's parity.  The hybrid's and the target's: over the subdomains without overlap, [s][k]; the hybrid's times
// hybrid_input_mask into d_hyb, the target's unmasked to where the caller points `out`.  encode() fills the sources.
enum class Enc { Input, Hybrid, Target };

Divider divider(fv3hip_reservoir_t m, int overlap)
{
    const int bx = m->rx / m->lx, by = m->ry / m->ly;
    return Divider{m->lx, bx + 2 * overlap, by + 2 * overlap, bx, by};
}

EncArgs encode_args(fv3hip_reservoir_t m, Enc which)
{
    EncArgs a{};
    a.tf = which == Enc::Input ? m->in.t : which == Enc::Hybrid ? m->hyb.t : m->out.t;
    a.div = divider(m, which == Enc::Input ? m->ov : 0);
    a.n_flat = which == Enc::Input ? m->n_in : which == Enc::Hybrid ? m->H : m->n_out;
    a.n_sub = m->n_sub;
    if (which == Enc::Input) {
        a.pmask = m->d_pmask;
        a.pmask_f32 = m->pmask_f32;
        a.out = m->d_u;
        a.out_ls = 1;
        a.out_lk = m->n_sub;
        a.parity = m->d_parity;
        return a;
    }
    a.out_ls = a.n_flat;
    a.out_lk = 1;
    if (which == Enc::Hybrid) {
        a.pmask = m->d_hmask;
        a.pmask_f32 = m->hmask_f32;
        a.out = m->d_hyb;
    }
    return a;
}

// One encoding of the sources: (x, y, z) arrays, or time t of [t, x, y, z] arrays when there are four strides per variable.
// `target_out`: where the target's goes.  A model without hybrid inputs has no hybrid encoding.
int encode(fv3hip_reservoir_t m, Enc which, const void *const *sources, const int *dtype, const int64_t *strides,
           int strides_per_var, int64_t t, double *target_out, hipStream_t st)
{
    if (which == Enc::Hybrid && m->H == 0) return FV3HIP_OK;
    EncArgs a = encode_args(m, which);
    if (which == Enc::Target) a.out = target_out;
    const int rc = fill_sources(a.tf.n_var, sources, dtype, strides, strides_per_var, t, a.src, &a.src_all_f32);
    if (rc) return rc;
    const int64_t n = a.n_sub * a.n_flat;
    hipLaunchKernelGGL(res_encode_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, st, a);
    return check_launch("res_encode_kernel");
}

template <int SB>
void launch_in_dense(fv3hip_reservoir_t m, hipStream_t st)
{
    const dim3 grid((unsigned)ceil_div(m->ldw / 2, 64), (unsigned)m->in_split, (unsigned)ceil_div(m->n_sub, SB));
    hipLaunchKernelGGL(res_in_dense_kernel<SB>, grid, dim3(64), 0, st, m->d_w, m->d_u, m->d_in_part, m->ldw, m->S,
                       m->n_sub, m->in_chunk, m->n_in, (int)m->kpad);
}

}  // namespace

extern "C" int fv3hip_reservoir_create(const fv3hip_reservoir_desc_t *desc, fv3hip_reservoir_t *out)
{
    FV3HIP_REQUIRE(out, "null output handle");
    *out = nullptr;
    fv3hip_reservoir *m = new fv3hip_reservoir();
    int rc = build(desc, m);
    if (!rc) rc = upload_all(desc, m);
    if (rc) {
        fv3hip_reservoir_destroy(m);
        return rc;
    }
    *out = m;
    return FV3HIP_OK;
}

extern "C" int fv3hip_reservoir_destroy(fv3hip_reservoir_t m)
{
    delete m;  // its DeviceAllocs frees the buffers
    return FV3HIP_OK;
}

extern "C" int fv3hip_reservoir_plan(fv3hip_reservoir_t m, int64_t out[8])
{
    FV3HIP_REQUIRE(m, "null reservoir handle");
    FV3HIP_REQUIRE(out, "null plan");
    out[0] = m->dense ? 1 : 0;
    out[1] = m->in_sb;
    out[2] = m->in_chunk;
    out[3] = m->in_split;
    out[4] = m->out_chunk;
    out[5] = m->out_split;
    out[6] = m->ldw;
    out[7] = m->ldc;
    return FV3HIP_OK;
}

namespace {

// The increment of time t of the sources: encode -> (noise) -> input product -> finish.
int increment_launches(fv3hip_reservoir_t m, const void *const *sources, const int *dtype, const int64_t *strides,
                       int strides_per_var, int64_t t, const double *noise, hipStream_t st)
{
    int rc = encode(m, Enc::Input, sources, dtype, strides, strides_per_var, t, nullptr, st);
    if (rc) return rc;
    if (noise) {
        const int64_t n = (int64_t)m->n_sub * m->n_in;
        hipLaunchKernelGGL(res_add_noise_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, st, m->d_u, noise,
                           m->d_pmask, (int64_t)m->n_in, (int64_t)m->n_sub);
        if ((rc = check_launch("res_add_noise_kernel"))) return rc;
    }
    if (m->dense) {
        switch (m->in_sb) {
        case 32: launch_in_dense<32>(m, st); break;
        case 16: launch_in_dense<16>(m, st); break;
        case 8: launch_in_dense<8>(m, st); break;
        case 4: launch_in_dense<4>(m, st); break;
        case 2: launch_in_dense<2>(m, st); break;
        default: launch_in_dense<1>(m, st); break;
        }
        if ((rc = check_launch("res_in_dense_kernel"))) return rc;
    }
    const FinishArgs f{m->dense ? m->d_in_part : nullptr, m->in_split, m->d_in_ptr, m->d_in_idx, m->d_in_val, m->d_u,
                       m->d_res_ptr, m->d_res_idx, m->d_res_val, m->d_state, m->d_parity, m->S, m->n_sub};
    hipLaunchKernelGGL(res_finish_kernel, dim3((unsigned)ceil_div(m->S, kBlock), (unsigned)m->n_sub), dim3(kBlock), 0, st, f);
    return check_launch("res_finish_kernel");
}

}  // namespace

extern "C" int fv3hip_reservoir_increment(fv3hip_reservoir_t m, const void *const *sources, const int *src_dtype,
                                          const int64_t *strides, void *stream)
{
    int rc = check_device(m);
    if (rc) return rc;
    return increment_launches(m, sources, src_dtype, strides, 3, 0, nullptr, as_stream(stream));
}

extern "C" int fv3hip_reservoir_predict(fv3hip_reservoir_t m, const void *const *hybrid_sources, const int *hybrid_dtype,
                                        const int64_t *hybrid_strides, void *const *outputs, const int64_t *out_strides,
                                        void *stream)
{
    int rc = check_device(m);
    if (rc) return rc;
    EpiArgs e{m->d_out_part, m->d_bias, m->out_split, m->ldc, m->n_out, m->n_sub, m->out.t,
              m->lx, m->rx / m->lx, m->ry / m->ly, {}, {}, {}, {}};
    XyzDst dst[kMaxVars];
    if ((rc = fill_outputs(m->out.t.n_var, outputs, out_strides, dst))) return rc;
    for (int v = 0; v < m->out.t.n_var; ++v) {  // the kernel reads one array per field
        e.out[v] = dst[v].p;
        e.ox[v] = dst[v].sx;
        e.oy[v] = dst[v].sy;
        e.oz[v] = dst[v].sz;
    }
    const hipStream_t st = as_stream(stream);
    if ((rc = encode(m, Enc::Hybrid, hybrid_sources, hybrid_dtype, hybrid_strides, 3, 0, nullptr, st))) return rc;
    const ReadArgs r{m->d_C, m->d_state, m->d_parity, m->d_hyb, m->d_out_part, m->ldc,
                     m->S, m->H, m->n_sub, m->out_chunk, m->square};
    const dim3 grid((unsigned)ceil_div(m->ldc / 2, kBlock), (unsigned)m->out_split, (unsigned)m->n_sub);
    hipLaunchKernelGGL(res_readout_kernel, grid, dim3(kBlock), 0, st, r);
    if ((rc = check_launch("res_readout_kernel"))) return rc;
    hipLaunchKernelGGL(res_epilogue_kernel, dim3((unsigned)ceil_div(m->n_sub * m->n_out, kBlock)), dim3(kBlock), 0, st, e);
    return check_launch("res_epilogue_kernel");
}

extern "C" int fv3hip_reservoir_get_state(fv3hip_reservoir_t m, double *state, void *stream)
{
    int rc = check_device(m);
    if (rc) return rc;
    FV3HIP_REQUIRE(state, "null state");
    const int64_t n = (int64_t)m->n_sub * m->S;
    hipLaunchKernelGGL(res_get_state_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, as_stream(stream),
                       m->d_state, m->d_parity, state, n);
    return check_launch("res_get_state_kernel");
}

extern "C" int fv3hip_reservoir_set_state(fv3hip_reservoir_t m, const double *state, void *stream)
{
    int rc = check_device(m);
    if (rc) return rc;
    FV3HIP_REQUIRE(state, "null state");
    const size_t bytes = (size_t)m->n_sub * m->S * sizeof(double);
    const hipStream_t st = as_stream(stream);
    FV3HIP_CHECK_HIP(hipMemcpyAsync(m->d_state, state, bytes, hipMemcpyDeviceToDevice, st));
    FV3HIP_CHECK_HIP(hipMemcpyAsync(m->d_state + (size_t)m->n_sub * m->S, state, bytes, hipMemcpyDeviceToDevice, st));
    return FV3HIP_OK;
}

extern "C" int fv3hip_reservoir_reset_state(fv3hip_reservoir_t m, void *stream)
{
    int rc = check_device(m);
    if (rc) return rc;
    FV3HIP_CHECK_HIP(hipMemsetAsync(m->d_state, 0, 2 * (size_t)m->n_sub * m->S * sizeof(double), as_stream(stream)));
    return FV3HIP_OK;
}

extern "C" int fv3hip_reservoir_train_series(fv3hip_reservoir_t m, const void *const *sources, const int *src_dtype,
                                             const int64_t *strides, const double *noise, const void *const *hybrid_sources,
                                             const int *hybrid_dtype, const int64_t *hybrid_strides, int64_t n_times,
                                             int square_even_elements, double *X, void *stream)
{
    int rc = check_device(m);
    if (rc) return rc;
    FV3HIP_REQUIRE(n_times >= 0 && n_times < (1ll << 30), "bad n_times %lld", (long long)n_times);
    FV3HIP_REQUIRE(X || n_times == 0, "null X");
    const hipStream_t st = as_stream(stream);
    const int64_t J = (int64_t)m->S + m->H;
    for (int64_t t = 0; t < n_times; ++t) {
        const double *noise_t = noise ? noise + t * m->n_sub * m->n_in : nullptr;
        if ((rc = increment_launches(m, sources, src_dtype, strides, 4, t, noise_t, st))) return rc;
        if ((rc = encode(m, Enc::Hybrid, hybrid_sources, hybrid_dtype, hybrid_strides, 4, t, nullptr, st))) return rc;
        const PackArgs p{m->d_state, m->d_parity, m->d_hyb, X + t * m->n_sub * J, m->S, m->H, m->n_sub,
                         square_even_elements ? FV3HIP_RESERVOIR_SQUARE_ELEMENTS : FV3HIP_RESERVOIR_SQUARE_NONE};
        hipLaunchKernelGGL(res_pack_kernel, dim3((unsigned)ceil_div(m->n_sub * J, kBlock)), dim3(kBlock), 0, st, p);
        if ((rc = check_launch("res_pack_kernel"))) return rc;
    }
    return FV3HIP_OK;
}

extern "C" int fv3hip_reservoir_encode_targets(fv3hip_reservoir_t m, const void *const *sources, const int *src_dtype,
                                               const int64_t *strides, int64_t n_times, double *Y, void *stream)
{
    int rc = check_device(m);
    if (rc) return rc;
    FV3HIP_REQUIRE(n_times >= 0 && n_times < (1ll << 30), "bad n_times %lld", (long long)n_times);
    FV3HIP_REQUIRE(Y || n_times == 0, "null Y");
    for (int64_t t = 0; t < n_times; ++t) {
        if ((rc = encode(m, Enc::Target, sources, src_dtype, strides, 4, t, Y + t * m->n_sub * m->n_out, as_stream(stream))))
            return rc;
    }
    return FV3HIP_OK;
}
