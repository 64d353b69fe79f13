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
#include <vector>

#include "common.h"

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

struct Src {
    const void *p;
    int64_t sx, sy, sz;
    int f64;
};

// a transformer as the kernels see it
struct Tf {
    int kind, n_var, zlat, nx, ny, nz0, mask_f32;
    int zoff[kMaxVars + 1];
    const float *center, *scale;
    const double *mask;
};

struct EncArgs {
    Tf tf;
    Src src[kMaxVars];
    int lx, sub_x, sub_y, step_x, step_y;  // divider
    int64_t n_flat, n_sub;
    const double *pmask;                   // per-subdomain mask [s][k] or null
    int pmask_f32, src_all_f32;
    double *out;
    int64_t out_ls, out_lk;                // out[s * out_ls + k * out_lk]
    int *parity;                           // flipped by thread 0 when not null
};

__device__ __forceinline__ double load_src(const Src &s, int64_t x, int64_t y, int64_t z)
{
    const int64_t off = x * s.sx + y * s.sy + z * s.sz;
    return s.f64 ? static_cast<const double *>(s.p)[off] : (double)static_cast<const float *>(s.p)[off];
}

__device__ __forceinline__ int var_of(const Tf &t, int zl)
{
    int v = 0;
    while (v + 1 < t.n_var && zl >= t.zoff[v + 1]) ++v;
    return v;
}

__global__ __launch_bounds__(kBlock) void res_encode_kernel(EncArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (a.parity && e == 0) *a.parity ^= 1;
    if (e >= a.n_sub * a.n_flat) return;
    const int64_t s = e / a.n_flat;
    const int64_t k = e - s * a.n_flat;
    const int zl = (int)(k % a.tf.zlat);
    const int64_t t = k / a.tf.zlat;
    const int yi = (int)(t % a.sub_y), xi = (int)(t / a.sub_y);
    const int64_t X = (s % a.lx) * a.step_x + xi, Y = (s / a.lx) * a.step_y + yi;
    const int v = var_of(a.tf, zl);
    const int zz = zl - a.tf.zoff[v];
    const double raw = load_src(a.src[v], X, Y, zz);
    double val;
    bool f32;
    if (a.tf.kind == FV3HIP_RESERVOIR_SCALE_SPATIAL) {
        // NormLayer.forward in float32: (x - center) / (scale + 1e-7), IEEE subtraction and division
        const int64_t fi = (int64_t)v * a.tf.nx * a.tf.ny * a.tf.nz0 + (X * a.tf.ny + Y) * a.tf.nz0 + zz;
        const float den = __fadd_rn(a.tf.scale[fi], 1.0e-7f);
        const float enc = __fdiv_rn(__fsub_rn((float)raw, a.tf.center[fi]), den);
        val = (double)enc;
        f32 = true;
        if (a.tf.mask) {  // float32 * float64 is float64 in numpy; float32 * float32 rounds to float32
            val = val * a.tf.mask[(X * a.tf.ny + Y) * a.tf.zlat + zl];
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
        if (threadIdx.x < nj) {
            const int j = j0 + threadIdx.x;
            double v;
            if (j < a.S) {
                v = st[j];
                // square_even_terms: of even subdomains (pure model, axis 0) or of even state elements (hybrid, axis -1)
                const bool sq = a.square == FV3HIP_RESERVOIR_SQUARE_SUBDOMAINS ? (s % 2 == 0)
                                : a.square == FV3HIP_RESERVOIR_SQUARE_ELEMENTS ? (j % 2 == 0)
                                                                                : false;
                if (sq) v = v * v;
            } else {
                v = a.hyb[(int64_t)s * a.H + (j - a.S)];
            }
            vin[threadIdx.x] = v;
        }
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
    const int zl = (int)(k % a.tf.zlat);
    const int64_t t = k / a.tf.zlat;
    const int yi = (int)(t % a.sub_y), xi = (int)(t / a.sub_y);
    const int64_t X = (s % a.lx) * a.sub_x + xi, Y = (s / a.lx) * a.sub_y + yi;
    const int v = var_of(a.tf, zl);
    const int zz = zl - a.tf.zoff[v];
    const int64_t off = X * a.ox[v] + Y * a.oy[v] + zz * a.oz[v];
    if (a.tf.kind == FV3HIP_RESERVOIR_SCALE_SPATIAL) {
        if (a.tf.mask) y = y * a.tf.mask[(X * a.tf.ny + Y) * a.tf.zlat + zl];
        // NormLayer.backward in float32: x * scale + center, two roundings
        const int64_t fi = (int64_t)v * a.tf.nx * a.tf.ny * a.tf.nz0 + (X * a.tf.ny + Y) * a.tf.nz0 + zz;
        static_cast<float *>(a.out[v])[off] = __fadd_rn(__fmul_rn((float)y, a.tf.scale[fi]), a.tf.center[fi]);
    } else {
        static_cast<double *>(a.out[v])[off] = y;
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
    const int j = (int)(e - s * J);
    double v;
    if (j < a.S) {
        v = a.state[(*a.parity ? (int64_t)a.n_sub * a.S : 0) + s * a.S + j];
        if (a.square && j % 2 == 0) v = v * v;  // square_even_terms(axis=-1), train.py:389
    } else {
        v = a.hyb[s * a.H + (j - a.S)];
    }
    a.row[e] = v;
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
    std::vector<void *> allocs;
};

namespace {

template <class T>
int upload(fv3hip_reservoir *m, T **dptr, const T *host, size_t n)
{
    FV3HIP_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(dptr), (n ? n : 1) * sizeof(T)));
    m->allocs.push_back(*dptr);
    if (host && n) FV3HIP_CHECK_HIP(hipMemcpy(*dptr, host, n * sizeof(T), hipMemcpyHostToDevice));
    return FV3HIP_OK;
}

template <class T>
int alloc(fv3hip_reservoir *m, T **dptr, size_t n)
{
    return upload<T>(m, dptr, nullptr, n);
}

int check_tf(const fv3hip_reservoir_transformer_t &d, const char *which, int nx, int ny, HostTf &h)
{
    FV3HIP_REQUIRE(d.kind == FV3HIP_RESERVOIR_DO_NOTHING || d.kind == FV3HIP_RESERVOIR_SCALE_SPATIAL,
                   "%s transformer: unknown kind %d", which, d.kind);
    FV3HIP_REQUIRE(d.n_variables >= 1 && d.n_variables <= kMaxVars, "%s transformer: n_variables must be in [1, %d], got %d",
                   which, kMaxVars, d.n_variables);
    FV3HIP_REQUIRE(d.var_nz, "%s transformer: null var_nz", which);
    Tf &t = h.t;
    t.kind = d.kind;
    t.n_var = d.n_variables;
    t.zoff[0] = 0;
    for (int v = 0; v < d.n_variables; ++v) {
        FV3HIP_REQUIRE(d.var_nz[v] >= 1 && d.var_nz[v] < (1 << 20), "%s transformer: bad z size %d of variable %d", which,
                       d.var_nz[v], v);
        t.zoff[v + 1] = t.zoff[v] + d.var_nz[v];
    }
    t.zlat = t.zoff[d.n_variables];
    t.nz0 = d.var_nz[0];
    if (d.kind == FV3HIP_RESERVOIR_SCALE_SPATIAL) {
        for (int v = 1; v < d.n_variables; ++v)
            FV3HIP_REQUIRE(d.var_nz[v] == d.var_nz[0], "%s transformer: scale-spatial variables must share one z size", which);
        FV3HIP_REQUIRE(d.nx == nx && d.ny == ny, "%s transformer: its spatial features (%d, %d) differ from the extent it "
                       "transforms (%d, %d)", which, d.nx, d.ny, nx, ny);
        FV3HIP_REQUIRE(d.center && d.scale, "%s transformer: null center or scale", which);
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
    if ((rc = check_tf(d->input, "input", d->rank_x + 2 * d->overlap, d->rank_y + 2 * d->overlap, m->in))) return rc;
    if ((rc = check_tf(d->output, "output", d->rank_x, d->rank_y, m->out))) return rc;
    const int64_t n_in = (int64_t)(bx + 2 * d->overlap) * (by + 2 * d->overlap) * m->in.t.zlat;
    FV3HIP_REQUIRE(d->input_size == n_in && n_in < (1 << 30), "input_size %d does not match the subdomain extent (%d, %d) "
                   "times the input transformer's %d latent levels", d->input_size, bx + 2 * d->overlap,
                   by + 2 * d->overlap, m->in.t.zlat);
    m->n_in = d->input_size;
    m->n_out = (int64_t)bx * by * m->out.t.zlat;
    if (d->n_hybrid > 0) {
        if ((rc = check_tf(d->hybrid, "hybrid", d->rank_x, d->rank_y, m->hyb))) return rc;
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
    if ((rc = upload(m, &c, h.center.data(), h.center.size())) || (rc = upload(m, &s, h.scale.data(), h.scale.size())))
        return rc;
    if (!h.mask.empty() && (rc = upload(m, &mk, h.mask.data(), h.mask.size()))) return rc;
    h.t.center = c;
    h.t.scale = s;
    h.t.mask = mk;
    return FV3HIP_OK;
}

int upload_all(const fv3hip_reservoir_desc_t *d, fv3hip_reservoir *m)
{
    int rc;
    FV3HIP_CHECK_HIP(hipGetDevice(&m->device));
    if ((rc = upload_tf(m, m->in)) || (rc = upload_tf(m, m->out)) || (rc = upload_tf(m, m->hyb))) return rc;
    const int64_t S = m->S, NS = m->n_sub, N = m->n_in;
    // state: both buffers hold the initial state, parity 0
    if ((rc = alloc(m, &m->d_state, (size_t)(2 * NS * S))) || (rc = alloc(m, &m->d_parity, 1))) return rc;
    FV3HIP_CHECK_HIP(hipMemset(m->d_parity, 0, sizeof(int)));
    if (d->state) {
        FV3HIP_CHECK_HIP(hipMemcpy(m->d_state, d->state, NS * S * sizeof(double), hipMemcpyHostToDevice));
        FV3HIP_CHECK_HIP(hipMemcpy(m->d_state + NS * S, d->state, NS * S * sizeof(double), hipMemcpyHostToDevice));
    } else {
        FV3HIP_CHECK_HIP(hipMemset(m->d_state, 0, 2 * NS * S * sizeof(double)));
    }
    if ((rc = alloc(m, &m->d_u, (size_t)(N * NS)))) return rc;
    const int64_t nnz_in = d->w_in_indptr[S];
    if (m->dense) {
        // column-major W_in, rows padded to an even count (16-byte pairs), k padded to whole LDS steps; duplicates summed
        m->ldw = (S + 1) / 2 * 2;
        m->kpad = (N + kInKT - 1) / kInKT * kInKT;
        std::vector<double> w((size_t)(m->kpad * m->ldw), 0.0);
        for (int64_t i = 0; i < S; ++i)
            for (int64_t n = d->w_in_indptr[i]; n < d->w_in_indptr[i + 1]; ++n)
                w[(size_t)d->w_in_indices[n] * m->ldw + i] += d->w_in_data[n];
        if ((rc = upload(m, &m->d_w, w.data(), w.size()))) return rc;
        // slices of k: enough waves to fill the chip, whole LDS steps each
        m->in_sb = NS >= 32 ? 32 : NS > 8 ? 16 : NS > 4 ? 8 : NS > 2 ? 4 : NS;
        const int64_t base = ceil_div(m->ldw / 2, 64) * ceil_div(NS, m->in_sb);
        const int64_t steps = m->kpad / kInKT;
        int64_t split = ceil_div(kInTargetWaves, base);
        split = split < 1 ? 1 : split > steps ? steps : split;
        m->in_chunk = (int)(ceil_div(steps, split) * kInKT);
        m->in_split = (int)ceil_div(m->kpad, m->in_chunk);
        if ((rc = alloc(m, &m->d_in_part, (size_t)(m->in_split * NS * S)))) return rc;
    } else {
        if ((rc = upload(m, &m->d_in_ptr, d->w_in_indptr, (size_t)(S + 1))) ||
            (rc = upload(m, &m->d_in_idx, d->w_in_indices, (size_t)nnz_in)) ||
            (rc = upload(m, &m->d_in_val, d->w_in_data, (size_t)nnz_in)))
            return rc;
    }
    const int64_t nnz_res = d->w_res_indptr[S];
    if ((rc = upload(m, &m->d_res_ptr, d->w_res_indptr, (size_t)(S + 1))) ||
        (rc = upload(m, &m->d_res_idx, d->w_res_indices, (size_t)nnz_res)) ||
        (rc = upload(m, &m->d_res_val, d->w_res_data, (size_t)nnz_res)))
        return rc;
    if (d->input_mask && (rc = upload(m, &m->d_pmask, d->input_mask, (size_t)(NS * N)))) return rc;
    const int64_t H = m->H, J = S + H;
    if (H > 0) {
        if ((rc = alloc(m, &m->d_hyb, (size_t)(NS * H)))) return rc;
        if (d->hybrid_mask && (rc = upload(m, &m->d_hmask, d->hybrid_mask, (size_t)(NS * H)))) return rc;
    }
    // readout: C rows padded to an even length for 16-byte loads
    m->ldc = (m->n_out + 1) / 2 * 2;
    if (m->ldc == m->n_out) {
        if ((rc = upload(m, &m->d_C, d->coefficients, (size_t)(NS * J * m->ldc)))) return rc;
    } else {
        std::vector<double> c((size_t)(NS * J * m->ldc), 0.0);
        for (int64_t r = 0; r < NS * J; ++r)
            memcpy(&c[(size_t)(r * m->ldc)], d->coefficients + r * m->n_out, m->n_out * sizeof(double));
        if ((rc = upload(m, &m->d_C, c.data(), c.size()))) return rc;
    }
    if ((rc = upload(m, &m->d_bias, d->intercepts, (size_t)(NS * m->n_out)))) return rc;
    // slices of j from the row length alone (not the subdomain count), so a single-subdomain model split off a larger
    // one adds in the same order
    const int64_t base = ceil_div(m->ldc / 2, kBlock);
    const int64_t steps = ceil_div(J, kReadRows);
    int64_t split = ceil_div(2 * kTargetBlocks, base);
    split = split < 1 ? 1 : split > steps ? steps : split;
    m->out_chunk = (int)(ceil_div(steps, split) * kReadRows);
    m->out_split = (int)ceil_div(J, m->out_chunk);
    return alloc(m, &m->d_out_part, (size_t)(m->out_split * NS * m->ldc));
}

int check_device(fv3hip_reservoir_t m)
{
    FV3HIP_REQUIRE(m, "null reservoir handle");
    int cur = -1;
    FV3HIP_CHECK_HIP(hipGetDevice(&cur));
    FV3HIP_REQUIRE(cur == m->device, "the reservoir lives on device %d but the current device is %d", m->device, cur);
    return FV3HIP_OK;
}

int fill_sources(const Tf &t, const void *const *p, const int *dtype, const int64_t *strides, Src *src, int *all_f32)
{
    FV3HIP_REQUIRE(p && dtype && strides, "null source pointer");
    *all_f32 = 1;
    for (int v = 0; v < t.n_var; ++v) {
        FV3HIP_REQUIRE(p[v], "source %d is null", v);
        FV3HIP_REQUIRE(dtype[v] == FV3HIP_F32 || dtype[v] == FV3HIP_F64, "source %d: dtype must be F32 or F64", v);
        src[v] = Src{p[v], strides[3 * v], strides[3 * v + 1], strides[3 * v + 2], dtype[v] == FV3HIP_F64 ? 1 : 0};
        if (dtype[v] == FV3HIP_F64) *all_f32 = 0;
    }
    return FV3HIP_OK;
}

int launch_encode(EncArgs &a, hipStream_t st)
{
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
    if (!m) return FV3HIP_OK;
    for (void *q : m->allocs) (void)hipFree(q);
    delete m;
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

// encode -> (noise) -> input product -> finish; a.src and a.src_all_f32 are filled by the caller
int increment_launches(fv3hip_reservoir_t m, EncArgs &a, const double *noise, hipStream_t st)
{
    int rc;
    a.tf = m->in.t;
    a.lx = m->lx;
    a.sub_x = m->rx / m->lx + 2 * m->ov;
    a.sub_y = m->ry / m->ly + 2 * m->ov;
    a.step_x = m->rx / m->lx;
    a.step_y = m->ry / m->ly;
    a.n_flat = m->n_in;
    a.n_sub = m->n_sub;
    a.pmask = m->d_pmask;
    a.pmask_f32 = m->pmask_f32;
    a.out = m->d_u;
    a.out_ls = 1;
    a.out_lk = m->n_sub;
    a.parity = m->d_parity;
    if ((rc = launch_encode(a, st))) return rc;
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
    FinishArgs f;
    memset(&f, 0, sizeof(f));
    f.part = m->dense ? m->d_in_part : nullptr;
    f.n_split = m->in_split;
    f.in_ptr = m->d_in_ptr;
    f.in_idx = m->d_in_idx;
    f.in_val = m->d_in_val;
    f.u = m->d_u;
    f.res_ptr = m->d_res_ptr;
    f.res_idx = m->d_res_idx;
    f.res_val = m->d_res_val;
    f.state = m->d_state;
    f.parity = m->d_parity;
    f.S = m->S;
    f.n_sub = m->n_sub;
    hipLaunchKernelGGL(res_finish_kernel, dim3((unsigned)ceil_div(m->S, kBlock), (unsigned)m->n_sub), dim3(kBlock), 0, st, f);
    return check_launch("res_finish_kernel");
}

}  // namespace

extern "C" int fv3hip_reservoir_increment(fv3hip_reservoir_t m, const void *const *sources, const int *src_dtype,
                                          const int64_t *strides, void *stream)
{
    int rc = check_device(m);
    if (rc) return rc;
    EncArgs a;
    memset(&a, 0, sizeof(a));
    if ((rc = fill_sources(m->in.t, sources, src_dtype, strides, a.src, &a.src_all_f32))) return rc;
    return increment_launches(m, a, nullptr, as_stream(stream));
}

extern "C" int fv3hip_reservoir_predict(fv3hip_reservoir_t m, const void *const *hybrid_sources, const int *hybrid_dtype,
                                        const int64_t *hybrid_strides, void *const *outputs, const int64_t *out_strides,
                                        void *stream)
{
    int rc = check_device(m);
    if (rc) return rc;
    FV3HIP_REQUIRE(outputs && out_strides, "null output pointer");
    EpiArgs e;
    memset(&e, 0, sizeof(e));
    for (int v = 0; v < m->out.t.n_var; ++v) {
        FV3HIP_REQUIRE(outputs[v], "output %d is null", v);
        e.out[v] = outputs[v];
        e.ox[v] = out_strides[3 * v];
        e.oy[v] = out_strides[3 * v + 1];
        e.oz[v] = out_strides[3 * v + 2];
    }
    const hipStream_t st = as_stream(stream);
    const int bx = m->rx / m->lx, by = m->ry / m->ly;
    if (m->H > 0) {
        EncArgs a;
        memset(&a, 0, sizeof(a));
        if ((rc = fill_sources(m->hyb.t, hybrid_sources, hybrid_dtype, hybrid_strides, a.src, &a.src_all_f32))) return rc;
        a.tf = m->hyb.t;
        a.lx = m->lx;
        a.sub_x = a.step_x = bx;
        a.sub_y = a.step_y = by;
        a.n_flat = m->H;
        a.n_sub = m->n_sub;
        a.pmask = m->d_hmask;
        a.pmask_f32 = m->hmask_f32;
        a.out = m->d_hyb;
        a.out_ls = m->H;
        a.out_lk = 1;
        if ((rc = launch_encode(a, st))) return rc;
    }
    ReadArgs r;
    r.C = m->d_C;
    r.state = m->d_state;
    r.parity = m->d_parity;
    r.hyb = m->d_hyb;
    r.part = m->d_out_part;
    r.ldc = m->ldc;
    r.S = m->S;
    r.H = m->H;
    r.n_sub = m->n_sub;
    r.j_chunk = m->out_chunk;
    r.square = m->square;
    const dim3 grid((unsigned)ceil_div(m->ldc / 2, kBlock), (unsigned)m->out_split, (unsigned)m->n_sub);
    hipLaunchKernelGGL(res_readout_kernel, grid, dim3(kBlock), 0, st, r);
    if ((rc = check_launch("res_readout_kernel"))) return rc;
    e.part = m->d_out_part;
    e.bias = m->d_bias;
    e.n_split = m->out_split;
    e.ldc = m->ldc;
    e.n_out = m->n_out;
    e.n_sub = m->n_sub;
    e.tf = m->out.t;
    e.lx = m->lx;
    e.sub_x = bx;
    e.sub_y = by;
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

namespace {

// the sources of time t of [t, x, y, z] arrays (strides: four per variable) as fill_sources takes them
int fill_sources_at(const Tf &tf, const void *const *p, const int *dtype, const int64_t *strides, int64_t t, Src *src, int *all_f32)
{
    FV3HIP_REQUIRE(p && dtype && strides, "null source pointer");
    const void *at[kMaxVars];
    int64_t xyz[3 * kMaxVars];
    for (int v = 0; v < tf.n_var; ++v) {
        FV3HIP_REQUIRE(p[v], "source %d is null", v);
        FV3HIP_REQUIRE(is_float(dtype[v]), "source %d: dtype must be F32 or F64", v);
        const int64_t bytes = dtype[v] == FV3HIP_F64 ? 8 : 4;
        at[v] = static_cast<const char *>(p[v]) + t * strides[4 * v] * bytes;
        for (int q = 0; q < 3; ++q) xyz[3 * v + q] = strides[4 * v + 1 + q];
    }
    return fill_sources(tf, at, dtype, xyz, src, all_f32);
}

// an encoding over the subdomains without overlap, [subdomain][feature] (the hybrid path of the readout)
void no_overlap_args(fv3hip_reservoir_t m, const Tf &tf, int64_t n_flat, EncArgs &a)
{
    a.tf = tf;
    a.lx = m->lx;
    a.sub_x = a.step_x = m->rx / m->lx;
    a.sub_y = a.step_y = m->ry / m->ly;
    a.n_flat = n_flat;
    a.n_sub = m->n_sub;
    a.out_ls = n_flat;
    a.out_lk = 1;
}

}  // namespace

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
        EncArgs a;
        memset(&a, 0, sizeof(a));
        if ((rc = fill_sources_at(m->in.t, sources, src_dtype, strides, t, a.src, &a.src_all_f32))) return rc;
        if ((rc = increment_launches(m, a, noise ? noise + t * m->n_sub * m->n_in : nullptr, st))) return rc;
        if (m->H > 0) {
            EncArgs h;
            memset(&h, 0, sizeof(h));
            if ((rc = fill_sources_at(m->hyb.t, hybrid_sources, hybrid_dtype, hybrid_strides, t, h.src, &h.src_all_f32)))
                return rc;
            no_overlap_args(m, m->hyb.t, m->H, h);
            h.pmask = m->d_hmask;
            h.pmask_f32 = m->hmask_f32;
            h.out = m->d_hyb;
            if ((rc = launch_encode(h, st))) return rc;
        }
        PackArgs p;
        p.state = m->d_state;
        p.parity = m->d_parity;
        p.hyb = m->d_hyb;
        p.row = X + t * m->n_sub * J;
        p.S = m->S;
        p.H = m->H;
        p.n_sub = m->n_sub;
        p.square = square_even_elements ? 1 : 0;
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
        EncArgs a;
        memset(&a, 0, sizeof(a));
        if ((rc = fill_sources_at(m->out.t, sources, src_dtype, strides, t, a.src, &a.src_all_f32))) return rc;
        no_overlap_args(m, m->out.t, m->n_out, a);
        a.out = Y + t * m->n_sub * m->n_out;
        if ((rc = launch_encode(a, as_stream(stream)))) return rc;
    }
    return FV3HIP_OK;
}
