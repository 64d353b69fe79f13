// Gram sums of the reservoir readout's ridge regression (fv3fit.reservoir readout.py:39-52): for
// every subdomain s, A[s] += X_s^T X_s [J1][J1] and B[s] += X_s^T Y_s [J1][n_out] in float64, X_s [T][J] and Y_s [T][n_out]
// strided views of the caller's series.  With add_bias J1 = J + 1 and column J of X_s is a column of ones that only the
// loader knows; otherwise J1 = J.
//
// gram_update_kernel: v_mfma_f64_16x16x4_f64 with the time index as k.  One workgroup (four waves, 2 x 2) per 64 x 64 tile
// of A or B and subdomain; a wave holds a 32 x 32 block as four 16 x 16 accumulators, loaded from the accumulator array as
// the MFMA's C operand and stored back.  Time runs ascending through one chain per accumulator: no split over time, no
// atomics, so the bits depend on the shapes only, and two updates of T1 and T2 steps equal one of T1 + T2 when T1 is a
// multiple of the k step (4).  Of A only the tiles on or above the diagonal are computed; the mirrored element is the same
// register's value (transposed through LDS off the diagonal, so that the mirrored rows are stored whole), so A[s] is
// bitwise symmetric.  The series is staged in LDS 32 time steps at a time, the next chunk fetched into registers under
// the MFMAs of the current one.  Rows past T and columns past J1 / n_out are zeros written by the loader (no clamped
// reads: a NaN behind the end of a series cannot enter), and their results are not stored.
// 72 VGPRs + 32 AGPRs and 40 KiB of LDS per workgroup: four workgroups per CU, four waves per SIMD by either count.
//
// f64 C/D map of the instruction: col = lane & 15, row = (lane >> 4) + 4 * reg; A operand A[i = lane & 15][k = lane >> 4],
// B operand B[k = lane >> 4][j = lane & 15], one double per lane each -- both are rows of the time-major series, read from
// LDS with no transpose.
#include "columns.h"

using namespace fv3hip;

namespace {

constexpr int kTile = 64;   // outputs per side of a workgroup's tile
constexpr int kSteps = 32;  // time steps staged in LDS at once
constexpr int kLd = 80;     // doubles per staged row: 64 + 16, so the four k rows of an operand read fall on distinct banks
constexpr int kThreads = 256;
constexpr int kTrLd = 65;   // doubles per row of the transposed tile that the mirrored stores read from LDS
static_assert(kTile * kTrLd <= 2 * kSteps * kLd, "the transposed tile must fit the staging buffers");

typedef double double4_t __attribute__((ext_vector_type(4)));

struct GramArgs {
    const double *X, *Y;
    int64_t x_st, x_ss, y_st, y_ss;  // strides of the time and subdomain dimensions, in elements (features contiguous)
    double *A, *B;
    int J, J1, n_out, T;
    int nt, n_a;                     // tiles per side of A; tiles of A on or above its diagonal
};

// X[t][s][col] with the bias column and the zero padding
__device__ __forceinline__ double x_at(const GramArgs &a, int s, int t, int col)
{
    if (t >= a.T || col >= a.J1) return 0.0;
    if (col >= a.J) return 1.0;
    return a.X[(int64_t)t * a.x_st + (int64_t)s * a.x_ss + col];
}

__device__ __forceinline__ double y_at(const GramArgs &a, int s, int t, int col)
{
    if (t >= a.T || col >= a.n_out) return 0.0;
    return a.Y[(int64_t)t * a.y_st + (int64_t)s * a.y_ss + col];
}

__global__ __launch_bounds__(kThreads) void gram_update_kernel(GramArgs a)
{
    __shared__ double lds[2 * kSteps * kLd];
    double *li = lds, *lj = lds + kSteps * kLd;
    const int s = blockIdx.y;
    // tile: the upper triangle of A row by row, then B
    int idx = blockIdx.x, bi, bj;
    const bool is_b = idx >= a.n_a;
    if (!is_b) {
        bi = 0;
        while (idx >= a.nt - bi) {
            idx -= a.nt - bi;
            ++bi;
        }
        bj = bi + idx;
    } else {
        idx -= a.n_a;
        bi = idx % a.nt;
        bj = idx / a.nt;
    }
    const bool diag = !is_b && bi == bj;
    const int i0 = bi * kTile, j0 = bj * kTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const bool active = !diag || wj >= wi;  // the block below the diagonal of a diagonal tile is its mirror
    const int ncols = is_b ? a.n_out : a.J1;
    double *dst = is_b ? a.B + (int64_t)s * a.J1 * a.n_out : a.A + (int64_t)s * a.J1 * a.J1;
    const int lr = lane >> 4, lc = lane & 15;

    double4_t acc[2][2];
    if (active) {
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = i0 + 32 * wi + 16 * ti + lr + 4 * r, col = j0 + 32 * wj + 16 * tj + lc;
                    acc[ti][tj][r] = (row < a.J1 && col < ncols) ? dst[(int64_t)row * ncols + col] : 0.0;
                }
    }
    const double *pj = diag ? li : lj;
    // the staged values of one time chunk, four elements of each operand per thread; the next chunk is fetched into
    // registers while the MFMAs of the current one run
    constexpr int kPer = kSteps * kTile / kThreads;
    double ni[kPer], nj[kPer];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int e = threadIdx.x + kThreads * q;
            const int kk = e >> 6, c = e & 63;
            ni[q] = x_at(a, s, t0 + kk, i0 + c);
            if (!diag) nj[q] = is_b ? y_at(a, s, t0 + kk, j0 + c) : x_at(a, s, t0 + kk, j0 + c);
        }
    };
    fetch(0);
    for (int t0 = 0; t0 < a.T; t0 += kSteps) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const int e = threadIdx.x + kThreads * q;
            const int kk = e >> 6, c = e & 63;
            li[kk * kLd + c] = ni[q];
            if (!diag) lj[kk * kLd + c] = nj[q];
        }
        __syncthreads();
        if (t0 + kSteps < a.T) fetch(t0 + kSteps);
        if (!active) continue;
        const int left = a.T - t0;
        const int kmax = left >= kSteps ? kSteps : (left + 3) / 4 * 4;
        for (int kk = 0; kk < kmax; kk += 4) {
            const double *ri = li + (kk + lr) * kLd + 32 * wi + lc;
            const double *rj = pj + (kk + lr) * kLd + 32 * wj + lc;
            const double a0 = ri[0], a1 = ri[16], b0 = rj[0], b1 = rj[16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    if (!is_b && !diag) {
        // a tile above the diagonal: its own rows straight from the registers, and its mirror through LDS (the staging
        // buffers are free now), transposed there so that the mirrored rows are written whole -- the same values, so A
        // stays bitwise symmetric
        __syncthreads();
        double *tr = li;  // [64][kTrLd], li and lj are one allocation
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rl = 32 * wi + 16 * ti + lr + 4 * r, cl = 32 * wj + 16 * tj + lc;
                    const double v = acc[ti][tj][r];
                    tr[cl * kTrLd + rl] = v;
                    if (i0 + rl < a.J1 && j0 + cl < a.J1) dst[(int64_t)(i0 + rl) * ncols + j0 + cl] = v;
                }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kTile * kTile / kThreads; ++q) {
            const int e = threadIdx.x + kThreads * q;
            const int rl = e >> 6, cl = e & 63;  // row of the mirrored tile (a column of this one), column within it
            if (j0 + rl < a.J1 && i0 + cl < a.J1) dst[(int64_t)(j0 + rl) * ncols + i0 + cl] = tr[rl * kTrLd + cl];
        }
        return;
    }
    if (!active) return;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + 32 * wi + 16 * ti + lr + 4 * r, col = j0 + 32 * wj + 16 * tj + lc;
                if (row >= a.J1 || col >= ncols) continue;
                const double v = acc[ti][tj][r];
                if (is_b) {
                    dst[(int64_t)row * ncols + col] = v;
                } else if (col >= row) {  // a diagonal tile: the elements on and above the diagonal, and their mirrors
                    dst[(int64_t)row * ncols + col] = v;
                    if (col > row) dst[(int64_t)col * ncols + row] = v;
                }
            }
}

}  // namespace

struct fv3hip_gram {
    int device = 0;
    int n_sub = 0, J = 0, J1 = 0, n_out = 0;
    double *A = nullptr, *B = nullptr;
};

namespace {

int check_device(fv3hip_gram_t g)
{
    FV3HIP_REQUIRE(g, "null Gram accumulator");
    return check_handle_device(g->device, "Gram accumulator");
}

size_t a_count(fv3hip_gram_t g) { return (size_t)g->n_sub * g->J1 * g->J1; }
size_t b_count(fv3hip_gram_t g) { return (size_t)g->n_sub * g->J1 * g->n_out; }

int allocate(fv3hip_gram *g)
{
    FV3HIP_CHECK_HIP(hipGetDevice(&g->device));
    FV3HIP_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(&g->A), a_count(g) * sizeof(double)));
    FV3HIP_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(&g->B), b_count(g) * sizeof(double)));
    FV3HIP_CHECK_HIP(hipMemset(g->A, 0, a_count(g) * sizeof(double)));
    FV3HIP_CHECK_HIP(hipMemset(g->B, 0, b_count(g) * sizeof(double)));
    return FV3HIP_OK;
}

}  // namespace

extern "C" int fv3hip_gram_create(int n_subdomains, int n_features, int n_outputs, int add_bias, fv3hip_gram_t *out)
{
    FV3HIP_REQUIRE(out, "null output handle");
    *out = nullptr;
    FV3HIP_REQUIRE(n_subdomains >= 1 && n_subdomains < 65536, "n_subdomains must be in [1, 65535], got %d", n_subdomains);
    FV3HIP_REQUIRE(n_features >= 1 && n_features < (1 << 24), "bad n_features %d", n_features);
    FV3HIP_REQUIRE(n_outputs >= 1 && n_outputs < (1 << 24), "bad n_outputs %d", n_outputs);
    fv3hip_gram *g = new fv3hip_gram();
    g->n_sub = n_subdomains;
    g->J = n_features;
    g->J1 = n_features + (add_bias ? 1 : 0);
    g->n_out = n_outputs;
    const int rc = allocate(g);
    if (rc) {
        fv3hip_gram_destroy(g);
        return rc;
    }
    *out = g;
    return FV3HIP_OK;
}

extern "C" int fv3hip_gram_destroy(fv3hip_gram_t g)
{
    if (!g) return FV3HIP_OK;
    if (g->A) (void)hipFree(g->A);
    if (g->B) (void)hipFree(g->B);
    delete g;
    return FV3HIP_OK;
}

extern "C" int fv3hip_gram_reset(fv3hip_gram_t g, void *stream)
{
    int rc = check_device(g);
    if (rc) return rc;
    FV3HIP_CHECK_HIP(hipMemsetAsync(g->A, 0, a_count(g) * sizeof(double), as_stream(stream)));
    FV3HIP_CHECK_HIP(hipMemsetAsync(g->B, 0, b_count(g) * sizeof(double), as_stream(stream)));
    return FV3HIP_OK;
}

extern "C" int fv3hip_gram_update(fv3hip_gram_t g, const double *X, int64_t x_time_stride, int64_t x_sub_stride,
                                  const double *Y, int64_t y_time_stride, int64_t y_sub_stride, int64_t n_times, void *stream)
{
    int rc = check_device(g);
    if (rc) return rc;
    FV3HIP_REQUIRE(n_times >= 0 && n_times < (1ll << 30), "bad n_times %lld", (long long)n_times);
    if (n_times == 0) return FV3HIP_OK;
    FV3HIP_REQUIRE(X && Y, "null X or Y");
    FV3HIP_REQUIRE(x_time_stride >= 0 && x_sub_stride >= 0 && y_time_stride >= 0 && y_sub_stride >= 0,
                   "strides must be non-negative");
    GramArgs a;
    a.X = X;
    a.Y = Y;
    a.x_st = x_time_stride;
    a.x_ss = x_sub_stride;
    a.y_st = y_time_stride;
    a.y_ss = y_sub_stride;
    a.A = g->A;
    a.B = g->B;
    a.J = g->J;
    a.J1 = g->J1;
    a.n_out = g->n_out;
    a.T = (int)n_times;
    a.nt = (int)ceil_div(g->J1, kTile);
    a.n_a = a.nt * (a.nt + 1) / 2;
    const int64_t tiles = a.n_a + (int64_t)a.nt * ceil_div(g->n_out, kTile);
    FV3HIP_REQUIRE(tiles < (1ll << 31), "too many tiles (%lld)", (long long)tiles);
    hipLaunchKernelGGL(gram_update_kernel, dim3((unsigned)tiles, (unsigned)g->n_sub), dim3(kThreads), 0, as_stream(stream), a);
    return check_launch("gram_update_kernel");
}

extern "C" int fv3hip_gram_get(fv3hip_gram_t g, int subdomain, double *A, double *B, void *stream)
{
    int rc = check_device(g);
    if (rc) return rc;
    FV3HIP_REQUIRE(subdomain >= -1 && subdomain < g->n_sub, "subdomain %d is outside [-1, %d)", subdomain, g->n_sub);
    const size_t na = (size_t)g->J1 * g->J1, nb = (size_t)g->J1 * g->n_out;
    const size_t first = subdomain < 0 ? 0 : (size_t)subdomain, count = subdomain < 0 ? (size_t)g->n_sub : 1;
    const hipStream_t st = as_stream(stream);
    if (A) FV3HIP_CHECK_HIP(hipMemcpyAsync(A, g->A + first * na, count * na * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (B) FV3HIP_CHECK_HIP(hipMemcpyAsync(B, g->B + first * nb, count * nb * sizeof(double), hipMemcpyDeviceToDevice, st));
    return FV3HIP_OK;
}
