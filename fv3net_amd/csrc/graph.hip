// fv3fit's graph U-Net autoregressor ("graph", external/fv3fit/fv3fit/pytorch/graph/unet.py, pytorch/predict.py:136-250) on
// gfx950 -- DESIGN.md section 16.
//
// Every activation is float32, channel-last: cell (sample s, tile t, x, y) of an array with row length ld and channel offset
// off holds its channels at base[s * sample_stride + ((t * n + x) * n + y) * ld + off + c].  A layer reads one such slice and
// writes another, so the U-Net's concatenation is two layers writing the two halves of one buffer.
//
// graph_gemm_kernel<NT, false> is SAGEConv(mean) on the cube's five-point graph: dst = act(src W_self + mean5(src) W_neigh + b)
// as one GEMM with K = 2 c_in on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32): M = the 256 cells of a 16 x 16 spatial tile, N =
// up to 64 output channels per block (further channels: gridDim.z), K walked in chunks of 8 source channels = 16 K rows (8
// "self" rows, then 8 "mean" rows).  The loader reads a cell and its four neighbours straight from the resident cube --
// across a seam by the rule of cube.h, corners are never needed -- and writes the cell's value and
//     mean5 = ((((self + x-low) + x-high) + y-low) + y-high) / 5      (float32, left to right, one correctly rounded division)
// into LDS: no gathered or averaged copy of the activations exists in memory.
// graph_gemm_kernel<NT, true> is the 2 x 2 / stride 2 transposed convolution on the same skeleton: K = c_in (16 channels per
// chunk, no mean rows), N = 4 c_out (column (2 di + dj) c_out + co), and the epilogue scatters column n of cell (x, y) to cell
// (2 x + di, 2 y + dj).
#include <cmath>

#include "common.h"
#include "cube.h"

using namespace fv3hip;

namespace {

constexpr int kTile = 16;     // spatial tile edge: 256 cells per block
constexpr int kBlock = 256;   // four waves, two 32-cell MFMA tiles each
constexpr int kRows = 16;     // K rows per chunk
constexpr int kMaxGraphVars = 16;

constexpr CubeLimits kLimits{10922, "10922", 16384};   // gridDim.y = 6 n_samples

struct GemmArgs {
    const float *src;        // channel offset applied
    float *dst;
    int64_t src_ld, src_ss, dst_ld, dst_ss;   // row length and sample stride, in elements
    const float *w0;         // SAGE: W_self [c_in][c_out];  UP: W [c_in][2][2][c_out]
    const float *w1;         // SAGE: W_neigh [c_in][c_out]
    const float *bias;       // [c_out]
    int n, C, N, c_out, act, tiles_y;
    CubeSeams seams;
};

// cell index (t * n + x) * n + y of (x, y) on tile t, where at most one of x, y lies one step outside the tile: then the cell
// of the neighbouring face that the one-cell halo shows there
__device__ inline int64_t cell_index(const GemmArgs &a, int t, int x, int y)
{
    const int n = a.n;
    const bool inx = (unsigned)x < (unsigned)n, iny = (unsigned)y < (unsigned)n;
    if (inx && iny) return ((int64_t)t * n + x) * n + y;
    // seam_side and seam_cross of cube.h with d = 0, written out: through the shared functions the compiler orders the
    // kernel's instructions differently, which measured 0.4 % slower on the m = 4 rollout (and as much faster on the wide ones)
    const int side = !inx ? (x < 0 ? 0 : 1) : (y < 0 ? 2 : 3);
    const int j = !inx ? y : x;
    const int q = t * 4 + side;
    const int line = (side & 1) ? 0 : n - 1;
    const int jj = a.seams.flip[q] ? n - 1 - j : j;
    const int xx = a.seams.nax[q] ? line : jj, yy = a.seams.nax[q] ? jj : line;
    return ((int64_t)a.seams.nbr[q] * n + xx) * n + yy;
}

template <int NT, bool UP>
__global__ __launch_bounds__(kBlock) void graph_gemm_kernel(const GemmArgs a)
{
    constexpr int CK = UP ? kRows : kRows / 2;   // source channels per chunk
    constexpr int AP = 288;                      // row stride of the cell panel: 32 mod 64 banks keeps the two lane halves apart
    constexpr int NG = NT * 32;
    constexpr int NGP = NT == 2 ? 96 : 32;
    __shared__ float al[kRows * AP];
    __shared__ float wl[kRows * NGP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (blockIdx.x / a.tiles_y) * kTile, y0 = (blockIdx.x % a.tiles_y) * kTile;
    const int s = blockIdx.y / 6, t = blockIdx.y % 6;
    const int n0 = blockIdx.z * NG;
    const int hh = lane >> 5, l31 = lane & 31;
    const float *src = a.src + (int64_t)s * a.src_ss;

    f32x16 acc[2][NT];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][nt][r] = 0.f;

    for (int c0 = 0; c0 < a.C; c0 += CK) {
        __syncthreads();
        for (int e = tid; e < CK * kTile * kTile; e += kBlock) {
            const int cc = e % CK, pix = e / CK;
            const int gx = x0 + (pix >> 4), gy = y0 + (pix & 15);
            const int c = c0 + cc;
            float v = 0.f, m = 0.f;
            if (c < a.C && gx < a.n && gy < a.n) {
                v = src[cell_index(a, t, gx, gy) * a.src_ld + c];
                if (!UP) {
                    const float xl = src[cell_index(a, t, gx - 1, gy) * a.src_ld + c];
                    const float xh = src[cell_index(a, t, gx + 1, gy) * a.src_ld + c];
                    const float yl = src[cell_index(a, t, gx, gy - 1) * a.src_ld + c];
                    const float yh = src[cell_index(a, t, gx, gy + 1) * a.src_ld + c];
                    m = ((((v + xl) + xh) + yl) + yh) / 5.0f;
                }
            }
            al[cc * AP + pix] = v;
            if (!UP) al[(CK + cc) * AP + pix] = m;
        }
        for (int e = tid; e < kRows * NG; e += kBlock) {
            const int j = e % NG, r = e / NG;
            const int c = c0 + (UP ? r : r % CK), nn = n0 + j;
            const float *w = (UP || r < CK) ? a.w0 : a.w1;
            wl[r * NGP + j] = (c < a.C && nn < a.N) ? w[(int64_t)c * a.N + nn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kp = 0; kp < kRows / 2; ++kp) {
            const int kr = 2 * kp + hh;
            const float xv0 = al[kr * AP + (2 * wave) * 32 + l31];
            const float xv1 = al[kr * AP + (2 * wave + 1) * 32 + l31];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float wv = wl[kr * NGP + nt * 32 + l31];
                acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv0, wv, acc[0][nt], 0, 0, 0);
                acc[1][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv1, wv, acc[1][nt], 0, 0, 0);
            }
        }
    }

    // epilogue: D[row][col], col = lane & 31 (channel), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (cell of the MFMA tile)
    float *dst = a.dst + (int64_t)s * a.dst_ss;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int nn = n0 + nt * 32 + l31;
            if (nn >= a.N) continue;
            const int co = UP ? nn % a.c_out : nn, dij = UP ? nn / a.c_out : 0;
            const float b = a.bias ? a.bias[co] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                const int gx = x0 + (2 * wave + mi) * 2 + (row >> 4), gy = y0 + (row & 15);
                if (gx >= a.n || gy >= a.n) continue;
                float v = acc[mi][nt][r] + b;
                if (a.act == FV3HIP_ACT_RELU)
                    v = v < 0.f ? 0.f : v;   // (a NaN stays a NaN, as in torch's relu: see mlp.hip)
                else if (a.act == FV3HIP_ACT_TANH)
                    v = tanhf(v);
                int64_t cell;
                if (UP) {
                    const int n2 = 2 * a.n;
                    cell = ((int64_t)t * n2 + 2 * gx + (dij >> 1)) * n2 + 2 * gy + (dij & 1);
                } else {
                    cell = ((int64_t)t * a.n + gx) * a.n + gy;
                }
                dst[cell * a.dst_ld + co] = v;
            }
        }
    }
}

// 2 x 2 mean per tile: ((a[2i][2j] + a[2i][2j+1]) + a[2i+1][2j]) + a[2i+1][2j+1], times 0.25 (exact), float32
__global__ __launch_bounds__(kBlock) void graph_pool2_kernel(const float *src, int64_t src_ld, int64_t src_ss, float *dst,
                                                             int64_t dst_ld, int64_t dst_ss, int64_t n_samples, int n, int c)
{
    const int m = n / 2;
    const int64_t total = n_samples * 6 * m * m * c;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int ch = (int)(e % c);
        int64_t r = e / c;
        const int j = (int)(r % m);
        r /= m;
        const int i = (int)(r % m);
        r /= m;
        const int t = (int)(r % 6);
        const int64_t s = r / 6;
        const float *p = src + s * src_ss + (((int64_t)t * n + 2 * i) * n + 2 * j) * src_ld + ch;
        const float v = ((p[0] + p[src_ld]) + p[(int64_t)n * src_ld]) + p[(int64_t)(n + 1) * src_ld];
        dst[s * dst_ss + (((int64_t)t * m + i) * m + j) * dst_ld + ch] = v * 0.25f;
    }
}

struct PackArgs {
    const void *p[kMaxGraphVars];          // pack: the sources; unpack: the float64 outputs
    int64_t st[kMaxGraphVars][5];          // pack: element strides (time, tile, x, y, level)
    int f64[kMaxGraphVars];
    int fstart[kMaxGraphVars + 1];
    int n_vars, n, F;
    const double *mean, *std;              // [F]
};

// state[w][t][tile][x][y][f] = (float)((x - mean[f]) / std[f]) in float64, from source time w * timesteps + t
__global__ __launch_bounds__(kBlock) void graph_pack_kernel(const PackArgs a, float *state, int64_t n_windows, int n_times,
                                                            int timesteps)
{
    const int n = a.n, F = a.F;
    const int64_t total = n_windows * n_times * 6 * n * n * F;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int f = (int)(e % F);
        int64_t r = e / F;
        const int y = (int)(r % n);
        r /= n;
        const int x = (int)(r % n);
        r /= n;
        const int t = (int)(r % 6);
        r /= 6;
        const int64_t time = (r / n_times) * timesteps + r % n_times;
        int v = 0;
        while (v + 1 < a.n_vars && f >= a.fstart[v + 1]) ++v;
        const int64_t off = time * a.st[v][0] + t * a.st[v][1] + x * a.st[v][2] + y * a.st[v][3] + (f - a.fstart[v]) * a.st[v][4];
        const double val = a.f64[v] ? static_cast<const double *>(a.p[v])[off] : (double)static_cast<const float *>(a.p[v])[off];
        state[e] = (float)((val - a.mean[f]) / a.std[f]);
    }
}

// out_v[row][tile][x][y][level] = (double)state * std + mean: the product is rounded before the sum (-ffp-contract=off)
__global__ __launch_bounds__(kBlock) void graph_unpack_kernel(const PackArgs a, const float *state, int64_t n_rows)
{
    const int F = a.F;
    const int64_t total = n_rows * 6 * a.n * a.n * F;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int f = (int)(e % F);
        const int64_t cell = e / F;
        int v = 0;
        while (v + 1 < a.n_vars && f >= a.fstart[v + 1]) ++v;
        const int nf = a.fstart[v + 1] - a.fstart[v];
        const double prod = (double)state[e] * a.std[f];
        static_cast<double *>(const_cast<void *>(a.p[v]))[cell * nf + (f - a.fstart[v])] = prod + a.mean[f];
    }
}

template <bool UP>
int launch_gemm(const GemmArgs &a, int64_t n_samples, hipStream_t st)
{
    const int nt = a.N > 32 ? 2 : 1;
    const int tiles = (int)ceil_div(a.n, kTile);
    dim3 grid((unsigned)(tiles * tiles), (unsigned)(n_samples * 6), (unsigned)ceil_div(a.N, nt * 32));
    if (nt == 1)
        hipLaunchKernelGGL((graph_gemm_kernel<1, UP>), grid, dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL((graph_gemm_kernel<2, UP>), grid, dim3(kBlock), 0, st, a);
    return check_launch("graph_gemm_kernel");
}

int fill_pack(PackArgs &a, const char *what, const void *const *ptrs, int n_vars, const int *nfeat, const double *mean,
              const double *std, int n)
{
    FV3HIP_REQUIRE(ptrs && nfeat && mean && std, "null pointer");
    FV3HIP_REQUIRE(n_vars >= 1 && n_vars <= kMaxGraphVars, "n_vars must be in [1, %d], got %d", kMaxGraphVars, n_vars);
    memset(&a, 0, sizeof(a));
    for (int v = 0; v < n_vars; ++v) {
        FV3HIP_REQUIRE(ptrs[v], "%s %d is null", what, v);
        FV3HIP_REQUIRE(nfeat[v] >= 1 && nfeat[v] <= 65536, "variable %d: nfeat must be in [1, 65536], got %d", v, nfeat[v]);
        a.p[v] = ptrs[v];
        a.fstart[v + 1] = a.fstart[v] + nfeat[v];
    }
    a.n_vars = n_vars;
    a.F = a.fstart[n_vars];
    a.n = n;
    a.mean = mean;
    a.std = std;
    return FV3HIP_OK;
}

}  // namespace

extern "C" int fv3hip_graph_sage(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride,
                                 const float *w_self, const float *w_neigh, const float *bias, float *dst, int64_t dst_ld,
                                 int64_t dst_off, int64_t dst_sample_stride, int64_t n_samples, int n, int c_in, int c_out,
                                 int act, void *stream)
{
    FV3HIP_REQUIRE(c_in >= 1 && c_out >= 1 && c_in <= (1 << 20) && c_out <= (1 << 20), "c_in and c_out must be in [1, 2^20], got %d, %d",
                   c_in, c_out);
    FV3HIP_REQUIRE(w_self && w_neigh, "null weights");
    if (act != FV3HIP_ACT_LINEAR && act != FV3HIP_ACT_RELU && act != FV3HIP_ACT_TANH)
        return fail(FV3HIP_EUNSUPPORTED, "activation code %d: FV3HIP_ACT_LINEAR, _RELU and _TANH are built", act);
    int rc;
    if ((rc = check_cube(n_samples, n, kLimits)) || (rc = check_slice("src", src, src_ld, src_off, c_in)) ||
        (rc = check_slice("dst", dst, dst_ld, dst_off, c_out)) || (rc = check_stride("src", &src_sample_stride, n, src_ld)) ||
        (rc = check_stride("dst", &dst_sample_stride, n, dst_ld)) ||
        (rc = check_no_alias(Slice{src, src_ld, src_off, src_sample_stride, c_in, n},
                             Slice{dst, dst_ld, dst_off, dst_sample_stride, c_out, n}, n_samples, true)))
        return rc;
    if (n_samples == 0) return FV3HIP_OK;
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src + src_off;
    a.dst = dst + dst_off;
    a.src_ld = src_ld;
    a.src_ss = src_sample_stride;
    a.dst_ld = dst_ld;
    a.dst_ss = dst_sample_stride;
    a.w0 = w_self;
    a.w1 = w_neigh;
    a.bias = bias;
    a.n = n;
    a.C = c_in;
    a.N = a.c_out = c_out;
    a.act = act;
    a.tiles_y = (int)ceil_div(n, kTile);
    a.seams = cube_seams();
    return launch_gemm<false>(a, n_samples, as_stream(stream));
}

extern "C" int fv3hip_graph_up2(const float *src, int64_t src_ld, int64_t src_off, const float *w, const float *bias, float *dst,
                                int64_t dst_ld, int64_t dst_off, int64_t n_samples, int n, int c_in, int c_out, void *stream)
{
    FV3HIP_REQUIRE(c_in >= 1 && c_out >= 1 && c_in <= (1 << 20) && c_out <= (1 << 18), "c_in must be in [1, 2^20] and c_out in [1, 2^18], got %d, %d",
                   c_in, c_out);
    FV3HIP_REQUIRE(w, "null weights");
    int rc;
    if ((rc = check_cube(n_samples, n, kLimits))) return rc;
    FV3HIP_REQUIRE(n <= 8192, "n must be at most 8192 (the output has 2 n cells per edge), got %d", n);
    int64_t src_ss = 0, dst_ss = 0;
    if ((rc = check_slice("src", src, src_ld, src_off, c_in)) || (rc = check_slice("dst", dst, dst_ld, dst_off, c_out)) ||
        (rc = check_stride("src", &src_ss, n, src_ld)) || (rc = check_stride("dst", &dst_ss, 2 * n, dst_ld)) ||
        (rc = check_no_alias(Slice{src, src_ld, src_off, src_ss, c_in, n}, Slice{dst, dst_ld, dst_off, dst_ss, c_out, 2 * n}, n_samples, true)))
        return rc;
    if (n_samples == 0) return FV3HIP_OK;
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src + src_off;
    a.dst = dst + dst_off;
    a.src_ld = src_ld;
    a.src_ss = src_ss;
    a.dst_ld = dst_ld;
    a.dst_ss = dst_ss;
    a.w0 = w;
    a.bias = bias;
    a.n = n;
    a.C = c_in;
    a.c_out = c_out;
    a.N = 4 * c_out;
    a.act = FV3HIP_ACT_LINEAR;
    a.tiles_y = (int)ceil_div(n, kTile);
    a.seams = cube_seams();
    return launch_gemm<true>(a, n_samples, as_stream(stream));
}

extern "C" int fv3hip_graph_pool2(const float *src, int64_t src_ld, int64_t src_off, float *dst, int64_t dst_ld, int64_t dst_off,
                                  int64_t n_samples, int n, int c, void *stream)
{
    FV3HIP_REQUIRE(c >= 1 && c <= (1 << 20), "c must be in [1, 2^20], got %d", c);
    int rc;
    if ((rc = check_cube(n_samples, n, kLimits))) return rc;
    FV3HIP_REQUIRE(n % 2 == 0, "n must be even to pool 2 x 2, got %d", n);
    int64_t src_ss = 0, dst_ss = 0;
    if ((rc = check_slice("src", src, src_ld, src_off, c)) || (rc = check_slice("dst", dst, dst_ld, dst_off, c)) ||
        (rc = check_stride("src", &src_ss, n, src_ld)) || (rc = check_stride("dst", &dst_ss, n / 2, dst_ld)) ||
        (rc = check_no_alias(Slice{src, src_ld, src_off, src_ss, c, n}, Slice{dst, dst_ld, dst_off, dst_ss, c, n / 2}, n_samples, true)))
        return rc;
    if (n_samples == 0) return FV3HIP_OK;
    const int64_t total = n_samples * 6 * (n / 2) * (n / 2) * c;
    hipLaunchKernelGGL(graph_pool2_kernel, dim3(grid_stride_blocks(total)), dim3(kBlock), 0, as_stream(stream), src + src_off,
                       src_ld, src_ss, dst + dst_off, dst_ld, dst_ss, n_samples, n, c);
    return check_launch("graph_pool2_kernel");
}

extern "C" int fv3hip_graph_pack(const void *const *sources, const int *src_dtype, const int64_t *src_strides, int n_vars,
                                 const int *nfeat, const double *mean, const double *std, int64_t n_windows, int n_times,
                                 int timesteps, int n, float *state, void *stream)
{
    PackArgs a;
    int rc = fill_pack(a, "source", sources, n_vars, nfeat, mean, std, n);
    if (rc) return rc;
    FV3HIP_REQUIRE(src_dtype && src_strides && state, "null pointer");
    FV3HIP_REQUIRE(n >= 1 && n <= 16384, "n must be in [1, 16384], got %d", n);
    FV3HIP_REQUIRE(n_windows >= 0 && n_times >= 1 && timesteps >= 0, "n_windows >= 0, n_times >= 1 and timesteps >= 0 are needed");
    for (int v = 0; v < n_vars; ++v) {
        FV3HIP_REQUIRE(is_float(src_dtype[v]), "source %d: dtype must be F32 or F64", v);
        a.f64[v] = src_dtype[v] == FV3HIP_F64 ? 1 : 0;
        for (int k = 0; k < 5; ++k) a.st[v][k] = src_strides[5 * v + k];
    }
    const int64_t total = n_windows * n_times * 6 * n * n * a.F;
    if (total == 0) return FV3HIP_OK;
    hipLaunchKernelGGL(graph_pack_kernel, dim3(grid_stride_blocks(total)), dim3(kBlock), 0, as_stream(stream), a, state, n_windows,
                       n_times, timesteps);
    return check_launch("graph_pack_kernel");
}

extern "C" int fv3hip_graph_unpack(const float *state, int64_t n_rows, int n, int n_vars, const int *nfeat, const double *mean,
                                   const double *std, double *const *outputs, void *stream)
{
    PackArgs a;
    int rc = fill_pack(a, "output", reinterpret_cast<const void *const *>(outputs), n_vars, nfeat, mean, std, n);
    if (rc) return rc;
    FV3HIP_REQUIRE(state, "null state");
    FV3HIP_REQUIRE(n >= 1 && n <= 16384, "n must be in [1, 16384], got %d", n);
    FV3HIP_REQUIRE(n_rows >= 0, "n_rows must not be negative");
    const int64_t total = n_rows * 6 * n * n * a.F;
    if (total == 0) return FV3HIP_OK;
    hipLaunchKernelGGL(graph_unpack_kernel, dim3(grid_stride_blocks(total)), dim3(kBlock), 0, as_stream(stream), a, state, n_rows);
    return check_launch("graph_unpack_kernel");
}
