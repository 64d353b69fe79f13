// fv3fit's CycleGAN generators ("cycle_gan", external/fv3fit/fv3fit/pytorch/cyclegan/generator.py:19-270, modules.py) on
// gfx950 -- DESIGN.md section 17.
//
// Activations are float32, channel-last, as in graph.hip: cell (sample s, tile t, x, y) of an array with row length ld and
// channel offset off holds its channels at base[s * sample_stride + ((t * n + x) * n + y) * ld + off + c].
//
// cyclegan_conv_kernel is every convolution of the network as one implicit GEMM on the exact-f32 MFMA
// (v_mfma_f32_32x32x2_f32).  M = output cells flattened over (sample, tile, x, y), 128 per block (one 32-row MFMA tile per
// wave): a 12 x 12 or 6 x 6 face at the bottom of the network fills the rows as well as a 48 x 48 one.  N = up to 64 output
// channels per block (gridDim.y: further channels).  K = taps x c_in flattened with the channel fastest, walked 16 rows at a
// time.  A block first writes, per (tap, row), the source cell that the tap reads -- on the face, on the neighbouring face
// across a cube seam (the rule of cube.h), or nowhere (corners, zero padding) -- into LDS; the loader
// then gathers the K rows through that table and applies the producing layer's instance norm, per-cell bias and ReLU on the
// way, with the statistics and the bias cell of the face the value comes from.
//   regular     k x k, stride 1, halo (k - 1) / 2:  output (x, y) reads (x + dx - h, y + dy - h)
//   strided     4 x 4, stride 2, halo 1:            output (x, y) reads (2 x - 1 + dx, 2 y - 1 + dy)
//               (3 x 3 as well behind fv3hip_cyclegan_train_conv: the discriminator's default)
//   transposed  ConvTranspose2d(4, stride 2) of the input padded by one halo line, cropped by 3: per axis output 2 m takes
//               tap 1 of cell m and tap 3 of cell m - 1, output 2 m + 1 tap 0 of cell m + 1 and tap 2 of cell m; the four
//               output parities are four 2 x 2 convolutions (gridDim.z) with their own weight blocks
//
// A regular convolution may take context channels (fv3hip_cyclegan_conv_context; the step layers of the recurrent generator,
// recurrent/generator.py:127-182): c_cell per-cell values [6][n][n][c_cell] and c_uni values that are
// the same on every cell, appended to the source's channels without ever being stored there.  Summation order: the
// taps x c_in source rows first, exactly as without a context, then the taps x (c_cell + c_uni) context rows (tap slowest,
// cell channels before uniform ones) as further 16-row chunks into the same accumulators.  A context row is gathered through
// the same table as the source: the cell context of a halo cell is that of the neighbouring face's cell, the uniform value is
// present wherever the table names a cell, and both are zero where it names none (corners, zero padding).  The loader's
// transform does not touch them.
#include <cmath>

#include "common.h"
#include "cube.h"

using namespace fv3hip;

namespace {

constexpr int kBlock = 256;   // four waves
constexpr int kBM = 128;      // output cells per block: one 32-row MFMA tile per wave
constexpr int kRows = 16;     // K rows per chunk
constexpr int kStatCh = 16;   // statistics: channels per block, 16 groups of cells each

constexpr CubeLimits kLimits{1 << 20, "2^20", 4096};

struct ConvArgs {
    const float *src;        // channel offset applied
    float *dst;
    int64_t src_ld, src_ss, dst_ld, dst_ss;
    const float *mean, *rstd;   // [sample][6][C] or null: the loader's (v - mean) * rstd
    const float *in_bias;       // [6][n][n][C] or null, added after the norm
    int in_relu;
    const float *w;             // [taps][C][N]; transposed: [parity][4][C][N]
    const float *bias;          // [N] or null
    const float *out_bias;      // [6][n_out][n_out][N] or null, added after the bias
    int n, n_out, mg;           // input edge, output edge, edge of the grid the rows are flattened over
    int C, N, kind, k, taps, h, cube;
    int64_t rows;               // n_samples * 6 * mg * mg
    const float *ctx_cell;      // [6][n][n][c_cell] or null
    const float *ctx_uni;       // [c_ctx - c_cell] or null
    const float *w_ctx;         // [taps][c_ctx][N]
    int c_cell, c_ctx;          // per-cell context channels; all context channels
    CubeSeams seams;
};

// cell (t * n + x) * n + y that position (x, y) of tile t's padded field shows, with the tile in bits 28-30; -1: a zero
__device__ inline int source_cell(const ConvArgs &a, int t, int x, int y)
{
    const int n = a.n;
    const bool inx = (unsigned)x < (unsigned)n, iny = (unsigned)y < (unsigned)n;
    if (inx && iny) return ((t * n + x) * n + y) | (t << 28);
    if (!a.cube || (!inx && !iny)) return -1;   // zero padding; the corners of the halo stay zero (modules.py:446-463)
    int side, d, j, tt, xx, yy;
    seam_side(n, x, y, inx, side, d, j);
    seam_cross(a.seams, n, t, side, d, j, tt, xx, yy);
    return ((tt * n + xx) * n + yy) | (tt << 28);
}

// VEC: c_in is a multiple of 16 and every pointer and stride of the source side a multiple of four floats, so a chunk is 16
// consecutive channels of one tap and a thread loads four of them at once.  CTX: context rows follow the source rows
template <int NT, bool VEC, bool CTX = false>
__global__ __launch_bounds__(kBlock) void cyclegan_conv_kernel(const ConvArgs a)
{
    constexpr int AP = kBM + 2;   // the 16 K rows of one loader pass land on 32 distinct banks
    constexpr int NG = NT * 32;
    extern __shared__ int sidx[];          // [taps][kBM]
    __shared__ int srow[kBM], srem[kBM];   // sample and cell (of the flattened grid) of every row; -1: past the end
    __shared__ float al[kRows * AP];
    __shared__ float wl[kRows * NG];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, l31 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * kBM;
    const int n0 = blockIdx.y * NG;
    const int px = blockIdx.z >> 1, py = blockIdx.z & 1;
    const int mg = a.mg, cells = 6 * mg * mg;

    if (tid < kBM) {
        const int64_t g = row0 + tid;
        srow[tid] = g < a.rows ? (int)(g / cells) : -1;
        srem[tid] = g < a.rows ? (int)(g % cells) : 0;
    }
    for (int e = tid; e < a.taps * kBM; e += kBlock) {
        const int r = e % kBM, tap = e / kBM;
        const int64_t g = row0 + r;
        int idx = -1;
        if (g < a.rows) {
            const int rem = (int)(g % cells);
            const int t = rem / (mg * mg), x = rem / mg % mg, y = rem % mg;
            int sx, sy;
            if (a.kind == FV3HIP_CYCLEGAN_CONV_REGULAR) {
                sx = x + tap / a.k - a.h;
                sy = y + tap % a.k - a.h;
            } else if (a.kind == FV3HIP_CYCLEGAN_CONV_STRIDED) {
                sx = 2 * x - 1 + tap / a.k;
                sy = 2 * y - 1 + tap % a.k;
            } else {
                const int ta = tap >> 1, tb = tap & 1;
                sx = x + (px ? 1 - ta : -ta);
                sy = y + (py ? 1 - tb : -tb);
            }
            idx = source_cell(a, t, sx, sy);
        }
        sidx[tap * kBM + r] = idx;
    }

    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    const int K = a.taps * a.C;
    const float *w = a.w + (a.kind == FV3HIP_CYCLEGAN_CONV_TRANSPOSED ? (int64_t)blockIdx.z * K * a.N : 0);
    const int kk = tid & 15;   // every loader pass of this thread fills K row kk of the chunk
    for (int k0 = 0; k0 < K; k0 += kRows) {
        __syncthreads();
        if (VEC) {
            const int tap = k0 / a.C, c = k0 - tap * a.C + 4 * (tid & 3);
#pragma unroll
            for (int i = 0; i < kRows * kBM / kBlock / 4; ++i) {
                const int r = (tid >> 2) + 64 * i;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                const int packed = sidx[tap * kBM + r];
                if (packed >= 0) {
                    const int idx = packed & 0x0fffffff, tt = packed >> 28;
                    const int64_t s = srow[r];
                    v = *reinterpret_cast<const float4 *>(a.src + s * a.src_ss + (int64_t)idx * a.src_ld + c);
                    if (a.mean) {
                        const int64_t st = (s * 6 + tt) * a.C + c;
                        const float4 m = *reinterpret_cast<const float4 *>(a.mean + st), q = *reinterpret_cast<const float4 *>(a.rstd + st);
                        v = make_float4((v.x - m.x) * q.x, (v.y - m.y) * q.y, (v.z - m.z) * q.z, (v.w - m.w) * q.w);
                    }
                    if (a.in_bias) {
                        const float4 b = *reinterpret_cast<const float4 *>(a.in_bias + (int64_t)idx * a.C + c);
                        v = make_float4(v.x + b.x, v.y + b.y, v.z + b.z, v.w + b.w);
                    }
                    if (a.in_relu) v = make_float4(v.x < 0.f ? 0.f : v.x, v.y < 0.f ? 0.f : v.y, v.z < 0.f ? 0.f : v.z, v.w < 0.f ? 0.f : v.w);
                }
                float *col = al + (4 * (tid & 3)) * AP + r;
                col[0] = v.x;
                col[AP] = v.y;
                col[2 * AP] = v.z;
                col[3 * AP] = v.w;
            }
        }
        const int kg = k0 + kk;
        const int tap = kg < K ? kg / a.C : 0, c = kg - tap * a.C;
#pragma unroll
        for (int i = 0; i < (VEC ? 0 : kRows * kBM / kBlock); ++i) {
            const int r = (tid >> 4) + 16 * i;
            float v = 0.f;
            const int packed = kg < K ? sidx[tap * kBM + r] : -1;
            if (packed >= 0) {
                const int idx = packed & 0x0fffffff, tt = packed >> 28;
                const int64_t s = srow[r];
                v = a.src[s * a.src_ss + (int64_t)idx * a.src_ld + c];
                if (a.mean) {
                    const int64_t st = (s * 6 + tt) * a.C + c;
                    v = (v - a.mean[st]) * a.rstd[st];
                }
                if (a.in_bias) v = v + a.in_bias[(int64_t)idx * a.C + c];
                if (a.in_relu) v = v < 0.f ? 0.f : v;   // (a NaN stays a NaN, as in torch's relu)
            }
            al[kk * AP + r] = v;
        }
        for (int e = tid; e < kRows * NG; e += kBlock) {
            const int j = e % NG, r = e / NG;
            const int nn = n0 + j;
            wl[r * NG + j] = (k0 + r < K && nn < a.N) ? w[(int64_t)(k0 + r) * a.N + nn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kp = 0; kp < kRows / 2; ++kp) {
            const int kr = 2 * kp + hh;
            const float xv = al[kr * AP + wave * 32 + l31];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, wl[kr * NG + nt * 32 + l31], acc[nt], 0, 0, 0);
        }
    }
    if (CTX) {
        // the context rows: few (45 against 2 304 at the production step layer), so every thread loads single values
        // (the panel fill and the MFMA sweep stand here a second time: as shared helpers -- functions or lambdas -- they
        // change the instruction order of all eight instantiations, which measured 0.3 - 0.8 % slower on the generator)
        const int KC = a.taps * a.c_ctx;
        for (int k0 = 0; k0 < KC; k0 += kRows) {
            __syncthreads();
            const int kg = k0 + kk;
            const int tap = kg < KC ? kg / a.c_ctx : 0, c = kg - tap * a.c_ctx;
            const bool cell = c < a.c_cell;
            const float uni = (kg < KC && !cell) ? a.ctx_uni[c - a.c_cell] : 0.f;
#pragma unroll
            for (int i = 0; i < kRows * kBM / kBlock; ++i) {
                const int r = (tid >> 4) + 16 * i;
                float v = 0.f;
                const int packed = kg < KC ? sidx[tap * kBM + r] : -1;
                if (packed >= 0) v = cell ? a.ctx_cell[(int64_t)(packed & 0x0fffffff) * a.c_cell + c] : uni;
                al[kk * AP + r] = v;
            }
            for (int e = tid; e < kRows * NG; e += kBlock) {
                const int j = e % NG, r = e / NG;
                const int nn = n0 + j;
                wl[r * NG + j] = (k0 + r < KC && nn < a.N) ? a.w_ctx[(int64_t)(k0 + r) * a.N + nn] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int kp = 0; kp < kRows / 2; ++kp) {
                const int kr = 2 * kp + hh;
                const float xv = al[kr * AP + wave * 32 + l31];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, wl[kr * NG + nt * 32 + l31], acc[nt], 0, 0, 0);
            }
        }
    }

    // epilogue: D[row][col], col = lane & 31 (channel), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (cell of the MFMA tile)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int nn = n0 + nt * 32 + l31;
        if (nn >= a.N) continue;
        const float b = a.bias ? a.bias[nn] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            const int64_t s = srow[rr];
            if (s < 0) continue;
            int64_t cell = srem[rr];
            if (a.kind == FV3HIP_CYCLEGAN_CONV_TRANSPOSED) {
                const int rem = srem[rr];
                const int t = rem / (mg * mg), x = rem / mg % mg, y = rem % mg;
                cell = ((int64_t)t * a.n_out + 2 * x + px) * a.n_out + 2 * y + py;
            }
            float v = acc[nt][r] + b;
            if (a.out_bias) v = v + a.out_bias[cell * a.N + nn];
            a.dst[s * a.dst_ss + cell * a.dst_ld + nn] = v;
        }
    }
}

// nn.InstanceNorm2d's statistics of one (sample, tile) face for 16 channels: the mean, then the biased variance about it in a
// second pass, both accumulated in float64 by 16 groups of cells and added in group order
__global__ __launch_bounds__(kBlock) void cyclegan_stats_kernel(const float *src, int64_t ld, int64_t ss, float *mean, float *rstd,
                                                                int n, int C, double eps)
{
    __shared__ double red[16][kStatCh];
    __shared__ double mu[kStatCh];
    const int tid = threadIdx.x, cl = tid % kStatCh, g = tid / kStatCh;
    const int64_t st = blockIdx.x;
    const int c = blockIdx.y * kStatCh + cl;
    const int cells = n * n;
    const float *p = src + (st / 6) * ss + (st % 6) * (int64_t)cells * ld + c;
    double sum = 0.0;
    if (c < C) {
#pragma unroll 4
        for (int i = g; i < cells; i += 16) sum += (double)p[(int64_t)i * ld];
    }
    red[g][cl] = sum;
    __syncthreads();
    if (g == 0) {
        double tot = 0.0;
        for (int j = 0; j < 16; ++j) tot += red[j][cl];
        mu[cl] = tot / cells;
    }
    __syncthreads();
    const double m = mu[cl];
    double m2 = 0.0;
    if (c < C) {
#pragma unroll 4
        for (int i = g; i < cells; i += 16) {
            const double d = (double)p[(int64_t)i * ld] - m;
            m2 += d * d;
        }
    }
    red[g][cl] = m2;
    __syncthreads();
    if (g == 0 && c < C) {
        double tot = 0.0;
        for (int j = 0; j < 16; ++j) tot += red[j][cl];
        mean[st * C + c] = (float)m;
        rstd[st * C + c] = (float)(1.0 / sqrt(tot / cells + eps));
    }
}

// dst = act((src - mean) * rstd [+ bias]) [+ res], element by element
__global__ __launch_bounds__(kBlock) void cyclegan_apply_kernel(const float *src, int64_t src_ld, int64_t src_ss, const float *mean,
                                                                const float *rstd, const float *bias, int relu, const float *res,
                                                                int64_t res_ld, int64_t res_ss, float *dst, int64_t dst_ld,
                                                                int64_t dst_ss, int64_t n_samples, int n, int C)
{
    const int64_t cells = 6LL * n * n, total = n_samples * cells * C;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int c = (int)(e % C);
        const int64_t r = e / C, cell = r % cells, s = r / cells;
        float v = src[s * src_ss + cell * src_ld + c];
        if (mean) {
            const int64_t st = (s * 6 + cell / ((int64_t)n * n)) * C + c;
            v = (v - mean[st]) * rstd[st];
        }
        if (bias) v = v + bias[cell * C + c];
        if (relu) v = v < 0.f ? 0.f : v;
        if (res) v = v + res[s * res_ss + cell * res_ld + c];
        dst[s * dst_ss + cell * dst_ld + c] = v;
    }
}

// dst[..., :C] = state [+ bias]; with lon: dst[..., C:C+5] = sin(lon + theta_s), cos(lon + theta_s), x, y, z
__global__ __launch_bounds__(kBlock) void cyclegan_input_kernel(const float *src, int64_t src_ld, int64_t src_ss, const float *bias,
                                                                const float *lon, const float *xyz, const float *theta, float *dst,
                                                                int64_t dst_ld, int64_t dst_ss, int64_t n_samples, int n, int C)
{
    const int CO = C + (lon ? 5 : 0);
    const int64_t cells = 6LL * n * n, total = n_samples * cells * CO;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int c = (int)(e % CO);
        const int64_t r = e / CO, cell = r % cells, s = r / cells;
        float v;
        if (c < C) {
            v = src[s * src_ss + cell * src_ld + c];
            if (bias) v = v + bias[cell * C + c];
        } else if (c < C + 2) {
            const float local = lon[cell] + theta[s];
            v = c == C ? sinf(local) : cosf(local);
        } else {
            v = xyz[cell * 3 + (c - C - 2)];
        }
        dst[s * dst_ss + cell * dst_ld + c] = v;
    }
}

bool same_slice(const Slice &a, const Slice &b)
{
    return a.p == b.p && a.ld == b.ld && a.off == b.off && a.ss == b.ss && a.c == b.c && a.n == b.n;
}

// all convolution entry points: every argument is checked here, before any HIP call.  train: the forward of the training
// layers (fv3hip_cyclegan_train_conv), which also takes the 3 x 3 strided convolution
int launch_conv(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride, const float *in_mean,
                const float *in_rstd, const float *in_bias, int in_relu, const float *w, const float *bias, const float *out_bias,
                float *dst, int64_t dst_ld, int64_t dst_off, int64_t dst_sample_stride, int64_t n_samples, int n, int c_in, int c_out,
                int kind, int k, int halo_mode, const float *ctx_cell, int c_cell, const float *ctx_uniform, int c_uni,
                const float *w_ctx, void *stream, bool train = false)
{
    FV3HIP_REQUIRE(c_in >= 1 && c_out >= 1 && c_in <= (1 << 16) && c_out <= (1 << 16), "c_in and c_out must be in [1, 2^16], got %d, %d",
                   c_in, c_out);
    FV3HIP_REQUIRE(w, "null weights");
    FV3HIP_REQUIRE((in_mean == nullptr) == (in_rstd == nullptr), "in_mean and in_rstd come together");
    FV3HIP_REQUIRE(halo_mode == FV3HIP_CYCLEGAN_HALO_ZEROS || halo_mode == FV3HIP_CYCLEGAN_HALO_CUBE, "unknown halo mode %d", halo_mode);
    int rc;
    if ((rc = check_cube(n_samples, n, kLimits))) return rc;
    int n_out = n, taps = k * k, h = (k - 1) / 2;
    if (kind == FV3HIP_CYCLEGAN_CONV_REGULAR) {
        if (k != 3 && k != 5 && k != 7) return fail(FV3HIP_EUNSUPPORTED, "regular convolution with k = %d: 3, 5 and 7 are built", k);
    } else if (kind == FV3HIP_CYCLEGAN_CONV_STRIDED || kind == FV3HIP_CYCLEGAN_CONV_TRANSPOSED) {
        if (train && kind == FV3HIP_CYCLEGAN_CONV_STRIDED) {
            if (k != 3 && k != 4) return fail(FV3HIP_EUNSUPPORTED, "strided convolution with k = %d: 3 and 4 are built", k);
        } else if (k != 4) {
            return fail(FV3HIP_EUNSUPPORTED, "strided and transposed convolutions are built for k = 4, got %d", k);
        }
        h = 1;
        if (kind == FV3HIP_CYCLEGAN_CONV_STRIDED) {
            FV3HIP_REQUIRE(n % 2 == 0, "n must be even for the stride-2 convolution, got %d", n);
            n_out = n / 2;
        } else {
            FV3HIP_REQUIRE(n <= 2048, "n must be at most 2048 (the output has 2 n cells per edge), got %d", n);
            n_out = 2 * n;
            taps = 4;
        }
    } else {
        return fail(FV3HIP_EUNSUPPORTED, "unknown convolution kind %d", kind);
    }
    FV3HIP_REQUIRE(h <= n, "the halo (%d cells) is wider than the face (%d)", h, n);
    FV3HIP_REQUIRE(c_cell >= 0 && c_uni >= 0 && c_cell <= (1 << 12) && c_uni <= (1 << 12),
                   "c_cell and c_uni must be in [0, 2^12], got %d, %d", c_cell, c_uni);
    FV3HIP_REQUIRE((ctx_cell != nullptr) == (c_cell > 0), "ctx_cell is %s with c_cell = %d", ctx_cell ? "given" : "null", c_cell);
    FV3HIP_REQUIRE((ctx_uniform != nullptr) == (c_uni > 0), "ctx_uniform is %s with c_uni = %d", ctx_uniform ? "given" : "null", c_uni);
    const int c_ctx = c_cell + c_uni;
    FV3HIP_REQUIRE((w_ctx != nullptr) == (c_ctx > 0), "w_ctx is %s with %d context channels", w_ctx ? "given" : "null", c_ctx);
    if (c_ctx > 0 && kind != FV3HIP_CYCLEGAN_CONV_REGULAR)
        return fail(FV3HIP_EUNSUPPORTED, "context channels are built for the regular convolution, got kind %d", kind);
    if ((rc = check_slice("src", src, src_ld, src_off, c_in)) || (rc = check_slice("dst", dst, dst_ld, dst_off, c_out)) ||
        (rc = check_stride("src", &src_sample_stride, n, src_ld)) || (rc = check_stride("dst", &dst_sample_stride, n_out, dst_ld)) ||
        (rc = check_no_alias(Slice{src, src_ld, src_off, src_sample_stride, c_in, n},
                             Slice{dst, dst_ld, dst_off, dst_sample_stride, c_out, n_out}, n_samples, false)))
        return rc;
    if (n_samples == 0) return FV3HIP_OK;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src + src_off;
    a.dst = dst + dst_off;
    a.src_ld = src_ld;
    a.src_ss = src_sample_stride;
    a.dst_ld = dst_ld;
    a.dst_ss = dst_sample_stride;
    a.mean = in_mean;
    a.rstd = in_rstd;
    a.in_bias = in_bias;
    a.in_relu = in_relu ? 1 : 0;
    a.w = w;
    a.bias = bias;
    a.out_bias = out_bias;
    a.n = n;
    a.n_out = n_out;
    a.mg = kind == FV3HIP_CYCLEGAN_CONV_TRANSPOSED ? n : n_out;
    a.C = c_in;
    a.N = c_out;
    a.kind = kind;
    a.k = k;
    a.taps = taps;
    a.h = h;
    a.cube = halo_mode == FV3HIP_CYCLEGAN_HALO_CUBE ? 1 : 0;
    a.rows = n_samples * 6 * a.mg * a.mg;
    a.ctx_cell = ctx_cell;
    a.ctx_uni = ctx_uniform;
    a.w_ctx = w_ctx;
    a.c_cell = c_cell;
    a.c_ctx = c_ctx;
    a.seams = cube_seams();
    const int nt = c_out > 32 ? 2 : 1;
    FV3HIP_REQUIRE(ceil_div(c_out, nt * 32) <= 65535 && ceil_div(a.rows, kBM) <= 0x7fffffff, "the grid of %lld cells x %d channels is too large",
                   (long long)a.rows, c_out);
    dim3 grid((unsigned)ceil_div(a.rows, kBM), (unsigned)ceil_div(c_out, nt * 32), kind == FV3HIP_CYCLEGAN_CONV_TRANSPOSED ? 4u : 1u);
    const bool vec = c_in % 16 == 0 && src_ld % 4 == 0 && src_off % 4 == 0 && src_sample_stride % 4 == 0 && aligned16(src) &&
                     aligned16(in_mean) && aligned16(in_rstd) && aligned16(in_bias);
    const size_t lds = (size_t)taps * kBM * sizeof(int);
    using Kernel = void (*)(const ConvArgs);
    static const Kernel kernels[2][2][2] = {   // [nt - 1][vec][ctx]
        {{cyclegan_conv_kernel<1, false, false>, cyclegan_conv_kernel<1, false, true>},
         {cyclegan_conv_kernel<1, true, false>, cyclegan_conv_kernel<1, true, true>}},
        {{cyclegan_conv_kernel<2, false, false>, cyclegan_conv_kernel<2, false, true>},
         {cyclegan_conv_kernel<2, true, false>, cyclegan_conv_kernel<2, true, true>}}};
    hipLaunchKernelGGL(kernels[nt - 1][vec][c_ctx > 0], grid, dim3(kBlock), lds, as_stream(stream), a);
    return check_launch(c_ctx > 0 ? "cyclegan_conv_kernel (context)" : "cyclegan_conv_kernel");
}

}  // namespace

extern "C" int fv3hip_cyclegan_conv(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride,
                                    const float *in_mean, const float *in_rstd, const float *in_bias, int in_relu, const float *w,
                                    const float *bias, const float *out_bias, float *dst, int64_t dst_ld, int64_t dst_off,
                                    int64_t dst_sample_stride, int64_t n_samples, int n, int c_in, int c_out, int kind, int k,
                                    int halo_mode, void *stream)
{
    return launch_conv(src, src_ld, src_off, src_sample_stride, in_mean, in_rstd, in_bias, in_relu, w, bias, out_bias, dst, dst_ld,
                       dst_off, dst_sample_stride, n_samples, n, c_in, c_out, kind, k, halo_mode, nullptr, 0, nullptr, 0, nullptr, stream);
}

extern "C" int fv3hip_cyclegan_train_conv(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride, const float *w,
                                          const float *bias, float *dst, int64_t dst_ld, int64_t dst_off, int64_t dst_sample_stride,
                                          int64_t n_samples, int n, int c_in, int c_out, int kind, int k, int halo_mode, void *stream)
{
    return launch_conv(src, src_ld, src_off, src_sample_stride, nullptr, nullptr, nullptr, 0, w, bias, nullptr, dst, dst_ld, dst_off,
                       dst_sample_stride, n_samples, n, c_in, c_out, kind, k, halo_mode, nullptr, 0, nullptr, 0, nullptr, stream, true);
}

extern "C" int fv3hip_cyclegan_conv_context(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride,
                                            const float *in_mean, const float *in_rstd, const float *in_bias, int in_relu,
                                            const float *w, const float *bias, const float *out_bias, float *dst, int64_t dst_ld,
                                            int64_t dst_off, int64_t dst_sample_stride, int64_t n_samples, int n, int c_in, int c_out,
                                            int kind, int k, int halo_mode, const float *ctx_cell, int c_cell,
                                            const float *ctx_uniform, int c_uni, const float *w_ctx, void *stream)
{
    return launch_conv(src, src_ld, src_off, src_sample_stride, in_mean, in_rstd, in_bias, in_relu, w, bias, out_bias, dst, dst_ld,
                       dst_off, dst_sample_stride, n_samples, n, c_in, c_out, kind, k, halo_mode, ctx_cell, c_cell, ctx_uniform, c_uni,
                       w_ctx, stream);
}

extern "C" int fv3hip_cyclegan_stats(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride, float *mean,
                                     float *rstd, int64_t n_samples, int n, int c, double eps, void *stream)
{
    FV3HIP_REQUIRE(c >= 1 && c <= (1 << 16), "c must be in [1, 2^16], got %d", c);
    FV3HIP_REQUIRE(mean && rstd, "null statistics");
    FV3HIP_REQUIRE(eps >= 0, "eps must not be negative");
    int rc;
    if ((rc = check_cube(n_samples, n, kLimits)) || (rc = check_slice("src", src, src_ld, src_off, c)) ||
        (rc = check_stride("src", &src_sample_stride, n, src_ld)))
        return rc;
    if (n_samples == 0) return FV3HIP_OK;
    dim3 grid((unsigned)(n_samples * 6), (unsigned)ceil_div(c, kStatCh));
    hipLaunchKernelGGL(cyclegan_stats_kernel, grid, dim3(kBlock), 0, as_stream(stream), src + src_off, src_ld, src_sample_stride, mean,
                       rstd, n, c, eps);
    return check_launch("cyclegan_stats_kernel");
}

extern "C" int fv3hip_cyclegan_apply(const float *src, int64_t src_ld, int64_t src_off, int64_t src_sample_stride, const float *mean,
                                     const float *rstd, const float *bias, int relu, const float *res, int64_t res_ld,
                                     int64_t res_off, int64_t res_sample_stride, float *dst, int64_t dst_ld, int64_t dst_off,
                                     int64_t dst_sample_stride, int64_t n_samples, int n, int c, void *stream)
{
    FV3HIP_REQUIRE(c >= 1 && c <= (1 << 16), "c must be in [1, 2^16], got %d", c);
    FV3HIP_REQUIRE((mean == nullptr) == (rstd == nullptr), "mean and rstd come together");
    int rc;
    if ((rc = check_cube(n_samples, n, kLimits)) || (rc = check_slice("src", src, src_ld, src_off, c)) ||
        (rc = check_slice("dst", dst, dst_ld, dst_off, c)) || (rc = check_stride("src", &src_sample_stride, n, src_ld)) ||
        (rc = check_stride("dst", &dst_sample_stride, n, dst_ld)))
        return rc;
    // the pass works element by element, so the destination may be the source or the residual itself; any other overlap is refused
    const Slice s{src, src_ld, src_off, src_sample_stride, c, n}, d{dst, dst_ld, dst_off, dst_sample_stride, c, n};
    if (!same_slice(s, d) && (rc = check_no_alias(s, d, n_samples, false))) return rc;
    if (res) {
        if ((rc = check_slice("res", res, res_ld, res_off, c)) || (rc = check_stride("res", &res_sample_stride, n, res_ld))) return rc;
        const Slice r{res, res_ld, res_off, res_sample_stride, c, n};
        if (!same_slice(r, d) && (rc = check_no_alias(r, d, n_samples, false))) return rc;
    }
    const int64_t total = n_samples * 6 * n * n * c;
    if (total == 0) return FV3HIP_OK;
    hipLaunchKernelGGL(cyclegan_apply_kernel, dim3(grid_stride_blocks(total)), dim3(kBlock), 0, as_stream(stream), src + src_off, src_ld,
                       src_sample_stride, mean, rstd, bias, relu ? 1 : 0, res ? res + res_off : nullptr, res_ld, res_sample_stride,
                       dst + dst_off, dst_ld, dst_sample_stride, n_samples, n, c);
    return check_launch("cyclegan_apply_kernel");
}

extern "C" int fv3hip_cyclegan_input(const float *state, int64_t state_ld, int64_t state_off, int64_t state_sample_stride,
                                     const float *bias, const float *lon, const float *xyz, const float *theta, float *dst,
                                     int64_t dst_ld, int64_t dst_off, int64_t dst_sample_stride, int64_t n_samples, int n, int c,
                                     void *stream)
{
    FV3HIP_REQUIRE(c >= 1 && c <= (1 << 16), "c must be in [1, 2^16], got %d", c);
    FV3HIP_REQUIRE((lon == nullptr) == (xyz == nullptr) && (lon == nullptr) == (theta == nullptr), "lon, xyz and theta come together");
    const int c_out = c + (lon ? 5 : 0);
    int rc;
    if ((rc = check_cube(n_samples, n, kLimits)) || (rc = check_slice("state", state, state_ld, state_off, c)) ||
        (rc = check_slice("dst", dst, dst_ld, dst_off, c_out)) || (rc = check_stride("state", &state_sample_stride, n, state_ld)) ||
        (rc = check_stride("dst", &dst_sample_stride, n, dst_ld)) ||
        (rc = check_no_alias(Slice{state, state_ld, state_off, state_sample_stride, c, n},
                             Slice{dst, dst_ld, dst_off, dst_sample_stride, c_out, n}, n_samples, false)))
        return rc;
    const int64_t total = n_samples * 6 * n * n * c_out;
    if (total == 0) return FV3HIP_OK;
    hipLaunchKernelGGL(cyclegan_input_kernel, dim3(grid_stride_blocks(total)), dim3(kBlock), 0, as_stream(stream), state + state_off,
                       state_ld, state_sample_stride, bias, lon, xyz, theta, dst + dst_off, dst_ld, dst_sample_stride, n_samples, n, c);
    return check_launch("cyclegan_input_kernel");
}
