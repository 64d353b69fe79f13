// Training the convolutional network (fv3fit's "convolutional" training function,
// external/fv3fit/fv3fit/keras/_models/convolutional.py:101-210, shared/convolutional_network.py:59-195) on gfx950 -- DESIGN.md
// section 23.
//
// Activations are float32, channel-last [sample][x][y][channel] with element strides for sample, x and y; kernels are
// [a][b][c_in][f] (Keras Conv2D, cross-correlation, "valid") with a leading dimension on the last axis, i.e. a matrix
// [k k c_in][f].  conv_gemm_kernel<MODE> is train_gemm_kernel's skeleton (mlp_train.hip: one 64 x 64 block tile on the
// exact-f32 MFMA v_mfma_f32_32x32x2_f32, four waves with one 32 x 32 accumulator each, the contraction walked in chunks
// through LDS) as an implicit GEMM in three orientations -- the taps are offsets into the gathered operand, no im2col buffer
// exists.  Against that skeleton: the chunks are 32 deep, the next chunk is loaded into registers while the MFMAs of the current
// one run, and where a tile's upper 32 columns are padding the two waves that would own them share the contraction instead.
//     NN  forward          H[p][f]       = act(sum_{(a,b,c)} A[row(s)][x + a][y + b][c] W[(a,b,c)][f] + bias[f]),  p = (s, x, y) of H
//     NT  backward data    dA[q][c]      = (sum_{(a,b,f)} dH[s][x - a][y - b][f] W[(a,b,c)][f]) where P[q][c] > 0,   q = (s, x, y) of A
//     TN  backward weight  dW[(a,b,c)][f] = sum_p A[row(s)][x + a][y + b][c] dH[p][f];  db[f] = sum_p dH[p][f] (a ones row)
// row(s) = idx[s] where a sample table is given; a sample outside the table reads as zeros.  The TN form splits the batch's
// pixels into chunks of kChunkPixels (blockIdx.z); with more than one chunk every chunk writes its partial [k k C + 1][F] to the
// workspace and conv_chunk_sum_kernel adds them in ascending order.  No atomics: every result is a fixed-order sum that depends
// on the shapes only.
#include "common.h"

using namespace fv3hip;

namespace {

constexpr int kBlock = 256;
constexpr int kBM = 64, kBN = 64, kBK = 32, kBKLog2 = 5;
constexpr int kFill = kBM * kBK / kBlock;   // panel elements per thread and chunk
constexpr int kChunkPixels = 512;     // fv3hip_train_conv_chunk_pixels()
constexpr int kKP = kBK + 1;          // row stride of a panel stored [tile index][k]: odd, so that 32 tile indices hit 32 banks
constexpr int kMP = 96;               // row stride of a panel stored [k][tile index]: 32 mod 64 banks keeps the two lane halves apart
constexpr int kPanel = kBK * kMP;     // floats per panel (>= 64 * kKP)
constexpr int64_t kMaxPixels = (int64_t)1 << 24;   // of one batch, halo included: pixel numbers fit an int, chunks fit gridDim.z

enum { NN = 0, NT = 1, TN = 2 };

struct View {            // [sample][x][y][channel], channel stride 1
    const float *p;
    int64_t ss, sx, sy;
};

struct ConvGemmArgs {
    View a;                  // NN, TN: the layer's input A;  NT: dH
    const int64_t *idx;      // NN, TN: sample table or null
    int64_t a_samples;
    View bv;                 // TN: dH
    const float *w;          // NN, NT: W [k k C][ldw]
    int64_t ldw;
    float *c;                // NN: H;  NT: dA;  TN: dW [k k C][ldc], or the workspace when n_chunks > 1
    int64_t c_ss, c_sx, c_sy, ldc;
    const float *bias;       // NN
    float *db;               // TN
    View pv;                 // NT: post-ReLU activations (p null: no mask)
    int n;                   // samples of the batch
    int X, Y, OX, OY;        // extents of the layer's input and output (OX = X - k + 1)
    int k, C, F;
    int act, n_chunks;
};

template <bool KFAST>
__device__ __forceinline__ int panel_at(int kk, int i)
{
    return KFAST ? i * kKP + kk : kk * kMP + i;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void conv_gemm_kernel(const ConvGemmArgs g)
{
    // which operand is contiguous along the contraction in memory: its panel is filled and stored with k fastest
    constexpr bool AK = MODE != TN, BK = MODE == NT;
    __shared__ float ap[kPanel];
    __shared__ float bp[kPanel];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, l31 = lane & 31;
    const int wm = wave & 1, wn = wave >> 1;
    const int KC = g.k * g.k * g.C, KF = g.k * g.k * g.F;
    // the pixel grid that the rows (NN, NT) or the contraction (TN) run over
    const int PX = MODE == NT ? g.X : g.OX, PY = MODE == NT ? g.Y : g.OY;
    const int n_pix = g.n * PX * PY;
    const int M = MODE == TN ? KC + 1 : n_pix;
    const int N = MODE == NT ? g.C : g.F;
    const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
    int c_begin = 0, c_end = MODE == NN ? KC : MODE == NT ? KF : n_pix;
    if (MODE == TN) {
        c_begin = blockIdx.z * kChunkPixels;
        c_end = c_begin + kChunkPixels < n_pix ? c_begin + kChunkPixels : n_pix;
    }

    // what does not change along the contraction, looked up once
    int64_t base[kFill];         // NN: offset of the pixel's window in A (-1: reads as zeros);  NT: offset of the sample in dH
    int px[kFill], py[kFill];    // NT: the pixel (far out of range for a row past the end)
    int64_t moff = -1;           // TN: offset of the row's tap and channel within a window (-1: the ones row or past the end)
    if (MODE != TN) {
#pragma unroll
        for (int it = 0; it < kFill; ++it) {
            const int m = m0 + (tid >> kBKLog2) + (kBlock >> kBKLog2) * it;
            base[it] = -1, px[it] = py[it] = -(1 << 24);
            if (m < M) {
                const int s = m / (PX * PY), r = m - s * (PX * PY), x = r / PY, y = r - x * PY;
                if (MODE == NN) {
                    const int64_t row = g.idx ? g.idx[s] : s;
                    if (row >= 0 && row < g.a_samples) base[it] = row * g.a.ss + x * g.a.sx + y * g.a.sy;
                } else {
                    base[it] = s * g.a.ss, px[it] = x, py[it] = y;
                }
            }
        }
    } else {
        const int m = m0 + (tid & 63);
        if (m < KC) {
            const int tap = m / g.C, ch = m - tap * g.C, a = tap / g.k, b = tap - a * g.k;
            moff = a * g.a.sx + b * g.a.sy + ch;
        }
    }

    // A filter / channel tile whose upper 32 columns are all padding (F = 32 in a 64-wide tile) would leave two of the four
    // waves without work: they take every other k-pair of the lower 32 columns instead, and the two partial sums are added
    // once at the end, even k-pairs first -- a fixed order that depends on the shapes only.
    const bool split = N - n0 <= 32;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    // One 16-deep chunk of both operands, from global memory into registers (fetch) and from there into the panels (stash):
    // the loads of chunk c + 1 are issued before the MFMAs of chunk c and waited for after them.
    float ra[kFill], rb[kFill];
    auto fetch = [&](int c0) {
        if (MODE != TN) {
            // this thread's place along the contraction is the same for its kFill elements of the k-fast panels: one decode
            const int kk = tid & (kBK - 1), c = c0 + kk;
            const bool live = c < c_end;
            const int L = MODE == NN ? g.C : g.F;     // the fastest index of the contraction: channel (NN), filter (NT)
            const int tap = c / L, ch = c - tap * L, a = tap / g.k, b = tap - a * g.k;
            const int64_t koff = a * g.a.sx + b * g.a.sy + ch;   // NN
#pragma unroll
            for (int it = 0; it < kFill; ++it) {
                const int i = (tid >> kBKLog2) + (kBlock >> kBKLog2) * it;
                float v = 0.f, wv = 0.f;
                if (MODE == NN) {
                    if (live && base[it] >= 0) v = g.a.p[base[it] + koff];
                    const int e = tid + kBlock * it, kb = e >> 6, j = e & 63;
                    if (c0 + kb < c_end && n0 + j < N) wv = g.w[(int64_t)(c0 + kb) * g.ldw + n0 + j];
                } else {
                    const int xx = px[it] - a, yy = py[it] - b;
                    if (live && xx >= 0 && xx < g.OX && yy >= 0 && yy < g.OY) v = g.a.p[base[it] + xx * g.a.sx + yy * g.a.sy + ch];
                    if (live && n0 + i < N) wv = g.w[((int64_t)tap * g.C + n0 + i) * g.ldw + ch];   // W[(a, b, channel n0 + i)][filter ch]
                }
                ra[it] = v, rb[it] = wv;
            }
        } else {
            const int i = tid & 63;
#pragma unroll
            for (int it = 0; it < kFill; ++it) {
                const int pix = c0 + (tid >> 6) + (kBlock >> 6) * it;
                float av = 0.f, bv = 0.f;
                if (pix < c_end) {
                    const int s = pix / (PX * PY), r = pix - s * (PX * PY), x = r / PY, y = r - x * PY;
                    if (moff >= 0) {
                        const int64_t row = g.idx ? g.idx[s] : s;
                        if (row >= 0 && row < g.a_samples) av = g.a.p[row * g.a.ss + x * g.a.sx + y * g.a.sy + moff];
                    } else if (m0 + i == KC) {
                        av = 1.f;
                    }
                    if (n0 + i < N) bv = g.bv.p[s * g.bv.ss + x * g.bv.sx + y * g.bv.sy + n0 + i];
                }
                ra[it] = av, rb[it] = bv;
            }
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int it = 0; it < kFill; ++it) {
            if (MODE != TN) {
                const int kk = tid & (kBK - 1), i = (tid >> kBKLog2) + (kBlock >> kBKLog2) * it;
                ap[panel_at<AK>(kk, i)] = ra[it];
                if (MODE == NN) {
                    const int e = tid + kBlock * it;
                    bp[panel_at<BK>(e >> 6, e & 63)] = rb[it];
                } else {
                    bp[panel_at<BK>(kk, i)] = rb[it];
                }
            } else {
                const int kk = (tid >> 6) + (kBlock >> 6) * it, i = tid & 63;
                ap[panel_at<AK>(kk, i)] = ra[it];
                bp[panel_at<BK>(kk, i)] = rb[it];
            }
        }
    };

    fetch(c_begin);
    for (int c0 = c_begin; c0 < c_end; c0 += kBK) {
        __syncthreads();   // (the MFMAs of the chunk before have read the panels)
        stash();
        __syncthreads();
        if (c0 + kBK < c_end) fetch(c0 + kBK);
        if (!split) {
#pragma unroll
            for (int kp = 0; kp < kBK / 2; ++kp) {
                const int kr = 2 * kp + hh;
                const float av = ap[panel_at<AK>(kr, wm * 32 + l31)];
                const float bv = bp[panel_at<BK>(kr, wn * 32 + l31)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
        } else {   // columns 0 .. 31 on both wave pairs: pair wn takes the k-pairs kp = wn (mod 2)
#pragma unroll
            for (int kp = 0; kp < kBK / 4; ++kp) {
                const int kr = 2 * (2 * kp + wn) + hh;
                const float av = ap[panel_at<AK>(kr, wm * 32 + l31)];
                const float bv = bp[panel_at<BK>(kr, l31)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
        }
    }

    if (split) {   // the even k-pairs' sum + the odd k-pairs' sum, through the panel the row half no longer needs
        float *red = wm ? bp : ap;
        __syncthreads();
        if (wn == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) red[r * kWave + lane] = acc[r];
        }
        __syncthreads();
        if (wn == 1) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += red[r * kWave + lane];
    }

    // epilogue: D[row][col], col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int nn = n0 + (split ? 0 : wn * 32) + l31;
    if (nn >= N) return;
    const float bias = (MODE == NN && g.bias) ? g.bias[nn] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (m >= M) continue;
        float v = acc[r];
        if (MODE != TN) {
            const int s = m / (PX * PY), q = m - s * (PX * PY), x = q / PY, y = q - x * PY;
            if (MODE == NN) {
                v += bias;
                if (g.act == FV3HIP_ACT_RELU) v = v < 0.f ? 0.f : v;   // (a NaN stays a NaN, as in torch's relu)
            } else if (g.pv.p && !(g.pv.p[s * g.pv.ss + x * g.pv.sx + y * g.pv.sy + nn] > 0.f)) {
                v = 0.f;   // relu'(0) = 0, as in torch
            }
            g.c[s * g.c_ss + x * g.c_sx + y * g.c_sy + nn] = v;
        } else if (g.n_chunks > 1) {
            g.c[((int64_t)blockIdx.z * M + m) * N + nn] = v;
        } else if (m == KC) {
            if (g.db) g.db[nn] = v;
        } else {
            g.c[(int64_t)m * g.ldc + nn] = v;
        }
    }
}

// dW[(a,b,c)][f], db[f] = the chunks' partials [chunk][k k C + 1][F], added in ascending order
__global__ __launch_bounds__(kBlock) void conv_chunk_sum_kernel(const float *ws, int n_chunks, int kc, int f, float *dw, int64_t lddw,
                                                                 float *db)
{
    const int64_t total = (int64_t)(kc + 1) * f;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        float s = ws[e];
        for (int z = 1; z < n_chunks; ++z) s += ws[z * total + e];
        const int64_t m = e / f, nn = e % f;
        if (m == kc) {
            if (db) db[nn] = s;
        } else {
            dw[m * lddw + nn] = s;
        }
    }
}

// TransposeInvariant (convolutional_network.py:20-26): both members of a pair (a, b), (b, a) from the one sum
__global__ __launch_bounds__(kBlock) void conv_constrain_kernel(float *w, int64_t ldw, int k, int c, int f)
{
    const int64_t per_tap = (int64_t)c * f, total = (int64_t)k * k * per_tap;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int tap = (int)(e / per_tap);
        const int64_t r = e - tap * per_tap;
        const int a = tap / k, b = tap - a * k;
        if (a > b) continue;
        const int64_t cc = r / f, ff = r - cc * f;
        const int64_t lo = ((int64_t)(a * k + b) * c + cc) * ldw + ff, hi = ((int64_t)(b * k + a) * c + cc) * ldw + ff;
        const float v = 0.5f * (w[lo] + w[hi]);
        w[lo] = v;
        w[hi] = v;
    }
}

int check_shape(int64_t n, int X, int Y, int k, int c, int f)
{
    FV3HIP_REQUIRE(k >= 1 && k % 2 == 1 && k <= 31, "kernel_size must be odd and in [1, 31], got %d", k);
    FV3HIP_REQUIRE(c >= 1 && f >= 1 && c <= (1 << 16) && f <= (1 << 16), "channels and filters must be in [1, 2^16], got %d, %d", c, f);
    FV3HIP_REQUIRE(X >= k && Y >= k && X <= (1 << 20) && Y <= (1 << 20), "an input of %d x %d cells does not hold a %d x %d kernel", X, Y, k, k);
    FV3HIP_REQUIRE(n >= 1 && n * X * Y <= kMaxPixels, "the batch must hold between 1 sample and 2^24 pixels, got %lld samples of %d x %d",
                   (long long)n, X, Y);
    return FV3HIP_OK;
}

int check_view(const char *what, const void *p, int64_t ss, int64_t sx, int64_t sy, int channels)
{
    FV3HIP_REQUIRE(p, "%s is null", what);
    const int64_t top = (int64_t)1 << 40;
    FV3HIP_REQUIRE(ss >= 0 && sx >= 0 && sy >= channels && ss <= top && sx <= top && sy <= top,
                   "%s: strides (%lld, %lld, %lld) do not hold %d contiguous channels", what, (long long)ss, (long long)sx, (long long)sy,
                   channels);
    return FV3HIP_OK;
}

int check_kernel(const char *what, const void *p, int64_t ld, int f)
{
    FV3HIP_REQUIRE(p, "%s is null", what);
    FV3HIP_REQUIRE(ld >= f && ld <= ((int64_t)1 << 24), "%s: leading dimension %lld does not hold %d filters", what, (long long)ld, f);
    return FV3HIP_OK;
}

void set_shape(ConvGemmArgs &g, int64_t n, int X, int Y, int k, int c, int f)
{
    g.n = (int)n, g.X = X, g.Y = Y, g.OX = X - k + 1, g.OY = Y - k + 1, g.k = k, g.C = c, g.F = f, g.n_chunks = 1;
}

}  // namespace

extern "C" int fv3hip_train_conv_chunk_pixels(void) { return kChunkPixels; }

extern "C" size_t fv3hip_train_conv_backward_weight_workspace_bytes(int64_t n, int X, int Y, int k, int c, int f)
{
    if (n < 1 || k < 1 || X < k || Y < k || c < 1 || f < 1) return 0;
    const int64_t pixels = n * (X - k + 1) * (Y - k + 1);
    if (pixels <= kChunkPixels) return 0;
    return (size_t)ceil_div(pixels, kChunkPixels) * ((size_t)k * k * c + 1) * (size_t)f * sizeof(float);
}

extern "C" int fv3hip_train_conv_forward(const float *A, int64_t a_ss, int64_t a_sx, int64_t a_sy, int64_t a_samples, const int64_t *idx,
                                         const float *W, int64_t ldw, const float *bias, float *H, int64_t h_ss, int64_t h_sx,
                                         int64_t h_sy, int64_t n, int X, int Y, int k, int c, int f, int act, void *stream)
{
    int rc;
    if ((rc = check_shape(n, X, Y, k, c, f)) || (rc = check_view("A", A, a_ss, a_sx, a_sy, c)) || (rc = check_kernel("W", W, ldw, f)) ||
        (rc = check_view("H", H, h_ss, h_sx, h_sy, f)))
        return rc;
    FV3HIP_REQUIRE(a_samples >= 1 && (idx || a_samples >= n), "A has %lld samples, the batch %lld", (long long)a_samples, (long long)n);
    if (act != FV3HIP_ACT_LINEAR && act != FV3HIP_ACT_RELU)
        return fail(FV3HIP_EUNSUPPORTED, "activation code %d: FV3HIP_ACT_LINEAR and _RELU are built", act);
    ConvGemmArgs g{};
    set_shape(g, n, X, Y, k, c, f);
    g.a = View{A, a_ss, a_sx, a_sy}, g.idx = idx, g.a_samples = a_samples, g.w = W, g.ldw = ldw, g.bias = bias;
    g.c = H, g.c_ss = h_ss, g.c_sx = h_sx, g.c_sy = h_sy, g.act = act;
    const dim3 grid((unsigned)ceil_div(n * g.OX * g.OY, kBM), (unsigned)ceil_div(f, kBN));
    hipLaunchKernelGGL(conv_gemm_kernel<NN>, grid, dim3(kBlock), 0, as_stream(stream), g);
    return check_launch("conv_gemm_kernel<NN>");
}

extern "C" int fv3hip_train_conv_backward_data(const float *dH, int64_t dh_ss, int64_t dh_sx, int64_t dh_sy, const float *W, int64_t ldw,
                                               const float *P, int64_t p_ss, int64_t p_sx, int64_t p_sy, float *dA, int64_t da_ss,
                                               int64_t da_sx, int64_t da_sy, int64_t n, int X, int Y, int k, int c, int f, void *stream)
{
    int rc;
    if ((rc = check_shape(n, X, Y, k, c, f)) || (rc = check_view("dH", dH, dh_ss, dh_sx, dh_sy, f)) || (rc = check_kernel("W", W, ldw, f)) ||
        (rc = check_view("dA", dA, da_ss, da_sx, da_sy, c)))
        return rc;
    if (P && (rc = check_view("P", P, p_ss, p_sx, p_sy, c))) return rc;
    ConvGemmArgs g{};
    set_shape(g, n, X, Y, k, c, f);
    g.a = View{dH, dh_ss, dh_sx, dh_sy}, g.w = W, g.ldw = ldw, g.pv = View{P, p_ss, p_sx, p_sy};
    g.c = dA, g.c_ss = da_ss, g.c_sx = da_sx, g.c_sy = da_sy;
    const dim3 grid((unsigned)ceil_div(n * X * Y, kBM), (unsigned)ceil_div(c, kBN));
    hipLaunchKernelGGL(conv_gemm_kernel<NT>, grid, dim3(kBlock), 0, as_stream(stream), g);
    return check_launch("conv_gemm_kernel<NT>");
}

extern "C" int fv3hip_train_conv_backward_weight(const float *A, int64_t a_ss, int64_t a_sx, int64_t a_sy, int64_t a_samples,
                                                 const int64_t *idx, const float *dH, int64_t dh_ss, int64_t dh_sx, int64_t dh_sy,
                                                 float *dW, int64_t lddw, float *db, float *workspace, size_t workspace_bytes,
                                                 int64_t n, int X, int Y, int k, int c, int f, void *stream)
{
    int rc;
    if ((rc = check_shape(n, X, Y, k, c, f)) || (rc = check_view("A", A, a_ss, a_sx, a_sy, c)) ||
        (rc = check_view("dH", dH, dh_ss, dh_sx, dh_sy, f)) || (rc = check_kernel("dW", dW, lddw, f)))
        return rc;
    FV3HIP_REQUIRE(a_samples >= 1 && (idx || a_samples >= n), "A has %lld samples, the batch %lld", (long long)a_samples, (long long)n);
    const int kc = k * k * c;
    const int64_t pixels = n * (X - k + 1) * (Y - k + 1);
    const int n_chunks = (int)ceil_div(pixels, kChunkPixels);
    const size_t need = fv3hip_train_conv_backward_weight_workspace_bytes(n, X, Y, k, c, f);
    FV3HIP_REQUIRE(n_chunks == 1 || (workspace && workspace_bytes >= need), "a batch of %lld pixels needs a workspace of %zu bytes, got %zu",
                   (long long)pixels, need, workspace ? workspace_bytes : (size_t)0);
    ConvGemmArgs g{};
    set_shape(g, n, X, Y, k, c, f);
    g.a = View{A, a_ss, a_sx, a_sy}, g.idx = idx, g.a_samples = a_samples, g.bv = View{dH, dh_ss, dh_sx, dh_sy}, g.db = db;
    g.c = n_chunks > 1 ? workspace : dW, g.ldc = lddw, g.n_chunks = n_chunks;
    const dim3 grid((unsigned)ceil_div(kc + 1, kBM), (unsigned)ceil_div(f, kBN), (unsigned)n_chunks);
    hipLaunchKernelGGL(conv_gemm_kernel<TN>, grid, dim3(kBlock), 0, as_stream(stream), g);
    if ((rc = check_launch("conv_gemm_kernel<TN>"))) return rc;
    if (n_chunks > 1) {
        hipLaunchKernelGGL(conv_chunk_sum_kernel, dim3(grid_stride_blocks((int64_t)(kc + 1) * f)), dim3(kBlock), 0, as_stream(stream),
                           workspace, n_chunks, kc, f, dW, lddw, db);
        return check_launch("conv_chunk_sum_kernel");
    }
    return FV3HIP_OK;
}

extern "C" int fv3hip_train_conv_constrain(float *W, int64_t ldw, int k, int c, int f, void *stream)
{
    int rc;
    FV3HIP_REQUIRE(k >= 1 && k % 2 == 1 && k <= 31, "kernel_size must be odd and in [1, 31], got %d", k);
    FV3HIP_REQUIRE(c >= 1 && f >= 1 && c <= (1 << 16) && f <= (1 << 16), "channels and filters must be in [1, 2^16], got %d, %d", c, f);
    if ((rc = check_kernel("W", W, ldw, f))) return rc;
    hipLaunchKernelGGL(conv_constrain_kernel, dim3(grid_stride_blocks((int64_t)k * k * c * f)), dim3(kBlock), 0, as_stream(stream), W,
                       ldw, k, c, f);
    return check_launch("conv_constrain_kernel");
}
