// Training fv3fit's CycleGAN (pytorch/cyclegan/train_cyclegan.py, cyclegan_trainer.py): the adjoints of the cube-halo
// convolutions of cyclegan.hip and of its instance norm -- DESIGN.md section 27.  The forward of the training layers is
// fv3hip_cyclegan_train_conv (cyclegan.hip: the forward kernel without the loader's transform).
//
// Write T(o, t) for the padded position that tap t of output cell o reads and x~ for the halo-extended face (the neighbour's
// cells by the seam rule of cube.h, corners zero; or zeros).  The forward is y[s,f,o] = sum_t W_t^T x~[s,f,T(o,t)].
//
// cyclegan_bwd_data_kernel is the gradient of the PADDED field, dx~[s,f,p] = sum_{(o,t): T(o,t)=p} W_t dy[s,f,o], as one implicit
// GEMM with the forward's skeleton: M = padded positions flattened over (sample, tile, X, Y), 128 per block, N = input channels,
// K = taps x c_out with the channel fastest.  A block first writes, per (tap, row), the output cell whose tap reads the row's
// position (or none) into LDS; the loader gathers dy through that table and reads W_t transposed.  Nothing in it knows the
// seams.  With zero padding the rows are the face's own cells and the result is dx itself.  With cube halos the padded gradient
// goes to the caller's workspace and cyclegan_fold_kernel adds, for every cell, its own position and the halo positions of the
// neighbouring faces that show it (the inverse of seam_cross; one per side the cell lies within the halo width of), in the fixed
// order own, x-low, x-high, y-low, y-high.  The face rotations make this no flipped-kernel convolution of a halo-extended dy.
//
// cyclegan_bwd_weight_kernel is dW_t[ci][co] = sum_{s,f,o} x~[s,f,T(o,t)][ci] dy[s,f,o][co] in the forward's weight layout: one
// block per (weight block, 64 input channels, 64 output channels, chunk of 512 rows); x~ is gathered through the forward's
// table (written once per block); db is the chunk's sum of dy in float64 (cyclegan_bias_grad_kernel).  The chunks' partials are added in
// ascending order by cyclegan_chunk_sum_kernel.  No atomics anywhere: every result is bitwise reproducible and a sample's dx
// does not depend on the batch it is in.
//
// Training the recurrent (FMR) generator, DESIGN.md section 28.  A layer with context channels (fv3hip_cyclegan_conv_context)
// has c_cell + c_uni further rows of x~ per tap: cyclegan_bwd_weight_kernel<true> lets the A loader run past c_in, into the
// per-cell table at the row's cell or the uniform values, both zero where the row shows no cell -- as the forward resolves
// them -- and writes those rows into their own block dw_ctx [taps][c_cell + c_uni][c_out].  The context has no gradient, so
// backward-data is unchanged.  fmr_loss_kernel is the window loss (identity on time 0, target on the later times) and its
// gradient added to the discriminator's, one writer per element; fmr_loss_finish_kernel adds the blocks' float64 partials
// in ascending order.
#include <cmath>

#include "common.h"
#include "cube.h"

using namespace fv3hip;

namespace {

constexpr int kBlock = 256;    // four waves
constexpr int kBM = 128;       // rows per block of the data gradient: one 32-row MFMA tile per wave
constexpr int kRows = 16;      // K rows per chunk of LDS
constexpr int kChunk = 512;    // fv3hip_cyclegan_train_chunk_cells(): rows per partial of the weight gradient
constexpr int kMP = 96;        // row stride of a [k][tile index] panel: 32 mod 64 banks keeps the two lane halves apart
constexpr int kStatCh = 16;    // norm backward: channels per block, 16 groups of cells each

constexpr CubeLimits kLimits{1 << 20, "2^20", 4096};

struct Geom {
    int kind, k, h;     // taps = k * k
    int n, n_out;       // the edges of x and of dy
    int cube;           // halo mode
};

// the checks of launch_conv (cyclegan.hip) with the 3 x 3 strided convolution
int check_geometry(int n, int kind, int k, int halo_mode, Geom &g)
{
    FV3HIP_REQUIRE(halo_mode == FV3HIP_CYCLEGAN_HALO_ZEROS || halo_mode == FV3HIP_CYCLEGAN_HALO_CUBE, "unknown halo mode %d", halo_mode);
    g.kind = kind, g.k = k, g.h = 1, g.n = n, g.n_out = n, g.cube = halo_mode == FV3HIP_CYCLEGAN_HALO_CUBE ? 1 : 0;
    if (kind == FV3HIP_CYCLEGAN_CONV_REGULAR) {
        if (k != 3 && k != 5 && k != 7) return fail(FV3HIP_EUNSUPPORTED, "regular convolution with k = %d: 3, 5 and 7 are built", k);
        g.h = (k - 1) / 2;
    } else if (kind == FV3HIP_CYCLEGAN_CONV_STRIDED) {
        if (k != 3 && k != 4) return fail(FV3HIP_EUNSUPPORTED, "strided convolution with k = %d: 3 and 4 are built", k);
        FV3HIP_REQUIRE(n % 2 == 0, "n must be even for the stride-2 convolution, got %d", n);
        g.n_out = n / 2;
    } else if (kind == FV3HIP_CYCLEGAN_CONV_TRANSPOSED) {
        if (k != 4) return fail(FV3HIP_EUNSUPPORTED, "transposed convolution is built for k = 4, got %d", k);
        FV3HIP_REQUIRE(n <= 2048, "n must be at most 2048 (the output has 2 n cells per edge), got %d", n);
        g.n_out = 2 * n;
    } else {
        return fail(FV3HIP_EUNSUPPORTED, "unknown convolution kind %d", kind);
    }
    FV3HIP_REQUIRE(g.h <= n, "the halo (%d cells) is wider than the face (%d)", g.h, n);
    return FV3HIP_OK;
}

int check_channels(int c_in, int c_out)
{
    FV3HIP_REQUIRE(c_in >= 1 && c_out >= 1 && c_in <= (1 << 16) && c_out <= (1 << 16), "c_in and c_out must be in [1, 2^16], got %d, %d",
                   c_in, c_out);
    return FV3HIP_OK;
}

// the weight block [c_in][c_out] of tap (tx, ty) in the forward's layout: [k][k], or the parity split [px][py][a][b] of the
// transposed kind (torch's kx = 1 + 2 a for px = 0, 2 a for px = 1)
__host__ __device__ inline int weight_block(const Geom &g, int tx, int ty)
{
    if (g.kind != FV3HIP_CYCLEGAN_CONV_TRANSPOSED) return tx * g.k + ty;
    return (((1 - (tx & 1)) * 2 + (1 - (ty & 1))) * 2 + (tx >> 1)) * 2 + (ty >> 1);
}

// per axis: the output index whose tap t reads padded position X (-h ... n + h - 1, relative to the face), or -1
__host__ __device__ inline int output_of(const Geom &g, int X, int t)
{
    int o;
    if (g.kind == FV3HIP_CYCLEGAN_CONV_REGULAR) {
        o = X - t + g.h;               // X = o + t - h
    } else if (g.kind == FV3HIP_CYCLEGAN_CONV_STRIDED) {
        const int o2 = X + 1 - t;      // X = 2 o - 1 + t
        if (o2 & 1) return -1;
        o = o2 >> 1;
    } else {
        o = 2 * X - 1 + t;             // cell m feeds outputs 2 m - 1 ... 2 m + 2 through taps 0 ... 3
    }
    return (unsigned)o < (unsigned)g.n_out ? o : -1;
}

// per axis: the padded position that tap t (slot: the tap of the parity for the transposed kind) of row index x reads; the rows
// are the output cells, for the transposed kind the input-grid cells x of output 2 x + par
__host__ __device__ inline int position_of(const Geom &g, int x, int t, int par)
{
    if (g.kind == FV3HIP_CYCLEGAN_CONV_REGULAR) return x + t - g.h;
    if (g.kind == FV3HIP_CYCLEGAN_CONV_STRIDED) return 2 * x - 1 + t;
    return x + (par ? 1 - t : -t);
}

// cell (t * n + x) * n + y that position (x, y) of tile t's padded field shows; -1: a zero (cyclegan.hip's source_cell)
__host__ __device__ inline int source_cell(const Geom &g, const CubeSeams &seams, int t, int x, int y)
{
    const int n = g.n;
    const bool inx = (unsigned)x < (unsigned)n, iny = (unsigned)y < (unsigned)n;
    if (inx && iny) return (t * n + x) * n + y;
    if (!g.cube || (!inx && !iny)) return -1;
    int side, d, j;
    if (!inx) {
        side = x < 0 ? 0 : 1;
        d = x < 0 ? -1 - x : x - n;
        j = y;
    } else {
        side = y < 0 ? 2 : 3;
        d = y < 0 ? -1 - y : y - n;
        j = x;
    }
    const int q = t * 4 + side;
    const int line = (side & 1) ? d : n - 1 - d;
    const int jj = seams.flip[q] ? n - 1 - j : j;
    const int tt = seams.nbr[q];
    return seams.nax[q] ? (tt * n + line) * n + jj : (tt * n + jj) * n + line;
}

// the inverse of the seam rule: cell (x, y) of tile t lies `d` lines inside its edge `side` (0 x-low, 1 x-high, 2 y-low,
// 3 y-high); the neighbouring face across that edge shows it at halo position (X, Y) of its own padded field
__host__ __device__ inline void alias_position(const CubeSeams &s, int n, int t, int side, int x, int y, int &tt, int &X, int &Y)
{
    const int d = side == 0 ? x : side == 1 ? n - 1 - x : side == 2 ? y : n - 1 - y;
    const int along = side < 2 ? y : x;
    tt = s.nbr[t * 4 + side];
    int e = 0;   // the neighbour's side that leads back (two faces share at most one edge)
    for (int q = 0; q < 4; ++q)
        if (s.nbr[tt * 4 + q] == t) e = q;
    const int j = s.flip[tt * 4 + e] ? n - 1 - along : along;
    const int out = (e & 1) ? n + d : -1 - d;
    X = e < 2 ? out : j;
    Y = e < 2 ? j : out;
}

__host__ __device__ inline int side_depth(int n, int side, int x, int y)
{
    return side == 0 ? x : side == 1 ? n - 1 - x : side == 2 ? y : n - 1 - y;
}

struct BwdDataArgs {
    const float *dy;         // channel offset applied
    float *dst;              // the padded gradient [sample][6][np][np][N] (cube halos), or dx itself (np = n)
    int64_t dy_ld, dy_ss, dst_ld, dst_ss;
    const float *w;          // the forward's weights
    Geom g;
    int np, hp;              // edge of the grid the rows are flattened over, and its offset: X = Xp - hp
    int C, N;                // K channels (c_out) and result channels (c_in)
    int64_t rows;            // n_samples * 6 * np * np
};

// VEC: c_out is a multiple of 16 and every pointer and stride of dy a multiple of four floats (as cyclegan_conv_kernel)
template <int NT, bool VEC>
__global__ __launch_bounds__(kBlock) void cyclegan_bwd_data_kernel(const BwdDataArgs a)
{
    constexpr int AP = kBM + 2;
    constexpr int NG = NT * 32;
    constexpr int WP = NG + 1;             // the loader writes 16 K rows of one column at once
    extern __shared__ int sidx[];          // [taps][kBM]: the dy cell, -1: none
    __shared__ int srow[kBM], srem[kBM];   // sample and padded cell of every row; -1: past the end
    __shared__ float al[kRows * AP];
    __shared__ float wl[kRows * WP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, l31 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * kBM;
    const int n0 = blockIdx.y * NG;
    const int np = a.np, cells = 6 * np * np, taps = a.g.k * a.g.k;

    if (tid < kBM) {
        const int64_t g = row0 + tid;
        srow[tid] = g < a.rows ? (int)(g / cells) : -1;
        srem[tid] = g < a.rows ? (int)(g % cells) : 0;
    }
    for (int e = tid; e < taps * kBM; e += kBlock) {
        const int r = e % kBM, tap = e / kBM;
        const int64_t g = row0 + r;
        int idx = -1;
        if (g < a.rows) {
            const int rem = (int)(g % cells);
            const int t = rem / (np * np), X = rem / np % np - a.hp, Y = rem % np - a.hp;
            const bool inx = (unsigned)X < (unsigned)a.g.n, iny = (unsigned)Y < (unsigned)a.g.n;
            if (inx || iny) {   // (the corners of the halo show no cell)
                const int ox = output_of(a.g, X, tap / a.g.k), oy = output_of(a.g, Y, tap % a.g.k);
                if (ox >= 0 && oy >= 0) idx = (t * a.g.n_out + ox) * a.g.n_out + oy;
            }
        }
        sidx[tap * kBM + r] = idx;
    }

    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    const int K = taps * a.C;
    const int kk = tid & 15;   // every loader pass of this thread fills K row kk of the chunk
    for (int k0 = 0; k0 < K; k0 += kRows) {
        __syncthreads();
        if (VEC) {
            const int tap = k0 / a.C, c = k0 - tap * a.C + 4 * (tid & 3);
#pragma unroll
            for (int i = 0; i < kRows * kBM / kBlock / 4; ++i) {
                const int r = (tid >> 2) + 64 * i;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                const int idx = sidx[tap * kBM + r];
                if (idx >= 0) v = *reinterpret_cast<const float4 *>(a.dy + (int64_t)srow[r] * a.dy_ss + (int64_t)idx * a.dy_ld + c);
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
            const int idx = kg < K ? sidx[tap * kBM + r] : -1;
            if (idx >= 0) v = a.dy[(int64_t)srow[r] * a.dy_ss + (int64_t)idx * a.dy_ld + c];
            al[kk * AP + r] = v;
        }
        // W_t transposed: K row (tap, co), column ci is w[block(tap)][ci][co]
        const int64_t wb = (int64_t)weight_block(a.g, tap / a.g.k, tap % a.g.k) * a.N;
        for (int j = tid >> 4; j < NG; j += kBlock / kRows) {
            const int nn = n0 + j;
            wl[kk * WP + j] = (kg < K && nn < a.N) ? a.w[(wb + nn) * a.C + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kp = 0; kp < kRows / 2; ++kp) {
            const int kr = 2 * kp + hh;
            const float xv = al[kr * AP + wave * 32 + l31];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, wl[kr * WP + nt * 32 + l31], acc[nt], 0, 0, 0);
        }
    }

    // epilogue: D[row][col], col = lane & 31 (channel), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (row of the MFMA tile)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int nn = n0 + nt * 32 + l31;
        if (nn >= a.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            const int64_t s = srow[rr];
            if (s < 0) continue;
            a.dst[s * a.dst_ss + (int64_t)srem[rr] * a.dst_ld + nn] = acc[nt][r];
        }
    }
}

// dx[s][t][x][y][c] = the padded gradient at the cell's own position + at every halo position that shows the cell
__global__ __launch_bounds__(kBlock) void cyclegan_fold_kernel(const float *pad, float *dx, int64_t dx_ld, int64_t dx_ss, int64_t n_samples,
                                                               int n, int h, int C, const CubeSeams seams)
{
    const int np = n + 2 * h;
    const int64_t cells = 6LL * n * n, pcube = 6LL * np * np * C, total = n_samples * cells * C;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int c = (int)(e % C);
        const int64_t r = e / C, s = r / cells;
        const int cell = (int)(r % cells);
        const int t = cell / (n * n), x = cell / n % n, y = cell % n;
        const float *p = pad + s * pcube + c;
        float v = p[(((int64_t)t * np + x + h) * np + y + h) * C];
        for (int side = 0; side < 4; ++side) {
            if (side_depth(n, side, x, y) >= h) continue;
            int tt, X, Y;
            alias_position(seams, n, t, side, x, y, tt, X, Y);
            v = v + p[(((int64_t)tt * np + X + h) * np + Y + h) * C];
        }
        dx[s * dx_ss + (int64_t)cell * dx_ld + c] = v;
    }
}

struct BwdWeightArgs {
    const float *x, *dy;     // channel offsets applied
    int64_t x_ld, x_ss, dy_ld, dy_ss;
    float *dw, *db, *ws;     // ws [chunk][blocks * (c_in + c_ctx) + 2][c_out]: the dW partial, the context rows' partial, then one
                             // float64 per channel (two words)
    const float *ctx_cell;   // [6][n][n][c_cell] or null
    const float *ctx_uni;    // [c_ctx - c_cell] or null
    float *dw_ctx;           // [blocks][c_ctx][c_out] or null
    int c_cell, c_ctx;       // per-cell context channels; all context channels
    Geom g;
    int mg;                  // edge of the grid the rows are flattened over: n_out, n for the transposed kind
    int c_in, c_out, blocks, mtiles, n_chunks;
    int64_t rows;            // n_samples * 6 * mg * mg
    CubeSeams seams;
};

// floats of one chunk's partial: dW [blocks][c_in][c_out], the context rows [blocks][c_ctx][c_out], then the float64 sum of dy
// per channel as (high, low) words -- the offset of that part may be odd, so it is not addressed as doubles
__host__ __device__ inline int64_t partial_floats(int blocks, int c_in, int c_ctx, int c_out)
{
    return ((int64_t)blocks * (c_in + c_ctx) + 2) * c_out;
}

// CTX: the A rows run on past c_in into the context channels (mtiles covers c_in + c_ctx); without it this is the kernel as it
// was, and a source row's sum does not depend on which of the two ran
template <bool CTX>
__global__ __launch_bounds__(kBlock) void cyclegan_bwd_weight_kernel(const BwdWeightArgs a)
{
    __shared__ int xcell[kChunk], ycell[kChunk], smp[kChunk];   // per row of the chunk: the cell of x~ (-1: a zero), of dy, the sample
    __shared__ float ap[kRows * kMP];
    __shared__ float bp[kRows * kMP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, l31 = lane & 31;
    const int wm = wave & 1, wn = wave >> 1;
    const int wblock = blockIdx.x / a.mtiles, ci0 = (blockIdx.x % a.mtiles) * 64, n0 = blockIdx.y * 64;
    const bool transposed = a.g.kind == FV3HIP_CYCLEGAN_CONV_TRANSPOSED;
    const int mg = a.mg, cells = 6 * mg * mg;
    const int c_begin = blockIdx.z * kChunk;
    const int len = (int64_t)c_begin + kChunk < a.rows ? kChunk : (int)(a.rows - c_begin);
    // the tap of this weight block: (tx, ty) of [k][k], or parity (px, py) and tap (ta, tb) of [px][py][a][b]
    const int tx = transposed ? (wblock >> 1) & 1 : wblock / a.g.k, ty = transposed ? wblock & 1 : wblock % a.g.k;
    const int px = transposed ? wblock >> 3 : 0, py = transposed ? (wblock >> 2) & 1 : 0;

    for (int r = tid; r < kChunk; r += kBlock) {
        int xc = -1, yc = 0, s = 0;
        if (r < len) {
            const int g = c_begin + r;
            s = g / cells;
            const int rem = g % cells;
            const int t = rem / (mg * mg), x = rem / mg % mg, y = rem % mg;
            xc = source_cell(a.g, a.seams, t, position_of(a.g, x, tx, px), position_of(a.g, y, ty, py));
            yc = transposed ? (t * a.g.n_out + 2 * x + px) * a.g.n_out + 2 * y + py : rem;
        }
        xcell[r] = xc, ycell[r] = yc, smp[r] = s;
    }

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    for (int c0 = 0; c0 < len; c0 += kRows) {
        __syncthreads();
        for (int e = tid; e < kRows * 64; e += kBlock) {
            const int kk = e >> 6, i = e & 63;
            const int r = c0 + kk, ci = ci0 + i;
            float v = 0.f;
            if (r < len && ci < a.c_in && xcell[r] >= 0) v = a.x[(int64_t)smp[r] * a.x_ss + (int64_t)xcell[r] * a.x_ld + ci];
            if (CTX && r < len && ci >= a.c_in && ci - a.c_in < a.c_ctx && xcell[r] >= 0) {
                const int j = ci - a.c_in;
                v = j < a.c_cell ? a.ctx_cell[(int64_t)xcell[r] * a.c_cell + j] : a.ctx_uni[j - a.c_cell];
            }
            ap[kk * kMP + i] = v;
            const int nn = n0 + i;
            float u = 0.f;
            if (r < len && nn < a.c_out) u = a.dy[(int64_t)smp[r] * a.dy_ss + (int64_t)ycell[r] * a.dy_ld + nn];
            bp[kk * kMP + i] = u;
        }
        __syncthreads();
#pragma unroll
        for (int kp = 0; kp < kRows / 2; ++kp) {
            const int kr = 2 * kp + hh;
            const float av = ap[kr * kMP + wm * 32 + l31];
            const float bv = bp[kr * kMP + wn * 32 + l31];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
    }

    // epilogue: D[row][col], col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int nn = n0 + wn * 32 + l31;
    if (nn >= a.c_out) return;
    float *ws = a.ws + (int64_t)blockIdx.z * partial_floats(a.blocks, a.c_in, a.c_ctx, a.c_out);
    float *wc = ws + (int64_t)a.blocks * a.c_in * a.c_out;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ci = ci0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (ci < a.c_in) ws[((int64_t)wblock * a.c_in + ci) * a.c_out + nn] = acc[r];
        if (CTX && ci >= a.c_in && ci - a.c_in < a.c_ctx) wc[((int64_t)wblock * a.c_ctx + ci - a.c_in) * a.c_out + nn] = acc[r];
    }
}

// the chunk's part of db: per channel the sum of dy over the chunk's rows in float64 -- four groups of rows, added in group
// order; a row of the transposed kind is an input-grid cell and stands for the four output cells 2 x + px, 2 y + py
__global__ __launch_bounds__(kBlock) void cyclegan_bias_grad_kernel(const BwdWeightArgs a)
{
    __shared__ double red[4][64];
    const int tid = threadIdx.x, j = tid & 63, grp = tid >> 6;
    const int nn = blockIdx.x * 64 + j;
    const bool transposed = a.g.kind == FV3HIP_CYCLEGAN_CONV_TRANSPOSED;
    const int mg = a.mg, cells = 6 * mg * mg, no = a.g.n_out;
    const int c_begin = blockIdx.y * kChunk;
    const int len = (int64_t)c_begin + kChunk < a.rows ? kChunk : (int)(a.rows - c_begin);
    double sum = 0.0;
    if (nn < a.c_out) {
        for (int r = grp; r < len; r += 4) {
            const int g = c_begin + r;
            const float *dy = a.dy + (int64_t)(g / cells) * a.dy_ss + nn;
            const int rem = g % cells;
            if (transposed) {
                const int t = rem / (mg * mg), x = rem / mg % mg, y = rem % mg;
                for (int p = 0; p < 4; ++p)
                    sum += (double)dy[(int64_t)((t * no + 2 * x + (p >> 1)) * no + 2 * y + (p & 1)) * a.dy_ld];
            } else {
                sum += (double)dy[(int64_t)rem * a.dy_ld];
            }
        }
    }
    red[grp][j] = sum;
    __syncthreads();
    if (grp == 0 && nn < a.c_out) {
        const double tot = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
        float *out = a.ws + (int64_t)blockIdx.y * partial_floats(a.blocks, a.c_in, a.c_ctx, a.c_out) +
                     (int64_t)a.blocks * (a.c_in + a.c_ctx) * a.c_out + 2 * nn;
        out[0] = __int_as_float(__double2hiint(tot));
        out[1] = __int_as_float(__double2loint(tot));
    }
}

// the chunks' partials added in ascending order; db in float64, rounded once
__global__ __launch_bounds__(kBlock) void cyclegan_chunk_sum_kernel(const BwdWeightArgs a)
{
    const int64_t ns = (int64_t)a.blocks * a.c_in * a.c_out, nw = ns + (int64_t)a.blocks * a.c_ctx * a.c_out;
    const int64_t part = partial_floats(a.blocks, a.c_in, a.c_ctx, a.c_out);
    const int64_t total = nw + (a.db ? a.c_out : 0);
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        if (e < nw) {
            float s = a.ws[e];
            for (int z = 1; z < a.n_chunks; ++z) s += a.ws[z * part + e];
            if (e < ns)
                a.dw[e] = s;
            else
                a.dw_ctx[e - ns] = s;
        } else {
            double s = 0.0;
            for (int z = 0; z < a.n_chunks; ++z) {
                const float *w = a.ws + z * part + nw + 2 * (e - nw);
                s += __hiloint2double(__float_as_int(w[0]), __float_as_int(w[1]));
            }
            a.db[e - nw] = (float)s;
        }
    }
}

struct NormArgs {
    const float *dy, *x;     // channel offsets applied
    float *dx;
    int64_t dy_ld, dy_ss, x_ld, x_ss, dx_ld, dx_ss;
    const float *mean, *rstd;   // [sample][6][C]
    const float *bias;          // [6][n][n][C] or null
    float *dbias;               // [6][n][n][C] or null
    float slope;
    int n, C;
    int64_t n_samples;
};

// g = dy * act'(x^ + bias) with the float32 pre-activation exactly as the forward forms it (cyclegan_apply_kernel), so that
// the mask is the forward's; and x^ = (x - mean) * rstd once more in float64 (of the float32 statistics) for the arithmetic
__device__ inline void norm_terms(const NormArgs &a, int64_t s, int64_t st, int64_t cell, int c, double &xh, float &g)
{
    const float v = a.x[s * a.x_ss + cell * a.x_ld + c];
    const float m = a.mean[st * a.C + c], q = a.rstd[st * a.C + c];
    const float xf = (v - m) * q;
    const float p = a.bias ? xf + a.bias[cell * a.C + c] : xf;
    const float d = a.dy[s * a.dy_ss + cell * a.dy_ld + c];
    g = p > 0.f ? d : d * a.slope;
    xh = ((double)v - (double)m) * (double)q;
}

// one (sample, tile) face and 16 channels per block: the face means of g and g x^ in float64 by 16 groups of cells added in
// group order (as cyclegan_stats_kernel), then dx = rstd (g - mean(g) - x^ mean(g x^)) in float64, rounded once: on faces of
// 2 x 2 or 3 x 3 cells the three terms cancel, and float32 steps between them would each cost a rounding of the largest
__global__ __launch_bounds__(kBlock) void cyclegan_norm_bwd_kernel(const NormArgs a)
{
    __shared__ double red[2][16][kStatCh];
    __shared__ double mu[2][kStatCh];
    const int tid = threadIdx.x, cl = tid % kStatCh, grp = tid / kStatCh;
    const int64_t st = blockIdx.x, s = st / 6;
    const int c = blockIdx.y * kStatCh + cl;
    const int cells = a.n * a.n;
    const int64_t cell0 = (st % 6) * (int64_t)cells;
    double s1 = 0.0, s2 = 0.0;
    if (c < a.C) {
        for (int i = grp; i < cells; i += 16) {
            double xh;
            float g;
            norm_terms(a, s, st, cell0 + i, c, xh, g);
            s1 += (double)g;
            s2 += (double)g * xh;
        }
    }
    red[0][grp][cl] = s1;
    red[1][grp][cl] = s2;
    __syncthreads();
    if (grp < 2) {
        double tot = 0.0;
        for (int j = 0; j < 16; ++j) tot += red[grp][j][cl];
        mu[grp][cl] = tot / cells;
    }
    __syncthreads();
    if (c >= a.C) return;
    const double m1 = mu[0][cl], m2 = mu[1][cl], q = (double)a.rstd[st * a.C + c];
    for (int i = grp; i < cells; i += 16) {
        double xh;
        float g;
        norm_terms(a, s, st, cell0 + i, c, xh, g);
        a.dx[s * a.dx_ss + (cell0 + i) * a.dx_ld + c] = (float)(q * (((double)g - m1) - xh * m2));
    }
}

// dbias[cell][c] = sum over the samples of g, in ascending order
__global__ __launch_bounds__(kBlock) void cyclegan_norm_dbias_kernel(const NormArgs a)
{
    const int64_t face = (int64_t)a.n * a.n, total = 6 * face * a.C;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int c = (int)(e % a.C);
        const int64_t cell = e / a.C, t = cell / face;
        float sum = 0.f;
        for (int64_t s = 0; s < a.n_samples; ++s) {
            double xh;
            float g;
            norm_terms(a, s, s * 6 + t, cell, c, xh, g);
            sum = s == 0 ? g : sum + g;
        }
        a.dbias[e] = sum;
    }
}

size_t data_workspace_bytes(int64_t n_samples, const Geom &g, int c_in)
{
    if (!g.cube) return 0;
    const int64_t np = g.n + 2 * g.h;
    return (size_t)n_samples * 6 * (size_t)(np * np) * (size_t)c_in * sizeof(float);
}

size_t weight_workspace_bytes(int64_t n_samples, const Geom &g, int c_in, int c_ctx, int c_out)
{
    const int64_t mg = g.kind == FV3HIP_CYCLEGAN_CONV_TRANSPOSED ? g.n : g.n_out;
    const int64_t chunks = ceil_div(n_samples * 6 * mg * mg, kChunk);
    return (size_t)chunks * (size_t)partial_floats(g.k * g.k, c_in, c_ctx, c_out) * sizeof(float);
}

struct Span {
    const char *what;
    uintptr_t lo, hi;   // lo == 0: absent
};

Span span(const char *what, const float *p, int64_t floats)
{
    return Span{what, (uintptr_t)p, (uintptr_t)p + (uintptr_t)floats * sizeof(float)};
}

// nothing written (spans first_written ...) may overlap what is read or another result
int check_spans(const Span *spans, int count, int first_written)
{
    for (int i = first_written; i < count; ++i)
        for (int k = 0; k < i; ++k)
            FV3HIP_REQUIRE(!spans[i].lo || !spans[k].lo || spans[i].hi <= spans[k].lo || spans[k].hi <= spans[i].lo,
                           "%s and %s overlap", spans[k].what, spans[i].what);
    return FV3HIP_OK;
}

int64_t cube_span(int64_t n_samples, int n, int64_t ld, int64_t ss) { return (n_samples - 1) * ss + 6LL * n * n * ld; }

}  // namespace

extern "C" int fv3hip_cyclegan_train_chunk_cells(void) { return kChunk; }

extern "C" size_t fv3hip_cyclegan_train_backward_data_workspace_bytes(int64_t n_samples, int n, int c_in, int kind, int k, int halo_mode)
{
    Geom g;
    if (n_samples < 1 || n < 1 || n > kLimits.max_n || c_in < 1 || check_geometry(n, kind, k, halo_mode, g)) return 0;
    return data_workspace_bytes(n_samples, g, c_in);
}

extern "C" size_t fv3hip_cyclegan_train_backward_weight_workspace_bytes(int64_t n_samples, int n, int c_in, int c_out, int kind, int k)
{
    Geom g;
    if (n_samples < 1 || n < 1 || n > kLimits.max_n || c_in < 1 || c_out < 1 || check_geometry(n, kind, k, FV3HIP_CYCLEGAN_HALO_CUBE, g))
        return 0;
    return weight_workspace_bytes(n_samples, g, c_in, 0, c_out);
}

extern "C" int fv3hip_cyclegan_train_backward_data(const float *dy, int64_t dy_ld, int64_t dy_off, int64_t dy_sample_stride,
                                                   const float *w, float *dx, int64_t dx_ld, int64_t dx_off, int64_t dx_sample_stride,
                                                   float *workspace, size_t workspace_bytes, int64_t n_samples, int n, int c_in,
                                                   int c_out, int kind, int k, int halo_mode, void *stream)
{
    int rc;
    Geom g;
    if ((rc = check_channels(c_in, c_out))) return rc;
    FV3HIP_REQUIRE(w, "null weights");
    if ((rc = check_cube(n_samples, n, kLimits)) || (rc = check_geometry(n, kind, k, halo_mode, g)) ||
        (rc = check_slice("dy", dy, dy_ld, dy_off, c_out)) || (rc = check_slice("dx", dx, dx_ld, dx_off, c_in)) ||
        (rc = check_stride("dy", &dy_sample_stride, g.n_out, dy_ld)) || (rc = check_stride("dx", &dx_sample_stride, n, dx_ld)) ||
        (rc = check_no_alias(Slice{dy, dy_ld, dy_off, dy_sample_stride, c_out, g.n_out}, Slice{dx, dx_ld, dx_off, dx_sample_stride, c_in, n},
                             n_samples, false)))
        return rc;
    if (n_samples == 0) return FV3HIP_OK;
    const size_t need = data_workspace_bytes(n_samples, g, c_in);
    FV3HIP_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "the padded gradient needs a workspace of %zu bytes, got %zu", need,
                   workspace ? workspace_bytes : (size_t)0);
    const int64_t blocks = (int64_t)g.k * g.k;
    const Span spans[] = {span("dy", dy, cube_span(n_samples, g.n_out, dy_ld, dy_sample_stride)), span("the weights", w, blocks * c_in * c_out),
                          span("dx", dx, cube_span(n_samples, n, dx_ld, dx_sample_stride)),
                          span("the workspace", need ? workspace : nullptr, (int64_t)(need / sizeof(float)))};
    // (dy and dx of one buffer may interleave in channels: check_no_alias has passed them)
    for (int i = 0; i < 3; ++i)
        FV3HIP_REQUIRE(!spans[3].lo || spans[3].hi <= spans[i].lo || spans[i].hi <= spans[3].lo, "%s and the workspace overlap", spans[i].what);
    FV3HIP_REQUIRE(spans[2].hi <= spans[1].lo || spans[1].hi <= spans[2].lo, "the weights and dx overlap");

    BwdDataArgs a;
    memset(&a, 0, sizeof(a));
    a.dy = dy + dy_off;
    a.dy_ld = dy_ld, a.dy_ss = dy_sample_stride;
    a.w = w;
    a.g = g;
    a.C = c_out, a.N = c_in;
    if (g.cube) {
        a.hp = g.h, a.np = n + 2 * g.h;
        a.dst = workspace;
        a.dst_ld = c_in, a.dst_ss = 6LL * a.np * a.np * c_in;
    } else {
        a.hp = 0, a.np = n;
        a.dst = dx + dx_off;
        a.dst_ld = dx_ld, a.dst_ss = dx_sample_stride;
    }
    a.rows = n_samples * 6 * a.np * a.np;
    const int nt = c_in > 32 ? 2 : 1;
    FV3HIP_REQUIRE(ceil_div(c_in, nt * 32) <= 65535 && ceil_div(a.rows, kBM) <= 0x7fffffff, "the grid of %lld cells x %d channels is too large",
                   (long long)a.rows, c_in);
    const dim3 grid((unsigned)ceil_div(a.rows, kBM), (unsigned)ceil_div(c_in, nt * 32));
    const bool vec = c_out % 16 == 0 && dy_ld % 4 == 0 && dy_off % 4 == 0 && dy_sample_stride % 4 == 0 && aligned16(dy);
    const size_t lds = (size_t)blocks * kBM * sizeof(int);
    using Kernel = void (*)(const BwdDataArgs);
    static const Kernel kernels[2][2] = {{cyclegan_bwd_data_kernel<1, false>, cyclegan_bwd_data_kernel<1, true>},
                                         {cyclegan_bwd_data_kernel<2, false>, cyclegan_bwd_data_kernel<2, true>}};
    hipLaunchKernelGGL(kernels[nt - 1][vec], grid, dim3(kBlock), lds, as_stream(stream), a);
    if ((rc = check_launch("cyclegan_bwd_data_kernel"))) return rc;
    if (g.cube) {
        hipLaunchKernelGGL(cyclegan_fold_kernel, dim3(grid_stride_blocks(n_samples * 6 * n * n * c_in)), dim3(kBlock), 0, as_stream(stream),
                           workspace, dx + dx_off, dx_ld, dx_sample_stride, n_samples, n, g.h, c_in, cube_seams());
        return check_launch("cyclegan_fold_kernel");
    }
    return FV3HIP_OK;
}

// both weight-gradient entry points: every argument is checked here, before any launch
static int launch_backward_weight(const float *x, int64_t x_ld, int64_t x_off, int64_t x_sample_stride, const float *dy, int64_t dy_ld,
                                  int64_t dy_off, int64_t dy_sample_stride, const float *ctx_cell, int c_cell, const float *ctx_uniform,
                                  int c_uni, float *dw, float *dw_ctx, float *db, float *workspace, size_t workspace_bytes,
                                  int64_t n_samples, int n, int c_in, int c_out, int kind, int k, int halo_mode, void *stream)
{
    int rc;
    Geom g;
    if ((rc = check_channels(c_in, c_out))) return rc;
    FV3HIP_REQUIRE(dw, "null weight gradient");
    FV3HIP_REQUIRE(c_cell >= 0 && c_uni >= 0 && c_cell <= (1 << 12) && c_uni <= (1 << 12),
                   "c_cell and c_uni must be in [0, 2^12], got %d, %d", c_cell, c_uni);
    FV3HIP_REQUIRE((ctx_cell != nullptr) == (c_cell > 0), "ctx_cell is %s with c_cell = %d", ctx_cell ? "given" : "null", c_cell);
    FV3HIP_REQUIRE((ctx_uniform != nullptr) == (c_uni > 0), "ctx_uniform is %s with c_uni = %d", ctx_uniform ? "given" : "null", c_uni);
    const int c_ctx = c_cell + c_uni;
    FV3HIP_REQUIRE((dw_ctx != nullptr) == (c_ctx > 0), "dw_ctx is %s with %d context channels", dw_ctx ? "given" : "null", c_ctx);
    if ((rc = check_cube(n_samples, n, kLimits)) || (rc = check_geometry(n, kind, k, halo_mode, g))) return rc;
    if (c_ctx > 0 && kind != FV3HIP_CYCLEGAN_CONV_REGULAR)
        return fail(FV3HIP_EUNSUPPORTED, "context channels are built for the regular convolution, got kind %d", kind);
    if ((rc = check_slice("x", x, x_ld, x_off, c_in)) || (rc = check_slice("dy", dy, dy_ld, dy_off, c_out)) ||
        (rc = check_stride("x", &x_sample_stride, n, x_ld)) || (rc = check_stride("dy", &dy_sample_stride, g.n_out, dy_ld)))
        return rc;
    FV3HIP_REQUIRE(n_samples >= 1, "n_samples must be positive");
    BwdWeightArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x + x_off, a.dy = dy + dy_off;
    a.x_ld = x_ld, a.x_ss = x_sample_stride, a.dy_ld = dy_ld, a.dy_ss = dy_sample_stride;
    a.dw = dw, a.db = db, a.ws = workspace;
    a.ctx_cell = ctx_cell, a.ctx_uni = ctx_uniform, a.dw_ctx = dw_ctx, a.c_cell = c_cell, a.c_ctx = c_ctx;
    a.g = g;
    a.mg = kind == FV3HIP_CYCLEGAN_CONV_TRANSPOSED ? n : g.n_out;
    a.c_in = c_in, a.c_out = c_out, a.blocks = k * k, a.mtiles = (int)ceil_div(c_in + c_ctx, 64);
    a.rows = n_samples * 6 * a.mg * a.mg;
    const int64_t chunks = ceil_div(a.rows, kChunk);
    FV3HIP_REQUIRE(chunks <= 65535, "%lld cells are more than 65535 chunks of %d", (long long)a.rows, kChunk);
    FV3HIP_REQUIRE(ceil_div(c_out, 64) <= 65535 && (int64_t)a.blocks * a.mtiles <= 0x7fffffff, "the grid of %d x %d channels is too large", c_in,
                   c_out);
    a.n_chunks = (int)chunks;
    a.seams = cube_seams();
    const size_t need = weight_workspace_bytes(n_samples, g, c_in, c_ctx, c_out);
    FV3HIP_REQUIRE(workspace && workspace_bytes >= need, "%lld cells need a workspace of %zu bytes, got %zu", (long long)a.rows, need,
                   workspace ? workspace_bytes : (size_t)0);
    const Span spans[] = {span("x", x, cube_span(n_samples, n, x_ld, x_sample_stride)),
                          span("dy", dy, cube_span(n_samples, g.n_out, dy_ld, dy_sample_stride)),
                          span("the cell context", ctx_cell, 6LL * n * n * c_cell), span("the uniform context", ctx_uniform, c_uni),
                          span("the weight gradient", dw, (int64_t)a.blocks * c_in * c_out),
                          span("the context rows' gradient", dw_ctx, (int64_t)a.blocks * c_ctx * c_out), span("db", db, c_out),
                          span("the workspace", workspace, (int64_t)(need / sizeof(float)))};
    if ((rc = check_spans(spans, 8, 4))) return rc;
    const dim3 grid((unsigned)(a.blocks * a.mtiles), (unsigned)ceil_div(c_out, 64), (unsigned)chunks);
    if (c_ctx > 0)
        hipLaunchKernelGGL(cyclegan_bwd_weight_kernel<true>, grid, dim3(kBlock), 0, as_stream(stream), a);
    else
        hipLaunchKernelGGL(cyclegan_bwd_weight_kernel<false>, grid, dim3(kBlock), 0, as_stream(stream), a);
    if ((rc = check_launch(c_ctx > 0 ? "cyclegan_bwd_weight_kernel (context)" : "cyclegan_bwd_weight_kernel"))) return rc;
    if (db) {
        hipLaunchKernelGGL(cyclegan_bias_grad_kernel, dim3((unsigned)ceil_div(c_out, 64), (unsigned)chunks), dim3(kBlock), 0,
                           as_stream(stream), a);
        if ((rc = check_launch("cyclegan_bias_grad_kernel"))) return rc;
    }
    hipLaunchKernelGGL(cyclegan_chunk_sum_kernel, dim3(grid_stride_blocks((int64_t)(a.blocks * (c_in + c_ctx) + 1) * c_out)), dim3(kBlock),
                       0, as_stream(stream), a);
    return check_launch("cyclegan_chunk_sum_kernel");
}

extern "C" int fv3hip_cyclegan_train_backward_weight(const float *x, int64_t x_ld, int64_t x_off, int64_t x_sample_stride, const float *dy,
                                                     int64_t dy_ld, int64_t dy_off, int64_t dy_sample_stride, float *dw, float *db,
                                                     float *workspace, size_t workspace_bytes, int64_t n_samples, int n, int c_in,
                                                     int c_out, int kind, int k, int halo_mode, void *stream)
{
    return launch_backward_weight(x, x_ld, x_off, x_sample_stride, dy, dy_ld, dy_off, dy_sample_stride, nullptr, 0, nullptr, 0, dw, nullptr,
                                  db, workspace, workspace_bytes, n_samples, n, c_in, c_out, kind, k, halo_mode, stream);
}

extern "C" size_t fv3hip_cyclegan_train_backward_weight_context_workspace_bytes(int64_t n_samples, int n, int c_in, int c_cell, int c_uni,
                                                                                int c_out, int k)
{
    Geom g;
    if (n_samples < 1 || n < 1 || n > kLimits.max_n || c_in < 1 || c_out < 1 || c_cell < 0 || c_uni < 0 || c_cell > (1 << 12) ||
        c_uni > (1 << 12) || check_geometry(n, FV3HIP_CYCLEGAN_CONV_REGULAR, k, FV3HIP_CYCLEGAN_HALO_CUBE, g))
        return 0;
    return weight_workspace_bytes(n_samples, g, c_in, c_cell + c_uni, c_out);
}

extern "C" int fv3hip_cyclegan_train_backward_weight_context(const float *x, int64_t x_ld, int64_t x_off, int64_t x_sample_stride,
                                                             const float *dy, int64_t dy_ld, int64_t dy_off, int64_t dy_sample_stride,
                                                             const float *ctx_cell, int c_cell, const float *ctx_uniform, int c_uni,
                                                             float *dw, float *dw_ctx, float *db, float *workspace,
                                                             size_t workspace_bytes, int64_t n_samples, int n, int c_in, int c_out,
                                                             int kind, int k, int halo_mode, void *stream)
{
    return launch_backward_weight(x, x_ld, x_off, x_sample_stride, dy, dy_ld, dy_off, dy_sample_stride, ctx_cell, c_cell, ctx_uniform, c_uni,
                                  dw, dw_ctx, db, workspace, workspace_bytes, n_samples, n, c_in, c_out, kind, k, halo_mode, stream);
}

extern "C" int fv3hip_cyclegan_train_norm_backward(const float *dy, int64_t dy_ld, int64_t dy_off, int64_t dy_sample_stride, const float *x,
                                                   int64_t x_ld, int64_t x_off, int64_t x_sample_stride, const float *mean,
                                                   const float *rstd, const float *bias, float slope, float *dx, int64_t dx_ld,
                                                   int64_t dx_off, int64_t dx_sample_stride, float *dbias, int64_t n_samples, int n, int c,
                                                   void *stream)
{
    FV3HIP_REQUIRE(c >= 1 && c <= (1 << 16), "c must be in [1, 2^16], got %d", c);
    FV3HIP_REQUIRE(mean && rstd, "null statistics");
    FV3HIP_REQUIRE(slope >= 0.f && slope <= 1.f, "the slope of the leaky ReLU must be in [0, 1], got %g", (double)slope);
    int rc;
    if ((rc = check_cube(n_samples, n, kLimits)) || (rc = check_slice("dy", dy, dy_ld, dy_off, c)) ||
        (rc = check_slice("x", x, x_ld, x_off, c)) || (rc = check_slice("dx", dx, dx_ld, dx_off, c)) ||
        (rc = check_stride("dy", &dy_sample_stride, n, dy_ld)) || (rc = check_stride("x", &x_sample_stride, n, x_ld)) ||
        (rc = check_stride("dx", &dx_sample_stride, n, dx_ld)) ||
        (rc = check_no_alias(Slice{dy, dy_ld, dy_off, dy_sample_stride, c, n}, Slice{dx, dx_ld, dx_off, dx_sample_stride, c, n}, n_samples,
                             false)) ||
        (rc = check_no_alias(Slice{x, x_ld, x_off, x_sample_stride, c, n}, Slice{dx, dx_ld, dx_off, dx_sample_stride, c, n}, n_samples,
                             false)))
        return rc;
    if (n_samples == 0) return FV3HIP_OK;
    const int64_t face = 6LL * n * n * c;
    const Span spans[] = {span("dy", dy, cube_span(n_samples, n, dy_ld, dy_sample_stride)),
                          span("x", x, cube_span(n_samples, n, x_ld, x_sample_stride)), span("the mean", mean, n_samples * 6 * c),
                          span("rstd", rstd, n_samples * 6 * c), span("the bias", bias, face), span("the bias gradient", dbias, face)};
    if ((rc = check_spans(spans, 6, 5))) return rc;
    const Span dxs = span("dx", dx, cube_span(n_samples, n, dx_ld, dx_sample_stride));
    for (int i = 2; i < 6; ++i)
        FV3HIP_REQUIRE(!spans[i].lo || spans[i].hi <= dxs.lo || dxs.hi <= spans[i].lo, "%s and dx overlap", spans[i].what);
    NormArgs a;
    memset(&a, 0, sizeof(a));
    a.dy = dy + dy_off, a.x = x + x_off, a.dx = dx + dx_off;
    a.dy_ld = dy_ld, a.dy_ss = dy_sample_stride, a.x_ld = x_ld, a.x_ss = x_sample_stride, a.dx_ld = dx_ld, a.dx_ss = dx_sample_stride;
    a.mean = mean, a.rstd = rstd, a.bias = bias, a.dbias = dbias, a.slope = slope;
    a.n = n, a.C = c, a.n_samples = n_samples;
    const dim3 grid((unsigned)(n_samples * 6), (unsigned)ceil_div(c, kStatCh));
    hipLaunchKernelGGL(cyclegan_norm_bwd_kernel, grid, dim3(kBlock), 0, as_stream(stream), a);
    if ((rc = check_launch("cyclegan_norm_bwd_kernel"))) return rc;
    if (dbias) {
        hipLaunchKernelGGL(cyclegan_norm_dbias_kernel, dim3(grid_stride_blocks(face)), dim3(kBlock), 0, as_stream(stream), a);
        return check_launch("cyclegan_norm_dbias_kernel");
    }
    return FV3HIP_OK;
}

// ---- the window loss of the recurrent generator (recurrent/train_fmr.py: identity on time 0, target on the later times) ----
namespace {

constexpr int kLossPer = 8;   // elements per thread: a block covers kBlock * kLossPer consecutive elements of (window, time, element)

struct LossArgs {
    const float *fake, *real, *dgan;   // dgan (or null) and dfake have fake's strides
    float *dfake;                      // null: the values only
    int64_t fake_ws, fake_ts, real_ws, real_ts;
    int64_t n_times, n_elems, total;   // total = n_windows * n_times * n_elems
    int kind[2];                       // identity, target
    double coef[2];                    // weight / count
    double *partials;                  // [blocks][2]
    double *values;
    int64_t n_blocks;
};

// per element, in float64: the loss term |f - r| or (f - r)^2 and dfake = dgan + coef sign(f - r) or dgan + 2 coef (f - r),
// rounded once.  A thread adds its kLossPer terms in ascending order, the block its 256 threads' sums pairwise in a fixed tree.
__global__ __launch_bounds__(kBlock) void fmr_loss_kernel(const LossArgs a)
{
    __shared__ double red[2][kBlock];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * kLossPer);
    const int64_t per_window = a.n_times * a.n_elems;
    double sum[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kLossPer; ++j) {
        const int64_t e = base + (int64_t)j * kBlock + tid;
        if (e >= a.total) break;
        const int64_t w = e / per_window, rem = e - w * per_window;
        const int64_t t = rem / a.n_elems, i = rem - t * a.n_elems;
        const int64_t fo = w * a.fake_ws + t * a.fake_ts + i;
        const double d = (double)a.fake[fo] - (double)a.real[w * a.real_ws + t * a.real_ts + i];
        const int which = t == 0 ? 0 : 1;
        const bool mse = a.kind[which] == FV3HIP_FMR_LOSS_MSE;
        sum[which] += mse ? d * d : fabs(d);
        if (a.dfake) {
            const double g = a.dgan ? (double)a.dgan[fo] : 0.0;
            const double s = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d;   // (a NaN stays a NaN; sign(0) = 0 as torch's L1Loss)
            a.dfake[fo] = (float)(mse ? g + (2.0 * a.coef[which]) * d : g + a.coef[which] * s);
        }
    }
    red[0][tid] = sum[0];
    red[1][tid] = sum[1];
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if (tid < half) {
            red[0][tid] += red[0][tid + half];
            red[1][tid] += red[1][tid + half];
        }
        __syncthreads();
    }
    if (tid < 2) a.partials[2 * (int64_t)blockIdx.x + tid] = red[tid][0];
}

// one wave: lane l adds the partials of blocks l, l + 64, ... in ascending order, lane 0 the 64 lane sums in ascending order
__global__ __launch_bounds__(64) void fmr_loss_finish_kernel(const LossArgs a)
{
    __shared__ double red[2][64];
    const int lane = threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t b = lane; b < a.n_blocks; b += 64) {
        s0 += a.partials[2 * b];
        s1 += a.partials[2 * b + 1];
    }
    red[0][lane] = s0;
    red[1][lane] = s1;
    __syncthreads();
    if (lane < 2) {
        double tot = 0.0;
        for (int j = 0; j < 64; ++j) tot += red[lane][j];
        a.values[lane] = a.coef[lane] * tot;
    }
}

int64_t loss_blocks(int64_t n_windows, int64_t n_times, int64_t n_elems) { return ceil_div(n_windows * n_times * n_elems, (int64_t)kBlock * kLossPer); }

// the (window, time) grid of `n_elems` contiguous floats each must not fold onto itself: one of the two strides is the inner one
int check_window_strides(const char *what, int64_t ws, int64_t ts, int64_t n_windows, int64_t n_times, int64_t n_elems)
{
    const bool window_major = ts >= n_elems && (n_windows == 1 || ws >= n_times * ts);
    const bool time_major = ws >= n_elems && ts >= n_windows * ws;
    FV3HIP_REQUIRE(window_major || time_major,
                   "%s: strides (window %lld, time %lld) fold %lld windows x %lld times of %lld floats onto themselves", what, (long long)ws,
                   (long long)ts, (long long)n_windows, (long long)n_times, (long long)n_elems);
    return FV3HIP_OK;
}

int64_t window_span(int64_t ws, int64_t ts, int64_t n_windows, int64_t n_times, int64_t n_elems)
{
    return (n_windows - 1) * ws + (n_times - 1) * ts + n_elems;
}

}  // namespace

extern "C" size_t fv3hip_fmr_loss_grad_workspace_bytes(int64_t n_windows, int64_t n_times, int64_t n_elements)
{
    if (n_windows < 1 || n_times < 2 || n_elements < 1 || n_windows > (1 << 20) || n_times > (1 << 20) || n_elements > (1LL << 31)) return 0;
    return (size_t)loss_blocks(n_windows, n_times, n_elements) * 2 * sizeof(double);
}

extern "C" int fv3hip_fmr_loss_grad(const float *fake, int64_t fake_window_stride, int64_t fake_time_stride, const float *real,
                                    int64_t real_window_stride, int64_t real_time_stride, const float *dgan, float *dfake,
                                    int64_t n_windows, int64_t n_times, int64_t n_elements, int identity_kind, double identity_weight,
                                    int target_kind, double target_weight, double *values, double *workspace, size_t workspace_bytes,
                                    void *stream)
{
    FV3HIP_REQUIRE(fake && real && values, "null fake, real or values");
    FV3HIP_REQUIRE(n_windows >= 1 && n_windows <= (1 << 20), "n_windows must be in [1, 2^20], got %lld", (long long)n_windows);
    FV3HIP_REQUIRE(n_times >= 2 && n_times <= (1 << 20),
                   "n_times must be in [2, 2^20] (the target loss is a mean over the times after the first), got %lld", (long long)n_times);
    FV3HIP_REQUIRE(n_elements >= 1 && n_elements <= (1LL << 31), "n_elements must be in [1, 2^31], got %lld", (long long)n_elements);
    const int64_t total = n_windows * n_times * n_elements;
    FV3HIP_REQUIRE(total <= (1LL << 40), "%lld elements are more than 2^40", (long long)total);
    for (int kind : {identity_kind, target_kind})
        FV3HIP_REQUIRE(kind == FV3HIP_FMR_LOSS_MSE || kind == FV3HIP_FMR_LOSS_MAE, "unknown loss kind %d", kind);
    FV3HIP_REQUIRE(std::isfinite(identity_weight) && std::isfinite(target_weight), "the loss weights must be finite");
    FV3HIP_REQUIRE(dfake || !dgan, "dgan is given without dfake");
    int rc;
    if ((rc = check_window_strides("fake", fake_window_stride, fake_time_stride, n_windows, n_times, n_elements)) ||
        (rc = check_window_strides("real", real_window_stride, real_time_stride, n_windows, n_times, n_elements)))
        return rc;
    const int64_t blocks = loss_blocks(n_windows, n_times, n_elements);
    const size_t need = (size_t)blocks * 2 * sizeof(double);
    FV3HIP_REQUIRE(workspace && workspace_bytes >= need, "%lld elements need a workspace of %zu bytes, got %zu", (long long)total, need,
                   workspace ? workspace_bytes : (size_t)0);
    FV3HIP_REQUIRE(blocks <= 0x7fffffff, "%lld elements are too many blocks", (long long)total);
    const int64_t fspan = window_span(fake_window_stride, fake_time_stride, n_windows, n_times, n_elements);
    const Span spans[] = {span("fake", fake, fspan),
                          span("real", real, window_span(real_window_stride, real_time_stride, n_windows, n_times, n_elements)),
                          span("dgan", dgan == dfake ? nullptr : dgan, fspan),   // in place: an element is read by its one writer
                          span("dfake", dfake, fspan), span("the values", (const float *)values, 4),
                          span("the workspace", (const float *)workspace, (int64_t)(need / sizeof(float)))};
    if ((rc = check_spans(spans, 6, 3))) return rc;

    LossArgs a;
    memset(&a, 0, sizeof(a));
    a.fake = fake, a.real = real, a.dgan = dgan, a.dfake = dfake;
    a.fake_ws = fake_window_stride, a.fake_ts = fake_time_stride, a.real_ws = real_window_stride, a.real_ts = real_time_stride;
    a.n_times = n_times, a.n_elems = n_elements, a.total = total;
    a.kind[0] = identity_kind, a.kind[1] = target_kind;
    a.coef[0] = identity_weight / (double)(n_windows * n_elements);
    a.coef[1] = target_weight / (double)(n_windows * (n_times - 1) * n_elements);
    a.partials = workspace, a.values = values, a.n_blocks = blocks;
    hipLaunchKernelGGL(fmr_loss_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), a);
    if ((rc = check_launch("fmr_loss_kernel"))) return rc;
    hipLaunchKernelGGL(fmr_loss_finish_kernel, dim3(1), dim3(64), 0, as_stream(stream), a);
    return check_launch("fmr_loss_finish_kernel");
}
