// Training fv3fit's graph U-Net (the "graph" training function, external/fv3fit/fv3fit/pytorch/graph/train.py:65-119,
// training_loop.py:75-198) on gfx950: the backward kernels of the layers of graph.hip -- DESIGN.md section 24.
//
// Buffers are addressed as in graph.hip: float32, channel-last, (base, ld, channel offset, sample stride).  The five-point graph
// is symmetric with in-degree 5 everywhere, so mean5 is its own adjoint and, with G = dH (.) act'(H) the masked gradient of a
// layer's output,
//     dX       = G W_self^T + mean5(G) W_neigh^T      graph_bwd_data_kernel<NT, false>: the forward GEMM on G with the weights
//                                                     read transposed by the loader, no bias, masked by act' of the layer's input
//     dW_self  = X^T G,  dW_neigh = mean5(X)^T G,     graph_bwd_weight_kernel<false>: one TN GEMM over the cells with M = 32 "self"
//     db       = 1^T G                                rows + 32 "mean" rows of the same input channels (mean5(X) formed in the
//                                                     loader as the forward forms it; X and G are read once) and a ones row
// and for the 2 x 2 / stride 2 transposed convolution
//     dLow[i][j][ci]       = sum_{di,dj,co} dCat[2i+di][2j+dj][co] w[ci][di][dj][co]     graph_bwd_data_kernel<NT, true>
//     dW[ci][di][dj][co]   = sum_{s,t,i,j} low[i][j][ci] dCat[2i+di][2j+dj][co]          graph_bwd_weight_kernel<true>
// All contractions run on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32).  The weight gradients cut the cells of the batch
// (S 6 n^2, in memory order) into chunks of kChunkCells (blockIdx.z); with more than one chunk every chunk writes its partial to
// the caller's workspace and graph_chunk_sum_kernel adds them in ascending order.  Nothing here uses an atomic: every sum has a
// fixed order that depends on the shapes only.
#include <cmath>

#include "common.h"
#include "cube.h"

using namespace fv3hip;

namespace {

constexpr int kTile = 16;     // spatial tile edge of the data gradient: 256 cells per block, as graph_gemm_kernel
constexpr int kBlock = 256;   // four waves
constexpr int kRows = 16;     // K rows per chunk of LDS
constexpr int kChunkCells = 512;   // fv3hip_graph_train_chunk_cells()
constexpr int kMP = 96;       // row stride of a [k][tile index] panel: 32 mod 64 banks keeps the two lane halves apart

constexpr CubeLimits kLimits{10922, "10922", 16384};   // gridDim.y = 6 n_samples

// cell index (t * n + x) * n + y of (x, y) on tile t, where at most one of x, y lies one step outside the tile: then the cell
// of the neighbouring face that the one-cell halo shows there, by the seam rule of cube.h at depth 0
__device__ inline int64_t seam_cell(const CubeSeams &sm, int n, int t, int x, int y)
{
    const bool inx = (unsigned)x < (unsigned)n, iny = (unsigned)y < (unsigned)n;
    if (inx && iny) return ((int64_t)t * n + x) * n + y;
    int side, d, j, tt, xx, yy;
    seam_side(n, x, y, inx, side, d, j);
    seam_cross(sm, n, t, side, d, j, tt, xx, yy);
    return ((int64_t)tt * n + xx) * n + yy;
}

// the value and the forward's mean5 of channel c at cell (t, x, y) of one sample
__device__ inline void load_mean5(const float *src, int64_t ld, const CubeSeams &sm, int n, int t, int x, int y, int c, float &v,
                                  float &m)
{
    v = src[seam_cell(sm, n, t, x, y) * ld + c];
    const float xl = src[seam_cell(sm, n, t, x - 1, y) * ld + c];
    const float xh = src[seam_cell(sm, n, t, x + 1, y) * ld + c];
    const float yl = src[seam_cell(sm, n, t, x, y - 1) * ld + c];
    const float yh = src[seam_cell(sm, n, t, x, y + 1) * ld + c];
    m = ((((v + xl) + xh) + yl) + yh) / 5.0f;
}

// v act'(.) from the stored output p: relu' = [p > 0] (relu'(0) = 0 as in torch; a NaN masks too), tanh' = 1 - p^2
__device__ inline float mask_grad(float v, float p, int act)
{
    if (act == FV3HIP_ACT_RELU) return p > 0.f ? v : 0.f;
    if (act == FV3HIP_ACT_TANH) return v * (1.f - p * p);
    return v;
}

struct BwdDataArgs {
    const float *g;          // SAGE: dH on n cells per edge;  UP: dCat on 2 n.  Channel offsets applied
    float *dst;              // dX / dLow on n
    const float *p;          // the post-activation behind dst, or null
    int64_t g_ld, g_ss, dst_ld, dst_ss, p_ld, p_ss;
    const float *w0;         // SAGE: W_self [N][C];  UP: w [N][C] with C = 4 c_out
    const float *w1;         // SAGE: W_neigh [N][C]
    int n, C, N, c_out, act, accumulate, tiles_y;   // C: the contraction (the layer's outputs), N: the layer's inputs
    CubeSeams seams;
};

template <int NT, bool UP>
__global__ __launch_bounds__(kBlock) void graph_bwd_data_kernel(const BwdDataArgs a)
{
    constexpr int CK = UP ? kRows : kRows / 2;   // contraction channels per chunk
    constexpr int AP = 288;
    constexpr int NG = NT * 32;
    constexpr int NGP = NT == 2 ? 96 : 32;
    __shared__ float al[kRows * AP];
    __shared__ float wl[kRows * NGP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (blockIdx.x / a.tiles_y) * kTile, y0 = (blockIdx.x % a.tiles_y) * kTile;
    const int s = blockIdx.y / 6, t = blockIdx.y % 6;
    const int n0 = blockIdx.z * NG;
    const int hh = lane >> 5, l31 = lane & 31;
    const float *g = a.g + (int64_t)s * a.g_ss;

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
                if (UP) {
                    const int dij = c / a.c_out, co = c % a.c_out, n2 = 2 * a.n;
                    v = g[(((int64_t)t * n2 + 2 * gx + (dij >> 1)) * n2 + 2 * gy + (dij & 1)) * a.g_ld + co];
                } else {
                    load_mean5(g, a.g_ld, a.seams, a.n, t, gx, gy, c, v, m);
                }
            }
            al[cc * AP + pix] = v;
            if (!UP) al[(CK + cc) * AP + pix] = m;
        }
        // the weights transposed: K row r, column j is w[n0 + j][c0 + r]; r runs fastest so that the reads are contiguous
        for (int e = tid; e < kRows * NG; e += kBlock) {
            const int r = e % kRows, j = e / kRows;
            const int c = c0 + (UP ? r : r % CK), nn = n0 + j;
            const float *w = (UP || r < CK) ? a.w0 : a.w1;
            wl[r * NGP + j] = (c < a.C && nn < a.N) ? w[(int64_t)nn * a.C + c] : 0.f;
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
    const float *p = a.p ? a.p + (int64_t)s * a.p_ss : nullptr;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int nn = n0 + nt * 32 + l31;
            if (nn >= a.N) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                const int gx = x0 + (2 * wave + mi) * 2 + (row >> 4), gy = y0 + (row & 15);
                if (gx >= a.n || gy >= a.n) continue;
                const int64_t cell = ((int64_t)t * a.n + gx) * a.n + gy;
                float v = acc[mi][nt][r];
                if (p) v = mask_grad(v, p[cell * a.p_ld + nn], a.act);
                if (a.accumulate) v = dst[cell * a.dst_ld + nn] + v;
                dst[cell * a.dst_ld + nn] = v;
            }
        }
    }
}

struct BwdWeightArgs {
    const float *x;          // SAGE: the layer's input X on n;  UP: low on n.  Channel offsets applied
    const float *g;          // SAGE: G on n;  UP: dCat on 2 n
    int64_t x_ld, x_ss, g_ld, g_ss;
    float *dw0, *dw1, *db;   // SAGE: dW_self, dW_neigh [c_in][N];  UP: dW [c_in][N] (dw1 unused)
    float *ws;               // [chunk][rows][N]
    int64_t cells;           // S 6 n^2
    int n, c_in, c_out, N, n_chunks, accumulate;   // N = c_out (SAGE) or 4 c_out (UP)
    CubeSeams seams;
};

// rows of a partial: SAGE c_in self rows, c_in mean rows, the ones row;  UP c_in rows, the ones row
template <bool UP>
__host__ __device__ inline int partial_rows(int c_in)
{
    return UP ? c_in + 1 : 2 * c_in + 1;
}

template <bool UP>
__global__ __launch_bounds__(kBlock) void graph_bwd_weight_kernel(const BwdWeightArgs a)
{
    constexpr int CT = UP ? 64 : 32;   // input channels per block: UP 64 rows, SAGE 32 self rows + 32 mean rows
    __shared__ float ap[kRows * kMP];
    __shared__ float bp[kRows * kMP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, l31 = lane & 31;
    const int wm = wave & 1, wn = wave >> 1;
    const int ci0 = blockIdx.x * CT, n0 = blockIdx.y * 64;
    const int n = a.n;
    // (at most 65535 chunks: a cell number fits 32 bits, whose division is the cheap one)
    const int face = n * n, cube = 6 * face;
    const int c_begin = blockIdx.z * kChunkCells;
    const int c_end = c_begin + kChunkCells < (int)a.cells ? c_begin + kChunkCells : (int)a.cells;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    for (int c0 = c_begin; c0 < c_end; c0 += kRows) {
        __syncthreads();
        for (int e = tid; e < kRows * CT; e += kBlock) {
            const int kk = e / CT, i = e % CT;
            const int cell = c0 + kk;
            const int ci = ci0 + i;
            float v = 0.f, m = 0.f;
            if (cell < c_end && ci <= a.c_in) {
                if (ci == a.c_in) {
                    v = 1.f;   // the ones row: db
                } else {
                    const int s = cell / cube, in_cube = cell % cube;
                    const float *x = a.x + (int64_t)s * a.x_ss;
                    if (UP) {
                        v = x[(int64_t)in_cube * a.x_ld + ci];
                    } else {
                        const int t = in_cube / face, xy = in_cube % face;
                        load_mean5(x, a.x_ld, a.seams, n, t, xy / n, xy % n, ci, v, m);
                    }
                }
            }
            ap[kk * kMP + i] = v;
            if (!UP) ap[kk * kMP + 32 + i] = m;
        }
        for (int e = tid; e < kRows * 64; e += kBlock) {
            const int kk = e >> 6, j = e & 63;
            const int cell = c0 + kk;
            const int nn = n0 + j;
            float v = 0.f;
            if (cell < c_end && nn < a.N) {
                const int s = cell / cube, in_cube = cell % cube;
                const float *g = a.g + (int64_t)s * a.g_ss;
                if (UP) {
                    const int dij = nn / a.c_out, co = nn % a.c_out, n2 = 2 * n;
                    const int t = in_cube / face, xy = in_cube % face;
                    v = g[(((int64_t)t * n2 + 2 * (xy / n) + (dij >> 1)) * n2 + 2 * (xy % n) + (dij & 1)) * a.g_ld + co];
                } else {
                    v = g[(int64_t)in_cube * a.g_ld + nn];
                }
            }
            bp[kk * kMP + j] = v;
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
    if (nn >= a.N) return;
    const int rows = partial_rows<UP>(a.c_in);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        const int ci = ci0 + (UP ? i : i & 31);
        if (ci > a.c_in) continue;
        int row;   // of the partial
        if (ci == a.c_in) {
            if (!UP && i >= 32) continue;   // (the mean of the ones row is not a result)
            row = rows - 1;
        } else {
            row = (!UP && i >= 32) ? a.c_in + ci : ci;
        }
        const float v = acc[r];
        if (UP || a.n_chunks > 1) {
            a.ws[((int64_t)blockIdx.z * rows + row) * a.N + nn] = v;
            continue;
        }
        float *out = row < a.c_in ? a.dw0 + (int64_t)row * a.N + nn
                     : row < 2 * a.c_in ? a.dw1 + (int64_t)(row - a.c_in) * a.N + nn
                                        : (a.db ? a.db + nn : nullptr);
        if (out) *out = a.accumulate ? *out + v : v;
    }
}

// the chunks' partials [chunk][rows][N] added in ascending order; UP: db[co] = the ones row's four columns (di, dj), in order
template <bool UP>
__global__ __launch_bounds__(kBlock) void graph_chunk_sum_kernel(const BwdWeightArgs a)
{
    const int rows = partial_rows<UP>(a.c_in);
    const int64_t total = (int64_t)rows * a.N;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int row = (int)(e / a.N), nn = (int)(e % a.N);
        float *out;
        float s;
        if (row == rows - 1) {
            if (!a.db || nn >= a.c_out) continue;
            out = a.db + nn;
            s = 0.f;
            for (int d = 0; d < (UP ? 4 : 1); ++d) {
                float col = a.ws[e + d * a.c_out];
                for (int z = 1; z < a.n_chunks; ++z) col += a.ws[z * total + e + d * a.c_out];
                s = d == 0 ? col : s + col;
            }
        } else {
            out = row < a.c_in ? a.dw0 + e : a.dw1 + (e - (int64_t)a.c_in * a.N);
            s = a.ws[e];
            for (int z = 1; z < a.n_chunks; ++z) s += a.ws[z * total + e];
        }
        *out = a.accumulate ? *out + s : s;
    }
}

// dst = (dst + 0.25f dPool[x / 2][y / 2]) act'(P), in place
__global__ __launch_bounds__(kBlock) void graph_pool2_bwd_kernel(const float *dpool, int64_t dp_ld, int64_t dp_ss, const float *p,
                                                                 int64_t p_ld, int64_t p_ss, float *dst, int64_t dst_ld,
                                                                 int64_t dst_ss, int64_t n_samples, int n, int c, int act)
{
    const int m = n / 2;
    const int64_t total = n_samples * 6 * n * n * c;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int ch = (int)(e % c);
        int64_t r = e / c;
        const int y = (int)(r % n);
        r /= n;
        const int x = (int)(r % n);
        r /= n;
        const int t = (int)(r % 6);
        const int64_t s = r / 6;
        const int64_t cell = ((int64_t)t * n + x) * n + y;
        float *d = dst + s * dst_ss + cell * dst_ld + ch;
        float v = *d + 0.25f * dpool[s * dp_ss + (((int64_t)t * m + x / 2) * m + y / 2) * dp_ld + ch];
        if (p) v = mask_grad(v, p[s * p_ss + cell * p_ld + ch], act);
        *d = v;
    }
}

int check_act(int act)
{
    if (act != FV3HIP_ACT_LINEAR && act != FV3HIP_ACT_RELU && act != FV3HIP_ACT_TANH)
        return fail(FV3HIP_EUNSUPPORTED, "activation code %d: FV3HIP_ACT_LINEAR, _RELU and _TANH are built", act);
    return FV3HIP_OK;
}

int check_channels(int c_in, int c_out)
{
    FV3HIP_REQUIRE(c_in >= 1 && c_out >= 1 && c_in <= (1 << 18) && c_out <= (1 << 18), "c_in and c_out must be in [1, 2^18], got %d, %d",
                   c_in, c_out);
    return FV3HIP_OK;
}

template <bool UP>
int launch_bwd_data(const BwdDataArgs &a, int64_t n_samples, hipStream_t st)
{
    const int nt = a.N > 32 ? 2 : 1;
    const int tiles = (int)ceil_div(a.n, kTile);
    dim3 grid((unsigned)(tiles * tiles), (unsigned)(n_samples * 6), (unsigned)ceil_div(a.N, nt * 32));
    if (nt == 1)
        hipLaunchKernelGGL((graph_bwd_data_kernel<1, UP>), grid, dim3(kBlock), 0, st, a);
    else
        hipLaunchKernelGGL((graph_bwd_data_kernel<2, UP>), grid, dim3(kBlock), 0, st, a);
    return check_launch("graph_bwd_data_kernel");
}

template <bool UP>
size_t weight_workspace_bytes(int64_t n_samples, int n, int c_in, int c_out)
{
    if (n_samples < 1 || n < 1 || c_in < 1 || c_out < 1) return 0;
    const int64_t chunks = ceil_div(n_samples * 6 * n * n, kChunkCells);
    if (!UP && chunks == 1) return 0;
    return (size_t)chunks * (size_t)partial_rows<UP>(c_in) * (size_t)(UP ? 4 * c_out : c_out) * sizeof(float);
}

struct Span {
    const char *what;
    uintptr_t lo, hi;   // lo == 0: absent
};

Span span(const char *what, const float *p, int64_t floats)
{
    return Span{what, (uintptr_t)p, (uintptr_t)p + (uintptr_t)floats * sizeof(float)};
}

template <bool UP>
int launch_bwd_weight(BwdWeightArgs &a, int64_t n_samples, float *workspace, size_t workspace_bytes, hipStream_t st)
{
    a.cells = n_samples * 6 * a.n * a.n;
    const int64_t chunks = ceil_div(a.cells, kChunkCells);
    FV3HIP_REQUIRE(chunks <= 65535, "%lld cells are more than 65535 chunks of %d", (long long)a.cells, kChunkCells);
    const size_t need = weight_workspace_bytes<UP>(n_samples, a.n, a.c_in, a.c_out);
    FV3HIP_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%lld cells need a workspace of %zu bytes, got %zu",
                   (long long)a.cells, need, workspace ? workspace_bytes : (size_t)0);
    // nothing written may overlap what is read or another result
    const int gn = UP ? 2 * a.n : a.n;
    const Span spans[] = {span("x", a.x, (n_samples - 1) * a.x_ss + 6LL * a.n * a.n * a.x_ld),
                          span("g", a.g, (n_samples - 1) * a.g_ss + 6LL * gn * gn * a.g_ld),
                          span("the weight gradient", a.dw0, (int64_t)a.c_in * a.N),
                          span("the neighbour weight gradient", a.dw1, (int64_t)a.c_in * a.N), span("db", a.db, a.c_out),
                          span("the workspace", need ? workspace : nullptr, (int64_t)(need / sizeof(float)))};
    for (int i = 2; i < 6; ++i)
        for (int k = 0; k < i; ++k)
            FV3HIP_REQUIRE(!spans[i].lo || !spans[k].lo || spans[i].hi <= spans[k].lo || spans[k].hi <= spans[i].lo,
                           "%s and %s overlap", spans[k].what, spans[i].what);
    a.n_chunks = (int)chunks;
    a.ws = workspace;
    a.seams = cube_seams();
    const dim3 grid((unsigned)ceil_div(a.c_in + 1, UP ? 64 : 32), (unsigned)ceil_div(a.N, 64), (unsigned)chunks);
    hipLaunchKernelGGL(graph_bwd_weight_kernel<UP>, grid, dim3(kBlock), 0, st, a);
    int rc;
    if ((rc = check_launch("graph_bwd_weight_kernel"))) return rc;
    if (need) {
        hipLaunchKernelGGL(graph_chunk_sum_kernel<UP>, dim3(grid_stride_blocks((int64_t)partial_rows<UP>(a.c_in) * a.N)), dim3(kBlock),
                           0, st, a);
        return check_launch("graph_chunk_sum_kernel");
    }
    return FV3HIP_OK;
}

}  // namespace

extern "C" int fv3hip_graph_train_chunk_cells(void) { return kChunkCells; }

extern "C" size_t fv3hip_graph_sage_backward_weight_workspace_bytes(int64_t n_samples, int n, int c_in, int c_out)
{
    return weight_workspace_bytes<false>(n_samples, n, c_in, c_out);
}

extern "C" size_t fv3hip_graph_up2_backward_weight_workspace_bytes(int64_t n_samples, int n, int c_in, int c_out)
{
    return weight_workspace_bytes<true>(n_samples, n, c_in, c_out);
}

extern "C" int fv3hip_graph_sage_backward_data(const float *dh, int64_t dh_ld, int64_t dh_off, int64_t dh_sample_stride,
                                               const float *w_self, const float *w_neigh, const float *p, int64_t p_ld, int64_t p_off,
                                               int64_t p_sample_stride, int p_act, float *dst, int64_t dst_ld, int64_t dst_off,
                                               int64_t dst_sample_stride, int accumulate, int64_t n_samples, int n, int c_in,
                                               int c_out, void *stream)
{
    int rc;
    if ((rc = check_channels(c_in, c_out))) return rc;
    FV3HIP_REQUIRE(w_self && w_neigh, "null weights");
    if ((rc = check_act(p_act)) || (rc = check_cube(n_samples, n, kLimits)) || (rc = check_slice("dh", dh, dh_ld, dh_off, c_out)) ||
        (rc = check_slice("dst", dst, dst_ld, dst_off, c_in)) || (rc = check_stride("dh", &dh_sample_stride, n, dh_ld)) ||
        (rc = check_stride("dst", &dst_sample_stride, n, dst_ld)) ||
        (rc = check_no_alias(Slice{dh, dh_ld, dh_off, dh_sample_stride, c_out, n},
                             Slice{dst, dst_ld, dst_off, dst_sample_stride, c_in, n}, n_samples, true)))
        return rc;
    if (p && ((rc = check_slice("p", p, p_ld, p_off, c_in)) || (rc = check_stride("p", &p_sample_stride, n, p_ld)) ||
              (rc = check_no_alias(Slice{p, p_ld, p_off, p_sample_stride, c_in, n},
                                   Slice{dst, dst_ld, dst_off, dst_sample_stride, c_in, n}, n_samples, true))))
        return rc;
    if (n_samples == 0) return FV3HIP_OK;
    BwdDataArgs a;
    memset(&a, 0, sizeof(a));
    a.g = dh + dh_off;
    a.dst = dst + dst_off;
    a.p = p ? p + p_off : nullptr;
    a.g_ld = dh_ld, a.g_ss = dh_sample_stride, a.dst_ld = dst_ld, a.dst_ss = dst_sample_stride, a.p_ld = p_ld, a.p_ss = p_sample_stride;
    a.w0 = w_self, a.w1 = w_neigh;
    a.n = n, a.C = c_out, a.N = c_in, a.c_out = c_out, a.act = p_act, a.accumulate = accumulate ? 1 : 0;
    a.tiles_y = (int)ceil_div(n, kTile);
    a.seams = cube_seams();
    return launch_bwd_data<false>(a, n_samples, as_stream(stream));
}

extern "C" int fv3hip_graph_sage_backward_weight(const float *x, int64_t x_ld, int64_t x_off, int64_t x_sample_stride, const float *g,
                                                 int64_t g_ld, int64_t g_off, int64_t g_sample_stride, float *dw_self, float *dw_neigh,
                                                 float *db, int accumulate, float *workspace, size_t workspace_bytes,
                                                 int64_t n_samples, int n, int c_in, int c_out, void *stream)
{
    int rc;
    if ((rc = check_channels(c_in, c_out))) return rc;
    FV3HIP_REQUIRE(dw_self && dw_neigh, "null weight gradients");
    if ((rc = check_cube(n_samples, n, kLimits)) || (rc = check_slice("x", x, x_ld, x_off, c_in)) ||
        (rc = check_slice("g", g, g_ld, g_off, c_out)) || (rc = check_stride("x", &x_sample_stride, n, x_ld)) ||
        (rc = check_stride("g", &g_sample_stride, n, g_ld)))
        return rc;
    FV3HIP_REQUIRE(n_samples >= 1, "n_samples must be positive");
    BwdWeightArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x + x_off, a.g = g + g_off;
    a.x_ld = x_ld, a.x_ss = x_sample_stride, a.g_ld = g_ld, a.g_ss = g_sample_stride;
    a.dw0 = dw_self, a.dw1 = dw_neigh, a.db = db;
    a.n = n, a.c_in = c_in, a.c_out = a.N = c_out, a.accumulate = accumulate ? 1 : 0;
    return launch_bwd_weight<false>(a, n_samples, workspace, workspace_bytes, as_stream(stream));
}

extern "C" int fv3hip_graph_up2_backward_data(const float *dcat, int64_t dcat_ld, int64_t dcat_off, const float *w, const float *p,
                                              int64_t p_ld, int64_t p_off, int p_act, float *dst, int64_t dst_ld, int64_t dst_off,
                                              int64_t n_samples, int n, int c_in, int c_out, void *stream)
{
    int rc;
    if ((rc = check_channels(c_in, c_out))) return rc;
    FV3HIP_REQUIRE(w, "null weights");
    if ((rc = check_act(p_act)) || (rc = check_cube(n_samples, n, kLimits))) return rc;
    FV3HIP_REQUIRE(n <= 8192, "n must be at most 8192 (the gradient has 2 n cells per edge), got %d", n);
    int64_t g_ss = 0, dst_ss = 0, p_ss = 0;
    if ((rc = check_slice("dcat", dcat, dcat_ld, dcat_off, c_out)) || (rc = check_slice("dst", dst, dst_ld, dst_off, c_in)) ||
        (rc = check_stride("dcat", &g_ss, 2 * n, dcat_ld)) || (rc = check_stride("dst", &dst_ss, n, dst_ld)) ||
        (rc = check_no_alias(Slice{dcat, dcat_ld, dcat_off, g_ss, c_out, 2 * n}, Slice{dst, dst_ld, dst_off, dst_ss, c_in, n},
                             n_samples, true)))
        return rc;
    if (p && ((rc = check_slice("p", p, p_ld, p_off, c_in)) || (rc = check_stride("p", &p_ss, n, p_ld)) ||
              (rc = check_no_alias(Slice{p, p_ld, p_off, p_ss, c_in, n}, Slice{dst, dst_ld, dst_off, dst_ss, c_in, n}, n_samples, true))))
        return rc;
    if (n_samples == 0) return FV3HIP_OK;
    BwdDataArgs a;
    memset(&a, 0, sizeof(a));
    a.g = dcat + dcat_off;
    a.dst = dst + dst_off;
    a.p = p ? p + p_off : nullptr;
    a.g_ld = dcat_ld, a.g_ss = g_ss, a.dst_ld = dst_ld, a.dst_ss = dst_ss, a.p_ld = p_ld, a.p_ss = p_ss;
    a.w0 = w;
    a.n = n, a.C = 4 * c_out, a.N = c_in, a.c_out = c_out, a.act = p_act;
    a.tiles_y = (int)ceil_div(n, kTile);
    a.seams = cube_seams();
    return launch_bwd_data<true>(a, n_samples, as_stream(stream));
}

extern "C" int fv3hip_graph_up2_backward_weight(const float *low, int64_t low_ld, int64_t low_off, const float *dcat, int64_t dcat_ld,
                                                int64_t dcat_off, float *dw, float *db, int accumulate, float *workspace,
                                                size_t workspace_bytes, int64_t n_samples, int n, int c_in, int c_out, void *stream)
{
    int rc;
    if ((rc = check_channels(c_in, c_out))) return rc;
    FV3HIP_REQUIRE(dw, "null weight gradient");
    if ((rc = check_cube(n_samples, n, kLimits))) return rc;
    FV3HIP_REQUIRE(n <= 8192, "n must be at most 8192 (the gradient has 2 n cells per edge), got %d", n);
    int64_t x_ss = 0, g_ss = 0;
    if ((rc = check_slice("low", low, low_ld, low_off, c_in)) || (rc = check_slice("dcat", dcat, dcat_ld, dcat_off, c_out)) ||
        (rc = check_stride("low", &x_ss, n, low_ld)) || (rc = check_stride("dcat", &g_ss, 2 * n, dcat_ld)))
        return rc;
    FV3HIP_REQUIRE(n_samples >= 1, "n_samples must be positive");
    BwdWeightArgs a;
    memset(&a, 0, sizeof(a));
    a.x = low + low_off, a.g = dcat + dcat_off;
    a.x_ld = low_ld, a.x_ss = x_ss, a.g_ld = dcat_ld, a.g_ss = g_ss;
    a.dw0 = dw, a.db = db;
    a.n = n, a.c_in = c_in, a.c_out = c_out, a.N = 4 * c_out, a.accumulate = accumulate ? 1 : 0;
    return launch_bwd_weight<true>(a, n_samples, workspace, workspace_bytes, as_stream(stream));
}

extern "C" int fv3hip_graph_pool2_backward(const float *dpool, int64_t dpool_ld, int64_t dpool_off, const float *p, int64_t p_ld,
                                           int64_t p_off, int p_act, float *dst, int64_t dst_ld, int64_t dst_off, int64_t n_samples,
                                           int n, int c, void *stream)
{
    FV3HIP_REQUIRE(c >= 1 && c <= (1 << 20), "c must be in [1, 2^20], got %d", c);
    int rc;
    if ((rc = check_act(p_act)) || (rc = check_cube(n_samples, n, kLimits))) return rc;
    FV3HIP_REQUIRE(n % 2 == 0, "n must be even to pool 2 x 2, got %d", n);
    int64_t dp_ss = 0, dst_ss = 0, p_ss = 0;
    if ((rc = check_slice("dpool", dpool, dpool_ld, dpool_off, c)) || (rc = check_slice("dst", dst, dst_ld, dst_off, c)) ||
        (rc = check_stride("dpool", &dp_ss, n / 2, dpool_ld)) || (rc = check_stride("dst", &dst_ss, n, dst_ld)) ||
        (rc = check_no_alias(Slice{dpool, dpool_ld, dpool_off, dp_ss, c, n / 2}, Slice{dst, dst_ld, dst_off, dst_ss, c, n}, n_samples,
                             true)))
        return rc;
    if (p && ((rc = check_slice("p", p, p_ld, p_off, c)) || (rc = check_stride("p", &p_ss, n, p_ld)) ||
              (rc = check_no_alias(Slice{p, p_ld, p_off, p_ss, c, n}, Slice{dst, dst_ld, dst_off, dst_ss, c, n}, n_samples, true))))
        return rc;
    if (n_samples == 0) return FV3HIP_OK;
    const int64_t total = n_samples * 6 * n * n * c;
    hipLaunchKernelGGL(graph_pool2_bwd_kernel, dim3(grid_stride_blocks(total)), dim3(kBlock), 0, as_stream(stream), dpool + dpool_off,
                       dpool_ld, dp_ss, p ? p + p_off : nullptr, p_ld, p_ss, dst + dst_off, dst_ld, dst_ss, n_samples, n, c, p_act);
    return check_launch("graph_pool2_bwd_kernel");
}
