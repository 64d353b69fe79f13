// Training the dense column network (fv3fit's "dense" training function, external/fv3fit/fv3fit/keras/_models/dense.py:165-310)
// and its Jacobian on gfx950 -- DESIGN.md section 21.
//
// Activations are float32, row-major [row][feature] with a leading dimension; weights are [in][out] (Keras Dense, h = x W + b).
// train_gemm_kernel<MODE> is one 64 x 64 block tile on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32, four waves, one 32 x 32
// accumulator each, the contraction walked in chunks of 16 through LDS as graph_gemm_kernel does) in three orientations:
//     NN  forward          H[n][o]  = act(sum_k A[row(n)][k] W[k][o] + b[o])
//     NT  backward data    dA[n][k] = (sum_o dH[n][o] W[k][o]) where P[n * p_stride][k] > 0, else 0
//     TN  backward weight  dW[k][o] = sum_n A[row(n)][k] dH[n][o];  db[o] = sum_n dH[n][o]  (the row k = K of a ones column)
// row(n) = idx[n] where a row table is given: the minibatch is read straight from the resident training set.  The TN form
// splits the batch into chunks of kChunkRows rows (blockIdx.z); with more than one chunk every chunk writes its partial
// [K + 1][O] to the workspace and train_chunk_sum_kernel adds them in ascending order.  Nothing here uses an atomic: every
// result is a fixed-order sum that depends on the shapes only.
#include <cmath>

#include "common.h"

using namespace fv3hip;

namespace {

constexpr int kBlock = 256;
constexpr int kBM = 64, kBN = 64, kBK = 16, kBKLog2 = 4;
constexpr int kFill = kBM * kBK / kBlock;   // panel elements per thread and chunk
constexpr int kChunkRows = 512;       // fv3hip_train_chunk_rows()
constexpr int kLossBlocks = 1024;     // most blocks of the two loss kernels = doubles of their workspace
constexpr int kKP = kBK + 1;          // row stride of a panel stored [tile index][k]: odd, so that 32 tile indices hit 32 banks
constexpr int kMP = 96;               // row stride of a panel stored [k][tile index]: 32 mod 64 banks keeps the two lane halves apart
constexpr int kPanel = kBK * kMP;     // floats per panel (>= 64 * kKP)

enum { NN = 0, NT = 1, TN = 2 };


struct TrainGemmArgs {
    const float *a;          // NN, TN: activations [rows][lda];  NT: dH [n][lda]
    const int64_t *idx;      // NN, TN: row table or null
    int64_t lda, a_rows;
    const float *b;          // NN, NT: W [k][ldb];  TN: dH [n][ldb]
    int64_t ldb;
    float *c;                // NN: H;  NT: dA;  TN: dW, or the workspace when n_chunks > 1
    int64_t ldc;
    const float *bias;       // NN
    float *db;               // TN
    const float *p;          // NT: post-ReLU activations or null
    int64_t ldp;
    int p_stride;
    int64_t n;               // batch rows
    int k, o;                // in and out features
    int act, n_chunks;
};

// panel element (kk, i): kk = index along the contraction within the chunk, i = index within the 64-wide tile
template <bool KFAST>
__device__ __forceinline__ int panel_at(int kk, int i)
{
    return KFAST ? i * kKP + kk : kk * kMP + i;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void train_gemm_kernel(const TrainGemmArgs g)
{
    // which operand is contiguous along the contraction in memory: its panel is filled and stored with k fastest
    constexpr bool AK = MODE != TN, BK = MODE == NT;
    __shared__ float ap[kPanel];
    __shared__ float bp[kPanel];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hh = lane >> 5, l31 = lane & 31;
    const int wm = wave & 1, wn = wave >> 1;
    const int64_t M = MODE == TN ? g.k + 1 : g.n;
    const int64_t N = MODE == NT ? g.k : g.o;
    const int64_t m0 = (int64_t)blockIdx.x * kBM, n0 = (int64_t)blockIdx.y * kBN;
    // the contraction range of this block
    int64_t c_begin = 0, c_end = MODE == NN ? g.k : MODE == NT ? g.o : g.n;
    if (MODE == TN) {
        c_begin = (int64_t)blockIdx.z * kChunkRows;
        c_end = c_begin + kChunkRows < g.n ? c_begin + kChunkRows : g.n;
    }

    // NN: the kFill rows of A this thread fills, looked up once; a row outside the table reads as zeros
    int64_t arow[kFill];
    if (MODE == NN) {
#pragma unroll
        for (int it = 0; it < kFill; ++it) {
            const int64_t m = m0 + (tid >> kBKLog2) + (kBlock >> kBKLog2) * it;
            int64_t r = -1;
            if (m < M) r = g.idx ? g.idx[m] : m;
            arow[it] = (r >= 0 && r < g.a_rows) ? r : -1;
        }
    }

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    for (int64_t c0 = c_begin; c0 < c_end; c0 += kBK) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kFill; ++it) {
            const int e = tid + kBlock * it;
            {   // A panel
                const int kk = AK ? e & (kBK - 1) : e >> 6, i = AK ? e >> kBKLog2 : e & 63;
                const int64_t c = c0 + kk, m = m0 + i;
                float v = 0.f;
                if (c < c_end && m < M) {
                    if (MODE == NN) {
                        if (arow[it] >= 0) v = g.a[arow[it] * g.lda + c];
                    } else if (MODE == NT) {
                        v = g.a[m * g.lda + c];
                    } else if (m == g.k) {
                        v = 1.f;
                    } else {
                        const int64_t r = g.idx ? g.idx[c] : c;
                        if (r >= 0 && r < g.a_rows) v = g.a[r * g.lda + m];
                    }
                }
                ap[panel_at<AK>(kk, i)] = v;
            }
            {   // B panel
                const int kk = BK ? e & (kBK - 1) : e >> 6, j = BK ? e >> kBKLog2 : e & 63;
                const int64_t c = c0 + kk, nn = n0 + j;
                float v = 0.f;
                if (c < c_end && nn < N) v = MODE == NT ? g.b[nn * g.ldb + c] : g.b[c * g.ldb + nn];
                bp[panel_at<BK>(kk, j)] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kp = 0; kp < kBK / 2; ++kp) {
            const int kr = 2 * kp + hh;
            const float av = ap[panel_at<AK>(kr, wm * 32 + l31)];
            const float bv = bp[panel_at<BK>(kr, wn * 32 + l31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
    }

    // epilogue: D[row][col], col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int64_t nn = n0 + wn * 32 + l31;
    if (nn >= N) return;
    const float bias = (MODE == NN && g.bias) ? g.bias[nn] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (m >= M) continue;
        float v = acc[r];
        if (MODE == NN) {
            v += bias;
            if (g.act == FV3HIP_ACT_RELU) v = v < 0.f ? 0.f : v;   // (a NaN stays a NaN, as in torch's relu)
            g.c[m * g.ldc + nn] = v;
        } else if (MODE == NT) {
            if (g.p && !(g.p[m * g.p_stride * g.ldp + nn] > 0.f)) v = 0.f;   // relu'(0) = 0, as in torch
            g.c[m * g.ldc + nn] = v;
        } else if (g.n_chunks > 1) {
            g.c[((int64_t)blockIdx.z * M + m) * N + nn] = v;
        } else if (m == g.k) {
            g.db[nn] = v;
        } else {
            g.c[m * g.ldc + nn] = v;
        }
    }
}

// dW[k][o], db[o] = the chunks' partials [chunk][K + 1][O], added in ascending order
__global__ __launch_bounds__(kBlock) void train_chunk_sum_kernel(const float *ws, int n_chunks, int k, int o, float *dw, int64_t lddw,
                                                                  float *db)
{
    const int64_t total = (int64_t)(k + 1) * o;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        float s = ws[e];
        for (int z = 1; z < n_chunks; ++z) s += ws[z * total + e];
        const int64_t m = e / o, nn = e % o;
        if (m == k)
            db[nn] = s;
        else
            dw[m * lddw + nn] = s;
    }
}

struct MseArgs {
    const float *yhat, *scale, *center, *inv_cstd2, *lo, *hi, *keep, *wnorm, *t;
    const int64_t *idx;
    float *dy;
    double *partial;
    int64_t ldy, ldt, lddy, t_rows, n;
    int f;
};

// a block's 256 doubles added pairwise in a fixed tree; the sum is in s[0] afterwards
__device__ __forceinline__ void block_tree_sum(double *s, int tid)
{
    for (int w = kBlock / 2; w >= 1; w >>= 1) {
        __syncthreads();
        if (tid < w) s[tid] += s[tid + w];
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void train_mse_grad_kernel(const MseArgs a)
{
    __shared__ double part[kBlock];
    const int tid = threadIdx.x;
    const int64_t total = a.n * a.f;
    double sum = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + tid; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t row = e / a.f;
        const int j = (int)(e % a.f);
        float grad = 0.f;
        if (a.keep[j] != 0.f) {
            const int64_t r = a.idx ? a.idx[row] : row;
            const float t = (r >= 0 && r < a.t_rows) ? a.t[r * a.ldt + j] : NAN;
            const float p = a.yhat[row * a.ldy + j] * a.scale[j] + a.center[j];
            const float lo = a.lo[j], hi = a.hi[j];
            const float pc = p < lo ? lo : (p > hi ? hi : p);
            const float d = pc - t;
            if (p >= lo && p <= hi) grad = 2.f * d * a.inv_cstd2[j] * a.scale[j] * a.wnorm[j];   // torch.clamp's gradient: bounds inclusive
            sum += (double)d * (double)d * (double)a.inv_cstd2[j] * (double)a.wnorm[j];
        }
        a.dy[row * a.lddy + j] = grad;
    }
    part[tid] = sum;
    block_tree_sum(part, tid);
    if (tid == 0) a.partial[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(kBlock) void train_loss_finish_kernel(const double *partial, int n_partials, double *loss)
{
    __shared__ double part[kBlock];
    const int tid = threadIdx.x;
    double sum = 0.0;
    for (int i = tid; i < n_partials; i += kBlock) sum += partial[i];
    part[tid] = sum;
    block_tree_sum(part, tid);
    if (tid == 0) loss[0] = part[0];
}

// The loss behind the closure of the precipitative model (fv3fit's "precipitative" training function, precipitative.py:181-279;
// DESIGN.md section 25) and its gradient with respect to the raw output yhat = [ t (nz) | q (nz) | dead (has_dead) | cp (nz) ] of the
// concatenated head layer.  One wave per batch row, four rows per block, lane = level (mod 64): every load and store along the
// features is coalesced.  Pass 1 forms the products cp[k] delp[k] 64 levels at a time, parks them in the wave's strip of LDS and
// every lane adds the strip in ascending order into one float32 accumulator from +0 -- the predictor's order
// (precip_closure_kernel in fit.hip), so the integral is the same bits, and every lane holds it without a broadcast.  Pass 2
// reads the row again (it is in L1 / L2) and writes the gradient, which needs the finished integral in every level of cp.
struct PrecipLossArgs {
    const float *yhat, *scale1, *center1, *scale2, *center2, *inv1, *inv2, *delp, *pp, *t1, *t2, *t3;
    const int64_t *idx;
    float *dy, *dq1, *dq2, *precip;
    double *partial;
    int64_t ldy, ldd, ldt, lddy, rows, n;
    int nz, couple, has_dead;
    float inv3, l1, l2, w12, w3;
};

constexpr int kWave = 64, kRowsPerBlock = kBlock / kWave;

// the gradient of (l1 |x| + l2 x^2) / n, sign(0) = 0 (a NaN stays one)
__device__ __forceinline__ float precip_reg_grad(float x, float l1, float l2, float n)
{
    const float s = x > 0.f ? 1.f : (x < 0.f ? -1.f : x);
    return (l1 * s + 2.f * l2 * x) / n;
}

__global__ __launch_bounds__(kBlock) void train_precip_loss_grad_kernel(const PrecipLossArgs a)
{
    __shared__ double part[kBlock];
    __shared__ float strips[kBlock];
    const float c_heat = (float)(-2.5e6 / 1004.6);  // -LV / CPD, as in fit.hip
    const float c_g = (float)(-1.0 / 9.80665);      // -1 / g
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    float *strip = strips + wave * kWave;
    const int nz = a.nz, cp0 = 2 * nz + a.has_dead;
    const bool reg = a.l1 != 0.f || a.l2 != 0.f;
    const float nf = (float)a.n;
    const double inv_n = 1.0 / (double)a.n;
    double sum = 0.0;
    for (int64_t row0 = (int64_t)blockIdx.x * kRowsPerBlock; row0 < a.n; row0 += (int64_t)gridDim.x * kRowsPerBlock) {
        const int64_t row = row0 + wave;
        const bool live = row < a.n;   // (the block's waves walk the same number of rows: the barriers below are uniform)
        const int64_t r = live ? (a.idx ? a.idx[row] : row) : -1;
        const bool in = r >= 0 && r < a.rows;
        const float *y = a.yhat + (live ? row : 0) * a.ldy;
        const float *d = a.delp + (in ? r : 0) * a.ldd;
        float acc = 0.0f;
        for (int k0 = 0; k0 < nz; k0 += kWave) {
            const int k = k0 + lane;
            float p = 0.f;
            if (live && k < nz) p = (y[cp0 + k] * a.scale2[k] + a.center2[k]) * (in ? d[k] : 0.f);
            __syncthreads();   // the strip's last reader is done
            strip[lane] = p;
            __syncthreads();
            const int m = nz - k0 < kWave ? nz - k0 : kWave;
            for (int j = 0; j < m; ++j) acc = acc + strip[j];
        }
        if (!live) continue;
        const float precip = (in ? a.pp[r] : 0.f) + c_g * acc;
        const float e3 = precip - (in ? a.t3[r] : NAN);
        const float g3 = 2.f * e3 * a.inv3 * a.w3;
        float *dy = a.dy + row * a.lddy;
        if (lane == 0) {
            sum += (double)e3 * (double)e3 * (double)a.inv3 * (double)a.w3;
            if (a.precip) a.precip[row] = precip;
            if (a.has_dead) {
                const float x = y[2 * nz];
                dy[2 * nz] = reg ? precip_reg_grad(x, a.l1, a.l2, nf) : 0.f;
                if (reg) sum += ((double)a.l1 * fabs((double)x) + (double)a.l2 * (double)x * (double)x) * inv_n;
            }
        }
        const float *t1 = a.t1 + (in ? r : 0) * a.ldt, *t2 = a.t2 + (in ? r : 0) * a.ldt;
        for (int k = lane; k < nz; k += kWave) {
            const float th = y[k], qh = y[nz + k], s1 = a.scale1[k], s2 = a.scale2[k], c2 = a.center2[k];
            const float t = th * s1 + a.center1[k], q = qh * s2 + c2, cp = y[cp0 + k] * s2 + c2;
            const float dq1 = a.couple ? t + c_heat * cp : t, dq2 = a.couple ? q + cp : q;
            const float e1 = dq1 - (in ? t1[k] : NAN), e2 = dq2 - (in ? t2[k] : NAN);
            const float inv1 = a.inv1[k], inv2 = a.inv2[k];
            const float g1 = 2.f * e1 * inv1 * a.w12, g2 = 2.f * e2 * inv2 * a.w12;
            float dt = g1 * s1, dq = g2 * s2;
            if (reg) {
                dt = dt + precip_reg_grad(th, a.l1, a.l2, nf);
                dq = dq + precip_reg_grad(qh, a.l1, a.l2, nf);
                sum += ((double)a.l1 * (fabs((double)th) + fabs((double)qh)) +
                        (double)a.l2 * ((double)th * (double)th + (double)qh * (double)qh)) * inv_n;
            }
            dy[k] = dt;
            dy[nz + k] = dq;
            dy[cp0 + k] = ((a.couple ? c_heat * g1 + g2 : 0.f) + (c_g * (in ? d[k] : 0.f)) * g3) * s2;
            sum += (double)e1 * (double)e1 * (double)inv1 * (double)a.w12 + (double)e2 * (double)e2 * (double)inv2 * (double)a.w12;
            if (a.dq1) a.dq1[row * nz + k] = dq1;
            if (a.dq2) a.dq2[row * nz + k] = dq2;
        }
    }
    part[tid] = sum;
    block_tree_sum(part, tid);
    if (tid == 0) a.partial[blockIdx.x] = part[0];
}

// The multi-variable loss of the microphysics emulators (fv3fit's "transformed" training function: emulation/losses.py:33-146
// CustomLoss / _MultiVariableLoss) and its gradient with respect to the raw output of the concatenated
// head layer.  Every head owns a run of blocks (block0[h] .. block0[h + 1]), so a block works on one head and its two partials
// belong to that head's two terms.  An MSE head is walked one (network row, column) per thread, columns fastest (dense heads:
// coalesced along the row); the thread evaluates the direct and the after term, so a dY element has one writer.  A
// cross-entropy point is one thread, which reads its C logits three times (maximum, sum, gradient: the second and third
// reads hit L1) rather than holding them in an array, which would live in scratch.
constexpr int kEmuHeads = FV3HIP_EMULATOR_MAX_HEADS, kEmuSlots = 2 * kEmuHeads;
constexpr int kEmuFinishThreads = 64;   // one wave: a thread per slot
constexpr int kEmuBlocksPerHead = 64;   // most blocks of one head; workspace = kEmuHeads * kEmuBlocksPerHead * 2 doubles

struct EmuLossArgs {
    fv3hip_emulator_head_t head[kEmuHeads];
    float wgrad_d[kEmuHeads], wgrad_a[kEmuHeads];
    int block0[kEmuHeads + 1];
    int n_heads, levels;
    const float *yhat;
    const int64_t *idx;
    float *dy;
    double *partial;
    int64_t ldy, lddy, rows, n;
};

__global__ __launch_bounds__(kBlock) void train_emulator_loss_grad_kernel(const EmuLossArgs a)
{
    __shared__ double part[kBlock];
    const int tid = threadIdx.x;
    int h = 0;
    while (h + 1 < a.n_heads && (int)blockIdx.x >= a.block0[h + 1]) ++h;
    const fv3hip_emulator_head_t &hd = a.head[h];
    const int block = (int)blockIdx.x - a.block0[h], blocks = a.block0[h + 1] - a.block0[h];
    const int L = a.levels, C = hd.ncol;
    const float wd = a.wgrad_d[h], wa = a.wgrad_a[h];
    double sum_d = 0.0, sum_a = 0.0;
    if (hd.kind == FV3HIP_EMULATOR_HEAD_XENT) {
        const int64_t total = a.n * L;
        for (int64_t m = (int64_t)block * kBlock + tid; m < total; m += (int64_t)blocks * kBlock) {
            const int64_t b = m / L;
            const int z = (int)(m % L);
            const int64_t r = a.idx ? a.idx[b] : b;
            const bool in = r >= 0 && r < a.rows;
            const float *x = a.yhat + m * a.ldy + hd.col0;
            const float *t = hd.target + (in ? r * hd.ld_target + (int64_t)z * C : 0);
            float mx = x[0];
            for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);   // (a NaN logit reaches s below)
            float s = 0.f, st = 0.f;
            for (int c = 0; c < C; ++c) {
                s = s + expf(x[c] - mx);
                st = st + (in ? t[c] : NAN);
            }
            const float lse = mx + logf(s);
            for (int c = 0; c < C; ++c) {
                const float xc = x[c], tc = in ? t[c] : NAN;
                sum_d += (double)(tc * (lse - xc));
                if (a.dy) a.dy[m * a.lddy + hd.col0 + c] = hd.is_loss ? (expf(xc - lse) * st - tc) * wd : 0.f;
            }
        }
    } else {
        const bool local = hd.kind == FV3HIP_EMULATOR_HEAD_MSE_LOCAL;
        const bool has_d = hd.slot >= 0, has_a = hd.slot_after >= 0;
        const int64_t total = a.n * L * C;   // dense: L = 1; local: C = 1
        for (int64_t e = (int64_t)block * kBlock + tid; e < total; e += (int64_t)blocks * kBlock) {
            const int64_t m = e / C;
            const int j = (int)(e % C);
            const int64_t b = local ? m / L : m;
            const int z = local ? (int)(m % L) : 0;
            const int t = local ? z : j;         // the tables' index, and the column of a target row
            float g = 0.f;
            if ((has_d || has_a) && !(local && hd.single_level && z != 0)) {
                const int64_t r = a.idx ? a.idx[b] : b;
                const bool in = r >= 0 && r < a.rows;
                const float y = a.yhat[m * a.ldy + hd.col0 + j];
                const float p = hd.scale ? y * hd.scale[t] + hd.center[t] : y;
                if (has_d) {
                    const float d = p - (in ? hd.target[r * hd.ld_target + t] : NAN);
                    const float inv = hd.inv[t];
                    sum_d += (double)(d * d * inv);
                    if (hd.is_loss) g = 2.f * d * inv * wd;   // (a metric term is reported and sends nothing into dY)
                }
                if (has_a) {
                    const float aft = (in ? hd.before[r * hd.ld_before + t] : 0.f) + p;
                    const float ea = aft - (in ? hd.target_after[r * hd.ld_target_after + t] : NAN);
                    const float inv = hd.inv_after[t];
                    sum_a += (double)(ea * ea * inv);
                    if (hd.is_loss_after) g = g + 2.f * ea * inv * wa;
                }
                if (hd.scale) g = g * hd.scale[t];
            }
            if (a.dy) a.dy[m * a.lddy + hd.col0 + j] = g;
        }
    }
    part[tid] = sum_d;
    block_tree_sum(part, tid);
    if (tid == 0) a.partial[2 * (int64_t)blockIdx.x] = part[0];
    __syncthreads();
    part[tid] = sum_a;
    block_tree_sum(part, tid);
    if (tid == 0) a.partial[2 * (int64_t)blockIdx.x + 1] = part[0];
}

struct EmuFinishArgs {
    double wval[kEmuSlots], weight[kEmuSlots];
    int is_loss[kEmuSlots];                      // 0: a metric slot, which does not enter the loss
    int first[kEmuSlots], count[kEmuSlots];      // the slot's partials: partial[first + 2 i], i < count
    int n_slots;
    const double *partial;
    double *values, *loss, *accum;
};

// values[slot] = (the slot's partials added in ascending block order) * wval; loss = the loss slots' weight * value added in
// slot order; one thread then adds loss and the values into accum (if given) in that order
__global__ __launch_bounds__(kEmuFinishThreads) void train_emulator_loss_finish_kernel(const EmuFinishArgs f)
{
    __shared__ double vals[kEmuSlots];
    const int s = threadIdx.x;
    if (s < f.n_slots) {
        const double *p = f.partial + f.first[s];
        double sum = 0.0;
        for (int i = 0; i < f.count[s]; ++i) sum += p[2 * i];
        vals[s] = sum * f.wval[s];
        f.values[s] = vals[s];
    }
    __syncthreads();
    if (s == 0) {
        double loss = 0.0;
        for (int i = 0; i < f.n_slots; ++i)
            if (f.is_loss[i]) loss += f.weight[i] * vals[i];
        f.loss[0] = loss;
        if (f.accum) {
            f.accum[0] += loss;
            for (int i = 0; i < f.n_slots; ++i) f.accum[1 + i] += vals[i];
        }
    }
}

// torch.optim.Adam's default update (no weight decay, no amsgrad) at step t = step[0] + 1, rounded as torch's kernels round
// it: the first moment is exp_avg.lerp_(grad, 1 - beta1) = fma(1 - beta1, g - m, m), which is beta1 m + (1 - beta1) g with one
// rounding fewer; the second is v beta2 + ((1 - beta2) g) g; the update p - (step_size m) / (sqrt(v) / bc2_sqrt + eps).
// DECAY: torch.optim.AdamW's decoupled weight decay first, p *= (float)(1 - lr weight_decay), one rounded product.
template <bool DECAY>
__global__ __launch_bounds__(kBlock) void train_adam_kernel(float *p, const float *grad, float *m, float *v, int64_t count,
                                                             const int64_t *step, double lr, double beta1, double beta2, double eps,
                                                             float decay)
{
    __shared__ float consts[2];
    if (threadIdx.x == 0) {
        const double t = (double)(step[0] + 1);
        consts[0] = (float)(lr / (1.0 - pow(beta1, t)));
        consts[1] = (float)sqrt(1.0 - pow(beta2, t));
    }
    __syncthreads();
    const float step_size = consts[0], bc2_sqrt = consts[1];
    const float omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2), epsf = (float)eps;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < count; e += (int64_t)gridDim.x * kBlock) {
        const float gr = grad[e];
        const float mm = fmaf(omb1, gr - m[e], m[e]);
        const float vv = b2 * v[e] + omb2 * gr * gr;
        m[e] = mm;
        v[e] = vv;
        const float denom = sqrtf(vv) / bc2_sqrt + epsf;
        const float pe = DECAY ? p[e] * decay : p[e];
        p[e] = pe - step_size * mm / denom;
    }
}

__global__ void train_step_advance_kernel(int64_t *step) { step[0] += 1; }

int check_layer(int64_t n, int k, int o)
{
    FV3HIP_REQUIRE(n >= 1 && n <= ((int64_t)1 << 24), "batch rows must be in [1, 2^24], got %lld", (long long)n);
    FV3HIP_REQUIRE(k >= 1 && o >= 1 && k <= (1 << 20) && o <= (1 << 20), "in and out features must be in [1, 2^20], got %d, %d", k, o);
    return FV3HIP_OK;
}

int check_ld(const char *what, const void *p, int64_t ld, int features)
{
    FV3HIP_REQUIRE(p, "%s is null", what);
    FV3HIP_REQUIRE(ld >= features && ld <= ((int64_t)1 << 24), "%s: leading dimension %lld does not hold %d features", what, (long long)ld,
                   features);
    return FV3HIP_OK;
}

}  // namespace

extern "C" int fv3hip_train_chunk_rows(void) { return kChunkRows; }

extern "C" size_t fv3hip_train_backward_weight_workspace_bytes(int64_t n, int k, int o)
{
    if (n <= kChunkRows || k < 1 || o < 1) return 0;
    return (size_t)ceil_div(n, kChunkRows) * (size_t)(k + 1) * (size_t)o * sizeof(float);
}

extern "C" int fv3hip_train_loss_workspace_doubles(void) { return kLossBlocks; }

extern "C" int fv3hip_train_linear_forward(const float *A, int64_t lda, int64_t a_rows, const int64_t *idx, const float *W, int64_t ldw,
                                           const float *bias, float *H, int64_t ldh, int64_t n, int k, int o, int act, void *stream)
{
    int rc;
    if ((rc = check_layer(n, k, o)) || (rc = check_ld("A", A, lda, k)) || (rc = check_ld("W", W, ldw, o)) || (rc = check_ld("H", H, ldh, o)))
        return rc;
    FV3HIP_REQUIRE(a_rows >= 1 && (idx || a_rows >= n), "A has %lld rows, the batch %lld", (long long)a_rows, (long long)n);
    if (act != FV3HIP_ACT_LINEAR && act != FV3HIP_ACT_RELU)
        return fail(FV3HIP_EUNSUPPORTED, "activation code %d: FV3HIP_ACT_LINEAR and _RELU are built", act);
    TrainGemmArgs g{};
    g.a = A, g.idx = idx, g.lda = lda, g.a_rows = a_rows, g.b = W, g.ldb = ldw, g.c = H, g.ldc = ldh, g.bias = bias;
    g.n = n, g.k = k, g.o = o, g.act = act, g.n_chunks = 1;
    const dim3 grid((unsigned)ceil_div(n, kBM), (unsigned)ceil_div(o, kBN));
    hipLaunchKernelGGL(train_gemm_kernel<NN>, grid, dim3(kBlock), 0, as_stream(stream), g);
    return check_launch("train_gemm_kernel<NN>");
}

extern "C" int fv3hip_train_linear_backward_data(const float *dH, int64_t lddh, const float *W, int64_t ldw, const float *P, int64_t ldp,
                                                 int p_stride, float *dA, int64_t ldda, int64_t n, int k, int o, void *stream)
{
    int rc;
    if ((rc = check_layer(n, k, o)) || (rc = check_ld("dH", dH, lddh, o)) || (rc = check_ld("W", W, ldw, o)) ||
        (rc = check_ld("dA", dA, ldda, k)))
        return rc;
    if (P && (rc = check_ld("P", P, ldp, k))) return rc;
    FV3HIP_REQUIRE(p_stride == 0 || p_stride == 1, "p_stride must be 0 (one shared activation row) or 1, got %d", p_stride);
    TrainGemmArgs g{};
    g.a = dH, g.lda = lddh, g.b = W, g.ldb = ldw, g.c = dA, g.ldc = ldda, g.p = P, g.ldp = ldp, g.p_stride = p_stride;
    g.n = n, g.k = k, g.o = o, g.n_chunks = 1;
    const dim3 grid((unsigned)ceil_div(n, kBM), (unsigned)ceil_div(k, kBN));
    hipLaunchKernelGGL(train_gemm_kernel<NT>, grid, dim3(kBlock), 0, as_stream(stream), g);
    return check_launch("train_gemm_kernel<NT>");
}

extern "C" int fv3hip_train_linear_backward_weight(const float *A, int64_t lda, int64_t a_rows, const int64_t *idx, const float *dH,
                                                   int64_t lddh, float *dW, int64_t lddw, float *db, float *workspace,
                                                   size_t workspace_bytes, int64_t n, int k, int o, void *stream)
{
    int rc;
    if ((rc = check_layer(n, k, o)) || (rc = check_ld("A", A, lda, k)) || (rc = check_ld("dH", dH, lddh, o)) ||
        (rc = check_ld("dW", dW, lddw, o)))
        return rc;
    FV3HIP_REQUIRE(db, "db is null");
    FV3HIP_REQUIRE(a_rows >= 1 && (idx || a_rows >= n), "A has %lld rows, the batch %lld", (long long)a_rows, (long long)n);
    const int n_chunks = (int)ceil_div(n, kChunkRows);
    const size_t need = fv3hip_train_backward_weight_workspace_bytes(n, k, o);
    FV3HIP_REQUIRE(n_chunks == 1 || (workspace && workspace_bytes >= need), "a batch of %lld rows needs a workspace of %zu bytes, got %zu",
                   (long long)n, need, workspace ? workspace_bytes : (size_t)0);
    TrainGemmArgs g{};
    g.a = A, g.idx = idx, g.lda = lda, g.a_rows = a_rows, g.b = dH, g.ldb = lddh, g.db = db;
    g.c = n_chunks > 1 ? workspace : dW, g.ldc = lddw;
    g.n = n, g.k = k, g.o = o, g.n_chunks = n_chunks;
    const dim3 grid((unsigned)ceil_div(k + 1, kBM), (unsigned)ceil_div(o, kBN), (unsigned)n_chunks);
    hipLaunchKernelGGL(train_gemm_kernel<TN>, grid, dim3(kBlock), 0, as_stream(stream), g);
    if ((rc = check_launch("train_gemm_kernel<TN>"))) return rc;
    if (n_chunks > 1) {
        hipLaunchKernelGGL(train_chunk_sum_kernel, dim3(grid_stride_blocks((int64_t)(k + 1) * o)), dim3(kBlock), 0, as_stream(stream),
                           workspace, n_chunks, k, o, dW, lddw, db);
        return check_launch("train_chunk_sum_kernel");
    }
    return FV3HIP_OK;
}

extern "C" int fv3hip_train_mse_grad(const float *yhat, int64_t ldy, const float *scale, const float *center, const float *inv_cstd2,
                                     const float *lo, const float *hi, const float *keep, const float *wnorm, const float *targets,
                                     int64_t ldt, int64_t t_rows, const int64_t *idx, float *dY, int64_t lddy, double *loss,
                                     double *loss_workspace, int64_t n, int f, void *stream)
{
    int rc;
    if ((rc = check_layer(n, 1, f)) || (rc = check_ld("yhat", yhat, ldy, f)) || (rc = check_ld("targets", targets, ldt, f)) ||
        (rc = check_ld("dY", dY, lddy, f)))
        return rc;
    FV3HIP_REQUIRE(scale && center && inv_cstd2 && lo && hi && keep && wnorm, "a per-feature array is null");
    FV3HIP_REQUIRE(loss && loss_workspace, "loss or its workspace is null");
    FV3HIP_REQUIRE(t_rows >= 1 && (idx || t_rows >= n), "the targets have %lld rows, the batch %lld", (long long)t_rows, (long long)n);
    MseArgs a{};
    a.yhat = yhat, a.scale = scale, a.center = center, a.inv_cstd2 = inv_cstd2, a.lo = lo, a.hi = hi, a.keep = keep, a.wnorm = wnorm;
    a.t = targets, a.idx = idx, a.dy = dY, a.partial = loss_workspace;
    a.ldy = ldy, a.ldt = ldt, a.lddy = lddy, a.t_rows = t_rows, a.n = n, a.f = f;
    const int64_t want = ceil_div(n * f, kBlock);
    const int blocks = (int)(want < kLossBlocks ? want : kLossBlocks);
    hipLaunchKernelGGL(train_mse_grad_kernel, dim3(blocks), dim3(kBlock), 0, as_stream(stream), a);
    if ((rc = check_launch("train_mse_grad_kernel"))) return rc;
    hipLaunchKernelGGL(train_loss_finish_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), loss_workspace, blocks, loss);
    return check_launch("train_loss_finish_kernel");
}

extern "C" int fv3hip_train_precip_loss_grad(const float *yhat, int64_t ldy, const float *scale1, const float *center1, const float *scale2,
                                             const float *center2, const float *inv_cstd2_1, const float *inv_cstd2_2, float inv_cstd2_3,
                                             const float *delp, int64_t ldd, const float *physics_precip, const float *T1, const float *T2,
                                             int64_t ldt, const float *T3, int64_t rows, const int64_t *idx, int couple, int has_dead,
                                             float l1, float l2, float *dY, int64_t lddy, double *loss, double *loss_workspace, float *dq1,
                                             float *dq2, float *precip, int64_t n, int nz, void *stream)
{
    int rc;
    if ((rc = check_layer(n, 1, nz))) return rc;
    FV3HIP_REQUIRE(has_dead == 0 || has_dead == 1, "has_dead must be 0 or 1, got %d", has_dead);
    FV3HIP_REQUIRE(couple == 0 || couple == 1, "couple must be 0 or 1, got %d", couple);
    const int f = 3 * nz + has_dead;
    if ((rc = check_ld("yhat", yhat, ldy, f)) || (rc = check_ld("dY", dY, lddy, f)) || (rc = check_ld("delp", delp, ldd, nz)) ||
        (rc = check_ld("T1", T1, ldt, nz)) || (rc = check_ld("T2", T2, ldt, nz)))
        return rc;
    FV3HIP_REQUIRE(scale1 && center1 && scale2 && center2 && inv_cstd2_1 && inv_cstd2_2, "a per-level array is null");
    FV3HIP_REQUIRE(physics_precip && T3, "physics_precip or T3 is null");
    FV3HIP_REQUIRE(loss && loss_workspace, "loss or its workspace is null");
    FV3HIP_REQUIRE(rows >= 1 && (idx || rows >= n), "the resident arrays have %lld rows, the batch %lld", (long long)rows, (long long)n);
    FV3HIP_REQUIRE(l1 >= 0.f && l2 >= 0.f && std::isfinite(l1) && std::isfinite(l2), "l1 and l2 must be finite and >= 0, got %g, %g",
                   (double)l1, (double)l2);
    PrecipLossArgs a{};
    a.yhat = yhat, a.scale1 = scale1, a.center1 = center1, a.scale2 = scale2, a.center2 = center2, a.inv1 = inv_cstd2_1, a.inv2 = inv_cstd2_2;
    a.delp = delp, a.pp = physics_precip, a.t1 = T1, a.t2 = T2, a.t3 = T3, a.idx = idx, a.dy = dY, a.dq1 = dq1, a.dq2 = dq2, a.precip = precip;
    a.partial = loss_workspace, a.ldy = ldy, a.ldd = ldd, a.ldt = ldt, a.lddy = lddy, a.rows = rows, a.n = n;
    a.nz = nz, a.couple = couple, a.has_dead = has_dead, a.inv3 = inv_cstd2_3, a.l1 = l1, a.l2 = l2;
    a.w12 = (float)(1.0 / ((double)n * (double)nz)), a.w3 = (float)(1.0 / (double)n);
    const int64_t want = ceil_div(n, kRowsPerBlock);
    const int blocks = (int)(want < kLossBlocks ? want : kLossBlocks);
    hipLaunchKernelGGL(train_precip_loss_grad_kernel, dim3(blocks), dim3(kBlock), 0, as_stream(stream), a);
    if ((rc = check_launch("train_precip_loss_grad_kernel"))) return rc;
    hipLaunchKernelGGL(train_loss_finish_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), loss_workspace, blocks, loss);
    return check_launch("train_loss_finish_kernel");
}

extern "C" int fv3hip_train_emulator_loss_workspace_doubles(void) { return kEmuHeads * kEmuBlocksPerHead * 2; }

extern "C" int fv3hip_train_emulator_loss_grad(const float *yhat, int64_t ldy, int64_t n, int levels, int f,
                                               const fv3hip_emulator_head_t *heads, int n_heads, int n_slots, int64_t rows,
                                               const int64_t *idx, float *dY, int64_t lddy, double *values, double *loss, double *accum,
                                               double *workspace, void *stream)
{
    int rc;
    const int64_t limit = (int64_t)1 << 24;
    FV3HIP_REQUIRE(n >= 1 && n <= limit && levels >= 1 && levels <= limit && n * levels <= limit,
                   "batch rows, levels and their product must be in [1, 2^24], got %lld, %d", (long long)n, levels);
    FV3HIP_REQUIRE(f >= 1 && f <= (1 << 20), "head features must be in [1, 2^20], got %d", f);
    if ((rc = check_ld("yhat", yhat, ldy, f))) return rc;
    if (dY && (rc = check_ld("dY", dY, lddy, f))) return rc;
    FV3HIP_REQUIRE(heads && n_heads >= 1, "the head table is null or empty");
    FV3HIP_REQUIRE(n_heads <= kEmuHeads, "%d heads: the head table holds at most %d", n_heads, kEmuHeads);
    FV3HIP_REQUIRE(n_slots >= 0 && n_slots <= kEmuSlots, "%d slots: at most %d", n_slots, kEmuSlots);
    FV3HIP_REQUIRE(values && loss && workspace, "values, loss or the workspace is null");
    FV3HIP_REQUIRE(rows >= 1 && (idx || rows >= n), "the resident arrays have %lld rows, the batch %lld", (long long)rows, (long long)n);

    EmuLossArgs a{};
    EmuFinishArgs fin{};
    bool used[kEmuSlots] = {};
    int end = 0;
    a.block0[0] = 0;
    for (int h = 0; h < n_heads; ++h) {
        const fv3hip_emulator_head_t &hd = heads[h];
        FV3HIP_REQUIRE(hd.ncol >= 1 && hd.col0 >= 0, "head %d: columns [%d, %d + %d)", h, hd.col0, hd.col0, hd.ncol);
        FV3HIP_REQUIRE(hd.col0 >= end, "head %d starts at column %d: it overlaps the head before it, which ends at %d", h, hd.col0, end);
        FV3HIP_REQUIRE(hd.col0 == end, "columns [%d, %d) belong to no head", end, hd.col0);
        FV3HIP_REQUIRE((int64_t)hd.col0 + hd.ncol <= f, "head %d ends at column %lld, past the %d head features", h,
                       (long long)hd.col0 + hd.ncol, f);
        end = hd.col0 + hd.ncol;
        const bool xent = hd.kind == FV3HIP_EMULATOR_HEAD_XENT, local = hd.kind == FV3HIP_EMULATOR_HEAD_MSE_LOCAL;
        FV3HIP_REQUIRE(xent || local || hd.kind == FV3HIP_EMULATOR_HEAD_MSE_DENSE, "head %d: unknown kind %d", h, hd.kind);
        FV3HIP_REQUIRE(hd.single_level == 0 || (hd.single_level == 1 && local), "head %d: single_level goes with a local MSE head", h);
        int64_t count, extent;
        if (xent) {
            FV3HIP_REQUIRE(hd.ncol >= 2 && hd.ncol <= 32, "head %d: a cross-entropy head has 2 to 32 channels, got %d", h, hd.ncol);
            FV3HIP_REQUIRE(hd.slot >= 0 && hd.slot_after < 0 && !hd.scale && !hd.center,
                           "head %d: a cross-entropy head has a direct term only and is unscaled", h);
            count = n * levels, extent = (int64_t)levels * hd.ncol;
        } else if (local) {
            FV3HIP_REQUIRE(hd.ncol == 1, "head %d: a local MSE head has one column, got %d", h, hd.ncol);
            count = hd.single_level ? n : n * levels, extent = hd.single_level ? 1 : levels;
        } else {
            FV3HIP_REQUIRE(levels == 1, "head %d: a dense MSE head needs levels == 1, got %d", h, levels);
            count = n * hd.ncol, extent = hd.ncol;
        }
        FV3HIP_REQUIRE(!hd.scale == !hd.center, "head %d: scale and center go together", h);
        const int slots[2] = {hd.slot, hd.slot_after};
        const double weights[2] = {hd.weight, hd.weight_after};
        const int is_loss[2] = {hd.is_loss, hd.is_loss_after};
        for (int which = 0; which < 2; ++which) {
            const int s = slots[which];
            if (s < 0) continue;
            FV3HIP_REQUIRE(s < n_slots && !used[s], "head %d: slot %d is out of range or used twice (%d slots)", h, s, n_slots);
            FV3HIP_REQUIRE(std::isfinite(weights[which]) && weights[which] >= 0.0, "head %d: weight %g must be finite and >= 0", h,
                           weights[which]);
            FV3HIP_REQUIRE(is_loss[which] == 0 || is_loss[which] == 1, "head %d: is_loss must be 0 or 1", h);
            used[s] = true;
            if (which == 0) {
                FV3HIP_REQUIRE(hd.target && (xent || hd.inv), "head %d: the direct term's target or inv is null", h);
                FV3HIP_REQUIRE(hd.ld_target >= extent, "head %d: ld_target %lld does not hold %lld values", h, (long long)hd.ld_target,
                               (long long)extent);
            } else {
                FV3HIP_REQUIRE(hd.target_after && hd.before && hd.inv_after, "head %d: the after term's target, before or inv is null", h);
                FV3HIP_REQUIRE(hd.ld_target_after >= extent && hd.ld_before >= extent,
                               "head %d: ld_target_after %lld or ld_before %lld does not hold %lld values", h,
                               (long long)hd.ld_target_after, (long long)hd.ld_before, (long long)extent);
            }
            const float wgrad = is_loss[which] ? (float)(weights[which] / (double)count) : 0.f;
            (which == 0 ? a.wgrad_d : a.wgrad_a)[h] = wgrad;
            fin.wval[s] = 1.0 / (double)count;
            fin.weight[s] = weights[which];
            fin.is_loss[s] = is_loss[which];
            fin.first[s] = 2 * a.block0[h] + which;
        }
        a.head[h] = hd;
        const int64_t want = ceil_div(n * levels * (xent ? 1 : hd.ncol), kBlock);
        const int blocks = (int)(want < kEmuBlocksPerHead ? want : kEmuBlocksPerHead);
        a.block0[h + 1] = a.block0[h] + blocks;
        for (int which = 0; which < 2; ++which)
            if (slots[which] >= 0) fin.count[slots[which]] = blocks;
    }
    FV3HIP_REQUIRE(end == f, "the heads end at column %d, the head layer has %d features", end, f);
    for (int s = 0; s < n_slots; ++s) FV3HIP_REQUIRE(used[s], "slot %d of %d belongs to no term", s, n_slots);

    a.n_heads = n_heads, a.levels = levels, a.yhat = yhat, a.idx = idx, a.dy = dY, a.partial = workspace;
    a.ldy = ldy, a.lddy = lddy, a.rows = rows, a.n = n;
    fin.n_slots = n_slots, fin.partial = workspace, fin.values = values, fin.loss = loss, fin.accum = accum;
    hipLaunchKernelGGL(train_emulator_loss_grad_kernel, dim3(a.block0[n_heads]), dim3(kBlock), 0, as_stream(stream), a);
    if ((rc = check_launch("train_emulator_loss_grad_kernel"))) return rc;
    hipLaunchKernelGGL(train_emulator_loss_finish_kernel, dim3(1), dim3(kEmuFinishThreads), 0, as_stream(stream), fin);
    return check_launch("train_emulator_loss_finish_kernel");
}

extern "C" int fv3hip_train_adam(float *params, const float *grad, float *m, float *v, int64_t count, int64_t *step, double lr,
                                 double beta1, double beta2, double eps, void *stream)
{
    FV3HIP_REQUIRE(params && grad && m && v && step, "a buffer is null");
    FV3HIP_REQUIRE(count >= 1, "count must be positive, got %lld", (long long)count);
    FV3HIP_REQUIRE(lr >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0, "lr, eps >= 0 and betas in [0, 1) expected");
    hipLaunchKernelGGL(train_adam_kernel<false>, dim3(grid_stride_blocks(count)), dim3(kBlock), 0, as_stream(stream), params, grad, m, v,
                       count, step, lr, beta1, beta2, eps, 1.f);
    int rc;
    if ((rc = check_launch("train_adam_kernel"))) return rc;
    hipLaunchKernelGGL(train_step_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), step);
    return check_launch("train_step_advance_kernel");
}

extern "C" int fv3hip_train_adamw(float *params, const float *grad, float *m, float *v, int64_t count, int64_t *step, double lr,
                                  double beta1, double beta2, double eps, double weight_decay, void *stream)
{
    FV3HIP_REQUIRE(params && grad && m && v && step, "a buffer is null");
    FV3HIP_REQUIRE(count >= 1, "count must be positive, got %lld", (long long)count);
    FV3HIP_REQUIRE(lr >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0 && weight_decay >= 0,
                   "lr, eps, weight_decay >= 0 and betas in [0, 1) expected");
    hipLaunchKernelGGL(train_adam_kernel<true>, dim3(grid_stride_blocks(count)), dim3(kBlock), 0, as_stream(stream), params, grad, m, v,
                       count, step, lr, beta1, beta2, eps, (float)(1.0 - lr * weight_decay));
    int rc;
    if ((rc = check_launch("train_adam_kernel"))) return rc;
    hipLaunchKernelGGL(train_step_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream), step);
    return check_launch("train_step_advance_kernel");
}
