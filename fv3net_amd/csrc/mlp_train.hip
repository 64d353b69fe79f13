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
constexpr int kLossBlocks = 1024;     // most blocks of train_mse_grad_kernel = doubles of its workspace
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
