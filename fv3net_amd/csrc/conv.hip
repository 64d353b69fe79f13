// fv3fit's convolutional predictor ("convolutional", external/fv3fit/fv3fit/keras/_models/convolutional.py:141-210,
// shared/convolutional_network.py:136-195) on gfx950 -- DESIGN.md section 13.
//
// One kernel runs every layer as an implicit GEMM on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32): M = the 256 pixels of a
// 16 x 16 spatial tile (eight 32-pixel MFMA tiles, two per wave), N = up to 64 output channels of the layer (one or two
// 32-wide MFMA tiles; further channels are other blocks, gridDim.z), K = k * k * c_in walked in chunks of CC channels.
// Per chunk the (16 + k - 1)^2 input patch and the chunk's weights are staged in LDS; there is no im2col buffer and no
// padded or normalised copy of the input.  The first layer's loader reads each variable through its own element strides,
// converts float64 on the way, applies (x - mean) / scale, and takes halo cells from (0) the input itself, (1) per-tile strip
// buffers [sample][side][depth][channel][n] or (2) the neighbouring faces of a resident six-tile cube; corners are raw zero.
// Later hidden layers and the 1 x 1 heads run the same kernel on the F-channel channel-last intermediate.
#include <cmath>
#include <vector>

#include "common.h"
#include "cube.h"

using namespace fv3hip;

namespace {

constexpr int kMaxConvInputs = 8;
constexpr int kMaxConvOutputs = 8;
constexpr int kMaxKernelSize = 7;
constexpr int kTile = 16;     // spatial tile edge: 256 output pixels per block
constexpr int kBlock = 256;   // four waves, two 32-pixel MFMA tiles each

struct ConvArray {           // one input variable or one output: element (batch b, tile t, x, y, channel c)
    const void *p;
    int64_t sb, st, sx, sy, sc;
    int f64;
};

struct LayerArgs {
    ConvArray src[kMaxConvInputs];
    ConvArray out[kMaxConvOutputs];   // float32
    const int *ch_src;       // first layer: input channel -> variable, channel inside it, mean, scale
    const int *ch_local;
    const float *ch_center;
    const float *ch_scale;
    const void *strips;      // halo mode 1: [sample][4][h][C][n]
    int strips_f64;
    int first;               // 1: multi-variable strided input with normalisation and halo modes
    int mode, h, n_tiles;
    int nx, ny;              // interior extent (first layer); in_x = nx + 2 h
    int in_x, in_y, out_x, out_y;
    int C, N;
    const float *w;          // [k][k][C][N]
    const float *bias;       // [N] or null
    const float *oscale;     // heads: y * scale + center; null for hidden layers
    const float *ocenter;
    const int *och_out;      // heads: output channel -> output array, channel inside it; null: array 0, channel n
    const int *och_local;
    int act;
    int tiles_y;
    int swap;                // 1: x is the faster axis in memory -> x runs fastest inside the tile
    int cfast;               // 1: the channel is the fastest axis in memory
    CubeSeams seams;         // halo mode 2
};

__device__ inline float load_value(const void *p, int f64, int64_t off)
{
    return f64 ? (float)reinterpret_cast<const double *>(p)[off] : reinterpret_cast<const float *>(p)[off];
}

// raw value of input channel c at (gx, gy) of the padded field of sample (b, t); the caller has checked gx < in_x, gy < in_y
__device__ inline float load_raw(const LayerArgs &a, int b, int t, int c, int gx, int gy)
{
    int si = 0, lc = c;
    if (a.first) {
        si = a.ch_src[c];
        lc = a.ch_local[c];
    }
    const ConvArray &s = a.src[si];
    const int x = gx - a.h, y = gy - a.h;
    const bool inx = (unsigned)x < (unsigned)a.nx, iny = (unsigned)y < (unsigned)a.ny;
    if (inx && iny) return load_value(s.p, s.f64, b * s.sb + t * s.st + x * s.sx + y * s.sy + lc * s.sc);
    if (!inx && !iny) return 0.f;   // the corners stay zero (halos.py:135-160)
    const int n = a.nx;             // (modes 1 and 2 need square tiles)
    int side, d, j;
    seam_side(n, x, y, inx, side, d, j);
    if (a.mode == FV3HIP_CONV_HALO_STRIPS) {
        const int64_t off = (((((int64_t)b * a.n_tiles + t) * 4 + side) * a.h + d) * a.C + c) * n + j;
        return load_value(a.strips, a.strips_f64, off);
    }
    int tt, xx, yy;   // resident cube
    seam_cross(a.seams, n, t, side, d, j, tt, xx, yy);
    return load_value(s.p, s.f64, b * s.sb + (int64_t)tt * s.st + xx * s.sx + yy * s.sy + lc * s.sc);
}

template <int K>
struct Chunk {
    static constexpr int CC = K <= 3 ? 8 : (K == 5 ? 4 : 2);   // channels per K chunk (LDS: patch + weights <= 40 KB)
};

template <int K, int NT, bool TR>
__global__ __launch_bounds__(kBlock) void conv_layer_kernel(const LayerArgs a)
{
    constexpr int CC = Chunk<K>::CC;
    constexpr int P = kTile + K - 1;
    // the two lane halves of an MFMA operand hold adjacent channels: channel strides of 34 (patch; a half spans 34 banks) and
    // 32 (weights) modulo the 64 banks keep them apart
    constexpr int PP = (P * P - 34 + 63) / 64 * 64 + 34;
    constexpr int NG = NT * 32;
    constexpr int NGP = NT == 2 ? 96 : 32;
    __shared__ float patch[CC * PP];
    __shared__ float wl[K * K * CC * NGP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (blockIdx.x / a.tiles_y) * kTile, y0 = (blockIdx.x % a.tiles_y) * kTile;
    const int b = blockIdx.y / a.n_tiles, t = blockIdx.y % a.n_tiles;
    const int n0 = blockIdx.z * NG;
    const int hh = lane >> 5, l31 = lane & 31;
    const int sxl = a.swap ? 1 : P, syl = a.swap ? P : 1;

    f32x16 acc[2][NT];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][nt][r] = 0.f;
    int base[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) base[mi] = ((2 * wave + mi) * 2 + (l31 >> 4)) * P + (l31 & 15);

    for (int c0 = 0; c0 < a.C; c0 += CC) {
        __syncthreads();
        for (int e = tid; e < CC * P * P; e += kBlock) {
            int cc, pos;
            if (a.cfast) {
                cc = e % CC;
                pos = e / CC;
            } else {
                pos = e % (P * P);
                cc = e / (P * P);
            }
            const int qa = pos / P, qb = pos % P;
            const int gx = x0 + (a.swap ? qb : qa), gy = y0 + (a.swap ? qa : qb);
            const int c = c0 + cc;
            float v = 0.f;
            if (c < a.C && gx < a.in_x && gy < a.in_y) {
                v = load_raw(a, b, t, c, gx, gy);
                if (a.first) v = (v - a.ch_center[c]) / a.ch_scale[c];
            }
            patch[cc * PP + pos] = v;
        }
        for (int e = tid; e < K * K * CC * NG; e += kBlock) {
            const int j = e % NG, r = e / NG;
            const int c = c0 + r % CC, tap = r / CC, n = n0 + j;
            wl[r * NGP + j] = (c < a.C && n < a.N) ? a.w[((int64_t)tap * a.C + c) * a.N + n] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int dx = 0; dx < K; ++dx) {
#pragma unroll
            for (int dy = 0; dy < K; ++dy) {
                const int toff = dx * sxl + dy * syl;
#pragma unroll
                for (int cp = 0; cp < CC / 2; ++cp) {
                    const int cc = 2 * cp + hh;
                    const float xv0 = patch[cc * PP + base[0] + toff];
                    const float xv1 = patch[cc * PP + base[1] + toff];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const float wv = wl[((dx * K + dy) * CC + cc) * NGP + nt * 32 + l31];
                        if (TR) {
                            acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, xv0, acc[0][nt], 0, 0, 0);
                            acc[1][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, xv1, acc[1][nt], 0, 0, 0);
                        } else {
                            acc[0][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv0, wv, acc[0][nt], 0, 0, 0);
                            acc[1][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv1, wv, acc[1][nt], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }

    // epilogue: D[row][col], col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5); rows are pixels, or filters if TR
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                const int pix = TR ? l31 : row, fil = TR ? row : l31;
                const int n = n0 + nt * 32 + fil;
                const int pa = (2 * wave + mi) * 2 + (pix >> 4), pb = pix & 15;
                const int ox = x0 + (a.swap ? pb : pa), oy = y0 + (a.swap ? pa : pb);
                if (n >= a.N || ox >= a.out_x || oy >= a.out_y) continue;
                float v = acc[mi][nt][r];
                if (a.bias) v += a.bias[n];
                if (a.act == FV3HIP_ACT_RELU)
                    v = v < 0.f ? 0.f : v;   // (a NaN stays a NaN, as in np.maximum(v, 0) and Keras' relu: see mlp.hip)
                else if (a.act == FV3HIP_ACT_TANH)
                    v = tanhf(v);
                if (a.oscale) v = v * a.oscale[n] + a.ocenter[n];
                int oi = 0, ol = n;
                if (a.och_out) {
                    oi = a.och_out[n];
                    ol = a.och_local[n];
                }
                const ConvArray &o = a.out[oi];
                reinterpret_cast<float *>(const_cast<void *>(o.p))[b * o.sb + t * o.st + ox * o.sx + oy * o.sy + ol * o.sc] = v;
            }
        }
    }
}

template <int K>
int launch_k(const LayerArgs &a, bool tr, dim3 grid, int nt, hipStream_t st)
{
    if (nt == 1) {
        if (tr)
            hipLaunchKernelGGL((conv_layer_kernel<K, 1, true>), grid, dim3(kBlock), 0, st, a);
        else
            hipLaunchKernelGGL((conv_layer_kernel<K, 1, false>), grid, dim3(kBlock), 0, st, a);
    } else {
        if (tr)
            hipLaunchKernelGGL((conv_layer_kernel<K, 2, true>), grid, dim3(kBlock), 0, st, a);
        else
            hipLaunchKernelGGL((conv_layer_kernel<K, 2, false>), grid, dim3(kBlock), 0, st, a);
    }
    return check_launch("conv_layer_kernel");
}

// one layer: `a` carries the arrays; the grid, the tile orientation and the kernel variant are chosen here
int launch_layer(LayerArgs &a, int k, int64_t n_samples, hipStream_t st)
{
    // One access pattern per launch, chosen from the FIRST input (swap; cfast from any input whose channel is its unit-stride
    // axis) and the FIRST output (TR).  Inputs or outputs laid out differently from those stay correct -- every element is
    // addressed through its own strides -- but are read or written with the strides of the other layout, i.e. uncoalesced.
    const ConvArray &s0 = a.src[0];
    auto mag = [](int64_t v) { return v < 0 ? -v : v; };
    a.swap = mag(s0.sx) < mag(s0.sy) ? 1 : 0;
    a.cfast = 0;
    for (int i = 0; i < (a.first ? kMaxConvInputs : 1); ++i)
        if (a.src[i].p && mag(a.src[i].sc) == 1 && mag(a.src[i].sx) > 1 && mag(a.src[i].sy) > 1) a.cfast = 1;
    const bool tr = mag(a.out[0].sc) != 1;   // channel-first output: pixels on the lanes, so that the stores run along x / y
    a.tiles_y = (int)ceil_div(a.out_y, kTile);
    const int nt = a.N > 32 ? 2 : 1;
    dim3 grid((unsigned)(ceil_div(a.out_x, kTile) * a.tiles_y), (unsigned)n_samples, (unsigned)ceil_div(a.N, nt * 32));
    switch (k) {
    case 1: return launch_k<1>(a, tr, grid, nt, st);
    case 3: return launch_k<3>(a, tr, grid, nt, st);
    case 5: return launch_k<5>(a, tr, grid, nt, st);
    case 7: return launch_k<7>(a, tr, grid, nt, st);
    }
    return fail(FV3HIP_EUNSUPPORTED, "kernel size %d is not built", k);
}

template <class T>
int upload(T **dptr, const std::vector<T> &v)
{
    if (v.empty()) return FV3HIP_OK;
    FV3HIP_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(dptr), v.size() * sizeof(T)));
    FV3HIP_CHECK_HIP(hipMemcpy(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return FV3HIP_OK;
}

struct HostConv {
    std::vector<int> ch_src, ch_local, och_out, och_local;
    std::vector<float> center, scale, hw, hb, hs, hc;
    std::vector<std::vector<float>> w, bias;
    int C = 0, NO = 0;
};

bool finite_all(const float *p, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

int build_host(const fv3hip_conv_desc_t *d, HostConv &h)
{
    FV3HIP_REQUIRE(d, "null descriptor");
    FV3HIP_REQUIRE(d->n_inputs >= 1 && d->n_inputs <= kMaxConvInputs, "n_inputs must be in [1, %d], got %d", kMaxConvInputs,
                   d->n_inputs);
    FV3HIP_REQUIRE(d->in_nfeat && d->in_center && d->in_scale, "null input arrays");
    for (int i = 0; i < d->n_inputs; ++i) {
        FV3HIP_REQUIRE(d->in_nfeat[i] >= 1 && d->in_nfeat[i] <= 4096, "input %d: nfeat must be in [1, 4096], got %d", i,
                       d->in_nfeat[i]);
        for (int c = 0; c < d->in_nfeat[i]; ++c) {
            h.ch_src.push_back(i);
            h.ch_local.push_back(c);
        }
    }
    h.C = (int)h.ch_src.size();
    FV3HIP_REQUIRE(finite_all(d->in_center, h.C) && finite_all(d->in_scale, h.C), "input center / scale must be finite");
    for (int c = 0; c < h.C; ++c) FV3HIP_REQUIRE(d->in_scale[c] != 0.f, "input scale of channel %d is zero", c);
    h.center.assign(d->in_center, d->in_center + h.C);
    h.scale.assign(d->in_scale, d->in_scale + h.C);
    const int k = d->kernel_size, F = d->filters;
    FV3HIP_REQUIRE(k >= 1 && k % 2 == 1, "kernel_size must be odd and positive, got %d", k);
    if (k > kMaxKernelSize) return fail(FV3HIP_EUNSUPPORTED, "kernel_size %d: at most %d is built", k, kMaxKernelSize);
    FV3HIP_REQUIRE(F >= 1 && F <= 4096, "filters must be in [1, 4096], got %d", F);
    FV3HIP_REQUIRE(d->n_hidden >= 1 && d->n_hidden <= 64, "n_hidden (depth - 1) must be in [1, 64], got %d", d->n_hidden);
    FV3HIP_REQUIRE(d->activation == FV3HIP_ACT_LINEAR || d->activation == FV3HIP_ACT_RELU || d->activation == FV3HIP_ACT_TANH,
                   "unknown activation code %d", d->activation);
    FV3HIP_REQUIRE(d->hidden_kernels, "null hidden_kernels");
    for (int l = 0; l < d->n_hidden; ++l) {
        const size_t cin = l == 0 ? h.C : F;
        FV3HIP_REQUIRE(d->hidden_kernels[l], "hidden kernel %d is null", l);
        FV3HIP_REQUIRE(finite_all(d->hidden_kernels[l], (size_t)k * k * cin * F), "hidden kernel %d is not finite", l);
        h.w.emplace_back(d->hidden_kernels[l], d->hidden_kernels[l] + (size_t)k * k * cin * F);
        const float *bp = d->hidden_biases ? d->hidden_biases[l] : nullptr;
        if (bp) {
            FV3HIP_REQUIRE(finite_all(bp, F), "hidden bias %d is not finite", l);
            h.bias.emplace_back(bp, bp + F);
        } else {
            h.bias.emplace_back();
        }
    }
    FV3HIP_REQUIRE(d->n_outputs >= 1 && d->n_outputs <= kMaxConvOutputs, "n_outputs must be in [1, %d], got %d",
                   kMaxConvOutputs, d->n_outputs);
    FV3HIP_REQUIRE(d->out_nfeat && d->out_kernel && d->out_bias && d->out_scale && d->out_center, "null output arrays");
    for (int j = 0; j < d->n_outputs; ++j) {
        FV3HIP_REQUIRE(d->out_nfeat[j] >= 1 && d->out_nfeat[j] <= 4096, "output %d: nfeat must be in [1, 4096], got %d", j,
                       d->out_nfeat[j]);
        for (int c = 0; c < d->out_nfeat[j]; ++c) {
            h.och_out.push_back(j);
            h.och_local.push_back(c);
        }
    }
    h.NO = (int)h.och_out.size();
    FV3HIP_REQUIRE(finite_all(d->out_kernel, (size_t)F * h.NO) && finite_all(d->out_bias, h.NO) &&
                       finite_all(d->out_scale, h.NO) && finite_all(d->out_center, h.NO),
                   "output kernel / bias / scale / center must be finite");
    h.hw.assign(d->out_kernel, d->out_kernel + (size_t)F * h.NO);
    h.hb.assign(d->out_bias, d->out_bias + h.NO);
    h.hs.assign(d->out_scale, d->out_scale + h.NO);
    h.hc.assign(d->out_center, d->out_center + h.NO);
    return FV3HIP_OK;
}

}  // namespace

struct fv3hip_conv {
    int device = 0;
    int n_inputs = 0, n_outputs = 0, n_hidden = 0, k = 0, F = 0, act = 0, C = 0, NO = 0;
    int in_nfeat[kMaxConvInputs] = {0};
    int *d_ch_src = nullptr, *d_ch_local = nullptr, *d_och_out = nullptr, *d_och_local = nullptr;
    float *d_center = nullptr, *d_scale = nullptr, *d_hw = nullptr, *d_hb = nullptr, *d_hs = nullptr, *d_hc = nullptr;
    std::vector<float *> d_w, d_bias;
};

extern "C" int fv3hip_conv_create(const fv3hip_conv_desc_t *desc, fv3hip_conv_t *out)
{
    FV3HIP_REQUIRE(out, "null output handle");
    *out = nullptr;
    HostConv h;
    int rc = build_host(desc, h);
    if (rc) return rc;
    fv3hip_conv *m = new fv3hip_conv();
    m->n_inputs = desc->n_inputs;
    m->n_outputs = desc->n_outputs;
    m->n_hidden = desc->n_hidden;
    m->k = desc->kernel_size;
    m->F = desc->filters;
    m->act = desc->activation;
    m->C = h.C;
    m->NO = h.NO;
    for (int i = 0; i < desc->n_inputs; ++i) m->in_nfeat[i] = desc->in_nfeat[i];
    m->d_w.assign(desc->n_hidden, nullptr);
    m->d_bias.assign(desc->n_hidden, nullptr);
    rc = [&]() -> int {
        FV3HIP_CHECK_HIP(hipGetDevice(&m->device));
        int r;
        if ((r = upload(&m->d_ch_src, h.ch_src)) || (r = upload(&m->d_ch_local, h.ch_local)) ||
            (r = upload(&m->d_och_out, h.och_out)) || (r = upload(&m->d_och_local, h.och_local)) ||
            (r = upload(&m->d_center, h.center)) || (r = upload(&m->d_scale, h.scale)) || (r = upload(&m->d_hw, h.hw)) ||
            (r = upload(&m->d_hb, h.hb)) || (r = upload(&m->d_hs, h.hs)) || (r = upload(&m->d_hc, h.hc)))
            return r;
        for (int l = 0; l < m->n_hidden; ++l)
            if ((r = upload(&m->d_w[l], h.w[l])) || (r = upload(&m->d_bias[l], h.bias[l]))) return r;
        return FV3HIP_OK;
    }();
    if (rc) {
        fv3hip_conv_destroy(m);
        return rc;
    }
    *out = m;
    return FV3HIP_OK;
}

extern "C" int fv3hip_conv_destroy(fv3hip_conv_t m)
{
    if (!m) return FV3HIP_OK;
    for (void *q : {(void *)m->d_ch_src, (void *)m->d_ch_local, (void *)m->d_och_out, (void *)m->d_och_local,
                    (void *)m->d_center, (void *)m->d_scale, (void *)m->d_hw, (void *)m->d_hb, (void *)m->d_hs, (void *)m->d_hc})
        if (q) (void)hipFree(q);
    for (float *q : m->d_w)
        if (q) (void)hipFree(q);
    for (float *q : m->d_bias)
        if (q) (void)hipFree(q);
    delete m;
    return FV3HIP_OK;
}

namespace {

// the two ping-pong buffers of hidden outputs: [sample][x][y][F] float32, the first layer's extent
size_t hidden_buffer_floats(fv3hip_conv_t m, int64_t n_samples, int nx, int ny)
{
    const int h = (m->k - 1) / 2 * m->n_hidden;
    const int64_t x1 = nx + 2 * h - (m->k - 1), y1 = ny + 2 * h - (m->k - 1);
    return (size_t)(n_samples * x1 * y1 * m->F + 63) / 64 * 64;
}

}  // namespace

extern "C" size_t fv3hip_conv_workspace_bytes(fv3hip_conv_t m, int64_t n_batch, int n_tiles, int nx, int ny)
{
    if (!m || n_batch < 0 || n_tiles < 1 || nx < 1 || ny < 1) return 0;
    return hidden_buffer_floats(m, n_batch * n_tiles, nx, ny) * sizeof(float) * (m->n_hidden > 1 ? 2 : 1);
}

extern "C" int fv3hip_conv_predict(fv3hip_conv_t m, const void *const *sources, const int *src_dtype,
                                   const int64_t *src_strides, int64_t n_batch, int n_tiles, int nx, int ny, int halo_mode,
                                   const void *strips, int strips_dtype, float *const *outputs, const int64_t *out_strides,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    FV3HIP_REQUIRE(m, "null conv handle");
    FV3HIP_REQUIRE(sources && src_dtype && src_strides && outputs && out_strides, "null pointer");
    FV3HIP_REQUIRE(n_tiles >= 1 && n_batch >= 0 && n_batch * n_tiles <= 65535,
                   "n_batch * n_tiles must be in [0, 65535], got %lld x %d", (long long)n_batch, n_tiles);
    FV3HIP_REQUIRE(nx >= 1 && ny >= 1 && nx <= (1 << 20) && ny <= (1 << 20), "nx and ny must be in [1, 2^20], got %d, %d", nx, ny);
    FV3HIP_REQUIRE(halo_mode == FV3HIP_CONV_HALO_INPUT || halo_mode == FV3HIP_CONV_HALO_STRIPS ||
                       halo_mode == FV3HIP_CONV_HALO_CUBE, "unknown halo mode %d", halo_mode);
    const int k = m->k, h = (k - 1) / 2 * m->n_hidden;
    if (halo_mode != FV3HIP_CONV_HALO_INPUT) {
        FV3HIP_REQUIRE(nx == ny, "halo modes STRIPS and CUBE need square tiles, got %d x %d", nx, ny);
        FV3HIP_REQUIRE(h <= nx, "the halo (%d cells) is wider than the tile (%d)", h, nx);
    }
    if (halo_mode == FV3HIP_CONV_HALO_CUBE) FV3HIP_REQUIRE(n_tiles == 6, "halo mode CUBE needs the six tiles, got %d", n_tiles);
    if (halo_mode == FV3HIP_CONV_HALO_STRIPS && h > 0) {
        FV3HIP_REQUIRE(strips, "halo mode STRIPS needs the strip buffer");
        FV3HIP_REQUIRE(strips_dtype == FV3HIP_F32 || strips_dtype == FV3HIP_F64, "strips: dtype must be F32 or F64");
    }
    int cur = -1;
    FV3HIP_CHECK_HIP(hipGetDevice(&cur));
    FV3HIP_REQUIRE(cur == m->device, "the model lives on device %d but the current device is %d", m->device, cur);
    const int64_t S = n_batch * n_tiles;
    if (S == 0) return FV3HIP_OK;
    FV3HIP_REQUIRE(workspace_bytes >= fv3hip_conv_workspace_bytes(m, n_batch, n_tiles, nx, ny) && workspace,
                   "workspace of %zu bytes, fv3hip_conv_workspace_bytes asks for %zu", workspace_bytes,
                   fv3hip_conv_workspace_bytes(m, n_batch, n_tiles, nx, ny));
    const hipStream_t st = as_stream(stream);
    const size_t buf = hidden_buffer_floats(m, S, nx, ny);
    float *hidden[2] = {static_cast<float *>(workspace), static_cast<float *>(workspace) + buf};

    LayerArgs a;
    int in_x = nx + 2 * h, in_y = ny + 2 * h;
    for (int l = 0; l <= m->n_hidden; ++l) {
        memset(&a, 0, sizeof(a));
        const bool head = l == m->n_hidden;
        const int kk = head ? 1 : k;
        a.n_tiles = n_tiles;
        a.in_x = in_x;
        a.in_y = in_y;
        a.out_x = in_x - (kk - 1);
        a.out_y = in_y - (kk - 1);
        if (l == 0) {
            a.first = 1;
            a.mode = halo_mode;
            a.h = halo_mode == FV3HIP_CONV_HALO_INPUT ? 0 : h;
            a.nx = halo_mode == FV3HIP_CONV_HALO_INPUT ? in_x : nx;
            a.ny = halo_mode == FV3HIP_CONV_HALO_INPUT ? in_y : ny;
            for (int i = 0; i < m->n_inputs; ++i) {
                FV3HIP_REQUIRE(sources[i], "source %d is null", i);
                FV3HIP_REQUIRE(src_dtype[i] == FV3HIP_F32 || src_dtype[i] == FV3HIP_F64, "source %d: dtype must be F32 or F64", i);
                const int64_t *s = src_strides + 5 * i;
                a.src[i] = ConvArray{sources[i], s[0], s[1], s[2], s[3], s[4], src_dtype[i] == FV3HIP_F64 ? 1 : 0};
            }
            a.ch_src = m->d_ch_src;
            a.ch_local = m->d_ch_local;
            a.ch_center = m->d_center;
            a.ch_scale = m->d_scale;
            a.strips = strips;
            a.strips_f64 = strips_dtype == FV3HIP_F64 ? 1 : 0;
            a.seams = cube_seams();
            a.C = m->C;
        } else {
            // the previous layer's output: [sample][x][y][F]
            a.nx = in_x;
            a.ny = in_y;
            const int64_t F = m->F;
            a.src[0] = ConvArray{hidden[(l - 1) & 1], (int64_t)n_tiles * in_x * in_y * F, (int64_t)in_x * in_y * F, in_y * F, F, 1, 0};
            a.C = m->F;
        }
        if (!head) {
            a.N = m->F;
            a.w = m->d_w[l];
            a.bias = m->d_bias[l];
            a.act = m->act;
            const int64_t F = m->F, ox = a.out_x, oy = a.out_y;
            a.out[0] = ConvArray{hidden[l & 1], (int64_t)n_tiles * ox * oy * F, ox * oy * F, oy * F, F, 1, 0};
        } else {
            a.N = m->NO;
            a.w = m->d_hw;
            a.bias = m->d_hb;
            a.act = FV3HIP_ACT_LINEAR;
            a.oscale = m->d_hs;
            a.ocenter = m->d_hc;
            a.och_out = m->d_och_out;
            a.och_local = m->d_och_local;
            for (int j = 0; j < m->n_outputs; ++j) {
                FV3HIP_REQUIRE(outputs[j], "output %d is null", j);
                const int64_t *s = out_strides + 5 * j;
                a.out[j] = ConvArray{outputs[j], s[0], s[1], s[2], s[3], s[4], 0};
            }
        }
        int rc = launch_layer(a, kk, S, st);
        if (rc) return rc;
        in_x = a.out_x;
        in_y = a.out_y;
    }
    return FV3HIP_OK;
}
