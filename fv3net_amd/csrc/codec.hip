// Column codecs of the reservoir models (fv3fit.reservoir.transformers: "dense-autoencoder" and "sk-transformer"),
// DESIGN.md section 19.  One launch per direction:
//
//   codec_encode_kernel<T>  a block takes tiles of `tc` columns.  Lanes walk z when they load: element i of a tile is
//                           (column i / K, feature i % K), so a wave reads a contiguous stretch of every variable.  The
//                           normalised tile goes to LDS as [tc][ldx] rows (ldx odd: the columns of a wave fall on different
//                           banks); then each layer runs one (column, unit) per lane, unit fastest: a wave reads one weight
//                           row contiguously and a handful of broadcast activations per step.  The last layer writes the
//                           latent [column][n_latent] straight to memory, coalesced.
//   codec_decode_kernel<T>  the same skeleton: the latent tile to LDS, the hidden layers, then the heads (one layer of K
//                           units) with the denormalisation, the clamp and the strided store in their epilogue.
//
// T is float for the dense autoencoder (Keras float32) and double for the affine StandardScaler + PCA codec, which is one
// linear layer per direction.  The weights of the layers that fit beside the tile are staged in LDS once per block (a block
// walks several tiles); a layer that does not fit -- a large PCA matrix, a 1024 x 256 first layer -- is read from memory,
// where it stays in L2.  A block holds at most 60 KiB of LDS, so two blocks share a CU.  Every sum is an fma chain in
// ascending input index; no atomics.
#include <algorithm>
#include <cmath>
#include <vector>

#include "columns.h"

using namespace fv3hip;

namespace {

constexpr int kMaxVars = FV3HIP_CODEC_MAX_VARIABLES;
constexpr int kMaxK = FV3HIP_CODEC_MAX_FEATURES;
constexpr int kMaxWidth = FV3HIP_CODEC_MAX_WIDTH;
constexpr int kMaxLayers = FV3HIP_CODEC_MAX_LAYERS;
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1024;       // tiles beyond this are walked by the same blocks
constexpr size_t kLdsBytes = 61440;    // per block: 60 KiB, below the 64 KiB a launch may ask for without an opt-in

__device__ __forceinline__ float fma_rn(float a, float b, float c) { return __fmaf_rn(a, b, c); }
__device__ __forceinline__ double fma_rn(double a, double b, double c) { return __fma_rn(a, b, c); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double add_rn(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ float sub_rn(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double sub_rn(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double div_rn(double a, double b) { return __ddiv_rn(a, b); }

template <class T>
struct Layer {
    const T *w;     // [in][out]
    const T *b;     // [out] or null
    const T *pdiv;  // [out] or null: the sum is divided by it (whitening)
    int in, out;
    int lds;        // offset of the staged copy (weights, then the bias) in the LDS weight region, -1: read from memory
};

// what both directions share
template <class T>
struct Net {
    Layer<T> layer[kMaxLayers + 1];
    int n_layers;
    int n_var, K, L, relu;
    int zoff[kMaxVars + 1];
    int tc, ldx, lda;  // columns per tile, LDS row lengths of the input tile and of an activation buffer
    int64_t ncol, n_tiles;
    int ny;
};

template <class T>
struct EncArgs {
    Net<T> n;
    XyzSrc src[kMaxVars];
    const T *sub, *div, *sub2;  // per feature, each optional: ((x - sub) / div) - sub2
    T *latent;
};

template <class T>
struct DecArgs {
    Net<T> n;
    const void *latent;
    int latent_f64;
    int has_head;               // the last layer is the heads (else the latent is the normalised column)
    XyzDst out[kMaxVars];
    const T *mul, *add;         // per feature, each optional: y * mul + add
    T lo[kMaxVars], hi[kMaxVars];  // per variable, NaN: no bound
    int positive;
};

// the staged copies of the layers that fit, once per block
template <class T>
__device__ __forceinline__ void stage_weights(const Net<T> &n, T *wl)
{
    for (int l = 0; l < n.n_layers; ++l) {
        const Layer<T> &ly = n.layer[l];
        if (ly.lds < 0) continue;
        const int nw = ly.in * ly.out;
        for (int i = threadIdx.x; i < nw; i += kBlock) wl[ly.lds + i] = ly.w[i];
        if (ly.b)
            for (int i = threadIdx.x; i < ly.out; i += kBlock) wl[ly.lds + nw + i] = ly.b[i];
    }
}

// acc[c][u] = sum over k ascending of h[c][k] * w[k][u]
template <class T>
__device__ __forceinline__ T dot(const T *hr, const T *w, int in, int out, int u)
{
    T acc = 0;
#pragma unroll 4
    for (int k = 0; k < in; ++k) acc = fma_rn(hr[k], w[(int64_t)k * out + u], acc);
    return acc;
}

// one layer over the nc columns of a tile: (column, unit) per lane, unit fastest
template <class T>
__device__ __forceinline__ void run_layer(const T *h, int ldh, const T *w, const T *b, const T *pdiv, int in, int out, int nc,
                                          int relu, T *dst, int64_t ldd)
{
    for (int i = threadIdx.x; i < nc * out; i += kBlock) {
        const int c = i / out, u = i - c * out;
        T acc = dot(h + c * ldh, w, in, out, u);
        if (b) acc = add_rn(acc, b[u]);
        if (relu) acc = acc < (T)0 ? (T)0 : acc;  // a NaN stays
        if (pdiv) acc = div_rn(acc, pdiv[u]);
        dst[c * ldd + u] = acc;
    }
}

template <class T>
__global__ __launch_bounds__(kBlock) void codec_encode_kernel(EncArgs<T> a)
{
    extern __shared__ __align__(16) unsigned char codec_lds[];
    const Net<T> &n = a.n;
    T *xs = reinterpret_cast<T *>(codec_lds);
    T *act0 = xs + n.tc * n.ldx;
    T *act1 = act0 + n.tc * n.lda;
    T *wl = act1 + n.tc * n.lda;
    stage_weights(n, wl);
    const int K = n.K;
    for (int64_t tile = blockIdx.x; tile < n.n_tiles; tile += gridDim.x) {
        __syncthreads();  // the weights are staged; the tile before this one is done with xs
        const int64_t c0 = tile * n.tc;
        const int nc = (int)(n.ncol - c0 < n.tc ? n.ncol - c0 : n.tc);
        for (int i = threadIdx.x; i < nc * K; i += kBlock) {
            const int c = i / K, k = i - c * K;
            const int v = var_of(n.zoff, n.n_var, k);
            const int64_t col = c0 + c;
            const int64_t x = col / n.ny, y = col - x * n.ny;
            T val = load_xyz<T>(a.src[v], x, y, k - n.zoff[v]);
            if (a.sub) val = sub_rn(val, a.sub[k]);
            if (a.div) val = div_rn(val, a.div[k]);
            if (a.sub2) val = sub_rn(val, a.sub2[k]);
            if (n.n_layers)
                xs[c * n.ldx + k] = val;
            else
                a.latent[col * n.L + k] = val;
        }
        __syncthreads();
        const T *h = xs;
        int ldh = n.ldx;
        for (int l = 0; l < n.n_layers; ++l) {
            const Layer<T> &ly = n.layer[l];
            T *dst = (l & 1) ? act1 : act0;
            const bool last = l + 1 == n.n_layers;
            // four calls, not one over selected pointers: each keeps its address spaces (LDS or global weights, LDS or
            // global destination); folded, the weights are read by flat loads and the double kernel's registers change
            if (ly.lds >= 0) {
                const T *w = wl + ly.lds;
                const T *b = ly.b ? w + ly.in * ly.out : nullptr;
                if (last)
                    run_layer(h, ldh, w, b, ly.pdiv, ly.in, ly.out, nc, n.relu, a.latent + c0 * n.L, (int64_t)n.L);
                else
                    run_layer(h, ldh, w, b, ly.pdiv, ly.in, ly.out, nc, n.relu, dst, (int64_t)n.lda);
            } else {
                if (last)
                    run_layer(h, ldh, ly.w, ly.b, ly.pdiv, ly.in, ly.out, nc, n.relu, a.latent + c0 * n.L, (int64_t)n.L);
                else
                    run_layer(h, ldh, ly.w, ly.b, ly.pdiv, ly.in, ly.out, nc, n.relu, dst, (int64_t)n.lda);
            }
            __syncthreads();
            h = dst;
            ldh = n.lda;
        }
    }
}

template <class T>
__global__ __launch_bounds__(kBlock) void codec_decode_kernel(DecArgs<T> a)
{
    extern __shared__ __align__(16) unsigned char codec_lds[];
    const Net<T> &n = a.n;
    T *act0 = reinterpret_cast<T *>(codec_lds);
    T *act1 = act0 + n.tc * n.lda;
    T *wl = act1 + n.tc * n.lda;
    stage_weights(n, wl);
    const int K = n.K, L = n.L;
    const int n_hidden = n.n_layers - (a.has_head ? 1 : 0);
    for (int64_t tile = blockIdx.x; tile < n.n_tiles; tile += gridDim.x) {
        __syncthreads();
        const int64_t c0 = tile * n.tc;
        const int nc = (int)(n.ncol - c0 < n.tc ? n.ncol - c0 : n.tc);
        for (int i = threadIdx.x; i < nc * L; i += kBlock) {
            const int c = i / L, j = i - c * L;
            const int64_t off = c0 * L + i;
            act0[c * n.lda + j] = a.latent_f64 ? (T) static_cast<const double *>(a.latent)[off]
                                               : (T) static_cast<const float *>(a.latent)[off];
        }
        __syncthreads();
        const T *h = act0;
        for (int l = 0; l < n_hidden; ++l) {
            const Layer<T> &ly = n.layer[l];
            T *dst = (l & 1) ? act0 : act1;
            if (ly.lds >= 0) {
                const T *w = wl + ly.lds;
                run_layer(h, n.lda, w, ly.b ? w + ly.in * ly.out : nullptr, ly.pdiv, ly.in, ly.out, nc, n.relu, dst,
                          (int64_t)n.lda);
            } else {
                run_layer(h, n.lda, ly.w, ly.b, ly.pdiv, ly.in, ly.out, nc, n.relu, dst, (int64_t)n.lda);
            }
            __syncthreads();
            h = dst;
        }
        // the heads (K units, linear) or the latent itself, denormalised, limited and stored
        const Layer<T> &hd = n.layer[n_hidden];
        const bool staged = a.has_head && hd.lds >= 0;
        const T *b = !a.has_head ? nullptr : staged ? (hd.b ? wl + hd.lds + hd.in * hd.out : nullptr) : hd.b;
        for (int i = threadIdx.x; i < nc * K; i += kBlock) {
            const int c = i / K, k = i - c * K;
            T yv;
            if (a.has_head) {
                yv = staged ? dot(h + c * n.lda, wl + hd.lds, hd.in, K, k) : dot(h + c * n.lda, hd.w, hd.in, K, k);
                if (b) yv = add_rn(yv, b[k]);
            } else {
                yv = h[c * n.lda + k];
            }
            if (a.mul) yv = mul_rn(yv, a.mul[k]);
            if (a.add) yv = add_rn(yv, a.add[k]);
            const int v = var_of(n.zoff, n.n_var, k);
            // OutputLimit._limit_activation: below min -> min, at or above max -> max; comparisons with a NaN are false
            T r = yv;
            if (yv < a.lo[v]) r = a.lo[v];
            if (yv >= a.hi[v]) r = a.hi[v];
            if (a.positive) r = r >= (T)0 ? r : (T)0;  // np.where(decoded >= 0, decoded, 0.0): a NaN becomes 0.0
            const int64_t col = c0 + c;
            const int64_t x = col / n.ny, y = col - x * n.ny;
            const XyzDst &o = a.out[v];
            static_cast<T *>(o.p)[x * o.sx + y * o.sy + (k - n.zoff[v]) * o.sz] = r;
        }
    }
}

template <class T>
struct HostLayer {
    std::vector<T> w, b, pdiv;
    int in = 0, out = 0;
};

// one precision of a codec: the device copies and the launch plan of both directions
template <class T>
struct Model {
    std::vector<HostLayer<T>> enc, dec;  // dec: the hidden layers, then the heads when has_head
    std::vector<T> sub, div, sub2, mul, add;
    T *d_sub = nullptr, *d_div = nullptr, *d_sub2 = nullptr, *d_mul = nullptr, *d_add = nullptr;
    Net<T> ne{}, nd{};
    size_t lds_enc = 0, lds_dec = 0;
};

}  // namespace

struct fv3hip_codec {
    int device = 0;
    int kind = 0, n_var = 0, K = 0, L = 0, has_head = 0, positive = 0;
    int zoff[kMaxVars + 1] = {0};
    double lo[kMaxVars], hi[kMaxVars];
    Model<float> f;
    Model<double> d;
    DeviceAllocs mem;
};

namespace {

// f(m->f) or f(m->d): the precision the codec computes in
template <class Fn>
int with_model(fv3hip_codec *m, Fn f)
{
    return m->kind == FV3HIP_CODEC_DENSE ? f(m->f) : f(m->d);
}

// an empty array is an absent one: a null pointer, which the kernels test
template <class T>
int to_device(fv3hip_codec *m, const std::vector<T> &host, T **dptr)
{
    *dptr = nullptr;
    return host.empty() ? FV3HIP_OK : m->mem.upload(dptr, host.data(), host.size());
}

inline int odd(int n) { return n | 1; }

// The tile and the staged layers of one direction.  `in_row`: the row length of the input tile (encode) or 0;
// `act`: the widest activation kept in LDS.
template <class T>
size_t plan(Net<T> &n, int in_row, int act)
{
    const int cap = (int)(kLdsBytes / sizeof(T));
    n.ldx = in_row ? odd(in_row) : 0;
    n.lda = act ? odd(act) : 0;
    const int per_col = n.ldx + 2 * n.lda;
    n.tc = 64;
    while (n.tc > 1 && n.tc * per_col > cap / 2) n.tc /= 2;
    int used = n.tc * per_col, w_used = 0;
    for (int l = 0; l < n.n_layers; ++l) {
        Layer<T> &ly = n.layer[l];
        const int need = ly.in * ly.out + (ly.b ? ly.out : 0);
        ly.lds = -1;
        if (used + w_used + need <= cap) {
            ly.lds = w_used;
            w_used += need;
        }
    }
    return (size_t)(used + w_used) * sizeof(T);
}

template <class T>
int upload_layers(fv3hip_codec *m, std::vector<HostLayer<T>> &host, Net<T> &n)
{
    n.n_layers = (int)host.size();
    for (size_t l = 0; l < host.size(); ++l) {
        T *w = nullptr, *b = nullptr, *p = nullptr;
        int rc;
        if ((rc = to_device(m, host[l].w, &w)) || (rc = to_device(m, host[l].b, &b)) || (rc = to_device(m, host[l].pdiv, &p)))
            return rc;
        n.layer[l] = Layer<T>{w, b, p, host[l].in, host[l].out, -1};
    }
    return FV3HIP_OK;
}

template <class T>
int finish(fv3hip_codec *m, Model<T> &mod, int relu)
{
    int rc;
    if ((rc = to_device(m, mod.sub, &mod.d_sub)) || (rc = to_device(m, mod.div, &mod.d_div)) ||
        (rc = to_device(m, mod.sub2, &mod.d_sub2)) || (rc = to_device(m, mod.mul, &mod.d_mul)) ||
        (rc = to_device(m, mod.add, &mod.d_add)))
        return rc;
    if ((rc = upload_layers(m, mod.enc, mod.ne)) || (rc = upload_layers(m, mod.dec, mod.nd))) return rc;
    for (Net<T> *n : {&mod.ne, &mod.nd}) {
        n->n_var = m->n_var;
        n->K = m->K;
        n->L = m->L;
        n->relu = relu;
        memcpy(n->zoff, m->zoff, sizeof(m->zoff));
    }
    int act_e = 0, act_d = m->L;
    for (size_t l = 0; l + 1 < mod.enc.size(); ++l) act_e = std::max(act_e, mod.enc[l].out);
    for (size_t l = 0; l + (m->has_head ? 1 : 0) < mod.dec.size(); ++l) act_d = std::max(act_d, mod.dec[l].out);
    mod.lds_enc = plan(mod.ne, mod.enc.empty() ? 0 : m->K, act_e);
    mod.lds_dec = plan(mod.nd, 0, act_d);
    return FV3HIP_OK;
}

int check_units(const char *side, int n, const int *units)
{
    FV3HIP_REQUIRE(n >= 0 && n <= kMaxLayers, "%s: %d layers exceed the cap of %d layers per side", side, n, kMaxLayers);
    FV3HIP_REQUIRE(n == 0 || units, "%s: null units", side);
    for (int l = 0; l < n; ++l)
        FV3HIP_REQUIRE(units[l] >= 1 && units[l] <= kMaxWidth, "%s layer %d: width %d is outside [1, %d] (the cap on layer "
                       "widths)", side, l, units[l], kMaxWidth);
    return FV3HIP_OK;
}

int add_layers(std::vector<HostLayer<float>> &dst, const char *side, int n, const int *units, const float *const *kernels,
               const float *const *biases, int *width)
{
    FV3HIP_REQUIRE(n == 0 || (kernels && biases), "%s: null kernels or biases", side);
    for (int l = 0; l < n; ++l) {
        FV3HIP_REQUIRE(kernels[l] && biases[l], "%s layer %d: null kernel or bias", side, l);
        HostLayer<float> h;
        h.in = *width;
        h.out = units[l];
        h.w.assign(kernels[l], kernels[l] + (size_t)h.in * h.out);
        h.b.assign(biases[l], biases[l] + h.out);
        dst.push_back(std::move(h));
        *width = units[l];
    }
    return FV3HIP_OK;
}

int build_dense(const fv3hip_codec_desc_t *d, fv3hip_codec *m)
{
    const int K = m->K;
    FV3HIP_REQUIRE(d->center && d->scale, "dense codec: null center or scale");
    int rc;
    if ((rc = check_units("encoder", d->n_enc, d->enc_units)) || (rc = check_units("decoder", d->n_dec, d->dec_units)))
        return rc;
    Model<float> &f = m->f;
    f.sub.assign(d->center, d->center + K);
    f.div.resize(K);
    for (int k = 0; k < K; ++k) f.div[k] = d->scale[k] + 1.0e-7f;  // NormLayer's forward scale, rounded once in float32
    f.mul.assign(d->scale, d->scale + K);
    f.add.assign(d->center, d->center + K);
    for (int v = 0; v < m->n_var; ++v) {
        m->lo[v] = d->out_min ? (double)d->out_min[v] : NAN;
        m->hi[v] = d->out_max ? (double)d->out_max[v] : NAN;
        FV3HIP_REQUIRE(!(m->hi[v] <= m->lo[v]), "output %d: max %g must be greater than min %g", v, m->hi[v], m->lo[v]);
    }
    if (d->n_enc == 0) {
        FV3HIP_REQUIRE(d->n_dec == 0 && !d->head_kernels, "a scale-only codec (n_enc 0) has no decoder layers or heads");
        FV3HIP_REQUIRE(d->n_latent == K, "a scale-only codec needs n_latent == K (%d), got %d", K, d->n_latent);
        m->has_head = 0;
        return FV3HIP_OK;
    }
    FV3HIP_REQUIRE(d->enc_units[d->n_enc - 1] == d->n_latent, "the last encoder layer has %d units but n_latent is %d",
                   d->enc_units[d->n_enc - 1], d->n_latent);
    FV3HIP_REQUIRE(d->head_kernels && d->head_biases, "dense codec: null head kernels or biases");
    int width = K;
    if ((rc = add_layers(f.enc, "encoder", d->n_enc, d->enc_units, d->enc_kernels, d->enc_biases, &width))) return rc;
    width = d->n_latent;
    if ((rc = add_layers(f.dec, "decoder", d->n_dec, d->dec_units, d->dec_kernels, d->dec_biases, &width))) return rc;
    // the heads side by side: one layer of K units
    HostLayer<float> h;
    h.in = width;
    h.out = K;
    h.w.resize((size_t)width * K);
    h.b.resize(K);
    for (int v = 0; v < m->n_var; ++v) {
        FV3HIP_REQUIRE(d->head_kernels[v] && d->head_biases[v], "head %d: null kernel or bias", v);
        const int nz = m->zoff[v + 1] - m->zoff[v];
        for (int i = 0; i < width; ++i)
            for (int z = 0; z < nz; ++z) h.w[(size_t)i * K + m->zoff[v] + z] = d->head_kernels[v][(size_t)i * nz + z];
        for (int z = 0; z < nz; ++z) h.b[m->zoff[v] + z] = d->head_biases[v][z];
    }
    f.dec.push_back(std::move(h));
    m->has_head = 1;
    return FV3HIP_OK;
}

int build_affine(const fv3hip_codec_desc_t *d, fv3hip_codec *m)
{
    const int K = m->K, L = m->L;
    FV3HIP_REQUIRE(d->pca_mean && d->components, "affine codec: null pca_mean or components");
    Model<double> &a = m->d;
    if (d->mean) {
        a.sub.assign(d->mean, d->mean + K);
        a.add.assign(d->mean, d->mean + K);
    }
    if (d->std) {
        a.div.assign(d->std, d->std + K);
        a.mul.assign(d->std, d->std + K);
    }
    a.sub2.assign(d->pca_mean, d->pca_mean + K);
    HostLayer<double> e, h;
    e.in = K;
    e.out = L;
    e.w.resize((size_t)K * L);
    h.in = L;
    h.out = K;
    h.w.resize((size_t)L * K);
    h.b.assign(d->pca_mean, d->pca_mean + K);
    if (d->explained_variance) e.pdiv.resize(L);
    for (int j = 0; j < L; ++j) {
        const double s = d->explained_variance ? std::sqrt(d->explained_variance[j]) : 1.0;
        if (d->explained_variance) e.pdiv[j] = s;
        for (int k = 0; k < K; ++k) {
            const double c = d->components[(size_t)j * K + k];
            e.w[(size_t)k * L + j] = c;
            h.w[(size_t)j * K + k] = d->explained_variance ? s * c : c;
        }
    }
    a.enc.push_back(std::move(e));
    a.dec.push_back(std::move(h));
    m->has_head = 1;
    m->positive = d->enforce_positive ? 1 : 0;
    for (int v = 0; v < m->n_var; ++v) m->lo[v] = m->hi[v] = NAN;
    return FV3HIP_OK;
}

int build(const fv3hip_codec_desc_t *d, fv3hip_codec *m)
{
    FV3HIP_REQUIRE(d, "null descriptor");
    FV3HIP_REQUIRE(d->kind == FV3HIP_CODEC_DENSE || d->kind == FV3HIP_CODEC_AFFINE, "unknown codec kind %d", d->kind);
    const int rc = fill_zoff(d->var_nz, d->n_variables, kMaxVars, "", m->zoff);
    if (rc) return rc;
    m->kind = d->kind;
    m->n_var = d->n_variables;
    const int K = m->zoff[m->n_var];
    FV3HIP_REQUIRE(K <= kMaxK, "K = sum(var_nz) = %d exceeds the cap of %d features", K, kMaxK);
    FV3HIP_REQUIRE(d->n_latent >= 1 && (d->n_latent <= kMaxWidth || (d->kind == FV3HIP_CODEC_DENSE && d->n_enc == 0)),
                   "n_latent %d is outside [1, %d] (the cap on n_latent)", d->n_latent, kMaxWidth);
    m->K = K;
    m->L = d->n_latent;
    return d->kind == FV3HIP_CODEC_DENSE ? build_dense(d, m) : build_affine(d, m);
}

int check_device(fv3hip_codec_t m)
{
    FV3HIP_REQUIRE(m, "null codec handle");
    return check_handle_device(m->device, "codec");
}

int check_extent(int nx, int ny)
{
    FV3HIP_REQUIRE(nx >= 1 && ny >= 1 && (int64_t)nx * ny < (1 << 28), "bad extent (%d, %d)", nx, ny);
    return FV3HIP_OK;
}

template <class T>
void set_extent(Net<T> &n, int nx, int ny)
{
    n.ncol = (int64_t)nx * ny;
    n.ny = ny;
    n.n_tiles = ceil_div(n.ncol, n.tc);
}

template <class T>
int launch_encode(fv3hip_codec_t m, Model<T> &mod, const void *const *sources, const int *src_dtype, const int64_t *strides,
                  int nx, int ny, void *latent, hipStream_t st)
{
    EncArgs<T> a{};
    const int rc = fill_sources(m->n_var, sources, src_dtype, strides, 3, 0, a.src, nullptr);
    if (rc) return rc;
    a.n = mod.ne;
    set_extent(a.n, nx, ny);
    a.sub = mod.d_sub;
    a.div = mod.d_div;
    a.sub2 = mod.d_sub2;
    a.latent = static_cast<T *>(latent);
    const unsigned grid = (unsigned)(a.n.n_tiles < kMaxBlocks ? a.n.n_tiles : kMaxBlocks);
    hipLaunchKernelGGL(codec_encode_kernel<T>, dim3(grid), dim3(kBlock), mod.lds_enc, st, a);
    return check_launch("codec_encode_kernel");
}

template <class T>
int launch_decode(fv3hip_codec_t m, Model<T> &mod, const void *latent, int latent_dtype, int nx, int ny, void *const *outputs,
                  const int64_t *out_strides, hipStream_t st)
{
    DecArgs<T> a{};
    const int rc = fill_outputs(m->n_var, outputs, out_strides, a.out);
    if (rc) return rc;
    a.n = mod.nd;
    set_extent(a.n, nx, ny);
    a.latent = latent;
    a.latent_f64 = latent_dtype == FV3HIP_F64 ? 1 : 0;
    a.has_head = m->has_head;
    for (int v = 0; v < m->n_var; ++v) {
        a.lo[v] = (T)m->lo[v];
        a.hi[v] = (T)m->hi[v];
    }
    a.mul = mod.d_mul;
    a.add = mod.d_add;
    a.positive = m->positive;
    const unsigned grid = (unsigned)(a.n.n_tiles < kMaxBlocks ? a.n.n_tiles : kMaxBlocks);
    hipLaunchKernelGGL(codec_decode_kernel<T>, dim3(grid), dim3(kBlock), mod.lds_dec, st, a);
    return check_launch("codec_decode_kernel");
}

}  // namespace

extern "C" int fv3hip_codec_create(const fv3hip_codec_desc_t *desc, fv3hip_codec_t *out)
{
    FV3HIP_REQUIRE(out, "null output handle");
    *out = nullptr;
    fv3hip_codec *m = new fv3hip_codec();
    int rc = build(desc, m);  // host checks only
    if (!rc) {
        hipError_t e = hipGetDevice(&m->device);
        if (e != hipSuccess) rc = fail(FV3HIP_EHIP, "hipGetDevice failed: %s", hipGetErrorString(e));
    }
    if (!rc) rc = m->kind == FV3HIP_CODEC_DENSE ? finish(m, m->f, 1) : finish(m, m->d, 0);
    if (rc) {
        fv3hip_codec_destroy(m);
        return rc;
    }
    *out = m;
    return FV3HIP_OK;
}

extern "C" int fv3hip_codec_destroy(fv3hip_codec_t m)
{
    delete m;  // its DeviceAllocs frees the buffers
    return FV3HIP_OK;
}

extern "C" int fv3hip_codec_encode(fv3hip_codec_t m, const void *const *sources, const int *src_dtype, const int64_t *strides,
                                   int nx, int ny, void *latent, void *stream)
{
    int rc = check_device(m);
    if (rc || (rc = check_extent(nx, ny))) return rc;
    FV3HIP_REQUIRE(sources && src_dtype && strides, "null source pointer");  // the first check, before the latent's
    FV3HIP_REQUIRE(latent, "null latent");
    return with_model(m, [&](auto &mod) {
        return launch_encode(m, mod, sources, src_dtype, strides, nx, ny, latent, as_stream(stream));
    });
}

extern "C" int fv3hip_codec_decode(fv3hip_codec_t m, const void *latent, int latent_dtype, int nx, int ny,
                                   void *const *outputs, const int64_t *out_strides, void *stream)
{
    int rc = check_device(m);
    if (rc || (rc = check_extent(nx, ny))) return rc;
    FV3HIP_REQUIRE(latent, "null latent");
    FV3HIP_REQUIRE(is_float(latent_dtype), "latent dtype must be F32 or F64");
    return with_model(m, [&](auto &mod) {
        return launch_decode(m, mod, latent, latent_dtype, nx, ny, outputs, out_strides, as_stream(stream));
    });
}
