// Random-forest regression (fv3fit.sklearn.RandomForest; sklearn's RandomForestRegressor / ExtraTreesRegressor .predict),
// bit-identical to sklearn: float32 inputs, float32 thresholds that route every float32 like sklearn's float64 ones,
// float64 leaf values summed in tree order, divided by the tree count, then y * std + mean (no FMA: -ffp-contract=off).
//
// Two kernels per slab of samples:
//   forest_walk_kernel  one lane per (sample, tree), the tree wave-uniform, so the top levels of a tree are broadcast
//                       loads; the inputs are read (and cast to float32) straight from the caller's strided arrays;
//                       writes the leaf's row of the value table (predict) or sklearn's node id (apply), [tree][sample].
//   forest_sum_kernel   one lane per (sample, pair of outputs): lanes of a sample read a leaf row together in 16-byte
//                       loads, eight trees' rows in flight, added in tree order in registers.  No atomics: the bits do
//                       not depend on the slab, the grid or the sample count.
#include <vector>

#include "common.h"

using namespace fv3hip;

namespace {

constexpr int kMaxForestSources = 32;
constexpr int kMaxForestOutputs = 32;
constexpr int kWalkBlock = 256;
constexpr int kSumBlock = 256;
constexpr int kSumAhead = 8;                               // leaf rows in flight per lane
constexpr size_t kLeafScratchBytes = (size_t)128 << 20;    // [tree][slab] leaf rows of one slab
constexpr int kMaxTreeGridY = 65535;

// 16-byte node record.  Internal: a / b = global ids of the left / right child, code = source << 24 | feature within the
// source (the clip start included) | missing-goes-left << 30.  Leaf: code = -1, a = row of the value table, b = the
// tree-local (sklearn) node id.
struct alignas(16) Node {
    int32_t a, b, code;
    float thr;
};

struct Src {
    const void *p;
    int64_t fs, ss;
    int64_t f64;
};

struct WalkArgs {
    const Node *nodes;
    const int64_t *root;   // [T] global id of each tree's root
    const int32_t *depth;  // [T]
    int32_t *leaf;         // [tree][ld]
    int64_t ld;
    int64_t n;             // samples of this launch
    int64_t s0;            // first sample (source offset)
    int t0;                // first tree of this launch
    Src src[kMaxForestSources];
};

struct SumArgs {
    const double *table;   // [rows][row_stride]
    const int32_t *leaf;   // [tree][ld]
    const int32_t *omap;   // [n_out] output << 24 | feature within the output
    const double *mean, *std;
    int64_t ld;
    int64_t n;             // samples of this slab
    int64_t s0;
    int T, n_out, row_stride, n_vec;
    void *out[kMaxForestOutputs];
    int64_t out_fs[kMaxForestOutputs], out_ss[kMaxForestOutputs];
};

__device__ __forceinline__ float load_input(const Src &s, int feat, int64_t sample)
{
    const int64_t off = (int64_t)feat * s.fs + sample * s.ss;
    // numpy astype(float32): round to nearest even, NaN stays NaN
    return s.f64 ? (float)static_cast<const double *>(s.p)[off] : static_cast<const float *>(s.p)[off];
}

template <bool APPLY>
__global__ __launch_bounds__(kWalkBlock) void forest_walk_kernel(WalkArgs a)
{
    const int64_t s = (int64_t)blockIdx.x * kWalkBlock + threadIdx.x;
    const int t = a.t0 + (int)blockIdx.y;
    if (s >= a.n) return;
    int64_t node = a.root[t];
    const int depth = a.depth[t];
    int32_t result = APPLY ? -1 : 0;  // (unreachable: create() checked that every walk ends at a leaf within `depth`)
    for (int d = 0; d <= depth; ++d) {
        const Node nd = a.nodes[node];
        if (nd.code < 0) {
            result = APPLY ? nd.b : nd.a;
            break;
        }
        const float x = load_input(a.src[(nd.code >> 24) & 63], nd.code & 0xffffff, a.s0 + s);
        const bool left = (x != x) ? ((nd.code >> 30) & 1) : (x <= nd.thr);
        node = left ? nd.a : nd.b;
    }
    a.leaf[(int64_t)t * a.ld + s] = result;
}

template <int VEC>
struct VecT;
template <>
struct VecT<1> {
    using type = double;
};
template <>
struct VecT<2> {
    using type = double2;
};

template <int VEC>
__device__ __forceinline__ void add_in(double (&acc)[VEC], const typename VecT<VEC>::type &v);
template <>
__device__ __forceinline__ void add_in<1>(double (&acc)[1], const double &v)
{
    acc[0] += v;
}
template <>
__device__ __forceinline__ void add_in<2>(double (&acc)[2], const double2 &v)
{
    acc[0] += v.x;
    acc[1] += v.y;
}

template <int VEC>
__global__ __launch_bounds__(kSumBlock) void forest_sum_kernel(SumArgs a)
{
    using V = typename VecT<VEC>::type;
    const int64_t item = (int64_t)blockIdx.x * kSumBlock + threadIdx.x;
    const int64_t s = item / a.n_vec;
    const int p = (int)(item - s * a.n_vec);
    if (s >= a.n) return;
    const int32_t *lf = a.leaf + s;
    const V *tab = reinterpret_cast<const V *>(a.table) + p;
    const int rs = a.row_stride / VEC;
    double acc[VEC];
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
    int t = 0;
    for (; t + kSumAhead <= a.T; t += kSumAhead) {
        int32_t r[kSumAhead];
        V v[kSumAhead];
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) r[u] = lf[(int64_t)(t + u) * a.ld];
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) v[u] = tab[(int64_t)r[u] * rs];
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) add_in<VEC>(acc, v[u]);  // tree order
    }
    for (; t < a.T; ++t) add_in<VEC>(acc, tab[(int64_t)lf[(int64_t)t * a.ld] * rs]);
    const double T = (double)a.T;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int f = p * VEC + e;
        if (f >= a.n_out) break;
        double y = acc[e] / T;      // ForestRegressor.predict: y_hat /= len(estimators_)
        y = y * a.std[f];           // StandardScaler.denormalize: two roundings
        y = y + a.mean[f];
        const int32_t m = a.omap[f];
        const int j = m >> 24, fj = m & 0xffffff;
        static_cast<double *>(a.out[j])[(int64_t)fj * a.out_fs[j] + (a.s0 + s) * a.out_ss[j]] = y;
    }
}

}  // namespace

struct fv3hip_forest {
    int device = 0;
    int T = 0, n_sources = 0, n_outputs = 0, n_out = 0, row_stride = 0;
    int64_t n_nodes = 0;
    Node *d_nodes = nullptr;
    int64_t *d_root = nullptr;
    int32_t *d_depth = nullptr;
    double *d_table = nullptr;
    int32_t *d_omap = nullptr;
    double *d_mean = nullptr, *d_std = nullptr;
    int32_t *d_leaf = nullptr;  // scratch, grown on demand
    size_t leaf_bytes = 0;
};

namespace {

template <class T>
int upload(T **dptr, const std::vector<T> &v)
{
    FV3HIP_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(dptr), v.size() * sizeof(T)));
    FV3HIP_CHECK_HIP(hipMemcpy(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return FV3HIP_OK;
}

// Everything the device copy needs, checked on the host before any HIP call.
struct HostForest {
    std::vector<Node> nodes;
    std::vector<int64_t> root;
    std::vector<int32_t> depth;
    std::vector<double> table;
    std::vector<int32_t> omap;
    std::vector<double> mean, std_;
    int K = 0, n_out = 0, row_stride = 0;
};

int build_host(const fv3hip_forest_desc_t *d, HostForest &h)
{
    FV3HIP_REQUIRE(d, "null descriptor");
    FV3HIP_REQUIRE(d->n_trees >= 1, "a forest needs at least one tree (n_trees = %d)", d->n_trees);
    FV3HIP_REQUIRE(d->node_offset && d->children_left && d->children_right && d->feature && d->threshold &&
                       d->missing_go_to_left && d->leaf_row && d->leaf_values && d->mean && d->std,
                   "null array in the forest descriptor");
    FV3HIP_REQUIRE(d->n_sources >= 1 && d->n_sources <= kMaxForestSources, "n_sources must be in [1, %d], got %d",
                   kMaxForestSources, d->n_sources);
    FV3HIP_REQUIRE(d->src_feat_start && d->src_nfeat, "null source feature ranges");
    FV3HIP_REQUIRE(d->n_outputs >= 1 && d->n_outputs <= kMaxForestOutputs, "n_outputs must be in [1, %d], got %d",
                   kMaxForestOutputs, d->n_outputs);
    FV3HIP_REQUIRE(d->out_nfeat, "null out_nfeat");
    // packed feature k -> (source, feature within the source)
    std::vector<int32_t> fmap;
    for (int i = 0; i < d->n_sources; ++i) {
        FV3HIP_REQUIRE(d->src_nfeat[i] >= 1 && d->src_feat_start[i] >= 0 &&
                           (int64_t)d->src_feat_start[i] + d->src_nfeat[i] <= (1 << 24),
                       "bad feature range [%d, %d + %d) of source %d", d->src_feat_start[i], d->src_feat_start[i],
                       d->src_nfeat[i], i);
        for (int k = 0; k < d->src_nfeat[i]; ++k) fmap.push_back((i << 24) | (d->src_feat_start[i] + k));
    }
    h.K = (int)fmap.size();
    for (int j = 0; j < d->n_outputs; ++j) {
        FV3HIP_REQUIRE(d->out_nfeat[j] >= 1 && d->out_nfeat[j] < (1 << 24), "bad out_nfeat[%d] = %d", j, d->out_nfeat[j]);
        for (int f = 0; f < d->out_nfeat[j]; ++f) h.omap.push_back((j << 24) | f);
    }
    h.n_out = (int)h.omap.size();
    FV3HIP_REQUIRE(d->n_leaf_rows >= 1, "the leaf value table is empty");
    const int T = d->n_trees;
    FV3HIP_REQUIRE(d->node_offset[0] == 0, "node_offset[0] must be 0");
    for (int t = 0; t < T; ++t)
        FV3HIP_REQUIRE(d->node_offset[t + 1] > d->node_offset[t] && d->node_offset[t + 1] - d->node_offset[t] < ((int64_t)1 << 31),
                       "tree %d has no nodes (or too many)", t);
    const int64_t N = d->node_offset[T];
    h.nodes.resize(N);
    h.root.resize(T);
    h.depth.resize(T);
    std::vector<int32_t> dep;
    for (int t = 0; t < T; ++t) {
        const int64_t o = d->node_offset[t];
        const int64_t nt = d->node_offset[t + 1] - o;
        dep.assign(nt, 0);
        int maxd = 0;
        for (int64_t i = 0; i < nt; ++i) {
            const int32_t l = d->children_left[o + i], r = d->children_right[o + i];
            Node &nd = h.nodes[o + i];
            if (l == -1) {  // sklearn's TREE_LEAF
                const int32_t row = d->leaf_row[o + i];
                FV3HIP_REQUIRE(row >= 0 && row < d->n_leaf_rows, "tree %d node %lld: leaf row %d is outside [0, %lld)", t,
                               (long long)i, row, (long long)d->n_leaf_rows);
                nd = Node{row, (int32_t)i, -1, 0.f};
                continue;
            }
            // children numbered after their parent: every walk moves to larger ids and ends
            FV3HIP_REQUIRE(l > i && r > i && l < nt && r < nt, "tree %d node %lld: children %d, %d must lie in (%lld, %lld)", t,
                           (long long)i, l, r, (long long)i, (long long)nt);
            const int32_t k = d->feature[o + i];
            FV3HIP_REQUIRE(k >= 0 && k < h.K, "tree %d node %lld: feature %d is outside [0, %d)", t, (long long)i, k, h.K);
            nd = Node{(int32_t)(o + l), (int32_t)(o + r), fmap[k] | (d->missing_go_to_left[o + i] ? (1 << 30) : 0),
                      d->threshold[o + i]};
            dep[l] = dep[l] > dep[i] + 1 ? dep[l] : dep[i] + 1;
            dep[r] = dep[r] > dep[i] + 1 ? dep[r] : dep[i] + 1;
            maxd = maxd > dep[i] + 1 ? maxd : dep[i] + 1;
        }
        h.root[t] = o;
        h.depth[t] = maxd;
    }
    FV3HIP_REQUIRE(N < ((int64_t)1 << 31), "the forest has %lld nodes, at most 2^31 - 1 are supported", (long long)N);
    // leaf table: rows padded to an even length for 16-byte loads (one output: no padding)
    h.row_stride = h.n_out == 1 ? 1 : (h.n_out + 1) / 2 * 2;
    h.table.assign((size_t)d->n_leaf_rows * h.row_stride, 0.0);
    for (int64_t r = 0; r < d->n_leaf_rows; ++r)
        for (int f = 0; f < h.n_out; ++f) h.table[(size_t)r * h.row_stride + f] = d->leaf_values[(size_t)r * h.n_out + f];
    h.mean.assign(d->mean, d->mean + h.n_out);
    h.std_.assign(d->std, d->std + h.n_out);
    return FV3HIP_OK;
}

int check_call(fv3hip_forest_t f, const void *const *sources, const int *src_dtype, const int64_t *fs, const int64_t *ss,
               int64_t n, Src *src)
{
    FV3HIP_REQUIRE(f, "null forest handle");
    FV3HIP_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "n_samples must be in [0, 2^31), got %lld", (long long)n);
    int cur = -1;
    FV3HIP_CHECK_HIP(hipGetDevice(&cur));
    FV3HIP_REQUIRE(cur == f->device, "the forest lives on device %d but the current device is %d: make the forest's "
                   "device current around the call", f->device, cur);
    FV3HIP_REQUIRE(sources && src_dtype && fs && ss, "null pointer");
    for (int i = 0; i < kMaxForestSources; ++i) src[i] = Src{nullptr, 0, 0, 0};
    for (int i = 0; i < f->n_sources; ++i) {
        FV3HIP_REQUIRE(sources[i] || n == 0, "source %d is null", i);  // (an empty array has no address)
        FV3HIP_REQUIRE(src_dtype[i] == FV3HIP_F32 || src_dtype[i] == FV3HIP_F64, "source %d: dtype must be F32 or F64", i);
        src[i] = Src{sources[i], fs[i], ss[i], src_dtype[i] == FV3HIP_F64 ? 1 : 0};
    }
    return FV3HIP_OK;
}

int launch_walk(fv3hip_forest_t f, bool apply, WalkArgs &a, hipStream_t st)
{
    a.nodes = f->d_nodes;
    a.root = f->d_root;
    a.depth = f->d_depth;
    const unsigned gx = (unsigned)ceil_div(a.n, kWalkBlock);
    for (int t0 = 0; t0 < f->T; t0 += kMaxTreeGridY) {
        a.t0 = t0;
        const unsigned gy = (unsigned)(f->T - t0 < kMaxTreeGridY ? f->T - t0 : kMaxTreeGridY);
        if (apply)
            hipLaunchKernelGGL(forest_walk_kernel<true>, dim3(gx, gy), dim3(kWalkBlock), 0, st, a);
        else
            hipLaunchKernelGGL(forest_walk_kernel<false>, dim3(gx, gy), dim3(kWalkBlock), 0, st, a);
        int rc = check_launch("forest_walk_kernel");
        if (rc) return rc;
    }
    return FV3HIP_OK;
}

}  // namespace

extern "C" int fv3hip_forest_create(const fv3hip_forest_desc_t *desc, fv3hip_forest_t *out)
{
    FV3HIP_REQUIRE(out, "null output handle");
    *out = nullptr;
    HostForest h;
    int rc = build_host(desc, h);
    if (rc) return rc;
    fv3hip_forest *f = new fv3hip_forest();
    f->T = desc->n_trees;
    f->n_sources = desc->n_sources;
    f->n_outputs = desc->n_outputs;
    f->n_out = h.n_out;
    f->row_stride = h.row_stride;
    f->n_nodes = (int64_t)h.nodes.size();
    rc = [&]() -> int {
        FV3HIP_CHECK_HIP(hipGetDevice(&f->device));
        int r;
        if ((r = upload(&f->d_nodes, h.nodes)) || (r = upload(&f->d_root, h.root)) || (r = upload(&f->d_depth, h.depth)) ||
            (r = upload(&f->d_table, h.table)) || (r = upload(&f->d_omap, h.omap)) || (r = upload(&f->d_mean, h.mean)) ||
            (r = upload(&f->d_std, h.std_)))
            return r;
        return FV3HIP_OK;
    }();
    if (rc) {
        fv3hip_forest_destroy(f);
        return rc;
    }
    *out = f;
    return FV3HIP_OK;
}

extern "C" int fv3hip_forest_destroy(fv3hip_forest_t f)
{
    if (!f) return FV3HIP_OK;
    for (void *q : {(void *)f->d_nodes, (void *)f->d_root, (void *)f->d_depth, (void *)f->d_table, (void *)f->d_omap,
                    (void *)f->d_mean, (void *)f->d_std, (void *)f->d_leaf})
        if (q) (void)hipFree(q);
    delete f;
    return FV3HIP_OK;
}

extern "C" int fv3hip_forest_apply(fv3hip_forest_t f, const void *const *sources, const int *src_dtype,
                                   const int64_t *src_feat_stride, const int64_t *src_sample_stride, int64_t n_samples,
                                   int32_t *leaf_node, void *stream)
{
    WalkArgs a;
    memset(&a, 0, sizeof(a));
    int rc = check_call(f, sources, src_dtype, src_feat_stride, src_sample_stride, n_samples, a.src);
    if (rc) return rc;
    if (n_samples == 0) return FV3HIP_OK;
    FV3HIP_REQUIRE(leaf_node, "null leaf_node");
    a.leaf = leaf_node;
    a.ld = n_samples;
    a.n = n_samples;
    a.s0 = 0;
    return launch_walk(f, true, a, as_stream(stream));
}

extern "C" int fv3hip_forest_predict(fv3hip_forest_t f, const void *const *sources, const int *src_dtype,
                                     const int64_t *src_feat_stride, const int64_t *src_sample_stride, int64_t n_samples,
                                     double *const *outputs, const int64_t *out_feat_stride,
                                     const int64_t *out_sample_stride, void *stream)
{
    WalkArgs a;
    memset(&a, 0, sizeof(a));
    int rc = check_call(f, sources, src_dtype, src_feat_stride, src_sample_stride, n_samples, a.src);
    if (rc) return rc;
    if (n_samples == 0) return FV3HIP_OK;
    FV3HIP_REQUIRE(outputs && out_feat_stride && out_sample_stride, "null pointer");
    SumArgs b;
    memset(&b, 0, sizeof(b));
    for (int j = 0; j < f->n_outputs; ++j) {
        FV3HIP_REQUIRE(outputs[j], "output %d is null", j);
        b.out[j] = outputs[j];
        b.out_fs[j] = out_feat_stride[j];
        b.out_ss[j] = out_sample_stride[j];
    }
    // slabs of samples whose [tree][sample] leaf rows fit the scratch
    int64_t slab = (int64_t)(kLeafScratchBytes / ((size_t)f->T * sizeof(int32_t)));
    slab = slab < kWalkBlock ? kWalkBlock : slab;
    slab = slab > n_samples ? n_samples : slab;
    const size_t need = (size_t)f->T * slab * sizeof(int32_t);
    if ((rc = grow(reinterpret_cast<void **>(&f->d_leaf), &f->leaf_bytes, need))) return rc;
    const hipStream_t st = as_stream(stream);
    const int vec = f->n_out == 1 ? 1 : 2;
    b.table = f->d_table;
    b.leaf = f->d_leaf;
    b.omap = f->d_omap;
    b.mean = f->d_mean;
    b.std = f->d_std;
    b.T = f->T;
    b.n_out = f->n_out;
    b.row_stride = f->row_stride;
    b.n_vec = (f->n_out + vec - 1) / vec;
    a.leaf = f->d_leaf;
    for (int64_t s0 = 0; s0 < n_samples; s0 += slab) {
        const int64_t n = n_samples - s0 < slab ? n_samples - s0 : slab;
        a.ld = n;
        a.n = n;
        a.s0 = s0;
        rc = launch_walk(f, false, a, st);
        if (rc) return rc;
        b.ld = n;
        b.n = n;
        b.s0 = s0;
        const unsigned gx = (unsigned)ceil_div(n * b.n_vec, kSumBlock);
        if (vec == 1)
            hipLaunchKernelGGL(forest_sum_kernel<1>, dim3(gx), dim3(kSumBlock), 0, st, b);
        else
            hipLaunchKernelGGL(forest_sum_kernel<2>, dim3(gx), dim3(kSumBlock), 0, st, b);
        rc = check_launch("forest_sum_kernel");
        if (rc) return rc;
    }
    return FV3HIP_OK;
}
