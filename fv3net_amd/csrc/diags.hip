// Reductions of the offline diagnostics (workflows/diagnostics/fv3net/diagnostics/offline/compute_diagnostics.py with
// _shared/transform.py, vcm/select.py, vcm/calc/histogram.py): sums per (group, level) over an indexed cell list, and
// np.histogram / np.histogram2d with explicit edges.
//
// group sums: a plan (ops.group_plan) lists the cells of every group contiguously in `order` and cuts every group into
// work items of at most kGsChunk cells.  One workgroup reduces one item on one level: each thread adds its cells in
// thread-stride order, the 64 lanes of a wave are folded by a fixed shuffle tree, the four waves are added in wave order
// and the ten partial sums are written with plain stores.  A second kernel adds a group's items in item order.  No
// floating-point atomic takes part, so a result depends on the plan alone and is bitwise identical from run to run.
//
// histograms: edges and per-workgroup integer counters live in LDS; a value's bin is found by bisection and counted with
// an LDS integer atomic; every workgroup then adds its non-zero counters to the global int64 counts with one integer
// atomic each (integer adds are exact, so the order does not matter).
#include "common.h"

namespace fv3hip {
namespace {

constexpr int kGsThreads = 256;
constexpr int kGsChunk = 2048;  // cells per work item: eight per thread
constexpr int kGsStats = 10;

constexpr int kHistThreads = 1024;
constexpr int kHistMaxBins = 4096;
constexpr int kHist2dMaxBins = 128;  // per axis

// nansum: a term enters its sum unless it is NaN (an infinity stays)
__device__ __forceinline__ void add_term(double &acc, double t)
{
    acc += (t == t) ? t : 0.0;
}

template <typename TA, typename TW, bool HAS_B, bool HAS_W>
__global__ __launch_bounds__(kGsThreads) void group_sums_items_kernel(
    const TA *__restrict__ a, const TA *__restrict__ b, const TW *__restrict__ w, int64_t n_batch, int nz, int64_t n_inner,
    const int32_t *__restrict__ order, int64_t n_order, const int64_t *__restrict__ start, int64_t n_groups,
    const int32_t *__restrict__ item_group, const int32_t *__restrict__ item_chunk, double *__restrict__ partial)
{
    const int64_t item = blockIdx.x;
    const int z = blockIdx.y;
    double acc[kGsStats];
#pragma unroll
    for (int s = 0; s < kGsStats; ++s) acc[s] = 0.0;

    const int64_t g = item_group[item];
    if (g >= 0 && g < n_groups) {
        int64_t lo = start[g] + (int64_t)item_chunk[item] * kGsChunk;
        int64_t hi = lo + kGsChunk;
        const int64_t g_end = start[g + 1];
        if (hi > g_end) hi = g_end;
        if (lo < 0) lo = 0;
        if (hi > n_order) hi = n_order;
        const int64_t n_cells = n_batch * n_inner;
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll 4
        for (int64_t p = lo + threadIdx.x; p < hi; p += kGsThreads) {
            int64_t c = order[p];
            const bool valid = c >= 0 && c < n_cells;  // (a cell id outside the arrays counts for nothing)
            c = valid ? c : 0;
            int64_t idx;
            if (n_batch == 1) {
                idx = (int64_t)z * n_inner + c;
            } else {
                const int64_t bt = c / n_inner;
                idx = (bt * nz + z) * n_inner + (c - bt * n_inner);
            }
            double wv = HAS_W ? (double)w[c] : 1.0;
            wv = valid ? wv : nan;  // a NaN weight: every term below is NaN and is skipped
            const double av = (double)a[idx];
            add_term(acc[0], wv);
            add_term(acc[1], (av == av) ? wv : nan);
            const double wa = wv * av;
            add_term(acc[2], wa);
            add_term(acc[3], wa * av);
            if (HAS_B) {
                const double bv = (double)b[idx];
                const double d = av - bv;
                add_term(acc[4], (bv == bv) ? wv : nan);
                const double wb = wv * bv;
                add_term(acc[5], wb);
                add_term(acc[6], wb * bv);
                add_term(acc[7], (d == d) ? wv : nan);
                const double wd = wv * d;
                add_term(acc[8], wd);
                add_term(acc[9], wd * d);
            }
        }
    }

    // fixed tree: lanes by shuffle, then the four waves in wave order
    __shared__ double wave_sums[kGsThreads / kWave][kGsStats];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int s = 0; s < kGsStats; ++s) {
        double v = acc[s];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
        if (lane == 0) wave_sums[wave][s] = v;
    }
    __syncthreads();
    if (threadIdx.x < kGsStats) {
        double v = wave_sums[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < kGsThreads / kWave; ++k) v += wave_sums[k][threadIdx.x];
        partial[(item * nz + z) * kGsStats + threadIdx.x] = v;
    }
}

// sums[s][g][z] = the partial sums of group g's items, added in item order
__global__ __launch_bounds__(256) void group_sums_finish_kernel(const double *__restrict__ partial,
                                                                const int64_t *__restrict__ group_item, int64_t n_groups, int nz,
                                                                int64_t n_items, double *__restrict__ sums)
{
    const int64_t total = n_groups * nz * kGsStats;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int s = (int)(t % kGsStats);
        const int64_t gz = t / kGsStats;
        const int z = (int)(gz % nz);
        const int64_t g = gz / nz;
        int64_t i0 = group_item[g], i1 = group_item[g + 1];
        if (i0 < 0) i0 = 0;
        if (i1 > n_items) i1 = n_items;
        double v = 0.0;
        for (int64_t i = i0; i < i1; ++i) v += partial[(i * nz + z) * kGsStats + s];
        sums[((int64_t)s * n_groups + g) * nz + z] = v;
    }
}

// np.histogram with array bins: bin i holds edges[i] <= v < edges[i + 1], the last one also v == edges[n_bins];
// -1: NaN or outside
__device__ __forceinline__ int find_bin(const double *edges, int n_bins, double v)
{
    if (!(v >= edges[0]) || !(v <= edges[n_bins])) return -1;
    if (v == edges[n_bins]) return n_bins - 1;
    int lo = 0, hi = n_bins;  // edges[lo] <= v < edges[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <typename T>
__global__ __launch_bounds__(kHistThreads) void histogram_kernel(const T *__restrict__ x, int64_t n, const double *__restrict__ edges,
                                                                 int n_bins, unsigned long long *__restrict__ counts)
{
    __shared__ double s_edges[kHistMaxBins + 1];
    __shared__ unsigned int s_counts[kHistMaxBins];
    for (int i = threadIdx.x; i <= n_bins; i += kHistThreads) s_edges[i] = edges[i];
    for (int i = threadIdx.x; i < n_bins; i += kHistThreads) s_counts[i] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kHistThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kHistThreads) {
        const int bin = find_bin(s_edges, n_bins, (double)x[i]);
        if (bin >= 0) atomicAdd(&s_counts[bin], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_bins; i += kHistThreads) {
        const unsigned int c = s_counts[i];
        if (c) atomicAdd(&counts[i], (unsigned long long)c);
    }
}

template <typename T>
__global__ __launch_bounds__(kHistThreads) void histogram2d_kernel(const T *__restrict__ x, const T *__restrict__ y, int64_t n,
                                                                   const double *__restrict__ xedges, int nx_bins,
                                                                   const double *__restrict__ yedges, int ny_bins,
                                                                   unsigned long long *__restrict__ counts)
{
    __shared__ double s_xe[kHist2dMaxBins + 1];
    __shared__ double s_ye[kHist2dMaxBins + 1];
    __shared__ unsigned int s_counts[kHist2dMaxBins * kHist2dMaxBins];
    const int n_cells = nx_bins * ny_bins;
    for (int i = threadIdx.x; i <= nx_bins; i += kHistThreads) s_xe[i] = xedges[i];
    for (int i = threadIdx.x; i <= ny_bins; i += kHistThreads) s_ye[i] = yedges[i];
    for (int i = threadIdx.x; i < n_cells; i += kHistThreads) s_counts[i] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kHistThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kHistThreads) {
        const int bx = find_bin(s_xe, nx_bins, (double)x[i]);
        const int by = find_bin(s_ye, ny_bins, (double)y[i]);
        if (bx >= 0 && by >= 0) atomicAdd(&s_counts[bx * ny_bins + by], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_cells; i += kHistThreads) {
        const unsigned int c = s_counts[i];
        if (c) atomicAdd(&counts[i], (unsigned long long)c);
    }
}

// workgroups of a histogram pass: enough to fill the chip, few enough that the per-workgroup flush stays small, and each
// counts fewer than 2^32 values
unsigned hist_blocks(int64_t n)
{
    int64_t blocks = ceil_div(n, (int64_t)kHistThreads * 16);
    if (blocks < 1) blocks = 1;
    if (blocks > 512) blocks = 512;
    const int64_t least = ceil_div(n, (int64_t)1 << 31);
    if (blocks < least) blocks = least;
    return (unsigned)blocks;
}

}  // namespace
}  // namespace fv3hip

using namespace fv3hip;

extern "C" int fv3hip_group_sums_chunk(void) { return kGsChunk; }

extern "C" size_t fv3hip_group_sums_workspace_bytes(int64_t n_items, int nz)
{
    if (n_items <= 0 || nz <= 0) return 0;
    return (size_t)n_items * (size_t)nz * kGsStats * sizeof(double);
}

extern "C" int fv3hip_group_sums(const void *a, const void *b, int dtype, const void *weights, int w_dtype, int64_t n_batch,
                                 int nz, int64_t n_inner, const int32_t *order, int64_t n_order, const int64_t *start,
                                 int64_t n_groups, const int32_t *item_group, const int32_t *item_chunk, int64_t n_items,
                                 const int64_t *group_item, double *sums, void *workspace, size_t workspace_bytes, void *stream)
{
    FV3HIP_REQUIRE(is_float(dtype), "unsupported dtype %d", dtype);
    FV3HIP_REQUIRE(!weights || is_float(w_dtype), "unsupported weight dtype %d", w_dtype);
    FV3HIP_REQUIRE(n_batch >= 0 && nz >= 0 && n_inner >= 0 && n_order >= 0 && n_groups >= 0 && n_items >= 0, "negative extent");
    FV3HIP_REQUIRE(nz <= 65535, "at most 65535 levels, got %d", nz);
    FV3HIP_REQUIRE(n_inner == 0 || n_batch <= (int64_t)0x7fffffff / n_inner, "cell ids are int32: %lld x %lld cells do not fit",
                   (long long)n_batch, (long long)n_inner);
    FV3HIP_REQUIRE(n_items <= 0x7fffffff, "too many work items: %lld", (long long)n_items);
    if (n_groups == 0 || nz == 0) return FV3HIP_OK;
    FV3HIP_REQUIRE(sums && group_item, "null pointer");
    hipStream_t st = as_stream(stream);
    if (n_items > 0) {
        FV3HIP_REQUIRE(a && order && start && item_group && item_chunk, "null pointer");
        FV3HIP_REQUIRE(workspace && workspace_bytes >= fv3hip_group_sums_workspace_bytes(n_items, nz),
                       "workspace of %zu bytes is smaller than fv3hip_group_sums_workspace_bytes (%zu)", workspace_bytes,
                       fv3hip_group_sums_workspace_bytes(n_items, nz));
        const dim3 grid((unsigned)n_items, (unsigned)nz);
        double *partial = static_cast<double *>(workspace);
        // the kernel for the operand types and for which of b and weights are there (without weights their type is float)
        auto launch = [&](auto ta, auto tw, auto has_w) {
            using TA = decltype(ta);
            using TW = decltype(tw);
            auto items = [&](auto has_b) {
                hipLaunchKernelGGL((group_sums_items_kernel<TA, TW, decltype(has_b)::value, decltype(has_w)::value>), grid,
                                   dim3(kGsThreads), 0, st, as<TA>(a), as<TA>(b), as<TW>(weights), n_batch, nz, n_inner, order,
                                   n_order, start, n_groups, item_group, item_chunk, partial);
            };
            if (b) items(std::true_type{});
            else items(std::false_type{});
        };
        with_float(dtype, [&](auto ta) {
            if (weights) with_float(w_dtype, [&](auto tw) { launch(ta, tw, std::true_type{}); });
            else launch(ta, float{}, std::false_type{});
        });
        int rc = check_launch("group_sums_items_kernel");
        if (rc != FV3HIP_OK) return rc;
    }
    int64_t blocks = ceil_div(n_groups * nz * kGsStats, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(group_sums_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const double *>(workspace),
                       group_item, n_groups, nz, n_items, sums);
    return check_launch("group_sums_finish_kernel");
}

extern "C" int fv3hip_histogram(const void *x, int dtype, int64_t n, const double *edges, int n_bins, int64_t *counts, void *stream)
{
    FV3HIP_REQUIRE(is_float(dtype), "unsupported dtype %d", dtype);
    FV3HIP_REQUIRE(n_bins >= 1 && n_bins <= kHistMaxBins, "1 to %d bins, got %d", kHistMaxBins, n_bins);
    FV3HIP_REQUIRE(n >= 0, "negative extent");
    FV3HIP_REQUIRE(edges && counts && (x || n == 0), "null pointer");
    hipStream_t st = as_stream(stream);
    FV3HIP_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)n_bins * sizeof(int64_t), st));
    if (n == 0) return FV3HIP_OK;
    with_float(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((histogram_kernel<T>), dim3(hist_blocks(n)), dim3(kHistThreads), 0, st, as<T>(x), n, edges, n_bins,
                           reinterpret_cast<unsigned long long *>(counts));
    });
    return check_launch("histogram_kernel");
}

extern "C" int fv3hip_histogram2d(const void *x, const void *y, int dtype, int64_t n, const double *xedges, int nx_bins,
                                  const double *yedges, int ny_bins, int64_t *counts, void *stream)
{
    FV3HIP_REQUIRE(is_float(dtype), "unsupported dtype %d", dtype);
    FV3HIP_REQUIRE(nx_bins >= 1 && nx_bins <= kHist2dMaxBins && ny_bins >= 1 && ny_bins <= kHist2dMaxBins,
                   "1 to %d bins per axis, got %d x %d", kHist2dMaxBins, nx_bins, ny_bins);
    FV3HIP_REQUIRE(n >= 0, "negative extent");
    FV3HIP_REQUIRE(xedges && yedges && counts && ((x && y) || n == 0), "null pointer");
    hipStream_t st = as_stream(stream);
    FV3HIP_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)nx_bins * ny_bins * sizeof(int64_t), st));
    if (n == 0) return FV3HIP_OK;
    with_float(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((histogram2d_kernel<T>), dim3(hist_blocks(n)), dim3(kHistThreads), 0, st, as<T>(x), as<T>(y), n, xedges,
                           nx_bins, yedges, ny_bins, reinterpret_cast<unsigned long long *>(counts));
    });
    return check_launch("histogram2d_kernel");
}
