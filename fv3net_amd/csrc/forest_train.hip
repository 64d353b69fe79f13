// Random-forest training (fv3fit's "sklearn_random_forest"; sklearn's RandomForestRegressor.fit with the squared-error
// criterion and the exact best-split search), one tree at a time, level by level over all open nodes.
//
// Every feature keeps the in-bag samples as a list sorted by the float32 feature value; the open nodes of a level are
// consecutive segments of every list, the same position ranges in each.  Per level:
//   ft_positions_kernel      position -> open node (binary search in the segment starts)
//   ft_chunk_tails_kernel    per (feature, chunk of 256 positions): the sums of w y_k, w and w sum_k y_k^2 after the chunk's
//                            last segment head, one thread per column, positions in order
//   ft_chunk_carry_kernel    per (feature, column): the tails, chunk after chunk, into the sum that enters each chunk
//   ft_node_stats_kernel     per node: its totals (the prefix at its last position in feature 0's list), value and impurity
//   ft_scan_kernel           per (feature, chunk): tiles of up to 32 positions x columns in LDS -- the running sums down the
//                            tile with one thread per column, then the proxy of every admissible position with one thread
//                            per position, the outputs in order
//   ft_best_kernel           per (node, feature): the greatest proxy and its lowest position
//   ft_decide_kernel         per node: the best feature (lowest index among equals), threshold, the leaf rules, the record
//   ft_children_kernel       one block: child ids and the children's segments by an exclusive scan over the nodes
//   ft_side_kernel           per sample: left, right or finished
//   ft_count_kernel / ft_count_carry_kernel / ft_scatter_kernel
//                            the stable partition of every list within every split segment
// No floating-point atomics, no workgroup waits for another: every sum has an order fixed by the shapes.  Every index read
// from a buffer is checked against the extent of what it indexes before it is used.
#include <cfloat>
#include <cmath>

#include "common.h"

using namespace fv3hip;

namespace {

constexpr int kChunk = 256;        // positions per block = threads per block
constexpr int kTileRows = 32;      // positions staged in LDS at a time
constexpr int kBestBlock = 128;
constexpr int kScanBlock = 1024;   // ft_children_kernel
constexpr size_t kMaxLds = 64 * 1024;
constexpr int kMaxOutputs = 3821;  // the most outputs of which one tile row fits kMaxLds (tile_shape)
constexpr uint8_t kLeft = 0, kRight = 1, kGone = 2;

typedef fv3hip_forest_train_t Ws;

struct Level {
    const int32_t *list;   // [F][n] this level's lists
    int32_t *list_next;
    const int64_t *seg;    // [K + 1]
    int64_t *seg_next;
    const int32_t *node;   // [K] tree node of each open node
    int32_t *node_next;
    int64_t K, m, n_chunks, n_nodes;
    int depth, is_final, rows, ldt;
    int64_t min_split, min_leaf;
};

__device__ __forceinline__ int32_t checked(int32_t i, int64_t extent) { return (uint64_t)(int64_t)i < (uint64_t)extent ? i : 0; }

// column c of sample s: w y_c for c < O, then w, then w sum_k y_k^2
__device__ __forceinline__ double column(const Ws &w, int32_t s, double wt, int c)
{
    if (c < w.O) return wt * w.y[(int64_t)s * w.O + c];
    return c == w.O ? wt : wt * w.ysq[s];
}

__device__ __forceinline__ bool chunk_has_head(const int32_t *pos_node, const int64_t *seg, int64_t K, int64_t p0, int64_t p1)
{
    const int32_t k0 = checked(pos_node[p0], K), k1 = checked(pos_node[p1 - 1], K);
    return k0 != k1 || seg[k0] == p0;
}

__global__ __launch_bounds__(kChunk) void ft_begin_kernel(Ws w, int64_t m)
{
    const int64_t s = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    if (s < w.n) {
        w.side[s] = w.weight[s] > 0 ? kLeft : kGone;
        w.pos_node[s] = 0;
    }
    if (s == 0) {
        w.seg_b[0] = 0, w.seg_b[1] = w.n;   // the presorted lists: one segment, compacted into list_a
        w.seg_a[0] = 0, w.seg_a[1] = m;
        w.node_a[0] = 0;
        w.dst_left[0] = 0, w.dst_right[0] = 0;
        w.level[0] = 1, w.level[1] = m, w.level[2] = 1, w.level[3] = 0;
    }
}

__global__ __launch_bounds__(kChunk) void ft_positions_kernel(const int64_t *seg, int64_t K, int64_t m, int32_t *pos_node)
{
    const int64_t p = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    if (p >= m) return;
    int64_t lo = 0, hi = K;  // the last k with seg[k] <= p
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) / 2;
        if (seg[mid] <= p) lo = mid; else hi = mid;
    }
    pos_node[p] = (int32_t)lo;
}

// ids / weights / heads of one chunk into LDS; returns the number of positions
__device__ __forceinline__ int stage_chunk(const Ws &w, const Level &L, int f, int64_t p0, int32_t *ids, int32_t *nodek, double *wts,
                                           uint8_t *head)
{
    const int64_t p1 = p0 + kChunk < L.m ? p0 + kChunk : L.m;
    const int j = threadIdx.x;
    const int64_t p = p0 + j;
    if (p < p1) {
        const int32_t s = checked(L.list[(int64_t)f * w.n + p], w.n);
        const int32_t k = checked(w.pos_node[p], L.K);
        ids[j] = s;
        nodek[j] = k;
        wts[j] = (double)w.weight[s];
        head[j] = L.seg[k] == p;
    }
    if (j == 0) ids[kChunk] = p1 < L.m ? checked(L.list[(int64_t)f * w.n + p1], w.n) : 0;
    return (int)(p1 - p0);
}

__global__ __launch_bounds__(kChunk) void ft_chunk_tails_kernel(Ws w, Level L)
{
    __shared__ int32_t ids[kChunk + 1], nodek[kChunk];
    __shared__ double wts[kChunk];
    __shared__ uint8_t head[kChunk];
    const int f = blockIdx.y;
    const int64_t ch = blockIdx.x;
    const int np = stage_chunk(w, L, f, ch * kChunk, ids, nodek, wts, head);
    __syncthreads();
    const int OC = w.O + 2;
    double *out = w.carry + ((int64_t)f * L.n_chunks + ch) * OC;
    for (int c = threadIdx.x; c < OC; c += kChunk) {
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < np; ++j) {
            const double v = column(w, ids[j], wts[j], c);
            acc = head[j] ? v : acc + v;
        }
        out[c] = acc;
    }
}

__global__ __launch_bounds__(kChunk) void ft_chunk_carry_kernel(Ws w, Level L, int nF)
{
    const int OC = w.O + 2;
    const int64_t i = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    if (i >= (int64_t)nF * OC) return;
    const int64_t f = i / OC;
    const int c = (int)(i - f * OC);
    double run = 0.0;
    for (int64_t ch = 0; ch < L.n_chunks; ++ch) {
        const int64_t p0 = ch * kChunk, p1 = p0 + kChunk < L.m ? p0 + kChunk : L.m;
        double *q = w.carry + (f * L.n_chunks + ch) * OC + c;
        const double t = *q;
        *q = run;
        run = chunk_has_head(w.pos_node, L.seg, L.K, p0, p1) ? t : run + t;
    }
}

__global__ __launch_bounds__(kChunk) void ft_node_stats_kernel(Ws w, Level L)
{
    const int64_t k = blockIdx.x;
    const int OC = w.O + 2;
    const int64_t a = L.seg[k], e = L.seg[k + 1] - 1;
    if (a < 0 || e < a || e >= L.m) return;
    const int64_t ch = e / kChunk, p0 = ch * kChunk, start = a > p0 ? a : p0;
    double *st = w.stats + k * OC;
    for (int c = threadIdx.x; c < OC; c += kChunk) {
        double acc = a < p0 ? w.carry[ch * OC + c] : 0.0;  // (feature 0)
        for (int64_t p = start; p <= e; ++p) {
            const int32_t s = checked(L.list[p], w.n);
            acc += column(w, s, (double)w.weight[s], c);
        }
        st[c] = acc;
    }
    __syncthreads();
    const int64_t node = checked(L.node[k], w.node_cap);
    const double W = st[w.O];
    for (int c = threadIdx.x; c < w.O; c += kChunk) w.value[node * w.O + c] = st[c] / W;
    if (threadIdx.x == 0) {
        double imp = st[w.O + 1] / W;   // sklearn's MSE.node_impurity, in its order
        for (int c = 0; c < w.O; ++c) {
            const double mean = st[c] / W;
            imp -= mean * mean;
        }
        w.impurity[node] = imp / w.O;
        w.weighted_n[node] = W;
        w.n_samples[node] = (int32_t)(e + 1 - a);
    }
}

__global__ __launch_bounds__(kChunk) void ft_scan_kernel(Ws w, Level L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int OC = w.O + 2;
    double *tile = reinterpret_cast<double *>(lds);   // [rows][ldt]
    double *run = tile + (size_t)L.rows * L.ldt;      // [OC]
    double *wts = run + OC;                           // [kChunk]
    int32_t *ids = reinterpret_cast<int32_t *>(wts + kChunk);  // [kChunk + 1]
    int32_t *nodek = ids + kChunk + 1;                // [kChunk]
    uint8_t *head = reinterpret_cast<uint8_t *>(nodek + kChunk);
    const int f = blockIdx.y;
    const int64_t ch = blockIdx.x, p0 = ch * kChunk;
    const int np = stage_chunk(w, L, f, p0, ids, nodek, wts, head);
    const double *carry = w.carry + ((int64_t)f * L.n_chunks + ch) * OC;
    for (int c = threadIdx.x; c < OC; c += kChunk) run[c] = carry[c];
    __syncthreads();
    const float *x = w.xt + (int64_t)f * w.n;
    double *proxy = w.proxy + (int64_t)f * w.n;
    for (int t0 = 0; t0 < np; t0 += L.rows) {
        const int nt = np - t0 < L.rows ? np - t0 : L.rows;
        for (int c = threadIdx.x; c < OC; c += kChunk) {
            double r = run[c];
#pragma unroll 8
            for (int j = 0; j < nt; ++j) {
                const double v = column(w, ids[t0 + j], wts[t0 + j], c);
                r = head[t0 + j] ? v : r + v;
                tile[j * L.ldt + c] = r;
            }
            run[c] = r;
        }
        __syncthreads();
        if ((int)threadIdx.x < nt) {
            const int j = threadIdx.x, jj = t0 + j;
            const int64_t p = p0 + jj;
            const int32_t k = nodek[jj];
            const int64_t a = L.seg[k], b = L.seg[k + 1];
            double out = -INFINITY;
            if (p + 1 < b && b <= L.m) {
                const int64_t n_left = p + 1 - a, n_right = b - (p + 1);
                const float xa = x[ids[jj]], xb = x[ids[jj + 1]];
                if (n_left >= L.min_leaf && n_right >= L.min_leaf && !(xb <= xa + 1e-7f)) {
                    const double *tot = w.stats + (int64_t)k * OC;
                    const double *row = tile + j * L.ldt;
                    const double wl = row[w.O], wr = tot[w.O] - wl;
                    if (wl > 0.0 && wr > 0.0) {
                        double pl = 0.0, pr = 0.0;
                        for (int c = 0; c < w.O; ++c) {
                            const double sl = row[c], sr = tot[c] - sl;
                            pl += sl * sl;
                            pr += sr * sr;
                        }
                        out = pl / wl + pr / wr;
                    }
                }
            }
            proxy[p] = out;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBestBlock) void ft_best_kernel(Ws w, Level L)
{
    __shared__ double bv[kBestBlock];
    __shared__ int64_t bp[kBestBlock];
    const int64_t k = blockIdx.x;
    const int f = blockIdx.y;
    int64_t a = L.seg[k], b = L.seg[k + 1];
    if (a < 0 || b > L.m) a = b = 0;
    const double *proxy = w.proxy + (int64_t)f * w.n;
    double best = -INFINITY;
    int64_t pos = INT64_MAX;
    for (int64_t p = a + threadIdx.x; p + 1 < b; p += kBestBlock) {
        const double v = proxy[p];
        if (v > best) best = v, pos = p;
    }
    bv[threadIdx.x] = best, bp[threadIdx.x] = pos;
    __syncthreads();
    for (int h = kBestBlock / 2; h > 0; h /= 2) {
        if ((int)threadIdx.x < h) {
            const double v = bv[threadIdx.x + h];
            const int64_t q = bp[threadIdx.x + h];
            if (v > bv[threadIdx.x] || (v == bv[threadIdx.x] && q < bp[threadIdx.x])) bv[threadIdx.x] = v, bp[threadIdx.x] = q;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        w.best_proxy[k * w.F + f] = bv[0];
        w.best_pos[k * w.F + f] = bp[0];
    }
}

__global__ __launch_bounds__(kChunk) void ft_decide_kernel(Ws w, Level L)
{
    const int64_t k = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    if (k >= L.K) return;
    const int64_t node = checked(L.node[k], w.node_cap);
    const int64_t a = L.seg[k], b = L.seg[k + 1], nn = b - a;
    bool leaf = L.is_final || nn < L.min_split || nn < 2 * L.min_leaf || w.impurity[node] <= DBL_EPSILON;
    double best = -INFINITY;
    int bf = -1;
    int64_t pos = -1;
    if (!leaf) {
        for (int f = 0; f < w.F; ++f) {
            const double v = w.best_proxy[k * w.F + f];
            if (v > best) best = v, bf = f, pos = w.best_pos[k * w.F + f];
        }
        leaf = bf < 0 || pos < a || pos + 1 >= b || b > L.m;
    }
    if (leaf) {
        w.left[node] = -1, w.right[node] = -1;
        w.feature[node] = -2, w.threshold[node] = -2.0;   // sklearn's TREE_UNDEFINED
        w.missing_left[node] = 0;
        w.n_left[k] = 0;
        return;
    }
    const int32_t *list = L.list + (int64_t)bf * w.n;
    const float *x = w.xt + (int64_t)bf * w.n;
    const double xa = x[checked(list[pos], w.n)], xb = x[checked(list[pos + 1], w.n)];
    double thr = xa / 2.0 + xb / 2.0;   // exact for two float32 values
    if (thr == xb || thr == INFINITY || thr == -INFINITY) thr = xa;
    const int64_t n_left = pos + 1 - a;
    w.feature[node] = bf, w.threshold[node] = thr;
    w.missing_left[node] = n_left > nn - n_left;
    w.n_left[k] = n_left;   // > 0: the node splits (its children are numbered by ft_children_kernel)
}

// exclusive scan of one value per thread over the block (Hillis-Steele in LDS); *total: the block's sum
__device__ __forceinline__ int64_t block_exclusive(int64_t v, int64_t *sh, int64_t *total)
{
    const int t = threadIdx.x, nthr = blockDim.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < nthr; d *= 2) {
        const int64_t add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const int64_t incl = sh[t];
    *total = sh[nthr - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kScanBlock) void ft_children_kernel(Ws w, Level L)
{
    __shared__ int64_t sh[kScanBlock];
    int64_t splits = 0, samples = 0;   // over the nodes before this round's
    int overflow = 0;
    for (int64_t k0 = 0; k0 < L.K; k0 += kScanBlock) {
        const int64_t k = k0 + threadIdx.x;
        const bool in = k < L.K;
        const int64_t nl = in ? w.n_left[k] : 0;
        const int64_t nn = in && nl > 0 ? L.seg[k + 1] - L.seg[k] : 0;
        int64_t tot_splits, tot_samples;
        const int64_t i = splits + block_exclusive(nl > 0 ? 1 : 0, sh, &tot_splits);
        const int64_t at = samples + block_exclusive(nn, sh, &tot_samples);
        if (in && nl > 0) {
            const int64_t node = checked(L.node[k], w.node_cap);
            const int64_t child = L.n_nodes + 2 * i;
            if (child + 1 < w.node_cap && 2 * i + 1 < w.k_cap) {
                w.left[node] = (int32_t)child, w.right[node] = (int32_t)(child + 1);
                L.node_next[2 * i] = (int32_t)child, L.node_next[2 * i + 1] = (int32_t)(child + 1);
                L.seg_next[2 * i] = at, L.seg_next[2 * i + 1] = at + nl;
            } else {
                overflow = 1;   // (cannot happen with buffers sized as the header says)
            }
            w.dst_left[k] = at, w.dst_right[k] = at + nl;
        }
        splits += tot_splits, samples += tot_samples;
    }
    overflow = __syncthreads_or(overflow);
    if (threadIdx.x == 0) {
        if (2 * splits < w.k_cap + 1) L.seg_next[2 * splits] = samples;
        w.level[0] = 2 * splits;
        w.level[1] = samples;
        w.level[2] = L.n_nodes + 2 * splits;
        w.level[3] = overflow;   // written every level: the record does not depend on what the buffer held
    }
}

__global__ __launch_bounds__(kChunk) void ft_side_kernel(Ws w, Level L)
{
    const int64_t p = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    if (p >= L.m) return;
    const int32_t s = checked(L.list[p], w.n);   // (feature 0: every list holds the same samples in each segment)
    const int32_t k = checked(w.pos_node[p], L.K);
    uint8_t side = kGone;
    if (w.n_left[k] > 0) {
        const int64_t node = checked(L.node[k], w.node_cap);
        const int32_t f = checked(w.feature[node], w.F);
        side = (double)w.xt[(int64_t)f * w.n + s] <= w.threshold[node] ? kLeft : kRight;
    }
    w.side[s] = side;
}

// The stable partition, for src lists of `m` positions in segments `seg` [K + 1]: the samples with side 0 of segment k go to
// dst_left[k] onwards, those with side 1 to dst_right[k] onwards, in their order; the others are dropped.
struct Part {
    const int32_t *src;
    int32_t *dst;
    const int64_t *seg;
    int64_t K, m, n_chunks;
};

__global__ __launch_bounds__(kChunk) void ft_count_kernel(Ws w, Part P)
{
    __shared__ int last_head;
    const int f = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    if (threadIdx.x == 0) last_head = -1;
    __syncthreads();
    bool left = false;
    if (p < P.m) {
        left = w.side[checked(P.src[(int64_t)f * w.n + p], w.n)] == kLeft;
        if (P.seg[checked(w.pos_node[p], P.K)] == p) atomicMax(&last_head, (int)threadIdx.x);
    }
    __syncthreads();
    const int cnt = __syncthreads_count(left && (int)threadIdx.x >= last_head);
    if (threadIdx.x == 0) w.count[(int64_t)f * P.n_chunks + blockIdx.x] = cnt;
}

__global__ __launch_bounds__(kChunk) void ft_count_carry_kernel(Ws w, Part P)
{
    const int f = blockIdx.x * kChunk + threadIdx.x;
    if (f >= w.F) return;
    int32_t run = 0;
    for (int64_t ch = 0; ch < P.n_chunks; ++ch) {
        const int64_t p0 = ch * kChunk, p1 = p0 + kChunk < P.m ? p0 + kChunk : P.m;
        int32_t *q = w.count + (int64_t)f * P.n_chunks + ch;
        const int32_t t = *q;
        *q = run;
        run = chunk_has_head(w.pos_node, P.seg, P.K, p0, p1) ? t : run + t;
    }
}

__global__ __launch_bounds__(kChunk) void ft_scatter_kernel(Ws w, Part P)
{
    __shared__ int incl[kChunk], hd[kChunk];
    const int f = blockIdx.y, t = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * kChunk + t;
    int32_t s = 0, k = 0;
    uint8_t side = kGone;
    bool head = false;
    if (p < P.m) {
        s = checked(P.src[(int64_t)f * w.n + p], w.n);
        k = checked(w.pos_node[p], P.K);
        side = w.side[s];
        head = P.seg[k] == p;
    }
    const int flag = side == kLeft;
    incl[t] = flag;
    hd[t] = head ? t : -1;
    __syncthreads();
    for (int d = 1; d < kChunk; d *= 2) {
        const int add = t >= d ? incl[t - d] : 0;
        const int h = t >= d ? hd[t - d] : -1;
        __syncthreads();
        incl[t] += add;
        hd[t] = hd[t] > h ? hd[t] : h;
        __syncthreads();
    }
    if (p >= P.m || side == kGone) return;
    const int h = hd[t];   // the last segment head at or before this position within the chunk
    const int before = incl[t] - flag;   // lefts of this chunk before this position
    const int64_t lefts = h > 0 ? before - incl[h - 1] : h == 0 ? before : (int64_t)w.count[(int64_t)f * P.n_chunks + blockIdx.x] + before;
    const int64_t dest = side == kLeft ? w.dst_left[k] + lefts : w.dst_right[k] + ((p - P.seg[k]) - lefts);
    if ((uint64_t)dest < (uint64_t)w.n) P.dst[(int64_t)f * w.n + dest] = s;
}

// what ft_scan_kernel keeps in LDS beside the tile, and one row of the tile (the leading dimension is odd: the 32 rows of one
// column fall on distinct banks)
constexpr size_t scan_fixed_bytes(int O) { return (size_t)(O + 2) * 8 + kChunk * 8 + (kChunk + 1) * 4 + kChunk * 4 + kChunk; }
constexpr size_t scan_row_bytes(int O) { return (size_t)((O + 2) | 1) * 8; }
static_assert(scan_fixed_bytes(kMaxOutputs) + scan_row_bytes(kMaxOutputs) <= kMaxLds &&
                  scan_fixed_bytes(kMaxOutputs + 1) + scan_row_bytes(kMaxOutputs + 1) > kMaxLds,
              "kMaxOutputs is not the greatest output count with a tile of one row");

// rows of the LDS tile and its leading dimension for O <= kMaxOutputs outputs
void tile_shape(int O, int *rows, int *ldt, size_t *bytes)
{
    *ldt = (O + 2) | 1;
    const size_t fixed = scan_fixed_bytes(O), per_row = scan_row_bytes(O);
    const size_t r = (kMaxLds - fixed) / per_row;
    *rows = (int)(r < (size_t)kTileRows ? r : (size_t)kTileRows);
    *bytes = fixed + (size_t)*rows * per_row;
}

int check_ws(const Ws *w)
{
    FV3HIP_REQUIRE(w, "null workspace");
    FV3HIP_REQUIRE(w->n >= 1 && w->n < ((int64_t)1 << 31), "n must be in [1, 2^31), got %lld", (long long)w->n);
    FV3HIP_REQUIRE(w->F >= 1 && w->F <= 65535, "the feature count must be in [1, 65535], got %d", w->F);
    FV3HIP_REQUIRE(w->O >= 1 && w->O <= kMaxOutputs, "the output count must be in [1, %d] (one row of the scan's LDS tile), got %d",
                   kMaxOutputs, w->O);
    FV3HIP_REQUIRE(w->k_cap >= 1 && w->node_cap >= 1 && w->node_cap < ((int64_t)1 << 31), "bad k_cap %lld or node_cap %lld",
                   (long long)w->k_cap, (long long)w->node_cap);
    FV3HIP_REQUIRE(w->xt && w->y && w->ysq && w->order && w->weight && w->list_a && w->list_b && w->side && w->pos_node &&
                       w->seg_a && w->seg_b && w->node_a && w->node_b && w->stats && w->carry && w->count && w->proxy &&
                       w->best_proxy && w->best_pos && w->n_left && w->dst_left && w->dst_right && w->left && w->right &&
                       w->feature && w->threshold && w->missing_left && w->value && w->impurity && w->weighted_n &&
                       w->n_samples && w->level,
                   "null pointer in the forest-training workspace");
    return FV3HIP_OK;
}

int partition(const Ws &w, const Part &P, hipStream_t st)
{
    if (P.m == 0) return FV3HIP_OK;
    const dim3 grid((unsigned)P.n_chunks, (unsigned)w.F);
    hipLaunchKernelGGL(ft_count_kernel, grid, dim3(kChunk), 0, st, w, P);
    hipLaunchKernelGGL(ft_count_carry_kernel, dim3((unsigned)ceil_div(w.F, kChunk)), dim3(kChunk), 0, st, w, P);
    hipLaunchKernelGGL(ft_scatter_kernel, grid, dim3(kChunk), 0, st, w, P);
    return check_launch("forest-training partition kernels");
}

}  // namespace

extern "C" int fv3hip_forest_train_chunk(void) { return kChunk; }

extern "C" int fv3hip_forest_train_begin(const fv3hip_forest_train_t *ws, int64_t n_inbag, void *stream)
{
    int rc = check_ws(ws);
    if (rc) return rc;
    FV3HIP_REQUIRE(n_inbag >= 1 && n_inbag <= ws->n, "n_inbag must be in [1, n], got %lld", (long long)n_inbag);
    const hipStream_t st = as_stream(stream);
    const int64_t n_chunks = ceil_div(ws->n, kChunk);
    hipLaunchKernelGGL(ft_begin_kernel, dim3((unsigned)n_chunks), dim3(kChunk), 0, st, *ws, n_inbag);
    rc = check_launch("ft_begin_kernel");
    if (rc) return rc;
    return partition(*ws, Part{ws->order, ws->list_a, ws->seg_b, 1, ws->n, n_chunks}, st);
}

extern "C" int fv3hip_forest_train_level(const fv3hip_forest_train_t *ws, int parity, int64_t n_open, int64_t n_positions,
                                         int64_t n_nodes, int depth, int max_depth, int64_t min_samples_split,
                                         int64_t min_samples_leaf, int phases, void *stream)
{
    int rc = check_ws(ws);
    if (rc) return rc;
    const Ws &w = *ws;
    FV3HIP_REQUIRE(parity == 0 || parity == 1, "parity must be 0 or 1");
    FV3HIP_REQUIRE(n_open >= 1 && n_open <= w.k_cap && n_open <= n_positions, "n_open must be in [1, min(k_cap, n_positions)], "
                   "got %lld", (long long)n_open);
    FV3HIP_REQUIRE(n_positions >= 1 && n_positions <= w.n, "n_positions must be in [1, n], got %lld", (long long)n_positions);
    FV3HIP_REQUIRE(n_nodes >= n_open && n_nodes <= w.node_cap, "n_nodes must be in [n_open, node_cap], got %lld", (long long)n_nodes);
    FV3HIP_REQUIRE(phases >= 1 && phases <= FV3HIP_FOREST_TRAIN_ALL, "phases must be a sum of FV3HIP_FOREST_TRAIN_* flags");
    FV3HIP_REQUIRE(depth >= 0 && min_samples_split >= 2 && min_samples_leaf >= 1, "bad depth, min_samples_split or min_samples_leaf");
    Level L;
    L.list = parity ? w.list_b : w.list_a;
    L.list_next = parity ? w.list_a : w.list_b;
    L.seg = parity ? w.seg_b : w.seg_a;
    L.seg_next = parity ? w.seg_a : w.seg_b;
    L.node = parity ? w.node_b : w.node_a;
    L.node_next = parity ? w.node_a : w.node_b;
    L.K = n_open, L.m = n_positions, L.n_chunks = ceil_div(n_positions, kChunk), L.n_nodes = n_nodes;
    L.depth = depth, L.is_final = max_depth >= 0 && depth >= max_depth;
    L.min_split = min_samples_split, L.min_leaf = min_samples_leaf;
    size_t lds;
    tile_shape(w.O, &L.rows, &L.ldt, &lds);
    const hipStream_t st = as_stream(stream);
    const int nF = L.is_final ? 1 : w.F;   // a last level needs its nodes' statistics only
    const int OC = w.O + 2;
    const unsigned pos_blocks = (unsigned)L.n_chunks;
    if (phases & FV3HIP_FOREST_TRAIN_SUMS) {
        hipLaunchKernelGGL(ft_positions_kernel, dim3(pos_blocks), dim3(kChunk), 0, st, L.seg, L.K, L.m, w.pos_node);
        hipLaunchKernelGGL(ft_chunk_tails_kernel, dim3(pos_blocks, (unsigned)nF), dim3(kChunk), 0, st, w, L);
        hipLaunchKernelGGL(ft_chunk_carry_kernel, dim3((unsigned)ceil_div((int64_t)nF * OC, kChunk)), dim3(kChunk), 0, st, w, L, nF);
        hipLaunchKernelGGL(ft_node_stats_kernel, dim3((unsigned)L.K), dim3(kChunk), 0, st, w, L);
        if ((rc = check_launch("forest-training statistics kernels"))) return rc;
    }
    if (!L.is_final && (phases & FV3HIP_FOREST_TRAIN_SCAN)) {
        hipLaunchKernelGGL(ft_scan_kernel, dim3(pos_blocks, (unsigned)w.F), dim3(kChunk), lds, st, w, L);
        hipLaunchKernelGGL(ft_best_kernel, dim3((unsigned)L.K, (unsigned)w.F), dim3(kBestBlock), 0, st, w, L);
        if ((rc = check_launch("forest-training scan kernels"))) return rc;
    }
    if (!(phases & FV3HIP_FOREST_TRAIN_SPLIT)) return FV3HIP_OK;
    hipLaunchKernelGGL(ft_decide_kernel, dim3((unsigned)ceil_div(L.K, kChunk)), dim3(kChunk), 0, st, w, L);
    hipLaunchKernelGGL(ft_children_kernel, dim3(1), dim3(kScanBlock), 0, st, w, L);
    if ((rc = check_launch("forest-training split kernels"))) return rc;
    if (!L.is_final) {
        hipLaunchKernelGGL(ft_side_kernel, dim3(pos_blocks), dim3(kChunk), 0, st, w, L);
        if ((rc = check_launch("ft_side_kernel"))) return rc;
        return partition(w, Part{L.list, L.list_next, L.seg, L.K, L.m, L.n_chunks}, st);
    }
    return FV3HIP_OK;
}
