// What every MLP path (the fused kernels, mlp_small_kernel and the layered path of mlp.hip, the split-bf16 kernel of
// mlp_bf16x3.hip) derives from fv3hip_mlp_desc_t on the host: the one check of the descriptor, the normalisation constants
// folded into weights and biases (each expression once), the input / output tables and the plain row-major matrices.
// Host-only plain C++: no HIP runtime call, nothing here touches the device.
#pragma once
#include <cfloat>
#include <cmath>
#include <vector>

#include "common.h"

namespace fv3hip {

struct KEntry {  // one network input feature (32 bytes)
    int src;     // source array, -1 for padding
    int feat;    // feature (level) index inside the source
    float center;
    float scale;
    int transform;
    float eps;
    int pad0, pad1;
};

struct OEntry {  // one network output feature as the host describes it (32 bytes, global memory)
    float scale, center, lo, hi;
    float mask;
    int out_feat;  // (output slot << 20) | feature inside the slot; -1 for padding
    int res;       // (residual slot << 8) | residual source; -1 for none
    int pad0;
};

// row of a 32x32 accumulator held by register r of a lane in half h is rho(r) + 4*h (constexpr: host and kernels alike)
constexpr int rho(int r) { return (r & 3) + 8 * (r >> 2); }

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct MlpDims {
    int K = 0, F = 0;  // network input / output features
    int hout = 0;      // 1: the last hidden layer's activations are an output of their own
};

// The one check of a descriptor: every create path calls it first, what a path does not support is refused after it.
// `out` is the caller's handle pointer (only tested for null); the limits are those of the kernels' argument tables.
inline int check_mlp_desc(const fv3hip_mlp_desc_t *d, const void *out, int max_sources, int max_outputs, MlpDims &dims)
{
    FV3HIP_REQUIRE(d && out, "null pointer");
    FV3HIP_REQUIRE(d->n_sources >= 1 && d->n_sources <= max_sources, "n_sources must be in [1, %d], got %d", max_sources, d->n_sources);
    FV3HIP_REQUIRE(d->n_inputs >= 1, "n_inputs must be >= 1");
    const int hout = d->hidden_output ? 1 : 0;
    FV3HIP_REQUIRE(d->n_outputs >= 1 || (d->n_outputs == 0 && hout), "n_outputs must be >= 1 (or 0 with hidden_output)");
    FV3HIP_REQUIRE(d->n_residual >= 0 && d->n_outputs + d->n_residual + hout <= max_outputs,
                   "n_outputs + n_residual (+ the hidden output) must be <= %d", max_outputs);
    FV3HIP_REQUIRE(d->width >= 1, "width must be >= 1");
    FV3HIP_REQUIRE(d->n_hidden >= 0, "negative n_hidden");
    FV3HIP_REQUIRE(d->hidden_activation == FV3HIP_ACT_RELU || d->hidden_activation == FV3HIP_ACT_LINEAR, "unknown activation %d", d->hidden_activation);
    int K = 0, F = 0;
    for (int i = 0; i < d->n_inputs; ++i) {
        FV3HIP_REQUIRE(d->in_source[i] >= 0 && d->in_source[i] < d->n_sources, "in_source[%d] out of range", i);
        FV3HIP_REQUIRE(d->in_nfeat[i] >= 1 && d->in_feat_start[i] >= 0, "bad feature range for input %d", i);
        K += d->in_nfeat[i];
    }
    for (int j = 0; j < d->n_outputs; ++j) {
        FV3HIP_REQUIRE(d->out_nfeat[j] >= 1 && d->out_nfeat[j] < (1 << 20), "bad out_nfeat[%d]", j);
        F += d->out_nfeat[j];
    }
    for (int r = 0; r < d->n_residual; ++r) {
        FV3HIP_REQUIRE(d->res_source[r] >= 0 && d->res_source[r] < d->n_sources, "res_source[%d] out of range", r);
        FV3HIP_REQUIRE(d->res_output[r] >= 0 && d->res_output[r] < d->n_outputs, "res_output[%d] out of range", r);
    }
    dims.K = K;
    dims.F = F;
    dims.hout = hout;
    return FV3HIP_OK;
}

// ---- the normalisation folded into weights and biases: each expression is written here and nowhere else ----
// An output's denormalisation y * scale + center goes into the output kernel's column and the output bias, so that the
// accumulator already holds the physical value; an input's 1 / (std + eps) goes into the row of the first kernel that
// multiplies it (one rounding per weight, once), so that the kernels only subtract the mean.
inline float oscale(const fv3hip_mlp_desc_t *d, int f) { return d->out_scale ? d->out_scale[f] : 1.f; }

inline float folded_out_bias(const fv3hip_mlp_desc_t *d, int f)
{
    return (float)((double)d->out_bias[f] * oscale(d, f) + (d->out_center ? d->out_center[f] : 0.f));
}

inline float in_rscale(const fv3hip_mlp_desc_t *d, int k) { return d->in_scale ? (float)(1.0 / (double)d->in_scale[k]) : 1.f; }

// (residual slot << 8) | residual source of the residual output `after = before + output j`, -1 if output j has none
inline int residual_code(const fv3hip_mlp_desc_t *d, int j)
{
    int res = -1;
    for (int r = 0; r < d->n_residual; ++r)
        if (d->res_output[r] == j) res = ((d->n_outputs + r) << 8) | d->res_source[r];
    return res;
}

// multiply-adds x 2 of one sample (no hidden layer: the output layer reads the inputs)
inline int64_t mlp_flops(int K, int width, int n_hidden, int F)
{
    return n_hidden ? 2 * ((int64_t)K * width + (int64_t)(n_hidden - 1) * width * width + (int64_t)width * F) : 2 * (int64_t)K * F;
}

// ---- the tables both kernel families of mlp.hip and its layered path read ----
struct InputTable {
    std::vector<KEntry> ktab;
    std::vector<int> perm;     // table row -> original input feature, -1 = padding
    int n_log = 0;             // input features that take the logarithm
    int n_log_padded = 0;      // rows at the head of the table that take the logarithm (padded to whole 32-row chunks if room)
    bool eps_normal = true;    // every logarithm's floor is a normal number
    bool short_log = false;    // the log block was padded to whole chunks, the real rows of its last chunk fit 8 of its 16 k-pair
                               // slots and a plain chunk follows: the fused fast-I/O kernels run that chunk with 8 slots
    int short_plain_slots = 0; // kShortPlainSlots where the partial plain chunk is the plain block's first and its real rows fit
                               // that many k-pair slots (the fused fast-I/O kernels then run it with as many); 0: it is the last
};

// The one slot count (two rows per k-pair slot) the fused fast-I/O kernels have a short plain body for: the Zhao-Carr
// emulator's partial plain chunk holds 26 real rows.
constexpr int kShortPlainSlots = 13;

// Network input k' is original input feature perm[k']: the log-transformed features come first (any order of the
// contraction index is the same dense layer), so that whole 32-row chunks are either with or without the transform.
// partial_plain_first (the fused path): where the plain block starts at a chunk boundary, spans two chunks or more and does
// not fill them, its partial chunk's real rows fit kShortPlainSlots slots, and the chunk ahead of the block is none or the
// 8-slot log chunk (short_log), that partial chunk is the block's FIRST, not its last -- real rows in unchanged order, then
// the zero rows, then the full chunks -- and short_plain_slots is set.  The real rows keep their order in the contraction;
// the zero rows, which add +-0 wherever they sit, move from the end of the table to the end of that chunk.
inline void build_input_table(const fv3hip_mlp_desc_t *d, int K, int n_ktab, InputTable &t, bool partial_plain_first = false)
{
    t.ktab.assign(n_ktab, KEntry{-1, 0, 0.f, 1.f, 0, 0.f, 0, 0});
    t.perm.clear();
    t.perm.reserve(n_ktab);
    std::vector<KEntry> orig(K);
    int k = 0;
    for (int i = 0; i < d->n_inputs; ++i)
        for (int f = 0; f < d->in_nfeat[i]; ++f, ++k) {
            KEntry &e = orig[k];
            e = KEntry{-1, 0, 0.f, 1.f, 0, 0.f, 0, 0};
            e.src = d->in_source[i];
            e.feat = d->in_feat_start[i] + f;
            e.center = d->in_center ? d->in_center[k] : 0.f;
            e.scale = in_rscale(d, k);  // reciprocal
            e.transform = d->in_transform ? d->in_transform[i] : 0;
            e.eps = d->in_eps ? d->in_eps[i] : 0.f;
        }
    for (int k2 = 0; k2 < K; ++k2)
        if (orig[k2].transform == FV3HIP_TRANSFORM_LOG) t.perm.push_back(k2);
    const int n_log = (int)t.perm.size();
    t.n_log = n_log;
    // if the chunk count allows, pad the log block to whole chunks (entries -1: zero weight rows reading a constant,
    // eps = 1 so that the logarithm is of a normal number) -- then no chunk mixes both kinds and every log chunk takes
    // the fast path
    const int n_pad = (32 - n_log % 32) % 32;
    if (n_log > 0 && n_log + n_pad + (K - n_log) <= n_ktab)
        for (int i = 0; i < n_pad; ++i) t.perm.push_back(-1);
    t.n_log_padded = (int)t.perm.size();
    const int n_plain = K - n_log, n_zero = n_ktab - t.n_log_padded - n_plain;  // (zero rows behind the plain block)
    t.short_log = t.n_log_padded % 32 == 0 && n_log % 32 >= 1 && n_log % 32 <= 16 && t.n_log_padded < n_ktab;
    t.short_plain_slots = 0;
    if (partial_plain_first && (n_log == 0 || t.short_log) && n_zero > 0 && n_zero < 32 && n_plain > 32 && 32 - n_zero <= 2 * kShortPlainSlots)
        t.short_plain_slots = kShortPlainSlots;
    int n_placed = 0;
    for (int k2 = 0; k2 < K; ++k2) {
        if (orig[k2].transform == FV3HIP_TRANSFORM_LOG) continue;
        if (t.short_plain_slots && n_placed == 32 - n_zero)
            for (int i = 0; i < n_zero; ++i) t.perm.push_back(-1);
        t.perm.push_back(k2);
        ++n_placed;
    }
    for (size_t k2 = 0; k2 < t.perm.size(); ++k2) {
        if (t.perm[k2] >= 0) {
            t.ktab[k2] = orig[t.perm[k2]];
        } else if ((int)k2 < t.n_log_padded) {
            t.ktab[k2].transform = FV3HIP_TRANSFORM_LOG;
            t.ktab[k2].eps = 1.f;
        }
    }
    t.eps_normal = true;
    for (int k2 = 0; k2 < t.n_log_padded; ++k2) t.eps_normal = t.eps_normal && t.ktab[k2].eps >= FLT_MIN;
}

// Rows [0, n_hidden_rows): the last hidden layer's features (hidden-output models), stored to the slot after the outputs
// and the residual outputs; rows first_out + f: output feature f.
inline void build_output_table(const fv3hip_mlp_desc_t *d, int n_otab, int first_out, int n_hidden_rows, std::vector<OEntry> &otab)
{
    otab.assign(n_otab, OEntry{1.f, 0.f, -INFINITY, INFINITY, 1.f, -1, -1, 0});
    for (int q = 0; q < n_hidden_rows; ++q) otab[q].out_feat = ((d->n_outputs + d->n_residual) << 20) | q;
    int f = 0;
    for (int j = 0; j < d->n_outputs; ++j) {
        const int res = residual_code(d, j);
        for (int q = 0; q < d->out_nfeat[j]; ++q, ++f) {
            OEntry &e = otab[first_out + f];
            e.scale = oscale(d, f);
            e.center = d->out_center ? d->out_center[f] : 0.f;
            e.lo = d->out_min ? d->out_min[f] : -INFINITY;
            e.hi = d->out_max ? d->out_max[f] : INFINITY;
            e.mask = d->out_mask ? d->out_mask[f] : 1.f;
            e.out_feat = (j << 20) | q;
            e.res = res;
        }
    }
}

// ---- the plain row-major matrices: the layered path's operands and mlp_small_kernel's copies of the fused weights ----
// The same folded values as the packed streams, rows of the first matrix in table order:
//   w1 [n_ktab][Wp], wh [max(n_hidden - 1, 1)][Wp][Wp], wo [Wp][Fp], bh [n_hidden][Wp], bo [Fp];
// without a hidden layer Wp is 0, w1 / wh / bh are empty and wo is [n_ktab][Fp].
struct PlainWeights {
    std::vector<float> w1, wh, wo, bh, bo;
};

inline void build_plain_weights(const fv3hip_mlp_desc_t *d, int F, int n_ktab, int Wp, int Fp, const InputTable &it, PlainWeights &p)
{
    const int nh = d->n_hidden, width = d->width;
    p.w1.assign(nh ? (size_t)n_ktab * Wp : 0, 0.f);
    p.wh.assign((size_t)(nh > 1 ? nh - 1 : 1) * Wp * Wp, 0.f);
    p.wo.assign((size_t)(nh ? Wp : n_ktab) * Fp, 0.f);
    p.bh.assign((size_t)nh * Wp, 0.f);
    p.bo.assign((size_t)Fp, 0.f);
    for (size_t k = 0; k < it.perm.size(); ++k) {
        if (it.perm[k] < 0) continue;
        if (nh)
            for (int f = 0; f < width; ++f) p.w1[k * Wp + f] = d->hidden_kernels[0][(size_t)it.perm[k] * width + f] * it.ktab[k].scale;
        else  // the only layer carries both foldings: 1 / std of its input row, the scale of its output column
            for (int f = 0; f < F; ++f)
                p.wo[k * Fp + f] = (float)((double)d->out_kernel[(size_t)it.perm[k] * F + f] * (double)it.ktab[k].scale * (double)oscale(d, f));
    }
    for (int l = 1; l < nh; ++l)
        for (int k = 0; k < width; ++k)
            for (int f = 0; f < width; ++f) p.wh[((size_t)(l - 1) * Wp + k) * Wp + f] = d->hidden_kernels[l][(size_t)k * width + f];
    for (int l = 0; l < nh; ++l)
        for (int f = 0; f < width; ++f) p.bh[(size_t)l * Wp + f] = d->hidden_biases[l][f];
    if (nh)
        for (int k = 0; k < width; ++k)
            for (int f = 0; f < F; ++f) p.wo[(size_t)k * Fp + f] = d->out_kernel[(size_t)k * F + f] * oscale(d, f);
    for (int f = 0; f < F; ++f) p.bo[f] = folded_out_bias(d, f);
}

}  // namespace fv3hip
