// The cubed sphere's seams and the checks of channel-last cube buffers, shared by conv.hip, graph.hip and cyclegan.hip
// (graph.hip takes the table and the checks; its cell_index writes the seam rule out for depth 0).
#pragma once
#include "common.h"

namespace fv3hip {

// [tile][x-low, x-high, y-low, y-high]: the neighbouring tile, 1 if it is joined through its x axis, 1 if the edge is walked
// in reverse.  A kernel takes the table by value with its arguments.
struct CubeSeams {
    signed char nbr[24], nax[24], flip[24];
};

// xgcm's FV3 face connections; the edge is reversed when the neighbour is joined through the other axis than the side's own
inline CubeSeams cube_seams()
{
    const signed char nbr[24] = {4, 1, 5, 2, 0, 3, 5, 2, 0, 3, 1, 4, 2, 5, 1, 4, 2, 5, 3, 0, 4, 1, 3, 0};
    const signed char nax[24] = {0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0};
    CubeSeams s;
    for (int q = 0; q < 24; ++q) {
        s.nbr[q] = nbr[q];
        s.nax[q] = nax[q];
        s.flip[q] = (nax[q] == 1) != (q % 4 < 2) ? 1 : 0;
    }
    return s;
}

// (x, y) relative to a face of n x n cells, with exactly one of the two outside [0, n) (inx: x is inside): the side it lies
// beyond, its depth d counted outward from the edge (0: the first halo line) and its position j along the edge
__device__ inline void seam_side(int n, int x, int y, bool inx, int &side, int &d, int &j)
{
    if (!inx) {
        side = x < 0 ? 0 : 1;
        d = x < 0 ? -1 - x : x - n;
        j = y;
    } else {
        side = y < 0 ? 2 : 3;
        d = y < 0 ? -1 - y : y - n;
        j = x;
    }
}

// the cell (tt, xx, yy) that halo position (side, d, j) of tile t shows: line d of the neighbour counted inward from the
// shared edge, along the edge as the connection says
__device__ inline void seam_cross(const CubeSeams &s, int n, int t, int side, int d, int j, int &tt, int &xx, int &yy)
{
    const int q = t * 4 + side;
    const int line = (side & 1) ? d : n - 1 - d;
    const int jj = s.flip[q] ? n - 1 - j : j;
    xx = s.nax[q] ? line : jj;
    yy = s.nax[q] ? jj : line;
    tt = s.nbr[q];
}

// channels [off, off + c) of a channel-last buffer [sample][6][n][n][ld] with ss elements between the samples
struct Slice {
    const float *p;
    int64_t ld, off, ss;
    int c, n;
};

inline int check_slice(const char *what, const void *p, int64_t ld, int64_t off, int c)
{
    FV3HIP_REQUIRE(p, "%s is null", what);
    FV3HIP_REQUIRE(off >= 0 && ld >= 1 && off + c <= ld && ld <= (1 << 24),
                   "%s: channels [%lld, %lld) do not fit a row of %lld", what, (long long)off, (long long)(off + c), (long long)ld);
    return FV3HIP_OK;
}

// a sample stride of 0 stands for densely packed cubes
inline int check_stride(const char *what, int64_t *ss, int n, int64_t ld)
{
    const int64_t cube = 6LL * n * n * ld;
    if (*ss == 0) *ss = cube;
    FV3HIP_REQUIRE(*ss >= cube, "%s: sample stride %lld is shorter than a cube of %lld elements", what, (long long)*ss, (long long)cube);
    return FV3HIP_OK;
}

struct CubeLimits {
    int64_t max_samples;
    const char *max_samples_text;
    int max_n;
};

inline int check_cube(int64_t n_samples, int n, const CubeLimits &lim)
{
    FV3HIP_REQUIRE(n_samples >= 0 && n_samples <= lim.max_samples, "n_samples must be in [0, %s], got %lld", lim.max_samples_text,
                   (long long)n_samples);
    FV3HIP_REQUIRE(n >= 1 && n <= lim.max_n, "n must be in [1, %d], got %d", lim.max_n, n);
    return FV3HIP_OK;
}

// a layer must not read what it writes: two slices of one buffer (same base, row length, stride and edge) must be disjoint in
// channels; two buffers must not overlap -- except, where the caller allows it, that cubes laid out with one common sample
// stride may interleave (time i and time i + 1 of a rollout array [sample][time][cube])
inline int check_no_alias(const Slice &a, const Slice &b, int64_t n_samples, bool may_interleave)
{
    if (a.p == b.p && a.ld == b.ld && a.ss == b.ss && a.n == b.n) {
        FV3HIP_REQUIRE(a.off + a.c <= b.off || b.off + b.c <= a.off,
                       "source channels [%lld, %lld) and destination channels [%lld, %lld) of one buffer overlap", (long long)a.off,
                       (long long)(a.off + a.c), (long long)b.off, (long long)(b.off + b.c));
        return FV3HIP_OK;
    }
    if (n_samples == 0) return FV3HIP_OK;
    const int64_t a_cube = 6LL * a.n * a.n * a.ld, b_cube = 6LL * b.n * b.n * b.ld;
    const uintptr_t a0 = (uintptr_t)a.p, a1 = a0 + (uintptr_t)((n_samples - 1) * a.ss + a_cube) * 4;
    const uintptr_t b0 = (uintptr_t)b.p, b1 = b0 + (uintptr_t)((n_samples - 1) * b.ss + b_cube) * 4;
    if (a1 <= b0 || b1 <= a0) return FV3HIP_OK;
    if (may_interleave && a.ss == b.ss) {   // the cubes of b sit in the gaps between the cubes of a
        const uintptr_t period = (uintptr_t)a.ss * 4;
        const uintptr_t shift = b0 >= a0 ? (b0 - a0) % period : (period - (a0 - b0) % period) % period;
        if (shift >= (uintptr_t)a_cube * 4 && shift + (uintptr_t)b_cube * 4 <= period) return FV3HIP_OK;
    }
    return fail(FV3HIP_EINVAL, "source and destination buffers overlap");
}

}  // namespace fv3hip
