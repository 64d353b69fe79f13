// What reservoir.hip and codec.hip share (gram.hip: the device check alone): how the caller's strided (x, y, z) arrays and
// the z sizes of their variables reach a kernel, and who owns a handle's device buffers.
#pragma once
#include <vector>

#include "common.h"

namespace fv3hip {

// one variable's (x, y, z) array as a kernel reads it (strides in elements) / writes it
struct XyzSrc {
    const void *p;
    int64_t sx, sy, sz;
    int f64;
};

struct XyzDst {
    void *p;
    int64_t sx, sy, sz;
};

template <class T>
__device__ __forceinline__ T load_xyz(const XyzSrc &s, int64_t x, int64_t y, int64_t z)
{
    const int64_t off = x * s.sx + y * s.sy + z * s.sz;
    return s.f64 ? (T) static_cast<const double *>(s.p)[off] : (T) static_cast<const float *>(s.p)[off];
}

// the variable that holds level k of the concatenated column; zoff: the prefix sums of the z sizes
__device__ __forceinline__ int var_of(const int *zoff, int n_var, int k)
{
    int v = 0;
    while (v + 1 < n_var && k >= zoff[v + 1]) ++v;
    return v;
}

// zoff[0 .. n_var] of var_nz, after the checks on the count and on every size; `what` names the owner in the messages
// ("" for none)
inline int fill_zoff(const int *var_nz, int n_var, int max_vars, const char *what, int *zoff)
{
    const char *sep = *what ? ": " : "";
    FV3HIP_REQUIRE(n_var >= 1 && n_var <= max_vars, "%s%sn_variables must be in [1, %d], got %d", what, sep, max_vars, n_var);
    FV3HIP_REQUIRE(var_nz, "%s%snull var_nz", what, sep);
    zoff[0] = 0;
    for (int v = 0; v < n_var; ++v) {
        FV3HIP_REQUIRE(var_nz[v] >= 1 && var_nz[v] < (1 << 20), "%s%sbad z size %d of variable %d", what, sep, var_nz[v], v);
        zoff[v + 1] = zoff[v] + var_nz[v];
    }
    return FV3HIP_OK;
}

// The sources of one launch from the caller's tables.  strides_per_var 3: (x, y, z) arrays.  4: [t, x, y, z] arrays, of
// which this takes time t (the time stride comes first; the offset is in bytes of the source's dtype).  all_f32 (may be
// null): whether every source is float32.
inline int fill_sources(int n_var, const void *const *p, const int *dtype, const int64_t *strides, int strides_per_var,
                        int64_t t, XyzSrc *src, int *all_f32)
{
    FV3HIP_REQUIRE(p && dtype && strides, "null source pointer");
    int f32 = 1;
    for (int v = 0; v < n_var; ++v) {
        FV3HIP_REQUIRE(p[v], "source %d is null", v);
        FV3HIP_REQUIRE(is_float(dtype[v]), "source %d: dtype must be F32 or F64", v);
        const int f64 = dtype[v] == FV3HIP_F64 ? 1 : 0;
        const int64_t *s = strides + (int64_t)strides_per_var * v;
        const char *at = static_cast<const char *>(p[v]);
        if (strides_per_var == 4) at += t * *s++ * (f64 ? 8 : 4);
        src[v] = XyzSrc{at, s[0], s[1], s[2], f64};
        if (f64) f32 = 0;
    }
    if (all_f32) *all_f32 = f32;
    return FV3HIP_OK;
}

inline int fill_outputs(int n_var, void *const *p, const int64_t *strides, XyzDst *dst)
{
    FV3HIP_REQUIRE(p && strides, "null output pointer");
    for (int v = 0; v < n_var; ++v) {
        FV3HIP_REQUIRE(p[v], "output %d is null", v);
        dst[v] = XyzDst{p[v], strides[3 * v], strides[3 * v + 1], strides[3 * v + 2]};
    }
    return FV3HIP_OK;
}

// The device buffers of a handle: freed with it, also when its creation fails half way.
class DeviceAllocs {
public:
    DeviceAllocs() = default;
    DeviceAllocs(const DeviceAllocs &) = delete;
    DeviceAllocs &operator=(const DeviceAllocs &) = delete;
    ~DeviceAllocs()
    {
        for (void *q : bufs_) (void)hipFree(q);
    }

    // n elements (at least one, so that the pointer is never null), filled from `host` when given
    template <class T>
    int upload(T **dptr, const T *host, size_t n)
    {
        FV3HIP_CHECK_HIP(hipMalloc(reinterpret_cast<void **>(dptr), (n ? n : 1) * sizeof(T)));
        bufs_.push_back(*dptr);
        if (host && n) FV3HIP_CHECK_HIP(hipMemcpy(*dptr, host, n * sizeof(T), hipMemcpyHostToDevice));
        return FV3HIP_OK;
    }

    template <class T>
    int alloc(T **dptr, size_t n)
    {
        return upload<T>(dptr, nullptr, n);
    }

private:
    std::vector<void *> bufs_;
};

// the launches of a handle go to the device it was created on; `what`: "reservoir", "codec", ...
inline int check_handle_device(int handle_device, const char *what)
{
    int cur = -1;
    FV3HIP_CHECK_HIP(hipGetDevice(&cur));
    FV3HIP_REQUIRE(cur == handle_device, "the %s lives on device %d but the current device is %d", what, handle_device, cur);
    return FV3HIP_OK;
}

}  // namespace fv3hip
