// Shared helpers for libfv3hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/fv3hip.h"

namespace fv3hip {

// Thread-local message of the last failure (fv3hip_last_error()).
char *last_error_buffer();
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define FV3HIP_CHECK_HIP(expr)                                                              \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return ::fv3hip::fail(FV3HIP_EHIP, "%s failed: %s (%s:%d)", #expr,              \
                                  hipGetErrorString(_e), __FILE__, __LINE__);               \
    } while (0)

#define FV3HIP_REQUIRE(cond, ...)                                       \
    do {                                                                \
        if (!(cond)) return ::fv3hip::fail(FV3HIP_EINVAL, __VA_ARGS__); \
    } while (0)

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Blocks of 256 threads for a grid-stride loop over `total` elements: one pass while they fit 64 blocks per CU.
inline unsigned grid_stride_blocks(int64_t total)
{
    const int64_t blocks = ceil_div(total, 256);
    return (unsigned)(blocks < 256 * 64 ? blocks : 256 * 64);
}

// f(T{}) with T the unsigned word of elem_size bytes (4 or 8) / the float type of a dtype code (F32 or F64); the
// caller has checked the code.
template <typename Fn>
auto with_word(int elem_size, Fn f)
{
    return elem_size == 4 ? f(uint32_t{}) : f(uint64_t{});
}

template <typename Fn>
auto with_float(int dtype, Fn f)
{
    return dtype == FV3HIP_F64 ? f(double{}) : f(float{});
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// After a launch: surface launch-configuration errors without synchronising.
inline int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FV3HIP_EHIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return FV3HIP_OK;
}

// A host vector to a fresh device buffer (an empty one: no buffer).  On failure the caller destroys its handle, which
// frees what was uploaded before.
template <typename T>
int upload(const std::vector<T> &v, void **dptr)
{
    *dptr = nullptr;
    if (v.empty()) return FV3HIP_OK;
    FV3HIP_CHECK_HIP(hipMalloc(dptr, v.size() * sizeof(T)));
    FV3HIP_CHECK_HIP(hipMemcpy(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return FV3HIP_OK;
}

constexpr int kWave = 64;  // gfx950 wavefront

// Running maximum of np.max: NaN once any value is NaN, so that `logit == max` is hot nowhere in a column of class logits
// with a NaN (the one-hot decode of emulation.hip and local.hip: logits == np.max(logits), ties all hot).
template <typename T>
__device__ __forceinline__ T running_max(T mx, T v)
{
    return (v > mx || v != v) ? v : mx;
}

}  // namespace fv3hip
