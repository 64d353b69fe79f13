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

// f(T{}) with T the unsigned word of elem_size bytes (4 or 8) / the float type of a dtype code (F32 or F64) /
// f(Ta{}, Tb{}) for two dtype codes; the caller has checked the code (is_float).
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

template <typename Fn>
auto with_float_pair(int a_dtype, int b_dtype, Fn f)
{
    return with_float(a_dtype, [&](auto a) { return with_float(b_dtype, [&](auto b) { return f(a, b); }); });
}

inline bool is_float(int dtype) { return dtype == FV3HIP_F32 || dtype == FV3HIP_F64; }

// An untyped array argument as the T array that a dispatch lambda launches on (const stays const).
template <typename T>
T *as(void *p)
{
    return static_cast<T *>(p);
}
template <typename T>
const T *as(const void *p)
{
    return static_cast<const T *>(p);
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

// A scratch buffer kept with a handle and grown on demand: a first call, or one that needs more than any before, allocates
// -- so warm a model up before capturing a graph.  After a failed hipMalloc the handle holds a null pointer and size 0
// (its destroy frees whatever it holds).
inline int grow(void **p, size_t *have, size_t need)
{
    if (*have >= need) return FV3HIP_OK;
    if (*p) FV3HIP_CHECK_HIP(hipFree(*p));
    *p = nullptr;
    *have = 0;
    FV3HIP_CHECK_HIP(hipMalloc(p, need));
    *have = need;
    return FV3HIP_OK;
}

constexpr int kWave = 64;  // gfx950 wavefront

using f32x16 = __attribute__((ext_vector_type(16))) float;   // the accumulator of one 32 x 32 MFMA tile

// Running maximum of np.max: NaN once any value is NaN, so that `logit == max` is hot nowhere in a column of class logits
// with a NaN (the one-hot decode of emulation.hip and local.hip: logits == np.max(logits), ties all hot).
template <typename T>
__device__ __forceinline__ T running_max(T mx, T v)
{
    return (v > mx || v != v) ? v : mx;
}

// Element i of an F32 or F64 array as T: (float) of a float64 is the Keras cast to the layer dtype, (double) holds either
// dtype exactly.
template <typename T>
__device__ __forceinline__ T load_as(const void *p, int dtype, int64_t i)
{
    return dtype == FV3HIP_F64 ? (T) static_cast<const double *>(p)[i] : (T) static_cast<const float *>(p)[i];
}

// np.max over the classes of column i of logits [n_class][n]; class c is hot where load_as<double>(its logit) equals it.
__device__ __forceinline__ double class_max(const void *logits, int dtype, int n_class, int64_t n, int64_t i)
{
    double mx = load_as<double>(logits, dtype, i);
    for (int c = 1; c < n_class; ++c) mx = running_max(mx, load_as<double>(logits, dtype, (int64_t)c * n + i));
    return mx;
}

}  // namespace fv3hip
