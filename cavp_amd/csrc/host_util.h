// Host-side helpers shared by the extern "C" entry points of every csrc/*.hip: argument checks, the launch status and the
// run-time dtype -> element type dispatch.  No device code lives here (that is common.h).
#pragma once
#include <type_traits>

#include "common.h"

inline bool dt_ok(int dt) { return dt == CAVP_F32 || dt == CAVP_BF16; }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// elements per 16-byte vector of a (validated) dtype code: Elem<T>::VE on the host
inline int dt_ve(int dt) { return dt == CAVP_F32 ? 4 : 8; }

// status of the launches since the last check
inline int launch_status() { return hipGetLastError() == hipSuccess ? CAVP_OK : CAVP_ERR_LAUNCH; }
#define CHECK_LAUNCH() return launch_status()

// f(T{}) with T = float / bf16_t for a dtype code the caller has validated (dt_ok), f32 instantiated first:
//   cavp_dispatch_dtype(dtype, [&](auto t) { using T = decltype(t);
//     kernel<T><<<grid, 256, 0, s>>>((const T*)x, (T*)y, n); });
// A pointer that has the same type for both dtypes (f32 statistics, ...) is passed as it is; a compile-time switch
// beside the dtype (kernel<T, true> / kernel<T, false>) stays inside the lambda.
template <typename F>
inline void cavp_dispatch_dtype(int dtype, F&& f) {
  if (dtype == CAVP_F32)
    f(float{});
  else
    f(bf16_t{});
}

// f(std::true_type{}) or f(std::false_type{}): a run-time flag becomes a template argument, true instantiated first:
//   cavp_dispatch_bool(vec, [&](auto v) { kernel<decltype(v)::value><<<grid, 256, 0, s>>>(x, n); });
template <typename F>
inline void cavp_dispatch_bool(bool flag, F&& f) {
  if (flag)
    f(std::true_type{});
  else
    f(std::false_type{});
}
