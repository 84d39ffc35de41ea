// drrt_host.h -- what the host halves of the translation units share: the library's error slot (defined in drrt_api.hip,
// one message buffer per host thread, read back by drrt_last_error()) and the launch of the one-thread-per-item operators
// (drrt_sensor.hip, drrt_ops.hip, drrt_source.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/drrt_hip.h"

namespace drrt {

int fail(int code, const char* msg);              // stores msg, returns code
int fail_hip(hipError_t e, const char* where);    // stores "where: <error string>", returns DRRT_ERR_HIP

// After the launches of a call: DRRT_OK, or the failed launch's error.
inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DRRT_OK : fail(DRRT_ERR_HIP, hipGetErrorString(e));
}

// One thread per item, 256 threads per block.
template <typename... P, typename... A>
inline int launch_1d(void (*kernel)(P...), size_t n, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, args...);
  return launch_status();
}

}  // namespace drrt
