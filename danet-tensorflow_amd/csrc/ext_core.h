/*
 * The host core of an extension library (every libdanet_<name>_hip.so; the core library keeps common.h and
 * error.cpp), once: the 16-byte vector type, the thread-local message, the two exports every library's header
 * declares, and the two checks an entry point returns through.  The one source of a library names its prefix twice
 * and includes this after its own header:
 *
 *     #include "danet_mix_hip.h"
 *     #define DANET_EXT mix
 *     #define DANET_EXT_UPPER MIX
 *     #include "ext_core.h"
 *
 * which defines danet_mix_last_error, danet_mix_abi_version (= DANET_MIX_ABI_VERSION), set_error(fmt, ...),
 * CHECK_ARG(cond, fmt, ...) -> return DANET_MIX_ERR_ARG and CHECK_LAUNCH() -> return DANET_MIX_ERR_LAUNCH.
 * __FILE__ and __LINE__ of a launch failure are those of the CHECK_LAUNCH() line.
 */
#ifndef DANET_EXT_CORE_H
#define DANET_EXT_CORE_H

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#if !defined(DANET_EXT) || !defined(DANET_EXT_UPPER)
#error "define DANET_EXT and DANET_EXT_UPPER (e.g. mix and MIX) before including ext_core.h"
#endif

#define DANET_EXT_CAT_(a, b, c) a##b##c
#define DANET_EXT_CAT(a, b, c) DANET_EXT_CAT_(a, b, c)

typedef float f32x4 __attribute__((ext_vector_type(4)));

static thread_local char g_err[512] = "";

static void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* DANET_EXT_CAT(danet_, DANET_EXT, _last_error)(void) { return g_err; }
extern "C" int DANET_EXT_CAT(danet_, DANET_EXT, _abi_version)(void) {
  return DANET_EXT_CAT(DANET_, DANET_EXT_UPPER, _ABI_VERSION);
}

#define CHECK_ARG(cond, ...)                                    \
  do {                                                          \
    if (!(cond)) {                                              \
      set_error(__VA_ARGS__);                                   \
      return DANET_EXT_CAT(DANET_, DANET_EXT_UPPER, _ERR_ARG);  \
    }                                                           \
  } while (0)

#define CHECK_LAUNCH()                                                                          \
  do {                                                                                          \
    const hipError_t e_ = hipGetLastError();                                                    \
    if (e_ != hipSuccess) {                                                                     \
      set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
      return DANET_EXT_CAT(DANET_, DANET_EXT_UPPER, _ERR_LAUNCH);                               \
    }                                                                                           \
  } while (0)

#endif
