// launch.h -- "did HIP accept that?", written once for the whole library: a function that fails in HIP returns TW_E_HIP
// and leaves the hipError_t and a message for tw_last_hip_error() / tw_last_error_message() (include/twoarmy.h).  The
// state is one copy per process (C++17 inline variables, hidden: the library exports nothing new).  Host code only; a
// host compiler takes this file too (tests/test_launch_cpu.py).
#ifndef TWOARMY_LAUNCH_H
#define TWOARMY_LAUNCH_H
#include <hip/hip_runtime_api.h>
#include <stdio.h>

#include "twoarmy.h"

#define TW_HIDDEN __attribute__((visibility("hidden")))
TW_HIDDEN inline int g_last_hip_error = 0;
TW_HIDDEN inline char g_last_error_msg[256] = "";

// Record a failed HIP call: `what` is the expression, or the ABI function whose launch failed.
TW_HIDDEN inline int tw_fail(hipError_t e, const char *what, int line) {
    g_last_hip_error = (int)e;
    snprintf(g_last_error_msg, sizeof(g_last_error_msg), "%s (line %d): %s", what, line, hipGetErrorString(e));
    return TW_E_HIP;
}

// Result of an ABI function whose last act was a kernel launch; `what` is that function's own name.
TW_HIDDEN inline int tw_launched(const char *what, int line = __builtin_LINE()) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? TW_OK : tw_fail(e, what, line);
}
TW_HIDDEN inline hipError_t tw_launch_status() { return hipGetLastError(); }    // for code that cleans up before it reports

#define hip_fail(e) tw_fail((e), "hip", __LINE__)
#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return tw_fail(_e, #expr, __LINE__); } while (0)
#define HIP_TRY_LAUNCHED() HIP_TRY(hipGetLastError())
#endif  // TWOARMY_LAUNCH_H
