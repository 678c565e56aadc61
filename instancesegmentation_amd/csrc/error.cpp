// The error plumbing of libisg.so: the thread's last error message and launch name
// (include/isg.h isg_last_error / isg_last_launch; csrc/launch.h isg_set_error /
// isg_check_launch). On its own so that host programs can link it without the kernels.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/isg.h"
#include "launch.h"

static thread_local std::string g_last_error;

int32_t isg_set_error(int32_t code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// the name of the thread's latest launch (isg_last_launch): every `what` is a string literal
static thread_local const char* g_last_launch = "";

int32_t isg_check_launch(const char* what) {
    g_last_launch = what;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return isg_set_error(ISG_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return ISG_OK;
}

extern "C" {

const char* isg_last_error(void) { return g_last_error.c_str(); }
const char* isg_last_launch(void) { return g_last_launch; }

}  // extern "C"
