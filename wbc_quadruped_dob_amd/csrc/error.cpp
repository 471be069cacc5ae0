// The library's error reporting: the thread-local message behind wbc_last_error() and the status names.  Plain C++ (no HIP header): the tick planner
// (tick_plan.cpp) links with this unit alone.
#include "host_internal.hpp"

static thread_local std::string g_err;
int wbc::fail(int code, const std::string& msg) { g_err = msg; return code; }

extern "C" const char* wbc_strerror(int st) {
  switch (st) {
    case WBC_OK: return "ok";
    case WBC_E_INVALID: return "invalid argument";
    case WBC_E_IO: return "cannot read URDF";
    case WBC_E_PARSE: return "URDF parse error";
    case WBC_E_TOPOLOGY: return "unsupported robot topology";
    case WBC_E_NODEVICE: return "no usable gfx950 device";
    case WBC_E_HIP: return "HIP runtime error";
    case WBC_E_CAPACITY: return "batch exceeds solver capacity";
    default: return "unknown status";
  }
}
extern "C" const char* wbc_last_error(void) { return g_err.c_str(); }
