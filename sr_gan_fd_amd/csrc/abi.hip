// abi.hip -- the process-wide state of libsrganfd_hip.so and the three entry points that only touch it.  Every other extern "C"
// function of include/srganfd.h is defined in the .hip file of the kernels it launches, against the header's prototype.
#include "common.hpp"
#include <stdarg.h>
#include <stdlib.h>

namespace srganfd {
thread_local char g_err[512] = {0};
int g_dry_run = 0;
thread_local char* g_describe = nullptr;
thread_local size_t g_describe_len = 0;
int set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace srganfd

using namespace srganfd;

extern "C" {

const char* srganfd_last_error(void) { return g_err; }
int srganfd_abi_version(void) { return SRGANFD_ABI_VERSION; }
void srganfd_set_dry_run(int on) { g_dry_run = on ? 1 : 0; }

}  // extern "C"
