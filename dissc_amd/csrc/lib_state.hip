// Process-wide state of the library: the thread-local error string, the option defaults and their C entry points.  Host only.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"

namespace dissc {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

Options g_defaults;
thread_local const Options* t_opts = nullptr;
int g_graph_hits = 0, g_graph_captures = 0;

}  // namespace dissc

using namespace dissc;

extern "C" {

const char* dissc_last_error(void) { return g_err; }
int dissc_abi_version(void) { return 9; }

int dissc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int dissc_device_name(int dev, char* buf, size_t buflen) {
  hipDeviceProp_t p;
  DISSC_HIP_CHECK(hipGetDeviceProperties(&p, dev));
  snprintf(buf, buflen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
  return DISSC_OK;
}

// The DEFAULTS (what handles created later start from), whatever handle the calling thread may be working for
int dissc_get_option(const char* key, int* value) {
  if (!key || !value) return DISSC_EINVAL;
  if (strcmp(key, "graph_hits") == 0) { *value = g_graph_hits; return DISSC_OK; }
  if (strcmp(key, "graph_captures") == 0) { *value = g_graph_captures; return DISSC_OK; }
  if (strcmp(key, "experimental") == 0) { *value = DISSC_EXPERIMENTAL; return DISSC_OK; }
  // the tile-shape tables, under the keys dissc_set_option takes: "conv_cfg_bm16|32|64|128|256", "conv32_cfg_bm32|64|128|256"
  for (int cls = 0; cls < 5; ++cls) {
    char name[32];
    snprintf(name, sizeof name, "conv_cfg_bm%d", 16 << cls);
    if (strcmp(key, name) == 0) { *value = g_defaults.cfg_for_bm[cls]; return DISSC_OK; }
    snprintf(name, sizeof name, "conv32_cfg_bm%d", 32 << cls);
    if (cls < 4 && strcmp(key, name) == 0) { *value = g_defaults.cfg32_for_bm[cls]; return DISSC_OK; }
  }
#define DISSC_OPT_GET(f, d, k) if (strcmp(key, k) == 0) { *value = g_defaults.f; return DISSC_OK; }
  DISSC_OPTION_LIST(DISSC_OPT_GET)
#undef DISSC_OPT_GET
  set_error("dissc_get_option: unknown key %s", key);
  return DISSC_EINVAL;
}

int dissc_set_option(const char* key, int value) {
  if (!key) return DISSC_EINVAL;
  if (strncmp(key, "conv_cfg_bm", 11) == 0) {  // "conv_cfg_bm16|32|64|128|256" -> tile config id
    const int bm = atoi(key + 11);
    int cls = 0;
    while ((16 << cls) < bm) ++cls;
    conv_set_cfg(cls, value);
    return DISSC_OK;
  }
  if (strncmp(key, "conv32_cfg_bm", 13) == 0) {
    const int bm = atoi(key + 13);
    int cls = 0;
    while ((32 << cls) < bm) ++cls;
    conv32_set_cfg(cls, value);
    return DISSC_OK;
  }
  if (strcmp(key, "pairw_chv") == 0) value = value == 2 ? 2 : 1;
#define DISSC_OPT_SET(f, d, k) if (strcmp(key, k) == 0) { g_defaults.f = value; return DISSC_OK; }
  DISSC_OPTION_LIST(DISSC_OPT_SET)
#undef DISSC_OPT_SET
  set_error("dissc_set_option: unknown key %s", key);
  return DISSC_EINVAL;
}

}  // extern "C"
