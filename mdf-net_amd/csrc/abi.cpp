// ABI version + thread-local error string.
#include "common.h"

namespace mdf {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
static thread_local const char* g_last_launch = "";
void note_launch(const char* kernel) { g_last_launch = kernel; }
static thread_local int g_wgrad_plan[MDF_WGRAD_PLAN_FIELDS] = {-1, 0, 0, 0, 0, 0, 0, 0, 0};
void note_wgrad_plan(int form, int R, int TH, int tv, long long n_tiles, int gx, int gy, int gz, int split) {
  const int v[MDF_WGRAD_PLAN_FIELDS] = {form, R, TH, tv, (int)(n_tiles < 0x7fffffffll ? n_tiles : 0x7fffffffll), gx, gy, gz, split};
  for (int i = 0; i < MDF_WGRAD_PLAN_FIELDS; ++i) g_wgrad_plan[i] = v[i];
}
}  // namespace mdf

extern "C" int mdf_abi_version(void) { return MDF_ABI_VERSION; }
extern "C" const char* mdf_last_error(void) { return mdf::g_err; }
extern "C" const char* mdf_last_launch(void) { return mdf::g_last_launch; }
extern "C" int mdf_wgrad_last_plan(int* out, int n) {
  MDF_REQUIRE(out && n >= 0, "null pointer argument");
  for (int i = 0; i < n && i < MDF_WGRAD_PLAN_FIELDS; ++i) out[i] = mdf::g_wgrad_plan[i];
  return MDF_WGRAD_PLAN_FIELDS;
}
