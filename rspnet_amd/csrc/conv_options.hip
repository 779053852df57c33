// The planning options of the convolution launchers (conv_igemm.hip, conv_wgrad.hip): ONE table (RSP_CONV_OPTIONS, common.h) of
// name, environment variable, kind and built-in default.  Host code only.
//
// An option's effective value is, in this order: what rsp_conv3d_set_option stored (>= 0), the environment variable, the default.
// The variable is read once per process, on the option's first use.  A FLAG variable counts as set when it is present at all (an
// empty value and "0" included: README and tools/ab_*.sh use the variables that way); an integer variable goes through atoi.
#include "common.h"
#include <atomic>
#include <climits>

namespace {

struct ConvOption {
  const char* name;
  const char* env;
  bool flag;
  int dflt;
  std::atomic<int> set{-1};              // >= 0: stored by rsp_conv3d_set_option; -1: the environment / the default
  std::atomic<int> env_value{INT_MIN};   // INT_MIN: the variable has not been read yet
};

#define RSP_OPTION_ROW(id, name, env, flag, dflt) {name, env, flag, dflt},
ConvOption g_options[RSP_OPT_COUNT] = {RSP_CONV_OPTIONS(RSP_OPTION_ROW)};
#undef RSP_OPTION_ROW

int from_environment(ConvOption& o) {
  int v = o.env_value.load(std::memory_order_relaxed);
  if (v == INT_MIN) {
    const char* e = getenv(o.env);
    v = !e ? o.dflt : (o.flag ? 1 : atoi(e));
    o.env_value.store(v, std::memory_order_relaxed);
  }
  return v;
}

}  // namespace

int rsp_conv_option(RspConvOption id) {
  ConvOption& o = g_options[id];
  const int set = o.set.load(std::memory_order_relaxed);
  return set >= 0 ? set : from_environment(o);
}

extern "C" int rsp_conv3d_set_option(const char* name, int32_t value) {
  for (int i = 0; name && i < RSP_OPT_COUNT; ++i) {
    if (strcmp(name, g_options[i].name)) continue;
    const int prev = rsp_conv_option((RspConvOption)i);
    g_options[i].set.store(value < 0 ? -1 : value, std::memory_order_relaxed);
    return prev;
  }
  rsp_set_error("rsp_conv3d_set_option: unknown option");
  return RSP_EINVAL;
}
