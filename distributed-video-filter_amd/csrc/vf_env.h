// vf_env.h — the library's environment readers: every VF_* switch under csrc/ goes through one
// of these three.  Host-only, no HIP.  Not installed.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace vf {

// The value, or nullptr when the variable is unset.
inline const char *env_str(const char *name) { return std::getenv(name); }

// An unsigned number (strtoull base 0: decimal, 0x.., 0..); unset, empty or malformed: dflt.
inline size_t env_size(const char *name, size_t dflt) {
  const char *v = env_str(name);
  if (!v || !*v) return dflt;
  char *end = nullptr;
  const unsigned long long x = std::strtoull(v, &end, 0);
  return (end && *end == 0) ? (size_t)x : dflt;
}

// An on-by-default flag: off only when the value is exactly "0".
inline bool flag_on(const char *v) { return !(v && std::strcmp(v, "0") == 0); }
inline bool env_on(const char *name) { return flag_on(env_str(name)); }

}  // namespace vf
