// Environment knobs (the TQ_* variables of INTEGRATION.md §8): the only readers of the
// environment in csrc/ (tq_capi.cpp's TQ_TRACE_FILE excepted: it needs the string).  Every knob is
// read through one of these, in one place, and that place decides whether the value is cached (a
// `static const` at the use site) or read on every call.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace tq {

// a switch that is on by default: off iff the value starts with '0'
inline bool env_on(const char* name) {
  const char* e = getenv(name);
  return !(e && e[0] == '0');
}
// a switch that is off by default: on iff the value starts with '1'
inline bool env_opt_in(const char* name) {
  const char* e = getenv(name);
  return e && e[0] == '1';
}
// presence only (any value, the empty string included)
inline bool env_set(const char* name) { return getenv(name) != nullptr; }
// a number: dflt when unset; a set value is clamped to [lo, hi] (the default is not)
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline int env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = getenv(name);
  return e ? std::max(lo, std::min(hi, atoi(e))) : dflt;
}
inline int64_t env_int64(const char* name, int64_t dflt) {
  const char* e = getenv(name);
  return e ? (int64_t)atoll(e) : dflt;
}
inline double env_double(const char* name, double dflt) {
  const char* e = getenv(name);
  return e ? atof(e) : dflt;
}

}  // namespace tq
