// The one way to read an ST2_* environment switch.  Never cached: every call asks the environment again (the tests flip
// the switches between evaluations of one process).  README.md lists every name (tests/test_boundary.py compares the two).
#pragma once
#include <stdlib.h>

namespace st2 {

inline const char* env_get(const char* name) { const char* e = getenv(name); return e && *e ? e : nullptr; }      // unset or empty: nullptr
inline bool env_off(const char* name) { const char* e = env_get(name); return e && *e == '0'; }
inline bool env_on(const char* name) { const char* e = env_get(name); return e && *e == '1'; }
inline long long env_int(const char* name, long long dflt) { const char* e = env_get(name); return e ? atoll(e) : dflt; }

}  // namespace st2
