// The RTAMD_* environment knobs.  Read at every call, never cached: tests and the benchmark change them between scene creations and
// renders of one process.  Ranges and clamps stay with the knob's user.
#pragma once
#include <cstdlib>

namespace rtamd {

static inline const char *env_str(const char *name) { return getenv(name); }                                      // null when unset
static inline bool env_flag(const char *name) { return getenv(name) != nullptr; }                                 // set, to whatever value
static inline int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; } // zero and negative values count
static inline int env_positive(const char *name, int dflt) { const int v = env_int(name, 0); return v > 0 ? v : dflt; } // anything below 1: the default
static inline double env_float(const char *name, double dflt) { const char *e = getenv(name); return e ? atof(e) : dflt; }

} // namespace rtamd
