// Status codes and the error type every entry point maps to its C-ABI status.
// Host-only (no HIP headers): the canonical reader includes this alone, so it
// also builds with plain g++ for the sanitizer targets (Makefile: asan, tsan).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>

namespace das {

constexpr uint32_t kNone = 0xFFFFFFFFu;

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

enum Status : int {
  DAS_S_OK = 0,
  DAS_E_INVALID = -1,     // bad argument / misuse          -> ValueError
  DAS_E_HIP = -2,         // HIP runtime failure            -> RuntimeError
  DAS_E_NOT_BUILT = -3,   // index not built                -> RuntimeError
  DAS_E_UNSUPPORTED = -4, // shape outside this build       -> NotImplementedError
  DAS_E_INTERNAL = -5,
  DAS_E_ATTRIBUTE = -6,   // the reference raises AttributeError here -> AttributeError
  DAS_E_SYNTAX = -7,      // malformed input where the reference asserts -> AssertionError
  DAS_E_LIMIT = -8,       // more work than the caller's limit allows   -> ValueError
};

#define DAS_CHECK(cond, code, msg)                 \
  do {                                             \
    if (!(cond)) throw ::das::Error((code), (msg)); \
  } while (0)

// The DAS_* environment switches are read through these helpers and nowhere
// else (here, not in das_internal.h: prims.h and the host-only reader use them
// too).  A call site is `static` when the switch is read once per process and
// plain when the tests flip it between calls; a site that tests one switch
// against several values reads it once with env_char.
inline const char* env_str(const char* name) { return std::getenv(name); }
inline bool env_set(const char* name) { return env_str(name) != nullptr; }
inline char env_char(const char* name) {          // the value's first character; 0: unset or empty
  const char* e = env_str(name);
  return e ? e[0] : '\0';
}
inline bool env_is(const char* name, char c) { return env_char(name) == c; }
inline long long env_int(const char* name, long long dflt) {
  const char* e = env_str(name);
  return e ? std::strtoll(e, nullptr, 10) : dflt;
}

}  // namespace das
