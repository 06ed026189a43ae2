// host/error.h — the library's one global message slot, read through dhw_last_error(NULL): errors of calls that have no
// handle (dhw_create, dhw_schedule, dhw_render, dhw_page, dhw_paths, dhw_truth, dhw_encode, dhw_prep, dhw_moments_update).  The slot itself lives in dhw_api.cpp.
#pragma once
#include <cstdarg>

#include "../abi_guard.h"

#pragma GCC visibility push(hidden)
void set_global_error(const char* fmt, va_list ap) noexcept;
#pragma GCC visibility pop

// records the message in the global slot and returns code: `return global_fail(DHW_ERR_ARG, "...", ...)`
__attribute__((format(printf, 2, 3))) inline int global_fail(int code, const char* fmt, ...) noexcept {
  va_list ap;
  va_start(ap, fmt);
  set_global_error(fmt, ap);
  va_end(ap);
  return code;
}
// the body of every handle-less extern "C" entry point runs inside this: no exception leaves the library (abi_guard.h)
#define GLOBAL_GUARD(fn, R, ...) \
  return abi_guard<R>(fn, [&](const char* f_, const char* w_) { return global_fail(DHW_ERR_INTERNAL, "%s: internal error: %s", f_, w_); }, [&]() -> R __VA_ARGS__)
