// host/error.h — the library's one global message slot, read through dhw_last_error(NULL): errors of calls that have no
// handle (dhw_create, dhw_schedule, dhw_render).  The slot itself lives in dhw_api.cpp.
#pragma once
#include <cstdarg>

#pragma GCC visibility push(hidden)
void set_global_error(const char* fmt, va_list ap) noexcept;
#pragma GCC visibility pop
