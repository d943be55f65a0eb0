// The error text of ONE shared library: the thread-local buffer, dvae::set_error (which the check macros of common.h report
// through) and the accessor that the library's dvae_*_last_error returns.  Every library keeps its own text, so this header is
// included by exactly one translation unit per library -- capi.hip and the score libraries' single sources -- and by nothing
// else: a second inclusion in one library is a duplicate definition of set_error at link time.
#pragma once
#include <stdarg.h>
#include <stdio.h>

namespace dvae {

static thread_local char g_last_error[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
  va_end(ap);
}

static inline const char* last_error() { return g_last_error; }

}  // namespace dvae
