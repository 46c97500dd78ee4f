// Options, tuning knobs and the calling thread's error message (tuning.cpp): plain C++, no HIP.  Private to the library; what
// is not part of the C ABI is hidden from the dynamic symbol table.
#pragma once
#include "../../include/nkp.h"

#include <string>

#define NKP_PRIVATE __attribute__ ((visibility ("hidden")))

// the error reporter behind nkp_last_error: formats the calling thread's message and returns `code`
NKP_PRIVATE int fail (int code, const char *fmt, ...) __attribute__ ((format (printf, 2, 3)));
// a step that reports on behalf of all ranks keeps a rank's own message across the collective
NKP_PRIVATE std::string last_error_message ();
NKP_PRIVATE void restore_error_message (const std::string &text);

// the tuning a launcher uses when its object carries none: the plain defaults (no environment)
const nkp_tuning &nkp_builtin_tuning ();
// the caller's knobs, or the defaults + environment (the one place a solver looks at the environment); *range_error tells a
// value out of range (out is filled) from a struct of the wrong size (out is not)
NKP_PRIVATE int resolve_tuning (const nkp_options *opt, nkp_tuning *out, bool *range_error = nullptr);
