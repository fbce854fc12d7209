// capi_common.hpp -- what the translation units of the C API (capi.hip, capi_apply.hip, capi_debug.hip) share: the calling thread's error text.
#pragma once
#include <string>

namespace sts {

extern thread_local std::string g_capi_err;       // what sts_last_error returns (defined in capi.hip)
inline int set_err(int code, const std::string& s) { g_capi_err = s; return code; }

}  // namespace sts
