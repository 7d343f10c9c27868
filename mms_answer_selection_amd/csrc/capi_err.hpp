// csrc/capi_err.hpp -- how a C entry point of include/mms_layer.h reports a failure: the message is copied,
// truncated to fit, into the caller's buffer (which may be absent).
#ifndef MMS_CAPI_ERR_HPP_
#define MMS_CAPI_ERR_HPP_

#include <cstdio>
#include <string>

inline void set_err(char* err, int err_len, const std::string& m) {
  if (err && err_len > 0) std::snprintf(err, err_len, "%s", m.c_str());
}

#endif  // MMS_CAPI_ERR_HPP_
