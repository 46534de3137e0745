// The library's exception and its check macro: all that host-only headers (das_gmres_host.hpp) need of das_common.hpp.
#pragma once
#include <stdexcept>
#include <string>

#include "../../include/dafoam_amd.h"

namespace das {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define DAS_CHECK(cond, code, msg)                    \
    do {                                              \
        if (!(cond)) throw das::Error((code), (msg)); \
    } while (0)

}  // namespace das
