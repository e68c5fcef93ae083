// require.hpp — the argument check of the C entry points and the error it records, as common.hpp has
// them but without any HIP header, for the plain C++ twins that also build on their own as host
// programs (monoinit_third.cpp).  common.hpp keeps its own text (the committed profiler summaries are
// keyed to its hash); monoinit_third.hip includes both with -Wmacro-redefined as an error, so the
// build fails if the two ever differ.
#pragma once

#include <string>

namespace mage {

// Thread-local last error (mage_last_error()).
void set_error(const std::string& msg);

}  // namespace mage

#define MAGE_REQUIRE(cond, code, msg)                                                       \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            ::mage::set_error(msg);                                                         \
            return code;                                                                    \
        }                                                                                   \
    } while (0)
