// The C boundary of the library: rt_last_error's text, and the one guard every extern "C" entry point runs its body in, so that nothing
// throws across the boundary.
#pragma once
#include <exception>
#include <string>
#include "../../../include/rtamd.h"
#include "hip_check.h"

namespace rtamd {

void set_error(const std::string &msg); // what rt_last_error returns on this thread (rtamd_scene.hip)

namespace { // internal linkage: the library exports none of these helpers

inline int fail(int code, const std::string &msg) {
    set_error(msg);
    return code;
}

// Runs `body` (an rt_status, or a count >= 0) and maps what it throws: HipError (HIP_CHECK) -> RT_ERR_HIP, any other std::exception
// (std::bad_alloc, the std::system_error of a thread that could not start, a scene the preparation refuses) -> `other`, anything else
// -> `other` with "unknown exception".  The message is `who` + what().  `other` is RT_ERR_INVALID_ARG except for the file front-end.
template <class F> int guarded(const std::string &who, F &&body, int other = RT_ERR_INVALID_ARG) {
    try {
        return body();
    } catch (const HipError &e) {
        return fail(RT_ERR_HIP, who + e.what());
    } catch (const std::exception &e) {
        return fail(other, who + e.what());
    } catch (...) {
        return fail(other, who + "unknown exception");
    }
}

} // namespace
} // namespace rtamd
