// The C boundary of libhmsg: include/hmsg.h promises an int status plus a last-error string, so no exception may leave an
// extern "C" function.  Every exported function that can throw runs its body under hmsg_boundary; nothing else in csrc/ maps an
// exception to a status.
//
// THE RULE (stated here and next to the status codes in include/hmsg.h, nowhere else):
//     hmsg_error                keeps its code and message
//     std::bad_alloc            HMSG_ERR_NOMEM,   "out of host memory"
//     any other std::exception  HMSG_ERR_INVALID, its what()
//     anything else             HMSG_ERR_INVALID, "unknown error"
#pragma once
#include "hmsg_common.h"
#include "hmsg_query.h"

#include <exception>
#include <new>
#include <type_traits>

// The exception in flight as an hmsg_error.  Call inside a `catch (...)`.
inline hmsg_error hmsg_current_error() noexcept {
    try {
        try {
            throw;
        } catch (const hmsg_error& e) {
            return e;
        } catch (const std::bad_alloc&) {
            return hmsg_error{HMSG_ERR_NOMEM, "out of host memory"};
        } catch (const std::exception& e) {
            return hmsg_error{HMSG_ERR_INVALID, e.what()};
        } catch (...) {
            return hmsg_error{HMSG_ERR_INVALID, "unknown error"};
        }
    } catch (...) {      // (no memory left even for the message)
        return hmsg_error{HMSG_ERR_NOMEM, std::string()};
    }
}

// Where a failed call's message goes: a handle's `err` field, or -- for entry points without a handle -- the function's name,
// which prints "name: message" to stderr.  A null sink drops the message.
struct hmsg_err_sink {
    std::string* str = nullptr;
    const char* name = nullptr;
    hmsg_err_sink(std::string* s) : str(s) {}
    hmsg_err_sink(const char* n) : name(n) {}
    hmsg_err_sink(std::nullptr_t) {}
    void put(hmsg_error& e) const noexcept {
        if (str) str->swap(e.msg);
        else if (name) fprintf(stderr, "%s: %s\n", name, e.msg.c_str());
    }
};

// Runs fn and returns HMSG_OK, or the status of what it threw (the message goes to the sink).  device >= 0: hipSetDevice(device)
// first, as part of the guarded body.
template <typename F>
int hmsg_boundary(hmsg_err_sink sink, int device, F&& fn) noexcept {
    static_assert(std::is_void<decltype(fn())>::value, "the guarded body reports failure by throwing, not by a return value");
    try {
        if (device >= 0) HIP_TRY(hipSetDevice(device));
        fn();
        return HMSG_OK;
    } catch (...) {
        hmsg_error e = hmsg_current_error();
        sink.put(e);
        return e.code;
    }
}
// the handles that carry a device: message to the handle, its device made current
template <typename F>
int hmsg_boundary(hmsg_ctx* h, F&& fn) noexcept {
    return hmsg_boundary(&h->err, h->cfg.device_id, fn);
}
template <typename F>
int hmsg_boundary(hmsg_index* ix, F&& fn) noexcept {
    return hmsg_boundary(&ix->err, ix->device, fn);
}
