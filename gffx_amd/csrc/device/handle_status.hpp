// handle_status.hpp -- what the device objects behind the C-ABI share around their state (closest, class map, pileup,
// profile, union): the first failure of the work on an object sticks to it -- every later call only reports it again --
// while a call that is refused for its arguments leaves the object usable.  Not part of the C-ABI.
#pragma once
#include <algorithm>
#include <string>

#include "gffx_device.hpp"

namespace gffx {

// The base of an object's struct.  The struct adds its two nouns for enter_handle's messages:
//   static constexpr const char *kName, *kNoun;    "<who>: <kName> is NULL", "<who>: the <kNoun> failed earlier: ..."
struct HandleStatus {
    int device = 0;
    int status = GFFX_OK;  // the first error: the object only reports it again
    std::string message;
};

inline int keep_failure(HandleStatus *h, int rc) {  // rc came from fail(): keep it and its message
    if (h->status == GFFX_OK) h->status = rc, h->message = g_last_error;
    return rc;
}
#define GFFX_KEEP_TRY(h, expr)                           \
    do {                                                 \
        const int _rc = (expr);                          \
        if (_rc) return ::gffx::keep_failure((h), _rc);  \
    } while (0)
// a HIP call of an entry point that works on the handle: its failure, too, is kept (argument errors are not: the call is
// refused and the handle stays usable)
#define GFFX_KEEP_HIP(h, expr) GFFX_KEEP_TRY(h, [&]() -> int { GFFX_HIP_TRY(expr); return GFFX_OK; }())

// the first step of every entry point `who`: the object is there, has not failed, and its device is current
template <class H>
int enter_handle(const H *h, const char *who) {
    if (!h) return fail(GFFX_E_INVALID, "%s: %s is NULL", who, H::kName);
    if (h->status != GFFX_OK) return fail(h->status, "%s: the %s failed earlier: %s", who, H::kNoun, h->message.c_str());
    GFFX_HIP_TRY(hipSetDevice(h->device));
    return GFFX_OK;
}

// room for n elements on the current device, for four at least (never an empty allocation)
template <typename T>
int dev_alloc_padded(T **p, uint64_t n) {
    *p = nullptr;
    GFFX_HIP_TRY(hipMalloc((void **)p, std::max<uint64_t>(n, 4) * sizeof(T)));
    return GFFX_OK;
}

}  // namespace gffx
