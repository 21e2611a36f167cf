// host.h — what the host side of all nine libraries shares: the thread-local error text behind each library's *_last_error(), the
// last-launch text behind *_last_launch() of the four grouped decode libraries, the launch check, and the small argument predicates.  Host code only; the two element types come from elem_types.h.
//
// Included by the ONE source file of a library that owns its error text: the source of each satellite library, and api.hip for
// libmbnb_hip.so, whose kernel sources include common.h alone and report through its set_error() / check_launch().  The functions
// have internal linkage and the text lives inside last_error(), so each of those files, and so each shared object, has exactly one
// buffer.  (with_dtype is a template, with ordinary linkage; its instantiations take a file's own lambdas.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "elem_types.h"

namespace mbnb {

constexpr int kErrorBytes = 512;

static char *last_error() {
    static thread_local char text[kErrorBytes] = "";
    return text;
}

// the text behind *_last_launch() of the libraries that have one: the form of this thread's last fused launch, written with
// snprintf(last_launch(), kLaunchBytes, ...) after a launch that succeeded
constexpr int kLaunchBytes = 128;

static char *last_launch() {
    static thread_local char text[kLaunchBytes] = "";
    return text;
}

// the one writer of the error text; returns `code` so that a check reads `return fail(...)`
static int vfail(int code, const char *fmt, va_list ap) {
    vsnprintf(last_error(), kErrorBytes, fmt, ap);
    return code;
}
static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    code = vfail(code, fmt, ap);
    va_end(ap);
    return code;
}

// after a launch: 0, or the hipError_t with "<what>: kernel launch failed: <hip text>" recorded
static int launch_status(const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail((int)e, "%s: kernel launch failed: %s", what, hipGetErrorString(e));
}

// The element-type codes of every public header (MBNB_F16, MBNB_TRAIN_F16, ...): a library that uses the helpers below states
// with static_asserts next to its include that its own enum has these values.
constexpr int kF16 = 0, kBF16 = 1, kF32 = 2;

static bool is16(int dtype) { return dtype == kF16 || dtype == kBF16; }
static int esize(int dtype) { return dtype == kF32 ? 4 : 2; }
static bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
static int64_t round256(int64_t b) { return (b + 255) & ~(int64_t)255; }
constexpr int64_t kMaxElems = (int64_t)1 << 38;   // element counts: every flat grid of 256-thread workgroups stays below 2^31

// dispatch on the element type: f(T{}) with T = f16_t / bf16_t / float
template <typename F> int with_dtype(int dtype, F &&f) {
    switch (dtype) {
        case kF16: return f(f16_t{});
        case kBF16: return f(bf16_t{});
        default: return f(float{});
    }
}

}  // namespace mbnb
