// Shared host-side helpers for the haconvdr C-ABI library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>

#include "../../include/haconvdr.h"

namespace hac {

typedef unsigned long long u64;
typedef unsigned int u32;

// thread-local error slot behind hac_last_error()
std::string &last_error_slot();
int fail(int code, const char *fmt, ...);

#define HAC_HIP(expr)                                                                           \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return hac::fail(_e == hipErrorOutOfMemory ? HAC_ERR_OOM : HAC_ERR_HIP,             \
                             "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,   \
                             __LINE__);                                                         \
    } while (0)

#define HAC_TRY(expr)                 \
    do {                              \
        int _rc = (expr);             \
        if (_rc != HAC_OK) return _rc; \
    } while (0)

// RAII device guard: the library never leaves the caller's current device changed.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// A buffer its holder owns: freed when the holder is destroyed or assigned over, so a struct of these needs no list of what to
// release.  Movable (a std::vector of them may grow), never copied.  release_all(w) frees every buffer of a struct of them at once
// -- where the owner's destroy wants it: under its DeviceGuard, behind the stream's last work -- by assigning an empty struct over it.
template <hipError_t (*FREE)(void *)>
struct OwnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept { *this = std::move(o); }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept {   // (a swap: what this held goes when o does)
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~OwnedBuf() { release(); }
    void release() {
        if (p) (void)FREE(p);
        p = nullptr;
        cap = 0;
    }
};
template <class W>
void release_all(W &w) { w = W(); }

// device buffer that only ever grows
struct GrowBuf : OwnedBuf<hipFree> {
    int reserve(size_t bytes) {
        if (bytes <= cap) return HAC_OK;
        release();
        size_t want = bytes + bytes / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            e = hipMalloc(&p, bytes);
            want = bytes;
        }
        if (e != hipSuccess) {
            p = nullptr;
            return fail(HAC_ERR_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        }
        cap = want;
        // A NEW buffer starts out as zeros, whatever the allocator recycled (fresh pages, which is what a first search sees, are
        // zero; recycled ones are not).  This is hygiene, not a guarantee: a buffer that is REUSED rather than regrown still holds
        // what earlier calls left in it, so no kernel may read beyond a device-side count without masking (what fixed the hang a
        // soak run found in the device-decided fallback: gather_rows_kernel zeroes the rows behind the count, padded queries'
        // thresholds are NaN).  Growth is rare; the null-stream memset + wait keeps the fill ahead of every stream, which also
        // means that a call that has to GROW a workspace synchronizes once (include/haconvdr.h: warm up at the largest shape
        // before capturing a *_device call into a graph).
        if (hipMemset(p, 0, want) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) {
            (void)hipGetLastError();
            release();
            return fail(HAC_ERR_HIP, "hipMemset(%zu) of a new workspace failed", want);
        }
        return HAC_OK;
    }
};

// pinned host buffer that only ever grows, to exactly the size asked for (how far ahead to grow is the caller's rule;
// needed: the size a failure names when the caller asked for more than it needs)
struct PinBuf : OwnedBuf<hipHostFree> {
    int reserve(size_t bytes, size_t needed = 0) {
        if (bytes <= cap) return HAC_OK;
        release();
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(HAC_ERR_OOM, "hipHostMalloc(%zu) failed: %s", needed ? needed : bytes, hipGetErrorString(e));
        }
        cap = bytes;
        return HAC_OK;
    }
};

// A kernel whose launches may pass the default 64 KiB of dynamic LDS, and the most any of them asks for.  Each translation unit
// keeps one table of these: its attribute loop raises every entry's limit, and the launches size their LDS by the same names.
struct LdsKernel {
    const void *fn;
    size_t bytes;
    template <class F>
    LdsKernel(F *f, size_t b) : fn((const void *)f), bytes(b) {}
};

// ---- options of a handle: one table of these per handle, read by apply_option alone (the searches and forwards read the plain
// members the rows store into).  A value outside the documented set is an error, never a silent default: a mistyped value in a
// cross-check test would otherwise exercise the wrong kernels and still pass.
struct OptChoice { const char *text; int value; };
template <class O>
struct Option {
    const char *name = nullptr;
    OptChoice choices[7] = {};                           // choice: the allowed strings and what each stores (ends at a null text)
    long lo = 0, hi = -1;                                // integer: one whole decimal number in [lo, hi] ...
    bool or_auto = false;                                // ... or "auto", which stores 0
    void (*store)(O &, long) = nullptr;                  // where an accepted choice or integer goes
    bool (*custom)(O &, const char *) = nullptr;         // custom: parses and stores by itself, all or nothing; false = rejected
    const char *custom_set = nullptr;                    // ... and its allowed set, as the message names it
    void (*after)(O &) = nullptr;                        // runs once the value is stored

    static Option choice(const char *name, void (*store)(O &, long), std::initializer_list<OptChoice> cs, void (*after)(O &) = nullptr) {
        Option o;
        o.name = name; o.store = store; o.after = after;
        assert(cs.size() < 7);
        std::copy(cs.begin(), cs.end(), o.choices);
        return o;
    }
    static Option integer(const char *name, void (*store)(O &, long), long lo, long hi, bool or_auto = false) {
        Option o;
        o.name = name; o.store = store; o.lo = lo; o.hi = hi; o.or_auto = or_auto;
        return o;
    }
    static Option custom_form(const char *name, const char *set, bool (*custom)(O &, const char *), void (*after)(O &) = nullptr) {
        Option o;
        o.name = name; o.custom_set = set; o.custom = custom; o.after = after;
        return o;
    }
};
// a row's `store`: the member (or nested member) FIELD of the owner
#define HAC_OPT_TO(O, FIELD) [](O &o, long v) { o.FIELD = (decltype(o.FIELD))v; }

// who: "index" | "encoder", for the messages
template <class O, size_t N>
int apply_option(const char *who, const Option<O> (&table)[N], O &owner, const char *name, const char *value) {
    for (const Option<O> &o : table) {
        if (strcmp(o.name, name) != 0) continue;
        std::string set;   // the allowed values, for the message
        long v = 0;
        bool ok = false;
        if (o.custom) {
            ok = o.custom(owner, value);
            set = o.custom_set;
        } else if (o.choices[0].text) {
            for (const OptChoice &c : o.choices) {
                if (!c.text) break;
                if (!strcmp(c.text, value)) { ok = true; v = c.value; }
                set += std::string(set.empty() ? "" : " | ") + c.text;
            }
        } else {
            char *end = nullptr;
            v = strtol(value, &end, 10);
            ok = *value && !*end && v >= o.lo && v <= o.hi;
            if (o.or_auto && !strcmp(value, "auto")) { ok = true; v = 0; }
            set = std::string(o.or_auto ? "auto | " : "") + "an integer " + std::to_string(o.lo) + (o.hi == LONG_MAX ? " or more" : ".." + std::to_string(o.hi));
        }
        if (!ok) return fail(HAC_ERR_INVALID, "%s option %s = '%s': %s", who, name, value, set.c_str());
        if (o.store) o.store(owner, v);
        if (o.after) o.after(owner);
        return HAC_OK;
    }
    return fail(HAC_ERR_INVALID, "unknown %s option '%s'", who, name);
}

}  // namespace hac
