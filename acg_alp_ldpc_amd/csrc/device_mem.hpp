// Owners of device and pinned host memory for the host code of the library.  Not part of the ABI.
// Every buffer the library allocates belongs to exactly one DeviceBuf / PinnedBuf: it is freed when its owner goes
// (a handle's members, a local of an entry point), so no return path can leak it.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "ldpc_internal.hpp"

namespace acg {

#define HIP_OK(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                       \
            return 10;                                                                          \
        }                                                                                       \
    } while (0)

struct DeviceMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void *p) { (void) hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void *p) { (void) hipHostFree(p); }
};

// Move-only owner of one allocation: a pointer and its size in bytes.
template <class Mem>
struct Owned {
    void *p = nullptr;
    size_t bytes = 0;
    Owned() = default;
    Owned(Owned &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    Owned &operator=(Owned &&o) noexcept {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~Owned() { reset(); }
    void reset() {
        if (p) Mem::release(p);
        p = nullptr;
        bytes = 0;
    }
    // Grow-only: afterwards the buffer holds at least `want` bytes (its contents are lost when it had to grow).
    // -> 0, or 10 with the error message set and the owner left empty.
    int reserve(size_t want) {
        if (want <= bytes) return 0;
        reset();
        HIP_OK(Mem::alloc(&p, want));
        bytes = want;
        return 0;
    }
    template <typename T = void>
    T *as() const { return static_cast<T *>(p); }
};
using DeviceBuf = Owned<DeviceMem>;
using PinnedBuf = Owned<PinnedMem>;

// A new device buffer holding h (room for at least min_elems elements, so an empty table still has an address).
// -> an empty owner, with the error message set, when the allocation or the copy fails.
template <typename T>
DeviceBuf upload(const std::vector<T> &h, size_t min_elems = 1) {
    DeviceBuf b;
    if (b.reserve(std::max(h.size(), min_elems) * sizeof(T))) return b;
    if (!h.empty() && hipMemcpy(b.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("hipMemcpy of a device table failed");
        b.reset();
    }
    return b;
}

// upload(h) with the owner kept in `keep` -> the device address, null on failure
template <typename T>
const T *upload_keep(const std::vector<T> &h, std::vector<DeviceBuf> &keep) {
    DeviceBuf b = upload(h);
    if (!b.p) return nullptr;
    keep.push_back(std::move(b));
    return keep.back().as<const T>();
}

}  // namespace acg
