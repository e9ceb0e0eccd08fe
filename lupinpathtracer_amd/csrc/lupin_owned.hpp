// Ownership of raw allocations, written once and without a HIP header: the allocate / free pair is a template parameter, so
// tests/owned_main.cpp runs this file over malloc / free under the sanitizers; lupin_internal.hpp instantiates it for HIP.
#pragma once
#include <cstddef>
#include <utility>

// An Owned holds one allocation or nothing and frees what it holds in its destructor.  Move-only.  Api provides `Error`, its
// value `success`, `static Error alloc(void **p, size_t bytes)` (sets *p only on success) and `static void free(void *p)`.
template <typename Api>
class Owned
{
    void *p_ = nullptr;

public:
    using Error = typename Api::Error;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); } return *this; }
    ~Owned() { reset(); }
    // *out holds `bytes` of new memory (what it held before is freed), or stays as it was if the allocation fails
    static Error make(size_t bytes, Owned *out)
    {
        Owned b;
        const Error e = Api::alloc(&b.p_, bytes);
        if (e == Api::success) *out = std::move(b);
        return e;
    }
    void reset() { if (p_) Api::free(std::exchange(p_, nullptr)); }   // frees now; the owner is empty afterwards
    void swap(Owned &o) noexcept { std::swap(p_, o.p_); }
    void *get() const { return p_; }
    template <typename T> T *as() const { return static_cast<T *>(p_); }
};

// *buf, a buffer its holder keeps from call to call, holds at least `bytes`: kept when it is large enough, replaced otherwise
// (the caller knows that nothing still uses the old one).  A failure keeps the old buffer and its recorded size.
template <typename Api>
static inline typename Api::Error grow_buffer(Owned<Api> *buf, size_t *have, size_t bytes)
{
    if (*have >= bytes) return Api::success;
    const typename Api::Error e = Owned<Api>::make(bytes, buf);
    if (e == Api::success) *have = bytes;
    return e;
}
