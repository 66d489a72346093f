// Ownership of device and pinned host memory: every buffer of the engine is a DevBuf / PinBuf, freed by its destructor.
// No HIP header here: the allocations go through the two funnel pairs below, defined once in engine.cpp (tests/devbuf_host_main.cpp
// puts them over malloc to run this header under the host sanitizers).
#pragma once
#include "../../include/st2.h"

#include <stddef.h>

#include <type_traits>

namespace st2e {
// The funnel.  alloc: ST_OK, or ST_ERR_HIP with the message set and *p untouched; free swallows a sticky error.  `bytes` is the
// requested size on both sides: the live-byte counters behind st_live_bytes are exact sums of requests.
int raw_alloc(void** p, size_t bytes);
void raw_free(void* p, size_t bytes);
int raw_pin_alloc(void** p, size_t bytes);
void raw_pin_free(void* p, size_t bytes);

// Move-only owner of `cap()` elements of T.  alloc(n) re-makes the buffer with exactly n elements, reserve(n) only grows it; both free
// the old block BEFORE they allocate (the peak at a grow is max(old, new)) and leave the buffer empty when the allocation fails.
// The block is never smaller than 1 element, 8 for bf16 (unsigned short): kernels read whole vectors at the tail.
template <class T, bool Pinned = false>
class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;
    static size_t bytes(size_t n)
    {
        const size_t least = std::is_same<T, unsigned short>::value ? 8 : 1;
        return (n > least ? n : least) * sizeof(T);
    }

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    void reset()
    {
        if (p_) (Pinned ? raw_pin_free : raw_free)(p_, bytes(cap_));
        p_ = nullptr; cap_ = 0;
    }
    int alloc(size_t n)
    {
        reset();
        void* q = nullptr;
        const int rc = (Pinned ? raw_pin_alloc : raw_alloc)(&q, bytes(n));
        if (rc != ST_OK) return rc;
        p_ = static_cast<T*>(q); cap_ = n;
        return ST_OK;
    }
    int reserve(size_t n) { return n > cap_ ? alloc(n) : ST_OK; }

    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    operator T*() const { return p_; }       // launch sites pass the buffer where they passed the raw pointer
};
template <class T> using PinBuf = DevBuf<T, true>;
}  // namespace st2e
