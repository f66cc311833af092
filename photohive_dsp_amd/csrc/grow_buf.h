// grow_buf.h -- the context's grow-only blocks (host only, no HIP here: the
// memory kinds DeviceMem and PinnedMem are in phd_host.h).
#pragma once

#include <cstddef>

namespace phd {

// A grow-only block of at least the bytes last asked for.  Mem: static
// void* alloc(size_t) (nullptr: failed), free(void*), idle(), failed(size_t)
// (sets the error of a failed allocation of that size).
template <class Mem>
struct GrowBuf {
    // keeps the block iff there is one of at least `need` bytes; else a new one of
    // need + 25 % + 4096.  The old block is freed only once Mem is idle: freed under
    // an in-flight copy or kernel it would be a use-after-unmap (every entry drains its
    // streams before it returns: belt and braces).  Failure leaves {nullptr, 0}.
    bool ensure(size_t need) {
        if (p_ && cap_ >= need) return true;
        if (p_) Mem::idle();
        release();
        const size_t sz = need + need / 4 + 4096;
        if (!(p_ = Mem::alloc(sz))) return Mem::failed(sz), false;
        cap_ = sz;
        return true;
    }
    void release() {
        if (p_) Mem::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    template <class T = void> T* as() const { return static_cast<T*>(p_); }
    size_t capacity() const { return cap_; }
private:
    void* p_ = nullptr;
    size_t cap_ = 0;
};

// A device block and the pinned block its table goes up from and its results
// come down to (the copies: Staged, phd_host.h).
template <class Dev, class Pin>
struct StagedBuf {
    GrowBuf<Dev> d;
    GrowBuf<Pin> h;
    bool reserve(size_t dev_bytes, size_t pin_bytes) { return d.ensure(dev_bytes) && h.ensure(pin_bytes); }
    void release() { d.release(), h.release(); }
};

}  // namespace phd
