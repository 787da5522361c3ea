// Growable buffer that owns its block: freed by the destructor, handed on by a move, never copied.  A template over the
// allocator so that the ownership rules run on the host under sanitizers (tests/cpp/test_dev_buf.cpp); handle.h makes
// DevBuf the instance over hipMalloc / hipFree.
//   Alloc::alloc(void** p, size_t bytes) -> 0 or the allocator's error;  Alloc::free(void* p);
//   Alloc::forget(int err): the first of reserve's two attempts failed, drop what it left behind;
//   Alloc::failed(size_t bytes, int err) -> the error code reserve returns, after recording its text.
#pragma once
#include <cstddef>

namespace vlq_detail {

template <class Alloc>
struct BasicDevBuf {
    void* p = nullptr;
    size_t cap = 0;
    BasicDevBuf() = default;
    BasicDevBuf(const BasicDevBuf&) = delete;
    BasicDevBuf& operator=(const BasicDevBuf&) = delete;
    BasicDevBuf(BasicDevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    BasicDevBuf& operator=(BasicDevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~BasicDevBuf() { release(); }
    // at least `bytes`; growth discards the old contents and asks for 1/8 + 256 bytes of slack, then for exactly `bytes`
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        release();
        size_t want = bytes + bytes / 8 + 256;
        int e = Alloc::alloc(&p, want);
        if (e) {
            Alloc::forget(e);
            e = Alloc::alloc(&p, bytes);
            want = bytes;
        }
        if (e) { p = nullptr; return Alloc::failed(bytes, e); }
        cap = want;
        return 0;
    }
    void release() { if (p) Alloc::free(p); p = nullptr; cap = 0; }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

}  // namespace vlq_detail
