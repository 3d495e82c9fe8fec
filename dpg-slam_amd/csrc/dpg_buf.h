// dpg_buf.h -- an array that owns its memory, for the resource owners under the context (private,
// C++ only).  The memory kind is a policy of static functions, so this header needs no HIP header
// and the growth rules run on the CPU under the sanitizers (tools/sanitize_check.cpp):
//   typedef stream_t;
//   int alloc(void** p, size_t bytes);                                      0 = ok
//   void free(void* p);
//   int copy(void* dst, const void* src, size_t bytes, stream_t s);         0 = ok, the copy is done
// dpg_ctx.h defines the two kinds in use: DevBuf<T> (device) and PinBuf<T> (pinned host).
#ifndef DPG_BUF_H
#define DPG_BUF_H

#include <stddef.h>

#include <algorithm>
#include <utility>

// Released when its owner goes (with the owner's device current).  Move-only; move-assignment swaps,
// so std::swap of two buffers exchanges pointer and capacity together.  Every growth form returns 0
// or -1.  Three forms, one per rule the callers had written out by hand:
//   reserve            exact size, contents dropped (a request for 0 elements of an empty buffer
//                      allocates nothing);
//   reserve_amortised  at least 1.5x, contents dropped, the old buffer released FIRST (peak = one
//                      buffer); a request for 0 elements still yields one element, because these
//                      pointers are handed to kernels (the solver's rule);
//   grow               at least 1.5x, the first `keep` elements kept, the old buffer released LAST
//                      (a failure leaves it intact).  It does not clamp a request for 0 elements (the
//                      scan store's rule; the incremental graph's call sites that can ask for 0 clamp
//                      themselves) and skips the copy and its wait when there is nothing to keep (no
//                      caller depends on that wait: the DPG store's append drains its stream first
//                      and never keeps 0 elements).
template <typename T, typename Mem>
struct OwnedBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf&) = delete;
    OwnedBuf& operator=(const OwnedBuf&) = delete;
    OwnedBuf(OwnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~OwnedBuf() { release(); }
    void release() {
        if (p) Mem::free(p);
        p = nullptr;
        cap = 0;
    }
    int reserve(size_t n) {
        if (n <= cap) return 0;
        release();
        return alloc_fresh(std::max<size_t>(n, 1), n);
    }
    int reserve_amortised(size_t n, size_t slack = 0) {
        n = std::max<size_t>(n, 1);
        if (p && n <= cap) return 0;
        const size_t nc = std::max(n, cap + cap / 2) + slack;
        release();
        return alloc_fresh(nc, nc);
    }
    int grow(size_t n, size_t keep, typename Mem::stream_t s) {
        if (n <= cap) return 0;
        const size_t nc = std::max(n, cap + cap / 2);
        void* q = nullptr;
        if (Mem::alloc(&q, nc * sizeof(T))) return -1;
        if (p && keep && Mem::copy(q, p, std::min(keep, cap) * sizeof(T), s)) {
            Mem::free(q);
            return -1;
        }
        if (p) Mem::free(p);
        p = static_cast<T*>(q);
        cap = nc;
        return 0;
    }

private:
    // into an empty buffer; on failure it stays empty
    int alloc_fresh(size_t n_alloc, size_t n_cap) {
        void* q = nullptr;
        if (Mem::alloc(&q, n_alloc * sizeof(T))) return -1;
        p = static_cast<T*>(q);
        cap = n_cap;
        return 0;
    }
};

#endif
