// The owning buffer of the library's handles: one block of device or pinned memory, released by its destructor.  The kind of
// memory is a policy type with  static int alloc(void **, size_t)  (0, or the library's error code after fail(...)) and
// static void release(void *);  alp_internal.h has the two HIP policies, the self-checking driver a counting one on malloc.
// Included by alp_internal.h; nothing here may include a HIP header.
#pragma once

#include <cstddef>

namespace alp {

// T: the element type its users read it as (Buffer converts to T * where a pointer is expected, so a kernel launch or an
// `if (!m->valid)` reads as it would with a plain pointer; `(const float *)p->w` casts a Buffer<.., void> like a void *).
template <typename Policy, typename T = void>
class Buffer {
public:
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept : ptr_(o.ptr_), cap_(o.cap_) { o.ptr_ = nullptr, o.cap_ = 0; }
    Buffer &operator=(Buffer &&o) noexcept {
        if (this != &o) {
            reset();
            ptr_ = o.ptr_, cap_ = o.cap_;
            o.ptr_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~Buffer() { reset(); }

    void reset() {
        if (ptr_) Policy::release(ptr_);
        ptr_ = nullptr, cap_ = 0;
    }
    // At least `bytes` bytes; a block that is large enough stays.  Otherwise the old block is released BEFORE the new one is
    // asked for (the two never coexist: alp_render_rasterize's work area is 5.3 GB), the contents are not kept, and a failure
    // leaves the buffer empty.
    int reserve(size_t bytes) {
        if (ptr_ && cap_ >= bytes) return 0;
        reset();
        void *q = nullptr;
        if (int rc = Policy::alloc(&q, bytes)) return rc;
        ptr_ = (T *)q, cap_ = bytes;
        return 0;
    }
    size_t capacity() const { return cap_; }
    T *get() const { return ptr_; }
    operator T *() const { return ptr_; }
    template <typename U>
    explicit operator U *() const { return (U *)ptr_; }

private:
    T *ptr_ = nullptr;
    size_t cap_ = 0;
};

template <typename... B>
void reset_all(B &...b) {
    (b.reset(), ...);
}

// reserve_all({bytes_a, bytes_b, ...}, a, b, ...): the buffers of a group in order; when one of them fails every buffer of the
// group is reset and the error returned -- a group is published whole or not at all
template <typename... B>
int reserve_all(const size_t (&bytes)[sizeof...(B)], B &...b) {
    int rc = 0, i = 0;
    ((rc = rc ? rc : b.reserve(bytes[i++])), ...);
    if (rc) reset_all(b...);
    return rc;
}

}  // namespace alp
