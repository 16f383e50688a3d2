// Who owns what libtxq allocates: a grow-only buffer, a handle for events and streams, and the one loop that frees a list of
// arena chunks.  Plain C++ with no HIP header: the memory primitives come in through a policy `Mem` (alloc(void**, size_t) -> 0
// or an error code, free(void*)) and a handle's through `Kind` (destroy(H)).  libtxq instantiates them with hipMalloc / hipFree,
// hipHostMalloc / hipHostFree, hipEventDestroy and hipStreamDestroy (txq_internal.hpp); tests/native/buffers_sim.cpp with a
// counting malloc.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace txq {

// How much a buffer that has to grow asks for: exactly the need, or half as much again and at least `floor` bytes.
struct Grow { size_t need, want; };
inline Grow exactly(size_t need) { return {need, need}; }
inline Grow half_more(size_t need, size_t floor) { return {need, need + need / 2 > floor ? need + need / 2 : floor}; }

// A move-only, grow-only allocation of `Mem`.  T types get() only: Buffer<void, Mem> takes any of them over (a retire list).
template <class T, class Mem>
class Buffer {
public:
    Buffer() = default;
    template <class U>
    Buffer(Buffer<U, Mem>&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            bytes_ = std::exchange(o.bytes_, 0);
        }
        return *this;
    }
    ~Buffer() { reset(); }
    T* get() const { return static_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) Mem::free(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // At least g.need bytes.  An allocation that is large enough stays.  Otherwise g.want bytes are allocated, and the
    // outgrown allocation (if there is one) goes to `outgrown` first, as a Buffer: the call site says there what has to
    // happen before it may be freed (free_after, retire_to, free_now below).  Returns 0 or Mem's error, after which the
    // buffer is empty.
    template <class Outgrown>
    int reserve(Grow g, Outgrown&& outgrown) {
        if (p_ && bytes_ >= g.need) return 0;
        if (p_) outgrown(Buffer<void, Mem>(std::move(*this)));
        if (int e = Mem::alloc(&p_, g.want)) {
            p_ = nullptr;
            return e;
        }
        bytes_ = g.want;
        return 0;
    }

private:
    template <class, class> friend class Buffer;
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

// What happens to an outgrown allocation (Buffer::reserve):
// freed once wait() has returned — a device-wide wait, or the event behind the last kernel that read it
template <class Wait>
auto free_after(Wait wait) {
    return [wait](auto&& old) { wait(); old.reset(); };
}
// kept on `list` and freed with it: something may still read it, and nobody wants to wait
template <class Mem>
auto retire_to(std::vector<Buffer<void, Mem>>& list) {
    return [&list](Buffer<void, Mem>&& old) { list.push_back(std::move(old)); };
}
// freed at once: the caller has already waited for whatever read it
inline auto free_now() {
    return [](auto&& old) { old.reset(); };
}

// A move-only event or stream (H: a pointer type; null = none).
template <class H, class Kind>
class Handle {
public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, H{})) {}
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) reset(std::exchange(o.h_, H{}));
        return *this;
    }
    ~Handle() { reset(); }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != H{}; }
    void reset(H h = H{}) {  // takes `h` over
        if (h_ != H{}) Kind::destroy(h_);
        h_ = h;
    }

private:
    H h_{};
};

// The chunks of a slot or block arena (txq_exec_plan.hpp keeps those lists raw: its planner is tested with made-up pointers).
template <class Mem, class Chunk>
void free_chunks(std::vector<Chunk>& chunks) {
    for (const Chunk& c : chunks) Mem::free(c.p);
    chunks.clear();
}

}  // namespace txq
