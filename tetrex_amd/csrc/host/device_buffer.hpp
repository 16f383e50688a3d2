// One RAII device allocation of the host side (txq_malloc / txq_free, include/txq.h).  Product code; requires a gfx950 GPU.
#pragma once
#include "../../../include/txq.h"

#include <algorithm>
#include <cstddef>

namespace tetrex {

// Throws std::runtime_error carrying txq_last_error() when a txq call fails.
void txq_check(int rc, const char* what);

// A device buffer that only grows: reserve() keeps what it has unless more is asked for, so a buffer sized for the largest
// batch of a call is neither freed nor allocated between the call's launches.  (txq_free waits for the kernels that read it.)
struct DeviceBuffer {
    void* p = nullptr;
    size_t cap = 0;
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t bytes) { reserve(bytes); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { if (p) txq_free(p); }
    void* reserve(size_t bytes) {
        if (bytes > cap || !p) {
            if (p) txq_free(p);
            p = nullptr;
            cap = 0;
            txq_check(txq_malloc(&p, std::max<size_t>(bytes, 256)), "txq_malloc");
            cap = std::max<size_t>(bytes, 256);
        }
        return p;
    }
};

}  // namespace tetrex
