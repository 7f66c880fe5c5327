// TEST INFRASTRUCTURE ONLY -- Madrona stand-in: the episode counter's atomic.
#pragma once

#include <atomic>
#include <cstdint>

namespace madrona {

class AtomicU32 {
public:
    AtomicU32(uint32_t v = 0) : v_(v) {}
    uint32_t fetch_add_relaxed(uint32_t d) { return v_.fetch_add(d, std::memory_order_relaxed); }
    uint32_t load_relaxed() const { return v_.load(std::memory_order_relaxed); }
    void store_relaxed(uint32_t v) { v_.store(v, std::memory_order_relaxed); }

private:
    std::atomic<uint32_t> v_;
};

}  // namespace madrona
