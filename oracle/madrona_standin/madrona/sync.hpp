// TEST INFRASTRUCTURE ONLY -- Madrona stand-in: the episode counter's atomic (AtomicU32) and the generic
// Atomic<T> the kitchen worlds keep in their components (rewards, flags, per-cell counters).
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

template <typename T>
class Atomic {
public:
    Atomic() = default;  // as for raw column memory: the value is whatever the storage holds
    Atomic(T v) : v_(v) {}
    T load_relaxed() const { return __atomic_load_n(&v_, __ATOMIC_RELAXED); }
    T load_acquire() const { return __atomic_load_n(&v_, __ATOMIC_ACQUIRE); }
    void store_relaxed(T v) { __atomic_store_n(&v_, v, __ATOMIC_RELAXED); }
    void store_release(T v) { __atomic_store_n(&v_, v, __ATOMIC_RELEASE); }
    T fetch_add_relaxed(T d) { return __atomic_fetch_add(&v_, d, __ATOMIC_RELAXED); }

private:
    T v_;
};

}  // namespace madrona
