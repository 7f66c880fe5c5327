// TEST INFRASTRUCTURE ONLY -- Madrona stand-in: one world's component storage, the registry, WorldBase
// and CustomContext.  Our own code; it holds no game logic.
//
// Storage model (what the drivers rely on):
//   - each world is one WorldStore; entity 0 is the world's singleton entity, every registered singleton
//     is a component of it; makeEntity<A>() hands out 1, 2, ... in creation order;
//   - every component instance is its own allocation, [kGuard bytes | payload | kGuard bytes], filled with
//     the store's fill byte (0x00 or 0xA5) when it is created.  A write past either end of a component
//     lands in a guard (guard_scan reports it); a read of bytes the simulation never wrote shows up as a
//     difference between two runs with different fill bytes;
//   - construct = false leaves a new component as raw fill bytes (no constructor runs, as for columns of
//     raw memory); construct = true default-initialises it (default member initialisers run).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "components.hpp"

namespace madrona {

namespace standin {

inline uint32_t next_type_id()
{
    static uint32_t counter = 0;
    return counter++;
}

template <typename T>
inline uint32_t type_id()
{
    static const uint32_t id = next_type_id();
    return id;
}

constexpr size_t kGuard = 64;

struct Slot {
    uint32_t type;
    uint32_t size;
    unsigned char *mem;  // kGuard + size + kGuard bytes, 64-byte aligned; payload at mem + kGuard
    void *payload() const { return mem + kGuard; }
};

struct GuardHit {
    uint32_t entity;
    uint32_t type;
    int32_t offset;  // relative to the payload end when >= 0 (0 = first byte past it); -1.. = bytes before the payload
    uint8_t value;
};

class WorldStore {
public:
    WorldStore(uint8_t fill, bool construct) : fill_(fill), construct_(construct) { entities_.emplace_back(); }
    ~WorldStore()
    {
        for (auto &e : entities_)
            for (auto &s : e) std::free(s.mem);
        for (void *p : raw_) std::free(p);
    }
    WorldStore(const WorldStore &) = delete;
    WorldStore &operator=(const WorldStore &) = delete;

    uint32_t num_entities() const { return (uint32_t)entities_.size(); }
    uint32_t new_entity()
    {
        entities_.emplace_back();
        return (uint32_t)entities_.size() - 1;
    }

    template <typename T>
    void add(uint32_t entity)
    {
        const size_t bytes = (2 * kGuard + sizeof(T) + 63) / 64 * 64;
        unsigned char *mem = (unsigned char *)std::aligned_alloc(64, bytes);
        if (!mem) throw std::bad_alloc();
        std::memset(mem, fill_, bytes);
        if (construct_) new (mem + kGuard) T;
        entities_[entity].push_back(Slot{type_id<T>(), (uint32_t)sizeof(T), mem});
        if (by_type_.size() <= type_id<T>()) by_type_.resize(type_id<T>() + 1);
        by_type_[type_id<T>()].push_back(entity);
    }

    // The entities that carry a T, in ascending creation order (what a node iterates instead of all entities).
    template <typename T>
    const std::vector<uint32_t> &entities_with()
    {
        if (by_type_.size() <= type_id<T>()) by_type_.resize(type_id<T>() + 1);
        return by_type_[type_id<T>()];
    }

    template <typename T>
    T *find(uint32_t entity)
    {
        const uint32_t t = type_id<T>();
        for (const Slot &s : entities_[entity])
            if (s.type == t) return static_cast<T *>(s.payload());
        return nullptr;
    }

    template <typename T>
    T &get(uint32_t entity)
    {
        T *p = find<T>(entity);
        if (!p) std::abort();  // the reference asked for a component its entity does not have
        return *p;
    }

    void *raw_alloc(size_t bytes)
    {
        void *p = std::aligned_alloc(64, (bytes + 63) / 64 * 64);
        if (!p) throw std::bad_alloc();
        std::memset(p, fill_, (bytes + 63) / 64 * 64);
        raw_.push_back(p);
        return p;
    }

    // Every guard byte that no longer holds the fill byte, reported and then restored.
    template <typename Fn>
    void guard_scan(Fn &&report)
    {
        for (uint32_t e = 0; e < entities_.size(); e++)
            for (const Slot &s : entities_[e]) {
                const size_t bytes = (2 * kGuard + s.size + 63) / 64 * 64;
                if (clean(s.mem, kGuard) && clean(s.mem + kGuard + s.size, bytes - kGuard - s.size)) continue;
                for (size_t b = 0; b < bytes; b++) {
                    if (b >= kGuard && b < kGuard + s.size) continue;
                    if (s.mem[b] == fill_) continue;
                    const int32_t off = b < kGuard ? (int32_t)b - (int32_t)kGuard : (int32_t)(b - kGuard - s.size);
                    report(GuardHit{e, s.type, off, s.mem[b]});
                    s.mem[b] = fill_;
                }
            }
    }

    void *data = nullptr;  // the world's Sim object (CustomContext::data)

private:
    // whether all `bytes` bytes at p still hold the fill byte
    bool clean(const unsigned char *p, size_t bytes) const
    {
        return bytes == 0 || (p[0] == fill_ && std::memcmp(p, p + 1, bytes - 1) == 0);
    }

    uint8_t fill_;
    bool construct_;
    std::vector<std::vector<Slot>> entities_;
    std::vector<std::vector<uint32_t>> by_type_;
    std::vector<void *> raw_;
};

}  // namespace standin

// Registration happens once (Sim::registerTypes is static); the registry remembers which singletons every
// world's entity 0 carries.  Component and archetype registration and the exports are bookkeeping the
// drivers do not need.
class ECSRegistry {
public:
    template <typename T>
    void registerSingleton()
    {
        singletons_.push_back([](standin::WorldStore &s) { s.add<T>(0); });
    }
    template <typename T>
    void registerComponent() {}
    template <typename A>
    void registerArchetype() {}
    template <typename T>
    void exportSingleton(uint32_t) {}
    template <typename A, typename T>
    void exportColumn(uint32_t) {}

    void make_singletons(standin::WorldStore &s) const
    {
        for (auto fn : singletons_) fn(s);
    }

private:
    std::vector<void (*)(standin::WorldStore &)> singletons_;
};

template <typename ContextT, typename DataT>
class CustomContext {
public:
    explicit CustomContext(standin::WorldStore &store) : store_(&store) {}

    DataT &data() { return *static_cast<DataT *>(store_->data); }

    template <typename T>
    T &get(Entity e) { return store_->get<T>(e.id); }

    template <typename T>
    T &singleton() { return store_->get<T>(0); }

    template <typename A>
    Entity makeEntity() { return make(static_cast<A *>(nullptr)); }

    standin::WorldStore &store() { return *store_; }

private:
    template <typename... Cs>
    Entity make(Archetype<Cs...> *)
    {
        const uint32_t e = store_->new_entity();
        (store_->add<Cs>(e), ...);
        return Entity{e};
    }

    standin::WorldStore *store_;
};

struct WorldBase {
    using base = WorldBase;

    template <typename ContextT>
    explicit WorldBase(ContextT &ctx) : store_(&ctx.store()) {}

    static void registerTypes(ECSRegistry &) {}

    void *rawAlloc(size_t bytes) { return store_->raw_alloc(bytes); }

private:
    standin::WorldStore *store_;
};

}  // namespace madrona
