// TEST INFRASTRUCTURE ONLY -- shared part of oracle/ref_driver_{hanabi,cartpole,balance,overcooked,simplecooked}.cpp: N worlds of a
// reference sim.cpp built against the Madrona stand-in (oracle/madrona_standin), stepped through the task
// graph its setupTasks builds.  No game logic here.
//
// Episode order: the worlds are constructed, and run within every node of the graph, in ascending world
// order, so the shared counter (EpisodeManager::curEpisode) hands out episode indices in ascending world
// order.  That order is this project's choice (csrc/episode_scan.hpp, oracle/*.c); under Madrona the
// order is whatever order the threads reach fetch_add_relaxed in, which the reference leaves open.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include <madrona/taskgraph_builder.hpp>

namespace refdrv {

template <typename EngineT, typename SimT>
struct Worlds {
    madrona::ECSRegistry registry;
    madrona::TaskGraphBuilder graph;
    std::vector<madrona::standin::WorldStore *> stores;
    std::vector<EngineT *> engines;
    std::vector<SimT *> sims;

    template <typename ConfigT, typename InitT>
    void create(uint32_t n, uint8_t fill, bool construct, const ConfigT &cfg, const InitT &init)
    {
        SimT::registerTypes(registry, cfg);
        SimT::setupTasks(graph, cfg);
        for (uint32_t w = 0; w < n; w++) {
            auto *store = new madrona::standin::WorldStore(fill, construct);
            registry.make_singletons(*store);
            auto *engine = new EngineT(*store);
            const size_t bytes = (sizeof(SimT) + 63) / 64 * 64;
            void *mem = std::aligned_alloc(64, bytes);
            if (!mem) throw std::bad_alloc();
            std::memset(mem, fill, bytes);
            store->data = mem;  // ctx.data() is live while the constructor runs (it resets the world)
            sims.push_back(new (mem) SimT(*engine, cfg, init));
            stores.push_back(store);
            engines.push_back(engine);
        }
    }

    // graph_order / reverse_entities: see madrona/taskgraph_builder.hpp; the defaults are insertion order and
    // ascending entities
    int graph_order = 0;
    bool reverse_entities = false;

    void step() { graph.run(engines, graph_order, reverse_entities); }

    ~Worlds()
    {
        for (size_t w = 0; w < sims.size(); w++) {
            sims[w]->~SimT();
            std::free(sims[w]);
            delete engines[w];
            delete stores[w];
        }
    }
};

template <typename... Ts>
inline int32_t type_code(uint32_t tid)
{
    const uint32_t ids[] = {madrona::standin::type_id<Ts>()...};
    for (uint32_t i = 0; i < sizeof...(Ts); i++)
        if (ids[i] == tid) return (int32_t)i;
    return -1;
}

// Dirty guard bytes of all worlds as rows of (world, entity, type code, offset, value); the guards are
// restored.  Returns the number of hits, which may exceed cap (only cap rows are written).
template <typename EngineT, typename SimT, typename... Ts>
inline uint32_t guards(Worlds<EngineT, SimT> &W, int32_t *out, uint32_t cap)
{
    uint32_t hits = 0;
    for (uint32_t w = 0; w < W.stores.size(); w++)
        W.stores[w]->guard_scan([&](const madrona::standin::GuardHit &g) {
            if (hits < cap) {
                int32_t *r = out + 5 * hits;
                r[0] = (int32_t)w;
                r[1] = (int32_t)g.entity;
                r[2] = type_code<Ts...>(g.type);
                r[3] = g.offset;
                r[4] = g.value;
            }
            hits++;
        });
    return hits;
}

}  // namespace refdrv
