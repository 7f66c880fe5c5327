// TEST INFRASTRUCTURE ONLY -- what oracle/ref_driver_overcooked.cpp and ref_driver_simplecooked.cpp share: the two
// kitchen sim.cpp files declare the same component names in two namespaces, so the drivers hand their
// namespace's types in through a traits struct.  No game logic here.
//
// The kitchens use no episode counter; nothing in their graphs depends on the order of the worlds.
#pragma once

#include "ref_driver_common.hpp"

namespace refdrv {

// cfg_i64: height, width, num_players, placement_in_pot_rew, dish_pickup_rew, soup_pickup_rew, horizon
enum { kHeight, kWidth, kPlayers, kPotRew, kDishRew, kSoupRew, kHorizon, kNumScalars };

template <typename K>
struct Kitchen {
    uint32_t n, players, cells, row;  // row = bytes of an observation row the simulation writes
    typename K::EpisodeManager mgr;
    Worlds<typename K::Engine, typename K::Sim> worlds;

    typename K::Engine &ctx(uint32_t w) { return *worlds.engines[w]; }

    static Kitchen *create(const int64_t *cfg_i64, const uint8_t *terrain, const uint8_t *start_x, const uint8_t *start_y,
                           const uint8_t *recipe_values, const uint8_t *recipe_times, uint32_t n, uint32_t fill,
                           int construct, int graph_order, int reverse_entities, uint32_t row_extra)
    {
        const int64_t cells = cfg_i64[kHeight] * cfg_i64[kWidth], players = cfg_i64[kPlayers];
        auto *s = new Kitchen();
        s->n = n;
        s->players = (uint32_t)players;
        s->cells = (uint32_t)cells;
        s->row = 5 * (uint32_t)players + row_extra;
        typename K::Config config{};
        config.height = cfg_i64[kHeight];
        config.width = cfg_i64[kWidth];
        config.num_players = players;
        config.placement_in_pot_rew = cfg_i64[kPotRew];
        config.dish_pickup_rew = cfg_i64[kDishRew];
        config.soup_pickup_rew = cfg_i64[kSoupRew];
        config.horizon = cfg_i64[kHorizon];
        for (int64_t c = 0; c < cells; c++) config.terrain[c] = (typename K::TerrainT)terrain[c];
        for (int64_t p = 0; p < players; p++) {
            config.start_player_x[p] = start_x[p];
            config.start_player_y[p] = start_y[p];
        }
        for (int r = 0; r < NUM_RECIPES; r++) {
            config.recipe_values[r] = recipe_values[r];
            config.recipe_times[r] = recipe_times[r];
        }
        typename K::WorldInit init{&s->mgr};
        s->worlds.graph_order = graph_order;
        s->worlds.reverse_entities = reverse_entities != 0;
        s->worlds.create(n, (uint8_t)fill, construct != 0, config, init);
        return s;
    }

    // actions: (P, N) int32
    void step(const int32_t *actions)
    {
        for (uint32_t w = 0; w < n; w++)
            for (uint32_t p = 0; p < players; p++)
                ctx(w).template get<typename K::Action>(worlds.sims[w]->agents[p]).choice =
                    (typename K::ActionT)actions[(size_t)p * n + w];
        worlds.step();
    }

    // obs (N, P, C, row) u8: the first `row` bytes of each LocationXObservation; reward (P, N) i32; done (N,) i32;
    // players (N, P, 6) u8 = position, orientation, held{name, onions, tomatoes, tick}; objects (N, C, 4) u8 =
    // name, onions, tomatoes, tick; timestep (N,) i32 -- the layout of the oracle's dump()
    void read(uint8_t *obs, int32_t *reward, int32_t *done, uint8_t *pl, uint8_t *ob, int32_t *timestep)
    {
        for (uint32_t w = 0; w < n; w++) {
            typename K::Engine &c = ctx(w);
            typename K::Sim &sim = *worlds.sims[w];
            for (uint32_t r = 0; r < players * cells; r++)
                std::memcpy(obs + ((size_t)w * players * cells + r) * row,
                            c.template get<typename K::LocationXObservation>(sim.locationXplayers[r]).x, row);
            for (uint32_t p = 0; p < players; p++) {
                reward[(size_t)p * n + w] = c.template get<typename K::Reward>(sim.agents[p]).rew;
                const typename K::PlayerState &ps = c.template get<typename K::PlayerState>(sim.agents[p]);
                uint8_t *o = pl + ((size_t)w * players + p) * 6;
                o[0] = ps.position;
                o[1] = ps.orientation;
                put(o + 2, ps.held_object);
            }
            for (uint32_t k = 0; k < cells; k++)
                put(ob + ((size_t)w * cells + k) * 4, c.template get<typename K::LocationData>(sim.locations[k]).object);
            timestep[w] = c.template singleton<typename K::WorldState>().timestep;
            done[w] = c.template singleton<typename K::WorldReset>().resetNow;
        }
    }

    // type codes: 0 LocationXObservation, 1 LocationData, 2 PlayerState, 3 WorldState, -1 any other component
    uint32_t guard_hits(int32_t *out, uint32_t cap)
    {
        return guards<typename K::Engine, typename K::Sim, typename K::LocationXObservation, typename K::LocationData,
                      typename K::PlayerState, typename K::WorldState>(worlds, out, cap);
    }

    // the node ids (in the order setupTasks added them) as run() executes them for graph_order; returns their number
    uint32_t node_order(int order, uint32_t *out, uint32_t cap) const
    {
        const std::vector<uint32_t> ids = worlds.graph.order(order);
        for (uint32_t i = 0; i < ids.size() && i < cap; i++) out[i] = ids[i];
        return (uint32_t)ids.size();
    }

private:
    template <typename ObjectT>
    static void put(uint8_t *o, const ObjectT &obj)
    {
        o[0] = (uint8_t)obj.name;
        o[1] = obj.num_onions;
        o[2] = obj.num_tomatoes;
        o[3] = (uint8_t)obj.cooking_tick;
    }
};

}  // namespace refdrv
