// TEST INFRASTRUCTURE ONLY -- the reference's Simplecooked (overcooked2_env) sim.cpp, compiled unchanged against
// the Madrona stand-in, behind an orc_simplecooked-shaped C ABI (oracle/ref.py: RefSimplecooked).  REF_SIM is
// the path of the reference's src/overcooked2_env/sim.cpp; oracle/Makefile.ref passes it in.  No game logic here.
#include REF_SIM

#include "ref_driver_kitchen.hpp"

namespace {

struct Types {
    using Engine = Simplecooked::Engine;
    using Sim = Simplecooked::Sim;
    using Config = Simplecooked::Config;
    using WorldInit = Simplecooked::WorldInit;
    using EpisodeManager = Simplecooked::EpisodeManager;
    using WorldState = Simplecooked::WorldState;
    using WorldReset = Simplecooked::WorldReset;
    using PlayerState = Simplecooked::PlayerState;
    using LocationData = Simplecooked::LocationData;
    using LocationXObservation = Simplecooked::LocationXObservation;
    using Action = Simplecooked::Action;
    using ActionT = Simplecooked::ActionT;
    using Reward = Simplecooked::Reward;
    using TerrainT = Simplecooked::TerrainT;
};
using Ref = refdrv::Kitchen<Types>;
constexpr uint32_t kRowExtra = 10;

static_assert(sizeof(Simplecooked::LocationXObservation) == 5 * MAX_NUM_PLAYERS + kRowExtra, "an observation row is 5P + 10 bytes");
static_assert(MAX_NUM_PLAYERS == 2, "the dish-pickup shaping reads agents[0] and agents[1]");

}  // namespace

extern "C" {

// NULL for what the C++ cannot hold: more than MAX_SIZE cells (Config.terrain), and any player count but two --
// with one player the dish-pickup shaping reads the PlayerState of agents[1], an entity that was never made
// (is_dish_pickup_useful loops p < 2), which is undefined under Madrona and aborts in the stand-in.
void *ref_simplecooked_create(const int64_t *cfg_i64, const uint8_t *terrain, const uint8_t *start_x, const uint8_t *start_y,
                              const uint8_t *recipe_values, const uint8_t *recipe_times, uint32_t n, uint32_t fill,
                              int construct, int graph_order, int reverse_entities)
{
    const int64_t h = cfg_i64[refdrv::kHeight], w = cfg_i64[refdrv::kWidth], p = cfg_i64[refdrv::kPlayers];
    if (h <= 0 || w <= 0 || h * w > MAX_SIZE || p != 2) return nullptr;
    return Ref::create(cfg_i64, terrain, start_x, start_y, recipe_values, recipe_times, n, fill, construct, graph_order,
                       reverse_entities, kRowExtra);
}

void ref_simplecooked_destroy(void *h) { delete static_cast<Ref *>(h); }

void ref_simplecooked_step(void *h, const int32_t *actions) { static_cast<Ref *>(h)->step(actions); }

// as ref_overcooked_read, plus dishes_out (N,) i32 = WorldState.num_dishes_out
void ref_simplecooked_read(void *h, uint8_t *obs, int32_t *reward, int32_t *done, uint8_t *players, uint8_t *objects,
                           int32_t *timestep, int32_t *dishes_out)
{
    auto *s = static_cast<Ref *>(h);
    s->read(obs, reward, done, players, objects, timestep);
    for (uint32_t w = 0; w < s->n; w++) dishes_out[w] = s->ctx(w).singleton<Simplecooked::WorldState>().num_dishes_out;
}

uint32_t ref_simplecooked_episodes(void *h) { return static_cast<Ref *>(h)->mgr.curEpisode.load_relaxed(); }

uint32_t ref_simplecooked_guards(void *h, int32_t *out, uint32_t cap) { return static_cast<Ref *>(h)->guard_hits(out, cap); }

uint32_t ref_simplecooked_node_order(void *h, int graph_order, uint32_t *out, uint32_t cap)
{
    return static_cast<Ref *>(h)->node_order(graph_order, out, cap);
}

}  // extern "C"
