// TEST INFRASTRUCTURE ONLY -- the reference's Overcooked sim.cpp, compiled unchanged against the Madrona
// stand-in, behind an orc_overcooked-shaped C ABI (oracle/ref.py: RefOvercooked).  REF_SIM is the path of the
// reference's src/overcooked_env/sim.cpp; oracle/Makefile.ref passes it in.  No game logic here.
#include REF_SIM

#include "ref_driver_kitchen.hpp"

namespace {

struct Types {
    using Engine = Overcooked::Engine;
    using Sim = Overcooked::Sim;
    using Config = Overcooked::Config;
    using WorldInit = Overcooked::WorldInit;
    using EpisodeManager = Overcooked::EpisodeManager;
    using WorldState = Overcooked::WorldState;
    using WorldReset = Overcooked::WorldReset;
    using PlayerState = Overcooked::PlayerState;
    using LocationData = Overcooked::LocationData;
    using LocationXObservation = Overcooked::LocationXObservation;
    using Action = Overcooked::Action;
    using ActionT = Overcooked::ActionT;
    using Reward = Overcooked::Reward;
    using TerrainT = Overcooked::TerrainT;
};
using Ref = refdrv::Kitchen<Types>;
constexpr uint32_t kRowExtra = 16;

static_assert(sizeof(Overcooked::LocationXObservation) == 5 * MAX_NUM_PLAYERS + kRowExtra, "an observation row is 5P + 16 bytes");
static_assert(sizeof(Overcooked::WorldState::size) == 1, "WorldState.size is one byte: 255 cells at most");

}  // namespace

extern "C" {

// NULL for what the C++ cannot hold: more than 255 cells (WorldState.size is uint8_t; 256 would make it 0 and
// the observation system divide by it) or more than MAX_NUM_PLAYERS players.
void *ref_overcooked_create(const int64_t *cfg_i64, const uint8_t *terrain, const uint8_t *start_x, const uint8_t *start_y,
                            const uint8_t *recipe_values, const uint8_t *recipe_times, uint32_t n, uint32_t fill,
                            int construct, int graph_order, int reverse_entities)
{
    const int64_t h = cfg_i64[refdrv::kHeight], w = cfg_i64[refdrv::kWidth], p = cfg_i64[refdrv::kPlayers];
    if (h <= 0 || w <= 0 || h * w > 255 || p <= 0 || p > MAX_NUM_PLAYERS) return nullptr;
    return Ref::create(cfg_i64, terrain, start_x, start_y, recipe_values, recipe_times, n, fill, construct, graph_order,
                       reverse_entities, kRowExtra);
}

void ref_overcooked_destroy(void *h) { delete static_cast<Ref *>(h); }

void ref_overcooked_step(void *h, const int32_t *actions) { static_cast<Ref *>(h)->step(actions); }

void ref_overcooked_read(void *h, uint8_t *obs, int32_t *reward, int32_t *done, uint8_t *players, uint8_t *objects,
                         int32_t *timestep)
{
    static_cast<Ref *>(h)->read(obs, reward, done, players, objects, timestep);
}

// the kitchens never draw an episode index: the counter stays where it started
uint32_t ref_overcooked_episodes(void *h) { return static_cast<Ref *>(h)->mgr.curEpisode.load_relaxed(); }

uint32_t ref_overcooked_guards(void *h, int32_t *out, uint32_t cap) { return static_cast<Ref *>(h)->guard_hits(out, cap); }

uint32_t ref_overcooked_node_order(void *h, int graph_order, uint32_t *out, uint32_t cap)
{
    return static_cast<Ref *>(h)->node_order(graph_order, out, cap);
}

}  // extern "C"
