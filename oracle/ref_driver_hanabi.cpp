// TEST INFRASTRUCTURE ONLY -- the reference's Hanabi sim.cpp, compiled unchanged against the Madrona
// stand-in, behind an orc_hanabi-shaped C ABI (oracle/ref.py: RefHanabi).  REF_SIM is the path of the
// reference's src/hanabi_env/sim.cpp; oracle/Makefile.ref passes it in.  No game logic here: every step
// runs the reference's actionSystem, observationSystem and checkDone through its own setupTasks.
// Episode order: see ref_driver_common.hpp.
#include REF_SIM

#include "ref_driver_common.hpp"

namespace {

struct ref_hanabi_config {
    uint32_t colors, ranks, players, max_information_tokens, max_life_tokens;
};

constexpr uint32_t kPlayers = 2;

struct RefHanabi {
    uint32_t n;
    Hanabi::EpisodeManager mgr;
    refdrv::Worlds<Hanabi::Engine, Hanabi::Sim> worlds;
    Hanabi::Engine &ctx(uint32_t w) { return *worlds.engines[w]; }
    madrona::Entity agent(uint32_t w, uint32_t a) { return worlds.sims[w]->agents[a]; }
};

}  // namespace

extern "C" {

// fill: byte every component starts as (0x00 or 0xA5); construct: default-initialise components
void *ref_hanabi_create(const ref_hanabi_config *cfg, uint32_t n, uint32_t first_episode, uint32_t fill, int construct)
{
    if (!cfg || cfg->players != kPlayers) return nullptr;
    auto *s = new RefHanabi();
    s->n = n;
    s->mgr.curEpisode.store_relaxed(first_episode);
    Hanabi::Config config{cfg->players};
    Hanabi::WorldInit init{&s->mgr, cfg->colors, cfg->ranks, cfg->players, cfg->max_information_tokens,
                           cfg->max_life_tokens};
    s->worlds.create(n, (uint8_t)fill, construct != 0, config, init);
    return s;
}

void ref_hanabi_destroy(void *h) { delete static_cast<RefHanabi *>(h); }

// actions: (2, N) int32
void ref_hanabi_step(void *h, const int32_t *actions)
{
    auto *s = static_cast<RefHanabi *>(h);
    for (uint32_t w = 0; w < s->n; w++)
        for (uint32_t a = 0; a < kPlayers; a++)
            s->ctx(w).get<Hanabi::Action>(s->agent(w, a)).choice = actions[(size_t)a * s->n + w];
    s->worlds.step();
}

// obs (2, N, 658) u8, state (2, N, 783) u8, mask (2, N, 20) i32, active (2, N) i32, reward (2, N) f32,
// done (N) i32 (the WorldReset singleton)
void ref_hanabi_read(void *h, uint8_t *obs, uint8_t *state, int32_t *mask, int32_t *active, float *reward,
                     int32_t *done)
{
    auto *s = static_cast<RefHanabi *>(h);
    for (uint32_t w = 0; w < s->n; w++) {
        Hanabi::Engine &c = s->ctx(w);
        for (uint32_t a = 0; a < kPlayers; a++) {
            const madrona::Entity e = s->agent(w, a);
            const size_t row = (size_t)a * s->n + w;
            std::memcpy(obs + row * OBS_SIZE, c.get<Hanabi::Observation>(e).bitvec, OBS_SIZE);
            std::memcpy(state + row * STATE_SIZE, c.get<Hanabi::State>(e).bitvec, STATE_SIZE);
            std::memcpy(mask + row * NUM_MOVES, c.get<Hanabi::ActionMask>(e).isValid, NUM_MOVES * sizeof(int32_t));
            active[row] = c.get<Hanabi::ActiveAgent>(e).isActive;
            reward[row] = c.get<Hanabi::Reward>(e).rew;
        }
        done[w] = c.singleton<Hanabi::WorldReset>().resetNow;
    }
}

uint32_t ref_hanabi_episodes(void *h) { return static_cast<RefHanabi *>(h)->mgr.curEpisode.load_relaxed(); }

// type codes: 0 Observation, 1 State, 2 ActionMask, 3 Hand, 4 Deck, 5 LastMove, -1 any other component
uint32_t ref_hanabi_guards(void *h, int32_t *out, uint32_t cap)
{
    auto *s = static_cast<RefHanabi *>(h);
    return refdrv::guards<Hanabi::Engine, Hanabi::Sim, Hanabi::Observation, Hanabi::State, Hanabi::ActionMask,
                          Hanabi::Hand, Hanabi::Deck, Hanabi::LastMove>(s->worlds, out, cap);
}

}  // extern "C"
