// TEST INFRASTRUCTURE ONLY -- the reference's balance-beam sim.cpp, compiled unchanged against the Madrona
// stand-in, behind an orc_balance-shaped C ABI (oracle/ref.py: RefBalance).  REF_SIM is the path of the
// reference's src/balance_beam_env/sim.cpp; oracle/Makefile.ref passes it in.  No game logic here.
// Episode order: see ref_driver_common.hpp.
#include REF_SIM

#include "ref_driver_common.hpp"

namespace {

constexpr uint32_t kAgents = 2, kObs = 2 * TIME + 1;

struct RefBalance {
    uint32_t n;
    Balance::EpisodeManager mgr;
    refdrv::Worlds<Balance::Engine, Balance::Sim> worlds;
    Balance::Engine &ctx(uint32_t w) { return *worlds.engines[w]; }
    madrona::Entity agent(uint32_t w, uint32_t a) { return worlds.sims[w]->agents[a]; }
};

static_assert(sizeof(Balance::Observation) == kObs * sizeof(int32_t), "an observation row is 7 int32");

}  // namespace

extern "C" {

void *ref_balance_create(uint32_t n, uint32_t first_episode, uint32_t fill, int construct)
{
    auto *s = new RefBalance();
    s->n = n;
    s->mgr.curEpisode.store_relaxed(first_episode);
    Balance::Config config{};
    Balance::WorldInit init{&s->mgr};
    s->worlds.create(n, (uint8_t)fill, construct != 0, config, init);
    return s;
}

void ref_balance_destroy(void *h) { delete static_cast<RefBalance *>(h); }

// actions: (2, N) int32
void ref_balance_step(void *h, const int32_t *actions)
{
    auto *s = static_cast<RefBalance *>(h);
    for (uint32_t w = 0; w < s->n; w++)
        for (uint32_t a = 0; a < kAgents; a++)
            s->ctx(w).get<Balance::Action>(s->agent(w, a)).choice = actions[(size_t)a * s->n + w];
    s->worlds.step();
}

// obs (2, N, 7) i32, loc (2, N) i32, time (N,) i32, reward (2, N) f32, done (N,) i32 (the WorldReset singleton)
void ref_balance_read(void *h, int32_t *obs, int32_t *loc, int32_t *time, float *reward, int32_t *done)
{
    auto *s = static_cast<RefBalance *>(h);
    for (uint32_t w = 0; w < s->n; w++) {
        Balance::Engine &c = s->ctx(w);
        for (uint32_t a = 0; a < kAgents; a++) {
            const madrona::Entity e = s->agent(w, a);
            const size_t row = (size_t)a * s->n + w;
            std::memcpy(obs + row * kObs, &c.get<Balance::Observation>(e), sizeof(Balance::Observation));
            loc[row] = c.get<Balance::Location>(e).x;
            reward[row] = c.get<Balance::Reward>(e).rew;
        }
        time[w] = c.singleton<Balance::WorldTime>().time;
        done[w] = c.singleton<Balance::WorldReset>().resetNow;
    }
}

uint32_t ref_balance_episodes(void *h) { return static_cast<RefBalance *>(h)->mgr.curEpisode.load_relaxed(); }

// type codes: 0 Observation, -1 any other component
uint32_t ref_balance_guards(void *h, int32_t *out, uint32_t cap)
{
    auto *s = static_cast<RefBalance *>(h);
    return refdrv::guards<Balance::Engine, Balance::Sim, Balance::Observation>(s->worlds, out, cap);
}

}  // extern "C"
