// TEST INFRASTRUCTURE ONLY -- the reference's Cartpole sim.cpp, compiled unchanged against the Madrona
// stand-in, behind an orc_cartpole-shaped C ABI (oracle/ref.py: RefCartpole).  REF_SIM is the path of the
// reference's src/cartpole_env/sim.cpp; oracle/Makefile.ref passes it in.  No game logic here.
// Arithmetic: g++ -ffp-contract=off on x86-64 (oracle/Makefile.ref), sinf / cosf from the C library.
// Episode order: see ref_driver_common.hpp.
#include REF_SIM

#include "ref_driver_common.hpp"

namespace {

struct RefCartpole {
    uint32_t n;
    Cartpole::EpisodeManager mgr;
    refdrv::Worlds<Cartpole::Engine, Cartpole::Sim> worlds;
    Cartpole::Engine &ctx(uint32_t w) { return *worlds.engines[w]; }
    madrona::Entity agent(uint32_t w) { return worlds.sims[w]->agents[0]; }
};

}  // namespace

extern "C" {

void *ref_cartpole_create(uint32_t n, uint32_t first_episode, uint32_t fill, int construct)
{
    auto *s = new RefCartpole();
    s->n = n;
    s->mgr.curEpisode.store_relaxed(first_episode);
    Cartpole::Config config{};
    Cartpole::WorldInit init{&s->mgr};
    s->worlds.create(n, (uint8_t)fill, construct != 0, config, init);
    return s;
}

void ref_cartpole_destroy(void *h) { delete static_cast<RefCartpole *>(h); }

// actions: (N,) int32
void ref_cartpole_step(void *h, const int32_t *actions)
{
    auto *s = static_cast<RefCartpole *>(h);
    for (uint32_t w = 0; w < s->n; w++) s->ctx(w).get<Cartpole::Action>(s->agent(w)).choice = actions[w];
    s->worlds.step();
}

// state (N, 4) f32 (x, x_dot, theta, theta_dot), reward (N,) f32, done (N,) i32 (the agent's WorldReset)
void ref_cartpole_read(void *h, float *state, float *reward, int32_t *done)
{
    auto *s = static_cast<RefCartpole *>(h);
    for (uint32_t w = 0; w < s->n; w++) {
        Cartpole::Engine &c = s->ctx(w);
        const madrona::Entity e = s->agent(w);
        const Cartpole::State &st = c.get<Cartpole::State>(e);
        state[4 * (size_t)w + 0] = st.x;
        state[4 * (size_t)w + 1] = st.x_dot;
        state[4 * (size_t)w + 2] = st.theta;
        state[4 * (size_t)w + 3] = st.theta_dot;
        reward[w] = c.get<Cartpole::Reward>(e).rew;
        done[w] = c.get<Cartpole::WorldReset>(e).resetNow;
    }
}

// overwrite every world's State with state (N, 4) f32 (lock-step tests re-synchronise from another implementation)
void ref_cartpole_set_state(void *h, const float *state)
{
    auto *s = static_cast<RefCartpole *>(h);
    for (uint32_t w = 0; w < s->n; w++) {
        Cartpole::State &st = s->ctx(w).get<Cartpole::State>(s->agent(w));
        st.x = state[4 * (size_t)w + 0];
        st.x_dot = state[4 * (size_t)w + 1];
        st.theta = state[4 * (size_t)w + 2];
        st.theta_dot = state[4 * (size_t)w + 3];
    }
}

uint32_t ref_cartpole_episodes(void *h) { return static_cast<RefCartpole *>(h)->mgr.curEpisode.load_relaxed(); }

// type codes: 0 State, -1 any other component
uint32_t ref_cartpole_guards(void *h, int32_t *out, uint32_t cap)
{
    auto *s = static_cast<RefCartpole *>(h);
    return refdrv::guards<Cartpole::Engine, Cartpole::Sim, Cartpole::State>(s->worlds, out, cap);
}

}  // extern "C"
