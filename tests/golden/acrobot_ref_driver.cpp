// TEST INFRASTRUCTURE ONLY -- the reference's Acrobot sim.cpp, compiled unchanged against the Madrona stand-in
// (oracle/madrona_standin, with tests/golden/acrobot_standin in front for <madrona/math.hpp>), behind a small C ABI for
// tests/golden/make_acrobot_golden.py.  REF_SIM is the path of the reference's src/acrobat_env/sim.cpp.  No game logic here.
// Arithmetic: g++ -ffp-contract=off on x86-64, sinf / cosf from the C library.  Episode order: oracle/ref_driver_common.hpp.
#include REF_SIM

#include "ref_driver_common.hpp"

namespace {

struct RefAcrobot {
    uint32_t n;
    Acrobat::EpisodeManager mgr;
    refdrv::Worlds<Acrobat::Engine, Acrobat::Sim> worlds;
    Acrobat::Engine &ctx(uint32_t w) { return *worlds.engines[w]; }
    madrona::Entity agent(uint32_t w) { return worlds.sims[w]->agents[0]; }
};

}  // namespace

extern "C" {

void *ref_acrobot_create(uint32_t n, uint32_t first_episode)
{
    auto *s = new RefAcrobot();
    s->n = n;
    s->mgr.curEpisode.store_relaxed(first_episode);
    s->mgr.episodeLength = 0;
    Acrobat::Config config{};
    Acrobat::WorldInit init{&s->mgr};
    s->worlds.create(n, 0, false, config, init);
    return s;
}

void ref_acrobot_destroy(void *h) { delete static_cast<RefAcrobot *>(h); }

// actions: (N,) int32
void ref_acrobot_step(void *h, const int32_t *actions)
{
    auto *s = static_cast<RefAcrobot *>(h);
    for (uint32_t w = 0; w < s->n; w++) s->ctx(w).get<Acrobat::Action>(s->agent(w)).choice = actions[w];
    s->worlds.step();
}

// state (N, 4) f32 (theta1, theta2, omega1, omega2), reward (N,) f32, done (N,) i32 (the agent's WorldReset)
void ref_acrobot_read(void *h, float *state, float *reward, int32_t *done)
{
    auto *s = static_cast<RefAcrobot *>(h);
    for (uint32_t w = 0; w < s->n; w++) {
        Acrobat::Engine &c = s->ctx(w);
        const madrona::Entity e = s->agent(w);
        const Acrobat::State &st = c.get<Acrobat::State>(e);
        state[4 * (size_t)w + 0] = st.theta1;
        state[4 * (size_t)w + 1] = st.theta2;
        state[4 * (size_t)w + 2] = st.omega1;
        state[4 * (size_t)w + 3] = st.omega2;
        reward[w] = c.get<Acrobat::Reward>(e).rew;
        done[w] = c.get<Acrobat::WorldReset>(e).resetNow;
    }
}

void ref_acrobot_set_state(void *h, const float *state)
{
    auto *s = static_cast<RefAcrobot *>(h);
    for (uint32_t w = 0; w < s->n; w++) {
        Acrobat::State &st = s->ctx(w).get<Acrobat::State>(s->agent(w));
        st.theta1 = state[4 * (size_t)w + 0];
        st.theta2 = state[4 * (size_t)w + 1];
        st.omega1 = state[4 * (size_t)w + 2];
        st.omega2 = state[4 * (size_t)w + 3];
    }
}

// the ONE episode length all worlds of the reference share (init.hpp)
void ref_acrobot_set_length(void *h, uint32_t length) { static_cast<RefAcrobot *>(h)->mgr.episodeLength = length; }
uint32_t ref_acrobot_length(void *h) { return static_cast<RefAcrobot *>(h)->mgr.episodeLength; }
uint32_t ref_acrobot_episodes(void *h) { return static_cast<RefAcrobot *>(h)->mgr.curEpisode.load_relaxed(); }

}  // extern "C"
