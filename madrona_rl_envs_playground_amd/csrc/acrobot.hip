// Acrobot world step for gfx950 (the reference's acrobat_env, Gym's Acrobot-v1): a two-link pendulum, three torques, one
// RK4 step of 0.2 s per environment step; one lane steps kWorlds worlds.
//
// Semantics: the reference's src/acrobat_env/sim.cpp:12-23 (constants), :68-94 (ds_dt, the dynamics "from the book"),
// :116-145 (rk4 over [0, dt]), :147-164 (wrap by repeated +-2 pi, bound), :166-187 (actionSystem: torque, step, wrap and
// clamp, reward -1 on EVERY step -- sim.hpp:51-53 promises 0 on the terminating one, the code never writes it),
// :189-206 (checkDone: -cos t1 - cos(t1 + t2) > 1, or episode length > 500), :45-66 (reset from the episode-seeded
// generator, rng.hpp:5-40: four draws mapped to -0.1 + r * 0.2).  Compiled with -ffp-contract=off like the rest.
//
// ONE DELIBERATE DEPARTURE: the episode length.  The reference keeps it in the EpisodeManager all worlds share
// (init.hpp:9, sim.cpp:52,169,199): every world increments the one counter and any reset zeroes it, so with N worlds
// "truncation" hits whichever world is visited first once the SUM passes 500, and only N = 1 behaves like Acrobot-v1 (an
// untouched episode ends at its 501st step).  Here the length is a word PER WORLD (the EPISODE_LENGTH tensor): every world
// behaves as the reference's N = 1 world does.
//
// Episode indices are taken in ascending world order within a step (see cartpole.hip):
//   mrl_step             one launch (mrl_acrobot_step_fused, in-kernel look-back, episode_scan.hpp)
//   mrl_step_phase1 / 2  mrl_acrobot_step : transition, done flag, ballot words, per-workgroup finished counts
//                        mrl::reseed_finished<AcrobotReseed>: exclusive prefix over the counts, re-seed finished worlds,
//                        zero their length (episode_scan.hpp)
// HBM traffic per world-step: action 4 + state r/w 32 + length r/w 8 + reward 4 + done 4 = 52 B.
//
// This is the one step in the tree that is bound by instruction issue, not by bytes: four derivative stages with four
// sines / cosines and three quotients each, two more cosines for the termination test.  What the default build does about
// it:
//   - per stage ONE range reduction per angle (sin and cos of theta1 and of theta2 from two reduced arguments and two
//     polynomial pairs); cos(theta1 - pi/2) and cos(theta1 + theta2 - pi/2) follow from the addition theorems, with the
//     reference's float pi / 2 (4.37e-8 above the real one) carried as a first-order term;
//   - the reduction is two fused multiply-adds while |angle| <= 128 (a live pendulum stays below 15); a world whose stage
//     angles leave that range, or whose new angles are more than two turns off, is stepped again by the plain
//     transition below -- per world, so a world's result never depends on its neighbours in the thread or the wave;
//   - quotients as v_rcp_f32 + one residual correction; the three by d1 share one reciprocal;
//   - kWorlds independent worlds per lane in one straight line of code for the scheduler to interleave.
// -DMRL_ACROBOT_PLAIN builds the straightforward variant instead: sinf / cosf called where the reference calls them,
// every expression typed and rounded as sim.cpp writes it, IEEE quotients (tools/acrobot_probe.py times one against the other).
#include "episode_host.hpp"
#include "episode_rng.hpp"
#include "random_policy.hpp"

namespace {

#ifndef MRL_ACROBOT_WORLDS
#define MRL_ACROBOT_WORLDS 4  // (a measurement build may ask for 1, 2 or 8: DESIGN.md section 10)
#endif
constexpr int kWorlds = MRL_ACROBOT_WORLDS;  // worlds per thread: independent dependency chains in one instruction stream
constexpr uint32_t kGroupWorlds = 1024;      // worlds per workgroup of the single-launch step
constexpr int kBlock = kGroupWorlds / kWorlds;
static_assert(kBlock * kWorlds == (int)kGroupWorlds && kBlock % 64 == 0 && kBlock <= 1024, "whole waves, one workgroup");
// Register budget: left to the compiler, which takes 162 VGPRs for the single-launch kernel and 147 for the two-launch one
// (three waves per SIMD, no scratch; of the 1024 workgroups of 1 M worlds 768 are resident and 256 follow as a second
// round).  Holding the kernels to 128 VGPRs -- four waves per SIMD, the whole grid resident in one round -- costs 144 / 68
// bytes of scratch per lane and was measured SLOWER at every size: the `four_waves` rows of
// profiles/acrobot_step_cost.json (tools/acrobot_probe.py builds it with -DMRL_ACROBOT_WAVES=4).
#ifndef MRL_ACROBOT_WAVES
#define MRL_ACROBOT_WAVES 1  // second argument of __launch_bounds__: the least waves per SIMD the compiler must make room for
#endif
constexpr int kWavesPerSimd = MRL_ACROBOT_WAVES;

#ifdef MRL_ACROBOT_PLAIN
constexpr bool kPlain = true;
#else
constexpr bool kPlain = false;
#endif

constexpr float kPi = 3.14159265358979323846f;  // madrona::math::pi is a float
constexpr float kStep = 0.2f;                   // sim.cpp:12, and t[1] - t[0] in rk4
constexpr float kHalfStep = (float)((double)kStep / 2.0);   // sim.cpp:131: float dt2 = dt / 2.0
constexpr float kSixthStep = (float)((double)kStep / 6.0);  // sim.cpp:132
constexpr float kMaxVel1 = 4 * kPi, kMaxVel2 = 9 * kPi;     // sim.cpp:22-23
constexpr float kGravity = 9.8f;
constexpr int32_t kMaxSteps = MRL_ACROBOT_MAX_STEPS;

// sim.cpp:59-65
__device__ __forceinline__ float4 fresh_state(uint32_t episode) { return mrl::uniform4(episode, -0.1f, 0.1f - (-0.1f)); }

// what the re-seeding launches store for a world that starts `episode` (mrl::reseed_finished, mrl::reseed_all)
struct AcrobotReseed {
    float4 *state;
    int32_t *length;
    __device__ __forceinline__ void operator()(uint32_t world, uint32_t episode) const
    {
        state[world] = fresh_state(episode);
        length[world] = 0;  // sim.cpp:52
    }
};

__device__ __forceinline__ float torque_of(int32_t action)
{
    // sim.cpp:171-174 indexes {-1, 0, +1} with the action; anything else applies no torque here
    return action == 0 ? -1.f : action == 2 ? 1.f : 0.f;
}

// ---- the plain transition: sim.cpp:68-206 expression by expression ----
// (theta1, theta2, omega1, omega2) -> their derivatives.  Constants folded where the folding is exact: m = l1 = I = 1,
// lc = 0.5, powf(0.5, 2) = 0.25, powf(x, 2) = x * x.  sim.cpp:86 writes cos(theta2) without the f: with <cmath> alone that is
// the C double function, so d2 is a double expression rounded to float once.
__device__ __forceinline__ void derivs_plain(float t1, float t2, float w1, float w2, float a, float &dw1, float &dw2)
{
    const float c2 = cosf(t2), s2 = sinf(t2);
    const float d1 = ((0.25f + (1.25f + c2)) + 1.f) + 1.f;
    const float d2 = (float)((0.25 + 0.5 * cos((double)t2)) + 1.0);
    const float phi2 = (0.5f * kGravity) * cosf((float)((double)(t1 + t2) - (double)kPi / 2.0));
    const float phi1 = (((-0.5f * (w2 * w2)) * s2 - (w2 * w1) * s2) + (1.5f * kGravity) * cosf(t1 - kPi / 2)) + phi2;
    dw2 = (((a + d2 / d1 * phi1) - (0.5f * (w1 * w1)) * s2) - phi2) / (1.25f - (d2 * d2) / d1);
    dw1 = -(d2 * dw2 + phi1) / d1;
}

// sim.cpp:147-159 with its two loops bounded: a value more than 64 turns off is brought back in one piece (the reference's
// loops would take as many trips, and never end once 2 pi is below the value's last place)
__device__ __forceinline__ float wrap_plain(float x)
{
    const float M = kPi, diff = kPi - (-kPi);
    for (int trips = 0; trips < 64 && x > M; trips++) x -= diff;
    for (int trips = 0; trips < 64 && x < -M; trips++) x += diff;
    if (fabsf(x) > M && fabsf(x) < __builtin_inff()) x = __builtin_fmaf(-rintf(x / diff), diff, x);
    return x;
}

__device__ __forceinline__ bool step_plain(float4 &s, float a)
{
    float k1[2], k2[2], k3[2], k4[2];
    derivs_plain(s.x, s.y, s.z, s.w, a, k1[0], k1[1]);
    const float w1b = s.z + k1[0] * kHalfStep, w2b = s.w + k1[1] * kHalfStep;
    derivs_plain(s.x + s.z * kHalfStep, s.y + s.w * kHalfStep, w1b, w2b, a, k2[0], k2[1]);
    const float w1c = s.z + k2[0] * kHalfStep, w2c = s.w + k2[1] * kHalfStep;
    derivs_plain(s.x + w1b * kHalfStep, s.y + w2b * kHalfStep, w1c, w2c, a, k3[0], k3[1]);
    const float w1d = s.z + k3[0] * kStep, w2d = s.w + k3[1] * kStep;
    derivs_plain(s.x + w1c * kStep, s.y + w2c * kStep, w1d, w2d, a, k4[0], k4[1]);
    // sim.cpp:140: y0 + (k1 + (2 k2 + (2 k3 + k4))) * dt6; the first two derivatives are the stages' velocities
    const float n0 = s.x + (s.z + (w1b * 2 + (w1c * 2 + w1d))) * kSixthStep;
    const float n1 = s.y + (s.w + (w2b * 2 + (w2c * 2 + w2d))) * kSixthStep;
    const float n2 = s.z + (k1[0] + (k2[0] * 2 + (k3[0] * 2 + k4[0]))) * kSixthStep;
    const float n3 = s.w + (k1[1] + (k2[1] * 2 + (k3[1] * 2 + k4[1]))) * kSixthStep;
    s.x = wrap_plain(n0);
    s.y = wrap_plain(n1);
    s.z = fminf(fmaxf(n2, -kMaxVel1), kMaxVel1);
    s.w = fminf(fmaxf(n3, -kMaxVel2), kMaxVel2);
    return -cosf(s.x) - cosf(s.y + s.x) > 1.0f;  // sim.cpp:195
}

// ---- the tuned transition ----
// sin and cos by minimax polynomials on [-pi/4, pi/4] (the classic single-precision kernels, < 1 ulp there), after a
// two-constant reduction by pi/2: k = rint(x 2/pi), r = x - k hi - k lo with hi = float(pi/2) and two fused multiply-adds.
// x - k hi is exact (both are multiples of hi's last place and the difference is small), so r is within half an ulp of
// x - k (hi + lo), and hi + lo is pi/2 to 1.7e-15: good for every |x| this path admits (kFastRange).
constexpr float kFastRange = 128.f;
__device__ __forceinline__ void sincos_fast(float x, float &sn, float &cs)
{
    const float k = rintf(x * 0.636619772f);
    float r = __builtin_fmaf(-k, 1.57079637f, x);
    r = __builtin_fmaf(-k, -4.37113883e-8f, r);
    const float z = r * r;
    float p = __builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
    p = __builtin_fmaf(p, z, -1.6666654611e-1f);
    const float ps = __builtin_fmaf(p * z, r, r);
    float q = __builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    q = __builtin_fmaf(q, z, 4.166664568298827e-2f);
    const float pc = __builtin_fmaf(q * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
    const uint32_t quadrant = (uint32_t)(int32_t)k;
    const bool odd = quadrant & 1u;
    const uint32_t sbits = __float_as_uint(odd ? pc : ps) ^ ((quadrant & 2u) << 30);
    const uint32_t cbits = __float_as_uint(odd ? ps : pc) ^ (((quadrant + 1u) & 2u) << 30);
    sn = __uint_as_float(sbits);
    cs = __uint_as_float(cbits);
}

// a / b to within an ulp: v_rcp_f32 (1 ulp) and one residual correction
__device__ __forceinline__ float quotient(float a, float b)
{
    const float r = __builtin_amdgcn_rcpf(b);
    const float q = a * r;
    return __builtin_fmaf(__builtin_fmaf(-b, q, a), r, q);
}

// The reference's cosf(x - pi/2) takes ITS pi / 2, the float 1.57079637 = pi/2 + 4.37e-8:
// cos(x - pi/2 - e) = sin x - e cos x + O(e^2)
constexpr float kHalfPiExcess = 4.37113883e-8f;

__device__ __forceinline__ void derivs_fast(float t1, float t2, float w1, float w2, float a, float &dw1, float &dw2)
{
    float s1, c1, s2, c2;
    sincos_fast(t1, s1, c1);
    sincos_fast(t2, s2, c2);
    const float s12 = __builtin_fmaf(s1, c2, c1 * s2), c12 = __builtin_fmaf(c1, c2, -(s1 * s2));
    const float d1 = c2 + 3.5f;                         // in [2.5, 4.5]
    const float d2 = __builtin_fmaf(0.5f, c2, 1.25f);   // in [0.75, 1.75]
    const float phi2 = (0.5f * kGravity) * __builtin_fmaf(-kHalfPiExcess, c12, s12);
    const float lower = __builtin_fmaf(1.5f * kGravity, __builtin_fmaf(-kHalfPiExcess, c1, s1), phi2);
    const float phi1 = __builtin_fmaf(-(w2 * s2), __builtin_fmaf(0.5f, w2, w1), lower);
    float inv_d1 = __builtin_amdgcn_rcpf(d1);
    inv_d1 = __builtin_fmaf(__builtin_fmaf(-d1, inv_d1, 1.f), inv_d1, inv_d1);
    const float ratio = d2 * inv_d1;
    const float den = __builtin_fmaf(-d2, ratio, 1.25f);  // >= 0.56
    const float num = __builtin_fmaf(-0.5f * w1, w1 * s2, __builtin_fmaf(ratio, phi1, a)) - phi2;
    dw2 = quotient(num, den);
    dw1 = -__builtin_fmaf(d2, dw2, phi1) * inv_d1;
}

// two trips of each of sim.cpp:150-157's loops as selects: enough for a new angle within two turns of [-pi, pi]
__device__ __forceinline__ float wrap_fast(float x)
{
    const float M = kPi, diff = kPi - (-kPi);
    x = x > M ? x - diff : x;
    x = x > M ? x - diff : x;
    x = x < -M ? x + diff : x;
    x = x < -M ? x + diff : x;
    return x;
}

// false: outside what this path is good for (stage angles beyond kFastRange, a new angle still unwrapped): the caller
// steps the world again with step_plain from its old state
__device__ __forceinline__ bool step_fast(float4 &s, float a, bool &over)
{
    float k1[2], k2[2], k3[2], k4[2];
    derivs_fast(s.x, s.y, s.z, s.w, a, k1[0], k1[1]);
    const float w1b = __builtin_fmaf(k1[0], kHalfStep, s.z), w2b = __builtin_fmaf(k1[1], kHalfStep, s.w);
    const float t1b = __builtin_fmaf(s.z, kHalfStep, s.x), t2b = __builtin_fmaf(s.w, kHalfStep, s.y);
    derivs_fast(t1b, t2b, w1b, w2b, a, k2[0], k2[1]);
    const float w1c = __builtin_fmaf(k2[0], kHalfStep, s.z), w2c = __builtin_fmaf(k2[1], kHalfStep, s.w);
    const float t1c = __builtin_fmaf(w1b, kHalfStep, s.x), t2c = __builtin_fmaf(w2b, kHalfStep, s.y);
    derivs_fast(t1c, t2c, w1c, w2c, a, k3[0], k3[1]);
    const float w1d = __builtin_fmaf(k3[0], kStep, s.z), w2d = __builtin_fmaf(k3[1], kStep, s.w);
    const float t1d = __builtin_fmaf(w1c, kStep, s.x), t2d = __builtin_fmaf(w2c, kStep, s.y);
    derivs_fast(t1d, t2d, w1d, w2d, a, k4[0], k4[1]);
    const float n0 = __builtin_fmaf(s.z + __builtin_fmaf(2.f, w1b + w1c, w1d), kSixthStep, s.x);
    const float n1 = __builtin_fmaf(s.w + __builtin_fmaf(2.f, w2b + w2c, w2d), kSixthStep, s.y);
    const float n2 = __builtin_fmaf(k1[0] + __builtin_fmaf(2.f, k2[0] + k3[0], k4[0]), kSixthStep, s.z);
    const float n3 = __builtin_fmaf(k1[1] + __builtin_fmaf(2.f, k2[1] + k3[1], k4[1]), kSixthStep, s.w);
    // the largest stage angle (a NaN falls through fmaxf and comes out of the arithmetic as a NaN either way)
    const float reach = fmaxf(fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fmaxf(fabsf(t1b), fabsf(t2b))),
                              fmaxf(fmaxf(fabsf(t1c), fabsf(t2c)), fmaxf(fabsf(t1d), fabsf(t2d))));
    const float t1 = wrap_fast(n0), t2 = wrap_fast(n1);
    const bool good = reach <= kFastRange && !(fabsf(t1) > kPi) && !(fabsf(t2) > kPi);
    s.x = t1;
    s.y = t2;
    s.z = fminf(fmaxf(n2, -kMaxVel1), kMaxVel1);
    s.w = fminf(fmaxf(n3, -kMaxVel2), kMaxVel2);
    float s1, c1, s2, c2;
    sincos_fast(t1, s1, c1);
    sincos_fast(t2, s2, c2);
    over = -c1 - __builtin_fmaf(c1, c2, -(s1 * s2)) > 1.0f;
    return good;
}

// sim.cpp:166-206 for the K worlds of a thread: new state, new episode length, over[u] = world u's done flag.  Pure in
// (state, length, action).  The ONE transition of this file: the two-launch step, the single-launch step and the
// single-launch step's recount all go through here, so they cannot disagree on a done flag.
template <int K>
__device__ __forceinline__ void advance(float4 (&s)[K], int32_t (&length)[K], const int32_t (&action)[K], bool (&over)[K])
{
    if constexpr (kPlain) {
#pragma unroll
        for (int u = 0; u < K; u++) over[u] = step_plain(s[u], torque_of(action[u]));
    } else {
        float4 old[K];
        bool good[K], all_good = true;
#pragma unroll
        for (int u = 0; u < K; u++) {
            old[u] = s[u];
            good[u] = step_fast(s[u], torque_of(action[u]), over[u]);
            all_good &= good[u];
        }
        if (!all_good) {  // never for a pendulum within the velocity bounds; one copy of the plain code, a world at a time
#pragma unroll 1
            for (int turn = 0; turn < K; turn++) {
                float4 in = old[0];
                float a = torque_of(action[0]);
                bool mine = !good[0];
#pragma unroll
                for (int u = 1; u < K; u++)
                    if (u == turn) {
                        in = old[u];
                        a = torque_of(action[u]);
                        mine = !good[u];
                    }
                if (mine) {
                    const bool finished = step_plain(in, a);
#pragma unroll
                    for (int u = 0; u < K; u++)
                        if (u == turn) {
                            s[u] = in;
                            over[u] = finished;
                        }
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < K; u++) {
        length[u] += 1;                       // sim.cpp:169
        over[u] |= length[u] > kMaxSteps;     // sim.cpp:199
    }
}

// the caller's action, or the uniform random policy's draw (include/mrl_envs.h: mrl_rollout_random)
__device__ __forceinline__ int32_t action_of(const int32_t *action, uint32_t w, bool sampled, uint64_t seed, uint32_t step)
{
    return sampled ? (int32_t)mrl::scale(mrl::policy_hash(seed, step, w, 0), 3u) : action[w];
}

// Both launches of the two-launch step run on the same grid: workgroup b owns worlds [b*chunk, (b+1)*chunk), chunk a
// multiple of kBlock, and walks it kWorlds * kBlock worlds per trip.  Besides the int32 done flags of the RESET tensor
// every wave stores the ballot of its 64 flags as one word of finished_mask (world i = bit i % 64 of word i / 64), which is
// what the reset launch reads (see cartpole.hip).
__global__ void __launch_bounds__(kBlock, kWavesPerSimd) mrl_acrobot_step(uint32_t n, uint32_t chunk, const int32_t *action,  // (no __restrict__: may be action_out)
                                                           float4 *__restrict__ state, int32_t *__restrict__ length,
                                                           float *__restrict__ reward, int32_t *__restrict__ done,
                                                           uint32_t *__restrict__ block_counts,
                                                           unsigned long long *__restrict__ finished_mask, int32_t *action_out,
                                                           uint64_t sample_seed, uint32_t sample_step)
{
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t first = blockIdx.x * chunk, last = min(n, first + chunk);
    const bool sampled = action_out != nullptr;
    uint32_t finished = 0;  // wave-uniform
    for (uint32_t i0 = first + threadIdx.x; i0 - threadIdx.x < last; i0 += kWorlds * kBlock) {  // uniform trip count
        float4 s[kWorlds];
        int32_t len[kWorlds], a[kWorlds];
#pragma unroll
        for (int u = 0; u < kWorlds; u++) {
            const uint32_t i = i0 + u * kBlock;
            const uint32_t ic = i < last ? i : first;  // clamped: loads stay in bounds
            s[u] = state[ic];
            len[u] = length[ic];
            a[u] = action_of(action, ic, sampled, sample_seed, sample_step);
            if (sampled && i < last) action_out[i] = a[u];
        }
        bool finishes[kWorlds];
        advance<kWorlds>(s, len, a, finishes);  // (rounds past the end run on world `first`'s values and are dropped)
#pragma unroll
        for (int u = 0; u < kWorlds; u++) {
            const uint32_t i = i0 + u * kBlock;
            const bool over = finishes[u] && i < last;
            if (i < last) {
                state[i] = s[u];
                length[i] = len[u];
                reward[i] = -1.f;  // sim.cpp:186
                done[i] = over ? 1 : 0;
            }
            finished += mrl::note_finished(over, i, i < last, finished_mask);
        }
    }
    mrl::post_wave_count(finished, s_wave);
    __syncthreads();
    mrl::store_block_count(s_wave, block_counts);
}

// How many of workgroup j's worlds finish in this step, worked out by ONE wave of another workgroup from j's inputs in HBM
// (state, length, and the action or its draw): what the healing look-back of the single-launch step calls for a workgroup
// whose own count has not appeared (episode_scan.hpp).  Unlike Cartpole's, the flag needs the whole transition.
__device__ __forceinline__ uint32_t recount_chunk(uint32_t n, const int32_t *action, const float4 *state, const int32_t *length, uint32_t j,
                                                   bool sampled, uint64_t seed, uint32_t step)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t first = j * kGroupWorlds, last = min(n, first + kGroupWorlds);
    uint32_t count = 0;
    for (uint32_t i0 = first; i0 < last; i0 += 64u) {
        const uint32_t i = i0 + lane, ic = i < last ? i : first;
        float4 s[1] = {state[ic]};
        int32_t len[1] = {length[ic]};
        const int32_t a[1] = {action_of(action, ic, sampled, seed, step)};
        bool over[1];
        advance<1>(s, len, a, over);
        count += (uint32_t)__popcll(__ballot(over[0] && i < last));
    }
    return count;
}

// The whole step in one launch (mrl_step / mrl_step_with_actions / mrl_rollout_random on one GPU): workgroup b owns worlds
// [1024 b, 1024 b + 1024), four per thread, in registers from the load to the store.
//
// Order of events in a workgroup (the protocol and its shared helpers: DESIGN.md 4.6): loads (state, length, action or its
// draw) -> the WHOLE transition of its 1024 worlds, because here the done flag is the end of the arithmetic (the height of
// the new pose, the new length) -> votes, tally -> the count is PUBLISHED and the publishing wave waits for that store to
// be acknowledged (s_waitcnt vmcnt(0), as in cartpole.hip) -> __syncthreads -> the first wave looks back while the other
// waves already store what needs no prefix: state and length of the worlds that go on, reward, done -> the finished
// worlds follow as their next episodes, length 0.  (The drawn actions of a rollout go out before the count: the recount
// draws them again from the hash and never reads ACTION.)
// kStats (mrl_enable_episode_stats): the lane also keeps its four worlds' episode returns and step counts.  They are loaded
// AFTER the transition, behind the first barrier -- its registers are what bounds this kernel, and the values are not needed
// before the stores, two barriers later -- and thread 0 adds the workgroup's finished episodes to TOTALS block b behind the
// last barrier (episode_stats.hpp).  171 VGPRs against 162, two waves per SIMD against three: DESIGN.md section 11 has the
// measurement that keeps this form.  Without kStats the kernel is what it was.
template <bool kStats>
__global__ void __launch_bounds__(kBlock, kWavesPerSimd) mrl_acrobot_step_fused(uint32_t n, const int32_t *action,  // (no __restrict__: may be action_out)
                                                                 float4 *__restrict__ state, int32_t *__restrict__ length,
                                                                 float *__restrict__ reward, int32_t *__restrict__ done, uint32_t *status,
                                                                 unsigned long long *group_total, uint32_t epoch,
                                                                 const uint32_t *episode_base, uint32_t *next_counter,
                                                                 uint32_t *__restrict__ reset_count, int32_t *action_out,
                                                                 uint64_t sample_seed, uint32_t sample_step, const mrl::HealTest heal,
                                                                 const mrl::DeviceCounter device_counter,
                                                                 const mrl::FusedExchange fx,  // sharded batch: the other ranks' counts (episode_scan.hpp)
                                                                 const mrl::StatsArg<kStats> stats)
{
    __shared__ uint32_t s_wave[kWorlds][kBlock / 64];
    __shared__ mrl::EpisodeNumbers s_numbers;
    const uint32_t b = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t first = b * kGroupWorlds, last = min(n, first + kGroupWorlds);
    const bool last_block = b == gridDim.x - 1, sampled = action_out != nullptr;
    device_counter.apply(episode_base, next_counter, epoch);  // (the launch state may live in device memory: common.hpp)
    mrl::heal_test_delay(heal, b, gridDim.x, epoch);          // test hook only
    const uint32_t base = *episode_base;
    float4 s[kWorlds];
    int32_t len[kWorlds], a[kWorlds];
    bool over[kWorlds];
    uint32_t rank[kWorlds];  // among the workgroup's finished worlds, in ascending world order (round u covers worlds first + 256 u ...)
#pragma unroll
    for (int u = 0; u < kWorlds; u++) {
        const uint32_t w = first + u * kBlock + threadIdx.x, wc = w < last ? w : first;  // clamped: loads stay in bounds
        s[u] = state[wc];
        len[u] = length[wc];
        a[u] = action_of(action, wc, sampled, sample_seed, sample_step);
        if (sampled && w < last) action_out[w] = a[u];
    }
    advance<kWorlds>(s, len, a, over);
#pragma unroll
    for (int u = 0; u < kWorlds; u++) {
        over[u] = over[u] && first + u * kBlock + threadIdx.x < last;
        rank[u] = mrl::cast_vote(over[u], s_wave[u]);
    }
    __syncthreads();
    using Stats = mrl::StatsWorlds<1>;
    [[maybe_unused]] Stats tally;
    [[maybe_unused]] typename Stats::World running[kWorlds];
    if constexpr (kStats) {  // (behind the barrier: not in flight during the transition)
#pragma unroll
        for (int u = 0; u < kWorlds; u++) {
            const uint32_t w = first + u * kBlock + threadIdx.x;
            running[u] = Stats::load(stats, w < last ? w : first);
        }
    }
    const uint32_t block_total = mrl::tally_votes<kWorlds, kBlock>(s_wave, rank);
    if (threadIdx.x == 0) mrl::publish_count(status, b, epoch, block_total);
    // The count is globally visible before any wave of this workgroup changes a world: the publishing wave waits for ITS
    // store to be acknowledged in front of the barrier (the barrier alone makes no wave wait for its stores; only the drawn
    // actions of a rollout are outstanding besides, so the wait is short).
    if (wave == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool needs_prefix = block_total != 0 || last_block;
    if (threadIdx.x < 64)  // (a workgroup that closes a group of 256 looks back whatever its count)
        mrl::fused_lookback(s_numbers, status, group_total, epoch, block_total, needs_prefix, heal, fx, [&](uint32_t j) {
            return recount_chunk(n, action, state, length, j, sampled, sample_seed, sample_step);
        });
    // what does not need the prefix goes out while the first wave is still looking back (the other three are here right
    // after the barrier; the first wave's loads come before its stores: behind them they would sit out their acknowledgement)
#pragma unroll
    for (int u = 0; u < kWorlds; u++) {
        const uint32_t w = first + u * kBlock + threadIdx.x;
        if (w < last) {
            if (!over[u]) {
                state[w] = s[u];
                length[w] = len[u];
            }
            reward[w] = -1.f;  // sim.cpp:186
            done[w] = over[u] ? 1 : 0;
            if constexpr (kStats) tally.finish(stats, w, running[u], -1.f, over[u]);
        }
    }
    if (!needs_prefix) return;  // uniform per workgroup
    [[maybe_unused]] double *s_sums = nullptr;
    if constexpr (kStats) {
        __shared__ double s_stats[kBlock / 64][2];
        s_sums = &s_stats[0][0];
        if (block_total != 0) tally.to_lds(s_sums, wave, lane);  // uniform per workgroup
    }
    mrl::lds_barrier();
    if constexpr (kStats) {
        if (threadIdx.x == 0 && block_total != 0) Stats::add_totals(stats, s_sums, kBlock / 64, b, block_total);
    }
    const uint32_t own_before = s_numbers.own_before, before = own_before + s_numbers.lower_ranks;
#pragma unroll
    for (int u = 0; u < kWorlds; u++) {
        const uint32_t w = first + u * kBlock + threadIdx.x;
        if (over[u]) {  // the finished world's next episode, stored in its place (over[u] implies w < last)
            state[w] = fresh_state(base + before + rank[u]);
            length[w] = 0;
        }
    }
    if (last_block && threadIdx.x == 0) mrl::close_step(own_before, block_total, base, s_numbers.all_counts, reset_count, next_counter);
}

struct AcrobotSim final : mrl::EpisodeSim {
    int32_t *done = nullptr, *world_id = nullptr, *length = nullptr;
    float4 *state = nullptr;
    float *reward = nullptr;

    void launch_fused(const int32_t *actions, const Drawn &drawn, const mrl::FusedExchange &fx, const Counters &c, hipStream_t stream) override
    {
        single_launch(mrl_acrobot_step_fused<true>, mrl_acrobot_step_fused<false>, kBlock, stream, num_worlds, actions ? actions : action, state,
                      length, reward, done, status, group_total, epoch, c.base, c.next, reset_count, drawn.action_out, drawn.seed, drawn.step, heal,
                      c.device, fx)();
    }
    void launch_step(const int32_t *actions, int32_t *action_out, uint64_t seed, uint32_t sample_step, hipStream_t stream) override
    {
        hipLaunchKernelGGL(mrl_acrobot_step, dim3(grid), dim3(kBlock), 0, stream, num_worlds, chunk, actions ? actions : action, state, length,
                           reward, done, block_counts, stepped.words, action_out, seed, sample_step);
        MRL_HIP(hipGetLastError());
    }
    void phase1(const int32_t *actions, hipStream_t stream) override { launch_step(actions, nullptr, 0, 0, stream); }
    void launch_reseed(const Finished &from, const mrl::GatheredCounts &gathered, const Counters &c, hipStream_t stream) override
    {
        hipLaunchKernelGGL((mrl::reseed_finished<kBlock, AcrobotReseed>), dim3(grid), dim3(kBlock), 0, stream, num_worlds, chunk,
                           AcrobotReseed{state, length}, from.block_counts, from.words, c.base, c.next, from.reset_count, gathered, c.device);
    }
    void reseed_shard(uint32_t world_offset, uint32_t num_worlds_total, hipStream_t stream) override
    {
        hipLaunchKernelGGL(mrl::reseed_all<AcrobotReseed>, dim3((num_worlds + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, num_worlds,
                           world_offset, AcrobotReseed{state, length});
        MRL_HIP(hipGetLastError());
        MRL_HIP(hipMemsetAsync(length, 0, sizeof(int32_t) * num_worlds, stream));
        MRL_HIP(hipMemsetAsync(done, 0, sizeof(int32_t) * num_worlds, stream));
        MRL_HIP(hipMemsetAsync(reward, 0, sizeof(float) * num_worlds, stream));
        set_episode_counter(num_worlds_total, stream);
    }

    bool tensor(int slot, mrl_tensor_desc *out) override
    {
        const int64_t N = num_worlds;
        switch (slot) {
        case MRL_ACROBOT_RESET: *out = mrl::make_desc(done, MRL_INT32, device, {N, 1}); return true;
        case MRL_ACROBOT_ACTION: *out = mrl::make_desc(action, MRL_INT32, device, {N, 1}); return true;
        case MRL_ACROBOT_STATE: *out = mrl::make_desc(state, MRL_FLOAT32, device, {N, 4}); return true;
        case MRL_ACROBOT_REWARD: *out = mrl::make_desc(reward, MRL_FLOAT32, device, {N, 1}); return true;
        case MRL_ACROBOT_WORLD_ID: *out = mrl::make_desc(world_id, MRL_INT32, device, {N, 1}); return true;
        case MRL_ACROBOT_RESET_COUNT: *out = mrl::make_desc(reset_count, MRL_UINT32, device, {1}); return true;
        case MRL_ACROBOT_SCAN_TIMEOUT: *out = mrl::make_desc(alarm.alarm().dev, MRL_UINT32, device, {1}); return true;
        case MRL_ACROBOT_SHARD_COUNT: *out = mrl::make_desc(shard_count, MRL_UINT32, device, {1}); return true;
        case MRL_ACROBOT_EPISODE_LENGTH: *out = mrl::make_desc(length, MRL_INT32, device, {N, 1}); return true;
        default: return false;
        }
    }

    size_t action_elems() const override { return (size_t)num_worlds; }
    const char *kernel_name() const override { return fused ? "mrl_acrobot_step_fused" : "mrl_acrobot_step"; }
    // action 4 + state r/w 32 + length r/w 8 + reward 4 + done 4
    uint64_t bytes_per_world_step() const override { return 52; }
    void launch_shape(uint32_t out[4]) const override
    {
        out[0] = fused ? fused_grid : grid;
        out[1] = kBlock;
        out[2] = 0;
        out[3] = kWorlds * 64;
    }
};

}  // namespace

mrl_sim *mrl::create_acrobot(int gpu_id, uint32_t num_worlds)
{
    return create_episode_sim<AcrobotSim>("acrobot", MRL_GAME_ACROBOT, gpu_id, num_worlds, [&](AcrobotSim *sim) {
        sim->size_scan_grid(kBlock);
        sim->action = sim->arena.alloc<int32_t>(num_worlds);
        sim->done = sim->arena.alloc<int32_t>(num_worlds);
        sim->world_id = sim->arena.alloc<int32_t>(num_worlds);
        sim->length = sim->arena.alloc<int32_t>(num_worlds);
        sim->state = sim->arena.alloc<float4>(num_worlds);
        sim->reward = sim->arena.alloc<float>(num_worlds);
        sim->alloc_episode(true, false);
        sim->alloc_fused(kGroupWorlds);
        sim->alarm.init(sim->arena);
        sim->launch_state.init(sim->arena);
        sim->read_step_knobs(sim->fused_grid != 0, sim->fused_grid);  // one launch wherever it exists
        mrl::fill_ids(sim->world_id, nullptr, 1, num_worlds);
        sim->reseed_shard(0, num_worlds, 0);  // Sim::Sim (sim.cpp:216-236): world w starts as episode w
        sim->inject_scan_timeout();
    });
}
