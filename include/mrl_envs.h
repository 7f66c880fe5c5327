/*
 * mrl_envs.h -- C ABI of the MI355X-native batched RL-environment step engine.
 *
 * One shared library (libmrl_envs.so, built by hipcc for gfx950) replaces, for
 * the step hot path only, what the reference exposes through its nanobind
 * modules.  Every entry point cites the reference interface it stands in for
 * (paths under /root/reference).  Plain C types only: no torch, no C++ classes.
 *
 *   reference                                         this ABI
 *   ------------------------------------------------  ---------------------------
 *   OvercookedSimulator.__init__                      mrl_overcooked_create
 *     src/overcooked_env/bindings.cpp:14-71,
 *     Manager::Impl::init mgr.cpp:138-188
 *   HanabiSimulator.__init__                          mrl_hanabi_create
 *     src/hanabi_env/bindings.cpp:10-36, mgr.cpp:144-166
 *   CartpoleSimulator.__init__                        mrl_cartpole_create
 *     src/cartpole_env/bindings.cpp:11-24, mgr.cpp:138-163
 *   Manager::step (all three)                         mrl_step
 *     src/overcooked_env/mgr.cpp:196-199,
 *     src/hanabi_env/mgr.cpp:174-177, src/cartpole_env/mgr.cpp:169-172
 *   Manager::*Tensor()  -> madrona::py::Tensor        mrl_tensor(slot)
 *     src/overcooked_env/mgr.cpp:201-259,
 *     src/hanabi_env/mgr.cpp:179-232, src/cartpole_env/mgr.cpp:174-202
 *   Manager::~Manager                                 mrl_destroy
 *   FATAL()/abort on error (mgr.cpp:177)              return code + mrl_last_error
 *
 * Ownership: the simulator owns every buffer it exports for its whole
 * lifetime (the reference's Manager owns its export buffers the same way,
 * mgr.hpp:63); mrl_tensor hands out device pointers that never move.  The
 * caller writes actions in place into the ACTION tensor before mrl_step and
 * reads results in place after it, exactly as the reference's Python wrappers
 * do (envs/overcooked_env.py:104-113, pantheonrl_extension/vectorenv.py:306-329).
 *
 * Streams: mrl_step only enqueues work on the HIP stream it is given (NULL =
 * the default stream) and never synchronises the host; ordering with the
 * caller's own work on that stream is the stream's.  A handle is bound to one
 * device and is not thread-safe (neither is the reference's Manager).
 *
 * New functionality with no reference counterpart (the reference is
 * single-device): the two-phase step and the episode
 * base used to keep episode numbering identical when worlds are sharded over
 * several GPUs.
 */
#ifndef MRL_ENVS_H
#define MRL_ENVS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRL_ABI_VERSION 4

/* return codes */
enum {
    MRL_OK = 0,
    MRL_ERR_INVALID = 1, /* bad argument / unsupported configuration          */
    MRL_ERR_DEVICE = 2,  /* no usable gfx950 device, or a HIP call failed      */
    MRL_ERR_SLOT = 3     /* tensor slot not exported by this game             */
};

/* element types of exported tensors (madrona::py::Tensor::ElementType subset) */
enum { MRL_INT8 = 0, MRL_UINT8 = 1, MRL_INT32 = 2, MRL_FLOAT32 = 3, MRL_UINT32 = 4 };
#define MRL_FLOAT64 5 /* the TOTALS tensor of mrl_enable_episode_stats */

enum { MRL_GAME_OVERCOOKED = 1, MRL_GAME_HANABI = 2, MRL_GAME_CARTPOLE = 3, MRL_GAME_SIMPLECOOKED = 4, MRL_GAME_BALANCE = 5, MRL_GAME_ACROBOT = 6 };

typedef struct mrl_sim mrl_sim;

#define MRL_MAX_DIMS 6
typedef struct mrl_tensor_desc {
    void *data;                    /* device pointer (HBM), valid until mrl_destroy   */
    int32_t dtype;                 /* MRL_INT8 ...                                    */
    int32_t ndim;
    int64_t shape[MRL_MAX_DIMS];
    int64_t strides[MRL_MAX_DIMS]; /* in elements; exported views may be strided      */
    int32_t device;                /* HIP device ordinal                              */
    int32_t reserved;
} mrl_tensor_desc;

/* ------------------------------------------------------------------ */
/* Overcooked  (reference: src/overcooked_env)                          */
/* ------------------------------------------------------------------ */

/* Mirrors Manager::Config (mgr.hpp:16-35): the Python layout transform
 * (envs/overcooked_env.py:261-371) produces exactly these fields.  Limits are
 * the reference's: height*width <= 255 (WorldState.size is uint8, sim.hpp:86),
 * num_players <= 64 (sim.hpp:14); reward / recipe entries are stored as uint8
 * (sim.hpp:95-99). */
typedef struct mrl_overcooked_config {
    int64_t height, width, num_players;
    int64_t placement_in_pot_rew, dish_pickup_rew, soup_pickup_rew;
    int64_t horizon;
    const int64_t *terrain;        /* height*width, row-major, TerrainT values 0..6 */
    const int64_t *start_player_x; /* num_players                                   */
    const int64_t *start_player_y; /* num_players                                   */
    const int64_t *recipe_values;  /* 16, index 4*onions + tomatoes                 */
    const int64_t *recipe_times;   /* 16                                            */
} mrl_overcooked_config;

/* Tensor slots = ExportID (sim.hpp:23-37) + this engine's world-major views.
 * P players, N worlds, C = height*width, F = 5P + 16.
 *   DONE              int32 (N)
 *   ACTIVE_AGENT      int32 (P, N)            all ones (sim.cpp:619)
 *   ACTION            int32 (P, N, 1)         written by the caller
 *   OBSERVATION       int8  (P*C, N, F)       strided view of OBS_WORLD_MAJOR; row id
 *                                             p*C + cell like LocationXID (sim.cpp:633).
 *                                             The reference pads rows to 336 bytes
 *                                             (sim.hpp:125-127) and callers slice [:F];
 *                                             here the last dimension is F already.
 *   ACTION_MASK       int32 (P, N, 6)         all ones (sim.cpp:616-618)
 *   REWARD            int32 (P, N)
 *   WORLD_ID          int32 (P, N)            [p, n] = n
 *   AGENT_ID          int32 (P, N)            [p, n] = p
 *   LOCATION_WORLD_ID int32 (P*C, N)          [r, n] = n
 *   LOCATION_ID       int32 (P*C, N)          [r, n] = r
 *   OBS_WORLD_MAJOR   int8  (N, P, H, W, F)   contiguous; what the kernel writes
 *   STATE_PLAYERS     uint8 (N, P, 8)         pos, orientation, pad, pad, held{name,on,tom,tick}
 *   STATE_OBJECTS     uint8 (N, C, 4)         name, onions, tomatoes, cooking_tick
 *   STATE_TIMESTEP    int32 (N)
 */
enum {
    MRL_OVERCOOKED_DONE = 0,
    MRL_OVERCOOKED_ACTIVE_AGENT = 1,
    MRL_OVERCOOKED_ACTION = 2,
    MRL_OVERCOOKED_OBSERVATION = 3,
    MRL_OVERCOOKED_ACTION_MASK = 4,
    MRL_OVERCOOKED_REWARD = 5,
    MRL_OVERCOOKED_WORLD_ID = 6,
    MRL_OVERCOOKED_AGENT_ID = 7,
    MRL_OVERCOOKED_LOCATION_WORLD_ID = 8,
    MRL_OVERCOOKED_LOCATION_ID = 9,
    MRL_OVERCOOKED_OBS_WORLD_MAJOR = 10,
    MRL_OVERCOOKED_STATE_PLAYERS = 11,
    MRL_OVERCOOKED_STATE_OBJECTS = 12,
    MRL_OVERCOOKED_STATE_TIMESTEP = 13
};

/* replaces OvercookedSimulator(exec_mode=CUDA, gpu_id, num_worlds, **layout)
 * (bindings.cpp:14-71).  There is no CPU execution mode behind this ABI. */
int mrl_overcooked_create(const mrl_overcooked_config *cfg, int gpu_id, uint32_t num_worlds, mrl_sim **out);

/* ------------------------------------------------------------------ */
/* Simplecooked  (reference: src/overcooked2_env, the world the trainer */
/* and the Colab notebook use: train/env_utils.py:3)                    */
/* ------------------------------------------------------------------ */

/* replaces SimplecookedSimulator(exec_mode=CUDA, gpu_id, num_worlds, **layout)
 * (src/overcooked2_env/bindings.cpp:15-71; Manager::Config mgr.hpp:16-35 has the fields of
 * mrl_overcooked_config, so the struct is shared).  Differences from Overcooked that the caller sees:
 * terrain values follow overcooked2's enum AIR, POT, COUNTER, ONION_SOURCE, DISH_SOURCE, SERVING,
 * TOMATO_SOURCE (sim.hpp:40); height*width <= 100 and num_players <= 2 (sim.hpp:12-13); rows are
 * F = 5P + 10 bytes (sim.hpp:121-123), so OBSERVATION is int8 (P*C, N, 5P+10) and OBS_WORLD_MAJOR
 * (N, P, H, W, 5P+10); dish_pickup_rew is paid (sim.cpp:241-246).  Slots: the MRL_OVERCOOKED_* ids
 * (ExportID is the same list, sim.hpp:22-37) plus STATE_DISHES_OUT int32 (N) = WorldState.num_dishes_out.
 * mrl_cnn_act and mrl_rollout_cnn take a Simplecooked simulator as they take an Overcooked one -- they read OBS_WORLD_MAJOR, DONE,
 * REWARD and ACTION under those same MRL_OVERCOOKED_* ids --, with one or two players: F = 5P + 10 is 15 or 20 channels, and the
 * ring of mrl_rollout_cnn is what mrl_mappo_update reads.  This is the reference's own training configuration (MAPPO's CNN
 * actor-critic on layout `simple`). */
enum { MRL_SIMPLECOOKED_STATE_DISHES_OUT = 14 };
int mrl_simplecooked_create(const mrl_overcooked_config *cfg, int gpu_id, uint32_t num_worlds, mrl_sim **out);

/* ------------------------------------------------------------------ */
/* Hanabi  (reference: src/hanabi_env; 2 players, hand of 5)            */
/* ------------------------------------------------------------------ */

typedef struct mrl_hanabi_config {
    uint32_t colors, ranks, players, max_information_tokens, max_life_tokens;
} mrl_hanabi_config;

#define MRL_HANABI_OBS_SIZE 658   /* OBS_SIZE   sim.hpp:29 */
#define MRL_HANABI_STATE_SIZE 783 /* STATE_SIZE sim.hpp:30 */
#define MRL_HANABI_NUM_MOVES 20   /* NUM_MOVES  sim.hpp:19 */

/* Slots = ExportID (src/hanabi_env/sim.hpp:38-49); shapes as mgr.cpp:179-232:
 *   DONE int32 (N); ACTIVE_AGENT int32 (2,N); ACTION int32 (2,N,1);
 *   OBSERVATION int8 (2,N,658); ACTION_MASK int32 (2,N,20); REWARD float32 (2,N);
 *   WORLD_ID / AGENT_ID int32 (2,N); STATE int8 (2,N,783);
 *   OBSERVATION, STATE and ACTION_MASK are strided views (see the strides in the
 *   descriptor) into one array of 896-byte blocks [state 784 | mask 80 | pad 32],
 *   world-major with the two agents of a world back to back: one step writes whole
 *   cache lines only.  OBSERVATION is the first 658 bytes of the STATE row -- the same
 *   memory: the reference fills the state by copying the observation and appending the
 *   own hand (generateObsState, sim.cpp:367-379), so the two tensors agree on those
 *   bytes by construction, always (also for the agent whose buffers stay stale: both
 *   are refreshed together), and this engine writes them once.  For a configuration
 *   smaller than the full game (fewer colours / tokens) the observation has fewer than
 *   658 entries and OBSERVATION is exported exactly that wide, (2, N, obs_size): the row
 *   continues with the agent's own hand, which is hidden from the observer (the reference
 *   declares 658 entries whatever the configuration; its wrappers read [:obs_size],
 *   envs/hanabi_env.py:92-104).
 *   ACTION: only the entry of the agent to move is read, and EVERY int32 there has a defined result, the same in every code
 *   variant and on every step path; for every move of the table it is the reference's own (sim.cpp:596-792 applies the
 *   integer without a legality check):
 *     0..4 discard and 5..9 play that slot, 10..10+K-1 the colour hint, 10+K..10+K+R-1 the rank hint at the partner, whether
 *     or not ACTION_MASK allows the move (a hint that touches no card still costs its token; a discard at a full pool adds
 *     a token above the maximum, and the rows then shift as described in csrc/hanabi.hip, followed up to 5 tokens above it);
 *     any other value -- at or past 10 + K + R, or negative -- is read as uint32 and acts as the in-table rank hint
 *     10 + K + (u mod R) at the PARTNER, with u = uint32(action) - 10 - K; the remainder is exact over all of uint32.
 *     This is a DEPARTURE from the reference, whose rank-hint branch (sim.cpp:742-754) takes the same rank u % R but the
 *     player (actor + 1 + u / R) % 2, i.e. the mover's OWN hand when u / R is odd (actions 20..24 of the full game):
 *     following it there slowed the full game's step by 0.8 %, so the partner it is, everywhere.
 *     ACTION_MASK rows 10+K+R..19 stay zero.
 *   One move is outside the contract: a hint while the pool holds zero tokens.  The pool wraps to 255 as the reference's
 *   uint8_t does (the reference then writes far past its rows); what that world's rows hold from then on is unspecified,
 *   but every write stays inside that world's own record and rows, and no other world is affected.
 *   Slots at or past the hand size cannot occur: the player to move always holds five cards in the two-player game.
 *   int64 actions: mrl_step_with_actions_i64 is not available for Hanabi (MRL_ERR_INVALID, nothing changes); a caller
 *   narrows to int32 itself, and the low 32 bits it keeps are the action as above.
 *   GAME uint8 (N, 176): the raw per-world game record (tests only; layout in
 *   csrc/hanabi.hip); RESET_COUNT uint32 (1): worlds that finished in the last completed step (written by
 *   phase 2); SHARD_COUNT uint32 (1): worlds that finished in the last mrl_step_phase1 -- what the ranks of a
 *   sharded batch all-gather between the phases (mrl_step_phase2_gathered); mrl_step does not update it. */
enum {
    MRL_HANABI_DONE = 0,
    MRL_HANABI_ACTIVE_AGENT = 1,
    MRL_HANABI_ACTION = 2,
    MRL_HANABI_OBSERVATION = 3,
    MRL_HANABI_ACTION_MASK = 4,
    MRL_HANABI_REWARD = 5,
    MRL_HANABI_WORLD_ID = 6,
    MRL_HANABI_AGENT_ID = 7,
    MRL_HANABI_STATE = 8,
    MRL_HANABI_GAME = 9,
    MRL_HANABI_RESET_COUNT = 10,
    MRL_HANABI_SCAN_TIMEOUT = 11, /* uint32 (1): see mrl_step */
    MRL_HANABI_SHARD_COUNT = 12
};

int mrl_hanabi_create(const mrl_hanabi_config *cfg, int gpu_id, uint32_t num_worlds, mrl_sim **out);

/* ------------------------------------------------------------------ */
/* Cartpole  (reference: src/cartpole_env)                              */
/* ------------------------------------------------------------------ */

/* Slots = ExportID (src/cartpole_env/sim.hpp:17-24); shapes as mgr.cpp:174-202:
 *   RESET int32 (N,1); ACTION int32 (N,1); STATE float32 (N,4) (the Python
 *   binding calls it observation_tensor, bindings.cpp:28); REWARD float32 (N,1);
 *   WORLD_ID int32 (N,1); RESET_COUNT uint32 (1); SHARD_COUNT uint32 (1) (both as for Hanabi). */
enum {
    MRL_CARTPOLE_RESET = 0,
    MRL_CARTPOLE_ACTION = 1,
    MRL_CARTPOLE_STATE = 2,
    MRL_CARTPOLE_REWARD = 3,
    MRL_CARTPOLE_WORLD_ID = 4,
    MRL_CARTPOLE_RESET_COUNT = 5,
    MRL_CARTPOLE_SCAN_TIMEOUT = 6, /* uint32 (1): see mrl_step */
    MRL_CARTPOLE_SHARD_COUNT = 7
};

int mrl_cartpole_create(int gpu_id, uint32_t num_worlds, mrl_sim **out);

/* ------------------------------------------------------------------ */
/* Balance beam  (reference: src/balance_beam_env)                      */
/* ------------------------------------------------------------------ */

/* Slots = ExportID (src/balance_beam_env/sim.hpp:22-32); shapes as mgr.cpp:177-223:
 *   DONE int32 (N); ACTIVE_AGENT int32 (2,N) all ones; ACTION int32 (2,N,1), values 0..3 = moves -2,-1,+1,+2;
 *   OBSERVATION int32 (2,N,7) = own position history x[0..2], partner's x[3..5] (positions + 2), steps left;
 *   ACTION_MASK int32 (2,N,4) all ones; REWARD float32 (2,N); WORLD_ID / AGENT_ID int32 (2,N);
 *   RESET_COUNT uint32 (1); SHARD_COUNT uint32 (1) (both as for Hanabi).  The observation IS the world state (sim.cpp:99-112).  Episodes are numbered
 *   in ascending world order like Cartpole's; mrl_step = phase 1 + phase 2. */
enum {
    MRL_BALANCE_DONE = 0,
    MRL_BALANCE_ACTIVE_AGENT = 1,
    MRL_BALANCE_ACTION = 2,
    MRL_BALANCE_OBSERVATION = 3,
    MRL_BALANCE_ACTION_MASK = 4,
    MRL_BALANCE_REWARD = 5,
    MRL_BALANCE_WORLD_ID = 6,
    MRL_BALANCE_AGENT_ID = 7,
    MRL_BALANCE_RESET_COUNT = 8,
    MRL_BALANCE_SHARD_COUNT = 9
};

/* replaces BalanceBeamSimulator(exec_mode=CUDA, gpu_id, num_worlds) (src/balance_beam_env/bindings.cpp:10-24) */
int mrl_balance_create(int gpu_id, uint32_t num_worlds, mrl_sim **out);

/* ------------------------------------------------------------------ */
/* Acrobot  (reference: src/acrobat_env, its spelling of Acrobot-v1)    */
/* ------------------------------------------------------------------ */

/* Slots = ExportID (src/acrobat_env/sim.hpp:15-22); shapes as mgr.cpp's export calls:
 *   RESET int32 (N,1); ACTION int32 (N,1), values 0/1/2 = torque -1/0/+1 (sim.hpp:28-35); STATE float32 (N,4) =
 *   (theta1, theta2, omega1, omega2) (sim.hpp:37-49; the Python binding calls it observation_tensor); REWARD float32 (N,1);
 *   WORLD_ID int32 (N,1); RESET_COUNT uint32 (1); SCAN_TIMEOUT uint32 (1); SHARD_COUNT uint32 (1) (all three as for
 *   Cartpole); EPISODE_LENGTH int32 (N,1): steps of the world's current episode.
 * One step = one RK4 step of sim.cpp:68-94 over [0, 0.2] (sim.cpp:116-145), angles wrapped into [-pi, pi], velocities clamped
 *   to +-4 pi and +-9 pi (sim.cpp:180-183); RESET = (-cos theta1 - cos(theta1 + theta2) > 1) || (EPISODE_LENGTH > 500)
 *   (sim.cpp:189-200).  A finished world is re-seeded from its new episode's index, four draws mapped to -0.1 + r * 0.2
 *   (sim.cpp:45-66); world w starts as episode w and the counter at N; episodes are numbered in ascending world order.
 * REWARD is -1 after every step, the terminating one included: sim.hpp:51-53 promises 0 there, sim.cpp:186 never writes it, and
 *   the code is what is followed.  It is 0 before the first step.
 * EPISODE_LENGTH is kept PER WORLD.  The reference keeps one length in the EpisodeManager all worlds share (init.hpp:9;
 *   sim.cpp:52,169,199): every world increments it and any reset zeroes it, which is Acrobot-v1's truncation for N = 1 only (an
 *   untouched episode ends at its 501st step).  Here every world behaves as the reference's N = 1 world does.
 * mrl_rollout_random: action = (h * 3) >> 32 with the hash h of (seed, step, world, player 0) given there. */
enum {
    MRL_ACROBOT_RESET = 0,
    MRL_ACROBOT_ACTION = 1,
    MRL_ACROBOT_STATE = 2,
    MRL_ACROBOT_REWARD = 3,
    MRL_ACROBOT_WORLD_ID = 4,
    MRL_ACROBOT_RESET_COUNT = 5,
    MRL_ACROBOT_SCAN_TIMEOUT = 6, /* uint32 (1): see mrl_step */
    MRL_ACROBOT_SHARD_COUNT = 7,
    MRL_ACROBOT_EPISODE_LENGTH = 8
};
#define MRL_ACROBOT_MAX_STEPS 500 /* sim.cpp:199 */

/* replaces AcrobatSimulator(exec_mode=CUDA, gpu_id, num_worlds) (src/acrobat_env/bindings.cpp) */
int mrl_acrobot_create(int gpu_id, uint32_t num_worlds, mrl_sim **out);

/* ------------------------------------------------------------------ */
/* Common                                                               */
/* ------------------------------------------------------------------ */

/* One environment step for every world: replaces Manager::step.
 * Hanabi, Cartpole and the balance beam number new episodes in ascending world order, which
 * takes a prefix sum over the worlds that finished.  Where the kernel exists (Cartpole up to 4 M
 * worlds, Hanabi up to 262144) mrl_step is ONE launch: every workgroup publishes its count of
 * finishing worlds and one of its waves looks back at the lower workgroups' counts while the others
 * already stream out results.  The look-back never depends on another workgroup making progress: a
 * count that has not appeared after a short bounded wait is recounted by the waiting wave from that
 * workgroup's inputs (csrc/episode_scan.hpp), so no dispatch order or co-residency is assumed.
 * Otherwise, for the sharded path and under mrl_debug_set("fused_step", 2), it is two launches
 * (phase 1, phase 2: the kernel boundary is the grid-wide hand-off).  The persistent multi-step
 * launches of mrl_rollout_random DO wait for other workgroups inside the kernel; they need all
 * their workgroups resident and are therefore launched cooperatively.  Those waits are
 * bounded; if one ever expired the SCAN_TIMEOUT tensor of the game becomes nonzero, the
 * episode numbers from that step on are unspecified, and every later mrl_step* /
 * mrl_rollout_random on the simulator returns MRL_ERR_DEVICE (the host learns it from a
 * word in mapped host memory: no device call, no sync). */
int mrl_step(mrl_sim *sim, void *hip_stream);

/* HIP graphs.  Every mrl_step* / mrl_rollout_random / mrl_step_sequence only enqueues kernels on the stream it is given, so
 * Overcooked and Simplecooked calls can be captured (hipStreamBeginCapture, torch.cuda.graph) and replayed as they are.
 * Hanabi, Cartpole and the balance beam keep launch-to-launch state on the host by default (which half of the
 * double-buffered episode counter is current, the epoch of the single-launch step's look-back) and pass it in kernel
 * arguments; captured as such, a replay would run with stale values, so those calls return MRL_ERR_INVALID while the stream
 * is capturing.  mrl_prepare_graph_capture(sim, stream) -- called once, OUTSIDE a capture; it synchronises the stream --
 * moves that state into device memory for the rest of the simulator's life: every step then enqueues a one-thread launch
 * that advances it in front of its kernels, which read it from there, and captured steps replay correctly (a replay of K
 * captured steps is K more steps).  The price is that extra launch per step (~2 us of GPU time), also outside graphs, and
 * mrl_rollout_random runs one launch per step on such a simulator (its persistent form is a cooperative launch, which
 * cannot be captured).  No-op for Overcooked and Simplecooked. */
int mrl_prepare_graph_capture(mrl_sim *sim, void *hip_stream);

/* Launch shape of the simulator's step kernel: out = {workgroups, threads per workgroup, LDS bytes per
 * workgroup, worlds per wavefront (0 where that is not how the game is mapped)}.  For DESIGN.md's
 * occupancy arithmetic and the tests that guard it; no reference counterpart. */
int mrl_launch_shape(const mrl_sim *sim, uint32_t out[4]);

/* 1 if an in-kernel wait of an earlier call expired (see mrl_step), else 0.  Reads host memory only. */
int mrl_scan_timed_out(const mrl_sim *sim);

/* Same step, but actions are read from caller memory instead of the ACTION
 * tensor (same dtype/shape/layout, device pointer).  Saves the copy the
 * reference wrappers make (static_actions.copy_, envs/overcooked_env.py:107). */
int mrl_step_with_actions(mrl_sim *sim, const int32_t *actions_dev, void *hip_stream);

/* Several simulators stepped by ONE launch: any mix of Overcooked layouts, sizes, player counts and world counts on one device
 * (the reference's Config holds a single terrain, src/overcooked_env/sim.hpp:44-57, so a curriculum over several layouts is
 * several simulators there, each with a step call of its own).  The grid is the concatenation of the simulators' grids and
 * every workgroup runs its simulator's step on that simulator's parameters, which travel in the kernel arguments.  Same
 * results as one mrl_step_with_actions per simulator (actions_dev_or_null == NULL or an entry NULL: that simulator's
 * ACTION tensor).  At most 8 simulators per call; the generic step kernel is used, so large single-layout batches are
 * better off with their own, specialised launch -- this is for many small sub-batches, where the launches are what
 * costs.  Overcooked only (MRL_ERR_INVALID otherwise, and for the few-worlds-of-a-large-layout configurations whose
 * workgroups share one state copy). */
int mrl_step_many(mrl_sim *const *sims, uint32_t count, const int32_t *const *actions_dev_or_null, void *hip_stream);

/* The same with the caller's actions as int64 (same shape and layout): what the reference's harness hands
 * `env.n_step` (scripts/overcooked_example.py:99-106: `torch.randint_like` of a long tensor), which the reference
 * wrapper narrows with a gather + copy kernel per step (envs/overcooked_env.py:104-107).  Here the step kernel reads
 * the 8-byte values itself and mirrors them into the ACTION tensor, so the wrapped step is one launch.  Overcooked and
 * Simplecooked; MRL_ERR_INVALID for the other games. */
int mrl_step_with_actions_i64(mrl_sim *sim, const int64_t *actions_dev, void *hip_stream);

/* Two-phase step for world batches sharded over several GPUs (Hanabi and
 * Cartpole draw each new episode's seed from one global counter,
 * src/hanabi_env/sim.cpp:449-451, src/cartpole_env/sim.cpp:51-53):
 *   phase 1 = transition + termination test, leaves the number of finishing
 *             worlds of this shard in SHARD_COUNT (a one-workgroup launch behind the
 *             step kernel that adds up its per-workgroup counts);
 *   phase 2 = re-seed and reset the finishing worlds, taking episode indices
 *             episode_base, episode_base+1, ... in ascending world order.
 * episode_base_dev is a device pointer to one uint32 (the caller computes it
 * from the gathered RESET_COUNTs of the lower ranks without a host sync);
 * NULL means "use and advance the simulator's own counter" (single GPU).
 * mrl_step gives the same results as phase 1 + phase 2(NULL).  Overcooked has no episode counter:
 * phase 1 is the whole step and phase 2 is a no-op. */
int mrl_step_phase1(mrl_sim *sim, const int32_t *actions_dev_or_null, void *hip_stream);
int mrl_step_phase2(mrl_sim *sim, const uint32_t *episode_base_dev, void *hip_stream);

/* Phase 2 for rank `rank` of `num_ranks` (1..1024) with the exchange left on the device: counts_dev holds the
 * SHARD_COUNT word of every rank for this step, in rank order -- exactly what one all-gather of the SHARD_COUNT
 * tensors delivers.  The re-seeding launch itself adds the lower ranks' counts to the simulator's own episode
 * counter to get its base and advances that counter by the sum over all ranks, so a sharded step is
 * phase 1 -> all-gather of one word per rank -> this call, with no other device work in between and no host
 * sync.  The counter must have been set by mrl_reseed_shard.  No-op for games without an episode counter. */
int mrl_step_phase2_gathered(mrl_sim *sim, const uint32_t *counts_dev, uint32_t num_ranks, uint32_t rank, void *hip_stream);

/* The same exchange WITHOUT a collective (round 4): a device-side mailbox.  Every rank owns a small block of device memory;
 * mrl_exchange_create allocates it for this rank of `num_ranks` (<= MRL_MAX_RANKS) and returns its IPC handle
 * (MRL_IPC_HANDLE_BYTES bytes, hipIpcGetMemHandle); the caller gives every rank the handles of all ranks, in rank order (one
 * all-gather of 64 bytes at set-up), and mrl_exchange_connect maps the peers' blocks (hipIpcOpenMemHandle).  From then on
 *     mrl_step_exchanged(sim, actions_or_null, stream)
 * is one whole step of the shard: phase 1; a one-workgroup launch that adds up the shard's finished worlds and stores
 * (step tag, count) into word `rank` of every rank's mailbox -- num_ranks stores over xGMI --; phase 2, whose
 * workgroups poll the num_ranks words of their own mailbox for this step's tag and number the episodes as
 * mrl_step_phase2_gathered does.  No host call and no collective between the launches, so a captured or free-running
 * loop needs no rendezvous; every rank must call it the same number of times (a rank that never publishes leaves the others'
 * phase 2 polling until the bounded wait expires: SCAN_TIMEOUT, as for the persistent rollouts).  One process per rank (a
 * rank's own handle is not opened).  Reference: one process-wide atomic, src/hanabi_env/sim.cpp:449-451. */
#define MRL_MAX_RANKS 16
#define MRL_IPC_HANDLE_BYTES 64
int mrl_exchange_create(mrl_sim *sim, uint32_t num_ranks, uint32_t rank, uint8_t *ipc_handle_out);
int mrl_exchange_connect(mrl_sim *sim, const uint8_t *ipc_handles_of_all_ranks);
int mrl_step_exchanged(mrl_sim *sim, const int32_t *actions_dev_or_null, void *hip_stream);

/* Rollout-buffer side of a trainer.  The reference's MAPPO loop clones the observation
 * and state tensors after every step and copies them into the buffer slot of that step
 * (train/MAPPO/main_player.py:245-247, utils/shared_buffer.py:115 chooseinsert).  Here the caller hands the step the
 * slot instead: from this call on every mrl_step* / mrl_rollout_random / mrl_step_sequence of the simulator writes
 * its observation slab -- int8 (N, P, H, W, F), the OBS_WORLD_MAJOR layout, `bytes` = N*P*H*W*F -- to obs_dev_or_null
 * and leaves the OBSERVATION / OBS_WORLD_MAJOR tensors untouched; NULL hands the output back to them.  Same bytes, same
 * stores, no copy: the kernels take the slab's address from their launch arguments and never read it back.  The
 * buffer must stay valid until the work enqueued before the next call of this function has finished.  A buffer that
 * starts on a 16-byte boundary costs nothing; one that does not (slot k of a dense (T, N, P, H, W, F) buffer whose
 * N*P*H*W*F is not a multiple of 16) is accepted too and STAGED: the kernels stream 16-byte chunks from an aligned base,
 * so the step writes a slab of the simulator's own (allocated at the first such call; the exported tensors stay
 * untouched) and one device-to-device copy behind the launch, on the same stream, moves it to the slot -- one more
 * pass over the slab per step.  Overcooked and Simplecooked (MRL_ERR_INVALID for the other games).  Host-only call
 * (but for that allocation): nothing is enqueued. */
int mrl_set_observation_output(mrl_sim *sim, void *obs_dev_or_null, uint64_t bytes);

/* The same for a whole rollout buffer: a ring of num_slots observation slots, slot s at base + s * slot_stride_bytes
 * (>= N*P*H*W*F; with base and stride multiples of 16 the slots are written in place, otherwise they are staged as
 * above and the multi-step launches run one launch + one copy per step).  Step number k counted from this call -- whether it is a launch of its own or step k of a
 * multi-step launch (mrl_rollout_random, mrl_step_sequence: the kernel moves on to the next slot itself) -- writes its
 * observations to slot k % num_slots.  One mrl_rollout_random(sim, T, ...) then fills a T-slot buffer with T steps of
 * random-policy experience in one launch.  base == NULL hands the output back to the simulator's own tensor; one slot is
 * mrl_set_observation_output.  The count lives on the host: a launch captured in a HIP graph keeps the slot(s) it was
 * captured with.  Overcooked and Simplecooked. */
int mrl_set_observation_ring(mrl_sim *sim, void *base_dev_or_null, uint64_t slot_stride_bytes, uint32_t num_slots);

/* Sets the simulator's own episode counter (next index handed out). Sharded
 * runs call it once after create with the global world offset semantics the
 * caller wants; it does not touch world state. */
int mrl_set_episode_counter(mrl_sim *sim, uint32_t next_episode, void *hip_stream);

/* Re-initialises world i of this shard as global world (world_offset + i) of a
 * num_worlds_total batch: episode index world_offset + i, counter starts at
 * num_worlds_total -- what a single simulator of the whole batch would hold
 * after construction.  No-op for Overcooked (its initial state is not seeded). */
int mrl_reseed_shard(mrl_sim *sim, uint32_t world_offset, uint32_t num_worlds_total, void *hip_stream);

/* num_steps steps driven by an open-loop action array: actions_dev holds num_steps consecutive
 * ACTION tensors (step k at offset k * elements(ACTION), same dtype and layout, device pointer).
 * Same results as num_steps calls of mrl_step_with_actions.  Overcooked layouts whose observation
 * slab fits the LDS tile run them in ONE launch with the worlds' state resident in LDS (every
 * step still writes its observations, rewards and dones); everything else is one launch per step. */
int mrl_step_sequence(mrl_sim *sim, const int32_t *actions_dev, uint32_t num_steps, void *hip_stream);

/* The random policies of the reference's benchmark harnesses, drawn on the device
 * (SURVEY.md section 8f item 1): num_steps environment steps with no action tensor to fill.
 *   Overcooked  randint(high=6) per agent            scripts/overcooked_example.py:99-106
 *   Cartpole    randint(high=2)                      scripts/cartpole_example.py:53-87
 *   Simplecooked randint(high=6) per agent; Balance beam randint(high=4) per agent (their example scripts)
 *   Acrobot     randint(high=3)                      (the reference ships no example script for it)
 *   Hanabi      argmax(rand * mask), i.e. a uniformly random legal move of the player
 *               to move                              scripts/hanabi_example.py:53-82
 * All draws come from one counter-based hash of (seed, step index k = first_step,
 * first_step+1, ..., world w, player q), so a stream can be replayed through mrl_step:
 *     h = lo32(seed) ^ k*0x9E3779B9 ^ w*0x85EBCA6B ^ (q+1)*0xC2B2AE35 ^ hi32(seed)*0x27D4EB2F
 *     h ^= h>>16; h *= 0x7FEB352D; h ^= h>>15; h *= 0x846CA68B; h ^= h>>16;   (all mod 2^32)
 *   Overcooked  action = (h * 6) >> 32
 *   Cartpole    action = h >> 31                      (q = 0)
 *   Acrobot     action = (h * 3) >> 32                (q = 0); one launch per step
 *   Hanabi      action = position of the j-th set bit of the mover's 20-bit legal-move
 *               mask, j = (h * popcount(mask)) >> 32  (q = the mover)
 * Every step writes its outputs exactly like mrl_step; afterwards the ACTION tensor holds
 * the last step's draws (Hanabi: the mover's entry).  Overcooked layouts whose observation
 * slab fits the LDS tile, and Hanabi / Cartpole batches whose workgroups all fit the GPU at
 * once (65536 Hanabi worlds, 1 M Cartpole worlds do), run all num_steps in ONE launch with
 * the worlds' state resident in LDS / registers; otherwise it is one launch per step. */
int mrl_rollout_random(mrl_sim *sim, uint32_t num_steps, uint64_t seed, uint32_t first_step, void *hip_stream);

/* Restart the worlds whose byte in mask_dev is nonzero (device pointer, N bytes; NULL = every world) as fresh
 * episodes, now, on hip_stream.  No reference counterpart (the reference restarts a world only when its episode ends
 * inside a step); EnvPool's reset(env_ids) is the same call.
 *   What a reset world becomes: world i is bit-identical to world 0 of a newly built simulator of the same configuration
 *     whose first episode has the index world i receives -- observations, Hanabi STATE / ACTION_MASK / ACTIVE_AGENT /
 *     GAME, the Overcooked STATE_* tensors (and Simplecooked's STATE_DISHES_OUT), Cartpole STATE, Acrobot STATE
 *     with EPISODE_LENGTH 0.  Overcooked and
 *     Simplecooked have no episode index: timestep 0, no objects, players on their start cells facing north, empty hands.
 *   Numbering (Hanabi, Cartpole, balance beam, Acrobot): the reset worlds take the episode indices counter, counter + 1, ... in
 *     ascending world order and the counter advances by their number; later episode ends go on from there exactly as if
 *     those worlds had finished in a step.  The call is the two-launch step's phase 2 run on the mask: it follows the
 *     same double-buffered counter (host mode, or the device-side state after mrl_prepare_graph_capture).
 *   Untouched: worlds outside the mask, in every tensor, and every per-step output -- DONE / RESET, REWARD, ACTION,
 *     RESET_COUNT, SHARD_COUNT, SCAN_TIMEOUT.  A mask with no byte set changes nothing, the counter included.
 *   Overcooked / Simplecooked observations go where the most recent step wrote: the simulator's tensor, the slot of
 *     mrl_set_observation_output, or ring slot (k - 1) mod T; where no step has run since that destination was set, where
 *     the next step will write.  A STAGED destination (off a 16-byte boundary) is refused with MRL_ERR_INVALID.
 *   Refused with MRL_ERR_INVALID: a Hanabi, Cartpole, balance-beam or Acrobot simulator that has been through mrl_reseed_shard or
 *     mrl_exchange_create (numbering across ranks would need an exchange between them); a capturing stream wherever
 *     mrl_step refuses one (a reset captured after mrl_prepare_graph_capture replays correctly); a NULL handle.
 *   It only enqueues work: no host synchronisation.  Every later mrl_step*, mrl_step_many, mrl_step_sequence,
 *   mrl_rollout_random and graph replay continues from the reset state.  The caller keeps mask_dev valid until the work
 *   has run.  Cost: one small launch that turns the mask into per-workgroup counts plus the re-seeding launch (counter
 *   games); one launch with a wavefront per world that copies the fresh world over the masked ones (Overcooked,
 *   Simplecooked).  DESIGN.md section 9. */
int mrl_reset_worlds(mrl_sim *sim, const uint8_t *mask_dev_or_null, void *hip_stream);

/* Episode returns and lengths as a product of the step.  The reference's training scripts keep them by hand, in torch, after
 * every step (scripts/cartpole_train_torch.py:223-226: ep_rewards += rewards; rewsum += sum(where(done, ep_rewards, 0));
 * numfin += sum(done); ep_rewards *= 1 - done -- six or seven launches around a step of a few microseconds), and its
 * environments never delivered the info["episode"] the commented-out lines beneath ask for.  No reference counterpart.
 *   mrl_enable_episode_stats allocates and zeroes five tensors, for the rest of the simulator's life (like
 *   mrl_prepare_graph_capture); a second call is a no-op.  MRL_ERR_INVALID for a NULL handle and on a capturing stream (the
 *   call allocates; it also synchronises the stream).  The memory is an allocation of its own: no exported tensor moves.
 *   Before the call the five slots answer MRL_ERR_SLOT and every entry point enqueues exactly what it did before.
 * Slots, the same numbers for all six games.  P = players; REWARD's and DONE's own shapes are (P,N) / (N), or (N,1) / (N,1):
 *   EPISODE_RETURN float32, REWARD's shape   sum of REWARD over the steps of the world's current episode since enabling
 *   EPISODE_STEPS  int32,   DONE's shape     steps of the current episode since enabling
 *   LAST_RETURN    float32, REWARD's shape   EPISODE_RETURN as it stood when the world last finished (0 before)
 *   LAST_STEPS     int32,   DONE's shape     the same for EPISODE_STEPS
 *   TOTALS         float64 (B, 2 + P), B = ceil(N / 1024): per block b of worlds [1024 b, 1024 b + 1024), since the last
 *                  mrl_clear_episode_totals: episodes finished, their steps, their return per player.  The totals
 *                  themselves are the column sums.
 * After every completed step, for every world w:
 *     ret[:, w] += float32(REWARD[:, w]);  steps[w] += 1                 (one IEEE float32 add per step and player)
 *     if DONE[w]:  last_ret[:, w] = ret[:, w];  last_steps[w] = steps[w]
 *                  TOTALS[w / 1024] += (1, steps[w], ret[:, w]);  ret[:, w] = 0;  steps[w] = 0
 * TOTALS takes no atomics: block b is read and written by exactly one workgroup of a launch, which sums what its finished
 * worlds contribute in a fixed order and touches the block only if one of its worlds finished -- the same bits from run to
 * run, and no 1024 workgroups queueing on one word.
 * A completed step is: mrl_step; mrl_step_with_actions and its _i64 form; every simulator of an mrl_step_many that has the
 * statistics enabled; mrl_step_exchanged; each step of mrl_step_sequence and mrl_rollout_random; of the two-phase calls,
 * phase 2 in any of its forms (Hanabi, Cartpole, balance beam, Acrobot) or phase 1 (Overcooked, Simplecooked, whose phase 2
 * does nothing); every replay of a captured step.  The update is one more launch behind the step's own
 * (mrl_episode_stats_update, 256 threads x 4 worlds), on the same stream; with statistics enabled mrl_step_sequence and
 * mrl_rollout_random run one step per launch, each followed by it (K steps equal K single calls either way), and
 * mrl_rollout_kernel_name says so.
 * mrl_reset_worlds zeroes EPISODE_RETURN / EPISODE_STEPS of the masked worlds and nothing else of these tensors -- a forced
 * restart is not a finished episode --, mrl_reseed_shard does the same for all worlds, mrl_clear_episode_totals zeroes TOTALS
 * only (MRL_ERR_INVALID before mrl_enable_episode_stats).  Totals are per simulator: a sharded batch adds its ranks' up. */
enum {
    MRL_STATS_EPISODE_RETURN = 64,
    MRL_STATS_EPISODE_STEPS = 65,
    MRL_STATS_LAST_RETURN = 66,
    MRL_STATS_LAST_STEPS = 67,
    MRL_STATS_TOTALS = 68
};
int mrl_enable_episode_stats(mrl_sim *sim, void *hip_stream);
int mrl_clear_episode_totals(mrl_sim *sim, void *hip_stream);

/* Policy rollouts on the device: the collection phase of PPO for Cartpole and Acrobot, and for the single-agent trainer of
 * the balance beam (its own paragraph below).  The reference's trainer runs, per
 * step, two three-layer tanh MLPs (scripts/cartpole_train_torch.py:105-131, Agent), a Categorical sample, a log_prob and six
 * buffer row copies in torch around the step (:204-218), then T sequential torch iterations for the advantages (:243-256).
 * Here the first is ONE launch per step in front of the simulator's ordinary step (mrl_policy_act) and the second one launch
 * (mrl_gae).  No reference counterpart as a call.
 *   Policy: critic and actor are Linear(D, 64), tanh, Linear(64, 64), tanh, Linear(64, 1 or A).  params_dev is one flat float32
 *     device array in the order of torch.nn.utils.parameters_to_vector(agent.parameters()) for that Agent: critic.0.weight
 *     (64, D) row-major, critic.0.bias, critic.2.weight, critic.2.bias, critic.4.weight, critic.4.bias, then actor.0 ... actor.4;
 *     mrl_mlp_policy_num_params floats.  The kernel reads it in place in every launch: between rollouts a trainer does its
 *     optimizer step and one flat copy.  hidden must be 64; num_actions 2 (Cartpole), 3 (Acrobot) or 4 (the beam).
 *   Observation: MRL_OBS_RAW, D = 4, is the STATE row; MRL_OBS_ACROBOT_GYM, D = 6, Acrobot only, is Gym's
 *     [cos theta1, sin theta1, cos theta2, sin theta2, omega1, omega2] computed from it.
 *     MRL_OBS_BALANCE, D = 7, the balance beam only, is seat 0's int32 OBSERVATION row as floats (below).
 *   Buffers: dense device arrays, T = num_steps; obs / next_obs start on a 16-byte (D = 4), 8-byte (D = 6) or 4-byte (D = 7)
 *     boundary.
 *   Row k < T, world w, from the tensors as they stand in front of step k of the call:
 *     obs[k,w,:] the observation; dones[k,w] = RESET[w] != 0 as 0.0 / 1.0 -- the previous step's flag, like `dones[step] =
 *     next_done` (:207) --; values[k,w] the critic; actions[k,w] the draw, also written to ACTION[w]; logprobs[k,w]; and for
 *     k > 0 rewards[k-1,w] = REWARD[w].  Then the step runs.  The closing launch (k = T) writes rewards[T-1], next_obs,
 *     next_done and next_value (:244) and draws nothing.  num_steps == 0 writes the next_* arrays only.
 *   Sampling, replayable on the host like mrl_rollout_random: h = the hash given there of (seed, first_step + k, w, player 0);
 *     u = (h >> 8) * 2^-24 (exact in float32); m = max logit; e_a = exp(l_a - m); p_a = e_a / sum e; action = the number of a in
 *     0..A-2 with u >= p_0 + ... + p_a; logprob = (l_action - m) - log(sum e); all in float32.  With MRL_POLICY_GREEDY in
 *     flags the action is the first arg-max of the logits (evaluation); logprob is written all the same.
 *   Arithmetic: every dot product starts from the bias and adds the inputs in ascending order with fused multiply-adds.
 * mrl_rollout_policy enqueues T x (act, step) + the closing act and never synchronises: two launches per step (plus the
 *   statistics update after mrl_enable_episode_stats, plus the advance launch after mrl_prepare_graph_capture).  The step is
 *   mrl_step reading the ACTION tensor, so the call equals, row for row, T times "act on the current state, mrl_step", and
 *   afterwards the simulator is exactly where T mrl_step_with_actions calls with actions[0..T-1] would have left it (and its
 *   ACTION tensor holds actions[T-1]): episode numbering, statistics and SCAN_TIMEOUT behave as there.
 *   MRL_ERR_INVALID: a game other than Cartpole, Acrobot or the balance beam (below); hidden != 64; num_actions other than the game's; an (obs_dim,
 *   obs_mode) other than (4, RAW) or, for Acrobot, (6, ACROBOT_GYM); any NULL pointer; a misaligned obs / next_obs; a capturing
 *   stream wherever mrl_step refuses one; a simulator that has been through mrl_exchange_create.  Capturing a rollout in a HIP
 *   graph is not supported in any mode: the row index travels in kernel arguments.
 *   The balance beam (scripts/balance_train_single.py: the same agent, 7 -> 64 -> 64 -> {4, 1}, as the ego of a two-seat game
 *   whose partner moves uniformly at random): hidden 64, obs_dim 7, num_actions 4, MRL_OBS_BALANCE.  Per world w the launch
 *   reads x = OBSERVATION[0,w,0..6] (int32 values 0..8 and 0..2, exact as floats) and writes obs[k,w,:] = x, dones[k,w] =
 *   DONE[w] != 0, rewards[k-1,w] = REWARD[0,w] (the ego's, as VectorMultiAgentEnv.step returns it), values, actions and
 *   logprobs as above, the ego's action also to ACTION[0,w,0] -- and, in the same launch, the partner's move ACTION[1,w,0] =
 *   (h1 * 4) >> 32 with h1 the hash of (seed, first_step + k, w, player 1): mrl_rollout_random's draw for that seat.  The
 *   closing launch draws nothing and leaves both seats' ACTION alone; MRL_POLICY_GREEDY changes the ego's choice only.
 *   Afterwards the simulator is where T mrl_step_with_actions calls with [actions[k], those partner moves] would have left it,
 *   and ACTION holds the last row of both seats.  MRL_ERR_INVALID for any other shape or mode on a beam, MRL_OBS_BALANCE on
 *   another game, a beam that has been through mrl_exchange_create, and a capturing stream in every mode.  A caller-supplied or
 *   learned partner is what mrl_rollout_mlpbase and the banks are for.  The other games are out of scope.  DESIGN.md section 25.
 *   A bank of policies (K seeds of one agent on one batch): policy->num_members = K > 0.  The field lies in
 *   what used to be the struct's four bytes of tail padding, so sizeof and every other offset are what they were, and 0 -- what
 *   every caller that zero-fills the struct passes -- is the behaviour above, bit for bit.  With K > 0 the simulator's N worlds
 *   are K members of W = N / K worlds: member k owns worlds [k W, (k + 1) W) and acts under the parameters that start k P floats
 *   behind params_dev, P = mrl_mlp_policy_num_params.  The bank is DENSE, there is no stride; P is odd for (4, 2) and (7, 4), 9155 and
 *   9669, so a row is only 4-byte aligned, which is all the kernel asks of any shape.  One launch per step serves all members ((ceil(W / 64), nets,
 *   K) workgroups).  Contract: for every world w of member k, every cell the call writes -- obs, dones, values, actions,
 *   logprobs, rewards, next_obs, next_value, next_done, ACTION[w] and on the beam ACTION[1,w] -- is bit for bit what the plain
 *   mrl_rollout_policy writes for world w under policy k alone on the same simulator state.  The draws are those of world w IN THE
 *   BATCH OF N (the hash of (seed, first_step + k, w, player) with w = k W + j), and the episode numbers are the batch's: they are
 *   not those of a simulator that holds the member's W worlds alone.  Everything the plain call refuses is refused in the same
 *   words; then, MRL_ERR_INVALID: K > 65535 (the member travels in the launch grid's third dimension), K > N, and N % K != 0.
 * mrl_gae is lines 247-256 with a lane per world, t = T-1 ... 0 in float32, one IEEE operation per operation of the script:
 *     nnt = 1 - (t == T-1 ? next_done[w] : dones[t+1,w]);  nv = t == T-1 ? next_value[w] : values[t+1,w]
 *     delta = rewards[t,w] + gamma * nv * nnt - values[t,w]
 *     advantages[t,w] = last = delta + gl * nnt * last;  returns[t,w] = advantages[t,w] + values[t,w]
 *   with gl = float32(double(gamma) * double(lambda)) (the script multiplies the two Python floats first).  All arrays (T, N)
 *   dense on device gpu_id, next_* (N); it only enqueues.  MRL_ERR_INVALID for a NULL array.  DESIGN.md section 12. */
enum { MRL_OBS_RAW = 0, MRL_OBS_ACROBOT_GYM = 1, MRL_OBS_BALANCE = 2 };
enum { MRL_POLICY_GREEDY = 1 };
typedef struct mrl_mlp_policy {
    const float *params_dev;
    uint32_t obs_dim, hidden, num_actions, obs_mode, flags;
    uint32_t num_members; /* 0: one policy.  K > 0: a bank, params_dev is (K, P) dense (below).  In what was tail padding. */
} mrl_mlp_policy;
typedef struct mrl_rollout_buffers { /* all device pointers, dense, T = num_steps */
    float *obs;                      /* (T, N, D) */
    int32_t *actions;                /* (T, N) */
    float *logprobs, *values, *rewards, *dones; /* (T, N) */
    float *next_obs;                 /* (N, D) */
    float *next_value, *next_done;   /* (N) */
    uint32_t num_steps;
} mrl_rollout_buffers;
uint64_t mrl_mlp_policy_num_params(uint32_t obs_dim, uint32_t hidden, uint32_t num_actions);
int mrl_rollout_policy(mrl_sim *sim, const mrl_mlp_policy *policy, const mrl_rollout_buffers *buffers, uint64_t seed,
                       uint32_t first_step, void *hip_stream);
int mrl_gae(const float *rewards, const float *values, const float *dones, const float *next_value, const float *next_done,
            uint32_t num_steps, uint32_t num_worlds, float gamma, float lambda, float *advantages, float *returns, int gpu_id,
            void *hip_stream);

/* The update phase of PPO on the device: scripts/cartpole_train_torch.py:275-315 -- gather, both forward passes, the clipped
 * losses, backward, clip_grad_norm_ and Adam.step() -- for the same actor-critic, on the flat parameter array the rollout
 * kernel reads.  That array is the only copy of the weights; it is updated in place.  No reference counterpart as a call.
 *   One call is K = num_minibatches steps in row order: row k gathers the B = minibatch_size samples indices[k, :] of the
 *     batch (the script's b_* arrays, :259-264, S = T * N samples) and takes one Adam step.  A trainer passes the E * M rows of
 *     its shuffles (:269-273); one that wants target_kl (:317-319) passes one epoch's rows per call and reads the stats.
 *   Per sample, in float32, with c = clip_coef: logp = log_softmax(actor(x)); newlogprob = logp[a]; ratio = exp(newlogprob -
 *     old); A = (adv - mean) / (std + 1e-8) over the row with MRL_PPO_NORM_ADV (torch's unbiased std), else adv; pg = max(-A
 *     ratio, -A clamp(ratio, 1 - c, 1 + c)); with MRL_PPO_CLIP_VLOSS v_loss = 0.5 max((v - R)^2, (v_old + clamp(v - v_old, -c, c)
 *     - R)^2), else 0.5 (v - R)^2; loss = mean(pg) - ent_coef mean(H) + vf_coef mean(v_loss).  The gradient is torch
 *     autograd's for those lines (a tie of the two arguments of a max halves the gradient between them, as torch.max does).
 *   Clipping: total = sqrt(sum g^2); g *= min(1, max_grad_norm / (total + 1e-6)); none for max_grad_norm <= 0.
 *   Adam (torch.optim.Adam, single tensor, no amsgrad, no weight decay), t = opt->step + 1 + k: m = beta1 m + (1 - beta1) g;
 *     v = beta2 v + (1 - beta2) g^2; p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps); the two scalars are
 *     formed in double on the host, as torch forms them in Python floats.  The caller adds K to its step count afterwards.
 *   stats (K, 8), optional: 0 pg_loss, 1 v_loss (the 0.5 mean, as the script logs it), 2 entropy, 3 old_approx_kl, 4 approx_kl,
 *     5 clipfrac, 6 total_norm before clipping, 7 loss.  grads (K, P), optional, P = mrl_mlp_policy_num_params: every row's
 *     summed, unclipped gradient in parameter order (tests and diagnostics).
 *   The call only enqueues on hip_stream of device gpu_id: it never synchronises or allocates.  Scratch is the caller's,
 *     mrl_ppo_workspace_bytes (a pure host function) says how much; it need not be cleared and holds nothing between calls.
 *     Launches: one for the rows' advantage statistics (MRL_PPO_NORM_ADV only) and three per row (gradient; sum of the
 *     workgroups' partial vectors and of g^2; clip, Adam and stats).  No float atomics, no wait between workgroups: the
 *     same inputs give the same bits on every run, and one call of K rows the same bits as K calls of one row.
 *   Index values (0 <= indices[k, b] < batch->size) are the caller's duty: there is no device-side check to synchronise on.
 *   shape->params_dev, obs_mode and flags are not read (the parameters are opt->params_dev; obs holds observations).
 *   MRL_ERR_INVALID: a NULL among shape, opt, batch, indices, cfg, workspace, the optimizer's three arrays and the batch's six;
 *     hidden != 64; (obs_dim, num_actions) other than (4, 2), (4, 3), (6, 3) and the balance beam's (7, 4); minibatch_size < 2
 *     with MRL_PPO_NORM_ADV; minibatch_size == 0 or batch->size == 0; workspace_bytes below mrl_ppo_workspace_bytes; obs off a
 *     16-byte (D = 4), 8-byte (D = 6) or 4-byte (D = 7: rows of 28 bytes, loaded float by float) boundary or workspace off a
 *     16-byte one; a capturing stream (the step number travels in kernel arguments).  num_minibatches == 0 enqueues nothing.
 *     mrl_ppo_workspace_bytes refuses the same shapes and a NULL out.  The words of a shape refusal: a call with neither
 *     obs_dim 7 nor num_actions 4 is told "(4, 2), (4, 3), (6, 3)", the float-state games' shapes, as before the beam had one;
 *     a call with either is told all four.  DESIGN.md sections 13 and 25.
 *   A bank update: opt->num_members = M > 0, a field in what used to be the struct's tail padding; 0 is the
 *     call above, bit for bit.  opt->params_dev, exp_avg and exp_avg_sq point at the first trained member's row and M dense rows
 *     of P floats follow in each (a caller trains members first .. first + M - 1 of a bank by offsetting the three pointers; P is
 *     odd for (4, 2) and (7, 4), so a row is only 4-byte aligned).  indices is (M, K, B), stats (M, K, 8), grads (M, K, P); the workspace is M times
 *     mrl_ppo_workspace_bytes and member m uses slice m.  The batch, the configuration -- learning rate, betas, loss options -- and
 *     step are shared by all members.  The launches are those of the plain call with the member in the grid's third dimension:
 *     1 + 3 K whatever M is.  Contract: for every trained member the parameter row, both moment rows, the stats and the grads are
 *     bit for bit what the plain mrl_ppo_update leaves for that member alone with indices[m] on the same batch; rows of the bank
 *     that are not trained keep every bit; one call of K rows equals K calls of one row.  MRL_ERR_INVALID, after the checks above
 *     in their order: M > 65535; the workspace refusal asks for M times the plain size.  mrl_agent_update, which takes the same
 *     struct, refuses num_members != 0. */
enum { MRL_PPO_NORM_ADV = 1, MRL_PPO_CLIP_VLOSS = 2 };
typedef struct mrl_ppo_config {
    float clip_coef, ent_coef, vf_coef, max_grad_norm; /* max_grad_norm <= 0: no clipping */
    float lr, beta1, beta2, eps;                        /* torch.optim.Adam, no amsgrad, no weight decay */
    uint32_t flags;
} mrl_ppo_config;
typedef struct mrl_ppo_batch { /* the script's b_* arrays (:259-264), dense, device */
    const float *obs;          /* (S, D); 16-byte (D = 4) / 8-byte (D = 6) / 4-byte (D = 7, the beam) aligned, as for rollouts */
    const int32_t *actions;    /* (S) */
    const float *logprobs, *advantages, *returns, *values; /* (S) */
    uint32_t size;             /* S = T * N */
} mrl_ppo_batch;
typedef struct mrl_ppo_optimizer {
    float *params_dev;           /* the tensor mrl_mlp_policy.params_dev points at; updated in place */
    float *exp_avg, *exp_avg_sq; /* (P) each */
    uint32_t step;               /* Adam steps taken BEFORE this call; row k uses step + 1 + k */
    uint32_t num_members;        /* 0: one policy.  M > 0: mrl_ppo_update steps M dense rows (above).  In what was tail padding. */
} mrl_ppo_optimizer;
int mrl_ppo_workspace_bytes(uint32_t obs_dim, uint32_t hidden, uint32_t num_actions, uint32_t minibatch_size,
                            uint32_t num_minibatches, uint64_t *out);
int mrl_ppo_update(const mrl_mlp_policy *shape, const mrl_ppo_optimizer *opt, const mrl_ppo_batch *batch,
                   const int32_t *indices_dev /* (K, B) */, uint32_t num_minibatches /* K */, uint32_t minibatch_size /* B */,
                   const mrl_ppo_config *cfg, void *workspace_dev, uint64_t workspace_bytes,
                   float *stats_dev_or_null /* (K, 8) */, float *grads_dev_or_null /* (K, P) */, int gpu_id, void *hip_stream);

/* The collection phase of the reference's CleanPPOAgent (pantheonrl_extension/vectoragent.py:116-372) on the device, for
 * Hanabi and the balance beam: the agent scripts/hanabi_train.py and scripts/balance_train.py build twice (ego and partner)
 * around env.step.  Per environment step and agent the reference casts observation and state to float, runs two four-layer
 * ReLU MLPs of width 512 for EVERY world, masks the logits, draws from a Categorical, writes about ten buffer rows
 * (:352-371) and reads torch.any(dones) on the host (:207); before each update it walks T steps backwards with boolean-mask
 * indexing (:230-262).  Here those are mrl_agent_act, mrl_agent_credit and mrl_gae_active; none of them synchronises.  The
 * learning phase (:268-330) is mrl_agent_update, below.  No reference counterpart as calls.  DESIGN.md section 14.
 *   Policy (CleanRLNetwork, :66-113): critic = Linear(S, 512), ReLU, Linear(512, 512), ReLU, Linear(512, 512), ReLU,
 *     Linear(512, 1); actor the same from D inputs to A outputs.  params_dev is one flat float32 device array in the order of
 *     parameters_to_vector(agent.parameters()): critic.0.weight (512, S) row-major, critic.0.bias, ..., critic.6.bias, then
 *     actor.0.weight, ...; mrl_wide_policy_num_params floats.  It is read in place in every call.  The width and the number of
 *     layers are fixed; 1 <= A <= MRL_WIDE_MAX_ACTIONS; D and S from 1 up, at most the simulator's row widths.
 *   mrl_agent_act acts for player `player` on the simulator's tensors as they stand: OBSERVATION, STATE (the balance beam's
 *     state is its observation), ACTION_MASK and ACTIVE_AGENT are read in place, in their own element types and at their own
 *     strides (the first D / S / A entries of a row); there is no float copy of the inputs.
 *     Rows: only worlds with ACTIVE_AGENT[player, w] != 0 are computed (an integer compaction in front of the layers); the
 *     others get action 0, log-prob 0 and value 0 -- the Hanabi step reads the mover's action only, and a trainer reads active
 *     rows only.  MRL_AGENT_ALL_ROWS computes every world, as the reference does.
 *     Arithmetic: every matrix layer runs on v_mfma_f32_32x32x2_f32 in exact float32; an output starts from 0 and adds the
 *     inputs in ascending order, one fused multiply-add each (a K that is not a multiple of 2 is padded with zeros); the bias
 *     is added to the finished sum, one more rounding.  (Unlike mrl_policy_act, whose chain starts from the bias: here the
 *     output layers' products are a hundred times smaller than their bias, and 512 of them rounded at the bias's ulp put
 *     the value 6 - 17 ulp from a float64 evaluation; bias last, it is within 3.)
 *     Head, float32, per computed world: legal = ACTION_MASK != 0; m = max legal logit; e_a = exp(l_a - m), 0 for illegal a;
 *     p_a = e_a / sum e (sum in ascending a); h = the hash of mrl_rollout_random of (seed, step, w, player); u = (h >> 8) * 2^-24;
 *     action = the number of a in 0..A-2 with u >= p_0 + ... + p_a; if that action is illegal (rounding left the cumulative sum
 *     below u) the last legal action; logprob = (l_action - m) - log(sum e).  MRL_POLICY_GREEDY: the first legal arg-max.  The
 *     action goes to ACTION[player, w].  A world with no legal action (undefined in the reference: NaN) yields action 0 and
 *     log-prob -inf.
 *     Recording, record != NULL (:354-371), row `row` < num_steps of dense buffers: obs (T, N, D) and states (T, N, S) in the
 *     inputs' own element types, action_masks (T, N, A) uint8 0/1, active (T, N) uint8, actions int32, logprobs, values,
 *     dones (the agent's next_done as 0.0 / 1.0, which is then cleared), rewards (row set to 0) (T, N); last_active[w] = row
 *     and new_game[w] = 0 where the world is active.  Inactive worlds get their obs / states / mask copies too.  logits, if
 *     non-NULL, (N, MRL_WIDE_MAX_ACTIONS): the A unmasked logits of every computed world (tests and diagnostics).
 *     MRL_AGENT_VALUE_ONLY (needs record): the critic alone; next_value[w] = its value (0 for a world not computed),
 *     next_active[w] = ACTIVE_AGENT != 0; nothing else is written, no action is drawn.
 *     workspace: mrl_agent_workspace_bytes(N) bytes of device memory, 16-byte aligned, the caller's; holds nothing between calls.
 *     Launches: compaction, bookkeeping and copies, four layers (a grid over row tile x column slab x net), head.
 *     MRL_ERR_INVALID: a game other than Hanabi or the balance beam; a NULL policy, parameter array or workspace; A > 64 or 0;
 *     D / S / A wider than the simulator's rows; player out of range; row >= num_steps, num_worlds other than the simulator's or
 *     a NULL buffer in a record; VALUE_ONLY without a record; a capturing stream wherever mrl_step refuses one (the row and the
 *     step number travel in kernel arguments: a captured call would replay them); a simulator that has been through
 *     mrl_exchange_create.
 *   mrl_agent_credit is update() (:197-219) as one launch, dones = the DONE tensor (int32, N): running_rewards[w] += r;
 *     rewards[last_active[w], w] += new_game[w] ? 0 : r; next_done[w] |= done; where done: the running return joins totals,
 *     then running_rewards[w] = 0 and new_game[w] = 1.  totals is float64 (ceil(N / 1024), 4) = finished episodes, the sum of
 *     their returns, their minimum, their maximum per block of 1024 worlds; the caller initialises it to (0, 0, +inf, -inf).
 *     One workgroup owns a block and adds its worlds in a fixed order; no float atomics.  (The reference's indexed assignment,
 *     self.rewards[self.last_active] += ..., selects whole ROWS and so also adds r[w] to column w of every row that is any
 *     world's last_active; those extra cells belong to steps at which w was not the one to act or which w has since left behind
 *     only if worlds get out of step with each other.  What is followed here is the documented intent, per world.)
 *   mrl_gae_active is :231-262, a lane per world, t = T-1 ... 0, float32, the reference's operations in its order,
 *     gl = float32(double(gamma) * double(lambda)):  boot = next_active[w]; nnt = boot ? 1 - next_done[w] : 0;
 *     nv = boot ? next_value[w] : 0; last = 0.  At t, if active[t, w]: a world not yet bootstrapped computes delta = r[t,w] +
 *     gamma * nv * nnt - v[t,w] (its nv and nnt are 0), advantages[t,w] = last = delta + gl * nnt * last, has active[t, w]
 *     CLEARED (the row only carries the bootstrap) and is bootstrapped from there on, its nnt and nv still 0 (the reference
 *     clears the flag through a view of the very mask it then indexes `nextnonterminal[mask] = ...` with, :245-261, so the row
 *     that bootstraps a world hands nothing on: the next earlier active row of that world computes r - v again); a world that
 *     was bootstrapped before t computes the same two lines and then sets nnt = 1 - dones[t,w], nv = v[t,w].  Everything else of
 *     advantages is 0; returns = advantages + values.
 *     One coupling between worlds exists in the reference and is kept: while any world of the batch is not yet bootstrapped
 *     (`if not torch.all(bootstrapped)`, :248), only the worlds being bootstrapped at that t are computed -- an already
 *     bootstrapped, active world keeps advantage 0 and its `last`, though its nnt and nv advance and its row stays active.
 *     With first[w] = T if next_active[w], else the largest t with active[t,w], else -1, and t* = min over w of first[w] (one
 *     integer-minimum launch in front, through record->first_step), that holds at every t >= t*.
 *     MRL_ERR_INVALID: a NULL record, array or buffer. */
enum { MRL_AGENT_ALL_ROWS = 2, MRL_AGENT_VALUE_ONLY = 4 }; /* flags of mrl_agent_act, beside MRL_POLICY_GREEDY */
#define MRL_WIDE_HIDDEN 512
#define MRL_WIDE_MAX_ACTIONS 64
typedef struct mrl_wide_policy {
    const float *params_dev;
    uint32_t obs_dim, state_dim, num_actions; /* D, S, A */
} mrl_wide_policy;
typedef struct mrl_agent_record { /* all device pointers, dense; T = num_steps, N = num_worlds */
    void *obs, *states;           /* (T, N, D), (T, N, S), the inputs' element types */
    uint8_t *action_masks;        /* (T, N, A) */
    uint8_t *active;              /* (T, N) */
    int32_t *actions;             /* (T, N) */
    float *logprobs, *values, *dones, *rewards; /* (T, N) */
    int32_t *last_active;         /* (N) */
    uint8_t *new_game, *next_done; /* (N) */
    float *running_rewards;       /* (N) */
    double *totals;               /* (ceil(N / 1024), 4) */
    float *next_value;            /* (N), written by MRL_AGENT_VALUE_ONLY */
    uint8_t *next_active;         /* (N), written by MRL_AGENT_VALUE_ONLY */
    int32_t *first_step;          /* (1), scratch of mrl_gae_active */
    float *logits;                /* (N, MRL_WIDE_MAX_ACTIONS) or NULL */
    uint32_t num_steps, num_worlds;
} mrl_agent_record;
uint64_t mrl_wide_policy_num_params(uint32_t obs_dim, uint32_t state_dim, uint32_t num_actions);
uint64_t mrl_agent_workspace_bytes(uint32_t num_worlds);
int mrl_agent_act(mrl_sim *sim, uint32_t player, const mrl_wide_policy *policy, const mrl_agent_record *record_or_null,
                  uint32_t row, uint64_t seed, uint32_t step, uint32_t flags, void *workspace_dev, void *hip_stream);
int mrl_agent_credit(const mrl_agent_record *record, const float *rewards_dev, const int32_t *dones_dev, uint32_t num_worlds,
                     int gpu_id, void *hip_stream);
int mrl_gae_active(const mrl_agent_record *record, const float *next_value, const uint8_t *next_active, float gamma, float lambda,
                   float *advantages, float *returns, int gpu_id, void *hip_stream);

/* The learning phase of CleanPPOAgent (pantheonrl_extension/vectoragent.py:268-330) on the device, for the wide policy above:
 * boolean-mask indexing, float copies of the int8 rows, autograd over both nets, clip_grad_norm_ and Adam.step() become
 * mrl_agent_update.  No reference counterpart as a call.  DESIGN.md section 17.
 *   Samples: the cells (t, w) of the record with active[t, w] != 0, in ascending flat order t N + w (the order of the
 *     reference's self.obs[self.active]); B of them.  The reference's per-epoch randperm (:281) only reorders a whole-batch
 *     mean, so there is no permutation and no index argument.
 *   One call is `epochs` epochs (:283-323).  Epoch k, float32: logits and values of the B samples are recomputed from rows
 *     record->obs / record->states (element types obs_type / state_type, converted on load; no float copy) with
 *     mrl_agent_act's own layer kernel, so on unchanged parameters they carry the record's bits; the masked soft-max, the
 *     log-prob of the recorded action and the entropy use mrl_agent_act's expressions; ratio = exp(new - old).  With
 *     MRL_PPO_NORM_ADV A = (adv - mean) / (std + 1e-8), mean and unbiased std over all B samples (summed in double, once per
 *     call); the losses, their gradient rules for max / clamp, the clipping and Adam's step are mrl_ppo_update's (above), with
 *     one clip over ALL parameters and t = opt->step + 1 + k; ReLU passes a gradient where the activation is > 0.
 *     cfg->lr .. eps are Adam's.  opt->params_dev is the parameter array (policy->params_dev is not read).
 *   Arithmetic of the backward pass: a weight gradient dW[c][k] = sum_j dY[j][c] X[j][k] and a bias gradient db[c] = sum_j
 *     dY[j][c] start from 0 and add the samples in list order, one fused multiply-add each, on v_mfma_f32_32x32x2_f32 (the
 *     sample pair is the instruction's k; an odd count is padded with a zero); an input gradient dX[j][k] = (X[j][k] > 0)
 *     sum_c dY[j][c] W[c][k] adds c ascending the same way.  Every gradient entry is written once; there are no partial
 *     vectors, no float atomics and no wait between workgroups: the same inputs give the same bits on every run, on any
 *     stream, and one call of K epochs the bits of K calls of one (with opt->step advanced by the caller).
 *   stats (epochs, 10), optional: mrl_ppo_update's eight columns, then 8 samples = B (exact: T N >= 2^24 is refused) and
 *     9 status: 0 done; 1 B < 2 (the reference's .std() is NaN there); 2 B > capacity.  With status 1 or 2 no byte of the
 *     parameters, the moments or grads changes and columns 0-7 are 0.  grads (epochs, P), optional: row k is epoch k's
 *     unclipped gradient in parameter order.
 *   A sample whose mask row has no legal action has log-prob -inf in the record; as in the reference the update then yields
 *     NaN.  It cannot occur for an active seat of either game.
 *   workspace: mrl_agent_update_workspace_bytes for `capacity` samples, 1 <= capacity <= T N, 16-byte aligned, the
 *     caller's; it holds nothing between calls.  With n = capacity and P = mrl_wide_policy_num_params, pad = up to a
 *     multiple of 256:  pad(4 n) + 256  +  2 * 6 * 2048 n  +  2 * 256 n  +  2 pad(4 n)  +  256  +  pad(64 ceil(n / 256))  +
 *     2 pad(4 P)  +  pad(4 ceil(P / 256))  bytes: the sample list and its three words; activations and hidden gradients
 *     (2 nets x 3 layers x n x 512 floats each); logits and d_logits; value and d_value; mean and std; partial stats; the
 *     gradient, its copy and the blocks' sums of squares.  About 25 KB per sample.
 *   The call only enqueues on hip_stream of device gpu_id: it never synchronises or allocates.  Every kernel reads B from a
 *     device word; grids are sized for capacity and tiles past B leave at once.  Launches: the list, the advantages' moments
 *     (MRL_PPO_NORM_ADV), and per epoch four forward layers, the loss head, three input-gradient layers, one weight-gradient
 *     launch over all eight layers and the two of the optimiser tail.
 *   MRL_ERR_INVALID: a NULL among policy, opt, record, cfg, advantages, returns, workspace, the optimizer's three arrays and
 *     the record's obs, states, action_masks, active, actions, logprobs, values; num_actions outside 1..64; obs_dim or
 *     state_dim 0; T N >= 2^24; capacity 0 or above T N; workspace_bytes too small; a workspace off a 16-byte boundary or a
 *     float / int32 array off a 4-byte one; flag bits other than MRL_PPO_NORM_ADV | MRL_PPO_CLIP_VLOSS; an element type
 *     other than MRL_INT8 .. MRL_UINT32; a capturing stream.  epochs == 0 enqueues nothing.
 *     mrl_agent_update_workspace_bytes refuses the same shapes (capacity 0 or >= 2^24) and a NULL out. */
int mrl_agent_update_workspace_bytes(uint32_t obs_dim, uint32_t state_dim, uint32_t num_actions, uint32_t capacity, uint64_t *out);
int mrl_agent_update(const mrl_wide_policy *policy, const mrl_ppo_optimizer *opt, const mrl_agent_record *record,
                     uint32_t obs_type, uint32_t state_type, const float *advantages, const float *returns /* (T, N) */,
                     uint32_t epochs, const mrl_ppo_config *cfg, uint32_t capacity, void *workspace_dev, uint64_t workspace_bytes,
                     float *stats_or_null /* (epochs, 10) */, float *grads_or_null /* (epochs, P) */, int gpu_id, void *hip_stream);

/* MAPPO's CNN actor-critic for the two kitchens, Overcooked and Simplecooked, on the device: what the reference's rollout loop runs in torch around every step
 * (train/MAPPO/main_player.py:211-261) -- for each seat an int8 -> float cast, a movedim, Conv2d, three Linear layers and a
 * Categorical, twice (actor and critic: train/MAPPO/utils/cnn.py:26-42, r_actor_critic.py, utils/distributions.py:55-68, hidden_size
 * 64 as the reference's Overcooked notebook sets it) -- as ONE launch per act, mrl_cnn_act, and a whole T-step collection as one
 * call, mrl_rollout_cnn.  No reference counterpart as calls.  DESIGN.md section 15.
 *   Networks, for a W x H kitchen with F channels (Overcooked: 5P + 16; Simplecooked: 5P + 10, P = 1 or 2) and npos = (W - 2)(H - 2): Conv2d(F, 32, 3 x 3, valid), ReLU, flatten,
 *     Linear(32 npos, 64), ReLU, Linear(64, 64), ReLU, then Linear(64, 6) (actor) or Linear(64, 1) (critic).  In both kitchens the
 *     critic's input IS the seat's observation (share_observation_space = observation_space) and no action is masked (Simplecooked's mask is all ones).
 *     params_dev is one flat float32 device array: the actor's eight tensors, then the critic's eight, each in
 *     parameters_to_vector order -- conv weight (32, F, 3, 3) and bias, fc1 weight (64, 32 npos) and bias, fc2 weight and bias, head
 *     weight and bias; mrl_cnn_policy_num_params(W, H, F, hidden, A) floats (0 for hidden != 64 or A != 6 or W, H < 3).  It is read
 *     in place in every call.  hidden must be 64; flags is 0 or MRL_POLICY_GREEDY, which both calls OR into their own flags
 *     (mrl_rollout_cnn has no flags argument of its own).
 *   Samples: (world n, seat p) for every seat whose bit is set in `players` (seats 0..31).  The kernel reads the int8 world-major
 *     block (N, P, H, W, F) where the simulator's most recent step wrote its observations -- its own OBS_WORLD_MAJOR tensor, the
 *     slot of mrl_set_observation_output, or ring slot (k - 1) mod T; where no step has run since that destination was set,
 *     where the next step will write -- in place, converting on load: there is no float copy of the observations.
 *   THE INDEX MAP: torch sees x[n, f, w, h] = obs[n, p, h, w, f], so for the conv weight Wc[c, f, i, j]
 *       conv[n, c, ow, oh] = bc[c] + sum over (f, i, j) of Wc[c, f, i, j] * obs[n, p, oh + j, ow + i, f],  ow < W - 2, oh < H - 2,
 *     and fc1's input index is c (W - 2)(H - 2) + ow (H - 2) + oh.
 *   Arithmetic: mrl_agent_act's rule.  Every product runs on v_mfma_f32_32x32x2_f32 in exact float32; an output starts from 0 and
 *     adds its products with one fused multiply-add each in ascending order of torch's flattened weight index (conv: k = 9 f + 3 i +
 *     j; the linear layers: their input index; an odd K -- the convolution's 9 F for an odd F, as one-player Simplecooked's 15 -- is padded with one zero product); the bias is added to the finished sum.
 *     No float atomics, no order that depends on timing: the same inputs give the same bits on every run and on any stream.
 *   Head, float32, A = 6: mrl_policy_act's rule above with the seat as the hash's player -- h = the hash of (seed, step, n, p);
 *     u = (h >> 8) * 2^-24; m = max logit; e_a = exp(l_a - m); p_a = e_a / sum e; action = the number of a in 0..4 with u >= p_0 +
 *     ... + p_a; logprob = (l_action - m) - log(sum e).  MRL_POLICY_GREEDY: the first arg-max (the reference's deterministic=True
 *     is probs.argmax).  The action goes to ACTION[p, n].  Without a record only the actor runs.
 *   Record (mrl_cnn_record), dense device arrays, T = num_steps: actions int32, logprobs, rewards, dones (T, N, P); values
 *     (T + 1, N, P), row T the closing value; next_done (N, P); logits (T, N, P, 6), optional (tests and diagnostics); all float32
 *     but actions.  An act at row k < T writes, for its seats, actions / logprobs / values / logits [k, n, p], dones[k, n, p] =
 *     DONE[n] != 0 as 0.0 / 1.0 -- the flag as it stands in front of step k, mrl_policy_act's convention -- and, for k > 0,
 *     rewards[k - 1, n, p] = (float)REWARD[p, n] (the same for every seat).  MRL_CNN_VALUE_ONLY needs row == T: the critic alone;
 *     it writes values[T], rewards[T - 1] (T > 0) and next_done and touches neither ACTION nor any other row.  Flattened to N P
 *     columns the arrays are what mrl_gae takes (next_value = values[T]).  Seats outside `players` keep every byte of their
 *     ACTION row and of their record columns.
 *   workspace: mrl_cnn_workspace_bytes(num_worlds, num_players) bytes of device memory on a 16-byte boundary, the caller's.  The
 *     fused kernel keeps every intermediate in LDS and does not touch it today; the amount is fixed (256 bytes) and is part of
 *     the call so that a later, larger tile need not change the ABI.
 *   Launches: one -- a workgroup of four wavefronts per (tile of 32 samples, net); with one seat (P = 1, or one bit in `players`) a
 *     tile is 32 worlds.  The call only enqueues on hip_stream; it never
 *     synchronises or allocates.
 *   Limit: the workgroup's LDS image -- 32 observation rows of H W F bytes (+ 3, rounded up to an odd number of dwords), the conv
 *     weights (32 rows of 9 F floats, padded to an odd count), 2 bytes per k, and the convolution's output, 32 rows of 32 npos + 1
 *     floats -- must fit 160 KiB.  The five standard two-player layouts do (Overcooked 9 x 5: 154 464 bytes; 5 x 4: 72 032; Simplecooked's rows are shorter); a larger kitchen or
 *     more players than that allows is refused, never computed wrongly.
 *   MRL_ERR_INVALID: a simulator that is neither Overcooked nor Simplecooked; hidden != 64; players == 0 or a bit >= P; a NULL policy, parameter array
 *     or workspace, or a NULL buffer but logits in a record; row >= T without MRL_CNN_VALUE_ONLY, row != T with it, or it without a
 *     record; workspace_bytes below mrl_cnn_workspace_bytes or a workspace off a 16-byte boundary; a shape beyond the limit; a
 *     capturing stream (row and step travel in kernel arguments, as for the sibling calls); a flag bit other than
 *     MRL_POLICY_GREEDY and MRL_CNN_VALUE_ONLY; a kitchen narrower or lower than 3; a simulator that has been through
 *     mrl_exchange_create.
 * mrl_rollout_cnn: obs_ring is int8 (T + 1, N, P, H, W, F), dense.  Slot 0 receives the current observations (one copy); for
 *   k < T: mrl_cnn_act on slot k at row k with step number first_step + k, then the ordinary step (mrl_step reading the ACTION
 *   tensor) writes slot k + 1 through the observation ring of mrl_set_observation_ring; then the closing MRL_CNN_VALUE_ONLY act on
 *   slot T.  Afterwards the simulator's observation output is what it was before the call (destination and ring position), and
 *   slot T is copied to where that output's most recent step wrote (one more device-to-device copy, T > 0): the simulator,
 *   its observations included, is exactly where T mrl_step_with_actions calls with actions[0..T-1] would have left it, and the
 *   next mrl_cnn_act or mrl_rollout_cnn reads the observations of the state it acts on -- two rollouts of T equal one of 2 T.  Seats outside `players`
 *   step with whatever their ACTION rows hold.  Simplecooked: the same call, P = 1 included.  A ring whose slots do not start on 16-byte boundaries is staged as
 *   mrl_set_observation_ring says.  It takes no workspace (its acts need none).  Refusals: those of mrl_cnn_act, a NULL record or ring. */
enum { MRL_CNN_VALUE_ONLY = 4 }; /* flag of mrl_cnn_act, beside MRL_POLICY_GREEDY */
typedef struct mrl_cnn_policy {
    const float *params_dev;
    uint32_t hidden, flags;
} mrl_cnn_policy;
typedef struct mrl_cnn_record { /* all device pointers, dense; T = num_steps */
    int32_t *actions;           /* (T, N, P) */
    float *logprobs;            /* (T, N, P) */
    float *values;              /* (T + 1, N, P) */
    float *rewards, *dones;     /* (T, N, P) */
    float *next_done;           /* (N, P) */
    float *logits;              /* (T, N, P, 6) or NULL */
    uint32_t num_steps;
} mrl_cnn_record;
uint64_t mrl_cnn_policy_num_params(uint32_t width, uint32_t height, uint32_t channels, uint32_t hidden, uint32_t num_actions);
uint64_t mrl_cnn_workspace_bytes(uint32_t num_worlds, uint32_t num_players);
int mrl_cnn_act(mrl_sim *sim, uint32_t players, const mrl_cnn_policy *policy, const mrl_cnn_record *record_or_null, uint32_t row,
                uint64_t seed, uint32_t step, uint32_t flags, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream);
int mrl_rollout_cnn(mrl_sim *sim, uint32_t players, const mrl_cnn_policy *policy, const mrl_cnn_record *record, void *obs_ring_dev,
                    uint64_t seed, uint32_t first_step, void *hip_stream);

/* A population of partners: a BANK of K CNN policies of one shape and a policy per (world, seat) cell, so that one batch of worlds
 * plays against many partners at once and a world's partner can change when its episode ends -- what the reference's
 * VectorMultiAgentEnv.add_partner_agent promises per episode and its vectorised reset can only do for the whole batch
 * (pantheonrl_extension/vectorenv.py:89-98, 202-210).  No reference counterpart as calls.  DESIGN.md section 19.
 *   Bank (mrl_cnn_bank): params_dev is a float32 device array of K = num_policies rows, `stride` floats apart (stride >=
 *     mrl_cnn_policy_num_params); row k is exactly an mrl_cnn_policy's params_dev, so mrl_cnn_act, mrl_mappo_update and the bank act
 *     read and write the same floats.  1 <= K <= 256.  hidden and flags as in mrl_cnn_policy.
 *   Assignment: ids, int32 (N, P), device memory, the caller's.  ids[n, p] = k >= 0: seat p of world n acts under row k.  -1 (any
 *     negative value): the cell is not acted -- its ACTION entry and its record cells keep every byte.  A value >= K is outside
 *     the contract: the cell is treated as -1 and, where its seat is in `players`, counted in the workspace's out_of_range word.
 *     A cell is acted when its seat's bit is set in `players` AND its id is valid.
 *   mrl_cnn_act_bank is the plan and the act, on hip_stream: two launches up to M = N P = 2048 cells (the plan is one workgroup),
 *     four beyond (the plan is then count, scan and place, the first and the last with a workgroup per 1024 cells; no workgroup
 *     waits for another inside a kernel).
 *     The plan writes the workspace, uint32 words, with Kp = K rounded up to a multiple of 4 and max_tiles = ceil(M / 32) + K:
 *         [0] tiles   [1] acted   [2] out_of_range   [3] 0
 *         [4, 4 + Kp)                          count[k], the acted cells of policy k
 *         [4 + Kp, 4 + 2 Kp)                   start[k], where policy k's list begins in `lists`
 *         [4 + 2 Kp, 4 + 2 Kp + 4 max_tiles)   the tile table, four words per tile: policy, first, rows (1..32), 0
 *         the next M words (rounded up to a multiple of 4): lists -- the cells s = n P + p of policy 0, then of policy 1, ...,
 *         each policy's in ascending s; tile t is lists[first, first + rows)
 *         then ceil(M / 1024) rows of Kp + 4 words, the plan's own: per chunk of 1024 cells what lies in front of it (M > 2048 only)
 *     mrl_cnn_bank_workspace_bytes(N, P, K) = 4 (4 + 2 Kp + 4 max_tiles + M rounded up to 4 + ceil(M / 1024) (Kp + 4)) (0 for K = 0
 *     or K > 256).  Every acted
 *     cell is in exactly one list, its own policy's; a tile holds one policy's cells; tiles = sum over k of ceil(count[k] / 32)
 *     <= ceil(M / 32) + K.  Words behind `tiles` entries of the table and behind `acted` entries of the lists are not written.
 *     The act is mrl_cnn_act's kernel body over those tiles: the same LDS image, the same products in the same order, the
 *     same hash of (seed, step, n, p), the same head and flags, the same observation source (the simulator's tensor, a redirected
 *     slot or a ring slot), with the tile's rows taken from the list and the parameters from params_dev + policy * stride.  A
 *     sample's arithmetic reads its own rows and the tile's common weights only, so every output is bit for bit what
 *     mrl_cnn_act gives that cell under that policy, whatever else shares the tile and whatever the order of the lists.  The
 *     grid is sized for the bound; workgroups past `tiles` leave at once.  Record rows are written for acted cells only; values,
 *     rewards and dones come from the critic of the cell's own policy.  ids_row, (N, P) int32 or NULL, receives the ids as this
 *     act used them: k for an acted cell, -1 for every other.
 *   Refusals (MRL_ERR_INVALID, nothing enqueued): those of mrl_cnn_act; K = 0 or K > 256; stride below
 *     mrl_cnn_policy_num_params; NULL ids; a workspace below mrl_cnn_bank_workspace_bytes or off a 16-byte boundary.
 * mrl_cnn_bank_resample: one launch, a lane per world.  Where DONE[n] != 0 (the world has just restarted itself):
 *     episodes[n] += 1, and every seat p of `players` with ids[n, p] >= 0 takes a new id from [first_id[p], first_id[p] +
 *     num_ids[p]) -- MRL_CNN_RESAMPLE_ROBIN: first + (id - first + 1) mod num (uint32 arithmetic); MRL_CNN_RESAMPLE_RANDOM: first +
 *     (((h >> 8) * num) >> 24) with h the hash of (seed, episodes[n] after the increment, n, p), exact in 32 bits for num <= 256.
 *     Nothing else changes: other worlds, seats outside `players`, negative cells.  first_id and num_ids are HOST arrays, one
 *     entry per seat of the simulator (entries of seats outside `players` are not read).  Refused: a NULL pointer, a mode other
 *     than the two, num_ids = 0 or first_id + num_ids > 256 for a seat of `players`, `players` as for mrl_cnn_act.
 * mrl_rollout_cnn_bank: mrl_rollout_cnn's loop with the bank act -- for k < T: the bank act on ring slot k at row k (ids_record
 *     row k, when given, receives that act's ids_row), the ordinary step, then, with a resample, mrl_cnn_bank_resample; then the
 *     closing MRL_CNN_VALUE_ONLY bank act at row T (ids_record row T).  No host wait inside.  The ring, the hand-back of the
 *     observation output and the copy of slot T are mrl_rollout_cnn's: two rollouts of T equal one of 2 T, ids and episodes
 *     included.  With resample NULL neither ids nor episodes change (episodes may then be NULL).  Refusals: those of
 *     mrl_cnn_act_bank and mrl_cnn_bank_resample, a NULL record or ring, NULL episodes with a resample. */
enum { MRL_CNN_RESAMPLE_ROBIN = 1, MRL_CNN_RESAMPLE_RANDOM = 2 };
typedef struct mrl_cnn_bank {
    const float *params_dev;    /* (num_policies, stride) */
    uint32_t num_policies;
    uint64_t stride;            /* floats between rows */
    uint32_t hidden, flags;
} mrl_cnn_bank;
typedef struct mrl_cnn_resample {
    uint32_t mode;                          /* MRL_CNN_RESAMPLE_ROBIN or MRL_CNN_RESAMPLE_RANDOM */
    const uint32_t *first_id, *num_ids;     /* host, one per seat */
    uint64_t seed;
} mrl_cnn_resample;
uint64_t mrl_cnn_bank_workspace_bytes(uint32_t num_worlds, uint32_t num_players, uint32_t num_policies);
int mrl_cnn_act_bank(mrl_sim *sim, uint32_t players, const mrl_cnn_bank *bank, const int32_t *ids_dev, const mrl_cnn_record *record_or_null,
                     int32_t *ids_row_or_null, uint32_t row, uint64_t seed, uint32_t step, uint32_t flags, void *workspace_dev,
                     uint64_t workspace_bytes, void *hip_stream);
int mrl_cnn_bank_resample(mrl_sim *sim, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev, int32_t *episodes_dev,
                          void *hip_stream);
int mrl_rollout_cnn_bank(mrl_sim *sim, uint32_t players, const mrl_cnn_bank *bank, int32_t *ids_dev, int32_t *episodes_dev,
                         const mrl_cnn_resample *resample_or_null, const mrl_cnn_record *record, int32_t *ids_record_or_null,
                         void *obs_ring_dev, uint64_t seed, uint32_t first_step, void *workspace_dev, uint64_t workspace_bytes,
                         void *hip_stream);

/* MAPPO's update for that actor-critic on the device: R_MAPPO.ppo_update (train/MAPPO/r_mappo.py:91-164, feed-forward networks, all
 * active masks one) with ValueNorm (utils/valuenorm.py) -- gather, both forward passes, the clipped losses, backward, two
 * clip_grad_norm_ and two Adam steps -- on the flat parameter array mrl_cnn_act reads, which is updated in place.  No reference
 * counterpart as a call.  DESIGN.md section 16.  The call sees no simulator: width, height and channels are the policy's, so a
 * Simplecooked ring (channels = 5P + 10, P = 1 or 2) runs as an Overcooked one does.
 *   Samples: s = (t N + n) P + p is row t, world n, seat p of an mrl_cnn_record; its observation is the H W F bytes at s H W F of
 *     batch->obs (the ring mrl_rollout_cnn filled: slot t is what the act of step t saw), read as int8 and converted on load.
 *   One call is K = num_minibatches steps in row order; row k takes the B = minibatch_size samples indices[k, :].  An index >= S
 *     is outside the contract; it is clamped to S - 1, so it stays memory-safe.
 *   Per sample, float32, c = clip_param: logits -> max m, e_a = exp(l_a - m), p_a = e_a / sum e, logp_a = (l_a - m) - log(sum e)
 *     (mrl_cnn_act's own expressions: on unchanged parameters logp[action] and v are the record's, bit for bit), H = -sum p logp;
 *     ratio = exp(logp[action] - old); actor loss = -mean(min(ratio A, clamp(ratio, 1 - c, 1 + c) A)) - entropy_coef mean(H), A =
 *     advantages[s] as given.  Critic: v_c = v_old + clamp(v - v_old, -c, c); target = (R - mean) / sqrt(var) of the ValueNorm
 *     state AFTER this row's update (MRL_MAPPO_VALUENORM), else R; e = target - v, e_c = target - v_c; value_loss = mean(max(L(e),
 *     L(e_c))) (MRL_MAPPO_CLIPPED_VALUE_LOSS) or mean(L(e)); L(e) = e^2 / 2, or with MRL_MAPPO_HUBER_LOSS the reference's
 *     huber_loss (utils/util.py:46-50) as written: e^2 / 2 for |e| <= delta, delta (|e| - delta / 2) for e > delta and 0 for e <
 *     -delta.  The critic differentiates value_loss_coef value_loss.  Gradients are autograd's: a tie of min / max halves the
 *     gradient between the arguments, clamp passes it on the closed interval, ReLU passes none at a pre-activation of 0.
 *   ValueNorm: value_norm_state = (running_mean, running_mean_sq, debiasing_term), 3 device floats.  Row k: m = mean of the row's
 *     gathered returns, q = mean of their squares; each of the three becomes x * beta + (m | q | 1) * one_minus_beta; then mean =
 *     running_mean / max(deb, epsilon), var = max(running_mean_sq / max(deb, epsilon) - mean^2, 0.01).  The K-row recurrence runs up
 *     front (it depends on no parameter) and leaves the final state in value_norm_state.  Without the flag the state is not
 *     touched and may be NULL.
 *   Clip and Adam, per net (actor with lr, critic with critic_lr): total = sqrt(sum g^2) over the net's own tensors; with
 *     MRL_MAPPO_MAX_GRAD_NORM g *= min(1, max_grad_norm / (total + 1e-6)); then mrl_ppo_update's Adam with t = opt->step + 1 + k.
 *   stats (K, 8), optional: 0 value_loss, 1 critic_grad_norm, 2 policy_loss, 3 dist_entropy, 4 actor_grad_norm, 5 ratio (the mean
 *     importance weight), 6 clipfrac (|ratio - 1| > c), 7 reserved (0).  grads (K, P), optional: each row's summed, unclipped
 *     gradient in parameter order (actor, then critic).
 *   Launches: two up front with MRL_MAPPO_VALUENORM, then three per row (gradient: a workgroup per (share of the row, net), tiles
 *     of 32 samples, everything between the int8 rows and the weight gradients in LDS; ordered sum of the workgroups' partial
 *     vectors; clip, Adam, stats).  At most 256 partial vectors per net, so mrl_mappo_workspace_bytes stops growing with B.  No
 *     float atomics, no wait between workgroups: the same inputs give the same bits on every run, one call of K rows the bits of
 *     K calls of one row.  The call only enqueues on hip_stream of device gpu_id.
 *   MRL_ERR_INVALID, nothing changed: a NULL among policy, opt, batch, indices, cfg, workspace, the arrays of opt and batch, or
 *     value_norm_state with MRL_MAPPO_VALUENORM; policy->params_dev != opt->params_dev; hidden != 64; a kitchen below 3 x 3 or
 *     whose LDS image (mrl_cnn_act's with room for three more 32-row arrays in its first region, plus 256 bytes: DESIGN.md
 *     section 16) does not fit 160 KiB; B == 0 or S == 0; a
 *     workspace below mrl_mappo_workspace_bytes or off a 16-byte boundary; params, moments, float arrays or indices off a 4-byte
 *     boundary; unknown flag bits; a capturing stream.  K == 0 enqueues nothing.  mrl_mappo_workspace_bytes refuses the same
 *     shapes and a NULL out.  Not built: active masks, PopArt, recurrent networks, update_actor = False, weight decay. */
enum { MRL_MAPPO_VALUENORM = 1, MRL_MAPPO_HUBER_LOSS = 2, MRL_MAPPO_CLIPPED_VALUE_LOSS = 4, MRL_MAPPO_MAX_GRAD_NORM = 8 };
typedef struct mrl_mappo_policy {
    const float *params_dev;     /* as mrl_cnn_policy */
    uint32_t hidden, flags;      /* flags: not read */
    uint32_t width, height, channels;
} mrl_mappo_policy;
typedef struct mrl_mappo_config {
    float clip_param, entropy_coef, value_loss_coef, max_grad_norm, huber_delta;
    float lr, critic_lr, beta1, beta2, opti_eps;             /* torch.optim.Adam, no amsgrad, no weight decay */
    float valuenorm_beta, valuenorm_one_minus_beta, valuenorm_epsilon;
    uint32_t flags;                                          /* MRL_MAPPO_* */
} mrl_mappo_config;
typedef struct mrl_mappo_batch {
    const int8_t *obs;           /* (S, H, W, F) */
    const int32_t *actions;      /* (S) */
    const float *logprobs, *value_preds, *returns, *advantages; /* (S) */
    uint32_t size;               /* S */
} mrl_mappo_batch;
typedef struct mrl_mappo_optimizer {
    float *params_dev;           /* the tensor mrl_cnn_policy.params_dev points at; updated in place */
    float *exp_avg, *exp_avg_sq; /* (P) each */
    uint32_t step;               /* Adam steps taken BEFORE this call (both nets step together) */
} mrl_mappo_optimizer;
int mrl_mappo_workspace_bytes(uint32_t width, uint32_t height, uint32_t channels, uint32_t hidden, uint32_t minibatch_size,
                              uint32_t num_minibatches, uint64_t *out);
int mrl_mappo_update(const mrl_mappo_policy *policy, const mrl_mappo_optimizer *opt, const mrl_mappo_batch *batch,
                     const int32_t *indices_dev /* (K, B) */, uint32_t num_minibatches /* K */, uint32_t minibatch_size /* B */,
                     const mrl_mappo_config *cfg, float *value_norm_state_dev_or_null /* (3) */, void *workspace_dev,
                     uint64_t workspace_bytes, float *stats_dev_or_null /* (K, 8) */, float *grads_dev_or_null /* (K, P) */,
                     int gpu_id, void *hip_stream);

/* MAPPO's MLP actor-critic for the balance beam on the device: what the reference's trainer runs in torch for `balance`
 * (train/trainer.py, train/env_utils.py:8-26; R_Actor / R_Critic pick MLPBase for a vector observation, train/MAPPO/
 * r_actor_critic.py:33, utils/mlp.py) -- act, rollout and update, the counterparts of mrl_cnn_act, mrl_rollout_cnn and
 * mrl_mappo_update.  No reference counterpart as calls.  DESIGN.md section 18.
 *   Networks (use_feature_normalization, use_ReLU, use_orthogonal at their defaults; hidden_size 64; layer_N 1 or 2; D = 7 inputs;
 *     A = 4 actions), per net: LayerNorm(7), Linear(7, 64), ReLU, LayerNorm(64), layer_N x [Linear(64, 64), ReLU, LayerNorm(64)],
 *     then Linear(64, 4) (actor, Categorical) or Linear(64, 1) (critic).  LayerNorm is (x - mean) / sqrt(var + 1e-5) * weight + bias
 *     with the biased variance over the row.  The critic's input IS the seat's observation (share_observation_space =
 *     observation_space).  The balance beam's ACTION_MASK is all ones in every state (src/balance_beam_env/sim.cpp:197): the
 *     kernels do not read it.
 *   params_dev is one flat float32 device array, the actor's tensors and then the critic's, each in parameters_to_vector order:
 *     base.feature_norm weight, bias (7, 7); base.mlp.fc1: Linear weight (64, 7), bias, LayerNorm weight, bias; base.mlp.fc_h:
 *     Linear weight (64, 64), bias, LayerNorm weight, bias; base.mlp.fc2.i, i < layer_N: the same four; then the head's weight
 *     (4, 64) or (1, 64) and bias.  mrl_mlpbase_policy_num_params(7, 64, layer_N, 4) floats: 27 361 for layer_N 2, 18 785 for 1 (0
 *     for any other shape).  fc_h IS PART OF THE TENSOR AND OF NO COMPUTATION: the reference registers it and its forward never
 *     uses it (mlp.py:20-27; fc2 are deep copies of it).  No kernel reads its 4 288 floats per net; its gradient is zero; its
 *     parameter bits never change and its moments stay what they were (zero moments stay zero) -- the reference's Adam and
 *     clip_grad_norm_ skip it because its grad is None.
 *   Samples: (world n, seat p) for every seat whose bit is set in `players`.  The act reads OBSERVATION int32 (2, N, 7) in place,
 *     converting on load.
 *   Arithmetic, float32.  Linear: mrl_cnn_act's rule on v_mfma_f32_32x32x2_f32 -- an output starts from 0 and adds its products
 *     with one fused multiply-add each in ascending input index, K = 7 padded with one zero product, the bias added to the
 *     finished sum.  LayerNorm: a wavefront per row, lane j column j (lanes past the width add 0); a sum over the row is six
 *     exchange steps, partners 32, 16, 8, 4, 2, 1 lanes apart, each lane adding its partner's partial sum to its own; mean = sum /
 *     width, var = sum((x - mean)^2) / width, xhat = (x - mean) * (1 / sqrtf(var + 1e-5)), y = xhat * weight + bias (a product,
 *     then a sum).  No float atomics, no order that depends on timing: the same inputs give the same bits on every run.
 *   Head: mrl_cnn_act's with A = 4 -- h = the hash of (seed, step, n, p); u = (h >> 8) * 2^-24; the cumulative draw over the
 *     soft-max; MRL_POLICY_GREEDY the first arg-max; the action goes to ACTION[p, n].  Without a record only the actor runs.
 *   Record (mrl_mlpbase_record), dense device arrays, T = num_steps: mrl_cnn_record's arrays and row convention (logits (T, N, P,
 *     4), optional; rewards[k - 1, n, p] = REWARD[p, n], float32 here) and obs int32 (T + 1, N, P, 7): row k receives the
 *     observation rows the act at row k read, the closing MRL_MLPBASE_VALUE_ONLY act's at row T included.  Seats outside
 *     `players` keep every byte of their ACTION row and of their record columns.
 *   mrl_rollout_mlpbase: for k < T mrl_mlpbase_act at row k with step number first_step + k, then the ordinary step (mrl_step
 *     reading the ACTION tensor); then the closing value-only act at row T.  No host in the loop; two rollouts of T equal one of
 *     2 T.  Seats outside `players` step with whatever their ACTION rows hold.
 *   mrl_mappo_mlp_update: mrl_mappo_update's samples (s = (t N + n) P + p; the observation is the seven int32 at 7 s of
 *     batch->obs, the record's obs), losses, ValueNorm, clip, Adam, stats (K, 8), grads (K, P) and launch plan on this network:
 *     two launches up front with MRL_MAPPO_VALUENORM, then three per row -- the gradient kernel (a workgroup per (share of the
 *     row, net), tiles of 32 samples, everything between the observation row and the weight gradients in LDS: forward keeping
 *     normalised rows, reciprocal standard deviations and ReLU signs, loss head, backward; LayerNorm backward dx = rstd (g -
 *     mean(g) - xhat mean(g xhat)) with g = dy weight, dweight = sum dy xhat, dbias = sum dy; every Linear weight gradient on the
 *     matrix instruction with the sample pair as k), the ordered sum of at most 256 partial vectors per net, and clip + Adam
 *     per net.  On unchanged parameters the recomputed log-prob and value are the record's bit for bit.  Same inputs, same
 *     bits; one call of K rows gives the bits of K calls of one row.
 *   MRL_ERR_INVALID, nothing changed.  Act and rollout: a simulator that is not the balance beam, or one that has been through
 *     mrl_exchange_create or mrl_prepare_graph_capture; a capturing stream; hidden != 64; layer_N not 1 or 2; players == 0 or a
 *     bit >= 2; a NULL policy or parameter array; a NULL buffer but logits in a record; int32 or float arrays off a 4-byte
 *     boundary; a flag bit other than MRL_POLICY_GREEDY and MRL_MLPBASE_VALUE_ONLY; row >= T without MRL_MLPBASE_VALUE_ONLY, row
 *     != T with it, or it without a record; a NULL record for the rollout.  Update: mrl_mappo_update's refusals with the shape
 *     check replaced by obs_dim != 7, hidden != 64, layer_N not 1 or 2, num_actions != 4; mrl_mappo_mlp_workspace_bytes refuses
 *     the same shapes, B == 0 and a NULL out. */
enum { MRL_MLPBASE_VALUE_ONLY = 4 }; /* flag of mrl_mlpbase_act, beside MRL_POLICY_GREEDY */
typedef struct mrl_mlpbase_policy {
    const float *params_dev;
    uint32_t hidden, layer_N, flags; /* flags: 0 or MRL_POLICY_GREEDY (mrl_rollout_mlpbase has no flags argument of its own) */
} mrl_mlpbase_policy;
typedef struct mrl_mlpbase_record { /* all device pointers, dense; T = num_steps */
    int32_t *actions;           /* (T, N, P) */
    float *logprobs;            /* (T, N, P) */
    float *values;              /* (T + 1, N, P) */
    float *rewards, *dones;     /* (T, N, P) */
    float *next_done;           /* (N, P) */
    float *logits;              /* (T, N, P, 4) or NULL */
    int32_t *obs;               /* (T + 1, N, P, 7) */
    uint32_t num_steps;
} mrl_mlpbase_record;
typedef struct mrl_mappo_mlp_batch {
    const int32_t *obs;          /* (S, 7) */
    const int32_t *actions;      /* (S) */
    const float *logprobs, *value_preds, *returns, *advantages; /* (S) */
    uint32_t size;               /* S */
} mrl_mappo_mlp_batch;
uint64_t mrl_mlpbase_policy_num_params(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions);
int mrl_mlpbase_act(mrl_sim *sim, uint32_t players, const mrl_mlpbase_policy *policy, const mrl_mlpbase_record *record_or_null,
                    uint32_t row, uint64_t seed, uint32_t step, uint32_t flags, void *hip_stream);
int mrl_rollout_mlpbase(mrl_sim *sim, uint32_t players, const mrl_mlpbase_policy *policy, const mrl_mlpbase_record *record,
                        uint64_t seed, uint32_t first_step, void *hip_stream);
int mrl_mappo_mlp_workspace_bytes(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions, uint32_t minibatch_size,
                                  uint32_t num_minibatches, uint64_t *out);

int mrl_mappo_mlp_update(const mrl_mlpbase_policy *policy, const mrl_mappo_optimizer *opt, const mrl_mappo_mlp_batch *batch,
                         const int32_t *indices_dev /* (K, B) */, uint32_t num_minibatches /* K */, uint32_t minibatch_size /* B */,
                         const mrl_mappo_config *cfg, float *value_norm_state_dev_or_null /* (3) */, void *workspace_dev,
                         uint64_t workspace_bytes, float *stats_dev_or_null /* (K, 8) */, float *grads_dev_or_null /* (K, P) */,
                         int gpu_id, void *hip_stream);

/* The RECURRENT MLPBase actor-critic (r_actor_critic.py with use_recurrent_policy, utils/rnn.py with recurrent_N 1): a GRU of width
 * 64 and a LayerNorm between the base and the head of both nets, through mrl_mlpbase_act, mrl_rollout_mlpbase, mrl_mappo_mlp_update
 * and the two size queries -- no new entry
 * point and no changed struct, MRL_ABI_VERSION stays 4.  DESIGN.md section 27.
 *   Network, per net, with x = the base's output row (the last hidden layer's LayerNorm output), h = the incoming state, m = 0 where
 *     DONE[world] is set at the time of the act and 1 otherwise (main_player.py:254; multiplying by m at every step equals the
 *     segment logic of rnn.py:41-69):
 *         h_in = h * m;  gi = W_ih x + b_ih;  gh = W_hh h_in + b_hh   (192 each, gate order r, z, n)
 *         r = sigmoid(gi_r + gh_r);  z = sigmoid(gi_z + gh_z);  n = tanh(gi_n + r * gh_n);  h' = (1 - z) * n + z * h_in
 *         head input = LayerNorm64(h');  new state = h' (before the LayerNorm, as rnn.py:79-80 returns it)
 *     sigmoid(x) = 1 / (1 + expf(-x)), tanh(x) = tanhf(x), one device function each.  Every 64 x 64 product follows the Linear
 *     rule above, the LayerNorm the LayerNorm rule; no float atomics; the same inputs give the same bits.
 *   Flat tensor: per net base.* exactly as above (fc_h included), then rnn.rnn.weight_ih_l0 (192, 64), weight_hh_l0 (192, 64),
 *     bias_ih_l0 (192), bias_hh_l0 (192), rnn.norm.weight (64), bias (64), then the head: 25 088 floats more per net.
 *     mrl_mlpbase_policy_num_params(7, 64, layer_N + MRL_MLPBASE_GRU_LAYERS, 4) is 77 537 for layer_N 2 and 68 961 for 1.
 *   MRL_MLPBASE_RECURRENT is a bit of mrl_mlpbase_policy.flags ONLY, never of the act's `flags` argument.  When it is set the
 *     `policy` pointer is read as an mrl_mlpbase_gru_policy and a non-NULL `record` pointer as an mrl_mlpbase_gru_record.
 *     h_actor and h_critic (N, P, 64) are the running states, read and written by the acts.
 *   Act: behind the base the workgroup of a (tile, net) loads its 32 state rows, applies m, runs the GRU, its LayerNorm and the
 *     head, and writes h' back.  Seats outside `players` keep every byte of their state rows.  With a record and row % L == 0
 *     (L = chunk_length) the INCOMING state, before the mask, goes to h0_*[row / L] ((T / L, N, P, 64)).  The closing
 *     MRL_MLPBASE_VALUE_ONLY act reads the critic's state and writes NOTHING to either state tensor (main_player.py:298 discards
 *     it: the next rollout's row 0 sees the same observation again).  Without a record only the actor runs and only h_actor
 *     advances.
 *   mrl_rollout_mlpbase: for k < T the recurrent act at row k, then the ordinary step; then the closing value-only act.  Two
 *     rollouts of T with the states carried equal one of 2 T, bit for bit (T a multiple of L).
 *   Refusals (MRL_ERR_INVALID, nothing changed) beyond mrl_mlpbase_act's: a NULL h_actor or h_critic, or one off a 4-byte boundary;
 *     with a record chunk_length == 0, num_steps % chunk_length != 0, a NULL h0_actor or h0_critic or one off a 4-byte boundary.
 *     The banks (mrl_mlpbase_act_bank, mrl_rollout_mlpbase_bank, mrl_mappo_mlp_bank_update) refuse the bit.
 *   mrl_mappo_mlp_update with the bit in policy->flags: `policy` is read as an mrl_mlpbase_gru_policy (its state pointers are not
 *     read) and `batch` as an mrl_mappo_mlp_gru_batch.  The unit of a minibatch is a CHUNK: c = (j N + n) P + p, j < T / L, covers
 *     samples s_i = ((j L + i) N + n) P + p, i < L.  `indices` is (K, Bc) chunk ids and minibatch_size = Bc; every mean of the
 *     losses runs over the Bc L samples of the row.  Per chunk the forward pass starts from h0_*[j, n, p] and applies m_i = 1 -
 *     dones[j L + i, n, p] at every step (dones[k] is what the act at row k saw), so on unchanged parameters the recomputed
 *     log-probs and values are the record's bit for bit.  Launch plan: one launch that writes every row's sample numbers and the
 *     ValueNorm recurrence up front (with MRL_MAPPO_VALUENORM), then three per row as for mrl_mappo_mlp_update.  The gradient
 *     kernel takes 32 chunks per tile: a forward sweep that keeps the incoming state of every step in the workgroup's own slice of
 *     the workspace, then a sweep from i = L - 1 down to 0 that recomputes the step's forward pass, runs the loss head for the
 *     step's 32 samples and goes back through the head, the LayerNorm, the GRU (dh carried to step i - 1 through z, W_hh and the
 *     mask) and the base.  A workgroup's partial vector is summed in ONE order: tiles ascending, within a tile the steps
 *     descending, within a step the samples ascending.  No float atomics, no wait on another workgroup; the same inputs give the
 *     same bits; a call of K rows gives the bits of K calls of one row; fc_h stays untouched.  1 <= L <=
 *     MRL_MLPBASE_GRU_MAX_CHUNK = 16.  mrl_mappo_mlp_workspace_bytes(7, 64, layer_N + MRL_MLPBASE_GRU_LAYERS, 4, Bc, K, &bytes)
 *     sizes the workspace, for any L up to the maximum.
 *     Refusals beyond mrl_mappo_mlp_update's: a NULL h0_actor, h0_critic or dones, or one off a 4-byte boundary; chunk_length 0
 *     or above the maximum; num_worlds * num_seats * (T / L) chunks inconsistent with base.size, i.e. base.size not a multiple of
 *     chunk_length * num_worlds * num_seats; minibatch_size above the batch's number of chunks.  mrl_mappo_mlp_bank_update
 *     refuses the bit.
 *   Not built: banks, population training and cross-play of recurrent policies, recurrent_N > 1, use_naive_recurrent_policy. */
enum { MRL_MLPBASE_RECURRENT = 16 };      /* bit of mrl_mlpbase_policy.flags */
enum { MRL_MLPBASE_GRU_LAYERS = 0x100 };  /* added to layer_N in the two size queries: the recurrent shape */
enum { MRL_MLPBASE_GRU_MAX_CHUNK = 16 };  /* the longest chunk mrl_mappo_mlp_update back-propagates through */
typedef struct mrl_mlpbase_gru_policy {
    mrl_mlpbase_policy base;    /* base.flags has MRL_MLPBASE_RECURRENT; base.params_dev is the recurrent flat tensor */
    float *h_actor, *h_critic;  /* (N, P, 64) */
} mrl_mlpbase_gru_policy;
typedef struct mrl_mlpbase_gru_record {
    mrl_mlpbase_record base;
    float *h0_actor, *h0_critic; /* (T / L, N, P, 64) */
    uint32_t chunk_length;       /* L */
} mrl_mlpbase_gru_record;
typedef struct mrl_mappo_mlp_gru_batch {
    mrl_mappo_mlp_batch base;                    /* base.obs .. base.advantages as for mrl_mappo_mlp_update; base.size = S = T N P */
    const float *h0_actor, *h0_critic, *dones;   /* the record's: (T / L, N, P, 64) twice and (T, N, P) */
    uint32_t chunk_length, num_worlds, num_seats; /* L, N, P */
} mrl_mappo_mlp_gru_batch;

/* A population of partners on the balance beam: a BANK of K MLPBase policies of one shape and a policy per (world, seat) cell,
 * the counterpart of mrl_cnn_bank and its calls above for the world where cross-play between trained conventions is the thing
 * measured (the reference's --seed_skip and --pop_size).  No reference counterpart as calls.  DESIGN.md section 20.
 *   Bank (mrl_mlpbase_bank): params_dev is a float32 device array of K = num_policies rows, `stride` floats apart (stride >=
 *     mrl_mlpbase_policy_num_params(7, 64, layer_N, 4)); row k is exactly an mrl_mlpbase_policy's params_dev, so mrl_mlpbase_act,
 *     mrl_mappo_mlp_update and the bank act read and write the same floats.  1 <= K <= 256.  hidden, layer_N and flags as in
 *     mrl_mlpbase_policy: one layer_N for the whole bank.
 *   Assignment: ids, int32 (N, P), device memory, the caller's, with mrl_cnn_act_bank's contract.  ids[n, p] = k >= 0: seat p of
 *     world n acts under row k.  -1 (any negative value): the cell is not acted -- its ACTION entry and its record cells,
 *     record.obs included, keep every byte.  A value >= K is outside the contract: the cell is treated as -1 and, where its seat
 *     is in `players`, counted in the workspace's out_of_range word [2].  A cell is acted when its seat's bit is set in `players`
 *     AND its id is valid.
 *   mrl_mlpbase_act_bank is the plan and the act, on hip_stream: two launches up to M = N P = 2048 cells, four beyond.  The plan
 *     is mrl_cnn_act_bank's own -- the same kernels, the same tile size of 32 and the same workspace words, described there -- and
 *     the workspace is mrl_cnn_bank_workspace_bytes(N, 2, K) bytes (mrl_mlpbase_bank_workspace_bytes(N, K) is that number).  The
 *     act is mrl_mlpbase_act's kernel body over the plan's tiles: the same LDS image, the same products in the same order, the
 *     same LayerNorm sums, the same hash of (seed, step, n, p), the same head and flags, the same OBSERVATION tensor read in
 *     place, with the tile's rows taken from the list and the parameters from params_dev + policy * stride.  A sample's arithmetic
 *     reads its own rows and the tile's common weights only, so every output is bit for bit what mrl_mlpbase_act gives that cell
 *     under that policy, whatever else shares the tile.  The grid is sized for the bound ceil(N seats / 32) + K; workgroups past
 *     `tiles` leave at once.  Record rows, the observation rows included, are written for acted cells only; values, rewards and
 *     dones come from the critic of the cell's own policy.  ids_row, (N, P) int32 or NULL, receives the ids as this act used
 *     them: k for an acted cell, -1 for every other.  No float atomics, no workgroup waits on another, no scratch.
 *   Refusals (MRL_ERR_INVALID, nothing enqueued): those of mrl_mlpbase_act; K = 0 or K > 256; stride below
 *     mrl_mlpbase_policy_num_params; NULL ids; ids or ids_row off a 4-byte boundary; a workspace below
 *     mrl_cnn_bank_workspace_bytes(N, 2, K) or off a 16-byte boundary.
 * mrl_mlpbase_bank_resample: mrl_cnn_bank_resample on a balance-beam simulator -- the same kernel, which reads DONE, the ids and
 *     the episodes only, the same mrl_cnn_resample descriptor, draws and refusals (`players` as for mrl_mlpbase_act); any other
 *     simulator is refused.
 * mrl_rollout_mlpbase_bank: mrl_rollout_mlpbase's loop with the bank act -- for k < T: the bank act at row k with step number
 *     first_step + k (ids_record row k, when given, receives that act's ids_row), the ordinary step, then, with a resample,
 *     mrl_mlpbase_bank_resample; then the closing MRL_MLPBASE_VALUE_ONLY bank act at row T (ids_record row T).  ids_record is
 *     int32 (T + 1, N, P).  No host wait inside; two rollouts of T equal one of 2 T, ids and episodes included.  With resample
 *     NULL neither ids nor episodes change (episodes may then be NULL).  Refusals: those of mrl_mlpbase_act_bank and
 *     mrl_mlpbase_bank_resample, a NULL record, NULL episodes with a resample. */
typedef struct mrl_mlpbase_bank {
    const float *params_dev;    /* (num_policies, stride) */
    uint32_t num_policies;
    uint64_t stride;            /* floats between rows */
    uint32_t hidden, layer_N, flags;
} mrl_mlpbase_bank;
uint64_t mrl_mlpbase_bank_workspace_bytes(uint32_t num_worlds, uint32_t num_policies);
int mrl_mlpbase_act_bank(mrl_sim *sim, uint32_t players, const mrl_mlpbase_bank *bank, const int32_t *ids_dev,
                         const mrl_mlpbase_record *record_or_null, int32_t *ids_row_or_null, uint32_t row, uint64_t seed, uint32_t step,
                         uint32_t flags, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream);
int mrl_mlpbase_bank_resample(mrl_sim *sim, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev, int32_t *episodes_dev,
                              void *hip_stream);
int mrl_rollout_mlpbase_bank(mrl_sim *sim, uint32_t players, const mrl_mlpbase_bank *bank, int32_t *ids_dev, int32_t *episodes_dev,
                             const mrl_cnn_resample *resample_or_null, const mrl_mlpbase_record *record, int32_t *ids_record_or_null,
                             uint64_t seed, uint32_t first_step, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream);

/* Training every member of a bank in one call: mrl_mappo_update and mrl_mappo_mlp_update with a member dimension, so that the
 * record one bank rollout wrote -- every cell under its own policy -- trains the whole population in the launches one policy
 * takes.  No reference counterpart as calls (the reference trains a population one run per seed).  DESIGN.md section 22.
 *   Bank (mrl_mappo_bank_optimizer): params_dev, exp_avg and exp_avg_sq are float32 device arrays of K = num_policies rows,
 *     row_bytes BYTES apart (one stride for all three; a multiple of 4, at least 4 P with P the policy's parameter count; a dense
 *     (K, P) tensor has row_bytes = 4 P).  Row k of params_dev is exactly what mrl_cnn_bank / mrl_mlpbase_bank call row k, and
 *     rows k of the three arrays are an mrl_mappo_optimizer's arrays: a member can also be stepped alone by the plain call.  1 <=
 *     K <= 256.  step: the Adam steps every member has taken before this call, one number for the bank.  The call trains the M =
 *     num_members consecutive rows first_member, ..., first_member + M - 1; no other row of any array is read or written.
 *     policy->params_dev must be opt->params_dev, the bank's first row, whatever first_member is.
 *   Arrays with a member dimension, member z = 0 .. M - 1 being bank row first_member + z:
 *         indices           (M, R, B) int32: row r of member z takes the samples indices[z, r, :]; R = num_minibatches and B =
 *                           minibatch_size are the same for every member
 *         value_norm_state  (K, 3) float32 or NULL: row k is bank row k's ValueNorm state (indexed by bank row, as the moments are)
 *         stats             (M, R, 8) or NULL;  grads (M, R, P) or NULL
 *         workspace         M times the plain call's: member z uses the bytes [z w, (z + 1) w), w = mrl_mappo_workspace_bytes (or
 *                           mrl_mappo_mlp_workspace_bytes) for the same shape, B and R, laid out as the plain call lays them out.
 *                           mrl_mappo_bank_workspace_bytes and mrl_mappo_mlp_bank_workspace_bytes return M w; like w it stops
 *                           growing with B at 256 partial vectors per net.
 *     The batch (the record's arrays, the observations, advantages, returns) and cfg -- both learning rates included -- are
 *     shared by all members.
 *   What a member computes: exactly the plain call on (its row of the bank and of the moments, step, its row of the ValueNorm
 *     state, indices[z], the shared batch and cfg) -- the same tiles, the same share of samples per workgroup (a function of B
 *     alone), the same chains of sums, its own two clip_grad_norm_ norms -- so bank row first_member + z, both moment rows, the
 *     ValueNorm row, stats[z] and grads[z] are bit for bit what that plain call leaves.  Members read nothing of each other.
 *   Launches: two up front with MRL_MAPPO_VALUENORM, then three per row, 2 + 3 R whatever M is: every kernel of the plain call
 *     with the member as a third grid dimension.  No float atomics, no wait between workgroups, no scratch memory: same inputs,
 *     same bits; one call of R rows gives the bits of R calls of one row.
 *   MRL_ERR_INVALID, nothing enqueued and nothing changed: everything the plain call refuses (with "opt's arrays" read as the
 *     bank's); num_members == 0; first_member + num_members > num_policies; num_policies == 0 or > 256; row_bytes below 4 P or
 *     not a multiple of 4; a workspace below M w or off a 16-byte boundary.  R == 0 enqueues nothing.  The workspace functions
 *     refuse the plain ones' shapes, num_members == 0 or > 256 and a NULL out.
 *   Not built: members with different B, learning rates or step counts; member sets that are not consecutive rows; the wide
 *     policy's bank. */
typedef struct mrl_mappo_bank_optimizer {
    float *params_dev;           /* (K, row_bytes / 4): the bank's params_dev; updated in place */
    float *exp_avg, *exp_avg_sq; /* (K, row_bytes / 4) each */
    uint64_t row_bytes;          /* bytes between rows of all three */
    uint32_t num_policies;       /* K */
    uint32_t first_member, num_members;
    uint32_t step;               /* Adam steps taken BEFORE this call, by every member */
} mrl_mappo_bank_optimizer;
int mrl_mappo_bank_workspace_bytes(uint32_t width, uint32_t height, uint32_t channels, uint32_t hidden, uint32_t minibatch_size,
                                   uint32_t num_minibatches, uint32_t num_members, uint64_t *out);
int mrl_mappo_bank_update(const mrl_mappo_policy *policy, const mrl_mappo_bank_optimizer *opt, const mrl_mappo_batch *batch,
                          const int32_t *indices_dev /* (M, R, B) */, uint32_t num_minibatches /* R */, uint32_t minibatch_size /* B */,
                          const mrl_mappo_config *cfg, float *value_norm_state_dev_or_null /* (K, 3) */, void *workspace_dev,
                          uint64_t workspace_bytes, float *stats_dev_or_null /* (M, R, 8) */, float *grads_dev_or_null /* (M, R, P) */,
                          int gpu_id, void *hip_stream);
int mrl_mappo_mlp_bank_workspace_bytes(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions, uint32_t minibatch_size,
                                       uint32_t num_minibatches, uint32_t num_members, uint64_t *out);
int mrl_mappo_mlp_bank_update(const mrl_mlpbase_policy *policy, const mrl_mappo_bank_optimizer *opt, const mrl_mappo_mlp_batch *batch,
                              const int32_t *indices_dev /* (M, R, B) */, uint32_t num_minibatches /* R */,
                              uint32_t minibatch_size /* B */, const mrl_mappo_config *cfg,
                              float *value_norm_state_dev_or_null /* (K, 3) */, void *workspace_dev, uint64_t workspace_bytes,
                              float *stats_dev_or_null /* (M, R, 8) */, float *grads_dev_or_null /* (M, R, P) */, int gpu_id,
                              void *hip_stream);

/* A population of partners for Hanabi and the balance beam under the wide policy: a BANK of K policies of mrl_agent_act's shape
 * and a policy per world for the seat that acts -- add_partner_agent's "randomly samples" a partner "at the start of every
 * episode" (pantheonrl_extension/vectorenv.py:89-98), per world.  No reference counterpart as calls.  DESIGN.md section 21.
 *   Bank (mrl_wide_bank): params_dev is a float32 device array of K = num_policies rows, `stride` floats apart (stride >=
 *     mrl_wide_policy_num_params(obs_dim, state_dim, num_actions)); row k is exactly an mrl_wide_policy's params_dev, so
 *     mrl_agent_act, mrl_agent_update and the bank act read and write the same floats.  1 <= K <= 256.
 *   Assignment: ids, int32 (N, P), device memory, the caller's; the call reads column `player`.  A world is COMPUTED when
 *     ACTIVE_AGENT[player, n] != 0, or always with MRL_AGENT_ALL_ROWS.  ids[n, player] = k, 0 <= k < K: a computed world acts
 *     under row k; one that is not computed gets action 0, exactly as mrl_agent_act writes it.  -1 (any negative value): the
 *     world's ACTION entry and its ids_row entry keep every byte.  A value >= K is outside the contract: the world is treated as
 *     -1 and counted in the workspace's out_of_range word, computed or not.
 *   mrl_agent_act_bank, on hip_stream: the effective ids (eff[n] = ids[n, player] where the world is computed or the id is not
 *     valid, -1 elsewhere; this launch also writes the action 0 of the worlds not computed), the plan over eff -- mrl_cnn_act_bank's
 *     own kernels with one seat and N cells, one launch up to 2048 worlds and three beyond --, four layer launches and the head.
 *     A layer launch is mrl_agent_act's layer kernel body over the plan's tiles: workgroup (t, slab, net) takes entry t of the tile
 *     table, its rows are list positions first .. first + rows (layer 1 gathers the worlds through the lists), its weights and
 *     bias are the layer's inside row `policy` of the bank; the grid's x extent is max_tiles = ceil(N / 32) + K and workgroups past
 *     `tiles` leave at once.  The head is mrl_agent_act's over list positions [0, acted): the same masks, the same draw
 *     policy_hash(seed, step, world, player).  Every world's logits, value and action are bit for bit what mrl_agent_act gives that
 *     world under row k alone.  flags: MRL_POLICY_GREEDY, MRL_AGENT_ALL_ROWS.  There is no record: population partners are
 *     frozen, and a learner trains a member through mrl_agent_act on its row.  ids_row, (N) int32 or NULL: k where the world
 *     acted under row k, -1 where it has a valid id and is not computed, untouched elsewhere.  No float atomics, no workgroup
 *     waits on another, no scratch: the same inputs give the same bits on every run.
 *   Workspace: mrl_agent_bank_workspace_bytes(N, K) bytes of device memory, 16-byte aligned, the caller's; holds nothing between
 *     calls.  With W = mrl_agent_workspace_bytes(N) and E = 4 N rounded up to a multiple of 256:
 *       [0, W)          mrl_agent_act's workspace, whose layout is: the world list (unused here), 4 N bytes rounded up to 256, plus
 *                       a 256-byte slot; two activation buffers of (2, N, 512) floats; the logits (N, 64) floats; the values (N)
 *                       floats, rounded up to 256 bytes.  Logits and values are indexed by POSITION IN THE PLAN'S LISTS.
 *       [W, W + E)      eff, int32 (N)
 *       [W + E, ...)    the plan's words exactly as mrl_cnn_act_bank describes them for M = N cells of one seat: [0] tiles, [1]
 *                       acted, [2] out_of_range, count[], start[], the tile table (policy, first, rows, 0), lists (worlds, every
 *                       policy's ascending), the chunk rows; mrl_cnn_bank_workspace_bytes(N, 1, K) bytes.
 *   Refusals (MRL_ERR_INVALID, nothing enqueued): those of mrl_agent_act (another game, an exchanged simulator, a capturing
 *     stream, a player beyond the seats); a NULL bank or parameter array; obs_dim, state_dim or num_actions of 0 or beyond
 *     the simulator's rows, num_actions above 64 (mrl_agent_act's rule: the rows of a Hanabi simulator are as wide as the full
 *     game's whatever its configuration, and a policy reads the head of a row); K = 0 or K > 256; stride below mrl_wide_policy_num_params; NULL ids; ids or ids_row off a 4-byte boundary; a
 *     workspace that is NULL, off a 16-byte boundary or below mrl_agent_bank_workspace_bytes; MRL_AGENT_VALUE_ONLY; unknown flags.
 * mrl_agent_bank_workspace_bytes: writes the size to *out; MRL_ERR_INVALID for K = 0, K > 256 or a NULL out.
 * mrl_agent_bank_resample: mrl_cnn_bank_resample on a Hanabi or balance-beam simulator -- the same kernel, which reads DONE, the
 *     ids and the episodes only, the same mrl_cnn_resample descriptor, draws and refusals; `players` is a mask of seats; any other
 *     simulator is refused. */
typedef struct mrl_wide_bank {
    const float *params_dev;    /* (num_policies, stride) */
    uint32_t num_policies;
    uint64_t stride;            /* floats between rows */
    uint32_t obs_dim, state_dim, num_actions;
} mrl_wide_bank;
int mrl_agent_bank_workspace_bytes(uint32_t num_worlds, uint32_t num_policies, uint64_t *out);
int mrl_agent_act_bank(mrl_sim *sim, uint32_t player, const mrl_wide_bank *bank, const int32_t *ids_dev /* (N, P) */,
                       int32_t *ids_row_or_null /* (N) */, uint64_t seed, uint32_t step, uint32_t flags, void *workspace_dev,
                       uint64_t workspace_bytes, void *hip_stream);
int mrl_agent_bank_resample(mrl_sim *sim, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev, int32_t *episodes_dev,
                            void *hip_stream);

int mrl_tensor(mrl_sim *sim, int slot, mrl_tensor_desc *out);
int mrl_game(const mrl_sim *sim);
uint32_t mrl_num_worlds(const mrl_sim *sim);
/* name of the dominant kernel of this simulator's step, as rocprofv3 prints it */
const char *mrl_kernel_name(const mrl_sim *sim);
/* name of the kernel the next mrl_rollout_random will run: a persistent one ("mrl_hanabi_rollout", "mrl_cartpole_rollout":
 * all steps in one cooperative launch) while the device can hold the whole grid at once, otherwise mrl_kernel_name's, once per
 * step.  A cooperative launch the runtime refuses switches the simulator to the latter for good; tests and benchmarks read
 * this to know which of the two they are looking at. */
const char *mrl_rollout_kernel_name(const mrl_sim *sim);
/* algorithmic HBM bytes one step moves per world */
uint64_t mrl_bytes_per_world_step(const mrl_sim *sim);
void mrl_destroy(mrl_sim *sim);

/* Test and measurement knobs, consulted by every LATER mrl_*_create until they are forgotten again (the library reads no
 * environment variable).  They are process-global: set them, create, forget them -- the Python binding's `debug_knobs`
 * context manager does exactly that, also when the create throws.  Keys (with their meanings: csrc/capi.hip, kDebugKeys):
 * overcooked.wpw, overcooked.whole_max, overcooked.lds_max, overcooked.share_max_players, overcooked.share_private,
 * overcooked.no_share, overcooked.lds_pad, overcooked.no_fixed, overcooked.no_direct, overcooked.whole_store,
 * overcooked.store_policy, overcooked.wide_rollout, overcooked.writeback, overcooked.groups, overcooked.shared_consts, overcooked.variant,
 * hanabi.variant, hanabi.pairing, hanabi.no_persistent, cartpole.no_persistent, cartpole.persistent_max, cartpole.variant, fused_step (0 the library's choice, 1 one launch,
 * 2 two launches), fused_heal_test, inject_scan_timeout, and (diagnostic build) ablate, stamps.  key == NULL forgets all of
 * them.  Unknown key: MRL_ERR_INVALID.  No reference counterpart (the reference has MADRONA_* environment variables for its
 * JIT cache only). */
int mrl_debug_set(const char *key, int64_t value);

/* Measurement aid for bench.py's roofline.peak_measured: one float4 stream over caller buffers on
 * device gpu_id, enqueued on hip_stream.  mode 0: copy src -> dst (reads + writes bytes each);
 * mode 1: fill dst, plain stores; mode 2: fill dst, write-through (sc1) stores like the step
 * kernels' observation stream; modes 3 / 4: mode 2's bytes and stores in two passes inside one launch, first the aligned
 * 64-byte (3) / 128-byte (4) blocks of a fixed pseudo-random quarter of the block indices, then the rest.
 * bytes: multiple of 16, buffers 16-byte aligned.  No reference counterpart. */
int mrl_probe_stream(void *dst_dev, const void *src_dev, uint64_t bytes, int mode, int gpu_id, void *hip_stream);

/* message of the last failing call on this thread ("" if none) */
const char *mrl_last_error(void);
int mrl_abi_version(void);
/* Which sources this binary was built from: the first 16 hex digits of a sha256 over the .hip and .hpp files of csrc/, its
 * Makefile and this header (the Makefile computes it and compiles it in; the Python binding computes the same value from the files
 * lying beside the library and refuses a library whose hash differs).  Measurements that cannot be taken inside a benchmark
 * run (PMC traffic, profiles/step_traffic.json) are keyed by it.  No reference counterpart. */
const char *mrl_build_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* MRL_ENVS_H */
