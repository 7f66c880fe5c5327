// mrl_agent_act, mrl_agent_credit and mrl_gae_active: what the reference's CleanPPOAgent does around env.step for Hanabi and
// the balance beam (pantheonrl_extension/vectoragent.py:197-262, :352-372), without the host in the loop
// (include/mrl_envs.h).
//
// One act is seven launches on one stream:
//   mrl_wide_rows      one workgroup turns ACTIVE_AGENT[player, :] into the ascending list of worlds to compute and its length
//                      (an integer prefix sum: the same list on every run); with MRL_AGENT_ALL_ROWS the list is 0..N-1.
//   mrl_agent_book     a lane per world: the per-world rows of the record, zeros for the worlds not computed; then the grid
//                      copies the observation, state and mask rows in their own element types.
//   mrl_wide_layer x4  out = act(bias + in W^T) for a 32-row x 128-column tile per workgroup, grid = (row tile, column slab,
//                      net).  Each of the four wavefronts owns a 32 x 32 tile of v_mfma_f32_32x32x2_f32: lane (r, half) feeds
//                      A[row r][k = 2 kk + half] and B[k][column r], so an output is 0, then fmaf over k ascending, and the
//                      bias is added to the finished sum (a chain begun at the bias rounds every product at the bias's
//                      ulp: DESIGN.md section 14).  The operands go through LDS in chunks of 64 k (rows 66 floats
//                      apart: lane r reads bank 2 r + half, no conflict), the next chunk's global loads are issued before the current chunk's products.  Layer 1
//                      reads the simulator's tensors themselves (int8 / int32, row-strided) through the world list; layers
//                      2-4 read the previous layer's activations from the workspace, which stays in L2.
//   mrl_agent_head     a lane per computed world: mask, soft-max, draw, log-prob; three passes over the world's <= 64 logits in
//                      the workspace instead of an array in registers (a dynamically indexed array would go to scratch).
// No float atomics, no workgroup waits on another, no scratch: the same inputs give the same bits on every run.
// The four layer launches are launch_wide_forward, which mrl_agent_update (wide_update.hip) also runs, over the record's rows:
// the log-probs and values an update recomputes on unchanged parameters carry the record's bits.
#include "wide_layer_body.hpp"

namespace mrl {

// ---------------------------------------------------------------- the world list

__global__ void __launch_bounds__(1024) mrl_wide_rows(WideInput active, uint32_t num_worlds, uint32_t all_rows,
                                                      uint32_t *__restrict__ rows, uint32_t *__restrict__ count)
{
    __shared__ uint32_t wave_total[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t base = 0;
    for (uint32_t start = 0; start < num_worlds; start += 1024u) {
        const uint32_t w = start + tid;
        const bool take = w < num_worlds && (all_rows || wide_nonzero(active, (int64_t)w * active.row_stride));
        const unsigned long long votes = __ballot(take);
        const uint32_t before = __popcll(votes & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[wave] = __popcll(votes);
        __syncthreads();
        uint32_t lower = 0, total = 0;
#pragma unroll
        for (uint32_t v = 0; v < 16; v++) {
            const uint32_t c = wave_total[v];
            lower += v < wave ? c : 0u;
            total += c;
        }
        if (take) rows[base + lower + before] = w;  // base + lower + before < number of taken worlds <= num_worlds
        base += total;
        __syncthreads();
    }
    if (tid == 0) *count = base;
}

// ---------------------------------------------------------------- per-world rows of the record and the copies

struct BookArgs {
    WideInput obs, state, mask, active;
    int32_t *action;
    int64_t action_stride;
    mrl_agent_record rec;
    uint32_t has_record, row, flags, D, S, A, num_worlds;
};

template <typename T>
__device__ __forceinline__ void copy_rows(T *__restrict__ dst, const WideInput &src, uint64_t num_worlds, uint32_t width)
{
    const uint64_t total = num_worlds * width, stride = (uint64_t)gridDim.x * blockDim.x;
    const T *__restrict__ from = static_cast<const T *>(src.data);
    for (uint64_t at = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; at < total; at += stride) {
        const uint64_t w = at / width, k = at - w * width;
        dst[at] = from[(int64_t)w * src.row_stride + (int64_t)k];
    }
}

__device__ __forceinline__ uint32_t elem_bytes(uint32_t type) { return type == MRL_INT8 || type == MRL_UINT8 ? 1u : 4u; }

__global__ void __launch_bounds__(256) mrl_agent_book(BookArgs a)
{
    const uint64_t N = a.num_worlds, stride = (uint64_t)gridDim.x * blockDim.x;
    const bool value_only = a.flags & MRL_AGENT_VALUE_ONLY, all_rows = a.flags & MRL_AGENT_ALL_ROWS;
    const mrl_agent_record &r = a.rec;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < N; w += stride) {
        const bool active = wide_nonzero(a.active, (int64_t)w * a.active.row_stride);
        const bool computed = active || all_rows;
        if (value_only) {
            r.next_active[w] = active ? 1 : 0;
            if (!computed) r.next_value[w] = 0.0f;
            continue;
        }
        if (!computed) a.action[(int64_t)w * a.action_stride] = 0;
        if (!a.has_record) continue;
        const uint64_t at = (uint64_t)a.row * N + w;
        if (!computed) {
            r.actions[at] = 0;
            r.logprobs[at] = 0.0f;
            r.values[at] = 0.0f;
        }
        r.active[at] = active ? 1 : 0;
        r.dones[at] = r.next_done[w] ? 1.0f : 0.0f;
        r.next_done[w] = 0;
        r.rewards[at] = 0.0f;
        if (active) {
            r.last_active[w] = (int32_t)a.row;
            r.new_game[w] = 0;
        }
    }
    if (!a.has_record || value_only) return;
    if (elem_bytes(a.obs.type) == 1)
        copy_rows(static_cast<uint8_t *>(r.obs) + (uint64_t)a.row * N * a.D, a.obs, N, a.D);
    else
        copy_rows(static_cast<uint32_t *>(r.obs) + (uint64_t)a.row * N * a.D, a.obs, N, a.D);
    if (elem_bytes(a.state.type) == 1)
        copy_rows(static_cast<uint8_t *>(r.states) + (uint64_t)a.row * N * a.S, a.state, N, a.S);
    else
        copy_rows(static_cast<uint32_t *>(r.states) + (uint64_t)a.row * N * a.S, a.state, N, a.S);
    uint8_t *__restrict__ masks = r.action_masks + (uint64_t)a.row * N * a.A;
    for (uint64_t at = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; at < N * a.A; at += stride) {
        const uint64_t w = at / a.A, k = at - w * a.A;
        masks[at] = wide_nonzero(a.mask, (int64_t)w * a.mask.row_stride + (int64_t)k) ? 1 : 0;
    }
}

// ---------------------------------------------------------------- one matrix layer and the head (wide_layer_body.hpp)

__global__ void __launch_bounds__(64) mrl_agent_head(HeadArgs a)
{
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= *a.count) return;
    wide_head_body(a, j, a.rows[j]);
}

void launch_wide_forward(const WideForwardArgs &g, hipStream_t stream)
{
    const uint32_t row_tiles = (g.max_rows + kTileRows - 1) / kTileRows;
    for (uint32_t layer = 0; layer < 4; layer++)
        hipLaunchKernelGGL(mrl_wide_layer<WidePlainTiles>, dim3(row_tiles, wide_layer_slabs(layer), g.nets), dim3(kLayerThreads), 0, stream,
                           wide_layer_args(g, layer), WidePlainTiles{});
    MRL_HIP(hipGetLastError());
}

void launch_agent_act(const AgentActArgs &g, hipStream_t stream)
{
    const uint32_t N = g.num_worlds;
    if (N == 0) return;
    const bool value_only = g.flags & MRL_AGENT_VALUE_ONLY;
    hipLaunchKernelGGL(mrl_wide_rows, dim3(1), dim3(1024), 0, stream, g.active, N, g.flags & MRL_AGENT_ALL_ROWS ? 1u : 0u, g.ws.rows,
                       g.ws.count);

    BookArgs book{};
    book.obs = g.obs, book.state = g.state, book.mask = g.mask, book.active = g.active;
    book.action = g.action, book.action_stride = g.action_stride;
    if (g.record) book.rec = *g.record;
    book.has_record = g.record ? 1u : 0u;
    book.row = g.row, book.flags = g.flags, book.D = g.D, book.S = g.S, book.A = g.A, book.num_worlds = N;
    const uint64_t copied = g.record && !value_only ? (uint64_t)N * (g.S > g.D ? g.S : g.D) : N;
    const uint32_t book_blocks = (uint32_t)((copied + 255) / 256 < 2048 ? (copied + 255) / 256 : 2048);
    hipLaunchKernelGGL(mrl_agent_book, dim3(book_blocks), dim3(256), 0, stream, book);

    WideForwardArgs fwd{};
    fwd.params = g.params, fwd.obs = g.obs, fwd.state = g.state;
    fwd.D = g.D, fwd.S = g.S, fwd.A = g.A, fwd.max_rows = N, fwd.nets = value_only ? 1u : 2u;
    fwd.rows = g.ws.rows, fwd.count = g.ws.count;
    for (uint32_t net = 0; net < 2; net++)
        for (uint32_t layer = 0; layer < 3; layer++) fwd.hidden[net][layer] = g.ws.hidden[layer & 1u] + (uint64_t)net * N * kWideHidden;
    fwd.logits = g.ws.logits, fwd.value = g.ws.value;
    launch_wide_forward(fwd, stream);

    HeadArgs head{};
    head.rows = g.ws.rows, head.count = g.ws.count, head.logits = g.ws.logits, head.value = g.ws.value;
    head.mask = g.mask, head.action = g.action, head.action_stride = g.action_stride;
    if (g.record) head.rec = *g.record;
    head.has_record = g.record ? 1u : 0u;
    head.row = g.row, head.flags = g.flags, head.A = g.A, head.num_worlds = N, head.player = g.player, head.step = g.step;
    head.seed = g.seed;
    hipLaunchKernelGGL(mrl_agent_head, dim3((N + 63) / 64), dim3(64), 0, stream, head);
    MRL_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- update(): reward bookkeeping

// vectoragent.py:197-219 with a lane per world; workgroup b owns worlds [1024 b, 1024 b + 1024) and row b of the totals
__global__ void __launch_bounds__(1024) mrl_agent_credit(mrl_agent_record r, const float *__restrict__ rewards,
                                                         const int32_t *__restrict__ dones, uint32_t num_worlds)
{
    __shared__ double sum[1024];
    __shared__ float low[1024], high[1024];
    __shared__ uint32_t finished[1024];
    const uint32_t tid = threadIdx.x, w = blockIdx.x * 1024u + tid;
    double mine = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    uint32_t fin = 0;
    if (w < num_worlds) {
        const float reward = rewards[w];
        const bool done = dones[w] != 0;
        const float running = r.running_rewards[w] + reward;
        const uint32_t credited = (uint32_t)r.last_active[w];  // a row mrl_agent_act wrote, or the caller's initial 0
        if (credited < r.num_steps) {
            float *cell = r.rewards + (uint64_t)credited * num_worlds + w;
            *cell = *cell + (r.new_game[w] ? 0.0f : reward);
        }
        if (done) {
            r.next_done[w] = 1;
            r.new_game[w] = 1;
            mine = running, lo = hi = running, fin = 1;
        }
        r.running_rewards[w] = done ? 0.0f : running;
    }
    sum[tid] = mine, low[tid] = lo, high[tid] = hi, finished[tid] = fin;
    __syncthreads();
    for (uint32_t step = 512; step > 0; step >>= 1) {  // a fixed tree: the same bits on every run
        if (tid < step) {
            sum[tid] += sum[tid + step];
            low[tid] = fminf(low[tid], low[tid + step]);
            high[tid] = fmaxf(high[tid], high[tid + step]);
            finished[tid] += finished[tid + step];
        }
        __syncthreads();
    }
    if (tid == 0 && finished[0]) {
        double *t = r.totals + 4 * (size_t)blockIdx.x;
        t[0] += (double)finished[0];
        t[1] += sum[0];
        t[2] = t[2] < (double)low[0] ? t[2] : (double)low[0];
        t[3] = t[3] > (double)high[0] ? t[3] : (double)high[0];
    }
}

void launch_agent_credit(const mrl_agent_record &record, const float *rewards, const int32_t *dones, uint32_t num_worlds,
                         hipStream_t stream)
{
    if (num_worlds == 0) return;
    hipLaunchKernelGGL(mrl_agent_credit, dim3((num_worlds + 1023) / 1024), dim3(1024), 0, stream, record, rewards, dones, num_worlds);
    MRL_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- activity-masked advantages

// t* = min over worlds of first[w] (include/mrl_envs.h); *first_step was set to 0x7f7f7f7f in front of the launch
__global__ void __launch_bounds__(256) mrl_gae_first(const uint8_t *__restrict__ active, const uint8_t *__restrict__ next_active,
                                                     uint32_t num_steps, uint32_t num_worlds, int32_t *first_step)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    int32_t first = 0x7f7f7f7f;
    if (w < num_worlds) {
        first = -1;
        if (next_active[w]) {
            first = (int32_t)num_steps;
        } else {
            for (uint32_t t = num_steps; t-- > 0;)
                if (active[(uint64_t)t * num_worlds + w]) {
                    first = (int32_t)t;
                    break;
                }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int32_t other = __shfl_xor(first, d);
        first = other < first ? other : first;
    }
    if ((threadIdx.x & 63u) == 0) atomicMin(first_step, first);
}

__global__ void __launch_bounds__(256) mrl_gae_active(mrl_agent_record r, const float *__restrict__ next_value,
                                                      const uint8_t *__restrict__ next_active, float gamma, float gamma_lambda,
                                                      float *__restrict__ advantages, float *__restrict__ returns)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x, N = r.num_worlds;
    if (w >= N) return;
    const int32_t coupled_from = *r.first_step;  // t*: at every t >= t* only the worlds being bootstrapped are computed
    bool boot = next_active[w] != 0;
    float nnt = boot ? 1.0f - (r.next_done[w] ? 1.0f : 0.0f) : 0.0f;
    float nv = boot ? next_value[w] : 0.0f;
    float last = 0.0f;
    for (uint32_t t = r.num_steps; t-- > 0;) {
        const uint64_t at = (uint64_t)t * N + w;
        const float v = r.values[at];
        float adv = 0.0f;
        if (r.active[at]) {
            if (!boot || (int32_t)t < coupled_from) {
                const float delta = r.rewards[at] + gamma * nv * nnt - v;
                adv = last = delta + gamma_lambda * nnt * last;
            }
            if (!boot) {  // the reference clears the flag through a view of the mask its last two lines index with: nnt and nv stay 0
                r.active[at] = 0;
                boot = true;
            } else {
                nnt = 1.0f - r.dones[at];
                nv = v;
            }
        }
        advantages[at] = adv;
        returns[at] = adv + v;
    }
}

void launch_gae_active(const mrl_agent_record &record, const float *next_value, const uint8_t *next_active, float gamma, float lambda,
                       float *advantages, float *returns, hipStream_t stream)
{
    const uint32_t N = record.num_worlds;
    if (N == 0) return;
    const float gamma_lambda = (float)((double)gamma * (double)lambda);
    MRL_HIP(hipMemsetAsync(record.first_step, 0x7f, sizeof(int32_t), stream));
    hipLaunchKernelGGL(mrl_gae_first, dim3((N + 255) / 256), dim3(256), 0, stream, record.active, next_active, record.num_steps, N,
                       record.first_step);
    hipLaunchKernelGGL(mrl_gae_active, dim3((N + 255) / 256), dim3(256), 0, stream, record, next_value, next_active, gamma, gamma_lambda,
                       advantages, returns);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
