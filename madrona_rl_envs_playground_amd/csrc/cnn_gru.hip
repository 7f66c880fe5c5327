// mrl_cnn_gru_act: mrl_cnn_act for the recurrent actor-critic (cnn_gru.hpp; include/mrl_envs.h, MRL_CNN_RECURRENT; DESIGN.md
// section 28), ONE launch per act.  Tiles and workgroups are mrl_cnn_act's: a workgroup of four wavefronts runs one net for a tile
// of 32 samples, blockIdx.y chooses the net.  In order:
//   1. CNNBase into LDS (cnn_gru_base: mrl_cnn_act's own device functions), which leaves h2 in region A;
//   2. the tile's cell and mask words, then its 32 state rows -- into the GRU image, which overlays the convolution's dead operands
//      and the activation image from kCnnFcBytes on (cnn_gru.hpp) --, written to the record's h0 row where the act starts a chunk
//      (the incoming state, before the mask) and multiplied by the mask from DONE[world];
//   3. the GRU and its LayerNorm (gru_step_forward, the beam's own), h' back to the state tensor -- except in the closing value-only
//      act, which changes neither state tensor --, the head and the plain act's tail (same hash, same record row).
// A thread reads and writes the state elements it owns (tid, tid + 256, ...); samples outside `players` are no row of any tile, so
// their state rows keep every byte.  No float atomics, no workgroup waits on another: the same inputs give the same bits.
#include "cnn_gru.hpp"

namespace mrl {

extern __shared__ __attribute__((aligned(16))) unsigned char cnn_gru_lds_image[];

__global__ void __launch_bounds__(kCnnThreads) mrl_cnn_gru_act(CnnGruActArgs g)
{
    const CnnActArgs &a = g.act;
    const uint32_t net = act_net(a);
    const uint32_t tid = threadIdx.x;
    const uint32_t S = a.W * a.H * a.F, out_dim = net ? 1u : kCnnActions;
    const CnnGruNetAt at = cnn_gru_net_at(a.lds.k1, kCnnChannels * a.lds.npos, out_dim);
    const float *__restrict__ params = a.params + (net ? cnn_gru_net_params(a.W, a.H, a.F, kCnnActions) : 0);
    const uint32_t tile0 = blockIdx.x * kCnnTile, total = a.num_worlds * a.num_seats;

    unsigned char *lds = cnn_gru_lds_image;
    // a row of the tile in the simulator's slab, or nullptr where the tile has no such row
    const auto row_address = [&](uint32_t rr) -> const uint8_t * {
        if (tile0 + rr >= total) return nullptr;
        uint32_t world, seat;
        seat_sample(a.players, a.num_seats, tile0 + rr, world, seat);
        return reinterpret_cast<const uint8_t *>(a.obs) + ((size_t)world * a.P + seat) * S;
    };
    cnn_gru_base(a, lds, row_address, nullptr, params, at, tid);

    // the convolution's operands and the activation image are dead: the GRU image takes their place
    float *chunk = reinterpret_cast<float *>(lds + kCnnChunkAt), *h2 = reinterpret_cast<float *>(lds + kCnnH2At);
    float *outs = reinterpret_cast<float *>(lds + kCnnOutAt), *img = reinterpret_cast<float *>(lds + kCnnFcBytes);
    uint32_t *cell = reinterpret_cast<uint32_t *>(img + kGruImgCell);
    float *keep = img + kGruImgKeep, *hin = img + kGruImgHin;
    if (tid < kCnnTile) {
        uint32_t c = kGruAbsent;
        float m = 0.0f;
        if (tile0 + tid < total) {
            uint32_t world, seat;
            seat_sample(a.players, a.num_seats, tile0 + tid, world, seat);
            c = world * a.P + seat;
            m = a.done[world] != 0 ? 0.0f : 1.0f;
        }
        cell[tid] = c;
        keep[tid] = m;
    }
    __syncthreads();
    // the tile's state rows: the incoming state to the record where a chunk starts, then h * m
    float *__restrict__ state = g.h[net], *__restrict__ h0 = g.h0_row[net];
    for (uint32_t idx = tid; idx < kGruTileFloats; idx += kCnnThreads) {
        const uint32_t rr = idx >> 6, col = idx & 63u, c = cell[rr];
        float v = 0.0f;
        if (c != kGruAbsent) {
            v = state[(size_t)c * kCnnHidden + col];
            if (h0) h0[(size_t)c * kCnnHidden + col] = v;
            v *= keep[rr];
        }
        hin[rr * kGruLd + col] = v;
    }
    __syncthreads();
    gru_step_forward(params + at.gru, h2, chunk, img, tid);
    if (g.write_state) {
        for (uint32_t idx = tid; idx < kGruTileFloats; idx += kCnnThreads) {
            const uint32_t rr = idx >> 6, col = idx & 63u, c = cell[rr];
            if (c != kGruAbsent) state[(size_t)c * kCnnHidden + col] = hin[rr * kGruLd + col];
        }
    }
    gru_step_head(params + at.head_w, out_dim, chunk, img, outs, tid);

    if (tid >= kCnnTile || tile0 + tid >= total) return;
    uint32_t world, seat;
    seat_sample(a.players, a.num_seats, tile0 + tid, world, seat);
    act_tail<(int)kCnnActions>(a, outs, net, tid, world, seat, a.reward);
}

void launch_cnn_gru_act(const CnnGruActArgs &args, hipStream_t stream)
{
    const uint64_t total = (uint64_t)args.act.num_worlds * args.act.num_seats;
    if (total == 0 || args.act.nets == 0) return;
    const uint32_t bytes = cnn_gru_act_lds_bytes(args.act.lds);
    allow_large_dynamic_lds<&mrl_cnn_gru_act>(bytes);
    const dim3 grid((uint32_t)((total + kCnnTile - 1) / kCnnTile), args.act.nets == 3u ? 2u : 1u);
    hipLaunchKernelGGL(mrl_cnn_gru_act, grid, dim3(kCnnThreads), bytes, stream, args);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
