// Recurrent language-model scorer of the LRS beam search (syncvsr_amd/lrs_lm.py RNNLM; reference
// LRS/video/espnet/nets/pytorch_backend/lm/default.py: stacked nn.LSTMCell / nn.GRUCell), gfx950, wave64.
//   * k_rnn_cell: ONE layer of ONE step for all R live hypotheses: gathers its input rows (the embedding row of each hypothesis' token,
//     or the bf16 output rows of the layer below) and the previous state rows through the parent index of the last selection, contracts
//     [x | h_prev] against the gate weights with MFMA, and applies the gates in the accumulator registers.
// Small M (R <= a few hundred), weight streaming: a workgroup owns 16 units and ALL their gates, so that a lane's accumulators hold every gate
// of its (hypothesis, unit) pairs — no pre-activation tensor, no second pass.  No LDS (no operand is shared between waves: each wave owns
// whole 16-row tiles), no atomics; every output is a pure function of the inputs.
#include "common.h"

#define RNN_MT 5                 // 16-row tiles a wave carries through one sweep over the weights (4 waves * 5 * 16 = 320 rows per sweep)
#define RNN_MAX_DIM 4096         // padded embed / unit width the entry point takes
#define RNN_MAX_ROWS 65536

// Packed weights (RNNLM.pack_cell): bf16 [Up / 16 unit tiles][Kp / 32 k-steps][G gates][64 lanes][8], the B fragment of
// mfma_f32_16x16x32_bf16 as lane l reads it: W_g[unit 16 t + (l & 15)][k = 32 s + 8 (l >> 4) + j], k over [x (Ep) | h_prev (Up)], zero-padded.
// G = 4 (LSTM: i, f, g, o) or 3 (GRU: r, z, n).  bias fp32 [Up / 16][4][16]: LSTM b_ih + b_hh per gate; GRU r, z summed, then b_in, b_hn.
__device__ __forceinline__ float tanh_fast(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

__device__ __forceinline__ bf16x8 frag_from_f32(const float* p) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    u32x4 v;
    v.x = pack2bf(a[0], a[1]); v.y = pack2bf(a[2], a[3]); v.z = pack2bf(b[0], b[1]); v.w = pack2bf(b[2], b[3]);
    return __builtin_bit_cast(bf16x8, v);
}

template <int GRU>
__global__ __launch_bounds__(256) void k_rnn_cell(const bf16_t* __restrict__ wpk, const float* __restrict__ bias, const bf16_t* __restrict__ x,
                                                  long x_pitch, int x_rows, const int64_t* __restrict__ xidx, long xidx_stride,
                                                  const float* __restrict__ h_prev, const float* __restrict__ c_prev,
                                                  const int64_t* __restrict__ src, int prev_rows, float* __restrict__ h_out,
                                                  float* __restrict__ c_out, bf16_t* __restrict__ h16_out, int R, int Ep, int Up, int U) {
    constexpr int G = GRU ? 3 : 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ut = blockIdx.x;                               // unit tile
    const int ksx = Ep >> 5, ksh = Up >> 5;
    const int row_tiles = (R + 15) >> 4;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const u32x4* wt = reinterpret_cast<const u32x4*>(wpk) + (long)ut * (ksx + ksh) * G * 64 + lane;
    const int arow = lane & 15, kq = (lane >> 4) * 8;        // A fragment: row of the tile, first of this lane's 8 k
    const int u = ut * 16 + (lane & 15);                     // C/D: column = unit, rows (lane >> 4) * 4 + i
    float bs[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bs[g] = bias[(ut * 4 + g) * 16 + (lane & 15)];

    for (int t0 = wave; t0 < row_tiles; t0 += 4 * RNN_MT) {  // (wave-uniform: whole waves leave; nothing synchronises across waves)
        const bf16_t* xp[RNN_MT];
        const float* hp[RNN_MT];
#pragma unroll
        for (int m = 0; m < RNN_MT; ++m) {
            const int r = (t0 + 4 * m) * 16 + arow;
            xp[m] = nullptr;
            hp[m] = nullptr;
            if (r < R) {
                const int64_t xi = xidx ? xidx[(long)r * xidx_stride] : (int64_t)r;
                if (xi >= 0 && xi < x_rows) xp[m] = x + xi * x_pitch + kq;
                const int64_t s = src ? src[r] : -1;
                if (s >= 0 && s < prev_rows) hp[m] = h_prev + s * Up + kq;
            }
        }
        f32x4 acc[RNN_MT][4];
#pragma unroll
        for (int m = 0; m < RNN_MT; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[m][g] = f32x4{0.f, 0.f, 0.f, 0.f};

        const u32x4* w = wt;
#pragma unroll 2
        for (int s = 0; s < ksx; ++s, w += G * 64) {         // x range: GRU's n gate goes to accumulator 2 (W_in x)
            bf16x8 b[G];
#pragma unroll
            for (int g = 0; g < G; ++g) b[g] = __builtin_bit_cast(bf16x8, w[g * 64]);
#pragma unroll
            for (int m = 0; m < RNN_MT; ++m) {
                if (t0 + 4 * m < row_tiles) {
                    const bf16x8 a = xp[m] ? __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(xp[m] + s * 32)) : zero8;
#pragma unroll
                    for (int g = 0; g < G; ++g) acc[m][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[g], acc[m][g], 0, 0, 0);
                }
            }
        }
#pragma unroll 2
        for (int s = 0; s < ksh; ++s, w += G * 64) {         // h range: GRU's n gate goes to accumulator 3 (W_hn h_prev)
            bf16x8 b[G];
#pragma unroll
            for (int g = 0; g < G; ++g) b[g] = __builtin_bit_cast(bf16x8, w[g * 64]);
#pragma unroll
            for (int m = 0; m < RNN_MT; ++m) {
                if (t0 + 4 * m < row_tiles) {
                    const bf16x8 a = hp[m] ? frag_from_f32(hp[m] + s * 32) : zero8;
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const int ag = (GRU && g == 2) ? 3 : g;
                        acc[m][ag] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[g], acc[m][ag], 0, 0, 0);
                    }
                }
            }
        }

#pragma unroll
        for (int m = 0; m < RNN_MT; ++m) {
            if (t0 + 4 * m >= row_tiles) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = (t0 + 4 * m) * 16 + (lane >> 4) * 4 + i;
                if (r >= R) continue;
                const int64_t s = src ? src[r] : -1;
                const bool live = s >= 0 && s < prev_rows;
                float h, c = 0.f;
                if (GRU) {
                    const float hprev = live ? h_prev[s * Up + u] : 0.f;
                    const float rg = sigmoid_fast(acc[m][0][i] + bs[0]), zg = sigmoid_fast(acc[m][1][i] + bs[1]);
                    const float ng = tanh_fast((acc[m][2][i] + bs[2]) + rg * (acc[m][3][i] + bs[3]));
                    h = (1.0f - zg) * ng + zg * hprev;
                } else {
                    const float cprev = live ? c_prev[s * Up + u] : 0.f;
                    const float ig = sigmoid_fast(acc[m][0][i] + bs[0]), fg = sigmoid_fast(acc[m][1][i] + bs[1]);
                    const float gg = tanh_fast(acc[m][2][i] + bs[2]), og = sigmoid_fast(acc[m][3][i] + bs[3]);
                    c = fg * cprev + ig * gg;
                    h = og * tanh_fast(c);
                }
                if (u >= U) { h = 0.f; c = 0.f; }            // the padded units stay exact zeros, whatever the packed weights hold there
                const long o = (long)r * Up + u;
                h_out[o] = h;
                if (!GRU) c_out[o] = c;
                if (h16_out) h16_out[o] = f2bf(h);
            }
        }
    }
}

extern "C" int svsr_rnn_cell_step(int gru, const void* wpk, const float* bias, const void* x, int64_t x_pitch, int x_rows, const int64_t* xidx,
                                  int64_t xidx_stride, const float* h_prev, const float* c_prev, const int64_t* src, int prev_rows, float* h_out,
                                  float* c_out, void* h16_out, int R, int Ep, int Up, int U, hipStream_t stream) {
    if (gru != 0 && gru != 1) return SVSR_ERR_ARG;
    if (R < 1 || R > RNN_MAX_ROWS || Ep < 64 || Up < 64 || Ep % 64 != 0 || Up % 64 != 0 || Ep > RNN_MAX_DIM || Up > RNN_MAX_DIM) return SVSR_ERR_ARG;
    if (U < 1 || U > Up || x_rows < 1 || x_pitch < Ep || x_pitch % 8 != 0 || prev_rows < 0) return SVSR_ERR_ARG;
    if (!wpk || !bias || !x || !h_out || (!gru && !c_out)) return SVSR_ERR_ARG;
    if (src && (prev_rows < 1 || !h_prev || (!gru && !c_prev))) return SVSR_ERR_ARG;
    if (xidx && xidx_stride < 1) return SVSR_ERR_ARG;
    if ((((uintptr_t)wpk | (uintptr_t)x | (uintptr_t)h_prev) & 15) != 0) return SVSR_ERR_ARG;      // 16-byte fragment loads
    if (h_out == h_prev || (c_out && c_out == c_prev)) return SVSR_ERR_ARG;                        // other workgroups still read the old rows
    const dim3 grid((unsigned)(Up / 16)), block(256);
    if (gru)
        hipLaunchKernelGGL(k_rnn_cell<1>, grid, block, 0, stream, (const bf16_t*)wpk, bias, (const bf16_t*)x, (long)x_pitch, x_rows, xidx, (long)xidx_stride,
                           h_prev, c_prev, src, prev_rows, h_out, c_out, (bf16_t*)h16_out, R, Ep, Up, U);
    else
        hipLaunchKernelGGL(k_rnn_cell<0>, grid, block, 0, stream, (const bf16_t*)wpk, bias, (const bf16_t*)x, (long)x_pitch, x_rows, xidx, (long)xidx_stride,
                           h_prev, c_prev, src, prev_rows, h_out, c_out, (bf16_t*)h16_out, R, Ep, Up, U);
    return svsr_check_launch();
}
