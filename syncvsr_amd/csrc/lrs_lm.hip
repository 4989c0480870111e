// Transformer language-model scorer of the LRS beam search (syncvsr_amd/lrs_lm.py; reference
// LRS/video/espnet/nets/pytorch_backend/lm/transformer.py), gfx950, wave64:
//   * k_mha_table: self-attention over an append-only pool of q | k | v rows that is addressed through a per-hypothesis row
//     table, so that a beam step never copies a key, a value or a layer output of an earlier position
//   * k_lm_embed: the tail of Encoder(input_layer="linear")'s input layer: LayerNorm -> ReLU -> x * sqrt(D) + pe[pos]
// Both are gather / latency bound (no contraction wider than one query row): plain vector loads and stores, no LDS, no atomics.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------
// One wave per (hypothesis b, query position j, head h).  table[b][p] = e names the pool row of position p of hypothesis b:
//   e >= 0   row e, visible as a key;
//   e == -1  no row (never a key; as a query it gives zeros);
//   e <= -2  row -e - 2, NOT visible as a key (the reference's `ys != 0` key mask: lm/transformer.py:135-138) but still a query.
// Rows outside [0, pool_rows) are treated as e == -1: a damaged table cannot make the kernel leave the pool.
// Keys 0..j in chunks of 64: lane l owns key c*64 + l for the scores (its 64 channels = 128 contiguous bytes), the running
// max / sum are wave reductions (online softmax in fp32), then lane l owns CHANNEL l for the weighted sum of the values: the
// probability and row of key k reach every lane through a wave-uniform readlane.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tbl_row(int e, int pool_rows) {
    const int r = e >= 0 ? e : -e - 2;           // e == -1 -> -1
    return (r >= 0 && r < pool_rows) ? r : -1;
}

__global__ __launch_bounds__(256) void k_mha_table(const bf16_t* __restrict__ pool, int pool_rows, long pitch, const int* __restrict__ table,
                                                   int table_pitch, int n, int Lq, int L, int H, float scale, bf16_t* __restrict__ ctx,
                                                   long ctx_pitch) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform by construction: say so
    if (w >= (long)n * Lq * H) return;                     // whole waves leave: nothing below synchronises across waves
    const int h = (int)(w % H);
    const long qi = w / H;                                 // output row b * Lq + jq
    const int b = (int)(qi / Lq), jq = (int)(qi - (long)b * Lq);
    const int j = L - Lq + jq;                             // absolute position of the query
    const int D = H * 64;
    const int* trow = table + (long)b * table_pitch;
    bf16_t* out = ctx + qi * ctx_pitch + h * 64 + lane;
    const int qrow = tbl_row(trow[j], pool_rows);
    if (qrow < 0) { *out = 0; return; }

    float q[64];
    {
        const u32x4* qp = reinterpret_cast<const u32x4*>(pool + (long)qrow * pitch + h * 64);
#pragma unroll
        for (int c = 0; c < 8; ++c) unpack8(qp[c], q + c * 8);
    }
    float m = -INFINITY, l = 0.f, acc = 0.f;
    for (int k0 = 0; k0 <= j; k0 += 64) {
        const int kk = k0 + lane;
        int e = -1;
        if (kk <= j) e = trow[kk];
        const int row = e >= 0 && e < pool_rows ? e : -1;  // negative entries are never keys
        float s = -INFINITY;
        if (row >= 0) {
            const u32x4* kp = reinterpret_cast<const u32x4*>(pool + (long)row * pitch + D + h * 64);
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float kf[8];
                unpack8(kp[c], kf);
#pragma unroll
                for (int t = 0; t < 8; ++t) d += q[c * 8 + t] * kf[t];
            }
            s = d * scale;
        }
        const float mc = wave_max(s);
        if (mc == -INFINITY) continue;                     // (wave-uniform) every key of this chunk is masked
        const float mn = fmaxf(m, mc);
        const float corr = __expf(m - mn);                 // m = -inf on the first live chunk: exp(-inf) = 0
        const float p = row >= 0 ? __expf(s - mn) : 0.f;
        l = l * corr + wave_sum(p);
        acc *= corr;
        m = mn;
        const int cnt = min(64, j + 1 - k0);
        const bf16_t* vbase = pool + 2 * D + h * 64 + lane;
        for (int k = 0; k < cnt; k += 4) {                 // (lanes behind key j hold row = -1, p = 0: the last group of four may run over cnt)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int rk = __builtin_amdgcn_readlane(row, k + t);
                const float pk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), k + t));
                const float vv = bf2f(vbase[(long)(rk >= 0 ? rk : qrow) * pitch]);        // unconditional load from a row that exists: four in flight
                acc += rk >= 0 ? pk * vv : 0.f;
            }
        }
    }
    *out = l > 0.f ? f2bf(acc / l) : (bf16_t)0;
}

extern "C" int svsr_mha_table_fwd(const void* pool, int pool_rows, int64_t pitch, const int* table, int table_pitch, int n, int Lq, int L, int H, float scale,
                       void* ctx, int64_t ctx_pitch, hipStream_t stream) {
    if (n < 1 || L < 1 || Lq < 1 || Lq > L || H < 1 || pool_rows < 1 || table_pitch < L) return SVSR_ERR_ARG;
    if (pitch < 3L * H * 64 || pitch % 8 != 0 || ctx_pitch < (int64_t)H * 64) return SVSR_ERR_ARG;       // 16-byte loads of 64-channel head slices
    if (((uintptr_t)pool & 15) != 0) return SVSR_ERR_ARG;
    const long waves = (long)n * Lq * H;
    if (waves > (1L << 30)) return SVSR_ERR_ARG;
    hipLaunchKernelGGL(k_mha_table, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, (const bf16_t*)pool, pool_rows, (long)pitch, table,
                       table_pitch, n, Lq, L, H, scale, (bf16_t*)ctx, (long)ctx_pitch);
    return svsr_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// out[r] = relu(LayerNorm(x[r]; gamma, beta, eps)) * scale + pe[pos[r]]: one wave per row, D % 8 == 0 up to 2048 (each lane holds up to
// four 8-channel pieces).  pos[r] is clamped to [0, pe_rows): the host builds the table long enough, the clamp only keeps a wrong
// position inside it.
// ---------------------------------------------------------------------------------------------------------------------
#define LME_MAXP 4

__global__ __launch_bounds__(256) void k_lm_embed(const bf16_t* __restrict__ x, long x_pitch, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, const float* __restrict__ pe, int pe_rows,
                                                  const int* __restrict__ pos, int R, int D, float eps, float scale, bf16_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= R) return;
    const int pieces = D >> 3;
    float v[LME_MAXP][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LME_MAXP; ++i) {
        const int pc = lane + i * 64;
        if (pc < pieces) {
            unpack8(*reinterpret_cast<const u32x4*>(x + r * x_pitch + pc * 8), v[i]);
#pragma unroll
            for (int t = 0; t < 8; ++t) s += v[i][t];
        }
    }
    const float mean = wave_sum(s) / (float)D;
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < LME_MAXP; ++i) {
        if (lane + i * 64 < pieces) {
#pragma unroll
            for (int t = 0; t < 8; ++t) { const float d = v[i][t] - mean; s2 += d * d; }
        }
    }
    const float rstd = rsqrtf(wave_sum(s2) / (float)D + eps);
    int p = pos[r];
    p = p < 0 ? 0 : (p >= pe_rows ? pe_rows - 1 : p);
#pragma unroll
    for (int i = 0; i < LME_MAXP; ++i) {
        const int pc = lane + i * 64;
        if (pc < pieces) {
            const int c0 = pc * 8;
            float o[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float y = (v[i][t] - mean) * rstd * gamma[c0 + t] + beta[c0 + t];
                o[t] = fmaxf(y, 0.f) * scale + pe[(long)p * D + c0 + t];
            }
            *reinterpret_cast<u32x4*>(out + r * D + c0) = pack8(o);
        }
    }
}

extern "C" int svsr_lm_embed_fwd(const void* x, int64_t x_pitch, const float* gamma, const float* beta, const float* pe, int pe_rows, const int* pos, int R,
                      int D, float eps, float scale, void* out, hipStream_t stream) {
    if (R < 1 || D < 8 || D % 8 != 0 || D > LME_MAXP * 512 || x_pitch < D || x_pitch % 8 != 0 || pe_rows < 1) return SVSR_ERR_ARG;
    if ((((uintptr_t)x | (uintptr_t)out) & 15) != 0) return SVSR_ERR_ARG;
    hipLaunchKernelGGL(k_lm_embed, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, stream, (const bf16_t*)x, (long)x_pitch, gamma, beta, pe, pe_rows,
                       pos, R, D, eps, scale, (bf16_t*)out);
    return svsr_check_launch();
}
