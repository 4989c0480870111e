// Dense temporal back-end of the DC-TCN word-level model (syncvsr_amd/dctcn.py; reference LRW/video/src/tcn/models/densetcn.py,
// se_module.py), eval path, gfx950, wave64.  Activations are channels-last bf16 rows [B*T][pitch]; a dense block's feature stack is ONE
// [B*T][1664] buffer: a layer reads a channel prefix through the pitch and writes its channels at an offset (no cat).
//   * k_tconv: up to three dilated temporal convolutions (one per kernel size) of the same rows in one launch, on MFMA, with the
//     squeeze-and-excitation gate applied where the rows are staged and BatchNorm(eval) + bias + activation + residual in the epilogue
//   * k_tcn_se: time mean -> Linear -> Swish -> Linear -> sigmoid, the three gates of a layer in one launch
//   * k_tcn_norm_pool: norm5 + masked mean over time
// No atomics (every output element has one writer, every sum a fixed order), no read outside [0, n_in) of a row or outside [0, T) of a clip.
#include "common.h"

#define TC_HALO 16            // rows of the same clip staged on either side of a 32-row time tile: (k - 1) * d / 2 <= TC_HALO
#define TC_TILE 32            // output rows (time steps) of one slot = one 32x32 MFMA tile
#define TC_ROWS (TC_TILE + 2 * TC_HALO)
#define TC_SLOTS 2            // (clip, time tile) slots per workgroup
#define TC_BN 64              // output channels per workgroup
#define TC_BK 64              // input channels per staged chunk: one 128-byte LDS row
#define TC_MAXK 7
#define TC_SLAB_BYTES (TC_SLOTS * TC_ROWS * TC_BK * 2)
#define TC_ACT_PRELU 3

struct TBranch {
    const bf16_t* w;          // [co][k][n_in]
    const float* gate;        // [B][n_in] or null
    const float* scale;       // [co]
    const float* shift;       // [co]
    const float* slope;       // [co] (PReLU) or null
    int k, out_off, res_off;
};
struct TArgs {
    TBranch br[3];
    const bf16_t* x;
    bf16_t* out;
    const bf16_t* res;
    long x_pitch, out_pitch, res_pitch;
    int B, T, n_in, d, act, res_act, n_tt, slots;
};

// 16-byte piece s (0..7) of 128-byte LDS row `row`: XOR swizzle on the row PAIR, so the 16 rows of a ds_read_b128 lane group (consecutive
// rows, one logical piece) land on 16 distinct (half bank row, 16-byte slot) positions
__device__ __forceinline__ int tc_off(int row, int s) { return row * 128 + ((s ^ ((row >> 1) & 7)) << 4); }

// One workgroup (4 waves): TC_SLOTS slots x 64 output channels of ONE branch; wave w owns slot w >> 1 and 32 of the channels.
// Per 64-channel chunk of the input: the rows [t0 - halo, t0 + 32 + halo) of each slot (zeros outside the clip), times the branch's gate,
// are staged ONCE and serve all k taps (a tap is a row offset into the slab); the chunk of the weights [64 co][k][64 ci] beside it.
__global__ __launch_bounds__(256) void k_tconv(TArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned char* slab = smem_raw;
    unsigned char* wts = smem_raw + TC_SLAB_BYTES;
    const TBranch br = a.br[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = br.k, halo = (k - 1) * a.d / 2;
    const int co0 = blockIdx.y * TC_BN;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    const int my_slot = wave >> 1, nh = wave & 1, r = lane & 31, h = lane >> 5;
    for (int c0 = 0; c0 < a.n_in; c0 += TC_BK) {
        __syncthreads();                                   // the previous chunk's fragments are read
#pragma unroll
        for (int i = 0; i < TC_SLOTS * TC_ROWS * 8 / 256; ++i) {
            const int p = tid + i * 256;
            const int s = p & 7, row = (p >> 3) & (TC_ROWS - 1), sl = p >> 9;
            const long gs = (long)blockIdx.x * TC_SLOTS + sl;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (gs < a.slots && row >= TC_HALO - halo && row < TC_HALO + TC_TILE + halo) {
                const int b = (int)(gs / a.n_tt);
                const int t = (int)(gs - (long)b * a.n_tt) * TC_TILE - TC_HALO + row;
                if (t >= 0 && t < a.T) {
                    v = *reinterpret_cast<const u32x4*>(a.x + ((long)b * a.T + t) * a.x_pitch + c0 + s * 8);
                    if (br.gate != nullptr) {
                        const float4* gp = reinterpret_cast<const float4*>(br.gate + (long)b * a.n_in + c0 + s * 8);
                        const float4 g0 = gp[0], g1 = gp[1];
                        float f[8];
                        unpack8(v, f);
                        f[0] *= g0.x; f[1] *= g0.y; f[2] *= g0.z; f[3] *= g0.w;
                        f[4] *= g1.x; f[5] *= g1.y; f[6] *= g1.z; f[7] *= g1.w;
                        v = pack8(f);
                    }
                }
            }
            *reinterpret_cast<u32x4*>(slab + tc_off(sl * TC_ROWS + row, s)) = v;
        }
        for (int p = tid; p < k * TC_BN * 8; p += 256) {
            const int s = p & 7, co = (p >> 3) & (TC_BN - 1), j = p >> 9;
            const u32x4 v = *reinterpret_cast<const u32x4*>(br.w + ((long)(co0 + co) * k + j) * a.n_in + c0 + s * 8);
            *reinterpret_cast<u32x4*>(wts + tc_off(j * TC_BN + co, s)) = v;
        }
        __syncthreads();
        for (int j = 0; j < k; ++j) {
            const int arow = my_slot * TC_ROWS + TC_HALO + r + (j - (k - 1) / 2) * a.d;
            const int brow = j * TC_BN + nh * 32 + r;
#pragma unroll
            for (int kk = 0; kk < TC_BK / 16; ++kk) {
                const bf16x8 af = *reinterpret_cast<const bf16x8*>(slab + tc_off(arow, 2 * kk + h));
                const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(wts + tc_off(brow, 2 * kk + h));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc, 0, 0, 0);
            }
        }
    }
    // epilogue: lane = output channel, registers = time rows
    const long gs = (long)blockIdx.x * TC_SLOTS + my_slot;
    if (gs >= a.slots) return;                             // (wave-uniform; nothing below synchronises)
    const int b = (int)(gs / a.n_tt);
    const int t0 = (int)(gs - (long)b * a.n_tt) * TC_TILE;
    const int co = co0 + nh * 32 + r;
    const float sc = br.scale[co], sh = br.shift[co];
    const float slope = (a.act == TC_ACT_PRELU) ? br.slope[co] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (t < a.T) {
            const long row = (long)b * a.T + t;
            float v = __builtin_fmaf(acc[i], sc, sh);
            if (a.act == SVSR_ACT_SWISH) v = swish(v);
            else if (a.act == TC_ACT_PRELU) v = v >= 0.f ? v : v * slope;
            else if (a.act == SVSR_ACT_RELU) v = fmaxf(v, 0.f);
            if (a.res != nullptr) {
                v += bf2f(a.res[row * a.res_pitch + br.res_off + co]);
                if (a.res_act == SVSR_ACT_SWISH) v = swish(v);
            }
            a.out[row * a.out_pitch + br.out_off + co] = f2bf(v);
        }
    }
}

// branches: HOST table of nb x 8 64-bit words {k, w, gate, scale, shift, slope, out_off, res_off} (read during the call only)
extern "C" int svsr_tconv_fwd(const void* x, int64_t x_pitch, int B, int T, int n_in, int d, int nb, const int64_t* branches, int co, int act,
                              void* out, int64_t out_pitch, const void* res, int64_t res_pitch, int res_act, hipStream_t stream) {
    if (x == nullptr || out == nullptr || branches == nullptr) return SVSR_ERR_ARG;
    if (B < 1 || T < 1 || d < 1 || n_in < 64 || n_in % 64 != 0 || x_pitch < n_in || x_pitch % 8 != 0 || ((uintptr_t)x & 15) != 0) return SVSR_ERR_ARG;
    if (nb < 1 || nb > 3 || co < TC_BN || co % TC_BN != 0 || out_pitch < co) return SVSR_ERR_ARG;
    if (act != SVSR_ACT_NONE && act != SVSR_ACT_RELU && act != SVSR_ACT_SWISH && act != TC_ACT_PRELU) return SVSR_ERR_ARG;
    if (res_act != SVSR_ACT_NONE && res_act != SVSR_ACT_SWISH) return SVSR_ERR_ARG;
    if (res != nullptr && res_pitch < co) return SVSR_ERR_ARG;
    TArgs a;
    int kmax = 1;
    for (int i = 0; i < 3; ++i) {
        const int64_t* e = branches + 8 * (i < nb ? i : 0);
        TBranch& br = a.br[i];
        br.k = (int)e[0];
        br.w = (const bf16_t*)(uintptr_t)e[1];
        br.gate = (const float*)(uintptr_t)e[2];
        br.scale = (const float*)(uintptr_t)e[3];
        br.shift = (const float*)(uintptr_t)e[4];
        br.slope = (const float*)(uintptr_t)e[5];
        br.out_off = (int)e[6];
        br.res_off = (int)e[7];
        if (e[0] < 1 || e[0] > TC_MAXK || e[0] % 2 == 0) return SVSR_ERR_ARG;
        if ((e[0] - 1) * (int64_t)d / 2 > TC_HALO) return SVSR_ERR_ARG;
        if (br.w == nullptr || ((uintptr_t)br.w & 15) != 0 || br.scale == nullptr || br.shift == nullptr) return SVSR_ERR_ARG;
        if (br.gate != nullptr && ((uintptr_t)br.gate & 15) != 0) return SVSR_ERR_ARG;
        if (act == TC_ACT_PRELU && br.slope == nullptr) return SVSR_ERR_ARG;
        if (e[6] < 0 || e[6] + co > out_pitch) return SVSR_ERR_ARG;
        if (res != nullptr && (e[7] < 0 || e[7] + co > res_pitch)) return SVSR_ERR_ARG;
        if (br.k > kmax) kmax = br.k;
    }
    const long n_tt = (T + TC_TILE - 1) / TC_TILE;
    const long slots = (long)B * n_tt;
    if (slots > (1L << 30) || co / TC_BN > 65535) return SVSR_ERR_ARG;
    a.x = (const bf16_t*)x; a.out = (bf16_t*)out; a.res = (const bf16_t*)res;
    a.x_pitch = x_pitch; a.out_pitch = out_pitch; a.res_pitch = res_pitch;
    a.B = B; a.T = T; a.n_in = n_in; a.d = d; a.act = act; a.res_act = res_act; a.n_tt = (int)n_tt; a.slots = (int)slots;
    const size_t lds = TC_SLAB_BYTES + (size_t)kmax * TC_BN * TC_BK * 2;
    // per call: the attribute belongs to the current device's copy of the kernel, and setting it costs a table lookup
    const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(k_tconv), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ae != hipSuccess) return (int)ae;
    hipLaunchKernelGGL(k_tconv, dim3((unsigned)((slots + TC_SLOTS - 1) / TC_SLOTS), (unsigned)(co / TC_BN), (unsigned)nb), dim3(256), lds, stream, a);
    return svsr_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// Squeeze-and-excitation gates of one layer (se_module.py:8-23, one SELayer per kernel size): for SE_CLIPS clips per workgroup
//   m[c] = mean_t x[b][t][c] (once, shared by the branches), hid = swish(W1 m) [n_in / red], gate = sigmoid(W2 hid) [n_in]
// W1 bf16 [nb][R][n_in], W2 bf16 [nb][n_in][R], gate fp32 [nb][B][n_in].  LDS: mean [SE_CLIPS][n_in] + hid [SE_CLIPS][R] floats.
// Sums run in a fixed order (t ascending; lane-strided partial dots + the wave_sum tree).
// ---------------------------------------------------------------------------------------------------------------------
#define SE_CLIPS 2

__global__ __launch_bounds__(256) void k_tcn_se(const bf16_t* __restrict__ x, long x_pitch, int B, int T, int n_in, int R, int nb,
                                                const bf16_t* __restrict__ w1, const bf16_t* __restrict__ w2, float* __restrict__ gate) {
    extern __shared__ float se_sm[];
    float* mean = se_sm;                        // [SE_CLIPS][n_in]
    float* hid = se_sm + SE_CLIPS * n_in;       // [SE_CLIPS][R]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b0 = blockIdx.x * SE_CLIPS;
    const int pieces = n_in >> 3;
    const float inv_t = 1.0f / (float)T;
    for (int p = tid; p < SE_CLIPS * pieces; p += 256) {
        const int cl = p / pieces, pc = p - cl * pieces;
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (b0 + cl < B) {
            const bf16_t* xp = x + (long)(b0 + cl) * T * x_pitch + pc * 8;
            for (int t = 0; t < T; ++t) {
                float f[8];
                unpack8(*reinterpret_cast<const u32x4*>(xp + (long)t * x_pitch), f);
#pragma unroll
                for (int i = 0; i < 8; ++i) s[i] += f[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) mean[cl * n_in + pc * 8 + i] = s[i] * inv_t;
    }
    for (int br = 0; br < nb; ++br) {
        __syncthreads();                        // mean is written; the previous branch's hid is read
        const bf16_t* w1b = w1 + (long)br * R * n_in;
        for (int j = wave; j < R; j += 4) {
            float d[SE_CLIPS];
#pragma unroll
            for (int cl = 0; cl < SE_CLIPS; ++cl) d[cl] = 0.f;
            for (int pc = lane; pc < pieces; pc += 64) {
                float f[8];
                unpack8(*reinterpret_cast<const u32x4*>(w1b + (long)j * n_in + pc * 8), f);
#pragma unroll
                for (int cl = 0; cl < SE_CLIPS; ++cl)
#pragma unroll
                    for (int i = 0; i < 8; ++i) d[cl] = __builtin_fmaf(f[i], mean[cl * n_in + pc * 8 + i], d[cl]);
            }
#pragma unroll
            for (int cl = 0; cl < SE_CLIPS; ++cl) {
                const float v = wave_sum(d[cl]);
                if (lane == 0) hid[cl * R + j] = swish(v);
            }
        }
        __syncthreads();
        const bf16_t* w2b = w2 + (long)br * n_in * R;
        for (int c = tid; c < n_in; c += 256) {
            float d[SE_CLIPS];
#pragma unroll
            for (int cl = 0; cl < SE_CLIPS; ++cl) d[cl] = 0.f;
            const uint2* wp = reinterpret_cast<const uint2*>(w2b + (long)c * R);      // R % 4 == 0: 8-byte pieces
            for (int q = 0; q < (R >> 2); ++q) {
                const uint2 u = wp[q];
                const float f0 = __uint_as_float(u.x << 16), f1 = __uint_as_float(u.x & 0xffff0000u);
                const float f2 = __uint_as_float(u.y << 16), f3 = __uint_as_float(u.y & 0xffff0000u);
#pragma unroll
                for (int cl = 0; cl < SE_CLIPS; ++cl) {
                    const float* hp = hid + cl * R + q * 4;
                    d[cl] = __builtin_fmaf(f0, hp[0], d[cl]);
                    d[cl] = __builtin_fmaf(f1, hp[1], d[cl]);
                    d[cl] = __builtin_fmaf(f2, hp[2], d[cl]);
                    d[cl] = __builtin_fmaf(f3, hp[3], d[cl]);
                }
            }
#pragma unroll
            for (int cl = 0; cl < SE_CLIPS; ++cl)
                if (b0 + cl < B) gate[((long)br * B + b0 + cl) * n_in + c] = sigmoid_fast(d[cl]);
        }
    }
}

extern "C" int svsr_tcn_se_fwd(const void* x, int64_t x_pitch, int B, int T, int n_in, int R, int nb, const void* w1, const void* w2, float* gate,
                               hipStream_t stream) {
    if (x == nullptr || w1 == nullptr || w2 == nullptr || gate == nullptr) return SVSR_ERR_ARG;
    if (B < 1 || T < 1 || n_in < 64 || n_in % 64 != 0 || x_pitch < n_in || x_pitch % 8 != 0 || nb < 1 || nb > 3) return SVSR_ERR_ARG;
    if (R < 4 || R % 4 != 0 || R > n_in || n_in > 8192) return SVSR_ERR_ARG;
    if ((((uintptr_t)x | (uintptr_t)w1) & 15) != 0 || ((uintptr_t)w2 & 7) != 0) return SVSR_ERR_ARG;
    const size_t lds = (size_t)SE_CLIPS * (n_in + R) * sizeof(float);
    if (lds > 64 * 1024) {
        const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(k_tcn_se), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ae != hipSuccess) return (int)ae;
    }
    hipLaunchKernelGGL(k_tcn_se, dim3((unsigned)((B + SE_CLIPS - 1) / SE_CLIPS)), dim3(256), lds, stream, (const bf16_t*)x, (long)x_pitch, B, T, n_in, R,
                       nb, (const bf16_t*)w1, (const bf16_t*)w2, gate);
    return svsr_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// norm5 (BatchNorm1d, eval: per-channel scale / shift) + masked mean over time (lightning.py:278-279):
//   h[b][t][c] = bf16(x * scale[c] + shift[c]);  pooled[b][c] = bf16(sum_t h * mask[b][t] / (sum_t mask[b][t] + 1e-6))   (t ascending)
// One thread per (clip, 8 channels); a clip whose mask is all zero pools to 0 (finite: the 1e-6 of the reference).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tcn_norm_pool(const bf16_t* __restrict__ x, long x_pitch, int B, int T, int C, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const float* __restrict__ mask, bf16_t* __restrict__ h,
                                                       bf16_t* __restrict__ pooled) {
    const int pieces = C >> 3;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)B * pieces) return;
    const int b = (int)(p / pieces), c0 = (int)(p - (long)b * pieces) * 8;
    float sc[8], sh[8], s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { sc[i] = scale[c0 + i]; sh[i] = shift[c0 + i]; s[i] = 0.f; }
    float msum = 0.f;
    for (int t = 0; t < T; ++t) {
        const long row = (long)b * T + t;
        float f[8];
        unpack8(*reinterpret_cast<const u32x4*>(x + row * x_pitch + c0), f);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = __builtin_fmaf(f[i], sc[i], sh[i]);
        const u32x4 v = pack8(f);
        *reinterpret_cast<u32x4*>(h + row * C + c0) = v;
        unpack8(v, f);                                    // the mean is taken over what is stored
        const float m = mask[row];
        msum += m;
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = __builtin_fmaf(f[i], m, s[i]);
    }
    const float inv = 1.0f / (msum + 1e-6f);
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] *= inv;
    *reinterpret_cast<u32x4*>(pooled + (long)b * C + c0) = pack8(s);
}

extern "C" int svsr_tcn_norm_pool_fwd(const void* x, int64_t x_pitch, int B, int T, int C, const float* scale, const float* shift, const float* mask,
                                      void* h, void* pooled, hipStream_t stream) {
    if (x == nullptr || scale == nullptr || shift == nullptr || mask == nullptr || h == nullptr || pooled == nullptr) return SVSR_ERR_ARG;
    if (B < 1 || T < 1 || C < 8 || C % 8 != 0 || x_pitch < C || x_pitch % 8 != 0) return SVSR_ERR_ARG;
    if ((((uintptr_t)x | (uintptr_t)h | (uintptr_t)pooled) & 15) != 0) return SVSR_ERR_ARG;
    const long n = (long)B * (C >> 3);
    if (n > (1L << 36)) return SVSR_ERR_ARG;
    hipLaunchKernelGGL(k_tcn_norm_pool, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)x, (long)x_pitch, B, T, C, scale, shift,
                       mask, (bf16_t*)h, (bf16_t*)pooled);
    return svsr_check_launch();
}
