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
#define TC_PLAIN 0           // k_tconv<MODE>: the eval forward; TC_SAVE: that and the fp32 accumulators; TC_EXT: the accumulators of the
#define TC_SAVE 1            // extended axis alone (batch-statistic stages)
#define TC_EXT 2

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
    float* save;              // k_tconv<true>: the fp32 accumulators, [B*T][save_pitch], branch i at channels [i * co, (i + 1) * co)
    long save_pitch;
    int co;
    int T_src, shift;         // tc_stage_rows' source axis: T and 0, or (k_tconv<TC_EXT>) the clip's own T under the extended axis a.T, and hmax
};

// 16-byte piece s (0..7) of 128-byte LDS row `row`: XOR swizzle on the row PAIR, so the 16 rows of a ds_read_b128 lane group (consecutive
// rows, one logical piece) land on 16 distinct (half bank row, 16-byte slot) positions
__device__ __forceinline__ int tc_off(int row, int s) { return row * 128 + ((s ^ ((row >> 1) & 7)) << 4); }

// The three staging / tap helpers below are shared by k_tconv, k_tconv_dgrad and (the first) k_tconv_wgrad<K>.  None of them synchronises:
// every caller puts one __syncthreads() in front of the staging (the previous chunk's fragments are read) and one behind it.

// Slab of one 64-channel chunk: the rows [t0 - halo, t0 + 32 + halo) of the TC_SLOTS slots from global slot gs0 on, channels
// [c, c + 64) of src (row pitch `pitch`), zeros outside the clip, outside the halo and for slots >= slots; with a gate (fp32 rows of
// gate_pitch, one per clip) the rows are bf16(x * gate[b]).  All TC_SLOTS * TC_ROWS LDS rows are written.
// The tiles count time on the launch's own axis (n_tt tiles a clip); the source holds T_src rows a clip and its row of tile time t is
// t_src = t - shift, zeros outside [0, T_src).  shift 0 with T_src = the launch's T is the plain case; the batch-statistic stages run the
// forward and the weight gradient on the extended axis of T + 2 * hmax rows over T-row inputs (shift = hmax) and the data gradient on the
// T-row axis over extended gradient rows (shift = -hmax).
__device__ __forceinline__ void tc_stage_rows(unsigned char* slab, const bf16_t* src, long pitch, int c, const float* gate, int gate_pitch, int halo,
                                              int T_src, int shift, int n_tt, int slots, long gs0, int tid) {
#pragma unroll
    for (int i = 0; i < TC_SLOTS * TC_ROWS * 8 / 256; ++i) {
        const int p = tid + i * 256;
        const int s = p & 7, row = (p >> 3) & (TC_ROWS - 1), sl = p >> 9;
        const long gs = gs0 + sl;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (gs < slots && row >= TC_HALO - halo && row < TC_HALO + TC_TILE + halo) {
            const int b = (int)(gs / n_tt);
            const int t = (int)(gs - (long)b * n_tt) * TC_TILE - TC_HALO + row - shift;
            if (t >= 0 && t < T_src) {
                v = *reinterpret_cast<const u32x4*>(src + ((long)b * T_src + t) * pitch + c + s * 8);
                if (gate != nullptr) {
                    const float4* gp = reinterpret_cast<const float4*>(gate + (long)b * gate_pitch + c + s * 8);
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
}

// Weight chunk [64 rows from row0][k][64 channels from c0] of w [rows][k][ld] -> wts, LDS row j * 64 + row
__device__ __forceinline__ void tc_stage_weights(unsigned char* wts, const bf16_t* w, int row0, int k, int ld, int c0, int tid) {
    for (int p = tid; p < k * TC_BN * 8; p += 256) {
        const int s = p & 7, co = (p >> 3) & (TC_BN - 1), j = p >> 9;
        const u32x4 v = *reinterpret_cast<const u32x4*>(w + ((long)(row0 + co) * k + j) * ld + c0 + s * 8);
        *reinterpret_cast<u32x4*>(wts + tc_off(j * TC_BN + co, s)) = v;
    }
}

// acc += the k taps of one staged chunk: tap j is the slab row offset (j - (k - 1) / 2) * d, four MFMAs over the 64 channels
__device__ __forceinline__ void tc_taps(f32x16& acc, const unsigned char* slab, const unsigned char* wts, int k, int d, int my_slot, int nh, int r, int h) {
    for (int j = 0; j < k; ++j) {
        const int arow = my_slot * TC_ROWS + TC_HALO + r + (j - (k - 1) / 2) * d;
        const int brow = j * TC_BN + nh * 32 + r;
#pragma unroll
        for (int kk = 0; kk < TC_BK / 16; ++kk) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(slab + tc_off(arow, 2 * kk + h));
            const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(wts + tc_off(brow, 2 * kk + h));
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc, 0, 0, 0);
        }
    }
}

// Host side of the same scheme.  Taps: odd k <= TC_MAXK whose reach fits the staged halo
static bool tc_taps_ok(int64_t k, int d) { return k >= 1 && k <= TC_MAXK && k % 2 != 0 && (k - 1) * (int64_t)d / 2 <= TC_HALO; }

// Time tiles per clip and (clip, tile) slots of B clips of T rows; false: more slots than the kernels index
static bool tc_geometry(int B, int T, int* n_tt, int* slots) {
    const long tt = (T + TC_TILE - 1) / TC_TILE, n = (long)B * tt;
    if (n > (1L << 30)) return false;
    *n_tt = (int)tt; *slots = (int)n;
    return true;
}

// Dynamic LDS of a slab and a kmax-tap weight chunk, announced to kernel fn.  Per call: the attribute belongs to the current device's copy of
// the kernel, and setting it costs a table lookup
static hipError_t tc_dynamic_lds(const void* fn, int kmax, size_t* lds) {
    *lds = TC_SLAB_BYTES + (size_t)kmax * TC_BN * TC_BK * 2;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds);
}

// One workgroup (4 waves): TC_SLOTS slots x 64 output channels of ONE branch; wave w owns slot w >> 1 and 32 of the channels.
// Per 64-channel chunk of the input: the rows [t0 - halo, t0 + 32 + halo) of each slot (zeros outside the clip), times the branch's gate,
// are staged ONCE and serve all k taps (a tap is a row offset into the slab); the chunk of the weights [64 co][k][64 ci] beside it.
// SAVE: the accumulator of every written element is stored too (svsr_tconv_fwd_save: the backward recomputes z = scale * acc + shift from it
// with the same fma); the bf16 outputs are the same bits either way.
template <int MODE>
__global__ __launch_bounds__(256) void k_tconv(TArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned char* slab = smem_raw;
    unsigned char* wts = smem_raw + TC_SLAB_BYTES;
    const TBranch br = a.br[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = br.k, halo = (k - 1) * a.d / 2;
    const int co0 = blockIdx.y * TC_BN;
    // TC_EXT: the branch's own rows of the extended axis are [lo, hi); a workgroup whose slots all lie outside them has nothing to store
    const int lo = a.shift - halo, hi = a.shift + a.T_src + halo;
    if (MODE == TC_EXT) {
        bool any = false;
        for (int s = 0; s < TC_SLOTS; ++s) {
            const long gs = (long)blockIdx.x * TC_SLOTS + s;
            const int t0 = (int)(gs % a.n_tt) * TC_TILE;
            any = any || (gs < a.slots && t0 < hi && t0 + TC_TILE > lo);
        }
        if (!any) return;                                  // (uniform over the workgroup, before the first barrier)
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    const int my_slot = wave >> 1, nh = wave & 1, r = lane & 31, h = lane >> 5;
    for (int c0 = 0; c0 < a.n_in; c0 += TC_BK) {
        __syncthreads();                                   // the previous chunk's fragments are read
        tc_stage_rows(slab, a.x, a.x_pitch, c0, br.gate, a.n_in, halo, a.T_src, a.shift, a.n_tt, a.slots, (long)blockIdx.x * TC_SLOTS, tid);
        tc_stage_weights(wts, br.w, co0, k, a.n_in, c0, tid);
        __syncthreads();
        tc_taps(acc, slab, wts, k, a.d, my_slot, nh, r, h);
    }
    // epilogue: lane = output channel, registers = time rows
    const long gs = (long)blockIdx.x * TC_SLOTS + my_slot;
    if (gs >= a.slots) return;                             // (wave-uniform; nothing below synchronises)
    const int b = (int)(gs / a.n_tt);
    const int t0 = (int)(gs - (long)b * a.n_tt) * TC_TILE;
    const int co = co0 + nh * 32 + r;
    if (MODE == TC_EXT) {                                  // accumulators only: the statistics come first (svsr_tcn_colstats, svsr_tconv_apply)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int t = t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (t >= lo && t < hi) a.save[((long)b * a.T + t) * a.save_pitch + (long)blockIdx.z * a.co + co] = acc[i];
        }
        return;
    }
    const float sc = br.scale[co], sh = br.shift[co];
    const float slope = (a.act == TC_ACT_PRELU) ? br.slope[co] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (t < a.T) {
            const long row = (long)b * a.T + t;
            float v = __builtin_fmaf(acc[i], sc, sh);
            if (MODE == TC_SAVE) a.save[row * a.save_pitch + (long)blockIdx.z * a.co + co] = acc[i];
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

// branches: HOST table of nb x 8 64-bit words {k, w, gate, scale, shift, slope, out_off, res_off} (read during the call only).
// mode TC_EXT (svsr_tconv_fwd_ext): the launch's axis is the extended one, T + 2 * hmax rows a clip over the T-row input; the accumulators are
// the only output, so there is no out and only k, w and gate of a table row are read (the other words may be zero).  hmax is 0 otherwise.
static int tconv_launch(const void* x, int64_t x_pitch, int B, int T, int n_in, int d, int nb, const int64_t* branches, int co, int act,
                        void* out, int64_t out_pitch, const void* res, int64_t res_pitch, int res_act, float* save, int64_t save_pitch, int mode,
                        int hmax, hipStream_t stream) {
    const bool ext = mode == TC_EXT;
    if (mode != TC_PLAIN && (save == nullptr || save_pitch < (int64_t)nb * co)) return SVSR_ERR_ARG;
    if (x == nullptr || branches == nullptr || (!ext && out == nullptr) || hmax < 0 || hmax > TC_HALO) return SVSR_ERR_ARG;
    if (B < 1 || T < 1 || d < 1 || n_in < 64 || n_in % 64 != 0 || x_pitch < n_in || x_pitch % 8 != 0 || ((uintptr_t)x & 15) != 0) return SVSR_ERR_ARG;
    if (nb < 1 || nb > 3 || co < TC_BN || co % TC_BN != 0 || (!ext && out_pitch < co)) return SVSR_ERR_ARG;
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
        if (!tc_taps_ok(e[0], d) || (ext && (e[0] - 1) * (int64_t)d / 2 > hmax)) return SVSR_ERR_ARG;
        if (br.w == nullptr || ((uintptr_t)br.w & 15) != 0) return SVSR_ERR_ARG;
        if (br.gate != nullptr && ((uintptr_t)br.gate & 15) != 0) return SVSR_ERR_ARG;
        if (br.k > kmax) kmax = br.k;
        if (ext) {          // (the other table words are not read: the kernel gets null / 0 for them)
            br.scale = nullptr; br.shift = nullptr; br.slope = nullptr; br.out_off = 0; br.res_off = 0;
            continue;
        }
        if (br.scale == nullptr || br.shift == nullptr) return SVSR_ERR_ARG;
        if (act == TC_ACT_PRELU && br.slope == nullptr) return SVSR_ERR_ARG;
        if (e[6] < 0 || e[6] + co > out_pitch) return SVSR_ERR_ARG;
        if (res != nullptr && (e[7] < 0 || e[7] + co > res_pitch)) return SVSR_ERR_ARG;
    }
    if (!tc_geometry(B, T + 2 * hmax, &a.n_tt, &a.slots) || co / TC_BN > 65535) return SVSR_ERR_ARG;
    a.x = (const bf16_t*)x; a.out = (bf16_t*)out; a.res = (const bf16_t*)res;
    a.x_pitch = x_pitch; a.out_pitch = out_pitch; a.res_pitch = res_pitch;
    a.B = B; a.T = T + 2 * hmax; a.n_in = n_in; a.d = d; a.act = act; a.res_act = res_act;
    a.save = save; a.save_pitch = save_pitch; a.co = co; a.T_src = T; a.shift = hmax;
    const dim3 grid((unsigned)((a.slots + TC_SLOTS - 1) / TC_SLOTS), (unsigned)(co / TC_BN), (unsigned)nb);
    void (*const fn)(TArgs) = ext ? k_tconv<TC_EXT> : mode == TC_SAVE ? k_tconv<TC_SAVE> : k_tconv<TC_PLAIN>;
    size_t lds;
    const hipError_t ae = tc_dynamic_lds(reinterpret_cast<const void*>(fn), kmax, &lds);
    if (ae != hipSuccess) return (int)ae;
    hipLaunchKernelGGL(fn, grid, dim3(256), lds, stream, a);
    return svsr_check_launch();
}

extern "C" int svsr_tconv_fwd(const void* x, int64_t x_pitch, int B, int T, int n_in, int d, int nb, const int64_t* branches, int co, int act,
                              void* out, int64_t out_pitch, const void* res, int64_t res_pitch, int res_act, hipStream_t stream) {
    return tconv_launch(x, x_pitch, B, T, n_in, d, nb, branches, co, act, out, out_pitch, res, res_pitch, res_act, nullptr, 0, TC_PLAIN, 0, stream);
}

// svsr_tconv_fwd that also stores every fp32 accumulator: acc[b*T + t][i * co + c] for branch i (acc_pitch >= nb * co)
extern "C" int svsr_tconv_fwd_save(const void* x, int64_t x_pitch, int B, int T, int n_in, int d, int nb, const int64_t* branches, int co, int act,
                                   void* out, int64_t out_pitch, const void* res, int64_t res_pitch, int res_act, float* acc, int64_t acc_pitch,
                                   hipStream_t stream) {
    return tconv_launch(x, x_pitch, B, T, n_in, d, nb, branches, co, act, out, out_pitch, res, res_pitch, res_act, acc, acc_pitch, TC_SAVE, 0, stream);
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

// =====================================================================================================================
// Backward of the back-end in the statistics mode the forward runs (running-statistic BatchNorm, no dropout).  Gradient rows are bf16,
// parameter gradients and per-channel sums fp32.  No atomics: every element has one writer per launch, every sum one fixed order.
// =====================================================================================================================

// out[i] = (add ? out[i] : 0) + sum_r part[r * n + i], r ascending
__global__ __launch_bounds__(256) void k_tcn_fold(const float* __restrict__ part, int rows, long n, float* __restrict__ out, int add) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += part[(long)r * n + i];
    out[i] = add ? out[i] + s : s;
}

extern "C" int svsr_tcn_fold(const float* part, int rows, int64_t n, float* out, int add, hipStream_t stream) {
    if (part == nullptr || out == nullptr || rows < 1 || n < 1 || n > (1L << 38)) return SVSR_ERR_ARG;
    hipLaunchKernelGGL(k_tcn_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part, rows, (long)n, out, add);
    return svsr_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// Epilogue backward.  With z = scale * acc + shift (the forward's fma on the stored accumulator), y = act(z) and, with a residual,
// u = y + res and the output res_act(u):   du = dy * res_act'(u) (dy without a residual), g = du * act'(z),
//   dacc = bf16(g * scale), dres = bf16(du), and per channel the sums of g, g * acc, du * min(z, 0) (the PReLU slope) and du,
// first per block of EB_ROWS rows (part [blocks][4][C]), then folded in block order by svsr_tcn_fold.
// ---------------------------------------------------------------------------------------------------------------------
#define EB_ROWS 64
struct EArgs {
    const bf16_t* dy; const float* acc; const float* scale; const float* shift; const float* slope; const bf16_t* res;
    bf16_t* dacc; bf16_t* dres; float* part;
    long dy_pitch, acc_pitch, res_pitch, dacc_pitch, dres_pitch, rows;
    int C, act, res_act;
};

__global__ __launch_bounds__(256) void k_tconv_epi_bwd(EArgs a) {
    __shared__ float red[4][4][64];
    const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6;
    const int c = blockIdx.y * 64 + cl;
    const float sc = a.scale[c], sh = a.shift[c];
    const float slope = a.act == TC_ACT_PRELU ? a.slope[c] : 0.f;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const long r0 = (long)blockIdx.x * EB_ROWS;
    for (int i = rl; i < EB_ROWS; i += 4) {
        const long row = r0 + i;
        if (row >= a.rows) break;
        const float ac = a.acc[row * a.acc_pitch + c];
        const float z = __builtin_fmaf(ac, sc, sh);
        float du = bf2f(a.dy[row * a.dy_pitch + c]);
        if (a.res != nullptr) {
            float y = z;
            if (a.act == SVSR_ACT_SWISH) y = swish(z);
            else if (a.act == TC_ACT_PRELU) y = z >= 0.f ? z : z * slope;
            else if (a.act == SVSR_ACT_RELU) y = fmaxf(z, 0.f);
            const float u = y + bf2f(a.res[row * a.res_pitch + c]);
            if (a.res_act == SVSR_ACT_SWISH) du *= swish_grad(u);
            a.dres[row * a.dres_pitch + c] = f2bf(du);
            s3 += du;
        }
        float g = du;
        if (a.act == SVSR_ACT_SWISH) g = du * swish_grad(z);
        else if (a.act == TC_ACT_PRELU) { g = z >= 0.f ? du : du * slope; s2 += du * fminf(z, 0.f); }
        else if (a.act == SVSR_ACT_RELU) g = z > 0.f ? du : 0.f;
        a.dacc[row * a.dacc_pitch + c] = f2bf(g * sc);
        s0 += g;
        s1 = __builtin_fmaf(g, ac, s1);
    }
    red[0][rl][cl] = s0; red[1][rl][cl] = s1; red[2][rl][cl] = s2; red[3][rl][cl] = s3;
    __syncthreads();
    // thread (stat = rl, channel = cl): the four row lanes in order
    const float t = ((red[rl][0][cl] + red[rl][1][cl]) + red[rl][2][cl]) + red[rl][3][cl];
    a.part[((long)blockIdx.x * 4 + rl) * a.C + c] = t;
}

extern "C" int svsr_tconv_epi_bwd(const void* dy, int64_t dy_pitch, const float* acc, int64_t acc_pitch, int64_t rows, int C, int act,
                                  const float* scale, const float* shift, const float* slope, const void* res, int64_t res_pitch, int res_act,
                                  void* dacc, int64_t dacc_pitch, void* dres, int64_t dres_pitch, float* part, float* sums, hipStream_t stream) {
    if (dy == nullptr || acc == nullptr || scale == nullptr || shift == nullptr || dacc == nullptr || part == nullptr || sums == nullptr) return SVSR_ERR_ARG;
    if (rows < 1 || rows > (1L << 30) || C < 64 || C % 64 != 0 || C / 64 > 65535 || dy_pitch < C || acc_pitch < C || dacc_pitch < C) return SVSR_ERR_ARG;
    if (act != SVSR_ACT_NONE && act != SVSR_ACT_RELU && act != SVSR_ACT_SWISH && act != TC_ACT_PRELU) return SVSR_ERR_ARG;
    if (act == TC_ACT_PRELU && slope == nullptr) return SVSR_ERR_ARG;
    if (res_act != SVSR_ACT_NONE && res_act != SVSR_ACT_SWISH) return SVSR_ERR_ARG;
    if (res != nullptr && (dres == nullptr || res_pitch < C || dres_pitch < C)) return SVSR_ERR_ARG;
    EArgs a;
    a.dy = (const bf16_t*)dy; a.acc = acc; a.scale = scale; a.shift = shift; a.slope = slope; a.res = (const bf16_t*)res;
    a.dacc = (bf16_t*)dacc; a.dres = (bf16_t*)dres; a.part = part;
    a.dy_pitch = dy_pitch; a.acc_pitch = acc_pitch; a.res_pitch = res_pitch; a.dacc_pitch = dacc_pitch; a.dres_pitch = dres_pitch; a.rows = rows;
    a.C = C; a.act = act; a.res_act = res_act;
    const long blocks = (rows + EB_ROWS - 1) / EB_ROWS;
    hipLaunchKernelGGL(k_tconv_epi_bwd, dim3((unsigned)blocks, (unsigned)(C / 64)), dim3(256), 0, stream, a);
    int rc = svsr_check_launch();
    if (rc != SVSR_OK) return rc;
    return svsr_tcn_fold(part, (int)blocks, 4L * C, sums, 0, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Data gradient of the multi-branch (gated) temporal convolution: the forward's slab scheme with the roles exchanged.  The staged rows are
// the nb branches' dacc (co channels each, at dy_off), the weights are the transposed, tap-flipped shadows wt [n_out][k][co]
// (wt[ci][j][c] = w[c][k - 1 - j][ci]), so tap j is again the row offset (j - (k - 1) / 2) * d.  One workgroup: TC_SLOTS slots x 64 input
// channels, the branches one after the other:
//   dxg_j = conv(dacc_j, wt_j);   gpart[j][b][tile][ci] = sum_t x[b][t][ci] * dxg_j[b][t][ci]   (gated branches; t ascending per lane, the two
//   lane halves added low + high);   out = bf16(addend + cadd[b][ci] * cadd_scale + sum_j gate_j[b][ci] * dxg_j)     — one write for all branches
// ---------------------------------------------------------------------------------------------------------------------
struct DBranch { const bf16_t* wt; const float* gate; int k, dy_off; };
struct DArgs {
    DBranch br[3];
    const bf16_t* dy; const bf16_t* x; const bf16_t* addend; const float* cadd; bf16_t* out; float* gpart;
    long dy_pitch, x_pitch, add_pitch, out_pitch;
    float cadd_scale;
    int B, T, co, n_out, d, nb, n_tt, slots;
    int T_src, shift;         // the gradient rows' axis: T and 0, or (svsr_tconv_dgrad_ext) T + 2 * hmax and -hmax
};

__global__ __launch_bounds__(256) void k_tconv_dgrad(DArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned char* slab = smem_raw;
    unsigned char* wts = smem_raw + TC_SLAB_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = blockIdx.y * TC_BN;
    const int my_slot = wave >> 1, nh = wave & 1, r = lane & 31, h = lane >> 5;
    const long gsw = (long)blockIdx.x * TC_SLOTS + my_slot;
    const bool valid = gsw < a.slots;
    const int wb = valid ? (int)(gsw / a.n_tt) : 0;
    const int wtt = valid ? (int)(gsw - (long)wb * a.n_tt) : 0;
    const int t0 = wtt * TC_TILE;
    const int ci = n0 + nh * 32 + r;
    f32x16 tot;
#pragma unroll
    for (int i = 0; i < 16; ++i) tot[i] = 0.f;
    for (int j = 0; j < a.nb; ++j) {
        const DBranch br = a.br[j];
        const int k = br.k, halo = (k - 1) * a.d / 2;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int c0 = 0; c0 < a.co; c0 += TC_BK) {
            __syncthreads();
            tc_stage_rows(slab, a.dy, a.dy_pitch, br.dy_off + c0, nullptr, 0, halo, a.T_src, a.shift, a.n_tt, a.slots, (long)blockIdx.x * TC_SLOTS, tid);
            tc_stage_weights(wts, br.wt, n0, k, a.co, c0, tid);
            __syncthreads();
            tc_taps(acc, slab, wts, k, a.d, my_slot, nh, r, h);
        }
        if (br.gate != nullptr) {
            const float gt = valid ? br.gate[(long)wb * a.n_out + ci] : 0.f;
            float gp = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int t = t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (valid && t < a.T) gp = __builtin_fmaf(bf2f(a.x[((long)wb * a.T + t) * a.x_pitch + ci]), acc[i], gp);
                tot[i] = __builtin_fmaf(gt, acc[i], tot[i]);
            }
            const float other = __shfl_xor(gp, 32);
            if (valid && h == 0) a.gpart[(((long)j * a.B + wb) * a.n_tt + wtt) * a.n_out + ci] = gp + other;
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) tot[i] += acc[i];
        }
    }
    if (!valid) return;
    const float ca = a.cadd != nullptr ? a.cadd[(long)wb * a.n_out + ci] * a.cadd_scale : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (t < a.T) {
            const long row = (long)wb * a.T + t;
            float v = tot[i] + ca;
            if (a.addend != nullptr) v += bf2f(a.addend[row * a.add_pitch + ci]);
            a.out[row * a.out_pitch + ci] = f2bf(v);
        }
    }
}

// branches: HOST table of nb x 4 64-bit words {k, wt, gate, dy_off}
// hmax: dy holds T + 2 * hmax rows a clip, the row of time t at t + hmax (0: the plain T-row gradient)
static int tconv_dgrad_launch(const void* dy, int64_t dy_pitch, int B, int T, int co, int d, int nb, const int64_t* branches, int n_out,
                              const void* x, int64_t x_pitch, const void* addend, int64_t add_pitch, const float* cadd, float cadd_scale,
                              void* out, int64_t out_pitch, float* gpart, int hmax, hipStream_t stream) {
    if (dy == nullptr || out == nullptr || branches == nullptr) return SVSR_ERR_ARG;
    if (hmax < 0 || hmax > TC_HALO) return SVSR_ERR_ARG;
    if (B < 1 || T < 1 || d < 1 || co < 64 || co % 64 != 0 || dy_pitch % 8 != 0 || ((uintptr_t)dy & 15) != 0) return SVSR_ERR_ARG;
    if (nb < 1 || nb > 3 || n_out < TC_BN || n_out % TC_BN != 0 || out_pitch < n_out) return SVSR_ERR_ARG;
    if (addend != nullptr && add_pitch < n_out) return SVSR_ERR_ARG;
    DArgs a;
    int kmax = 1;
    bool gated = false;
    for (int i = 0; i < 3; ++i) {
        const int64_t* e = branches + 4 * (i < nb ? i : 0);
        DBranch& br = a.br[i];
        br.k = (int)e[0];
        br.wt = (const bf16_t*)(uintptr_t)e[1];
        br.gate = (const float*)(uintptr_t)e[2];
        br.dy_off = (int)e[3];
        if (!tc_taps_ok(e[0], d)) return SVSR_ERR_ARG;
        if (hmax > 0 && (e[0] - 1) * (int64_t)d / 2 > hmax) return SVSR_ERR_ARG;          // (the branch reads rows [t - h, t + h] of the extended axis)
        if (br.wt == nullptr || ((uintptr_t)br.wt & 15) != 0) return SVSR_ERR_ARG;
        if (e[3] < 0 || e[3] % 8 != 0 || e[3] + co > dy_pitch) return SVSR_ERR_ARG;
        if (br.gate != nullptr) gated = true;
        if (br.k > kmax) kmax = br.k;
    }
    if (gated && (x == nullptr || gpart == nullptr || x_pitch < n_out)) return SVSR_ERR_ARG;
    if (!tc_geometry(B, T, &a.n_tt, &a.slots) || n_out / TC_BN > 65535) return SVSR_ERR_ARG;
    a.dy = (const bf16_t*)dy; a.x = (const bf16_t*)x; a.addend = (const bf16_t*)addend; a.cadd = cadd; a.out = (bf16_t*)out; a.gpart = gpart;
    a.dy_pitch = dy_pitch; a.x_pitch = x_pitch; a.add_pitch = add_pitch; a.out_pitch = out_pitch; a.cadd_scale = cadd_scale;
    a.B = B; a.T = T; a.co = co; a.n_out = n_out; a.d = d; a.nb = nb; a.T_src = T + 2 * hmax; a.shift = -hmax;
    size_t lds;
    const hipError_t ae = tc_dynamic_lds(reinterpret_cast<const void*>(k_tconv_dgrad), kmax, &lds);
    if (ae != hipSuccess) return (int)ae;
    hipLaunchKernelGGL(k_tconv_dgrad, dim3((unsigned)((a.slots + TC_SLOTS - 1) / TC_SLOTS), (unsigned)(n_out / TC_BN)), dim3(256), lds, stream, a);
    return svsr_check_launch();
}

extern "C" int svsr_tconv_dgrad(const void* dy, int64_t dy_pitch, int B, int T, int co, int d, int nb, const int64_t* branches, int n_out,
                                const void* x, int64_t x_pitch, const void* addend, int64_t add_pitch, const float* cadd, float cadd_scale,
                                void* out, int64_t out_pitch, float* gpart, hipStream_t stream) {
    return tconv_dgrad_launch(dy, dy_pitch, B, T, co, d, nb, branches, n_out, x, x_pitch, addend, add_pitch, cadd, cadd_scale, out, out_pitch, gpart, 0,
                              stream);
}

// svsr_tconv_dgrad over the gradient of the extended accumulators (svsr_tconv_bn_bwd): dy bf16 [B * (T + 2 * hmax)][dy_pitch]
extern "C" int svsr_tconv_dgrad_ext(const void* dy, int64_t dy_pitch, int B, int T, int co, int d, int nb, const int64_t* branches, int n_out,
                                    const void* x, int64_t x_pitch, const void* addend, int64_t add_pitch, const float* cadd, float cadd_scale,
                                    void* out, int64_t out_pitch, float* gpart, int hmax, hipStream_t stream) {
    return tconv_dgrad_launch(dy, dy_pitch, B, T, co, d, nb, branches, n_out, x, x_pitch, addend, add_pitch, cadd, cadd_scale, out, out_pitch, gpart,
                              hmax, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient of one branch: dW[c][j][ci] = sum_{b,t} dacc[b][t][c] * bf16(x * gate)[b][t + (j - (K-1)/2) d][ci], fp32 on MFMA over the rows.
// One workgroup: 64 output channels x 64 input channels x all K taps; wave w owns the output-channel half w >> 1 and the input-channel half
// w & 1, K accumulators.  Per pair of slots the gated rows are staged as the forward stages them (one slab serves the K taps), the dacc tile
// beside them; the MFMA's K dimension is time, so a lane gathers its 8 consecutive rows of one channel with 2-byte LDS reads.  Split s of S
// takes the slot pairs s, s + S, ... and writes part[s][co][K][n_in]; k_tconv_wgrad_fold adds the splits in order and writes the parameter's
// own [co][n_valid][K] layout.
// ---------------------------------------------------------------------------------------------------------------------
struct WArgs {
    const bf16_t* x; const bf16_t* dy; const float* gate; float* part;
    long x_pitch, dy_pitch;
    int B, T, n_in, co, d, n_tt, slots, S;
    int T_x, shift;           // x's own rows a clip under the launch's axis T: T and 0, or (svsr_tconv_wgrad_ext) T - 2 * hmax and hmax
};

__device__ __forceinline__ bf16x8 tc_gather8(const unsigned char* base, int row0, int ch) {
    u32x4 v;
    unsigned w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned lo = *reinterpret_cast<const unsigned short*>(base + tc_off(row0 + 2 * q, ch >> 3) + (ch & 7) * 2);
        const unsigned hi = *reinterpret_cast<const unsigned short*>(base + tc_off(row0 + 2 * q + 1, ch >> 3) + (ch & 7) * 2);
        w[q] = lo | (hi << 16);
    }
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    return __builtin_bit_cast(bf16x8, v);
}

template <int K>
__global__ __launch_bounds__(256) void k_tconv_wgrad(WArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char slab[TC_SLAB_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char dyt[TC_SLOTS * TC_TILE * 128];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int halo = (K - 1) * a.d / 2;
    const int ci0 = blockIdx.y * 64, co0 = blockIdx.z * 64;
    const int mh = wave >> 1, nh = wave & 1, r = lane & 31, h = lane >> 5;
    f32x16 acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    const int npairs = (a.slots + TC_SLOTS - 1) / TC_SLOTS;
    for (int pr = blockIdx.x; pr < npairs; pr += a.S) {
        __syncthreads();
        tc_stage_rows(slab, a.x, a.x_pitch, ci0, a.gate, a.n_in, halo, a.T_x, a.shift, a.n_tt, a.slots, (long)pr * TC_SLOTS, tid);
#pragma unroll
        for (int i = 0; i < TC_SLOTS * TC_TILE * 8 / 256; ++i) {
            const int p = tid + i * 256;
            const int s = p & 7, row = (p >> 3) & (TC_TILE - 1), sl = p >> 8;
            const long gs = (long)pr * TC_SLOTS + sl;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (gs < a.slots) {
                const int b = (int)(gs / a.n_tt);
                const int t = (int)(gs - (long)b * a.n_tt) * TC_TILE + row;
                if (t < a.T) v = *reinterpret_cast<const u32x4*>(a.dy + ((long)b * a.T + t) * a.dy_pitch + co0 + s * 8);
            }
            *reinterpret_cast<u32x4*>(dyt + tc_off(sl * TC_TILE + row, s)) = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int sl = 0; sl < TC_SLOTS; ++sl)
#pragma unroll 1
            for (int kk = 0; kk < TC_TILE / 16; ++kk) {
                const bf16x8 af = tc_gather8(dyt, sl * TC_TILE + 16 * kk + 8 * h, mh * 32 + r);
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const bf16x8 bfr = tc_gather8(slab, sl * TC_ROWS + TC_HALO + 16 * kk + 8 * h + (j - (K - 1) / 2) * a.d, nh * 32 + r);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc[j], 0, 0, 0);
                }
            }
    }
    // lane = input channel, registers = output channels
    const int ci = ci0 + nh * 32 + r;
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = co0 + mh * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            a.part[(((long)blockIdx.x * a.co + c) * K + j) * a.n_in + ci] = acc[j][i];
        }
}

__global__ __launch_bounds__(256) void k_tconv_wgrad_fold(const float* __restrict__ part, int S, int co, int K, int n_in, int n_valid,
                                                          float* __restrict__ dw, int add) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)co * n_valid * K;
    if (i >= n) return;
    const int j = (int)(i % K);
    const long q = i / K;
    const int ci = (int)(q % n_valid);
    const int c = (int)(q / n_valid);
    const long stride = (long)co * K * n_in;
    const float* p = part + ((long)c * K + j) * n_in + ci;
    float s = 0.f;
    for (int sp = 0; sp < S; ++sp) s += p[sp * stride];
    dw[i] = add ? dw[i] + s : s;
}

// hmax: dy holds T + 2 * hmax rows a clip (the gradient of the extended accumulators) and the sum runs over all of them; x keeps T rows
static int tconv_wgrad_launch(const void* x, int64_t x_pitch, const float* gate, const void* dy, int64_t dy_pitch, int B, int T, int n_in, int co,
                              int k, int d, int splits, float* part, float* dw, int n_valid, int add, int hmax, hipStream_t stream) {
    if (x == nullptr || dy == nullptr || part == nullptr || dw == nullptr) return SVSR_ERR_ARG;
    if (hmax < 0 || hmax > TC_HALO || (hmax > 0 && (k - 1) * (int64_t)d / 2 > hmax)) return SVSR_ERR_ARG;
    if (B < 1 || T < 1 || d < 1 || n_in < 64 || n_in % 64 != 0 || x_pitch < n_in || x_pitch % 8 != 0 || ((uintptr_t)x & 15) != 0) return SVSR_ERR_ARG;
    if (co < 64 || co % 64 != 0 || dy_pitch < co || dy_pitch % 8 != 0 || ((uintptr_t)dy & 15) != 0) return SVSR_ERR_ARG;
    if (!tc_taps_ok(k, d)) return SVSR_ERR_ARG;
    if (gate != nullptr && ((uintptr_t)gate & 15) != 0) return SVSR_ERR_ARG;
    if (n_valid < 1 || n_valid > n_in) return SVSR_ERR_ARG;
    WArgs a;
    if (!tc_geometry(B, T + 2 * hmax, &a.n_tt, &a.slots)) return SVSR_ERR_ARG;
    if (splits < 1 || splits > (a.slots + TC_SLOTS - 1) / TC_SLOTS || splits > 65535 || n_in / 64 > 65535 || co / 64 > 65535) return SVSR_ERR_ARG;
    a.x = (const bf16_t*)x; a.dy = (const bf16_t*)dy; a.gate = gate; a.part = part; a.x_pitch = x_pitch; a.dy_pitch = dy_pitch;
    a.B = B; a.T = T + 2 * hmax; a.n_in = n_in; a.co = co; a.d = d; a.S = splits; a.T_x = T; a.shift = hmax;
    const dim3 grid((unsigned)splits, (unsigned)(n_in / 64), (unsigned)(co / 64));
    if (k == 1) hipLaunchKernelGGL(k_tconv_wgrad<1>, grid, dim3(256), 0, stream, a);
    else if (k == 3) hipLaunchKernelGGL(k_tconv_wgrad<3>, grid, dim3(256), 0, stream, a);
    else if (k == 5) hipLaunchKernelGGL(k_tconv_wgrad<5>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_tconv_wgrad<7>, grid, dim3(256), 0, stream, a);
    int rc = svsr_check_launch();
    if (rc != SVSR_OK) return rc;
    const long n = (long)co * n_valid * k;
    hipLaunchKernelGGL(k_tconv_wgrad_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const float*)part, splits, co, k, n_in, n_valid, dw, add);
    return svsr_check_launch();
}

extern "C" int svsr_tconv_wgrad(const void* x, int64_t x_pitch, const float* gate, const void* dy, int64_t dy_pitch, int B, int T, int n_in, int co,
                                int k, int d, int splits, float* part, float* dw, int n_valid, int add, hipStream_t stream) {
    return tconv_wgrad_launch(x, x_pitch, gate, dy, dy_pitch, B, T, n_in, co, k, d, splits, part, dw, n_valid, add, 0, stream);
}

// svsr_tconv_wgrad over dy bf16 [B * (T + 2 * hmax)][dy_pitch]; splits <= the slot pairs of the extended axis
extern "C" int svsr_tconv_wgrad_ext(const void* x, int64_t x_pitch, const float* gate, const void* dy, int64_t dy_pitch, int B, int T, int n_in, int co,
                                    int k, int d, int splits, float* part, float* dw, int n_valid, int add, int hmax, hipStream_t stream) {
    return tconv_wgrad_launch(x, x_pitch, gate, dy, dy_pitch, B, T, n_in, co, k, d, splits, part, dw, n_valid, add, hmax, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Squeeze-and-excitation backward, SE_CLIPS clips per workgroup as k_tcn_se: the time mean m and a1 = W1 m are recomputed, the gate is the
// forward's.  dgate = sum over time tiles of gpart (ascending); da2 = dgate * gate * (1 - gate); dhid = W2^T da2; da1 = dhid * swish'(a1);
// dm += W1^T da1 over the branches in order.  Written per clip: da2 [nb][B][n_in], da1 and hid [nb][B][R], mean and dm [B][n_in] — the
// weight gradients dW2 = sum_b da2 (x) hid, dW1 = sum_b da1 (x) m are k_tcn_se_wgrad's (b ascending).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tcn_se_bwd(const bf16_t* __restrict__ x, long x_pitch, int B, int T, int n_in, int R, int nb, int n_tt,
                                                    const bf16_t* __restrict__ w1, const bf16_t* __restrict__ w2, const float* __restrict__ gate,
                                                    const float* __restrict__ gpart, float* __restrict__ da2_o, float* __restrict__ da1_o,
                                                    float* __restrict__ hid_o, float* __restrict__ mean_o, float* __restrict__ dm_o) {
    extern __shared__ float se_sm[];
    float* mean = se_sm;                               // [SE_CLIPS][n_in]
    float* da2 = mean + SE_CLIPS * n_in;               // [SE_CLIPS][n_in]
    float* dm = da2 + SE_CLIPS * n_in;                 // [SE_CLIPS][n_in]
    float* a1 = dm + SE_CLIPS * n_in;                  // [SE_CLIPS][R]
    float* da1 = a1 + SE_CLIPS * R;                    // [SE_CLIPS][R]
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
        for (int i = 0; i < 8; ++i) {
            mean[cl * n_in + pc * 8 + i] = s[i] * inv_t;
            dm[cl * n_in + pc * 8 + i] = 0.f;
        }
    }
    for (int br = 0; br < nb; ++br) {
        __syncthreads();
        const bf16_t* w1b = w1 + (long)br * R * n_in;
        const bf16_t* w2b = w2 + (long)br * n_in * R;
        for (int j = wave; j < R; j += 4) {             // a1 = W1 m, exactly as the forward sums it
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
                if (lane == 0) a1[cl * R + j] = v;
            }
        }
        for (int p = tid; p < SE_CLIPS * n_in; p += 256) {
            const int cl = p / n_in, c = p - cl * n_in;
            float v = 0.f;
            if (b0 + cl < B) {
                const long base = ((long)br * B + b0 + cl);
                float dg = 0.f;
                for (int tt = 0; tt < n_tt; ++tt) dg += gpart[(base * n_tt + tt) * n_in + c];
                const float g = gate[base * n_in + c];
                v = dg * g * (1.0f - g);
                da2_o[base * n_in + c] = v;
            }
            da2[p] = v;
        }
        __syncthreads();
        for (int j = wave; j < R; j += 4) {             // dhid[j] = sum_c W2[c][j] da2[c]
            float d[SE_CLIPS];
#pragma unroll
            for (int cl = 0; cl < SE_CLIPS; ++cl) d[cl] = 0.f;
            for (int c = lane; c < n_in; c += 64) {
                const float w = bf2f(w2b[(long)c * R + j]);
#pragma unroll
                for (int cl = 0; cl < SE_CLIPS; ++cl) d[cl] = __builtin_fmaf(w, da2[cl * n_in + c], d[cl]);
            }
#pragma unroll
            for (int cl = 0; cl < SE_CLIPS; ++cl) {
                const float v = wave_sum(d[cl]);
                if (lane == 0) {
                    const float z = a1[cl * R + j];
                    const float g1 = v * swish_grad(z);
                    da1[cl * R + j] = g1;
                    if (b0 + cl < B) {
                        da1_o[((long)br * B + b0 + cl) * R + j] = g1;
                        hid_o[((long)br * B + b0 + cl) * R + j] = swish(z);
                    }
                }
            }
        }
        __syncthreads();
        for (int p = tid; p < SE_CLIPS * n_in; p += 256) {       // dm[c] += sum_j W1[j][c] da1[j]
            const int cl = p / n_in, c = p - cl * n_in;
            float s = 0.f;
            for (int j = 0; j < R; ++j) s = __builtin_fmaf(bf2f(w1b[(long)j * n_in + c]), da1[cl * R + j], s);
            dm[p] += s;
        }
    }
    __syncthreads();
    for (int p = tid; p < SE_CLIPS * n_in; p += 256) {
        const int cl = p / n_in, c = p - cl * n_in;
        if (b0 + cl < B) {
            mean_o[(long)(b0 + cl) * n_in + c] = mean[p];
            dm_o[(long)(b0 + cl) * n_in + c] = dm[p];
        }
    }
}

struct SEW { float* dw1[3]; float* dw2[3]; };
// blockIdx.y = branch, blockIdx.z = 0: dW1 [R][n_in], 1: dW2 [n_in][R]
__global__ __launch_bounds__(256) void k_tcn_se_wgrad(const float* __restrict__ da2, const float* __restrict__ da1, const float* __restrict__ hid,
                                                      const float* __restrict__ mean, int B, int n_in, int R, SEW o, int add) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n_in * R) return;
    const int br = blockIdx.y;
    float s = 0.f;
    float* dst;
    if (blockIdx.z == 0) {
        const int j = (int)(i / n_in), c = (int)(i - (long)j * n_in);
        for (int b = 0; b < B; ++b) s = __builtin_fmaf(da1[((long)br * B + b) * R + j], mean[(long)b * n_in + c], s);
        dst = o.dw1[br] + i;
    } else {
        const int c = (int)(i / R), j = (int)(i - (long)c * R);
        for (int b = 0; b < B; ++b) s = __builtin_fmaf(da2[((long)br * B + b) * n_in + c], hid[((long)br * B + b) * R + j], s);
        dst = o.dw2[br] + i;
    }
    *dst = add ? *dst + s : s;
}

// work: fp32 scratch of nb*B*n_in + 2*nb*B*R + B*n_in floats; dm fp32 [B][n_in]; dw: HOST table of 2 x nb pointers {dW1_0.., dW2_0..}
extern "C" int svsr_tcn_se_bwd(const void* x, int64_t x_pitch, int B, int T, int n_in, int R, int nb, const void* w1, const void* w2, const float* gate,
                               const float* gpart, float* work, float* dm, const int64_t* dw, int add, hipStream_t stream) {
    if (x == nullptr || w1 == nullptr || w2 == nullptr || gate == nullptr || gpart == nullptr || work == nullptr || dm == nullptr || dw == nullptr) return SVSR_ERR_ARG;
    if (B < 1 || T < 1 || n_in < 64 || n_in % 64 != 0 || x_pitch < n_in || x_pitch % 8 != 0 || nb < 1 || nb > 3) return SVSR_ERR_ARG;
    if (R < 4 || R % 4 != 0 || R > n_in) return SVSR_ERR_ARG;
    if ((((uintptr_t)x | (uintptr_t)w1) & 15) != 0) return SVSR_ERR_ARG;
    const size_t lds = (size_t)SE_CLIPS * (3 * n_in + 2 * R) * sizeof(float);
    if (lds > 64 * 1024) return SVSR_ERR_ARG;
    SEW o;
    for (int i = 0; i < 3; ++i) {
        o.dw1[i] = (float*)(uintptr_t)dw[i < nb ? i : 0];
        o.dw2[i] = (float*)(uintptr_t)dw[nb + (i < nb ? i : 0)];
        if (o.dw1[i] == nullptr || o.dw2[i] == nullptr) return SVSR_ERR_ARG;
    }
    const int n_tt = (T + TC_TILE - 1) / TC_TILE;
    float* da2 = work;
    float* da1 = da2 + (long)nb * B * n_in;
    float* hid = da1 + (long)nb * B * R;
    float* mean = hid + (long)nb * B * R;
    hipLaunchKernelGGL(k_tcn_se_bwd, dim3((unsigned)((B + SE_CLIPS - 1) / SE_CLIPS)), dim3(256), lds, stream, (const bf16_t*)x, (long)x_pitch, B, T, n_in, R,
                       nb, n_tt, (const bf16_t*)w1, (const bf16_t*)w2, gate, gpart, da2, da1, hid, mean, dm);
    int rc = svsr_check_launch();
    if (rc != SVSR_OK) return rc;
    const long n = (long)n_in * R;
    hipLaunchKernelGGL(k_tcn_se_wgrad, dim3((unsigned)((n + 255) / 256), (unsigned)nb, 2u), dim3(256), 0, stream, (const float*)da2, (const float*)da1,
                       (const float*)hid, (const float*)mean, B, n_in, R, o, add);
    return svsr_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// norm5 + masked mean backward: g[b][t][c] = dh[b][t][c] + dpooled[b][c] * mask[b][t] / (sum_t mask + 1e-6), then
//   running statistics (BS false): dx = bf16(g * scale[c]);  part[b][0][c] = sum_t g, part[b][1][c] = sum_t g * x (t ascending), folded over
//     the clips in order into sums [2][C];
//   batch statistics (BS true): dx = bf16(scale * (g - ca - xhat * cb)), xhat = (x - mean) * invstd, with ca, cb from the first launch's sums;
//     no sums of its own.
// ---------------------------------------------------------------------------------------------------------------------
template <bool BS>
__global__ __launch_bounds__(256) void k_tcn_norm_pool_bwd(const bf16_t* __restrict__ dh, const bf16_t* __restrict__ dpooled, const bf16_t* __restrict__ x,
                                                           long x_pitch, int B, int T, int C, const float* __restrict__ scale,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ ca, const float* __restrict__ cb,
                                                           const float* __restrict__ mask, bf16_t* __restrict__ dx, long dx_pitch, float* __restrict__ part) {
    const int pieces = C >> 3;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)B * pieces) return;
    const int b = (int)(p / pieces), c0 = (int)(p - (long)b * pieces) * 8;
    float sc[8], dp[8], mu[8], is[8], a0[8], b0[8], s0[8], s1[8];
    unpack8(*reinterpret_cast<const u32x4*>(dpooled + (long)b * C + c0), dp);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = scale[c0 + i];
        if (BS) { mu[i] = mean[c0 + i]; is[i] = invstd[c0 + i]; a0[i] = ca[c0 + i]; b0[i] = cb[c0 + i]; }
        else { s0[i] = 0.f; s1[i] = 0.f; }
    }
    float msum = 0.f;
    for (int t = 0; t < T; ++t) msum += mask[(long)b * T + t];
    const float inv = 1.0f / (msum + 1e-6f);
    for (int t = 0; t < T; ++t) {
        const long row = (long)b * T + t;
        float g[8], xv[8];
        unpack8(*reinterpret_cast<const u32x4*>(dh + row * C + c0), g);
        unpack8(*reinterpret_cast<const u32x4*>(x + row * x_pitch + c0), xv);
        const float m = mask[row] * inv;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            g[i] = __builtin_fmaf(dp[i], m, g[i]);
            if (BS) g[i] = sc[i] * ((g[i] - a0[i]) - (xv[i] - mu[i]) * is[i] * b0[i]);
            else {
                s0[i] += g[i];
                s1[i] = __builtin_fmaf(g[i], xv[i], s1[i]);
                g[i] *= sc[i];
            }
        }
        *reinterpret_cast<u32x4*>(dx + row * dx_pitch + c0) = pack8(g);
    }
    if (BS) return;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        part[((long)b * 2) * C + c0 + i] = s0[i];
        part[((long)b * 2 + 1) * C + c0 + i] = s1[i];
    }
}

// Both entry points' checks and launch; bs: mean / invstd / ca / cb are read, part is not
static int norm_pool_bwd_launch(bool bs, const void* dh, const void* dpooled, const void* x, int64_t x_pitch, int B, int T, int C, const float* scale,
                                const float* mean, const float* invstd, const float* ca, const float* cb, const float* mask, void* dx,
                                int64_t dx_pitch, float* part, hipStream_t stream) {
    if (dh == nullptr || dpooled == nullptr || x == nullptr || scale == nullptr || mask == nullptr || dx == nullptr) return SVSR_ERR_ARG;
    if (B < 1 || T < 1 || C < 8 || C % 8 != 0 || x_pitch < C || x_pitch % 8 != 0 || dx_pitch < C || dx_pitch % 8 != 0) return SVSR_ERR_ARG;
    if ((((uintptr_t)dh | (uintptr_t)dpooled | (uintptr_t)x | (uintptr_t)dx) & 15) != 0) return SVSR_ERR_ARG;
    const long n = (long)B * (C >> 3);
    if (n > (1L << 36)) return SVSR_ERR_ARG;
    hipLaunchKernelGGL(bs ? k_tcn_norm_pool_bwd<true> : k_tcn_norm_pool_bwd<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       (const bf16_t*)dh, (const bf16_t*)dpooled, (const bf16_t*)x, (long)x_pitch, B, T, C, scale, mean, invstd, ca, cb, mask, (bf16_t*)dx,
                       (long)dx_pitch, part);
    return svsr_check_launch();
}

extern "C" int svsr_tcn_norm_pool_bwd(const void* dh, const void* dpooled, const void* x, int64_t x_pitch, int B, int T, int C, const float* scale,
                                      const float* mask, void* dx, int64_t dx_pitch, float* part, float* sums, hipStream_t stream) {
    if (part == nullptr || sums == nullptr) return SVSR_ERR_ARG;
    int rc = norm_pool_bwd_launch(false, dh, dpooled, x, x_pitch, B, T, C, scale, nullptr, nullptr, nullptr, nullptr, mask, dx, dx_pitch, part, stream);
    if (rc != SVSR_OK) return rc;
    return svsr_tcn_fold(part, B, 2L * C, sums, 0, stream);
}

// norm5 under batch statistics (ca, cb from svsr_tcn_norm_pool_bwd's sums)
extern "C" int svsr_tcn_norm_pool_bwd_bs(const void* dh, const void* dpooled, const void* x, int64_t x_pitch, int B, int T, int C, const float* scale,
                                         const float* mean, const float* invstd, const float* ca, const float* cb, const float* mask, void* dx,
                                         int64_t dx_pitch, hipStream_t stream) {
    if (mean == nullptr || invstd == nullptr || ca == nullptr || cb == nullptr) return SVSR_ERR_ARG;
    return norm_pool_bwd_launch(true, dh, dpooled, x, x_pitch, B, T, C, scale, mean, invstd, ca, cb, mask, dx, dx_pitch, nullptr, stream);
}

// =====================================================================================================================
// Batch-statistic stages (loss_and_backend_grads(train_stats=True)).  The reference's TemporalConvLayer is Conv1d(padding = (k - 1) d) ->
// BatchNorm1d -> symmetric chomp -> activation: in training mode the statistics of a branch are taken over T + (k - 1) d positions a clip,
// of which (k - 1) d are chomped off afterwards.  So a stage is convolution -> statistics -> apply, on the EXTENDED axis: with
// h_i = (k_i - 1) d / 2 and hmax >= every h_i of the launch, a clip owns T_ext = T + 2 * hmax rows, the row of time t is t + hmax, and branch
// i's positions are the rows [hmax - h_i, hmax + h_i + T).  Rows of a branch's channels outside its own extent are never written by the
// forward and never read by anything; their gradient rows are written as zeros, so the data and weight gradients need no extent of their own.
// A 64-channel block never straddles two branches (co is a multiple of 64): the extent is uniform per workgroup.
// =====================================================================================================================
struct XGeo { int T, T_ext, hmax, co, h[3]; };

static bool xgeo_make(XGeo* g, int T, int hmax, int co, int nb, const int* h) {
    if (T < 1 || hmax < 0 || hmax > TC_HALO || co < 64 || co % 64 != 0 || nb < 1 || nb > 3) return false;
    g->T = T; g->T_ext = T + 2 * hmax; g->hmax = hmax; g->co = co;
    for (int i = 0; i < 3; ++i) {
        g->h[i] = h[i < nb ? i : 0];
        if (g->h[i] < 0 || g->h[i] > hmax) return false;
    }
    return true;
}

// svsr_tconv_fwd's convolution on the extended axis: the fp32 accumulators alone, acc[(b * T_ext + u)][i * co + c] for branch i and its own
// rows u.  branches: svsr_tconv_fwd's table; k, w and gate are read.
extern "C" int svsr_tconv_fwd_ext(const void* x, int64_t x_pitch, int B, int T, int n_in, int d, int nb, const int64_t* branches, int co, int hmax,
                                  float* acc, int64_t acc_pitch, hipStream_t stream) {
    return tconv_launch(x, x_pitch, B, T, n_in, d, nb, branches, co, SVSR_ACT_NONE, nullptr, 0, nullptr, 0, SVSR_ACT_NONE, acc, acc_pitch, TC_EXT, hmax,
                        stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Column statistics: per channel the mean and the CENTRED second moment sum (x - mean)^2 over the channel's own rows of every clip.
// One workgroup per (clip, 64 channels): the clip's mean first (four row lanes, added in order), then the squares against it; the clips are
// merged in ascending order with Chan's update (equal counts).  No atomics, no E[x^2] - mean^2.  TIn float: the extended accumulators;
// bf16_t: a [B*T][C] activation stack (norm5; hmax = 0).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float cs_ld(const float* p) { return *p; }
__device__ __forceinline__ float cs_ld(const bf16_t* p) { return bf2f(*p); }

template <typename TIn>
__global__ __launch_bounds__(256) void k_tcn_colstats(const TIn* __restrict__ x, long pitch, int C, XGeo g, float* __restrict__ part) {
    __shared__ float red[4][64];
    const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6;
    const int b = blockIdx.x, c = blockIdx.y * 64 + cl;
    const int h = g.h[(blockIdx.y * 64) / g.co];
    const int n = g.T + 2 * h;
    const TIn* base = x + ((long)b * g.T_ext + g.hmax - h) * pitch + c;
    float s = 0.f;
    for (int i = rl; i < n; i += 4) s += cs_ld(base + (long)i * pitch);
    red[rl][cl] = s;
    __syncthreads();
    const float m = (((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl]) / (float)n;
    float q = 0.f;
    for (int i = rl; i < n; i += 4) {
        const float dl = cs_ld(base + (long)i * pitch) - m;
        q = __builtin_fmaf(dl, dl, q);
    }
    __syncthreads();                                       // every thread has read the sums
    red[rl][cl] = q;
    __syncthreads();
    if (rl == 0) {
        part[((long)b * 2) * C + c] = m;
        part[((long)b * 2 + 1) * C + c] = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
    }
}

__global__ __launch_bounds__(256) void k_tcn_colstats_merge(const float* __restrict__ part, int B, int C, XGeo g, float* __restrict__ stats) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float n = (float)(g.T + 2 * g.h[c / g.co]);
    float mean = part[c], m2 = part[C + c];
    for (int b = 1; b < B; ++b) {
        const float na = n * (float)b, tot = na + n;
        const float dl = part[((long)b * 2) * C + c] - mean;
        mean = __builtin_fmaf(dl, n / tot, mean);
        m2 = (m2 + part[((long)b * 2 + 1) * C + c]) + dl * dl * (na * n / tot);
    }
    stats[c] = mean;
    stats[C + c] = m2;
}

// x: fp32 (is_bf16 0) or bf16 rows [B * (T + 2 * hmax)][pitch]; channels [i * co, (i + 1) * co) belong to branch i with half reach h[i];
// part: fp32 scratch [B][2][C]; stats fp32 [2][C] = (mean, sum (x - mean)^2) over B * (T + 2 * h[i]) rows
extern "C" int svsr_tcn_colstats(const void* x, int64_t pitch, int is_bf16, int B, int T, int C, int co, int hmax, int nb, const int* h, float* part,
                                 float* stats, hipStream_t stream) {
    XGeo g;
    if (x == nullptr || h == nullptr || part == nullptr || stats == nullptr || B < 1 || B > 65535 * 32) return SVSR_ERR_ARG;
    if (!xgeo_make(&g, T, hmax, co, nb, h) || C != nb * co || pitch < C || C / 64 > 65535) return SVSR_ERR_ARG;
    const dim3 grid((unsigned)B, (unsigned)(C / 64));
    if (is_bf16) hipLaunchKernelGGL(k_tcn_colstats<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)x, (long)pitch, C, g, part);
    else hipLaunchKernelGGL(k_tcn_colstats<float>, grid, dim3(256), 0, stream, (const float*)x, (long)pitch, C, g, part);
    int rc = svsr_check_launch();
    if (rc != SVSR_OK) return rc;
    hipLaunchKernelGGL(k_tcn_colstats_merge, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, (const float*)part, B, C, g, stats);
    return svsr_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// The epilogue of a batch-statistic stage and its backward.  k_tconv's epilogue continued: z = fma(acc, scale, shift), y = act(z), then
// dropout (element row * C + c of the stage's [B*T][C] output: y * m with m = 1 / (1 - p) where kept, 0 where dropped), then + res and
// res_act.  Backward: du = dy * res_act'(u) (dy without a residual), dd = du * m, g = dd * act'(z).
// ---------------------------------------------------------------------------------------------------------------------
struct PArgs {
    const float* acc; const float* scale; const float* shift; const float* slope; const bf16_t* res; const bf16_t* dy;
    const float* mean; const float* invstd; const float* ca; const float* cb;
    bf16_t* out; bf16_t* dres; bf16_t* dacc; float* part;
    long acc_pitch, res_pitch, dy_pitch, out_pitch, dres_pitch, dacc_pitch, rows;
    XGeo g;
    int C, act, res_act, drop;
    unsigned key, thresh;
    float dscale;
};

__device__ __forceinline__ float pa_mult(const PArgs& a, long row, int c) {
    if (!a.drop) return 1.f;
    return drop_keep(a.key, a.thresh, (unsigned)(row * a.C + c)) ? a.dscale : 0.f;
}

__device__ __forceinline__ float pa_act(int act, float z, float slope) {
    if (act == SVSR_ACT_SWISH) return swish(z);
    if (act == TC_ACT_PRELU) return z >= 0.f ? z : z * slope;
    if (act == SVSR_ACT_RELU) return fmaxf(z, 0.f);
    return z;
}

// -> g; du (the residual branch's gradient) and z by reference
__device__ __forceinline__ float pa_grad(const PArgs& a, long row, int c, float ac, float sc, float sh, float slope, float& du, float& z, float& dd) {
    z = __builtin_fmaf(ac, sc, sh);
    du = bf2f(a.dy[row * a.dy_pitch + c]);
    const float m = pa_mult(a, row, c);
    if (a.res != nullptr) {
        float y = pa_act(a.act, z, slope);
        if (a.drop) y *= m;
        const float u = y + bf2f(a.res[row * a.res_pitch + c]);
        if (a.res_act == SVSR_ACT_SWISH) du *= swish_grad(u);
    }
    dd = a.drop ? du * m : du;
    float g = dd;
    if (a.act == SVSR_ACT_SWISH) g = dd * swish_grad(z);
    else if (a.act == TC_ACT_PRELU) g = z >= 0.f ? dd : dd * slope;
    else if (a.act == SVSR_ACT_RELU) g = z > 0.f ? dd : 0.f;
    return g;
}

__global__ __launch_bounds__(256) void k_tconv_apply(PArgs a) {
    const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6;
    const int c = blockIdx.y * 64 + cl;
    const float sc = a.scale[c], sh = a.shift[c];
    const float slope = a.act == TC_ACT_PRELU ? a.slope[c] : 0.f;
    const long r0 = (long)blockIdx.x * EB_ROWS;
    for (int i = rl; i < EB_ROWS; i += 4) {
        const long row = r0 + i;
        if (row >= a.rows) break;
        const long b = row / a.g.T;
        const long er = b * a.g.T_ext + a.g.hmax + (row - b * a.g.T);
        float v = pa_act(a.act, __builtin_fmaf(a.acc[er * a.acc_pitch + c], sc, sh), slope);
        if (a.drop) v *= pa_mult(a, row, c);
        if (a.res != nullptr) {
            v += bf2f(a.res[row * a.res_pitch + c]);
            if (a.res_act == SVSR_ACT_SWISH) v = swish(v);
        }
        a.out[row * a.out_pitch + c] = f2bf(v);
    }
}

// Pass 1 of the backward: per channel the sums of g, g * acc, dd * min(z, 0) (the PReLU slope) and du over the T interior rows, and dres = du
__global__ __launch_bounds__(256) void k_tconv_epi_bwd_bs(PArgs a) {
    __shared__ float red[4][4][64];
    const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6;
    const int c = blockIdx.y * 64 + cl;
    const float sc = a.scale[c], sh = a.shift[c];
    const float slope = a.act == TC_ACT_PRELU ? a.slope[c] : 0.f;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const long r0 = (long)blockIdx.x * EB_ROWS;
    for (int i = rl; i < EB_ROWS; i += 4) {
        const long row = r0 + i;
        if (row >= a.rows) break;
        const long b = row / a.g.T;
        const long er = b * a.g.T_ext + a.g.hmax + (row - b * a.g.T);
        const float ac = a.acc[er * a.acc_pitch + c];
        float du, z, dd;
        const float g = pa_grad(a, row, c, ac, sc, sh, slope, du, z, dd);
        if (a.res != nullptr) {
            a.dres[row * a.dres_pitch + c] = f2bf(du);
            s3 += du;
        }
        if (a.act == TC_ACT_PRELU) s2 += dd * fminf(z, 0.f);
        s0 += g;
        s1 = __builtin_fmaf(g, ac, s1);
    }
    red[0][rl][cl] = s0; red[1][rl][cl] = s1; red[2][rl][cl] = s2; red[3][rl][cl] = s3;
    __syncthreads();
    const float t = ((red[rl][0][cl] + red[rl][1][cl]) + red[rl][2][cl]) + red[rl][3][cl];
    a.part[((long)blockIdx.x * 4 + rl) * a.C + c] = t;
}

// Pass 2: the gradient of every extended accumulator, dacc = bf16(scale * (g - ca - xhat * cb)) on the branch's own rows (g recomputed on the
// T interior rows, 0 on the chomped ones; xhat = (acc - mean) * invstd; ca = sum g / N, cb = sum g xhat / N from pass 1), zeros elsewhere.
__global__ __launch_bounds__(256) void k_tconv_bn_bwd(PArgs a) {
    const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6;
    const int c = blockIdx.y * 64 + cl;
    const int h = a.g.h[(blockIdx.y * 64) / a.g.co];
    const float sc = a.scale[c], sh = a.shift[c], mean = a.mean[c], istd = a.invstd[c], ca = a.ca[c], cb = a.cb[c];
    const float slope = a.act == TC_ACT_PRELU ? a.slope[c] : 0.f;
    const long r0 = (long)blockIdx.x * EB_ROWS, erows = a.rows / a.g.T * a.g.T_ext;
    for (int i = rl; i < EB_ROWS; i += 4) {
        const long er = r0 + i;
        if (er >= erows) break;
        const long b = er / a.g.T_ext;
        const int u = (int)(er - b * a.g.T_ext), t = u - a.g.hmax;
        float v = 0.f;
        if (t >= -h && t < a.g.T + h) {
            const float ac = a.acc[er * a.acc_pitch + c];
            float g = 0.f;
            if (t >= 0 && t < a.g.T) {
                float du, z, dd;
                g = pa_grad(a, b * a.g.T + t, c, ac, sc, sh, slope, du, z, dd);
            }
            v = sc * ((g - ca) - (ac - mean) * istd * cb);
        }
        a.dacc[er * a.dacc_pitch + c] = f2bf(v);
    }
}

static bool pa_fill(PArgs* a, const float* acc, int64_t acc_pitch, int B, int T, int C, int co, int hmax, int nb, const int* h, int act,
                    const float* scale, const float* shift, const float* slope, const void* res, int64_t res_pitch, int res_act, unsigned drop_key,
                    float drop_p) {
    if (acc == nullptr || scale == nullptr || shift == nullptr || h == nullptr || B < 1 || (long)B * (T + 2L * TC_HALO) > (1L << 30)) return false;
    if (!xgeo_make(&a->g, T, hmax, co, nb, h) || C != nb * co || C / 64 > 65535 || acc_pitch < C) return false;
    if (act != SVSR_ACT_NONE && act != SVSR_ACT_RELU && act != SVSR_ACT_SWISH && act != TC_ACT_PRELU) return false;
    if (act == TC_ACT_PRELU && slope == nullptr) return false;
    if (res_act != SVSR_ACT_NONE && res_act != SVSR_ACT_SWISH) return false;
    if (res != nullptr && res_pitch < C) return false;
    if (!(drop_p >= 0.f && drop_p < 1.f)) return false;
    if (drop_p > 0.f && (long)B * T * C > (1L << 32)) return false;          // the mask's element index row * C + c is a 32-bit counter
    a->acc = acc; a->scale = scale; a->shift = shift; a->slope = slope; a->res = (const bf16_t*)res; a->dy = nullptr;
    a->mean = nullptr; a->invstd = nullptr; a->ca = nullptr; a->cb = nullptr; a->out = nullptr; a->dres = nullptr; a->dacc = nullptr; a->part = nullptr;
    a->acc_pitch = acc_pitch; a->res_pitch = res_pitch; a->dy_pitch = 0; a->out_pitch = 0; a->dres_pitch = 0; a->dacc_pitch = 0;
    a->rows = (long)B * T; a->C = C; a->act = act; a->res_act = res_act;
    a->drop = drop_p > 0.f; a->key = drop_key;
    const double th = (double)drop_p * 4294967296.0;
    a->thresh = th >= 4294967295.0 ? 4294967295u : (unsigned)th;
    a->dscale = 1.0f / (1.0f - drop_p);
    return true;
}

// acc fp32 [B * (T + 2 * hmax)][acc_pitch] (svsr_tconv_fwd_ext) -> out bf16 [B * T][out_pitch], channels [0, C) (C = nb * co).
// drop_p > 0: dropout with the key drop_key (dropout.site_key), element index row * C + c.
extern "C" int svsr_tconv_apply(const float* acc, int64_t acc_pitch, int B, int T, int C, int co, int hmax, int nb, const int* h, int act,
                                const float* scale, const float* shift, const float* slope, const void* res, int64_t res_pitch, int res_act,
                                unsigned drop_key, float drop_p, void* out, int64_t out_pitch, hipStream_t stream) {
    PArgs a;
    if (out == nullptr || out_pitch < C) return SVSR_ERR_ARG;
    if (!pa_fill(&a, acc, acc_pitch, B, T, C, co, hmax, nb, h, act, scale, shift, slope, res, res_pitch, res_act, drop_key, drop_p)) return SVSR_ERR_ARG;
    a.out = (bf16_t*)out; a.out_pitch = out_pitch;
    hipLaunchKernelGGL(k_tconv_apply, dim3((unsigned)((a.rows + EB_ROWS - 1) / EB_ROWS), (unsigned)(C / 64)), dim3(256), 0, stream, a);
    return svsr_check_launch();
}

// Pass 1.  part: fp32 scratch [ceil(B * T / 64)][4][C]; sums fp32 [4][C] as svsr_tconv_epi_bwd's; dres bf16 [B * T][dres_pitch] with a residual
extern "C" int svsr_tconv_epi_bwd_bs(const void* dy, int64_t dy_pitch, const float* acc, int64_t acc_pitch, int B, int T, int C, int co, int hmax, int nb,
                                     const int* h, int act, const float* scale, const float* shift, const float* slope, const void* res,
                                     int64_t res_pitch, int res_act, unsigned drop_key, float drop_p, void* dres, int64_t dres_pitch, float* part,
                                     float* sums, hipStream_t stream) {
    PArgs a;
    if (dy == nullptr || dy_pitch < C || part == nullptr || sums == nullptr) return SVSR_ERR_ARG;
    if (res != nullptr && (dres == nullptr || dres_pitch < C)) return SVSR_ERR_ARG;
    if (!pa_fill(&a, acc, acc_pitch, B, T, C, co, hmax, nb, h, act, scale, shift, slope, res, res_pitch, res_act, drop_key, drop_p)) return SVSR_ERR_ARG;
    a.dy = (const bf16_t*)dy; a.dy_pitch = dy_pitch; a.dres = (bf16_t*)dres; a.dres_pitch = dres_pitch; a.part = part;
    const long blocks = (a.rows + EB_ROWS - 1) / EB_ROWS;
    hipLaunchKernelGGL(k_tconv_epi_bwd_bs, dim3((unsigned)blocks, (unsigned)(C / 64)), dim3(256), 0, stream, a);
    int rc = svsr_check_launch();
    if (rc != SVSR_OK) return rc;
    return svsr_tcn_fold(part, (int)blocks, 4L * C, sums, 0, stream);
}

// Pass 2.  mean, invstd, ca, cb fp32 [C]; dacc bf16 [B * (T + 2 * hmax)][dacc_pitch]: every row of channels [0, C) is written
extern "C" int svsr_tconv_bn_bwd(const void* dy, int64_t dy_pitch, const float* acc, int64_t acc_pitch, int B, int T, int C, int co, int hmax, int nb,
                                 const int* h, int act, const float* scale, const float* shift, const float* slope, const void* res, int64_t res_pitch,
                                 int res_act, unsigned drop_key, float drop_p, const float* mean, const float* invstd, const float* ca,
                                 const float* cb, void* dacc, int64_t dacc_pitch, hipStream_t stream) {
    PArgs a;
    if (dy == nullptr || dy_pitch < C || mean == nullptr || invstd == nullptr || ca == nullptr || cb == nullptr || dacc == nullptr || dacc_pitch < C)
        return SVSR_ERR_ARG;
    if (!pa_fill(&a, acc, acc_pitch, B, T, C, co, hmax, nb, h, act, scale, shift, slope, res, res_pitch, res_act, drop_key, drop_p)) return SVSR_ERR_ARG;
    a.dy = (const bf16_t*)dy; a.dy_pitch = dy_pitch; a.mean = mean; a.invstd = invstd; a.ca = ca; a.cb = cb;
    a.dacc = (bf16_t*)dacc; a.dacc_pitch = dacc_pitch;
    const long erows = (long)B * a.g.T_ext;
    hipLaunchKernelGGL(k_tconv_bn_bwd, dim3((unsigned)((erows + EB_ROWS - 1) / EB_ROWS), (unsigned)(C / 64)), dim3(256), 0, stream, a);
    return svsr_check_launch();
}
