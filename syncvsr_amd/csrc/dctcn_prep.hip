// Device-side training inputs of the DC-TCN word-level path, gfx950, wave64: what the reference's LRWDatasetForDCTCN does per clip in the
// loader workers (LRW/video/src/data.py:70-139: 2 x / 255 - 1, _mask_frames, _trim_frames, then the transform chain, which divides by 255
// a SECOND time in front of Normalize) and the clip mixup of its module (lightning.py:264-270), from the stored uint8 crops and a few
// host-drawn integers per clip (syncvsr_amd/augment.py DeviceDCTCNPipeline.plan), in at most three launches per batch:
//   * k_dctcn_clip_sums: exact integer sums [B][T] of the stored frames — what _mask_frames' clip mean is made of
//   * k_dctcn_clip_mix:  dst[b][0][t] = Normalize(lerp(val(b, t), val(b - 1, t), lam)); every output element is written once
//   * k_dctcn_wave_trim: the waveform rolled by ashift and zeroed from azero on
// The spatial sampling is csrc/clip_sample.h.  No atomics and no order that depends on arrival: every output is a pure function of the
// inputs, whatever the grid.
#include "common.h"
#include "clip_sample.h"

#define DT_MAXT 256          // frames per clip
#define DT_ROWS 32           // output rows per item of k_dctcn_clip_mix
#define DT_ROW 9             // ints per clip: {top, left, h, w, flip, shift, trunc, mask_off, mask_len}

// ---------------------------------------------------------------------------------------------------------------------
// Frame sums.  One item = one stored frame (clip b, frame t), walked in a grid-stride loop by whole workgroups.  Integer adds: the
// result is exact and does not depend on the partition (Hs * Ws <= 2^24 keeps 255 Hs Ws inside 32 bits).  With `vec` (frames that are
// whole, aligned 4-byte words) a thread reads four pixels at a time.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dctcn_clip_sums(const unsigned char* __restrict__ src, unsigned* __restrict__ fsum, long frames, int HWs,
                                                         int vec) {
    __shared__ unsigned red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long item = blockIdx.x; item < frames; item += gridDim.x) {
        const unsigned char* f = src + item * HWs;
        unsigned acc = 0;
        if (vec) {
            const unsigned* f4 = reinterpret_cast<const unsigned*>(f);
            for (int q = threadIdx.x; q < (HWs >> 2); q += 256) {
                const unsigned v = f4[q];
                acc += (v & 0xffu) + ((v >> 8) & 0xffu) + ((v >> 16) & 0xffu) + (v >> 24);
            }
        } else {
            for (int q = threadIdx.x; q < HWs; q += 256) acc += f[q];
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) red[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) fsum[item] = red[0] + red[1] + red[2] + red[3];
        __syncthreads();                                          // (red is rewritten by the next item)
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Mix.  val(s, t), the value of frame t of clip s in front of Normalize, is one of
//   0                       t >= trunc_s                                        (trimmed)
//   m_s / 255               the source frame ts = (t - shift_s) mod T lies in clip s's mask run;  m_s = 2 S_s / (255 T Hs Ws) - 1 with
//                           S_s the clip's T frame sums added in 64-bit integer, evaluated in double and rounded once
//   (2 u / 255 - 1) / 255   u = clip_sample of stored frame ts with clip s's window and flip
// The first two are constants of the frame: DtSource.f is null and .c holds the value.  All table entries are clamped (trunc, mask_off
// into [0, T], mask_len into [0, T - mask_off], shift reduced mod T, the window by clip_window_row): nothing outside src is read.
// ---------------------------------------------------------------------------------------------------------------------
struct DtSource { const unsigned char* f; float c; ClipWindow w; };

__device__ __forceinline__ DtSource dt_source(const unsigned char* __restrict__ src, const int* __restrict__ table, const unsigned* __restrict__ fsum,
                                              int s, int t, int T, int Hs, int Ws) {
    const int* row = table + (long)s * DT_ROW;
    DtSource r;
    r.f = nullptr;
    r.c = 0.f;
    r.w = clip_window_row(row, Hs, Ws);
    int trunc = row[6], off = row[7], len = row[8];
    trunc = trunc < 0 ? 0 : (trunc > T ? T : trunc);
    if (t >= trunc) return r;
    int ts = (t - row[5] % T) % T;                                // (|shift % T| < T: no overflow)
    if (ts < 0) ts += T;
    off = off < 0 ? 0 : (off > T ? T : off);
    len = len < 0 ? 0 : (len > T - off ? T - off : len);
    if (fsum != nullptr && ts >= off && ts < off + len) {
        unsigned long long S = 0;
        for (int i = 0; i < T; ++i) S += fsum[(long)s * T + i];      // (uniform in the workgroup)
        const double m = 2.0 * (double)S / (255.0 * (double)T * (double)Hs * (double)Ws) - 1.0;
        r.c = (float)(m / 255.0);
        return r;
    }
    r.f = src + ((long)s * T + ts) * Hs * Ws;
    return r;
}

__device__ __forceinline__ float dt_value(const DtSource& s, int Ws, int y, int x, int H, int W) {
    if (s.f == nullptr) return s.c;
    return __builtin_fmaf(clip_sample(s.f, s.w, Ws, y, x, H, W), 2.0f / 255.0f, -1.0f) * (1.0f / 255.0f);
}

// One item = (sample b, frame t, block of DT_ROWS output rows).  With lam != 0 the neighbour b' = (b - 1 + B) mod B is evaluated at the same
// (t, y, x) with ITS row of the table and x = a + lam (n - a); with lam == 0 it is not touched.  An item whose sources are all constants
// is a fill.  A thread produces four neighbouring pixels of a row and stores them as one 16-byte vector where the rows are 16-byte
// aligned (W % 4 == 0 and dst aligned); otherwise pixel by pixel.
__global__ __launch_bounds__(256) void k_dctcn_clip_mix(const unsigned char* __restrict__ src, const int* __restrict__ table,
                                                        const unsigned* __restrict__ fsum, float* __restrict__ dst, int B, int T, int Hs, int Ws,
                                                        int H, int W, float lam, float mean, float inv_std, int vec) {
    const int nrb = (H + DT_ROWS - 1) / DT_ROWS, W4 = (W + 3) >> 2;
    const long items = (long)B * T * nrb;
    const bool mix = lam != 0.f;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const int rb = (int)(item % nrb);
        const long bt = item / nrb;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const int y_lo = rb * DT_ROWS, rows = H - y_lo < DT_ROWS ? H - y_lo : DT_ROWS;
        float* out = dst + (bt * H + y_lo) * W;
        const DtSource a = dt_source(src, table, fsum, b, t, T, Hs, Ws);
        DtSource n = a;
        if (mix) n = dt_source(src, table, fsum, b == 0 ? B - 1 : b - 1, t, T, Hs, Ws);
        if (a.f == nullptr && n.f == nullptr) {                    // (the same in every thread of the workgroup)
            const float x = mix ? a.c + lam * (n.c - a.c) : a.c;
            const float v = (x - mean) * inv_std;
            if (vec) {
                const f32x4 v4 = {v, v, v, v};
                for (int q = threadIdx.x; q < rows * W4; q += 256) reinterpret_cast<f32x4*>(out)[q] = v4;
            } else {
                for (int q = threadIdx.x; q < rows * W; q += 256) out[q] = v;
            }
            continue;
        }
        for (int q = threadIdx.x; q < rows * W4; q += 256) {
            const int yr = q / W4, x4 = (q - yr * W4) * 4;
            float px[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x4 + j < W ? x4 + j : W - 1;          // (a ragged last quad samples its last column again; only x < W is stored)
                float v = dt_value(a, Ws, y_lo + yr, x, H, W);
                if (mix) v = v + lam * (dt_value(n, Ws, y_lo + yr, x, H, W) - v);
                px[j] = (v - mean) * inv_std;
            }
            if (vec) {
                const f32x4 v4 = {px[0], px[1], px[2], px[3]};
                reinterpret_cast<f32x4*>(out)[q] = v4;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x4 + j < W) out[yr * W + x4 + j] = px[j];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Waveform trim.  One thread = four neighbouring samples of one clip: out[b][i] = i < azero_b ? wave[b][(i - ashift_b) mod L] : 0, azero
// clamped into [0, L], ashift reduced mod L.  The reads are shifted, so they stay scalar; the store is one 16-byte vector where the rows
// are 16-byte aligned (L % 4 == 0 and out aligned).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dctcn_wave_trim(const float* __restrict__ wave, const int* __restrict__ table, float* __restrict__ out, int B,
                                                         int L, int vec) {
    const long L4 = ((long)L + 3) >> 2, quads = (long)B * L4;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
        const int b = (int)(q / L4), i0 = (int)(q - (long)b * L4) * 4;
        const float* w = wave + (long)b * L;
        float* o = out + (long)b * L;
        int azero = table[2 * b + 1];
        azero = azero < 0 ? 0 : (azero > L ? L : azero);
        const int sh = table[2 * b] % L;                          // (|sh| < L)
        float px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + j < L ? i0 + j : L - 1;
            int k = i - sh;                                       // in (-L, 2 L)
            k = k < 0 ? k + L : (k >= L ? k - L : k);
            px[j] = i < azero ? w[k] : 0.f;
        }
        if (vec) {
            const f32x4 v4 = {px[0], px[1], px[2], px[3]};
            *reinterpret_cast<f32x4*>(o + i0) = v4;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < L) o[i0 + j] = px[j];
        }
    }
}

static inline int dt_grid(long items, int max_blocks) {
    const long g = items < 1 ? 1 : items;
    const int cap = max_blocks > 0 ? max_blocks : 16384;
    return (int)(g > cap ? cap : g);
}

extern "C" {

/* exact integer sums of the stored frames; see include/syncvsr_hip.h */
int svsr_dctcn_clip_sums(const void* src_u8, unsigned* frame_sums, int B, int T, int Hs, int Ws, int max_blocks, hipStream_t stream) {
    if (B < 1 || T < 1 || T > DT_MAXT || Hs < 1 || Ws < 1 || (long)Hs * Ws > (1 << 24) || (long)B * T > (1 << 24) || max_blocks < 0 ||
        src_u8 == nullptr || frame_sums == nullptr)
        return SVSR_ERR_ARG;
    const int HWs = Hs * Ws, vec = HWs % 4 == 0 && ((uintptr_t)src_u8 & 3) == 0;
    hipLaunchKernelGGL(k_dctcn_clip_sums, dim3(dt_grid((long)B * T, max_blocks)), dim3(256), 0, stream, (const unsigned char*)src_u8, frame_sums,
                       (long)B * T, HWs, vec);
    return svsr_check_launch();
}

/* uint8 clips -> fp32 [B][1][T][H][W]: scaling, frame mask, trim, crop / flip, mixup with the batch neighbour, Normalize; see include/syncvsr_hip.h */
int svsr_dctcn_clip_mix(const void* src_u8, const int* table, const unsigned* frame_sums, float* dst, int B, int T, int Hs, int Ws, int H, int W,
                        float lam, float mean, float std, int max_blocks, hipStream_t stream) {
    if (B < 1 || T < 1 || T > DT_MAXT || Hs < 1 || Ws < 1 || H < 1 || W < 1 || (long)Hs * Ws > (1 << 24) || (long)H * W > (1 << 24) ||
        (long)B * T > (1 << 24) || !(std > 0.f) || !(lam >= 0.f && lam <= 0.5f) || max_blocks < 0 || src_u8 == nullptr || table == nullptr ||
        dst == nullptr)
        return SVSR_ERR_ARG;
    const long items = (long)B * T * ((H + DT_ROWS - 1) / DT_ROWS);
    const int vec = W % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    hipLaunchKernelGGL(k_dctcn_clip_mix, dim3(dt_grid(items, max_blocks)), dim3(256), 0, stream, (const unsigned char*)src_u8, table, frame_sums, dst,
                       B, T, Hs, Ws, H, W, lam, mean, 1.0f / std, vec);
    return svsr_check_launch();
}

/* waveforms rolled and zeroed behind a length, out of place; see include/syncvsr_hip.h */
int svsr_dctcn_wave_trim(const float* wave, const int* table, float* out, int B, int L, int max_blocks, hipStream_t stream) {
    if (B < 1 || L < 1 || L > (1 << 30) || max_blocks < 0 || wave == nullptr || table == nullptr || out == nullptr ||
        out == wave)
        return SVSR_ERR_ARG;
    const long blocks = ((long)B * (((long)L + 3) >> 2) + 255) / 256;
    const int vec = L % 4 == 0 && ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL(k_dctcn_wave_trim, dim3(dt_grid(blocks, max_blocks)), dim3(256), 0, stream, wave, table, out, B, L, vec);
    return svsr_check_launch();
}

}  // extern "C"
