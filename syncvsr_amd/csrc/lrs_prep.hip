// Device-side input pipeline of the sentence-level (LRS) path, gfx950, wave64: what the reference runs per sample in its dataloader
// workers (LRS/video/datamodule/transforms.py VideoTransform("train") / AudioTransform, av_dataset.py:30-41 for val / test) as one video
// launch and two audio launches per batch; the random decisions are made on the host (syncvsr_amd/lrs_data.py DeviceLRSPipeline.draw).
//   * k_lrs_clip_prep: packed uint8 frames of clips of different lengths -> fp32 [B][Tpad][1][H][W], padding frames and masked frames
//     included (every output element is written: no zero-fill launch beside it)
//   * k_wave_stats / k_wave_apply: babble noise at a drawn SNR (torchaudio.functional.add_noise) and the layer norm over the whole
//     waveform, per clip over its real samples
// No float atomics and no order that depends on arrival: every output is a pure function of the inputs, whatever the grid.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------
// Video.  One item = (clip b, frame t, block of LP_ROWS output rows); workgroups walk the items in a grid-stride loop.  A frame t of clip
// b is the packed frame off[b] + t when t < T_b = off[b + 1] - off[b]; frames behind T_b are padding (0.0, what collate_pad pads the
// normalised clip with) and a frame marked in tmask is a zeroed frame behind Normalize, (0 - mean) / std (AdaptiveTimeMask in front of
// Normalize, transforms.py:101).  The sampling formulas are k_clip_prep's (csrc/loss_optim.hip; the same formulas, not bit-identical results): bilinear,
// align_corners = False, no antialias, source coordinates clamped to the window, the flip mirrors the output.
// A thread produces four neighbouring pixels of a row and stores them as one 16-byte vector where the rows are 16-byte aligned (W % 4 == 0
// and dst aligned); otherwise pixel by pixel.
// ---------------------------------------------------------------------------------------------------------------------
#define LP_ROWS 32

__global__ __launch_bounds__(256) void k_lrs_clip_prep(const unsigned char* __restrict__ src, const int* __restrict__ off,
                                                       const int* __restrict__ params, const unsigned char* __restrict__ tmask,
                                                       float* __restrict__ dst, int B, int Tpad, long total_frames, int Hs, int Ws, int H, int W,
                                                       float mean, float inv_std, float masked, int vec) {
    const int nrb = (H + LP_ROWS - 1) / LP_ROWS, W4 = (W + 3) >> 2;
    const long items = (long)B * Tpad * nrb;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const int rb = (int)(item % nrb);
        const long bt = item / nrb;
        const int t = (int)(bt % Tpad), b = (int)(bt / Tpad);
        const int y_lo = rb * LP_ROWS, rows = H - y_lo < LP_ROWS ? H - y_lo : LP_ROWS;
        float* out = dst + (bt * H + y_lo) * W;
        const long first = off[b], frame = first + t;
        // a frame outside the packed buffer is padding whatever the offsets say: nothing is read outside src
        const bool real = t < off[b + 1] - first && first >= 0 && frame < total_frames;
        if (!real || (tmask != nullptr && tmask[bt] != 0)) {
            const float v = real ? masked : 0.f;
            if (vec) {
                const f32x4 v4 = {v, v, v, v};
                for (int q = threadIdx.x; q < rows * W4; q += 256) reinterpret_cast<f32x4*>(out)[q] = v4;
            } else {
                for (int q = threadIdx.x; q < rows * W; q += 256) out[q] = v;
            }
            continue;
        }
        int top = params[b * 5 + 0], left = params[b * 5 + 1], ch = params[b * 5 + 2], cw = params[b * 5 + 3];
        const int flip = params[b * 5 + 4];
        // the window is clamped into the stored frame: no read outside it whatever the host drew
        top = top < 0 ? 0 : (top > Hs - 1 ? Hs - 1 : top);
        left = left < 0 ? 0 : (left > Ws - 1 ? Ws - 1 : left);
        ch = ch < 1 ? 1 : (ch > Hs - top ? Hs - top : ch);
        cw = cw < 1 ? 1 : (cw > Ws - left ? Ws - left : cw);
        const unsigned char* f = src + frame * Hs * Ws + (long)top * Ws + left;
        const float sy = (float)ch / (float)H, sx = (float)cw / (float)W;
        for (int q = threadIdx.x; q < rows * W4; q += 256) {
            const int yr = q / W4, x4 = (q - yr * W4) * 4;
            // source coordinates inside the window (pixel centres), clamped to the window like torch's upsample_bilinear2d
            float fy = ((float)(y_lo + yr) + 0.5f) * sy - 0.5f;
            fy = fmaxf(fy, 0.f);
            int y0 = (int)fy;
            if (y0 > ch - 1) y0 = ch - 1;
            const int y1 = y0 + 1 < ch ? y0 + 1 : ch - 1;
            const float wy = fy - (float)y0;
            const unsigned char* r0 = f + y0 * Ws;
            const unsigned char* r1 = f + y1 * Ws;
            float px[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x4 + j < W ? x4 + j : W - 1;          // (a ragged last quad samples its last column again; only x < W is stored)
                const int xo = flip ? W - 1 - x : x;
                float fx = ((float)xo + 0.5f) * sx - 0.5f;
                fx = fmaxf(fx, 0.f);
                int x0 = (int)fx;
                if (x0 > cw - 1) x0 = cw - 1;
                const int x1 = x0 + 1 < cw ? x0 + 1 : cw - 1;
                const float wx = fx - (float)x0;
                const float v00 = r0[x0], v01 = r0[x1], v10 = r1[x0], v11 = r1[x1];
                const float v = (1.f - wy) * ((1.f - wx) * v00 + wx * v01) + wy * ((1.f - wx) * v10 + wx * v11);
                px[j] = (v * (1.0f / 255.0f) - mean) * inv_std;
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
// Audio.  Per clip b over its L = len[b] real samples, x = wave (int16: v / 32768, exact in fp32), n = noise[nstart[b] + i]:
//   Ex = sum x^2, En = sum n^2, scale = sqrt(Ex / En) * 10^(-snr_db / 20)         (torchaudio.functional.add_noise)
//   y = x + scale * n,  out = (y - mean(y)) / sqrt(var_biased(y) + eps)           (F.layer_norm(x, x.shape, eps = 1e-8))
// scale is 0 where Ex == 0 or En == 0 (the quotient would be 0 / 0 or x / 0), where no noise is given and where the clip's noise segment
// does not lie inside the bank (nothing is read outside it): the noise-free normalisation.  snr_db = 999999 underflows 10^(-snr_db / 20)
// to 0, so scale is an exact 0 there as well.
// mean(y) and var(y) need scale, which needs the whole clip, so the first launch sums the five moments they are made of,
//   Sx, Sn, Sxx, Snn, Sxn:   sum y = Sx + scale Sn,   sum y^2 = Sxx + 2 scale Sxn + scale^2 Snn,
// in DOUBLE (the products of two fp32 values are exact in it): E[y^2] - mean^2 of a waveform with a DC offset of 0.5 and an amplitude of
// 1e-3 cancels 6 decimal digits, all of fp32's and a third of fp64's.  One partial row of 5 doubles per WP_CHUNK samples of a clip — the
// partition depends on the lengths alone, not on the grid — each summed in a fixed order (a thread its samples in index order, the 64 lanes
// in a butterfly, the 4 waves in wave order); the second launch adds a clip's rows in index order, and out is also evaluated in double and
// rounded once.  Two runs, and two grids, give the same bits.
// ---------------------------------------------------------------------------------------------------------------------
#define WP_CHUNK 4096
#define WP_SUMS 5

struct WaveArgs {
    const void* wave; int wave_i16;
    const int* len; const float* noise; long Nn; const int* nstart; const float* snr_db;
    float* out; int B, Spad; double* part;        // part: [B][ceil(Spad / WP_CHUNK)][WP_SUMS]
};

__device__ __forceinline__ float wave_load(const WaveArgs& a, long i) {
    return a.wave_i16 ? (float)reinterpret_cast<const short*>(a.wave)[i] * (1.0f / 32768.0f) : reinterpret_cast<const float*>(a.wave)[i];
}
__device__ __forceinline__ int wave_len(const WaveArgs& a, int b) { const int L = a.len[b]; return L < 0 ? 0 : (L > a.Spad ? a.Spad : L); }
// the clip's noise segment, or null where it would leave the bank
__device__ __forceinline__ const float* wave_noise(const WaveArgs& a, int b, int L) {
    if (a.noise == nullptr) return nullptr;
    const long s = a.nstart[b];
    return s >= 0 && s + L <= a.Nn ? a.noise + s : nullptr;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_wave_stats(const WaveArgs a) {
    __shared__ double red[4][WP_SUMS];
    const int np = (a.Spad + WP_CHUNK - 1) / WP_CHUNK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long item = blockIdx.x; item < (long)a.B * np; item += gridDim.x) {
        const int b = (int)(item / np), p = (int)(item % np);
        const int L = wave_len(a, b), lo = p * WP_CHUNK;
        if (lo >= L) continue;                                    // (rows behind the clip's length are never read)
        const int hi = lo + WP_CHUNK < L ? lo + WP_CHUNK : L;
        const float* nz = wave_noise(a, b, L);
        double s[WP_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = lo + threadIdx.x; i < hi; i += 256) {
            const double x = (double)wave_load(a, (long)b * a.Spad + i), n = nz != nullptr ? (double)nz[i] : 0.0;
            s[0] += x; s[1] += n; s[2] += x * x; s[3] += n * n; s[4] += x * n;
        }
#pragma unroll
        for (int k = 0; k < WP_SUMS; ++k) s[k] = wave_sum_f64(s[k]);
        if (lane == 0)
#pragma unroll
            for (int k = 0; k < WP_SUMS; ++k) red[wave][k] = s[k];
        __syncthreads();
        if (threadIdx.x < WP_SUMS) a.part[item * WP_SUMS + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_wave_apply(const WaveArgs a, float eps) {
    __shared__ double tot[WP_SUMS];
    __shared__ double coef[3];                                    // scale, mean, 1 / sqrt(var + eps)
    const int np = (a.Spad + WP_CHUNK - 1) / WP_CHUNK;
    for (long item = blockIdx.x; item < (long)a.B * np; item += gridDim.x) {
        const int b = (int)(item / np), c = (int)(item % np);
        const int L = wave_len(a, b), lo = c * WP_CHUNK;
        const int hi = lo + WP_CHUNK < a.Spad ? lo + WP_CHUNK : a.Spad;
        float* out = a.out + (long)b * a.Spad;
        if (lo >= L) {                                            // padding only
            for (int i = lo + threadIdx.x; i < hi; i += 256) out[i] = 0.f;
            continue;
        }
        const float* nz = wave_noise(a, b, L);
        if (threadIdx.x < WP_SUMS) {
            const double* row = a.part + (long)b * np * WP_SUMS + threadIdx.x;
            double s = 0.0;
            for (int p = 0; p * WP_CHUNK < L; ++p) s += row[p * WP_SUMS];
            tot[threadIdx.x] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const double Sx = tot[0], Sn = tot[1], Sxx = tot[2], Snn = tot[3], Sxn = tot[4];
            const double scale = nz != nullptr && Sxx > 0.0 && Snn > 0.0 ? sqrt(Sxx / Snn) * pow(10.0, -(double)a.snr_db[b] / 20.0) : 0.0;
            const double mu = (Sx + scale * Sn) / (double)L;
            double var = (Sxx + 2.0 * scale * Sxn + scale * scale * Snn) / (double)L - mu * mu;
            var = var > 0.0 ? var : 0.0;
            coef[0] = scale; coef[1] = mu; coef[2] = 1.0 / sqrt(var + (double)eps);
        }
        __syncthreads();
        const double scale = coef[0], mu = coef[1], rstd = coef[2];
        for (int i = lo + threadIdx.x; i < hi; i += 256) {
            float v = 0.f;
            if (i < L) {
                const double x = (double)wave_load(a, (long)b * a.Spad + i), n = nz != nullptr ? (double)nz[i] : 0.0;
                v = (float)(((x + scale * n) - mu) * rstd);
            }
            out[i] = v;
        }
        __syncthreads();                                          // (tot / coef are rewritten by the next item)
    }
}

static inline int item_grid(long items, int max_blocks, int dflt) {
    long g = items < 1 ? 1 : items;
    const int cap = max_blocks > 0 ? max_blocks : dflt;
    return (int)(g > cap ? cap : g);
}

extern "C" {

/* packed uint8 frames [sum T_b][Hs][Ws] -> fp32 [B][Tpad][1][H][W]; see include/syncvsr_hip.h */
int svsr_lrs_clip_prep(const void* src_u8, int64_t total_frames, const int* off, const int* params, const void* tmask, float* dst, int B, int Tpad,
                       int Hs, int Ws, int H, int W, float mean, float std, int max_blocks, hipStream_t stream) {
    if (B < 1 || Tpad < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1 || total_frames < 0 || !(std > 0.f) || max_blocks < 0 || src_u8 == nullptr ||
        off == nullptr || params == nullptr || dst == nullptr)
        return SVSR_ERR_ARG;
    const long items = (long)B * Tpad * ((H + LP_ROWS - 1) / LP_ROWS);
    const int vec = W % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    hipLaunchKernelGGL(k_lrs_clip_prep, dim3(item_grid(items, max_blocks, 16384)), dim3(256), 0, stream, (const unsigned char*)src_u8, off, params,
                       (const unsigned char*)tmask, dst, B, Tpad, (long)total_frames, Hs, Ws, H, W, mean, 1.0f / std, -mean / std, vec);
    return svsr_check_launch();
}

int64_t svsr_wave_prep_ws_bytes(int B, int Spad) {
    if (B < 1 || Spad < 1) return 0;
    return (int64_t)B * ((Spad + WP_CHUNK - 1) / WP_CHUNK) * WP_SUMS * (int64_t)sizeof(double);
}

/* noise at a drawn SNR + layer norm over each clip's real samples, two launches; see include/syncvsr_hip.h */
int svsr_wave_prep(const void* wave, int wave_i16, const int* len, const float* noise, int64_t Nn, const int* nstart, const float* snr_db, float* out,
                   int B, int Spad, float eps, void* ws, int64_t ws_bytes, int max_blocks, hipStream_t stream) {
    if (B < 1 || Spad < 1 || Spad > (1 << 30) || wave == nullptr || len == nullptr || out == nullptr || ws == nullptr || ((uintptr_t)ws & 7) != 0 ||
        ws_bytes < svsr_wave_prep_ws_bytes(B, Spad) || max_blocks < 0 || !(eps >= 0.f) || (noise != nullptr && (nstart == nullptr || snr_db == nullptr || Nn < 0)))
        return SVSR_ERR_ARG;
    const WaveArgs a{wave, wave_i16, len, noise, (long)Nn, nstart, snr_db, out, B, Spad, (double*)ws};
    const int grid = item_grid((long)B * ((Spad + WP_CHUNK - 1) / WP_CHUNK), max_blocks, 16384);
    hipLaunchKernelGGL(k_wave_stats, dim3(grid), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_wave_apply, dim3(grid), dim3(256), 0, stream, a, eps);
    return svsr_check_launch();
}

}  // extern "C"
