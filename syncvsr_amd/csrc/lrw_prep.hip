// Device-side training inputs of the word-level (LRW) path, gfx950, wave64: the reference's per-clip chain
//   x / 255 -> RandomHorizontalFlip -> RandomResizedCrop | Identity -> Grayscale -> TimeMask -> Normalize     (LRW/video/src/data.py:157-164)
// and the frame splice of its sequential CutMix (LRW/video/src/augment.py:27-118) in two launches per batch, no second pass over the
// fp32 clips.  The random decisions are made on the host (syncvsr_amd/augment.py DeviceLRWPipeline.plan).
//   * k_lrw_clip_sums: per-frame sums [B][T] of the sampled clip in front of Normalize, x_s[t] — what TimeMask's clip mean is made of
//   * k_lrw_clip_mix:  out[b][0][t] = Normalize(TimeMask(x_s))[t] with s = frame_src[b][t]; every output element is written once
// The sampling is csrc/clip_sample.h, so a frame that is neither masked nor spliced has k_clip_prep's bits.
// No float atomics and no order that depends on arrival: every output is a pure function of the inputs, whatever the grid.
#include "common.h"
#include "clip_sample.h"

#define LW_MAXT 256          // frames per clip: one thread per frame sum in k_lrw_clip_mix
#define LW_ROWS 32           // output rows per item of k_lrw_clip_mix

// ---------------------------------------------------------------------------------------------------------------------
// Frame sums.  One item = (clip s, frame t), walked in a grid-stride loop by whole workgroups, so the partition of a frame's H * W pixels
// depends on H * W alone: thread i adds pixels i, i + 256, ... in index order, the 64 lanes of a wave in a butterfly, the 4 waves in wave
// order.  fsum[s][t] = sum over the frame of clip_sample / 255.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lrw_clip_sums(const unsigned char* __restrict__ src, const int* __restrict__ params,
                                                       float* __restrict__ fsum, int B, int T, int Hs, int Ws, int H, int W) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, HW = H * W;
    for (long item = blockIdx.x; item < (long)B * T; item += gridDim.x) {
        const int s = (int)(item / T);
        const ClipWindow w = clip_window(params, s, Hs, Ws);
        const unsigned char* f = src + item * Hs * Ws;
        float acc = 0.f;
        for (int q = threadIdx.x; q < HW; q += 256) {
            const int y = q / W;
            acc += clip_sample(f, w, Ws, y, q - y * W, H, W) * (1.0f / 255.0f);
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) red[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) fsum[item] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();                                          // (red is rewritten by the next item)
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Mix.  One item = (sample b, frame t, block of LW_ROWS output rows).  s = frame_src[b][t] (clamped into [0, B)) is the ORIGINAL clip the
// frame comes from after the reference's in-place chain; crop, flip and time mask are that clip's.  Frame t of clip s is masked when a run
// (start, len) of clip s with len > 0 covers it (runs clamped into [0, T]).  The fill of a run is the mean of the clip AS MASKED SO FAR
// (a later run sees the earlier fills), derived by one thread from the clip's T frame sums in run order:
//     S = sum_t fs[t];   per run: m = S / (T H W), for t in the run: S += H W m - cur[t], cur[t] = H W m
// A masked frame is the constant (fill - mean) / std (fill = 0 with replace_with_zero: no sums needed); any other frame is sampled.
// Only the items of masked frames walk the recurrence — those that have nothing to sample.
// A thread produces four neighbouring pixels of a row and stores them as one 16-byte vector where the rows are 16-byte aligned (W % 4 == 0
// and dst aligned); otherwise pixel by pixel.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lrw_clip_mix(const unsigned char* __restrict__ src, const int* __restrict__ params,
                                                      const int* __restrict__ frame_src, const int* __restrict__ runs,
                                                      const float* __restrict__ fsum, float* __restrict__ dst, int B, int T, int Hs, int Ws,
                                                      int H, int W, int n_mask, int zero_fill, float mean, float inv_std, int vec) {
    __shared__ float cur[LW_MAXT];
    __shared__ float fill_sh;
    const int nrb = (H + LW_ROWS - 1) / LW_ROWS, W4 = (W + 3) >> 2;
    const long items = (long)B * T * nrb;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const int rb = (int)(item % nrb);
        const long bt = item / nrb;
        const int t = (int)(bt % T);
        const int y_lo = rb * LW_ROWS, rows = H - y_lo < LW_ROWS ? H - y_lo : LW_ROWS;
        float* out = dst + (bt * H + y_lo) * W;
        int s = frame_src[bt];
        s = s < 0 ? 0 : (s > B - 1 ? B - 1 : s);
        const int* rs = runs + (long)s * n_mask * 2;
        bool masked = false;                                      // (the same in every thread of the workgroup)
        for (int j = 0; j < n_mask; ++j) {
            int st = rs[2 * j], ln = rs[2 * j + 1];
            st = st < 0 ? 0 : (st > T ? T : st);
            ln = ln < 0 ? 0 : (ln > T - st ? T - st : ln);
            masked = masked || (t >= st && t < st + ln);
        }
        if (masked) {
            float fill = 0.f;
            if (!zero_fill) {
                if (threadIdx.x < T) cur[threadIdx.x] = fsum[(long)s * T + threadIdx.x];
                __syncthreads();
                if (threadIdx.x == 0) {
                    const float hw = (float)(H * W), n = (float)T * hw;
                    float S = 0.f, m_t = 0.f;
                    for (int i = 0; i < T; ++i) S += cur[i];
                    for (int j = 0; j < n_mask; ++j) {
                        int st = rs[2 * j], ln = rs[2 * j + 1];
                        st = st < 0 ? 0 : (st > T ? T : st);
                        ln = ln < 0 ? 0 : (ln > T - st ? T - st : ln);
                        const float m = S / n, filled = hw * m;
                        for (int i = st; i < st + ln; ++i) {
                            S += filled - cur[i];
                            cur[i] = filled;
                        }
                        if (t >= st && t < st + ln) m_t = m;          // the last run that covers t decides
                    }
                    fill_sh = m_t;
                }
                __syncthreads();
                fill = fill_sh;
                __syncthreads();                                  // (cur / fill_sh are rewritten by the next masked item)
            }
            const float v = (fill - mean) * inv_std;
            if (vec) {
                const f32x4 v4 = {v, v, v, v};
                for (int q = threadIdx.x; q < rows * W4; q += 256) reinterpret_cast<f32x4*>(out)[q] = v4;
            } else {
                for (int q = threadIdx.x; q < rows * W; q += 256) out[q] = v;
            }
            continue;
        }
        const ClipWindow w = clip_window(params, s, Hs, Ws);
        const unsigned char* f = src + ((long)s * T + t) * Hs * Ws;
        for (int q = threadIdx.x; q < rows * W4; q += 256) {
            const int yr = q / W4, x4 = (q - yr * W4) * 4;
            float px[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x4 + j < W ? x4 + j : W - 1;          // (a ragged last quad samples its last column again; only x < W is stored)
                px[j] = clip_normalize(clip_sample(f, w, Ws, y_lo + yr, x, H, W), mean, inv_std);
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

static inline int lrw_grid(long items, int max_blocks) {
    const long g = items < 1 ? 1 : items;
    const int cap = max_blocks > 0 ? max_blocks : 16384;
    return (int)(g > cap ? cap : g);
}

static inline bool lrw_shape_ok(int B, int T, int Hs, int Ws, int H, int W) {
    return B >= 1 && T >= 1 && T <= LW_MAXT && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1 && (long)Hs * Ws <= (1 << 24) && (long)H * W <= (1 << 24) &&
           (long)B * T <= (1 << 24);
}

extern "C" {

/* per-frame sums of the sampled clips in front of Normalize; see include/syncvsr_hip.h */
int svsr_lrw_clip_sums(const void* src_u8, const int* params, float* frame_sums, int B, int T, int Hs, int Ws, int H, int W, int max_blocks,
                       hipStream_t stream) {
    if (!lrw_shape_ok(B, T, Hs, Ws, H, W) || max_blocks < 0 || src_u8 == nullptr || params == nullptr || frame_sums == nullptr) return SVSR_ERR_ARG;
    hipLaunchKernelGGL(k_lrw_clip_sums, dim3(lrw_grid((long)B * T, max_blocks)), dim3(256), 0, stream, (const unsigned char*)src_u8, params, frame_sums,
                       B, T, Hs, Ws, H, W);
    return svsr_check_launch();
}

/* uint8 clips -> fp32 [B][1][T][H][W]: crop / flip / time mask of the source clip, Normalize, CutMix frame splice; see include/syncvsr_hip.h */
int svsr_lrw_clip_mix(const void* src_u8, const int* params, const int* frame_src, const int* runs, const float* frame_sums, float* dst, int B, int T,
                      int Hs, int Ws, int H, int W, int n_mask, int replace_with_zero, float mean, float std, int max_blocks, hipStream_t stream) {
    if (!lrw_shape_ok(B, T, Hs, Ws, H, W) || !(std > 0.f) || max_blocks < 0 || n_mask < 0 || n_mask > (1 << 16) || src_u8 == nullptr ||
        params == nullptr || frame_src == nullptr || dst == nullptr || (n_mask > 0 && runs == nullptr) ||
        (n_mask > 0 && !replace_with_zero && frame_sums == nullptr))
        return SVSR_ERR_ARG;
    const long items = (long)B * T * ((H + LW_ROWS - 1) / LW_ROWS);
    const int vec = W % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    hipLaunchKernelGGL(k_lrw_clip_mix, dim3(lrw_grid(items, max_blocks)), dim3(256), 0, stream, (const unsigned char*)src_u8, params, frame_src, runs,
                       frame_sums, dst, B, T, Hs, Ws, H, W, n_mask, replace_with_zero != 0, mean, 1.0f / std, vec);
    return svsr_check_launch();
}

}  // extern "C"
