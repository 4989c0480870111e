// The frozen wav2vec2 audio tokeniser of SyncVSR's `wav2vec2` codec (gfx950): raw waveform -> (i0, 320 + i1) per 20 ms frame.
//
// Replaces, for the reference's
//     feats = self.wav2vec.wav2vec2.feature_extractor(audios).transpose(1, 2)
//     _, feats = self.wav2vec.wav2vec2.feature_projection(feats)
//     indices = self.wav2vec.quantizer(feats)[0].unflatten(-1, (2, -1))[..., 0].long()
// (LRS/video/espnet/nets/pytorch_backend/e2e_asr_transformer.py:167-180, LRW/video/src/lightning.py:121-131; HF transformers
// Wav2Vec2FeatureEncoder / Wav2Vec2FeatureProjection / Wav2Vec2GumbelVectorQuantizer) the launch chain
//     k_w2v_conv0                    layer 0 (C_in = 1, k = 10, s = 5) in fp32 FMAs, + bias + LayerNorm + GELU ("layer" models) or the
//                                    pre-norm output + per-(clip, channel) partial sums of its GroupNorm ("group" models)
//     svsr_w2v_norm_gelu             the row pass behind layers 1-6 ("layer": LayerNorm(512) + GELU) or the finalise-and-apply of layer 0's
//                                    GroupNorm ("group")
//     svsr_igemm_fwd (x6)            layers 1-6 as dense contractions over channels-last rows (python side: syncvsr_amd/audio_codec.py)
//     k_w2v_quantize                 LayerNorm(512) of feature_projection + weight_proj (MFMA) + per-group argmax (eval) or argmax of
//                                    logits + Gumbel noise (training), int64 tokens out; no logits tensor in memory
// Activations are channels-last bf16 rows [B][rows per clip][512].  Every reduction is a fixed-order sum (no floating-point atomics).
#include "common.h"
#include "../../include/syncvsr_hip.h"

#define W2V_C 512
#define W2V_FB 64                 // frames per workgroup of k_w2v_conv0: four waves x 16 frames
#define W2V_V 320                 // codevectors per group
#define W2V_G 2                   // groups
#define W2V_QB 32                 // rows per workgroup of k_w2v_quantize
#define W2V_QP (W2V_C + 8)        // LDS row pitch (elements) of the normalised features: 1,040 bytes, rows fall on different banks

struct W2vConv0Args {
    const float* wave;     // [B][L_in] fp32; samples L_in .. L_in + pad - 1 of every row are zeros
    int L_in, F0, out_rows, nblk, mode;
    const float* w;        // [512][10]
    const float* bias;     // [512] or null
    const float* gamma;    // layer mode: LayerNorm affine
    const float* beta;
    float eps;
    bf16_t* out;           // [B][out_rows][512]
    float* part;           // group mode: [B][nblk][2][512] sums / sums of squares of this block's frames
};

// one lane = 8 channels of a frame, one wave = 16 frames, one workgroup = 64 frames of one clip
__global__ __launch_bounds__(256) void k_w2v_conv0(const W2vConv0Args p) {
    __shared__ float sx[W2V_FB * 5 + 8];
    __shared__ float sred[4][2][W2V_C];
    const int b = blockIdx.y, blk = blockIdx.x, f0 = blk * W2V_FB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* xrow = p.wave + (long)b * p.L_in;
    const long s0 = (long)f0 * 5;
    for (int i = tid; i < W2V_FB * 5 + 5; i += 256) {
        const long s = s0 + i;
        sx[i] = s < p.L_in ? xrow[s] : 0.f;
    }
    const int c0 = lane * 8;
    float w[8][10], bs[8], g[8], be[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int k = 0; k < 10; ++k) w[c][k] = p.w[(c0 + c) * 10 + k];
        bs[c] = p.bias != nullptr ? p.bias[c0 + c] : 0.f;
        g[c] = p.mode == 0 ? p.gamma[c0 + c] : 1.f;
        be[c] = p.mode == 0 ? p.beta[c0 + c] : 0.f;
    }
    __syncthreads();
    float gs[8], gq[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { gs[c] = 0.f; gq[c] = 0.f; }
    for (int i = 0; i < 16; ++i) {
        const int fl = wave * 16 + i, f = f0 + fl;
        if (f >= p.F0) break;                                      // (wave-uniform)
        float xs[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) xs[k] = sx[fl * 5 + k];
        float a[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float s = bs[c];
#pragma unroll
            for (int k = 0; k < 10; ++k) s = __builtin_fmaf(w[c][k], xs[k], s);
            a[c] = s;
        }
        if (p.mode == 0) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) s += a[c];
            const float mean = wave_sum(s) * (1.0f / W2V_C);
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) { const float d = a[c] - mean; q = __builtin_fmaf(d, d, q); }
            const float rstd = rsqrtf(wave_sum(q) * (1.0f / W2V_C) + p.eps);
#pragma unroll
            for (int c = 0; c < 8; ++c) a[c] = gelu_erf(__builtin_fmaf((a[c] - mean) * rstd, g[c], be[c]));
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) { gs[c] += a[c]; gq[c] = __builtin_fmaf(a[c], a[c], gq[c]); }
        }
        *reinterpret_cast<u32x4*>(p.out + ((long)b * p.out_rows + f) * W2V_C + c0) = pack8(a);
    }
    if (p.mode == 1) {
#pragma unroll
        for (int c = 0; c < 8; ++c) { sred[wave][0][c0 + c] = gs[c]; sred[wave][1][c0 + c] = gq[c]; }
        __syncthreads();
        float* dst = p.part + ((long)b * p.nblk + blk) * 2 * W2V_C;
        for (int c = tid; c < W2V_C; c += 256) {
            dst[c] = ((sred[0][0][c] + sred[1][0][c]) + sred[2][0][c]) + sred[3][0][c];
            dst[W2V_C + c] = ((sred[0][1][c] + sred[1][1][c]) + sred[2][1][c]) + sred[3][1][c];
        }
    }
}

// GroupNorm(512 groups) statistics of layer 0: per (clip, channel) the partial rows of k_w2v_conv0 added in block order, in double.
// ms [B][2][512] = {mean, rstd} (biased variance over the clip's F0 frames, as nn.GroupNorm)
__global__ __launch_bounds__(256) void k_w2v_gn_stats(const float* part, int nblk, int F0, float eps, float* ms) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= W2V_C) return;
    double s = 0.0, q = 0.0;
    const float* src = part + (long)b * nblk * 2 * W2V_C + c;
    for (int k = 0; k < nblk; ++k) { s += (double)src[(long)k * 2 * W2V_C]; q += (double)src[(long)k * 2 * W2V_C + W2V_C]; }
    const double mean = s / F0;
    double var = q / F0 - mean * mean;
    if (var < 0.0) var = 0.0;
    ms[(long)b * 2 * W2V_C + c] = (float)mean;
    ms[(long)b * 2 * W2V_C + W2V_C + c] = (float)(1.0 / sqrt(var + (double)eps));
}

// y = GELU(norm(x) * gamma + beta) in place over the valid rows (clip b, frame f < F) of [B][rows][512]; one wave per row.
// ms == null: LayerNorm over the row's 512 channels; else the GroupNorm statistics of k_w2v_gn_stats
__global__ __launch_bounds__(256) void k_w2v_norm_gelu(bf16_t* x, int B, int F, int rows, const float* gamma, const float* beta, float eps,
                                                      const float* ms) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long)B * F) return;
    const int b = (int)(r / F), f = (int)(r - (long)b * F);
    bf16_t* row = x + ((long)b * rows + f) * W2V_C;
    const int c0 = lane * 8;
    float a[8];
    unpack8(*reinterpret_cast<const u32x4*>(row + c0), a);
    float mean[8], rstd[8];
    if (ms == nullptr) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) s += a[c];
        const float m = wave_sum(s) * (1.0f / W2V_C);
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) { const float d = a[c] - m; q = __builtin_fmaf(d, d, q); }
        const float rs = rsqrtf(wave_sum(q) * (1.0f / W2V_C) + eps);
#pragma unroll
        for (int c = 0; c < 8; ++c) { mean[c] = m; rstd[c] = rs; }
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) { mean[c] = ms[(long)b * 2 * W2V_C + c0 + c]; rstd[c] = ms[(long)b * 2 * W2V_C + W2V_C + c0 + c]; }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) a[c] = gelu_erf(__builtin_fmaf((a[c] - mean[c]) * rstd[c], gamma[c0 + c], beta[c0 + c]));
    *reinterpret_cast<u32x4*>(row + c0) = pack8(a);
}

struct W2vQuantArgs {
    const bf16_t* feat;    // [R][512] rows of the last convolution (R = clips x F frames)
    int R, F, keep;        // tokens of frames t < keep of every clip are written
    const float* gamma;    // feature_projection.layer_norm
    const float* beta;
    float eps;
    const bf16_t* w;       // weight_proj [640][512] bf16
    const float* bias;     // [640]
    const unsigned* seed;  // null: argmax; else argmax(logits + Gumbel noise of hash(*seed, site, row * 640 + column))
    unsigned site;
    long* tok;             // [R / F][keep][2]: (i0, 320 + i1)
    float* logits;         // optional [R][640] fp32 (tests)
};

// Workgroup = 32 rows, two waves.  The rows' LayerNorm (one wave per row, fp32) goes to LDS as bf16; then wave g contracts them with the
// 320 weight rows of group g on MFMA 32x32x16 — weight rows as the A operand, feature rows as B — so the accumulator gives a lane one ROW
// (lane & 31) and, per 32-column tile, 16 of its columns (the same transposed form as k_linear_ce in audio_head.hip): the argmax is a
// register loop plus one exchange with lane ^ 32.  The weight fragments come straight from global memory (640 x 512 bf16 = 640 KiB: L2).
__global__ __launch_bounds__(128) void k_w2v_quantize(const W2vQuantArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t sF[W2V_QB * W2V_QP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * W2V_QB;
    {
        const int c0 = lane * 8;
        float g[8], be[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { g[c] = p.gamma[c0 + c]; be[c] = p.beta[c0 + c]; }
        for (int i = 0; i < W2V_QB / 2; ++i) {
            const int rl = wave * (W2V_QB / 2) + i, r = m0 + rl;
            float a[8];
            if (r < p.R) {
                unpack8(*reinterpret_cast<const u32x4*>(p.feat + (long)r * W2V_C + c0), a);
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < 8; ++c) s += a[c];
                const float m = wave_sum(s) * (1.0f / W2V_C);
                float q = 0.f;
#pragma unroll
                for (int c = 0; c < 8; ++c) { const float d = a[c] - m; q = __builtin_fmaf(d, d, q); }
                const float rs = rsqrtf(wave_sum(q) * (1.0f / W2V_C) + p.eps);
#pragma unroll
                for (int c = 0; c < 8; ++c) a[c] = __builtin_fmaf((a[c] - m) * rs, g[c], be[c]);
            } else {
#pragma unroll
                for (int c = 0; c < 8; ++c) a[c] = 0.f;
            }
            *reinterpret_cast<u32x4*>(sF + rl * W2V_QP + c0) = pack8(a);
        }
    }
    __syncthreads();
    const int grp = wave, half = lane >> 5;
    const int row = m0 + (lane & 31);
    const bool row_ok = row < p.R;
    unsigned key = 0;
    if (p.seed != nullptr) key = svsr_mix(p.seed[0] * 0x9E3779B9u + p.site * 0x7F4A7C15u + 0x165667B1u);
    float best = -INFINITY;
    int best_i = 0;                    // (a group of -inf logits gives index 0, as torch.argmax)
    const bf16_t* fsrc = sF + (lane & 31) * W2V_QP + half * 8;
    for (int h = 0; h < 2; ++h) {
        const int colh = grp * W2V_V + h * 160;                        // first weight row (logit column) of this half
        const bf16_t* wsrc = p.w + (long)(colh + (lane & 31)) * W2V_C + half * 8;
        f32x16 acc[5];
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll 4
        for (int ks = 0; ks < W2V_C / 16; ++ks) {
            const bf16x8 fh = *reinterpret_cast<const bf16x8*>(fsrc + ks * 16);
            bf16x8 fw[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) fw[j] = *reinterpret_cast<const bf16x8*>(wsrc + (long)j * 32 * W2V_C + ks * 16);
#pragma unroll
            for (int j = 0; j < 5; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[j], fh, acc[j], 0, 0, 0);
        }
        // lane: row `row`, columns colh + j*32 + 8q + 4*half + e (register 4q + e of tile j), visited in ascending order
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int col = colh + j * 32 + 8 * q + 4 * half + e;
                    const float z = acc[j][4 * q + e] + p.bias[col];
                    if (p.logits != nullptr && row_ok) p.logits[(long)row * (W2V_G * W2V_V) + col] = z;
                    float v = z;
                    if (p.seed != nullptr) {
                        const unsigned hsh = svsr_mix((unsigned)((long)row * (W2V_G * W2V_V) + col) * 2654435761u + key);
                        const double u = ((double)hsh + 0.5) * 2.3283064365386962890625e-10;      // (h + 0.5) 2^-32, in (0, 1)
                        v = z + (float)(-log(-log(u)));
                    }
                    // NaN counts as the maximum (torch.argmax returns the first NaN): the token stays inside the vocabulary
                    if (__builtin_isnan(v) ? !__builtin_isnan(best) : v > best) { best = v; best_i = col - grp * W2V_V; }
                }
    }
    // lanes l and l ^ 32 hold the same row: a NaN, else the larger value wins; a tie goes to the lower index (torch.argmax)
    const auto xb = __builtin_amdgcn_permlane32_swap(__float_as_int(best), __float_as_int(best), false, false);
    const auto xi = __builtin_amdgcn_permlane32_swap(best_i, best_i, false, false);
    const float b0 = __int_as_float(xb[0]), b1 = __int_as_float(xb[1]);
    const int i0 = xi[0], i1 = xi[1];
    const bool n0 = __builtin_isnan(b0), n1 = __builtin_isnan(b1);
    const bool take1 = n1 ? (!n0 || i1 < i0) : (!n0 && (b1 > b0 || (b1 == b0 && i1 < i0)));
    const int win = take1 ? i1 : i0;
    const int clip = row / p.F, t = row - clip * p.F;
    if (row_ok && half == 0 && t < p.keep) p.tok[((long)clip * p.keep + t) * W2V_G + grp] = (long)(win + grp * W2V_V);
}

extern "C" int64_t svsr_w2v_stats_floats(int B, int F0) {
    if (B < 1 || F0 < 1) return -SVSR_ERR_ARG;
    const long nblk = (F0 + W2V_FB - 1) / W2V_FB;
    return (int64_t)B * nblk * 2 * W2V_C + (int64_t)B * 2 * W2V_C;
}

extern "C" int svsr_w2v_conv0(const float* wave, int B, int L_in, int pad, const float* w, const float* bias, const float* gamma,
                              const float* beta, float eps, void* out, int out_rows, float* stats, int mode, hipStream_t stream) {
    if (wave == nullptr || w == nullptr || out == nullptr || B < 1 || L_in < 1 || pad < 0 || (mode != 0 && mode != 1)) return SVSR_ERR_ARG;
    const long L = (long)L_in + pad;
    if (L < 10 || L >= (1L << 30)) return SVSR_ERR_ARG;
    const int F0 = (int)((L - 10) / 5 + 1);
    if (out_rows < F0) return SVSR_ERR_ARG;
    if (mode == 0 && (gamma == nullptr || beta == nullptr)) return SVSR_ERR_ARG;
    if (mode == 1 && stats == nullptr) return SVSR_ERR_ARG;
    W2vConv0Args a;
    a.wave = wave; a.L_in = L_in; a.F0 = F0; a.out_rows = out_rows; a.nblk = (F0 + W2V_FB - 1) / W2V_FB; a.mode = mode;
    a.w = w; a.bias = bias; a.gamma = gamma; a.beta = beta; a.eps = eps; a.out = (bf16_t*)out; a.part = stats;
    hipLaunchKernelGGL(k_w2v_conv0, dim3(a.nblk, B), dim3(256), 0, stream, a);
    return svsr_check_launch();
}

extern "C" int svsr_w2v_norm_gelu(void* x, int B, int F, int rows, const float* gamma, const float* beta, float eps, float* stats, int F0,
                                  int mode, hipStream_t stream) {
    if (x == nullptr || gamma == nullptr || beta == nullptr || B < 1 || F < 1 || rows < F || (mode != 0 && mode != 1)) return SVSR_ERR_ARG;
    const float* ms = nullptr;
    if (mode == 1) {      // GroupNorm of layer 0: stats = the partial rows k_w2v_conv0 wrote for F0 = F frames; {mean, rstd} go behind them
        if (stats == nullptr || F0 != F) return SVSR_ERR_ARG;
        const int nblk = (F0 + W2V_FB - 1) / W2V_FB;
        float* msw = stats + (long)B * nblk * 2 * W2V_C;
        hipLaunchKernelGGL(k_w2v_gn_stats, dim3(W2V_C / 256, B), dim3(256), 0, stream, stats, nblk, F0, eps, msw);
        const int rc = svsr_check_launch();
        if (rc != SVSR_OK) return rc;
        ms = msw;
    }
    const long nrows = (long)B * F;
    hipLaunchKernelGGL(k_w2v_norm_gelu, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, stream, (bf16_t*)x, B, F, rows, gamma, beta, eps, ms);
    return svsr_check_launch();
}

extern "C" int svsr_w2v_quantize(const void* feat, int R, int F, int keep, const float* gamma, const float* beta, float eps, const void* w, const float* bias,
                                 const unsigned* seed, unsigned site, int64_t* tok, float* logits_out, hipStream_t stream) {
    if (feat == nullptr || gamma == nullptr || beta == nullptr || w == nullptr || bias == nullptr || tok == nullptr || R < 1) return SVSR_ERR_ARG;
    if (F < 1 || R % F != 0 || keep < 1 || keep > F) return SVSR_ERR_ARG;
    if ((long)R * W2V_G * W2V_V >= (1L << 32)) return SVSR_ERR_ARG;         // the noise counter is 32 bits
    W2vQuantArgs a;
    a.feat = (const bf16_t*)feat; a.R = R; a.F = F; a.keep = keep; a.gamma = gamma; a.beta = beta; a.eps = eps; a.w = (const bf16_t*)w; a.bias = bias;
    a.seed = seed; a.site = site; a.tok = (long*)tok; a.logits = logits_out;
    hipLaunchKernelGGL(k_w2v_quantize, dim3((R + W2V_QB - 1) / W2V_QB), dim3(128), 0, stream, a);
    return svsr_check_launch();
}
