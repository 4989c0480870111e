// The frozen vq-wav2vec k-means audio tokeniser of SyncVSR's `vq` codec (gfx950): raw waveform -> (i0, i1) per 10 ms frame, both in 0..319.
//
// Replaces, for the reference's
//     audio_tokens = self.wav2vec.feature_extractor(audios)
//     audio_tokens = self.wav2vec.vector_quantizer.forward_idx(audio_tokens)[1]
// (LRW/video/src/lightning.py:121-131; fairseq Wav2VecModel / ConvFeatureExtractionModel / KmeansVectorQuantizer) the launch chain
//     k_vq_conv0<false>              layer 0 (C_in = 1, k = 10, s = 5) in fp32 FMAs: only the partial sums of its clip-wide GroupNorm(1, 512)
//     k_vq_conv0<true>               layer 0 again, + GroupNorm + affine + ReLU, bf16 rows out: the layer's output crosses memory once
//     svsr_igemm_fwd (x7)            layers 1-7 as dense contractions over channels-last rows (python side: syncvsr_amd/audio_codec.py)
//     k_vq_gn_partial, k_vq_gn_relu  behind each of them: partial sums over the valid rows; GroupNorm(1, 512) + affine + ReLU in place
//                                    (+ log(x + 1) behind layer 7)
//     k_vq_project                   the quantiser's grouped 256 -> 256 projection (MFMA), fp32 out, + partial sums of its GroupNorm(2, 512)
//     k_vq_assign                    GroupNorm(2, 512) + affine, scores |e|^2 - 2 z.e against the 320 centroids of each group (MFMA), argmin
// Activations are channels-last bf16 rows [B][rows per clip][512].  Every GroupNorm here takes its statistics over ALL frames of a clip, so a
// producer writes per-(clip, block) partial {sum, sum of squares} with plain stores and the consumer adds them in block order in double
// (vq_finalize): no floating-point atomics, the same bits every run.
#include "common.h"
#include "../../include/syncvsr_hip.h"

#define VQ_C 512
#define VQ_FB 64                  // frames / rows per partial-sum block of k_vq_conv0 and k_vq_gn_partial: four waves x 16
#define VQ_V 320                  // centroids per group
#define VQ_G 2                    // groups
#define VQ_D 256                  // channels per group
#define VQ_QB 32                  // rows per workgroup of k_vq_project and k_vq_assign (= rows per partial-sum block of the projection)
#define VQ_QP (VQ_D + 8)          // LDS row pitch (elements) of the normalised projections: 528 bytes, rows fall on different banks

// {mean, 1 / sqrt(biased variance + eps)} of `count` values from nblk partial {sum, sum of squares} pairs, added in double by one whole
// wave (all 64 lanes must be active): lane l adds blocks l, l + 64, ... in order, then a butterfly over the lanes — a fixed association,
// and the same bits in every lane (each step adds the same two values in both partners).  3,890 frames are 61 blocks: one add and six
// exchanges instead of a chain of 61.
// A NaN partial gives NaN statistics (the comparison below is false for it): the clip's tokens then are (0, 0), see k_vq_assign.
__device__ __forceinline__ void vq_finalize(const float* part, int nblk, double count, float eps, float& mean, float& rstd) {
    double s = 0.0, q = 0.0;
    for (int k = threadIdx.x & 63; k < nblk; k += 64) { s += (double)part[2 * k]; q += (double)part[2 * k + 1]; }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { s += __shfl_xor(s, off, 64); q += __shfl_xor(q, off, 64); }
    const double m = s / count;
    double var = q / count - m * m;
    if (var < 0.0) var = 0.0;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// ReLU that keeps a NaN (fmaxf would drop it): a NaN waveform must reach k_vq_assign as NaN scores
__device__ __forceinline__ float vq_relu(float v) { return v < 0.f ? 0.f : v; }

// the four waves' {sum, sum of squares} -> part[0..1], waves added in order
__device__ __forceinline__ void vq_block_partial(float s, float q, float (*sred)[2], float* dst) {
    const int tid = threadIdx.x;
    s = wave_sum(s);
    q = wave_sum(q);
    if ((tid & 63) == 0) { sred[tid >> 6][0] = s; sred[tid >> 6][1] = q; }
    __syncthreads();
    if (tid == 0) {
        dst[0] = ((sred[0][0] + sred[1][0]) + sred[2][0]) + sred[3][0];
        dst[1] = ((sred[0][1] + sred[1][1]) + sred[2][1]) + sred[3][1];
    }
}

struct VqConv0Args {
    const float* wave;     // [B][L_in] fp32; samples L_in .. L_in + pad - 1 of every row are zeros
    int L_in, F0, out_rows, nblk;
    const float* w;        // [512][10]
    const float* gamma;    // apply: GroupNorm affine [512]
    const float* beta;
    float eps;
    bf16_t* out;           // apply: [B][out_rows][512]
    float* part;           // [B][nblk][2]: written by the statistics pass, read by the apply pass
};

// one lane = 8 channels of a frame, one wave = 16 frames, one workgroup = 64 frames of one clip.  APPLY = false: the partial sums of the
// block's F x 512 pre-norm values.  APPLY = true: the same convolution again, normalised with the clip's statistics.
template <bool APPLY>
__global__ __launch_bounds__(256) void k_vq_conv0(const VqConv0Args p) {
    __shared__ float sx[VQ_FB * 5 + 8];
    __shared__ float sred[4][2];
    const int b = blockIdx.y, blk = blockIdx.x, f0 = blk * VQ_FB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* xrow = p.wave + (long)b * p.L_in;
    const long s0 = (long)f0 * 5;
    for (int i = tid; i < VQ_FB * 5 + 5; i += 256) {
        const long s = s0 + i;
        sx[i] = s < p.L_in ? xrow[s] : 0.f;
    }
    const int c0 = lane * 8;
    float w[8][10], g[8], be[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int k = 0; k < 10; ++k) w[c][k] = p.w[(c0 + c) * 10 + k];
        g[c] = APPLY ? p.gamma[c0 + c] : 1.f;
        be[c] = APPLY ? p.beta[c0 + c] : 0.f;
    }
    float mean = 0.f, rstd = 1.f;
    if (APPLY) vq_finalize(p.part + (long)b * p.nblk * 2, p.nblk, (double)p.F0 * VQ_C, p.eps, mean, rstd);
    __syncthreads();
    float ts = 0.f, tq = 0.f;
    for (int i = 0; i < 16; ++i) {
        const int fl = wave * 16 + i, f = f0 + fl;
        if (f >= p.F0) break;                                      // (wave-uniform)
        float xs[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) xs[k] = sx[fl * 5 + k];
        float a[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) s = __builtin_fmaf(w[c][k], xs[k], s);
            a[c] = s;
        }
        if (APPLY) {
#pragma unroll
            for (int c = 0; c < 8; ++c) a[c] = vq_relu(__builtin_fmaf((a[c] - mean) * rstd, g[c], be[c]));
            *reinterpret_cast<u32x4*>(p.out + ((long)b * p.out_rows + f) * VQ_C + c0) = pack8(a);
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) { ts += a[c]; tq = __builtin_fmaf(a[c], a[c], tq); }
        }
    }
    if (!APPLY) vq_block_partial(ts, tq, sred, p.part + ((long)b * p.nblk + blk) * 2);
}

// partial {sum, sum of squares} of rows f0 .. f0 + 63 (f < F) of clip b of x [B][rows][512] -> part [B][nblk][2]
__global__ __launch_bounds__(256) void k_vq_gn_partial(const bf16_t* x, int F, int rows, int nblk, float* part) {
    __shared__ float sred[4][2];
    const int b = blockIdx.y, blk = blockIdx.x, f0 = blk * VQ_FB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = lane * 8;
    float ts = 0.f, tq = 0.f;
    for (int i = 0; i < 16; ++i) {
        const int f = f0 + wave * 16 + i;
        if (f >= F) break;                                         // (wave-uniform)
        float a[8];
        unpack8(*reinterpret_cast<const u32x4*>(x + ((long)b * rows + f) * VQ_C + c0), a);
#pragma unroll
        for (int c = 0; c < 8; ++c) { ts += a[c]; tq = __builtin_fmaf(a[c], a[c], tq); }
    }
    vq_block_partial(ts, tq, sred, part + ((long)b * nblk + blk) * 2);
}

// y = relu(GroupNorm(1, 512)(x) * gamma + beta) in place over the valid rows (clip b, frame f < F) of [B][rows][512], one wave per row;
// mode 1 (behind the last layer): y = log(y + 1).  Padding rows f >= F are not touched.
__global__ __launch_bounds__(256) void k_vq_gn_relu(bf16_t* x, int B, int F, int rows, int nblk, const float* gamma, const float* beta, float eps,
                                                    const float* part, int mode) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long)B * F) return;
    const int b = (int)(r / F), f = (int)(r - (long)b * F);
    float mean, rstd;
    vq_finalize(part + (long)b * nblk * 2, nblk, (double)F * VQ_C, eps, mean, rstd);
    bf16_t* row = x + ((long)b * rows + f) * VQ_C;
    const int c0 = lane * 8;
    float a[8];
    unpack8(*reinterpret_cast<const u32x4*>(row + c0), a);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        a[c] = vq_relu(__builtin_fmaf((a[c] - mean) * rstd, gamma[c0 + c], beta[c0 + c]));
        if (mode == 1) a[c] = logf(a[c] + 1.0f);
    }
    *reinterpret_cast<u32x4*>(row + c0) = pack8(a);
}

// Workgroup = 32 rows of one clip, two waves; wave g computes the 256 outputs of group g on MFMA 32x32x16 with the weight rows as the A
// operand and the feature rows as B (fragments straight from global memory: the weights are 256 KiB, L2), so a lane owns one ROW (lane & 31)
// and, per 32-channel tile, 16 of its channels.  ze fp32 [B * F][512]; part [B][2][nblk][2] = the block's {sum, sum of squares} per group.
__global__ __launch_bounds__(128) void k_vq_project(const bf16_t* x, int F, int nblk, const bf16_t* w, float* ze, float* part) {
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, blk = blockIdx.x, half = lane >> 5;
    const int f = blk * VQ_QB + (lane & 31);
    const bool ok = f < F;
    const long row = (long)b * F + f;
    const bf16_t* src = x + row * VQ_C + g * VQ_D + half * 8;
    const bf16_t* wsrc = w + (long)(g * VQ_D + (lane & 31)) * VQ_D + half * 8;
    f32x16 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 2
    for (int ks = 0; ks < VQ_D / 16; ++ks) {
        const bf16x8 fh = ok ? *reinterpret_cast<const bf16x8*>(src + ks * 16) : zero;
        bf16x8 fw[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) fw[j] = *reinterpret_cast<const bf16x8*>(wsrc + (long)j * 32 * VQ_D + ks * 16);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[j], fh, acc[j], 0, 0, 0);
    }
    // lane: row `row`, channels g*256 + j*32 + 8q + 4*half + e (register 4q + e of tile j); rows past the clip hold zeros and add nothing
    float ts = 0.f, tq = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = acc[j][4 * q + e]; ts += v[e]; tq = __builtin_fmaf(v[e], v[e], tq); }
            if (ok) *reinterpret_cast<f32x4*>(ze + row * VQ_C + g * VQ_D + j * 32 + 8 * q + 4 * half) = v;
        }
    ts = wave_sum(ts);
    tq = wave_sum(tq);
    if (lane == 0) {
        float* dst = part + (((long)b * VQ_G + g) * nblk + blk) * 2;
        dst[0] = ts;
        dst[1] = tq;
    }
}

struct VqAssignArgs {
    const float* ze;       // [B * F][512] fp32 projections
    int F, keep, nblk;     // tokens of frames t < keep of every clip are written
    const float* gamma;    // vector_quantizer.projection.1 (GroupNorm(2, 512) affine)
    const float* beta;
    float eps;
    const float* part;     // [B][2][nblk][2] of k_vq_project
    const bf16_t* emb;     // centroids [2][320][256] bf16
    const float* e2;       // [2][320] squared norms of the centroids
    long* tok;             // [B][keep][2]
    float* scores;         // optional [B * F][2][320] fp32 (tests)
};

// Workgroup = 32 rows of one clip, two waves; wave g: GroupNorm of group g (statistics of the clip, per-channel affine) to LDS as bf16, then the
// 320 centroids of the group as the A operand of MFMA 32x32x16 and the normalised rows as B (the transposed form of k_w2v_quantize): the
// accumulator gives a lane one ROW and 16 centroids per tile; score = |e|^2 - 2 z.e; argmin in registers plus one exchange with lane ^ 32.
__global__ __launch_bounds__(128) void k_vq_assign(const VqAssignArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t sZ[VQ_G][VQ_QB * VQ_QP];
    __shared__ int sNan[VQ_G][VQ_QB];
    const int lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, f0 = blockIdx.x * VQ_QB, half = lane >> 5;
    {
        float mean, rstd;
        vq_finalize(p.part + ((long)b * VQ_G + g) * p.nblk * 2, p.nblk, (double)p.F * VQ_D, p.eps, mean, rstd);
        const int c0 = lane * 4;
        float gm[4], be[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { gm[c] = p.gamma[g * VQ_D + c0 + c]; be[c] = p.beta[g * VQ_D + c0 + c]; }
        for (int i = 0; i < VQ_QB; ++i) {
            const int f = f0 + i;
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            if (f < p.F) {                                         // (wave-uniform)
                const f32x4 v = *reinterpret_cast<const f32x4*>(p.ze + ((long)b * p.F + f) * VQ_C + g * VQ_D + c0);
#pragma unroll
                for (int c = 0; c < 4; ++c) a[c] = __builtin_fmaf((v[c] - mean) * rstd, gm[c], be[c]);
            }
            uint2 pk;
            pk.x = pack2bf(a[0], a[1]);
            pk.y = pack2bf(a[2], a[3]);
            *reinterpret_cast<uint2*>(&sZ[g][i * VQ_QP + c0]) = pk;
        }
    }
    __syncthreads();
    const int f = f0 + (lane & 31);
    const bool row_ok = f < p.F;
    const long row = (long)b * p.F + f;
    float best = INFINITY;
    int best_i = 0, any_nan = 0;
    const bf16_t* fsrc = &sZ[g][(lane & 31) * VQ_QP + half * 8];
    for (int h = 0; h < 2; ++h) {
        const int v0 = h * 160;                                     // first centroid of this half
        const bf16_t* wsrc = p.emb + ((long)g * VQ_V + v0 + (lane & 31)) * VQ_D + half * 8;
        f32x16 acc[5];
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll 4
        for (int ks = 0; ks < VQ_D / 16; ++ks) {
            const bf16x8 fh = *reinterpret_cast<const bf16x8*>(fsrc + ks * 16);
            bf16x8 fw[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) fw[j] = *reinterpret_cast<const bf16x8*>(wsrc + (long)j * 32 * VQ_D + ks * 16);
#pragma unroll
            for (int j = 0; j < 5; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[j], fh, acc[j], 0, 0, 0);
        }
        // lane: row `row`, centroids v0 + j*32 + 8q + 4*half + e (register 4q + e of tile j), visited in ascending order
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int v = v0 + j * 32 + 8 * q + 4 * half + e;
                    const float s = __builtin_fmaf(-2.0f, acc[j][4 * q + e], p.e2[g * VQ_V + v]);
                    if (p.scores != nullptr && row_ok) p.scores[(row * VQ_G + g) * VQ_V + v] = s;
                    any_nan |= __builtin_isnan(s) ? 1 : 0;
                    if (s < best) { best = s; best_i = v; }
                }
    }
    // lanes l and l ^ 32 hold the same row: the smaller score wins, a tie goes to the lower index; a NaN score in EITHER group (the other
    // wave's flag comes through LDS) makes both tokens of the row 0
    const auto xb = __builtin_amdgcn_permlane32_swap(__float_as_int(best), __float_as_int(best), false, false);
    const auto xi = __builtin_amdgcn_permlane32_swap(best_i, best_i, false, false);
    const auto xn = __builtin_amdgcn_permlane32_swap(any_nan, any_nan, false, false);
    const float b0 = __int_as_float(xb[0]), b1 = __int_as_float(xb[1]);
    const int i0 = xi[0], i1 = xi[1];
    const bool take1 = b1 < b0 || (b1 == b0 && i1 < i0);
    if (half == 0) sNan[g][lane] = xn[0] | xn[1];
    __syncthreads();
    const int win = (sNan[0][lane & 31] | sNan[1][lane & 31]) ? 0 : (take1 ? i1 : i0);
    if (row_ok && half == 0 && f < p.keep) p.tok[((long)b * p.keep + f) * VQ_G + g] = (long)win;
}

static inline int vq_frames0(int L_in, int pad) {
    const long L = (long)L_in + pad;
    if (L_in < 1 || pad < 0 || L < 10 || L >= (1L << 30)) return -1;
    return (int)((L - 10) / 5 + 1);
}

extern "C" int64_t svsr_vq_part_floats(int B, int F, int kind) {
    if (B < 1 || F < 1 || (kind != 0 && kind != 1)) return -SVSR_ERR_ARG;
    if (kind == 0) return (int64_t)B * ((F + VQ_FB - 1) / VQ_FB) * 2;
    return (int64_t)B * VQ_G * ((F + VQ_QB - 1) / VQ_QB) * 2;
}

extern "C" int svsr_vq_conv0_stats(const float* wave, int B, int L_in, int pad, const float* w, float* part, hipStream_t stream) {
    const int F0 = vq_frames0(L_in, pad);
    if (wave == nullptr || w == nullptr || part == nullptr || B < 1 || B > 65535 || F0 < 1) return SVSR_ERR_ARG;
    VqConv0Args a;
    a.wave = wave; a.L_in = L_in; a.F0 = F0; a.out_rows = 0; a.nblk = (F0 + VQ_FB - 1) / VQ_FB;
    a.w = w; a.gamma = nullptr; a.beta = nullptr; a.eps = 0.f; a.out = nullptr; a.part = part;
    hipLaunchKernelGGL(k_vq_conv0<false>, dim3(a.nblk, B), dim3(256), 0, stream, a);
    return svsr_check_launch();
}

extern "C" int svsr_vq_conv0_apply(const float* wave, int B, int L_in, int pad, const float* w, const float* gamma, const float* beta, float eps,
                                   const float* part, void* out, int out_rows, hipStream_t stream) {
    const int F0 = vq_frames0(L_in, pad);
    if (wave == nullptr || w == nullptr || gamma == nullptr || beta == nullptr || part == nullptr || out == nullptr) return SVSR_ERR_ARG;
    if (B < 1 || B > 65535 || F0 < 1 || out_rows < F0) return SVSR_ERR_ARG;
    VqConv0Args a;
    a.wave = wave; a.L_in = L_in; a.F0 = F0; a.out_rows = out_rows; a.nblk = (F0 + VQ_FB - 1) / VQ_FB;
    a.w = w; a.gamma = gamma; a.beta = beta; a.eps = eps; a.out = (bf16_t*)out; a.part = const_cast<float*>(part);
    hipLaunchKernelGGL(k_vq_conv0<true>, dim3(a.nblk, B), dim3(256), 0, stream, a);
    return svsr_check_launch();
}

extern "C" int svsr_vq_gn_partial(const void* x, int B, int F, int rows, float* part, hipStream_t stream) {
    if (x == nullptr || part == nullptr || B < 1 || B > 65535 || F < 1 || rows < F) return SVSR_ERR_ARG;
    const int nblk = (F + VQ_FB - 1) / VQ_FB;
    hipLaunchKernelGGL(k_vq_gn_partial, dim3(nblk, B), dim3(256), 0, stream, (const bf16_t*)x, F, rows, nblk, part);
    return svsr_check_launch();
}

extern "C" int svsr_vq_gn_relu(void* x, int B, int F, int rows, const float* gamma, const float* beta, float eps, const float* part, int mode,
                               hipStream_t stream) {
    if (x == nullptr || gamma == nullptr || beta == nullptr || part == nullptr || B < 1 || F < 1 || rows < F || (mode != 0 && mode != 1))
        return SVSR_ERR_ARG;
    const long nrows = (long)B * F;
    if ((nrows + 3) / 4 >= (1L << 31)) return SVSR_ERR_ARG;
    const int nblk = (F + VQ_FB - 1) / VQ_FB;
    hipLaunchKernelGGL(k_vq_gn_relu, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, stream, (bf16_t*)x, B, F, rows, nblk, gamma, beta, eps, part,
                       mode);
    return svsr_check_launch();
}

extern "C" int svsr_vq_project(const void* x, int B, int F, const void* w, float* ze, float* part, hipStream_t stream) {
    if (x == nullptr || w == nullptr || ze == nullptr || part == nullptr || B < 1 || B > 65535 || F < 1) return SVSR_ERR_ARG;
    const int nblk = (F + VQ_QB - 1) / VQ_QB;
    hipLaunchKernelGGL(k_vq_project, dim3(nblk, B), dim3(128), 0, stream, (const bf16_t*)x, F, nblk, (const bf16_t*)w, ze, part);
    return svsr_check_launch();
}

extern "C" int svsr_vq_assign(const float* ze, int B, int F, int keep, const float* gamma, const float* beta, float eps, const float* part,
                              const void* emb, const float* e2, int64_t* tok, float* scores_out, hipStream_t stream) {
    if (ze == nullptr || gamma == nullptr || beta == nullptr || part == nullptr || emb == nullptr || e2 == nullptr || tok == nullptr) return SVSR_ERR_ARG;
    if (B < 1 || B > 65535 || F < 1 || keep < 1 || keep > F) return SVSR_ERR_ARG;
    VqAssignArgs a;
    a.ze = ze; a.F = F; a.keep = keep; a.nblk = (F + VQ_QB - 1) / VQ_QB; a.gamma = gamma; a.beta = beta; a.eps = eps; a.part = part;
    a.emb = (const bf16_t*)emb; a.e2 = e2; a.tok = (long*)tok; a.scores = scores_out;
    hipLaunchKernelGGL(k_vq_assign, dim3(a.nblk, B), dim3(128), 0, stream, a);
    return svsr_check_launch();
}
