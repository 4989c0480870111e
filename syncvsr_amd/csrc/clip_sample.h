// The sampling of the word-level clip kernels (k_clip_prep in loss_optim.hip; k_lrw_clip_sums / k_lrw_clip_mix in lrw_prep.hip;
// k_dctcn_clip_mix in dctcn_prep.hip): one stored
// uint8 frame, a crop window (top, left, h, w) resized to H x W with bilinear sampling (align_corners = False, no antialias, source
// coordinates clamped to the window like torch's upsample_bilinear2d), the flip mirroring the output.
// Every kernel that includes this header gets the SAME bits for a pixel: the fused multiply-adds are written out and the compiler's own
// contraction is switched off inside the functions, so the rounding sequence does not depend on the code around the call.  The sequence
// is the one hipcc chose for k_clip_prep under -ffp-contract=fast when the expression stood there in plain arithmetic:
//   fy  = fma(y + 0.5, ch / H, -0.5)                    (fx likewise)
//   top = fma(wx, v01, (1 - wx) * v00),  bot = fma(wx, v11, (1 - wx) * v10),  v = fma(1 - wy, top, wy * bot)
//   out = fma(v, 1 / 255, -mean) * inv_std
#pragma once

struct ClipWindow { int top, left, ch, cw, flip; };

// row = one clip's {top, left, h, w, flip}; the window is clamped into the stored frame: no read outside it whatever the host drew
__device__ __forceinline__ ClipWindow clip_window_row(const int* __restrict__ row, int Hs, int Ws) {
    int top = row[0], left = row[1], ch = row[2], cw = row[3];
    const int flip = row[4];
    top = top < 0 ? 0 : (top > Hs - 1 ? Hs - 1 : top);
    left = left < 0 ? 0 : (left > Ws - 1 ? Ws - 1 : left);
    ch = ch < 1 ? 1 : (ch > Hs - top ? Hs - top : ch);
    cw = cw < 1 ? 1 : (cw > Ws - left ? Ws - left : cw);
    return ClipWindow{top, left, ch, cw, flip};
}

// params [B][5]: clip b's window
__device__ __forceinline__ ClipWindow clip_window(const int* __restrict__ params, int b, int Hs, int Ws) {
    return clip_window_row(params + b * 5, Hs, Ws);
}

// output pixel (y, x) of the H x W frame sampled from stored frame f [Hs][Ws]: a value in [0, 255] (x / 255 comes with clip_normalize)
__device__ __forceinline__ float clip_sample(const unsigned char* __restrict__ f, const ClipWindow& w, int Ws, int y, int x, int H, int W) {
#pragma clang fp contract(off)
    const int xo = w.flip ? W - 1 - x : x;
    // source coordinates inside the window (pixel centres), clamped to the window like torch's upsample_bilinear2d
    float fy = __builtin_fmaf((float)y + 0.5f, (float)w.ch / (float)H, -0.5f);
    float fx = __builtin_fmaf((float)xo + 0.5f, (float)w.cw / (float)W, -0.5f);
    fy = fmaxf(fy, 0.f); fx = fmaxf(fx, 0.f);
    int y0 = (int)fy, x0 = (int)fx;
    if (y0 > w.ch - 1) y0 = w.ch - 1;
    if (x0 > w.cw - 1) x0 = w.cw - 1;
    const int y1 = y0 + 1 < w.ch ? y0 + 1 : w.ch - 1, x1 = x0 + 1 < w.cw ? x0 + 1 : w.cw - 1;
    const float wy = fy - (float)y0, wx = fx - (float)x0;
    const float v00 = f[(w.top + y0) * Ws + w.left + x0], v01 = f[(w.top + y0) * Ws + w.left + x1];
    const float v10 = f[(w.top + y1) * Ws + w.left + x0], v11 = f[(w.top + y1) * Ws + w.left + x1];
    const float top = __builtin_fmaf(wx, v01, (1.f - wx) * v00);
    const float bot = __builtin_fmaf(wx, v11, (1.f - wx) * v10);
    return __builtin_fmaf(1.f - wy, top, wy * bot);
}

// Normalize(x / 255) of a sampled value
__device__ __forceinline__ float clip_normalize(float v, float mean, float inv_std) {
#pragma clang fp contract(off)
    return __builtin_fmaf(v, 1.0f / 255.0f, -mean) * inv_std;
}
