// Scoring of the LRS inference surface (syncvsr_amd/lrs_eval.py), gfx950, wave64:
//   * k_edit_distance: Levenshtein distance of N (hypothesis, reference) pairs of 64-bit ids with its split into substitutions, deletions
//     and insertions: what the reference's test_step asks of torchaudio.functional.edit_distance (lightning.py:17-20,127), for a batch.
// Integers only, no atomics, no LDS: every output is a pure function of the inputs.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------
// The table.  Row i = the first i hypothesis ids, column j = the first j reference ids, a cell = (cost, S, D, I):
//   cell(0,0) = 0;  cell(i,0) = i insertions;  cell(0,j) = j deletions;  for i, j >= 1 the candidates, in priority order,
//     1. cell(i-1,j-1), plus one substitution unless hyp[i-1] == ref[j-1]
//     2. cell(i,j-1) plus one deletion
//     3. cell(i-1,j) plus one insertion
//   the smallest cost wins, a tie goes to the earlier candidate, the counts travel with the chosen predecessor.
// One wave per pair.  Lane l owns the K = ceil(R / 64) consecutive columns l*K+1 .. l*K+K: their reference ids and the cells of the row it
// finished last stay in registers (2 * ED_STRIP 64-bit ids and 2 * ED_STRIP packed cells at most).  The lanes sweep the rows skewed by one
// row per lane: at step s lane l computes row s - l + 1, left to right.  What crosses lanes each step, one lane up: the last cell of the
// strip (the next lane's left neighbour) and the row's hypothesis id, which therefore is read from memory by lane 0 alone — and lane 0
// takes it from a 64-id chunk the wave loaded coalesced 64 steps earlier (the chunk after it is already in flight).  A pair takes
// H + (R - 1) / K <= H + 63 steps of at most K cells.  A cell is two words: cost, and S | D << 16 (I = cost - S - D; all <= 1024).
// Nothing behind a row's length is read; lengths are cut to [0, min(row stride, ED_MAX_LEN)].
// ---------------------------------------------------------------------------------------------------------------------
#define ED_MAX_LEN 1024
#define ED_STRIP (ED_MAX_LEN / 64)

__global__ __launch_bounds__(64) void k_edit_distance(const long* __restrict__ hyp, long ldh, const int* __restrict__ hyp_len,
                                                      const long* __restrict__ ref, long ldr, const int* __restrict__ ref_len,
                                                      int* __restrict__ out) {
    const long p = blockIdx.x;
    const int lane = threadIdx.x;
    const long capH = ldh < ED_MAX_LEN ? ldh : ED_MAX_LEN, capR = ldr < ED_MAX_LEN ? ldr : ED_MAX_LEN;
    int H = hyp_len[p], R = ref_len[p];
    H = __builtin_amdgcn_readfirstlane(H < 0 ? 0 : (H > capH ? (int)capH : H));
    R = __builtin_amdgcn_readfirstlane(R < 0 ? 0 : (R > capR ? (int)capR : R));
    int* o = out + p * 4;
    if (H == 0 || R == 0) {                                // a border cell: nothing to read
        if (lane == 0) { o[0] = H + R; o[1] = 0; o[2] = R; o[3] = H; }
        return;
    }
    const long* hy = hyp + p * ldh;
    const long* rf = ref + p * ldr;
    const int K = (R + 63) >> 6;                           // 1 .. ED_STRIP, the same for every lane
    const int j0 = lane * K;                               // this lane's columns: j0 + 1 .. j0 + ncols
    const int ncols = R - j0 < 0 ? 0 : (R - j0 < K ? R - j0 : K);
    long rid[ED_STRIP];
    int pa[ED_STRIP], pb[ED_STRIP];                        // the cells above: row 0 = j deletions
#pragma unroll
    for (int c = 0; c < ED_STRIP; ++c) {
        rid[c] = c < ncols ? rf[j0 + c] : 0;
        pa[c] = j0 + c + 1;
        pb[c] = (j0 + c + 1) << 16;
    }
    int da = j0, db = j0 << 16;                            // cell(i-1, j0) of the lane's next row (lane 0: i - 1 insertions)
    const int lr = (R - 1) / K;                            // the lane that owns column R
    const int nsteps = H + lr;
    long cur = lane < H ? hy[lane] : 0;
    long nxt = 64 + lane < H ? hy[64 + lane] : 0;
    int oa = 0, ob = 0, tlo = 0, thi = 0;                  // what this lane hands to the next: its strip's last cell and the row's id
    for (int s = 0; s < nsteps; ++s) {
        if ((s & 63) == 0 && s > 0) {
            cur = nxt;
            nxt = s + 64 + lane < H ? hy[s + 64 + lane] : 0;
        }
        const int hlo = __builtin_amdgcn_readlane((int)cur, s & 63), hhi = __builtin_amdgcn_readlane((int)(cur >> 32), s & 63);
        int la = __shfl_up(oa, 1, 64), lb = __shfl_up(ob, 1, 64), glo = __shfl_up(tlo, 1, 64), ghi = __shfl_up(thi, 1, 64);
        if (lane == 0) { la = s + 1; lb = 0; glo = hlo; ghi = hhi; }          // cell(i, 0) = i insertions, and hyp[i-1] = hyp[s]
        const int i = s - lane + 1;
        if (i >= 1 && i <= H && ncols > 0) {
            const long tok = (long)(((unsigned long)(unsigned)ghi << 32) | (unsigned)glo);
            int ca = da, cb = db, fa = la, fb = lb;        // diagonal and left neighbour of the strip's first cell
#pragma unroll
            for (int c = 0; c < ED_STRIP; ++c) {
                if (c < K) {
                    if (c < ncols) {
                        const int ua = pa[c], ub = pb[c];
                        const int neq = tok != rid[c] ? 1 : 0;
                        int na = ca + neq, nb = cb + neq;
                        if (fa + 1 < na) { na = fa + 1; nb = fb + 0x10000; }
                        if (ua + 1 < na) { na = ua + 1; nb = ub; }
                        ca = ua; cb = ub;
                        pa[c] = na; pb[c] = nb;
                        fa = na; fb = nb;
                    }
                }
            }
            da = la; db = lb;
            oa = fa; ob = fb;
            tlo = glo; thi = ghi;
        }
    }
    if (lane == lr) {                                      // its last finished row is row H
        const int cl = R - 1 - lr * K;
        int a = 0, b = 0;
#pragma unroll
        for (int c = 0; c < ED_STRIP; ++c)
            if (c == cl) { a = pa[c]; b = pb[c]; }
        const int S = b & 0xffff, D = (b >> 16) & 0xffff;
        o[0] = a; o[1] = S; o[2] = D; o[3] = a - S - D;
    }
}

extern "C" {

// one wave per pair, no LDS
int svsr_edit_distance(const int64_t* hyp, int64_t ldh, const int* hyp_len, const int64_t* ref, int64_t ldr, const int* ref_len, int N, int* out,
                       hipStream_t stream) {
    if (N < 1 || ldh < 0 || ldr < 0 || (hyp == nullptr && ldh > 0) || (ref == nullptr && ldr > 0) || hyp_len == nullptr || ref_len == nullptr ||
        out == nullptr)
        return SVSR_ERR_ARG;
    hipLaunchKernelGGL(k_edit_distance, dim3((unsigned)N), dim3(64), 0, stream, (const long*)hyp, (long)ldh, hyp_len, (const long*)ref, (long)ldr,
                       ref_len, out);
    return svsr_check_launch();
}

}  // extern "C"
