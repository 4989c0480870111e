// Multi-clip beam search of the LRS inference surface (syncvsr_amd/lrs_infer.py BatchBeamSearch.forward_clips), gfx950, wave64:
//   * k_beam_select_slices / k_beam_select_merge: the selection step of one search position for every clip at once — the weighted
//     sum of the scorers' planes, the running score, and the per-clip top `beam` (the torch statement: lrs_infer.beam_select_reference)
//   * k_ctc_prefix_score_clips: the CTC prefix recursion of both searches, every hypothesis walking the frames of ITS clip
//   * k_mha_src_step: source attention of one query row per hypothesis against the keys / values of its clip
//   * k_ctc_align: CTC forced alignment (Viterbi over the CTC lattice) of a batch of clips, the back end of lrs_align.align_clips
//   * k_ctc_frame_best / k_ctc_collapse: CTC best-path (greedy) decoding of a batch of clips, the back end of lrs_align.greedy_clips
// No float atomics and no order that depends on arrival anywhere: every output is a pure function of the inputs.
#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------
// Selection.  Element (r, v) of clip c (rows lo_c .. hi_c - 1 of the planes, flat index f = (r - lo_c) * V + v) has the total
//   t = ((((0 + w0 * s0[r][v]) + w1 * s1[r][v]) + ...) + run[r])          every product and sum rounded on its own (no FMA)
// which is, operation for operation, what `weighted = zeros; weighted += w_k * s_k ...; weighted += score[:, None]` evaluates.
// Order: higher t first, ties to the lower f.  Both are carried by ONE 64-bit key, key = ord(t) << 20 | (2^20 - 1 - f) with ord() the
// usual monotone map of fp32 bits to unsigned (NaN above everything, as torch.topk sorts it): keys of one clip are distinct, so
// "the k largest keys" is a set that no schedule can change.
// Stage 1 (grid: slices x clips): a workgroup owns SL consecutive f, 256 threads hold BS_PER keys each in registers, and `k` rounds of a
// workgroup-wide max (wave reduction by DPP shuffles, then 4 partials through LDS) peel off the slice's best min(k, slice) keys in order.
// Stage 2 (grid: clips): the same rounds over the slices' candidates (at most BS_CAND); the winner's planes are read again for the
// outputs, so the totals are recomputed, not decoded.
// ---------------------------------------------------------------------------------------------------------------------
#define BS_THREADS 256
#define BS_PER 16
#define BS_CAND (BS_THREADS * BS_PER)          // keys one workgroup ranks: the largest slice, and slices * beam of the merge
#define BS_IDX_BITS 20
#define BS_IDX_MASK ((1u << BS_IDX_BITS) - 1u)
#define BS_MAX_PLANES 4

struct BeamPlanes {
    const float* s[BS_MAX_PLANES];
    float w[BS_MAX_PLANES];
    int n;
};

// (the library is built with -ffp-contract=fast, and neither `#pragma clang fp contract(off)` nor __fmul_rn keeps the compiler from fusing
// these into v_fmac_f32 after inlining: the two instructions are named, so each rounds on its own)
__device__ __forceinline__ float mul_rn(float a, float b) { float r; asm volatile("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float add_rn(float a, float b) { float r; asm volatile("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

__device__ __forceinline__ float beam_total(const BeamPlanes& p, const float* __restrict__ run, long ldv, int r, int v) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < BS_MAX_PLANES; ++i)
        if (i < p.n) t = add_rn(t, mul_rn(p.w[i], p.s[i][(long)r * ldv + v]));
    return add_rn(t, run[r]);
}

__device__ __forceinline__ unsigned beam_ord(float t) {
    if (t != t) return 0xffffffffu;
    const unsigned u = __float_as_uint(t);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)k, o, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        k = other > k ? other : k;
    }
    return k;
}

// the `rounds` largest of the workgroup's keys (0 = no key), in order, into win[0 .. rounds): every thread returns with win[] complete
__device__ __forceinline__ void beam_rounds(unsigned long long (&key)[BS_PER], int rounds, unsigned long long* part, unsigned long long* win) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long cur = 0;
#pragma unroll
    for (int i = 0; i < BS_PER; ++i) cur = key[i] > cur ? key[i] : cur;
    for (int k = 0; k < rounds; ++k) {
        const unsigned long long wm = wave_max_u64(cur);
        if (lane == 0) part[(k & 1) * 4 + wave] = wm;
        __syncthreads();                                  // (part is double buffered: one barrier per round is enough)
        unsigned long long best = part[(k & 1) * 4];
#pragma unroll
        for (int w = 1; w < BS_THREADS / 64; ++w) { const unsigned long long o = part[(k & 1) * 4 + w]; best = o > best ? o : best; }
        if (threadIdx.x == 0) win[k] = best;
        if (best != 0 && cur == best) {                   // keys are distinct: exactly one thread owns the winner
            cur = 0;
#pragma unroll
            for (int i = 0; i < BS_PER; ++i) {
                if (key[i] == best) key[i] = 0;
                cur = key[i] > cur ? key[i] : cur;
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(BS_THREADS) void k_beam_select_slices(BeamPlanes p, const float* __restrict__ run, const int* __restrict__ row_lo,
                                                                   long ldv, int V, int beam, int SL, int n,
                                                                   unsigned long long* __restrict__ cand) {
    __shared__ unsigned long long part[8];
    __shared__ unsigned long long win[BS_CAND / 16];      // beam <= 256
    const int c = blockIdx.y, g = blockIdx.x;
    int lo = row_lo[c], hi = row_lo[c + 1];
    lo = lo < 0 ? 0 : lo; hi = hi > n ? n : hi;           // (a damaged range cannot make the kernel leave the planes)
    const long N = hi > lo ? (long)(hi - lo) * V : 0;
    const long f0 = (long)g * SL;
    if (f0 >= N) return;                                  // whole workgroups leave
    const int len = (int)(N - f0 < SL ? N - f0 : SL);
    unsigned long long key[BS_PER];
#pragma unroll
    for (int i = 0; i < BS_PER; ++i) {
        const int j = i * BS_THREADS + threadIdx.x;       // consecutive lanes read consecutive tokens
        key[i] = 0;
        if (j < len) {
            const unsigned f = (unsigned)f0 + (unsigned)j;                  // N <= 2^20: 32-bit index arithmetic
            const int r = lo + (int)(f / (unsigned)V), v = (int)(f % (unsigned)V);
            key[i] = ((unsigned long long)beam_ord(beam_total(p, run, ldv, r, v)) << BS_IDX_BITS) | (unsigned long long)(BS_IDX_MASK - (unsigned)f);
        }
    }
    const int k = beam < len ? beam : len;
    beam_rounds(key, k, part, win);
    unsigned long long* out = cand + ((long)c * gridDim.x + g) * beam;
    for (int i = threadIdx.x; i < k; i += BS_THREADS) out[i] = win[i];
}

__global__ __launch_bounds__(BS_THREADS) void k_beam_select_merge(BeamPlanes p, const float* __restrict__ run, const int* __restrict__ clip_of,
                                                                  const int* __restrict__ row_lo, const int* __restrict__ out_off, long ldv, int V,
                                                                  int beam, int SL, int G, int n, int out_rows,
                                                                  const unsigned long long* __restrict__ cand, long* __restrict__ prev,
                                                                  long* __restrict__ tok, float* __restrict__ total, float* __restrict__ vals,
                                                                  int* __restrict__ clip_out, int* __restrict__ count) {
    __shared__ unsigned long long part[8];
    __shared__ unsigned long long win[BS_CAND / 16];
    const int c = blockIdx.x;
    int lo = row_lo[c], hi = row_lo[c + 1];
    lo = lo < 0 ? 0 : lo; hi = hi > n ? n : hi;
    const long N = hi > lo ? (long)(hi - lo) * V : 0;
    const int k = (int)(N < beam ? N : beam);
    if (threadIdx.x == 0) count[c] = k;
    if (k == 0) return;
    const int Gc = (int)((N + SL - 1) / SL);              // slices of this clip that hold elements (<= G)
    unsigned long long key[BS_PER];
#pragma unroll
    for (int i = 0; i < BS_PER; ++i) {
        const int j = i * BS_THREADS + threadIdx.x;       // candidate j = slice j / beam, rank j % beam
        key[i] = 0;
        const int g = j / beam, q = j - g * beam;
        if (g < Gc && g < G) {
            const long left = N - (long)g * SL;
            const int len = (int)(left < SL ? left : SL);
            if (q < (beam < len ? beam : len)) key[i] = cand[((long)c * G + g) * beam + q];
        }
    }
    beam_rounds(key, k, part, win);
    const int o0 = out_off[c];
    for (int i = threadIdx.x; i < k; i += BS_THREADS) {
        const int o = o0 + i;
        if (o < 0 || o >= out_rows) continue;
        const unsigned f = BS_IDX_MASK - (unsigned)(win[i] & BS_IDX_MASK);
        if ((long)f >= N) continue;                       // (cannot happen with keys this launch pair made)
        const int r = lo + (int)(f / (unsigned)V), v = (int)(f % (unsigned)V);
        prev[o] = r;
        tok[o] = v;
        total[o] = beam_total(p, run, ldv, r, v);
        for (int i2 = 0; i2 < p.n; ++i2) vals[(long)i2 * out_rows + o] = p.s[i2][(long)r * ldv + v];
        clip_out[o] = clip_of[r];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// CTC prefix scores for beam search (Watanabe et al., "Hybrid CTC/attention architecture for end-to-end speech recognition",
// Algorithm 2; the reference vectorises it in torch, espnet/nets/ctc_prefix_score.py:11-165, one launch of ~10 small kernels per
// frame).  Here one thread owns one (hypothesis, candidate label) pair and walks the frames of the recursion in registers:
//   r_n[t] = logaddexp(r_n[t-1], phi[t-1]) + logp[t][c]         phi[t] = r_b_prev[t] if c == last label else logaddexp(r_n_prev[t], r_b_prev[t])
//   r_b[t] = logaddexp(r_n[t-1], r_b[t-1]) + logp[t][blank]
//   psi    = logsumexp(r_n[start-1], phi[t-1] + logp[t][c] for t in [start, T)),   start = max(#labels in the prefix, 1)
// eos gets logaddexp(r_n_prev[T-1], r_b_prev[T-1]), blank gets LOGZERO.  r_new [n][S][Tmax][2] is the state of each extension.
// Hypothesis h belongs to clip c = clip_of[h] (null: clip 0) and walks the Tc = tlen[c] (null: Tmax) frames of logp[c]; frames
// Tc .. Tmax - 1 of the new state are LOGZERO and nothing reads the padding of logp or r_prev.  Candidate ids and last labels are compared
// as int64, before any narrowing: an id outside [0, V) (2^32 + 5 included) is an impossible extension, and a last label outside [0, V)
// matches no candidate.
// ---------------------------------------------------------------------------------------------------------------------
#define CTC_LOGZERO (-1.0e10f)
__device__ __forceinline__ float lae(float a, float b) {
    const float m = fmaxf(a, b);
    return m + __logf(__expf(a - m) + __expf(b - m));
}

__global__ __launch_bounds__(256) void k_ctc_prefix_score_clips(const float* __restrict__ logp, const float* __restrict__ r_prev,
                                                                const long* __restrict__ last, const long* __restrict__ ids,
                                                                const int* __restrict__ clip_of, const int* __restrict__ tlen,
                                                                float* __restrict__ r_new, float* __restrict__ psi, int C, int Tmax, int V, int ldp,
                                                                int n, int S, int out_len, int blank, int eos) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)n * S) return;
    const int h = (int)(idx / S), j = (int)(idx - (long)h * S);
    float* rn_out = r_new + idx * Tmax * 2;
    const int clip = clip_of != nullptr ? clip_of[h] : 0;
    const long id = ids != nullptr ? ids[(long)h * S + j] : (long)j;           // ranged as the 64-bit value it is: 2^32 + 5 is not label 5
    const int c = (int)id;
    int T = (clip >= 0 && clip < C) ? (tlen != nullptr ? tlen[clip] : Tmax) : 0;
    T = T > Tmax ? Tmax : T;
    if (T < 1 || id < 0 || id >= (long)V) {                // no clip / no such label: an impossible extension, never a stray read
        for (int t = 0; t < Tmax; ++t) { rn_out[2 * t] = CTC_LOGZERO; rn_out[2 * t + 1] = CTC_LOGZERO; }
        psi[idx] = CTC_LOGZERO;
        return;
    }
    const float* lp = logp + (long)clip * Tmax * ldp;
    const float* rp = r_prev + (long)h * Tmax * 2;
    const bool same = id == last[h];                       // (64-bit too: a last label outside [0, V) equals no candidate)
    const int start = out_len > 1 ? out_len : 1;
    for (int t = 0; t < start - 1 && t < T; ++t) { rn_out[2 * t] = CTC_LOGZERO; rn_out[2 * t + 1] = CTC_LOGZERO; }
    float rn = (out_len == 0) ? lp[c] : CTC_LOGZERO, rb = CTC_LOGZERO;          // r[start-1]
    if (start - 1 < T) { rn_out[2 * (start - 1)] = rn; rn_out[2 * (start - 1) + 1] = rb; }
    float acc = rn;
    for (int t = start; t < T; ++t) {
        const float pn = rp[2 * (t - 1)], pb = rp[2 * (t - 1) + 1];
        const float phi = same ? pb : lae(pn, pb);
        const float x = lp[(long)t * ldp + c], xb = lp[(long)t * ldp + blank];
        acc = lae(acc, phi + x);
        const float nn = lae(rn, phi) + x;
        const float nb = lae(rn, rb) + xb;
        rn = nn; rb = nb;
        rn_out[2 * t] = rn; rn_out[2 * t + 1] = rb;
    }
    for (int t = T; t < Tmax; ++t) { rn_out[2 * t] = CTC_LOGZERO; rn_out[2 * t + 1] = CTC_LOGZERO; }
    if (c == eos) acc = lae(rp[2 * (T - 1)], rp[2 * (T - 1) + 1]);
    if (c == blank) acc = CTC_LOGZERO;
    psi[idx] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// CTC forced alignment: the Viterbi member of the lattice family (k_ctc_lattice sums the paths, this keeps the best one).  What the
// reference's CTC.forced_align_batch computes with a numpy loop over frames (ctc.py:246-328), for one clip per workgroup:
//   ext = [blank, y1, blank, ..., yL, blank], S = 2L + 1;   d[0][0] = lp[0][blank], d[0][1] = lp[0][y1], -inf elsewhere
//   d[t][s] = best(d[t-1][s], d[t-1][s-1], d[t-1][s-2]) + lp[t][ext[s]]      s-2 only for odd s >= 3 with ext[s] != ext[s-2]
//   end: the larger of d[T-1][S-2] and d[T-1][S-1] (S-2 on a tie), then the back-pointers down to frame 0.
// The results are EQUAL to the reference's, not close: best() compares in that order with strict > (the first maximum wins, argmax's rule; a
// missing candidate is the reference's -inf, which strict > never selects, and all -inf selects "stay"), and a cell is ONE fp32 add of the
// selected candidate and the emission.  States are strided over the 256 threads (up to CA_PER each, in registers: S <= 2048), prev / cur
// rows in LDS, one barrier per frame, one back-pointer byte (0, 1, 2 states back) per cell in bp [B][Tmax][2 Lmax + 1].  The emissions are
// a gather of S values per frame: the loads of frame t + 1 are issued before the barrier of frame t.  Then one thread walks the
// back-pointers and leaves the state of every frame in LDS, and all threads write frames and spans (each word has one writer).
// This is a chain of T dependent steps per clip — latency, not throughput.
// The transcript is everything in front of the run of -1 at the tail of labels[b]; a clip with a label outside [0, V) (compared as the
// int64 it is) or equal to blank, with no label or no frame, or whose best path is -inf (too few frames, emissions at -inf) is
// infeasible: score -inf, frames and spans -1, and nothing of logp is read through such a label.
// ---------------------------------------------------------------------------------------------------------------------
#define CA_THREADS 256
#define CA_PER 8
#define CA_MAX_S (CA_THREADS * CA_PER)
#define CA_MAX_LDS 65536

__device__ __forceinline__ void ctc_align_none(int* fr, int* sp, float* sc, int Tmax, int Lmax) {
    for (int t = threadIdx.x; t < Tmax; t += CA_THREADS) fr[t] = -1;
    for (int i = threadIdx.x; i < 2 * Lmax; i += CA_THREADS) sp[i] = -1;
    if (threadIdx.x == 0) *sc = -INFINITY;
}

__global__ __launch_bounds__(CA_THREADS) void k_ctc_align(const float* __restrict__ logp, int ldp, const int* __restrict__ tlen,
                                                          const long* __restrict__ labels, int Lmax, int Tmax, int V, int blank,
                                                          unsigned char* bp, int* __restrict__ frames, int* __restrict__ spans,
                                                          float* __restrict__ score) {
    extern __shared__ float sm[];             // prev[Smax], cur[Smax], ext (int)[Smax], path (u16)[Tmax]
    __shared__ int s_red[8];
    __shared__ int s_end;
    const int Smax = 2 * Lmax + 1;
    float* prev = sm;
    float* cur = sm + Smax;
    int* ext = reinterpret_cast<int*>(sm + 2 * Smax);
    unsigned short* path = reinterpret_cast<unsigned short*>(sm + 3 * Smax);
    const int b = blockIdx.x, tid = threadIdx.x;
    const long* lab = labels + (long)b * Lmax;
    int* fr = frames + (long)b * Tmax;
    int* sp = spans + (long)b * Lmax * 2;

    int L = 0, hole = Lmax;                   // labels in front of the -1 tail; the first entry that is no label of this vocabulary
    for (int l = tid; l < Lmax; l += CA_THREADS) {
        const long v = lab[l];
        if (v != -1) L = l + 1;
        if ((v < 0 || v >= (long)V || v == (long)blank) && l < hole) hole = l;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int oL = __shfl_xor(L, o, 64), oh = __shfl_xor(hole, o, 64);
        L = oL > L ? oL : L;
        hole = oh < hole ? oh : hole;
    }
    if ((tid & 63) == 0) { s_red[tid >> 6] = L; s_red[4 + (tid >> 6)] = hole; }
    __syncthreads();
    L = max(max(s_red[0], s_red[1]), max(s_red[2], s_red[3]));
    hole = min(min(s_red[4], s_red[5]), min(s_red[6], s_red[7]));
    const bool bad = hole < L;                // (a -1 in front of a label included: the padding is the tail only)
    int T = tlen[b];
    T = T > Tmax ? Tmax : T;
    if (bad || L < 1 || T < 1) {              // (the same for every thread of the workgroup)
        ctc_align_none(fr, sp, score + b, Tmax, Lmax);
        return;
    }
    const int S = 2 * L + 1, nk = (S + CA_THREADS - 1) / CA_THREADS;
    const float* lpb = logp + (long)b * Tmax * ldp;
    unsigned char* bpb = bp + (long)b * Tmax * Smax;

    int col[CA_PER];                          // ext of this thread's states, and whether they may be entered from two states back
    bool skip[CA_PER];
    float e[CA_PER];                          // their emissions at the frame about to be computed
#pragma unroll
    for (int k = 0; k < CA_PER; ++k) {
        const int s = tid + k * CA_THREADS;
        col[k] = blank; skip[k] = false; e[k] = 0.f;
        if (k < nk && s < S) {
            if (s & 1) {
                col[k] = (int)lab[s >> 1];
                skip[k] = s >= 3 && lab[s >> 1] != lab[(s >> 1) - 1];
            }
            ext[s] = col[k];
            prev[s] = s == 0 ? lpb[blank] : (s == 1 ? lpb[col[k]] : -INFINITY);
            if (T > 1) e[k] = lpb[(long)ldp + col[k]];
        }
    }
    __syncthreads();
    for (int t = 1; t < T; ++t) {
        float en[CA_PER];
#pragma unroll
        for (int k = 0; k < CA_PER; ++k) {    // the gather of frame t + 1: in flight across this frame's barrier
            const int s = tid + k * CA_THREADS;
            en[k] = 0.f;
            if (k < nk && s < S && t + 1 < T) en[k] = lpb[(long)(t + 1) * ldp + col[k]];
        }
#pragma unroll
        for (int k = 0; k < CA_PER; ++k) {
            const int s = tid + k * CA_THREADS;
            if (k < nk && s < S) {
                float best = prev[s];
                unsigned char back = 0;
                if (s >= 1) { const float c = prev[s - 1]; if (c > best) { best = c; back = 1; } }
                if (skip[k]) { const float c = prev[s - 2]; if (c > best) { best = c; back = 2; } }
                cur[s] = best + e[k];
                bpb[(long)t * Smax + s] = back;
            }
        }
        __syncthreads();
        float* tmp = prev; prev = cur; cur = tmp;
#pragma unroll
        for (int k = 0; k < CA_PER; ++k) e[k] = en[k];
    }
    if (tid == 0) {
        int s = prev[S - 1] > prev[S - 2] ? S - 1 : S - 2;
        const float sc = prev[s];
        const bool ok = sc > -INFINITY;      // (false for NaN too)
        score[b] = ok ? sc : -INFINITY;
        s_end = ok ? s : -1;
        if (ok) {
            for (int t = T - 1; t >= 1; --t) {
                path[t] = (unsigned short)s;
                s -= bpb[(long)t * Smax + s];
            }
            path[0] = (unsigned short)s;
        }
    }
    __syncthreads();
    if (s_end < 0) {
        ctc_align_none(fr, sp, score + b, Tmax, Lmax);
        return;
    }
    for (int t = tid; t < Tmax; t += CA_THREADS) {
        int tok = -1;
        if (t < T) {
            const int st = path[t];
            tok = ext[st];
            if (st & 1) {                     // every label state is visited: each of its two words has exactly one writer
                if (t == 0 || path[t - 1] != st) sp[st - 1] = t;          // spans[l][0], l = st >> 1
                if (t == T - 1 || path[t + 1] != st) sp[st] = t;           // spans[l][1]
            }
        }
        fr[t] = tok;
    }
    for (int i = 2 * L + tid; i < 2 * Lmax; i += CA_THREADS) sp[i] = -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// CTC best-path (greedy) decoding, two launches.  What `CTC.argmax` (ctc.py:172) and the host `groupby` behind it compute, without the
// [C][Tmax][V] log-softmax in between.
// k_ctc_frame_best: one wave per row (c, t) of the fp32 LOGITS, one pass.  A lane walks its columns in rising order and carries
//   m   the largest value so far (strict >: the first maximum wins; NaN never wins here)     idx   its column
//   s   sum of exp(x - m) over what it has seen, rescaled whenever m rises                   nan   its first NaN column
// 16-byte loads over the whole groups of four columns below V when the rows are 16-byte aligned (four loads in flight per lane), single
// loads for the V % 4 columns behind them and for unaligned rows: no column >= V and no row t >= tlen[c] is ever read.  The 64 triples
// are merged by a fixed xor butterfly — the larger m, on equal m the lower column, s rescaled to the common m — so every lane ends with
// the same bits whatever the launch, and nothing is accumulated through memory.  best = the first NaN's column if the row has one
// (torch.argmax's rule), else idx; best_logp = x[best] - logsumexp(x) = -log(s) (NaN for a row with a NaN or of -inf only).
// HBM-bound by construction: rows * V * 4 bytes read once, 8 written per row.
// ---------------------------------------------------------------------------------------------------------------------
#define CG_NONE 0x7fffffff

struct FrameBest {
    float m, s;
    int idx, nan;
};

__device__ __forceinline__ void fb_take4(FrameBest& a, const f32x4 x, int j) {
    float mc = a.m;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (x[k] > mc) { mc = x[k]; a.idx = j + k; }
        if (x[k] != x[k]) a.nan = min(a.nan, j + k);
    }
    if (mc > -INFINITY)                                    // (all -inf so far: s stays 0 and exp(-inf - -inf) is never formed)
        a.s = a.s * __expf(a.m - mc) + ((__expf(x[0] - mc) + __expf(x[1] - mc)) + (__expf(x[2] - mc) + __expf(x[3] - mc)));
    a.m = mc;
}

__device__ __forceinline__ void fb_take1(FrameBest& a, float x, int j) {
    float mc = a.m;
    if (x > mc) { mc = x; a.idx = j; }
    if (x != x) a.nan = min(a.nan, j);
    if (mc > -INFINITY) a.s = a.s * __expf(a.m - mc) + __expf(x - mc);
    a.m = mc;
}

__device__ __forceinline__ void fb_merge(float& m, float& sum, int& idx, int& nan, float bm, float bs, int bi, int bn) {
    const bool tb = bm > m || (bm == m && bi < idx);
    const float nm = tb ? bm : m;
    sum = nm > -INFINITY ? sum * __expf(m - nm) + bs * __expf(bm - nm) : 0.f;
    m = nm;
    idx = tb ? bi : idx;
    nan = min(nan, bn);
}

__global__ __launch_bounds__(64) void k_ctc_frame_best(const float* __restrict__ logits, long ldp, const int* __restrict__ tlen, int Tmax, int V,
                                                       int vec, int* __restrict__ best, float* __restrict__ best_logp) {
    const int row = (int)blockIdx.x, lane = threadIdx.x;  // (rows < 2^31: the launcher checks)
    const int c = row / Tmax, t = row - c * Tmax;
    if (t >= tlen[c]) {                                    // (the same for the whole wave) padding: nothing of the row is read
        if (lane == 0) { best[row] = -1; best_logp[row] = 0.f; }
        return;
    }
    const float* x = logits + (long)row * ldp;
    FrameBest a = {-INFINITY, 0.f, CG_NONE, CG_NONE};
    int done = 0;                                          // columns [0, done) go through 16-byte loads
    if (vec) {
        const f32x4* xv = reinterpret_cast<const f32x4*>(x);
        const int nq = V >> 2;
        done = nq << 2;
        int q = lane;
        for (; q + 192 < nq; q += 256) {
            const f32x4 v0 = xv[q], v1 = xv[q + 64], v2 = xv[q + 128], v3 = xv[q + 192];
            fb_take4(a, v0, q * 4);
            fb_take4(a, v1, (q + 64) * 4);
            fb_take4(a, v2, (q + 128) * 4);
            fb_take4(a, v3, (q + 192) * 4);
        }
        for (; q < nq; q += 64) fb_take4(a, xv[q], q * 4);
    }
    for (int j = done + lane; j < V; j += 64) fb_take1(a, x[j], j);
    float m = a.m, sum = a.s;
    int idx = a.idx, nan = a.nan;
#pragma unroll
    for (int o = 1; o <= 32; o <<= 1)
        fb_merge(m, sum, idx, nan, __shfl_xor(m, o, 64), __shfl_xor(sum, o, 64), __shfl_xor(idx, o, 64), __shfl_xor(nan, o, 64));
    if (lane == 0) {
        const bool isnan_row = nan != CG_NONE;
        best[row] = isnan_row ? nan : (idx == CG_NONE ? 0 : idx);             // (every column -inf: all equal, the first wins)
        best_logp[row] = (isnan_row || !(m > -INFINITY)) ? __builtin_nanf("") : -logf(sum);     // (a row of -inf has no softmax: NaN, as torch)
    }
}

// k_ctc_collapse: one workgroup per clip.  The winners and their log-probabilities of the clip's T = tlen[c] frames go to LDS; frame t starts
// a token when best[t] != blank and (t == 0 or best[t] != best[t-1]).  A thread owns a stretch of consecutive frames; the token number of
// a start is the exclusive prefix sum of the flags (per-thread counts, a wave scan, four wave totals through LDS: positions follow from
// the frames alone, never from arrival).  The thread that owns a start walks its run to the end: the fp32 sum of best_logp in frame order
// over the run length (a correctly rounded division) is token_logp.  Thread 0 adds up the clip's score, also in frame order.  Rows behind
// ntok are filled: tokens -1, spans (-1, -1), token_logp 0.  Nothing is written at or behind row Lcap.  Short dependent chains on a few
// KB: latency, not throughput.
// dynamic LDS: winners (int)[Tmax] | log-probabilities [Tmax] | wave totals (int)[4]
#define CG_THREADS 256
#define CG_MAX_T 4096

__global__ __launch_bounds__(CG_THREADS) void k_ctc_collapse(const int* __restrict__ best, const float* __restrict__ best_logp,
                                                             const int* __restrict__ tlen, int Tmax, int Lcap, int blank, long* __restrict__ tokens,
                                                             int* __restrict__ spans, float* __restrict__ token_logp, int* __restrict__ ntok,
                                                             float* __restrict__ score) {
    extern __shared__ __attribute__((aligned(16))) int cg_sm[];
    int* sb = cg_sm;
    float* sl = reinterpret_cast<float*>(cg_sm + Tmax);
    int* wtot = cg_sm + 2 * Tmax;
    const int c = blockIdx.x, tid = threadIdx.x;
    int T = tlen[c];
    T = T > Tmax ? Tmax : (T < 0 ? 0 : T);
    long* tk = tokens + (long)c * Lcap;
    int* sp = spans + (long)c * Lcap * 2;
    float* tl = token_logp + (long)c * Lcap;
    for (int t = tid; t < T; t += CG_THREADS) {
        sb[t] = best[(long)c * Tmax + t];
        sl[t] = best_logp[(long)c * Tmax + t];
    }
    __syncthreads();
    const int per = (T + CG_THREADS - 1) / CG_THREADS;
    const int t0 = min(tid * per, T), t1 = min(t0 + per, T);
    int cnt = 0;
    for (int t = t0; t < t1; ++t) cnt += (sb[t] != blank && (t == 0 || sb[t] != sb[t - 1])) ? 1 : 0;
    int inc = cnt;                                         // inclusive scan of the counts within the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if ((tid & 63) >= o) inc += up;
    }
    if ((tid & 63) == 63) wtot[tid >> 6] = inc;
    __syncthreads();
    int l = inc - cnt, total = 0;
#pragma unroll
    for (int w = 0; w < CG_THREADS / 64; ++w) {
        if (w < (tid >> 6)) l += wtot[w];
        total += wtot[w];
    }
    for (int t = t0; t < t1; ++t) {
        const int v = sb[t];
        if (v == blank || (t > 0 && v == sb[t - 1])) continue;
        float sum = sl[t];
        int e = t;
        while (e + 1 < T && sb[e + 1] == v) { ++e; sum += sl[e]; }
        if (l < Lcap) {
            tk[l] = (long)v;
            sp[2 * l] = t;
            sp[2 * l + 1] = e;
            tl[l] = __fdiv_rn(sum, (float)(e - t + 1));
        }
        ++l;
    }
    for (int i = total + tid; i < Lcap; i += CG_THREADS) {
        tk[i] = -1;
        sp[2 * i] = -1;
        sp[2 * i + 1] = -1;
        tl[i] = 0.f;
    }
    if (tid == 0) {
        float sc = 0.f;
        for (int t = 0; t < T; ++t) sc += sl[t];
        score[c] = sc;
        ntok[c] = total;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Source attention of a beam step: one wave per (hypothesis r, head h).  The query is row r of q; the keys / values are rows
// clip_of[r] * Tmax + [0, tlen[clip]) of kv (k | v per row, projected once per clip and layer).  Structure of k_mha_table (lrs_lm.hip):
// keys in chunks of 64, lane l owns key c * 64 + l for the scores, online softmax in fp32, then lane l owns channel l of the weighted
// sum of the values.  A row without a clip or a clip without frames writes zeros.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mha_src_step(const bf16_t* __restrict__ q, long q_pitch, const bf16_t* __restrict__ kv, long kv_pitch,
                                                      const int* __restrict__ clip_of, const int* __restrict__ tlen, int C, int Tmax, int n, int H,
                                                      float scale, bf16_t* __restrict__ ctx, long ctx_pitch) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= (long)n * H) return;                          // whole waves leave: nothing below synchronises across waves
    const int h = (int)(w % H), r = (int)(w / H);
    const int D = H * 64;
    bf16_t* out = ctx + (long)r * ctx_pitch + h * 64 + lane;
    const int clip = clip_of[r];
    int T = (clip >= 0 && clip < C) ? tlen[clip] : 0;
    T = T > Tmax ? Tmax : T;
    if (T < 1) { *out = 0; return; }
    const bf16_t* base = kv + (long)clip * Tmax * kv_pitch + h * 64;

    float qf[64];
    {
        const u32x4* qp = reinterpret_cast<const u32x4*>(q + (long)r * q_pitch + h * 64);
#pragma unroll
        for (int c = 0; c < 8; ++c) unpack8(qp[c], qf + c * 8);
    }
    float m = -INFINITY, l = 0.f, acc = 0.f;
    for (int k0 = 0; k0 < T; k0 += 64) {
        const int kk = k0 + lane;
        float s = -INFINITY;
        if (kk < T) {
            const u32x4* kp = reinterpret_cast<const u32x4*>(base + (long)kk * kv_pitch);
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float kf[8];
                unpack8(kp[c], kf);
#pragma unroll
                for (int t = 0; t < 8; ++t) d += qf[c * 8 + t] * kf[t];
            }
            s = d * scale;
        }
        const float mc = wave_max(s);                      // (lane 0 of every chunk holds a live key: mc is finite unless a score is)
        const float mn = fmaxf(m, mc);
        const float corr = __expf(m - mn);                 // m = -inf on the first chunk: exp(-inf) = 0
        const float p = kk < T ? __expf(s - mn) : 0.f;
        l = l * corr + wave_sum(p);
        acc *= corr;
        m = mn;
        const int cnt = min(64, T - k0);
        const bf16_t* vbase = base + D + lane;
        for (int k = 0; k < cnt; ++k) {
            const float pk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), k));
            acc += pk * bf2f(vbase[(long)(k0 + k) * kv_pitch]);
        }
    }
    *out = l > 0.f ? f2bf(acc / l) : (bf16_t)0;
}

extern "C" {

// elements per stage-1 workgroup: the shortest slice whose candidates (slices * beam) one merge workgroup can rank; 0: none does
static int beam_slice_len(int V, int beam, int max_rows) {
    const long N = (long)max_rows * V;
    for (int SL = 1024; SL <= BS_CAND; SL *= 2)
        if ((N + SL - 1) / SL * beam <= BS_CAND) return SL;
    return 0;
}

/* slices per clip of svsr_beam_select for clips of at most max_rows rows (cand holds C * slices * beam 64-bit words); 0: unsupported */
int svsr_beam_select_slices(int V, int beam, int max_rows) {
    if (V < 1 || beam < 1 || beam > BS_CAND / 16 || max_rows < 1 || (long)max_rows * V > (long)BS_IDX_MASK + 1) return 0;
    const int SL = beam_slice_len(V, beam, max_rows);
    return SL == 0 ? 0 : (int)(((long)max_rows * V + SL - 1) / SL);
}

int svsr_beam_select(const float* s0, const float* s1, const float* s2, const float* s3, float w0, float w1, float w2, float w3, int nplanes,
                     int64_t ldv, const float* run, const int* clip_of, const int* row_lo, const int* out_off, int n, int C, int V, int beam,
                     int max_rows, int out_rows, void* cand, int64_t* prev, int64_t* tok, float* total, float* vals, int* clip_out, int* count,
                     hipStream_t stream) {
    if (nplanes < 1 || nplanes > BS_MAX_PLANES || n < 1 || C < 1 || V < 1 || ldv < V || beam < 1 || beam > BS_CAND / 16 || max_rows < 1 ||
        max_rows > n || out_rows < 1)
        return SVSR_ERR_ARG;
    if ((long)max_rows * V > (long)BS_IDX_MASK + 1) return SVSR_ERR_ARG;        // the flat index of a clip's element has BS_IDX_BITS bits
    const int SL = beam_slice_len(V, beam, max_rows);
    if (SL == 0) return SVSR_ERR_ARG;                                           // slices * beam candidates must fit one merge workgroup
    const int G = svsr_beam_select_slices(V, beam, max_rows);
    const float* s[BS_MAX_PLANES] = {s0, s1, s2, s3};
    const float w[BS_MAX_PLANES] = {w0, w1, w2, w3};
    BeamPlanes p;
    p.n = nplanes;
    for (int i = 0; i < BS_MAX_PLANES; ++i) {
        if (i < nplanes && s[i] == nullptr) return SVSR_ERR_ARG;
        p.s[i] = i < nplanes ? s[i] : nullptr;
        p.w[i] = i < nplanes ? w[i] : 0.f;
    }
    if (C > 65535) return SVSR_ERR_ARG;
    hipLaunchKernelGGL(k_beam_select_slices, dim3(G, C), dim3(BS_THREADS), 0, stream, p, run, row_lo, (long)ldv, V, beam, SL, n,
                       (unsigned long long*)cand);
    hipLaunchKernelGGL(k_beam_select_merge, dim3(C), dim3(BS_THREADS), 0, stream, p, run, clip_of, row_lo, out_off, (long)ldv, V, beam, SL, G, n,
                       out_rows, (const unsigned long long*)cand, (long*)prev, (long*)tok, total, vals, clip_out, count);
    return svsr_check_launch();
}

// one thread per (hypothesis, candidate), no grid-stride loop in the kernel: the grid covers every pair (full-vocabulary scoring at a
// wide beam exceeds a capped grid)
static int ctc_prefix_launch(const float* logp, int ldp, const float* r_prev, const int64_t* last, const int64_t* ids, const int* clip_of,
                             const int* tlen, float* r_new, float* psi, int C, int Tmax, int V, int n, int S, int out_len, int blank, int eos,
                             hipStream_t stream) {
    if (((long)n * S + 255) / 256 > 0x7fffffffL) return SVSR_ERR_ARG;
    hipLaunchKernelGGL(k_ctc_prefix_score_clips, dim3((unsigned)(((long)n * S + 255) / 256)), dim3(256), 0, stream, logp, r_prev, (const long*)last,
                       (const long*)ids, clip_of, tlen, r_new, psi, C, Tmax, V, ldp, n, S, out_len, blank, eos);
    return svsr_check_launch();
}

int svsr_ctc_prefix_score_clips(const float* logp, int ldp, const float* r_prev, const int64_t* last, const int64_t* ids, const int* clip_of,
                                const int* tlen, float* r_new, float* psi, int C, int Tmax, int V, int n, int S, int out_len, int blank, int eos,
                                hipStream_t stream) {
    if (C < 1 || Tmax < 1 || V < 2 || n < 1 || S < 1 || (ids == nullptr && S != V) || ldp < V || out_len < 0 || blank < 0 || blank >= V || eos < 0 ||
        eos >= V || clip_of == nullptr || tlen == nullptr)
        return SVSR_ERR_ARG;
    return ctc_prefix_launch(logp, ldp, r_prev, last, ids, clip_of, tlen, r_new, psi, C, Tmax, V, n, S, out_len, blank, eos, stream);
}

// one clip of T frames: the same kernel with every hypothesis in clip 0 and no length table
int svsr_ctc_prefix_score(const float* logp, int ldp, const float* r_prev, const int64_t* last, const int64_t* ids, float* r_new, float* psi, int T,
                          int V, int n, int S, int out_len, int blank, int eos, hipStream_t stream) {
    if (T < 1 || V < 2 || n < 1 || S < 1 || (ids == nullptr && S != V) || ldp < V || out_len < 0 || blank < 0 || blank >= V || eos < 0 || eos >= V)
        return SVSR_ERR_ARG;
    return ctc_prefix_launch(logp, ldp, r_prev, last, ids, nullptr, nullptr, r_new, psi, 1, T, V, n, S, out_len, blank, eos, stream);
}

// one workgroup per clip; dynamic LDS: prev | cur | ext rows of 2 Lmax + 1 words and the state of every frame (16 bits)
int svsr_ctc_align(const float* logp, int ldp, const int* tlen, const int64_t* labels, int Lmax, int B, int Tmax, int V, int blank, unsigned char* bp,
                   int* frames, int* spans, float* score, hipStream_t stream) {
    if (B < 1 || Tmax < 1 || Lmax < 1 || V < 2 || ldp < V || blank < 0 || blank >= V || logp == nullptr || tlen == nullptr || labels == nullptr ||
        bp == nullptr || frames == nullptr || spans == nullptr || score == nullptr)
        return SVSR_ERR_ARG;
    if (2L * Lmax + 1 > CA_MAX_S) return SVSR_ERR_ARG;                          // CA_PER states per thread
    const size_t lds = (size_t)3 * (2 * Lmax + 1) * sizeof(float) + (((size_t)Tmax * 2 + 3) & ~(size_t)3);
    if (lds > CA_MAX_LDS) return SVSR_ERR_ARG;
    hipLaunchKernelGGL(k_ctc_align, dim3(B), dim3(CA_THREADS), lds, stream, logp, ldp, tlen, (const long*)labels, Lmax, Tmax, V, blank, bp, frames, spans,
                       score);
    return svsr_check_launch();
}

// one wave per row; 16-byte loads when every row starts on a 16-byte boundary
int svsr_ctc_frame_best(const float* logits, int64_t ldp, const int* tlen, int C, int Tmax, int V, int* best, float* best_logp, hipStream_t stream) {
    if (C < 1 || Tmax < 1 || V < 1 || ldp < (int64_t)V || logits == nullptr || tlen == nullptr || best == nullptr || best_logp == nullptr)
        return SVSR_ERR_ARG;
    const long rows = (long)C * Tmax;
    if (rows > 0x7fffffffL) return SVSR_ERR_ARG;
    const int vec = ((uintptr_t)logits & 15) == 0 && ldp % 4 == 0;
    hipLaunchKernelGGL(k_ctc_frame_best, dim3((unsigned)rows), dim3(64), 0, stream, logits, (long)ldp, tlen, Tmax, V, vec, best, best_logp);
    return svsr_check_launch();
}

// one workgroup per clip; dynamic LDS: the clip's winners and log-probabilities, 8 Tmax + 16 bytes
int svsr_ctc_collapse(const int* best, const float* best_logp, const int* tlen, int C, int Tmax, int Lcap, int blank, int64_t* tokens, int* spans,
                      float* token_logp, int* ntok, float* score, hipStream_t stream) {
    if (C < 1 || Tmax < 1 || Tmax > CG_MAX_T || Lcap < 1 || best == nullptr || best_logp == nullptr || tlen == nullptr || tokens == nullptr ||
        spans == nullptr || token_logp == nullptr || ntok == nullptr || score == nullptr)
        return SVSR_ERR_ARG;
    const size_t lds = (size_t)2 * Tmax * sizeof(float) + 4 * sizeof(int);
    hipLaunchKernelGGL(k_ctc_collapse, dim3(C), dim3(CG_THREADS), lds, stream, best, best_logp, tlen, Tmax, Lcap, blank, (long*)tokens, spans,
                       token_logp, ntok, score);
    return svsr_check_launch();
}

int svsr_mha_src_step_fwd(const void* q, int64_t q_pitch, const void* kv, int64_t kv_pitch, const int* clip_of, const int* tlen, int C, int Tmax, int n,
                          int H, float scale, void* ctx, int64_t ctx_pitch, hipStream_t stream) {
    if (C < 1 || Tmax < 1 || n < 1 || H < 1 || clip_of == nullptr || tlen == nullptr) return SVSR_ERR_ARG;
    if (q_pitch < (int64_t)H * 64 || q_pitch % 8 != 0 || kv_pitch < 2L * H * 64 || kv_pitch % 8 != 0 || ctx_pitch < (int64_t)H * 64) return SVSR_ERR_ARG;
    if ((((uintptr_t)q | (uintptr_t)kv) & 15) != 0) return SVSR_ERR_ARG;       // 16-byte loads of 64-channel head slices
    const long waves = (long)n * H;
    if (waves > (1L << 30)) return SVSR_ERR_ARG;
    hipLaunchKernelGGL(k_mha_src_step, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, (const bf16_t*)q, (long)q_pitch, (const bf16_t*)kv,
                       (long)kv_pitch, clip_of, tlen, C, Tmax, n, H, scale, (bf16_t*)ctx, (long)ctx_pitch);
    return svsr_check_launch();
}

}  // extern "C"
