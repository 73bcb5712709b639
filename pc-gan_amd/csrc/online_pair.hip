// End of the Elo encoder's online-pair-selection trainer (siamese_online.py): order the batch's pairs by squared rating distance, keep
// the k hardest (or easiest), draw-aware binary cross entropy on the kept ones, the rating regularizer, the gradient of both, the
// pseudo-label candidates from the other end of the order and the 0 / 1 / 2 prediction of every pair, ONE launch.
//
// Replaces, in the reference,
//   EmbeddingDistancePairSelector.get_pairs: three .cpu() copies, numpy argsort, LongTensor, .cuda()       siamese_online.py:218-265
//   OnlineBinaryCrossEntropyLoss.__call__: LUT[label], two index ops, two logsigmoid, mean                   siamese_online.py:324-342
//   get_prediction: sigmoid, the draw band, the compares                                                     siamese_online.py:385-394
//   reg1 = feat1.pow(2).mean(); reg2 = ...; this_loss = (reg1 + reg2) * lambda_regularization                siamese_online.py:630-635
// and the backward pass of all of it.
//
// LABEL CONVENTION: target = (1, 0.5, 0)[label], i.e. label 0 means "the first image rates HIGHER".  That is the reverse of siamese.py's
// BinaryNLLLoss (0, 0.5, 1); it is what the reference's online script does (LUT = [1, 0.5, 0], :329).
//
// Geometry: ONE workgroup (the batch is at most 4096 pairs; the bound is latency, not bytes: 4096 pairs are 64 KB in and 48 KB out).
// Lane t owns the pairs t, t + 1024, ... (Q = ceil(N / 1024) of them, in registers); for N <= 1024 the workgroup has N rounded up to whole
// waves.  No workspace, no atomics, every order fixed: two calls give the same bits.
//   1. key[n] = s * s with s = f1 - f2 (fp32, one rounding each: the unit is built with -ffp-contract=off, so these are the bits of the
//      reference's (A - B).pow(2)), or the caller's key.  The key becomes an unsigned word whose integer order is numpy's sort order:
//      -0 counts as +0, negative values below positive ones, every NaN after +inf.
//   2. the position of every pair in the stable ascending order (equal words: the lower index first): a bitonic network in LDS over
//      the 64-bit entries (word << 32 | index) -- all different, so the network's result IS the stable order -- padded with all-ones
//      entries to P, the power of two >= N; each entry's final place is then written to its pair's slot.  (Why not rank by counting, every
//      lane reading all N words: N compares per lane with N / 256 waves on a SIMD; the call measured 42.5 us at N = 1024 and 553 us at
//      4096 that way, 21.7 and 71.7 us with the network, and below 256 pairs both hide behind the host's time to issue a launch.)
//      descending: position = N - 1 - rank, the exact reverse of the ascending list, so ties then go to the higher index.
//      sel = positions [0, k), pseudo = positions [N - k, N): each lane writes its own pair's index where its position says.
//   3. per pair in float64: p = sigmoid(s), the term -(t logsigmoid(s) + (1 - t) logsigmoid(-s)) with logsigmoid(x) = min(x, 0) -
//      log1p(exp(-|x|)), p - t (for t = 1 as -sigmoid(-s): no cancellation), the gradients, the prediction.  The three sums (terms of sel,
//      f1^2, f2^2) are added by ONE lane in ascending pair index, 1024 pairs at a time through LDS (a term outside sel is +0: adding it
//      changes nothing; eight loads in flight ahead of the dependent additions), and rounded to fp32 once.
#include <math.h>
#include "common.h"

namespace pcgan {

static constexpr int OP_MAX_N = 4096;
static constexpr int OP_THREADS = 1024;
static constexpr unsigned OP_NAN_WORD = 0xfffffffeu;      // every NaN key: after +inf, before the padding word
static constexpr unsigned OP_PAD_WORD = 0xffffffffu;      // fills the sort buffer past N: after every pair

struct OnlinePairArgs {
    const float* f1;
    const float* f2;
    const int64_t* label;
    const float* key;
    float* loss;
    float* df1;
    float* df2;
    int32_t* picks;
    int N, k, descending, P;                     // P: entries of the sorting network
    double draw_thresh, lambda_reg, gscale;      // the caller's fp32 values, widened exactly
};

// fp32 key -> unsigned word, ascending in numpy's order
__device__ __forceinline__ unsigned op_key_word(float key) {
    if (key != key) return OP_NAN_WORD;
    if (key == 0.f) key = 0.f;                            // -0 and +0 are one key
    const unsigned u = __float_as_uint(key);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);    // +inf -> 0xff800000 < OP_NAN_WORD
}

__device__ __forceinline__ double op_logsigmoid(double x) { return fmin(x, 0.0) - log1p(exp(-fabs(x))); }

// sum += v[0] + v[1] + ... in index order; SQUARE: of the squares (exact products of widened fp32 values)
template <typename T, bool SQUARE> __device__ __forceinline__ void op_add_in_order(const T* v, int n, double& sum) {
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        double r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = (double)v[i + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += SQUARE ? r[u] * r[u] : r[u];
    }
    for (; i < n; ++i) {
        const double r = (double)v[i];
        sum += SQUARE ? r * r : r;
    }
}

// Q: pairs per lane.  The sorting network has P entries, the power of two >= N (at least 2): fixed by Q above 1024 pairs
template <int Q>
__global__ void __launch_bounds__(OP_THREADS) online_pair_kernel(const OnlinePairArgs a) {
    // the sort buffer; afterwards the staging of the three sums (16 KB)
    __shared__ __attribute__((aligned(16))) unsigned long long buf[Q > 2 ? 4 * OP_THREADS : 2 * OP_THREADS];
    __shared__ unsigned place[Q * OP_THREADS];           // the position of every pair
    double* term_s = reinterpret_cast<double*>(buf);
    float* f1_s = reinterpret_cast<float*>(buf + OP_THREADS);
    float* f2_s = f1_s + OP_THREADS;
    const int tid = threadIdx.x, N = a.N, k = a.k, nt = blockDim.x;
    const int P = Q > 2 ? 4 * OP_THREADS : (Q == 2 ? 2 * OP_THREADS : a.P);

    float x1[Q], x2[Q], s[Q];
    unsigned w[Q];
    int lab[Q], rank[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int n = q * OP_THREADS + tid;
        x1[q] = x2[q] = s[q] = 0.f;
        w[q] = OP_PAD_WORD;
        lab[q] = 1;
        rank[q] = 0;
        if (n < N) {
            x1[q] = a.f1[n];
            x2[q] = a.f2[n];
            s[q] = x1[q] - x2[q];
            w[q] = op_key_word(a.key ? a.key[n] : s[q] * s[q]);
            const int64_t l = a.label[n];
            lab[q] = l < 0 ? 0 : (l > 2 ? 2 : (int)l);   // clamped: the target table is never read out of bounds
        }
    }

#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int n = q * OP_THREADS + tid;               // w is the padding word past N: (pad << 32 | n) sorts after every pair
        buf[n] = ((unsigned long long)w[q] << 32) | (unsigned)n;
    }
    for (int n = Q * nt + tid; n < P; n += nt) buf[n] = ~0ull;      // (Q > 1: nt = OP_THREADS; Q = 1: the lanes wrote [0, nt))
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < P / 2; t += nt) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;          // lo: t with a zero inserted at the stride's bit
                const unsigned long long u = buf[lo], v = buf[hi];
                if ((u > v) == ((lo & size) == 0)) {                                   // ascending where the size bit is clear
                    buf[lo] = v;
                    buf[hi] = u;
                }
            }
        }
    }
    __syncthreads();
    for (int p = tid; p < N; p += nt) place[(unsigned)buf[p]] = (unsigned)p;          // the N pairs are the first N entries
    __syncthreads();                                                                   // ... and buf is free for the sums
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int n = q * OP_THREADS + tid;
        if (n < N) rank[q] = (int)place[n];
    }

    const double inv_k = 1.0 / (double)k;                 // only in the gradient; the loss divides its sum by k
    double lsum = 0.0, q1sum = 0.0, q2sum = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int n = q * OP_THREADS + tid;
        double term = 0.0;
        if (n < N) {
            const int pos = a.descending ? N - 1 - rank[q] : rank[q];
            const bool kept = pos < k;
            if (a.picks) {
                if (kept) a.picks[pos] = n;
                if (pos >= N - k) a.picks[k + pos - (N - k)] = n;
            }
            const double sd = (double)s[q];
            const double t = lab[q] == 0 ? 1.0 : (lab[q] == 1 ? 0.5 : 0.0);
            const double e = exp(-fabs(sd));
            const double p = sd >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
            const double np1 = sd >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);      // 1 - p = sigmoid(-s) without the cancellation
            const double pt = lab[q] == 0 ? -np1 : (lab[q] == 1 ? p - 0.5 : p);   // p - t
            if (kept) term = -(t * op_logsigmoid(sd) + (1.0 - t) * op_logsigmoid(-sd));
            if (a.picks) a.picks[2 * k + n] = fabs(0.5 - p) < a.draw_thresh ? 1 : (p > 0.5 ? 0 : 2);
            if (a.df1 || a.df2) {
                const double g = kept ? pt * inv_k : 0.0;
                const double r = a.lambda_reg * 2.0 / (double)N;
                if (a.df1) a.df1[n] = (float)(a.gscale * (g + r * (double)x1[q]));
                if (a.df2) a.df2[n] = (float)(a.gscale * (-g + r * (double)x2[q]));
            }
        }
        if (a.loss) {                                     // uniform: the barriers below are reached by every lane
            term_s[tid] = term;
            f1_s[tid] = x1[q];
            f2_s[tid] = x2[q];
            __syncthreads();
            if (tid == 0) {
                const int cn = N - q * OP_THREADS < nt ? N - q * OP_THREADS : nt;
                op_add_in_order<double, false>(term_s, cn, lsum);
                if (a.lambda_reg != 0.0) {
                    op_add_in_order<float, true>(f1_s, cn, q1sum);
                    op_add_in_order<float, true>(f2_s, cn, q2sum);
                }
            }
            if (q + 1 < Q) __syncthreads();
        }
    }
    if (a.loss && tid == 0) {
        const double l0 = lsum / (double)k;
        const double l1 = a.lambda_reg != 0.0 ? a.lambda_reg * (q1sum / (double)N + q2sum / (double)N) : 0.0;
        a.loss[0] = (float)l0;
        a.loss[1] = (float)l1;
        a.loss[2] = (float)(l0 + l1);
    }
}

}  // namespace pcgan

using namespace pcgan;

extern "C" int pcgan_online_pair_bce(const float* f1, const float* f2, const int64_t* label, const float* key, float* loss, float* df1,
                                     float* df2, int32_t* picks, int N, int k, int descending, float draw_thresh, float lambda_reg,
                                     float gscale, pcgan_stream_t s) {
    PCGAN_CHECK(N >= 1 && N <= OP_MAX_N, "online_pair_bce: N %d outside 1 <= N <= %d", N, OP_MAX_N);
    PCGAN_CHECK(k >= 1 && k <= N, "online_pair_bce: k %d outside 1 <= k <= N = %d", k, N);
    PCGAN_CHECK(f1 && f2 && label, "online_pair_bce: null f1 / f2 / label");
    OnlinePairArgs a;
    a.f1 = f1; a.f2 = f2; a.label = label; a.key = key; a.loss = loss; a.df1 = df1; a.df2 = df2; a.picks = picks;
    a.N = N; a.k = k; a.descending = descending ? 1 : 0;
    a.draw_thresh = (double)draw_thresh; a.lambda_reg = (double)lambda_reg; a.gscale = (double)gscale;
    const int Q = (N + OP_THREADS - 1) / OP_THREADS;
    const int threads = Q > 1 ? OP_THREADS : (N + 63) / 64 * 64;
    hipStream_t st = (hipStream_t)s;
    a.P = 2;
    while (a.P < N) a.P <<= 1;
    switch (Q) {
        case 1: hipLaunchKernelGGL(online_pair_kernel<1>, dim3(1), dim3(threads), 0, st, a); break;
        case 2: hipLaunchKernelGGL(online_pair_kernel<2>, dim3(1), dim3(threads), 0, st, a); break;
        case 3: hipLaunchKernelGGL(online_pair_kernel<3>, dim3(1), dim3(threads), 0, st, a); break;
        default: hipLaunchKernelGGL(online_pair_kernel<4>, dim3(1), dim3(threads), 0, st, a); break;
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}
