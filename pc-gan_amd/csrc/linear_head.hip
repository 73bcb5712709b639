// Training pass of the attribute classifier's head: nn.Linear(C -> K) + CrossEntropyLoss(weight), forward and backward.
//
// Replaces, in the reference,
//   output = net.forward(img0); loss = criterion(output, label); get_prediction(output)     classification.py:330-332, 376-384
//   self.model(x) -> ... -> self.fc(x)                                                        models/networks.py:1284-1285
//   loss.backward() through the fc layer                                                      classification.py:383
//
// Small, latency-bound launches (batch 100: 100 x 512 x K, K = 2 .. 10): one workgroup per batch row (forward, dx) or per class (dw, db),
// 128-bit loads along c, wave64 shuffle reductions; the matrix pipe is not used.  Every sum runs in a fixed order in float64 (the sizes
// are tiny: the launches are bound by latency, not by arithmetic) and is rounded to fp32 once, so results are bit-identical from run to run and carry one
// rounding against exact arithmetic.  No float atomics.  The two batch-wide scalars of the forward pass (loss, correct) are finished by
// the LAST ARRIVING workgroup of the same launch, which sums the row partials in index order (common.h, "cross-workgroup finish").
#include "common.h"

namespace pcgan {

static constexpr int LH_THREADS = 256;
static constexpr int LH_WAVES = LH_THREADS / 64;
static constexpr int LH_MAX_N = 512, LH_MAX_C = 2048, LH_MAX_K = 1024;

// four consecutive floats: one 16-byte access when the tensor allows it (vec), else four 4-byte ones
__device__ __forceinline__ float4 lh_ld4(const float* p, int vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void lh_st4(float* p, const float4& v, int vec) {
    if (vec) {
        *reinterpret_cast<float4*>(p) = v;
    } else {
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}

// workspace layout (doubles): [0] the ticket word (an unsigned in the first 4 bytes), [1 .. N] weighted row losses, [N + 1 .. 2 N] row hits
struct LinearCeArgs {
    const float *x, *w, *b, *wt;
    const long long* y;
    float *logits, *dlogits, *loss;
    long long* pred;
    int* correct;
    double* ws;
    int N, C, K, vec;
};

__global__ void __launch_bounds__(LH_THREADS) linear_ce_fwd_kernel(const LinearCeArgs a) {
    __shared__ float xs[LH_MAX_C];
    __shared__ double lg[LH_MAX_K];
    __shared__ double scratch[LH_WAVES];
    __shared__ double bmax;
    __shared__ int barg;
    __shared__ int last_flag;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, K = a.K, C4 = C >> 2;

    // the denominator of the mean reduction, sum_n wt[y_n], in row order: every workgroup computes the same value
    double wpart = 0.0;
    for (int i = tid; i < a.N; i += LH_THREADS) {
        const long long yi = a.y[i];
        if (yi >= 0 && yi < K) wpart += a.wt ? (double)a.wt[yi] : 1.0;
    }
    const double wsum = block_sum_d<LH_WAVES>(wpart, scratch);

    const float* xr = a.x + (size_t)n * C;
    for (int i = tid; i < C4; i += LH_THREADS) {
        const float4 v = lh_ld4(xr + 4 * i, a.vec);
        xs[4 * i + 0] = v.x; xs[4 * i + 1] = v.y; xs[4 * i + 2] = v.z; xs[4 * i + 3] = v.w;
    }
    __syncthreads();
    // one wave per class: lanes stride over c, float64 partial sums, xor-shuffle tree
    for (int k = wave; k < K; k += LH_WAVES) {
        const float* wr = a.w + (size_t)k * C;
        double s = 0.0;
        for (int i = lane; i < C4; i += 64) {
            const float4 v = lh_ld4(wr + 4 * i, a.vec);
            s += (double)xs[4 * i + 0] * (double)v.x;
            s += (double)xs[4 * i + 1] * (double)v.y;
            s += (double)xs[4 * i + 2] * (double)v.z;
            s += (double)xs[4 * i + 3] * (double)v.w;
        }
        s = wave_sum_d(s);
        if (lane == 0) lg[k] = s + (a.b ? (double)a.b[k] : 0.0);
    }
    __syncthreads();
    // the prediction is the first maximum of the fp32 logits the caller sees (numpy.argmax on `output`)
    if (wave == 0) {
        float m = -INFINITY;
        int mi = 0x7fffffff;
        for (int k = lane; k < K; k += 64) {
            const float v = (float)lg[k];
            if (v > m || mi == 0x7fffffff) { m = v; mi = k; }       // k ascends within a lane: a later equal value does not replace
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(m, o, 64);
            const int oi = __shfl_xor(mi, o, 64);
            if (oi != 0x7fffffff && (mi == 0x7fffffff || om > m || (om == m && oi < mi))) { m = om; mi = oi; }
        }
        if (lane == 0) {
            barg = mi;
            bmax = lg[mi];
        }
    }
    __syncthreads();
    const double mx = bmax;
    double epart = 0.0;
    for (int k = tid; k < K; k += LH_THREADS) epart += exp(lg[k] - mx);
    const double esum = block_sum_d<LH_WAVES>(epart, scratch);
    const long long yn = a.y[n];
    const bool valid = yn >= 0 && yn < K;          // a label outside [0, K) is an ignored row: weight 0, no table look-up
    const double wy = valid ? (a.wt ? (double)a.wt[yn] : 1.0) : 0.0;
    const double gscale = wy / wsum;
    float* lrow = a.logits ? a.logits + (size_t)n * K : nullptr;
    float* drow = a.dlogits ? a.dlogits + (size_t)n * K : nullptr;
    for (int k = tid; k < K; k += LH_THREADS) {
        if (lrow) lrow[k] = (float)lg[k];
        if (drow) drow[k] = (float)(gscale * (exp(lg[k] - mx) / esum - ((long long)k == yn ? 1.0 : 0.0)));
    }
    if (tid == 0) {
        const double row_loss = valid ? wy * (log(esum) - (lg[yn] - mx)) : 0.0;
        if (a.pred) a.pred[n] = barg;
        st_wt(a.ws + 1 + n, row_loss);
        st_wt(a.ws + 1 + a.N + n, (valid && (long long)barg == yn) ? 1.0 : 0.0);
        last_flag = ticket_arrive(reinterpret_cast<unsigned*>(a.ws), 0, (unsigned)a.N);
    }
    __syncthreads();
    if (!last_flag) return;
    double lpart = 0.0, hpart = 0.0;
    for (int i = tid; i < a.N; i += LH_THREADS) {
        lpart += ld_wt(a.ws + 1 + i);
        hpart += ld_wt(a.ws + 1 + a.N + i);
    }
    const double lsum = block_sum_d<LH_WAVES>(lpart, scratch);
    const double hsum = block_sum_d<LH_WAVES>(hpart, scratch);
    if (tid == 0) {
        if (a.loss) a.loss[0] = (float)(lsum / wsum);
        if (a.correct) a.correct[0] = (int)hsum;
    }
}

struct LinearBwdArgs {
    const float *dl, *x, *w;
    float *dx, *dw, *db;
    int N, C, K, accumulate, vec, dx_blocks;
};

// workgroups [0, dx_blocks): dx of one row; the rest: dw and db of one class.  A thread owns 4 consecutive c (twice for C > 1024).
__global__ void __launch_bounds__(LH_THREADS) linear_bwd_kernel(const LinearBwdArgs a) {
    __shared__ float col[LH_MAX_K > LH_MAX_N ? LH_MAX_K : LH_MAX_N];
    const int tid = threadIdx.x, C = a.C, K = a.K, N = a.N, C4 = C >> 2;
    if ((int)blockIdx.x < a.dx_blocks) {
        const int n = blockIdx.x;
        for (int k = tid; k < K; k += LH_THREADS) col[k] = a.dl[(size_t)n * K + k];
        __syncthreads();
        for (int i = tid; i < C4; i += LH_THREADS) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int k = 0; k < K; ++k) {
                const float4 v = lh_ld4(a.w + (size_t)k * C + 4 * i, a.vec);
                const double d = (double)col[k];
                s0 += d * (double)v.x; s1 += d * (double)v.y; s2 += d * (double)v.z; s3 += d * (double)v.w;
            }
            lh_st4(a.dx + (size_t)n * C + 4 * i, make_float4((float)s0, (float)s1, (float)s2, (float)s3), a.vec);
        }
        return;
    }
    const int k = blockIdx.x - a.dx_blocks;
    for (int n = tid; n < N; n += LH_THREADS) col[n] = a.dl[(size_t)n * K + k];
    __syncthreads();
    if (a.dw) {
        for (int i = tid; i < C4; i += LH_THREADS) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int n = 0; n < N; ++n) {
                const float4 v = lh_ld4(a.x + (size_t)n * C + 4 * i, a.vec);
                const double d = (double)col[n];
                s0 += d * (double)v.x; s1 += d * (double)v.y; s2 += d * (double)v.z; s3 += d * (double)v.w;
            }
            float* o = a.dw + (size_t)k * C + 4 * i;
            if (a.accumulate) {
                const float4 p = lh_ld4(o, a.vec);
                s0 += (double)p.x; s1 += (double)p.y; s2 += (double)p.z; s3 += (double)p.w;
            }
            lh_st4(o, make_float4((float)s0, (float)s1, (float)s2, (float)s3), a.vec);
        }
    }
    if (a.db && tid < 64) {
        double s = 0.0;
        for (int n = tid; n < N; n += 64) s += (double)col[n];
        s = wave_sum_d(s);
        if (tid == 0) a.db[k] = (float)(a.accumulate ? s + (double)a.db[k] : s);
    }
}

static bool head_sizes_ok(const char* what, int N, int C, int K, int dtype) {
    if (dtype != PCGAN_F32) {
        set_error("%s: fp32 tensors only (dtype %d)", what, dtype);
        return false;
    }
    if (N < 1 || N > LH_MAX_N || C < 4 || C > LH_MAX_C || (C & 3) != 0 || K < 1 || K > LH_MAX_K) {
        set_error("%s: N %d C %d K %d outside 1 <= N <= %d, C a multiple of 4 in [4, %d], 1 <= K <= %d", what, N, C, K, LH_MAX_N, LH_MAX_C,
                  LH_MAX_K);
        return false;
    }
    return true;
}

}  // namespace pcgan

using namespace pcgan;

extern "C" size_t pcgan_linear_ce_workspace_bytes(int N) { return N > 0 && N <= LH_MAX_N ? (size_t)(1 + 2 * N) * sizeof(double) : 0; }

extern "C" int pcgan_linear_ce_fwd(const void* x, const float* w, const float* b, const int64_t* labels, const float* class_weight,
                                   void* logits, void* dlogits, float* loss, int64_t* pred, int32_t* correct, void* workspace,
                                   size_t workspace_bytes, int N, int C, int K, int dtype, pcgan_stream_t s) {
    if (!head_sizes_ok("linear_ce_fwd", N, C, K, dtype)) return 1;
    PCGAN_CHECK(x && w && labels, "linear_ce_fwd: null x / w / labels");
    PCGAN_CHECK(workspace && workspace_bytes >= pcgan_linear_ce_workspace_bytes(N), "linear_ce_fwd: workspace of %zu bytes, need %zu",
                workspace_bytes, pcgan_linear_ce_workspace_bytes(N));
    PCGAN_CHECK((reinterpret_cast<size_t>(workspace) & 7) == 0, "linear_ce_fwd: the workspace must be 8-byte aligned");
    LinearCeArgs a;
    a.x = (const float*)x; a.w = w; a.b = b; a.wt = class_weight;
    a.y = (const long long*)labels;
    a.logits = (float*)logits; a.dlogits = (float*)dlogits; a.loss = loss;
    a.pred = (long long*)pred;
    a.correct = correct;
    a.ws = (double*)workspace;
    a.N = N; a.C = C; a.K = K;
    a.vec = ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(w)) & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(linear_ce_fwd_kernel, dim3(N), dim3(LH_THREADS), 0, (hipStream_t)s, a);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcgan_linear_bwd(const void* dlogits, const void* x, const float* w, void* dx, float* dw, float* db, int N, int C, int K,
                                int accumulate, int dtype, pcgan_stream_t s) {
    if (!head_sizes_ok("linear_bwd", N, C, K, dtype)) return 1;
    PCGAN_CHECK(dlogits, "linear_bwd: null dlogits");
    PCGAN_CHECK(dx || dw || db, "linear_bwd: nothing to compute (dx, dw and db are all NULL)");
    PCGAN_CHECK(!dx || w, "linear_bwd: dx needs w");
    PCGAN_CHECK(!dw || x, "linear_bwd: dw needs x");
    LinearBwdArgs a;
    a.dl = (const float*)dlogits; a.x = (const float*)x; a.w = w;
    a.dx = (float*)dx; a.dw = dw; a.db = db;
    a.N = N; a.C = C; a.K = K;
    a.accumulate = accumulate ? 1 : 0;
    const size_t addr = reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(w) | reinterpret_cast<size_t>(dx) | reinterpret_cast<size_t>(dw);
    a.vec = (addr & 15) == 0 ? 1 : 0;
    a.dx_blocks = dx ? N : 0;
    const int blocks = a.dx_blocks + ((dw || db) ? K : 0);
    hipLaunchKernelGGL(linear_bwd_kernel, dim3(blocks), dim3(LH_THREADS), 0, (hipStream_t)s, a);
    PCGAN_LAUNCH_CHECK();
    return 0;
}
