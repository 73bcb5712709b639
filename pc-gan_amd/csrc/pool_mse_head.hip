// End of the attribute regressor: global pooling + nn.MSELoss + "within delta" accuracy + the gradient of the loss, ONE launch.
//
// Replaces, in the reference,
//   output = net.forward(img0); loss = criterion(output, label); get_accuracy(output, label, opt.delta)      regression.py:359-363
//   nn.AvgPool2d(output.size(2))(output) / nn.MaxPool2d(output.size(2))(output)                              models/networks.py:1115-1118
//   loss.backward() through the loss and the pooling                                                         regression.py:365
//
// The planes the regressor pools are 9 .. 64 elements (3x3 .. 8x8 maps) and start element-aligned only, N F of them with N F from 1
// (validation, one image, cnn_dim [.., 1]) to ~50 000 (batch 100, 512 channels, no cnn_dim).  A wave per plane would leave most lanes
// idle, so for HW <= 64 a workgroup takes 128 CONSECUTIVE planes: their elements are one contiguous run (it starts on a multiple of 128
// elements, so 128-bit accesses work whenever the tensor's base allows them, whatever HW is), staged in LDS with coalesced loads; then
// ONE LANE PER PLANE walks its plane in LDS in index order (odd row stride: no bank conflicts), and all threads write the gradient
// back coalesced.  Longer planes (must be correct, need not be fast) take one workgroup per plane.
//
// Every sum runs in a fixed order in float64 and is rounded to fp32 once; no float atomics: results are bit-identical from run to run.
// The two batch-wide scalars (loss, hits) are finished by the LAST ARRIVING workgroup of the same launch, which sums the workgroup
// partials by index (common.h, "cross-workgroup finish").
#include <float.h>
#include "common.h"

namespace pcgan {

static constexpr int PM_THREADS = 256;
static constexpr int PM_WAVES = PM_THREADS / 64;
static constexpr int PM_PLANES = 128;          // planes per workgroup on the staged path (64: 17.6 us against 13.9 us at 51 200 planes)
static constexpr int PM_SHORT = 64;            // longest plane of the staged path
static constexpr int PM_LD1 = PM_PLANES * PM_SHORT / PM_THREADS, PM_LD4 = PM_LD1 / 4;      // loads per thread: elements, groups of four
static constexpr int PM_MAX_NF = 1 << 22, PM_MAX_HW = 1 << 20;

// workspace layout (doubles): [0] the ticket word (an unsigned in the first 4 bytes), [1 .. B] squared-error sums of the B workgroups,
// [B + 1 .. 2 B] their hit counts
struct PoolMseArgs {
    const void* x;
    const float* target;
    float* pred;
    int32_t* argmax;
    void* dx;
    float* loss;
    int32_t* hits;
    double* ws;
    int NF, HW, is_max, vec;
    float delta;
    double g2;          // 2 gscale
};

// what one plane contributes once its pooled value is known: pred / argmax stores, squared error, hit, and its gradient factor
__device__ __forceinline__ float pm_plane(const PoolMseArgs& a, int plane, float pr, int arg, double& sq, double& hit) {
    const float t = a.target[plane];
    const double d = (double)pr - (double)t;
    sq = d * d;
    hit = fabsf(pr - t) < a.delta ? 1.0 : 0.0;            // fp32, strict: torch.abs(pred - target) < delta on the returned pred
    if (a.pred) a.pred[plane] = pr;
    if (a.argmax && a.is_max) a.argmax[plane] = arg;
    const double den = a.is_max ? (double)a.NF : (double)a.NF * (double)a.HW;      // exact: NF HW < 2^53
    return (float)(a.g2 * d / den);
}

// partials out, ticket, and in the last workgroup the two scalars
__device__ __forceinline__ void pm_finish(const PoolMseArgs& a, double bsq, double bhit, double* scratch, int* last_flag) {
    const int tid = threadIdx.x, B = gridDim.x;
    if (tid == 0) {
        st_wt(a.ws + 1 + blockIdx.x, bsq);
        st_wt(a.ws + 1 + B + blockIdx.x, bhit);
        *last_flag = ticket_arrive(reinterpret_cast<unsigned*>(a.ws), 0, (unsigned)B);
    }
    __syncthreads();
    if (!*last_flag) return;
    double lpart = 0.0, hpart = 0.0;
    for (int i = tid; i < B; i += PM_THREADS) {
        lpart += ld_wt(a.ws + 1 + i);
        hpart += ld_wt(a.ws + 1 + B + i);
    }
    const double lsum = block_sum_d<PM_WAVES>(lpart, scratch);
    const double hsum = block_sum_d<PM_WAVES>(hpart, scratch);
    if (tid == 0) {
        if (a.loss) a.loss[0] = (float)(lsum / (double)a.NF);
        if (a.hits) a.hits[0] = (int)hsum;
    }
}

// HW <= PM_SHORT: workgroup b owns planes [128 b, 128 b + np)
template <typename T>
__global__ void __launch_bounds__(PM_THREADS) pool_mse_short_kernel(const PoolMseArgs a) {
    __shared__ float xs[PM_PLANES * (PM_SHORT + 1)];
    __shared__ float gs[PM_PLANES];
    __shared__ int as[PM_PLANES];
    __shared__ double scratch[PM_WAVES];
    __shared__ int last_flag;
    const int tid = threadIdx.x, HW = a.HW;
    const int p0 = blockIdx.x * PM_PLANES;
    const int np = a.NF - p0 < PM_PLANES ? a.NF - p0 : PM_PLANES;
    const int pad = (HW & 1) ^ 1, stride = HW + pad;           // odd row stride in LDS
    const int ne = np * HW;                                     // <= 128 * 64
    const size_t e0 = (size_t)p0 * HW;                          // a multiple of 128 elements
    const T* xb = (const T*)a.x + e0;
    const int n4 = a.vec ? (ne >> 2) : 0;

    // every global load of the thread is issued before the first LDS store: one round trip to memory, not one per iteration
    if (a.vec) {
        float4 v[PM_LD4];
#pragma unroll
        for (int r = 0; r < PM_LD4; ++r) {
            const int q = tid + r * PM_THREADS;
            if (q < n4) v[r] = ld4(xb + 4 * q);
        }
#pragma unroll
        for (int r = 0; r < PM_LD4; ++r) {
            const int q = tid + r * PM_THREADS;
            if (q < n4) {
                const float f[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
                int pl = (4 * q) / HW, i = 4 * q - pl * HW;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    xs[pl * stride + i] = f[j];
                    if (++i == HW) { i = 0; ++pl; }
                }
            }
        }
        for (int e = 4 * n4 + tid; e < ne; e += PM_THREADS) xs[pad ? e + e / HW : e] = ld1(xb + e);      // at most 3 elements
    } else {
        float v[PM_LD1];
#pragma unroll
        for (int r = 0; r < PM_LD1; ++r) {
            const int e = tid + r * PM_THREADS;
            if (e < ne) v[r] = ld1(xb + e);
        }
#pragma unroll
        for (int r = 0; r < PM_LD1; ++r) {
            const int e = tid + r * PM_THREADS;
            if (e < ne) xs[pad ? e + e / HW : e] = v[r];
        }
    }
    __syncthreads();

    double sq = 0.0, hit = 0.0;
    if (tid < np) {
        const float* xp = xs + tid * stride;
        float pr;
        int arg = 0;
        if (a.is_max) {
            pr = xp[0];
            for (int i = 1; i < HW; ++i) {
                const float v = xp[i];
                if (v > pr) { pr = v; arg = i; }                // strict: the FIRST maximum stays
            }
        } else {
            double s = 0.0;
            for (int i = 0; i < HW; ++i) s += (double)xp[i];
            pr = (float)(s / (double)HW);
        }
        gs[tid] = pm_plane(a, p0 + tid, pr, arg, sq, hit);
        as[tid] = arg;
    }
    __syncthreads();

    if (a.dx) {
        T* db = (T*)a.dx + e0;
        const int is_max = a.is_max;
        for (int q = tid; q < n4; q += PM_THREADS) {
            float f[4];
            int pl = (4 * q) / HW, i = 4 * q - pl * HW;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f[j] = (!is_max || i == as[pl]) ? gs[pl] : 0.f;
                if (++i == HW) { i = 0; ++pl; }
            }
            st4(db + 4 * q, make_float4(f[0], f[1], f[2], f[3]));
        }
        for (int e = 4 * n4 + tid; e < ne; e += PM_THREADS) {
            const int pl = e / HW, i = e - pl * HW;
            st1(db + e, (!is_max || i == as[pl]) ? gs[pl] : 0.f);
        }
    }
    const double bsq = block_sum_d<PM_WAVES>(sq, scratch);
    const double bhit = block_sum_d<PM_WAVES>(hit, scratch);
    pm_finish(a, bsq, bhit, scratch, &last_flag);
}

// HW > PM_SHORT: one workgroup per plane, threads stride over the plane
template <typename T>
__global__ void __launch_bounds__(PM_THREADS) pool_mse_long_kernel(const PoolMseArgs a) {
    __shared__ double scratch[PM_WAVES];
    __shared__ float wbest[PM_WAVES];
    __shared__ int warg[PM_WAVES];
    __shared__ float g_sh;
    __shared__ int arg_sh;
    __shared__ int last_flag;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, HW = a.HW;
    const int plane = blockIdx.x;
    const T* xp = (const T*)a.x + (size_t)plane * HW;
    float pr = 0.f;
    int arg = 0;
    if (a.is_max) {
        float m = -INFINITY;
        int mi = 0x7fffffff;                                    // no element seen yet
        for (int i = tid; i < HW; i += PM_THREADS) {
            const float v = ld1(xp + i);
            if (v > m || mi == 0x7fffffff) { m = v; mi = i; }   // i ascends within a thread: a later equal value does not replace
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(m, o, 64);
            const int oi = __shfl_xor(mi, o, 64);
            if (oi != 0x7fffffff && (mi == 0x7fffffff || om > m || (om == m && oi < mi))) { m = om; mi = oi; }
        }
        if (lane == 0) { wbest[wave] = m; warg[wave] = mi; }
        __syncthreads();
        if (tid == 0) {
            pr = wbest[0];
            arg = warg[0];                                      // wave 0 holds element 0: never the sentinel
            for (int w = 1; w < PM_WAVES; ++w)
                if (warg[w] != 0x7fffffff && (wbest[w] > pr || (wbest[w] == pr && warg[w] < arg))) { pr = wbest[w]; arg = warg[w]; }
        }
    } else {
        double s = 0.0;
        for (int i = tid; i < HW; i += PM_THREADS) s += (double)ld1(xp + i);
        s = block_sum_d<PM_WAVES>(s, scratch);
        pr = (float)(s / (double)HW);
    }
    double sq = 0.0, hit = 0.0;
    if (tid == 0) {
        g_sh = pm_plane(a, plane, pr, arg, sq, hit);
        arg_sh = arg;
    }
    __syncthreads();
    if (a.dx) {
        T* dp = (T*)a.dx + (size_t)plane * HW;
        const float g = g_sh;
        const int am = a.is_max ? arg_sh : -1;
        for (int i = tid; i < HW; i += PM_THREADS) st1(dp + i, (am < 0 || i == am) ? g : 0.f);
    }
    pm_finish(a, sq, hit, scratch, &last_flag);                // thread 0 alone carries the plane's terms; pm_finish reads only its
}

static inline int pool_mse_blocks(int NF, int HW) { return HW <= PM_SHORT ? (NF + PM_PLANES - 1) / PM_PLANES : NF; }

}  // namespace pcgan

using namespace pcgan;

extern "C" size_t pcgan_pool_mse_workspace_bytes(int NF) { return NF > 0 && NF <= PM_MAX_NF ? (size_t)(1 + 2 * (size_t)NF) * sizeof(double) : 0; }

extern "C" int pcgan_pool_mse_fwd(const void* x, const float* target, float* pred, int32_t* argmax, void* dx, float* loss, int32_t* hits,
                                  void* ws, size_t ws_bytes, int N, int F, int HW, int is_max, float delta, float gscale, int dtype,
                                  pcgan_stream_t s) {
    PCGAN_CHECK(dtype == PCGAN_F32 || dtype == PCGAN_BF16, "pool_mse_fwd: unknown dtype %d (PCGAN_F32 / PCGAN_BF16)", dtype);
    PCGAN_CHECK(N >= 1 && F >= 1 && HW >= 1 && HW <= PM_MAX_HW && (long long)N * F <= PM_MAX_NF,
                "pool_mse_fwd: N %d F %d HW %d outside N, F >= 1, N F <= %d, 1 <= HW <= %d", N, F, HW, PM_MAX_NF, PM_MAX_HW);
    PCGAN_CHECK(x && target, "pool_mse_fwd: null x / target");
    PCGAN_CHECK(!(is_max && dx) || argmax, "pool_mse_fwd: the gradient of the maximum needs argmax");
    const int NF = N * F;
    PCGAN_CHECK(ws && ws_bytes >= pcgan_pool_mse_workspace_bytes(NF), "pool_mse_fwd: workspace of %zu bytes, need %zu", ws ? ws_bytes : (size_t)0,
                pcgan_pool_mse_workspace_bytes(NF));
    PCGAN_CHECK((reinterpret_cast<size_t>(ws) & 7) == 0, "pool_mse_fwd: the workspace must be 8-byte aligned");
    PoolMseArgs a;
    a.x = x; a.target = target; a.pred = pred; a.argmax = argmax; a.dx = dx; a.loss = loss; a.hits = hits;
    a.ws = (double*)ws;
    a.NF = NF; a.HW = HW; a.is_max = is_max ? 1 : 0;
    a.delta = delta;
    a.g2 = 2.0 * (double)gscale;
    // four elements per access: 16 bytes of fp32, 8 bytes of bf16
    const size_t mask = dtype == PCGAN_F32 ? 15 : 7;
    a.vec = ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(dx)) & mask) == 0 ? 1 : 0;
    const int blocks = pool_mse_blocks(NF, HW);
    if (HW <= PM_SHORT)
        PCGAN_DTYPE_SWITCH(dtype, T, hipLaunchKernelGGL(pool_mse_short_kernel<T>, dim3(blocks), dim3(PM_THREADS), 0, (hipStream_t)s, a));
    else
        PCGAN_DTYPE_SWITCH(dtype, T, hipLaunchKernelGGL(pool_mse_long_kernel<T>, dim3(blocks), dim3(PM_THREADS), 0, (hipStream_t)s, a));
    PCGAN_LAUNCH_CHECK();
    return 0;
}
