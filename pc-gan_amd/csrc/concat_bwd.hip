// Backward pass of pcgan_concat_z (pointwise.hip) in ONE launch: dimg = dy[:, :C] (a bit-exact copy) and dz[n][j] = the sum over the plane
// dy[n][C + j][:] in fp32, summed over n as well when one rating is shared by the batch (z_batch == 1).  The call site it replaces formed
// them with a strided copy of each part of dy, the two launches of pcgan_channel_sum and, for a shared rating, a transposed copy and two
// more: three to five launches and a workspace, in steps that are host-bound.
//
// The workgroups of the one grid are split between the two jobs: the first `red` workgroups reduce, the rest copy.  An output that is
// NULL gets no workgroups, so its planes of dy are never read (a dz-only call touches N * nz planes).
//
//   reduce   one 256-lane workgroup per (n, j) plane; with a shared rating one per j, walking n = 0 .. N - 1.  A lane adds the accesses
//            it owns (index lane, lane + 256, ...) one after the other into one fp32 partial sum, the 64 partial sums of a wave are summed
//            by a butterfly (6 levels), the four wave results are added in wave order through LDS (common.h: block_sum).  The shared form
//            then adds the plane sums s_n in ascending n: ((s_0 + s_1) + ...) + s_{N-1}.  Every order is fixed by the launch geometry:
//            no atomics, no workspace, no second launch, so two calls give the same bits.
//            Longest chain of additions an element passes through: log2(V) inside one access + ceil(accesses of the plane / 256) in the
//            lane (the first of them is 0 + x, exact) + 6 + 4 (the first of them 0 + x again), + N - 1 with a shared rating.
//   copy     one workgroup per 4096 elements of a plane, raw bits (no conversion: bf16 NaN payloads survive).
//
// 16-byte accesses (V = 4 fp32 / 8 bf16 elements) when the plane size in bytes and every base pointer handed in are multiples of 16, so
// every plane starts on a 16-byte boundary; element accesses (V = 1) otherwise, e.g. for a view of dy at an odd storage offset.
// Bound: bytes moved, but at the shapes of the models latency: measured on one MI355X (scripts/bench_bigan.py, profiles/bigan_step.json),
// dz alone at [32, 3 + 1, 256, 256] fp32 takes 10.4 us (32 workgroups, 8.4 MB, 0.81 TB/s) -- what a launch costs -- and both outputs
// 20.5 us (2.9 TB/s).  A SHARED rating is the weak case: the one workgroup of a rating channel takes 1.1 us per 32 KiB plane to 6.4 us per
// 256 KiB plane, 213 us for 32 planes of 256 x 256 fp32; the host side (hip/functional.py: fused_serves) keeps the old chain there.
#include <limits.h>
#include "common.h"

namespace pcgan {

static constexpr int CZB_THREADS = 256;
static constexpr int CZB_COPY_CHUNK = 4096;       // elements of a plane one copy workgroup moves (concat_z_kernel's chunk)

template <typename T> struct CzbBits;
template <> struct CzbBits<float> { typedef unsigned type; static constexpr int V = 4; };
template <> struct CzbBits<bf16> { typedef unsigned short type; static constexpr int V = 8; };

// the sum of one 16-byte access: a balanced tree, log2(V) levels
__device__ __forceinline__ float czb_vec_sum(const float* p) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    return (v.x + v.y) + (v.z + v.w);
}
__device__ __forceinline__ float czb_vec_sum(const bf16* p) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const float a = __uint_as_float(u.x << 16) + __uint_as_float(u.x & 0xffff0000u);
    const float b = __uint_as_float(u.y << 16) + __uint_as_float(u.y & 0xffff0000u);
    const float c = __uint_as_float(u.z << 16) + __uint_as_float(u.z & 0xffff0000u);
    const float d = __uint_as_float(u.w << 16) + __uint_as_float(u.w & 0xffff0000u);
    return (a + b) + (c + d);
}

// fp32 sum of the plane p[0 .. HW), valid in every lane; four loads in flight, added in index order
template <typename T, bool WIDE>
__device__ __forceinline__ float czb_plane_sum(const T* __restrict__ p, int HW, float* scratch) {
    constexpr int V = WIDE ? CzbBits<T>::V : 1;
    const int na = HW / V;          // accesses of the plane (WIDE: HW is a multiple of V)
    float s = 0.f;
    int i = threadIdx.x;
    for (; i + 3 * CZB_THREADS < na; i += 4 * CZB_THREADS) {
        float t0, t1, t2, t3;
        if constexpr (WIDE) {
            t0 = czb_vec_sum(p + (size_t)i * V);
            t1 = czb_vec_sum(p + (size_t)(i + CZB_THREADS) * V);
            t2 = czb_vec_sum(p + (size_t)(i + 2 * CZB_THREADS) * V);
            t3 = czb_vec_sum(p + (size_t)(i + 3 * CZB_THREADS) * V);
        } else {
            t0 = ld1(p + i);
            t1 = ld1(p + i + CZB_THREADS);
            t2 = ld1(p + i + 2 * CZB_THREADS);
            t3 = ld1(p + i + 3 * CZB_THREADS);
        }
        s += t0;
        s += t1;
        s += t2;
        s += t3;
    }
    for (; i < na; i += CZB_THREADS) {
        if constexpr (WIDE) s += czb_vec_sum(p + (size_t)i * V);
        else s += ld1(p + i);
    }
    return block_sum(s, scratch);
}

// blockIdx.x < red: reduce job (plane (n, j) = blockIdx.x, or rating channel j = blockIdx.x walking n when z_batch == 1);
// otherwise copy job blockIdx.x - red = (image plane (n, c)) * chunks + chunk
template <typename T, bool WIDE>
__global__ void __launch_bounds__(CZB_THREADS) concat_z_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dimg, float* __restrict__ dz,
                                                                    int N, int C, int nz, int HW, int z_batch, int red, int chunks) {
    __shared__ float scratch[16];
    const int Ct = C + nz;
    if ((int)blockIdx.x < red) {
        if (z_batch == 1) {
            const int j = blockIdx.x;
            float acc = czb_plane_sum<T, WIDE>(dy + (size_t)(C + j) * HW, HW, scratch);
            for (int n = 1; n < N; ++n) acc += czb_plane_sum<T, WIDE>(dy + ((size_t)n * Ct + C + j) * HW, HW, scratch);
            if (threadIdx.x == 0) dz[j] = acc;
        } else {
            const int n = blockIdx.x / nz, j = blockIdx.x % nz;
            const float s = czb_plane_sum<T, WIDE>(dy + ((size_t)n * Ct + C + j) * HW, HW, scratch);
            if (threadIdx.x == 0) dz[blockIdx.x] = s;
        }
        return;
    }
    typedef typename CzbBits<T>::type B;
    const int job = blockIdx.x - red;
    const int plane = job / chunks, chunk = job % chunks;       // plane = n * C + c
    const int n = plane / C, c = plane % C;
    const int lo = chunk * CZB_COPY_CHUNK, hi = lo + CZB_COPY_CHUNK < HW ? lo + CZB_COPY_CHUNK : HW;
    const B* src = reinterpret_cast<const B*>(dy) + ((size_t)n * Ct + c) * HW;
    B* dst = reinterpret_cast<B*>(dimg) + (size_t)plane * HW;
    if constexpr (WIDE) {
        constexpr int V = CzbBits<T>::V;        // lo, hi and HW are multiples of V
        for (int i = lo + threadIdx.x * V; i < hi; i += CZB_THREADS * V)
            *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(src + i);
    } else {
        for (int i = lo + threadIdx.x; i < hi; i += CZB_THREADS) dst[i] = src[i];
    }
}

static inline bool czb_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace pcgan

using namespace pcgan;

extern "C" int pcgan_concat_z_bwd(const void* dy, void* dimg, float* dz, int N, int C, int nz, int HW, int z_batch, int dtype,
                                  pcgan_stream_t s) {
    PCGAN_CHECK(dy, "concat_z_bwd: null pointer (dy)");
    PCGAN_CHECK(dimg || dz, "concat_z_bwd: no output wanted (dimg and dz are both null)");
    PCGAN_CHECK(N > 0 && C > 0 && HW > 0, "concat_z_bwd: N = %d, C = %d, HW = %d must be positive", N, C, HW);
    PCGAN_CHECK(nz > 0, "concat_z_bwd: nz = %d must be positive", nz);
    PCGAN_CHECK(z_batch == 1 || z_batch == N, "concat_z_bwd: z batch %d must be 1 or N = %d", z_batch, N);
    PCGAN_CHECK(dtype == PCGAN_F32 || dtype == PCGAN_BF16, "concat_z_bwd: unknown dtype %d", dtype);
    const int chunks = (int)(((long long)HW + CZB_COPY_CHUNK - 1) / CZB_COPY_CHUNK);
    const long long elems = (long long)N * ((long long)C + nz) * HW;
    const long long red = dz ? (long long)z_batch * nz : 0;
    const long long blocks = red + (dimg ? (long long)N * C * chunks : 0);
    PCGAN_CHECK((long long)C + nz <= INT_MAX && elems <= INT_MAX && blocks <= INT_MAX,
                "concat_z_bwd: N * (C + nz) * HW = %lld elements, %lld workgroups overflow int", elems, blocks);
    const size_t esize = dtype == PCGAN_F32 ? 4 : 2;
    const bool wide = ((size_t)HW * esize) % 16 == 0 && czb_aligned16(dy) && (!dimg || czb_aligned16(dimg)) && (!dz || czb_aligned16(dz));
    const dim3 grid((unsigned)blocks), block(CZB_THREADS);
    hipStream_t st = (hipStream_t)s;
    if (wide) {
        PCGAN_DTYPE_SWITCH(dtype, T, hipLaunchKernelGGL((concat_z_bwd_kernel<T, true>), grid, block, 0, st, (const T*)dy, (T*)dimg, dz,
                                                        N, C, nz, HW, z_batch, (int)red, chunks));
    } else {
        PCGAN_DTYPE_SWITCH(dtype, T, hipLaunchKernelGGL((concat_z_bwd_kernel<T, false>), grid, block, 0, st, (const T*)dy, (T*)dimg, dz,
                                                        N, C, nz, HW, z_batch, (int)red, chunks));
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}
