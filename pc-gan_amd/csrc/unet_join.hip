// Skip join of the U-Net generator (reference models/networks.py:729-733: torch.cat([x, self.model(x)], 1), with the parent block's
// in-place ReLU folded into either half) and its gradient.  Pure data movement plus a sign test: HBM-bound, no LDS, no atomics, and
// bit-exact -- every output element is a copy of an input element or zero.
//
// Per sample each half is ONE contiguous run: a[n] is La = Ca * HW elements, b[n] is Lb = Cb * HW, out[n] is the two runs back to
// back.  A flat index over out therefore maps to (n, r) by one division and the half by one comparison; when La and Lb are both
// multiples of the vector width (and the three pointers are 16-byte aligned) a 16-byte vector never straddles the seam, so the whole
// tensor moves as 128-bit accesses (4 fp32 or 8 bf16 elements).  Everything else takes the element-by-element form of the same loop.
#include "common.h"

namespace pcgan {

static constexpr unsigned JOIN_THREADS = 256;
static constexpr unsigned JOIN_MAX_BLOCKS = 1024;     // 4 workgroups per CU on 256 CUs; larger tensors wrap the grid-stride loop

// ---- one access: V elements of storage type T, as raw bits (the values are never re-rounded) ------------------------------------
template <typename T, int V> struct JoinVec;
template <> struct JoinVec<float, 1> { typedef float type; };
template <> struct JoinVec<float, 4> { typedef float4 type; };
template <> struct JoinVec<bf16, 1> { typedef unsigned short type; };
template <> struct JoinVec<bf16, 8> { typedef uint4 type; };

__device__ __forceinline__ bool join_pos(float v) { return v > 0.f; }
__device__ __forceinline__ bool join_pos(unsigned short h) { return __uint_as_float((unsigned)h << 16) > 0.f; }
// the bf16 pair packed in one 32-bit word: keep each half where its sign source (same layout) is positive
__device__ __forceinline__ unsigned join_keep2(unsigned v, unsigned src) {
    const unsigned lo = join_pos((unsigned short)(src & 0xffffu)) ? 0x0000ffffu : 0u;
    const unsigned hi = join_pos((unsigned short)(src >> 16)) ? 0xffff0000u : 0u;
    return v & (lo | hi);
}

// v where src > 0, else +0
__device__ __forceinline__ float join_mask(float v, float src) { return join_pos(src) ? v : 0.f; }
__device__ __forceinline__ unsigned short join_mask(unsigned short v, unsigned short src) { return join_pos(src) ? v : (unsigned short)0; }
__device__ __forceinline__ float4 join_mask(const float4& v, const float4& s) {
    return make_float4(join_mask(v.x, s.x), join_mask(v.y, s.y), join_mask(v.z, s.z), join_mask(v.w, s.w));
}
__device__ __forceinline__ uint4 join_mask(const uint4& v, const uint4& s) {
    return make_uint4(join_keep2(v.x, s.x), join_keep2(v.y, s.y), join_keep2(v.z, s.z), join_keep2(v.w, s.w));
}

// out[n][0..La) = act_a(a[n]), out[n][La..La+Lb) = act_b(b[n]); act: 0 = copy, else ReLU.  La, Lb, total in elements, multiples of V.
template <typename T, int V>
__global__ void __launch_bounds__(JOIN_THREADS) skip_join_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out,
                                                                      size_t La, size_t Lb, size_t total, int relu_a, int relu_b) {
    typedef typename JoinVec<T, V>::type vec;
    const size_t L = La + Lb;
    const size_t stride = (size_t)gridDim.x * blockDim.x * V;
    for (size_t e = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V; e < total; e += stride) {
        const size_t n = e / L, r = e - n * L;
        const bool first = r < La;
        const T* src = first ? a + n * La + r : b + n * Lb + (r - La);
        vec v = *reinterpret_cast<const vec*>(src);
        if (first ? relu_a : relu_b) v = join_mask(v, v);
        *reinterpret_cast<vec*>(out + e) = v;
    }
}

// da[n] = dout[n][0..La) where a[n] > 0 (relu_a) or everywhere; db likewise from dout[n][La..).  da / db may be null (not wanted).
template <typename T, int V>
__global__ void __launch_bounds__(JOIN_THREADS) skip_join_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ a, const T* __restrict__ b,
                                                                      T* __restrict__ da, T* __restrict__ db, size_t La, size_t Lb, size_t total,
                                                                      int relu_a, int relu_b) {
    typedef typename JoinVec<T, V>::type vec;
    const size_t L = La + Lb;
    const size_t stride = (size_t)gridDim.x * blockDim.x * V;
    for (size_t e = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V; e < total; e += stride) {
        const size_t n = e / L, r = e - n * L;
        const bool first = r < La;
        const size_t o = first ? n * La + r : n * Lb + (r - La);
        T* dst = first ? da : db;
        if (dst == nullptr) continue;
        vec g = *reinterpret_cast<const vec*>(dout + e);
        if (first ? relu_a : relu_b) g = join_mask(g, *reinterpret_cast<const vec*>((first ? a : b) + o));
        *reinterpret_cast<vec*>(dst + o) = g;
    }
}

static inline bool join_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static inline int join_check_act(int act) { return act == PCGAN_ACT_NONE || act == PCGAN_ACT_RELU; }

}  // namespace pcgan

using namespace pcgan;

extern "C" int pcgan_skip_join_fwd(const void* a, const void* b, void* out, int N, int Ca, int Cb, int HW, int act_a, int act_b, int dtype,
                                   pcgan_stream_t s) {
    PCGAN_CHECK(a && b && out, "skip_join_fwd: null pointer");
    PCGAN_CHECK(N > 0 && Ca > 0 && Cb > 0 && HW > 0, "skip_join_fwd: N=%d Ca=%d Cb=%d HW=%d must be positive", N, Ca, Cb, HW);
    PCGAN_CHECK(join_check_act(act_a) && join_check_act(act_b), "skip_join_fwd: act must be PCGAN_ACT_NONE or PCGAN_ACT_RELU (got %d, %d)", act_a, act_b);
    PCGAN_CHECK(dtype == PCGAN_F32 || dtype == PCGAN_BF16, "skip_join_fwd: unknown dtype %d", dtype);
    const size_t La = (size_t)Ca * HW, Lb = (size_t)Cb * HW, total = (size_t)N * (La + Lb);
    const size_t V = dtype == PCGAN_F32 ? 4 : 8;
    const bool wide = La % V == 0 && Lb % V == 0 && join_aligned16(a) && join_aligned16(b) && join_aligned16(out);
    const dim3 grid(capped_blocks(wide ? total / V : total, JOIN_THREADS, JOIN_MAX_BLOCKS)), block(JOIN_THREADS);
    hipStream_t st = (hipStream_t)s;
    const int ra = act_a == PCGAN_ACT_RELU, rb = act_b == PCGAN_ACT_RELU;
    if (dtype == PCGAN_F32) {
        if (wide) hipLaunchKernelGGL((skip_join_fwd_kernel<float, 4>), grid, block, 0, st, (const float*)a, (const float*)b, (float*)out, La, Lb, total, ra, rb);
        else hipLaunchKernelGGL((skip_join_fwd_kernel<float, 1>), grid, block, 0, st, (const float*)a, (const float*)b, (float*)out, La, Lb, total, ra, rb);
    } else {
        if (wide) hipLaunchKernelGGL((skip_join_fwd_kernel<bf16, 8>), grid, block, 0, st, (const bf16*)a, (const bf16*)b, (bf16*)out, La, Lb, total, ra, rb);
        else hipLaunchKernelGGL((skip_join_fwd_kernel<bf16, 1>), grid, block, 0, st, (const bf16*)a, (const bf16*)b, (bf16*)out, La, Lb, total, ra, rb);
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcgan_skip_join_bwd(const void* dout, const void* a, const void* b, void* da, void* db, int N, int Ca, int Cb, int HW,
                                   int act_a, int act_b, int dtype, pcgan_stream_t s) {
    PCGAN_CHECK(dout, "skip_join_bwd: null dout");
    PCGAN_CHECK(da || db, "skip_join_bwd: neither da nor db is wanted");
    PCGAN_CHECK(N > 0 && Ca > 0 && Cb > 0 && HW > 0, "skip_join_bwd: N=%d Ca=%d Cb=%d HW=%d must be positive", N, Ca, Cb, HW);
    PCGAN_CHECK(join_check_act(act_a) && join_check_act(act_b), "skip_join_bwd: act must be PCGAN_ACT_NONE or PCGAN_ACT_RELU (got %d, %d)", act_a, act_b);
    PCGAN_CHECK(!(da && act_a == PCGAN_ACT_RELU) || a, "skip_join_bwd: da through a ReLU needs a");
    PCGAN_CHECK(!(db && act_b == PCGAN_ACT_RELU) || b, "skip_join_bwd: db through a ReLU needs b");
    PCGAN_CHECK(dtype == PCGAN_F32 || dtype == PCGAN_BF16, "skip_join_bwd: unknown dtype %d", dtype);
    const size_t La = (size_t)Ca * HW, Lb = (size_t)Cb * HW, total = (size_t)N * (La + Lb);
    const size_t V = dtype == PCGAN_F32 ? 4 : 8;
    // a half that is not wanted is never dereferenced: mask it out of the ReLU and the alignment test
    const int ra = da && act_a == PCGAN_ACT_RELU, rb = db && act_b == PCGAN_ACT_RELU;
    const bool wide = La % V == 0 && Lb % V == 0 && join_aligned16(dout) && join_aligned16(da) && join_aligned16(db) &&
                      (!ra || join_aligned16(a)) && (!rb || join_aligned16(b));
    const dim3 grid(capped_blocks(wide ? total / V : total, JOIN_THREADS, JOIN_MAX_BLOCKS)), block(JOIN_THREADS);
    hipStream_t st = (hipStream_t)s;
    if (dtype == PCGAN_F32) {
        if (wide) hipLaunchKernelGGL((skip_join_bwd_kernel<float, 4>), grid, block, 0, st, (const float*)dout, (const float*)a, (const float*)b, (float*)da, (float*)db, La, Lb, total, ra, rb);
        else hipLaunchKernelGGL((skip_join_bwd_kernel<float, 1>), grid, block, 0, st, (const float*)dout, (const float*)a, (const float*)b, (float*)da, (float*)db, La, Lb, total, ra, rb);
    } else {
        if (wide) hipLaunchKernelGGL((skip_join_bwd_kernel<bf16, 8>), grid, block, 0, st, (const bf16*)dout, (const bf16*)a, (const bf16*)b, (bf16*)da, (bf16*)db, La, Lb, total, ra, rb);
        else hipLaunchKernelGGL((skip_join_bwd_kernel<bf16, 1>), grid, block, 0, st, (const bf16*)dout, (const bf16*)a, (const bf16*)b, (bf16*)da, (bf16*)db, La, Lb, total, ra, rb);
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}
