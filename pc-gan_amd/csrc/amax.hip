// Operand maxima of the fp16 two-piece routes: the largest magnitude of a tensor (as partial maxima, one per workgroup), the audit of
// such maxima against a fresh pass, and the largest magnitude of every row of a weight matrix.  Every fp16-route convolution scales
// its operands by powers of two derived from these (pow2_scale, common.h): the window kernel and the per-tap weight gradient of this
// family (halo_conv.hip, hsplit_wgrad.hip), hgemm.hip, thin_conv.hip, wgrad_direct.hip and wgrad_rowring.hip.  Replaces the
// `x.abs().max()` passes a host would make; callers: pcgan_absmax / pcgan_amax_audit (hip/ops.py) and launch_weight_row_absmax
// (common.h) from the pack calls.
#include "common.h"

namespace pcgan {

// partial maxima of |x|: out[blockIdx.x] = the largest magnitude this workgroup saw (consumers take the largest of the partials)
template <typename TA>
__global__ void __launch_bounds__(256) absmax_kernel(const TA* __restrict__ x, size_t n, float* __restrict__ out) {
    float m = 0.f;
    // scalar head up to a 16-byte boundary (a weight tensor may be a view into the optimizer's flat buffer), vector body, scalar tail
    size_t head = ((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / sizeof(TA);
    head = head < n ? head : n;
    const TA* xb = x + head;
    const size_t nb = n - head, n4 = nb / 4, stride = (size_t)gridDim.x * blockDim.x;
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {       // four independent 16-byte loads in flight per thread
        const float4 a = ld4(xb + 4 * i), b = ld4(xb + 4 * (i + stride)), c = ld4(xb + 4 * (i + 2 * stride)), d = ld4(xb + 4 * (i + 3 * stride));
        m = fmaxf(m, fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))), fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w)))));
        m = fmaxf(m, fmaxf(fmaxf(fmaxf(fabsf(c.x), fabsf(c.y)), fmaxf(fabsf(c.z), fabsf(c.w))), fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fmaxf(fabsf(d.z), fabsf(d.w)))));
    }
    for (; i < n4; i += stride) {
        const float4 v = ld4(xb + 4 * i);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) m = fmaxf(m, fabsf(ld1(x + threadIdx.x)));
        if (threadIdx.x < (nb & 3)) m = fmaxf(m, fabsf(ld1(xb + 4 * n4 + threadIdx.x)));
    }
    __shared__ float red[16];
    m = block_max(m, red);
    if (threadIdx.x == 0) out[blockIdx.x] = m;
}

// Audit of operand maxima (round 4): `claimed` = the partial maxima a tensor carries (its producer's, or an earlier absmax pass),
// `fresh` = the partials of an absmax pass made NOW.  Both are maxima over the same stored values, so their largest entries must be
// EQUAL; counts[0] += 1 when the tensor holds a larger value than claimed (an fp16 piece would overflow), counts[1] += 1 when its
// largest value is below 2^-8 of the claim (the scaled operand sits >= 8 bits under the fp16 target range: low pieces go subnormal and
// precision is lost SILENTLY -- the case the non-finite sentinel cannot see), counts[2] += 1 for any other mismatch.
__global__ void __launch_bounds__(256) amax_audit_kernel(const float* __restrict__ claimed, int nc, const float* __restrict__ fresh, int nf,
                                                         unsigned* __restrict__ counts) {
    __shared__ float red[16];
    float c = 0.f, f = 0.f;
    for (int i = threadIdx.x; i < nc; i += 256) c = fmaxf(c, claimed[i]);
    for (int i = threadIdx.x; i < nf; i += 256) f = fmaxf(f, fresh[i]);
    c = block_max(c, red);
    __syncthreads();
    f = block_max(f, red);
    if (threadIdx.x == 0 && f != c) {
        if (!(f <= c)) atomicAdd(counts + 0, 1u);                  // larger than claimed (or NaN)
        else if (f < c * 0.00390625f) atomicAdd(counts + 1, 1u);    // under-scaled by 2^8 or more
        else atomicAdd(counts + 2, 1u);
    }
}

// largest magnitude of every ROW of a convolution's weight matrix, w[K][C][T]: by_c = 0 the rows of the forward GEMM (output channel k:
// C * T contiguous values), by_c = 1 the rows of the data gradient (input channel c: K runs of T values).  One workgroup per row.
__global__ void __launch_bounds__(256) weight_row_absmax_kernel(const float* __restrict__ w, int K, int C, int T, int by_c, float* __restrict__ out) {
    const int row = blockIdx.x;
    float m = 0.f;
    if (!by_c) {
        const float* p = w + (size_t)row * C * T;
        for (int i = threadIdx.x; i < C * T; i += 256) m = fmaxf(m, fabsf(p[i]));
    } else {
        for (int i = threadIdx.x; i < K * T; i += 256) {
            const int k = i / T, t = i - k * T;
            m = fmaxf(m, fabsf(w[((size_t)k * C + row) * T + t]));
        }
    }
    __shared__ float red[16];
    m = block_max(m, red);
    if (threadIdx.x == 0) out[row] = m;
}

int launch_weight_row_absmax(const float* w, int K, int C, int T, int by_c, float* out, hipStream_t st) {
    hipLaunchKernelGGL(weight_row_absmax_kernel, dim3((unsigned)(by_c ? C : K)), dim3(256), 0, st, w, K, C, T, by_c, out);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace pcgan

extern "C" int pcgan_absmax_slots(size_t n) {
    const size_t want = (n / 4 + 1023) / 1024;       // ~4 vector loads per thread
    return (int)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
}

extern "C" int pcgan_absmax(const void* x, size_t n, int dtype, float* out, int slots, pcgan_stream_t s) {
    PCGAN_CHECK(x && out && n > 0 && slots > 0 && slots <= 1024, "absmax: null pointer, empty tensor or bad slot count");
    PCGAN_CHECK(dtype == PCGAN_F32 || dtype == PCGAN_BF16, "absmax: dtype %d", dtype);
    hipStream_t st = (hipStream_t)s;
    const dim3 grid((unsigned)slots);
    if (dtype == PCGAN_BF16) hipLaunchKernelGGL(pcgan::absmax_kernel<pcgan::bf16>, grid, dim3(256), 0, st, (const pcgan::bf16*)x, n, out);
    else hipLaunchKernelGGL(pcgan::absmax_kernel<float>, grid, dim3(256), 0, st, (const float*)x, n, out);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcgan_amax_audit(const float* claimed, int n_claimed, const float* fresh, int n_fresh, unsigned int* counts, pcgan_stream_t s) {
    PCGAN_CHECK(claimed && fresh && counts && n_claimed > 0 && n_fresh > 0, "amax_audit: null pointer or empty maxima");
    hipLaunchKernelGGL(pcgan::amax_audit_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, claimed, n_claimed, fresh, n_fresh, counts);
    PCGAN_LAUNCH_CHECK();
    return 0;
}
