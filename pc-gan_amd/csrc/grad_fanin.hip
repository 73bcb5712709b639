// Gradient fan-in: y = ((src0 + src1) + src2) + ... for up to 8 equally shaped tensors in ONE launch -- the sum autograd forms with
// n_src - 1 binary adds when one tensor feeds several consumers.  The chain of binary adds moves 3 * (k - 1) * n elements through HBM
// (every partial sum is written and read back); this kernel moves (k + 1) * n: each source is read once, the result written once.
// Pure streaming, HBM-bound: no LDS, no atomics, no workspace.  Bound: bytes moved, (k + 1) * n * sizeof(T).
//
// The source pointers travel inside the by-value kernel argument (AddNSrcs): no device-side pointer table, no upload.  The source count
// is a template parameter, so the k loads of a thread are k independent instructions in flight before the first add, and the pointer
// array is only ever indexed by constants (it stays in scalar registers).  Sums run strictly left to right in fp32 -- there is no
// multiply, so nothing can contract: fp32 tensors get the bits of the sequential fp32 sum, bf16 tensors are widened, summed in fp32 and
// rounded once (RNE) at the store.
//
// 16-byte accesses (4 fp32 / 8 bf16 elements) over the first n / V * V elements when y and every source are 16-byte aligned, and an
// element-by-element tail; the element form alone when any pointer is misaligned (a contiguous view at an odd storage offset).
#include "common.h"

namespace pcgan {

static constexpr unsigned ADDN_THREADS = 256;
static constexpr unsigned ADDN_MAX_BLOCKS = 2048;     // 8 workgroups per CU on 256 CUs; larger tensors wrap the grid-stride loop
static constexpr int ADDN_MAX_SRC = PCGAN_ADD_N_MAX;

struct AddNSrcs { const void* p[ADDN_MAX_SRC]; };

// ---- one access of V elements of storage type T, widened to V floats and back ----------------------------------------------------
template <typename T, int V> struct AddNVec;
template <> struct AddNVec<float, 4> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const float4 u = *reinterpret_cast<const float4*>(p);
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
__device__ __forceinline__ unsigned addn_bf16_bits(float v) { return (unsigned)__builtin_bit_cast(unsigned short, (bf16)v); }
template <> struct AddNVec<bf16, 8> {
    static __device__ __forceinline__ void load(const bf16* p, float (&v)[8]) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
        v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
        v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
        v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
    }
    static __device__ __forceinline__ void store(bf16* p, const float (&v)[8]) {
        *reinterpret_cast<uint4*>(p) = make_uint4(addn_bf16_bits(v[0]) | (addn_bf16_bits(v[1]) << 16), addn_bf16_bits(v[2]) | (addn_bf16_bits(v[3]) << 16),
                                                  addn_bf16_bits(v[4]) | (addn_bf16_bits(v[5]) << 16), addn_bf16_bits(v[6]) | (addn_bf16_bits(v[7]) << 16));
    }
};

// K sources, V elements per access (V = 1: element accesses only), index type I (unsigned where n allows it, else size_t)
template <typename T, int V, int K, typename I>
__global__ void __launch_bounds__(ADDN_THREADS) add_n_kernel(const AddNSrcs srcs, T* __restrict__ y, const I n) {
    const I tid = (I)blockIdx.x * ADDN_THREADS + threadIdx.x;
    const I stride = (I)gridDim.x * ADDN_THREADS;
    I done = 0;
    if constexpr (V > 1) {
        const I nv = n / V;
        for (I i = tid; i < nv; i += stride) {
            float in[K][V];
#pragma unroll
            for (int k = 0; k < K; ++k) AddNVec<T, V>::load(static_cast<const T*>(srcs.p[k]) + i * V, in[k]);
#pragma unroll
            for (int k = 1; k < K; ++k)
#pragma unroll
                for (int e = 0; e < V; ++e) in[0][e] += in[k][e];
            AddNVec<T, V>::store(y + i * V, in[0]);
        }
        done = nv * V;
    }
    for (I i = done + tid; i < n; i += stride) {      // the whole tensor (V = 1) or the tail of fewer than V elements
        float in[K];
#pragma unroll
        for (int k = 0; k < K; ++k) in[k] = ld1(static_cast<const T*>(srcs.p[k]) + i);
#pragma unroll
        for (int k = 1; k < K; ++k) in[0] += in[k];
        st1(y + i, in[0]);
    }
}

template <typename T, int V, int K>
static void add_n_launch(const AddNSrcs& srcs, T* y, size_t n, hipStream_t st) {
    const dim3 grid(capped_blocks(V > 1 ? n / V + 1 : n, ADDN_THREADS, ADDN_MAX_BLOCKS)), block(ADDN_THREADS);
    // 32-bit indices while the largest value formed, i + stride with i < n, stays below 2^32
    if (n <= 0x80000000ull) hipLaunchKernelGGL((add_n_kernel<T, V, K, unsigned>), grid, block, 0, st, srcs, y, (unsigned)n);
    else hipLaunchKernelGGL((add_n_kernel<T, V, K, size_t>), grid, block, 0, st, srcs, y, n);
}

template <typename T, int V>
static void add_n_dispatch(const AddNSrcs& srcs, int n_src, T* y, size_t n, hipStream_t st) {
    switch (n_src) {
        case 1: add_n_launch<T, V, 1>(srcs, y, n, st); break;
        case 2: add_n_launch<T, V, 2>(srcs, y, n, st); break;
        case 3: add_n_launch<T, V, 3>(srcs, y, n, st); break;
        case 4: add_n_launch<T, V, 4>(srcs, y, n, st); break;
        case 5: add_n_launch<T, V, 5>(srcs, y, n, st); break;
        case 6: add_n_launch<T, V, 6>(srcs, y, n, st); break;
        case 7: add_n_launch<T, V, 7>(srcs, y, n, st); break;
        default: add_n_launch<T, V, 8>(srcs, y, n, st); break;
    }
}

static inline bool addn_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace pcgan

using namespace pcgan;

extern "C" int pcgan_add_n(const void* const* srcs, int n_src, void* y, size_t n, int dtype, pcgan_stream_t s) {
    PCGAN_CHECK(n_src >= 1 && n_src <= ADDN_MAX_SRC, "add_n: n_src = %d outside 1 .. %d", n_src, ADDN_MAX_SRC);
    PCGAN_CHECK(srcs && y, "add_n: null pointer (%s)", srcs ? "y" : "srcs");
    PCGAN_CHECK(n > 0, "add_n: n == 0");
    PCGAN_CHECK(dtype == PCGAN_F32 || dtype == PCGAN_BF16, "add_n: unknown dtype %d", dtype);
    const size_t bytes = n * (dtype == PCGAN_F32 ? 4 : 2);
    const uintptr_t y0 = reinterpret_cast<uintptr_t>(y);
    AddNSrcs a;
    bool wide = addn_aligned16(y);
    for (int k = 0; k < ADDN_MAX_SRC; ++k) {
        a.p[k] = k < n_src ? srcs[k] : nullptr;
        if (k >= n_src) continue;
        PCGAN_CHECK(srcs[k], "add_n: null pointer (source %d)", k);
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(srcs[k]);
        PCGAN_CHECK(y0 + bytes <= s0 || s0 + bytes <= y0, "add_n: y may not alias a source (overlaps source %d)", k);
        wide = wide && addn_aligned16(srcs[k]);
    }
    hipStream_t st = (hipStream_t)s;
    if (dtype == PCGAN_F32) {
        if (wide) add_n_dispatch<float, 4>(a, n_src, (float*)y, n, st);
        else add_n_dispatch<float, 1>(a, n_src, (float*)y, n, st);
    } else {
        if (wide) add_n_dispatch<bf16, 8>(a, n_src, (bf16*)y, n, st);
        else add_n_dispatch<bf16, 1>(a, n_src, (bf16*)y, n, st);
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}
