// The two device steps of `siamese.py --mode attention`: the Grad-CAM map of a captured activation (util/gradcam.py: generate of the
// reference) and the heat-map overlay (feature2image / tensor2image and the blend of attention_gradcam, siamese.py:401-410, 965-978).
// Both are ONE launch each, take no workspace and use no atomics; every order of summation is fixed by the launch geometry, so two
// calls on the same input give the same bits.  The unit is compiled with -ffp-contract=off (csrc/Makefile): every operation below
// rounds once, like the separate torch / numpy operations it stands for.
//
// pcgan_gradcam_map     map[n][p] = post(sum_c term(n, c, p)), term = A | g * A | w * A | (w * g) * A, post = abs (raw) or relu, with
//                       w[n][c] = (sum over the plane of relu(g[n][c][:])) / HW.  All arithmetic fp32, bf16 widened exactly.
//   geometry   1024-lane workgroups, one per (image, tile of LP access units of the plane): LP = min(64, the next power of two >= the
//              units of the plane), a unit being V consecutive pixels (V = 4 fp32 / 8 bf16 in the 16-byte form, 1 in the element form).
//              The S = 1024 / LP slices of a workgroup split the channels: slice s adds its ceil(C / S) channels in ascending c into V
//              fp32 sums per lane (starting from 0: the first addition is exact), the S partial sums of a pixel meet in LDS in a halving
//              tree (log2(S) levels: slice s += slice s + h, h = S/2 .. 1), slice 0 applies abs / relu and stores.
//   weights    cw_pos / pw_cw: EVERY workgroup first computes all C plane means of its image into LDS, wave v taking the planes v, v + 16,
//              ...: a lane adds the units it owns (lane, lane + 64, ...) in index order, the relu'd elements of a unit in a balanced tree
//              (log2(V) levels), then the wave64 butterfly (6 levels) and one division by HW; where a plane is one access per lane, 16
//              (element form) or 8 planes of a wave are in flight and share their butterfly (gc_batch_wave_sum), four otherwise.
//              There is no second launch and no workspace, at the price of redundant reads: an image cut into `tiles` tiles reads its
//              gradient tiles times, i.e. (tiles - 1) * C * HW * sizeof(T) bytes more than needed, all of them L2 hits after the first
//              workgroup.  At the default layer (64 x 56 x 56 fp32: 13 tiles) that is 12 * 0.8 MB = 9.6 MB; at 7 x 7 planes (one tile)
//              nothing.  The means live in LDS, so the weighted types take at most 4096 channels.
//   longest chain of roundings of an element (tests/test_gpu_gradcam.py mirrors it): ceil(C / S) + log2(S) additions, + 1 (g * A), and
//              for the weighted types + log2(V) + ceil(units / 64) + 6 + 1 for w and + 1 (w * A) or + 2 ((w * g) * A).
//   16-byte accesses when HW * sizeof(T) and every pointer handed in are multiples of 16, element accesses otherwise.
//   Bound: latency.  The largest call of the encoder (64 x 56 x 56) moves 0.8 - 1.6 MB.
//
// pcgan_heatmap_overlay one 1024-lane workgroup per image: the minimum and maximum of the image's Cm * HW map values (selections: lane,
//              wave butterfly, the 16 wave results through LDS), then out = ((m - lo) / (hi - lo) * 255) * (1 - alpha) +
//              ((img * std + mean) * 255) * alpha per element, the heat term being 0 where hi == lo (the reference divides by zero
//              there).  4-element accesses when HW % 4 == 0 and the pointers allow, element accesses otherwise.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace pcgan {

static constexpr int GC_THREADS = 1024;
static constexpr int GC_WAVES = GC_THREADS / 64;
static constexpr int GC_MAX_C_WEIGHTED = 4096;       // plane means kept in LDS beside at most 32 KiB of partial sums: 48 KiB in all

template <typename T, int V> struct GcLoad;
template <typename T> struct GcLoad<T, 1> {
    static __device__ __forceinline__ void run(const T* p, float (&v)[1]) { v[0] = ld1(p); }
};
template <> struct GcLoad<float, 4> {
    static __device__ __forceinline__ void run(const float* p, float (&v)[4]) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    }
};
template <> struct GcLoad<bf16, 8> {
    static __device__ __forceinline__ void run(const bf16* p, float (&v)[8]) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
        v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
        v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
        v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
    }
};

__device__ __forceinline__ float gc_relu(float v) { return v > 0.f ? v : 0.f; }

// the sum of the relu'd elements of one unit: a balanced tree, log2(V) levels
template <int V> __device__ __forceinline__ float gc_relu_sum(const float (&v)[V]) {
    if constexpr (V == 1) return gc_relu(v[0]);
    else if constexpr (V == 4) return (gc_relu(v[0]) + gc_relu(v[1])) + (gc_relu(v[2]) + gc_relu(v[3]));
    else return ((gc_relu(v[0]) + gc_relu(v[1])) + (gc_relu(v[2]) + gc_relu(v[3]))) +
                ((gc_relu(v[4]) + gc_relu(v[5])) + (gc_relu(v[6]) + gc_relu(v[7])));
}

// relu'd sum of the plane g[0 .. units * V) over the wave, the same bits in every lane
template <typename T, int V> __device__ __forceinline__ float gc_plane_relu_sum(const T* __restrict__ g, int units, int lane) {
    float s = 0.f;
#pragma unroll 4
    for (int i = lane; i < units; i += 64) {
        float v[V];
        GcLoad<T, V>::run(g + (size_t)i * V, v);
        s += gc_relu_sum<V>(v);
    }
    return s;
}

// The wave sums of PB per-lane values at once (PB a power of two <= 64): lane l returns the sum over the wave of s[l % PB].  A butterfly per
// value costs 6 cross-lane moves each, and at 2048 x 7 x 7 those moves, not memory, were the weights' time; here the first log2(PB)
// levels fold two values into one register -- the lanes whose bit is clear keep the even value and hand over the odd one, the others the
// reverse -- so all PB sums take PB - 1 + 6 - log2(PB) moves.  Every value still passes 6 additions, its partner lanes at distance 1, 2, ..., 32.
template <int PB> __device__ __forceinline__ float gc_batch_wave_sum(float (&s)[PB], int lane) {
    int step = 0;
#pragma unroll
    for (int n = PB; n > 1; n >>= 1, ++step) {
        const int d = 1 << step;
        const bool up = (lane & d) != 0;
#pragma unroll
        for (int k = 0; k < n / 2; ++k) {
            const float keep = up ? s[2 * k + 1] : s[2 * k], give = up ? s[2 * k] : s[2 * k + 1];
            s[k] = keep + __shfl_xor(give, d, 64);
        }
    }
    float r = s[0];
#pragma unroll
    for (int d = PB; d < 64; d <<= 1) r += __shfl_xor(r, d, 64);
    return r;
}

// TYPE: PCGAN_GCAM_RAW / _PW / _CW_POS / _PW_CW.  Dynamic LDS: GC_THREADS * V floats of partial sums, then C plane means (weighted types).
template <typename T, int V, int TYPE>
__global__ void __launch_bounds__(GC_THREADS) gradcam_map_kernel(const T* __restrict__ act, const T* __restrict__ grad, float* __restrict__ out,
                                                                  int C, int HW, int lp_log2, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float gc_smem[];
    float* part = gc_smem;
    float* wts = gc_smem + GC_THREADS * V;
    constexpr bool WEIGHTED = TYPE == PCGAN_GCAM_CW_POS || TYPE == PCGAN_GCAM_PW_CW;
    constexpr bool USES_G = TYPE != PCGAN_GCAM_RAW;
    const int tid = threadIdx.x;
    const int n = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int units = HW / V;
    const T* an = act + (size_t)n * C * HW;
    const T* gn = USES_G ? grad + (size_t)n * C * HW : nullptr;

    if constexpr (WEIGHTED) {
        const int lane = tid & 63, wave = tid >> 6;
        const float hw = (float)HW;
        if (units <= 64) {
            // a plane is one access per lane: GC_SMALL_BATCH planes of a wave in flight, as many as the registers hold (at 2048 x 7 x 7
            // the loads of four planes at a time left the one workgroup of an image waiting on memory 32 times in a row)
            constexpr int GC_SMALL_BATCH = V == 1 ? 16 : 8;
            for (int c0 = wave; c0 < C; c0 += GC_SMALL_BATCH * GC_WAVES) {
                float s[GC_SMALL_BATCH];
#pragma unroll
                for (int k = 0; k < GC_SMALL_BATCH; ++k) {
                    const int c = c0 + k * GC_WAVES;
                    s[k] = 0.f;
                    if (c < C && lane < units) {
                        float v[V];
                        GcLoad<T, V>::run(gn + (size_t)c * HW + (size_t)lane * V, v);
                        s[k] += gc_relu_sum<V>(v);
                    }
                }
                const float total = gc_batch_wave_sum<GC_SMALL_BATCH>(s, lane);      // plane k of the batch in the lanes with lane % batch == k
                const int c = c0 + lane * GC_WAVES;
                if (lane < GC_SMALL_BATCH && c < C) wts[c] = total / hw;
            }
        } else {
            for (int c0 = wave; c0 < C; c0 += 4 * GC_WAVES) {       // four planes of a wave in flight
                float s[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = c0 + k * GC_WAVES;
                    s[k] = c < C ? gc_plane_relu_sum<T, V>(gn + (size_t)c * HW, units, lane) : 0.f;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int c = c0 + k * GC_WAVES;
                        if (c < C) wts[c] = s[k] / hw;
                    }
                }
            }
        }
        __syncthreads();
    }

    const int LP = 1 << lp_log2, S = GC_THREADS >> lp_log2;
    const int lp = tid & (LP - 1), sl = tid >> lp_log2;
    const int u = tile * LP + lp;                                // this lane's unit of the plane
    const int cps = (C + S - 1) / S;
    const int c_lo = sl * cps < C ? sl * cps : C, c_hi = c_lo + cps < C ? c_lo + cps : C;
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    if (u < units) {
        const size_t off = (size_t)u * V;
        constexpr int UNROLL = V == 1 ? 8 : 4;                  // channels of a slice in flight
#pragma unroll UNROLL
        for (int c = c_lo; c < c_hi; ++c) {
            float a[V];
            GcLoad<T, V>::run(an + (size_t)c * HW + off, a);
            if constexpr (TYPE == PCGAN_GCAM_RAW) {
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] += a[j];
            } else if constexpr (TYPE == PCGAN_GCAM_CW_POS) {
                const float w = wts[c];
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] += w * a[j];
            } else {
                float g[V];
                GcLoad<T, V>::run(gn + (size_t)c * HW + off, g);
                if constexpr (TYPE == PCGAN_GCAM_PW) {
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] += g[j] * a[j];
                } else {
                    const float w = wts[c];
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] += (w * g[j]) * a[j];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) part[tid * V + j] = acc[j];
    for (int h = S >> 1; h >= 1; h >>= 1) {                      // slice sl += slice sl + h
        __syncthreads();
        if (sl < h) {
#pragma unroll
            for (int j = 0; j < V; ++j) part[tid * V + j] += part[(tid + h * LP) * V + j];
        }
    }
    if (sl == 0 && u < units) {                                  // (with S == 1 the thread reads back its own partial sums)
        float* o = out + (size_t)n * HW + (size_t)u * V;
        float r[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float v = part[tid * V + j];
            r[j] = TYPE == PCGAN_GCAM_RAW ? fabsf(v) : gc_relu(v);
        }
        if constexpr (V == 1) {
            o[0] = r[0];
        } else {
#pragma unroll
            for (int j = 0; j < V; j += 4) *reinterpret_cast<float4*>(o + j) = make_float4(r[j], r[j + 1], r[j + 2], r[j + 3]);
        }
    }
}

struct GcBlend {
    float mean[3], std[3], alpha;
};

// smallest / largest over the workgroup, valid in every thread; scratch: 2 * GC_WAVES floats
__device__ __forceinline__ void gc_block_minmax(float& lo, float& hi, float* scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
        scratch[wave] = lo;
        scratch[GC_WAVES + wave] = hi;
    }
    __syncthreads();
    lo = scratch[0];
    hi = scratch[GC_WAVES];
    for (int i = 1; i < GC_WAVES; ++i) {
        lo = fminf(lo, scratch[i]);
        hi = fmaxf(hi, scratch[GC_WAVES + i]);
    }
}

__device__ __forceinline__ float gc_blend(float m, float x, float lo, float range, bool flat, float keep, float mean, float std, float alpha) {
    const float heat = flat ? 0.f : ((m - lo) / range) * 255.f;
    const float pix = (x * std + mean) * 255.f;
    return heat * keep + pix * alpha;
}

template <typename T, bool WIDE>
__global__ void __launch_bounds__(GC_THREADS) heatmap_overlay_kernel(const float* __restrict__ map, const T* __restrict__ img,
                                                                      float* __restrict__ out, float* __restrict__ lohi, GcBlend b, int Cm, int HW) {
    __shared__ float scratch[2 * GC_WAVES];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* mp = map + (size_t)n * Cm * HW;
    const int total = Cm * HW;
    float lo = INFINITY, hi = -INFINITY;
    if constexpr (WIDE) {
        for (int i = tid * 4; i < total; i += GC_THREADS * 4) {
            const float4 v = *reinterpret_cast<const float4*>(mp + i);
            lo = fminf(lo, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
            hi = fmaxf(hi, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        }
    } else {
        for (int i = tid; i < total; i += GC_THREADS) {
            const float v = mp[i];
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    gc_block_minmax(lo, hi, scratch);
    if (tid == 0) {
        lohi[2 * n] = lo;
        lohi[2 * n + 1] = hi;
    }
    const float range = hi - lo, keep = 1.f - b.alpha;
    const bool flat = !(hi > lo);
    for (int c = 0; c < 3; ++c) {
        const float* mc = mp + (size_t)(Cm == 1 ? 0 : c) * HW;
        const T* ip = img + ((size_t)n * 3 + c) * HW;
        float* op = out + ((size_t)n * 3 + c) * HW;
        const float mean = b.mean[c], std = b.std[c];
        if constexpr (WIDE) {
            for (int i = tid * 4; i < HW; i += GC_THREADS * 4) {
                const float4 m = *reinterpret_cast<const float4*>(mc + i);
                const float4 x = ld4(ip + i);
                float4 o;
                o.x = gc_blend(m.x, x.x, lo, range, flat, keep, mean, std, b.alpha);
                o.y = gc_blend(m.y, x.y, lo, range, flat, keep, mean, std, b.alpha);
                o.z = gc_blend(m.z, x.z, lo, range, flat, keep, mean, std, b.alpha);
                o.w = gc_blend(m.w, x.w, lo, range, flat, keep, mean, std, b.alpha);
                *reinterpret_cast<float4*>(op + i) = o;
            }
        } else {
            for (int i = tid; i < HW; i += GC_THREADS) op[i] = gc_blend(mc[i], ld1(ip + i), lo, range, flat, keep, mean, std, b.alpha);
        }
    }
}

static inline bool gc_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

template <typename T, int V>
static int gc_launch_map(int type, const T* act, const T* grad, float* out, int C, int HW, int lp_log2, int tiles, unsigned blocks, size_t lds,
                         hipStream_t st) {
    const dim3 grid(blocks), block(GC_THREADS);
    switch (type) {
        case PCGAN_GCAM_RAW:
            hipLaunchKernelGGL((gradcam_map_kernel<T, V, PCGAN_GCAM_RAW>), grid, block, lds, st, act, grad, out, C, HW, lp_log2, tiles);
            break;
        case PCGAN_GCAM_PW:
            hipLaunchKernelGGL((gradcam_map_kernel<T, V, PCGAN_GCAM_PW>), grid, block, lds, st, act, grad, out, C, HW, lp_log2, tiles);
            break;
        case PCGAN_GCAM_CW_POS:
            hipLaunchKernelGGL((gradcam_map_kernel<T, V, PCGAN_GCAM_CW_POS>), grid, block, lds, st, act, grad, out, C, HW, lp_log2, tiles);
            break;
        default:
            hipLaunchKernelGGL((gradcam_map_kernel<T, V, PCGAN_GCAM_PW_CW>), grid, block, lds, st, act, grad, out, C, HW, lp_log2, tiles);
            break;
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace pcgan

using namespace pcgan;

extern "C" int pcgan_gradcam_map(const void* act, const void* grad, float* map, int N, int C, int H, int W, int type, int dtype,
                                 pcgan_stream_t s) {
    PCGAN_CHECK(type == PCGAN_GCAM_RAW || type == PCGAN_GCAM_PW || type == PCGAN_GCAM_CW_POS || type == PCGAN_GCAM_PW_CW,
                "gradcam_map: unknown map type %d", type);
    PCGAN_CHECK(N > 0 && C > 0 && H > 0 && W > 0, "gradcam_map: N = %d, C = %d, H = %d, W = %d must be positive", N, C, H, W);
    PCGAN_CHECK(act && map, "gradcam_map: null pointer (act or map)");
    PCGAN_CHECK(grad || type == PCGAN_GCAM_RAW, "gradcam_map: null pointer (grad): only the raw type needs no gradient");
    PCGAN_CHECK(dtype == PCGAN_F32 || dtype == PCGAN_BF16, "gradcam_map: unknown dtype %d", dtype);
    const bool weighted = type == PCGAN_GCAM_CW_POS || type == PCGAN_GCAM_PW_CW;
    PCGAN_CHECK(!weighted || C <= GC_MAX_C_WEIGHTED, "gradcam_map: C = %d channels, the weighted types keep at most %d plane means in LDS", C,
                GC_MAX_C_WEIGHTED);
    const long long HW = (long long)H * W, elems = (long long)N * C * HW;
    PCGAN_CHECK(elems <= INT_MAX, "gradcam_map: N * C * H * W = %lld elements overflow int", elems);
    if (type == PCGAN_GCAM_RAW) grad = nullptr;        // neither read nor required
    const size_t esize = dtype == PCGAN_F32 ? 4 : 2;
    const bool wide = ((size_t)HW * esize) % 16 == 0 && gc_aligned(act, 16) && gc_aligned(grad, 16) && gc_aligned(map, 16);
    const int V = wide ? (int)(16 / esize) : 1;
    const int units = (int)(HW / V);
    int lp_log2 = 0;
    while (lp_log2 < 6 && (1 << lp_log2) < units) ++lp_log2;
    const int LP = 1 << lp_log2, tiles = (units + LP - 1) / LP;
    const long long blocks = (long long)N * tiles;
    PCGAN_CHECK(blocks <= INT_MAX, "gradcam_map: %lld workgroups overflow int", blocks);
    const size_t lds = ((size_t)GC_THREADS * V + (weighted ? (size_t)C : 0)) * sizeof(float);
    hipStream_t st = (hipStream_t)s;
    if (dtype == PCGAN_F32) {
        if (wide) return gc_launch_map<float, 4>(type, (const float*)act, (const float*)grad, map, C, (int)HW, lp_log2, tiles, (unsigned)blocks, lds, st);
        return gc_launch_map<float, 1>(type, (const float*)act, (const float*)grad, map, C, (int)HW, lp_log2, tiles, (unsigned)blocks, lds, st);
    }
    if (wide) return gc_launch_map<bf16, 8>(type, (const bf16*)act, (const bf16*)grad, map, C, (int)HW, lp_log2, tiles, (unsigned)blocks, lds, st);
    return gc_launch_map<bf16, 1>(type, (const bf16*)act, (const bf16*)grad, map, C, (int)HW, lp_log2, tiles, (unsigned)blocks, lds, st);
}

extern "C" int pcgan_heatmap_overlay(const float* map, const void* img, const float* mean, const float* std, float alpha, float* out,
                                     float* lohi, int N, int Cm, int H, int W, int dtype, pcgan_stream_t s) {
    PCGAN_CHECK(N > 0 && H > 0 && W > 0, "heatmap_overlay: N = %d, H = %d, W = %d must be positive", N, H, W);
    PCGAN_CHECK(Cm == 1 || Cm == 3, "heatmap_overlay: the map has %d channels, 1 or 3 expected", Cm);
    PCGAN_CHECK(map && img && out && lohi, "heatmap_overlay: null pointer (map, img, out or lohi)");
    PCGAN_CHECK(mean && std, "heatmap_overlay: null pointer (mean or std, host arrays of 3)");
    PCGAN_CHECK(dtype == PCGAN_F32 || dtype == PCGAN_BF16, "heatmap_overlay: unknown dtype %d", dtype);
    const long long HW = (long long)H * W, elems = (long long)N * 3 * HW;
    PCGAN_CHECK(elems <= INT_MAX, "heatmap_overlay: N * 3 * H * W = %lld elements overflow int", elems);
    GcBlend b;
    for (int c = 0; c < 3; ++c) {
        b.mean[c] = mean[c];
        b.std[c] = std[c];
    }
    b.alpha = alpha;
    const size_t esize = dtype == PCGAN_F32 ? 4 : 2;
    const bool wide = HW % 4 == 0 && gc_aligned(map, 16) && gc_aligned(out, 16) && gc_aligned(img, (unsigned)(4 * esize));
    const dim3 grid((unsigned)N), block(GC_THREADS);
    hipStream_t st = (hipStream_t)s;
    if (wide) {
        PCGAN_DTYPE_SWITCH(dtype, T, hipLaunchKernelGGL((heatmap_overlay_kernel<T, true>), grid, block, 0, st, map, (const T*)img, out, lohi, b,
                                                        Cm, (int)HW));
    } else {
        PCGAN_DTYPE_SWITCH(dtype, T, hipLaunchKernelGGL((heatmap_overlay_kernel<T, false>), grid, block, 0, st, map, (const T*)img, out, lohi, b,
                                                        Cm, (int)HW));
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}
