// Internal header of the implicit-GEMM convolution family (not installed): what its kernel units share -- the range-checked
// gathers, the argument structs of a launch, the tap / pixel arithmetic -- and the launchers through which the host unit
// (igemm_conv.hip, whose header lists the units) reaches the kernels.
#pragma once
#include "common.h"
#include <type_traits>

namespace pcgan {

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { MODE_FWD_ZERO = 0, MODE_FWD_REFLECT = 1, MODE_BWD = 2, MODE_BWD_REFLECT = 3 };

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
static constexpr unsigned OOB = 0x80000000u;  // byte offset beyond any tensor (< 2 GiB): hardware returns 0

// Range-checked buffer loads: an invalid lane gets voffset = OOB and reads 0 -- no exec-mask
// branches, no 64-bit address arithmetic in the gather.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float ld_b32(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ float4 ld_b128(__amdgpu_buffer_rsrc_t r, unsigned voff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// Activation tensors (x, y, dy, dx) are stored as TA = float or bf16 (common.h); the gathers go through range-checked buffer
// loads with BYTE offsets, so every offset of an activation tensor is scaled by ES = sizeof(TA).  Weights (packed A operands),
// partial sums and weight gradients are always fp32.
template <typename TA>
__device__ __forceinline__ float ldx(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff);
template <>
__device__ __forceinline__ float ldx<float>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) { return ld_b32(r, voff, soff); }
template <>
__device__ __forceinline__ float ldx<bf16>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0) << 16);
}
// four consecutive elements
template <typename TA>
__device__ __forceinline__ float4 ldx4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff);
template <>
__device__ __forceinline__ float4 ldx4<float>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
template <>
__device__ __forceinline__ float4 ldx4<bf16>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
    return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                       __uint_as_float(v.y & 0xffff0000u));
}

// ---- bf16 tensors on the fp32-MFMA kernels without a conversion instruction per element ---------------------------------
// A gathered bf16 element arrives zero-extended in the LOW half of a VGPR; the fp32 value it stands for has those 16 bits in
// the HIGH half.  Shifting in the vector ALU costs one VALU instruction per element, which these VALU-starved loops feel
// (4 VALU per MFMA = 18 %; measured +20-30 % on igemm2, +95 % on wgrad2 with the shift).  Instead the LDS
// operand tiles of the ACTIVATIONS are zeroed once per workgroup and every element is stored with a 16-bit LDS write into the
// high half of its fp32 slot (ds_write_b16 / ds_write_b16_d16_hi: same instruction count as the 32-bit store they replace).
//   ldr / ldr4   raw gathered element(s): the fp32 value itself, or (bf16) the zero-extended / packed 16-bit pattern(s)
//   put1 / put4 / put4p  store raw element(s) into consecutive fp32 LDS slots
//   raw2f        the fp32 value of a raw element (where arithmetic on it is needed before the store)
template <typename TA>
__device__ __forceinline__ float ldr(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff);
template <>
__device__ __forceinline__ float ldr<float>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) { return ld_b32(r, voff, soff); }
template <>
__device__ __forceinline__ float ldr<bf16>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0));
}
template <typename TA>
__device__ __forceinline__ float raw2f(float raw) {
    if constexpr (sizeof(TA) == 2) return __uint_as_float(__float_as_uint(raw) << 16);
    else return raw;
}
template <typename TA>
__device__ __forceinline__ void put1(float* slot, float raw) {
    if constexpr (sizeof(TA) == 2) reinterpret_cast<unsigned short*>(slot)[1] = (unsigned short)__float_as_uint(raw);
    else *slot = raw;
}
template <typename TA>
__device__ __forceinline__ void put4(float* slot, float r0, float r1, float r2, float r3) {
    if constexpr (sizeof(TA) == 2) {
        unsigned short* p = reinterpret_cast<unsigned short*>(slot);
        p[1] = (unsigned short)__float_as_uint(r0);
        p[3] = (unsigned short)__float_as_uint(r1);
        p[5] = (unsigned short)__float_as_uint(r2);
        p[7] = (unsigned short)__float_as_uint(r3);
    } else {
        *reinterpret_cast<float4*>(slot) = make_float4(r0, r1, r2, r3);
    }
}
// four CONSECUTIVE elements: fp32: four values; bf16: two dwords of two packed elements each (in .x, .y)
template <typename TA>
__device__ __forceinline__ float4 ldr4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    if constexpr (sizeof(TA) == 2) {
        typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), 0.f, 0.f);
    } else {
        return ldx4<float>(r, voff, soff);
    }
}
template <typename TA>
__device__ __forceinline__ void put4p(float* slot, const float4& raw) {
    if constexpr (sizeof(TA) == 2) {
        unsigned short* p = reinterpret_cast<unsigned short*>(slot);
        const unsigned a = __float_as_uint(raw.x), b = __float_as_uint(raw.y);
        p[1] = (unsigned short)a;
        p[3] = (unsigned short)(a >> 16);       // ds_write_b16_d16_hi
        p[5] = (unsigned short)b;
        p[7] = (unsigned short)(b >> 16);
    } else {
        *reinterpret_cast<float4*>(slot) = raw;
    }
}
// zero an LDS tile (all threads of the workgroup; the caller's next barrier publishes it)
template <typename TA>
__device__ __forceinline__ void zero_tile(float* tile, int n) {
    if constexpr (sizeof(TA) == 2)
        for (int i = threadIdx.x; i < n; i += blockDim.x) tile[i] = 0.f;
}

struct PhaseArgs {
    const float* A;  // [M][Kp], k = (tap_index * Cgp + c)
    int Kp;
    int Hs, Ws;      // pixel sub-grid of this phase
    int fy, fx;      // output coordinate = sub * ostep + f
    int r0, s0, nR, nS;  // taps: r = r0 + i*tstep (i < nR), s = s0 + j*tstep (j < nS)
    int Ptot;        // N * Hs * Ws
    const float* As; // small-M strip kernel: weights as [c][sj][8][4] (row taps and outputs zero-padded)
    int ymap;        // 1: sub-grid row sy is output row {0, pad+1 .. H-2-pad, H-1}[sy] (rows without a mirror image)
};

struct IgemmArgs {
    const void* X;      // gathered tensor [N][Cg][Hg][Wg], storage type TA
    void* Y;            // output tensor   [N][M][Yh][Yw], storage type TA
    int dtype;          // PCGAN_F32 / PCGAN_BF16: which TA instantiation runs
    const float* bias;  // [M] or null
    int M, N, Cg, Cgp, Hg, Wg;
    int Yh, Yw;
    int ostep, sl, pad, tstep;
    int act;
    float slope;
    unsigned x_bytes;
    int nphase;
    int rowfold;  // MODE_BWD_REFLECT: the row mirrors are folded into per-phase weights, only column mirrors are gathered
    int chunked;  // K order of ph[].A: 1 = (16-channel chunk, tap, channel) -> igemm2_kernel, 0 = (tap, channel)
    int ksplit;   // > 1: blockIdx.z takes a contiguous range of K stages and stores a raw partial sum
    float* Ypart; // [ksplit][N][M][Yh][Yw] partial sums (then reduced + bias + activation by splitk_reduce)
    int tstart[17];  // igemm2_kernel: first pixel tile of each phase in the linearised grid (no empty workgroups)
    PhaseArgs ph[16];
    // fp16 two-piece form (hgemm_kernel): partial maxima of |X| and the largest |weight| (device); hsplit selects the kernel
    const float* x_amax;
    const float* w_amax;
    int x_namax, hsplit;
    unsigned* ovf;      // non-finite sentinel (common.h); may be null
};

struct Geom {
    int Hg, Wg, sl, pad;
};

// spatial offset of tap (r, s) for the pixel (py, px) of this thread
template <int MODE>
__device__ __forceinline__ bool tap_offset(const Geom& a, int py, int px, int r, int s, int& off) {
    if (MODE == MODE_BWD || MODE == MODE_BWD_REFLECT) {
        const int ty = py + a.pad - r, tx = px + a.pad - s;
        const int oy = ty >> a.sl, ox = tx >> a.sl;  // divisible by construction of the phase
        off = oy * a.Wg + ox;
        return (ty >= 0) & (tx >= 0) & (oy < a.Hg) & (ox < a.Wg);  // '&': straight-line code, no branches
    } else {
        int iy = (py << a.sl) - a.pad + r;
        int ix = (px << a.sl) - a.pad + s;
        if (MODE == MODE_FWD_REFLECT) {
            iy = iy < 0 ? -iy : iy;
            iy = iy >= a.Hg ? 2 * (a.Hg - 1) - iy : iy;
            ix = ix < 0 ? -ix : ix;
            ix = ix >= a.Wg ? 2 * (a.Wg - 1) - ix : ix;
            off = iy * a.Wg + ix;
            return true;
        } else {
            off = iy * a.Wg + ix;
            return ((unsigned)iy < (unsigned)a.Hg) & ((unsigned)ix < (unsigned)a.Wg);
        }
    }
}

// wave-uniform iterator over the K slots (ri, sj, c) with c fastest
struct KIter {
    int ri, sj, c;
    __device__ __forceinline__ void advance(int n, int Cgp, int nS) {
        c += n;
        while (c >= Cgp) {
            c -= Cgp;
            if (++sj == nS) {
                sj = 0;
                ++ri;
            }
        }
    }
};

static constexpr int NTAP_FWD = 25;   // filter taps the offset table holds (5x5)
static constexpr int NTAP_MIR = 9;    // ... for the fused reflect data gradient (4 source combinations)
static constexpr int NTAP_CG4 = 49;   // ... for 3-/4-channel tensors (7x7 stems)

// index along one axis of the gathered tensor for filter tap `tap`, or 0xffffffff if the tap falls outside.
// Forward modes: p = output coordinate.  Backward modes: base = p + pad (or the padded-grid index of the mirror
// image of p for the fused reflect gradient; base_ok = false if there is none).
template <int MODE>
__device__ __forceinline__ unsigned axis_entry(int p, int base, bool base_ok, int tap, int n, int sl, int pad) {
    int i;
    bool ok;
    if (MODE == MODE_BWD || MODE == MODE_BWD_REFLECT) {
        const int t = base - tap;
        i = t >> sl;  // divisible by construction of the phase
        ok = base_ok & (t >= 0) & (i < n);
    } else {
        i = (p << sl) - pad + tap;
        if (MODE == MODE_FWD_REFLECT) {
            i = i < 0 ? -i : i;
            i = i >= n ? 2 * (n - 1) - i : i;
            ok = true;
        } else {
            ok = (unsigned)i < (unsigned)n;
        }
    }
    return ok ? (unsigned)i : 0xffffffffu;
}

__device__ __forceinline__ float4 ld_b128s(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// Pixel enumeration of a phase: index -> (image, y, x) on the output grid (row-major, lanes stay coalesced).
__device__ __forceinline__ int refl_inner(int i, int n, int p) { return i == 0 ? 0 : (i == n - 2 * p - 1 ? n - 1 : i + p); }
__device__ __forceinline__ void pix_coord(const IgemmArgs& a, const PhaseArgs& P, int pg, int& n, int& py, int& px) {
    const int HsWs = P.Hs * P.Ws;
    n = pg / HsWs;
    const int rem = pg - n * HsWs;
    const int sy = rem / P.Ws;
    py = P.ymap ? refl_inner(sy, a.Yh, a.pad) : sy * a.ostep + P.fy;
    px = (rem - sy * P.Ws) * a.ostep + P.fx;
}

struct WgradArgs {
    const void* dY;   // [N][M][Ho][Wo], storage type TA
    const void* X;    // [N][Cg][Hg][Wg], storage type TA
    int dtype;
    float* Wp;        // [splits][M][Kp]   (k = tap*Cgp + c)
    int M, Kp, N, Cg, Cgp, Hg, Wg, Ho, Wo;
    int sl, pad, S;
    int magicS;  // ceil(65536 / S): tap / S == (tap * magicS) >> 16 for tap <= 512
    int Ptot, chunks_per_split;
    unsigned x_bytes, dy_bytes;
};

static constexpr unsigned SM_INV = 0x40000000u;  // row/column marker: any sum with it is >= 1 GiB => out of range

// ---- host side ----------------------------------------------------------------------------------------------------------------
static inline int round4(int v) { return (v + 3) & ~3; }
static inline size_t esz(const pcgan_conv_desc* d) { return d->dtype == PCGAN_BF16 ? 2 : 4; }   // bytes per activation element

// launch KERNEL<template arguments..., TA> with TA = the activation storage type `dt` (256 threads, stream `st`)
#define LAUNCH_TA(dt, KERNEL, GRID, ARG, ...)                                                                   \
    do {                                                                                                        \
        if ((dt) == PCGAN_BF16) hipLaunchKernelGGL((KERNEL<__VA_ARGS__, bf16>), GRID, dim3(256), 0, st, ARG);    \
        else hipLaunchKernelGGL((KERNEL<__VA_ARGS__, float>), GRID, dim3(256), 0, st, ARG);                      \
    } while (0)

// ---- the host unit (igemm_conv.hip) for the kernel units ---------------------------------------------------------------------
// record of the last launch launch_igemm decided (pcgan_igemm_last_launch)
void record_launch(int form, int mode, int bm, int bp, int ks, int nphase);
int launch_splitk_reduce(int dtype, hipStream_t st, const float* part, void* y, const float* bias, int ks, size_t out_elems, int M,
                         int HW, int act, float slope);

// ---- the kernel units for the host unit: each picks the instantiation of a launch the host has sized; `mode` is a MODE_* value ----
// fp32 MFMA kernels: a.chunked selects igemm2_kernel<.., 16> (grid2), igemm2_kernel<.., 4> (grid2) or igemm_kernel (grid);
// MODE_BWD_REFLECT exists for a.chunked == 1 only
int launch_igemm_f32(int mode, const IgemmArgs& a, int bm, int bp, dim3 grid, dim3 grid2, hipStream_t st);
// hgemm_kernel, TA = a.dtype (fp32 tensors: the fp16 two-piece form; bf16 tensors: the bf16 form); bm >= 64, no MODE_BWD_REFLECT
int launch_hgemm(int mode, const IgemmArgs& a, int bm, int bp, dim3 grid2, hipStream_t st);
int launch_hgemm_presplit(float* A, int M, int Kp4, const float* rowmax, hipStream_t st);
// a.M <= 4: kernel choice, channel split (into part_ws, if given) and launch; pmax = largest Ptot of the phases
int launch_smallm(int mode, IgemmArgs& a, int pmax, hipStream_t st, float* part_ws, size_t part_bytes);
int launch_transpose4(const float* A, float* At, int M, int Kp, hipStream_t st);
int launch_pack_strip(const float* A, float* Ws, int M, int Cg, int Cgp, int nR, int nS, hipStream_t st);
// weight gradient: number of pixel splits (and the chunks of each) of the kernel launch_wgrad picks; partial sums a.Wp -> dw
int wgrad_splits(const pcgan_conv_desc* d, int* chunks_per_split);
int launch_wgrad(const pcgan_conv_desc* d, const WgradArgs& a, int splits, float* dw, int accumulate, hipStream_t st);

}  // namespace pcgan
