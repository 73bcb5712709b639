// Inception-v3 feature network for FID (forward only, fp32 tensors).  Replaces the torchvision blocks the reference's
// models/inception.py takes from inception_v3(pretrained=True): BasicConv2d (Conv2d(bias=False) + eval BatchNorm2d(eps=0.001) + ReLU),
// the branch pools of InceptionA..E, and the input resize + normalisation of its forward.
//
//   iconv          implicit GEMM on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): rows = output channels, columns = output pixels
//                  (n, p, q), reduction over (c, r, s).  Per-axis zero padding, stride 1 or 2, R != S.  The epilogue adds the folded
//                  bias, applies ReLU and writes channel slice [k_off, k_off + K) of an NCHW output with K_total channels (each branch of
//                  a Mixed block lands in its slice: no concatenation pass).
//   iconv_pack     folds eval BatchNorm into weight and bias in fp32 and writes the kernel's layout: bias[Kpad], then W^T[CRSpad][Kpad].
//                  With pool_expand a 1x1 weight becomes the 3x3 pad-1 weight with every tap w / 9: avg_pool2d(3, 1, 1,
//                  count_include_pad=True) followed by a 1x1 conv is exactly that linear map.
//   maxpool_slice  max pool (no padding, floor mode) into a channel slice (the InceptionB / D pool branches).
//   inception_prep bilinear resize (align_corners=False, ATen's source-index rule) + per-channel affine, one pass.
//   linear_fwd + softmax_rows   the classifier head of the Inception Score: nn.Linear on the exact-fp32 MFMA, then a row softmax.
#include "common.h"
#include <float.h>

namespace pcgan {
namespace {

constexpr int IC_BM = 64;    // output channels per workgroup (2 waves x 32)
constexpr int IC_BN = 128;   // output pixels per workgroup (2 waves x 2 x 32)
constexpr int IC_BK = 16;    // reduction rows per stage (8 MFMA k-steps of 2)
constexpr int IC_THREADS = 256;

// unsigned division by a runtime constant d >= 1, exact for n < 2^31: q = (umulhi(n, m) + n) >> l (Granlund-Montgomery)
struct FastDiv {
    uint32_t m, l;
};
static FastDiv make_fastdiv(uint32_t d) {
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    const uint64_t m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
    return FastDiv{(uint32_t)m, l};
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, FastDiv f) { return (__umulhi(n, f.m) + n) >> f.l; }

struct IconvArgs {
    const float* x;
    const float* packed;   // bias[Kpad] then W^T[CRSpad][Kpad]
    float* y;
    int C, H, W, K, S, RS, stride, pad_h, pad_w, P, Q, k_off, K_total, Kpad, CRS, CRSpad, NPQ, relu;
    FastDiv fd_rs, fd_s;
};

typedef float f32x16 __attribute__((ext_vector_type(16)));

// 256 threads: wave (wm, wn) computes output channels m0 + 32 wm .. + 31 x pixels n0 + 64 wn .. + 63 (two 32 x 32 accumulators).
// Per stage of 16 reduction rows the workgroup stages A (16 x 64, one float4 per thread from the packed weights) and B (16 x 128,
// eight gathered pixels per thread) in LDS; the next stage's global loads are issued before this stage's MFMAs.
__global__ void __launch_bounds__(IC_THREADS) iconv_fwd_kernel(IconvArgs a) {
    __shared__ float As[IC_BK][IC_BM + 4];
    __shared__ float Bs[IC_BK][IC_BN + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int m0 = blockIdx.y * IC_BM;
    const int n0 = blockIdx.x * IC_BN;
    const int HW = a.H * a.W, PQ = a.P * a.Q;

    // this thread's gather column (one output pixel) and its first row (wave-uniform: rows brow + 2 i)
    const int bcol = tid & (IC_BN - 1);
    const int brow = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int pix = n0 + bcol;
    int ih0 = -(1 << 20), iw0 = 0;   // a column past the end: every tap fails the bounds test, nothing is read
    const float* xp = a.x;
    if (pix < a.NPQ) {
        const int n = pix / PQ, pq = pix - n * PQ;
        const int p = pq / a.Q, q = pq - p * a.Q;
        ih0 = p * a.stride - a.pad_h;
        iw0 = q * a.stride - a.pad_w;
        xp = a.x + (size_t)n * a.C * HW;
    }
    // this thread's weight float4: stage row akk, channels m0 + am .. + 3 (Kpad and CRSpad are whole tiles: always in bounds)
    const int akk = tid >> 4, am = (tid & 15) * 4;
    const float* wt = a.packed + a.Kpad;

    float4 areg;
    float breg[IC_BK / 2];
    auto load_stage = [&](int kb) {
        areg = *reinterpret_cast<const float4*>(wt + (size_t)(kb + akk) * a.Kpad + m0 + am);
#pragma unroll
        for (int i = 0; i < IC_BK / 2; ++i) {
            const int kr = kb + brow + 2 * i;     // wave-uniform: the (c, r, s) decode runs on the scalar unit
            float v = 0.f;
            if (kr < a.CRS) {
                const int c = (int)fdiv((uint32_t)kr, a.fd_rs);
                const int rs = kr - c * a.RS;
                const int r = (int)fdiv((uint32_t)rs, a.fd_s);
                const int s = rs - r * a.S;
                const int ih = ih0 + r, iw = iw0 + s;
                if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W) v = xp[(size_t)c * HW + ih * a.W + iw];
            }
            breg[i] = v;
        }
    };

    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;

    const int arow = lane >> 5, acol = lane & 31;   // 32x32x2 operands: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
    load_stage(0);
    for (int kb = 0; kb < a.CRSpad; kb += IC_BK) {
        As[akk][am + 0] = areg.x;
        As[akk][am + 1] = areg.y;
        As[akk][am + 2] = areg.z;
        As[akk][am + 3] = areg.w;
#pragma unroll
        for (int i = 0; i < IC_BK / 2; ++i) Bs[brow + 2 * i][bcol] = breg[i];
        __syncthreads();
        if (kb + IC_BK < a.CRSpad) load_stage(kb + IC_BK);
        // blocked summation: the stage's 16 products go into fresh accumulators, which are then added to the running sums.  One
        // fma chain over the whole reduction (up to 4032 terms here) was measured at 2.2x torch's fp32 CPU error for C = 1280 1x1
        // convolutions; chains of 16 + CRS / 16 terms stay well inside it, for two vector adds per stage
        f32x16 p0 = {}, p1 = {};
#pragma unroll
        for (int kk = 0; kk < IC_BK; kk += 2) {
            const float av = As[kk + arow][wm * 32 + acol];
            const float b0 = Bs[kk + arow][wn * 64 + acol];
            const float b1 = Bs[kk + arow][wn * 64 + 32 + acol];
            p0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, p0, 0, 0, 0);
            p1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, p1, 0, 0, 0);
        }
        acc0 += p0;
        acc1 += p1;
        __syncthreads();
    }

    // epilogue: register i of lane l holds row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31
    const float* bias = a.packed;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int j = n0 + wn * 64 + t * 32 + acol;
        if (j >= a.NPQ) continue;
        const int n = j / PQ, pq = j - n * PQ;
        float* yp = a.y + ((size_t)n * a.K_total + a.k_off) * PQ + pq;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int k = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * arow;
            if (k >= a.K) continue;
            float v = (t == 0 ? acc0[i] : acc1[i]) + bias[k];
            if (a.relu) v = v > 0.f ? v : 0.f;
            yp[(size_t)k * PQ] = v;
        }
    }
}

// one thread per element of W^T[CRSpad][Kpad]; row 0's threads also write bias[k]
__global__ void iconv_pack_kernel(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                  const float* __restrict__ mean, const float* __restrict__ var, float eps, int K, int C, int RS,
                                  int pool_expand, int Kpad, int CRSpad, float* __restrict__ packed) {
    const size_t total = (size_t)CRSpad * Kpad;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int kr = (int)(e / Kpad), k = (int)(e - (size_t)kr * Kpad);
        float scale = 1.f, shift = 0.f;
        if (k < K && gamma) {
            scale = gamma[k] / sqrtf(var[k] + eps);
            shift = beta[k] - mean[k] * scale;
        }
        if (kr == 0) packed[k] = k < K ? shift : 0.f;
        float v = 0.f;
        if (k < K && kr < C * RS) {
            if (pool_expand) v = (w[(size_t)k * C + kr / 9] * scale) / 9.f;
            else v = w[(size_t)k * C * RS + kr] * scale;
        }
        packed[Kpad + e] = v;
    }
}

// one thread per output element of [N][C][P][Q], written to channel k_off + c of a K_total-channel output
__global__ void maxpool_slice_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int H, int W, int k, int stride,
                                     int P, int Q, int k_off, int K_total, size_t total) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t nc = e / ((size_t)P * Q);
        const int me = (int)(e - nc * P * Q);
        const int n = (int)(nc / C), c = (int)(nc - (size_t)n * C);
        const int p = me / Q, q = me - p * Q;
        const float* w0 = x + nc * H * W + (size_t)(p * stride) * W + q * stride;
        float best = w0[0];
        for (int r = 0; r < k; ++r)
            for (int s = 0; s < k; ++s) {
                const float v = w0[r * W + s];
                if (v > best || v != v) best = v;   // NaN propagates, as torch's max_pool2d
            }
        y[((size_t)n * K_total + k_off + c) * P * Q + me] = best;
    }
}

// ATen's area_pixel_compute_source_index (align_corners=False, clamped at 0) + guard_index_and_lambda, fp32.  This file is compiled with
// -ffp-contract=off (Makefile), so the fused steps are explicit: ATen's CPU kernels are built with contraction (measured: the unfused
// source index puts a pixel's lambda one rounding away and the result up to 3e-6 off), the normalisation is two separate torch ops
__device__ __forceinline__ void prep_src(int dst, float ratio, int in_size, int& i0, int& i1, float& l0, float& l1) {
    float src = fmaf(ratio, (float)dst + 0.5f, -0.5f);
    if (src < 0.f) src = 0.f;
    i0 = (int)floorf(src);
    if (i0 > in_size - 1) i0 = in_size - 1;
    const float l = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = l;
    l0 = 1.f - l;
}

// one thread per output element of [N][3][OH][OW]; rows first, then columns, as ATen's separable CPU loop
__global__ void inception_prep_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int OH, int OW, float rh,
                                      float rw, int affine, float s0, float s1, float s2, float t0, float t1, float t2, size_t total) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t nc = e / ((size_t)OH * OW);
        const int me = (int)(e - nc * OH * OW);
        const int c = (int)(nc % 3);
        const int p = me / OW, q = me - p * OW;
        int y0, y1, x0, x1;
        float hy0, hy1, wx0, wx1;
        prep_src(p, rh, H, y0, y1, hy0, hy1);
        prep_src(q, rw, W, x0, x1, wx0, wx1);
        const float* xp = x + nc * H * W;
        const float u0 = fmaf(xp[y0 * W + x1], wx1, xp[y0 * W + x0] * wx0);     // ATen: out = t0 * w0; out += t1 * w1
        const float u1 = fmaf(xp[y1 * W + x1], wx1, xp[y1 * W + x0] * wx0);
        float v = fmaf(u1, hy1, u0 * hy0);
        if (affine) {
            const float sc = c == 0 ? s0 : (c == 1 ? s1 : s2), sh = c == 0 ? t0 : (c == 1 ? t1 : t2);
            v = v * sc + sh;
        }
        y[e] = v;
    }
}

static inline int ew_grid(size_t n) {
    const size_t b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

// ---- classifier head: logits = x W^T + b, probs = softmax(logits, dim=1) --------------------------------------------------------------
// The op is bound by W (8 MB at K = 1000, C = 2048), not by its arithmetic, so one workgroup owns a tile of LS_KT classes and a batch
// tile of LS_NB rows and reads its W tile once for all of them.  The four waves split the reduction: wave w takes the 16-wide chunks
// w, w + 4, w + 8, ... of C (exact-fp32 v_mfma_f32_16x16x4_f32, a k-ordered fma chain), and the four partial sums meet in LDS, added in
// wave order.  No atomics: every result has one fixed summation order, whatever runs beside it.
constexpr int LS_KT = 16;        // classes per workgroup (the MFMA's 16 columns)
constexpr int LS_NB = 64;        // rows per workgroup (four 16-row MFMA tiles)
constexpr int LS_WAVES = 4;
constexpr int LS_THREADS = 64 * LS_WAVES;
constexpr int SM_THREADS = 256;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// 4 consecutive elements row[c .. c + 3], zeros past C or for a row outside the tensor; vec: 16-byte loads (C % 4 == 0, aligned rows)
__device__ __forceinline__ float4 ls_load4(const float* __restrict__ row, bool row_ok, int c, int C, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row_ok || c >= C) return v;
    if (vec) return *reinterpret_cast<const float4*>(row + c);
    v.x = row[c];
    if (c + 1 < C) v.y = row[c + 1];
    if (c + 2 < C) v.z = row[c + 2];
    if (c + 3 < C) v.w = row[c + 3];
    return v;
}

__global__ void __launch_bounds__(LS_THREADS) linear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ b, float* __restrict__ y, int N, int C,
                                                                int K, int vec) {
    __shared__ float part[LS_WAVES][LS_NB * LS_KT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k0 = blockIdx.x * LS_KT, n0 = blockIdx.y * LS_NB;
    const int col = lane & 15, kq = (lane >> 4) * 4;   // operand lanes: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]
    const bool vec4 = vec != 0;

    const bool w_ok = k0 + col < K;
    const float* wrow = w + (size_t)(w_ok ? k0 + col : 0) * C;
    const float* xrow[LS_NB / 16];
    bool x_ok[LS_NB / 16];
#pragma unroll
    for (int s = 0; s < LS_NB / 16; ++s) {
        const int n = n0 + 16 * s + col;
        x_ok[s] = n < N;
        xrow[s] = x + (size_t)(x_ok[s] ? n : 0) * C;
    }

    f32x4 acc[LS_NB / 16];
#pragma unroll
    for (int s = 0; s < LS_NB / 16; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};

    // lane l holds elements c0 + kq .. + 3 of its rows; MFMA t multiplies element t, so the four k slots of one instruction are
    // c0 + t, c0 + 4 + t, c0 + 8 + t, c0 + 12 + t (A and B alike)
    for (int c0 = 16 * wave; c0 < C; c0 += 16 * LS_WAVES) {
        const float4 wv = ls_load4(wrow, w_ok, c0 + kq, C, vec4);
        float4 xv[LS_NB / 16];
#pragma unroll
        for (int s = 0; s < LS_NB / 16; ++s) xv[s] = ls_load4(xrow[s], x_ok[s], c0 + kq, C, vec4);
#pragma unroll
        for (int s = 0; s < LS_NB / 16; ++s) {
            acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].x, wv.x, acc[s], 0, 0, 0);
            acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].y, wv.y, acc[s], 0, 0, 0);
            acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].z, wv.z, acc[s], 0, 0, 0);
            acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[s].w, wv.w, acc[s], 0, 0, 0);
        }
    }

    // D[i][j]: lane l, register r holds row (l >> 4) * 4 + r, column l & 15
#pragma unroll
    for (int s = 0; s < LS_NB / 16; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][(16 * s + kq + r) * LS_KT + col] = acc[s][r];
    __syncthreads();
    for (int e = tid; e < LS_NB * LS_KT; e += LS_THREADS) {
        const int n = n0 + e / LS_KT, k = k0 + e % LS_KT;
        if (n >= N || k >= K) continue;
        float v = part[0][e];
#pragma unroll
        for (int q = 1; q < LS_WAVES; ++q) v += part[q][e];
        if (b) v += b[k];
        y[(size_t)n * K + k] = v;
    }
}

// one workgroup per row: p = exp(l - max) / sum, full-precision expf, the sum in a fixed order (each thread's elements in index order,
// then the wave butterfly, then the waves in order).  src may be dst (the logits were staged in the probability buffer).
__global__ void __launch_bounds__(SM_THREADS) softmax_rows_kernel(const float* src, float* dst, int K) {
    __shared__ float scratch[SM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* l = src + (size_t)blockIdx.x * K;
    float* p = dst + (size_t)blockIdx.x * K;
    float m = -INFINITY;
    for (int i = tid; i < K; i += SM_THREADS) m = fmaxf(m, l[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) scratch[wave] = m;
    __syncthreads();
    m = scratch[0];
#pragma unroll
    for (int q = 1; q < SM_THREADS / 64; ++q) m = fmaxf(m, scratch[q]);
    float s = 0.f;
    for (int i = tid; i < K; i += SM_THREADS) s += expf(l[i] - m);
    s = block_sum(s, scratch);     // barrier first: every thread has read the row maximum from scratch
    for (int i = tid; i < K; i += SM_THREADS) p[i] = expf(l[i] - m) / s;
}

}  // namespace

// geometry check shared by the queries and the launches; sets the error text
static bool iconv_geometry_ok(const pcgan_iconv_desc* d) {
    if (!d) {
        set_error("iconv: null descriptor");
        return false;
    }
    if (d->dtype != PCGAN_F32) {
        set_error("iconv: fp32 tensors only (dtype %d: the Inception kernels have no bf16 form)", d->dtype);
        return false;
    }
    if (d->N <= 0 || d->C <= 0 || d->H <= 0 || d->W <= 0 || d->K <= 0 || d->R <= 0 || d->S <= 0) {
        set_error("iconv: non-positive size (N %d C %d H %d W %d K %d R %d S %d)", d->N, d->C, d->H, d->W, d->K, d->R, d->S);
        return false;
    }
    if (d->stride != 1 && d->stride != 2) {
        set_error("iconv: stride %d unsupported (1 or 2)", d->stride);
        return false;
    }
    if (d->R > 7 || d->S > 7 || d->pad_h < 0 || d->pad_w < 0 || d->pad_h >= d->R || d->pad_w >= d->S) {
        set_error("iconv: kernel %dx%d with padding (%d, %d) unsupported (R, S <= 7, 0 <= pad < kernel)", d->R, d->S, d->pad_h, d->pad_w);
        return false;
    }
    if (d->H + 2 * d->pad_h < d->R || d->W + 2 * d->pad_w < d->S) {
        set_error("iconv: kernel %dx%d larger than the padded %dx%d input", d->R, d->S, d->H + 2 * d->pad_h, d->W + 2 * d->pad_w);
        return false;
    }
    const int P = (d->H + 2 * d->pad_h - d->R) / d->stride + 1, Q = (d->W + 2 * d->pad_w - d->S) / d->stride + 1;
    if (d->P != P || d->Q != Q) {
        set_error("iconv: output dims %dx%d do not match (expected %dx%d)", d->P, d->Q, P, Q);
        return false;
    }
    if (d->k_off < 0 || d->K_total < d->k_off + d->K) {
        set_error("iconv: channel slice [%d, %d) outside an output of %d channels", d->k_off, d->k_off + d->K, d->K_total);
        return false;
    }
    if ((double)d->N * P * Q + IC_BN >= 2147483647.0 || (double)d->C * d->H * d->W >= 2147483647.0 ||
        (double)d->C * d->R * d->S >= 1048576.0 || (double)d->K + IC_BM >= 65535.0 * IC_BM) {
        set_error("iconv: problem too large for the kernel's 32-bit pixel / reduction indices");
        return false;
    }
    return true;
}

static inline int iconv_kpad(const pcgan_iconv_desc* d) { return (d->K + IC_BM - 1) / IC_BM * IC_BM; }
static inline int iconv_crspad(const pcgan_iconv_desc* d) { return (d->C * d->R * d->S + IC_BK - 1) / IC_BK * IC_BK; }

}  // namespace pcgan

using namespace pcgan;

extern "C" int pcgan_iconv_supported(const pcgan_iconv_desc* d) { return iconv_geometry_ok(d) ? 1 : 0; }

extern "C" size_t pcgan_iconv_packed_bytes(const pcgan_iconv_desc* d) {
    if (!iconv_geometry_ok(d)) return 0;
    const size_t kpad = iconv_kpad(d), crspad = iconv_crspad(d);
    return (kpad + crspad * kpad) * sizeof(float);
}

extern "C" int pcgan_iconv_pack(const pcgan_iconv_desc* d, int pool_expand, const float* w, const float* gamma, const float* beta,
                                const float* mean, const float* var, float eps, void* packed, pcgan_stream_t s) {
    if (!iconv_geometry_ok(d)) return 1;
    PCGAN_CHECK(w && packed, "iconv_pack: null weight / packed buffer");
    const bool bn = gamma != nullptr;
    PCGAN_CHECK(bn == (beta != nullptr) && bn == (mean != nullptr) && bn == (var != nullptr),
                "iconv_pack: the BatchNorm parameters (gamma, beta, mean, var) are all given or all NULL");
    PCGAN_CHECK(!bn || eps > 0.f, "iconv_pack: eps must be positive");
    PCGAN_CHECK(!pool_expand || (d->R == 3 && d->S == 3 && d->pad_h == 1 && d->pad_w == 1 && d->stride == 1),
                "iconv_pack: pool_expand takes the descriptor of the expanded 3x3 pad-1 stride-1 convolution (got %dx%d pad (%d, %d) stride %d)",
                d->R, d->S, d->pad_h, d->pad_w, d->stride);
    const int kpad = iconv_kpad(d), crspad = iconv_crspad(d);
    hipLaunchKernelGGL(iconv_pack_kernel, dim3(ew_grid((size_t)crspad * kpad)), dim3(256), 0, (hipStream_t)s, w, gamma, beta, mean, var,
                       eps, d->K, d->C, d->R * d->S, pool_expand ? 1 : 0, kpad, crspad, (float*)packed);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcgan_iconv_fwd(const pcgan_iconv_desc* d, const void* x, const void* packed, void* y, int relu, pcgan_stream_t s) {
    if (!iconv_geometry_ok(d)) return 1;
    PCGAN_CHECK(x && packed && y, "iconv_fwd: null pointer");
    PCGAN_CHECK((reinterpret_cast<size_t>(packed) & 15) == 0, "iconv_fwd: packed weights must be 16-byte aligned");
    IconvArgs a;
    a.x = (const float*)x;
    a.packed = (const float*)packed;
    a.y = (float*)y;
    a.C = d->C; a.H = d->H; a.W = d->W; a.K = d->K; a.S = d->S; a.RS = d->R * d->S;
    a.stride = d->stride; a.pad_h = d->pad_h; a.pad_w = d->pad_w; a.P = d->P; a.Q = d->Q;
    a.k_off = d->k_off; a.K_total = d->K_total;
    a.Kpad = iconv_kpad(d);
    a.CRS = d->C * a.RS;
    a.CRSpad = iconv_crspad(d);
    a.NPQ = d->N * d->P * d->Q;
    a.relu = relu ? 1 : 0;
    a.fd_rs = make_fastdiv((uint32_t)a.RS);
    a.fd_s = make_fastdiv((uint32_t)d->S);
    const dim3 grid((a.NPQ + IC_BN - 1) / IC_BN, a.Kpad / IC_BM);
    hipLaunchKernelGGL(iconv_fwd_kernel, grid, dim3(IC_THREADS), 0, (hipStream_t)s, a);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcgan_maxpool_slice_fwd(const void* x, void* y, int N, int C, int H, int W, int k, int stride, int P, int Q, int k_off,
                                       int K_total, int dtype, pcgan_stream_t s) {
    PCGAN_CHECK(dtype == PCGAN_F32, "maxpool_slice_fwd: fp32 tensors only (dtype %d)", dtype);
    PCGAN_CHECK(x && y && N > 0 && C > 0 && k > 0 && stride > 0 && H >= k && W >= k, "maxpool_slice_fwd: bad arguments");
    PCGAN_CHECK(P == (H - k) / stride + 1 && Q == (W - k) / stride + 1, "maxpool_slice_fwd: output dims do not match (floor mode, no padding)");
    PCGAN_CHECK(k_off >= 0 && K_total >= k_off + C, "maxpool_slice_fwd: channel slice [%d, %d) outside an output of %d channels", k_off,
                k_off + C, K_total);
    const size_t total = (size_t)N * C * P * Q;
    hipLaunchKernelGGL(maxpool_slice_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)s, (const float*)x, (float*)y, C, H, W, k,
                       stride, P, Q, k_off, K_total, total);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcgan_inception_prep(const void* x, void* y, int N, int C, int H, int W, int OH, int OW, const float* scale,
                                    const float* shift, int dtype, pcgan_stream_t s) {
    PCGAN_CHECK(dtype == PCGAN_F32, "inception_prep: fp32 tensors only (dtype %d)", dtype);
    PCGAN_CHECK(x && y && N > 0 && C == 3 && H > 0 && W > 0 && OH > 0 && OW > 0, "inception_prep: bad arguments (RGB images: C == 3)");
    PCGAN_CHECK((scale == nullptr) == (shift == nullptr), "inception_prep: scale and shift are both given or both NULL");
    PCGAN_CHECK((double)H * W < 2147483647.0 && (double)OH * OW < 2147483647.0, "inception_prep: image too large");
    const float rh = (float)H / (float)OH, rw = (float)W / (float)OW;
    const size_t total = (size_t)N * C * OH * OW;
    hipLaunchKernelGGL(inception_prep_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)s, (const float*)x, (float*)y, H, W, OH,
                       OW, rh, rw, scale ? 1 : 0, scale ? scale[0] : 1.f, scale ? scale[1] : 1.f, scale ? scale[2] : 1.f,
                       shift ? shift[0] : 0.f, shift ? shift[1] : 0.f, shift ? shift[2] : 0.f, total);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

extern "C" int pcgan_linear_softmax_fwd(const void* x, const float* w, const float* b, void* logits, void* probs, int N, int C, int K,
                                        int dtype, pcgan_stream_t s) {
    PCGAN_CHECK(dtype == PCGAN_F32, "linear_softmax_fwd: fp32 tensors only (dtype %d)", dtype);
    PCGAN_CHECK(N > 0 && C > 0 && K > 0, "linear_softmax_fwd: non-positive size (N %d C %d K %d)", N, C, K);
    PCGAN_CHECK(x && w && probs, "linear_softmax_fwd: null x / w / probs");
    PCGAN_CHECK((N + LS_NB - 1) / LS_NB <= 65535, "linear_softmax_fwd: N %d too large (at most %d rows)", N, 65535 * LS_NB);
    const size_t addr = reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(w);
    const int vec = (C % 4 == 0 && (addr & 15) == 0) ? 1 : 0;
    // without a logits buffer the logits are staged in probs and the softmax runs in place
    float* lg = logits ? (float*)logits : (float*)probs;
    const dim3 grid((K + LS_KT - 1) / LS_KT, (N + LS_NB - 1) / LS_NB);
    hipLaunchKernelGGL(linear_fwd_kernel, grid, dim3(LS_THREADS), 0, (hipStream_t)s, (const float*)x, w, b, lg, N, C, K, vec);
    PCGAN_LAUNCH_CHECK();
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(N), dim3(SM_THREADS), 0, (hipStream_t)s, (const float*)lg, (float*)probs, K);
    PCGAN_LAUNCH_CHECK();
    return 0;
}
