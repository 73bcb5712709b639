// Helper kernels around the GEMM kernels of the piece-split family: the weight packs (forward image, the data gradient's row
// classes), the padded copy of an input, the pack of dy as an A operand and the fixed-order sum of split partial sums.  They stand
// for no call of the reference of their own: the packs run once per optimizer step (pcgan_conv2d_bsplit_pack, _dgrad_pack,
// _hsplit_pack), the copies and the sum inside the weight gradients (pcgan_conv2d_bwd_weight_bsplit / _hsplit).  Called from the
// host unit, bf16x6_conv.hip, through the launchers at the end of each section (declared in bsplit.h).
#include "bsplit.h"

namespace pcgan {

// weights w[M][C][R][S] -> [piece][mt][stage][half][BM][8] bf16 (BM = 128 << bm_shift), stage = chunk * T + tap, k in stage =
// channel in chunk
// np = 2: two fp16 pieces of w[m][..] * pow2_scale(rowmax[m]) (the fp16 route: ONE power of two per output row, so that a filter
// row far below the tensor's largest weight keeps its 22 bits -- the epilogue divides row m by the same power)
__global__ void bsplit_pack_kernel(const float* __restrict__ w, __bf16* __restrict__ A, int M, int C, int T, int nMt, int nst,
                                   int bm_shift, int np, const float* __restrict__ rowmax = nullptr) {
    const int BM = 128 << bm_shift;
    const size_t per_piece = (size_t)nMt * nst * 16 * BM;
    // a thread builds one 16-byte entry (8 consecutive channels of a row and tap) of every piece: 8 loads in flight, one store per piece
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < per_piece / 8; e += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(e & (BM - 1)), half = (int)((e >> (7 + bm_shift)) & 1);
        const size_t q = e >> (8 + bm_shift);
        const int st = (int)(q % nst), mt = (int)(q / nst);
        const int m = mt * BM + row, c0 = (st / T) * 16 + half * 8, tap = st % T;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = m < M ? w[((size_t)m * C + c0 + j) * T + tap] : 0.f;
        const float wscale = (np == 2 && m < M) ? pow2_scale(rowmax[m]) : 1.f;
        pack_store8(A, e, per_piece, np, wscale, v);
    }
}

int launch_bsplit_pack(const float* w, void* packed, int M, int C, int T, int nMt, int nst, int bm, int np, const float* rowmax, hipStream_t st) {
    const size_t per_piece = (size_t)nMt * nst * 16 * bm;
    hipLaunchKernelGGL(bsplit_pack_kernel, dim3(capped_blocks(per_piece / 8, 256, 4096)), dim3(256), 0, st, w, (__bf16*)packed, M, C, T, nMt, nst,
                       bm == 256 ? 1 : 0, np, rowmax);      // 8 values per thread
    PCGAN_LAUNCH_CHECK();
    return 0;
}

// data-gradient weights of the reflect-padded 3x3 convolution: A[phase][piece][mt][stage][half][BM][8], rows = input channels c,
// k = (16-chunk of output channels, tap (r', s'), channel), value = wf[c][k][r'][s'] = w[k][c][2-r'][2-s'] with the row mirror
// folded in: row class 1 (row 1) reads row 0 through tap r'=0 for itself AND for padded row -1: wf'[0] = wf[0] + wf[2];
// row class 2 (row H-2): wf'[2] = wf[2] + wf[0].
// nphase = 1: only row class 0, the plain flipped weights (all the window kernel reads)
__global__ void bsplit_pack_dgrad_kernel(const float* __restrict__ w, __bf16* __restrict__ A, int K, int C, int nMt, int nst, int bm_shift,
                                         int np, const float* __restrict__ rowmax = nullptr, int nphase = 3) {
    const int BM = 128 << bm_shift;      // (rowmax: per INPUT channel c -- the rows of the data gradient -- as in bsplit_pack_kernel)
    const size_t per_piece = (size_t)nMt * nst * 16 * BM, per_phase = (size_t)np * per_piece;
    // (nphase row classes x per_piece / 8 entries of 8 values; each entry writes its np pieces.  A folded row-class weight is at most
    // twice the largest weight: still far inside the fp16 range)
    const size_t per_phase8 = per_piece / 8;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)nphase * per_phase8; i += (size_t)gridDim.x * blockDim.x) {
        const int phase = (int)(i / per_phase8);
        const size_t e = i - (size_t)phase * per_phase8;
        const int row = (int)(e & (BM - 1)), half = (int)((e >> (7 + bm_shift)) & 1);
        const size_t q = e >> (8 + bm_shift);
        const int st = (int)(q % nst), mt = (int)(q / nst);
        const int c = mt * BM + row, k0 = (st / 9) * 16 + half * 8, tap = st % 9;
        const int rp = tap / 3, sp = tap - rp * 3;
        const bool fold = (phase == 1 && rp == 0) || (phase == 2 && rp == 2);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[j] = 0.f;
            if (c < C) {
                const float* wk = w + ((size_t)(k0 + j) * C + c) * 9;
                v[j] = wk[(2 - rp) * 3 + (2 - sp)];
                if (fold) v[j] += wk[rp * 3 + (2 - sp)];   // + wf[2 - rp][sp]
            }
        }
        const float wscale = (np == 2 && c < C) ? pow2_scale(rowmax[c]) : 1.f;
        pack_store8(A + (size_t)phase * per_phase, e, per_piece, np, wscale, v);
    }
}

int launch_bsplit_pack_dgrad(const float* w, void* packed, int K, int C, int nMt, int nst, int bm, int np, const float* rowmax, int nphase,
                             hipStream_t st) {
    const size_t total = (size_t)nphase * nMt * nst * 2 * bm;      // 16-byte entries of the row classes
    hipLaunchKernelGGL(bsplit_pack_dgrad_kernel, dim3(capped_blocks(total, 256, 4096)), dim3(256), 0, st, w, (__bf16*)packed, K, C, nMt, nst,
                       bm == 256 ? 1 : 0, np, rowmax, nphase);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

// ---- weight gradient as the same GEMM with the roles turned: rows = output channels k (operand A = dy, re-split per call), columns
// = (c, r, s), reduction = (n, y, x) in stages of 16 consecutive x.  The reflection padding is materialised once (xpad), so that
// the gather address is separable: column part (c, r, s) in the lane's offset, reduction part (n, y, x) in the scalar offset.
template <typename TA>
__global__ void bsplit_pad_reflect_kernel(const TA* __restrict__ x, TA* __restrict__ xp, int H, int W, int pad, int reflect = 1) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const TA* src = x + (size_t)blockIdx.y * H * W;
    TA* dst = xp + (size_t)blockIdx.y * Hp * Wp;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Hp * Wp; i += gridDim.x * blockDim.x) {
        int y = i / Wp - pad, xx = i % Wp - pad;
        if (!reflect) {      // zero padding
            const bool in = (unsigned)y < (unsigned)H && (unsigned)xx < (unsigned)W;
            TA v;
            st1(&v, 0.f);
            dst[i] = in ? src[y * W + xx] : v;
            continue;
        }
        y = y < 0 ? -y : (y >= H ? 2 * (H - 1) - y : y);
        xx = xx < 0 ? -xx : (xx >= W ? 2 * (W - 1) - xx : xx);
        dst[i] = src[y * W + xx];
    }
}

// the same copy for small planes (the residual blocks: 8192 planes of 34 x 34): one WAVE per plane, a lane writes PAIRS of neighbouring
// elements (padded width even: a pair never leaves its row, every pair is 8- / 4-byte aligned), row / column advanced without
// a division.  The element-per-thread form above spent its time in 40960 workgroups of one element per thread (0.030 ms).
template <typename TA>
__global__ void __launch_bounds__(256) bsplit_pad_wave_kernel(const TA* __restrict__ x, TA* __restrict__ xp, int planes, int H, int W, int pad, int reflect) {
    const int lane = threadIdx.x & 63;
    const int plane = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const int Hp = H + 2 * pad, Wp = W + 2 * pad, half = Wp >> 1;
    const TA* src = x + (size_t)plane * H * W;
    TA* dst = xp + (size_t)plane * Hp * Wp;
    int row = lane / half, cp = lane - row * half;
    const int drow = 64 / half, dcp = 64 - drow * half;
    typedef TA pair_t __attribute__((ext_vector_type(2)));
    while (row < Hp) {
        int y = row - pad, x0 = 2 * cp - pad, x1 = x0 + 1;
        bool in0 = (unsigned)y < (unsigned)H, in1 = in0;
        if (reflect) {
            y = y < 0 ? -y : (y >= H ? 2 * (H - 1) - y : y);
            x0 = x0 < 0 ? -x0 : (x0 >= W ? 2 * (W - 1) - x0 : x0);
            x1 = x1 < 0 ? -x1 : (x1 >= W ? 2 * (W - 1) - x1 : x1);
            in0 = in1 = true;
        } else {
            in0 = in0 && (unsigned)x0 < (unsigned)W;
            in1 = in1 && (unsigned)x1 < (unsigned)W;
        }
        TA zero;
        st1(&zero, 0.f);
        pair_t v;
        v.x = in0 ? src[y * W + x0] : zero;
        v.y = in1 ? src[y * W + x1] : zero;
        *reinterpret_cast<pair_t*>(dst + row * Wp + 2 * cp) = v;
        cp += dcp;
        row += drow;
        if (cp >= half) {
            cp -= half;
            ++row;
        }
    }
}

int pad_copy_form(int planes, int H, int W, int pad) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    return (Wp % 2 == 0 && Wp <= 128 && Hp * Wp <= 8192 && planes >= 1024) ? 2 : 1;
}

int launch_pad(const void* x, void* xpad, int planes, int H, int W, int pad, int reflect, bool half, hipStream_t st) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    if (pad_copy_form(planes, H, W, pad) == 2) {
        const dim3 grid((planes + 3) / 4);
        if (half) hipLaunchKernelGGL(bsplit_pad_wave_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)x, (bf16*)xpad, planes, H, W, pad, reflect);
        else hipLaunchKernelGGL(bsplit_pad_wave_kernel<float>, grid, dim3(256), 0, st, (const float*)x, (float*)xpad, planes, H, W, pad, reflect);
        PCGAN_LAUNCH_CHECK();
        return 0;
    }
    const dim3 pgrid((Hp * Wp + 255) / 256, planes);
    if (half) hipLaunchKernelGGL(bsplit_pad_reflect_kernel<bf16>, pgrid, dim3(256), 0, st, (const bf16*)x, (bf16*)xpad, H, W, pad, reflect);
    else hipLaunchKernelGGL(bsplit_pad_reflect_kernel<float>, pgrid, dim3(256), 0, st, (const float*)x, (float*)xpad, H, W, pad, reflect);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

// dy[N][K][HW] -> [piece][stage][half][BM][8] bf16 pieces, stage = 16 consecutive elements of the (n, y, x) reduction
template <typename TA>
__global__ void bsplit_pack_dy_kernel(const TA* __restrict__ dy, __bf16* __restrict__ A, int K, int HW, int nst, int bm_shift, int np) {
    const int BM = 128 << bm_shift;
    const size_t per_piece = (size_t)nst * 16 * BM;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < per_piece; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7), row = (int)((i >> 3) & (BM - 1)), half = (int)((i >> (10 + bm_shift)) & 1);
        const size_t st = i >> (11 + bm_shift);
        const size_t e = st * 16 + half * 8 + j;
        const size_t n = e / HW, r = e - n * HW;
        const float v = row < K ? ld1(dy + (n * K + row) * HW + r) : 0.f;
        __bf16 h, mm, l;
        split3(v, h, mm, l);
        A[i] = h;
        if (np == 3) {
            A[per_piece + i] = mm;
            A[2 * per_piece + i] = l;
        }
    }
}

int launch_pack_dy(const void* dy, void* packed, int K, int HW, int nst, int bm, int np, bool half, hipStream_t st) {
    const size_t per_piece = (size_t)nst * 16 * bm;
    const dim3 grid(capped_blocks(per_piece, 256, 8192));
    if (half) hipLaunchKernelGGL(bsplit_pack_dy_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)dy, (__bf16*)packed, K, HW, nst, bm == 256 ? 1 : 0, np);
    else hipLaunchKernelGGL(bsplit_pack_dy_kernel<float>, grid, dim3(256), 0, st, (const float*)dy, (__bf16*)packed, K, HW, nst, bm == 256 ? 1 : 0, np);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

// dw[i] (+)= sum over the splits in a fixed order
__global__ void bsplit_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int splits, size_t total, int accumulate) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= total) return;
    float a0 = 0.f, a1 = 0.f;
    int sp = 0;
    for (; sp + 1 < splits; sp += 2) {
        a0 += part[(size_t)sp * total + i];
        a1 += part[(size_t)(sp + 1) * total + i];
    }
    if (sp < splits) a0 += part[(size_t)sp * total + i];
    const float v = a0 + a1;
    dw[i] = accumulate ? dw[i] + v : v;
}

int launch_wgrad_reduce(const float* part, float* dw, int splits, size_t total, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(bsplit_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, dw, splits, total, accumulate);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace pcgan
