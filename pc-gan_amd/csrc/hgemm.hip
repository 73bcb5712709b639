// The packed implicit GEMM on the f16 / bf16 matrix pipe (hgemm_kernel), the pre-split of its packed weights, and their launchers.
// Shared gathers, argument structs and tap arithmetic: igemm.h.
#include "igemm.h"

namespace pcgan {

// ------------------------------------------------------------------------------------
// fp16 two-piece form of the chunked-K kernel (fp32 tensors; forward with zero / reflection padding and the plain data gradient,
// any stride, <= 25 taps, channel count a multiple of 16): the same gather tables, K order, phases and split-K as igemm2_kernel,
// but both operands are scaled by a power of two and split into two fp16 pieces on their way to LDS (x * 2^e = h + l, common.h
// pow2_scale / split2h) and a 16-deep K stage is THREE v_mfma_f32_32x32x16_f16 per 32 x 32 block -- (l,h) (h,l) (h,h) -- instead of
// eight v_mfma_f32_32x32x2_f32.  Measured error at the fp32 kernel's level (scripts/micro/bf16_split: 5.3e-7 at K = 2304, fp32
// MFMA 6.1e-7).  a.x_amax[0 .. x_namax) are partial maxima of |X| (device), a.w_amax the largest |weight|.
//   LDS images [piece][k half][row or pixel][8 fp16]: every operand read is one conflict-free ds_read_b128;
//   per wave and stage (128 x 128 tile): 12 MFMA, 8 LDS reads; weights 2 x 16-byte loads, pixels 8 x 4-byte gathers per thread;
//   global loads two stages ahead in registers, LDS one stage ahead, operands of the next stage read under this stage's MFMAs.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// TA = bf16 (the bf16 path, desc.dtype = PCGAN_BF16): the stored bf16 activations go to LDS as they are, the fp32 weights are rounded
// to bf16 on their way there, ONE v_mfma_f32_32x32x16_bf16 per block and stage, no scaling -- plain mixed precision as in the
// one-product form of the residual-convolution kernels (halo_conv.hip, hsplit_wgrad.hip).
typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4v __attribute__((ext_vector_type(4)));

template <int MODE, int BM, int BP, typename TA>
__global__ void __launch_bounds__(256) hgemm_kernel(IgemmArgs a) {
    static_assert(MODE == MODE_FWD_ZERO || MODE == MODE_FWD_REFLECT || MODE == MODE_BWD, "forward and plain data gradient");
    constexpr bool HALF = sizeof(TA) == 2;      // bf16 tensors: one piece, one product
    constexpr int NP = HALF ? 1 : 2;
    constexpr unsigned ES = sizeof(TA);
    constexpr int WM = (BM == 128 || (BM == 64 && BP == 64)) ? 2 : 1;
    constexpr int WP = 4 / WM;
    constexpr int WMT = BM / WM, WPT = BP / WP;
    constexpr int MI = WMT / 32, PJ = WPT / 32;
    constexpr int KPT = BP / 16;        // channels of its pixel a thread gathers per stage (8 or 4)
    constexpr int ACH = BM * 4 / 256;   // float4 of the weight tile per thread (2 or 1)
    constexpr int TROWS = NTAP_FWD + 1; // + one all-out-of-range row for dead stages
    // four neighbouring lanes write the two k halves of one weight row: 128 bytes of padding between the halves put them on disjoint banks
    constexpr int AH = BM + 8;
    __shared__ __attribute__((aligned(16))) f16x8 As[2][NP][2 * AH];     // [buffer][piece][k half * AH + row]
    __shared__ __attribute__((aligned(16))) f16x8 Bs[2][NP][2 * BP];     // [buffer][piece][k half * BP + pixel]
    __shared__ unsigned offT[TROWS][BP];
    __shared__ __attribute__((aligned(16))) float biasS[BM];
    __shared__ __attribute__((aligned(16))) float iswS[BM];     // fp16 route: 1 / (the power of two row m0 + i of the weights was scaled by)

    const int nMt = (a.M + BM - 1) / BM;
    const int mt = blockIdx.x % nMt;
    int pt = blockIdx.x / nMt;
    int phase = 0;
    while (phase + 1 < a.nphase && pt >= a.tstart[phase + 1]) ++phase;
    pt -= a.tstart[phase];
    const PhaseArgs& P = a.ph[phase];
    const int tid = threadIdx.x;
    const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WP, wp = wave % WP;
    const int Ptot = P.Ptot, Kp = P.Kp;
    const int m0 = mt * BM, p0 = pt * BP;
    const int ph_nS = P.nS;
    const int T = P.nR * ph_nS;
    const int HgWg4 = a.Hg * a.Wg * (int)ES;     // bytes of one channel plane
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.X, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rA = make_rsrc(P.A, (unsigned)a.M * (unsigned)Kp * 4u);

    float sx = 1.f;
    // gather-offset table of this workgroup's BP pixels (as in igemm2_kernel)
    const int pl = tid % BP;
    {
        const int pg = p0 + pl;
        const bool pvalid = pg < Ptot;
        int gn = 0, py = 0, px = 0;
        if (pvalid) pix_coord(a, P, pg, gn, py, px);
        const unsigned vbase = (unsigned)gn * (unsigned)a.Cg * (unsigned)(a.Hg * a.Wg);
        for (int t = tid / BP; t <= T; t += 256 / BP) {
            const int ri = t / ph_nS, sj = t - ri * ph_nS;
            const int r = P.r0 + ri * a.tstep, sxx = P.s0 + sj * a.tstep;
            const bool live = pvalid && t < T;
            const unsigned y = axis_entry<MODE>(py, py + a.pad, true, r, a.Hg, a.sl, a.pad);
            const unsigned x = axis_entry<MODE>(px, px + a.pad, true, sxx, a.Wg, a.sl, a.pad);
            offT[t][pl] = (live && y != 0xffffffffu && x != 0xffffffffu) ? (vbase + y * (unsigned)a.Wg + x) * ES : OOB;
        }
    }
    const int ksub = __builtin_amdgcn_readfirstlane(tid / BP);
    __syncthreads();

    const int nst_all = Kp >> 4;
    const int nst_per = a.ksplit > 1 ? (nst_all + a.ksplit - 1) / a.ksplit : nst_all;
    const int st_begin = a.ksplit > 1 ? (int)blockIdx.z * nst_per : 0;
    const int st_end = st_begin + nst_per < nst_all ? st_begin + nst_per : nst_all;
    const int nst_here = st_end > st_begin ? st_end - st_begin : 0;

    // load-side iterator (scalar): tap, first channel and weight column of the next stage to load
    int it_tap, it_c, it_k0, it_left = nst_here;
    {
        const int cc0 = st_begin / T;
        it_tap = st_begin - cc0 * T;
        it_c = cc0 * 16;
        it_k0 = st_begin * 16;
    }
    unsigned a_base[ACH];
#pragma unroll
    for (int j = 0; j < ACH; ++j) {
        const int q = tid + 256 * j;
        const int row = q >> 2, kc = (q & 3) * 4;
        a_base[j] = (m0 + row < a.M) ? (unsigned)((m0 + row) * Kp + kc) * 4u : OOB;
    }
    struct Stage {
        u32x4 av[ACH];      // 4 consecutive k of this thread's weight row(s)
        unsigned bv[KPT];   // KPT consecutive channels of this thread's pixel
    };
    auto load = [&](Stage& r) {
        const bool live = it_left > 0;
        const unsigned vo = offT[live ? it_tap : T][pl];
        const unsigned so = (unsigned)((it_c + ksub * KPT) * HgWg4);
#pragma unroll
        for (int j = 0; j < ACH; ++j) r.av[j] = __builtin_amdgcn_raw_buffer_load_b128(rA, live ? a_base[j] : OOB, (unsigned)it_k0 * 4u, 0);
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            if constexpr (HALF) r.bv[i] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rX, vo, so + (unsigned)(i * HgWg4), 0);
            else r.bv[i] = __builtin_amdgcn_raw_buffer_load_b32(rX, vo, so + (unsigned)(i * HgWg4), 0);
        }
        --it_left;
        const int t1 = it_tap + 1;
        const bool wr = t1 == T;
        it_tap = wr ? 0 : t1;
        it_c += wr ? 16 : 0;
        it_k0 += 16;
    };
    auto stash = [&](const Stage& r, int buf) {
        if constexpr (HALF) {
#pragma unroll
            for (int j = 0; j < ACH; ++j) {
                const int q = tid + 256 * j;
                const int row = q >> 2, kc = (q & 3) * 4;
                bf16x4v h;
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = (__bf16)__uint_as_float(r.av[j][e]);      // weights: round to nearest even
                *reinterpret_cast<bf16x4v*>(reinterpret_cast<__bf16*>(&As[buf][0][(kc >> 3) * AH + row]) + (kc & 4)) = h;
            }
            typedef unsigned short usK __attribute__((ext_vector_type(KPT)));
            usK v;
#pragma unroll
            for (int e = 0; e < KPT; ++e) v[e] = (unsigned short)r.bv[e];                     // stored bf16 patterns as they are
            if constexpr (KPT == 8) *reinterpret_cast<usK*>(&Bs[buf][0][ksub * BP + pl]) = v;
            else *reinterpret_cast<usK*>(reinterpret_cast<unsigned short*>(&Bs[buf][0][(ksub >> 1) * BP + pl]) + (ksub & 1) * 4) = v;
            return;
        }
        // the weights arrive PRE-SPLIT (pcgan_conv2d_hgemm_pack: they only change once per optimizer step while every net runs 2-4
        // times in between): the 16 bytes a thread loaded are [4 x fp16 high pieces | 4 x fp16 low pieces] of 4 consecutive k of its
        // row, scaled by the same power of two the epilogue divides by -- two 8-byte LDS stores, no arithmetic
#pragma unroll
        for (int j = 0; j < ACH; ++j) {
            const int q = tid + 256 * j;
            const int row = q >> 2, kc = (q & 3) * 4;
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            u32x2 h, l;
            h[0] = r.av[j][0]; h[1] = r.av[j][1];
            l[0] = r.av[j][2]; l[1] = r.av[j][3];
            _Float16* d0 = reinterpret_cast<_Float16*>(&As[buf][0][(kc >> 3) * AH + row]) + (kc & 4);
            _Float16* d1 = reinterpret_cast<_Float16*>(&As[buf][NP - 1][(kc >> 3) * AH + row]) + (kc & 4);
            *reinterpret_cast<u32x2*>(d0) = h;
            *reinterpret_cast<u32x2*>(d1) = l;
        }
        if constexpr (KPT == 8) {
            f16x8 h, l;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                _Float16 x, y;
                split2h(__uint_as_float(r.bv[e]) * sx, x, y);
                h[e] = x;
                l[e] = y;
            }
            Bs[buf][0][ksub * BP + pl] = h;
            Bs[buf][NP - 1][ksub * BP + pl] = l;
        } else {
            f16x4 h, l;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                _Float16 x, y;
                split2h(__uint_as_float(r.bv[e]) * sx, x, y);
                h[e] = x;
                l[e] = y;
            }
            *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(&Bs[buf][0][(ksub >> 1) * BP + pl]) + (ksub & 1) * 4) = h;
            *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(&Bs[buf][NP - 1][(ksub >> 1) * BP + pl]) + (ksub & 1) * 4) = l;
        }
    };

    f32x16 acc[MI][PJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < PJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    struct Operands {
        f16x8 A[NP][MI], B[NP][PJ];
    };
    auto fetch = [&](Operands& o, int buf) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int i = 0; i < MI; ++i) o.A[p][i] = As[buf][p][hi * AH + wm * WMT + i * 32 + lo];
#pragma unroll
            for (int j = 0; j < PJ; ++j) o.B[p][j] = Bs[buf][p][hi * BP + wp * WPT + j * 32 + lo];
        }
    };
    auto mma = [&](const Operands& o) {      // (l,h) (h,l) (h,h): smallest terms first
        if constexpr (HALF) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < PJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8v, o.A[0][i]), __builtin_bit_cast(bf16x8v, o.B[0][j]),
                                                                         acc[i][j], 0, 0, 0);
            return;
        }
        constexpr int PA[3] = {NP - 1, 0, 0}, PB[3] = {0, NP - 1, 0};
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < PJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(o.A[PA[q]][i], o.B[PB[q]][j], acc[i][j], 0, 0, 0);
    };
    auto interleave = [&]() {
        constexpr int NM = (HALF ? 1 : 3) * MI * PJ, NRD = NP * (MI + PJ);
#pragma unroll
        for (int q = 0; q < NM; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                            // one MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, (NRD + NM - 1) / NM, 0);          // LDS reads of the next stage first
            __builtin_amdgcn_sched_group_barrier(0x002, 48 / NM + 1, 0);                  // split arithmetic
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                            // LDS writes
            __builtin_amdgcn_sched_group_barrier(0x020, (ACH + KPT + NM - 1) / NM, 0);    // global loads
        }
    };

    Stage rg[2];
    if (nst_here > 0) {      // the first two stages' global loads go out before the scale reduction below (their latency covers it)
        load(rg[0]);
        load(rg[1]);
    }
    // operand scales: the largest of the partial maxima the producer of X left; the weights were scaled ROW BY ROW by the pack call
    // (a.w_amax[m] = largest magnitude of row m), the epilogue divides each row by its own power of two
    if constexpr (!HALF) {
        const float m = thread_max_of_partials(a.x_amax, a.x_namax, tid, 256);
        sx = pow2_scale(block_max(m, biasS));
        if (tid < BM) iswS[tid] = m0 + tid < a.M ? 1.f / pow2_scale(a.w_amax[m0 + tid]) : 1.f;
        __syncthreads();      // (biasS was the reduction's scratch)
    }
    if (tid < BM) biasS[tid] = (a.bias != nullptr && m0 + tid < a.M) ? a.bias[m0 + tid] : 0.f;
    if (nst_here == 0) __syncthreads();      // (with stages, the barriers below order biasS before the epilogue)
    if (nst_here > 0) {
        Operands op[2];
        stash(rg[0], 0);
        __syncthreads();
        load(rg[0]);
        fetch(op[0], 0);
        stash(rg[1], 1);
        __syncthreads();
        load(rg[1]);
        const int nst2 = (nst_here + 1) & ~1;      // an odd count is rounded up: the dead stage gathered zeros
        for (int s = 0; s < nst2; s += 2) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fetch(op[t ^ 1], t ^ 1);           // operands of stage s+t+1
                mma(op[t]);                        // stage s+t
                stash(rg[t], t);                   // stage s+t+2
                load(rg[t]);                       // stage s+t+4
                interleave();
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    // epilogue (as igemm2_kernel): scale back (powers of two: exact), bias + activation or raw partial sum of a K split
    const float isx = 1.f / sx;
    const int YhYw = a.Yh * a.Yw;
    bool bad = false;
    if constexpr (!HALF) {       // (before the ragged-tile `continue`s below: every lane of the wave takes part in the ballot)
#pragma unroll
        for (int j = 0; j < PJ; ++j)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) bad |= is_nonfinite(acc[i][j][r]);
        report_nonfinite(a.ovf, bad);
    }
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        const int pix = p0 + wp * WPT + j * 32 + lo;
        if (pix >= Ptot) continue;
        int n, oy, ox;
        pix_coord(a, P, pix, n, oy, ox);
        if (a.ksplit > 1) {
            float* Yp = a.Ypart + ((size_t)blockIdx.z * a.N + n) * a.M * YhYw + oy * a.Yw + ox;
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ml = wm * WMT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const int m = m0 + ml;
                    if (m < a.M) Yp[(size_t)m * YhYw] = (acc[i][j][r] * isx) * (HALF ? 1.f : iswS[ml]);
                }
            continue;
        }
        TA* Yp = (TA*)a.Y + (size_t)n * a.M * YhYw + oy * a.Yw + ox;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = wm * WMT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (m0 + ml < a.M) st1(Yp + (size_t)(m0 + ml) * YhYw, act_apply((acc[i][j][r] * isx) * (HALF ? 1.f : iswS[ml]) + biasS[ml], a.act, a.slope));
            }
    }
}

// 3 modes x 4 tiles x 2 storage types
template <int MODE>
static void launch_mode(const IgemmArgs& a, int bm, int bp, dim3 grid2, hipStream_t st) {
    if (bm == 128 && bp == 128) LAUNCH_TA(a.dtype, hgemm_kernel, grid2, a, MODE, 128, 128);
    else if (bm == 128) LAUNCH_TA(a.dtype, hgemm_kernel, grid2, a, MODE, 128, 64);
    else if (bp == 128) LAUNCH_TA(a.dtype, hgemm_kernel, grid2, a, MODE, 64, 128);
    else LAUNCH_TA(a.dtype, hgemm_kernel, grid2, a, MODE, 64, 64);
}
int launch_hgemm(int mode, const IgemmArgs& a, int bm, int bp, dim3 grid2, hipStream_t st) {
    switch (mode) {
        case MODE_FWD_ZERO: launch_mode<MODE_FWD_ZERO>(a, bm, bp, grid2, st); break;
        case MODE_FWD_REFLECT: launch_mode<MODE_FWD_REFLECT>(a, bm, bp, grid2, st); break;
        case MODE_BWD: launch_mode<MODE_BWD>(a, bm, bp, grid2, st); break;
        default: PCGAN_CHECK(false, "hgemm: no kernel for mode %d", mode);
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace pcgan

using namespace pcgan;

// in-place pre-split of one packed fp32 weight matrix A[M][Kp] for hgemm_kernel: every aligned group of 4 consecutive floats of row m
// (what one thread feeds to LDS per stage) becomes [4 fp16 high pieces][4 fp16 low pieces] of the values scaled by
// pow2_scale(rowmax[m]) -- one power of two per ROW, so a filter row far below the tensor's largest weight keeps its 22 bits
__global__ void __launch_bounds__(256) hgemm_presplit_kernel(float* __restrict__ A, int M, int Kp4, const float* __restrict__ rowmax) {
    const size_t n4 = (size_t)M * Kp4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float s = pow2_scale(rowmax[i / Kp4]);
        const float4 v = reinterpret_cast<const float4*>(A)[i];
        f16x4 h, l;
        _Float16 x, y;
        split2h(v.x * s, x, y); h[0] = x; l[0] = y;
        split2h(v.y * s, x, y); h[1] = x; l[1] = y;
        split2h(v.z * s, x, y); h[2] = x; l[2] = y;
        split2h(v.w * s, x, y); h[3] = x; l[3] = y;
        reinterpret_cast<f16x4*>(A)[2 * i] = h;
        reinterpret_cast<f16x4*>(A)[2 * i + 1] = l;
    }
}

int pcgan::launch_hgemm_presplit(float* A, int M, int Kp4, const float* rowmax, hipStream_t st) {
    hipLaunchKernelGGL(hgemm_presplit_kernel, dim3(capped_blocks((size_t)M * Kp4, 256, 2048)), dim3(256), 0, st, A, M, Kp4, rowmax);
    PCGAN_LAUNCH_CHECK();
    return 0;
}
