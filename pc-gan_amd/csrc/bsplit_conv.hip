// Stride-1 convolution forward -- and the data and weight gradients of the reflection-padded 3x3 convolution -- on the bf16
// matrix pipe, in two precisions that share one kernel skeleton (template parameters NP = pieces per operand, TA = storage):
//   NP = 3, TA = float  fp32 tensors, fp32-level accuracy (the default route of the residual-block convolutions, below);
//   NP = 1, TA = bf16   the bf16 path (desc.dtype = PCGAN_BF16): activations stored as bf16, weights rounded to bf16 by the
//                       pack kernel, ONE product per term, fp32 accumulators -- plain mixed precision, 6x fewer MFMAs.
//
// An fp32 value is the exact sum of three bf16 pieces, x = h + m + l (8 + 8 + 8 significand bits).  A product a*b then needs
// the piece pairs (h,h) | (h,m) (m,h) | (h,l) (m,m) (l,h) to keep every term above 2^-24 |a||b|; everything is accumulated in
// the fp32 accumulators of v_mfma_f32_32x32x16_bf16.  scripts/micro/bf16_split measures, for K = 2304 (the residual-block
// convolution): relative L2 error 7.0e-7 against float64, fp32 MFMA 6.1e-7; sustained rate of the six instructions that stand
// for one fp32 K = 16 step 304 TFLOP/s fp32-equivalent against 155 TFLOP/s of v_mfma_f32_32x32x2_f32.  This kernel: 0.171-0.179 ms
// on the residual convolution (fp32 implicit GEMM: 0.269 ms).
//
// Replaces the same call sites as the fp32 implicit GEMM (nn.ReflectionPad2d + nn.Conv2d of the ResnetBlocks,
// models/networks.py:621-648; stride-1 nn.Conv2d elsewhere) when the gathered channel count is a multiple of 16.
//
// Y[m][pix] = sum_k A[m][k] * G(k, pix), K ordered (16-channel chunk, tap, channel).  Workgroup = 128 output channels x 128
// pixels, 4 waves of 64 x 64 (2 x 2 accumulators), one K stage = 16 channels of one tap:
//   weights  pre-split by the pack kernel, stored [piece][M tile][stage][k half][128 rows][8 bf16]: a stage is 3 coalesced
//            16-byte loads per thread that go to LDS unchanged;
//   pixels   8 channels of one pixel per thread (lanes along pixels: coalesced), split into the three pieces in registers,
//            three 16-byte LDS writes;
//   LDS      [piece][k half][row or pixel][8 bf16]: every access 16 bytes, 16 consecutive lanes = 256 contiguous bytes;
//   per wave and stage 12 ds_read_b128 and 24 MFMAs (smallest terms first); global loads run three stages ahead, the LDS reads
//   of the next stage sit under the MFMAs of the current one (operands double-buffered in registers), one barrier per stage.
//
// The per-tap gather kernel of the family: it runs PCGAN_SPLIT=bf16 and the bf16 tensors on the shapes the window kernel
// (halo_conv.hip) refuses, the data gradient through three row classes, and the weight gradient of pcgan_conv2d_bwd_weight_bsplit.
// Called from the host unit, bf16x6_conv.hip, through launch_bsplit (bsplit.h); the packed weights come from bsplit_pack.hip.
#include "bsplit.h"

namespace pcgan {

// BM = 128: 4 waves, two workgroups per CU, each thread gathers 8 channels of its pixel per stage.
// BM = 256: 8 waves (4 x 2 of 64 x 64) share ONE gathered / split pixel tile for all 256 output channels: half the gathers, split
//           arithmetic and pixel LDS writes per MFMA; each thread gathers 4 channels; one workgroup per CU.
template <int MODE, int BM, int NP, typename TA>
__global__ void __launch_bounds__(BM * 2) bsplit_conv_fwd_kernel(BsplitArgs a) {
    static_assert((NP == 3 && sizeof(TA) == 4) || (NP == 1 && sizeof(TA) == 2), "3 pieces of fp32 tensors, or bf16 tensors as they are");
    constexpr unsigned ES = sizeof(TA);
    constexpr bool REFLECT = MODE == BS_FWD_REFLECT;
    constexpr bool DGRAD = MODE == BS_DGRAD_REFLECT;
    constexpr bool WGRAD = MODE == BS_WGRAD;
    constexpr int NT = BM * 2;              // threads
    constexpr int KB = 2048 / NT;           // channels of one pixel a thread gathers per stage (8 or 4)
    constexpr unsigned ASTAGE = BM * 32;    // bytes of one stage of one piece of the weights
    __shared__ __attribute__((aligned(16))) bf16x8 As[2][NP][2 * BM];   // [buffer][piece][half * BM + row]
    __shared__ __attribute__((aligned(16))) bf16x8 Bs[2][NP][256];      // [buffer][piece][half * 128 + pixel]
    __shared__ unsigned offT[BS_MAXTAP][128];

    const int tid = threadIdx.x;
    const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wp = wave & 1;
    const int mt = blockIdx.x % a.nMt;
    int pt = blockIdx.x / a.nMt;
    int phase = 0;
    if (DGRAD) {
        phase = (pt >= a.tstart[1]) + (pt >= a.tstart[2]);
        pt -= a.tstart[phase];
    }
    const int Hs = DGRAD ? (phase == 0 ? a.H - 2 : 1) : a.P;      // rows per image of this phase's pixel list
    const int T = a.R * a.S, PQ = WGRAD ? a.C * T : Hs * a.Q, Ptot = WGRAD ? PQ : a.N * PQ;
    const int Hp = a.H + 2 * a.pad, Wp = a.W + 2 * a.pad;          // WGRAD: padded planes of xpad
    const int HW4 = a.H * a.W * (int)ES;      // bytes of one channel plane
    const int pl = tid & 127;
    const int kq = __builtin_amdgcn_readfirstlane(tid >> 7);      // which KB-channel slice of the 16-channel stage
    const int half = (kq * KB) >> 3;

    // gather offsets (bytes, channel 0) of this workgroup's 128 pixels for every tap
    {
        const int pg = pt * 128 + pl;
        const bool pv = pg < Ptot;
        const int n = pv ? pg / PQ : 0, rem = pv ? pg - n * PQ : 0;
        int py = rem / a.Q;
        const int px = rem - py * a.Q;
        if (DGRAD) py = phase == 0 ? (py == 0 ? 0 : (py == Hs - 1 ? a.H - 1 : py + 1)) : (phase == 1 ? 1 : a.H - 2);
        const unsigned nbase = (unsigned)n * (unsigned)a.C * (unsigned)(a.H * a.W);
        if (WGRAD) {   // column (c, r, s) -> offset of xpad[0][c][r][s]; the reduction part comes through the scalar offset
            const int c = pg / T, tap = pg - c * T, r = tap / a.S, sx = tap - r * a.S;
            if (kq == 0) offT[0][pl] = pv ? (unsigned)((c * Hp + r) * Wp + sx) * ES : BS_OOB;
        }
        for (int t = kq; !WGRAD && t < T; t += NT / 128) {
            const int r = t / a.S, s = t - r * a.S;
            int iy = py - a.pad + r, ix = px - a.pad + s;
            bool ok = pv;
            if (REFLECT) {
                iy = iy < 0 ? -iy : iy;
                iy = iy >= a.H ? 2 * (a.H - 1) - iy : iy;
                ix = ix < 0 ? -ix : ix;
                ix = ix >= a.W ? 2 * (a.W - 1) - ix : ix;
            } else {
                ok = ok & ((unsigned)iy < (unsigned)a.H) & ((unsigned)ix < (unsigned)a.W);
            }
            offT[t][pl] = ok ? (nbase + (unsigned)(iy * a.W + ix)) * ES : BS_OOB;
            if (DGRAD) {   // column mirror: column 1 also receives padded column -1 (source column 0 through tap s'=2), column W-2 padded column W
                const int ix2 = (px == 1 && s == 2) ? 0 : ((px == a.W - 2 && s == 0) ? a.W - 1 : -1);
                const bool ok2 = pv & (ix2 >= 0) & ((unsigned)iy < (unsigned)a.H);
                offT[9 + t][pl] = ok2 ? (nbase + (unsigned)(iy * a.W + ix2)) * ES : BS_OOB;
            }
        }
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.X), 0, (int)a.x_bytes, 0x00020000);
    // one activation element: its fp32 value -- except on the one-piece route without mirror sums (RAW), where the stored
    // bf16 pattern goes to LDS as it is (zero-extended here, truncated again in stash: no shift, no conversion instruction)
    constexpr bool RAW = NP == 1 && !DGRAD;
    auto ldx = [&](unsigned voff, unsigned soff) -> float {
        if constexpr (ES == 4) return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rX, voff, soff, 0));
        else if constexpr (RAW) return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rX, voff, soff, 0));
        else return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rX, voff, soff, 0) << 16);
    };
    const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.A), 0, (int)a.a_bytes, 0x00020000);
    const unsigned piece_bytes = (unsigned)a.nMt * (unsigned)a.nst * ASTAGE;
    const unsigned a_tile = (DGRAD ? (unsigned)phase * a.phase_bytes : 0u) + (unsigned)mt * (unsigned)a.nst * ASTAGE;

    struct Stage {
        u32x4 ap[NP];
        float b[KB];
        float b2[DGRAD ? KB : 1];     // column-mirror source (two lanes per image row are in range)
    };
    const int nst_here = WGRAD ? min(a.nst_split, a.nst - (int)blockIdx.y * a.nst_split) : a.nst;
    const int st0 = WGRAD ? (int)blockIdx.y * a.nst_split : 0;
    auto load = [&](Stage& r, int s) {
        const bool live = s < nst_here;
        const int gs = st0 + (live ? s : 0);
        const unsigned avo = live ? (unsigned)tid * 16u : BS_OOB;
        const unsigned aso = a_tile + (unsigned)gs * ASTAGE;
#pragma unroll
        for (int p = 0; p < NP; ++p) r.ap[p] = __builtin_amdgcn_raw_buffer_load_b128(rA, avo, aso + p * piece_bytes, 0);
        if (WGRAD) {   // 16 consecutive x of image n, row y: scalar offset of xpad[n][0][y][x0], the thread's KB values are consecutive
            const int e0 = gs * 16, hw = a.H * a.W;
            const int n = e0 / hw, rem = e0 - n * hw, y = rem / a.W, x0 = rem - y * a.W;
            const unsigned bvo = live ? offT[0][pl] : BS_OOB;
            const unsigned bso = (unsigned)(((n * a.C) * Hp + y) * Wp + x0 + kq * KB) * ES;
#pragma unroll
            for (int j = 0; j < KB; ++j) r.b[j] = ldx(bvo, bso + j * ES);
            return;
        }
        const int cc = gs / T, tap = gs - cc * T;
        const unsigned bvo = live ? offT[tap][pl] : BS_OOB;
        const unsigned bso = live ? (unsigned)(cc * 16 + kq * KB) * (unsigned)HW4 : 0u;
#pragma unroll
        for (int j = 0; j < KB; ++j) r.b[j] = ldx(bvo, bso + j * HW4);
        if (DGRAD) {
            const unsigned bvo2 = live ? offT[9 + tap][pl] : BS_OOB;
#pragma unroll
            for (int j = 0; j < KB; ++j) r.b2[j] = ldx(bvo2, bso + j * HW4);
        }
    };
    auto stash = [&](const Stage& r, int buf) {
#pragma unroll
        for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x4*>(&As[buf][p][tid]) = r.ap[p];
        typedef __bf16 bfv __attribute__((ext_vector_type(KB)));
        bfv h, m, l;
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const float v = DGRAD ? r.b[j] + r.b2[j] : r.b[j];
            if constexpr (NP == 3) {
                __bf16 x, y, z;
                split3(v, x, y, z);
                h[j] = x;
                m[j] = y;
                l[j] = z;
            } else if constexpr (RAW) {
                h[j] = __builtin_bit_cast(__bf16, (unsigned short)__float_as_uint(v));
            } else {
                h[j] = (__bf16)v;      // the mirror sum of the data gradient is rounded once
            }
        }
        // this thread's KB consecutive k of pixel pl: offset (kq * KB) % 8 inside the pixel's 8-wide half
        const int sub = (kq * KB) & 7;
        *reinterpret_cast<bfv*>(reinterpret_cast<__bf16*>(&Bs[buf][0][half * 128 + pl]) + sub) = h;
        if constexpr (NP == 3) {
            *reinterpret_cast<bfv*>(reinterpret_cast<__bf16*>(&Bs[buf][1][half * 128 + pl]) + sub) = m;
            *reinterpret_cast<bfv*>(reinterpret_cast<__bf16*>(&Bs[buf][2][half * 128 + pl]) + sub) = l;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    struct Operands {
        bf16x8 A[NP][2], B[NP][2];
    };
    auto fetch = [&](Operands& o, int buf) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                o.A[p][i] = As[buf][p][hi * BM + wm * 64 + i * 32 + lo];
                o.B[p][i] = Bs[buf][p][hi * 128 + wp * 64 + i * 32 + lo];
            }
    };
    auto mma = [&](const Operands& o) {
        // smallest terms first: (l,h) (h,l) (m,m) | (m,h) (h,m) | (h,h); the four accumulators take turns, so consecutive
        // MFMAs are independent
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int q = (NP == 3 ? 0 : 5); q < 6; ++q)       // one piece: only the (h, h) product
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o.A[PA[q]][i], o.B[PB[q]][j], acc[i][j], 0, 0, 0);
    };

    // Software pipeline, stage pair unrolled so that every register set is static:
    //   global loads run three stages ahead of the MFMAs (two register sets r0 / r1),
    //   LDS holds stages s+1 and s+2 while the MFMAs of stage s run out of registers (two operand sets),
    //   so the LDS reads of the next stage and the writes of the one after sit under the matrix instructions; one barrier per stage.
    // An odd stage count is rounded up: dead stages load zeros (out-of-range offsets) and add nothing.
    Stage r0, r1;
    Operands oa, ob;
    load(r0, 0);
    load(r1, 1);
    stash(r0, 0);
    __syncthreads();
    load(r0, 2);
    fetch(oa, 0);
    stash(r1, 1);
    __syncthreads();
    load(r1, 3);
    const int nst2 = (nst_here + 1) & ~1;
    // issue order inside a stage (a hint the scheduler follows where dependences allow): every MFMA is followed by its share of
    // the other work -- LDS reads of the next stage first, then the split arithmetic and LDS writes of the stage after, then the
    // global loads three stages ahead (0.178 -> 0.171 ms)
    auto interleave = [&]() {
        if constexpr (NP == 3) {
#pragma unroll
            for (int q = 0; q < 24; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                 // one MFMA
                if (q < 12) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);     // one LDS read
                __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                 // two VALU
                if (q >= 12 && q < 18) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // one LDS write
                if (q >= 14 && q < 14 + 3 + KB) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // one global load
            }
        } else {   // 4 MFMAs per stage: one LDS read, then the two LDS writes / the global loads behind each of them
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                if (q < 2) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, (1 + KB * (DGRAD ? 2 : 1) + 3) / 4, 0);
            }
        }
    };
    for (int s = 0; s < nst2; s += 2) {
        fetch(ob, 1);         // operands of stage s+1
        mma(oa);              // stage s
        stash(r0, 0);         // stage s+2 -> buffer 0 (its stage s was read before the last barrier)
        load(r0, s + 4);
        interleave();
        __syncthreads();
        fetch(oa, 0);         // operands of stage s+2
        mma(ob);              // stage s+1
        stash(r1, 1);         // stage s+3 -> buffer 1
        load(r1, s + 5);
        interleave();
        __syncthreads();
    }

    // epilogue: acc[i][j][r] = Y[m0 + wm*64 + i*32 + (r/4)*8 + hi*4 + r%4][pixel wp*64 + j*32 + lo]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int pg = pt * 128 + wp * 64 + j * 32 + lo;
        if (pg >= Ptot) continue;
        const int n = pg / PQ;
        int rem = pg - n * PQ;
        if (DGRAD) {
            const int sy = rem / a.Q, x = rem - sy * a.Q;
            const int y = phase == 0 ? (sy == 0 ? 0 : (sy == Hs - 1 ? a.H - 1 : sy + 1)) : (phase == 1 ? 1 : a.H - 2);
            rem = y * a.Q + x;
        }
        const int PQo = WGRAD ? PQ : a.P * a.Q;
        const size_t yo = (WGRAD ? (size_t)blockIdx.y : (size_t)n) * a.M * PQo + rem;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * BM + wm * 64 + i * 32 + (r >> 2) * 8 + hi * 4 + (r & 3);
                if (m < a.M) {
                    const float v = act_apply(acc[i][j][r] + (a.bias ? a.bias[m] : 0.f), a.act, a.slope);
                    if constexpr (WGRAD) ((float*)a.Y)[yo + (size_t)m * PQo] = v;      // fp32 partial sums
                    else st1((TA*)a.Y + yo + (size_t)m * PQo, v);
                }
            }
    }
}

// bsplit_conv_fwd_kernel<MODE, BM, NP, TA> for the tile / storage type at hand
template <int MODE>
static void launch_mode(int dtype, int bm, dim3 grid, hipStream_t st, const BsplitArgs& a) {
    if (dtype == PCGAN_BF16) {
        if (bm == 256) hipLaunchKernelGGL((bsplit_conv_fwd_kernel<MODE, 256, 1, bf16>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((bsplit_conv_fwd_kernel<MODE, 128, 1, bf16>), grid, dim3(256), 0, st, a);
    } else {
        if (bm == 256) hipLaunchKernelGGL((bsplit_conv_fwd_kernel<MODE, 256, 3, float>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((bsplit_conv_fwd_kernel<MODE, 128, 3, float>), grid, dim3(256), 0, st, a);
    }
}

int launch_bsplit(int mode, int dtype, int bm, dim3 grid, const BsplitArgs& a, hipStream_t st) {
    switch (mode) {
        case BS_FWD_ZERO: launch_mode<BS_FWD_ZERO>(dtype, bm, grid, st, a); break;
        case BS_FWD_REFLECT: launch_mode<BS_FWD_REFLECT>(dtype, bm, grid, st, a); break;
        case BS_DGRAD_REFLECT: launch_mode<BS_DGRAD_REFLECT>(dtype, bm, grid, st, a); break;
        case BS_WGRAD: launch_mode<BS_WGRAD>(dtype, bm, grid, st, a); break;
        default: PCGAN_CHECK(false, "bsplit: no kernel for mode %d", mode);
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace pcgan
