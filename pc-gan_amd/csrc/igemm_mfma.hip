// fp32-MFMA kernels of the implicit-GEMM convolution (v_mfma_f32_32x32x2_f32, exact f32 fma chain) and their launcher.
// Shared gathers, argument structs and tap arithmetic: igemm.h.  What bounds the kernels: DESIGN.md section 3.
#include "igemm.h"

namespace pcgan {

// Generic-K-order kernel: K ordered (tap, channel) with the channel count padded to 4, so a 16-deep K stage may
// straddle filter taps (3-/4-channel stems, odd channel counts, > 25 taps).  Block tile BM (output channels) x BP
// (pixels), K stage 16, 4 waves, double-buffered LDS, one barrier per stage.  LDS images (all accesses 128-bit):
//   As[row][20]      : 16 k of one output channel per row (+4 floats pad => ds_read_b128 conflict-free)
//   Bs[k/4][pix][4]  : 4 consecutive k of one pixel per 16-byte slot
// The MFMA consumes K in a permuted order (half-wave h takes k = 4*(2q+h)+j in step (q,j)); A and B use the same
// permutation so the sum is unchanged.  The layers that matter for the step time use igemm2_kernel below.
template <int MODE, int BM, int BP, typename TA>
__global__ void __launch_bounds__(256) igemm_kernel(IgemmArgs a) {
    static_assert(MODE != MODE_BWD_REFLECT, "the mirror-gather data gradient exists only in the chunked-K kernel");
    constexpr unsigned ES = sizeof(TA);
    constexpr int WM = (BM == 128 || (BM == 64 && BP == 64)) ? 2 : 1;  // waves along M
    constexpr int WP = 4 / WM;                                         // waves along pixels
    constexpr int WMT = BM / WM, WPT = BP / WP;
    static_assert(WMT % 32 == 0 && WPT % 32 == 0, "wave tile must be a multiple of 32x32");
    constexpr int MI = WMT / 32, PJ = WPT / 32;
    constexpr int AP = 20;
    constexpr int KPT = BP / 16;                 // K slots per thread per stage (8 or 4)
    constexpr int ACH = (BM * 4 + 255) / 256;    // float4 chunks of A per thread
    __shared__ __attribute__((aligned(16))) float As[2][BM * AP];
    __shared__ __attribute__((aligned(16))) float Bs[2][4 * BP * 4];

    const PhaseArgs& P = a.ph[blockIdx.y];
    const int tid = threadIdx.x;
    const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WP, wp = wave % WP;
    const int nMt = (a.M + BM - 1) / BM;
    const int mt = blockIdx.x % nMt, pt = blockIdx.x / nMt;
    const int m0 = mt * BM, p0 = pt * BP;
    const int Ptot = P.Ptot, Kp = P.Kp;
    if (p0 >= Ptot) return;  // phases of unequal size share one grid
    const int ph_r0 = P.r0, ph_s0 = P.s0, ph_nR = P.nR, ph_nS = P.nS, ph_Ws = P.Ws, ph_fy = P.fy, ph_fx = P.fx;

    const Geom g{a.Hg, a.Wg, a.sl, a.pad};
    const int HsWs = P.Hs * ph_Ws;
    const int HgWg = a.Hg * a.Wg;
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.X, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rA = make_rsrc(P.A, (unsigned)a.M * (unsigned)Kp * 4u);

    // --- this thread's gather pixel -------------------------------------------------
    const int pl = tid % BP;
    const int pg = p0 + pl;
    const bool pvalid = pg < Ptot;
    int vbase = 0, py = 0, px = 0;
    if (pvalid) {
        const int gn = pg / HsWs;
        const int rem = pg - gn * HsWs;
        const int sy = rem / ph_Ws;
        py = sy * a.ostep + ph_fy;
        px = (rem - sy * ph_Ws) * a.ostep + ph_fx;
        vbase = gn * a.Cg * HgWg;
    }
    const int ksub = __builtin_amdgcn_readfirstlane(tid / BP);  // which KPT-slice of the stage this wave gathers

    // K-stage range of this workgroup (split-K: small problems are cut along K to fill the 256 CUs)
    const int nst_all = (Kp + 15) / 16;
    const int nst_per = a.ksplit > 1 ? (nst_all + a.ksplit - 1) / a.ksplit : nst_all;
    const int st_begin = a.ksplit > 1 ? (int)blockIdx.z * nst_per : 0;
    const int st_end = st_begin + nst_per < nst_all ? st_begin + nst_per : nst_all;

    KIter it{0, 0, 0};
    it.advance(st_begin * 16 + ksub * KPT, a.Cgp, ph_nS);

    float4 areg[ACH];
    float breg[KPT];
    bool a_ok[ACH];
    unsigned a_off[ACH];
#pragma unroll
    for (int j = 0; j < ACH; ++j) {
        const int q = tid + 256 * j;
        const int row = q >> 2, kc = (q & 3) * 4;
        a_ok[j] = (row < BM) & (m0 + row < a.M);
        a_off[j] = (unsigned)((m0 + row) * Kp + kc) * 4u;
    }

    auto load_stage = [&](int k0) {
#pragma unroll
        for (int j = 0; j < ACH; ++j) {
            const int kc = ((tid + 256 * j) & 3) * 4;
            areg[j] = ld_b128(rA, (a_ok[j] & (k0 + kc < Kp)) ? a_off[j] + (unsigned)k0 * 4u : OOB);
        }
        KIter e = it;
        unsigned voff = OOB;
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            if (i == 0 || e.c == 0) {  // wave-uniform: the tap changed
                voff = OOB;
                if (e.ri < ph_nR) {
                    int off;
                    const bool ok = tap_offset<MODE>(g, py, px, ph_r0 + e.ri * a.tstep, ph_s0 + e.sj * a.tstep, off);
                    voff = (ok && pvalid) ? (unsigned)(vbase + off) * ES : OOB;
                }
            }
            breg[i] = (e.c < a.Cg) ? ldr<TA>(rX, voff, (unsigned)(e.c * HgWg) * ES) : 0.f;
            e.advance(1, a.Cgp, ph_nS);
        }
        it.advance(16, a.Cgp, ph_nS);
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < ACH; ++j) {
            const int q = tid + 256 * j;
            const int row = q >> 2, kc = (q & 3) * 4;
            if (BM * 4 >= 256 || row < BM) *reinterpret_cast<float4*>(&As[buf][row * AP + kc]) = areg[j];
        }
#pragma unroll
        for (int gq = 0; gq < KPT / 4; ++gq)
            put4<TA>(&Bs[buf][((ksub * (KPT / 4) + gq) * BP + pl) * 4], breg[gq * 4 + 0], breg[gq * 4 + 1], breg[gq * 4 + 2], breg[gq * 4 + 3]);
    };

    f32x16 acc[MI][PJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < PJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float av0[MI][4], bv0[PJ][4], av1[MI][4], bv1[PJ][4];
    auto read_ops = [&](int buf, int q, float (&av)[MI][4], float (&bv)[PJ][4]) {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const float4 t = *reinterpret_cast<const float4*>(&As[buf][(wm * WMT + i * 32 + lo) * AP + (2 * q + hi) * 4]);
            av[i][0] = t.x; av[i][1] = t.y; av[i][2] = t.z; av[i][3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < PJ; ++j) {
            const float4 t = *reinterpret_cast<const float4*>(&Bs[buf][((2 * q + hi) * BP + wp * WPT + j * 32 + lo) * 4]);
            bv[j][0] = t.x; bv[j][1] = t.y; bv[j][2] = t.z; bv[j][3] = t.w;
        }
    };
    auto mfma_group = [&](const float (&av)[MI][4], const float (&bv)[PJ][4]) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < PJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][jj], bv[j][jj], acc[i][j], 0, 0, 0);
    };
    if (st_begin < st_end) {  // (empty K range of a split-K tail: accumulators stay zero, stored below)
        if constexpr (sizeof(TA) == 2) {
            zero_tile<TA>(&Bs[0][0], 2 * 4 * BP * 4);
            __syncthreads();
        }
        load_stage(st_begin * 16);
        store_stage(0);
        __syncthreads();
        read_ops(0, 0, av0, bv0);
        for (int st = st_begin; st < st_end; ++st) {
            const int buf = (st - st_begin) & 1;
            const bool more = st + 1 < st_end;
            read_ops(buf, 1, av1, bv1);
            if (more) load_stage((st + 1) * 16);
            mfma_group(av0, bv0);
            mfma_group(av1, bv1);
            if (more) store_stage(buf ^ 1);
            __syncthreads();
            if (more) read_ops(buf ^ 1, 0, av0, bv0);
        }
    }

    // --- epilogue: bias + activation, NCHW store (pixel on the lane -> coalesced) -----
    const int YhYw = a.Yh * a.Yw;
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        const int pix = p0 + wp * WPT + j * 32 + lo;
        if (pix >= Ptot) continue;
        const int n = pix / HsWs;
        const int rem = pix - n * HsWs;
        const int sy = rem / ph_Ws;
        const int oy = sy * a.ostep + ph_fy;
        const int ox = (rem - sy * ph_Ws) * a.ostep + ph_fx;
        if (a.ksplit > 1) {  // raw partial sum; bias / activation happen in splitk_reduce_kernel
            float* Yp = a.Ypart + ((size_t)blockIdx.z * a.N + n) * a.M * YhYw + oy * a.Yw + ox;
#pragma unroll
            for (int i = 0; i < MI; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * WMT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (m < a.M) Yp[(size_t)m * YhYw] = acc[i][j][r];
                }
            }
            continue;
        }
        TA* Yp = (TA*)a.Y + (size_t)n * a.M * YhYw + oy * a.Yw + ox;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * WMT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (m < a.M) {
                    float v = acc[i][j][r];
                    if (a.bias) v += a.bias[m];
                    v = act_apply(v, a.act, a.slope);
                    st1(Yp + (size_t)m * YhYw, v);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// Chunked-K kernel (C % 16 == 0, <= 25 filter taps): the hot kernel of the step.
//
// K order (16-channel chunk, tap, channel-in-chunk): one K stage = 16 channels of ONE filter tap, consecutive
// stages walk the taps of the same 16 channel planes (L2-resident).
//
// What bounds this kernel (measured, scripts/micro/mfma_mix.hip): on one SIMD every vector-ALU, LDS and
// vector-memory instruction issued between two v_mfma costs the matrix pipe ~4-6 cycles -- they do not hide
// under the 64 cycles of a 32x32x2 fp32 MFMA; only scalar instructions are free.  So the loop is written to
// need as few non-scalar instructions per stage as possible:
//   * the gather offset of (pixel, tap) -- padding / reflection / stride arithmetic, validity in bit 31 -- is
//     tabulated once per workgroup in LDS: a stage needs ONE 4-byte LDS read (+1 VALU for its address);
//   * channel and K offsets go through the scalar offset operand of the buffer loads;
//   * the LDS buffer index is a compile-time constant (loop unrolled by two), so every LDS address is a
//     per-thread base register + immediate;
//   * the K iterator lives in SGPRs.
// Per wave and stage (128x128 tile): 32 MFMA, 9 LDS reads, 4 LDS writes, 10 global loads, ~2 VALU.
//
// Pipeline (a wave issues in order and stops at every wait, so each wait must come long after its request):
//     first half of the MFMA chain (operands av0/bv0, already in registers)
//         + LDS reads of this stage's second-half operands av1/bv1
//         + LDS write of stage t+1 (its global loads were issued one stage ago)
//         + global gathers of stage t+2
//     barrier  (stage t+1 is now visible; nobody still reads the buffer written next)
//     second half of the chain (av1/bv1)
//         + LDS reads of stage t+1's first-half operands av0/bv0
//         + offset-table read for the gathers of stage t+3
// so the LDS write -> barrier -> LDS read latency chain of a hand-over sits under matrix instructions instead
// of between two stages.  Two LDS buffers suffice (the buffer written in stage t was last read before the
// barrier of stage t-1).  Stages past the end of the K range are gathered as all-out-of-range (zeros) and
// written to LDS but never consumed.  Source order in the loop IS the issue order (sched_barrier(0) per slot).

// CPS = channels per K stage: 16 (chunked order, channel count a multiple of 16) or 4 (image-like tensors of 3-4 channels,
// K order (tap, channel) with the channels padded to 4: one stage = 4 filter taps x 4 channels, up to 7x7 taps).
template <int MODE, int BM, int BP, int CPS, typename TA>
__global__ void __launch_bounds__(256) igemm2_kernel(IgemmArgs a) {
    constexpr unsigned ES = sizeof(TA);
    constexpr int WM = (BM == 128 || (BM == 64 && BP == 64)) ? 2 : 1;
    constexpr int WP = 4 / WM;
    constexpr int WMT = BM / WM, WPT = BP / WP;
    constexpr int MI = WMT / 32, PJ = WPT / 32;
    constexpr int AP = 20;
    constexpr int KPT = BP / 16;
    constexpr int ACH = (BM * 4 + 255) / 256;
    constexpr bool MIR = MODE == MODE_BWD_REFLECT;
    static_assert(CPS == 16 || (CPS == 4 && !MIR), "4-channel stages: forward and plain data gradient only");
    constexpr int TROWS = (MIR ? NTAP_MIR : (CPS == 4 ? NTAP_CG4 : NTAP_FWD)) + 1;   // + one all-out-of-range row for dead stages
    constexpr int NCOMB = MIR ? 4 : 1;
    __shared__ __attribute__((aligned(16))) float As[2][BM * AP];
    __shared__ __attribute__((aligned(16))) float Bs[2][4 * BP * 4];
    __shared__ unsigned offT[NCOMB][TROWS][BP];
    __shared__ __attribute__((aligned(16))) float biasS[BM];

    const int nMt = (a.M + BM - 1) / BM;
    const int mt = blockIdx.x % nMt;
    int pt = blockIdx.x / nMt;
    int phase = 0;
    while (phase + 1 < a.nphase && pt >= a.tstart[phase + 1]) ++phase;   // grid.x = all phases' tiles back to back
    pt -= a.tstart[phase];
    const PhaseArgs& P = a.ph[phase];
    const int tid = threadIdx.x;
    const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WP, wp = wave % WP;
    const int Ptot = P.Ptot, Kp = P.Kp;
    const int m0 = mt * BM, p0 = pt * BP;
    const int ph_nS = P.nS, ph_Ws = P.Ws, ph_fy = P.fy, ph_fx = P.fx;
    const int T = P.nR * ph_nS;
    const int HsWs = P.Hs * ph_Ws;
    const int HgWg4 = a.Hg * a.Wg * (int)ES;     // bytes of one channel plane
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.X, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rA = make_rsrc(P.A, (unsigned)a.M * (unsigned)Kp * 4u);

    // --- gather-offset table of this workgroup's BP pixels ------------------------------
    const int pl = tid % BP;
    int myr = -1, mxr = -1;
    {
        const int pg = p0 + pl;
        const bool pvalid = pg < Ptot;
        int gn = 0, py = 0, px = 0;
        if (pvalid) pix_coord(a, P, pg, gn, py, px);
        const unsigned vbase = (unsigned)gn * (unsigned)a.Cg * (unsigned)(a.Hg * a.Wg);
        if (MIR && pvalid) {  // padded row j holds input row reflect(j - pad): row py also appears at these padded rows
            if (py >= 1 && py <= a.pad) myr = a.pad - py;
            else if (py >= a.Yh - 1 - a.pad && py <= a.Yh - 2) myr = a.pad + 2 * (a.Yh - 1) - py;
            if (px >= 1 && px <= a.pad) mxr = a.pad - px;
            else if (px >= a.Yw - 1 - a.pad && px <= a.Yw - 2) mxr = a.pad + 2 * (a.Yw - 1) - px;
            if (a.rowfold) myr = -1;   // this phase's weights already carry the row mirror
        }
        for (int t = tid / BP; t <= T; t += 256 / BP) {
            const int ri = t / ph_nS, sj = t - ri * ph_nS;
            const int r = P.r0 + ri * a.tstep, sx = P.s0 + sj * a.tstep;
            const bool live = pvalid && t < T;
            const unsigned y = axis_entry<MODE>(py, py + a.pad, true, r, a.Hg, a.sl, a.pad);
            const unsigned x = axis_entry<MODE>(px, px + a.pad, true, sx, a.Wg, a.sl, a.pad);
            offT[0][t][pl] = (live && y != 0xffffffffu && x != 0xffffffffu) ? (vbase + y * (unsigned)a.Wg + x) * ES : OOB;
            if (MIR) {
                const unsigned yb = axis_entry<MODE>(py, myr, myr >= 0, r, a.Hg, a.sl, a.pad);
                const unsigned xb = axis_entry<MODE>(px, mxr, mxr >= 0, sx, a.Wg, a.sl, a.pad);
                offT[NCOMB > 1 ? 1 : 0][t][pl] = (live && y != 0xffffffffu && xb != 0xffffffffu) ? (vbase + y * (unsigned)a.Wg + xb) * ES : OOB;
                offT[NCOMB > 1 ? 2 : 0][t][pl] = (live && yb != 0xffffffffu && x != 0xffffffffu) ? (vbase + yb * (unsigned)a.Wg + x) * ES : OOB;
                offT[NCOMB > 1 ? 3 : 0][t][pl] = (live && yb != 0xffffffffu && xb != 0xffffffffu) ? (vbase + yb * (unsigned)a.Wg + xb) * ES : OOB;
            }
        }
        if (tid < BM) biasS[tid] = (a.bias != nullptr && m0 + tid < a.M) ? a.bias[m0 + tid] : 0.f;
        zero_tile<TA>(&Bs[0][0], 2 * 4 * BP * 4);     // (published by the barrier in front of the first stage)
    }
    const int ksub = __builtin_amdgcn_readfirstlane(tid / BP);

    const int nst_all = (Kp + 15) >> 4;
    const int nst_per = a.ksplit > 1 ? (nst_all + a.ksplit - 1) / a.ksplit : nst_all;
    const int st_begin = a.ksplit > 1 ? (int)blockIdx.z * nst_per : 0;
    const int st_end = st_begin + nst_per < nst_all ? st_begin + nst_per : nst_all;

    // load-side iterator (scalar; runs two stages ahead of the MFMA chain)
    int it_c, it_tap, it_k0;
    if (CPS == 4) {
        it_tap = st_begin * 4;
        it_c = 0;
    } else {
        const int cc0 = st_begin / T;
        it_tap = st_begin - cc0 * T;
        it_c = cc0 * 16;
    }
    it_k0 = st_begin * 16;
    unsigned a_base[ACH];
#pragma unroll
    for (int j = 0; j < ACH; ++j) {
        const int q = tid + 256 * j;
        const int row = q >> 2, kc = (q & 3) * 4;
        a_base[j] = ((row < BM) & (m0 + row < a.M)) ? (unsigned)((m0 + row) * Kp + kc) * 4u : OOB;
    }

    float4 areg[ACH];
    float breg[KPT];
    float bmir[MIR ? 3 : 1][MIR ? KPT : 1];
    unsigned vo[NCOMB];          // gather offsets of the next load (bit 31 = out of range)
    unsigned vo_b = OOB;         // CPS 4, BP 128: offset of this thread's second filter tap
    int vo_c = 0, vo_k0 = 0;     // channel chunk / A column of the stage `vo` belongs to

    // offset-table read for the stage the iterator points at + iterator advance
    auto next_offsets = [&](auto nm_tag) {
        constexpr int NM = decltype(nm_tag)::value;
        if constexpr (CPS == 4) {   // this thread's KPT K-slots = KPT / 4 consecutive taps x 4 channels
            const int tA = it_tap + ksub * (KPT / 4);
            vo[0] = offT[0][tA < T ? tA : T][pl];
            if (KPT == 8) vo_b = offT[0][tA + 1 < T ? tA + 1 : T][pl];
            vo_k0 = it_k0;
            it_tap += 4;
            it_k0 += 16;
            return;
        }
        const int row = it_c >= a.Cg ? T : it_tap;     // stage past the end of K: the all-out-of-range row
        const unsigned* tp = &offT[0][0][pl] + row * BP;
        vo[0] = tp[0];
        if constexpr (NM >= 1) vo[NCOMB > 1 ? 1 : 0] = tp[(NCOMB > 1 ? 1 : 0) * TROWS * BP];
        if constexpr (NM >= 3) {
            vo[NCOMB > 1 ? 2 : 0] = tp[(NCOMB > 1 ? 2 : 0) * TROWS * BP];
            vo[NCOMB > 1 ? 3 : 0] = tp[(NCOMB > 1 ? 3 : 0) * TROWS * BP];
        }
        vo_c = it_c;
        vo_k0 = it_k0;
        const int t1 = it_tap + 1;
        const bool wr = t1 == T;
        it_tap = wr ? 0 : t1;
        it_c += wr ? 16 : 0;
        it_k0 += 16;
    };
    auto load_a = [&](int j) { areg[j] = ld_b128s(rA, a_base[j], (unsigned)vo_k0 * 4u); };
    auto load_b = [&](int i, auto nm_tag) {
        constexpr int NM = decltype(nm_tag)::value;
        if constexpr (CPS == 4) {
            const unsigned v = (i & 3) < a.Cg ? (i < 4 ? vo[0] : vo_b) : OOB;   // 3-channel tensors: the pad channel reads 0
            breg[i] = ldr<TA>(rX, v, (unsigned)((i & 3) * HgWg4));
            return;
        }
        const unsigned so = (unsigned)((vo_c + ksub * KPT + i) * HgWg4);
        breg[i] = ldr<TA>(rX, vo[0], so);
        if constexpr (NM >= 1) bmir[0][i] = ldr<TA>(rX, vo[NCOMB > 1 ? 1 : 0], so);
        if constexpr (NM >= 3) {   // (NCOMB > 1 ? .. : 0 -- bmir and vo have one row in the instantiations without mirrors, which never run this)
            bmir[NCOMB > 1 ? 1 : 0][i] = ldr<TA>(rX, vo[NCOMB > 1 ? 2 : 0], so);
            bmir[NCOMB > 1 ? 2 : 0][i] = ldr<TA>(rX, vo[NCOMB > 1 ? 3 : 0], so);
        }
    };
    auto store_a = [&](int buf, int j) {
        const int q = tid + 256 * j;
        const int row = q >> 2, kc = (q & 3) * 4;
        if (BM * 4 >= 256 || row < BM) *reinterpret_cast<float4*>(&As[buf][row * AP + kc]) = areg[j];
    };
    auto store_b = [&](int buf, int gq, auto nm_tag) {
        constexpr int NM = decltype(nm_tag)::value;
        float* slot = &Bs[buf][((ksub * (KPT / 4) + gq) * BP + pl) * 4];
        if constexpr (NM == 0) {       // raw elements straight into their slots
            put4<TA>(slot, breg[gq * 4 + 0], breg[gq * 4 + 1], breg[gq * 4 + 2], breg[gq * 4 + 3]);
        } else {                       // border workgroups of the fused reflect gradient: sum the mirror images as fp32 values
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = gq * 4 + e;
                v[e] = raw2f<TA>(breg[i]);
                if constexpr (NM == 1) v[e] += raw2f<TA>(bmir[0][i]);
                if constexpr (NM == 3) v[e] += (raw2f<TA>(bmir[0][i]) + raw2f<TA>(bmir[NCOMB > 1 ? 1 : 0][i])) + raw2f<TA>(bmir[NCOMB > 1 ? 2 : 0][i]);
            }
            *reinterpret_cast<float4*>(slot) = make_float4(v[0], v[1], v[2], v[3]);
        }
    };

    f32x16 acc[MI][PJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < PJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float av0[MI][4], bv0[PJ][4], av1[MI][4], bv1[PJ][4];
    auto read_a = [&](int buf, int q, int i, float (&av)[MI][4]) {
        const float4 t = *reinterpret_cast<const float4*>(&As[buf][(wm * WMT + i * 32 + lo) * AP + (2 * q + hi) * 4]);
        av[i][0] = t.x; av[i][1] = t.y; av[i][2] = t.z; av[i][3] = t.w;
    };
    auto read_b = [&](int buf, int q, int j, float (&bv)[PJ][4]) {
        const float4 t = *reinterpret_cast<const float4*>(&Bs[buf][((2 * q + hi) * BP + wp * WPT + j * 32 + lo) * 4]);
        bv[j][0] = t.x; bv[j][1] = t.y; bv[j][2] = t.z; bv[j][3] = t.w;
    };
    // g-th matrix instruction of a half stage; consecutive ones hit different accumulators
    auto mfma_one = [&](int g, const float (&av)[MI][4], const float (&bv)[PJ][4]) {
        const int jj = g / (MI * PJ), i = (g / PJ) % MI, j = g % PJ;
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][jj], bv[j][jj], acc[i][j], 0, 0, 0);
    };

    auto run = [&](auto nm_tag) {
        constexpr int NH = MI * PJ * 4;                      // matrix instructions per half stage
        // non-MFMA work of the first half, in issue order: operand reads (second half of this stage), LDS writes of
        // stage st+1, global loads of stage st+2
        constexpr int I_RA = 0, I_RB = I_RA + MI, I_WA = I_RB + PJ, I_WB = I_WA + ACH, I_LA = I_WB + KPT / 4,
                      I_LB = I_LA + ACH, NI1 = I_LB + KPT;
        // second half: operand reads of stage st+1 (first half), offset-table read for stage st+3
        constexpr int J_RA = 0, J_RB = J_RA + MI, J_TA = J_RB + PJ, NI2 = J_TA + 1;
        if (st_begin >= st_end) return;
        __syncthreads();                                     // table visible
        next_offsets(nm_tag);
#pragma unroll
        for (int j = 0; j < ACH; ++j) load_a(j);             // stage 0
#pragma unroll
        for (int i = 0; i < KPT; ++i) load_b(i, nm_tag);
        next_offsets(nm_tag);
#pragma unroll
        for (int j = 0; j < ACH; ++j) store_a(0, j);
#pragma unroll
        for (int gq = 0; gq < KPT / 4; ++gq) store_b(0, gq, nm_tag);
#pragma unroll
        for (int j = 0; j < ACH; ++j) load_a(j);             // stage 1
#pragma unroll
        for (int i = 0; i < KPT; ++i) load_b(i, nm_tag);
        next_offsets(nm_tag);                                // offsets of stage 2
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MI; ++i) read_a(0, 0, i, av0);
#pragma unroll
        for (int j = 0; j < PJ; ++j) read_b(0, 0, j, bv0);

        auto stage = [&](auto buf_tag) {
            constexpr int buf = decltype(buf_tag)::value;
#pragma unroll
            for (int g = 0; g < NH; ++g) {
                mfma_one(g, av0, bv0);
#pragma unroll
                for (int k = 0; k < NI1; ++k) {
                    if (k * NH / NI1 != g) continue;
                    if (k < I_RB) read_a(buf, 1, k - I_RA, av1);
                    else if (k < I_WA) read_b(buf, 1, k - I_RB, bv1);
                    else if (k < I_WB) store_a(buf ^ 1, k - I_WA);
                    else if (k < I_LA) store_b(buf ^ 1, k - I_WB, nm_tag);
                    else if (k < I_LB) load_a(k - I_LA);
                    else load_b(k - I_LB, nm_tag);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < NH; ++g) {
                mfma_one(g, av1, bv1);
#pragma unroll
                for (int k = 0; k < NI2; ++k) {
                    if (k * NH / NI2 != g) continue;
                    if (k < J_RB) read_a(buf ^ 1, 0, k - J_RA, av0);
                    else if (k < J_TA) read_b(buf ^ 1, 0, k - J_RB, bv0);
                    else next_offsets(nm_tag);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        for (int st = st_begin; st < st_end; st += 2) {
            stage(std::integral_constant<int, 0>{});
            if (st + 1 < st_end) stage(std::integral_constant<int, 1>{});
        }
    };
    if (MIR) {  // workgroup-uniform: how many mirror images do its pixels receive at most?
        const int any2 = __syncthreads_or((myr >= 0) & (mxr >= 0));
        const int any1 = __syncthreads_or((myr >= 0) | (mxr >= 0));
        if (any2 || (any1 && !a.rowfold)) run(std::integral_constant<int, 3>{});
        else if (any1) run(std::integral_constant<int, 1>{});      // column mirrors only (table slot 1)
        else run(std::integral_constant<int, 0>{});
    } else {
        run(std::integral_constant<int, 0>{});
    }

    // --- epilogue: bias (from LDS) + activation, NCHW store (pixel on the lane -> coalesced) ------
    const int YhYw = a.Yh * a.Yw;
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        const int pix = p0 + wp * WPT + j * 32 + lo;
        if (pix >= Ptot) continue;
        int n, oy, ox;
        pix_coord(a, P, pix, n, oy, ox);
        if (a.ksplit > 1) {
            float* Yp = a.Ypart + ((size_t)blockIdx.z * a.N + n) * a.M * YhYw + oy * a.Yw + ox;
#pragma unroll
            for (int i = 0; i < MI; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * WMT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (m < a.M) Yp[(size_t)m * YhYw] = acc[i][j][r];
                }
            }
            continue;
        }
        TA* Yp = (TA*)a.Y + (size_t)n * a.M * YhYw + oy * a.Yw + ox;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int ml = wm * WMT + i * 32 + 8 * rq + 4 * hi;      // 4 consecutive output channels
                const float4 bq = *reinterpret_cast<const float4*>(&biasS[ml]);
                const float bb[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int m = m0 + ml + e;
                    if (m < a.M) st1(Yp + (size_t)m * YhYw, act_apply(acc[i][j][rq * 4 + e] + bb[e], a.act, a.slope));
                }
            }
        }
    }
}

// ---- launcher ------------------------------------------------------------------------------------------------------------------
// 5 tiles x 2 storage types of: igemm2_kernel<MODE, .., 16> for the four modes; igemm2_kernel<MODE, .., 4> and igemm_kernel<MODE, ..>
// for the three modes without the mirror gather
template <int MODE, int BM, int BP>
static void launch_tile(const IgemmArgs& a, dim3 grid, dim3 grid2, hipStream_t st) {
    if (a.chunked == 1) LAUNCH_TA(a.dtype, igemm2_kernel, grid2, a, MODE, BM, BP, 16);
    else if constexpr (MODE != MODE_BWD_REFLECT) {
        if (a.chunked == 2) LAUNCH_TA(a.dtype, igemm2_kernel, grid2, a, MODE, BM, BP, 4);
        else LAUNCH_TA(a.dtype, igemm_kernel, grid, a, MODE, BM, BP);
    }
}
template <int MODE>
static void launch_mode(const IgemmArgs& a, int bm, int bp, dim3 grid, dim3 grid2, hipStream_t st) {
    if (bm == 128 && bp == 128) launch_tile<MODE, 128, 128>(a, grid, grid2, st);
    else if (bm == 128) launch_tile<MODE, 128, 64>(a, grid, grid2, st);
    else if (bm == 64 && bp == 128) launch_tile<MODE, 64, 128>(a, grid, grid2, st);
    else if (bm == 64) launch_tile<MODE, 64, 64>(a, grid, grid2, st);
    else launch_tile<MODE, 32, 128>(a, grid, grid2, st);
}
int launch_igemm_f32(int mode, const IgemmArgs& a, int bm, int bp, dim3 grid, dim3 grid2, hipStream_t st) {
    switch (mode) {
        case MODE_FWD_ZERO: launch_mode<MODE_FWD_ZERO>(a, bm, bp, grid, grid2, st); break;
        case MODE_FWD_REFLECT: launch_mode<MODE_FWD_REFLECT>(a, bm, bp, grid, grid2, st); break;
        case MODE_BWD: launch_mode<MODE_BWD>(a, bm, bp, grid, grid2, st); break;
        default: launch_mode<MODE_BWD_REFLECT>(a, bm, bp, grid, grid2, st); break;   // the caller has checked a.chunked == 1
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace pcgan
