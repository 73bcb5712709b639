// Weight gradient of the implicit-GEMM convolution: Wp[split][m][k] = sum over a pixel range of dY[m][pix] * G(k; pix), then a
// deterministic second-pass sum over the splits (wgrad_reduce_kernel, no atomics).  Shared gathers and argument structs: igemm.h.
#include "igemm.h"
#include <mutex>

namespace pcgan {

// ------------------------------------------------------------------------------------
// backward-weight
// ------------------------------------------------------------------------------------

// Wp[m][kcol] = sum over a pixel range of dY[m][pix] * G(kcol; pix).  Tile BM x 128 (kcol), stage = 32
// pixels.  LDS rows hold 32 pixels of one m / one kcol at pitch 36 floats (ds_read_b128 conflict-free);
// the MFMA consumes the pixels in the same permuted order for both operands.
// VECA: dY planes are a multiple of 4 pixels, so a thread fetches 4 consecutive pixels with one 16-byte load.
// KMODE: 0 = generic (Cgp % 8 == 0), 1 = SMALLC (per-thread tap), 2 = ONETAP (Cgp % 128 == 0: the whole 128-column
// tile lies inside one filter tap -> one spatial offset per stage, straight-line code, interleaved schedule)
template <int MODE, int BM, int KMODE, bool VECA, typename TA>
__global__ void __launch_bounds__(256) wgrad_kernel(WgradArgs a) {
    constexpr unsigned ES = sizeof(TA);
    constexpr bool SMALLC = KMODE == 1;
    constexpr bool ONETAP = KMODE == 2;
    constexpr int BN = 128;
    constexpr int WM = (BM == 128) ? 2 : 1;
    constexpr int WN = 4 / WM;
    constexpr int WMT = BM / WM, WNT = BN / WN;
    constexpr int MI = WMT / 32, NJ = WNT / 32;
    constexpr int PT = 36;
    constexpr int AR = BM / 8, BR = BN / 8;
    constexpr int AV = BM / 32;  // float4 chunks of dY per thread (VECA)
    __shared__ __attribute__((aligned(16))) float As[2][BM * PT];
    __shared__ __attribute__((aligned(16))) float Gs[2][BN * PT];

    const int tid = threadIdx.x;
    const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int pl = tid & 31, rg = tid >> 5;

    const int nKt = (a.Kp + BN - 1) / BN;
    const int kt = blockIdx.x % nKt, mt = blockIdx.x / nKt;
    const int m0 = mt * BM, kb = kt * BN;
    const int split = blockIdx.y;
    const int HoWo = a.Ho * a.Wo, HgWg = a.Hg * a.Wg;
    const Geom g{a.Hg, a.Wg, a.sl, a.pad};
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.X, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rY = make_rsrc(a.dY, a.dy_bytes);

    // K-column bookkeeping.  Fast path (Cgp % 8 == 0): for row-group offset i the tap of column
    // kb + 8*i + rg is block-uniform and c = c_i + rg.
    int tap_b = 0, c_b = 0;
    if (!SMALLC) {
        tap_b = kb / a.Cgp;
        c_b = kb - tap_b * a.Cgp;
    }

    float areg[AR], breg[BR];
    auto load_stage = [&](int chunk) {
        // ---- dY tile -----------------------------------------------------------------
        if (VECA) {
            const int pc = (tid & 7) * 4;  // same pixel quad for all of this thread's rows
            const int pg = chunk * 32 + pc;
            unsigned vb = OOB;
            {
                const int n = pg / HoWo;
                const unsigned vv = (unsigned)((n * a.M + m0) * HoWo + (pg - n * HoWo)) * ES;
                vb = (pg < a.Ptot) ? vv : OOB;
            }
#pragma unroll
            for (int j = 0; j < AV; ++j) {
                const int row = (tid >> 3) + 32 * j;
                const float4 v = ldr4<TA>(rY, ((vb != OOB) & (m0 + row < a.M)) ? vb + (unsigned)(row * HoWo) * ES : OOB, 0u);
                areg[4 * j + 0] = v.x; areg[4 * j + 1] = v.y; areg[4 * j + 2] = v.z; areg[4 * j + 3] = v.w;
            }
        }
        // ---- this thread's gather pixel ------------------------------------------------
        const int pg = chunk * 32 + pl;
        const bool pvalid = pg < a.Ptot;
        // (computed for out-of-range pixels too: selects instead of branches keep the stage one basic block)
        const int n = pg / HoWo;
        const int rem = pg - n * HoWo;
        const int oy = rem / a.Wo;
        const int ox = rem - oy * a.Wo;
        if (!VECA) {
            const unsigned vb = pvalid ? (unsigned)((n * a.M + m0 + rg) * HoWo + rem) * ES : OOB;
#pragma unroll
            for (int i = 0; i < AR; ++i)
                areg[i] = ldr<TA>(rY, (pvalid & (m0 + rg + 8 * i < a.M)) ? vb : OOB, (unsigned)(8 * i * HoWo) * ES);
        }
        const int vbase = n * a.Cg * HgWg;
        if (ONETAP) {
            const int r = (tap_b * a.magicS) >> 16;
            const int s = tap_b - r * a.S;
            int off;
            const bool ok = tap_offset<MODE>(g, oy, ox, r, s, off) & pvalid;
            const unsigned voff = ok ? (unsigned)(vbase + off + rg * HgWg) * ES : OOB;
#pragma unroll
            for (int i = 0; i < BR; ++i)
                breg[i] = ldr<TA>(rX, (c_b + 8 * i + rg < a.Cg) ? voff : OOB, (unsigned)((c_b + 8 * i) * HgWg) * ES);
        } else if (!SMALLC) {
            int tap = tap_b, c = c_b;
            unsigned voff = OOB;
#pragma unroll
            for (int i = 0; i < BR; ++i) {
                if (i == 0 || c == 0) {  // block-uniform: the tap changed (c is a multiple of 8)
                    const int r = (tap * a.magicS) >> 16;
                    const int s = tap - r * a.S;
                    int off;
                    const bool ok = tap_offset<MODE>(g, oy, ox, r, s, off) & pvalid;
                    voff = ok ? (unsigned)(vbase + off + rg * HgWg) * ES : OOB;
                }
                const bool okc = (c + rg < a.Cg) & (kb + 8 * i + rg < a.Kp);
                breg[i] = ldr<TA>(rX, okc ? voff : OOB, (unsigned)(c * HgWg) * ES);
                c += 8;
                if (c >= a.Cgp) {
                    c -= a.Cgp;
                    ++tap;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < BR; ++i) {
                const int kcol = kb + 8 * i + rg;
                const int tap = kcol / a.Cgp, c = kcol - tap * a.Cgp;
                const int r = (tap * a.magicS) >> 16;
                const int s = tap - r * a.S;
                int off;
                const bool ok = tap_offset<MODE>(g, oy, ox, r, s, off) && pvalid && kcol < a.Kp && c < a.Cg;
                breg[i] = ldr<TA>(rX, ok ? (unsigned)(vbase + c * HgWg + off) * ES : OOB, 0u);
            }
        }
    };
    auto store_stage = [&](int buf) {
        if (VECA) {
#pragma unroll
            for (int j = 0; j < AV; ++j)
                put4p<TA>(&As[buf][((tid >> 3) + 32 * j) * PT + (tid & 7) * 4],
                          make_float4(areg[4 * j + 0], areg[4 * j + 1], areg[4 * j + 2], areg[4 * j + 3]));
        } else {
#pragma unroll
            for (int i = 0; i < AR; ++i) put1<TA>(&As[buf][(rg + 8 * i) * PT + pl], areg[i]);
        }
#pragma unroll
        for (int i = 0; i < BR; ++i) put1<TA>(&Gs[buf][(rg + 8 * i) * PT + pl], breg[i]);
    };

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nchunks = (a.Ptot + 31) / 32;
    const int c_begin = split * a.chunks_per_split;
    int c_end = c_begin + a.chunks_per_split;
    if (c_end > nchunks) c_end = nchunks;
    const int nst = c_end - c_begin;
    if (nst > 0) {
        if constexpr (sizeof(TA) == 2) {
            zero_tile<TA>(&As[0][0], 2 * BM * PT);
            zero_tile<TA>(&Gs[0][0], 2 * BN * PT);
            __syncthreads();
        }
        load_stage(c_begin);
        store_stage(0);
        __syncthreads();
        auto compute = [&](int buf) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float av[MI][4], bv[NJ][4];
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    const float4 t = *reinterpret_cast<const float4*>(&As[buf][(wm * WMT + i * 32 + lo) * PT + (2 * q + hi) * 4]);
                    av[i][0] = t.x; av[i][1] = t.y; av[i][2] = t.z; av[i][3] = t.w;
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const float4 t = *reinterpret_cast<const float4*>(&Gs[buf][(wn * WNT + j * 32 + lo) * PT + (2 * q + hi) * 4]);
                    bv[j][0] = t.x; bv[j][1] = t.y; bv[j][2] = t.z; bv[j][3] = t.w;
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][jj], bv[j][jj], acc[i][j], 0, 0, 0);
            }
        };
        // same fine-grained interleave as the forward kernel: the next stage's gathers and their address
        // arithmetic are issued between this stage's MFMAs (a wave cannot issue past a waiting MFMA)
        constexpr int NMFMA = MI * NJ * 16;
        constexpr int NLD = (VECA ? AV : AR) + BR;
        for (int st = 0; st + 1 < nst; ++st) {
            const int buf = st & 1;
            load_stage(c_begin + st + 1);
            compute(buf);
            if (ONETAP) {
#pragma unroll
                for (int gI = 0; gI < NMFMA; ++gI) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (gI < 4 * (MI + NJ)) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    if (gI < NMFMA / 2) {
                        __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
                        __builtin_amdgcn_sched_group_barrier(0x004, 3, 0);
                        __builtin_amdgcn_sched_group_barrier(0x020, (NLD + NMFMA / 2 - 1) / (NMFMA / 2), 0);
                    } else {
                        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                        __builtin_amdgcn_sched_group_barrier(0x004, 2, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            store_stage(buf ^ 1);
            __syncthreads();
        }
        compute((nst - 1) & 1);
    }
    // partial tile store: row = m, column = k (lane) -> coalesced
    float* Wp = a.Wp + (size_t)split * a.M * a.Kp;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int kcol = kb + wn * WNT + j * 32 + lo;
        if (kcol >= a.Kp) continue;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * WMT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (m < a.M) Wp[(size_t)m * a.Kp + kcol] = acc[i][j][r];
            }
        }
    }
}

// Weight gradient for M <= 4: Wp[split][m][kb..kb+15] = sum_pix dY[m][pix] * G(k; pix).  One workgroup per
// 16-column slab of K (one tap, 16 channels: needs Cgp % 16 == 0) and pixel split; every thread keeps the
// 4x16 partial sums of its pixels in registers and the workgroup reduces them once at the end.
template <int MODE, typename TA>
__global__ void __launch_bounds__(256) smallm_wgrad_kernel(WgradArgs a) {
    constexpr unsigned ES = sizeof(TA);
    __shared__ float red[4][64];
    const int tid = threadIdx.x;
    const int kb = blockIdx.x * 16;
    const int tap = kb / a.Cgp, c0 = kb - tap * a.Cgp;
    const int r = (tap * a.magicS) >> 16, s = tap - r * a.S;
    const Geom g{a.Hg, a.Wg, a.sl, a.pad};
    const int HoWo = a.Ho * a.Wo, HgWg = a.Hg * a.Wg;
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.X, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rY = make_rsrc(a.dY, a.dy_bytes);
    float acc[4][16];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[m][j] = 0.f;
    const int pbeg = blockIdx.y * a.chunks_per_split * 32;
    int pend = pbeg + a.chunks_per_split * 32;
    if (pend > a.Ptot) pend = a.Ptot;
    for (int pg = pbeg + tid; pg < pend; pg += 256) {
        const int n = pg / HoWo;
        const int rem = pg - n * HoWo;
        const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
        int off;
        const bool ok = tap_offset<MODE>(g, oy, ox, r, s, off);
        const unsigned voff = ok ? (unsigned)(n * a.Cg * HgWg + off) * ES : OOB;
        const unsigned yoff = (unsigned)(n * a.M * HoWo + rem) * ES;
        float dy[4], x[16];
#pragma unroll
        for (int m = 0; m < 4; ++m) dy[m] = ldx<TA>(rY, m < a.M ? yoff : OOB, (unsigned)(m * HoWo) * ES);
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = ldx<TA>(rX, (c0 + j < a.Cg) ? voff : OOB, (unsigned)((c0 + j) * HgWg) * ES);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[m][j] += dy[m] * x[j];
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float v = wave_sum(acc[m][j]);
            if (lane == 0) red[wave][m * 16 + j] = v;
        }
    __syncthreads();
    if (tid < 64) {
        const int m = tid >> 4, j = tid & 15;
        if (m < a.M && kb + j < a.Kp)
            a.Wp[((size_t)blockIdx.y * a.M + m) * a.Kp + kb + j] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    }
}

// Weight gradient for <= 3 output channels, stride 1, <= NT x NT taps (the generator head 64 -> 3, 7x7): sliding-window
// strips like smallm_strip_kernel.  One workgroup = one input channel c and a range of strips; one thread = 8 vertically
// consecutive output pixels of one column (lanes along the row => coalesced).  The 8 x M values of dY are loaded once per
// strip; for each filter column the 8 + NT - 1 input values are loaded once and reused by all NT row taps:
// M * NT * 8 fused multiply-adds per 8 + NT - 1 gathers.  Every thread keeps the NT x NT x M partial sums of ITS pixels in
// registers; the workgroup reduces them once at the end (wave shuffles, then LDS) and writes Wp[split][m][tap * Cgp + c].
template <int MODE, int NT, typename TA>
__global__ void __launch_bounds__(256) smallm_wgrad_strip_kernel(WgradArgs a) {
    constexpr unsigned ES = sizeof(TA);
    constexpr int PX = 8, NW = PX + NT - 1, MO = 3;
    constexpr int SG = NT > 4 ? 4 : NT;     // filter columns per workgroup (blockIdx.z picks the group): keeps the
                                            // accumulators at SG x NT x 3 registers so that 2-3 waves fit a SIMD
    __shared__ float red[4][SG * NT * MO];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const int s_lo = blockIdx.z * SG;
    const int R = a.Kp / a.Cgp / a.S;       // taps: R x S
    const int HoWo = a.Ho * a.Wo, HgWg = a.Hg * a.Wg;
    const int spc = (a.Ho + PX - 1) / PX;   // strips per column
    const int nstrips = a.N * spc * a.Wo;
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.X, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rY = make_rsrc(a.dY, a.dy_bytes);
    float acc[SG][NT][MO];   // [s - s_lo][r][m]
#pragma unroll
    for (int sj = 0; sj < SG; ++sj)
#pragma unroll
        for (int ri = 0; ri < NT; ++ri)
#pragma unroll
            for (int m = 0; m < MO; ++m) acc[sj][ri][m] = 0.f;
    const int sbeg = blockIdx.y * a.chunks_per_split;      // (strips per split)
    int send = sbeg + a.chunks_per_split;
    if (send > nstrips) send = nstrips;
    for (int sg = sbeg + tid; sg < send; sg += 256) {
        const int n = sg / (spc * a.Wo);
        const int rem = sg - n * spc * a.Wo;
        const int ss = rem / a.Wo;
        const int ox = rem - ss * a.Wo;
        const int oy0 = ss * PX;
        // input rows under the strip
        unsigned rowoff[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            int iy = oy0 - a.pad + k;
            if (MODE == MODE_FWD_REFLECT) {
                iy = iy < 0 ? -iy : iy;
                iy = iy >= a.Hg ? 2 * (a.Hg - 1) - iy : iy;
            }
            rowoff[k] = ((unsigned)iy < (unsigned)a.Hg) ? (unsigned)((n * a.Cg + c) * HgWg + iy * a.Wg) * ES : SM_INV;
        }
        auto col_off = [&](int sj) {
            int ix = ox - a.pad + s_lo + sj;
            if (MODE == MODE_FWD_REFLECT) {
                ix = ix < 0 ? -ix : ix;
                ix = ix >= a.Wg ? 2 * (a.Wg - 1) - ix : ix;
            }
            return (s_lo + sj < a.S && (unsigned)ix < (unsigned)a.Wg) ? (unsigned)ix * ES : SM_INV;
        };
        float xin[2][NW];
        {
            const unsigned co = col_off(0);
#pragma unroll
            for (int k = 0; k < NW; ++k) xin[0][k] = ldx<TA>(rX, rowoff[k] + co, 0u);
        }
        // dY of the strip (rows past the end: 0)
        float dyv[MO][PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const unsigned vo = (oy0 + j < a.Ho) ? (unsigned)(n * a.M * HoWo + (oy0 + j) * a.Wo + ox) * ES : OOB;
#pragma unroll
            for (int m = 0; m < MO; ++m) dyv[m][j] = m < a.M ? ldx<TA>(rY, vo, (unsigned)(m * HoWo) * ES) : 0.f;
        }
#pragma unroll
        for (int sj = 0; sj < SG; ++sj) {
            if (sj + 1 < SG) {   // next filter column in flight while this one is consumed
                const unsigned co = col_off(sj + 1);
#pragma unroll
                for (int k = 0; k < NW; ++k) xin[(sj + 1) & 1][k] = ldx<TA>(rX, rowoff[k] + co, 0u);
            }
            // One v_fmac_f32 per term, written out.  WORKAROUND, cause not established: left to itself the compiler pairs the
            // accumulators into v_pk_fma_f32 with operand selects, and THAT build of this kernel returned different sums from run to
            // run whenever an f16-MFMA kernel of another stream shared the CUs (scripts/diag_race.py: 30 / 30; alone, or beside
            // fp32-MFMA / copy kernels, exact).  Round 4's ISA study (scripts/micro/head_wgrad_isa.md) shows the compiler's wait counts
            // are correct (no read or overwrite of a register with an outstanding load) and that the one form unique to that build is
            // `op_sel:[0,1,0]` (high dword of src1 broadcast) -- absent from every other kernel; tests/test_isa_guard.py bans it from
            // the library.  Same arithmetic, same order.
#pragma unroll
            for (int ri = 0; ri < NT; ++ri)
#pragma unroll
                for (int j = 0; j < PX; ++j)
#pragma unroll
                    for (int m = 0; m < MO; ++m)
                        asm("v_fmac_f32 %0, %1, %2" : "+v"(acc[sj][ri][m]) : "v"(dyv[m][j]), "v"(xin[sj & 1][j + ri]));
        }
    }
    // workgroup reduction: 6 shuffle steps inside each wave, then the 4 waves through LDS
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int sj = 0; sj < SG; ++sj)
#pragma unroll
        for (int ri = 0; ri < NT; ++ri)
#pragma unroll
            for (int m = 0; m < MO; ++m) {
                float v = acc[sj][ri][m];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
                if (lane == 0) red[wave][(sj * NT + ri) * MO + m] = v;
            }
    __syncthreads();
    if (tid < SG * NT * MO) {
        const int m = tid % MO, ri = (tid / MO) % NT, sj = s_lo + tid / (MO * NT);
        if (m < a.M && ri < R && sj < a.S) {
            const float v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
            a.Wp[((size_t)blockIdx.y * a.M + m) * a.Kp + (ri * a.S + sj) * a.Cgp + c] = v;
        }
    }
}

// ------------------------------------------------------------------------------------
// Weight gradient, pipelined version for tap-aligned K tiles (padded channel count a multiple of 128, or 64):
// same recipe as igemm2_kernel -- few non-scalar instructions per matrix instruction, every wait long after its
// request, source order = issue order.
//   tile  : BM output channels x 128 K-columns (one filter tap x 128 channels, or two taps x 64), reduction over
//           pixels in stages of 32, split over pixel ranges (blockIdx.y) with a deterministic second-pass sum
//   offsets: the per-pixel gather offsets (padding / reflection / stride arithmetic, two integer divisions) are
//           computed by all 256 threads for 8 stages at a time into a 16-slot LDS ring; a stage then needs
//           NT + 1 four-byte LDS reads
//   stage t: group 0/1 of the MFMA chain + LDS writes of stage t+1 (loaded one stage ago)
//            group 2/3 + global loads of stage t+2; the barrier sits between group 2 and 3, the operands of
//            stage t+1's first group are read under group 3
template <int MODE, int BM, bool VECA, int NT, typename TA>
__global__ void __launch_bounds__(256) wgrad2_kernel(WgradArgs a) {
    constexpr unsigned ES = sizeof(TA);
    constexpr int BN = 128;
    constexpr int WM = (BM == 128) ? 2 : 1;
    constexpr int WN = 4 / WM;
    constexpr int WMT = BM / WM, WNT = BN / WN;
    constexpr int MI = WMT / 32, NJ = WNT / 32;
    constexpr int PT = 36;
    constexpr int AR = BM / 8, BR = BN / 8;
    constexpr int AV = BM / 32;
    constexpr int NA = VECA ? AV : AR;          // dY loads / LDS writes per thread and stage
    constexpr int RING = 16;
    __shared__ __attribute__((aligned(16))) float As[2][BM * PT];
    __shared__ __attribute__((aligned(16))) float Gs[2][BN * PT];
    __shared__ unsigned xoffT[RING][NT][32];
    __shared__ unsigned yoffT[RING][32];

    const int tid = threadIdx.x;
    const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int pl = tid & 31, rg = tid >> 5;

    const int nKt = (a.Kp + BN - 1) / BN;
    const int kt = blockIdx.x % nKt, mt = blockIdx.x / nKt;
    const int m0 = mt * BM, kb = kt * BN;
    const int split = blockIdx.y;
    const int HoWo = a.Ho * a.Wo, HgWg = a.Hg * a.Wg;
    const int HoWo4 = HoWo * (int)ES, HgWg4 = HgWg * (int)ES;     // bytes of one plane
    const Geom g{a.Hg, a.Wg, a.sl, a.pad};
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.X, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rY = make_rsrc(a.dY, a.dy_bytes);
    const int tap_b = kb / a.Cgp, c_b = kb - tap_b * a.Cgp;
    const int ntaps = a.Kp / a.Cgp;

    const int nchunks = (a.Ptot + 31) / 32;
    const int c_begin = split * a.chunks_per_split;
    int c_end = c_begin + a.chunks_per_split;
    if (c_end > nchunks) c_end = nchunks;
    const int nst = c_end - c_begin;

    // offsets of 8 stages (relative chunks tb .. tb+7) -> ring slots
    auto refill = [&](int tb) {
        const int rel = tb + (tid >> 5);
        const int slot = rel & (RING - 1);
        const int pg = (c_begin + rel) * 32 + pl;
        const bool valid = (pg < a.Ptot) & (c_begin + rel < c_end);
        const int n = pg / HoWo;
        const int rem = pg - n * HoWo;
        const int oy = rem / a.Wo;
        const int ox = rem - oy * a.Wo;
        yoffT[slot][pl] = valid ? (unsigned)((n * a.M + m0) * HoWo + rem) * ES : OOB;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            const int tap = tap_b + ti;
            const int r = tap / a.S, sx = tap - r * a.S;
            int off;
            const bool ok = tap_offset<MODE>(g, oy, ox, r, sx, off) & valid & (tap < ntaps);
            xoffT[slot][ti][pl] = ok ? (unsigned)(n * a.Cg * HgWg + off) * ES : OOB;
        }
    };

    // per-thread constant parts of the load offsets (bit 31 = row out of range)
    const int pc = (tid & 7) * 4;
    const unsigned yrow = VECA ? (unsigned)((tid >> 3) * HoWo4) : (unsigned)(rg * HoWo4);
    unsigned yflag[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int row = VECA ? (tid >> 3) + 32 * j : rg + 8 * j;
        yflag[j] = (m0 + row < a.M) ? 0u : OOB;
    }
    const unsigned xrow = (unsigned)(rg * HgWg4);

    float areg[VECA ? 4 * AV : AR], breg[BR];
    unsigned yo = OOB, xo[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) xo[ti] = OOB;
    unsigned yraw = OOB, xraw[NT];
    auto read_offsets = [&](int rel) {   // ring-table entries of relative chunk `rel` (raw: used one group later)
        const int slot = rel & (RING - 1);
        yraw = yoffT[slot][VECA ? pc : pl];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) xraw[ti] = xoffT[slot][ti][pl];
    };
    auto combine_offsets = [&]() {
        yo = yraw + yrow;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) xo[ti] = xraw[ti] + xrow;
    };
    auto load_a = [&](int j) {
        if (VECA) {
            const float4 v = ldr4<TA>(rY, yo | yflag[j], (unsigned)(32 * j * HoWo4));
            areg[4 * j + 0] = v.x; areg[4 * j + 1] = v.y; areg[4 * j + 2] = v.z; areg[4 * j + 3] = v.w;
        } else {
            areg[j] = ldr<TA>(rY, yo | yflag[j], (unsigned)(8 * j * HoWo4));
        }
    };
    auto load_b = [&](int i) {
        constexpr int PER = BR / NT;   // K-columns (i) per tap
        breg[i] = ldr<TA>(rX, xo[i / PER], (unsigned)((c_b + 8 * (i % PER)) * HgWg4));
    };
    auto store_a = [&](int buf, int j) {
        if (VECA) {
            put4p<TA>(&As[buf][((tid >> 3) + 32 * j) * PT + pc], make_float4(areg[4 * j + 0], areg[4 * j + 1], areg[4 * j + 2], areg[4 * j + 3]));
        } else {
            put1<TA>(&As[buf][(rg + 8 * j) * PT + pl], areg[j]);
        }
    };
    auto store_b = [&](int buf, int i) { put1<TA>(&Gs[buf][(rg + 8 * i) * PT + pl], breg[i]); };

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float av[2][MI][4], bv[2][NJ][4];   // operand sets of two consecutive MFMA groups
    auto read_op = [&](int buf, int q, int k, int set) {   // k-th operand read of group q: A rows first, then B
        if (k < MI) {
            const float4 t = *reinterpret_cast<const float4*>(&As[buf][(wm * WMT + k * 32 + lo) * PT + (2 * q + hi) * 4]);
            av[set][k][0] = t.x; av[set][k][1] = t.y; av[set][k][2] = t.z; av[set][k][3] = t.w;
        } else {
            const int j = k - MI;
            const float4 t = *reinterpret_cast<const float4*>(&Gs[buf][(wn * WNT + j * 32 + lo) * PT + (2 * q + hi) * 4]);
            bv[set][j][0] = t.x; bv[set][j][1] = t.y; bv[set][j][2] = t.z; bv[set][j][3] = t.w;
        }
    };
    auto mfma_one = [&](int gidx, int set) {
        const int jj = gidx / (MI * NJ), i = (gidx / NJ) % MI, j = gidx % NJ;
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[set][i][jj], bv[set][j][jj], acc[i][j], 0, 0, 0);
    };

    if (nst > 0) {
        zero_tile<TA>(&As[0][0], 2 * BM * PT);
        zero_tile<TA>(&Gs[0][0], 2 * BN * PT);
        refill(0);
        refill(8);
        __syncthreads();
        read_offsets(0);
        combine_offsets();
#pragma unroll
        for (int j = 0; j < NA; ++j) load_a(j);
#pragma unroll
        for (int i = 0; i < BR; ++i) load_b(i);
        read_offsets(1);
        combine_offsets();
#pragma unroll
        for (int j = 0; j < NA; ++j) store_a(0, j);
#pragma unroll
        for (int i = 0; i < BR; ++i) store_b(0, i);
#pragma unroll
        for (int j = 0; j < NA; ++j) load_a(j);
#pragma unroll
        for (int i = 0; i < BR; ++i) load_b(i);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MI + NJ; ++k) read_op(0, 0, k, 0);

        constexpr int NG = MI * NJ * 4;            // matrix instructions per group
        constexpr int NOP = MI + NJ;               // operand reads per group
        constexpr int NWR = NA + BR, NLD = NA + BR;
        constexpr int NW0 = NWR / 2, NL0 = NLD / 2;
        auto stage = [&](int t, auto buf_tag) {
            constexpr int buf = decltype(buf_tag)::value;
            // group q computes with operand set q & 1 and issues: the reads of group q+1's operands, plus its share of
            // LDS writes (groups 0, 1) / global loads (groups 2, 3)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n_extra = q == 0 ? NW0 + 1 : (q == 1 ? NWR - NW0 : (q == 2 ? NL0 + 1 : NLD - NL0));
                const int n_items = NOP + n_extra;
                if (q == 3) {
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int gI = 0; gI < NG; ++gI) {
                    mfma_one(gI, q & 1);
#pragma unroll
                    for (int k = 0; k < n_items; ++k) {
                        if (k * NG / n_items != gI) continue;
                        if (k < NOP) {
                            if (q < 3) read_op(buf, q + 1, k, (q + 1) & 1);
                            else read_op(buf ^ 1, 0, k, 0);
                        } else {
                            const int e = k - NOP;
                            if (q == 0) {
                                if (e == 0) read_offsets(t + 2);
                                else if (e - 1 < NA) store_a(buf ^ 1, e - 1);
                                else store_b(buf ^ 1, e - 1 - NA);
                            } else if (q == 1) {
                                const int w = NW0 + e;
                                if (w < NA) store_a(buf ^ 1, w);
                                else store_b(buf ^ 1, w - NA);
                            } else if (q == 2) {
                                if (e == 0) combine_offsets();
                                else if (e - 1 < NA) load_a(e - 1);
                                else load_b(e - 1 - NA);
                            } else {
                                const int l = NL0 + e;
                                if (l < NA) load_a(l);
                                else load_b(l - NA);
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        for (int t = 0; t < nst; t += 2) {
            if ((t & 7) == 0 && t > 0) refill(t + 8);
            stage(t, std::integral_constant<int, 0>{});
            if (t + 1 < nst) stage(t + 1, std::integral_constant<int, 1>{});
        }
    }
    // partial tile store: row = m, column = k (lane) -> coalesced
    float* Wp = a.Wp + (size_t)split * a.M * a.Kp;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int kcol = kb + wn * WNT + j * 32 + lo;
        if (kcol >= a.Kp) continue;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * WMT + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (m < a.M) Wp[(size_t)m * a.Kp + kcol] = acc[i][j][r];
            }
        }
    }
}

// dw[k][c][r][s] = sum_split Wp[split][k][tap*Cgp + c].  One workgroup = 64 consecutive partial-sum columns; its 4 waves
// take the splits round-robin (4 loads in flight per thread) and are combined in a fixed order: the sequential sum over up to
// 512 splits of the first version was pure load latency (23 us average, 38 us on the few-tile layers).
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ Wp, float* __restrict__ dw, int splits, int K,
                                                           int C, int Cgp, int RS, int accumulate) {
    __shared__ float red[3][64];
    const int Kp = RS * Cgp;
    const int total = K * Kp;
    const int wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    float acc = 0.f;
    if (i < total) {
        const float* p = Wp + i;
        int sp = wave;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (; sp + 12 < splits; sp += 16) {
            a0 += p[(size_t)sp * total];
            a1 += p[(size_t)(sp + 4) * total];
            a2 += p[(size_t)(sp + 8) * total];
            a3 += p[(size_t)(sp + 12) * total];
        }
        for (; sp < splits; sp += 4) a0 += p[(size_t)sp * total];
        acc = (a0 + a1) + (a2 + a3);
    }
    if (wave > 0) red[wave - 1][threadIdx.x & 63] = acc;
    __syncthreads();
    if (wave > 0 || i >= total) return;
    acc = (acc + red[0][threadIdx.x]) + (red[1][threadIdx.x] + red[2][threadIdx.x]);
    const int k = i / Kp;
    const int j = i - k * Kp;
    const int tap = j / Cgp, c = j - tap * Cgp;
    if (c >= C) return;
    float* o = dw + ((size_t)k * C + c) * RS + tap;
    *o = accumulate ? *o + acc : acc;   // accumulate: dw is the parameter's .grad buffer (fused "grad +=")
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static inline bool smallm_wgrad(const pcgan_conv_desc* d) { return d->K <= 4 && (round4(d->C) % 16) == 0; }

// strip weight-gradient kernel: <= 3 output channels, stride 1, <= 7x7 taps, columns long enough for 8-pixel strips
static inline bool smallm_wgrad_strip(const pcgan_conv_desc* d) {
    return d->K <= 3 && d->stride == 1 && d->R <= 7 && d->S <= 7 && d->R >= 3 && d->P >= 16 && d->C >= 16;
}

// option "wgrad_ks" > 0 (tests): that many splits for every family, cut to [1, units]; the callers re-derive the units of a split
static inline int forced_splits(int units) {
    const int fk = option(OPT_WGRAD_KS);
    return fk <= 0 ? 0 : (fk > units ? (units > 0 ? units : 1) : fk);
}

int wgrad_splits(const pcgan_conv_desc* d, int* chunks_per_split) {
    const int Cgp = round4(d->C);
    if (smallm_wgrad_strip(d)) {   // one workgroup per input channel and strip range; ~2048 workgroups, >= 4 strips per thread
        const int nstrips = d->N * ((d->P + 7) / 8) * d->Q;
        int splits = 1024 / d->C;
        if (splits > nstrips / 1024) splits = nstrips / 1024;
        if (splits < 1) splits = 1;
        if (const int fk = forced_splits(nstrips)) splits = fk;
        const int sps = (nstrips + splits - 1) / splits;
        *chunks_per_split = sps;
        return (nstrips + sps - 1) / sps;
    }
    const int Kp = d->R * d->S * Cgp;
    if (smallm_wgrad(d)) {  // one workgroup per 16 K-columns and pixel split; aim at ~2048 workgroups
        const int chunks = (d->N * d->P * d->Q + 31) / 32;
        int splits = 2048 / (Kp / 16);
        if (splits > chunks / 64) splits = chunks / 64;  // >= 8 pixels per thread
        if (splits < 1) splits = 1;
        if (const int fk = forced_splits(chunks)) splits = fk;
        int cps = (chunks + splits - 1) / splits;
        *chunks_per_split = cps;
        return (chunks + cps - 1) / cps;
    }
    const int bm = d->K > 64 ? 128 : (d->K > 32 ? 64 : 32);
    const int tiles = ((d->K + bm - 1) / bm) * ((Kp + 127) / 128);
    const int Ptot = d->N * d->P * d->Q;
    const int chunks = (Ptot + 31) / 32;
    // Two workgroups fit on a CU (74-80 KB of LDS each): `slots` run at once.  The workgroup count tiles x splits is
    // kept just BELOW a whole number of rounds of slots -- a few workgroups over and the kernel waits for a nearly empty
    // extra round.  One round if it fills >= 90 % of the slots (fewest partial sums to write and reduce), else the
    // round count (<= 4) with the best fill.
    static int slots = 0;
    if (!slots) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        slots = 2 * cus;
    }
    int splits = 1;
    {
        double best = -1.0;
        for (int r = 1; r <= 4; ++r) {
            const int sp = (r * slots) / tiles;
            if (sp < 1) continue;
            const double fill = (double)sp * tiles / ((double)r * slots);
            if (fill > best + 1e-9) {
                best = fill;
                splits = sp;
            }
            if (fill >= 0.9) break;
        }
    }
    if (splits > chunks / 8) splits = chunks / 8;  // at least 8 stages of work per block
    if (splits < 1) splits = 1;
    if (splits > 512) splits = 512;
    if (const int fk = forced_splits(chunks)) splits = fk;   // (not subject to the 8-stage floor)
    int cps = (chunks + splits - 1) / splits;
    splits = (chunks + cps - 1) / cps;
    *chunks_per_split = cps;
    return splits;
}

// kernel choice -- 2 modes (zero / reflection padding) x 2 storage types of:
//   smallm_wgrad_strip_kernel<MODE, NT = 4 | 7>, smallm_wgrad_kernel<MODE>,
//   wgrad2_kernel<MODE, BM = 128 | 64 | 32, VECA, NT = 2 | 1>, wgrad_kernel<MODE, BM = 128 | 64 | 32, KMODE = 0 | 1 | 2, VECA>
// (which: {family PCGAN_WGRAD_*, BM, VECA, variant} of the instantiation launched, for the launch record)
template <int MODE, int BM, bool VECA>
static void launch_tile(const pcgan_conv_desc* d, const WgradArgs& a, dim3 grid, hipStream_t st, int* which) {
    const int Cgp = a.Cgp;
    which[0] = PCGAN_WGRAD_TILE; which[1] = BM; which[2] = VECA;
    if ((d->C % 64) == 0 && ((Cgp % 128) == 0 || Cgp == 64)) {
        which[0] = PCGAN_WGRAD_TILE2; which[3] = Cgp == 64 ? 2 : 1;
        if (Cgp == 64) LAUNCH_TA(a.dtype, wgrad2_kernel, grid, a, MODE, BM, VECA, 2);
        else LAUNCH_TA(a.dtype, wgrad2_kernel, grid, a, MODE, BM, VECA, 1);
    } else if ((Cgp % 8) != 0) {
        which[3] = 1;
        LAUNCH_TA(a.dtype, wgrad_kernel, grid, a, MODE, BM, 1, VECA);
    } else if ((Cgp % 128) == 0) {
        which[3] = 2;
        LAUNCH_TA(a.dtype, wgrad_kernel, grid, a, MODE, BM, 2, VECA);
    } else {
        which[3] = 0;
        LAUNCH_TA(a.dtype, wgrad_kernel, grid, a, MODE, BM, 0, VECA);
    }
}
template <int MODE>
static void launch_mode(const pcgan_conv_desc* d, const WgradArgs& a, int splits, hipStream_t st, int* which) {
    if (smallm_wgrad_strip(d)) {
        const bool nt4 = d->R <= 4 && d->S <= 4;
        const dim3 sgrid((unsigned)d->C, (unsigned)splits, (unsigned)(nt4 ? 1 : (d->S + 3) / 4));
        which[0] = PCGAN_WGRAD_STRIP; which[3] = nt4 ? 4 : 7;
        if (nt4) LAUNCH_TA(a.dtype, smallm_wgrad_strip_kernel, sgrid, a, MODE, 4);
        else LAUNCH_TA(a.dtype, smallm_wgrad_strip_kernel, sgrid, a, MODE, 7);
        return;
    }
    if (smallm_wgrad(d)) {
        const dim3 sgrid((unsigned)(a.Kp / 16), (unsigned)splits);
        which[0] = PCGAN_WGRAD_SMALLM;
        LAUNCH_TA(a.dtype, smallm_wgrad_kernel, sgrid, a, MODE);
        return;
    }
    const int bm = a.M > 64 ? 128 : (a.M > 32 ? 64 : 32);
    const dim3 grid((unsigned)(((a.M + bm - 1) / bm) * ((a.Kp + 127) / 128)), (unsigned)splits);
    const bool veca = ((d->P * d->Q) % 4) == 0;
    if (bm == 128 && veca) launch_tile<MODE, 128, true>(d, a, grid, st, which);
    else if (bm == 128) launch_tile<MODE, 128, false>(d, a, grid, st, which);
    else if (bm == 64 && veca) launch_tile<MODE, 64, true>(d, a, grid, st, which);
    else if (bm == 64) launch_tile<MODE, 64, false>(d, a, grid, st, which);
    else if (veca) launch_tile<MODE, 32, true>(d, a, grid, st, which);
    else launch_tile<MODE, 32, false>(d, a, grid, st, which);
}

// host-side record of the last launch launch_wgrad decided (pcgan_wgrad_last_launch): a record of its own -- the implicit GEMM's
// (record_launch, igemm_conv.hip) does not move when a weight gradient runs
static std::mutex g_wgrad_mu;
static int g_wgrad_rec[PCGAN_WGRAD_LAUNCH_INFO] = {0};

int launch_wgrad(const pcgan_conv_desc* d, const WgradArgs& a, int splits, float* dw, int accumulate, hipStream_t st) {
    int which[4] = {0, 0, 0, 0};
    if (d->pad_mode == 1) launch_mode<MODE_FWD_REFLECT>(d, a, splits, st, which);
    else launch_mode<MODE_FWD_ZERO>(d, a, splits, st, which);
    {
        std::lock_guard<std::mutex> lk(g_wgrad_mu);
        const int v[PCGAN_WGRAD_LAUNCH_INFO] = {g_wgrad_rec[0] + 1, which[0], d->pad_mode == 1 ? 1 : 0, which[1], which[2], which[3], a.dtype, splits, a.chunks_per_split};
        for (int i = 0; i < PCGAN_WGRAD_LAUNCH_INFO; ++i) g_wgrad_rec[i] = v[i];
    }
    PCGAN_LAUNCH_CHECK();
    const int RS = d->R * d->S;
    const size_t total = (size_t)d->K * RS * a.Cgp;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st, (const float*)a.Wp, dw, splits, d->K, d->C,
                       a.Cgp, RS, accumulate);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace pcgan

extern "C" int pcgan_wgrad_last_launch(int* info, int n) {
    using namespace pcgan;
    PCGAN_CHECK(info != nullptr && n > 0, "wgrad_last_launch: null output");
    std::lock_guard<std::mutex> lk(g_wgrad_mu);
    for (int i = 0; i < n; ++i) info[i] = i < PCGAN_WGRAD_LAUNCH_INFO ? g_wgrad_rec[i] : 0;
    return 0;
}
