// Convolutions that PRODUCE <= 4 channels on the vector ALU (forward and data gradient), the weight layouts they read
// (transpose4, pack_strip), and their launchers.  Shared gathers, argument structs and tap arithmetic: igemm.h.
#include "igemm.h"

namespace pcgan {

// ------------------------------------------------------------------------------------
// Small-M path (M <= 4 output channels): the generator head (64->3), the last PatchGAN / Elo-head conv
// (->1) and every data gradient that lands on an image (3-4 channels).  A 32-row MFMA tile would be >= 87 %
// padding there, so these run on the vector ALU: one thread = one pixel x 4 outputs, weights broadcast
// through the scalar cache as [k][4] rows, gathers coalesced along pixels.  Bound: L1/TA (one 4-byte
// gather per 4 FMA).
// ------------------------------------------------------------------------------------
__global__ void transpose4_kernel(const float* __restrict__ A, float* __restrict__ At, int M, int Kp) {
    const int total = Kp * 4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int k = i >> 2, m = i & 3;
        At[i] = m < M ? A[(size_t)m * Kp + k] : 0.f;
    }
}

// strip-kernel weights: Ws[c][sj][8][4] from A[m][(ri*nS + sj)*Cgp + c] (zero for ri >= nR, m >= M)
__global__ void pack_strip_kernel(const float* __restrict__ A, float* __restrict__ Ws, int M, int Cg, int Cgp, int nR, int nS) {
    const int total = Cg * nS * 32;
    const int Kp = nR * nS * Cgp;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int m = i & 3, ri = (i >> 2) & 7, cs = i >> 5;
        const int c = cs / nS, sj = cs - c * nS;
        Ws[i] = (m < M && ri < nR) ? A[(size_t)m * Kp + (ri * nS + sj) * Cgp + c] : 0.f;
    }
}

// 64 pixels per workgroup; the 4 waves split the channels of the gathered tensor and are summed through
// LDS.  Loop order channel -> tap keeps one channel's (R x S) neighbourhood L1-resident across its taps;
// the separable gather offsets (row part, column part) are tabulated per pixel in LDS once per workgroup.
template <int MODE, typename TA>
__global__ void __launch_bounds__(256) smallm_conv_kernel(IgemmArgs a) {
    constexpr unsigned ES = sizeof(TA);
    __shared__ unsigned rowoff[12][64], coloff[12][64];
    __shared__ float red[3][4][64];
    const PhaseArgs& P = a.ph[blockIdx.y];
    const int Ptot = P.Ptot;
    const int p0 = blockIdx.x * 64;
    if (p0 >= Ptot) return;
    const int tid = threadIdx.x;
    const int pl = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pg = p0 + pl;
    const bool pvalid = pg < Ptot;
    const int HsWs = P.Hs * P.Ws, HgWg = a.Hg * a.Wg;
    int n = 0, py = 0, px = 0;
    if (pvalid) {
        n = pg / HsWs;
        const int rem = pg - n * HsWs;
        const int sy = rem / P.Ws;
        py = sy * a.ostep + P.fy;
        px = (rem - sy * P.Ws) * a.ostep + P.fx;
    }
    // separable offset tables (bytes): wave w fills entries w, w+4, w+8 of its pixel lane
    for (int i = wave; i < P.nR; i += 4) {
        const int r = P.r0 + i * a.tstep;
        int iy;
        bool ok = true;
        if (MODE == MODE_BWD) {
            const int ty = py + a.pad - r;
            iy = ty >> a.sl;
            ok = ty >= 0 && iy < a.Hg;
        } else {
            iy = (py << a.sl) - a.pad + r;
            if (MODE == MODE_FWD_REFLECT) {
                iy = iy < 0 ? -iy : iy;
                iy = iy >= a.Hg ? 2 * (a.Hg - 1) - iy : iy;
            } else {
                ok = (unsigned)iy < (unsigned)a.Hg;
            }
        }
        rowoff[i][pl] = ok ? (unsigned)(iy * a.Wg) * ES : SM_INV;
    }
    for (int j = wave; j < P.nS; j += 4) {
        const int s = P.s0 + j * a.tstep;
        int ix;
        bool ok = true;
        if (MODE == MODE_BWD) {
            const int tx = px + a.pad - s;
            ix = tx >> a.sl;
            ok = tx >= 0 && ix < a.Wg;
        } else {
            ix = (px << a.sl) - a.pad + s;
            if (MODE == MODE_FWD_REFLECT) {
                ix = ix < 0 ? -ix : ix;
                ix = ix >= a.Wg ? 2 * (a.Wg - 1) - ix : ix;
            } else {
                ok = (unsigned)ix < (unsigned)a.Wg;
            }
        }
        coloff[j][pl] = ok ? (unsigned)ix * ES : SM_INV;
    }
    __syncthreads();
    const unsigned vbase = pvalid ? (unsigned)(n * a.Cg * HgWg) * ES : SM_INV;
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.X, a.x_bytes);
    const float4* __restrict__ At = reinterpret_cast<const float4*>(P.A);  // [Kp][4]
    const int cpw = (a.Cg + 3) >> 2;
    const int c_lo = wave * cpw;
    const int c_hi = (c_lo + cpw < a.Cg) ? c_lo + cpw : a.Cg;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    for (int c = c_lo; c < c_hi; ++c) {
        const unsigned soff = (unsigned)(c * HgWg) * ES;
        for (int ri = 0; ri < P.nR; ++ri) {
            const unsigned ro = vbase + rowoff[ri][pl];
            const float4* __restrict__ wrow = At + (ri * P.nS) * a.Cgp + c;
#pragma unroll 4
            for (int sj = 0; sj < P.nS; ++sj) {
                const float x = ldx<TA>(rX, ro + coloff[sj][pl], soff);
                const float4 w = wrow[sj * a.Cgp];  // wave-uniform address -> scalar load
                acc0 += x * w.x; acc1 += x * w.y; acc2 += x * w.z; acc3 += x * w.w;
            }
        }
    }
    if (wave > 0) {
        red[wave - 1][0][pl] = acc0; red[wave - 1][1][pl] = acc1; red[wave - 1][2][pl] = acc2; red[wave - 1][3][pl] = acc3;
    }
    __syncthreads();
    if (wave > 0 || !pvalid) return;
    const float out[4] = {acc0 + (red[0][0][pl] + red[1][0][pl]) + red[2][0][pl], acc1 + (red[0][1][pl] + red[1][1][pl]) + red[2][1][pl],
                          acc2 + (red[0][2][pl] + red[1][2][pl]) + red[2][2][pl], acc3 + (red[0][3][pl] + red[1][3][pl]) + red[2][3][pl]};
    const int YhYw = a.Yh * a.Yw;
    TA* Yp = (TA*)a.Y + (size_t)n * a.M * YhYw + py * a.Yw + px;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (m < a.M) {
            float v = out[m];
            if (a.bias) v += a.bias[m];
            st1(Yp + (size_t)m * YhYw, act_apply(v, a.act, a.slope));
        }
    }
}

// Strip variant: one thread = PX vertically consecutive pixels of one column x MO outputs; lanes run along the row, so
// every gather instruction reads consecutive addresses.  For a fixed (channel, filter column) the PX + NR - 1 input
// values above/below the strip are loaded ONCE into registers and reused by all NR row taps of all PX pixels (sliding
// window): MO * NR * PX fused multiply-adds per PX + NR - 1 gathers instead of MO per gather, which moves the kernel
// from the L1/TA bound of smallm_conv_kernel towards the vector-ALU bound.  Weights come in through the scalar cache
// ([c][sj][8][4], wave-uniform addresses, no branches).  The 4 waves split the channels and are summed through LDS.
// Needs unit pixel stride along the column in the gathered tensor: forward with stride 1, or any data-gradient phase.
template <int MODE, int NR, int MO, typename TA>
__global__ void __launch_bounds__(256) smallm_strip_kernel(IgemmArgs a) {
    constexpr unsigned ES = sizeof(TA);
    constexpr int PX = 8, NW = PX + NR - 1;
    constexpr bool BWD = MODE == MODE_BWD;
    __shared__ unsigned coltab[12][64];
    __shared__ float red[3][MO * PX][64];
    const PhaseArgs& P = a.ph[blockIdx.y];
    const int spc = (P.Hs + PX - 1) / PX;   // strips per column
    const int nstrips = a.N * spc * P.Ws;
    if ((int)(blockIdx.x * 64) >= nstrips) return;
    const int tid = threadIdx.x;
    const int pl = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sg = blockIdx.x * 64 + pl;
    const bool svalid = sg < nstrips;
    const int HgWg = a.Hg * a.Wg;
    int n = 0, sy0 = 0, sx = 0;
    if (svalid) {
        n = sg / (spc * P.Ws);
        const int rem = sg - n * spc * P.Ws;
        const int ss = rem / P.Ws;
        sy0 = ss * PX;
        sx = rem - ss * P.Ws;
    }
    const int px = sx * a.ostep + P.fx;
    for (int j = wave; j < P.nS; j += 4) {   // column part of the gather offset, per filter column
        const int sc = P.s0 + j * a.tstep;
        int ix;
        bool ok = svalid;
        if (BWD) {
            const int tx = px + a.pad - sc;
            ix = tx >> a.sl;
            ok = ok && tx >= 0 && ix < a.Wg;
        } else {
            ix = px - a.pad + sc;
            if (MODE == MODE_FWD_REFLECT) {
                ix = ix < 0 ? -ix : ix;
                ix = ix >= a.Wg ? 2 * (a.Wg - 1) - ix : ix;
            } else {
                ok = ok && (unsigned)ix < (unsigned)a.Wg;
            }
        }
        coltab[j][pl] = ok ? (unsigned)ix * ES : SM_INV;
    }
    // row part (+ image base): window position k holds input row y0 + k; pixel j and row tap ri meet at k = j + ri
    // (forward) or k = j - ri + NR - 1 (data gradient: source row = sub-grid row + q0 - ri)
    unsigned rowoff[NW];
    {
        const int y0 = BWD ? sy0 + ((P.fy + a.pad - P.r0) >> a.sl) - (NR - 1) : sy0 - a.pad + P.r0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            int iy = y0 + k;
            if (MODE == MODE_FWD_REFLECT) {
                iy = iy < 0 ? -iy : iy;
                iy = iy >= a.Hg ? 2 * (a.Hg - 1) - iy : iy;
            }
            const bool ok = (unsigned)iy < (unsigned)a.Hg;   // (reflect: strips past the last row are never stored)
            rowoff[k] = ok ? (unsigned)(n * a.Cg * HgWg + iy * a.Wg) * ES : SM_INV;
        }
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.X, a.x_bytes);
    const int nS = P.nS;
    // channels: split over blockIdx.z (few-strip launches, partial sums reduced by splitk_reduce_kernel), then over waves
    const int cps = a.ksplit > 1 ? (a.Cg + a.ksplit - 1) / a.ksplit : a.Cg;
    const int cz0 = (int)blockIdx.z * cps;
    const int cz1 = cz0 + cps < a.Cg ? cz0 + cps : a.Cg;
    const int cpw = (cz1 - cz0 + 3) >> 2;
    const int c_lo = cz0 + wave * cpw;
    const int c_hi = (c_lo + cpw < cz1) ? c_lo + cpw : cz1;
    float acc[MO][PX];
#pragma unroll
    for (int m = 0; m < MO; ++m)
#pragma unroll
        for (int j = 0; j < PX; ++j) acc[m][j] = 0.f;

    const float4* __restrict__ Ws4 = reinterpret_cast<const float4*>(P.As);   // [c][sj][8] float4
    auto issue = [&](float (&buf)[NW], float4 (&wb)[NR], int c, int sj) {
        const unsigned co = coltab[sj][pl];
        const unsigned so = (unsigned)(c * HgWg) * ES;
#pragma unroll
        for (int k = 0; k < NW; ++k) buf[k] = ldx<TA>(rX, rowoff[k] + co, so);
        const float4* __restrict__ wr = Ws4 + (size_t)(c * nS + sj) * 8;   // wave-uniform -> scalar loads, no branches
#pragma unroll
        for (int ri = 0; ri < NR; ++ri) wb[ri] = wr[ri];
    };
    auto compute = [&](const float (&buf)[NW], const float4 (&wb)[NR]) {
#pragma unroll
        for (int ri = 0; ri < NR; ++ri) {
            const float w[4] = {wb[ri].x, wb[ri].y, wb[ri].z, wb[ri].w};
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const float x = buf[BWD ? j - ri + NR - 1 : j + ri];
#pragma unroll
                for (int m = 0; m < MO; ++m) acc[m][j] += x * w[m];
            }
        }
    };
    const int T = (c_hi - c_lo) * nS;
    if (T > 0) {
        float b0[NW], b1[NW];
        float4 w0[NR], w1[NR];
        int c = c_lo, sj = 0;           // (c, sj) of the stage being issued
        auto adv = [&](int& cx, int& sx_) {
            if (++sx_ == nS) {
                sx_ = 0;
                ++cx;
            }
        };
        issue(b0, w0, c, sj);
        adv(c, sj);
        for (int t = 0; t < T; t += 2) {
            if (t + 1 < T) {
                issue(b1, w1, c, sj);
                adv(c, sj);
            }
            compute(b0, w0);
            if (t + 1 < T) {
                if (t + 2 < T) {
                    issue(b0, w0, c, sj);
                    adv(c, sj);
                }
                compute(b1, w1);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int m = 0; m < MO; ++m)
#pragma unroll
            for (int j = 0; j < PX; ++j) red[wave - 1][m * PX + j][pl] = acc[m][j];
    }
    __syncthreads();
    if (wave > 0 || !svalid) return;
    const int YhYw = a.Yh * a.Yw;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        if (sy0 + j >= P.Hs) break;
        const int py = (sy0 + j) * a.ostep + P.fy;
        const size_t yo = (size_t)n * a.M * YhYw + py * a.Yw + px;
#pragma unroll
        for (int m = 0; m < MO; ++m) {
            if (m < a.M) {
                float v = acc[m][j] + (red[0][m * PX + j][pl] + red[1][m * PX + j][pl]) + red[2][m * PX + j][pl];
                if (a.ksplit > 1) {   // raw fp32 partial sum; bias / activation happen in splitk_reduce_kernel
                    a.Ypart[(size_t)blockIdx.z * a.N * a.M * YhYw + yo + (size_t)m * YhYw] = v;
                    continue;
                }
                if (a.bias) v += a.bias[m];
                st1((TA*)a.Y + yo + (size_t)m * YhYw, act_apply(v, a.act, a.slope));
            }
        }
    }
}

// Variant for phases with few taps (<= 9, e.g. the stride phases of 4x4/s2 and 11x11/s4 data gradients): one
// thread per pixel, tap-outer loop; no tables, no cross-wave reduction.
template <int MODE, typename TA>
__global__ void __launch_bounds__(256) smallm_conv_fewtaps_kernel(IgemmArgs a) {
    constexpr unsigned ES = sizeof(TA);
    const PhaseArgs& P = a.ph[blockIdx.y];
    const int Ptot = P.Ptot;
    if ((int)(blockIdx.x * 256) >= Ptot) return;
    const int pg = blockIdx.x * 256 + threadIdx.x;
    const bool pvalid = pg < Ptot;
    const Geom g{a.Hg, a.Wg, a.sl, a.pad};
    const int HsWs = P.Hs * P.Ws, HgWg = a.Hg * a.Wg;
    int n = 0, py = 0, px = 0;
    if (pvalid) {
        n = pg / HsWs;
        const int rem = pg - n * HsWs;
        const int sy = rem / P.Ws;
        py = sy * a.ostep + P.fy;
        px = (rem - sy * P.Ws) * a.ostep + P.fx;
    }
    const int vbase = n * a.Cg * HgWg;
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.X, a.x_bytes);
    const float4* __restrict__ At = reinterpret_cast<const float4*>(P.A);  // [Kp][4]
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
    for (int ri = 0; ri < P.nR; ++ri) {
        for (int sj = 0; sj < P.nS; ++sj) {
            int off;
            const bool ok = tap_offset<MODE>(g, py, px, P.r0 + ri * a.tstep, P.s0 + sj * a.tstep, off) && pvalid;
            const unsigned voff = ok ? (unsigned)(vbase + off) * ES : OOB;
            const int kbase = (ri * P.nS + sj) * a.Cgp;
            int c = 0;
            for (; c + 8 <= a.Cg; c += 8) {
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) x[u] = ldx<TA>(rX, voff, (unsigned)((c + u) * HgWg) * ES);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float4 w = At[kbase + c + u];  // wave-uniform address -> scalar load
                    acc0 += x[u] * w.x; acc1 += x[u] * w.y; acc2 += x[u] * w.z; acc3 += x[u] * w.w;
                }
            }
            for (; c < a.Cg; ++c) {
                const float x = ldx<TA>(rX, voff, (unsigned)(c * HgWg) * ES);
                const float4 w = At[kbase + c];
                acc0 += x * w.x; acc1 += x * w.y; acc2 += x * w.z; acc3 += x * w.w;
            }
        }
    }
    if (!pvalid) return;
    const int YhYw = a.Yh * a.Yw;
    TA* Yp = (TA*)a.Y + (size_t)n * a.M * YhYw + py * a.Yw + px;
    const float out[4] = {acc0, acc1, acc2, acc3};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (m < a.M) {
            float v = out[m];
            if (a.bias) v += a.bias[m];
            st1(Yp + (size_t)m * YhYw, act_apply(v, a.act, a.slope));
        }
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
int launch_transpose4(const float* A, float* At, int M, int Kp, hipStream_t st) {
    hipLaunchKernelGGL(transpose4_kernel, dim3((Kp * 4 + 255) / 256), dim3(256), 0, st, A, At, M, Kp);
    PCGAN_LAUNCH_CHECK();
    return 0;
}
int launch_pack_strip(const float* A, float* Ws, int M, int Cg, int Cgp, int nR, int nS, hipStream_t st) {
    hipLaunchKernelGGL(pack_strip_kernel, dim3((Cg * nS * 32 + 255) / 256), dim3(256), 0, st, A, Ws, M, Cg, Cgp, nR, nS);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

// 3 modes x 2 storage types of: smallm_strip_kernel<MODE, NR = 4 | 7, MO = 3 | 4>, smallm_conv_fewtaps_kernel, smallm_conv_kernel
enum { SM_STRIP, SM_FEWTAPS, SM_GENERIC };
template <int MODE>
static void launch_mode(int kernel, const IgemmArgs& a, dim3 grid, int nr, int mo, hipStream_t st) {
    if (kernel == SM_FEWTAPS) LAUNCH_TA(a.dtype, smallm_conv_fewtaps_kernel, grid, a, MODE);
    else if (kernel == SM_GENERIC) LAUNCH_TA(a.dtype, smallm_conv_kernel, grid, a, MODE);
    else if (nr == 4 && mo == 3) LAUNCH_TA(a.dtype, smallm_strip_kernel, grid, a, MODE, 4, 3);
    else if (nr == 4) LAUNCH_TA(a.dtype, smallm_strip_kernel, grid, a, MODE, 4, 4);
    else if (mo == 3) LAUNCH_TA(a.dtype, smallm_strip_kernel, grid, a, MODE, 7, 3);
    else LAUNCH_TA(a.dtype, smallm_strip_kernel, grid, a, MODE, 7, 4);
}
static int launch_kernel(int mode, int kernel, const IgemmArgs& a, dim3 grid, int nr, int mo, hipStream_t st) {
    switch (mode == MODE_BWD_REFLECT ? MODE_BWD : mode) {   // no mirror-gather form here: the plain data gradient
        case MODE_FWD_ZERO: launch_mode<MODE_FWD_ZERO>(kernel, a, grid, nr, mo, st); break;
        case MODE_FWD_REFLECT: launch_mode<MODE_FWD_REFLECT>(kernel, a, grid, nr, mo, st); break;
        default: launch_mode<MODE_BWD>(kernel, a, grid, nr, mo, st); break;
    }
    PCGAN_LAUNCH_CHECK();
    return 0;
}

// vector-ALU path; ph[].A already holds the transposed [Kp][4] weights
// (tests/conv_f32_cases.py restates the kernel choice and the channel split below in Python: a retune here must be mirrored there)
int launch_smallm(int mode, IgemmArgs& a, int pmax, hipStream_t st, float* part_ws, size_t part_bytes) {
    PCGAN_CHECK(a.x_bytes < SM_INV, "small-M conv: gathered tensor must be < 1 GiB");
    for (int i = 0; i < a.nphase; ++i)
        PCGAN_CHECK(a.ph[i].nR <= 12 && a.ph[i].nS <= 12, "small-M conv: more than 12 taps per axis");
    // strip kernel: unit pixel stride along the column, columns long enough for 8-pixel strips, <= 7 row taps
    int maxR = 0, minH = 1 << 30, maxstrips = 0, maxtaps = 0;
    for (int i = 0; i < a.nphase; ++i) {
        maxR = a.ph[i].nR > maxR ? a.ph[i].nR : maxR;
        minH = a.ph[i].Hs < minH ? a.ph[i].Hs : minH;
        const int ns = a.N * ((a.ph[i].Hs + 7) / 8) * a.ph[i].Ws;
        maxstrips = ns > maxstrips ? ns : maxstrips;
        maxtaps = a.ph[i].nR * a.ph[i].nS > maxtaps ? a.ph[i].nR * a.ph[i].nS : maxtaps;
    }
    const int nr = maxR <= 4 ? 4 : 7, mo = a.M <= 3 ? 3 : 4;   // the strip kernel's NR / MO: launched and recorded from these
    const bool unit = mode == MODE_BWD || mode == MODE_BWD_REFLECT || (a.sl == 0 && a.ostep == 1);
    if (unit && maxR >= 3 && maxR <= 7 && minH >= 8) {   // (1-2 row taps: nothing to reuse)
        // few strips but many channels (the last PatchGAN conv, 512 -> 1 on 14x14): cut the channels over blockIdx.z
        const int wgs = ((maxstrips + 63) / 64) * a.nphase;
        int ks = 1;
        const size_t out_elems = (size_t)a.N * a.M * a.Yh * a.Yw;
        if (part_ws != nullptr && a.nphase == 1 && wgs < 128 && a.Cg >= 64) {
            ks = 256 / wgs;
            if (ks > 8) ks = 8;
            if (ks > a.Cg / 16) ks = a.Cg / 16;
            if ((size_t)ks * out_elems * 4 > part_bytes) ks = 1;
        }
        a.ksplit = ks;
        a.Ypart = part_ws;
        // small-M record: bm = kernel (1 strip | 2 few taps | 3 generic), bp = NR * 10 + MO of the strip instantiation
        record_launch(PCGAN_IGEMM_SMALLM, mode, 1, nr * 10 + mo, ks, a.nphase);
        const dim3 gs((unsigned)((maxstrips + 63) / 64), (unsigned)a.nphase, (unsigned)ks);
        if (int e = launch_kernel(mode, SM_STRIP, a, gs, nr, mo, st)) return e;
        if (ks > 1 && launch_splitk_reduce(a.dtype, st, part_ws, a.Y, a.bias, ks, out_elems, a.M, a.Yh * a.Yw, a.act, a.slope)) return 2;
        return 0;
    }
    record_launch(PCGAN_IGEMM_SMALLM, mode, maxtaps <= 9 ? 2 : 3, 0, 1, a.nphase);
    if (maxtaps <= 9) return launch_kernel(mode, SM_FEWTAPS, a, dim3((unsigned)((pmax + 255) / 256), (unsigned)a.nphase), nr, mo, st);
    return launch_kernel(mode, SM_GENERIC, a, dim3((unsigned)((pmax + 63) / 64), (unsigned)a.nphase), nr, mo, st);
}

}  // namespace pcgan
