// Implicit-GEMM convolution family for gfx950 (MI355X), fp32 in / fp32 accumulate on the matrix cores
// (v_mfma_f32_32x32x2_f32, exact f32 fma chain): the HOST side -- descriptor checks, tile choice, K split, workspace layout,
// weight packing, the launch record and every entry point of the C-ABI.
//
//   forward          Y[n][m][oy][ox] = act( sum_k A[m][k] * G(k; n,oy,ox) + bias[m] )
//   backward-data    the same kernels with the transposed gather; stride phases (only the structurally non-zero taps)
//                    and, for reflection padding, row classes with folded weights are phases of ONE launch
//   backward-weight  Wp[m][k] = sum_pix dY[m][pix] * G(k; pix)   (split over pixel ranges, deterministic second-pass
//                    sum, no atomics)
//
// Layout: activations NCHW fp32.  The GEMM "N" dimension is the flattened pixel index, so consecutive lanes touch
// consecutive addresses of one channel plane (coalesced loads and epilogue stores: the 32x32 accumulator has its COLUMN
// on the lane, so the pixel is the column and the output channel the row).
//
// Kernels, each in the unit that owns its launcher (igemm.h declares the launchers):
//   igemm_mfma.hip   igemm2_kernel -- channel counts that are multiples of 16: the step's hot fp32 kernel
//                    igemm_kernel  -- generic K order (3-/4-channel stems, odd channel counts, > 25 taps)
//   hgemm.hip        hgemm_kernel  -- the fp16 two-piece / bf16 form of igemm2_kernel, and the pre-split of its weights
//   smallm_conv.hip  smallm_*      -- <= 4 output channels (vector ALU); transpose4 / pack_strip: their weight layouts
//   wgrad_igemm.hip  wgrad2_kernel / wgrad_kernel / smallm_wgrad* / wgrad_reduce -- the weight gradient
//   here             repack_* (weight packing: pcgan_conv2d_pack_weights, once per optimizer step), splitk_reduce, reflect_fold
// What bounds them and why they are written the way they are: DESIGN.md section 3.
//
// Reference call sites replaced: see include/pcgan_hip.h.
#include "igemm.h"
#include <stdlib.h>
#include <mutex>

namespace pcgan {

// y = act( sum_s part[s] + bias[channel] ) over the split-K partial sums
template <typename TA>
__global__ void splitk_reduce_kernel(const float* __restrict__ part, TA* __restrict__ y, const float* __restrict__ bias,
                                     int ks, size_t n, int M, int HW, int act, float slope) {
    const size_t n4 = (n & 3) ? 0 : (n >> 2);  // 16-byte path only when every split's base stays aligned
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 acc = reinterpret_cast<const float4*>(part)[i];
        for (int s = 1; s < ks; ++s) {
            const float4 v = reinterpret_cast<const float4*>(part + (size_t)s * n)[i];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        float o[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t e = i * 4 + u;
            if (bias) o[u] += bias[(e / HW) % M];
            o[u] = act_apply(o[u], act, slope);
        }
        st4(y + 4 * i, make_float4(o[0], o[1], o[2], o[3]));
    }
    for (size_t e = (n4 << 2) + blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += stride) {
        float acc = 0.f;
        for (int s = 0; s < ks; ++s) acc += part[(size_t)s * n + e];
        if (bias) acc += bias[(e / HW) % M];
        st1(y + e, act_apply(acc, act, slope));
    }
}

// ------------------------------------------------------------------------------------
// weight re-layout kernels
// ------------------------------------------------------------------------------------
// forward: A[k][tap][c] (Cgp-padded) from w[K][C][R][S]
// chunked != 0 (igemm2_kernel): K order (16-channel chunk, tap, channel-in-chunk), so the 9..49 taps of one
// channel chunk are consecutive K stages and re-read the same small input tile from L1/L2 instead of
// streaming the whole input once per tap from beyond L2
__global__ void repack_fwd_kernel(const float* __restrict__ w, float* __restrict__ A, int K, int C, int Cgp,
                                  int RS, int chunked) {
    const int Kp = RS * Cgp;
    const size_t total = (size_t)K * Kp;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i / Kp);
        const int j = (int)(i - (size_t)k * Kp);
        int tap, c;
        if (chunked) {
            const int t2 = j >> 4;
            const int cc = t2 / RS;
            tap = t2 - cc * RS;
            c = cc * 16 + (j & 15);
        } else {
            tap = j / Cgp;
            c = j - tap * Cgp;
        }
        A[i] = (c < C) ? w[((size_t)k * C + c) * RS + tap] : 0.f;
    }
}
// backward-data, one stride phase: A[c][(ri,sj)][k] (Kgp-padded) from w[K][C][R][S]
__global__ void repack_bwd_kernel(const float* __restrict__ w, float* __restrict__ A, int K, int C, int Kgp,
                                  int R, int S, int r0, int s0, int tstep, int nR, int nS, int chunked, int fold) {
    const int Kp = nR * nS * Kgp;
    const size_t total = (size_t)C * Kp;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i / Kp);
        const int j = (int)(i - (size_t)c * Kp);
        int t, k;
        if (chunked) {
            const int t2 = j >> 4;
            const int kc = t2 / (nR * nS);
            t = t2 - kc * (nR * nS);
            k = kc * 16 + (j & 15);
        } else {
            t = j / Kgp;
            k = j - t * Kgp;
        }
        const int ri = t / nS, sj = t - ri * nS;
        const int r = r0 + ri * tstep, s = s0 + sj * tstep;
        float v = (k < K) ? w[(((size_t)k * C + c) * R + r) * S + s] : 0.f;
        // reflection pad 1, 3 taps: output row 1 also receives padded row 0 = input row 1 through tap 0, from the
        // source row that its tap 2 reads (fold 1); output row H-2 the other way round (fold 2)
        if (k < K && fold == 1 && r == R - 1) v += w[(((size_t)k * C + c) * R + 0) * S + s];
        if (k < K && fold == 2 && r == 0) v += w[(((size_t)k * C + c) * R + (R - 1)) * S + s];
        A[i] = v;
    }
}

// all phases / row classes of one data-gradient weight pack in ONE launch (blockIdx.y = entry): these kernels are
// launch-latency bound (a few microseconds each, up to 16 per layer)
struct PackBwdArgs {
    const float* w;
    int K, C, Kgp, R, S, tstep, chunked, n;
    struct Entry {
        float* A;
        int r0, s0, nR, nS, fold;
    } e[16];
};
__global__ void repack_bwd_multi_kernel(PackBwdArgs a) {
    const PackBwdArgs::Entry& E = a.e[blockIdx.y];
    const int RS = E.nR * E.nS;
    const int Kp = RS * a.Kgp;
    const size_t total = (size_t)a.C * Kp;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i / Kp);
        const int j = (int)(i - (size_t)c * Kp);
        int t, k;
        if (a.chunked) {
            const int t2 = j >> 4;
            const int kc = t2 / RS;
            t = t2 - kc * RS;
            k = kc * 16 + (j & 15);
        } else {
            t = j / a.Kgp;
            k = j - t * a.Kgp;
        }
        const int ri = t / E.nS, sj = t - ri * E.nS;
        const int r = E.r0 + ri * a.tstep, sx = E.s0 + sj * a.tstep;
        float v = 0.f;
        if (k < a.K) {
            const float* wk = a.w + ((size_t)k * a.C + c) * a.R * a.S;
            v = wk[r * a.S + sx];
            if (E.fold == 1 && r == a.R - 1) v += wk[sx];                       // see repack_bwd_kernel
            if (E.fold == 2 && r == 0) v += wk[(a.R - 1) * a.S + sx];
        }
        E.A[i] = v;
    }
}

// fold the gradient of a reflection-padded tensor back onto the unpadded tensor (+ bias[plane % C], once per element: the padded
// grid must be written WITHOUT the bias, every mirror image would carry it again)
// grid = (row groups, planes): one thread = 4 consecutive pixels of one row, plane-local 32-bit index math
template <typename TA>
__global__ void reflect_fold_kernel(const TA* __restrict__ t, TA* __restrict__ dx, int NC, int H, int W,
                                    int pad, const float* __restrict__ bias, int C) {
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int W4 = (W + 3) >> 2;
    const TA* tp = t + (size_t)blockIdx.y * Hp * Wp;
    TA* dp = dx + (size_t)blockIdx.y * H * W;
    const float bv = bias ? bias[blockIdx.y % C] : 0.f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H * W4; i += gridDim.x * blockDim.x) {
        const int y = i / W4, x0 = (i - y * W4) * 4;
        int ys[3], ny = 0;
        ys[ny++] = y + pad;
        if (y >= 1 && y <= pad) ys[ny++] = pad - y;
        if (y >= H - 1 - pad && y <= H - 2) ys[ny++] = pad + 2 * (H - 1) - y;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < ny; ++a) {
            const TA* row = tp + ys[a] * Wp;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                if (x >= W) continue;
                float v = ld1(row + x + pad);
                if (x >= 1 && x <= pad) v += ld1(row + pad - x);
                if (x >= W - 1 - pad && x <= W - 2) v += ld1(row + pad + 2 * (W - 1) - x);
                acc[j] += v;
            }
        }
        if (bias) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += bv;
        }
        if ((W & 3) == 0) {
            st4(dp + y * W + x0, make_float4(acc[0], acc[1], acc[2], acc[3]));
        } else {
            for (int j = 0; j < 4 && x0 + j < W; ++j) st1(dp + y * W + x0 + j, acc[j]);
        }
    }
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
int launch_splitk_reduce(int dtype, hipStream_t st, const float* part, void* y, const float* bias, int ks, size_t out_elems, int M,
                         int HW, int act, float slope) {
    const dim3 b(capped_blocks(out_elems / 4, 256, 4096));
    if (dtype == PCGAN_BF16)
        hipLaunchKernelGGL(splitk_reduce_kernel<bf16>, b, dim3(256), 0, st, part, (bf16*)y, bias, ks, out_elems, M, HW, act, slope);
    else
        hipLaunchKernelGGL(splitk_reduce_kernel<float>, b, dim3(256), 0, st, part, (float*)y, bias, ks, out_elems, M, HW, act, slope);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

static int check_desc(const pcgan_conv_desc* d) {
    PCGAN_CHECK(d != nullptr, "conv: null descriptor");
    PCGAN_CHECK(d->N > 0 && d->C > 0 && d->H > 0 && d->W > 0 && d->K > 0 && d->R > 0 && d->S > 0,
                "conv: non-positive dimension");
    PCGAN_CHECK(ilog2_exact(d->stride) >= 0 && d->stride <= 4, "conv: stride %d unsupported (1,2,4)", d->stride);
    PCGAN_CHECK(d->pad_mode == 0 || d->pad_mode == 1, "conv: pad_mode %d", d->pad_mode);
    PCGAN_CHECK(d->dtype == PCGAN_F32 || d->dtype == PCGAN_BF16, "conv: dtype %d (PCGAN_F32 / PCGAN_BF16)", d->dtype);
    const int P = (d->H + 2 * d->pad - d->R) / d->stride + 1, Q = (d->W + 2 * d->pad - d->S) / d->stride + 1;
    PCGAN_CHECK(P == d->P && Q == d->Q, "conv: output dims %dx%d do not match geometry %dx%d", d->P, d->Q, P, Q);
    if (d->pad_mode == 1)
        PCGAN_CHECK(d->pad < d->H && d->pad < d->W, "conv: reflection pad %d >= input size", d->pad);
    // range-checked buffer loads address tensors with 32-bit byte offsets; the out-of-range marker is 2 GiB
    const size_t xin = (size_t)d->N * d->C * (d->H + 2 * d->pad) * (d->W + 2 * d->pad) * 4;
    const size_t yout = (size_t)d->N * d->K * d->P * d->Q * 4;
    PCGAN_CHECK(xin < (1ull << 31) && yout < (1ull << 31),
                "conv: tensor of %zu bytes exceeds the 2 GiB addressing limit of one launch (split the batch)",
                xin > yout ? xin : yout);
    PCGAN_CHECK((size_t)d->K * round4(d->C) * d->R * d->S * 4 < (1ull << 31) &&
                    (size_t)d->C * round4(d->K) * d->R * d->S * 4 < (1ull << 31), "conv: weight tensor too large");
    PCGAN_CHECK(d->R * d->S <= 512, "conv: filter too large");
    return 0;
}

// (tests/conv_f32_cases.py restates chunked_k, cg4_k, may_split, choose_tile, bwd_plan and the part-workspace rules in Python to pin the
// instantiation each test case runs: a retune here must be mirrored there)
// tile choice: the largest tile that still gives the 256 CUs >= ~1.5 workgroups each; problems with few
// pixels but a long K loop (the encoder's 7x7 / 14x14 stages, the PatchGAN's 16x16 stage) keep the big tile
// and are cut along K instead (split-K, partial sums reduced by splitk_reduce_kernel)
// chunked K order / igemm2_kernel: gathered channel count a multiple of 16, taps fit the LDS tables, MFMA path
static inline bool chunked_k(int Cg, int M, int R, int S) { return (Cg % 16) == 0 && M > 4 && R * S <= NTAP_FWD; }
// 4-channel stages (igemm2_kernel<.., 4>): 3-/4-channel gathered tensor, MFMA path, taps fit the table; weights stay in
// the generic (tap, channel) order
static inline bool cg4_k(int Cg, int M, int R, int S) { return round4(Cg) == 4 && M > 4 && R * S <= NTAP_CG4; }
static inline long tile_blocks(int M, int ptot_max, int nphase, int mm, int pp) {
    return (long)((M + mm - 1) / mm) * ((ptot_max + pp - 1) / pp) * nphase;
}
static inline long split_below() { return 192; }     // tiles (BP = 128) below which a long-K layer is cut along K (profiles/r01_tile_sweep.txt)
static inline bool may_split(int M, int ptot_max, int nphase) {
    if (option(OPT_HGEMM_KS) > 1) return M > 4;      // forced K split (measurement): every layer gets the room
    const int m = M > 64 ? 128 : (M > 32 ? 64 : 32);
    return M > 4 && tile_blocks(M, ptot_max, nphase, m, 128) < split_below();
}
static void choose_tile(int M, int ptot_max, int nphase, int nst, bool allow_split, int* bm, int* bp, int* ks) {
    int m = M > 64 ? 128 : (M > 32 ? 64 : 32);
    int p = 128;
    *ks = 1;
    // options "hgemm_tile" / "hgemm_ks" (measurement, scripts/sweep_hgemm.py): a forced tile and K split for layers with > 32 rows
    const int ft = option(OPT_HGEMM_TILE), fk = option(OPT_HGEMM_KS);
    if ((ft || fk) && M > 32) {
        if (ft) {
            m = ft / 1000;
            p = ft % 1000;
        } else {      // the heuristic's tile for an unsplit launch
            if (tile_blocks(M, ptot_max, nphase, m, p) < 384) p = 64;
            if (m == 128 && tile_blocks(M, ptot_max, nphase, m, p) < 384) m = 64;
        }
        if (M <= 64 && m == 128) m = 64;
        int k = fk > 0 ? fk : 1;
        if (!allow_split) k = 1;
        if (k > nst / 4) k = nst / 4 > 0 ? nst / 4 : 1;
        *bm = m;
        *bp = p;
        *ks = k;
        return;
    }
    if (allow_split && may_split(M, ptot_max, nphase) && nst >= 32) {
        const long b = tile_blocks(M, ptot_max, nphase, m, 128);
        int k = (int)(512 / b);
        if (k > 8) k = 8;
        if (k > nst / 8) k = nst / 8;
        if (k >= 2) {
            *bm = m;
            *bp = 128;
            *ks = k;
            return;
        }
    }
    if (m >= 64 && tile_blocks(M, ptot_max, nphase, m, p) < 384) p = 64;
    if (m == 128 && tile_blocks(M, ptot_max, nphase, m, p) < 384) m = 64;
    *bm = m;
    *bp = p;
}

// host-side record of the last launch launch_igemm decided (pcgan_igemm_last_launch): kernel form, mode, tile and K split as launched,
// after every clamp -- a forced hgemm_tile / hgemm_ks may be cut by the shape, so a test reads back which instantiation it checked
static std::mutex g_launch_mu;
static int g_launch[PCGAN_IGEMM_LAUNCH_INFO] = {0};
void record_launch(int form, int mode, int bm, int bp, int ks, int nphase) {
    std::lock_guard<std::mutex> lk(g_launch_mu);
    const int seq = g_launch[0] + 1;
    const int v[PCGAN_IGEMM_LAUNCH_INFO] = {seq, form, mode, bm, bp, ks, nphase};
    for (int i = 0; i < PCGAN_IGEMM_LAUNCH_INFO; ++i) g_launch[i] = v[i];
}

// one convolution launch: kernel family, tile and K split; the unit that owns the kernel picks the instantiation
static int launch_igemm(int mode, IgemmArgs& a, hipStream_t st, float* part_ws = nullptr, size_t part_bytes = 0) {
    int pmax = 0;
    for (int i = 0; i < a.nphase; ++i) pmax = a.ph[i].Ptot > pmax ? a.ph[i].Ptot : pmax;
    if (pmax <= 0 || a.nphase <= 0) return 0;
    if (a.M <= 4) return launch_smallm(mode, a, pmax, st, part_ws, part_bytes);
    int bm, bp, ks;
    int nst_min = 1 << 30;
    for (int i = 0; i < a.nphase; ++i) nst_min = (a.ph[i].Kp + 15) / 16 < nst_min ? (a.ph[i].Kp + 15) / 16 : nst_min;
    const size_t out_elems = (size_t)a.N * a.M * a.Yh * a.Yw;
    choose_tile(a.M, pmax, a.nphase, nst_min, part_ws != nullptr, &bm, &bp, &ks);
    if (ks > 1 && (size_t)ks * out_elems * 4 > part_bytes) ks = 1;
    a.ksplit = ks;
    a.Ypart = part_ws;
    const dim3 grid((unsigned)(((a.M + bm - 1) / bm) * ((pmax + bp - 1) / bp)), (unsigned)a.nphase, (unsigned)ks);
    a.tstart[0] = 0;
    for (int i = 0; i < a.nphase; ++i) a.tstart[i + 1] = a.tstart[i] + (a.ph[i].Ptot + bp - 1) / bp;
    const dim3 grid2((unsigned)(((a.M + bm - 1) / bm) * a.tstart[a.nphase]), 1u, (unsigned)ks);
    const bool cg16 = a.chunked == 1, cg4 = a.chunked == 2;
    PCGAN_CHECK(cg16 || mode != MODE_BWD_REFLECT, "igemm: fused reflect data-gradient needs K %% 16 == 0");
    if (cg4) {
        PCGAN_CHECK(a.Cgp == 4, "igemm: 4-channel stages need a 3-/4-channel tensor");
        for (int i = 0; i < a.nphase; ++i)
            PCGAN_CHECK(a.ph[i].nR * a.ph[i].nS <= NTAP_CG4, "igemm: 4-channel stages: more than %d taps", NTAP_CG4);
    }
    if (cg16) {
        PCGAN_CHECK((a.Cg % 16) == 0, "igemm: chunked K order needs a multiple of 16 channels");
        for (int i = 0; i < a.nphase; ++i)
            PCGAN_CHECK(a.ph[i].nR * a.ph[i].nS <= (mode == MODE_BWD_REFLECT ? NTAP_MIR : NTAP_FWD) && (a.ph[i].Kp % 16) == 0,
                        "igemm: chunked K order: bad phase");
    }
    // bf16 tensors take the one-product bf16 MFMA form of the kernel whenever the shape allows (option "hgemm_bf16" = 0: the fp32 MFMA kernels)
    const bool half = a.dtype == PCGAN_BF16 && option(OPT_HGEMM_BF16) != 0;
    if ((half || (a.hsplit && a.dtype == PCGAN_F32)) && cg16 && mode != MODE_BWD_REFLECT && bm >= 64) {
        // fp16 two-piece form (fp32 tensors) / bf16 form (bf16 tensors) of the same launch: same tiles, phases, K splits
        record_launch(half ? PCGAN_IGEMM_HGEMM_BF16 : PCGAN_IGEMM_HGEMM_F16X2, mode, bm, bp, ks, a.nphase);
        if (int e = launch_hgemm(mode, a, bm, bp, grid2, st)) return e;
    } else {
        record_launch(cg16 ? PCGAN_IGEMM_IGEMM2_CG16 : (cg4 ? PCGAN_IGEMM_IGEMM2_CG4 : PCGAN_IGEMM_GENERIC), mode, bm, bp, ks, a.nphase);
        if (int e = launch_igemm_f32(mode, a, bm, bp, grid, grid2, st)) return e;
    }
    if (ks > 1 && launch_splitk_reduce(a.dtype, st, part_ws, a.Y, a.bias, ks, out_elems, a.M, a.Yh * a.Yw, a.act, a.slope)) return 2;
    return 0;
}

}  // namespace pcgan

using namespace pcgan;

// room for split-K partial sums (upper bound: 8 splits), 0 when the problem never splits
static size_t fwd_part_bytes(const pcgan_conv_desc* d) {
    const int ptot = d->N * d->P * d->Q;
    if (d->K <= 4) return (ptot <= 65536 && d->C >= 64) ? align_up((size_t)8 * d->K * ptot * 4, 256) : 0;   // strip kernel, channel split
    return may_split(d->K, ptot, 1) ? align_up((size_t)8 * d->N * d->K * d->P * d->Q * 4, 256) : 0;
}
static size_t bwd_part_bytes(const pcgan_conv_desc* d) {
    const int s = d->stride;
    const int pmax = d->N * ((d->H + s - 1) / s) * ((d->W + s - 1) / s);
    return may_split(d->C, pmax, s * s) ? align_up((size_t)8 * d->N * d->C * d->H * d->W * 4, 256) : 0;
}
static size_t fwd_base_bytes(const pcgan_conv_desc* d) {
    // A matrix (+ small-M path: RS*C*16 bytes for the [k][4] transposed weights and S*C*128 for the strip layout)
    return align_up((size_t)d->K * d->R * d->S * round4(d->C) * 4 + (size_t)d->R * d->S * round4(d->C) * 16 +
                    (d->K <= 4 ? (size_t)d->S * d->C * 128 : 0), 256);
}
// fused reflect data gradient (mirror images gathered on the unpadded grid) and its row-folded form (pad 1, 3 rows)
static bool bwd_fused_reflect(const pcgan_conv_desc* d) {
    return d->pad_mode == 1 && chunked_k(d->K, d->C, d->R, d->S) && d->R * d->S <= NTAP_MIR && d->H >= 2 * d->pad + 2 &&
           d->W >= 2 * d->pad + 2;
}
static bool bwd_rowfold(const pcgan_conv_desc* d) { return bwd_fused_reflect(d) && d->pad == 1 && d->R == 3 && d->stride == 1; }
static size_t bwd_base_bytes(const pcgan_conv_desc* d) {
    const size_t a = (size_t)d->C * d->R * d->S * round4(d->K) * 4;
    // small-M path: [k][4] transposed copies + strip layout (sum over the stride phases of nS = stride * S columns)
    return align_up((bwd_rowfold(d) ? 3 * a : a) + (size_t)d->R * d->S * round4(d->K) * 16 +
                    (d->C <= 4 ? (size_t)d->stride * d->S * d->K * 128 : 0), 256);
}

extern "C" size_t pcgan_conv2d_workspace_bytes(const pcgan_conv_desc* d, int pass) {
    if (!d) return 0;
    const size_t RS = (size_t)d->R * d->S;
    if (pass == PCGAN_PASS_FWD) return fwd_base_bytes(d) + fwd_part_bytes(d);
    if (pass == PCGAN_PASS_BWD_DATA) {
        size_t b = bwd_base_bytes(d) + bwd_part_bytes(d);
        if (d->pad_mode == 1)
            b += align_up((size_t)d->N * d->C * (d->H + 2 * d->pad) * (d->W + 2 * d->pad) * 4, 256);
        return b;
    }
    int cps;
    const int splits = wgrad_splits(d, &cps);
    return align_up((size_t)splits * d->K * RS * round4(d->C) * 4, 256);
}

// forward weight pack: A[K][Kp] (+ its [Kp][4] transpose behind it for the small-M path)
static int pack_fwd(const pcgan_conv_desc* d, const float* w, float* A, hipStream_t st) {
    const int Cgp = round4(d->C), RS = d->R * d->S;
    const size_t total = (size_t)d->K * RS * Cgp;
    hipLaunchKernelGGL(repack_fwd_kernel, dim3(capped_blocks(total, 256, 4096)), dim3(256), 0, st, w, A, d->K, d->C, Cgp, RS,
                       (int)chunked_k(d->C, d->K, d->R, d->S));
    PCGAN_LAUNCH_CHECK();
    if (d->K <= 4) {
        if (int e = launch_transpose4(A, A + total, d->K, RS * Cgp, st)) return e;
        if (int e = launch_pack_strip(A, A + total + (size_t)RS * Cgp * 4, d->K, d->C, Cgp, d->R, d->S, st)) return e;
    }
    return 0;
}

// operand maxima of the fp16 two-piece form (null: the fp32 MFMA kernels)
struct HsplitOpt {
    const float* x_amax;
    int n_amax;
    const float* w_amax;
};
static void apply_hsplit(IgemmArgs& a, const HsplitOpt* hs) {
    if (!hs) return;
    a.hsplit = 1; a.x_amax = hs->x_amax; a.x_namax = hs->n_amax; a.w_amax = hs->w_amax;
    a.ovf = pcgan::nonfinite_counter();
}

static int conv2d_fwd_impl(const pcgan_conv_desc* d, const void* x, const float* w, const float* packed,
                           const float* bias, void* y, int act, float slope, void* ws, size_t ws_bytes,
                           pcgan_stream_t s, const HsplitOpt* hs = nullptr) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(x && (w || packed) && y, "conv2d_fwd: null pointer");
    PCGAN_CHECK(ws && ws_bytes >= pcgan_conv2d_workspace_bytes(d, PCGAN_PASS_FWD),
                "conv2d_fwd: workspace too small (%zu)", ws_bytes);
    hipStream_t st = (hipStream_t)s;
    const int Cgp = round4(d->C), RS = d->R * d->S;
    float* A = packed ? const_cast<float*>(packed) : (float*)ws;
    if (!packed && pack_fwd(d, w, A, st)) return 2;
    IgemmArgs a;
    memset(&a, 0, sizeof(a));
    a.X = x; a.Y = y; a.bias = bias; a.dtype = d->dtype;
    a.M = d->K; a.N = d->N; a.Cg = d->C; a.Cgp = Cgp; a.Hg = d->H; a.Wg = d->W;
    a.Yh = d->P; a.Yw = d->Q;
    a.ostep = 1; a.sl = ilog2_exact(d->stride); a.pad = d->pad; a.tstep = 1;
    a.act = act; a.slope = slope;
    a.x_bytes = (unsigned)((size_t)d->N * d->C * d->H * d->W * esz(d));
    a.nphase = 1;
    a.chunked = chunked_k(d->C, d->K, d->R, d->S) ? 1 : (cg4_k(d->C, d->K, d->R, d->S) ? 2 : 0);
    apply_hsplit(a, hs);
    PhaseArgs& p = a.ph[0];
    p.A = A; p.Kp = RS * Cgp; p.Hs = d->P; p.Ws = d->Q; p.fy = 0; p.fx = 0;
    if (d->K <= 4) {  // small-M path reads the weights as [k][4] / [c][ri][8][4]
        p.A = A + (size_t)d->K * RS * Cgp;
        p.As = p.A + (size_t)RS * Cgp * 4;
    }
    p.r0 = 0; p.s0 = 0; p.nR = d->R; p.nS = d->S; p.Ptot = d->N * d->P * d->Q;
    float* part = fwd_part_bytes(d) ? (float*)((char*)ws + fwd_base_bytes(d)) : nullptr;
    return launch_igemm(d->pad_mode == 1 ? MODE_FWD_REFLECT : MODE_FWD_ZERO, a, st, part, fwd_part_bytes(d));
}

extern "C" int pcgan_conv2d_fwd(const pcgan_conv_desc* d, const void* x, const float* w, const float* bias,
                                void* y, int act, float slope, void* ws, size_t ws_bytes, pcgan_stream_t s) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(w, "conv2d_fwd: null weight pointer");
    return conv2d_fwd_impl(d, x, w, nullptr, bias, y, act, slope, ws, ws_bytes, s);
}
extern "C" int pcgan_conv2d_fwd_packed(const pcgan_conv_desc* d, const void* x, const float* packed,
                                       const float* bias, void* y, int act, float slope, void* ws, size_t ws_bytes,
                                       pcgan_stream_t s) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(packed, "conv2d_fwd_packed: null packed-weight pointer");
    pcgan::TimerScope timer(pcgan::timer_kind_res(d, pcgan::TIMER_RES_FWD), (hipStream_t)s);
    return conv2d_fwd_impl(d, x, nullptr, packed, bias, y, act, slope, ws, ws_bytes, s);
}

namespace pcgan {
// dx = the gradient of a reflection-padded tensor `padded` [NC][H + 2 pad][W + 2 pad] folded back onto the unpadded grid
int launch_reflect_fold(const void* padded, void* dx, int NC, int H, int W, int pad, int dtype, hipStream_t st, const float* bias, int C) {
    PCGAN_CHECK(NC <= 65535, "conv2d_bwd_data: more than 65535 planes in the reflect fold");
    const dim3 grid((H * ((W + 3) / 4) + 255) / 256, NC);
    if (dtype == PCGAN_BF16)
        hipLaunchKernelGGL(reflect_fold_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)padded, (bf16*)dx, NC, H, W, pad, bias, C);
    else
        hipLaunchKernelGGL(reflect_fold_kernel<float>, grid, dim3(256), 0, st, (const float*)padded, (float*)dx, NC, H, W, pad, bias, C);
    PCGAN_LAUNCH_CHECK();
    return 0;
}
}  // namespace pcgan

// The phases of one data-gradient launch and where their weights lie in the packed buffer -- the one place that knows; the
// packer, the launch and the pre-split of pcgan_conv2d_hgemm_pack all walk this list.
//   reflection padding: the mirror images are gathered directly (fused: needs K % 16 == 0 and H, W >= 2 pad + 2; with pad 1 and
//   3 rows the row mirrors are folded into the weights of three row classes, `rowfold`); otherwise the gradient of the PADDED
//   input is computed (`padded`: pad 0 on the larger grid H x W) and folded back.
//   Else one phase per (y % stride, x % stride) with only the taps that are structurally non-zero for it.
struct BwdPhase {
    int fy, fx, r0, s0, nR, nS, Hs, Ws;
    int fold;                     // rowfold: 0 = rows without a mirror image | 1 = row 1 | 2 = row H-2
    size_t a_off, at_off, as_off; // floats from the start of the packed buffer: A | small-M: its [k][4] transpose | strip layout
};
struct BwdPlan {
    bool fused, rowfold, padded;
    int H, W, pad;                // the grid the launch writes
    bool need_zero;               // some pixels belong to no phase (e.g. 1x1 stride 2)
    int n;
    BwdPhase ph[16];
};
static void bwd_plan(const pcgan_conv_desc* d, BwdPlan& pl) {
    memset(&pl, 0, sizeof(pl));
    pl.fused = bwd_fused_reflect(d);
    pl.rowfold = bwd_rowfold(d);
    pl.padded = d->pad_mode == 1 && !pl.fused;
    const int H = pl.H = pl.padded ? d->H + 2 * d->pad : d->H;
    const int W = pl.W = pl.padded ? d->W + 2 * d->pad : d->W;
    const int pad = pl.pad = pl.padded ? 0 : d->pad;
    const int stv = d->stride, Kgp = round4(d->K), RS = d->R * d->S;
    if (pl.rowfold) {
        for (int f = 0; f < 3; ++f) {
            BwdPhase& p = pl.ph[pl.n++];
            p.nR = d->R; p.nS = d->S; p.Ws = W; p.fold = f;
            p.Hs = f == 0 ? H - 2 : 1;
            p.fy = f == 0 ? 0 : (f == 1 ? 1 : H - 2);
            p.a_off = (size_t)f * d->C * RS * Kgp;
        }
        return;
    }
    size_t a_off = 0;
    size_t at_off = (size_t)d->C * RS * Kgp;          // transposed copies for the small-M path live behind the A's
    size_t as_off = at_off + (size_t)RS * Kgp * 4;    // ... and the strip layouts behind those
    for (int fy = 0; fy < stv; ++fy) {
        for (int fx = 0; fx < stv; ++fx) {
            const int r0 = (fy + pad) % stv, s0 = (fx + pad) % stv;
            const int nR = r0 < d->R ? (d->R - r0 + stv - 1) / stv : 0;
            const int nS = s0 < d->S ? (d->S - s0 + stv - 1) / stv : 0;
            const int Hs = fy < H ? (H - fy + stv - 1) / stv : 0;
            const int Ws = fx < W ? (W - fx + stv - 1) / stv : 0;
            if (Hs * Ws == 0) continue;
            if (nR * nS == 0) {
                pl.need_zero = true;
                continue;
            }
            const BwdPhase p = {fy, fx, r0, s0, nR, nS, Hs, Ws, 0, a_off, at_off, as_off};
            pl.ph[pl.n++] = p;
            a_off += (size_t)d->C * nR * nS * Kgp;
            at_off += (size_t)nR * nS * Kgp * 4;
            as_off += (size_t)d->K * nS * 32;
        }
    }
}

// data-gradient weight pack into `packed` (pcgan_conv2d_packed_bytes): small-M one phase after the other (the [k][4] and strip
// layouts are derived from A right away), otherwise every phase / row class in one launch
static int pack_bwd(const pcgan_conv_desc* d, const BwdPlan& pl, const float* w, float* packed, hipStream_t st) {
    const int Kgp = round4(d->K);
    const int chunked = (int)chunked_k(d->K, d->C, d->R, d->S);
    if (d->C <= 4) {
        for (int i = 0; i < pl.n; ++i) {
            const BwdPhase& p = pl.ph[i];
            float* A = packed + p.a_off;
            const size_t total = (size_t)d->C * p.nR * p.nS * Kgp;
            hipLaunchKernelGGL(repack_bwd_kernel, dim3(capped_blocks(total, 256, 4096)), dim3(256), 0, st, w, A, d->K, d->C, Kgp, d->R,
                               d->S, p.r0, p.s0, d->stride, p.nR, p.nS, chunked, 0);
            PCGAN_LAUNCH_CHECK();
            if (int e = launch_transpose4(A, packed + p.at_off, d->C, p.nR * p.nS * Kgp, st)) return e;
            if (int e = launch_pack_strip(A, packed + p.as_off, d->C, d->K, Kgp, p.nR, p.nS, st)) return e;
        }
        return 0;
    }
    if (pl.n == 0) return 0;
    size_t max_total = 0;
    PackBwdArgs pk;
    memset(&pk, 0, sizeof(pk));
    pk.w = w; pk.K = d->K; pk.C = d->C; pk.Kgp = Kgp; pk.R = d->R; pk.S = d->S; pk.tstep = d->stride; pk.chunked = chunked; pk.n = pl.n;
    for (int i = 0; i < pl.n; ++i) {
        const BwdPhase& p = pl.ph[i];
        const size_t total = (size_t)d->C * p.nR * p.nS * Kgp;
        max_total = total > max_total ? total : max_total;
        PackBwdArgs::Entry& pe = pk.e[i];
        pe.A = packed + p.a_off; pe.r0 = p.r0; pe.s0 = p.s0; pe.nR = p.nR; pe.nS = p.nS; pe.fold = p.fold;
    }
    hipLaunchKernelGGL(repack_bwd_multi_kernel, dim3(capped_blocks(max_total, 256, 2048), pk.n), dim3(256), 0, st, pk);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

static int conv2d_bwd_data_impl(const pcgan_conv_desc* d, const void* dy, const float* w, const float* packed,
                                const float* bias, void* dx, void* ws, size_t ws_bytes, pcgan_stream_t s, const HsplitOpt* hs = nullptr) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(dy && (w || packed), "conv2d_bwd_data: null pointer");
    PCGAN_CHECK(ws && ws_bytes >= pcgan_conv2d_workspace_bytes(d, PCGAN_PASS_BWD_DATA),
                "conv2d_bwd_data: workspace too small (%zu)", ws_bytes);
    PCGAN_CHECK(d->pad_mode == 0 || d->stride == 1, "conv2d_bwd_data: reflection padding needs stride 1");
    hipStream_t st = (hipStream_t)s;
    const int Kgp = round4(d->K), stv = d->stride;
    BwdPlan pl;
    bwd_plan(d, pl);
    float* Abase = packed ? const_cast<float*>(packed) : (float*)ws;
    if (!packed && pack_bwd(d, pl, w, Abase, st)) return 2;
    const size_t a_bytes = bwd_base_bytes(d);
    const int H = pl.H, W = pl.W;
    void* out = pl.padded ? (void*)((char*)ws + a_bytes) : dx;

    IgemmArgs a;
    memset(&a, 0, sizeof(a));
    a.X = dy; a.Y = out; a.dtype = d->dtype;
    a.bias = pl.padded ? nullptr : bias;   // padded fallback: the fold adds it, once per element
    a.M = d->C; a.N = d->N; a.Cg = d->K; a.Cgp = Kgp; a.Hg = d->P; a.Wg = d->Q;
    a.Yh = H; a.Yw = W;
    a.ostep = stv; a.sl = ilog2_exact(stv); a.pad = pl.pad; a.tstep = stv;
    a.act = PCGAN_ACT_NONE; a.slope = 0.f;
    a.chunked = chunked_k(d->K, d->C, d->R, d->S) ? 1 : (cg4_k(d->K, d->C, d->R, d->S) ? 2 : 0);
    a.rowfold = pl.rowfold;
    apply_hsplit(a, hs);
    a.x_bytes = (unsigned)((size_t)d->N * d->K * d->P * d->Q * esz(d));
    a.nphase = pl.n;
    for (int i = 0; i < pl.n; ++i) {
        const BwdPhase& q = pl.ph[i];
        PhaseArgs& p = a.ph[i];
        p.A = Abase + q.a_off; p.Kp = q.nR * q.nS * Kgp; p.Hs = q.Hs; p.Ws = q.Ws; p.fy = q.fy; p.fx = q.fx;
        if (d->C <= 4) {   // small-M path reads the weights as [k][4] / [c][sj][8][4]
            p.A = Abase + q.at_off;
            p.As = Abase + q.as_off;
        }
        p.r0 = q.r0; p.s0 = q.s0; p.nR = q.nR; p.nS = q.nS; p.Ptot = d->N * q.Hs * q.Ws;
        p.ymap = pl.rowfold && q.fold == 0;
    }
    if (pl.rowfold) return launch_igemm(MODE_BWD_REFLECT, a, st, nullptr, 0);
    if (pl.need_zero) {
        // pixels that no phase writes would also miss the bias; never happens for the nets on the hot path
        PCGAN_CHECK(!bias, "conv2d_bwd_data: bias with uncovered phases is unsupported");
        hipError_t e = hipMemsetAsync(out, 0, (size_t)d->N * d->C * H * W * esz(d), st);
        PCGAN_CHECK(e == hipSuccess, "memset failed: %s", hipGetErrorString(e));
    }
    // split-K partials live behind the A matrices (not with the padded-grid fallback or uncovered phases)
    float* part = (bwd_part_bytes(d) && !pl.padded && !pl.need_zero) ? (float*)((char*)ws + a_bytes) : nullptr;
    if (launch_igemm(pl.fused ? MODE_BWD_REFLECT : MODE_BWD, a, st, part, bwd_part_bytes(d))) return 2;
    if (pl.padded) return pcgan::launch_reflect_fold(out, dx, d->N * d->C, d->H, d->W, d->pad, d->dtype, st, bias, d->C);
    return 0;
}

extern "C" int pcgan_conv2d_bwd_data(const pcgan_conv_desc* d, const void* dy, const float* w,
                                     const float* bias, void* dx, void* ws, size_t ws_bytes,
                                     pcgan_stream_t s) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(w && dx, "conv2d_bwd_data: null pointer");
    return conv2d_bwd_data_impl(d, dy, w, nullptr, bias, dx, ws, ws_bytes, s);
}
extern "C" int pcgan_conv2d_bwd_data_packed(const pcgan_conv_desc* d, const void* dy, const float* packed,
                                            const float* bias, void* dx, void* ws, size_t ws_bytes,
                                            pcgan_stream_t s) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(packed && dx, "conv2d_bwd_data_packed: null pointer");
    pcgan::TimerScope timer(pcgan::timer_kind_res(d, pcgan::TIMER_RES_DGRAD), (hipStream_t)s);
    return conv2d_bwd_data_impl(d, dy, nullptr, packed, bias, dx, ws, ws_bytes, s);
}

// ---- fp16 two-piece form of the packed calls (fp32 tensors, hgemm_kernel): same packed weights, workspace and results layout as
// pcgan_conv2d_fwd_packed / pcgan_conv2d_bwd_data_packed; x_amax[0 .. n_amax) partial maxima of |x| (pcgan_absmax or a producer's
// plane maxima) and w_amax[0 .. 64) partial maxima of |weight| (pcgan_absmax with 64 slots), both on the device
extern "C" int pcgan_conv2d_hgemm_supported(const pcgan_conv_desc* d, int pass) {
    if (!d || d->dtype != PCGAN_F32) return 0;
    if (pass == PCGAN_PASS_FWD) return chunked_k(d->C, d->K, d->R, d->S) && d->K > 32;
    if (pass == PCGAN_PASS_BWD_DATA) return d->pad_mode == 0 && chunked_k(d->K, d->C, d->R, d->S) && d->C > 32;
    return 0;
}
extern "C" int pcgan_conv2d_fwd_packed_hsplit(const pcgan_conv_desc* d, const void* x, const float* x_amax, int n_amax, const float* packed,
                                              const float* w_amax, const float* bias, void* y, int act, float slope, void* ws,
                                              size_t ws_bytes, pcgan_stream_t s) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(pcgan_conv2d_hgemm_supported(d, PCGAN_PASS_FWD), "conv2d_fwd_packed_hsplit: unsupported shape");
    PCGAN_CHECK(packed && x_amax && n_amax > 0 && w_amax, "conv2d_fwd_packed_hsplit: null pointer");
    const HsplitOpt hs = {x_amax, n_amax, w_amax};
    return conv2d_fwd_impl(d, x, nullptr, packed, bias, y, act, slope, ws, ws_bytes, s, &hs);
}
extern "C" int pcgan_conv2d_bwd_data_packed_hsplit(const pcgan_conv_desc* d, const void* dy, const float* dy_amax, int n_amax,
                                                   const float* packed, const float* w_amax, const float* bias, void* dx, void* ws,
                                                   size_t ws_bytes, pcgan_stream_t s) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(pcgan_conv2d_hgemm_supported(d, PCGAN_PASS_BWD_DATA), "conv2d_bwd_data_packed_hsplit: unsupported shape");
    PCGAN_CHECK(packed && dx && dy_amax && n_amax > 0 && w_amax, "conv2d_bwd_data_packed_hsplit: null pointer");
    const HsplitOpt hs = {dy_amax, n_amax, w_amax};
    return conv2d_bwd_data_impl(d, dy, nullptr, packed, bias, dx, ws, ws_bytes, s, &hs);
}

extern "C" int pcgan_conv2d_hgemm_pack(const pcgan_conv_desc* d, int pass, const float* w, float* w_rowmax, float* packed,
                                       pcgan_stream_t s) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(pcgan_conv2d_hgemm_supported(d, pass), "conv2d_hgemm_pack: unsupported shape or pass");
    PCGAN_CHECK(w && w_rowmax && packed, "conv2d_hgemm_pack: null pointer");
    hipStream_t st = (hipStream_t)s;
    const bool fwd = pass == PCGAN_PASS_FWD;
    const int M = fwd ? d->K : d->C, RS = d->R * d->S;
    if (launch_weight_row_absmax(w, d->K, d->C, RS, fwd ? 0 : 1, w_rowmax, st)) return 2;
    if (pcgan_conv2d_pack_weights(d, pass, w, packed, s)) return 1;
    // in-place pre-split of every A matrix of the packed buffer: one for the forward pass, one per phase of the data gradient
    if (fwd) return launch_hgemm_presplit(packed, M, RS * round4(d->C) / 4, w_rowmax, st);
    BwdPlan pl;
    bwd_plan(d, pl);
    for (int i = 0; i < pl.n; ++i)
        if (int e = launch_hgemm_presplit(packed + pl.ph[i].a_off, M, pl.ph[i].nR * pl.ph[i].nS * round4(d->K) / 4, w_rowmax, st)) return e;
    return 0;
}

extern "C" int pcgan_igemm_last_launch(int* info, int n) {
    PCGAN_CHECK(info != nullptr && n > 0, "igemm_last_launch: null output");
    std::lock_guard<std::mutex> lk(g_launch_mu);
    for (int i = 0; i < n; ++i) info[i] = i < PCGAN_IGEMM_LAUNCH_INFO ? g_launch[i] : 0;
    return 0;
}

extern "C" size_t pcgan_conv2d_packed_bytes(const pcgan_conv_desc* d, int pass) {
    if (!d) return 0;
    if (pass == PCGAN_PASS_FWD) return fwd_base_bytes(d);
    if (pass == PCGAN_PASS_BWD_DATA) return bwd_base_bytes(d);
    return 0;
}
extern "C" int pcgan_conv2d_pack_weights(const pcgan_conv_desc* d, int pass, const float* w, float* packed,
                                         pcgan_stream_t s) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(w && packed, "conv2d_pack_weights: null pointer");
    if (pass == PCGAN_PASS_FWD) return pack_fwd(d, w, packed, (hipStream_t)s);
    PCGAN_CHECK(pass == PCGAN_PASS_BWD_DATA, "conv2d_pack_weights: pass %d has no packed weights", pass);
    PCGAN_CHECK(d->pad_mode == 0 || d->stride == 1, "conv2d_bwd_data: reflection padding needs stride 1");
    BwdPlan pl;
    bwd_plan(d, pl);
    return pack_bwd(d, pl, w, packed, (hipStream_t)s);
}

extern "C" int pcgan_conv2d_bwd_weight(const pcgan_conv_desc* d, const void* x, const void* dy, float* dw,
                                       int accumulate, void* ws, size_t ws_bytes, pcgan_stream_t s) {
    if (check_desc(d)) return 1;
    PCGAN_CHECK(x && dy && dw, "conv2d_bwd_weight: null pointer");
    PCGAN_CHECK(ws && ws_bytes >= pcgan_conv2d_workspace_bytes(d, PCGAN_PASS_BWD_WEIGHT),
                "conv2d_bwd_weight: workspace too small (%zu)", ws_bytes);
    hipStream_t st = (hipStream_t)s;
    pcgan::TimerScope timer(pcgan::timer_kind_res(d, pcgan::TIMER_RES_WGRAD), st);
    const int Cgp = round4(d->C), RS = d->R * d->S;
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.dY = dy; a.X = x; a.Wp = (float*)ws; a.dtype = d->dtype;
    a.M = d->K; a.Kp = RS * Cgp; a.N = d->N; a.Cg = d->C; a.Cgp = Cgp;
    a.Hg = d->H; a.Wg = d->W; a.Ho = d->P; a.Wo = d->Q;
    a.sl = ilog2_exact(d->stride); a.pad = d->pad; a.S = d->S;
    a.magicS = (65536 + d->S - 1) / d->S;
    a.Ptot = d->N * d->P * d->Q;
    a.x_bytes = (unsigned)((size_t)d->N * d->C * d->H * d->W * esz(d));
    a.dy_bytes = (unsigned)((size_t)d->N * d->K * d->P * d->Q * esz(d));
    const int splits = wgrad_splits(d, &a.chunks_per_split);
    return launch_wgrad(d, a, splits, dw, accumulate, st);
}
