// The window ("halo") kernel: forward and data gradient of the reflection-padded 3x3 stride-1 convolution of the residual blocks
// (nn.ReflectionPad2d + nn.Conv2d of the ResnetBlocks, models/networks.py:621-648, and autograd's data gradient of them) -- the
// default route of both, on two scaled fp16 pieces (PK_F16X2), and the PCGAN_SPLIT=bf16 / bf16-tensor forms of the same shapes.
// "The kernel above" in the text below is bsplit_conv_fwd_kernel (bsplit_conv.hip), whose packed weights (bsplit_pack.hip) and MFMA
// order this kernel shares.  Called from the host unit, bf16x6_conv.hip, through launch_halo (bsplit.h).
//
// ---- "halo" form of the reflection-padded 3x3 stride-1 convolution (forward and data gradient), image width 32 or 64 -----------
// The kernel above gathers every input element once per tap (9 loads, 9 splits, 9 LDS writes per element and workgroup).  Here a
// pixel tile is RT = 128 / W full image rows, and per 16-channel chunk its (RT + 2) x (W + 2) window is loaded, split and written
// to LDS ONCE; the nine taps read it at shifted addresses ([piece][k half][window pixel][8 bf16]: a tap is a constant added to the
// lane's LDS address, 32 consecutive lanes still read 512 contiguous bytes).  The packed weights and the MFMA order are those of the
// kernel above; a wave owns 32 output channels x all 128 pixels and loads its weight fragments from memory into registers (no
// weight stage in LDS, one barrier per 16-channel chunk: see the A operand below).
//   forward        the window holds the reflection-padded input (the mirror is applied when the window is built);
//   data gradient  the window holds dy with a ring of zeros; the contributions of the padded rows / columns -1 and H / W, which
//                  fold onto rows / columns 1 and H-2 / W-2, become two extra window rows and columns of SUMS
//                  (dy[2] + dy[0] for output row 1 through tap r' = 2, dy[H-3] + dy[H-1] for row H-2 through r' = 0; columns
//                  alike; the corners sum four sources): a lane on row 1 / column 1 / ... reads the sum entry instead of the shifted
//                  one.  One set of plain flipped weights serves every row (the kernel above needs three row classes).
#include "bsplit.h"

namespace pcgan {

template <int MODE, int PK, typename TA, int QW>
__global__ void __launch_bounds__(512) bsplit_halo_kernel(HaloArgs a) {
    constexpr int NP = PK == PK_BF16X3 ? 3 : (PK == PK_F16X2 ? 2 : 1);
    static_assert((PK != PK_BF16 && sizeof(TA) == 4) || (PK == PK_BF16 && sizeof(TA) == 2), "pieces of fp32 tensors, or bf16 tensors as they are");
    static_assert(QW == 32 || QW == 64, "image width");
    constexpr unsigned ES = sizeof(TA);
    constexpr bool DG = MODE == BH_DGRAD;
    constexpr int BM = 256, NT = 512;
    constexpr int RT = 128 / QW;                    // image rows of a pixel tile
    constexpr int WR = RT + 2, WC = QW + 2;         // window = tile + a ring of one pixel
    constexpr int HR = WR + (DG ? 2 : 0), QH = WC + (DG ? 2 : 0);     // + the two sum rows / columns of the data gradient
    constexpr int NPX = HR * QH;
    constexpr int NBASE = WR * WC, NRB = (NBASE * 4 + NT - 1) / NT;   // window entries x 4 channel quads, rounds over the threads
    constexpr int NPATCH = DG ? 2 * WR + 2 * QH : 0, NRP = DG ? (NPATCH * 4 + NT - 1) / NT : 0;
    constexpr unsigned ASTAGE = BM * 32;            // bytes of one stage of one piece of the weights
    constexpr unsigned XPIECE = 2 * NPX * 16, XBUF = NP * XPIECE;
    __shared__ __attribute__((aligned(16))) bf16x8 Xs[2 * NP * 2 * NPX];  // [buffer][piece][half][window entry]
    __shared__ float red_scratch[16];

    const int tid = threadIdx.x;
    const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NI = 1, NJ = 4;                   // a wave's tile: 32 output channels x all 128 pixels (its weight fragments are its own: no wave loads another's)
    const int mt = blockIdx.x % a.nMt, pt = blockIdx.x / a.nMt;
    const int TPI = a.H / RT;
    const int n = pt / TPI, y0 = (pt - n * TPI) * RT;
    const int HW = a.H * QW;
    char* const xs_bytes = reinterpret_cast<char*>(&Xs[0]);

    // ---- window builder tables: which source element(s) a thread loads per chunk and where their pieces go
    unsigned bvo[NRB], blds[NRB];
#pragma unroll
    for (int i = 0; i < NRB; ++i) {
        const int u = tid + i * NT;
        const bool valid = u < NBASE * 4;
        const int q = u / NBASE, e = u - q * NBASE, hb = e / WC, wb = e - hb * WC;
        int iy = y0 - 1 + hb, ix = wb - 1;
        bool ok = valid;
        if (DG) {
            ok = ok & ((unsigned)iy < (unsigned)a.H) & ((unsigned)ix < (unsigned)QW);
        } else {
            iy = iy < 0 ? -iy : iy;
            iy = iy >= a.H ? 2 * (a.H - 1) - iy : iy;
            ix = ix < 0 ? -ix : ix;
            ix = ix >= QW ? 2 * (QW - 1) - ix : ix;
        }
        bvo[i] = ok ? (unsigned)(q * 4 * HW + iy * QW + ix) * ES : BS_OOB;
        blds[i] = valid ? (unsigned)(((q >> 1) * NPX + hb * QH + wb) * 16 + (q & 1) * 8) : 0xffffffffu;
    }
    unsigned pvo[DG ? NRP : 1][4], plds[DG ? NRP : 1];
    if constexpr (DG) {
        const bool use_lo = y0 <= 1 && 1 < y0 + RT;               // the tile holds row 1: sum row {2, 0}
        const bool use_hi = y0 <= a.H - 2 && a.H - 2 < y0 + RT;   // the tile holds row H-2: sum row {H-3, H-1}
#pragma unroll
        for (int i = 0; i < NRP; ++i) {
            const int u = tid + i * NT;
            const bool valid = u < NPATCH * 4;
            const int q = u / NPATCH, pe = u - q * NPATCH;
            int h, w;
            if (pe < 2 * WR) {
                h = pe >> 1;
                w = WC + (pe & 1);
            } else {
                const int p2 = pe - 2 * WR;
                h = WR + p2 / QH;
                w = p2 - (p2 / QH) * QH;
            }
            int r0, r1, c0, c1;
            if (h < WR) {
                r0 = y0 - 1 + h;
                r0 = (unsigned)r0 < (unsigned)a.H ? r0 : -1;
                r1 = -1;
            } else if (h == WR) {
                r0 = use_hi ? a.H - 3 : -1;
                r1 = use_hi ? a.H - 1 : -1;
            } else {
                r0 = use_lo ? 2 : -1;
                r1 = use_lo ? 0 : -1;
            }
            if (w < WC) {
                c0 = w - 1;
                c0 = (unsigned)c0 < (unsigned)QW ? c0 : -1;
                c1 = -1;
            } else if (w == WC) {
                c0 = QW - 3;
                c1 = QW - 1;
            } else {
                c0 = 2;
                c1 = 0;
            }
            const int rr[4] = {r0, r0, r1, r1}, cc[4] = {c0, c1, c0, c1};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                pvo[i][k] = (valid && rr[k] >= 0 && cc[k] >= 0) ? (unsigned)(q * 4 * HW + rr[k] * QW + cc[k]) * ES : BS_OOB;
            plds[i] = valid ? (unsigned)(((q >> 1) * NPX + h * QH + w) * 16 + (q & 1) * 8) : 0xffffffffu;
        }
    }

    // ---- LDS addresses of this lane's two pixel columns (j = 0, 1) of the B operand, per tap
    unsigned boff[NJ], rowb[DG ? NJ : 1][3], colb[DG ? NJ : 1][3];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int p = j * 32 + lo, ty = p / QW, tx = p - ty * QW;
        boff[j] = (unsigned)((hi * NPX + ty * QH + tx) * 16);
        if constexpr (DG) {
            const int y = y0 + ty;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int rs = (y == 1 && t == 2) ? WR + 1 : ((y == a.H - 2 && t == 0) ? WR : ty + t);
                const int cs = (tx == 1 && t == 2) ? WC + 1 : ((tx == QW - 2 && t == 0) ? WC : tx + t);
                rowb[j][t] = (unsigned)(rs * QH * 16);
                colb[j][t] = (unsigned)((hi * NPX + cs) * 16);
            }
        }
    }

    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.X), 0, (int)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.A), 0, (int)a.a_bytes, 0x00020000);
    // an activation element as loaded: fp32 value; bf16 storage: the stored pattern, zero-extended (RAW: it goes to LDS unchanged)
    auto ldraw = [&](unsigned voff, unsigned soff) -> unsigned {
        if constexpr (ES == 4) return __builtin_amdgcn_raw_buffer_load_b32(rX, voff, soff, 0);
        else return (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rX, voff, soff, 0);
    };
    auto tofloat = [&](unsigned raw) -> float { return __uint_as_float(ES == 4 ? raw : raw << 16); };
    const unsigned piece_bytes = (unsigned)a.nMt * (unsigned)(a.nch * 9) * ASTAGE;
    const unsigned a_tile = (unsigned)mt * (unsigned)(a.nch * 9) * ASTAGE;
    const int nst = a.nch * 9;

    // write 4 consecutive channels of one window entry (8 bytes per piece)
    typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
    typedef _Float16 hf4 __attribute__((ext_vector_type(4)));
    float sx = 1.f;
    if constexpr (PK == PK_F16X2) {      // largest of the partial maxima the producer left (one per plane, or a single value)
        const float m = thread_max_of_partials(a.x_amax, a.x_namax, tid, NT);
        sx = pow2_scale(block_max(m, red_scratch));
        __syncthreads();
    }
    // sum = a sum entry of the data gradient: up to FOUR dy elements added before the split.  Four sources at the top of [2^13, 2^14)
    // scale to as much as 4 (2^14 - 1) < 2^16, past fp16's 65504 (dy = 1 - 2^-13 everywhere: 65528, the cast gave inf and the four
    // corner pixels of every plane NaN).  Below 2^16 the high piece saturates at 65504 and the low piece takes the rest (< 32, to
    // 2^-7: the split keeps its 2^-22); every value the cast already kept finite splits as before, bit for bit.  From 2^16 on the
    // maximum the scale came from was not one: that still overflows and the sentinel counts it
    auto put_split = [&](unsigned lds, int buf, const float (&v)[4], const bool sum = false) {
        char* dst = xs_bytes + (unsigned)buf * XBUF + lds;
        if constexpr (PK == PK_F16X2) {
            hf4 h, l;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float s = v[j] * sx;
                _Float16 x = (_Float16)((sum && fabsf(s) < 65536.f) ? __builtin_amdgcn_fmed3f(s, -65504.f, 65504.f) : s);
                h[j] = x;
                l[j] = (_Float16)(s - (float)x);
            }
            *reinterpret_cast<hf4*>(dst) = h;
            *reinterpret_cast<hf4*>(dst + XPIECE) = l;
        } else {
            bf4 h, m, l;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (NP == 3) {
                    __bf16 x, y, z;
                    split3(v[j], x, y, z);
                    h[j] = x;
                    m[j] = y;
                    l[j] = z;
                } else {
                    h[j] = (__bf16)v[j];
                }
            }
            *reinterpret_cast<bf4*>(dst) = h;
            if constexpr (NP == 3) {
                *reinterpret_cast<bf4*>(dst + XPIECE) = m;
                *reinterpret_cast<bf4*>(dst + 2 * XPIECE) = l;
            }
        }
    };
    unsigned tb[NRB][4];
    auto base_load = [&](int ch) {       // (a chunk past the end: out-of-range offsets, zeros come back)
        const bool live = ch < a.nch;
        const unsigned so = live ? (unsigned)((n * a.C + ch * 16) * HW) * ES : 0u;
#pragma unroll
        for (int i = 0; i < NRB; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) tb[i][j] = ldraw(live ? bvo[i] : BS_OOB, so + (unsigned)(j * HW) * ES);
    };
    auto base_write = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NRB; ++i) {
            if (blds[i] == 0xffffffffu) continue;
            if constexpr (PK == PK_BF16) {     // stored bf16 patterns as they are
                typedef unsigned short us4 __attribute__((ext_vector_type(4)));
                us4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (unsigned short)tb[i][j];
                *reinterpret_cast<us4*>(xs_bytes + (unsigned)buf * XBUF + blds[i]) = v;
            } else {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = tofloat(tb[i][j]);
                put_split(blds[i], buf, v);
            }
        }
    };
    unsigned tp[DG ? NRP : 1][4][4];
    auto patch_load = [&](int ch) {
        if constexpr (DG) {
            const bool live = ch < a.nch;
            const unsigned so = live ? (unsigned)((n * a.C + ch * 16) * HW) * ES : 0u;
#pragma unroll
            for (int i = 0; i < NRP; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j) tp[i][k][j] = ldraw(live ? pvo[i][k] : BS_OOB, so + (unsigned)(j * HW) * ES);
        }
    };
    auto patch_write = [&](int buf) {
        if constexpr (DG) {
#pragma unroll
            for (int i = 0; i < NRP; ++i) {
                if (plds[i] == 0xffffffffu) continue;
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[j] = (tofloat(tp[i][0][j]) + tofloat(tp[i][1][j])) + (tofloat(tp[i][2][j]) + tofloat(tp[i][3][j]));
                put_split(plds[i], buf, v, true);
            }
        }
    };

    // the A operand (weights) never touches LDS: the packed image holds, per stage and piece, [k half][256 rows][8 values] -- exactly
    // the 16 bytes a lane feeds to the MFMA (row wave * 32 + lo, k half hi) -- so every wave loads ITS fragments from memory
    // (32 rows x 16 bytes contiguous per half-wave; every byte of the image is loaded by exactly one wave of the workgroup) two or three stages ahead.
    // No weight stage in LDS means no barrier per stage (one per 16-channel chunk, for the window), none of this chip's slow LDS stores
    // (~80 B/clk), half the LDS reads, and waves that drift apart so that one wave's window work sits under another's MFMAs.
    struct OpA {
        bf16x8 A[NP][NI];
    };
    const unsigned a_lane = (unsigned)((hi * BM + wave * 32 + lo) * 16);
    auto aload = [&](OpA& o, int s) {
        const bool live = s < nst;
        const unsigned avo = live ? a_lane : BS_OOB;
        const unsigned aso = a_tile + (unsigned)(live ? s : 0) * ASTAGE;
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int i = 0; i < NI; ++i)
                o.A[p][i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rA, avo, aso + p * piece_bytes + i * 512, 0));
    };

    f32x16 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    struct OpB {
        bf16x8 B[NP][NJ];
    };
    // B operand of one stage: pixels of tap (tr, ts) from window buffer xbuf
    auto fetch = [&](OpB& o, int xbuf, int tr, int ts) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            unsigned ad;
            if constexpr (DG) ad = rowb[j][tr] + colb[j][ts];
            else ad = boff[j] + (unsigned)((tr * QH + ts) * 16);
#pragma unroll
            for (int p = 0; p < NP; ++p)
                o.B[p][j] = *reinterpret_cast<const bf16x8*>(xs_bytes + ad + (unsigned)xbuf * XBUF + p * XPIECE);
        }
    };
    auto mma = [&](const OpA& oa, const OpB& ob) {
        if constexpr (PK == PK_F16X2) {       // (l,h) (h,l) (h,h)
            constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, oa.A[PA[q]][i]),
                                                                            __builtin_bit_cast(f16x8, ob.B[PB[q]][j]), acc[i][j], 0, 0, 0);
        } else {
            constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
            for (int q = (NP == 3 ? 0 : 5); q < 6; ++q)
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(oa.A[PA[q]][i], ob.B[PB[q]][j], acc[i][j], 0, 0, 0);
        }
    };
    // issue order inside a stage (a hint): every MFMA is followed by its share of the other work
    auto interleave = [&]() {
        if constexpr (NP == 2) {
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                   // one MFMA
                if (q < 8) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);        // LDS reads of the next stage first
                if (q < 2) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);        // weight fragments two stages ahead
                __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);                   // VALU (split arithmetic of a window)
                if (q >= 4) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);       // LDS writes
                if (q >= 4) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);       // window loads
            }
        } else if constexpr (NP == 3) {
#pragma unroll
            for (int q = 0; q < 24; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                   // one MFMA
                if (q < 12) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);       // LDS reads of the next stage first
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                   // VALU (split arithmetic of a window)
                if (q >= 8) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);       // LDS writes
                if (q >= 2) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);       // global loads
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 12, 0);
                __builtin_amdgcn_sched_group_barrier(0x200, 3, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 6, 0);
            }
        }
    };

    // window of chunk 0, then the stage loop unrolled over a PAIR of chunks (18 stages) so that window buffer, tap and register sets
    // are all static.  Stage t of the pair: MFMAs of stage t out of registers | B fetch (LDS) of stage t+1 | weight fragments of
    // stage t+NA-1 from memory | window of the next chunk:
    //   t = 0 / 9    loads of the window proper                       (registers only)
    //   t = 3 / 12   its split + LDS writes; loads of the sum rows / columns (data gradient)
    //   t = 6 / 15   their split + LDS writes
    // ONE barrier per chunk, at the end of t = 7 / 16: behind every wave's window writes and its last fetch from the window before
    // (during t = 7 / 16), in front of the first fetch from the new window (during t = 8 / 17) and of the next writes (t = 3 / 12).
    constexpr int NA = NP == 3 ? 2 : 3;       // register sets of weight fragments (18 = 0 mod NA)
    base_load(0);
    patch_load(0);
    OpA oa[NA];
    OpB ob[2];
#pragma unroll
    for (int i = 0; i < NA - 1; ++i) aload(oa[i], i);
    base_write(0);
    patch_write(0);
    __syncthreads();
    fetch(ob[0], 0, 0, 0);
    for (int c = 0; c < a.nch; c += 2) {
        const int s0 = c * 9;
#pragma unroll
        for (int t = 0; t < 18; ++t) {
            const int tn = (t + 1) % 18, tapn = tn % 9;
            aload(oa[(t + NA - 1) % NA], s0 + t + NA - 1);                   // weight fragments of stage t+NA-1
            fetch(ob[(t + 1) & 1], tn / 9, tapn / 3, tapn % 3);              // pixels of stage t+1
            mma(oa[t % NA], ob[t & 1]);                                      // stage t
            if (t == 0) base_load(c + 1);
            if (t == 9) base_load(c + 2);
            if (t == 3 || t == 12) {
                base_write(t == 3 ? 1 : 0);
                patch_load(t == 3 ? c + 1 : c + 2);
            }
            if (t == 6 || t == 15) patch_write(t == 6 ? 1 : 0);
            interleave();
            __builtin_amdgcn_sched_barrier(0);      // nothing moves across a stage boundary (MFMAs of the next stage would wait on its own LDS reads)
            if (t == 7 || t == 16) {
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    // epilogue: acc[i][j][r] = Y[m0 + wave*32 + (r/4)*8 + hi*4 + r%4][pixel j*32 + lo]; a tile is RT full rows of image n
    const float isx = 1.f / sx;    // powers of two: exact
    float iswr[NI][16];            // ... and one per weight ROW (the pack call scaled row m by pow2_scale(w_amax[m]))
    if constexpr (PK == PK_F16X2) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * BM + wave * 32 + i * 32 + (r >> 2) * 8 + hi * 4 + (r & 3);
                iswr[i][r] = m < a.M ? 1.f / pow2_scale(a.w_amax[m]) : 1.f;
            }
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const size_t yo = (size_t)n * a.M * HW + (size_t)y0 * QW + j * 32 + lo;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * BM + wave * 32 + i * 32 + (r >> 2) * 8 + hi * 4 + (r & 3);
                if (m < a.M) {
                    const float av = PK == PK_F16X2 ? (acc[i][j][r] * isx) * iswr[i][r] : acc[i][j][r];
                    if constexpr (PK == PK_F16X2) bad |= is_nonfinite(av);
                    float v = act_apply(av + (a.bias ? a.bias[m] : 0.f), a.act, a.slope);
                    if (a.R) v += ld1((const TA*)a.R + yo + (size_t)m * HW);
                    st1((TA*)a.Y + yo + (size_t)m * HW, v);
                }
            }
    }
    if constexpr (PK == PK_F16X2) report_nonfinite(a.ovf, bad);
}

template <int MODE>
static void launch_mode(int pk, int W, dim3 grid, hipStream_t st, const HaloArgs& a) {
    if (pk == PK_BF16) {
        if (W == 32) hipLaunchKernelGGL((bsplit_halo_kernel<MODE, PK_BF16, bf16, 32>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((bsplit_halo_kernel<MODE, PK_BF16, bf16, 64>), grid, dim3(512), 0, st, a);
    } else if (pk == PK_F16X2) {
        if (W == 32) hipLaunchKernelGGL((bsplit_halo_kernel<MODE, PK_F16X2, float, 32>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((bsplit_halo_kernel<MODE, PK_F16X2, float, 64>), grid, dim3(512), 0, st, a);
    } else {
        if (W == 32) hipLaunchKernelGGL((bsplit_halo_kernel<MODE, PK_BF16X3, float, 32>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((bsplit_halo_kernel<MODE, PK_BF16X3, float, 64>), grid, dim3(512), 0, st, a);
    }
}

int launch_halo(int mode, int pk, int W, const HaloArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((long)a.N * a.H * W / 128 * a.nMt));      // a pixel tile = 128 / W full image rows
    if (mode == BH_FWD) launch_mode<BH_FWD>(pk, W, grid, st, a);
    else launch_mode<BH_DGRAD>(pk, W, grid, st, a);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace pcgan
