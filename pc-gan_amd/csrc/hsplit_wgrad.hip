// The per-tap weight gradient: every convolution with >= 32 output channels that the row-ring and direct forms (wgrad_rowring.hip,
// wgrad_direct.hip) do not take -- the generator's down / up-sampling layers, the PatchGAN and, with those two switched off, the
// residual blocks.  Called from the host unit, bf16x6_conv.hip (pcgan_conv2d_bwd_weight_hsplit), through launch_hsplit_wgrad
// (bsplit.h); the padded copy it may read and the sum of its split partials are in bsplit_pack.hip.
//
// ---- fp16 two-piece route (fp32 tensors) / bf16 one-product route (bf16 tensors): weight gradient of a padded convolution -----------
// dW[k][(c, r, s)] = sum over (n, y, x) of dy[n][k][y][x] * xpad[n][c][y * STRIDE + r][x * STRIDE + s]: rows = output channels (one tile of
// BM = 128 or 256), columns = (c, tap) in tiles of 128, reduction over output pixels in stages of 16 consecutive x (output width a
// multiple of 16).  xpad = the input with its padding materialised once (reflection or zeros), so that the gather address separates into
// a column part (lane offset) and a pixel part (scalar offset).  Both operands are split on their way to LDS (no packed copy of dy):
//   A  dy[n][row][y][x0 + 8 half .. + 8): two 16-byte loads per thread, one 16-byte LDS write per piece;
//   B  xpad[n][c][y STRIDE + r][(x0 + KB q + j) STRIDE + s], j < KB = 2048 / threads: KB element loads (the tap shifts the alignment), one
//      8- or 16-byte LDS write per piece;
// 12 MFMAs (fp16 route; bf16: 4) and 8 (4) ds_read_b128 per wave and stage; blockIdx.y takes a range of stages and writes a raw partial
// sum, combined in a fixed order by bsplit_wgrad_reduce_kernel.  Replaces autograd's weight gradient of nn.Conv2d /
// nn.ConvTranspose2d of the generator's down / up-sampling layers, the residual blocks and the PatchGAN (models/networks.py:584-648, 734-763).
#include "bsplit.h"

namespace pcgan {

// NC = column tiles of 128 per workgroup (2 with the 256-row tile: the dy tile is loaded and split once for 256 columns)
// GEN (zero padding <= 1, fp32 or bf16 tensors): the padding is applied inside the gather (rows outside the image select an
// out-of-range offset, the at most one column per side is zeroed in registers when the run is split / stored) and the output width
// may be ragged (stages of 16 columns per output row, the dy values beyond column Q masked to zero: the PatchGAN's 15 x 15 layer;
// bf16 tensors then load dy by 2-byte elements, a ragged row starts on a 2-byte boundary)
template <int BM, int STRIDE, typename TA, int NC, int GEN = 0>
__global__ void __launch_bounds__(BM * 2) hsplit_wgrad_kernel(HWgradArgs a) {
    constexpr int NT = BM * 2;
    constexpr int CW = 128 * NC;                // columns per workgroup
    constexpr bool HALF = sizeof(TA) == 2;      // bf16 tensors: one piece, one product, no scaling
    constexpr int NP = HALF ? 1 : 2;
    constexpr unsigned ES = sizeof(TA);
    constexpr int KB = 16 * CW / NT;            // consecutive output pixels of its column a thread gathers per stage (4 or 8)
    // the two k halves of a row are written by neighbouring lanes: 128 bytes of padding between the halves put them on disjoint banks
    constexpr int AH = BM + 8;
    __shared__ __attribute__((aligned(16))) bf16x8 As[2][NP][2 * AH];     // [buffer][piece][half * AH + row]
    constexpr int BH = CW + 8;
    __shared__ __attribute__((aligned(16))) bf16x8 Bs[2][NP][2 * BH];     // [buffer][piece][half * BH + column]
    const int tid = threadIdx.x;
    const int lane = tid & 63, lo = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wp = wave & 1;
    const int T = a.R * a.S, CT = a.C * T, PQ = a.P * a.Q;
    // workgroups go to the 8 XCDs round-robin: give each XCD a CONTIGUOUS run of (split, column tile) pairs, so that the column tiles
    // of one split -- which all read the same dy rows -- share one L2 (dispatch order put them on all eight: dy crossed the fabric 8x)
    const int wg = ((int)blockIdx.x & 7) * ((int)gridDim.x >> 3) + ((int)blockIdx.x >> 3);
    if (wg >= a.nwg) return;
    const int bx = wg % a.ntile, byz = wg / a.ntile;
    const int by = byz % a.splits, m0 = (byz / a.splits) * BM;      // (the column tiles of one (row tile, split) pair are neighbours: same dy rows)

    float sx = 1.f, sdy = 1.f;
    if constexpr (!HALF) {
        const float m = thread_max_of_partials(a.x_amax, a.x_namax, tid, NT), g = thread_max_of_partials(a.dy_amax, a.dy_namax, tid, NT);
        float* scratch = reinterpret_cast<float*>(&As[0][0][0]);
        sx = pow2_scale(block_max(m, scratch));
        sdy = pow2_scale(block_max(g, scratch));
        __syncthreads();
    }

    // loaders: neighbouring lanes read neighbouring bytes of one row / one column's pixel run (64 contiguous bytes per 4 lanes of fp32
    // data: a wave's load touches 16 lines, not 32-64 -- the vector memory path, not the matrix pipe, was the limit of this kernel).
    // fp32 A: rows tid / 4 and NT / 4 + tid / 4, floats 4 * (tid % 4) ..+3 of the stage's 16;  bf16 A: row tid / 2, 8 values
    // B: column tid / BT, pixels KB * (tid % BT) ..+KB-1
    constexpr int AR = NT / 4;
    constexpr int BT = 16 / KB;
    const int arow = HALF ? tid >> 1 : tid >> 2, aq = HALF ? (tid & 1) * 2 : tid & 3;
    const int ahalf = aq >> 1, asub = (aq & 1) * 4;
    const unsigned avo = m0 + arow < a.K ? (unsigned)((m0 + arow) * PQ + aq * 4) * ES : BS_OOB;
    const unsigned avo1 = (!HALF && m0 + arow + AR < a.K) ? (unsigned)((m0 + arow + AR) * PQ + aq * 4) * ES : BS_OOB;
    const int bcol = tid / BT, bq = tid % BT;
    const int col = bx * CW + bcol;
    unsigned bvo = BS_OOB;
    int tr = 1, fixl = 0, fixr = 0;      // inline reflection: this thread's tap row; whether its first / last element can fall on column -1 / W
    int lm = 0, rmk = 0;                 // GEN: elements of the run that lie in the zero padding in the first / last stage of a row (bit j), bit 8 = rotate
    if (col < CT) {
        const int c = col / T, tap = col - c * T, r = tap / a.S, s = tap - r * a.S;
        if constexpr (GEN) {
            const int cs = bq * KB * STRIDE + s - a.pad;      // column of the run's first element in the row's first stage (-1 at most)
            bvo = (unsigned)(((c * a.Hp + r) * a.Wp + cs) * (int)ES);      // (may wrap: its sum with the stage's part below does not)
            tr = r;
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                lm |= (cs + j * STRIDE < 0) ? 1 << j : 0;
                rmk |= ((a.Qs - 16) * STRIDE + cs + j * STRIDE >= a.Wp) ? 1 << j : 0;
            }
            // a run whose first element is column -1 is loaded one element late and rotated when it is split: in the first row of the
            // tensor its offset would be "-4", which does not wrap in the hardware's range check (every later element of the run,
            // reached through the instruction's immediate offset, would read as 0 too)
            if (cs < 0) lm |= 256;
        } else
        if (a.reflect_inline) {      // row term chosen per stage (ro0 / ro1 / ro2 below); a left-edge lane's run starts at column -1
            bvo = (unsigned)((c * a.Hp) * a.Wp + s - 1 + bq * KB) * ES;      // (may be "-4": the per-stage sum below is not)
            tr = r;
            fixl = (s == 0 && bq == 0);
            fixr = (s == 2 && bq == BT - 1);
        } else {
            bvo = (unsigned)((c * a.Hp + r) * a.Wp + s + bq * KB * STRIDE) * ES;
        }
    }
    const __amdgpu_buffer_rsrc_t rD = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.DY), 0, (int)a.dy_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.XP), 0, (int)a.xp_bytes, 0x00020000);

    const int st0 = by * a.nst_split;
    const int nst_here = min(a.nst_split, a.nst - st0);
    // position of the next stage to LOAD (scalar): image, output row, first output column
    int ln, ly, lx;
    {
        const int Qrow = GEN ? a.Qs : a.Q;      // stage positions count the (padded) row width
        const int e0 = st0 * 16;
        ln = e0 / (a.P * Qrow);
        const int rem = e0 - ln * (a.P * Qrow);
        ly = rem / Qrow;
        lx = rem - ly * Qrow;
    }
    struct Stage {
        unsigned a[HALF ? 4 : 8];     // 8 consecutive dy values of this thread's row (bf16: packed pairs)
        unsigned b[KB];               // KB consecutive output pixels of this thread's column
        int fix;                      // inline reflection: 1 = the run starts at column -1, loaded from column 0 instead (rotate), 2 = the last is column W
                                      // GEN: bit j = element j of the run lies in the zero padding, bit 8 = the run was loaded from column 0 (rotate)
        int am;                       // GEN: how many of this thread's 4 consecutive dy values lie inside the row (>= 4: all)
    };
    int lcount = 0;
    auto load = [&](Stage& r) {
        const bool live = lcount < nst_here;
        const unsigned aso = (unsigned)(ln * a.K * PQ + ly * a.Q + lx) * ES;
        unsigned bso = (unsigned)(((ln * a.C) * a.Hp + ly * STRIDE) * a.Wp + lx * STRIDE) * ES;
        unsigned bvt = bvo;
        r.fix = 0;
        r.am = 4;
        if constexpr (GEN) {
            const int yy = ly * STRIDE - a.pad;      // source row of tap row 0 (scalar)
            const bool rowok = (unsigned)(yy + tr) < (unsigned)a.Hp;
            r.fix = (lx == 0 ? lm : 0) | (lx == a.Qs - 16 ? rmk : 0);
            bvt = rowok ? bvo + (unsigned)((((ln * a.C) * a.Hp + yy) * a.Wp + lx * STRIDE) * (int)ES) + ((r.fix & 256) ? STRIDE * ES : 0u) : BS_OOB;
            bso = 0;
            r.am = a.Q - lx - aq * 4;
        } else
        if constexpr (STRIDE == 1) {
            if (a.reflect_inline) {      // source row of tap row tr under reflection padding 1 (scalars per stage), selected by the lane's tap row
                const int y0 = ly == 0 ? 1 : ly - 1, y2 = ly == a.Hp - 1 ? a.Hp - 2 : ly + 1;
                const unsigned base = (unsigned)((ln * a.C) * a.Hp * a.Wp + lx) * ES;
                const unsigned ro0 = base + (unsigned)(y0 * a.Wp) * ES, ro1 = base + (unsigned)(ly * a.Wp) * ES, ro2 = base + (unsigned)(y2 * a.Wp) * ES;
                r.fix = (lx == 0 && fixl) ? 1 : ((lx + 16 == a.Q && fixr) ? 2 : 0);
                // a run that would start at column -1 is loaded from column 0 and rotated when it is split (the first row of the tensor
                // has nothing in front of it, and an offset of "-4" does not wrap in the hardware's range check: the whole load would
                // return 0); a run that ends at column W reads one element of the next row -- in range, or zero at the very end
                bvt = bvo + (tr == 0 ? ro0 : (tr == 1 ? ro1 : ro2)) + (r.fix == 1 ? ES : 0u);
                bso = 0;
            }
        }
        const unsigned av = live ? avo : BS_OOB, bv = live ? bvt : BS_OOB;
        if constexpr (HALF) {
            if (GEN && a.Qs != a.Q) {      // ragged rows start on 2-byte boundaries: element loads, the values beyond column Q enter as zero
                const int am = a.Q - lx - aq * 4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned e0 = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rD, av, aso + (unsigned)(2 * i) * ES, 0);
                    const unsigned e1 = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rD, av, aso + (unsigned)(2 * i + 1) * ES, 0);
                    r.a[i] = (2 * i < am ? (e0 & 0xffffu) : 0u) | (2 * i + 1 < am ? e1 << 16 : 0u);
                }
            } else {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rD, av, aso, 0);
                r.a[0] = v.x; r.a[1] = v.y; r.a[2] = v.z; r.a[3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < KB; ++j) r.b[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rX, bv, bso + (unsigned)(j * STRIDE) * ES, 0);
        } else {
            const u32x4 v0 = __builtin_amdgcn_raw_buffer_load_b128(rD, av, aso, 0), v1 = __builtin_amdgcn_raw_buffer_load_b128(rD, live ? avo1 : BS_OOB, aso, 0);
            r.a[0] = v0.x; r.a[1] = v0.y; r.a[2] = v0.z; r.a[3] = v0.w;
            r.a[4 % (HALF ? 4 : 8)] = v1.x; r.a[5 % (HALF ? 4 : 8)] = v1.y; r.a[6 % (HALF ? 4 : 8)] = v1.z; r.a[7 % (HALF ? 4 : 8)] = v1.w;
            if constexpr (STRIDE == 1) {      // KB consecutive floats (any 4-byte alignment): 16 bytes per load
#pragma unroll
                for (int j = 0; j < KB; j += 4) {
                    const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rX, bv, bso + (unsigned)j * ES, 0);
                    r.b[j] = w.x; r.b[j + 1] = w.y; r.b[j + 2] = w.z; r.b[j + 3] = w.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < KB; ++j) r.b[j] = __builtin_amdgcn_raw_buffer_load_b32(rX, bv, bso + (unsigned)(j * STRIDE) * ES, 0);
            }
        }
        ++lcount;
        lx += 16;
        if (lx == (GEN ? a.Qs : a.Q)) {
            lx = 0;
            if (++ly == a.P) {
                ly = 0;
                ++ln;
            }
        }
    };
    // the thread's KB consecutive k (pixels) of column bcol: k half (bq * KB) / 8, offset (bq * KB) % 8 inside it
    const int bhalf = (bq * KB) >> 3, bsub = (bq * KB) & 7;
    // fp16 route: the pieces of a stage in registers (split), then to LDS (write) -- two steps, a barrier apart in the loop below
    typedef _Float16 hf4 __attribute__((ext_vector_type(4)));
    typedef _Float16 hfK __attribute__((ext_vector_type(KB)));
    struct Pieces {
        hf4 ah[2], al[2];      // rows arow and arow + AR: 4 values each
        hfK bh, bl;
    };
    auto split = [&](const Stage& r, Pieces& q) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                _Float16 x, y;
                unsigned aj = r.a[(i * 4 + j) % (HALF ? 4 : 8)];
                if constexpr (GEN) aj = j < r.am ? aj : 0u;                // dy beyond the row's last column
                split2h(__uint_as_float(aj) * sdy, x, y);
                q.ah[i][j] = x;
                q.al[i][j] = y;
            }
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            unsigned bj = r.b[j];
            if constexpr (GEN) {
                bj = (r.fix & 256) ? (j == 0 ? 0u : r.b[j == 0 ? 0 : j - 1]) : bj;      // run loaded one element late
                bj = (r.fix >> j & 1) ? 0u : bj;                            // zero padding
            } else {
            if (j == 0) bj = r.fix == 1 ? r.b[1] : bj;                     // run loaded from column 0: wanted (col 1, col 0, col 1, col 2, ...)
            else bj = r.fix == 1 ? r.b[j - 1] : bj;
            if (j == KB - 1) bj = r.fix == 2 ? r.b[KB - 3] : bj;           // column W mirrors to column W - 2
            }
            _Float16 x, y;
            split2h(__uint_as_float(bj) * sx, x, y);
            q.bh[j] = x;
            q.bl[j] = y;
        }
    };
    auto write = [&](const Pieces& q, int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<hf4*>(reinterpret_cast<_Float16*>(&As[buf][0][ahalf * AH + arow + i * AR]) + asub) = q.ah[i];
            *reinterpret_cast<hf4*>(reinterpret_cast<_Float16*>(&As[buf][NP - 1][ahalf * AH + arow + i * AR]) + asub) = q.al[i];
        }
        *reinterpret_cast<hfK*>(reinterpret_cast<_Float16*>(&Bs[buf][0][bhalf * BH + bcol]) + bsub) = q.bh;
        *reinterpret_cast<hfK*>(reinterpret_cast<_Float16*>(&Bs[buf][NP - 1][bhalf * BH + bcol]) + bsub) = q.bl;
    };

    auto stash = [&](const Stage& r, int buf) {
        if constexpr (!HALF) {
            Pieces q;
            split(r, q);
            write(q, buf);
        } else {                   // stored bf16 patterns as they are
            u32x4 v;
            v.x = r.a[0]; v.y = r.a[1]; v.z = r.a[2]; v.w = r.a[3];
            *reinterpret_cast<u32x4*>(&As[buf][0][ahalf * AH + arow]) = v;
            typedef unsigned short usK __attribute__((ext_vector_type(KB)));
            usK w;
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                unsigned bj = r.b[j];
                if constexpr (GEN) {
                    bj = (r.fix & 256) ? (j == 0 ? 0u : r.b[j == 0 ? 0 : j - 1]) : bj;      // run loaded one element late
                    bj = (r.fix >> j & 1) ? 0u : bj;                                         // zero padding
                } else if constexpr (STRIDE == 1) {                                          // inline reflection, as in split() above
                    if (j == 0) bj = r.fix == 1 ? r.b[1] : bj;
                    else bj = r.fix == 1 ? r.b[j - 1] : bj;
                    if (j == KB - 1) bj = r.fix == 2 ? r.b[KB - 3] : bj;
                }
                w[j] = (unsigned short)bj;
            }
            *reinterpret_cast<usK*>(reinterpret_cast<unsigned short*>(&Bs[buf][0][bhalf * BH + bcol]) + bsub) = w;
        }
    };
    constexpr int NJ = 2 * NC;                  // 32-column blocks of a wave (its half of the workgroup's columns)
    f32x16 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    struct Operands {
        bf16x8 A[NP][2], B[NP][NJ];
    };
    auto fetch = [&](Operands& o, int buf) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int i = 0; i < 2; ++i) o.A[p][i] = As[buf][p][hi * AH + wm * 64 + i * 32 + lo];
#pragma unroll
            for (int j = 0; j < NJ; ++j) o.B[p][j] = Bs[buf][p][hi * BH + wp * (CW / 2) + j * 32 + lo];
        }
    };
    auto mma = [&](const Operands& o) {
        if constexpr (HALF) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(o.A[0][i], o.B[0][j], acc[i][j], 0, 0, 0);
        } else {      // (l,h) (h,l) (h,h)
            constexpr int PA[3] = {NP - 1, 0, 0}, PB[3] = {0, NP - 1, 0};
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, o.A[PA[q]][i]),
                                                                            __builtin_bit_cast(f16x8, o.B[PB[q]][j]), acc[i][j], 0, 0, 0);
        }
    };
    auto interleave = [&]() {
        if constexpr (HALF) {
#pragma unroll
            for (int q = 0; q < 4 * NC; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 12 * NC; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                   // one MFMA
                if (q < 4 + 4 * NC) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // LDS reads of the next stage first
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);                   // split arithmetic
                if (q >= 8) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);       // LDS writes
                if (q >= 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);       // global loads
            }
        }
    };

    // the software pipeline of the convolution kernels above: global loads three stages ahead, LDS one, operands in registers
    Stage rg[2];
    Operands op[2];
    load(rg[0]);
    load(rg[1]);
    stash(rg[0], 0);
    __syncthreads();
    load(rg[0]);
    fetch(op[0], 0);
    stash(rg[1], 1);
    __syncthreads();
    load(rg[1]);
    const int nst2 = (nst_here + 1) & ~1;
    if constexpr (HALF) {
        for (int s = 0; s < nst2; s += 2) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fetch(op[(t + 1) & 1], (t + 1) & 1);     // operands of stage s+t+1
                mma(op[t]);                              // stage s+t
                stash(rg[t], t);                         // stage s+t+2
                load(rg[t]);                             // stage s+t+4
                interleave();
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
        // fp16 route: TWO SLOTS per stage, and the two waves of a SIMD (w and w + 4) run them in opposite order --
        //   slot X   the 12 MFMAs of stage k (operands in registers) with the split arithmetic of stage k+2 between them
        //   slot Y   pieces of stage k+2 to LDS, global loads of stage k+4, LDS reads of the operands of stage k+1
        // waves 4-7 start one slot late, so that in every slot one wave of each SIMD feeds the matrix pipe while the other works
        // the LDS / memory side (with all eight waves in the same phase the two kinds of work ran one after the other: the kernel
        // took the SUM of its MFMA time and its load / split / LDS time).  Buffer k & 1 holds stage k: written in the Y slots
        // 2k-3 (waves 0-3) and 2k-2 (waves 4-7), read in the Y slots 2k-1 and 2k, rewritten from slot 2k+1 on; a barrier ends
        // every slot.
        const bool late = wave >= NT / 128;
        if (late) {
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        for (int s = 0; s < nst2; s += 2) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                Pieces q;
                split(rg[t], q);                         // stage s+t+2
                mma(op[0]);                              // stage s+t
#pragma unroll
                for (int m = 0; m < 12; ++m) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
                write(q, t);                             // stage s+t+2 over stage s+t
                load(rg[t]);                             // stage s+t+4
                fetch(op[0], (t + 1) & 1);               // operands of stage s+t+1
                __builtin_amdgcn_sched_barrier(0);
                __syncthreads();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (!late) {
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // epilogue: acc[i][j][r] = part[split][row wm*64 + i*32 + (r/4)*8 + hi*4 + r%4][column wp*64 + j*32 + lo]
    const float isx = 1.f / sx, isd = 1.f / sdy;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cg = bx * CW + wp * (CW / 2) + j * 32 + lo;
        if (cg >= CT) continue;
        float* out = a.part + (size_t)by * a.K * CT + cg;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + (r >> 2) * 8 + hi * 4 + (r & 3);
                const float v = (acc[i][j][r] * isx) * isd;
                if (m < a.K) {
                    out[(size_t)m * CT] = v;
                    if constexpr (!HALF) bad |= is_nonfinite(v);
                }
            }
    }
    if constexpr (!HALF) report_nonfinite(a.ovf, bad);
}

// the instantiation for the tile BM x (128 or 256 columns), the form (GEN or padded copy / inline reflection) and the storage type
template <int BM, int STRIDE>
static void launch_tile(const HWgradArgs& a, int cw, bool gen, bool half, dim3 grid, hipStream_t st) {
    if (gen) {
        if (half && cw == 256) hipLaunchKernelGGL((hsplit_wgrad_kernel<256, STRIDE, bf16, 2, 1>), grid, dim3(512), 0, st, a);
        else if (half) hipLaunchKernelGGL((hsplit_wgrad_kernel<BM, STRIDE, bf16, 1, 1>), grid, dim3(BM * 2), 0, st, a);
        else hipLaunchKernelGGL((hsplit_wgrad_kernel<BM, STRIDE, float, 1, 1>), grid, dim3(BM * 2), 0, st, a);
        return;
    }
    if constexpr (BM == 256) {      // 256 columns per workgroup exist with the 256-row tile only
        if (cw == 256) {
            if (half) hipLaunchKernelGGL((hsplit_wgrad_kernel<256, STRIDE, bf16, 2>), grid, dim3(512), 0, st, a);
            else hipLaunchKernelGGL((hsplit_wgrad_kernel<256, STRIDE, float, 2>), grid, dim3(512), 0, st, a);
            return;
        }
    }
    if (half) hipLaunchKernelGGL((hsplit_wgrad_kernel<BM, STRIDE, bf16, 1>), grid, dim3(BM * 2), 0, st, a);
    else hipLaunchKernelGGL((hsplit_wgrad_kernel<BM, STRIDE, float, 1>), grid, dim3(BM * 2), 0, st, a);
}

int launch_hsplit_wgrad(const HWgradArgs& a, int bm, int stride, int cw, bool gen, bool half, dim3 grid, hipStream_t st) {
    if (bm == 256 && stride == 1) launch_tile<256, 1>(a, cw, gen, half, grid, st);
    else if (bm == 256) launch_tile<256, 2>(a, cw, gen, half, grid, st);
    else if (stride == 1) launch_tile<128, 1>(a, cw, gen, half, grid, st);
    else launch_tile<128, 2>(a, cw, gen, half, grid, st);
    PCGAN_LAUNCH_CHECK();
    return 0;
}

}  // namespace pcgan
