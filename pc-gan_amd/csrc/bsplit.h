// Internal header of the piece-split convolution family (not installed): what its kernel units share -- the vector types, the piece
// splits, the argument structs of a launch -- and the launchers through which the host unit (bf16x6_conv.hip, whose header lists
// the units) reaches the kernels.
#pragma once
#include "common.h"

namespace pcgan {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
static constexpr unsigned BS_OOB = 0x80000000u;
static constexpr int BS_MAXTAP = 25;

__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
    h = (__bf16)x;
    const float r1 = x - (float)h;
    m = (__bf16)r1;
    l = (__bf16)(r1 - (float)m);
}

struct BsplitArgs {
    const void* X;       // [N][C][H][W], storage type TA
    const void* A;       // packed weights (layout: bsplit_conv.hip)
    const float* bias;   // [M] or null
    void* Y;             // [N][M][P][Q], storage type TA (weight gradient: fp32 partial sums)
    int N, C, H, W, M, R, S, pad, reflect, P, Q;
    int nMt, nst, act;
    float slope;
    unsigned x_bytes, a_bytes;
    // data gradient of the reflection-padded 3x3 convolution: three row classes (rows without a mirror image | row 1 | row H-2),
    // each with its own packed weights (the row mirror is folded into them) and its own run of pixel tiles in the grid
    int tstart[4];       // first pixel tile of each phase, tstart[3] = total
    unsigned phase_bytes;
    // weight gradient: blockIdx.y takes stages [y * nst_split, (y + 1) * nst_split) of the pixel reduction and writes a raw partial sum
    int nst_split;
};

enum { BS_FWD_ZERO = 0, BS_FWD_REFLECT = 1, BS_DGRAD_REFLECT = 2, BS_WGRAD = 3 };

// one 16-byte entry (8 values) of every piece of a packed weight image: entry e of piece p sits at A + p * per_piece + 8 e
__device__ __forceinline__ void pack_store8(__bf16* __restrict__ A, size_t e, size_t per_piece, int np, float wscale, const float (&v)[8]) {
    if (np == 2) {       // two fp16 pieces of the scaled value
        f16x8 h, l;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            _Float16 x, y;
            split2h(v[j] * wscale, x, y);
            h[j] = x;
            l[j] = y;
        }
        *reinterpret_cast<f16x8*>(reinterpret_cast<_Float16*>(A) + 8 * e) = h;
        *reinterpret_cast<f16x8*>(reinterpret_cast<_Float16*>(A) + per_piece + 8 * e) = l;
        return;
    }
    bf16x8 h, mm, l;     // np == 1: the weight rounded to nearest-even bf16; np == 3: the exact three-piece split
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        __bf16 x, y, z;
        split3(v[j], x, y, z);
        h[j] = x;
        mm[j] = y;
        l[j] = z;
    }
    *reinterpret_cast<bf16x8*>(A + 8 * e) = h;
    if (np == 3) {
        *reinterpret_cast<bf16x8*>(A + per_piece + 8 * e) = mm;
        *reinterpret_cast<bf16x8*>(A + 2 * per_piece + 8 * e) = l;
    }
}

// the window kernel (halo_conv.hip)
enum { BH_FWD = 0, BH_DGRAD = 1 };

struct HaloArgs {
    const void* X;       // [N][C][H][W], storage type TA (data gradient: dy, C = the convolution's output channels)
    const void* A;       // packed weights [piece][M tile][chunk * 9 + tap][k half][256 rows][8 bf16]
    const float* bias;   // [M] or null
    void* Y;             // [N][M][H][W]
    int N, C, H, M, nMt, nch, act;
    float slope;
    unsigned x_bytes, a_bytes;
    const float* x_amax;   // PK_F16X2: x_namax partial maxima of |X| (device), and the largest magnitude of every weight ROW [M]
    const float* w_amax;   //           (the pack call scaled row m by pow2_scale(w_amax[m]); the epilogue divides by it)
    int x_namax;
    unsigned* ovf;         // non-finite sentinel (common.h), PK_F16X2 only; may be null
    const void* R;         // optional [N][M][H][W] tensor added to the result (after bias / activation): the skip connection's gradient
                           // summed into the data gradient of a residual block's first convolution (autograd's `grad +=` pass)
};

// piece kinds: what an operand element becomes on its way to the matrix pipe
enum { PK_BF16X3 = 0,      // fp32 tensors, three bf16 pieces, six products (exact terms above 2^-24)
       PK_BF16 = 1,        // bf16 tensors as they are, one product
       PK_F16X2 = 2 };     // fp32 tensors, two scaled fp16 pieces, three products

// the per-tap weight gradient (hsplit_wgrad.hip)
struct HWgradArgs {
    const void* XP;        // padded input [N][C][Hp][Wp], storage type TA
    const void* DY;        // [N][K][P][Q]
    float* part;           // [splits][K][C * T]
    int N, C, K, P, Q, Hp, Wp, R, S, nst, nst_split;
    unsigned xp_bytes, dy_bytes;
    const float* x_amax;   // fp16 route: partial maxima of |x| and |dy| (device)
    const float* dy_amax;
    int x_namax, dy_namax;
    int ntile, nwg;        // column tiles, workgroups that have work (the grid is padded to a multiple of 8)
    unsigned* ovf;         // non-finite sentinel (common.h), fp32 tensors only; may be null
    int reflect_inline;    // stride 1, 3x3, reflection padding 1: XP is the UNPADDED input (Hp = H, Wp = W) and the mirror is applied
                           // in the gather -- a per-stage row select and one register move at the two image edges -- instead of by a padded copy
    int splits, nmt;       // splits of the pixel reduction; row tiles of BM output channels (K > 256: the PatchGAN's 512-channel layer)
    int Qs, pad;           // GEN kernels: Q rounded up to a multiple of 16 (the stages of a row; dy beyond column Q enters as zero) and the
                           // ZERO padding (0 or 1) applied inside the gather -- XP is the unpadded input (Hp = H, Wp = W), no padded copy
};

// ---- host side ----------------------------------------------------------------------------------------------------------------
// pieces per operand / bytes per activation element of the descriptor's storage type
static inline int np_of(const pcgan_conv_desc* d) { return d->dtype == PCGAN_BF16 ? 1 : 3; }
static inline size_t es_of(const pcgan_conv_desc* d) { return d->dtype == PCGAN_BF16 ? 2 : 4; }

// ---- the kernel units for the host unit: each picks the instantiation of a launch the host has sized, launches it on `st` and
// returns 0, or a non-zero status with the error text set ----
// bsplit_pack.hip -- padded copy of `planes` planes (reflect = 0: zeros); weights w[M][C][T] -> packed image of M-tile bm with np
// pieces (np = 2: fp16 pieces scaled per row by rowmax); the data gradient's image(s) of the 3x3 convolution w[K][C][3][3] (nphase = 3:
// the three row classes, 1: the plain flipped weights); dy -> the weight gradient's A operand; fixed-order sum of the split partials
int launch_pad(const void* x, void* xpad, int planes, int H, int W, int pad, int reflect, bool half, hipStream_t st);
int pad_copy_form(int planes, int H, int W, int pad);      // the copy kernel launch_pad picks: 1 = one element per thread, 2 = one wave per plane
int launch_bsplit_pack(const float* w, void* packed, int M, int C, int T, int nMt, int nst, int bm, int np, const float* rowmax, hipStream_t st);
int launch_bsplit_pack_dgrad(const float* w, void* packed, int K, int C, int nMt, int nst, int bm, int np, const float* rowmax, int nphase,
                             hipStream_t st);
int launch_pack_dy(const void* dy, void* packed, int K, int HW, int nst, int bm, int np, bool half, hipStream_t st);
int launch_wgrad_reduce(const float* part, float* dw, int splits, size_t total, int accumulate, hipStream_t st);
// bsplit_conv.hip -- bsplit_conv_fwd_kernel: mode = a BS_* value, dtype = the storage type of the activations, bm = 128 or 256
int launch_bsplit(int mode, int dtype, int bm, dim3 grid, const BsplitArgs& a, hipStream_t st);
// halo_conv.hip -- bsplit_halo_kernel over all pixel tiles of a: mode = a BH_* value, pk = a PK_* value, W = image width (32 or 64)
int launch_halo(int mode, int pk, int W, const HaloArgs& a, hipStream_t st);
// hsplit_wgrad.hip -- hsplit_wgrad_kernel: bm = 128 or 256 rows, stride 1 or 2, cw = 128 or 256 columns per workgroup (256 with bm = 256
// only), gen = the form that applies zero padding in the gather, half = bf16 tensors
int launch_hsplit_wgrad(const HWgradArgs& a, int bm, int stride, int cw, bool gen, bool half, dim3 grid, hipStream_t st);

}  // namespace pcgan
