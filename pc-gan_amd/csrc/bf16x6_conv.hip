// Convolutions on the bf16 / fp16 matrix pipe with operands split into pieces (fp32 tensors: three bf16 pieces and six products, or
// two scaled fp16 pieces and three -- the "fp16 route", the default of the residual blocks; bf16 tensors: as they are, one product):
// the HOST side -- shape predicates, tile choice, packed sizes, workspace layouts and every entry point of the C-ABI.
//
// Kernels, each in the unit that owns its launcher (bsplit.h declares the launchers):
//   halo_conv.hip     bsplit_halo_kernel     -- the window kernel: residual forward and data gradient, the step's hot kernel
//   hsplit_wgrad.hip  hsplit_wgrad_kernel    -- per-tap weight gradient of every >= 32-channel layer outside the row ring
//   bsplit_conv.hip   bsplit_conv_fwd_kernel -- per-tap gather on bf16 pieces: PCGAN_SPLIT=bf16 and what the window kernel refuses
//   bsplit_pack.hip   bsplit_pack_* / bsplit_pad_* / bsplit_wgrad_reduce -- weight packs, padded copy, pack of dy, sum of splits
//   amax.hip          absmax / amax_audit / weight_row_absmax -- the operand maxima the fp16 routes scale by
// What bounds them: DESIGN.md sections 3 and 8.  Reference call sites replaced: see include/pcgan_hip.h and the kernel units.
#include "bsplit.h"

#include <mutex>

namespace pcgan {

// M tile: 256 rows (8 waves share one gathered pixel tile) when the produced channels fill it, else 128
static inline int bsplit_bm(int rows) { return rows % 256 == 0 ? 256 : 128; }

// bytes of a packed operand image [piece][M tile][stage][k half][bm rows][8 values of 2 bytes]
static inline size_t packed_image_bytes(int np, int nMt, int nst, int bm) { return (size_t)np * nMt * nst * 32 * bm; }

// the packed weights of one pass: rows = the channels the pass produces (forward: K, data gradient: C) in tiles of bm, stages =
// (16-channel chunk of the gathered channels, tap); bytes = one image (the per-tap data gradient holds three, one per row class)
struct PackGeom {
    int bm, nMt, nst;
    size_t bytes;
};
static PackGeom pack_geom(const pcgan_conv_desc* d, int pass, int np, int bm) {
    const int rows = pass == PCGAN_PASS_BWD_DATA ? d->C : d->K, chan = pass == PCGAN_PASS_BWD_DATA ? d->K : d->C;
    PackGeom g;
    g.bm = bm;
    g.nMt = (rows + bm - 1) / bm;
    g.nst = (chan / 16) * d->R * d->S;
    g.bytes = packed_image_bytes(np, g.nMt, g.nst, bm);
    return g;
}
// bf16 pieces (three of fp32 tensors, bf16 tensors as they are) | two fp16 pieces, always the window kernel's 256-row tile
static PackGeom bsplit_geom(const pcgan_conv_desc* d, int pass) {
    return pack_geom(d, pass, np_of(d), bsplit_bm(pass == PCGAN_PASS_BWD_DATA ? d->C : d->K));
}
static PackGeom hsplit_geom(const pcgan_conv_desc* d, int pass) { return pack_geom(d, pass, 2, 256); }

// shape rule of the bf16-piece forward: what pcgan_conv2d_bsplit_supported answers, and which rule refuses for bsplit_check's text
enum { BS_TAKES = 0, BS_NO_DESC, BS_NO_SHAPE, BS_NO_PAD, BS_NO_SIZE };
static int bsplit_refusal(const pcgan_conv_desc* d) {
    if (!d) return BS_NO_DESC;
    if (!(d->stride == 1 && d->C % 16 == 0 && d->R * d->S <= BS_MAXTAP && d->K >= 32)) return BS_NO_SHAPE;
    if (!(d->pad_mode == 0 || (d->pad < d->H && d->pad < d->W))) return BS_NO_PAD;
    if (!((size_t)d->N * d->C * d->H * d->W * 4 < 0x80000000ull)) return BS_NO_SIZE;
    return BS_TAKES;
}

static int bsplit_check(const pcgan_conv_desc* d) {
    const int no = bsplit_refusal(d);
    PCGAN_CHECK(no != BS_NO_DESC, "conv2d_bsplit: null descriptor");
    PCGAN_CHECK(d->dtype == PCGAN_F32 || d->dtype == PCGAN_BF16, "conv2d_bsplit: dtype %d", d->dtype);
    PCGAN_CHECK(no != BS_NO_SHAPE, "conv2d_bsplit: unsupported shape");
    PCGAN_CHECK(d->P == d->H + 2 * d->pad - d->R + 1 && d->Q == d->W + 2 * d->pad - d->S + 1, "conv2d_bsplit: output dims");
    PCGAN_CHECK(no != BS_NO_PAD, "conv2d_bsplit: reflection pad too large");
    PCGAN_CHECK(no != BS_NO_SIZE, "conv2d_bsplit: input beyond 2 GiB");
    return 0;
}

// the halo kernel takes a layer when a pixel tile is whole image rows and the chunks come in pairs; option "bsplit_halo" = 0 keeps
// every layer on the per-tap gather kernel (A/B measurement)
static bool halo_enabled() { return option(OPT_BSPLIT_HALO) != 0; }
static bool halo_geometry(int chan, int rows_out, int H, int W) {
    return (W == 32 || W == 64) && H >= 4 && H % (128 / W) == 0 && chan % 32 == 0 && rows_out % 256 == 0;
}
static bool halo_shape(int chan, int rows_out, int H, int W) { return halo_enabled() && halo_geometry(chan, rows_out, H, W); }
static inline int bsplit_pk(const pcgan_conv_desc* d) { return d->dtype == PCGAN_BF16 ? PK_BF16 : PK_BF16X3; }

// arguments of the window kernel for one pass: X = the tensor it gathers (forward: x, data gradient: dy), a_bytes = the packed image it
// reads.  x_amax given = the fp16 route: the row maxima of the weights sit behind the image and the non-finite sentinel is on
static HaloArgs halo_args(const pcgan_conv_desc* d, int pass, const void* X, const void* packed, size_t a_bytes, const float* bias, void* Y,
                          int act, float slope, const float* x_amax = nullptr, int n_amax = 0) {
    const int rows = pass == PCGAN_PASS_BWD_DATA ? d->C : d->K, chan = pass == PCGAN_PASS_BWD_DATA ? d->K : d->C;
    HaloArgs h{};
    h.X = X; h.A = packed; h.bias = bias; h.Y = Y;
    h.N = d->N; h.C = chan; h.H = d->H; h.M = rows; h.nMt = (rows + 255) / 256; h.nch = chan / 16; h.act = act; h.slope = slope;
    h.x_bytes = (unsigned)((size_t)d->N * chan * d->H * d->W * es_of(d));
    h.a_bytes = (unsigned)a_bytes;
    if (x_amax) {
        h.x_amax = x_amax;
        h.x_namax = n_amax;
        h.w_amax = (const float*)((const char*)packed + a_bytes);
        h.ovf = nonfinite_counter();
    }
    return h;
}

// arguments of the per-tap kernel for one pass over the packed weights g: X = the tensor it gathers.  The data gradient adds its row
// classes and the weight gradient its split of the reduction (both zero here)
static BsplitArgs bsplit_args(const pcgan_conv_desc* d, int pass, const PackGeom& g, const void* X, const void* packed, const float* bias,
                              void* Y, int act, float slope) {
    BsplitArgs a{};
    a.X = X; a.A = packed; a.bias = bias; a.Y = Y;
    a.N = d->N; a.C = pass == PCGAN_PASS_BWD_DATA ? d->K : d->C; a.H = d->H; a.W = d->W; a.M = pass == PCGAN_PASS_BWD_DATA ? d->C : d->K;
    a.R = d->R; a.S = d->S; a.pad = d->pad; a.reflect = d->pad_mode;
    a.P = d->P; a.Q = d->Q;
    a.nMt = g.nMt; a.nst = g.nst;
    a.act = act; a.slope = slope;
    a.x_bytes = (unsigned)((size_t)d->N * a.C * d->H * d->W * es_of(d));
    a.a_bytes = (unsigned)g.bytes;
    return a;
}

// host-side record of the last launch the bsplit entries issued (pcgan_bsplit_last_launch): a record of its own, written by the forward,
// the data gradient and the weight gradient once their main kernel's launch has been attempted, before its status is read
static std::mutex g_bsplit_mu;
static int g_bsplit_rec[PCGAN_BSPLIT_LAUNCH_INFO] = {0};
static void bsplit_record(int kernel, int mode, int bm, int dtype, int row_tiles, long tiles, int nst, int splits, int nst_split, int copy) {
    std::lock_guard<std::mutex> lk(g_bsplit_mu);
    const int v[PCGAN_BSPLIT_LAUNCH_INFO] = {g_bsplit_rec[0] + 1, kernel, mode, bm, dtype, row_tiles, (int)tiles, nst, splits, nst_split, copy};
    for (int i = 0; i < PCGAN_BSPLIT_LAUNCH_INFO; ++i) g_bsplit_rec[i] = v[i];
}
// the window kernel's launch in the same terms: one 256-row tile form, pixel tiles of 128 pixels, stages = (16-channel chunk, tap)
static int launch_halo_recorded(int mode, const pcgan_conv_desc* d, const HaloArgs& h, hipStream_t st) {
    const int e = launch_halo(mode, bsplit_pk(d), d->W, h, st);
    bsplit_record(1, mode, 256, d->dtype, h.nMt, (long)d->N * d->H * d->W / 128, h.nch * 9, 1, h.nch * 9, 0);
    return e;
}

}  // namespace pcgan

using namespace pcgan;

extern "C" int pcgan_conv2d_bsplit_supported(const pcgan_conv_desc* d) { return bsplit_refusal(d) == BS_TAKES; }

extern "C" size_t pcgan_conv2d_bsplit_packed_bytes(const pcgan_conv_desc* d) {
    return pcgan_conv2d_bsplit_supported(d) ? bsplit_geom(d, PCGAN_PASS_FWD).bytes : 0;
}

extern "C" int pcgan_conv2d_bsplit_pack(const pcgan_conv_desc* d, const float* w, void* packed, pcgan_stream_t s) {
    if (bsplit_check(d)) return 1;
    PCGAN_CHECK(w && packed, "conv2d_bsplit_pack: null pointer");
    const PackGeom g = bsplit_geom(d, PCGAN_PASS_FWD);
    return launch_bsplit_pack(w, packed, d->K, d->C, d->R * d->S, g.nMt, g.nst, g.bm, np_of(d), nullptr, (hipStream_t)s);
}

extern "C" int pcgan_conv2d_fwd_bsplit(const pcgan_conv_desc* d, const void* x, const void* packed, const float* bias, void* y,
                                       int act, float slope, pcgan_stream_t s) {
    if (bsplit_check(d)) return 1;
    PCGAN_CHECK(x && packed && y, "conv2d_fwd_bsplit: null pointer");
    TimerScope timer(timer_kind_res(d, TIMER_RES_FWD), (hipStream_t)s);
    const PackGeom g = bsplit_geom(d, PCGAN_PASS_FWD);
    PCGAN_CHECK(g.bytes < 0x80000000ull, "conv2d_fwd_bsplit: packed weights beyond 2 GiB");
    if (d->pad_mode == 1 && d->R == 3 && d->S == 3 && d->pad == 1 && halo_shape(d->C, d->K, d->H, d->W))
        return launch_halo_recorded(BH_FWD, d, halo_args(d, PCGAN_PASS_FWD, x, packed, g.bytes, bias, y, act, slope), (hipStream_t)s);
    const long ptiles = ((long)d->N * d->P * d->Q + 127) / 128;
    const int mode = d->pad_mode == 1 ? BS_FWD_REFLECT : BS_FWD_ZERO;
    const int e = launch_bsplit(mode, d->dtype, g.bm, dim3((unsigned)(ptiles * g.nMt)), bsplit_args(d, PCGAN_PASS_FWD, g, x, packed, bias, y, act, slope),
                                (hipStream_t)s);
    bsplit_record(0, mode, g.bm, d->dtype, g.nMt, ptiles, g.nst, 1, g.nst, 0);
    return e;
}

// ---- data gradient of the reflection-padded 3x3 stride-1 convolution ---------------------------------------------------------
extern "C" int pcgan_conv2d_bsplit_dgrad_supported(const pcgan_conv_desc* d) {
    return d && d->stride == 1 && d->pad_mode == 1 && d->pad == 1 && d->R == 3 && d->S == 3 && d->K % 16 == 0 && d->C >= 32 &&
           d->H >= 4 && d->W >= 4 && d->P == d->H && d->Q == d->W && (size_t)d->N * d->K * d->H * d->W * 4 < 0x80000000ull;
}

extern "C" size_t pcgan_conv2d_bsplit_dgrad_packed_bytes(const pcgan_conv_desc* d) {
    return pcgan_conv2d_bsplit_dgrad_supported(d) ? 3 * bsplit_geom(d, PCGAN_PASS_BWD_DATA).bytes : 0;      // three row classes
}

extern "C" int pcgan_conv2d_bsplit_dgrad_pack(const pcgan_conv_desc* d, const float* w, void* packed, pcgan_stream_t s) {
    PCGAN_CHECK(pcgan_conv2d_bsplit_dgrad_supported(d), "conv2d_bsplit_dgrad_pack: unsupported shape");
    PCGAN_CHECK(w && packed, "conv2d_bsplit_dgrad_pack: null pointer");
    const PackGeom g = bsplit_geom(d, PCGAN_PASS_BWD_DATA);
    return launch_bsplit_pack_dgrad(w, packed, d->K, d->C, g.nMt, g.nst, g.bm, np_of(d), nullptr, 3, (hipStream_t)s);
}

extern "C" int pcgan_conv2d_bwd_data_bsplit(const pcgan_conv_desc* d, const void* dy, const void* packed, void* dx, pcgan_stream_t s) {
    PCGAN_CHECK(pcgan_conv2d_bsplit_dgrad_supported(d), "conv2d_bwd_data_bsplit: unsupported shape");
    PCGAN_CHECK(d->dtype == PCGAN_F32 || d->dtype == PCGAN_BF16, "conv2d_bwd_data_bsplit: dtype %d", d->dtype);
    PCGAN_CHECK(dy && packed && dx, "conv2d_bwd_data_bsplit: null pointer");
    TimerScope timer(timer_kind_res(d, TIMER_RES_DGRAD), (hipStream_t)s);
    const PackGeom g = bsplit_geom(d, PCGAN_PASS_BWD_DATA);      // one row class
    PCGAN_CHECK(3 * g.bytes < 0x80000000ull, "conv2d_bwd_data_bsplit: packed weights beyond 2 GiB");
    if (halo_shape(d->K, d->C, d->H, d->W))      // plain flipped weights = row class 0 of the packed buffer
        return launch_halo_recorded(BH_DGRAD, d, halo_args(d, PCGAN_PASS_BWD_DATA, dy, packed, g.bytes, nullptr, dx, PCGAN_ACT_NONE, 0.f),
                                    (hipStream_t)s);
    BsplitArgs a = bsplit_args(d, PCGAN_PASS_BWD_DATA, g, dy, packed, nullptr, dx, PCGAN_ACT_NONE, 0.f);
    a.phase_bytes = (unsigned)g.bytes;
    a.a_bytes = (unsigned)(3 * g.bytes);
    const long rows[3] = {(long)d->H - 2, 1, 1};
    long t = 0;
    for (int p = 0; p < 3; ++p) {
        a.tstart[p] = (int)t;
        t += ((long)d->N * rows[p] * d->W + 127) / 128;
    }
    a.tstart[3] = (int)t;
    const int e = launch_bsplit(BS_DGRAD_REFLECT, d->dtype, g.bm, dim3((unsigned)(t * a.nMt)), a, (hipStream_t)s);
    bsplit_record(0, BS_DGRAD_REFLECT, g.bm, d->dtype, g.nMt, t, g.nst, 1, g.nst, 0);
    return e;
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------
extern "C" int pcgan_conv2d_bsplit_wgrad_supported(const pcgan_conv_desc* d) {
    return d && d->stride == 1 && d->pad_mode == 1 && d->R == 3 && d->S == 3 && d->pad == 1 && d->W % 16 == 0 &&
           (d->K == 128 || d->K == 256) &&      // one full row tile: all pcgan_conv2d_bwd_weight_bsplit builds
           d->P == d->H && d->Q == d->W && (size_t)d->N * d->C * (d->H + 2) * (d->W + 2) * 4 < 0x80000000ull &&
           (size_t)d->N * d->H * d->W * 3 * 2 * (size_t)bsplit_bm(d->K) < 0x80000000ull;
}

static inline int bsplit_wgrad_splits(const pcgan_conv_desc* d, int bm, int* nst_split) {
    const int nst = d->N * d->H * d->W / 16;
    const long tiles = (long)((d->C * 9 + 127) / 128) * ((d->K + bm - 1) / bm);
    long want = (bm == 256 ? 256 : 512) / tiles;          // one round of resident workgroups
    if (want < 1) want = 1;
    if (want > nst / 8) want = nst / 8 > 0 ? nst / 8 : 1;
    *nst_split = (int)((nst + want - 1) / want);
    return (nst + *nst_split - 1) / *nst_split;
}

// workspace: [padded copy of x][dy packed as the A operand][partial sums of the splits], the first two padded to 256 bytes
struct BsplitWgradWs {
    int bm, nMt, nst, splits, nst_split;
    size_t xpad, packed, part;      // bytes
};
static BsplitWgradWs bsplit_wgrad_ws(const pcgan_conv_desc* d) {
    BsplitWgradWs w;
    w.bm = bsplit_bm(d->K);
    w.nMt = (d->K + w.bm - 1) / w.bm;
    w.nst = d->N * d->H * d->W / 16;      // stages of 16 consecutive elements of the (n, y, x) reduction
    w.splits = bsplit_wgrad_splits(d, w.bm, &w.nst_split);
    w.xpad = align_up((size_t)d->N * d->C * (d->H + 2) * (d->W + 2) * 4, 256);
    w.packed = align_up(packed_image_bytes(3, w.nMt, w.nst, w.bm), 256);      // (sized for the fp32 / 3-piece case; the bf16 path uses less of it)
    w.part = (size_t)w.splits * w.nMt * w.bm * d->C * 9 * 4;
    return w;
}

extern "C" size_t pcgan_conv2d_bsplit_wgrad_workspace_bytes(const pcgan_conv_desc* d) {
    if (!pcgan_conv2d_bsplit_wgrad_supported(d)) return 0;
    const BsplitWgradWs w = bsplit_wgrad_ws(d);
    return w.xpad + w.packed + w.part;
}

extern "C" int pcgan_conv2d_bwd_weight_bsplit(const pcgan_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate,
                                              void* ws, size_t ws_bytes, pcgan_stream_t s) {
    PCGAN_CHECK(pcgan_conv2d_bsplit_wgrad_supported(d), "conv2d_bwd_weight_bsplit: unsupported shape");
    PCGAN_CHECK(d->dtype == PCGAN_F32 || d->dtype == PCGAN_BF16, "conv2d_bwd_weight_bsplit: dtype %d", d->dtype);
    PCGAN_CHECK(x && dy && dw && ws && ws_bytes >= pcgan_conv2d_bsplit_wgrad_workspace_bytes(d), "conv2d_bwd_weight_bsplit: null pointer or small workspace");
    TimerScope timer(timer_kind_res(d, TIMER_RES_WGRAD), (hipStream_t)s);
    const BsplitWgradWs w = bsplit_wgrad_ws(d);
    PCGAN_CHECK(d->K % w.bm == 0, "conv2d_bwd_weight_bsplit: output channels must fill the %d-row tile", w.bm);
    hipStream_t st = (hipStream_t)s;
    const bool half = d->dtype == PCGAN_BF16;
    void* xpad = ws;
    void* packed = (char*)ws + w.xpad;
    float* part = (float*)((char*)ws + w.xpad + w.packed);
    PCGAN_CHECK(d->N * d->C <= 65535, "conv2d_bwd_weight_bsplit: more than 65535 planes");
    if (int e = launch_pad(x, xpad, d->N * d->C, d->H, d->W, 1, 1, half, st)) return e;
    PCGAN_CHECK(w.nMt == 1, "conv2d_bwd_weight_bsplit: more than one %d-row tile of output channels is not built", w.bm);
    if (int e = launch_pack_dy(dy, packed, d->K, d->H * d->W, w.nst, w.bm, np_of(d), half, st)) return e;
    // the GEMM with the roles turned: the "weights" are the packed dy, the "pixels" the columns (c, r, s), gathered from the padded copy
    const PackGeom g{w.bm, w.nMt, w.nst, packed_image_bytes(np_of(d), w.nMt, w.nst, w.bm)};
    BsplitArgs a = bsplit_args(d, PCGAN_PASS_BWD_WEIGHT, g, xpad, packed, nullptr, part, PCGAN_ACT_NONE, 0.f);
    a.P = 1; a.Q = d->C * 9;
    a.nst_split = w.nst_split;
    a.x_bytes = (unsigned)((size_t)d->N * d->C * (d->H + 2) * (d->W + 2) * es_of(d));
    const dim3 grid((unsigned)(((d->C * 9 + 127) / 128) * w.nMt), (unsigned)w.splits);
    const int e = launch_bsplit(BS_WGRAD, d->dtype, w.bm, grid, a, st);
    bsplit_record(0, BS_WGRAD, w.bm, d->dtype, w.nMt, (d->C * 9 + 127) / 128, w.nst, w.splits, w.nst_split, pad_copy_form(d->N * d->C, d->H, d->W, 1));
    if (e) return e;
    return launch_wgrad_reduce(part, dw, w.splits, (size_t)d->K * d->C * 9, accumulate, st);
}

// ---- fp16 two-piece route of the reflection-padded 3x3 convolution (forward + data gradient), fp32 tensors -------------------------
// packed buffer: [2 pieces][M tile][stage][k half][256 rows][8 fp16] (data gradient: the plain flipped weights -- the window kernel
// has no row classes) followed by the largest magnitude of every weight ROW (one float per produced channel, padded to 256 bytes):
// row m is scaled by its own power of two, pow2_scale(rowmax[m]), which the epilogue divides out again -- exactly
extern "C" int pcgan_conv2d_hsplit_supported(const pcgan_conv_desc* d, int pass) {
    if (!d || d->dtype != PCGAN_F32 || d->stride != 1 || d->pad_mode != 1 || d->pad != 1 || d->R != 3 || d->S != 3) return 0;
    if (d->P != d->H || d->Q != d->W || (size_t)d->N * (d->C > d->K ? d->C : d->K) * d->H * d->W * 4 >= 0x80000000ull) return 0;
    if (pass == PCGAN_PASS_FWD) return halo_geometry(d->C, d->K, d->H, d->W) && hsplit_geom(d, pass).bytes < 0x80000000ull;
    if (pass == PCGAN_PASS_BWD_DATA) return halo_geometry(d->K, d->C, d->H, d->W) && hsplit_geom(d, pass).bytes < 0x80000000ull;
    return 0;
}

static size_t hsplit_tail_bytes(const pcgan_conv_desc* d, int pass) {
    return align_up((size_t)(pass == PCGAN_PASS_FWD ? d->K : d->C) * 4, 256);
}
extern "C" size_t pcgan_conv2d_hsplit_packed_bytes(const pcgan_conv_desc* d, int pass) {
    return pcgan_conv2d_hsplit_supported(d, pass) ? hsplit_geom(d, pass).bytes + hsplit_tail_bytes(d, pass) : 0;
}

extern "C" int pcgan_conv2d_hsplit_pack(const pcgan_conv_desc* d, int pass, const float* w, void* packed, pcgan_stream_t s) {
    PCGAN_CHECK(pcgan_conv2d_hsplit_supported(d, pass), "conv2d_hsplit_pack: unsupported shape or pass");
    PCGAN_CHECK(w && packed, "conv2d_hsplit_pack: null pointer");
    hipStream_t st = (hipStream_t)s;
    const PackGeom g = hsplit_geom(d, pass);
    float* amax = (float*)((char*)packed + g.bytes);     // the tail: the largest magnitude of every row of this pass's weight matrix
    if (int e = launch_weight_row_absmax(w, d->K, d->C, 9, pass == PCGAN_PASS_FWD ? 0 : 1, amax, st)) return e;
    if (pass == PCGAN_PASS_FWD) return launch_bsplit_pack(w, packed, d->K, d->C, 9, g.nMt, g.nst, g.bm, 2, amax, st);
    return launch_bsplit_pack_dgrad(w, packed, d->K, d->C, g.nMt, g.nst, g.bm, 2, amax, 1, st);      // one row class
}

extern "C" int pcgan_conv2d_fwd_hsplit(const pcgan_conv_desc* d, const void* x, const float* x_amax, int n_amax, const void* packed,
                                       const float* bias, void* y, int act, float slope, pcgan_stream_t s) {
    PCGAN_CHECK(pcgan_conv2d_hsplit_supported(d, PCGAN_PASS_FWD), "conv2d_fwd_hsplit: unsupported shape");
    PCGAN_CHECK(x && x_amax && n_amax > 0 && packed && y, "conv2d_fwd_hsplit: null pointer");
    TimerScope timer(timer_kind_res(d, TIMER_RES_FWD), (hipStream_t)s);
    const HaloArgs h = halo_args(d, PCGAN_PASS_FWD, x, packed, hsplit_geom(d, PCGAN_PASS_FWD).bytes, bias, y, act, slope, x_amax, n_amax);
    return launch_halo(BH_FWD, PK_F16X2, d->W, h, (hipStream_t)s);
}

extern "C" int pcgan_conv2d_bwd_data_hsplit(const pcgan_conv_desc* d, const void* dy, const float* dy_amax, int n_amax, const void* packed,
                                            void* dx, pcgan_stream_t s) {
    return pcgan_conv2d_bwd_data_hsplit_add(d, dy, dy_amax, n_amax, packed, nullptr, dx, s);
}

extern "C" int pcgan_conv2d_bwd_data_hsplit_add(const pcgan_conv_desc* d, const void* dy, const float* dy_amax, int n_amax, const void* packed,
                                                const void* add, void* dx, pcgan_stream_t s) {
    PCGAN_CHECK(pcgan_conv2d_hsplit_supported(d, PCGAN_PASS_BWD_DATA), "conv2d_bwd_data_hsplit: unsupported shape");
    PCGAN_CHECK(dy && dy_amax && n_amax > 0 && packed && dx, "conv2d_bwd_data_hsplit: null pointer");
    TimerScope timer(timer_kind_res(d, TIMER_RES_DGRAD), (hipStream_t)s);
    HaloArgs h = halo_args(d, PCGAN_PASS_BWD_DATA, dy, packed, hsplit_geom(d, PCGAN_PASS_BWD_DATA).bytes, nullptr, dx, PCGAN_ACT_NONE, 0.f,
                           dy_amax, n_amax);      // plain flipped weights
    h.R = add;
    return launch_halo(BH_DGRAD, PK_F16X2, d->W, h, (hipStream_t)s);
}

// weight gradient on the fp16 route (fp32 tensors) / bf16 route (bf16 tensors): padded copy of x (workspace), hsplit_wgrad_kernel over
// splits of the pixel reduction, reduce
// the general form of the kernel (GEN): zero padding of at most 1 applied inside the gather (no padded copy), ragged output width, row
// tiles.  Option "wgrad_gen" = 0 keeps the padded copy (A/B measurement; the ragged widths and K > 256 then leave this route)
static bool hsplit_wgrad_gen(const pcgan_conv_desc* d) {
    if (!option(OPT_WGRAD_GEN) || d->pad_mode != 0 || d->pad > 1) return false;
    return d->dtype == PCGAN_F32 || d->dtype == PCGAN_BF16;      // (bf16 tensors with ragged rows: element loads of dy, rows start on 2-byte boundaries)
}

// the residual-block shape (3x3, stride 1, reflection padding 1): the mirror is applied inside the gather, no padded copy
static bool hsplit_wgrad_inline_reflect(const pcgan_conv_desc* d) {
    return d->stride == 1 && d->pad_mode == 1 && d->pad == 1 && d->R == 3 && d->S == 3 && d->H >= 2 && d->W >= 16 && d->P == d->H &&
           d->Q == d->W && !option(OPT_WGRAD_PADCOPY);
}

extern "C" int pcgan_conv2d_hsplit_wgrad_inline(const pcgan_conv_desc* d) {
    if (!d || !pcgan_conv2d_hsplit_wgrad_supported(d)) return 0;
    return (hsplit_wgrad_inline_reflect(d) || d->pad == 0 || hsplit_wgrad_gen(d)) ? 1 : 0;
}

extern "C" int pcgan_conv2d_hsplit_wgrad_supported(const pcgan_conv_desc* d) {
    if (!d || (d->dtype != PCGAN_F32 && d->dtype != PCGAN_BF16)) return 0;
    if (d->stride != 1 && d->stride != 2) return 0;
    if (d->pad_mode == 1 && (d->stride != 1 || d->pad >= d->H || d->pad >= d->W)) return 0;
    if (d->K < 32 || d->R * d->S > 49 || d->P < 1 || d->Q < 1) return 0;
    const bool gen = hsplit_wgrad_gen(d);
    const int Qs = (d->Q + 15) & ~15;
    if (!gen && (d->Q % 16 != 0 || d->K > 256)) return 0;
    if ((Qs - d->Q) * 4 > Qs) return 0;           // ragged rows: at least three quarters of every 16-column stage are real columns
    if (d->P != (d->H + 2 * d->pad - d->R) / d->stride + 1 || d->Q != (d->W + 2 * d->pad - d->S) / d->stride + 1) return 0;
    // the gather reads xpad rows up to (P-1) stride + R - 1 and columns up to (Q-1) stride + S - 1: inside the padded plane by the two lines above
    return (size_t)d->N * d->C * (d->H + 2 * d->pad) * (d->W + 2 * d->pad) * 4 < 0x80000000ull && (size_t)d->N * d->K * d->P * d->Q * 4 < 0x80000000ull &&
           d->N * d->C <= 65535;
}

static inline int hsplit_wgrad_bm(const pcgan_conv_desc* d) { return d->K > 128 ? 256 : 128; }

// 256 columns per workgroup with the 256-row tile when that still leaves at least 8 column tiles: the dy tile is loaded, split and
// written to LDS once for 256 columns and a wave's 64 x 128 tile needs 12 LDS operand reads for 24 MFMAs instead of 8 for 12.
// bf16 tensors since round 2 (26.5 -> 26.0 ms per bf16 step).  fp32 tensors: the kernel ALONE gains (238 VGPRs, no spills: residual
// shape 0.153 -> 0.139 ms incl. the reduce of twice as many split partials), the STEP loses 1 % (1206 -> 1194 img/s, three interleaved
// pairs on one box: beside the data-gradient kernel of the main stream the wide workgroups take 0.292 instead of 0.277 ms and the
// parameter-gradient stream is the longer one) -- so fp32 tensors keep 128 columns; option "wgrad_cw" = 256 selects the wide form (A/B).
static inline int hsplit_wgrad_cw(const pcgan_conv_desc* d) {
    const int force = option(OPT_WGRAD_CW);      // 0: as measured best; 256: fp32 too; 128: bf16 too
    const bool wide = (d->dtype == PCGAN_BF16 && force != 128) || (d->dtype == PCGAN_F32 && d->pad_mode == 1 && force == 256);
    return wide && hsplit_wgrad_bm(d) == 256 && d->C * d->R * d->S >= 8 * 256 ? 256 : 128;
}

static inline int hsplit_wgrad_splits(const pcgan_conv_desc* d, int* nst_split) {
    const int nst = d->N * d->P * ((d->Q + 15) / 16);
    const int cw = hsplit_wgrad_cw(d);
    const int bmr = hsplit_wgrad_bm(d);
    const long tiles = (long)((d->C * d->R * d->S + cw - 1) / cw) * ((d->K + bmr - 1) / bmr);      // column tiles x row tiles
    long want = (hsplit_wgrad_bm(d) == 256 ? 256 : 512) / tiles;          // one round of resident workgroups
    if (want < 1) want = 1;
    if (want > nst / 8) want = nst / 8 > 0 ? nst / 8 : 1;
    // option "hwgrad_ks" > 0 (tests): that many splits, cut to [1, stages]; the stages of a split and the final count are re-derived below
    const int fk = option(OPT_HWGRAD_KS);
    if (fk > 0) want = fk < nst ? fk : nst;
    *nst_split = (int)((nst + want - 1) / want);
    return (nst + *nst_split - 1) / *nst_split;
}

// workspace of the kernel's own route: [padded copy of x, padded to 256 bytes; none with the GEN form][partial sums of the splits]
struct HsplitWgradWs {
    int splits, nst_split;
    size_t xpad, part;      // bytes
};
static HsplitWgradWs hsplit_wgrad_ws(const pcgan_conv_desc* d) {
    HsplitWgradWs w;
    w.splits = hsplit_wgrad_splits(d, &w.nst_split);
    w.xpad = hsplit_wgrad_gen(d) ? 0 : align_up((size_t)d->N * d->C * (d->H + 2 * d->pad) * (d->W + 2 * d->pad) * 4, 256);
    w.part = (size_t)w.splits * d->K * d->C * d->R * d->S * 4;
    return w;
}

extern "C" size_t pcgan_conv2d_hsplit_wgrad_workspace_bytes(const pcgan_conv_desc* d) {
    if (!pcgan_conv2d_hsplit_wgrad_supported(d)) return 0;
    const HsplitWgradWs w = hsplit_wgrad_ws(d);
    const size_t own = w.xpad + w.part;
    // (option "wgrad_direct": the residual-block shape is handed to the image-innermost form of wgrad_direct.hip, which needs more room)
    const size_t direct = option(OPT_WGRAD_DIRECT) ? pcgan_conv2d_wgrad_direct_workspace_bytes(d) : 0;
    // (option "wgrad_rowring": the same shapes' row-ring form, wgrad_rowring.hip)
    const size_t ring = option(OPT_WGRAD_ROWRING) ? pcgan_conv2d_wgrad_rowring_workspace_bytes(d) : 0;
    const size_t other = direct > ring ? direct : ring;
    return own > other ? own : other;
}

// host-side record of the last launch of hsplit_wgrad_kernel (pcgan_hwgrad_last_launch): a record of its own, written only when the
// per-tap kernel itself is launched
static std::mutex g_hwgrad_mu;
static int g_hwgrad_rec[PCGAN_HWGRAD_LAUNCH_INFO] = {0};

extern "C" int pcgan_conv2d_bwd_weight_hsplit(const pcgan_conv_desc* d, const void* x, const float* x_amax, int n_xamax, const void* dy,
                                              const float* dy_amax, int n_dyamax, float* dw, int accumulate, void* ws, size_t ws_bytes,
                                              pcgan_stream_t s) {
    PCGAN_CHECK(pcgan_conv2d_hsplit_wgrad_supported(d), "conv2d_bwd_weight_hsplit: unsupported shape");
    const bool half = d->dtype == PCGAN_BF16;
    PCGAN_CHECK(x && dy && dw && ws && ws_bytes >= pcgan_conv2d_hsplit_wgrad_workspace_bytes(d), "conv2d_bwd_weight_hsplit: null pointer or small workspace");
    PCGAN_CHECK(half || (x_amax && dy_amax && n_xamax > 0 && n_dyamax > 0), "conv2d_bwd_weight_hsplit: fp32 tensors need their operand maxima");
    if (option(OPT_WGRAD_DIRECT) && pcgan_conv2d_wgrad_direct_supported(d))
        return pcgan_conv2d_bwd_weight_direct(d, x, x_amax, n_xamax, dy, dy_amax, n_dyamax, dw, accumulate, ws, ws_bytes, s);
    if (option(OPT_WGRAD_ROWRING) && pcgan_conv2d_wgrad_rowring_supported(d))
        return pcgan_conv2d_bwd_weight_rowring(d, x, x_amax, n_xamax, dy, dy_amax, n_dyamax, dw, accumulate, ws, ws_bytes, s);
    hipStream_t st = (hipStream_t)s;
    const bool res_like = timer_kind_res(d, 0) == 0;
    TimerScope timer(res_like ? TIMER_RES_WGRAD : -1, st);       // padded copy + main kernel + reduce
    const HsplitWgradWs w = hsplit_wgrad_ws(d);
    const int Hp = d->H + 2 * d->pad, Wp = d->W + 2 * d->pad;
    const size_t es = es_of(d);
    const bool gen = hsplit_wgrad_gen(d);
    void* xpad = ws;
    float* part = (float*)((char*)ws + w.xpad);
    const void* xin = x;
    const bool inline_reflect = hsplit_wgrad_inline_reflect(d);
    int Hx = Hp, Wx = Wp;
    int copy = 0;      // which padded-copy kernel ran (the record)
    if (inline_reflect || gen) {
        Hx = d->H;
        Wx = d->W;
    } else if (d->pad > 0) {
        if (int e = launch_pad(x, xpad, d->N * d->C, d->H, d->W, d->pad, d->pad_mode, half, st)) return e;
        xin = xpad;
        copy = pad_copy_form(d->N * d->C, d->H, d->W, d->pad);
    }
    const int bm = hsplit_wgrad_bm(d), cw = hsplit_wgrad_cw(d);
    HWgradArgs a;
    a.XP = xin; a.DY = dy; a.part = part;
    a.N = d->N; a.C = d->C; a.K = d->K; a.P = d->P; a.Q = d->Q; a.Hp = Hx; a.Wp = Wx; a.R = d->R; a.S = d->S;
    a.reflect_inline = inline_reflect ? 1 : 0;
    a.Qs = (d->Q + 15) & ~15;
    a.pad = d->pad;
    a.splits = w.splits;
    a.nmt = (d->K + bm - 1) / bm;
    a.nst = d->N * d->P * (a.Qs / 16);
    a.nst_split = w.nst_split;
    a.xp_bytes = (unsigned)((size_t)d->N * d->C * Hx * Wx * es);
    a.dy_bytes = (unsigned)((size_t)d->N * d->K * d->P * d->Q * es);
    a.x_amax = x_amax; a.x_namax = n_xamax; a.dy_amax = dy_amax; a.dy_namax = n_dyamax;
    a.ovf = half ? nullptr : nonfinite_counter();
    a.ntile = (d->C * d->R * d->S + cw - 1) / cw;
    a.nwg = a.ntile * w.splits * a.nmt;
    const dim3 grid((unsigned)((a.nwg + 7) & ~7));
    int e;
    {
        TimerScope timer_main(res_like ? TIMER_RES_WGRAD_MAIN : -1, st);
        e = launch_hsplit_wgrad(a, bm, d->stride, cw, gen, half, grid, st);
    }
    {
        std::lock_guard<std::mutex> lk(g_hwgrad_mu);
        const int v[PCGAN_HWGRAD_LAUNCH_INFO] = {g_hwgrad_rec[0] + 1, bm, d->stride, d->dtype, cw, gen ? 2 : (inline_reflect ? 1 : 0), copy, a.nmt, a.ntile,
                                                 w.splits, w.nst_split, a.nst};
        for (int i = 0; i < PCGAN_HWGRAD_LAUNCH_INFO; ++i) g_hwgrad_rec[i] = v[i];
    }
    if (e) return e;
    return launch_wgrad_reduce(part, dw, w.splits, (size_t)d->K * d->C * d->R * d->S, accumulate, st);
}

extern "C" int pcgan_bsplit_last_launch(int* info, int n) {
    using namespace pcgan;
    PCGAN_CHECK(info != nullptr && n > 0, "bsplit_last_launch: null output");
    std::lock_guard<std::mutex> lk(g_bsplit_mu);
    for (int i = 0; i < n; ++i) info[i] = i < PCGAN_BSPLIT_LAUNCH_INFO ? g_bsplit_rec[i] : 0;
    return 0;
}

extern "C" int pcgan_hwgrad_last_launch(int* info, int n) {
    using namespace pcgan;
    PCGAN_CHECK(info != nullptr && n > 0, "hwgrad_last_launch: null output");
    std::lock_guard<std::mutex> lk(g_hwgrad_mu);
    for (int i = 0; i < n; ++i) info[i] = i < PCGAN_HWGRAD_LAUNCH_INFO ? g_hwgrad_rec[i] : 0;
    return 0;
}
