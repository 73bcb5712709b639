"""The packed implicit GEMM on the matrix pipe (csrc/hgemm.hip hgemm_kernel) held to float64, instantiation by instantiation.

hgemm_kernel is the forward and data-gradient route of every fp32 convolution with a multiple of 16 gathered channels outside the
residual trunk (two scaled fp16 pieces, three products) and of the same layers for bf16 tensors (one bf16 product).  It comes in four
tiles (BM x BP = 128x128, 128x64, 64x128, 64x64), two element forms, three modes (forward with zero / reflection padding, data gradient)
and a K split of 1 .. 8 whose partial sums splitk_reduce_kernel adds up (bias and activation in that epilogue).  The host heuristic picks
tile and split from the shape; the library options "hgemm_tile" / "hgemm_ks" force them, and pcgan_igemm_last_launch reports what ran
after the library's clamps -- every case below asserts that record, so a test cannot silently check another instantiation.

Calls go through ops.conv2d_fwd / ops.conv2d_bwd_data with a pack cache (the production path); the reference is oracle.ops_ref.conv2d in
float64.  Bounds (fp32 tensors): relative L2 error < 3e-6 and < 2 x that of the fp32 MFMA kernels + 5e-7, and
max |error| <= 2e-5 of the largest reference magnitude (one wrong edge pixel cannot hide under the norm).  bf16 tensors: per element,
see _bf16_bound.  The per-element and exact-piece cases of every instantiation are in tests/test_gpu_hgemm_cases.py."""
import pytest
import torch

from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

TILES = (128128, 128064, 64128, 64064)
ACTS = (0, 1, 2, 3, 4)       # none, ReLU, LeakyReLU(0.2), tanh, sigmoid: fused into the epilogue / the split-K reduce
SLOPE = 0.2


@pytest.fixture
def force_hgemm():
    """sets the library's "hgemm_tile" / "hgemm_ks" options (cached launch plans hold workspace sizes that depend on them: dropped on
    every change) and restores the heuristic afterwards"""
    from pcgan_amd.hip import lib as L, ops

    def force(tile, ks):
        L.set_option('hgemm_tile', tile)
        L.set_option('hgemm_ks', ks)
        ops.clear_plans()
    try:
        yield force
    finally:
        L.set_option('hgemm_tile', 0)
        L.set_option('hgemm_ks', 0)
        ops.clear_plans()


def _nphase(H, W, k, stride, pad):
    """data gradient: the (y mod stride, x mod stride) phases that own taps (csrc/igemm_conv.hip bwd_plan)"""
    n = 0
    for fy in range(stride):
        for fx in range(stride):
            r0, s0 = (fy + pad) % stride, (fx + pad) % stride
            if r0 < k and s0 < k and fy < H and fx < W:
                n += 1
    return n


def _run(dev, mode, x, w, b, stride, pad, pad_mode, in_hw=None, act=0, dtype=torch.float32):
    """one production call on a fresh pack cache; returns (output on the CPU as float64, the route counted, the launch record)"""
    from pcgan_amd.hip import ops
    xd, wd = x.to(dev).to(dtype), w.to(dev)
    bd = b.to(dev) if b is not None else None
    r0 = dict(ops.ROUTE_STATS)
    seq0 = ops.igemm_last_launch()['seq']
    if mode == 'fwd':
        y = ops.conv2d_fwd(xd, wd, bd, stride, pad, pad_mode, act, SLOPE, pack_cache={})
    else:
        y = ops.conv2d_bwd_data(xd, wd, in_hw, stride, pad, pad_mode, pack_cache={})
    torch.cuda.synchronize()
    rec = ops.igemm_last_launch()
    assert rec['seq'] == seq0 + 1, 'exactly one implicit-GEMM launch per call: %r' % rec
    routes = {k: v - r0.get(k, 0) for k, v in ops.ROUTE_STATS.items() if v != r0.get(k, 0)}
    return y.double().cpu(), routes, rec


def _ref_fwd(x, w, b, stride, pad, pad_mode, act=0):
    y = R.conv2d(x.double(), w.double(), None if b is None else b.double(), stride, pad, pad_mode)
    return R.activation(y, act, SLOPE)


def _ref_dgrad(dy, w, in_hw, stride, pad, pad_mode):
    N, C = dy.shape[0], w.shape[1]
    xz = torch.zeros(N, C, in_hw[0], in_hw[1], dtype=torch.float64, requires_grad=True)
    R.conv2d(xz, w.double(), None, stride, pad, pad_mode).backward(dy.double())
    return xz.grad


def _errs(y, ref):
    return float((y - ref).norm() / ref.norm()), float((y - ref).abs().max() / ref.abs().max())


def _check_fp32(y, y32, ref, what):
    e, emax = _errs(y, ref)
    e32 = _errs(y32, ref)[0]
    assert e < 3e-6 and e < 2 * e32 + 5e-7, '%s: relative L2 %.3e (fp32 MFMA kernels %.3e)' % (what, e, e32)
    assert emax <= 2e-5, '%s: max |error| %.3e of the largest magnitude' % (what, emax)


def _bf16_bound(ref, absref, kp):
    """per-element bound of the bf16 form against float64 on the SAME operands (x as stored in bf16, w rounded to bf16 to nearest even,
    as the kernel rounds it on its way to LDS).  Derivation: a bf16 x bf16 product is exact in fp32 (8 + 8 significand bits), so the
    kernel's only arithmetic error before the store is the fp32 accumulation of the kp products (over MFMA steps, K slices and the split-K
    reduce, plus the bias): |acc - ref| <= g * S with S = sum |x * w| (+ |bias|) and g = (kp + 16) * 2^-24 (one rounding per addition in
    the longest chain; the 16 covers the reduce over <= 8 slices and the bias).  The store rounds to bf16 to nearest even: at most half
    an ulp, 2^-8 of the stored magnitude.  The fused activations are 1-Lipschitz (the LeakyReLU slope is 0.2), so
        |y - act(ref)| <= 2^-8 * (|act(ref)| + g * S) + g * S + 2^-22 * |act(ref)| + 1e-30
    (2^-22: the fp32 tanh / sigmoid of the epilogue; 1e-30 keeps exact zeros exact).  S is computed in float64 as the same convolution of
    |x| with |w|.  Calibration on the matrix below: the largest ratio |error| / bound is 0.98 -- the half-ulp output rounding is attained
    (results just above a power of two), the accumulation term is the margin.  Being per element, the bound holds an entry at a tenth
    of the largest magnitude ten times tighter than the former 4e-3 of the largest magnitude (tests/test_gpu_bf16.py)."""
    g = (kp + 16) * 2.0 ** -24
    a = ref.abs()
    return 2.0 ** -8 * (a + g * absref) + g * absref + 2.0 ** -22 * a + 1e-30


def _check_bf16(y, ref, absref, kp, what):
    bound = _bf16_bound(ref, absref, kp)
    ratio = (y - ref).abs() / bound
    worst = float(ratio.max())
    assert worst <= 1.0, '%s: |error| / bound up to %.3f at %s (error %.3e, bound %.3e)' % (
        what, worst, tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0]), float((y - ref).abs().flatten()[int(ratio.argmax())]),
        float(bound.flatten()[int(ratio.argmax())]))
    return worst


# ---- 1. the forced matrix ----------------------------------------------------------------------------------------------------------------
# (mode, tile) -> (N, C, H, W, K, k, stride, pad, pad_mode, ks of the split case).  Ragged everywhere: M (output rows) not a multiple of
# BM, pixel counts not a multiple of BP, 1x1 / 3x3 / 4x4 / 5x5 filters, odd H / W under stride 2 (data-gradient phases of unequal pixel
# and K length: the split is sized by the smallest phase), and K splits whose last slice is empty (C = 16, 5x5: 25 stages, ks = 6 gives
# slices of 5 and a sixth starting at stage 25 -- the kernel's nst_here == 0 branch).  Every forced combination is legal for its shape:
# BM = 128 needs M > 64, ks <= stages / 4 of the smallest phase.
GEOM = {
    ('fwd_zero', 128128): (2, 16, 13, 13, 200, 5, 1, 2, 0, 6),      # empty last slice
    ('fwd_zero', 128064): (2, 128, 15, 9, 80, 1, 1, 0, 0, 2),
    ('fwd_zero', 64128): (2, 48, 13, 11, 80, 3, 2, 1, 0, 3),        # M = 80: a full and a 16-row tile
    ('fwd_zero', 64064): (3, 32, 11, 13, 40, 4, 2, 1, 0, 8),
    ('fwd_reflect', 128128): (2, 32, 12, 12, 80, 3, 1, 1, 1, 4),
    ('fwd_reflect', 128064): (2, 16, 9, 14, 136, 5, 1, 2, 1, 6),    # empty last slice, M = 128 + 8
    ('fwd_reflect', 64128): (2, 64, 11, 11, 64, 4, 2, 1, 1, 8),
    ('fwd_reflect', 64064): (3, 32, 7, 10, 48, 3, 1, 1, 1, 2),
    ('dgrad_s1', 128128): (2, 200, 13, 11, 32, 3, 1, 1, 0, 3),
    ('dgrad_s1', 128064): (2, 80, 12, 12, 16, 5, 1, 2, 0, 6),       # empty last slice
    ('dgrad_s1', 64128): (2, 48, 10, 13, 128, 1, 1, 0, 0, 2),
    ('dgrad_s1', 64064): (2, 40, 9, 9, 48, 4, 1, 1, 0, 8),
    ('dgrad_s2', 128128): (2, 80, 13, 11, 128, 3, 2, 1, 0, 2),      # phases of 1, 2, 2, 4 taps
    ('dgrad_s2', 128064): (2, 136, 11, 9, 64, 4, 2, 1, 0, 4),       # phases of 6 / 5 rows, 5 / 4 columns
    ('dgrad_s2', 64128): (2, 48, 13, 13, 32, 5, 2, 2, 0, 2),        # phases of 9, 6, 6, 4 taps
    ('dgrad_s2', 64064): (2, 40, 15, 9, 128, 3, 2, 1, 0, 2),
}
MATRIX = [(m, t, split) for (m, t) in GEOM for split in (False, True)]


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('mode,tile,split', MATRIX, ids=['%s-%d-%s' % (m, t, 'split' if s else 'whole') for m, t, s in MATRIX])
def test_forced_instantiation_against_float64(dev, force_hgemm, monkeypatch, mode, tile, split, dt):
    from pcgan_amd.hip import ops
    N, C, H, W, K, k, stride, pad, pm, ks_split = GEOM[(mode, tile)]
    ks = ks_split if split else 1
    fwd = mode.startswith('fwd')
    g = torch.Generator().manual_seed(tile + 7 * ks + len(mode))
    w = torch.randn(K, C, k, k, generator=g) * (2.0 / (C * k * k)) ** 0.5
    P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    tdt = torch.float32 if dt == 'fp32' else torch.bfloat16
    if fwd:
        src = torch.randn(N, C, H, W, generator=g).relu_()
        b = torch.randn(K, generator=g) * 0.1
        M, kp, nph = K, k * k * C, 1
    else:
        src = torch.randn(N, K, P, Q, generator=g)
        b = None
        M, kp, nph = C, k * k * K, _nphase(H, W, k, stride, pad)
    src = src.to(tdt).float()         # the bf16 cases: the reference sees the stored values
    wq = w if dt == 'fp32' else w.to(torch.bfloat16).float()
    force_hgemm(tile, ks)
    want = {'form': 'hgemm_f16x2' if dt == 'fp32' else 'hgemm_bf16', 'mode': 'dgrad' if not fwd else mode, 'bm': tile // 1000,
            'bp': tile % 1000, 'ks': ks, 'nphase': nph}
    route = ('fwd' if fwd else 'dgrad', 'hgemm' if dt == 'fp32' else 'packed')
    assert M % want['bm'] != 0 or (N * P * Q) % want['bp'] != 0, 'the case must be ragged'

    def call(act, dtype=tdt):
        if fwd:
            return _run(dev, 'fwd', src, w, b, stride, pad, pm, act=act, dtype=dtype)
        return _run(dev, 'dgrad', src, w, None, stride, pad, pm, in_hw=(H, W), dtype=dtype)

    if dt == 'bf16':
        if fwd:
            absref = _ref_fwd(src.abs(), wq.abs(), b.abs(), stride, pad, pm)
        else:
            absref = _ref_dgrad(src.abs(), wq.abs(), (H, W), stride, pad, pm)
    for act in (ACTS if fwd else (0,)):
        y, routes, rec = call(act)
        assert routes == {route: 1}, routes
        got = {kk: rec[kk] for kk in want}
        assert got == want, 'launched %r, forced %r' % (got, want)
        ref = _ref_fwd(src, wq, b, stride, pad, pm, act) if fwd else _ref_dgrad(src, wq, (H, W), stride, pad, pm)
        what = '%s tile %d ks %d act %d' % (mode, tile, ks, act)
        if dt == 'bf16':
            _check_bf16(y, ref, absref, kp, what)
            continue
        with monkeypatch.context() as mp:
            mp.setattr(ops, 'HSPLIT', False)
            mp.setattr(ops, 'BF16X6', False)
            y32, _, rec32 = call(act)
            assert rec32['form'] == 'igemm2_cg16' and rec32['ks'] == ks, rec32
        _check_fp32(y, y32, ref, what)


def test_forced_options_are_clamped_and_recorded(dev, force_hgemm):
    """the clamps the record exists for: a 128-row tile on <= 64 rows runs as 64 rows; a K split is cut to stages / 4; the data gradient
    of a 1x1 stride-2 convolution (pixels no phase writes, zeroed first) gets no split workspace -- and the results still hold"""
    g = torch.Generator().manual_seed(3)
    cases = [   # (mode, N, C, H, W, K, k, stride, pad, tile, ks) -> (bm, bp, ks)
        ('fwd', 2, 32, 9, 9, 48, 3, 1, 1, 128128, 2, (64, 128, 2)),
        ('fwd', 2, 16, 9, 9, 80, 3, 1, 1, 64064, 8, (64, 64, 2)),        # 9 stages: at most 2 slices
        ('dgrad', 2, 40, 15, 9, 128, 1, 2, 0, 64128, 4, (64, 128, 1)),
    ]
    for mode, N, C, H, W, K, k, stride, pad, tile, ks, want in cases:
        w = torch.randn(K, C, k, k, generator=g) * 0.1
        force_hgemm(tile, ks)
        if mode == 'fwd':
            x = torch.randn(N, C, H, W, generator=g)
            y, _, rec = _run(dev, 'fwd', x, w, None, stride, pad, 0)
            ref = _ref_fwd(x, w, None, stride, pad, 0)
        else:
            P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
            dy = torch.randn(N, K, P, Q, generator=g)
            y, _, rec = _run(dev, 'dgrad', dy, w, None, stride, pad, 0, in_hw=(H, W))
            ref = _ref_dgrad(dy, w, (H, W), stride, pad, 0)
        assert rec['form'] == 'hgemm_f16x2' and (rec['bm'], rec['bp'], rec['ks']) == want, (mode, tile, ks, rec)
        e, emax = _errs(y, ref)
        assert e < 3e-6 and emax <= 2e-5, (mode, tile, ks, e, emax)


# ---- 3. operand ranges on the heuristic tile -----------------------------------------------------------------------------------------------
RANGE_SHAPES = [   # (mode, N, C, H, W, K, k, stride, pad)
    ('fwd', 2, 64, 17, 15, 128, 3, 2, 1),
    ('fwd', 2, 48, 12, 12, 96, 3, 1, 1),
    ('dgrad', 2, 64, 17, 15, 128, 3, 2, 1),
    ('dgrad', 2, 96, 12, 12, 48, 4, 1, 1),
]


def _scaled(g, src, w, data):
    """operand families as in test_gpu_bf16x6.py::test_hsplit_forward_has_fp32_accuracy"""
    if data == 'relu_normal':
        return src.relu(), w
    if data == 'wide_range':          # magnitudes over twelve decades inside one tensor
        return (src * torch.pow(10.0, torch.rand(src.shape, generator=g) * 12 - 9),
                w * torch.pow(10.0, torch.rand(w.shape, generator=g) * 6 - 3))
    if data == 'tiny':
        return src * 1e-30, w * 1e-6
    return src * 1e12, w * 1e8


@pytest.mark.parametrize('shape', RANGE_SHAPES, ids=['%s-%dx%d-s%d' % (s[0], s[6], s[6], s[7]) for s in RANGE_SHAPES])
@pytest.mark.parametrize('data', ['relu_normal', 'wide_range', 'tiny', 'huge'])
def test_operand_ranges_on_the_heuristic_tile(dev, monkeypatch, shape, data):
    from pcgan_amd.hip import ops
    mode, N, C, H, W, K, k, stride, pad = shape
    g = torch.Generator().manual_seed(N + C + K + k)
    P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    w = torch.randn(K, C, k, k, generator=g) * 0.05
    src = torch.randn(*((N, C, H, W) if mode == 'fwd' else (N, K, P, Q)), generator=g)
    src, w = _scaled(g, src, w, data)
    in_hw = None if mode == 'fwd' else (H, W)
    y, routes, rec = _run(dev, mode, src, w, None, stride, pad, 0, in_hw=in_hw)
    assert routes == {(mode, 'hgemm'): 1} and rec['form'] == 'hgemm_f16x2', (routes, rec)
    ref = _ref_fwd(src, w, None, stride, pad, 0) if mode == 'fwd' else _ref_dgrad(src, w, (H, W), stride, pad, 0)
    monkeypatch.setattr(ops, 'HSPLIT', False)
    monkeypatch.setattr(ops, 'BF16X6', False)
    y32 = _run(dev, mode, src, w, None, stride, pad, 0, in_hw=in_hw)[0]
    _check_fp32(y, y32, ref, '%s %s' % (mode, data))


@pytest.mark.parametrize('mode', ['fwd', 'dgrad'])
def test_attached_operand_maxima_match_the_absmax_pass(dev, mode):
    """a producer's per-plane maxima (_attach_amax, N * C partial slots) and one pcgan_absmax pass give the same power-of-two operand
    scale: bit-identical results"""
    from pcgan_amd.hip import ops
    g = torch.Generator().manual_seed(11)
    N, C, H, K = 3, 64, 14, 96
    w = (torch.randn(K, C, 3, 3, generator=g) * 0.05).to(dev)
    src = torch.randn(N, C if mode == 'fwd' else K, H, H, generator=g).to(dev)
    src = src * torch.pow(10.0, torch.rand(src.shape, generator=g) * 6 - 3).to(dev)

    def call(t):
        if mode == 'fwd':
            return ops.conv2d_fwd(t, w, None, 1, 1, 0, pack_cache={})
        return ops.conv2d_bwd_data(t, w, (H, H), 1, 1, 0, pack_cache={})
    a0 = dict(ops.AMAX_STATS)
    plain = call(src.clone())
    assert ops.AMAX_STATS['computed'] == a0['computed'] + 1
    x = src.clone()
    ops._attach_amax(x, x.abs().amax(dim=(2, 3)).reshape(-1).contiguous())
    a1 = dict(ops.AMAX_STATS)
    attached = call(x)
    assert ops.AMAX_STATS['attached'] == a1['attached'] + 1 and ops.AMAX_STATS['computed'] == a1['computed']
    assert ops.igemm_last_launch()['form'] == 'hgemm_f16x2'
    assert torch.equal(plain, attached)


# ---- 4. the production layers at batch 32 -------------------------------------------------------------------------------------------------
# config 2 (bench.py defaults): every forward / data gradient on hgemm_kernel, with the heuristic's launch (BM, BP, ks, phases) pinned --
# a changed heuristic shows up here in review.  The generator's up-convolutions are the data gradients (forward) and forwards (backward)
# of G.down2 / G.down1's descriptors, so those rows cover them.  name: (N, C, H, W, K, k, stride, pad) -> (fwd launch, dgrad launch)
PRODUCTION = {
    'G.down1 / up2': ((32, 64, 128, 128, 128, 3, 2, 1), ((128, 128, 1, 1), (64, 128, 1, 4))),
    'G.down2 / up1': ((32, 128, 64, 64, 256, 3, 2, 1), ((128, 128, 1, 1), (128, 128, 1, 4))),
    'D.c1': ((32, 64, 64, 64, 128, 4, 2, 1), ((128, 64, 1, 1), (64, 128, 1, 4))),
    'D.c2': ((32, 128, 32, 32, 256, 4, 2, 1), ((128, 128, 4, 1), (128, 64, 1, 4))),
    'D.c3': ((32, 256, 16, 16, 512, 4, 1, 1), ((128, 64, 1, 1), (128, 128, 4, 1))),
    'E.layer1': ((32, 64, 56, 56, 64, 3, 1, 1), ((64, 128, 1, 1), (64, 128, 1, 1))),
    'E.layer2.0': ((32, 64, 56, 56, 128, 3, 2, 1), ((128, 64, 1, 1), (64, 128, 1, 4))),
    'E.layer2.ds': ((32, 64, 56, 56, 128, 1, 2, 0), ((128, 64, 1, 1), (64, 64, 1, 1))),
    'E.layer2': ((32, 128, 28, 28, 128, 3, 1, 1), ((128, 64, 1, 1), (128, 64, 1, 1))),
    'E.layer3.0': ((32, 128, 28, 28, 256, 3, 2, 1), ((128, 128, 5, 1), (128, 64, 1, 4))),
    'E.layer3.ds': ((32, 128, 28, 28, 256, 1, 2, 0), ((64, 64, 1, 1), (64, 64, 1, 1))),
    'E.layer3': ((32, 256, 14, 14, 256, 3, 1, 1), ((128, 128, 5, 1), (128, 128, 5, 1))),
    'E.layer4.0': ((32, 256, 14, 14, 512, 3, 2, 1), ((128, 128, 8, 1), (128, 128, 4, 4))),
    'E.layer4.ds': ((32, 256, 14, 14, 512, 1, 2, 0), ((64, 64, 1, 1), (64, 64, 1, 1))),
    'E.layer4': ((32, 512, 7, 7, 512, 3, 1, 1), ((128, 128, 8, 1), (128, 128, 8, 1))),
}


@pytest.mark.parametrize('name', list(PRODUCTION))
def test_production_layer_at_batch_32(dev, monkeypatch, name):
    from pcgan_amd.hip import ops
    (N, C, H, W, K, k, stride, pad), (want_f, want_d) = PRODUCTION[name]
    P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    g = torch.Generator(device=dev).manual_seed(len(name))
    w = torch.randn(K, C, k, k, device=dev, generator=g) * (2.0 / (C * k * k)) ** 0.5
    x = torch.randn(N, C, H, W, device=dev, generator=g).relu_()
    dy = torch.randn(N, K, P, Q, device=dev, generator=g)
    wc = w.cpu()
    got = {}
    for mode, src, want in (('fwd', x, want_f), ('dgrad', dy, want_d)):
        in_hw = None if mode == 'fwd' else (H, W)
        r0 = dict(ops.ROUTE_STATS)
        cache = {}
        if mode == 'fwd':
            y = ops.conv2d_fwd(src, w, None, stride, pad, 0, pack_cache=cache)
        else:
            y = ops.conv2d_bwd_data(src, w, in_hw, stride, pad, 0, pack_cache=cache)
        rec = ops.igemm_last_launch()
        assert ops.ROUTE_STATS.get((mode, 'hgemm'), 0) == r0.get((mode, 'hgemm'), 0) + 1, (name, mode, ops.ROUTE_STATS)
        assert rec['form'] == 'hgemm_f16x2' and rec['mode'] == ('fwd_zero' if mode == 'fwd' else 'dgrad'), rec
        got[mode] = (rec['bm'], rec['bp'], rec['ks'], rec['nphase'])
        s0 = src[:1].cpu()
        ref = _ref_fwd(s0, wc, None, stride, pad, 0) if mode == 'fwd' else _ref_dgrad(s0, wc, (H, W), stride, pad, 0)
        with monkeypatch.context() as mp:
            mp.setattr(ops, 'HSPLIT', False)
            mp.setattr(ops, 'BF16X6', False)
            if mode == 'fwd':
                y32 = ops.conv2d_fwd(src, w, None, stride, pad, 0, pack_cache={})
            else:
                y32 = ops.conv2d_bwd_data(src, w, in_hw, stride, pad, 0, pack_cache={})
        assert y.shape[0] == N
        _check_fp32(y[:1].double().cpu(), y32[:1].double().cpu(), ref, '%s %s' % (name, mode))
        del y, y32
    assert (got['fwd'], got['dgrad']) == (want_f, want_d), '%s: heuristic launches (BM, BP, ks, phases) %r, pinned %r' % (
        name, (got['fwd'], got['dgrad']), (want_f, want_d))
