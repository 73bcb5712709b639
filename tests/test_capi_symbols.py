"""CPU: the C-ABI library loads and exports every symbol include/pcgan_hip.h declares, and the
ctypes signature table covers exactly that set (no compute calls: there is no GPU here)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, 'include', 'pcgan_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(pcgan_[a-z0-9_]+)\s*\(', text)))


def test_header_declares_the_expected_families():
    names = _declared()
    for must in ('pcgan_conv2d_fwd', 'pcgan_conv2d_bwd_data', 'pcgan_conv2d_bwd_weight', 'pcgan_norm_act_fwd',
                 'pcgan_bce_loss', 'pcgan_adam_step', 'pcgan_bilinear_fwd', 'pcgan_maxpool_fwd'):
        assert must in names
    assert len(names) >= 30


def test_library_exports_every_declared_symbol():
    from pcgan_amd.hip import lib
    handle = lib.load()
    for name in _declared():
        assert hasattr(handle, name), 'libpcgan_hip.so does not export %s' % name


def test_ctypes_table_matches_header():
    from pcgan_amd.hip import lib
    assert sorted(lib.SIGNATURES) == _declared()


def test_version_and_error_channel():
    from pcgan_amd.hip import lib
    handle = lib.load()
    assert handle.pcgan_version() >= 100
    assert handle.pcgan_last_error() is not None
    # argument validation happens before any launch, so it can be exercised without a GPU
    import ctypes
    d = lib.ConvDesc(1, 3, 8, 8, 4, 3, 3, 3, 1, 0, 8, 8)     # stride 3 is unsupported
    st = handle.pcgan_conv2d_fwd(ctypes.byref(d), None, None, None, None, 0, 0.0, None, 0, None)
    assert st != 0 and b'stride' in handle.pcgan_last_error()
    d = lib.ConvDesc(1, 3, 8, 8, 4, 3, 3, 1, 1, 0, 7, 7)     # wrong output size
    st = handle.pcgan_conv2d_fwd(ctypes.byref(d), None, None, None, None, 0, 0.0, None, 0, None)
    assert st != 0 and b'output dims' in handle.pcgan_last_error()
    assert handle.pcgan_conv2d_workspace_bytes(ctypes.byref(lib.ConvDesc(2, 4, 8, 8, 8, 3, 3, 1, 1, 0, 8, 8)), 0) >= 8 * 9 * 4 * 4


def test_weight_gradient_route_predicates():
    """host-side predicates of the matrix-pipe weight gradient (no launch): which shapes the route takes, which of them need no
    padded copy of x, and that the workspace of those holds whole split partials only (reference layers: models/networks.py:584-648,
    753-775)"""
    import ctypes
    from pcgan_amd.hip import lib
    h = lib.load()

    def desc(N, C, H, W, K, k, stride, pad, mode, dt):
        P, Q = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        d = lib.ConvDesc(N, C, H, W, K, k, k, stride, pad, mode, P, Q)
        d.dtype = dt
        return d

    for dt in (lib.F32, lib.BF16):
        # PatchGAN 256 -> 512, 4x4 stride 1 pad 1 at 16 x 16: output 15 x 15 (ragged stage), two row tiles, padding in the gather
        d = desc(32, 256, 16, 16, 512, 4, 1, 1, 0, dt)
        assert h.pcgan_conv2d_hsplit_wgrad_supported(ctypes.byref(d)) == 1 and h.pcgan_conv2d_hsplit_wgrad_inline(ctypes.byref(d)) == 1
        ws = h.pcgan_conv2d_hsplit_wgrad_workspace_bytes(ctypes.byref(d))
        assert ws > 0 and ws % (512 * 256 * 16 * 4) == 0
        # the residual block's convolution: reflection applied in the gather
        d = desc(32, 256, 32, 32, 256, 3, 1, 1, 1, dt)
        assert h.pcgan_conv2d_hsplit_wgrad_supported(ctypes.byref(d)) == 1 and h.pcgan_conv2d_hsplit_wgrad_inline(ctypes.byref(d)) == 1
        # the generator's first down-sampling layer (134 MB input with fp32 tensors): no padded copy
        d = desc(32, 64, 128, 128, 128, 3, 2, 1, 0, dt)
        assert h.pcgan_conv2d_hsplit_wgrad_inline(ctypes.byref(d)) == 1
        # 7 x 7 maps: less than three quarters of a 16-column stage would be real columns
        d = desc(32, 512, 7, 7, 512, 3, 1, 1, 0, dt)
        assert h.pcgan_conv2d_hsplit_wgrad_supported(ctypes.byref(d)) == 0 and h.pcgan_conv2d_hsplit_wgrad_inline(ctypes.byref(d)) == 0
        # the generator's stem: reflection padding 3 keeps the padded copy
        d = desc(32, 4, 128, 128, 64, 7, 1, 3, 1, dt)
        assert h.pcgan_conv2d_hsplit_wgrad_supported(ctypes.byref(d)) == 1 and h.pcgan_conv2d_hsplit_wgrad_inline(ctypes.byref(d)) == 0
        # zero padding 2 (AlexNet's 5 x 5 layer): padded copy, so whole stages and at most 256 rows only
        d = desc(32, 64, 27, 27, 192, 5, 1, 2, 0, dt)
        assert h.pcgan_conv2d_hsplit_wgrad_supported(ctypes.byref(d)) == 0
        # fewer than 32 output channels / stride 4: other kernels
        assert h.pcgan_conv2d_hsplit_wgrad_supported(ctypes.byref(desc(32, 512, 15, 15, 1, 4, 1, 1, 0, dt))) == 0
        assert h.pcgan_conv2d_hsplit_wgrad_supported(ctypes.byref(desc(32, 3, 224, 224, 64, 11, 4, 2, 0, dt))) == 0


def test_library_reads_no_environment_and_options_are_explicit():
    """round 4: no getenv in the library's sources; the routing options are an explicit, validated table"""
    import glob
    from pcgan_amd.hip import lib
    for src in glob.glob(os.path.join(ROOT, 'pc-gan_amd', 'csrc', '*')):
        assert 'getenv' not in open(src).read(), src
    h = lib.load()
    for key, default in (('bsplit_halo', 1), ('wgrad_gen', 1), ('wgrad_padcopy', 0), ('wgrad_cw', 0), ('hgemm_bf16', 1), ('wgrad_direct', 0),
                         ('hgemm_tile', 0), ('hgemm_ks', 0), ('wgrad_rowring', 1), ('wgrad_ks', 0), ('hwgrad_ks', 0)):
        if not any(os.environ.get(e) for e, k, _ in lib._ENV_OPTIONS if k == key):
            assert lib.get_option(key) == default, key
    lib.set_option('wgrad_cw', 256)
    assert lib.get_option('wgrad_cw') == 256
    lib.set_option('wgrad_cw', 0)
    assert h.pcgan_set_option(b'no_such_option', 1) != 0 and b'unknown option' in h.pcgan_last_error()
    assert h.pcgan_set_option(b'wgrad_cw', 77) != 0
    assert h.pcgan_set_option(b'hgemm_tile', 96096) != 0 and h.pcgan_set_option(b'hgemm_ks', 9) != 0
    assert h.pcgan_set_option(b'wgrad_ks', 513) != 0 and b'wgrad_ks' in h.pcgan_last_error() and h.pcgan_set_option(b'wgrad_ks', -1) != 0
    assert lib.get_option('wgrad_ks') == 0 and not any(k == 'wgrad_ks' for _, k, _ in lib._ENV_OPTIONS)
    assert h.pcgan_set_option(b'hwgrad_ks', 513) != 0 and b'hwgrad_ks' in h.pcgan_last_error() and h.pcgan_set_option(b'hwgrad_ks', -1) != 0
    assert lib.get_option('hwgrad_ks') == 0 and not any(k == 'hwgrad_ks' for _, k, _ in lib._ENV_OPTIONS)


def test_igemm_launch_record_query():
    """pcgan_igemm_last_launch reads host memory only (callable without a GPU): entries past the record are 0, a null output is refused"""
    import ctypes
    from pcgan_amd.hip import lib
    h = lib.load()
    buf = (ctypes.c_int * 9)(*([-1] * 9))
    assert h.pcgan_igemm_last_launch(buf, 9) == 0 and list(buf)[7:] == [0, 0] and min(buf) >= 0
    assert h.pcgan_igemm_last_launch(None, 7) != 0 and b'igemm_last_launch' in h.pcgan_last_error()


def test_wgrad_launch_record_query():
    """pcgan_wgrad_last_launch reads host memory only (callable without a GPU): entries past the record are 0, a null output is refused,
    and it is a record of its own -- the query leaves the implicit GEMM's where it was"""
    import ctypes
    from pcgan_amd.hip import lib, ops
    h = lib.load()
    ig = (ctypes.c_int * 7)()
    assert h.pcgan_igemm_last_launch(ig, 7) == 0
    buf = (ctypes.c_int * 11)(*([-1] * 11))
    assert h.pcgan_wgrad_last_launch(buf, 11) == 0 and list(buf)[9:] == [0, 0] and min(buf) >= 0
    assert h.pcgan_wgrad_last_launch(None, 9) != 0 and b'wgrad_last_launch' in h.pcgan_last_error()
    assert h.pcgan_wgrad_last_launch(buf, 0) != 0
    rec = ops.wgrad_last_launch()
    assert sorted(rec) == ['bm', 'dtype', 'family', 'mode', 'seq', 'splits', 'units', 'variant', 'veca'] and rec['seq'] == buf[0]
    ig2 = (ctypes.c_int * 7)()
    assert h.pcgan_igemm_last_launch(ig2, 7) == 0 and list(ig2) == list(ig)


def test_hwgrad_launch_record_query():
    """pcgan_hwgrad_last_launch reads host memory only (callable without a GPU): entries past the record are 0, a null output and n <= 0
    are refused, and it is a record of its own -- the query leaves the other two where they were"""
    import ctypes
    from pcgan_amd.hip import lib, ops
    h = lib.load()
    ig, wg = (ctypes.c_int * 7)(), (ctypes.c_int * 9)()
    assert h.pcgan_igemm_last_launch(ig, 7) == 0 and h.pcgan_wgrad_last_launch(wg, 9) == 0
    buf = (ctypes.c_int * 14)(*([-1] * 14))
    assert h.pcgan_hwgrad_last_launch(buf, 14) == 0 and list(buf)[12:] == [0, 0] and min(buf) >= 0
    short = (ctypes.c_int * 3)(*([-1] * 3))
    assert h.pcgan_hwgrad_last_launch(short, 2) == 0 and list(short)[:2] == list(buf)[:2] and short[2] == -1
    assert h.pcgan_hwgrad_last_launch(None, 12) != 0 and b'hwgrad_last_launch' in h.pcgan_last_error()
    assert h.pcgan_hwgrad_last_launch(buf, 0) != 0 and h.pcgan_hwgrad_last_launch(buf, -1) != 0
    rec = ops.hwgrad_last_launch()
    assert tuple(rec) == ops.HWGRAD_FIELDS and len(rec) == 12 and rec['seq'] == buf[0]
    ig2, wg2 = (ctypes.c_int * 7)(), (ctypes.c_int * 9)()
    assert h.pcgan_igemm_last_launch(ig2, 7) == 0 and h.pcgan_wgrad_last_launch(wg2, 9) == 0
    assert list(ig2) == list(ig) and list(wg2) == list(wg)


def test_bsplit_launch_record_query():
    """pcgan_bsplit_last_launch reads host memory only (callable without a GPU): entries past the record are 0, a null output and n <= 0
    are refused, and it is a record of its own -- the query leaves the other three where they were"""
    import ctypes
    from pcgan_amd.hip import lib, ops
    h = lib.load()
    ig, wg, hw = (ctypes.c_int * 7)(), (ctypes.c_int * 9)(), (ctypes.c_int * 12)()
    assert h.pcgan_igemm_last_launch(ig, 7) == 0 and h.pcgan_wgrad_last_launch(wg, 9) == 0 and h.pcgan_hwgrad_last_launch(hw, 12) == 0
    buf = (ctypes.c_int * 13)(*([-1] * 13))
    assert h.pcgan_bsplit_last_launch(buf, 13) == 0 and list(buf)[11:] == [0, 0] and min(buf) >= 0
    short = (ctypes.c_int * 3)(*([-1] * 3))
    assert h.pcgan_bsplit_last_launch(short, 2) == 0 and list(short)[:2] == list(buf)[:2] and short[2] == -1
    assert h.pcgan_bsplit_last_launch(None, 11) != 0 and b'bsplit_last_launch' in h.pcgan_last_error()
    assert h.pcgan_bsplit_last_launch(buf, 0) != 0 and h.pcgan_bsplit_last_launch(buf, -1) != 0
    rec = ops.bsplit_last_launch()
    assert tuple(rec) == ops.BSPLIT_FIELDS and len(rec) == 11 and rec['seq'] == buf[0]
    ig2, wg2, hw2 = (ctypes.c_int * 7)(), (ctypes.c_int * 9)(), (ctypes.c_int * 12)()
    assert h.pcgan_igemm_last_launch(ig2, 7) == 0 and h.pcgan_wgrad_last_launch(wg2, 9) == 0 and h.pcgan_hwgrad_last_launch(hw2, 12) == 0
    assert list(ig2) == list(ig) and list(wg2) == list(wg) and list(hw2) == list(hw)


def test_forced_hwgrad_splits_size_the_workspace():
    """option "hwgrad_ks" (host arithmetic only): pcgan_conv2d_hsplit_wgrad_workspace_bytes holds exactly the forced number of partial
    sums, cut to the number of 16-column stages, behind the padded copy where there is one; 0 gives the heuristic's size back"""
    import ctypes
    from pcgan_amd.hip import lib
    h = lib.load()

    def nbytes(d):
        return int(h.pcgan_conv2d_hsplit_wgrad_workspace_bytes(ctypes.byref(d)))

    def up(v):
        return (v + 255) // 256 * 256
    gen = lib.ConvDesc(1, 8, 7, 16, 32, 3, 3, 1, 1, 0, 7, 16)          # zero padding in the gather: 7 stages, no padded copy
    copy = lib.ConvDesc(1, 8, 7, 16, 32, 5, 5, 1, 2, 0, 7, 16)         # zero padding 2: 7 stages behind a copy of 8 planes of 11 x 20
    before = [nbytes(d) for d in (gen, copy)]
    assert before == [32 * 72 * 4, up(8 * 11 * 20 * 4) + 32 * 200 * 4]      # (7 stages: under the 8-stage floor, one split)
    try:
        for ks, splits in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 4), (7, 7), (100, 7), (512, 7)):      # (5 over 7: 2 stages per split -> 4)
            lib.set_option('hwgrad_ks', ks)
            assert nbytes(gen) == splits * 32 * 72 * 4, ks
            assert nbytes(copy) == up(8 * 11 * 20 * 4) + splits * 32 * 200 * 4, ks
    finally:
        lib.set_option('hwgrad_ks', 0)
    assert [nbytes(d) for d in (gen, copy)] == before


def test_forced_wgrad_splits_size_the_workspace():
    """option "wgrad_ks" (host arithmetic only): the workspace query holds exactly the forced number of partial sums, cut to the number
    of 32-pixel chunks (strips), for the tile, small-M and strip families; 0 gives the heuristic's size back"""
    import ctypes
    from pcgan_amd.hip import lib
    h = lib.load()

    def nbytes(d):
        return int(h.pcgan_conv2d_workspace_bytes(ctypes.byref(d), lib.PASS_BWD_WEIGHT))

    def up(v):
        return (v + 255) // 256 * 256
    tile = lib.ConvDesc(1, 24, 10, 20, 8, 3, 3, 1, 1, 0, 10, 20)        # 200 pixels: 7 chunks; Kp = 9 * 24
    smallm = lib.ConvDesc(1, 16, 10, 20, 2, 1, 1, 1, 0, 0, 10, 20)      # 7 chunks; Kp = 16
    strip = lib.ConvDesc(2, 16, 19, 13, 3, 3, 3, 1, 1, 0, 19, 13)       # 2 * 3 * 13 = 78 strips; Kp = 9 * 16
    before = [nbytes(d) for d in (tile, smallm, strip)]
    try:
        for ks, units in ((1, (1, 1, 1)), (3, (3, 3, 3)), (4, (4, 4, 4)), (5, (4, 4, 5)), (7, (7, 7, 7)), (100, (7, 7, 78)), (512, (7, 7, 78))):
            lib.set_option('wgrad_ks', ks)      # (5 over 7 chunks: 2 chunks per split -> 4 splits; 5 over 78 strips: 16 per split -> 5)
            assert nbytes(tile) == up(units[0] * 8 * 9 * 24 * 4), ks
            assert nbytes(smallm) == up(units[1] * 2 * 16 * 4), ks
            assert nbytes(strip) == up(units[2] * 3 * 9 * 16 * 4), ks
    finally:
        lib.set_option('wgrad_ks', 0)
    assert [nbytes(d) for d in (tile, smallm, strip)] == before
