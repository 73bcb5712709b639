"""GPU: every packed-weight form of hip/ops.py (_PACK_FORMS, one record per cache pass) against the library's `*_packed_bytes` / `*_pack`
entry points called directly -- the calls are written out here, not read from the table, so a record that names the wrong query or
pack call packs different bytes.  Byte-exact: both sides run the same pack kernel on the same weights.

Shapes: the smallest each form's `*_supported` query accepts -- one image; the window kernels of the fp16 two-piece route need a
32-wide plane and 256 rows, the per-tap bf16 split 128 channels, hgemm > 32 rows and a multiple of 16 gathered channels (48 -> 64: the
two passes then have different row counts), thin <= 4 gathered channels and a multiple of 64 rows, the fp32 form anything (odd counts).
"""
import ctypes

import pytest
import torch

from pcgan_amd.hip import ops, lib as L

pytestmark = pytest.mark.gpu

_p = ops._p
RES256 = (1, 256, 4, 32, 256, 3, 3, 1, 1, 1)
RES128 = (1, 128, 16, 16, 128, 3, 3, 1, 1, 1)
HG = (1, 48, 16, 16, 64, 3, 3, 1, 1, 0)
ODD = (1, 5, 16, 16, 7, 3, 3, 1, 1, 0)

# cache pass -> (N, C, H, W, K, R, S, stride, pad, pad_mode), supported(lib, d), bytes(lib, d), pack(lib, d, w, buf, rowmax, s), rowmax rows
CASES = {
    'fwd': (lambda: L.PASS_FWD, ODD, lambda lib, d: True,
            lambda lib, d: lib.pcgan_conv2d_packed_bytes(d, L.PASS_FWD),
            lambda lib, d, w, buf, rm, s: lib.pcgan_conv2d_pack_weights(d, L.PASS_FWD, w, buf, s), None),
    'dgrad': (lambda: L.PASS_BWD_DATA, ODD, lambda lib, d: True,
              lambda lib, d: lib.pcgan_conv2d_packed_bytes(d, L.PASS_BWD_DATA),
              lambda lib, d, w, buf, rm, s: lib.pcgan_conv2d_pack_weights(d, L.PASS_BWD_DATA, w, buf, s), None),
    'fwd_bsplit': (lambda: ops.PASS_FWD_BSPLIT, RES128, lambda lib, d: lib.pcgan_conv2d_bsplit_supported(d),
                   lambda lib, d: lib.pcgan_conv2d_bsplit_packed_bytes(d),
                   lambda lib, d, w, buf, rm, s: lib.pcgan_conv2d_bsplit_pack(d, w, buf, s), None),
    'dgrad_bsplit': (lambda: ops.PASS_BWD_BSPLIT, RES128, lambda lib, d: lib.pcgan_conv2d_bsplit_dgrad_supported(d),
                     lambda lib, d: lib.pcgan_conv2d_bsplit_dgrad_packed_bytes(d),
                     lambda lib, d, w, buf, rm, s: lib.pcgan_conv2d_bsplit_dgrad_pack(d, w, buf, s), None),
    'fwd_hsplit': (lambda: ops.PASS_FWD_HSPLIT, RES256, lambda lib, d: lib.pcgan_conv2d_hsplit_supported(d, L.PASS_FWD),
                   lambda lib, d: lib.pcgan_conv2d_hsplit_packed_bytes(d, L.PASS_FWD),
                   lambda lib, d, w, buf, rm, s: lib.pcgan_conv2d_hsplit_pack(d, L.PASS_FWD, w, buf, s), None),
    'dgrad_hsplit': (lambda: ops.PASS_BWD_HSPLIT, RES256, lambda lib, d: lib.pcgan_conv2d_hsplit_supported(d, L.PASS_BWD_DATA),
                     lambda lib, d: lib.pcgan_conv2d_hsplit_packed_bytes(d, L.PASS_BWD_DATA),
                     lambda lib, d, w, buf, rm, s: lib.pcgan_conv2d_hsplit_pack(d, L.PASS_BWD_DATA, w, buf, s), None),
    'fwd_hgemm': (lambda: ops.PASS_FWD_HGEMM, HG, lambda lib, d: lib.pcgan_conv2d_hgemm_supported(d, L.PASS_FWD),
                  lambda lib, d: lib.pcgan_conv2d_packed_bytes(d, L.PASS_FWD),
                  lambda lib, d, w, buf, rm, s: lib.pcgan_conv2d_hgemm_pack(d, L.PASS_FWD, w, rm, buf, s), 64),
    'dgrad_hgemm': (lambda: ops.PASS_BWD_HGEMM, HG, lambda lib, d: lib.pcgan_conv2d_hgemm_supported(d, L.PASS_BWD_DATA),
                    lambda lib, d: lib.pcgan_conv2d_packed_bytes(d, L.PASS_BWD_DATA),
                    lambda lib, d, w, buf, rm, s: lib.pcgan_conv2d_hgemm_pack(d, L.PASS_BWD_DATA, w, rm, buf, s), 48),
    'fwd_thin': (lambda: ops.PASS_FWD_THIN, (1, 3, 16, 16, 64, 7, 7, 1, 3, 1), lambda lib, d: lib.pcgan_conv2d_thin_supported(d, L.PASS_FWD),
                 lambda lib, d: lib.pcgan_conv2d_thin_packed_bytes(d, L.PASS_FWD),
                 lambda lib, d, w, buf, rm, s: lib.pcgan_conv2d_thin_pack(d, L.PASS_FWD, w, buf, s), None),
    'dgrad_thin': (lambda: ops.PASS_BWD_THIN, (1, 64, 16, 16, 3, 7, 7, 1, 3, 1), lambda lib, d: lib.pcgan_conv2d_thin_supported(d, L.PASS_BWD_DATA),
                   lambda lib, d: lib.pcgan_conv2d_thin_packed_bytes(d, L.PASS_BWD_DATA),
                   lambda lib, d, w, buf, rm, s: lib.pcgan_conv2d_thin_pack(d, L.PASS_BWD_DATA, w, buf, s), None),
}


def _direct_pack(lib, d, w, nbytes, pack, rows):
    """the library's pack call into zeroed buffers of this test's own"""
    buf = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=w.device)
    rowmax = torch.zeros(rows, dtype=torch.float32, device=w.device) if rows else None
    L.check(pack(lib, ctypes.byref(d), _p(w), _p(buf), _p(rowmax), ops._stream()), 'direct pack')
    return buf, rowmax


def _weight(shape, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape[4], shape[1], shape[5], shape[6], generator=g) * 0.1).to(dev)


def test_every_pack_form_has_a_case():
    assert sorted(ops._PACK_FORMS) == sorted(c[0]() for c in CASES.values())


@pytest.mark.parametrize('name', list(CASES))
def test_packed_weights_equal_the_direct_pack_call(dev, name):
    pass_, shape, supported, nbytes, pack, rows = CASES[name]
    pass_ = pass_()
    lib = L.load()
    d = ops.make_desc(*shape)
    assert supported(lib, ctypes.byref(d)), 'the case must be a shape the form supports'
    nb = int(nbytes(lib, ctypes.byref(d)))
    assert nb > 0
    w = _weight(shape, dev, 11)
    cache = {}
    pk, rowmax = ops._packed_weights(lib, d, pass_, w, cache, True)
    assert list(cache) == [(pass_, d.stride, d.pad, d.pad_mode, d.dtype)] and pk.numel() == max(nb, 256)
    # bytes a pack leaves alone are whatever the allocator handed out: pack once more, into the same buffer, over zeros
    pk.zero_()
    ops.invalidate_packed_weights()
    pk2, rowmax2 = ops._packed_weights(lib, d, pass_, w, cache, True)
    assert pk2 is pk and pk2 is ops._packed_weights(lib, d, pass_, w, cache)
    want, want_rowmax = _direct_pack(lib, d, w, nb, pack, rows)
    assert torch.equal(pk2, want)
    assert bool(want.any())
    if rows:
        assert rowmax2 is rowmax and rowmax2.shape == (rows,) and torch.equal(rowmax2, want_rowmax)
    else:
        assert rowmax is None and rowmax2 is None


def test_a_rewritten_weight_is_packed_again_into_the_same_buffer(dev):
    pass_, shape, _, nbytes, pack, rows = CASES['fwd_hgemm']
    pass_ = pass_()
    lib = L.load()
    d = ops.make_desc(*shape)
    w = _weight(shape, dev, 12)
    cache = {}
    pk, rowmax = ops._packed_weights(lib, d, pass_, w, cache, True)
    stamp = cache[(pass_, d.stride, d.pad, d.pad_mode, d.dtype)][0]
    old, old_rowmax = pk.clone(), rowmax.clone()
    pk.zero_()            # (as above: compare over zeros)
    w.mul_(-1.5)          # through an op: the tensor version, and with it the stamp, moves on
    pk2, rowmax2 = ops._packed_weights(lib, d, pass_, w, cache, True)
    assert pk2 is pk and rowmax2 is rowmax and cache[(pass_, d.stride, d.pad, d.pad_mode, d.dtype)][0] != stamp
    want, want_rowmax = _direct_pack(lib, d, w, int(nbytes(lib, ctypes.byref(d))), pack, rows)
    assert torch.equal(pk2, want) and torch.equal(rowmax2, want_rowmax)
    assert not torch.equal(pk2, old) and not torch.equal(rowmax2, old_rowmax)
