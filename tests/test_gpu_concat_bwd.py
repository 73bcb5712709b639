"""pcgan_concat_z_bwd (csrc/concat_bwd.hip), the one-launch backward pass of the rating join, against float64 numpy, and the autograd
function built on it (hip.functional._ConcatZFusedFn inside fused_concat_bwd()) against the default function and against float64 torch
twins of the three networks that join a rating to an image.

The bound on dz.  Inputs are taken as stored (bf16 values are widened exactly), every addition is an fp32 addition, so
|dz - exact| <= d * 2^-24 * sum |dy| over the plane(s), d = the longest chain of additions an element passes through in the kernel as
written (chain_length below mirrors it):
    log2(V)               inside one 16-byte access of V = 4 (fp32) / 8 (bf16) elements, a balanced tree; V = 1 in the element form
  + ceil(accesses / 256)  the lane's partial sum, one addition per access it owns (accesses = HW / V); the first is 0 + x, exact
  + 6                     the wave64 butterfly
  + 4                     the four wave results in wave order, starting from 0 (exact again)
  + N - 1                 with a shared rating: the plane sums in ascending n, for the sum over all N planes.
Two of the counted additions are exact, which covers the second-order terms of (1 + 2^-24)^d - 1.  The largest d here is 27 (63 x 67
planes, element form: 17 + 6 + 4), + 2 shared; the 16-byte form of 64 x 66 has 2 + 5 + 6 + 4 = 17 (fp32), 3 + 3 + 6 + 4 = 16 (bf16)."""
import copy
import math

import numpy as np
import pytest
import torch

from oracle import networks_ref as N
from oracle import weights as W
from test_gpu_nets import _assert_mostly_close, _run, record_decisions
from test_gpu_unet import record_unet_decisions
from unet_ref import UnetGeneratorRef
from util_cmp import assert_close

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 1, 1, 1), (2, 3, 1, 5, 7), (3, 1, 2, 8, 8), (2, 3, 5, 4, 4), (2, 3, 1, 63, 67), (1, 3, 2, 64, 66)]
PAD = 64                    # canary elements on either side of an output (a multiple of 16 bytes in every type used)
U = 2.0 ** -24


def chain_length(HW, esize, wide):
    V = 16 // esize if wide else 1
    return int(math.log2(V)) + -(-(HW // V) // 256) + 6 + 4


def _wide(HW, esize, *ptrs):
    return (HW * esize) % 16 == 0 and all(p % 16 == 0 for p in ptrs)


class Guarded(object):
    """an output buffer with PAD canary elements on either side, the whole of it filled with the canary"""

    def __init__(self, numel, dtype, dev, canary):
        self.buf = torch.full((numel + 2 * PAD,), canary, dtype=dtype, device=dev)
        self.before = self.buf.clone()
        self.body = self.buf[PAD:PAD + numel]

    def pads_intact(self):
        n = self.buf.numel()
        return torch.equal(self.buf[:PAD], self.before[:PAD]) and torch.equal(self.buf[n - PAD:], self.before[n - PAD:])

    def untouched(self):
        return torch.equal(self.buf, self.before)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _call(dy, C, z_batch, want_img, want_z):
    """one pcgan_concat_z_bwd call into guarded buffers; returns (dimg buffer, dz buffer, took the 16-byte form)"""
    from pcgan_amd.hip import lib, ops
    Nb, Ct, H, Wd = dy.shape
    nz = Ct - C
    gi = Guarded(Nb * C * H * Wd, dy.dtype, dy.device, -7.0)
    gz = Guarded(z_batch * nz, torch.float32, dy.device, -9.0)
    pi = gi.body.data_ptr() if want_img else None
    pz = gz.body.data_ptr() if want_z else None
    dt = lib.F32 if dy.dtype == torch.float32 else lib.BF16
    lib.check(lib.load().pcgan_concat_z_bwd(dy.data_ptr(), pi, pz, Nb, C, nz, H * Wd, z_batch, dt, ops._stream()), 'concat_z_bwd')
    torch.cuda.synchronize()
    assert gi.pads_intact() and gz.pads_intact(), 'a canary beside an output changed'
    if not want_img:
        assert gi.untouched(), 'dimg was not wanted and the buffer standing in its place changed'
    if not want_z:
        assert gz.untouched(), 'dz was not wanted and the buffer standing in its place changed'
    wide = _wide(H * Wd, dy.element_size(), dy.data_ptr(), *([pi] if want_img else []), *([pz] if want_z else []))
    return gi, gz, wide


def _check(dy, C, shared, label):
    """dz-only, dimg-only and both, against float64 numpy on the values as stored"""
    Nb, Ct, H, Wd = dy.shape
    nz, HW = Ct - C, H * Wd
    z_batch = 1 if shared else Nb
    ref = dy.detach().cpu().double().numpy()
    planes = ref[:, C:].reshape(Nb, nz, HW)
    exact, mass = planes.sum(axis=2), np.abs(planes).sum(axis=2)
    if shared:
        exact, mass = exact.sum(axis=0, keepdims=True), mass.sum(axis=0, keepdims=True)
    for want_img, want_z in ((False, True), (True, False), (True, True)):
        gi, gz, wide = _call(dy, C, z_batch, want_img, want_z)
        if want_img:
            assert torch.equal(_bits(gi.body.view(Nb, C, H, Wd)), _bits(dy[:, :C])), '%s: dimg is not a bit-exact copy' % label
        if want_z:
            d = chain_length(HW, dy.element_size(), wide) + (Nb - 1 if shared else 0)
            assert d <= 64
            got = gz.body.view(z_batch, nz).cpu().double().numpy()
            err, bound = np.abs(got - exact), d * U * mass
            print('%s img=%d: d = %d (%s form), worst error / bound %.3f' % (label, want_img, d, '16-byte' if wide else 'element',
                                                                          float((err / np.maximum(bound, 1e-300)).max())))
            assert (err <= bound).all(), '%s: dz off by %r, bound %r' % (label, err, bound)
            again = _call(dy, C, z_batch, want_img, want_z)[1]
            assert torch.equal(_bits(again.body), _bits(gz.body)), '%s: two calls, different bits' % label


def _dy(shape, dtype, dev, seed):
    Nb, C, nz, H, Wd = shape
    dy = W.seeded_normal((Nb, C + nz, H, Wd), seed).to(dtype)
    flat = dy.view(-1)
    flat[0] = -0.0                                            # the copy keeps the sign of zero ...
    if flat.numel() > C * H * Wd and C * H * Wd > 2:
        flat[1] = float('nan')                                # ... and a NaN of the image part (never summed)
    return dy.to(dev)


@pytest.mark.parametrize('shared', [False, True], ids=['z_batch_N', 'z_batch_1'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_kernel_against_float64(shape, dtype, shared, dev):
    dy = _dy(shape, dtype, dev, 500 + sum(shape))
    _check(dy, shape[1], shared, 'shape %r %s' % (shape, 'shared' if shared else 'per-sample'))


@pytest.mark.parametrize('shared', [False, True], ids=['z_batch_N', 'z_batch_1'])
def test_cancellation(shared, dev):
    """a plane of alternating +-1e4 with 1e-2 riding on it: the plane sum is 1e-6 of the magnitudes summed; same bound"""
    Nb, C, nz, H, Wd = 2, 3, 1, 64, 66
    dy = W.seeded_normal((Nb, C + nz, H, Wd), 77)
    sign = torch.ones(H * Wd)
    sign[1::2] = -1.0
    dy[:, C:] = (sign * 1e4 + 1e-2).view(1, 1, H, Wd)
    _check(dy.to(dev), C, shared, 'cancellation')


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_view_at_an_odd_storage_offset(dtype, dev):
    """dy one element into its storage, HW % 4 == 0: the base pointer is not 16-byte aligned, so the element form must be taken"""
    Nb, C, nz, H, Wd = 2, 3, 2, 8, 8
    store = torch.zeros(Nb * (C + nz) * H * Wd + 1, dtype=dtype, device=dev)
    store[1:] = W.seeded_normal((store.numel() - 1,), 91).to(dtype).to(dev)
    dy = store[1:].view(Nb, C + nz, H, Wd)
    assert dy.is_contiguous() and dy.storage_offset() == 1 and dy.data_ptr() % 16 != 0
    for shared in (False, True):
        _check(dy, C, shared, 'offset view')
    assert not _call(dy, C, Nb, True, True)[2]


# ---------------------------------------------------------------------------------------------------------------- the autograd function
def _join(img, z, dy, fused):
    from pcgan_amd.hip import functional as HF
    img, z = img.clone().requires_grad_(True), z.clone().requires_grad_(True)
    with HF.fused_concat_bwd(fused):
        out = HF.concat_z(img, z)
    node = type(out.grad_fn).__name__
    out.backward(dy)
    return out.detach(), img.grad, z.grad, node


@pytest.mark.parametrize('zb', ['N', '1'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_fused_function_equals_the_default(dtype, zb, dev, monkeypatch):
    from pcgan_amd.hip import functional as HF
    monkeypatch.setattr(HF, '_CONCATZ_FUSED_ENV', True)
    Nb, C, nz, H, Wd = 4, 3, 1, 32, 32
    img = W.seeded_tensor((Nb, C, H, Wd), 11).to(dtype).to(dev)
    z = W.seeded_normal((Nb if zb == 'N' else 1, nz, 1, 1), 12).to(dev)
    dy = W.seeded_normal((Nb, C + nz, H, Wd), 13).to(dtype).to(dev)
    out_f, dimg_f, dz_f, node_f = _join(img, z, dy, True)
    out_c, dimg_c, dz_c, node_c = _join(img, z, dy, False)
    assert node_f == '_ConcatZFusedFnBackward' and node_c == '_ConcatZFnBackward'
    assert torch.equal(_bits(out_f), _bits(out_c)) and torch.equal(_bits(dimg_f), _bits(dimg_c))
    assert dz_f.shape == z.shape == dz_c.shape and dz_f.dtype == torch.float32
    planes = dy[:, C:].double().abs().sum(dim=(2, 3))
    mass = planes if zb == 'N' else planes.sum(dim=0, keepdim=True)
    d = chain_length(H * Wd, dy.element_size(), True) + (Nb - 1 if zb == '1' else 0)
    assert bool(((dz_f.double() - dz_c.double()).abs().view_as(mass) <= 2 * d * U * mass).all())
    # only the rating needs a gradient: dimg is not formed; neither: no call
    calls = []
    from pcgan_amd.hip import ops
    orig = ops.concat_z_bwd
    monkeypatch.setattr(ops, 'concat_z_bwd', lambda *a: (calls.append(a[3:]), orig(*a))[1])
    zz = z.clone().requires_grad_(True)
    with HF.fused_concat_bwd():
        HF.concat_z(img, zz).backward(dy)
    assert calls == [(False, True)] and torch.equal(zz.grad, dz_f)
    # PCGAN_CONCATZ_FUSED=0 keeps the default function inside the context
    monkeypatch.setattr(HF, '_CONCATZ_FUSED_ENV', False)
    assert _join(img, z, dy, True)[3] == '_ConcatZFnBackward'


def _rating_gradient(hip, twin, inputs, seed_dy, dev, recorder, zero_dz=False):
    """the network inside fused_concat_bwd() against its float64 twin replaying the HIP pass's decisions: the output, the image gradient
    and the gradient of the rating, which is what the new launch produces"""
    from pcgan_amd.hip import functional as HF
    hip.load_state_dict({k: v.clone() for k, v in twin.state_dict().items()})
    hip.to(dev)
    ref64 = copy.deepcopy(twin).double()
    taken = []
    orig = HF._ConcatZFusedFn.apply
    with recorder() as rec, HF.fused_concat_bwd():
        HF._ConcatZFusedFn.apply = staticmethod(lambda *a: (taken.append(1), orig(*a))[1])
        try:
            ys, dins, _ = _run(hip, [i.to(dev) for i in inputs], seed_dy)
        finally:
            del HF._ConcatZFusedFn.apply
    torch.cuda.synchronize()
    assert taken == [1], 'the network did not join its rating through the fused function'
    N.DecisionTape.replay = iter(rec.tape)
    try:
        ys_r, dins_r, _ = _run(ref64, [i.double() for i in inputs], seed_dy)
        assert next(N.DecisionTape.replay, None) is None, 'the twin consumed fewer decisions than the HIP pass recorded'
    finally:
        N.DecisionTape.replay = None
    assert_close(ys[0], ys_r[0], 1e-4, 'output vs fp64 twin on the HIP decisions')
    _assert_mostly_close(dins[0], dins_r[0], 'image gradient vs fp64 twin on the HIP decisions', 5e-4)
    assert dins[1].shape == inputs[1].shape and dins[1].dtype == torch.float32
    if zero_dz:
        assert float(dins_r[1].abs().max()) < 1e-9 and float(dins[1].abs().max()) < 1e-3
    else:
        assert float(dins_r[1].abs().max()) > 1e-6
        _assert_mostly_close(dins[1], dins_r[1], 'rating gradient vs fp64 twin on the HIP decisions', 5e-4)


def test_rating_gradient_of_the_discriminator(dev):
    from pcgan_amd.models import networks
    twin = N.NLayerDiscriminatorRef(3, 1, 8, 3, 'batch', True)
    twin.load_state_dict(W.fill_state_dict(twin.state_dict(), 88))
    hip = networks.define_D(3, 1, 8, 'n_layers', 3, 'batch', True, 'normal')
    _rating_gradient(hip, twin, [W.seeded_tensor((4, 3, 32, 32), 188), W.seeded_normal((4, 1, 1, 1), 288)], 388, dev, record_decisions)


@pytest.mark.parametrize('norm', ['batch', 'instance'])
def test_rating_gradient_of_the_resnet_generator(norm, dev):
    """under InstanceNorm the rating's plane adds a constant to every plane of the first (reflection-padded) convolution, which the norm
    removes: the true gradient is 0 and only rounding noise remains (test_gpu_nets._compare: below 1e-3).  BatchNorm does not remove a
    constant that differs from sample to sample, so there the gradient is held to 5e-4."""
    from pcgan_amd.models import networks
    twin = N.ResnetGeneratorRef(3, 3, 1, 8, norm, 2)
    twin.load_state_dict(W.fill_state_dict(twin.state_dict(), 89))
    hip = networks.define_G(3, 3, 1, 8, 'resnet_2blocks', norm=norm, init_type='normal')
    _rating_gradient(hip, twin, [W.seeded_tensor((4, 3, 32, 32), 189), W.seeded_normal((4, 1, 1, 1), 289)], 389, dev, record_decisions,
                     zero_dz=(norm == 'instance'))


def test_rating_gradient_of_the_unet_generator(dev):
    from pcgan_amd.models import networks
    twin = UnetGeneratorRef(3, 3, 1, 7, 8, 'instance')
    twin.load_state_dict(W.fill_state_dict(twin.state_dict(), 90))
    hip = networks.define_G(3, 3, 1, 8, 'unet', norm='instance', init_type='normal')
    _rating_gradient(hip, twin, [W.seeded_tensor((1, 3, 128, 128), 190), W.seeded_normal((1, 1, 1, 1), 290)], 390, dev,
                     record_unet_decisions)
