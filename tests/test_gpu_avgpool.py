"""GPU: the windowed average pool (pcgan_avgpool_fwd / pcgan_avgpool_bwd, count_include_pad=False) and the pyramid node built on it.

The criterion is BIT EQUALITY with F.avg_pool2d(..., count_include_pad=False) and its autograd on the CPU in float32: the kernels sum the
in-bounds taps in scan order from the first tap and divide once by their number (an IEEE division), and the gradient adds the quotients
dy[p][q] / count(p, q) in ascending (p, q) from 0 -- the order ATen's CPU kernels use, so nothing is left to a tolerance.  With bf16
storage the kernels round the float32 result ONCE: the expectation is the float32 CPU result on the up-cast (bf16-valued) inputs, cast to
bf16 (ATen's own bf16 gradient rounds every partial sum and is not the yardstick; its bf16 forward is, and is checked as well).  `base`
rides into the gradient as one more float32 add before that single rounding, out of place and with dx aliasing base.

Shapes (NC, H, W), k = 3, stride 2, pad 1 unless stated: one tap; one output of count 4; counts 4 / 6 / 9 on odd and even sides; planes that are
only element-aligned; a plane of more than one grid sweep (a sweep is 32 x 256 elements); more planes than gridDim.y allows; a window without
padding (2, 2, 0) and an overlapping stride-1 one (3, 1, 1).
"""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

DEFAULT = (3, 2, 1)
SHAPES = [((1, 1, 1), DEFAULT), ((1, 2, 2), DEFAULT), ((3, 2, 3), DEFAULT), ((5, 5, 4), DEFAULT), ((2, 7, 9), DEFAULT), ((8, 16, 16), DEFAULT),
          ((6, 33, 31), DEFAULT), ((3, 256, 256), DEFAULT), ((70000, 2, 2), DEFAULT), ((4, 9, 9), (2, 2, 0)), ((4, 9, 9), (3, 1, 1))]
IDS = ['%dx%dx%d-k%ds%dp%d' % (s + c) for s, c in SHAPES]


def _pool(x, cfg):
    k, s, p = cfg
    return F.avg_pool2d(x, k, stride=s, padding=p, count_include_pad=False)


@functools.lru_cache(maxsize=None)
def _case(shape, cfg, bf16):
    """seeded x, dy, base of a shape (bf16-valued float32 tensors when bf16) and the float32 CPU results: computed once, never modified"""
    NC, H, W = shape
    g = torch.Generator().manual_seed(NC * 131 + H * 17 + W + 1000 * int(bf16))
    x = torch.randn(1, NC, H, W, generator=g)
    if bf16:
        x = x.to(BF).float()
    xr = x.clone().requires_grad_(True)
    y = _pool(xr, cfg)
    dy = torch.randn(y.shape, generator=g)
    base = torch.randn(x.shape, generator=g)
    if bf16:
        dy, base = dy.to(BF).float(), base.to(BF).float()
    y.backward(dy)
    return SimpleNamespace(x=x, dy=dy, base=base, y=y.detach(), dx=xr.grad, dx_base=base + xr.grad)


@pytest.mark.parametrize('shape,cfg', SHAPES, ids=IDS)
def test_fp32_is_bit_equal_to_the_cpu(shape, cfg, dev):
    from pcgan_amd.hip import ops
    c = _case(shape, cfg, False)
    x, dy, base = c.x.to(dev), c.dy.to(dev), c.base.to(dev)
    hw = tuple(x.shape[2:])
    y = ops.avgpool_fwd(x, *cfg)
    assert y.shape == c.y.shape and y.dtype == torch.float32
    assert torch.equal(y.cpu(), c.y), 'forward'
    dx = ops.avgpool_bwd(dy, hw, *cfg)
    assert torch.equal(dx.cpu(), c.dx), 'gradient'
    dxb = ops.avgpool_bwd(dy, hw, *cfg, base=base)
    assert dxb.data_ptr() != base.data_ptr() and torch.equal(base.cpu(), c.base), 'out of place: base is left alone'
    assert torch.equal(dxb.cpu(), c.dx_base), 'gradient + base'
    # dx aliasing base, inside a guarded buffer one element off a 16-byte boundary: nothing outside the tensor is written
    n = base.numel()
    flat = torch.full((n + 9,), 7.0, device=dev)
    inplace = flat[1:1 + n].view(base.shape)
    inplace.copy_(base)
    got = ops.avgpool_bwd(dy, hw, *cfg, base=inplace, out=inplace)
    assert got.data_ptr() == inplace.data_ptr()
    assert torch.equal(inplace.cpu(), c.dx_base), 'gradient + base, dx aliasing base'
    assert float(flat[0]) == 7.0 and bool((flat[1 + n:] == 7.0).all()), 'wrote outside dx'
    # repeats
    assert torch.equal(ops.avgpool_fwd(x, *cfg), y) and torch.equal(ops.avgpool_bwd(dy, hw, *cfg), dx)
    assert torch.equal(ops.avgpool_bwd(dy, hw, *cfg, base=base), dxb)


@pytest.mark.parametrize('shape,cfg', SHAPES, ids=IDS)
def test_bf16_rounds_the_fp32_result_once(shape, cfg, dev):
    from pcgan_amd.hip import ops
    c = _case(shape, cfg, True)
    x, dy, base = c.x.to(dev).to(BF), c.dy.to(dev).to(BF), c.base.to(dev).to(BF)
    assert torch.equal(x.float().cpu(), c.x) and torch.equal(dy.float().cpu(), c.dy)         # bf16-valued: the casts lose nothing
    hw = tuple(x.shape[2:])
    y = ops.avgpool_fwd(x, *cfg)
    assert y.dtype == BF
    assert torch.equal(y.cpu(), c.y.to(BF)), 'forward'
    assert torch.equal(y.cpu(), _pool(c.x.to(BF), cfg)), "forward against torch's own bf16 forward"
    dx = ops.avgpool_bwd(dy, hw, *cfg)
    assert dx.dtype == BF and torch.equal(dx.cpu(), c.dx.to(BF)), 'gradient'
    want = c.dx_base.to(BF)                                                                  # (base.float() + grad).to(bf16)
    assert torch.equal(ops.avgpool_bwd(dy, hw, *cfg, base=base).cpu(), want), 'gradient + base'
    inplace = base.clone()
    ops.avgpool_bwd(dy, hw, *cfg, base=inplace, out=inplace)
    assert torch.equal(inplace.cpu(), want), 'gradient + base, dx aliasing base'
    assert torch.equal(ops.avgpool_bwd(dy, hw, *cfg), dx)


def test_wrappers_refuse_what_the_kernel_cannot_serve(dev):
    from pcgan_amd.hip import ops
    x = torch.zeros(1, 2, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match='entirely in the padding'):
        ops.avgpool_fwd(x, 3, 2, 2)
    with pytest.raises(RuntimeError, match='share a storage type'):
        ops.avgpool_bwd(torch.zeros(1, 2, 4, 4, device=dev), (8, 8), 3, 2, 1, base=x.to(BF))
    with pytest.raises(RuntimeError, match='base of shape'):
        ops.avgpool_bwd(torch.zeros(1, 2, 4, 4, device=dev), (8, 8), 3, 2, 1, base=x[:, :1].contiguous())
    with pytest.raises(RuntimeError, match='floor mode'):
        ops.avgpool_bwd(torch.zeros(1, 2, 5, 4, device=dev), (8, 8), 3, 2, 1)


# ---- the pyramid node ------------------------------------------------------------------------------------------------------------------------
PYRAMIDS = [(2, (2, 3, 32, 32)), (3, (2, 3, 32, 32)), (2, (1, 3, 35, 37)), (3, (1, 3, 35, 37))]


def _cpu_pyramid(x, levels):
    out = [x.view_as(x)]
    for _ in range(levels - 1):
        out.append(_pool(out[-1], DEFAULT))
    return out


def _seeds(outs, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g) for o in outs]


@pytest.mark.parametrize('levels,shape', PYRAMIDS)
def test_pyramid_matches_the_chained_pools(levels, shape, dev):
    from pcgan_amd.hip import functional as HF
    x = torch.randn(shape, generator=torch.Generator().manual_seed(levels + shape[2]))
    xc = x.clone().requires_grad_(True)
    ref = _cpu_pyramid(xc, levels)
    gs = _seeds(ref, 5)
    xd = x.to(dev).requires_grad_(True)
    outs = HF.avg_pool_pyramid(xd, levels)
    assert isinstance(outs, tuple) and len(outs) == levels
    assert outs[0].data_ptr() == xd.data_ptr() and outs[0].shape == xd.shape, 'x0 shares storage with x'
    for a, b in zip(outs, ref):
        assert torch.equal(a.detach().cpu(), b.detach())
    # every subset of live gradients the module can meet: all, g0 missing, only the coarsest
    for live in (list(range(levels)), list(range(1, levels)), [levels - 1]):
        xc.grad = xd.grad = None
        torch.autograd.backward([ref[i] for i in live], [gs[i] for i in live], retain_graph=True)
        torch.autograd.backward([outs[i] for i in live], [gs[i].to(dev) for i in live], retain_graph=True)
        assert torch.equal(xd.grad.cpu(), xc.grad), 'input gradient with levels %r live' % (live,)


def test_pyramid_edge_cases(dev, monkeypatch):
    from pcgan_amd.hip import functional as HF, ops
    calls = []
    orig = ops.avgpool_bwd
    monkeypatch.setattr(ops, 'avgpool_bwd', lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    x = torch.randn(2, 3, 32, 32, device=dev)
    # one level: x itself, nothing launched
    assert HF.avg_pool_pyramid(x, 1)[0] is x
    # no gradient at all: None, nothing launched
    ctx = SimpleNamespace(needs_input_grad=(True, False, False, False, False), hw=[(32, 32), (16, 16), (8, 8)], cfg=DEFAULT)
    assert HF._AvgPoolPyramidFn.backward(ctx, None, None, None) == (None,) * 5 and not calls
    # one launch per level below the coarsest live one
    xg = x.clone().requires_grad_(True)
    outs = HF.avg_pool_pyramid(xg, 3)
    torch.autograd.backward(list(outs), [torch.ones_like(o) for o in outs])
    assert len(calls) == 2 and xg.grad is not None
    # an input that needs no gradient (netD(fake.detach()), netD(real)): the backward pass of what follows launches nothing here
    del calls[:]
    w = torch.ones(1, device=dev, requires_grad=True)
    outs = HF.avg_pool_pyramid(x, 3)
    assert not any(o.requires_grad for o in outs)
    sum((o * w).sum() for o in outs).backward()
    assert w.grad is not None and not calls
    # bf16 storage passes through every level
    outs = HF.avg_pool_pyramid(x.to(BF), 3)
    assert all(o.dtype == BF for o in outs) and [tuple(o.shape[2:]) for o in outs] == [(32, 32), (16, 16), (8, 8)]
