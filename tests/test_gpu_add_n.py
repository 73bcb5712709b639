"""pcgan_add_n (csrc/grad_fanin.hip), the n-ary gradient sum, and hip.functional.fan_out on the GPU.

The kernel adds strictly left to right in fp32 and never multiplies, so its result is DEFINED bit for bit: the sequential float32 sum the
CPU forms, rounded once (to nearest even) for bf16 tensors.  Every value comparison here is torch.equal on the raw bits.  Sizes: below,
at and above one 16-byte access (4 fp32 / 8 bf16 elements), a tail, more than one workgroup, and one size just past the span of the
capped grid (2048 workgroups x 256 threads x elements per access) so that the grid-stride loop runs a second time."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCKS, THREADS = 2048, 256       # ADDN_MAX_BLOCKS, ADDN_THREADS of csrc/grad_fanin.hip
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def _values(n, k, dtype, seed):
    """k tensors of n values: magnitudes 1e-8 .. 1e4, both signs, one in ten an exact zero"""
    rs = np.random.RandomState(seed)
    v = np.power(10.0, rs.uniform(-8.0, 4.0, size=(k, n))) * rs.choice([-1.0, 1.0], size=(k, n))
    v[rs.uniform(size=(k, n)) < 0.1] = 0.0
    return [torch.from_numpy(v[i].astype(np.float32)).to(dtype) for i in range(k)]


def _cpu_sum(srcs):
    """the sequential float32 sum, rounded once to the storage type"""
    acc = srcs[0].float()
    for s in srcs[1:]:
        acc = acc + s.float()
    return acc.to(srcs[0].dtype)


def _bits(t):
    return t.cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('k', [1, 2, 3, 5, 8])
def test_add_n_is_the_sequential_fp32_sum(k, dtype, dev):
    from pcgan_amd.hip import ops
    for n in (1, 3, 4, 5, 1023, 4096 + 7):
        srcs = _values(n, k, DTYPES[dtype], 100 * k + n % 97)
        got = ops.add_n([s.to(dev) for s in srcs])
        assert got.dtype == DTYPES[dtype] and got.data_ptr() not in [s.data_ptr() for s in srcs]
        assert torch.equal(_bits(got), _bits(_cpu_sum(srcs))), 'n = %d, %d sources, %s' % (n, k, dtype)


@pytest.mark.parametrize('dtype,k', [('fp32', 2), ('fp32', 5), ('bf16', 5), ('bf16', 8)])
def test_add_n_wraps_the_capped_grid(dtype, k, dev):
    from pcgan_amd.hip import ops
    per_access = 4 if dtype == 'fp32' else 8
    n = BLOCKS * THREADS * per_access + per_access + 3        # every thread once, the first a second time, and a tail
    srcs = _values(n, k, DTYPES[dtype], 7 + k)
    got = ops.add_n([s.to(dev) for s in srcs])
    assert torch.equal(_bits(got), _bits(_cpu_sum(srcs)))


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_add_n_misaligned_views_take_the_element_route(dtype, dev):
    """a contiguous view at storage offset 1 (4 or 2 bytes past a 16-byte boundary) for y, and for one source: same bits"""
    from pcgan_amd.hip import ops
    for n in (5, 4096 + 7, BLOCKS * THREADS + 5):           # the last: past the span of the element route's grid
        srcs = _values(n, 3, DTYPES[dtype], 31 + n % 89)
        want = _bits(_cpu_sum(srcs))
        on_dev = [s.to(dev) for s in srcs]
        y = torch.zeros(n + 2, dtype=DTYPES[dtype], device=dev)
        out = ops.add_n(on_dev, out=y[1:n + 1])
        assert out.data_ptr() % 16 != 0 and torch.equal(_bits(out), want)
        assert float(y[0]) == 0.0 and float(y[n + 1]) == 0.0          # nothing written outside the view
        shifted = torch.zeros(n + 1, dtype=DTYPES[dtype], device=dev)
        shifted[1:].copy_(on_dev[1])
        assert shifted[1:].data_ptr() % 16 != 0
        assert torch.equal(_bits(ops.add_n([on_dev[0], shifted[1:], on_dev[2]])), want)


def test_add_n_refuses_on_the_host(dev):
    from pcgan_amd.hip import ops
    a = torch.ones(8, device=dev)
    with pytest.raises(ValueError):
        ops.add_n([a] * 9)
    with pytest.raises(ValueError):
        ops.add_n([])
    with pytest.raises(RuntimeError, match='alias'):
        ops.add_n([a, torch.ones(8, device=dev)], out=a)
    with pytest.raises(RuntimeError, match='storage type'):
        ops.add_n([a, a.to(torch.bfloat16)])
    with pytest.raises(RuntimeError, match='equal shapes'):
        ops.add_n([a, torch.ones(9, device=dev)])


@pytest.mark.parametrize('consumers', [1, 2, 5])
def test_fan_out_gradient(consumers, dev, monkeypatch):
    """d/dx of sum_i <w_i, tanh(c_i * x_i)> with x_i the aliases: against plain autograd in float64, 1e-6 relative L2"""
    from pcgan_amd.hip import functional as HF
    from pcgan_amd.hip import ops
    calls = []
    orig = ops.add_n
    monkeypatch.setattr(ops, 'add_n', lambda ts, out=None: (calls.append(len(ts)), orig(ts, out))[1])
    x = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, size=(2, 3, 17, 19)).astype(np.float32))
    w = [torch.from_numpy(np.random.RandomState(10 + i).normal(size=x.shape).astype(np.float32)) for i in range(consumers)]
    x64 = x.double().requires_grad_(True)
    sum((w[i].double() * torch.tanh((i + 1) * x64)).sum() for i in range(consumers)).backward()
    xd = x.to(dev).requires_grad_(True)
    outs = HF.fan_out(xd, consumers)
    assert len(outs) == consumers and all(o.data_ptr() == xd.data_ptr() for o in outs)        # aliases: no copy
    sum((w[i].to(dev) * torch.tanh((i + 1) * outs[i])).sum() for i in range(consumers)).backward()
    err = float((xd.grad.double().cpu() - x64.grad).norm() / x64.grad.norm())
    assert err <= 1e-6, 'relative L2 %.3e' % err
    assert calls == ([consumers] if consumers > 1 else [])          # ONE launch over all of them; none for a single consumer


def test_fan_out_skips_unused_outputs_and_hands_a_single_gradient_on(dev, monkeypatch):
    from pcgan_amd.hip import functional as HF
    from pcgan_amd.hip import ops
    calls = []
    orig = ops.add_n
    monkeypatch.setattr(ops, 'add_n', lambda ts, out=None: (calls.append(len(ts)), orig(ts, out))[1])
    leaf = torch.linspace(-1, 1, 40, device=dev).requires_grad_(True)
    # outputs 1 and 3 of 4 are never used: their gradients are None and are left out of the sum
    outs = HF.fan_out(leaf * 1.0, 4)
    ((outs[0] * 2.0).sum() + (outs[2] * 3.0).sum()).backward()
    assert calls == [2] and torch.equal(leaf.grad, torch.full_like(leaf, 5.0))
    # nothing used at all: no gradient, no launch
    leaf.grad = None
    x = leaf * 1.0
    HF.fan_out(x, 3)
    x.sum().backward()
    assert calls == [2] and torch.equal(leaf.grad, torch.ones_like(leaf))
    # one consumer of three: the incoming tensor itself goes on (same storage), no launch
    seen = {}
    x = leaf * 1.0
    x.register_hook(lambda g: seen.__setitem__('x', g.data_ptr()))
    outs = HF.fan_out(x, 3)
    outs[1].register_hook(lambda g: seen.__setitem__('o', g.data_ptr()))
    (outs[1] * 4.0).sum().backward()
    assert calls == [2] and seen['x'] == seen['o']
    with pytest.raises(RuntimeError, match='mixed dtypes'):
        HF._FanOutFn.backward(None, torch.ones(4, device=dev), torch.ones(4, device=dev, dtype=torch.bfloat16))
