"""pcgan_pool_exchange (csrc/image_pool.hip) and util.image_pool.ImagePool on the GPU against the plain-torch restatement of the
reference's loop (disc_ref.pool_apply).  The kernel only copies, so everything is compared as INTEGER bit patterns: the data are random
bits, which hold NaN payloads of every kind, plus an explicit -0.0 and a signalling-NaN pattern.  After every call the returned batch
AND the whole pool are checked, and the launch count is the structural one: one launch per lib.POOL_PLAN_MAX images, none at pool size 0.

Sizes: 1, 3, 7 (element form: the image stride is no multiple of 16 bytes), 4 (one 16-byte vector), 8 * 256 * 4 + 5 (more than one
workgroup), 256 * 2048 + 3 elements and 4 * (256 * 2048 + 2) elements (more elements / vectors than the capped grid has threads: the
grid-stride loop wraps); bf16 at 8 (one vector), 9 and 15 (element form); views at an odd storage offset (element form although the
image stride allows vectors)."""
import os
import random

import numpy as np
import pytest
import torch

import disc_ref as C

pytestmark = pytest.mark.gpu

GRID_THREADS = 256 * 2048         # POOL_THREADS * POOL_MAX_BLOCKS of csrc/image_pool.hip
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
NEG_ZERO = {torch.float32: -0x80000000, torch.bfloat16: -0x8000}
SNAN = {torch.float32: 0x7f800001, torch.bfloat16: 0x7f81}


def _bits(shape, dtype, seed):
    info = torch.iinfo(INT[dtype])
    t = torch.randint(info.min, info.max + 1, shape, dtype=torch.int64, generator=torch.Generator().manual_seed(seed)).to(INT[dtype])
    t.view(-1)[0] = NEG_ZERO[dtype]
    t.view(-1)[-1] = SNAN[dtype]
    return t


def _on_device(bits, dtype, dev, offset=0):
    """the bit pattern as a contiguous `dtype` tensor on the device, `offset` elements into its storage"""
    buf = torch.empty(bits.numel() + offset, dtype=INT[dtype], device=dev)
    view = buf[offset:].view(bits.shape)
    view.copy_(bits)
    return view.view(dtype)


def check(dev, dtype, n, pool_size, plan, seed, offset=0):
    from pcgan_amd.hip import lib, ops
    B = len(plan)
    x_bits, pool_bits = _bits((B, n), dtype, seed), _bits((pool_size, n), dtype, seed + 1)
    x, pool = _on_device(x_bits, dtype, dev, offset), _on_device(pool_bits, dtype, dev, offset)
    assert x.is_contiguous() and pool.is_contiguous() and x.storage_offset() == offset
    want_pool = pool_bits.clone()
    want_y = C.pool_apply(want_pool, x_bits, plan)
    before = lib.pool_exchange_launches()
    y = ops.pool_exchange(pool, x, plan)
    assert lib.pool_exchange_launches() - before == (B + lib.POOL_PLAN_MAX - 1) // lib.POOL_PLAN_MAX
    assert y.dtype == dtype and y.shape == x.shape and y.data_ptr() != x.data_ptr()
    what = '%s n %d pool %d plan %s offset %d' % (dtype, n, pool_size, plan if B <= 8 else '(%d entries)' % B, offset)
    assert torch.equal(y.view(INT[dtype]).cpu(), want_y), 'returned batch: ' + what
    assert torch.equal(pool.view(INT[dtype]).cpu(), want_pool), 'pool after the call: ' + what
    assert torch.equal(x.view(INT[dtype]).cpu(), x_bits), 'the input batch was written: ' + what


PLANS3 = [
    [0, 2, 4, 1, -1, 5],        # the fill phase running into the exchange phase within one batch
    [-1, 3, 3, -1, 3],          # one slot exchanged twice (three times): each receives its predecessor
    [2, 3, -1, 2, 3],           # a slot stored and exchanged in the same batch: the image comes straight back, twice
    [-1, -1, -1, -1],           # all-pass: the pool is untouched bit for bit
    [5],                        # a single image
]


@pytest.mark.parametrize('n', [1, 3, 4, 7, 8 * 256 * 4 + 5])
def test_pool_exchange_fp32_sizes_and_plans(n, dev):
    for i, plan in enumerate(PLANS3):
        check(dev, torch.float32, n, 3, plan, 10 * n + i)
    check(dev, torch.float32, n, 1, [0, 1, 1, -1, 1], n + 7)       # pool size 1


@pytest.mark.parametrize('n', [8, 9, 15])
def test_pool_exchange_bf16(n, dev):
    for i, plan in enumerate(PLANS3):
        check(dev, torch.bfloat16, n, 3, plan, 100 * n + i)
    check(dev, torch.bfloat16, n, 1, [0, 1, 1, -1, 1], n + 9)


@pytest.mark.parametrize('dtype,n,offset', [(torch.float32, 8, 1), (torch.float32, 4 * 300, 3), (torch.bfloat16, 16, 1), (torch.bfloat16, 8 * 40, 4)])
def test_pool_exchange_view_at_odd_storage_offset(dtype, n, offset, dev):
    """the image stride allows 16-byte accesses, the base addresses do not: the element form"""
    check(dev, dtype, n, 3, PLANS3[0], 5 * n + offset, offset)
    check(dev, dtype, n, 3, PLANS3[1], 5 * n + offset + 1, offset)


@pytest.mark.parametrize('n', [GRID_THREADS + 3, 4 * (GRID_THREADS + 2)])
def test_pool_exchange_grid_stride_wraps(n, dev):
    check(dev, torch.float32, n, 2, [0, 1, -1, 3], n % 1000)


@pytest.mark.parametrize('B', [65, 2 * 64 + 6])
def test_pool_exchange_longer_than_one_launch(B, dev):
    """capacity + 1 and 2 * capacity + 6 images: several launches, the pool carrying the state from one to the next (slots stored by
    one launch are exchanged by a later one)"""
    from pcgan_amd.hip import lib
    assert lib.POOL_PLAN_MAX == 64
    rng = random.Random(B)
    plan = [0, 2, 4] + [rng.choice([-1, 1, 3, 5]) for _ in range(B - 3)]
    plan[63], plan[64] = 3, 3             # the same slot on both sides of a launch boundary
    check(dev, torch.float32, 7, 3, plan, B)
    check(dev, torch.bfloat16, 9, 3, plan, B + 1)
    check(dev, torch.float32, 8, 3, plan, B + 2)      # 16-byte form


def test_ops_pool_exchange_refuses_mismatches(dev):
    from pcgan_amd.hip import ops
    pool, x = torch.zeros(3, 2, 4, device=dev), torch.zeros(2, 2, 4, device=dev)
    with pytest.raises(RuntimeError, match='one image shape'):
        ops.pool_exchange(pool, torch.zeros(2, 2, 5, device=dev), [-1, -1])
    with pytest.raises(RuntimeError, match='plan of 3 entries for 2 images'):
        ops.pool_exchange(pool, x, [-1, -1, -1])
    with pytest.raises(RuntimeError, match='share a storage type'):
        ops.pool_exchange(pool, x.to(torch.bfloat16), [-1, -1])
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.pool_exchange(pool, torch.zeros(2, 4, 2, device=dev).transpose(1, 2), [-1, -1])
    with pytest.raises(RuntimeError, match='slot 3 outside'):
        ops.pool_exchange(pool, x, [0, 7])
    with pytest.raises(RuntimeError, match='overlap'):
        ops.pool_exchange(x, x, [-1, -1])


def test_image_pool_size_zero_launches_nothing(dev):
    from pcgan_amd.hip import lib
    from pcgan_amd.util.image_pool import ImagePool
    x = torch.randn(4, 3, 8, 8, device=dev)
    before, state = lib.pool_exchange_launches(), random.getstate()
    assert ImagePool(0).query(x) is x
    assert lib.pool_exchange_launches() == before and random.getstate() == state


@pytest.mark.parametrize('size', [3, 1])
def test_image_pool_reproduces_the_reference(size, dev):
    """after random.seed(k), ImagePool makes the reference's decisions and returns its batches (tests/golden/disc_pool.npz), one launch
    per query; the result is detached and fresh; a change of image shape or dtype afterwards raises"""
    from pcgan_amd.hip import lib
    from pcgan_amd.util.image_pool import ImagePool
    gold = np.load(os.path.join(C.GOLD, 'disc_pool.npz'))
    random.seed(int(gold['seed']))
    pool = ImagePool(size)
    for q in range(6):
        x = torch.from_numpy(gold['size%d/q%d/x' % (size, q)]).to(dev).requires_grad_(True)
        before = lib.pool_exchange_launches()
        y = pool.query(x * 1.0)
        assert lib.pool_exchange_launches() - before == 1
        assert not y.requires_grad and y.data_ptr() != x.data_ptr()
        assert torch.equal(y.cpu().view(torch.int32), torch.from_numpy(gold['size%d/q%d/y' % (size, q)]).view(torch.int32)), 'query %d' % q
    assert tuple(pool.images.shape) == (size, 2, 3, 5) and pool.images.dtype == torch.float32 and pool.num_imgs == size
    for bad in (torch.zeros(4, 2, 3, 6, device=dev), torch.zeros(4, 2, 3, 5, device=dev, dtype=torch.bfloat16)):
        with pytest.raises(RuntimeError, match='ImagePool holds'):
            pool.query(bad)
    # an injected plan: exchange() is the launch alone
    kept = pool.images.clone()
    x = torch.randn(2, 2, 3, 5, device=dev)
    y = pool.exchange(x, [lib.pool_swap(0), lib.POOL_PASS])
    assert torch.equal(y[0], kept[0]) and torch.equal(y[1], x[1]) and torch.equal(pool.images[0], x[0])
