"""CPU: the multi-scale PatchGAN discriminator's host side and its oracle twins.

* tests/multid_ref.py (the CPU twins the GPU tests judge with) reproduces tests/golden/multi_d.npz, recorded from the reference's own
  define_D(..., 'n_layers_multi', ...) by scripts/make_multid_golden.py: keys, shapes, every scale's output, the gradients -- assert_close
  at 1e-5 in float32 with an absolute floor of 1e-6 of the largest parameter gradient where the true gradient is 0 (a bias in front of a
  train-mode norm: every inner convolution of this network), tests/test_projection.py's tolerances for its twin.
* define_D builds the product module with exactly those keys and shapes, its seeded initialisation draws the reference's numbers, the widths
  follow the reference's cumulative rule, and checkpoints load strictly.
* what is refused: a rating (nz >= 1), an input too small for the coarsest scale, CPU tensors, bad arguments of the two C entry points
  (validated before any launch, so this runs without a GPU).
* the step twin against tests/golden/cycle_multid_step.npz with tests/test_cycle_oracle_golden.py's tolerances.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import multid_ref as M
from oracle import weights as W
from test_cycle_oracle_golden import check_against_golden, cycle_inputs
from util_cmp import assert_close

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'multi_d.npz')
STEP_GOLD = os.path.join(HERE, 'golden', 'cycle_multid_step.npz')
TOL = 1e-5


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def case(gold, prefix):
    """(define_D arguments, state dict, x, dy seed) of a golden configuration; weights and inputs that the file does not hold come from its
    recorded seeds"""
    ndf, nl, sigm, num, bs, size, wseed, xseed, dyseed = (int(v) for v in gold[prefix + '/case'])
    norm = str(gold[prefix + '/norm'])
    keys = [str(k) for k in gold[prefix + '/keys']]
    shapes = [tuple(int(d) for d in str(s).split(',') if d) for s in gold[prefix + '/shapes']]
    if prefix + '/x' in gold.files:
        sd = {k: torch.from_numpy(gold['%s/sd/%s' % (prefix, k)]) for k in keys}
        x = torch.from_numpy(gold[prefix + '/x'])
    else:
        like = {k: torch.empty(s, dtype=torch.int64 if k.endswith('num_batches_tracked') else torch.float32) for k, s in zip(keys, shapes)}
        sd = W.fill_state_dict(like, wseed)
        x = W.seeded_tensor((bs, 3, size, size), xseed)
    return dict(ndf=ndf, nl=nl, sigm=bool(sigm), num=num, norm=norm, keys=keys, shapes=shapes, sd=sd, x=x, dyseed=dyseed)


def twin_of(c):
    twin = M.MultiScaleDiscriminatorRef(3, c['ndf'], c['nl'], c['norm'], c['sigm'], c['num'])
    twin.load_state_dict(c['sd'], strict=True)
    return twin


def product_of(c, init_type='normal'):
    from pcgan_amd.models import networks
    return networks.define_D(3, 0, c['ndf'], 'n_layers_multi', c['nl'], c['norm'], c['sigm'], init_type, num_Ds=c['num'])


# ---- the twin against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prefix', ['M0', 'M1', 'M2'])
def test_twin_reproduces_the_reference(gold, prefix):
    c = case(gold, prefix)
    twin = twin_of(c)
    assert list(twin.state_dict().keys()) == c['keys']
    assert [tuple(v.shape) for v in twin.state_dict().values()] == c['shapes']
    x = c['x'].clone().requires_grad_(True)
    out = twin(x)
    outs = out if isinstance(out, list) else [out]
    assert isinstance(out, list) == (c['num'] > 1) and len(outs) == c['num']
    torch.autograd.backward(outs, [W.seeded_normal(tuple(o.shape), c['dyseed'] + j) for j, o in enumerate(outs)])
    for j, o in enumerate(outs):
        assert_close(o, torch.from_numpy(gold['%s/out%d' % (prefix, j)]), TOL, 'out%d' % j)
    if prefix == 'M0':
        return          # keys and output only
    stride = int(gold['stride'])
    if prefix + '/din0' in gold.files:
        assert_close(x.grad, torch.from_numpy(gold[prefix + '/din0']), TOL, 'dx')
    else:
        assert_close(x.grad.reshape(-1)[::stride], torch.from_numpy(gold[prefix + '/din0_samp']), TOL, 'dx sample')
        st = gold[prefix + '/din0_stat']
        assert abs(float(x.grad.double().norm()) - st[2]) <= TOL * st[2]
    wmax = max(float(p.grad.abs().max()) for p in twin.parameters())
    for k, p in twin.named_parameters():
        full, samp = '%s/dparam/full/%s' % (prefix, k), '%s/dparam/samp/%s' % (prefix, k)
        got, want = (p.grad, gold[full]) if full in gold.files else (p.grad.reshape(-1)[::stride], gold[samp])
        # a bias in front of a normalisation has a true gradient of 0: fp32 noise on both sides, held by an absolute floor
        assert_close(got, torch.from_numpy(want), TOL, 'd' + k, atol=1e-6 * wmax)
        st = gold['%s/dparam/stat/%s' % (prefix, k)]
        assert abs(float(p.grad.double().norm()) - st[2]) <= TOL * st[2] + 1e-6 * wmax, 'l2 of d' + k
    for k, b in twin.named_buffers():
        if 'running' in k:
            ref = gold['%s/buf/%s' % (prefix, k)]
            assert abs(float(b.double().sum()) - ref[0]) <= 1e-5 * (abs(ref[1]) + 1), 'buffer ' + k
            full = '%s/buf_full/%s' % (prefix, k)
            if full in gold.files:
                assert_close(b, torch.from_numpy(gold[full]), TOL, 'buffer ' + k, atol=1e-7)


def test_patch_maps_of_the_step_configuration(gold):
    """--n_layers_D 2 --num_Ds 2 at 32 x 32, batch 4: (4, 1, 6, 6) and (4, 1, 2, 2), as the reference's step produced them"""
    step = np.load(STEP_GOLD)
    assert step['patch_shapes'].tolist() == [[4, 1, 6, 6], [4, 1, 2, 2]]
    assert [tuple(gold['M1/out%d' % j].shape) for j in range(2)] == [(4, 1, 6, 6), (4, 1, 2, 2)]
    assert [tuple(gold['M2/out%d' % j].shape) for j in range(3)] == [(2, 1, 14, 14), (2, 1, 6, 6), (2, 1, 2, 2)]


# ---- the product module on the CPU (fails where define_D refuses the name) ------------------------------------------------------------------
@pytest.mark.parametrize('prefix', ['M0', 'M1', 'M2'])
def test_define_D_builds_the_references_state_dict(gold, prefix):
    from pcgan_amd.hip import nn as hnn
    from pcgan_amd.models import networks
    c = case(gold, prefix)
    net = product_of(c)
    assert isinstance(net, networks.D_NLayersMulti) and net.num_D == c['num']
    sd = net.state_dict()
    assert list(sd.keys()) == c['keys']
    assert [tuple(v.shape) for v in sd.values()] == c['shapes']
    convs = [m for m in net.modules() if isinstance(m, hnn.Conv2d)]
    assert len(convs) == c['num'] * (c['nl'] + 2) and all(m.bias is not None for m in convs), 'every convolution carries a bias'
    assert hasattr(net, 'model') == (c['num'] == 1) and hasattr(net, 'model0') == (c['num'] > 1)
    net.load_state_dict(c['sd'], strict=True)
    assert all(torch.equal(v, c['sd'][k]) for k, v in net.state_dict().items())
    assert all(p.requires_grad for p in net.parameters())


@pytest.mark.parametrize('prefix', ['M0', 'M1'])
def test_seeded_initialisation_draws_the_references_weights(gold, prefix):
    """modules are created in the reference's order and init_weights visits them in it: the same seed, the same numbers"""
    c = case(gold, prefix)
    torch.manual_seed(int(gold['init_seed']))
    net = product_of(c)
    for k, v in net.state_dict().items():
        ref = gold['init/%s/%s' % (prefix, k)]
        a = v.double()
        assert abs(float(a.sum()) - ref[0]) <= 1e-9 * (ref[1] + 1) and abs(float(a.abs().sum()) - ref[1]) <= 1e-9 * (ref[1] + 1), k


def test_widths_shrink_cumulatively(gold):
    from pcgan_amd.models import networks
    rows = {int(r[0]): [int(v) for v in r[1:]] for r in gold['widths']}
    assert rows[64] == [64, 32, 8] and rows[16] == [16, 8, 2] and rows[8] == [8, 4, 1] and sorted(rows) == [8, 12, 16, 64]
    for ndf, want in rows.items():
        net = networks.D_NLayersMulti(3, ndf, n_layers=1, num_D=3)
        assert [getattr(net, 'model%d' % i)[0].out_channels for i in range(3)] == want, ndf
        assert M.widths(ndf, 3) == want


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_a_rating_stays_refused():
    from pcgan_amd.models import networks
    for nz in (1, 2):
        with pytest.raises(NotImplementedError) as e:
            networks.define_D(3, nz, 8, 'n_layers_multi', 2, 'batch', True, num_Ds=2)
        msg = str(e.value)
        assert 'outside the MI355X hot path' in msg and 'unconditional' in msg and '--model wsgan_cycle' in msg
    for name in ('pixel', 'pyramid', 'gan_stability', 'gan_stability_class', 'mnist_fc'):
        for nz in (0, 1):
            with pytest.raises(NotImplementedError, match='outside the MI355X hot path'):
                networks.define_D(3, nz, 8, name, 3, 'batch', True)


@pytest.mark.parametrize('nl,num', [(2, 2), (3, 2), (2, 3), (1, 1), (2, 1)])
def test_smallest_admissible_side_is_what_the_stacks_accept(nl, num):
    """min_side() is exact: the torch twin (the reference's layers) runs at that side and dies inside conv2d one pixel below it, and the
    product module raises ValueError, naming the side, before anything is launched"""
    from pcgan_amd.models import networks
    net = networks.D_NLayersMulti(3, 16, n_layers=nl, num_D=num)
    m = net.min_side()
    twin = M.MultiScaleDiscriminatorRef(3, 16, nl, 'batch', False, num)
    out = twin(torch.zeros(2, 3, m, m))
    last = out[-1] if num > 1 else out
    assert tuple(last.shape) == (2, 1, 1, 1)
    with pytest.raises(RuntimeError):
        twin(torch.zeros(2, 3, m - 1, m - 1))
    for shape in ((2, 3, m - 1, m - 1), (2, 3, m + 5, m - 1), (2, 3, m - 1, m)):
        with pytest.raises(ValueError, match=r'at least %d\b' % m):
            net(torch.zeros(shape))


def test_too_small_input_of_the_golden_configuration(gold):
    net = product_of(case(gold, 'M1'))
    assert net.min_side() == 23          # 23 -> (pool) 12 -> 6 -> 3 -> 2 -> 1
    with pytest.raises(ValueError, match='n_layers = 2 and num_D = 2.*at least 23'):
        net(torch.zeros(4, 3, 16, 16))


def test_module_and_wrappers_refuse_cpu_tensors(gold):
    from pcgan_amd.hip import functional as HF, ops
    for prefix in ('M0', 'M1'):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            product_of(case(gold, prefix))(torch.zeros(4, 3, 32, 32))
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.avgpool_fwd(x, 3, 2, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.avgpool_bwd(torch.zeros(2, 3, 4, 4), (8, 8), 3, 2, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.avgpool_bwd(torch.zeros(2, 3, 4, 4), (8, 8), 3, 2, 1, base=x, out=x)
    for levels in (1, 2, 3):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            HF.avg_pool_pyramid(x, levels)
    with pytest.raises(ValueError, match='levels'):
        HF.avg_pool_pyramid(x, 0)
    from pcgan_amd.models import networks
    with pytest.raises(ValueError, match='no channels left'):
        networks.D_NLayersMulti(3, 4, n_layers=2, num_D=3)           # 4 -> 2 -> int(round(0.5)) = 0


# ---- the C entry points ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound():
    from pcgan_amd.hip import lib
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'pcgan_hip.h')).read()
    h = lib.load()
    for name, nargs in (('pcgan_avgpool_fwd', 12), ('pcgan_avgpool_bwd', 13)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
        decl = re.search(r'int %s\(([^;]*)\);' % name, header)
        assert decl is not None and decl.group(1).count(',') == nargs - 1, name
        getattr(h, name)
    assert 'models/networks.py:1897, 1948' in header


def test_avgpool_entry_points_refuse_bad_arguments_before_any_launch():
    from pcgan_amd.hip import lib
    h = lib.load()
    one, two = ctypes.c_void_p(4096), ctypes.c_void_p(8192)      # non-null addresses that are never dereferenced: every call fails its checks

    def fwd(x=one, y=two, NC=2, H=8, W=8, k=3, stride=2, pad=1, P=4, Q=4, dtype=lib.F32):
        return h.pcgan_avgpool_fwd(x, y, NC, H, W, k, stride, pad, P, Q, dtype, None)

    def bwd(dy=one, base=None, dx=two, NC=2, H=8, W=8, k=3, stride=2, pad=1, P=4, Q=4, dtype=lib.F32):
        return h.pcgan_avgpool_bwd(dy, base, dx, NC, H, W, k, stride, pad, P, Q, dtype, None)
    for call, who in ((fwd, b'avgpool_fwd'), (bwd, b'avgpool_bwd')):
        for bad in (dict(NC=0), dict(H=0), dict(W=-1), dict(k=0), dict(stride=0), dict(pad=-1), dict(P=0), dict(Q=0)):
            assert call(**bad) != 0 and who in h.pcgan_last_error() and b'positive' in h.pcgan_last_error(), bad
        for bad in (dict(pad=2), dict(k=2, pad=2, P=5, Q=5), dict(k=1, pad=1, stride=1, P=10, Q=10)):
            assert call(**bad) != 0 and b'entirely in the padding' in h.pcgan_last_error(), bad
        for bad in (dict(P=5), dict(Q=3), dict(H=9, W=9, P=4, Q=4)):
            assert call(**bad) != 0 and b'floor mode' in h.pcgan_last_error(), bad
        assert call(H=1, W=1, k=4, pad=1, P=1, Q=1) != 0 and who in h.pcgan_last_error()          # the window does not fit the padded plane
        assert call(dtype=7) != 0 and b'dtype' in h.pcgan_last_error()
    assert fwd(x=None) != 0 and fwd(y=None) != 0 and b'null' in h.pcgan_last_error()
    assert bwd(dy=None) != 0 and bwd(dx=None) != 0 and b'null' in h.pcgan_last_error()
    assert bwd(dx=one) != 0 and b'dx may alias base, not dy' in h.pcgan_last_error()


# ---- the step twin against the reference's step ---------------------------------------------------------------------------------------------
def test_cycle_step_twin_matches_the_reference():
    torch.set_num_threads(4)
    gold = np.load(STEP_GOLD)
    m = M.build_cycle_multid_oracle()
    assert list(m.netD.state_dict().keys()) == [str(k) for k in gold['netD_keys']]
    for it in range(2):
        A, attr = cycle_inputs(it)
        torch.manual_seed(4321 + it)
        m.set_input(A, attr)
        m.optimize_parameters()
        check_against_golden(gold, 'it%d' % it, m.losses(), {k: getattr(m, k) for k in ('fake_x', 'rec_x', 'fake_y', 'rec_y', 'real_y')},
                             m.grads, {'G': m.netG, 'D': m.netD, 'E': m.netE})
