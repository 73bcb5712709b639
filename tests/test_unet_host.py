"""CPU: the U-Net generator's host side -- the twin (tests/unet_ref.py) against the vectors recorded from the reference
(tests/golden/unet.npz, scripts/make_unet_golden.py), and define_G's `unet` / `unet_256` wiring: key lists, shapes, parameter counts,
refusals.  No kernel runs here: the HIP modules are only constructed."""
import os

import numpy as np
import pytest
import torch

from oracle import weights as W
from unet_ref import REFERENCE_COUNTS, UnetGeneratorRef

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'unet.npz')
TOL = 1e-5


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def golden_case(gold, prefix):
    """(twin in float32 with the case's weights, image, z, dy seed) of a recorded case"""
    nl, ngf, bs, size, wseed, dyseed, sx, sz = (int(v) for v in gold[prefix + '/case'])
    net = UnetGeneratorRef(3, 3, 1, nl, ngf, str(gold[prefix + '/norm']))
    net.load_state_dict(W.fill_state_dict(net.state_dict(), wseed))
    return net, W.seeded_tensor((bs, 3, size, size), sx), W.seeded_normal((bs, 1, 1, 1), sz), dyseed


def _close(got, want, name):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, '%s: shape %s vs %s' % (name, got.shape, want.shape)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    assert err <= TOL * scale + 1e-9, '%s: max abs error %.3e > %.0e * %.3e' % (name, err, TOL, scale)


@pytest.mark.parametrize('prefix', ['U5i', 'U5b'])
def test_twin_reproduces_the_reference(prefix, gold):
    """output, every gradient, the running statistics and the eval-mode output after the train-mode pass: the out-of-place twin (skip =
    LeakyReLU(x)) IS the reference's in-place network"""
    net, x, z, dyseed = golden_case(gold, prefix)
    assert list(net.state_dict().keys()) == list(gold[prefix + '/keys'])
    assert [','.join(str(d) for d in v.shape) for v in net.state_dict().values()] == list(gold[prefix + '/shapes'])
    x, z = x.clone().requires_grad_(True), z.clone().requires_grad_(True)
    x0 = x.detach().clone()
    y = net(x, z)
    y.backward(W.seeded_normal(tuple(y.shape), dyseed))
    assert torch.equal(x.detach(), x0), 'the twin must not write into its input'
    _close(y.detach(), gold[prefix + '/out0'], 'output')
    _close(x.grad, gold[prefix + '/din0'], 'image gradient')
    _close(z.grad, gold[prefix + '/din1'], 'z gradient')
    stride, wmax = int(gold['stride']), max(float(np.abs(gold[k]).max()) for k in gold.files if k.startswith(prefix + '/dparam/full/'))
    seen = 0
    for k, p in net.named_parameters():
        g = p.grad.numpy()
        full, samp = '%s/dparam/full/%s' % (prefix, k), '%s/dparam/samp/%s' % (prefix, k)
        assert (full in gold.files) != (samp in gold.files), k
        want = gold[full] if full in gold.files else gold[samp]
        got = g if full in gold.files else g.reshape(-1)[::stride]
        if np.abs(want).max() < 1e-5 * wmax:         # a bias that the following affine-less InstanceNorm cancels: fp32 noise on both sides
            assert np.abs(got).max() < 1e-4 * wmax, k
        else:
            _close(got, want, 'd' + k)
            a = g.astype(np.float64)
            _close(np.array([np.abs(a).sum(), np.sqrt((a * a).sum())]), gold['%s/dparam/stat/%s' % (prefix, k)][1:], 'statistics of d' + k)
        seen += 1
    assert seen == len(list(net.parameters())) > 0
    nbuf = 0
    for k, b in net.named_buffers():
        want = gold['%s/buf/%s' % (prefix, k)]
        if k.endswith('num_batches_tracked'):
            assert int(b) == int(want) == (1 if prefix == 'U5b' else 0)      # InstanceNorm2d never counts its calls
        else:
            _close(b.numpy(), want, 'buffer ' + k)
        nbuf += 1
    assert nbuf > 0
    net.eval()
    with torch.no_grad():
        _close(net(x.detach(), z.detach()), gold[prefix + '/out_eval'], 'eval-mode output')


def test_skip_carries_the_leaky_relu_of_the_block_input():
    net = UnetGeneratorRef(3, 3, 1, 5, 8, 'instance')
    blk = net.model.model[1]
    x = W.seeded_normal((2, 8, 16, 16), 5)
    with torch.no_grad():
        out = blk(x.clone())
    assert torch.equal(out[:, :8], torch.nn.functional.leaky_relu(x, 0.2)) and not torch.equal(out[:, :8], x)


def test_recorded_counts_are_the_table(gold):
    got = {tuple(n.split(',')): tuple(int(v) for v in row) for n, row in zip(gold['counts/names'], gold['counts/values'])}
    assert {(w, int(nl), int(ngf), norm): v for (w, nl, ngf, norm), v in got.items()} == REFERENCE_COUNTS


@pytest.mark.parametrize('which,nl,ngf', [('unet', 5, 8), ('unet', 6, 8), ('unet', 7, 64), ('unet_256', 8, 64)])
@pytest.mark.parametrize('norm', ['instance', 'batch'])
def test_define_G_layout_and_counts(which, nl, ngf, norm):
    from pcgan_amd.models import networks
    kw = {'n_layers_G': nl} if which == 'unet' else {}
    net = networks.define_G(3, 3, 1, ngf, which, norm=norm, init_type='normal', **kw)
    assert isinstance(net, networks.UnetGenerator) and net.num_downs == nl
    twin = UnetGeneratorRef(3, 3, 1, nl, ngf, norm)
    sd, sd_t = net.state_dict(), twin.state_dict()
    assert list(sd.keys()) == list(sd_t.keys())
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in sd_t.values()]
    params, entries = REFERENCE_COUNTS[(which, nl, ngf, norm)]
    assert sum(p.numel() for p in net.parameters()) == params and len(sd) == entries
    net.load_state_dict(sd_t, strict=True)            # checkpoints interchange


def test_define_G_layout_is_the_recorded_one(gold):
    from pcgan_amd.models import networks
    for prefix, norm in (('U5i', 'instance'), ('U5b', 'batch')):
        sd = networks.define_G(3, 3, 1, 8, 'unet', norm=norm, init_type='normal', n_layers_G=5).state_dict()
        assert list(sd.keys()) == list(gold[prefix + '/keys'])
        assert [','.join(str(d) for d in v.shape) for v in sd.values()] == list(gold[prefix + '/shapes'])
    assert tuple(sd['model.model.1.model.5.weight'].shape) == (32, 8, 4, 4) and tuple(sd['model.model.3.weight'].shape) == (16, 3, 4, 4)


def test_unet_128_names_the_spelling_that_works():
    from pcgan_amd.models import networks
    with pytest.raises(NotImplementedError) as e:
        networks.define_G(3, 3, 1, 8, 'unet_128')
    assert '--which_model_netG unet' in str(e.value) and '--n_layers_G 7' in str(e.value)


@pytest.mark.parametrize('name', ['unet_128_input', 'unet_128_all', 'unet_256_input', 'unet_256_all', 'unet_all', 'gan_stability', 'mnist_fc'])
def test_other_generators_keep_their_refusal(name):
    from pcgan_amd.models import networks
    with pytest.raises(NotImplementedError, match='outside the MI355X hot path'):
        networks.define_G(3, 3, 1, 8, name)


def test_refusals_of_the_unet():
    from pcgan_amd.models import networks
    for which in ('unet', 'unet_256'):
        with pytest.raises(NotImplementedError, match='dropout'):
            networks.define_G(3, 3, 1, 8, which, norm='instance', dropout=0.5)
    with pytest.raises(ValueError, match='n_layers_G'):
        networks.define_G(3, 3, 1, 8, 'unet', norm='instance', n_layers_G=4)
    net = networks.define_G(3, 3, 1, 8, 'unet', norm='instance', init_type='normal', n_layers_G=5)
    for side in (48, 16):        # no multiple of 32; below 32 -- refused before anything is launched (these are CPU tensors)
        with pytest.raises(ValueError) as e:
            net(torch.zeros(1, 3, side, side), torch.zeros(1, 1, 1, 1))
        assert str(side) in str(e.value) and 'num_downs = 5' in str(e.value)
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 32, 48), torch.zeros(1, 1, 1, 1))


def test_skip_join_has_no_cpu_fallback():
    from pcgan_amd.hip import functional as F, ops
    from pcgan_amd.hip.lib import ACT_RELU
    a, b = torch.zeros(1, 2, 2, 2), torch.zeros(1, 3, 2, 2)
    with pytest.raises(RuntimeError, match='GPU tensors'):
        F.skip_join(a, b)
    with pytest.raises(RuntimeError, match='GPU tensors'):
        ops.skip_join_bwd(torch.zeros(1, 5, 2, 2), a, b, 2, ACT_RELU, ACT_RELU)


def test_library_refuses_bad_join_arguments():
    """argument validation happens before any launch, so it runs without a GPU"""
    from pcgan_amd.hip import lib
    h = lib.load()
    assert h.pcgan_skip_join_fwd(None, None, None, 1, 1, 1, 1, 0, 0, 0, None) != 0 and b'skip_join_fwd' in h.pcgan_last_error()
    assert h.pcgan_skip_join_fwd(16, 16, 16, 1, 1, 1, 1, 3, 0, 0, None) != 0 and b'PCGAN_ACT_RELU' in h.pcgan_last_error()
    assert h.pcgan_skip_join_fwd(16, 16, 16, 1, 0, 1, 1, 0, 0, 0, None) != 0 and b'positive' in h.pcgan_last_error()
    assert h.pcgan_skip_join_bwd(16, None, None, None, None, 1, 1, 1, 1, 0, 0, 0, None) != 0 and b'neither' in h.pcgan_last_error()
    assert h.pcgan_skip_join_bwd(16, None, None, 16, None, 1, 1, 1, 1, 1, 0, 0, None) != 0 and b'needs a' in h.pcgan_last_error()
    assert h.pcgan_skip_join_bwd(16, None, None, 16, None, 1, 1, 1, 1, 0, 0, 7, None) != 0 and b'dtype' in h.pcgan_last_error()
