"""CPU: the projection discriminator's host side and its oracle twin.

* define_D(..., 'n_layers_proj', ...) constructs with the reference's state_dict keys and shapes (tests/golden/projection_d.npz, recorded
  from the reference's own define_D by scripts/make_projection_golden.py) and loads the golden weights strictly.
* tests/projection_ref.py (the CPU twin the GPU tests judge with) reproduces the golden outputs and gradients: assert_close at 1e-5 in
  float32 -- the same arithmetic as the reference, only the summation order of the head differs.
* what the build refuses, and the argument validation of pcgan_proj_head_fwd / pcgan_proj_head_bwd, which happens before any launch and
  therefore runs without a GPU.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import projection_ref as P
from oracle import weights as W
from util_cmp import assert_close

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'projection_d.npz')
TOL = 1e-5


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def case(gold, prefix):
    """(define_D arguments, state dict, x, y, dy seed) of a golden configuration; P2's weights and inputs come from its recorded seeds"""
    nz, ndf, nl, sigm, bs, size, wseed, dyseed, sx, sy = (int(v) for v in gold[prefix + '/case'])
    norm = str(gold[prefix + '/norm'])
    keys = [str(k) for k in gold[prefix + '/keys']]
    shapes = [tuple(int(d) for d in str(s).split(',') if d) for s in gold[prefix + '/shapes']]
    if prefix + '/x' in gold.files:
        sd = {k: torch.from_numpy(gold['%s/sd/%s' % (prefix, k)]) for k in keys}
        x, y = torch.from_numpy(gold[prefix + '/x']), torch.from_numpy(gold[prefix + '/y'])
    else:
        like = {k: torch.empty(s, dtype=torch.int64 if k.endswith('num_batches_tracked') else torch.float32) for k, s in zip(keys, shapes)}
        sd = W.fill_state_dict(like, wseed)
        x, y = W.seeded_tensor((bs, 3, size, size), sx), W.seeded_normal((bs, nz, 1, 1), sy)
    return dict(nz=nz, ndf=ndf, nl=nl, sigm=bool(sigm), norm=norm, keys=keys, shapes=shapes, sd=sd, x=x, y=y, dyseed=dyseed)


@pytest.mark.parametrize('prefix', ['P1', 'P2'])
def test_define_D_builds_the_references_state_dict(gold, prefix):
    from pcgan_amd.models import networks
    c = case(gold, prefix)
    net = networks.define_D(3, c['nz'], c['ndf'], 'n_layers_proj', c['nl'], c['norm'], c['sigm'])
    assert isinstance(net, networks.NLayerProjectionDiscriminator)
    sd = net.state_dict()
    assert list(sd.keys()) == c['keys']
    assert [tuple(v.shape) for v in sd.values()] == c['shapes']
    C = c['ndf'] * min(2 ** c['nl'], 8)
    assert tuple(sd['psi.weight'].shape) == (1, C, 1, 1) and tuple(sd['psi.bias'].shape) == (1,)
    assert tuple(sd['l_y.weight'].shape) == (C, c['nz'], 1, 1) and tuple(sd['l_y.bias'].shape) == (C,)
    net.load_state_dict(c['sd'], strict=True)
    assert torch.equal(net.psi.weight, c['sd']['psi.weight']) and torch.equal(net.l_y.bias, c['sd']['l_y.bias'])
    twin = P.ProjectionDiscriminatorRef(3, c['nz'], c['ndf'], c['nl'], c['norm'], c['sigm'])
    assert list(twin.state_dict().keys()) == c['keys']


def test_init_weights_treats_the_head_as_the_convolutions_it_is():
    from pcgan_amd.models import networks
    torch.manual_seed(3)
    net = networks.define_D(3, 2, 16, 'n_layers_proj', 3, 'batch', False, 'normal')
    for m in (net.psi, net.l_y):
        assert float(m.bias.detach().abs().max()) == 0.0
    w = torch.cat([net.psi.weight.reshape(-1), net.l_y.weight.reshape(-1)])        # 128 + 256 draws of N(0, 0.02)
    assert 0.015 < float(w.std()) < 0.025 and abs(float(w.mean())) < 0.005
    assert all(p.requires_grad for p in net.parameters())


@pytest.mark.parametrize('prefix', ['P1', 'P2'])
def test_twin_reproduces_the_reference(gold, prefix):
    c = case(gold, prefix)
    twin = P.ProjectionDiscriminatorRef(3, c['nz'], c['ndf'], c['nl'], c['norm'], c['sigm'])
    twin.load_state_dict(c['sd'], strict=True)
    x, y = c['x'].clone().requires_grad_(True), c['y'].clone().requires_grad_(True)
    out = twin(x, y)
    assert tuple(out.shape) == (x.shape[0], 1, 3, 3)
    out.backward(W.seeded_normal(tuple(out.shape), c['dyseed']))
    assert_close(out, torch.from_numpy(gold[prefix + '/out0']), TOL, 'out')
    assert_close(y.grad, torch.from_numpy(gold[prefix + '/din1']), TOL, 'dy')
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


def test_twin_head_broadcasts_a_single_rating(gold):
    """y of batch 1 stands for every image (the reference's l_y(y) broadcasts in h * w_y)"""
    c = case(gold, 'P1')
    twin = P.ProjectionDiscriminatorRef(3, c['nz'], c['ndf'], c['nl'], c['norm'], c['sigm']).eval()
    twin.load_state_dict(c['sd'], strict=True)
    with torch.no_grad():
        one = twin(c['x'], c['y'][:1])
        rep = twin(c['x'], c['y'][:1].expand(4, 1, 1, 1))
    assert torch.equal(one, rep)


def test_refusals():
    from pcgan_amd.models import networks
    with pytest.raises(NotImplementedError, match='use_projection=False'):
        networks.define_D(3, 1, 8, 'n_layers_proj', 3, 'batch', True, use_projection=False)
    with pytest.raises(NotImplementedError, match='use_projection=False'):
        networks.NLayerProjectionDiscriminator(3, 1, 8, 3, proj=False)
    with pytest.raises(NotImplementedError, match='wsgan_cycle'):
        networks.define_D(3, 0, 8, 'n_layers_proj', 4, 'batch', True)           # wsgan_cycle's call: nz = 0
    for name in ('n_layers_multi', 'pixel', 'pyramid'):                          # the other refused names keep their message
        with pytest.raises(NotImplementedError, match='outside the MI355X hot path'):
            networks.define_D(3, 1, 8, name, 3, 'batch', True)


def test_module_and_wrappers_refuse_cpu_tensors():
    from pcgan_amd.hip import functional as HF, ops
    from pcgan_amd.models import networks
    net = networks.define_D(3, 1, 8, 'n_layers_proj', 3, 'batch', True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.zeros(2, 3, 32, 32), torch.zeros(2, 1, 1, 1))
    p, y = torch.zeros(2, 64, 3, 3), torch.zeros(2, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.proj_head_fwd(p, y, net.psi.weight, net.psi.bias, net.l_y.weight, net.l_y.bias, True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        HF.projection_head(p, y, net.psi.weight, net.psi.bias, net.l_y.weight, net.l_y.bias, True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.proj_head_bwd(torch.zeros(2, 1, 3, 3), torch.zeros(2, 64), y, net.psi.weight, net.psi.bias, net.l_y.weight, net.l_y.bias, (3, 3), True)
    with pytest.raises(RuntimeError, match='needs the rating'):
        net(torch.zeros(2, 3, 32, 32))


# ---- C-ABI argument validation (no launch) -------------------------------------------------------------------------------------------
def test_proj_head_fwd_refuses_bad_arguments_before_any_launch():
    from pcgan_amd.hip import lib
    h = lib.load()
    one = ctypes.c_void_p(4096)         # a non-null address that is never dereferenced: every call below fails its checks

    def call(B=4, C=64, HW=9, nz=1, By=4, dtype=lib.F32, p=one, y=one, psi_w=one, out=one, hh=one):
        return h.pcgan_proj_head_fwd(p, y, psi_w, one, one, one, out, hh, B, C, HW, nz, By, 0, dtype, None)
    assert call(p=None) != 0 and b'null p' in h.pcgan_last_error()
    assert call(y=None) != 0 and call(psi_w=None) != 0 and b'proj_head_fwd' in h.pcgan_last_error()
    assert call(out=None) != 0 and call(hh=None) != 0 and b'null out / h' in h.pcgan_last_error()
    for bad in (dict(nz=0), dict(nz=17), dict(nz=-1)):
        assert call(**bad) != 0 and b'nz' in h.pcgan_last_error(), bad
    for bad in (dict(By=2), dict(By=0), dict(By=5)):
        assert call(**bad) != 0 and b'By' in h.pcgan_last_error(), bad
    for bad in (dict(B=0, By=1), dict(C=0), dict(HW=0), dict(HW=(1 << 27) + 1), dict(B=1 << 16, C=1 << 15, By=1)):
        assert call(**bad) != 0 and b'proj_head_fwd' in h.pcgan_last_error(), bad
    assert call(dtype=7) != 0 and b'dtype' in h.pcgan_last_error()


def test_proj_head_bwd_refuses_bad_arguments_before_any_launch():
    from pcgan_amd.hip import lib
    h = lib.load()
    one = ctypes.c_void_p(4096)

    def call(B=4, C=64, HW=9, nz=1, By=4, dtype=lib.F32, g=one, hh=one, y=one, dp=one, dw=one, dy=one, ws=one, ws_bytes=1 << 20):
        return h.pcgan_proj_head_bwd(g, hh, y, one, one, one, one, dp, dw, dw, dw, dw, dy, ws, ws_bytes, B, C, HW, nz, By, 1, 0, dtype, None)
    assert call(g=None) != 0 and b'null g' in h.pcgan_last_error()
    assert call(hh=None) != 0 and call(y=None) != 0 and b'proj_head_bwd' in h.pcgan_last_error()
    assert call(dp=None, dw=None, dy=None) != 0 and b'nothing to compute' in h.pcgan_last_error()
    for bad in (dict(nz=0), dict(nz=17)):
        assert call(**bad) != 0 and b'nz' in h.pcgan_last_error(), bad
    for bad in (dict(By=3), dict(By=0)):
        assert call(**bad) != 0 and b'By' in h.pcgan_last_error(), bad
    assert call(C=0) != 0 and call(HW=0) != 0 and call(B=0, By=1) != 0 and call(dtype=-1) != 0
    assert call(ws=None) != 0 and b'workspace' in h.pcgan_last_error()
    assert call(ws_bytes=8) != 0 and b'workspace' in h.pcgan_last_error()
    assert call(ws=ctypes.c_void_p(4100)) != 0 and b'aligned' in h.pcgan_last_error()
    assert h.pcgan_proj_head_bwd_workspace_bytes(32, 3) == (64 + 96) * 8
    assert h.pcgan_proj_head_bwd_workspace_bytes(0, 1) == 0 and h.pcgan_proj_head_bwd_workspace_bytes(4, 0) == 0
    assert h.pcgan_proj_head_bwd_workspace_bytes(4, 17) == 0
