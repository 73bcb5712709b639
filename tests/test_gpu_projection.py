"""GPU parity of the projection discriminator (`--which_model_netD n_layers_proj`): the two head kernels, the module, the training step.

Kernels (pcgan_proj_head_fwd / pcgan_proj_head_bwd) against float64, by the project's rule (`_rule` of tests/test_gpu_inception.py): for each of
out, h, dp, the four parameter gradients and dy,  ||hip - f64|| <= 2 ||torch fp32 on the CPU - f64|| + 1e-30.  The kernels sum in float64
and round once, so they sit at or below stock fp32 everywhere.  With bf16 storage the float64 side is fed the bf16-rounded values; fp32
results keep the rule, bf16 results (out, dp) are within 2^-8 relative per element -- one bf16 rounding is 2^-9, doubled -- plus the fp32
term.  Bit-identical repeats, accumulation into seeded buffers, every optional output alone, and a tensor that is only element-aligned
(the element-wise path) giving the bits of the 16-byte aligned one.

Module: both golden configurations (tests/golden/projection_d.npz, from the reference's own define_D) and the float64 twin
(tests/projection_ref.py), by test_gpu_nets._compare -- the tolerances that file states for the n_layers discriminator: outputs 1e-4,
gradients SHARP at 5e-4 relative L2 against the twin replaying the HIP run's LeakyReLU decisions (floor 1e-6 where the true value is 0),
running statistics 1e-4.

Step: one optimize_parameters() of wsgan_emb (ngf = ndf = 8, resnet_2blocks, 32x32, batch 4) against oracle/step_ref.py's WSGANEmbStepRef
given the twin as netD, with tests/test_gpu_step.py's tolerances for its small configuration (losses 1e-4, images 2e-4, SHARP 5e-4, LOOSE
2e-1), also with --lr_E > 0 (dy flows into the encoder) and with --dtype bf16 against test_gpu_bf16.py's band (twice what PyTorch's CPU bf16
autocast of the oracle loses, + 2e-2 / 5e-2); then netD round-trips through BaseModel's save / load.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import projection_ref as P
from oracle import networks_ref as N
from oracle import step_ref as S
from oracle import weights as W
from oracle.make_golden import step_batch, LR_E_ARGS
from test_gpu_inception import _rule
from test_gpu_nets import _compare, record_decisions
from test_projection import GOLD, case
from util_cmp import assert_close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# (B, C, H, W, nz, By): one plane of one element; a block of planes ending inside a 16-byte piece (HW = 9); 7x7, 15x15 and 31x31 maps of
# the PatchGAN trunk at 128 / 256 / 512 pixel inputs (planes only element-aligned), more than one workgroup, C that is no multiple of the
# 8 planes a workgroup owns or of the 256 channels of a parameter-gradient workgroup, y broadcast over the batch, nz 1 .. 16
SHAPES = [(1, 8, 1, 1, 1, 1), (4, 64, 3, 3, 1, 4), (5, 512, 7, 7, 1, 5), (3, 40, 15, 15, 2, 3), (2, 512, 31, 31, 1, 1), (7, 136, 15, 15, 3, 7),
          (1, 1, 2, 3, 16, 1)]
NAMES = ('out', 'h', 'dp', 'dpsi_w', 'dpsi_b', 'dly_w', 'dly_b', 'dy')


def _inputs(shape, leaky, seed=0):
    B, C, H, Wd, nz, By = shape
    g = torch.Generator().manual_seed(1000 * seed + B * 7 + C)
    p = torch.randn(B, C, H, Wd, generator=g)
    if leaky:
        p = torch.nn.functional.leaky_relu(p, 0.2)
    y = torch.randn(By, nz, generator=g)
    psi_w = torch.randn(1, C, 1, 1, generator=g) * 0.1
    psi_b = torch.randn(1, generator=g) * 0.1
    ly_w = torch.randn(C, nz, 1, 1, generator=g) * 0.1
    ly_b = torch.randn(C, generator=g) * 0.1
    gout = torch.randn(B, 1, 3, 3, generator=g)
    return p, y, (psi_w, psi_b, ly_w, ly_b), gout


def _cpu(p, y, params, gout, sigmoid, dtype):
    """the head and its gradients on the CPU in `dtype`: the dict of NAMES"""
    p, y = p.detach().clone().to(dtype).requires_grad_(True), y.detach().clone().to(dtype).requires_grad_(True)      # never the caller's tensors
    ps = [t.detach().clone().to(dtype).requires_grad_(True) for t in params]
    out = P.head(p, y, *ps, sigmoid)
    out.backward(gout.to(dtype))
    h = p.detach().sum(dim=(2, 3))
    return dict(out=out.detach(), h=h, dp=p.grad, dpsi_w=ps[0].grad, dpsi_b=ps[1].grad, dly_w=ps[2].grad, dly_b=ps[3].grad, dy=y.grad)


def _hip(p, y, params, gout, sigmoid, dev, act=torch.float32, **kw):
    from pcgan_amd.hip import ops
    pd, yd, gd = p.to(dev).to(act), y.to(dev), gout.to(dev).to(act)
    ps = [t.to(dev) for t in params]
    out, h = ops.proj_head_fwd(pd, yd, *ps, sigmoid)
    res = ops.proj_head_bwd(gd, h, yd, *ps, tuple(p.shape[2:]), sigmoid, **kw)
    return dict(zip(NAMES, (out, h) + res))


@pytest.mark.parametrize('leaky', [True, False])
@pytest.mark.parametrize('sigmoid', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_head_kernels_against_float64(shape, sigmoid, leaky, dev):
    p, y, params, gout = _inputs(shape, leaky)
    r64, r32 = _cpu(p, y, params, gout, sigmoid, torch.float64), _cpu(p, y, params, gout, sigmoid, torch.float32)
    got = _hip(p, y, params, gout, sigmoid, dev)
    assert tuple(got['out'].shape) == (shape[0], 1, 3, 3) and got['out'].dtype == torch.float32
    for k in NAMES:
        assert got[k].shape == r64[k].shape, k
        _rule(got[k], r32[k], r64[k], '%s of %r' % (k, shape))
    again = _hip(p, y, params, gout, sigmoid, dev)
    for k in NAMES:
        assert torch.equal(got[k], again[k]), 'run-to-run difference in ' + k


@pytest.mark.parametrize('sigmoid', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_head_kernels_bf16_storage(shape, sigmoid, dev):
    p, y, params, gout = _inputs(shape, True, seed=1)
    p, gout = p.to(BF).float(), gout.to(BF).float()           # bf16 values: what the kernel reads
    r64, r32 = _cpu(p, y, params, gout, sigmoid, torch.float64), _cpu(p, y, params, gout, sigmoid, torch.float32)
    got = _hip(p, y, params, gout, sigmoid, dev, act=BF)
    assert got['out'].dtype == BF and got['dp'].dtype == BF and all(got[k].dtype == torch.float32 for k in NAMES[3:] + ('h',))
    for k in NAMES:
        if got[k].dtype == BF:
            a, b = got[k].double().cpu(), r64[k]
            fp32_term = 2 * float((r32[k].double() - b).abs().max())
            bad = (a - b).abs() > 2.0 ** -8 * b.abs() + fp32_term + 1e-30
            assert not bool(bad.any()), '%s of %r: %d elements outside 2^-8 relative, worst %.3e' % (
                k, shape, int(bad.sum()), float(((a - b).abs() / (b.abs() + 1e-30)).max()))
        else:
            _rule(got[k], r32[k], r64[k], 'bf16 storage: %s of %r' % (k, shape))


@pytest.mark.parametrize('shape', [(5, 512, 7, 7, 1, 5), (3, 40, 15, 15, 2, 3), (1, 1, 2, 3, 16, 1)])
def test_accumulate_and_optional_outputs(shape, dev):
    p, y, params, gout = _inputs(shape, True, seed=2)
    r64, r32 = _cpu(p, y, params, gout, True, torch.float64), _cpu(p, y, params, gout, True, torch.float32)
    full = _hip(p, y, params, gout, True, dev)
    g = torch.Generator().manual_seed(5)
    seeds = [torch.randn(t.shape, generator=g) for t in params]
    into = [s.clone().to(dev) for s in seeds]
    acc = _hip(p, y, params, gout, True, dev, into=into)
    for k, s, buf in zip(NAMES[3:7], seeds, into):
        assert acc[k].data_ptr() == buf.data_ptr()
        _rule(buf, s + r32[k], s.double() + r64[k], 'accumulated ' + k)
    assert torch.equal(acc['dp'], full['dp']) and torch.equal(acc['dy'], full['dy'])        # always overwritten
    # each optional output alone
    none = (False, False, False, False)
    alone = _hip(p, y, params, gout, True, dev, want_dp=True, want_params=none, want_dy=False)
    assert torch.equal(alone['dp'], full['dp']) and all(alone[k] is None for k in NAMES[3:])
    alone = _hip(p, y, params, gout, True, dev, want_dp=False, want_params=none, want_dy=True)
    assert torch.equal(alone['dy'], full['dy']) and all(alone[k] is None for k in NAMES[2:7])
    for i, k in enumerate(NAMES[3:7]):
        want = tuple(j == i for j in range(4))
        alone = _hip(p, y, params, gout, True, dev, want_dp=False, want_params=want, want_dy=False)
        assert torch.equal(alone[k], full[k]), k + ' alone'
        assert all(alone[o] is None for o in NAMES[2:] if o != k)


@pytest.mark.parametrize('act', [torch.float32, BF])
@pytest.mark.parametrize('shape', [(5, 512, 7, 7, 1, 5), (3, 40, 15, 15, 2, 3), (2, 512, 31, 31, 1, 1), (1, 1, 2, 3, 16, 1)])
def test_element_aligned_tensors_give_the_same_bits(shape, act, dev):
    """p (forward) and dp (backward) one element past a 16-byte boundary take the element-wise path: same bits as the 128-bit path"""
    from pcgan_amd.hip import lib, ops
    p, y, params, gout = _inputs(shape, True, seed=3)
    B, C, H, Wd, nz, By = shape
    n = p.numel()
    pd = p.to(dev).to(act)
    flat = torch.zeros(n + 16, dtype=act, device=dev)
    shifted = flat[1:1 + n].view(B, C, H, Wd)
    shifted.copy_(pd)
    assert pd.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == pd.element_size() and shifted.is_contiguous()
    yd, ps = y.to(dev), [t.to(dev) for t in params]
    out_a, h_a = ops.proj_head_fwd(pd, yd, *ps, True)
    out_s, h_s = ops.proj_head_fwd(shifted, yd, *ps, True)
    assert torch.equal(out_a, out_s) and torch.equal(h_a, h_s)
    gd = gout.to(dev).to(act)
    dp_a = ops.proj_head_bwd(gd, h_a, yd, *ps, (H, Wd), True, want_params=(False,) * 4, want_dy=False)[0]
    flat.fill_(7.0)
    handle = lib.load()
    nbytes = handle.pcgan_proj_head_bwd_workspace_bytes(B, nz)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    vp = ctypes.c_void_p
    st = handle.pcgan_proj_head_bwd(vp(gd.data_ptr()), vp(h_a.data_ptr()), vp(yd.data_ptr()), vp(ps[0].data_ptr()), vp(ps[1].data_ptr()),
                                    vp(ps[2].data_ptr()), vp(ps[3].data_ptr()), vp(shifted.data_ptr()), None, None, None, None, None,
                                    vp(ws.data_ptr()), nbytes, B, C, H * Wd, nz, By, 1, 0, lib.F32 if act == torch.float32 else lib.BF16,
                                    vp(torch.cuda.current_stream().cuda_stream))
    assert st == 0, handle.pcgan_last_error()
    torch.cuda.synchronize()
    assert torch.equal(shifted, dp_a)
    assert float(flat[0]) == 7.0 and bool((flat[1 + n:] == 7.0).all()), 'wrote outside dp'


def test_autograd_node_scales_with_the_upstream_factor(dev):
    """HF.projection_head under autograd: gradients reach p, y and the four parameters and follow a factor applied downstream"""
    from pcgan_amd.hip import functional as HF
    shape = (3, 40, 15, 15, 2, 3)
    p, y, params, gout = _inputs(shape, True, seed=4)
    r64 = _cpu(p, y, params, gout * 0.25, False, torch.float64)
    leaves = [t.to(dev).requires_grad_(True) for t in (p, y) + tuple(params)]
    out = HF.projection_head(*leaves, False)
    (out * 0.25).backward(gout.to(dev))
    for t, k in zip(leaves, ('dp', 'dy', 'dpsi_w', 'dpsi_b', 'dly_w', 'dly_b')):
        assert t.grad is not None and t.grad.shape == t.shape, k
        assert_close(t.grad, r64[k].reshape(t.shape), 1e-5, k)


@pytest.mark.parametrize('sigmoid', [True, False])
def test_autograd_node_adds_into_fused_gradient_buffers(sigmoid, dev):
    """parameters that FusedAdam owns (marked `_pcgan_fused_grad`, `.grad` a slice of its flat buffer): the backward pass ADDS the four
    gradients to those buffers and hands autograd None for them; p and y still receive theirs.  Rule of the kernel tests."""
    from pcgan_amd.hip import functional as HF
    shape = (3, 40, 15, 15, 2, 3)
    p, y, params, gout = _inputs(shape, True, seed=6)
    r64, r32 = _cpu(p, y, params, gout, sigmoid, torch.float64), _cpu(p, y, params, gout, sigmoid, torch.float32)
    g = torch.Generator().manual_seed(9)
    seeds = [torch.randn(t.shape, generator=g) for t in params]
    flat = torch.cat([s.reshape(-1) for s in seeds]).to(dev)            # one flat gradient buffer, the parameters' .grad are its slices
    pd, yd = p.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    leaves, o = [], 0
    for t in params:
        q = torch.nn.Parameter(t.to(dev))
        q.grad = flat[o:o + t.numel()].view(t.shape)
        q._pcgan_fused_grad = True
        o += t.numel()
        leaves.append(q)
    ptrs = [q.grad.data_ptr() for q in leaves]
    out = HF.projection_head(pd, yd, *leaves, sigmoid)
    out.backward(gout.to(dev))
    assert [q.grad.data_ptr() for q in leaves] == ptrs, 'autograd replaced a fused gradient buffer'
    for q, s, k in zip(leaves, seeds, NAMES[3:7]):
        _rule(q.grad, s + r32[k], s.double() + r64[k], 'fused ' + k)
    _rule(pd.grad, r32['dp'], r64['dp'], 'dp beside fused buffers')
    _rule(yd.grad, r32['dy'], r64['dy'], 'dy beside fused buffers')
    # a second pass adds once more (D runs several times per step).  The buffer has then been rounded to fp32 twice (2 * 2^-24 of its
    # value) on top of the fp32 plane sums every gradient is made of (2^-24 each): below 1e-6 of the largest element
    out = HF.projection_head(pd.detach().requires_grad_(True), yd.detach(), *leaves, sigmoid)
    out.backward(gout.to(dev))
    for q, s, k in zip(leaves, seeds, NAMES[3:7]):
        assert_close(q.grad, s.double() + 2 * r64[k], 1e-6, 'fused twice ' + k)


# ---- the module against the golden vectors and the twin -------------------------------------------------------------------------------
@pytest.mark.parametrize('prefix', ['P1', 'P2'])
def test_discriminator_matches_reference_and_twin(prefix, dev):
    from pcgan_amd.models import networks
    gold = np.load(GOLD)
    c = case(gold, prefix)
    ref = P.ProjectionDiscriminatorRef(3, c['nz'], c['ndf'], c['nl'], c['norm'], c['sigm'])
    ref.load_state_dict(c['sd'], strict=True)
    hip = networks.define_D(3, c['nz'], c['ndf'], 'n_layers_proj', c['nl'], c['norm'], c['sigm'], 'normal')
    _compare(hip, ref, [c['x'], c['y']], c['dyseed'], dev, gold, prefix)


# ---- the training step ---------------------------------------------------------------------------------------------------------------------
def _damp(sd):
    sd = dict(sd)
    sd['model.19.weight'] = sd['model.19.weight'] * 0.05       # the 2-block generator's last convolution (oracle/weights.py: damp_generator_head)
    return sd


def _damp_head(sd):
    """Step fixtures only, as oracle/weights.py damps the generator's head: fill_state_dict's He scale gives l_y.weight (fan-in nz = 1) a
    standard deviation of 1.4 and psi.weight 0.18, against the 0.02 of the reference's initialisation, and the head SUMS over C * H * W
    activations: the fp32 oracle's own sigmoid then returns exactly 1.0 for some cells (BCE's log clamp, a zero gradient), and bf16
    storage rounds a quarter of them to 1.0.  At 0.05 of that scale the logits stay in the sigmoid's working range."""
    sd = dict(sd)
    for k in ('psi.weight', 'l_y.weight'):
        sd[k] = sd[k] * 0.05
    return sd


def _oracle_step(lr_E=0.0):
    G = N.ResnetGeneratorRef(3, 3, 1, 8, 'instance', 2)
    G.load_state_dict(_damp(W.fill_state_dict(G.state_dict(), 19)))
    D = P.ProjectionDiscriminatorRef(3, 1, 8, 3, 'batch', True)
    D.load_state_dict(_damp_head(W.fill_state_dict(D.state_dict(), 20)))
    E = N.SiameseFeatureRef(N.ResNetFeatureRef('resnet18'), 'avg', (32, 1), 1, 0.7, False)
    E.load_state_dict(W.fill_state_dict(E.state_dict(), 30))
    IP = N.AlexNetFeatureRef(3, 'None')
    IP.load_state_dict(W.fill_state_dict(IP.state_dict(), 40))
    return S.WSGANEmbStepRef(G, D, E, IP, fineSize_E=64, fineSize_IP=64, embedding_mean=[0.1], embedding_std=[0.8], noisy=False,
                             bayesian=False, noisy_var_type='', bnn_T=10, lambda_L1=0.0, lambda_IP=1.0, lambda_z=1.0, lambda_A_GAN=0.0,
                             use_real_A=False, detach_fake_B=False, lr_E=lr_E)


def _hip_step(tmp_path, extra):
    from test_gpu_step import build_hip_model
    import oracle.weights as OW
    orig = OW.damp_generator_head
    OW.damp_generator_head = _damp                      # build_hip_model damps the 9-block generator's head by its key
    try:
        model, opt = build_hip_model('default', tmp_path, ['--which_model_netG', 'resnet_2blocks', '--which_model_netD', 'n_layers_proj']
                                     + list(extra))
    finally:
        OW.damp_generator_head = orig
    model.netD.load_state_dict(_damp_head(W.fill_state_dict(model.netD.state_dict(), 20)))
    return model, opt


def _oracle_set_input(m, dtype=torch.float32):
    b = step_batch('default', 0)
    m.set_input(b['A'].to(dtype), b['B'].to(dtype), [int(v) for v in b['label']])


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize('lr_E', [False, True])
def test_step_matches_the_oracle(lr_E, tmp_path, dev):
    from pcgan_amd.hip import ops
    from pcgan_amd.models import networks
    extra = LR_E_ARGS if lr_E else []
    model, opt = _hip_step(tmp_path, extra)
    assert isinstance(model.netD, networks.NLayerProjectionDiscriminator) and (opt.lr_E > 0) == lr_E
    lr = float(LR_E_ARGS[1]) if lr_E else 0.0
    oracle, twin = _oracle_step(lr), _oracle_step(lr)
    for net in (twin.netG, twin.netD, twin.netE, twin.netIP):
        net.double()
    grabbed = []
    optims = [('G', model.optimizer_G, model.netG)] + ([('E', model.optimizer_E, model.netE)] if lr_E else []) + [('D', model.optimizer_D, model.netD)]
    for tag, optim, net in optims:
        def stepper(orig=optim.step, tag=tag, net=net):
            grabbed.append((tag, {k: q.grad.detach().clone() for k, q in net.named_parameters() if q.grad is not None}))
            return orig()
        optim.step = stepper
    if lr_E:
        # between update_G_and_E's two phases the HIP model and the twin take the oracle's stepped G / E weights (tests/test_gpu_step.py:
        # Adam turns noise-level gradients into +-lr moves, the second phase is compared on identical weights)
        stepped = {}

        def snap(orig=oracle.backward_G_alone):
            stepped['G'] = {k: v.detach().clone() for k, v in oracle.netG.named_parameters()}
            stepped['E'] = {k: v.detach().clone() for k, v in oracle.netE.named_parameters()}
            return orig()
        oracle.backward_G_alone = snap

        def align(nets, orig, dtype):
            def run():
                with torch.no_grad():
                    for tag, net in nets:
                        for k, q in net.named_parameters():
                            q.data.copy_(stepped[tag][k].to(dtype))
                ops.invalidate_packed_weights()
                return orig()
            return run
        model.backward_G_alone = align((('G', model.netG), ('E', model.netE)), model.backward_G_alone, torch.float32)
        twin.backward_G_alone = align((('G', twin.netG), ('E', twin.netE)), twin.backward_G_alone, torch.float64)
    torch.manual_seed(1234)
    _oracle_set_input(oracle)
    oracle.optimize_parameters()
    with record_decisions({'G': model.netG, 'D': model.netD, 'E': model.netE, 'IP': model.netIP}) as rec:
        model.set_input(step_batch('default', 0))
        model.optimize_parameters()
    assert [t for t, _ in grabbed] == (['G', 'E', 'G', 'D'] if lr_E else ['G', 'D'])
    queues = {k: iter(v) for k, v in rec.tapes.items()}
    for name, tnet in (('G', twin.netG), ('D', twin.netD), ('E', twin.netE), ('IP', twin.netIP)):
        N.DecisionTape.bind(tnet, queues[name])
    try:
        _oracle_set_input(twin, torch.float64)
        twin.optimize_parameters()
        for name, q in queues.items():
            assert next(q, None) is None, 'the twin consumed fewer %s decisions than the HIP step recorded' % name
    finally:
        for tnet in (twin.netG, twin.netD, twin.netE, twin.netIP):
            N.DecisionTape.bind(tnet, None)
    got, ol = model.get_current_losses(), oracle.losses()
    for n, v in ol.items():
        assert abs(got[n] - v) <= 1e-4 * max(1.0, abs(v)), 'loss %s: hip %r vs oracle %r' % (n, got[n], v)
    for k in ('fake_B', 'rec_A', 'embedding_A', 'embedding_B', 'y_A', 'y_B'):
        assert_close(getattr(model, k), getattr(oracle, k), 2e-4, '%s vs oracle' % k)
    if lr_E:
        sets = (('G', grabbed[0][1], oracle.grads_G, twin.grads_G), ('E', grabbed[1][1], oracle.grads_E, twin.grads_E),
                ('G_alone', grabbed[2][1], oracle.grads_G_alone, twin.grads_G_alone), ('D', grabbed[3][1], oracle.grads_D, twin.grads_D))
    else:
        sets = (('G', grabbed[0][1], oracle.grads_G, twin.grads_G), ('D', grabbed[1][1], oracle.grads_D, twin.grads_D))
    nzc = opt.embedding_nc
    for tag, hgrads, ograds, tgrads in sets:
        checked = 0
        for k, og in ograds.items():
            if og is None:
                continue
            hg, g64 = hgrads[k], tgrads[k]
            if tag.startswith('G') and ((k.endswith('.bias') and k != 'model.19.bias') or k == 'model.1.weight'):
                # in front of an affine-less InstanceNorm (bias; the constant rating plane's filter slice): true gradient 0, noise only
                wmax = float(ograds[k[:-4] + 'weight'].abs().max()) if k.endswith('.bias') else float(og.abs().max())
                noise = hg if k.endswith('.bias') else hg[:, -nzc:]
                assert float(noise.abs().max()) <= 1e-3 * wmax + 1e-6, 'grad %s %s should be ~0' % (tag, k)
                if k.endswith('.bias'):
                    continue
                hg, og, g64 = hg[:, :-nzc], og[:, :-nzc], g64[:, :-nzc]
            if float(g64.abs().max()) < 1e-9:
                continue
            e_hip = _rel_l2(hg, g64)
            assert e_hip <= 5e-4, 'grad %s %s: SHARP rel-L2 vs the fp64 twin on the HIP decisions %.3e' % (tag, k, e_hip)
            assert _rel_l2(hg, og) <= 2e-1, 'grad %s %s: LOOSE vs the fp32 oracle' % (tag, k)
            checked += 1
        assert checked > 0, tag
        if tag == 'D':
            assert {'psi.weight', 'psi.bias', 'l_y.weight', 'l_y.bias'} <= set(hgrads), sorted(hgrads)
    # state after the step, as tests/test_gpu_step.py holds it: Adam moves every weight by about lr per optimizer step whatever |g| is, so
    # weights are only held to 2.5 lr per step taken (G and E step twice in the --lr_E form); the plain form uses that file's 5e-4 / 1e-6
    # for the running statistics, the --lr_E form its 1e-3 / 1e-5 and compares the encoder as well
    nets = [('G', model.netG, oracle.netG), ('D', model.netD, oracle.netD)] + ([('E', model.netE, oracle.netE)] if lr_E else [])
    rtol, atol, steps = (1e-3, 1e-5, 2) if lr_E else (5e-4, 1e-6, 1)
    for tag, hnet, onet in nets:
        osd = onet.state_dict()
        for k, v in hnet.state_dict().items():
            if k.endswith('num_batches_tracked'):
                assert int(v) == int(osd[k]), k
            elif 'running' in k:
                assert_close(v, osd[k], rtol, '%s %s after step' % (tag, k), atol=atol)
            elif v.dim() > 1:
                rate = opt.lr_E if tag == 'E' else opt.lr
                assert float((v.cpu() - osd[k]).abs().max()) <= 2.5 * rate * steps, '%s %s after step' % (tag, k)
    # checkpoint round trip of the discriminator through BaseModel
    model.save_networks('latest')
    live = {k: v.detach().clone() for k, v in model.netD.state_dict().items()}
    sd = torch.load(os.path.join(model.save_dir, 'latest_net_D.pth'), map_location='cpu')
    assert list(sd.keys()) == list(live.keys())
    for k in sd:
        assert torch.equal(sd[k], live[k].cpu()), k
    with torch.no_grad():
        model.netD.psi.weight.add_(1.0)
    model.load_networks('latest')
    for k, v in model.netD.state_dict().items():
        assert torch.equal(v, live[k]), 'after load: ' + k


def test_step_bf16_vs_fp32_oracle(tmp_path, dev):
    from test_gpu_bf16 import autocast_bf16, _param_errors
    from test_gpu_step import _grab_grads
    model, opt = _hip_step(tmp_path, ['--dtype', 'bf16'])
    assert model.act_dtype == BF
    oracle, sim = _oracle_step(), _oracle_step()
    for net in (sim.netG, sim.netD, sim.netE, sim.netIP):
        autocast_bf16(net)
    grabbed = _grab_grads(model)
    for o in (oracle, sim):
        _oracle_set_input(o)
        o.optimize_parameters()
    model.set_input(step_batch('default', 0))
    model.optimize_parameters()
    assert model.fake_B.dtype == BF
    got, want, lsim = model.get_current_losses(), oracle.losses(), sim.losses()
    report = ['losses (hip / autocast / fp32) ' + ', '.join('%s %.5f/%.5f/%.5f' % (k, got[k], lsim[k], v) for k, v in want.items())]
    for k, v in want.items():
        assert abs(got[k] - v) <= 2 * abs(lsim[k] - v) + 2e-2 * abs(v) + 1e-3, \
            'bf16 step loss %s: %.6g vs fp32 oracle %.6g (bf16 autocast of the oracle: %.6g)' % (k, got[k], v, lsim[k])
    for k in ('fake_B', 'rec_A', 'y_A', 'y_B'):
        e_hip, e_sim = _rel_l2(getattr(model, k).float(), getattr(oracle, k)), _rel_l2(getattr(sim, k), getattr(oracle, k))
        report.append('%s %.3e / %.3e' % (k, e_hip, e_sim))
        assert e_hip <= 2 * e_sim + 2e-2, 'bf16 step %s: relative L2 %.3e (autocast %.3e)' % (k, e_hip, e_sim)
    for tag, ograds, sgrads in (('G', oracle.grads_G, sim.grads_G), ('D', oracle.grads_D, sim.grads_D)):
        hg, og, sg = dict(grabbed[tag]), dict(ograds), dict(sgrads)
        if tag == 'G':      # the rating channel's filter slice has a true gradient of 0
            hg['model.1.weight'], og['model.1.weight'], sg['model.1.weight'] = (t[:, :-1] for t in (hg['model.1.weight'], og['model.1.weight'], sg['model.1.weight']))
        assert all(g.dtype == torch.float32 for g in hg.values()), 'parameter gradients stay fp32'
        errs, overall = _param_errors(hg, og)
        errs_s, overall_s = _param_errors(sg, og)
        worst = max(errs, key=errs.get)
        report.append('grad%s overall %.3e / %.3e, worst %s %.3e / %.3e' % (tag, overall, overall_s, worst, errs[worst], errs_s[worst]))
        assert overall <= 2 * overall_s + 2e-2, 'bf16 step grad%s overall %.3e (autocast %.3e)' % (tag, overall, overall_s)
        for k in errs:
            if errs_s[k] > 0.2:
                assert errs[k] <= 2.0, 'bf16 step grad%s %s: relative L2 %.3e (autocast %.3e)' % (tag, k, errs[k], errs_s[k])
                continue
            assert errs[k] <= 2 * errs_s[k] + 5e-2, 'bf16 step grad%s %s: relative L2 %.3e (autocast %.3e)' % (tag, k, errs[k], errs_s[k])
    print('bf16 parity projection step (HIP bf16 path / PyTorch CPU bf16 autocast of the oracle nets, relative L2 vs the fp32 oracle): ' + '; '.join(report))
