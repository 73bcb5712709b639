"""GPU: the U-Net generator on the HIP path (`--which_model_netG unet` / `unet_256`).

  1  the skip-join kernel (csrc/unet_join.hip) and its gradient are BIT-equal to torch.cat / relu / masking on the same device tensors;
  2  the U-Net's extreme layer shapes (one output pixel per image, windows that are mostly padding) on the existing convolution
     kernels, every element against float64 torch.nn.functional: forward and data gradient 2e-5 of the largest magnitude, weight
     gradient 1e-4 (the tolerances of tests/test_gpu_fullsize.py);
  3  whole nets against the vectors recorded from the reference (tests/golden/unet.npz) and the float64 twin (tests/unet_ref.py), with
     the two gradient checks of tests/test_gpu_nets.py: SHARP 5e-4 relative L2 against the twin replaying the HIP run's sign decisions,
     LOOSE 3e-2 against the twin's own;
  4  unet_256 at 256 x 256; 5 bf16 activations by the rule of tests/test_gpu_bf16.py; 6 the models; 7 the join beside matrix-pipe work.

Decisions: the HIP blocks fold every activation into the kernel above it, so the HIP tape reads, per block, [LeakyReLU of the block
input] ... [ReLU in the up-normalisation], and the join's ReLU on the skip half decides nothing new (relu(t) has t's sign).  The twin
applies ONE ReLU to the whole concatenation instead: the recorder below replaces the up-normalisation's entry by the mask of the whole
joined tensor."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from oracle import networks_ref as N
from oracle import weights as W
from test_gpu_nets import record_decisions, _assert_mostly_close, _run
from unet_ref import UnetGeneratorRef
from util_cmp import assert_close

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'unet.npz')
BF = torch.bfloat16


# ----------------------------------------------------------------------------------------------------------- 1. the join kernel
# (N, Ca, Cb, H, W): one-element planes on the element path; 2 x 2; odd run lengths; the 16-byte path; unequal halves on the 16-byte
# path (513 * 64 and 511 * 64 elements); 2^22 elements: more than the capped grid covers in one sweep, so the grid-stride loop wraps
JOIN_CASES = [(1, 3, 5, 1, 1), (3, 8, 8, 2, 2), (3, 16, 8, 3, 3), (2, 64, 64, 32, 32), (2, 513, 511, 8, 8), (2, 64, 64, 128, 128)]


def _join_inputs(case, dtype, dev):
    n, ca, cb, h, w = case
    g = torch.Generator().manual_seed(sum(case))
    ts = [torch.randn(n, c, h, w, generator=g) for c in (ca, cb, ca + cb)]
    for t in ts[:2]:
        t.view(-1)[::7] = 0.0            # exact zeros: relu(0) = 0 and a zero input passes no gradient
    return [t.to(dev).to(dtype) for t in ts]


@pytest.mark.parametrize('dtype', [torch.float32, BF], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', JOIN_CASES, ids=['x'.join(str(v) for v in c) for c in JOIN_CASES])
def test_skip_join_is_bit_exact(case, dtype, dev):
    from pcgan_amd.hip import ops
    from pcgan_amd.hip.lib import ACT_NONE, ACT_RELU
    a, b, dout = _join_inputs(case, dtype, dev)
    ca = case[1]
    zero = torch.zeros((), dtype=dtype, device=dev)
    for act_a in (ACT_NONE, ACT_RELU):
        for act_b in (ACT_NONE, ACT_RELU):
            out = ops.skip_join_fwd(a, b, act_a, act_b)
            want = torch.cat((torch.relu(a) if act_a else a, torch.relu(b) if act_b else b), 1)
            assert out.dtype == dtype and out.is_contiguous() and '_pcgan_amax' not in out.__dict__
            assert torch.equal(out, want), 'forward, act (%d, %d)' % (act_a, act_b)
            da_ref = torch.where(a > 0, dout[:, :ca], zero) if act_a else dout[:, :ca]
            db_ref = torch.where(b > 0, dout[:, ca:], zero) if act_b else dout[:, ca:]
            da, db = ops.skip_join_bwd(dout, a, b, ca, act_a, act_b)
            assert torch.equal(da, da_ref) and torch.equal(db, db_ref), 'backward, act (%d, %d)' % (act_a, act_b)
            da, none = ops.skip_join_bwd(dout, a, None, ca, act_a, act_b, True, False)      # db not wanted: b is not needed either
            assert none is None and torch.equal(da, da_ref), 'backward without db, act (%d, %d)' % (act_a, act_b)
            none, db = ops.skip_join_bwd(dout, None, b, ca, act_a, act_b, False, True)
            assert none is None and torch.equal(db, db_ref), 'backward without da, act (%d, %d)' % (act_a, act_b)


@pytest.mark.parametrize('dtype', [torch.float32, BF], ids=['fp32', 'bf16'])
def test_skip_join_autograd_and_unaligned_views(dtype, dev):
    """F.skip_join through autograd (an input that wants no gradient gets none), and operands that start 4 bytes into their
    allocation: run lengths fit the 16-byte path, the addresses do not -- the element path must take them, same bits"""
    from pcgan_amd.hip import functional as F
    from pcgan_amd.hip.lib import ACT_NONE, ACT_RELU
    case = (2, 4, 12, 4, 4)
    a, b, dout = _join_inputs(case, dtype, dev)
    a.requires_grad_(True)
    out = F.skip_join(a, b, ACT_RELU, ACT_NONE)
    assert torch.equal(out, torch.cat((torch.relu(a.detach()), b), 1))
    out.backward(dout)
    assert b.grad is None and torch.equal(a.grad, torch.where(a.detach() > 0, dout[:, :4], torch.zeros((), dtype=dtype, device=dev)))

    def shifted(t):
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
        off = 4 // t.element_size()
        v = buf[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v
    from pcgan_amd.hip import ops
    a2, b2, d2 = shifted(a.detach()), shifted(b), shifted(dout)
    assert torch.equal(ops.skip_join_fwd(a2, b2, ACT_RELU, ACT_RELU), torch.cat((torch.relu(a2), torch.relu(b2)), 1))
    da, db = ops.skip_join_bwd(d2, a2, b2, 4, ACT_RELU, ACT_NONE)
    assert torch.equal(da, torch.where(a2 > 0, d2[:, :4], torch.zeros((), dtype=dtype, device=dev))) and torch.equal(db, d2[:, 4:])


def test_skip_join_refuses_what_it_cannot_join(dev):
    from pcgan_amd.hip import ops
    from pcgan_amd.hip.lib import ACT_TANH
    a, b = torch.zeros(2, 3, 4, 4, device=dev), torch.zeros(2, 5, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match='ACT_NONE or ACT_RELU'):
        ops.skip_join_fwd(a, b, ACT_TANH, 0)
    with pytest.raises(RuntimeError, match='share a storage type'):
        ops.skip_join_fwd(a, b.to(BF))
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.skip_join_fwd(a, torch.zeros(2, 4, 4, 5, device=dev).permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match='joins'):
        ops.skip_join_fwd(a, torch.zeros(2, 5, 4, 3, device=dev))
    with pytest.raises(RuntimeError, match='ReLU mask'):
        ops.skip_join_bwd(torch.zeros(2, 8, 4, 4, device=dev), None, b, 3, 1, 0)


# ----------------------------------------------------------------------------------------------------------- 2. extreme layer shapes
# (name, transposed, Cin, Cout, input side, bias)
LAYER_CASES = [
    ('conv 512->512 2x2->1x1', False, 512, 512, 2, False),
    ('conv 512->512 4x4->2x2', False, 512, 512, 4, False),
    ('conv 4->64 64x64', False, 4, 64, 64, False),
    ('convT 512->512 1x1->2x2', True, 512, 512, 1, False),
    ('convT 1024->512 2x2->4x4', True, 1024, 512, 2, False),
    ('convT 128->3 32x32->64x64 bias', True, 128, 3, 32, True),
]


@pytest.mark.parametrize('n', [2, 3])
@pytest.mark.parametrize('case', LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_unet_layer_shapes_against_float64(case, n, dev):
    """the layers as the modules run them (packed weights, the route the host chooses): forward, data gradient, weight gradient and,
    where there is one, bias gradient -- every element"""
    from pcgan_amd.hip import nn as hnn
    import torch.nn.functional as TF
    name, transposed, cin, cout, side, bias = case
    g = torch.Generator().manual_seed(sum(map(ord, name)) + n)
    layer = (hnn.ConvTranspose2d if transposed else hnn.Conv2d)(cin, cout, kernel_size=4, stride=2, padding=1, bias=bias)
    fan = cin * 16
    with torch.no_grad():
        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * fan ** -0.5)
        if bias:
            layer.bias.copy_(torch.randn(cout, generator=g) * 0.1)
    x = torch.rand(n, cin, side, side, generator=g) * 2 - 1
    w64 = layer.weight.detach().double().requires_grad_(True)
    b64 = layer.bias.detach().double().requires_grad_(True) if bias else None
    x64 = x.double().requires_grad_(True)
    y64 = (TF.conv_transpose2d if transposed else TF.conv2d)(x64, w64, b64, stride=2, padding=1)
    dy = torch.randn(y64.shape, generator=g)
    y64.backward(dy.double())
    layer.to(dev)
    xd = x.to(dev).requires_grad_(True)
    y = layer(xd)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(y64.shape)
    assert_close(y, y64.detach(), 2e-5, name + ' forward')
    assert_close(xd.grad, x64.grad, 2e-5, name + ' data gradient')
    assert_close(layer.weight.grad, w64.grad, 1e-4, name + ' weight gradient')
    if bias:
        assert_close(layer.bias.grad, b64.grad, 1e-4, name + ' bias gradient')


# ----------------------------------------------------------------------------------------------------------- 3 / 4. whole nets
class record_unet_decisions(record_decisions):
    """test_gpu_nets.record_decisions plus the join: with the parent's ReLU folded in (act_a = ReLU on the skip half, the new half
    already passed through the ReLU of its up-normalisation, whose mask is the tape's last entry) the twin's single ReLU over the
    concatenation takes (joined > 0) = cat(t > 0, up > 0) in place of that entry"""

    def __enter__(self):
        super().__enter__()
        from pcgan_amd.hip import functional as F
        from pcgan_amd.hip.lib import ACT_NONE, ACT_RELU
        orig, rec = F.skip_join, self
        self.saved.append((F, 'skip_join', orig))

        def skip_join(a, b, act_a=ACT_NONE, act_b=ACT_NONE):
            y = orig(a, b, act_a, act_b)
            if act_a == ACT_RELU:
                assert act_b == ACT_NONE and tuple(rec.tape[-1].shape) == tuple(b.shape)
                up = rec.tape.pop()
                mask = (y.detach() > 0).cpu()
                assert torch.equal(mask[:, a.shape[1]:], up), 'the up half is not the ReLU output the tape recorded'
                rec.tape.append(mask)
            return y
        F.skip_join = skip_join
        return self


def _compare_unet(hip, twin, inputs, seed_dy, dev, gold=None, prefix=None, loose=True):
    """test_gpu_nets._compare for a U-Net: outputs at rtol 1e-4, SHARP gradients, LOOSE gradients (optional), running statistics;
    returns the float64 twin after ITS one train-mode pass"""
    hip.load_state_dict({k: v.clone() for k, v in twin.state_dict().items()})
    hip.to(dev)
    ref64 = twin.double()
    with record_unet_decisions() as rec:
        ys, dins, dps = _run(hip, [i.to(dev) for i in inputs], seed_dy)
    torch.cuda.synchronize()
    twin_r = copy.deepcopy(ref64)
    N.DecisionTape.replay = iter(rec.tape)
    try:
        ys_r, dins_r, dps_r = _run(twin_r, [i.double() for i in inputs], seed_dy)
        assert next(N.DecisionTape.replay, None) is None, 'the twin consumed fewer decisions than the HIP pass recorded'
    finally:
        N.DecisionTape.replay = None
    report = []
    report.append('out vs twin on HIP decisions %.2e' % assert_close(ys[0], ys_r[0], 1e-4, 'output vs fp64 twin on the HIP decisions'))
    for j, (a, b) in enumerate(zip(dins, dins_r)):
        _assert_mostly_close(a, b, 'SHARP din%d vs fp64 twin on the HIP decisions' % j, 5e-4)
    wmax = max(float(g.abs().max()) for g in dps_r.values())
    worst = 0.0
    for k, g in dps.items():
        gr = dps_r[k]
        if float(gr.abs().max()) < 1e-5 * wmax:        # a bias that the following affine-less InstanceNorm cancels
            assert float(g.abs().max()) < 1e-3 * wmax + 1e-6, 'd%s should be ~0' % k
            continue
        _assert_mostly_close(g, gr, 'SHARP d%s vs fp64 twin on the HIP decisions' % k, 5e-4)
        worst = max(worst, float((g.double().cpu() - gr).norm() / gr.norm()))
    report.append('worst SHARP parameter gradient %.2e' % worst)
    ys64, dins64, dps64 = _run(ref64, [i.double() for i in inputs], seed_dy)
    assert_close(ys[0], ys64[0], 1e-4, 'output vs fp64 twin')
    if gold is not None:
        assert_close(ys[0], torch.from_numpy(gold[prefix + '/out0']), 1e-4, 'output vs reference golden')
    if loose:
        for j, (a, b) in enumerate(zip(dins, dins64)):
            _assert_mostly_close(a, b, 'LOOSE din%d vs fp64 twin' % j)
            if gold is not None:
                _assert_mostly_close(a, torch.from_numpy(gold['%s/din%d' % (prefix, j)]), 'LOOSE din%d vs reference golden' % j)
        for k, g in dps.items():
            g64 = dps64[k]
            if float(g64.abs().max()) < 1e-5 * wmax:
                continue
            _assert_mostly_close(g, g64, 'LOOSE d' + k)
            if gold is not None and ('%s/dparam/full/%s' % (prefix, k)) in gold.files:
                _assert_mostly_close(g, torch.from_numpy(gold['%s/dparam/full/%s' % (prefix, k)]), 'LOOSE d%s vs reference golden' % k)
    hb = dict(hip.named_buffers())
    for k, b in ref64.named_buffers():
        if 'running' in k:
            assert_close(hb[k], b, 1e-5, 'buffer %s vs fp64 twin' % k)
            if gold is not None:
                assert_close(hb[k], torch.from_numpy(gold['%s/buf/%s' % (prefix, k)]), 1e-5, 'buffer %s vs reference golden' % k)
        else:
            assert int(hb[k]) == int(b), 'buffer ' + k
    print('unet parity: ' + '; '.join(report))
    return ref64


@pytest.mark.parametrize('norm', ['instance', 'batch'])
@pytest.mark.parametrize('nl,size', [(5, 32), (6, 64)])
def test_unet_against_reference_and_twin(nl, size, norm, dev):
    from pcgan_amd.models import networks
    gold = prefix = None
    if nl == 5:
        gold, prefix = np.load(GOLD), 'U5i' if norm == 'instance' else 'U5b'
        gnl, ngf, bs, gsize, wseed, dyseed, sx, sz = (int(v) for v in gold[prefix + '/case'])
        assert (gnl, ngf, bs, gsize, str(gold[prefix + '/norm'])) == (nl, 8, 3, size, norm)
    else:
        wseed, dyseed, sx, sz = 62 + (norm == 'batch'), 362, 162, 262
    twin = UnetGeneratorRef(3, 3, 1, nl, 8, norm)
    twin.load_state_dict(W.fill_state_dict(twin.state_dict(), wseed))
    hip = networks.define_G(3, 3, 1, 8, 'unet', norm=norm, init_type='normal', n_layers_G=nl)
    x, z = W.seeded_tensor((3, 3, size, size), sx), W.seeded_normal((3, 1, 1, 1), sz)
    ref64 = _compare_unet(hip, twin, [x, z], dyseed, dev, gold, prefix)
    # eval mode after that one train-mode pass: the running statistics normalise
    hip.eval()
    ref64.eval()
    with torch.no_grad():
        out = hip(x.to(dev), z.to(dev))
        assert_close(out, ref64(x.double(), z.double()), 1e-4, 'eval-mode output vs fp64 twin')
    if gold is not None:
        assert_close(out, torch.from_numpy(gold[prefix + '/out_eval']), 1e-4, 'eval-mode output vs reference golden')


def test_unet_256_against_twin(dev):
    """8 downsamplings at 256 x 256 (1 x 1 bottleneck), one image: forward and SHARP gradients"""
    from pcgan_amd.models import networks
    twin = UnetGeneratorRef(3, 3, 1, 8, 8, 'instance')
    twin.load_state_dict(W.fill_state_dict(twin.state_dict(), 64))
    hip = networks.define_G(3, 3, 1, 8, 'unet_256', norm='instance', init_type='normal')
    _compare_unet(hip, twin, [W.seeded_tensor((1, 3, 256, 256), 164), W.seeded_normal((1, 1, 1, 1), 264)], 364, dev, loose=False)


def test_unet_refuses_a_side_it_cannot_halve(dev):
    from pcgan_amd.models import networks
    hip = networks.define_G(3, 3, 1, 8, 'unet', norm='instance', init_type='normal', n_layers_G=5).to(dev)
    with pytest.raises(ValueError, match='48'):
        hip(torch.zeros(1, 3, 48, 48, device=dev), torch.zeros(1, 1, 1, 1, device=dev))
    with torch.no_grad():      # a larger multiple works: 64 x 64 through 5 downsamplings
        assert tuple(hip(torch.zeros(1, 3, 64, 64, device=dev), torch.zeros(1, 1, 1, 1, device=dev)).shape) == (1, 3, 64, 64)


# ----------------------------------------------------------------------------------------------------------- 5. bf16 activations
@pytest.mark.parametrize('norm', ['instance', 'batch'])
def test_unet_bf16_vs_fp32_twin(norm, dev):
    """the rule of tests/test_gpu_bf16.py::test_networks_bf16_vs_fp32_oracle: relative L2 error against the fp32 twin on fp32 inputs
    <= 2 x what the twin loses under stock PyTorch's CPU bf16 autocast + 1e-2 -- output, image gradient, parameter gradients overall
    and per tensor"""
    from pcgan_amd.models import networks
    from test_gpu_bf16 import autocast_bf16, _param_errors, _rel_l2, _run_net
    ref = UnetGeneratorRef(3, 3, 1, 5, 8, norm)
    ref.load_state_dict(W.fill_state_dict(ref.state_dict(), 65))
    hip = networks.define_G(3, 3, 1, 8, 'unet', norm=norm, init_type='normal', n_layers_G=5)
    hip.load_state_dict({k: v.clone() for k, v in ref.state_dict().items()})
    hip.to(dev)
    x, z = W.seeded_tensor((3, 3, 32, 32), 165), W.seeded_normal((3, 1, 1, 1), 265)
    dy = W.seeded_normal((3, 3, 32, 32), 365)
    sim = autocast_bf16(copy.deepcopy(ref))
    y_ref, din_ref, dp_ref = _run_net(ref, [x, z], dy)
    y_sim, din_sim, dp_sim = _run_net(sim, [x, z], dy)
    y, din, dp = _run_net(hip, [x.to(dev).to(BF), z.to(dev)], dy)
    torch.cuda.synchronize()
    assert y.dtype == BF and all(g.dtype == torch.float32 for g in dp.values())
    errs, overall = _param_errors(dp, dp_ref)
    errs_s, overall_s = _param_errors(dp_sim, dp_ref)
    rows = [('output', _rel_l2(y.float(), y_ref), _rel_l2(y_sim, y_ref)),
            ('image gradient', _rel_l2(din[0].float(), din_ref[0]), _rel_l2(din_sim[0], din_ref[0])),
            ('parameter gradients overall', overall, overall_s)] + [('d' + k, errs[k], errs_s[k]) for k in errs]
    print('unet bf16 parity, %s norm (relative L2 vs the fp32 twin: HIP bf16 / CPU bf16 autocast): ' % norm +
          '; '.join('%s %.3e / %.3e' % r for r in rows))
    for name, e_hip, e_sim in rows:
        assert e_hip <= 2 * e_sim + 1e-2, '%s: relative L2 %.3e, bf16 autocast of the twin loses %.3e' % (name, e_hip, e_sim)


# ----------------------------------------------------------------------------------------------------------- 6. the models
def _parse(argv):
    from pcgan_amd.options.train_options import TrainOptions
    old, sys.argv = sys.argv, argv
    try:
        return TrainOptions().parse()
    finally:
        sys.argv = old


def _damp_head(sd):
    """as oracle.weights.damp_generator_head: shrink the last ConvT so that tanh stays off its saturated range on random weights"""
    sd = dict(sd)
    sd['model.model.3.weight'] = sd['model.model.3.weight'] * 0.05
    return sd


def build_emb_unet(tmp_path, name, extra=()):
    """wsgan_emb through the option parser with --which_model_netG unet --n_layers_G 5 and the tiny encoder of tests/test_gpu_step.py"""
    from pcgan_amd.models import create_model
    e = N.SiameseFeatureRef(N.ResNetFeatureRef('resnet18', 0.0), 'avg', (32, 1), 1, 0.7, False, 0.0)
    e_path, ip_path = str(tmp_path / ('E_%s.pth' % name)), str(tmp_path / ('IP_%s.pth' % name))
    torch.save(W.fill_state_dict(e.state_dict(), 30), e_path)
    torch.save(W.fill_state_dict(N.AlexNetFeatureRef(3, 'None').state_dict(), 40), ip_path)
    opt = _parse(['train.py', '--dataroot', 'synthetic', '--model', 'wsgan_emb', '--name', name, '--checkpoints_dir', str(tmp_path),
                  '--gpu_ids', '0', '--which_model_netG', 'unet', '--n_layers_G', '5', '--which_model_netD', 'n_layers', '--n_layers_D', '3',
                  '--ngf', '8', '--ndf', '8', '--fineSize', '32', '--loadSize', '32', '--fineSize_E', '64', '--fineSize_IP', '64',
                  '--batchSize', '4', '--pretrained_model_path_E', e_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1',
                  '--embedding_bins', '[-1.0, 0.0, 1.5]', '--embedding_mean', '0.1', '--embedding_std', '0.8'] + list(extra))
    model = create_model(opt)
    model.setup(opt)
    model.netG.load_state_dict(_damp_head(W.fill_state_dict(model.netG.state_dict(), 19)))
    model.netD.load_state_dict(W.fill_state_dict(model.netD.state_dict(), 20))
    return model, opt


def _emb_run(tmp_path, name, steps=2):
    from oracle.make_golden import step_batch
    from pcgan_amd.models import networks
    torch.manual_seed(11)
    np.random.seed(11)
    model, opt = build_emb_unet(tmp_path, name)
    assert isinstance(model.netG, networks.UnetGenerator) and model.netG.num_downs == 5
    before = {k: v.detach().clone() for k, v in model.netG.state_dict().items()}
    calls = []
    hook = model.netG.register_forward_hook(lambda m, args, out: calls.append((args[0].detach().clone(), args[1].detach().clone(), out.detach().clone())))
    losses = []
    for it in range(steps):
        model.set_input(step_batch('default', it))
        model.optimize_parameters()
        losses.append(dict(model.get_current_losses()))
        if it == 0:
            hook.remove()
    torch.cuda.synchronize()
    state = {'G.' + k: v.detach().clone() for k, v in model.netG.state_dict().items()}
    state.update({'D.' + k: v.detach().clone() for k, v in model.netD.state_dict().items()})
    state['fake_B'], state['rec_A'] = model.fake_B.detach().clone(), model.rec_A.detach().clone()
    return model, before, calls, losses, state


def test_wsgan_emb_trains_a_unet(tmp_path, dev):
    from pcgan_amd.hip import ops
    assert ops.SIDE_STREAM and ops.BRANCH_STREAMS, 'this test is about the default four-stream schedule'
    model, before, calls, losses, state = _emb_run(tmp_path, 'u_a')
    for it, ls in enumerate(losses):
        assert ls and all(np.isfinite(v) for v in ls.values()), 'step %d: %r' % (it, ls)
    # the first generator call of the first step is fake_B = G(real_A, embedding_B), on the weights the model started from
    real_A, emb_B, fake_B = calls[0]
    twin = UnetGeneratorRef(3, 3, 1, 5, 8, 'instance')
    twin.load_state_dict({k: v.cpu() for k, v in before.items()})
    with torch.no_grad():
        want = twin.double()(real_A.double().cpu(), emb_B.double().cpu())
    assert_close(fake_B, want, 1e-4, 'fake_B vs the twin on the same weights and inputs')
    after = model.netG.state_dict()
    for k, p in model.netG.named_parameters():
        assert not torch.equal(before[k], after[k]), 'generator parameter %s did not move in two steps' % k
    # the same two steps from the same seed, side streams on: the same bits
    _, _, _, losses2, state2 = _emb_run(tmp_path, 'u_b')
    assert losses == losses2, (losses, losses2)
    for k in state:
        assert torch.equal(state[k], state2[k]), 'run-to-run difference in ' + k


def test_wsgan_emb_unet_bf16_step(tmp_path, dev):
    """--dtype bf16 with a U-Net generator: one step, finite losses, bf16 images, fp32 parameters that moved"""
    from oracle.make_golden import step_batch
    model, opt = build_emb_unet(tmp_path, 'u_bf16', ['--dtype', 'bf16'])
    before = {k: v.detach().clone() for k, v in model.netG.named_parameters()}
    model.set_input(step_batch('default', 0))
    model.optimize_parameters()
    torch.cuda.synchronize()
    assert model.fake_B.dtype == BF and all(np.isfinite(v) for v in model.get_current_losses().values())
    for k, p in model.netG.named_parameters():
        assert p.dtype == torch.float32 and not torch.equal(before[k], p.detach()), k


def test_wsgan_cycle_runs_a_unet(tmp_path, dev):
    """wsgan_cycle does not hand --n_layers_G to define_G (neither does the reference's): its `unet` is the 7-downsampling network, so
    the step runs at 128 x 128"""
    from pcgan_amd.models import create_model, networks
    base_path, ip_path = str(tmp_path / 'resnet18_base.pth'), str(tmp_path / 'IP.pth')
    torch.save(W.fill_state_dict(N.ResNetFeatureRef('resnet18').model.state_dict(), 31), base_path)
    torch.save(W.fill_state_dict(N.AlexNetFeatureRef(3, 'None').state_dict(), 40), ip_path)
    opt = _parse(['train.py', '--dataroot', 'synthetic', '--model', 'wsgan_cycle', '--name', 'u_cycle', '--checkpoints_dir', str(tmp_path),
                  '--gpu_ids', '0', '--which_model_netG', 'unet', '--which_model_netD', 'n_layers', '--n_layers_D', '3',
                  '--ngf', '8', '--ndf', '8', '--fineSize', '128', '--loadSize', '128', '--fineSize_E', '64', '--fineSize_IP', '64',
                  '--batchSize', '2', '--pretrained_model_path_E', base_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1',
                  '--attr_bins', '[10, 30, 50]', '--attr_mean', '35.0', '--attr_std', '20.0'])
    model = create_model(opt)
    model.setup(opt)
    assert isinstance(model.netG, networks.UnetGenerator) and model.netG.num_downs == 7
    model.netG.load_state_dict(_damp_head(W.fill_state_dict(model.netG.state_dict(), 19)))
    before = {k: v.detach().clone() for k, v in model.netG.named_parameters()}
    A, attr = W.seeded_tensor((2, 3, 128, 128), 700), (W.seeded_tensor((2, 1, 1, 1), 800) + 1.0) * 30.0
    model.set_input({'A': A, 'B_attr': attr, 'A_paths': ['a'] * 2, 'B_paths': ['b'] * 2})
    model.optimize_parameters()
    torch.cuda.synchronize()
    ls = model.get_current_losses()
    assert ls and all(np.isfinite(v) for v in ls.values()), ls
    assert tuple(model.fake_x.shape) == (2, 3, 128, 128)
    for k, p in model.netG.named_parameters():
        assert not torch.equal(before[k], p.detach()), 'generator parameter %s did not move' % k


# ----------------------------------------------------------------------------------------------------------- 7. company
def test_skip_join_is_bit_stable_beside_f16_mfma_kernels(dev):
    """the scheme of tests/test_gpu_concurrency.py: the join alone == the join while another stream runs f16-MFMA convolutions"""
    from pcgan_amd.hip import ops
    from pcgan_amd.hip.lib import ACT_NONE, ACT_RELU
    g = torch.Generator().manual_seed(4)
    nb = 16
    a, b, dout = (torch.randn(nb, c, 64, 64, generator=g).to(dev) for c in (64, 64, 128))
    a16, b16, dout16 = a.to(BF), b.to(BF), dout.to(BF)
    victims = {
        'join forward fp32': lambda: ops.skip_join_fwd(a, b, ACT_RELU, ACT_NONE),
        'join backward fp32': lambda: torch.cat(ops.skip_join_bwd(dout, a, b, 64, ACT_RELU, ACT_RELU), 1),
        'join forward bf16': lambda: ops.skip_join_fwd(a16, b16, ACT_RELU, ACT_NONE),
        'join backward bf16': lambda: torch.cat(ops.skip_join_bwd(dout16, a16, b16, 64, ACT_RELU, ACT_RELU), 1),
    }
    xr = torch.randn(nb, 256, 32, 32, generator=g).to(dev)
    wr = (torch.randn(256, 256, 3, 3, generator=g) * 0.05).to(dev)
    we = (torch.randn(128, 128, 3, 3, generator=g) * 0.05).to(dev)
    de = torch.randn(nb, 128, 28, 28, generator=g).to(dev)
    cr, ce = {}, {}

    def company():
        for _ in range(3):
            ops.conv2d_fwd(xr, wr, None, 1, 1, 1, pack_cache=cr)
            ops.conv2d_bwd_data(de, we, (28, 28), 1, 1, 0, pack_cache=ce)
            ops.conv2d_bwd_weight(xr, xr, (256, 256, 3, 3), 1, 1, 1)
    company()
    torch.cuda.synchronize()
    other = torch.cuda.Stream()
    failures = []
    for name, fn in victims.items():
        ref = fn().clone()
        torch.cuda.synchronize()
        bad = 0
        for _ in range(8):
            other.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(other):
                company()
            out = fn()
            torch.cuda.synchronize()
            bad += int(not torch.equal(out, ref))
        if bad:
            failures.append('%s: %d / 8 runs differ from the kernel running alone' % (name, bad))
    assert not failures, failures
