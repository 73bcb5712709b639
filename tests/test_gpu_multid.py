"""GPU parity of the multi-scale PatchGAN discriminator (`--which_model_netD n_layers_multi --num_Ds N`): the module and the wsgan_cycle step.

Module: the golden configurations M1 (two scales, batch norm, sigmoid) and M2 (three scales, instance norm, widths 16 / 8 / 2) of
tests/golden/multi_d.npz -- recorded from the reference's own define_D -- and the float64 twin (tests/multid_ref.py), by
test_gpu_nets._compare with the tolerances that file states for the n_layers discriminator: outputs 1e-4, gradients SHARP at 5e-4 relative
L2 against the twin replaying the HIP run's LeakyReLU decisions, floor 1e-6 where the true value is 0 (here: the bias of EVERY inner
convolution, which sits in front of a train-mode norm), running statistics 1e-4.  M1 again with bf16 storage against test_gpu_bf16.py's band
for whole networks: at most twice what PyTorch's CPU bf16 autocast of the twin loses, + 1e-2, per output, for the image gradient, for the
parameter gradients overall and per tensor; running statistics 2e-2 (+ 1e-3).  One scale (M0) returns a tensor.

Step: one optimize_parameters() of wsgan_cycle built through the unchanged option parser with --which_model_netD n_layers_multi --num_Ds 2
--n_layers_D 2 --ndf 8 --ngf 8 --fineSize 32 --batchSize 4 against tests/golden/cycle_multid_step.npz (the reference's own step) and the
float64 step twin, with tests/test_gpu_cycle.py's tolerances and structure: losses, images, every gradient tensor of G, D and E, the state after
the step; then netD round-trips through BaseModel's save / load with identical keys.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import multid_ref as M
from oracle import networks_ref as N
from oracle import weights as W
from test_cycle_oracle_golden import cycle_inputs
from test_gpu_bf16 import _param_errors, _rel_l2
from test_gpu_nets import _compare
from test_multid import GOLD, STEP_GOLD, case, product_of, twin_of
from util_cmp import assert_close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.mark.parametrize('prefix', ['M1', 'M2'])
def test_discriminator_matches_reference_and_twin(prefix, dev):
    gold = np.load(GOLD)
    c = case(gold, prefix)
    _compare(product_of(c), twin_of(c), [c['x']], c['dyseed'], dev, gold, prefix)


def test_one_scale_returns_a_tensor(dev):
    gold = np.load(GOLD)
    c = case(gold, 'M0')
    net = product_of(c)
    net.load_state_dict(c['sd'], strict=True)
    net.to(dev)
    out = net(c['x'].to(dev))
    assert isinstance(out, torch.Tensor)
    assert_close(out, torch.from_numpy(gold['M0/out0']), 1e-4, 'one scale vs reference golden')


def _run(net, x, dys):
    x = x.clone().requires_grad_(True)
    ys = net(x)
    torch.autograd.backward(list(ys), [d.to(device=y.device, dtype=y.dtype) for d, y in zip(dys, ys)])
    return ys, x.grad, {k: p.grad for k, p in net.named_parameters()}


def test_discriminator_bf16_vs_fp32_twin(dev):
    gold = np.load(GOLD)
    c = case(gold, 'M1')
    ref, hip = twin_of(c), product_of(c)
    hip.load_state_dict(c['sd'], strict=True)
    hip.to(dev)
    sim = copy.deepcopy(ref)
    plain = sim.forward

    def autocast(x):        # test_gpu_bf16.autocast_bf16 for a net that returns a list
        with torch.autocast('cpu', dtype=BF):
            ys = plain(x)
        return [y.float() for y in ys]
    sim.forward = autocast
    dys = [W.seeded_normal(tuple(gold['M1/out%d' % j].shape), c['dyseed'] + j) for j in range(c['num'])]
    y_ref, din_ref, dp_ref = _run(ref, c['x'], dys)
    y_sim, din_sim, dp_sim = _run(sim, c['x'], dys)
    y, din, dp = _run(hip, c['x'].to(dev).to(BF), dys)
    assert all(t.dtype == BF for t in y) and din.dtype == BF and all(g.dtype == torch.float32 for g in dp.values())
    errs, overall = _param_errors(dp, dp_ref)
    errs_s, overall_s = _param_errors(dp_sim, dp_ref)
    rows = [('output %d' % j, _rel_l2(a.float(), b), _rel_l2(s, b)) for j, (a, b, s) in enumerate(zip(y, y_ref, y_sim))]
    rows += [('input gradient', _rel_l2(din.float(), din_ref), _rel_l2(din_sim, din_ref)), ('parameter gradients overall', overall, overall_s)]
    rows += [('d' + k, errs[k], errs_s[k]) for k in errs]
    print('bf16 parity multi-scale D (relative L2 vs the fp32 twin: HIP bf16 path / PyTorch CPU bf16 autocast of the twin): ' +
          '; '.join('%s %.3e / %.3e' % r for r in rows))
    for name, e_hip, e_sim in rows:
        assert e_hip <= 2 * e_sim + 1e-2, '%s: relative L2 %.3e, bf16 autocast of the twin loses %.3e' % (name, e_hip, e_sim)
    hb = dict(hip.named_buffers())
    for k, b in ref.named_buffers():
        if 'running' in k:
            assert_close(hb[k], b, 2e-2, 'buffer ' + k, atol=1e-3)


# ---- the training step ---------------------------------------------------------------------------------------------------------------------
def build_hip_cycle_multid(tmp_path):
    """tests/test_gpu_cycle.py: build_hip_cycle with the multi-scale discriminator's flags"""
    from pcgan_amd.options.train_options import TrainOptions
    from pcgan_amd.models import create_model
    base = N.ResNetFeatureRef('resnet18')
    base_path = str(tmp_path / 'resnet18_base.pth')
    torch.save(W.fill_state_dict(base.model.state_dict(), 31), base_path)
    ip = N.AlexNetFeatureRef(3, 'None')
    ip_path = str(tmp_path / 'IP.pth')
    torch.save(W.fill_state_dict(ip.state_dict(), 40), ip_path)
    argv = ['train.py', '--dataroot', 'synthetic', '--model', 'wsgan_cycle', '--name', 'g_cycle_multid', '--checkpoints_dir', str(tmp_path),
            '--gpu_ids', '0', '--which_model_netG', 'resnet_9blocks', '--loadSize', '32', '--fineSize_E', '64', '--fineSize_IP', '64',
            '--pretrained_model_path_E', base_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1',
            '--attr_bins', '[10, 30, 50]', '--attr_mean', '35.0', '--attr_std', '20.0',
            '--which_model_netD', 'n_layers_multi', '--num_Ds', '2', '--n_layers_D', '2', '--ndf', '8', '--ngf', '8', '--fineSize', '32',
            '--batchSize', '4']
    old, sys.argv = sys.argv, argv
    try:
        opt = TrainOptions().parse()
    finally:
        sys.argv = old
    model = create_model(opt)
    model.setup(opt)
    model.netG.load_state_dict(W.damp_generator_head(W.fill_state_dict(model.netG.state_dict(), 19)))
    model.netD.load_state_dict(W.fill_state_dict(model.netD.state_dict(), 20))
    esd = model.netE.state_dict()
    filled = W.fill_state_dict({k: v.cpu() for k, v in esd.items()}, 33)
    model.netE.load_state_dict({k: (filled[k] if k.startswith('cnn') else v) for k, v in esd.items()})
    return model, opt


def test_cycle_step_matches_reference_and_twin(tmp_path, dev):
    from pcgan_amd.models import networks
    gold = np.load(STEP_GOLD)
    names = list(gold['loss_names'])
    model, opt = build_hip_cycle_multid(tmp_path)
    assert isinstance(model.netD, networks.D_NLayersMulti) and model.netD.num_D == 2
    assert model.loss_names == names and model.model_names == ['G', 'E', 'D']
    assert list(model.netD.state_dict().keys()) == [str(k) for k in gold['netD_keys']]
    oracle = M.build_cycle_multid_oracle()
    twin = M.build_cycle_multid_oracle(torch.float64)
    grabbed = {}
    for tag, optim, net in (('G', model.optimizer_G, model.netG), ('D', model.optimizer_D, model.netD), ('E', model.optimizer_E, model.netE)):
        orig = optim.step

        def stepper(orig=orig, tag=tag, net=net):
            grabbed[tag] = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
            return orig()
        optim.step = stepper

    A, attr = cycle_inputs(0)
    oracle.set_input(A, attr)
    oracle.optimize_parameters()
    twin.set_input(A.double(), attr.double())
    twin.optimize_parameters()
    model.set_input({'A': A, 'B_attr': attr, 'A_paths': ['a'] * 4, 'B_paths': ['b'] * 4})
    model.optimize_parameters()

    got = model.get_current_losses()
    for i, n in enumerate(names):
        ref = gold['it0/losses'][i]
        assert abs(got[n] - ref) <= 2e-4 * max(1.0, abs(ref)), 'loss %s: hip %.7g reference %.7g' % (n, got[n], ref)
    for k in ('fake_x', 'rec_x', 'fake_y', 'rec_y', 'real_y'):
        assert_close(getattr(model, k), torch.from_numpy(gold['it0/' + k]), 2e-4, k + ' vs reference')
    for tag in ('G', 'D', 'E'):
        for k, g64 in twin.grads[tag].items():
            if g64 is None:
                continue
            hip, ref32 = grabbed[tag][k], oracle.grads[tag][k]
            scale = float(g64.norm())
            e_hip = float((hip.double().cpu() - g64).norm())
            e_ref = float((ref32.double() - g64).norm())
            assert e_hip <= 2 * e_ref + 3e-2 * scale + 1e-6, \
                'grad%s %s: |hip-g64| %.3e, |ref32-g64| %.3e, |g64| %.3e' % (tag, k, e_hip, e_ref, scale)
            st = gold['it0/grad%s/stat/%s' % (tag, k)]
            assert abs(float(hip.double().norm()) - st[2]) <= 3e-2 * st[2] + 1e-4, 'grad%s %s norm vs reference' % (tag, k)   # (+1e-4: tensors whose true gradient is 0 carry only noise)
    # parameters after the three Adam steps (tests/test_gpu_cycle.py: the first Adam step moves every parameter by lr * sign(gradient);
    # where the true gradient is 0 the sign is noise, so each entry may differ from the reference by up to 2 lr)
    for tag, net in (('G', model.netG), ('D', model.netD), ('E', model.netE)):
        for k, v in net.state_dict().items():
            ref = gold['it0/after%s/%s' % (tag, k)]
            slack = 2e-3 * (ref[1] + 1e-3) + 2.02 * opt.lr * v.numel()
            assert abs(float(v.double().abs().sum()) - ref[1]) <= slack, 'after-step %s %s' % (tag, k)

    # second iteration keeps running (from slightly different weights: Adam turns gradient noise into +-lr moves)
    A, attr = cycle_inputs(1)
    model.set_input({'A': A, 'B_attr': attr, 'A_paths': ['a'] * 4, 'B_paths': ['b'] * 4})
    model.optimize_parameters()
    got = model.get_current_losses()
    for i, n in enumerate(names):
        ref = gold['it1/losses'][i]
        assert abs(got[n] - ref) <= 5e-2 * max(1.0, abs(ref)), 'it1 loss %s: hip %.6g reference %.6g' % (n, got[n], ref)

    # checkpoint round trip of the discriminator through BaseModel
    model.save_networks('latest')
    live = {k: v.detach().clone() for k, v in model.netD.state_dict().items()}
    sd = torch.load(os.path.join(model.save_dir, 'latest_net_D.pth'), map_location='cpu')
    assert list(sd.keys()) == list(live.keys()) == [str(k) for k in gold['netD_keys']]
    for k in sd:
        assert torch.equal(sd[k], live[k].cpu()), k
    with torch.no_grad():
        model.netD.model1[0].weight.add_(1.0)
    model.load_networks('latest')
    for k, v in model.netD.state_dict().items():
        assert torch.equal(v, live[k]), 'after load: ' + k
    # (last: a train-mode pass moves the running statistics) the patch maps of the reference's step
    with torch.no_grad():
        maps = model.netD(model.real_x)
    assert isinstance(maps, list) and [list(m.shape) for m in maps] == gold['patch_shapes'].tolist()
