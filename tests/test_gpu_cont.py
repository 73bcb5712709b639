"""GPU parity of the wsgan_cont step: WSGANContModel.optimize_parameters() on the HIP path, built through the unchanged option parser
for every fixture variant (tests/cont_ref.py), against the reference's recorded vectors (tests/golden/cont_step*.npz, iteration 0:
identical weights) and against the float64 twin for every gradient tensor.

Tolerances are those of test_gpu_cycle.py: losses 2e-4, images 2e-4 of the largest magnitude; every gradient tensor
|hip - g64| <= 2 |ref32 - g64| + 3e-2 |g64| + 1e-6 and its norm against the reference to 3e-2 (+1e-4); parameters after the Adam steps
to 2e-3 of their |.|-sum plus 2.02 lr per entry (the first Adam step moves an entry whose true gradient is 0 by +-lr, the sign being
noise); iteration 1 losses to 5e-2.  Running statistics are untouched by Adam: 2e-3 without that slack.

SHARP check, first: the float64 twin replaying the HIP step's own ReLU / max-pool decisions, 5e-4 relative L2 per gradient tensor
(test_gpu_step.py's number) -- on the same smooth branch the HIP gradients are right to operator precision."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cont_ref as C
from oracle import networks_ref as N
from oracle import weights as W
from test_gpu_nets import record_decisions
from util_cmp import assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _checkpoints(tmp_path):
    """the regressor's whole state dict (what regression.py --mode train writes) and AlexNet's, with the fixture's seeded values"""
    import regression_ref as R
    e = R.RegressionNetworkRef(R.ResNetTrunkRef('resnet18'), 'avg', (64, 1), 1, 0.7)
    e_path, ip_path = str(tmp_path / 'E.pth'), str(tmp_path / 'IP.pth')
    torch.save(C.regressor_weights(e.state_dict()), e_path)
    ip = N.AlexNetFeatureRef(3, 'None')
    torch.save(W.fill_state_dict(ip.state_dict(), C.SEED_IP), ip_path)
    return e_path, ip_path


def build_hip(name, tmp_path):
    from pcgan_amd.options.train_options import TrainOptions
    from pcgan_amd.models import create_model
    e_path, ip_path = _checkpoints(tmp_path)
    old, sys.argv = sys.argv, C.argv(name, str(tmp_path), e_path, ip_path, '0')
    try:
        opt = TrainOptions().parse()
    finally:
        sys.argv = old
    model = create_model(opt)
    model.setup(opt)
    model.netG.load_state_dict(C.generator_weights({k: v.cpu() for k, v in model.netG.state_dict().items()}, opt.which_model_netG))
    model.netD.load_state_dict(W.fill_state_dict({k: v.cpu() for k, v in model.netD.state_dict().items()}, C.SEED_D))
    return model, opt


def grab_gradients(model):
    """{'G' | 'D' | 'E': {name: gradient}} as each optimizer sees them when it steps"""
    grabbed = {}
    for tag, optim, net in (('G', model.optimizer_G, model.netG), ('D', model.optimizer_D, model.netD), ('E', model.optimizer_E, model.netE)):
        orig = optim.step

        def stepper(orig=orig, tag=tag, net=net):
            grabbed[tag] = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
            return orig()
        optim.step = stepper
    return grabbed


def hip_step(model, name, it):
    torch.manual_seed(1234 + it)
    np.random.seed(C.NP_SEED + it)
    model.set_input(C.batch(name, it))
    model.optimize_parameters()


def twin_step(twin, name, it):
    torch.manual_seed(1234 + it)
    np.random.seed(C.NP_SEED + it)
    twin.set_input(C.batch(name, it))
    twin.optimize_parameters()


@pytest.mark.parametrize('name', list(C.VARIANTS))
def test_cont_step_matches_reference_and_twin(name, tmp_path, dev):
    gold = np.load(C.fixture_path(name))
    names = list(gold['loss_names'])
    model, opt = build_hip(name, tmp_path)
    assert model.loss_names == names and model.model_names == ['G', 'D', 'E']
    assert model.visual_names == list(gold['visual_names'])
    assert [type(o).__name__ for o in model.optimizers] == ['FusedAdam'] * 3 and model.optimizers[2] is model.optimizer_E
    ref32, twin = C.build_twin(name), C.build_twin(name, torch.float64)
    grabbed = grab_gradients(model)
    twin_step(ref32, name, 0)
    twin_step(twin, name, 0)
    # the HIP step; its ReLU / max-pool decisions are recorded per network (the regressor is entered through regress(), not
    # forward(): its decisions are the ones filed under no network)
    with record_decisions({'G': model.netG, 'D': model.netD, 'IP': model.netIP}) as rec:
        hip_step(model, name, 0)
    assert [int(v) for v in model.label_AB] == [int(v) for v in gold['it0/label_AB']]

    got = model.get_current_losses()
    for i, n in enumerate(names):
        ref = gold['it0/losses'][i]
        print('loss %-13s hip %.7g reference %.7g' % (n, got[n], ref))
        assert abs(got[n] - ref) <= 2e-4 * max(1.0, abs(ref)), 'loss %s: hip %.7g reference %.7g' % (n, got[n], ref)
    for k in ('fake_B', 'rec_A'):
        assert_close(getattr(model, k), torch.from_numpy(gold['it0/' + k]), 2e-4, k + ' vs reference')
    if name != 'unet':
        # SHARP (test_gpu_step.py: 5e-4 relative L2): the float64 twin on the HIP step's own decisions differentiates the same smooth
        # branch, so the mask flips that the bound above has to allow for are gone.  (The U-Net's folded joins need the recorder of
        # test_gpu_unet.py, which files by pass and not by network: that variant keeps the bound above, which it meets with room.)
        sharp = C.build_twin(name, torch.float64)
        queues = {k: iter(v) for k, v in rec.tapes.items()}
        queues['E'] = iter(rec.tape)
        nets = {'G': sharp.netG, 'D': sharp.netD, 'E': sharp.netE, 'IP': sharp.netIP}
        for k, tnet in nets.items():
            N.DecisionTape.bind(tnet, queues[k])
        try:
            twin_step(sharp, name, 0)
            for k, q in queues.items():
                assert next(q, None) is None, 'the twin consumed fewer %s decisions than the HIP step recorded' % k
        finally:
            for tnet in nets.values():
                N.DecisionTape.bind(tnet, None)
        for k in ('fake_B', 'rec_A'):
            assert_close(getattr(model, k), getattr(sharp, k), 2e-4, k + ' vs the twin on the HIP decisions')
        for tag in ('G', 'D', 'E'):
            for k, g64 in sharp.grads[tag].items():
                if g64 is None or float(twin.grads[tag][k].norm()) < 1e-9:        # (true gradient 0: judged by the absolute term above)
                    continue
                err = float((grabbed[tag][k].double().cpu() - g64).norm() / g64.norm())
                if err > 1e-4:
                    print('sharp grad%s %s: relative L2 %.3e' % (tag, k, err))
                assert err <= 5e-4, 'grad%s %s against the twin on the HIP decisions: relative L2 %.3e' % (tag, k, err)

    for tag in ('G', 'D', 'E'):
        keys = list(gold['grad%s/keys' % tag])
        assert sorted(grabbed[tag]) == sorted(keys), 'grad%s: tensors that received a gradient' % tag
        for k, st in zip(keys, gold['it0/grad%s/stat' % tag]):
            g64, hip, r32 = twin.grads[tag][k], grabbed[tag][k], ref32.grads[tag][k]
            scale = float(g64.norm())
            e_hip = float((hip.double().cpu() - g64).norm())
            e_ref = float((r32.double() - g64).norm())
            if e_hip > 0.5 * (2 * e_ref + 3e-2 * scale + 1e-6):
                print('grad%s %s: |hip-g64| %.3e, |ref32-g64| %.3e, |g64| %.3e' % (tag, k, e_hip, e_ref, scale))
            assert e_hip <= 2 * e_ref + 3e-2 * scale + 1e-6, \
                'grad%s %s: |hip-g64| %.3e, |ref32-g64| %.3e, |g64| %.3e' % (tag, k, e_hip, e_ref, scale)
            assert abs(float(hip.double().norm()) - st[2]) <= 3e-2 * st[2] + 1e-4, 'grad%s %s norm vs reference' % (tag, k)
    for tag, net in (('G', model.netG), ('D', model.netD), ('E', model.netE)):
        sd = net.state_dict()
        keys = list(gold['after%s/keys' % tag])
        assert list(sd.keys()) == keys
        for k, ref in zip(keys, gold['it0/after%s' % tag]):
            v = sd[k].double()
            if 'running_' in k:     # D's moved five times (four under --lambda_A_GAN 0), E's two or three: no optimizer touches them
                assert abs(float(v.abs().sum()) - ref[1]) <= 2e-3 * (ref[1] + 1e-3), 'running statistics %s %s' % (tag, k)
                assert abs(float(v.sum()) - ref[0]) <= 2e-3 * (ref[1] + 1e-3), 'running statistics %s %s (sum)' % (tag, k)
                continue
            slack = 2e-3 * (ref[1] + 1e-3) + 2.02 * opt.lr * v.numel()
            assert abs(float(v.abs().sum()) - ref[1]) <= slack, 'after-step %s %s' % (tag, k)

    # second iteration keeps running (now from slightly different weights: Adam turns gradient noise into +-lr moves)
    hip_step(model, name, 1)
    got = model.get_current_losses()
    for i, n in enumerate(names):
        ref = gold['it1/losses'][i]
        assert abs(got[n] - ref) <= 5e-2 * max(1.0, abs(ref)), 'it1 loss %s: hip %.6g reference %.6g' % (n, got[n], ref)

    # the visuals and the two samplers
    s = opt.fineSize
    vis = model.get_current_visuals()
    assert list(vis.keys()) == ['real_A', 'fake_B', 'real_B', 'rec_A', 'attr_0', 'attr_1', 'attr_2']
    for k, v in vis.items():
        assert tuple(v.shape) == ((1 if k.startswith('attr_') else opt.batchSize), 3, s, s) and bool(torch.isfinite(v.float()).all()), k
    with torch.no_grad():
        for image in (model.sample_from_label(1), model.sample_from_prior()):
            assert tuple(image.shape) == (opt.batchSize, 3, s, s) and bool(torch.isfinite(image.float()).all())
        assert not torch.equal(model.sample_from_label(0), model.sample_from_label(2))


def _one_step(tmp_path, sub, name='aux_on_fake_L1'):
    """(gradients, fake_B, rec_A, losses) of iteration 0 of a freshly built model -- the variant with all five readers of fake_B"""
    os.makedirs(str(tmp_path / sub))
    model, _ = build_hip(name, tmp_path / sub)
    grabbed = grab_gradients(model)
    hip_step(model, name, 0)
    return grabbed, model.fake_B.detach().clone(), model.rec_A.detach().clone(), model.get_current_losses()


def test_fan_out_switch_and_determinism(tmp_path, dev, monkeypatch):
    from pcgan_amd.hip import ops
    from pcgan_amd.models import wsgan_shared as M
    assert M._FANOUT is (os.environ.get('PCGAN_FANOUT', '1') != '0')
    calls = []
    orig = ops.add_n
    monkeypatch.setattr(ops, 'add_n', lambda ts, out=None: (calls.append(len(ts)), orig(ts, out))[1])
    monkeypatch.setattr(M, '_FANOUT', True)
    first = _one_step(tmp_path, 'a')
    # fake_B: D, second generator pass, L1 and the shared resize; the shared resize: IP and E; rec_A: D and the cycle L1
    assert sorted(calls) == [2, 2, 4], calls
    again = _one_step(tmp_path, 'b')
    for tag in ('G', 'D', 'E'):
        for k, g in first[0][tag].items():
            assert torch.equal(g, again[0][tag][k]), 'the same step twice: grad%s %s differs' % (tag, k)
    assert torch.equal(first[1], again[1]) and torch.equal(first[2], again[2]) and first[3] == again[3]

    del calls[:]
    monkeypatch.setattr(M, '_FANOUT', False)       # the switch as PCGAN_FANOUT=0 sets it: autograd accumulates with binary adds
    plain = _one_step(tmp_path, 'c')
    assert calls == []
    assert torch.equal(first[1], plain[1]) and torch.equal(first[2], plain[2])          # the forward pass is the same launches
    twin = C.build_twin('aux_on_fake_L1', torch.float64)
    twin_step(twin, 'aux_on_fake_L1', 0)
    for tag in ('G', 'D', 'E'):
        for k, g in first[0][tag].items():
            a, b = g.double(), plain[0][tag][k].double()
            if float(twin.grads[tag][k].norm()) < 1e-9:      # true gradient 0: both hold rounding noise only (test_gpu_cycle.py: 1e-4)
                assert float(a.norm()) <= 1e-4 and float(b.norm()) <= 1e-4, 'grad%s %s' % (tag, k)
                continue
            err = float((a - b).norm() / b.norm())
            assert err <= 1e-5, 'fan-out on / off: grad%s %s relative L2 %.3e' % (tag, k, err)


def test_train_then_test_scripts(tmp_path, dev):
    e_path, ip_path = _checkpoints(tmp_path)
    common = ['--dataroot', 'synthetic', '--model', 'wsgan_cont', '--name', 'run', '--checkpoints_dir', str(tmp_path / 'ck'),
              '--which_model_netG', 'resnet_9blocks', '--ngf', '8', '--fineSize', '32', '--loadSize', '32', '--gpu_ids', '0',
              '--attr_bins', '[10, 30, 50]', '--attr_mean', '35.0', '--attr_std', '20.0']
    train = [sys.executable, os.path.join(ROOT, 'train.py')] + common + [
        '--which_model_netD', 'n_layers', '--n_layers_D', '3', '--ndf', '8', '--fineSize_E', '64', '--fineSize_IP', '64', '--batchSize', '4',
        '--max_dataset_size', '8', '--nThreads', '0', '--niter', '1', '--niter_decay', '0', '--print_freq', '1', '--save_epoch_freq', '1',
        '--display_id', '-1', '--seed', '3', '--pretrained_model_path_E', e_path, '--pretrained_model_path_IP', ip_path]
    p = subprocess.run(train, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in open(tmp_path / 'ck' / 'run' / 'loss_log.txt') if ln.startswith('(epoch')]
    assert len(lines) == 2 and all(('%s: ' % n) in lines[1] for n in C.LOSS_NAMES), lines
    assert ' nan' not in lines[1] and ' inf' not in lines[1]
    for tag in 'GDE':
        assert os.path.exists(tmp_path / 'ck' / 'run' / ('latest_net_%s.pth' % tag))
    test = [sys.executable, os.path.join(ROOT, 'test.py')] + common + ['--results_dir', str(tmp_path / 'res'), '--how_many', '2']
    p = subprocess.run(test, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    names = sorted(os.listdir(tmp_path / 'res' / 'run' / 'test_latest' / 'images'))
    assert len(names) == 8 and sum(n.endswith('_real_A.png') for n in names) == 2 and sum('_attr_' in n for n in names) == 6, names
