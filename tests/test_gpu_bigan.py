"""GPU parity of the wsgan_bigan step: WSGANBiGANModel.optimize_parameters() on the HIP path, built through the unchanged option parser
for every fixture variant (tests/bigan_ref.py), against the reference's recorded vectors (tests/golden/bigan_step*.npz, iteration 0:
identical weights) and against the float64 twin for every gradient tensor.

Tolerances are those of test_gpu_cont.py: losses 2e-4, images and ratings 2e-4 of the largest magnitude; every gradient tensor
|hip - g64| <= 2 |ref32 - g64| + 3e-2 |g64| + 1e-6 and its norm against the reference to 3e-2 (+1e-4); parameters after the Adam steps
to 2e-3 of their |.|-sum plus 2.02 lr per entry (the first Adam step moves an entry whose true gradient is 0 by +-lr, the sign being
noise); iteration 1 losses to 5e-2.  Running statistics are untouched by Adam: 2e-3 without that slack.

SHARP check, first: the float64 twin replaying the HIP step's own ReLU / max-pool decisions, 5e-4 relative L2 per gradient tensor
(test_gpu_step.py's number) -- on the same smooth branch the HIP gradients are right to operator precision.  In the lambda_y_0 variant
the encoder's whole gradient is the E_GAN term, i.e. the discriminator's gradient with respect to its rating input, which is what
csrc/concat_bwd.hip produces (tests/bigan_ref.py records the shares)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bigan_ref as C
from oracle import networks_ref as N
from oracle import weights as W
from test_gpu_nets import record_decisions
from util_cmp import assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _checkpoints(tmp_path):
    """the plain ResNet state dict load_base reads and AlexNet's, with the fixture's seeded values"""
    e_path, ip_path = str(tmp_path / 'resnet18_base.pth'), str(tmp_path / 'IP.pth')
    torch.save(C.encoder_base_weights(N.ResNetFeatureRef('resnet18').model.state_dict()), e_path)
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
    model.netE.load_state_dict(C.encoder_weights(model.netE.state_dict()))
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


def step(m, name, it):
    torch.manual_seed(1234 + it)
    m.set_input(C.batch(name, it))
    m.optimize_parameters()


@pytest.mark.parametrize('name', list(C.VARIANTS))
def test_bigan_step_matches_reference_and_twin(name, tmp_path, dev, monkeypatch):
    from pcgan_amd.hip import functional as HF
    gold = np.load(C.fixture_path(name))
    names = list(gold['loss_names'])
    model, opt = build_hip(name, tmp_path)
    assert model.loss_names == names and model.model_names == list(gold['model_names']) == ['G', 'E', 'D']
    assert model.visual_names == list(gold['visual_names'])
    assert [type(o).__name__ for o in model.optimizers] == ['FusedAdam'] * 3
    assert model.optimizers == [model.optimizer_G, model.optimizer_D, model.optimizer_E]
    ref32, twin = C.build_twin(name), C.build_twin(name, torch.float64)
    grabbed = grab_gradients(model)
    step(ref32, name, 0)
    step(twin, name, 0)
    # which joins took the one-launch backward pass: the two whose rating needs a gradient, rec_x = G(real_x, fake_y) in forward() and
    # D(real_x, fake_y) in backward_GE(); G(real_x, real_y), D(fake_x, real_y) and the two of backward_D() did not
    joins = []
    for fn in (HF._ConcatZFn, HF._ConcatZFusedFn):
        monkeypatch.setattr(fn, 'apply', staticmethod(lambda *a, fn=fn, orig=fn.apply: (joins.append(fn.__name__), orig(*a))[1]))
    with record_decisions({'G': model.netG, 'D': model.netD, 'E': model.netE, 'IP': model.netIP}) as rec:
        step(model, name, 0)
    fused = '_ConcatZFusedFn' if HF._CONCATZ_FUSED_ENV else '_ConcatZFn'
    assert joins == ['_ConcatZFn', fused] + ['_ConcatZFn'] * 2 + ['_ConcatZFn', fused], joins
    monkeypatch.undo()

    got = model.get_current_losses()
    for i, n in enumerate(names):
        ref = gold['it0/losses'][i]
        print('loss %-8s hip %.7g reference %.7g' % (n, got[n], ref))
        assert abs(got[n] - ref) <= 2e-4 * max(1.0, abs(ref)), 'loss %s: hip %.7g reference %.7g' % (n, got[n], ref)
    for k in C.IMAGES:
        assert_close(getattr(model, k), torch.from_numpy(gold['it0/' + k]), 2e-4, k + ' vs reference')
    if name != 'unet':
        # SHARP (test_gpu_step.py: 5e-4 relative L2): the float64 twin on the HIP step's own decisions differentiates the same smooth
        # branch, so the mask flips that the bound below has to allow for are gone.  (The U-Net's folded joins need the recorder of
        # test_gpu_unet.py, which files by pass and not by network: that variant keeps the bound below, as in test_gpu_cont.py.)
        sharp = C.build_twin(name, torch.float64)
        queues = {k: iter(v) for k, v in rec.tapes.items()}
        assert not rec.tape, 'decisions outside the four networks'
        nets = {'G': sharp.netG, 'D': sharp.netD, 'E': sharp.netE, 'IP': sharp.netIP}
        for k, tnet in nets.items():
            N.DecisionTape.bind(tnet, queues[k])
        try:
            step(sharp, name, 0)
            for k, q in queues.items():
                assert next(q, None) is None, 'the twin consumed fewer %s decisions than the HIP step recorded' % k
        finally:
            for tnet in nets.values():
                N.DecisionTape.bind(tnet, None)
        for k in C.IMAGES:
            assert_close(getattr(model, k), getattr(sharp, k), 2e-4, k + ' vs the twin on the HIP decisions')
        for tag in ('G', 'D', 'E'):
            for k, g64 in sharp.grads[tag].items():
                if g64 is None or float(twin.grads[tag][k].norm()) < 1e-9:        # (true gradient 0: judged by the absolute term below)
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
            if 'running_' in k:     # D's moved four times, E's twice: no optimizer touches them
                assert abs(float(v.abs().sum()) - ref[1]) <= 2e-3 * (ref[1] + 1e-3), 'running statistics %s %s' % (tag, k)
                assert abs(float(v.sum()) - ref[0]) <= 2e-3 * (ref[1] + 1e-3), 'running statistics %s %s (sum)' % (tag, k)
                continue
            slack = 2e-3 * (ref[1] + 1e-3) + 2.02 * opt.lr * v.numel()
            assert abs(float(v.abs().sum()) - ref[1]) <= slack, 'after-step %s %s' % (tag, k)

    # second iteration keeps running (now from slightly different weights: Adam turns gradient noise into +-lr moves)
    step(model, name, 1)
    got = model.get_current_losses()
    for i, n in enumerate(names):
        ref = gold['it1/losses'][i]
        assert abs(got[n] - ref) <= 5e-2 * max(1.0, abs(ref)), 'it1 loss %s: hip %.6g reference %.6g' % (n, got[n], ref)

    # the visuals and the two samplers
    s = opt.fineSize
    vis = model.get_current_visuals()
    assert list(vis.keys()) == list(gold['current_visuals']) == ['real_x', 'fake_x', 'rec_x', 'attr_0', 'attr_1', 'attr_2']
    for k, v in vis.items():
        assert tuple(v.shape) == ((1 if k.startswith('attr_') else opt.batchSize), 3, s, s) and bool(torch.isfinite(v.float()).all()), k
    with torch.no_grad():
        for image in (model.sample_from_label(1), model.sample_from_prior()):
            assert tuple(image.shape) == (opt.batchSize, 3, s, s) and bool(torch.isfinite(image.float()).all())
    assert model.test() is None


_CHILD = """
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
from pathlib import Path
import test_gpu_bigan as T
from pcgan_amd.hip import functional as HF
assert HF._CONCATZ_FUSED_ENV is False
model, _ = T.build_hip('lambda_y_0', Path(%(tmp)r))
grabbed = T.grab_gradients(model)
T.step(model, 'lambda_y_0', 0)
torch.save({k: g.cpu() for k, g in grabbed['E'].items()}, %(out)r)
"""


def test_fused_and_chained_backward_agree_on_the_encoder(tmp_path, dev):
    """lambda_y_0: the encoder's gradient is the E_GAN term alone, so every bit of it has passed through the rating gradient of D's join.
    PCGAN_CONCATZ_FUSED=0 in a fresh child process (the switch is read at import) takes the chain of copies and channel sums: the
    summation order differs, nothing else does -- relative L2 <= 1e-5 per tensor."""
    from pcgan_amd.hip import functional as HF
    assert HF._CONCATZ_FUSED_ENV, 'this test compares the default (fused) run with a PCGAN_CONCATZ_FUSED=0 child'
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    model, _ = build_hip('lambda_y_0', tmp_path / 'a')
    grabbed = grab_gradients(model)
    step(model, 'lambda_y_0', 0)
    out = str(tmp_path / 'chain.pt')
    code = _CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests'), tmp=str(tmp_path / 'b'), out=out)
    env = dict(os.environ, PCGAN_CONCATZ_FUSED='0')
    p = subprocess.run(['timeout', '-k', '10', '300', sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    chain = torch.load(out)
    twin = C.build_twin('lambda_y_0', torch.float64)
    step(twin, 'lambda_y_0', 0)
    assert sorted(chain) == sorted(grabbed['E'])
    worst = 0.0
    for k, g in grabbed['E'].items():
        a, b = g.double().cpu(), chain[k].double()
        if float(twin.grads['E'][k].norm()) < 1e-9:      # true gradient 0 (a bias in front of BatchNorm): rounding noise on both sides
            assert float(a.norm()) <= 1e-4 and float(b.norm()) <= 1e-4, 'gradE %s' % k
            continue
        err = float((a - b).norm() / b.norm())
        worst = max(worst, err)
        assert err <= 1e-5, 'fused / chained rating gradient: gradE %s relative L2 %.3e' % (k, err)
    print('fused vs chained: worst relative L2 of an encoder gradient tensor %.3e' % worst)


def test_generate_images_by_label(tmp_path, dev):
    """generate_images.py --model wsgan_bigan --how_to_sample label on two synthetic images with the same pixels: two files, and class 0
    differs from class 2.  (The U-Net: under InstanceNorm the resnet generator's first normalisation removes the rating's plane.)"""
    from PIL import Image
    import unet_ref as U
    ck = tmp_path / 'ck' / 'run'
    os.makedirs(str(ck))
    G = U.UnetGeneratorRef(3, 3, 1, 7, 8, 'instance')
    torch.save(W.fill_state_dict(G.state_dict(), C.SEED_G), str(ck / 'latest_net_G.pth'))      # (head not shrunk: differences of whole grey levels)
    E = N.SiameseFeatureRef(N.ResNetFeatureRef('resnet18'), 'max', (64, 1), 1, 0.7, False)
    torch.save(C.encoder_weights(E.state_dict()), str(ck / 'latest_net_E.pth'))
    os.makedirs(str(tmp_path / 'src'))
    pixels = np.random.RandomState(1).randint(0, 256, size=(128, 128, 3), dtype=np.uint8)
    stems = ['12_face0', '51_face1']
    for stem in stems:
        Image.fromarray(pixels).save(str(tmp_path / 'src' / (stem + '.png')))
    (tmp_path / 'list.txt').write_text('\n'.join(stem + '.png' for stem in stems) + '\n')
    (tmp_path / 'labels.txt').write_text('0\n2\n')
    gen = ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'generate_images.py'), '--model', 'wsgan_bigan', '--how_to_sample',
           'label', '--sample_label_file', str(tmp_path / 'labels.txt'), '--dataset_mode', 'single', '--sourcefile_A', str(tmp_path / 'list.txt'),
           '--dataroot', str(tmp_path / 'src'), '--name', 'run', '--checkpoints_dir', str(tmp_path / 'ck'), '--which_epoch', 'latest',
           '--which_model_netG', 'unet', '--ngf', '8', '--fineSize', '128', '--loadSize', '128', '--gpu_ids', '0', '--attr_bins', '[10, 30, 50]',
           '--attr_mean', str(C.ATTR_MEAN), '--attr_std', str(C.ATTR_STD), '--output_dir', str(tmp_path / 'out'), '--how_many', '2']
    p = subprocess.run(gen, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    written = sorted(os.listdir(str(tmp_path / 'out')))
    assert len(written) == 2 and [n.split('_')[0] for n in written] == ['0', '2'], written
    a, b = (np.asarray(Image.open(str(tmp_path / 'out' / n))).astype(np.int32) for n in written)
    assert a.shape == b.shape == (128, 128, 3) and int(np.abs(a - b).max()) >= 1, 'class 0 and class 2 gave the same image'
