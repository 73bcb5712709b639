"""GPU parity of the wsgan_disc step: WSGANDiscModel.optimize_parameters() on the HIP path, built through the unchanged option parser
for every fixture variant (tests/disc_ref.py), against the reference's recorded vectors (tests/golden/disc_step*.npz, iteration 0:
identical weights) and against the float64 twin for every gradient tensor.

Tolerances are those of test_gpu_cont.py, unchanged: losses 2e-4, images 2e-4 of the largest magnitude; every gradient tensor
|hip - g64| <= 2 |ref32 - g64| + 3e-2 |g64| + 1e-6 and its norm against the reference to 3e-2 (+1e-4); parameters after the Adam steps
to 2e-3 of their |.|-sum plus 2.02 lr per entry (the first Adam step moves an entry whose true gradient is 0 by +-lr, the sign being
noise); later iterations' losses to 5e-2.  Running statistics are untouched by Adam: 2e-3 without that slack.

SHARP check, first: the float64 twin replaying the HIP step's own ReLU / max-pool decisions, 5e-4 relative L2 per gradient tensor
(test_gpu_step.py's number) -- on the same smooth branch the HIP gradients are right to operator precision.  The U-Net variant is
excused from it as in test_gpu_cont.py, and for the same reason.

Draws: on Python <= 3.10 (disc_ref.REFERENCE_DRAWS) the model draws its label triple and its pool's plan itself and both are asserted
equal to the recorded ones; on a newer interpreter they are set from the fixture (disc_ref.step) and only the plan's use is checked."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import disc_ref as C
import classifier_ref as CR
from oracle import networks_ref as N
from oracle import weights as W
from test_gpu_nets import record_decisions
from util_cmp import assert_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ('G', 'D', 'AC')


def _checkpoints(tmp_path):
    """the classifier's whole state dict (what classification.py writes) and AlexNet's, with the fixture's seeded values"""
    ac = CR.ResNetClassifierRef('resnet18', C.K)
    ac_path, ip_path = str(tmp_path / 'AC.pth'), str(tmp_path / 'IP.pth')
    torch.save(C.classifier_weights(ac.state_dict()), ac_path)
    ip = N.AlexNetFeatureRef(3, 'None')
    torch.save(W.fill_state_dict(ip.state_dict(), C.SEED_IP), ip_path)
    return ac_path, ip_path


def build_hip(name, tmp_path):
    from pcgan_amd.options.train_options import TrainOptions
    from pcgan_amd.models import create_model
    ac_path, ip_path = _checkpoints(tmp_path)
    old, sys.argv = sys.argv, C.argv(name, str(tmp_path), ac_path, ip_path, '0')
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
    """{'G' | 'D' | 'AC': {name: gradient}} as each optimizer sees them when it steps"""
    grabbed = {}
    for tag, optim, net in (('G', model.optimizer_G, model.netG), ('D', model.optimizer_D, model.netD), ('AC', model.optimizer_AC, model.netAC)):
        orig = optim.step

        def stepper(orig=orig, tag=tag, net=net):
            grabbed[tag] = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
            return orig()
        optim.step = stepper
    return grabbed


def watch_pools(model):
    """[(class, plan)] of every query with a pool behind it, in order"""
    log = []
    for L, pool in enumerate(model.fake_B_pool):
        orig = pool.exchange
        pool.exchange = (lambda images, plan, orig=orig, L=L: (log.append((L, list(plan))), orig(images, plan))[1])
    return log


@pytest.mark.parametrize('name', list(C.VARIANTS))
def test_disc_step_matches_reference_and_twin(name, tmp_path, dev):
    from pcgan_amd.hip import lib
    gold = np.load(C.fixture_path(name))
    names = list(gold['loss_names'])
    model, opt = build_hip(name, tmp_path)
    assert model.loss_names == names and model.model_names == ['G', 'D', 'AC']
    assert model.visual_names == list(gold['visual_names'])
    assert [type(o).__name__ for o in model.optimizers] == ['FusedAdam'] * 3
    assert model.optimizers[0] is model.optimizer_G and model.optimizers[1] is model.optimizer_D and model.optimizers[2] is model.optimizer_AC
    assert [tuple(t.shape) for t in model.one_hot_labels] == [(1, C.K, 1, 1)] * C.K and model.one_hot_labels[1].dtype == torch.float32
    assert model.one_hot_labels[1].is_cuda and model.one_hot_labels[1].flatten().tolist() == [0.0, 1.0, 0.0]
    ref32, twin = C.build_twin(name), C.build_twin(name, torch.float64)
    grabbed = grab_gradients(model)
    pool_log = watch_pools(model)
    launches = lib.pool_exchange_launches()
    C.step(ref32, name, 0, gold)
    C.step(twin, name, 0, gold)
    # the HIP step; its ReLU / max-pool decisions are recorded per network (the classifier is entered through classify(), not
    # forward(): its decisions are the ones filed under no network)
    with record_decisions({'G': model.netG, 'D': model.netD, 'IP': model.netIP}) as rec:
        C.step(model, name, 0, gold)
    if C.REFERENCE_DRAWS:
        assert [model.label_A, model.label_B, model.label_B_not] == [int(v) for v in gold['it0/labels']]
    history = [model.fake_B.detach().clone()]
    seen = [model._fake_B_from_pool.detach().clone()]
    assert model.netAC.training and model.netD.training

    got = model.get_current_losses()
    for i, n in enumerate(names):
        ref = gold['it0/losses'][i]
        print('loss %-13s hip %.7g reference %.7g' % (n, got[n], ref))
        assert abs(got[n] - ref) <= 2e-4 * max(1.0, abs(ref)), 'loss %s: hip %.7g reference %.7g' % (n, got[n], ref)
    for k in ('fake_B', 'rec_A'):
        assert_close(getattr(model, k), torch.from_numpy(gold['it0/' + k]), 2e-4, k + ' vs reference')
    if name != 'unet':
        # SHARP (test_gpu_step.py: 5e-4 relative L2): the float64 twin on the HIP step's own decisions differentiates the same smooth
        # branch, so the mask flips that the bound below has to allow for are gone.  (The U-Net's folded joins need the recorder of
        # test_gpu_unet.py, which files by pass and not by network: that variant keeps the bound below.)
        sharp = C.build_twin(name, torch.float64)
        queues = {k: iter(v) for k, v in rec.tapes.items()}
        queues['AC'] = iter(rec.tape)
        nets = {'G': sharp.netG, 'D': sharp.netD, 'AC': sharp.netAC, 'IP': sharp.netIP}
        for k, tnet in nets.items():
            N.DecisionTape.bind(tnet, queues[k])
        try:
            C.step(sharp, name, 0, gold)
            for k, q in queues.items():
                assert next(q, None) is None, 'the twin consumed fewer %s decisions than the HIP step recorded' % k
        finally:
            for tnet in nets.values():
                N.DecisionTape.bind(tnet, None)
        for k in ('fake_B', 'rec_A'):
            assert_close(getattr(model, k), getattr(sharp, k), 2e-4, k + ' vs the twin on the HIP decisions')
        for tag in TAGS:
            for k, g64 in sharp.grads[tag].items():
                if g64 is None or float(twin.grads[tag][k].norm()) < 1e-9:        # (true gradient 0: judged by the absolute term below)
                    continue
                err = float((grabbed[tag][k].double().cpu() - g64).norm() / g64.norm())
                if err > 1e-4:
                    print('sharp grad%s %s: relative L2 %.3e' % (tag, k, err))
                assert err <= 5e-4, 'grad%s %s against the twin on the HIP decisions: relative L2 %.3e' % (tag, k, err)

    for tag in TAGS:
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
    for tag, net in (('G', model.netG), ('D', model.netD), ('AC', model.netAC)):
        sd = net.state_dict()
        keys = list(gold['after%s/keys' % tag])
        assert list(sd.keys()) == keys
        for k, ref in zip(keys, gold['it0/after%s' % tag]):
            v = sd[k].double()
            if 'running_' in k or 'num_batches_tracked' in k:     # D's moved five times (four under --lambda_A_GAN 0), AC's two or three
                assert abs(float(v.abs().sum()) - ref[1]) <= 2e-3 * (ref[1] + 1e-3), 'running statistics %s %s' % (tag, k)
                assert abs(float(v.sum()) - ref[0]) <= 2e-3 * (ref[1] + 1e-3), 'running statistics %s %s (sum)' % (tag, k)
                continue
            slack = 2e-3 * (ref[1] + 1e-3) + 2.02 * opt.lr * v.numel()
            assert abs(float(v.abs().sum()) - ref[1]) <= slack, 'after-step %s %s' % (tag, k)

    # later iterations keep running (now from slightly different weights: Adam turns gradient noise into +-lr moves)
    for it in range(1, C.iterations(name)):
        C.step(model, name, it, gold)
        history.append(model.fake_B.detach().clone())
        seen.append(model._fake_B_from_pool.detach().clone())
        got = model.get_current_losses()
        for i, n in enumerate(names):
            ref = gold['it%d/losses' % it][i]
            assert abs(got[n] - ref) <= 5e-2 * max(1.0, abs(ref)), 'it%d loss %s: hip %.6g reference %.6g' % (it, n, got[n], ref)
        if C.REFERENCE_DRAWS:
            assert [model.label_A, model.label_B, model.label_B_not] == [int(v) for v in gold['it%d/labels' % it]]

    if name == 'pool':
        # the plan of every query is the recorded one; the batch D received is, image by image, bit-equal to the fake_B -- of this or
        # of an earlier iteration of THIS run -- the plan names; one launch per query
        assert lib.pool_exchange_launches() - launches == 3 and len(pool_log) == 3
        owner = {}
        for it, (L, plan) in enumerate(pool_log):
            assert L == 1 and plan == [int(v) for v in gold['it%d/pool_plan' % it]], 'iteration %d: class %d, plan %s' % (it, L, plan)
            for i, op in enumerate(plan):
                src = owner[op // 2] if op >= 0 and op % 2 == 1 else (it, i)
                if op >= 0:
                    owner[op // 2] = (it, i)
                assert torch.equal(seen[it][i].view(torch.int32), history[src[0]][src[1]].view(torch.int32)), \
                    'iteration %d image %d: D did not see fake_B[%d] of iteration %d' % (it, i, src[1], src[0])
        assert any(op >= 0 and op % 2 == 1 for _, plan in pool_log[1:] for op in plan)
    else:
        # --pool_size 0: D sees fake_B itself and nothing is launched
        assert lib.pool_exchange_launches() == launches and pool_log == []
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(seen, history))

    # the visuals and the two samplers, against the twin's generator holding the HIP generator's present weights
    s = opt.fineSize
    vis = model.get_current_visuals()
    assert list(vis.keys()) == list(gold['visual_names']) + ['attr_%d' % L for L in range(C.K)]
    for k, v in vis.items():
        assert tuple(v.shape) == ((1 if k.startswith('attr_') else opt.batchSize), 3, s, s) and bool(torch.isfinite(v.float()).all()), k
    g64 = C.build_twin(name, torch.float64).netG
    g64.load_state_dict({k: v.detach().cpu().double() for k, v in model.netG.state_dict().items()})
    real_A = model.real_A.detach().cpu().double()
    eye = torch.eye(C.K, dtype=torch.float64)
    attrs = [5.0, 12.0, 35.0, 70.0][:opt.batchSize]           # bins [10, 30, 50, inf): 5 matches none and falls to the last class
    classes = [2, 0, 1, 2][:opt.batchSize]
    model.attr_B = torch.tensor(attrs, device=dev).view(-1, 1, 1, 1)
    with torch.no_grad():
        for L in range(C.K):
            assert_close(vis['attr_%d' % L], g64(real_A[0:1], eye[L].view(1, C.K, 1, 1)), 2e-4, 'attr_%d vs twin' % L)
        assert_close(model.sample_from_label(1), g64(real_A, eye[1].view(1, C.K, 1, 1)), 2e-4, 'sample_from_label vs twin')
        assert_close(model.sample_from_prior(), g64(real_A, eye[classes].view(-1, C.K, 1, 1)), 2e-4, 'sample_from_prior vs twin')
        assert not torch.equal(model.sample_from_label(0), model.sample_from_label(2))


def test_unet_128_is_answered_as_before(tmp_path, dev):
    """the model's default generator name is the reference's `unet_128`, which define_G answers with the name to use instead"""
    from pcgan_amd.options.train_options import TrainOptions
    from pcgan_amd.models import create_model
    ac_path, ip_path = _checkpoints(tmp_path)
    argv = [a for a in C.argv('default', str(tmp_path), ac_path, ip_path, '0')]
    i = argv.index('--which_model_netG')
    del argv[i:i + 2]
    old, sys.argv = sys.argv, argv
    try:
        opt = TrainOptions().parse()
    finally:
        sys.argv = old
    assert opt.which_model_netG == 'unet_128'
    with pytest.raises(NotImplementedError, match='--which_model_netG unet'):
        create_model(opt)


def test_train_then_generate_scripts(tmp_path, dev):
    from PIL import Image
    ac_path, ip_path = _checkpoints(tmp_path)
    common = ['--model', 'wsgan_disc', '--name', 'run', '--checkpoints_dir', str(tmp_path / 'ck'), '--which_model_netG', 'resnet_9blocks',
              '--ngf', '8', '--fineSize', '32', '--loadSize', '32', '--gpu_ids', '0', '--num_classes', str(C.K), '--embedding_nc', str(C.K),
              '--attr_bins', '[10, 30, 50]']
    train = ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'train.py'), '--dataroot', 'synthetic'] + common + [
        '--which_model_netD', 'n_layers', '--n_layers_D', '3', '--ndf', '8', '--fineSize_AC', '64', '--fineSize_IP', '64', '--batchSize', '4',
        '--max_dataset_size', '12', '--nThreads', '0', '--niter', '1', '--niter_decay', '0', '--print_freq', '1', '--save_epoch_freq', '1',
        '--display_id', '-1', '--seed', '3', '--pool_size', '2', '--pretrained_model_path_AC', ac_path, '--pretrained_model_path_IP', ip_path]
    p = subprocess.run(train, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in open(tmp_path / 'ck' / 'run' / 'loss_log.txt') if ln.startswith('(epoch')]
    assert len(lines) == 3 and all(('%s: ' % n) in lines[2] for n in C.LOSS_NAMES), lines
    assert ' nan' not in lines[2] and ' inf' not in lines[2]
    for tag in TAGS:
        assert os.path.exists(tmp_path / 'ck' / 'run' / ('latest_net_%s.pth' % tag))
    os.makedirs(tmp_path / 'src')
    rs = np.random.RandomState(1)
    stems = ['%d_face%d' % (a, i) for i, a in enumerate((12, 33, 51, 70))]
    for stem in stems:
        Image.fromarray(rs.randint(0, 256, size=(32, 32, 3), dtype=np.uint8)).save(str(tmp_path / 'src' / (stem + '.png')))
    (tmp_path / 'list.txt').write_text('\n'.join(stem + '.png' for stem in stems) + '\n')
    (tmp_path / 'labels.txt').write_text('2\n0\n1\n')
    gen = ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'generate_images.py'), '--how_to_sample', 'label',
           '--sample_label_file', str(tmp_path / 'labels.txt'), '--dataset_mode', 'single', '--sourcefile_A', str(tmp_path / 'list.txt'),
           '--dataroot', str(tmp_path / 'src'), '--which_epoch', 'latest', '--output_dir', str(tmp_path / 'out'), '--how_many', '4'] + common
    p = subprocess.run(gen, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    written = sorted(os.listdir(tmp_path / 'out'))
    assert len(written) == 4 and sorted(n.split('_')[0] for n in written) == ['0', '1', '2', '2'], written
    assert all(Image.open(str(tmp_path / 'out' / n)).size == (32, 32) for n in written)
