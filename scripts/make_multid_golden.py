"""Fixture generator of the multi-scale PatchGAN discriminator (test infrastructure).  Run ONCE where the reference is present:

    python scripts/make_multid_golden.py     # writes tests/golden/multi_d.npz and tests/golden/cycle_multid_step.npz

Like scripts/make_projection_golden.py it IMPORTS the reference's models/networks.py on the CPU (oracle/make_golden.py's import with the
torchvision stub), builds the reference's own define_D(..., 'n_layers_multi', ...), fills it with the deterministic weights of
oracle/weights.py and records one forward + backward pass (oracle/make_golden.py: run_net -- every scale's output, the input gradient, the
parameter gradients for a seeded dy per scale, the running statistics):

  M1  define_D(3, 0, 8, 'n_layers_multi', 2, 'batch', True, num_Ds=2)        input (4, 3, 32, 32)     everything in full
  M2  define_D(3, 0, 16, 'n_layers_multi', 2, 'instance', False, num_Ds=3)   input (2, 3, 64, 64)     three scales, widths 16, 8, 2
      keys, shapes and outputs in full, a statistic plus a strided sample of the gradients; weights and inputs are regenerated from the
      recorded seeds (oracle/weights.py is reference-free)
  M0  define_D(3, 0, 8, 'n_layers_multi', 2, 'batch', True, num_Ds=1)        input (4, 3, 32, 32)     keys, shapes and the output
  init/M1, init/M0   per-tensor sum and absolute sum of the freshly built nets (define_D's init_net) under torch.manual_seed(INIT_SEED)

and two optimize_parameters() calls of the reference's wsgan_cycle model with --which_model_netD n_layers_multi --num_Ds 2 --n_layers_D 2
--ndf 8 --ngf 8 --fineSize 32 --batchSize 4, recorded the way oracle/make_golden.py: golden_cycle_step records the n_layers step (losses,
images, ratings, per-tensor gradient statistics, the state after each step), less the strided gradient samples of G and E, which no test
reads and which alone would put the file over 512 KB.

Only the .npz files are committed; nothing that runs in the tests reads the reference.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import weights as W  # noqa: E402

# prefix -> (ndf, n_layers_D, norm, use_sigmoid, num_Ds), batch, size, weight seed, input seed, dy seed (scale j: dy seed + j)
CASES = {
    'M0': ((8, 2, 'batch', True, 1), 4, 32, 60, 160, 360),
    'M1': ((8, 2, 'batch', True, 2), 4, 32, 61, 161, 361),
    'M2': ((16, 2, 'instance', False, 3), 2, 64, 62, 162, 362),
}
STRIDE = 97
INIT_SEED = 7
LIMIT = 512 * 1024
STEP_FLAGS = ['--which_model_netD', 'n_layers_multi', '--num_Ds', '2', '--n_layers_D', '2', '--ndf', '8', '--ngf', '8', '--fineSize', '32',
              '--batchSize', '4']


def build(rn, prefix):
    (ndf, nl, norm, sigm, num), _, _, _, _, _ = CASES[prefix]
    return rn.define_D(3, 0, ndf, 'n_layers_multi', nl, norm, sigm, num_Ds=num)


def nets(rn, out):
    out['stride'] = np.array(STRIDE)
    out['init_seed'] = np.array(INIT_SEED)
    for prefix, ((ndf, nl, norm, sigm, num), bs, size, wseed, xseed, dyseed) in CASES.items():
        net = build(rn, prefix)
        sd = W.fill_state_dict(net.state_dict(), wseed)
        net.load_state_dict(sd, strict=True)
        out['%s/case' % prefix] = np.array([ndf, nl, int(sigm), num, bs, size, wseed, xseed, dyseed])
        out['%s/norm' % prefix] = np.array(norm)
        out['%s/keys' % prefix] = np.array(list(sd.keys()))
        out['%s/shapes' % prefix] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
        x = W.seeded_tensor((bs, 3, size, size), xseed)
        rec = {}
        G.run_net(net, [x], dyseed, rec, prefix, prefix == 'M1')
        if prefix == 'M0':
            rec = {k: v for k, v in rec.items() if k.startswith('M0/out')}
        elif prefix == 'M1':
            out['M1/x'] = G.t2n(x)
            for k, v in sd.items():
                out['M1/sd/%s' % k] = G.t2n(v)
            for k, b in net.named_buffers():        # the running statistics in full, beside run_net's sums
                if 'running' in k:
                    rec['M1/buf_full/%s' % k] = G.t2n(b)
        else:
            a = rec.pop('M2/din0')
            d = a.astype(np.float64)
            rec['M2/din0_stat'] = np.array([d.sum(), np.abs(d).sum(), np.sqrt((d * d).sum())])
            rec['M2/din0_samp'] = a.reshape(-1)[::STRIDE].copy()
        out.update(rec)
    rows = []
    for ndf in (64, 16, 8, 12):         # the width rule: first-layer widths of three scales as the reference's constructor builds them
        net = rn.D_NLayersMulti(3, ndf, n_layers=1, num_D=3)
        rows.append([ndf] + [net.model[i][0].out_channels for i in range(3)])
    out['widths'] = np.array(rows)
    for prefix in ('M0', 'M1'):
        torch.manual_seed(INIT_SEED)
        net = build(rn, prefix)
        for k, v in net.state_dict().items():
            a = G.t2n(v).astype(np.float64)
            out['init/%s/%s' % (prefix, k)] = np.array([a.sum(), np.abs(a).sum()])


def cycle_step(rn, out):
    """oracle/make_golden.py: golden_cycle_step with the multi-scale discriminator's flags"""
    from options.train_options import TrainOptions
    from models import create_model
    tmp = tempfile.mkdtemp(prefix='pcgan_golden_cycle_multid_')
    base = rn.ResNetFeature(3, 'resnet18')
    base_path = os.path.join(tmp, 'resnet18_base.pth')
    torch.save(W.fill_state_dict(base.model.state_dict(), 31), base_path)
    ip = rn.AlexNetFeature(input_nc=3, pooling='None')
    ip_path = os.path.join(tmp, 'IP.pth')
    torch.save(W.fill_state_dict(ip.state_dict(), 40), ip_path)
    sys.argv = ['train.py', '--dataroot', tmp, '--model', 'wsgan_cycle', '--name', 'g_cycle_multid', '--checkpoints_dir', tmp,
                '--gpu_ids', '-1', '--which_model_netG', 'resnet_9blocks', '--loadSize', '32', '--fineSize_E', '64', '--fineSize_IP', '64',
                '--pretrained_model_path_E', base_path, '--pretrained_model_path_IP', ip_path, '--display_id', '-1',
                '--attr_bins', '[10, 30, 50]', '--attr_mean', '35.0', '--attr_std', '20.0'] + STEP_FLAGS
    opt = TrainOptions().parse()
    model = create_model(opt)
    model.setup(opt)
    assert type(model.netD).__name__ == 'D_NLayersMulti' and model.netD.num_D == 2
    model.netG.load_state_dict(W.damp_generator_head(W.fill_state_dict(model.netG.state_dict(), 19)))
    model.netD.load_state_dict(W.fill_state_dict(model.netD.state_dict(), 20))
    esd = model.netE.state_dict()
    filled = W.fill_state_dict(esd, 33)
    for k in esd:
        if k.startswith('cnn'):
            esd[k] = filled[k]
    model.netE.load_state_dict(esd)
    for it in range(2):
        A = W.seeded_tensor((4, 3, 32, 32), 700 + it)
        attr = (W.seeded_tensor((4, 1, 1, 1), 800 + it) + 1.0) * 30.0
        torch.manual_seed(4321 + it)
        grabbed, origs = {}, {}
        for tag, optim, net in (('G', model.optimizer_G, model.netG), ('D', model.optimizer_D, model.netD), ('E', model.optimizer_E, model.netE)):
            orig = origs[tag] = optim.step

            def stepper(orig=orig, tag=tag, net=net):
                grabbed[tag] = [(k, None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()]
                return orig()
            optim.step = stepper
        model.set_input({'A': A, 'B_attr': attr, 'A_paths': ['a'] * 4, 'B_paths': ['b'] * 4})
        model.optimize_parameters()
        model.optimizer_G.step, model.optimizer_D.step, model.optimizer_E.step = origs['G'], origs['D'], origs['E']
        p = 'it%d' % it
        losses = model.get_current_losses()
        out[p + '/losses'] = np.array([losses[k] for k in model.loss_names], dtype=np.float64)
        for k in ('fake_x', 'rec_x', 'fake_y', 'rec_y', 'real_y'):
            out['%s/%s' % (p, k)] = G.t2n(getattr(model, k))
        for tag in ('G', 'D', 'E'):
            G.grads_summary(grabbed[tag], '%s/grad%s' % (p, tag), out, False)
            if tag != 'D':      # the file stays under 512 KB: G's and E's strided samples (nothing reads them) go, their statistics stay
                for k in [k for k in out if k.startswith('%s/grad%s/samp/' % (p, tag))]:
                    del out[k]
        for tag, net in (('G', model.netG), ('D', model.netD), ('E', model.netE)):
            for k, v in net.state_dict().items():
                a = G.t2n(v).astype(np.float64)
                out['%s/after%s/%s' % (p, tag, k)] = np.array([a.sum(), np.abs(a).sum()])
    with torch.no_grad():
        maps = model.netD(model.real_x)
    out['patch_shapes'] = np.array([list(m.shape) for m in maps])
    out['loss_names'] = np.array(model.loss_names)
    out['netD_keys'] = np.array(list(model.netD.state_dict().keys()))


def main():
    torch.set_num_threads(4)        # the tests run the twins with 4 threads too: the reductions of a convolution's gradient follow the thread count
    rn = G.import_reference()
    gold =os.path.join(ROOT, 'tests', 'golden')
    for name, fill in (('multi_d.npz', nets), ('cycle_multid_step.npz', cycle_step)):
        out = {}
        fill(rn, out)
        path = os.path.join(gold, name)
        np.savez_compressed(path, **out)
        print('wrote %s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
        assert os.path.getsize(path) < LIMIT


if __name__ == '__main__':
    main()
