"""Fixture generator of the wsgan_bigan step (test infrastructure).  Run ONCE where the reference is present:

    python scripts/make_bigan_golden.py [variant ...]    # writes tests/golden/bigan_step.npz and bigan_step_<variant>.npz
    python scripts/make_bigan_golden.py --shares         # the conditions on the fixtures, measured on the float64 twin alone

Like scripts/make_cont_golden.py it IMPORTS the reference on the CPU at run time (oracle.make_golden's import with the torchvision
stub), builds the reference's own WSGANBiGANModel through its own option parser and create_model for every variant of tests/bigan_ref.py
(command lines, seeded weights and seeded batches are described there, once), runs optimize_parameters() twice and records, per
iteration: the 7 losses, fake_x, rec_x, fake_y, rec_y and real_y in full, per gradient tensor of G, D and E the float64 (sum, |sum|, L2)
and every GRAD_STRIDE-th element, and (sum, |sum|) of every state-dict entry after the step (running statistics of D and E included) --
the statistics as one row per tensor beside a key list; per file loss_names, visual_names and model_names, and in the default variant
the parsed option names with their defaults as strings.  The U-Net variant's images are 16 times larger: its second iteration keeps every
UNET_IT1_STRIDE-th pixel (32: with cont's 16 the file came out 4 KB above the largest fixture committed so far).  One file per variant
keeps each under the size limit for committed files.  Only the .npz files are committed; nothing that runs in the tests reads the
reference."""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import make_golden as G  # noqa: E402
from oracle import weights as W  # noqa: E402
import bigan_ref as C  # noqa: E402


def run_variant(rn, name, tmp):
    from options.train_options import TrainOptions
    from models import create_model
    base = rn.ResNetFeature(3, 'resnet18')
    e_path = os.path.join(tmp, 'resnet18_base.pth')
    torch.save(C.encoder_base_weights(base.model.state_dict()), e_path)        # plain ResNet state dict (load_base)
    ip = rn.AlexNetFeature(input_nc=3, pooling='None')
    ip_path = os.path.join(tmp, 'IP.pth')
    torch.save(W.fill_state_dict(ip.state_dict(), C.SEED_IP), ip_path)
    sys.argv = C.argv(name, tmp, e_path, ip_path, '-1')
    options = TrainOptions()
    opt = options.parse()
    model = create_model(opt)
    model.setup(opt)
    model.netG.load_state_dict(C.generator_weights(model.netG.state_dict(), opt.which_model_netG))
    model.netD.load_state_dict(W.fill_state_dict(model.netD.state_dict(), C.SEED_D))
    model.netE.load_state_dict(C.encoder_weights(model.netE.state_dict()))
    assert model.netD.model[0].weight.shape[1] == 3 + 1       # D's first convolution reads the image and the rating
    nets = (('G', 'optimizer_G', model.netG), ('D', 'optimizer_D', model.netD), ('E', 'optimizer_E', model.netE))
    out = {}
    for it in range(2):
        torch.manual_seed(1234 + it)
        grabbed, origs = {}, {}
        for tag, oname, net in nets:
            optim = getattr(model, oname)
            orig = origs[oname] = optim.step

            def stepper(orig=orig, tag=tag, net=net):
                grabbed[tag] = [(k, None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()]
                return orig()
            optim.step = stepper
        model.set_input(C.batch(name, it))
        model.optimize_parameters()
        for oname, orig in origs.items():
            getattr(model, oname).step = orig
        p = 'it%d' % it
        losses = model.get_current_losses()
        out[p + '/losses'] = np.array([losses[k] for k in model.loss_names], dtype=np.float64)
        for k in C.IMAGES:
            a = G.t2n(getattr(model, k))
            if name == 'unet' and it == 1 and a.size > 64:
                out['%s/samp/%s' % (p, k)] = a.reshape(-1)[::C.UNET_IT1_STRIDE].copy()
            else:
                out['%s/%s' % (p, k)] = a
        for tag, _, net in nets:
            # one (sum, |sum|, L2) row per gradient tensor and one (sum, |sum|) row per state-dict entry, in the order of the key lists
            grads = [(k, G.t2n(g).astype(np.float64)) for k, g in grabbed[tag] if g is not None]
            out['grad%s/keys' % tag] = np.array([k for k, _ in grads])
            out['%s/grad%s/stat' % (p, tag)] = np.array([[a.sum(), np.abs(a).sum(), np.sqrt((a * a).sum())] for _, a in grads])
            for k, a in grads:
                out['%s/grad%s/samp/%s' % (p, tag, k)] = a.astype(np.float32).reshape(-1)[::C.GRAD_STRIDE].copy()
            state = [(k, G.t2n(v).astype(np.float64)) for k, v in net.state_dict().items()]
            out['after%s/keys' % tag] = np.array([k for k, _ in state])
            out['%s/after%s' % (p, tag)] = np.array([[a.sum(), np.abs(a).sum()] for _, a in state])
    out['loss_names'] = np.array(model.loss_names)
    out['visual_names'] = np.array(model.visual_names)
    out['model_names'] = np.array(model.model_names)
    out['current_visuals'] = np.array(list(model.get_current_visuals().keys()))
    if name == 'default':
        # settings only: every option name of the parser with its default, as strings (paths of this run are not defaults)
        keys = sorted(vars(opt))
        out['option_names'] = np.array(keys)
        out['option_defaults'] = np.array([str(options.parser.get_default(k)) for k in keys])
    path = C.fixture_path(name)
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %.1f KB, losses it0 %s' % (path, len(out), os.path.getsize(path) / 1024.0, out['it0/losses']))


def main():
    torch.set_num_threads(4)        # the tests run the twin with 4 threads too: the reductions of a convolution's gradient follow the thread count
    if sys.argv[1:] == ['--shares']:
        for name in C.VARIANTS:
            if C.options(name)['netG'] == 'unet':
                continue
            y, e = C.shares(name)
            print('%-18s cycle_y share of grad G (median over tensors) %.3f, E_GAN share of grad E %.3f' % (name, y, e))
        return
    rn = G.import_reference()
    tmp = tempfile.mkdtemp(prefix='pcgan_golden_bigan_')
    for name in (sys.argv[1:] or list(C.VARIANTS)):
        run_variant(rn, name, tmp)


if __name__ == '__main__':
    main()
