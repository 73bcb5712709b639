"""Fixture generator of the wsgan_disc step and of the image pool (test infrastructure).  Run ONCE where the reference is present:

    python scripts/make_disc_golden.py [variant ... | pool_alone]   # tests/golden/disc_step.npz, disc_step_<variant>.npz, disc_pool.npz

Like scripts/make_cont_golden.py it IMPORTS the reference on the CPU at run time (oracle.make_golden's import with the torchvision
stub), builds the reference's own WSGANDiscModel through its own option parser and create_model for every variant of tests/disc_ref.py
(command lines, seeds, seeded weights and seeded batches are described there, once), runs optimize_parameters() for the variant's
number of iterations with Python's `random` seeded per iteration before set_input, and records, per iteration: the drawn (label_A,
label_B, label_B_not), the 11 losses, fake_B and rec_A in full, per gradient tensor of G, D and AC the float64 (sum, |sum|, L2) and
every GRAD_STRIDE-th element, and (sum, |sum|) of every state-dict entry after the step (running statistics of D and AC included);
with --pool_size > 0 also the decisions of the pool's query (as plan entries: -1 pass, 2 s store into slot s, 2 s + 1 exchange with
slot s -- found by repeating the reference's draws from the saved generator state and CHECKED against the batch its query returned)
and the float64 sum of the batch D saw; per file the loss / visual / model names, and in the default file the parsed option names with
their defaults as strings.  The U-Net variant's images are 8 times larger: its second iteration keeps every 16th pixel.

disc_pool.npz: the reference's ImagePool(3) and ImagePool(1) over six seeded queries of four [2, 3, 5] images after random.seed(31):
inputs, returned batches in full, and the plans.  Only the .npz files are committed; nothing that runs in the tests reads the
reference."""
import os
import random
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import make_golden as G  # noqa: E402
from oracle import weights as W  # noqa: E402
import disc_ref as C  # noqa: E402

POOL_SEED = 31


def watched_query(pool, images, log):
    """the reference pool's query, with its decisions recovered as a plan: the draws are repeated from the saved generator state by
    the restatement's plan_for, and the restatement's data path under that plan must return what the reference returned"""
    if pool.pool_size == 0:
        return type(pool).query(pool, images)
    shadow = pool.__dict__.setdefault('_shadow', C.PoolRef(pool.pool_size))
    state = random.getstate()
    plan = shadow.plan_for(images.shape[0])
    after = random.getstate()
    random.setstate(state)
    ret = type(pool).query(pool, images)
    assert random.getstate() == after, 'the restated draws are not the reference\'s'
    mine = shadow.query(images.detach().clone(), plan)
    assert torch.equal(mine, ret.detach()), 'the restated pool returns another batch than the reference under plan %s' % plan
    log.append((plan, ret.detach().clone()))
    return ret


def pool_alone():
    from util.image_pool import ImagePool
    out = {'seed': np.array(POOL_SEED)}
    for size in (3, 1):
        random.seed(POOL_SEED)
        pool, log = ImagePool(size), []
        for q in range(6):
            x = W.seeded_tensor((4, 2, 3, 5), 300 + 10 * size + q)
            y = watched_query(pool, x, log)
            out['size%d/q%d/x' % (size, q)] = G.t2n(x)
            out['size%d/q%d/y' % (size, q)] = G.t2n(y)
            out['size%d/q%d/plan' % (size, q)] = np.array(log[-1][0], dtype=np.int32)
    path = os.path.join(C.GOLD, 'disc_pool.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %.1f KB; plans of size 3: %s' % (path, len(out), os.path.getsize(path) / 1024.0,
                                                           [list(out['size3/q%d/plan' % q]) for q in range(6)]))


def run_variant(rn, name, tmp):
    from options.train_options import TrainOptions
    from models import create_model
    ac = rn.define_AC('resnet18', 3, 'normal', C.K, gpu_ids=[])
    ac_path = os.path.join(tmp, 'AC.pth')
    torch.save(C.classifier_weights(ac.state_dict()), ac_path)
    ip = rn.AlexNetFeature(input_nc=3, pooling='None')
    ip_path = os.path.join(tmp, 'IP.pth')
    torch.save(W.fill_state_dict(ip.state_dict(), C.SEED_IP), ip_path)
    sys.argv = C.argv(name, tmp, ac_path, ip_path, '-1')
    options = TrainOptions()
    opt = options.parse()
    model = create_model(opt)
    model.setup(opt)
    model.netG.load_state_dict(C.generator_weights(model.netG.state_dict(), opt.which_model_netG))
    model.netD.load_state_dict(W.fill_state_dict(model.netD.state_dict(), C.SEED_D))
    nets = (('G', 'optimizer_G', model.netG), ('D', 'optimizer_D', model.netD), ('AC', 'optimizer_AC', model.netAC))
    pool_log = []
    for pool in model.fake_B_pool:
        pool.query = (lambda images, pool=pool: watched_query(pool, images, pool_log))
    out = {}
    for it in range(C.iterations(name)):
        torch.manual_seed(1234 + it)
        random.seed(C.PY_SEED + it)
        grabbed, origs = {}, {}
        for tag, oname, net in nets:
            optim = getattr(model, oname)
            orig = origs[oname] = optim.step

            def stepper(orig=orig, tag=tag, net=net):
                grabbed[tag] = [(k, None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()]
                return orig()
            optim.step = stepper
        del pool_log[:]
        model.set_input(C.batch(name, it))
        model.optimize_parameters()
        for oname, orig in origs.items():
            getattr(model, oname).step = orig
        p = 'it%d' % it
        out[p + '/labels'] = np.array([model.label_A, model.label_B, model.label_B_not], dtype=np.int64)
        if opt.pool_size > 0:
            assert len(pool_log) == 1
            out[p + '/pool_plan'] = np.array(pool_log[0][0], dtype=np.int32)
            out[p + '/pool_sum'] = np.array(float(pool_log[0][1].double().sum()))
        losses = model.get_current_losses()
        out[p + '/losses'] = np.array([losses[k] for k in model.loss_names], dtype=np.float64)
        for k in ('fake_B', 'rec_A'):
            a = G.t2n(getattr(model, k))
            if name == 'unet' and it == 1:
                out['%s/samp16/%s' % (p, k)] = a.reshape(-1)[::16].copy()
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
    if name == 'default':
        # settings only: every option name of the parser with its default, as strings (paths of this run are not defaults)
        keys = sorted(vars(opt))
        out['option_names'] = np.array(keys)
        out['option_defaults'] = np.array([str(options.parser.get_default(k)) for k in keys])
    path = C.fixture_path(name)
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %.1f KB, labels it0 %s, losses it0 %s' % (path, len(out), os.path.getsize(path) / 1024.0, out['it0/labels'],
                                                                    out['it0/losses']))


def main():
    torch.set_num_threads(4)        # the tests run the twin with 4 threads too: the reductions of a convolution's gradient follow the thread count
    rn = G.import_reference()
    tmp = tempfile.mkdtemp(prefix='pcgan_golden_disc_')
    for name in (sys.argv[1:] or list(C.VARIANTS) + ['pool_alone']):
        if name == 'pool_alone':
            pool_alone()
        else:
            run_variant(rn, name, tmp)


if __name__ == '__main__':
    main()
