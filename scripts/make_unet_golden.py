"""Fixture generator of the U-Net generator (test infrastructure).  Run ONCE where the reference is present:

    python scripts/make_unet_golden.py            # writes tests/golden/unet.npz

Like scripts/make_projection_golden.py it IMPORTS the reference's models/networks.py on the CPU (oracle/make_golden.py's import with
the torchvision stub), builds the reference's own define_G(3, 3, 1, 8, 'unet', norm, n_layers_G=5), fills it with the deterministic
weights of oracle/weights.py and records, for norm = instance (U5i) and batch (U5b) at input (3, 3, 32, 32), z (3, 1, 1, 1):

  out0, din0, din1      the train-mode output and the gradients of image and z for the seeded upstream gradient, in full
  dparam/full/<key>     parameter gradients of at most FULL_MAX elements in full
  dparam/samp/<key>     every STRIDE-th element of the larger ones, dparam/stat/<key> = (sum, abs-sum, l2) of every one
  buf/<key>             running_mean / running_var / num_batches_tracked after that pass, in full
  out_eval              the eval-mode output (running statistics) after that train-mode pass
  keys, shapes          the state_dict layout

and `counts/*`: parameters and state_dict entries of the four network sizes x two norms of tests/unet_ref.py: REFERENCE_COUNTS.
Weights and inputs are not stored: the tests regenerate them from the recorded seeds (oracle/weights.py is reference-free).  Only the
.npz is committed; nothing that runs in the tests reads the reference.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import weights as W  # noqa: E402

# prefix -> (norm, n_layers_G, ngf, batch, size, weight seed, (image seed, z seed), dy seed)
CASES = {
    'U5i': ('instance', 5, 8, 3, 32, 60, (160, 260), 360),
    'U5b': ('batch', 5, 8, 3, 32, 61, (161, 261), 361),
}
FULL_MAX = 16384
STRIDE = 11
COUNTED = (('unet', 5, 8), ('unet', 6, 8), ('unet', 7, 64), ('unet_256', 8, 64))


def case_inputs(prefix):
    _, _, _, bs, size, _, (sx, sz), _ = CASES[prefix]
    return W.seeded_tensor((bs, 3, size, size), sx), W.seeded_normal((bs, 1, 1, 1), sz)


def main():
    rn = G.import_reference()
    out = {'stride': np.array(STRIDE), 'full_max': np.array(FULL_MAX)}
    for prefix, (norm, nl, ngf, bs, size, wseed, (sx, sz), dyseed) in CASES.items():
        net = rn.define_G(3, 3, 1, ngf, 'unet', norm=norm, init_type='normal', n_layers_G=nl)
        sd = W.fill_state_dict(net.state_dict(), wseed)
        net.load_state_dict(sd, strict=True)
        net.train()
        out['%s/case' % prefix] = np.array([nl, ngf, bs, size, wseed, dyseed, sx, sz])
        out['%s/norm' % prefix] = np.array(norm)
        out['%s/keys' % prefix] = np.array(list(sd.keys()))
        out['%s/shapes' % prefix] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
        x, z = case_inputs(prefix)
        rec = {}
        G.run_net(net, [x, z], dyseed, rec, prefix, True)
        for k, p in net.named_parameters():
            if p.numel() > FULL_MAX:
                rec['%s/dparam/samp/%s' % (prefix, k)] = rec.pop('%s/dparam/full/%s' % (prefix, k)).reshape(-1)[::STRIDE].copy()
        for k in [k for k in rec if '/buf/' in k]:
            del rec[k]              # run_net keeps sums of the running statistics; these nets are small enough for all of them
        for k, b in net.named_buffers():
            rec['%s/buf/%s' % (prefix, k)] = G.t2n(b).copy()
        net.eval()
        with torch.no_grad():
            rec['%s/out_eval' % prefix] = G.t2n(net(x, z))
        out.update(rec)
    names, values = [], []
    for which, nl, ngf in COUNTED:
        for norm in ('instance', 'batch'):
            net = rn.define_G(3, 3, 1, ngf, which, norm=norm, init_type='normal', n_layers_G=nl)
            names.append('%s,%d,%d,%s' % (which, nl, ngf, norm))
            values.append([sum(p.numel() for p in net.parameters()), len(net.state_dict())])
    out['counts/names'], out['counts/values'] = np.array(names), np.array(values, dtype=np.int64)
    path = os.path.join(ROOT, 'tests', 'golden', 'unet.npz')
    np.savez(path, **out)
    print('wrote %s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == '__main__':
    main()
