"""Fixture generator of the projection discriminator (test infrastructure).  Run ONCE where the reference is present:

    python scripts/make_projection_golden.py            # writes tests/golden/projection_d.npz

Like scripts/make_classification_golden.py it IMPORTS the reference's models/networks.py on the CPU (oracle/make_golden.py's import with
the torchvision stub), builds the reference's own define_D(..., 'n_layers_proj', ...), fills it with the deterministic weights of
oracle/weights.py and records one forward + backward pass (oracle/make_golden.py: run_net -- output, input gradients, parameter
gradients for the seeded dy, running statistics) for two configurations:

  P1  define_D(3, 1, 8, 'n_layers_proj', 3, 'batch', True)                      input (4, 3, 32, 32), y (4, 1, 1, 1)
      everything in full: the state dict, the input, y, the output, both input gradients, every parameter gradient
  P2  define_D(3, 2, 8, 'n_layers_proj', 4, 'instance', False)                  input (2, 3, 64, 64), y (2, 2, 1, 1)
      the file stays under 512 KB, which P1 in full nearly fills: P2 keeps its key list and shapes, the output and dy's gradient in
      full, and statistics plus a strided sample of the image gradient and the parameter gradients (psi / l_y in full); its weights
      and inputs are regenerated from the recorded seeds (oracle/weights.py is reference-free), as tests/golden/nets.npz does

Only the .npz is committed; nothing that runs in the tests reads the reference.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as G  # noqa: E402
from oracle import weights as W  # noqa: E402

# prefix -> (define_D arguments after input_nc: nz, ndf, n_layers_D, norm, use_sigmoid), batch, size, weight seed, input seeds, dy seed
CASES = {
    'P1': ((1, 8, 3, 'batch', True), 4, 32, 50, (150, 250), 350),
    'P2': ((2, 8, 4, 'instance', False), 2, 64, 51, (151, 251), 351),
}
STRIDE = 97


def case_inputs(prefix):
    (nz, _, _, _, _), bs, size, _, (sx, sy), _ = CASES[prefix]
    return W.seeded_tensor((bs, 3, size, size), sx), W.seeded_normal((bs, nz, 1, 1), sy)


def main():
    rn = G.import_reference()
    out = {'stride': np.array(STRIDE)}
    for prefix, ((nz, ndf, nl, norm, sigm), bs, size, wseed, (sx, sy), dyseed) in CASES.items():
        net = rn.define_D(3, nz, ndf, 'n_layers_proj', nl, norm, sigm)
        sd = W.fill_state_dict(net.state_dict(), wseed)
        net.load_state_dict(sd, strict=True)
        out['%s/case' % prefix] = np.array([nz, ndf, nl, int(sigm), bs, size, wseed, dyseed, sx, sy])
        out['%s/norm' % prefix] = np.array(norm)
        out['%s/keys' % prefix] = np.array(list(sd.keys()))
        out['%s/shapes' % prefix] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
        x, y = case_inputs(prefix)
        full = prefix == 'P1'
        rec = {}
        G.run_net(net, [x, y], dyseed, rec, prefix, full)
        if full:
            out['%s/x' % prefix], out['%s/y' % prefix] = G.t2n(x), G.t2n(y)
            for k, v in sd.items():
                out['%s/sd/%s' % (prefix, k)] = G.t2n(v)
        else:
            a = rec.pop('%s/din0' % prefix)
            d = a.astype(np.float64)
            rec['%s/din0_stat' % prefix] = np.array([d.sum(), np.abs(d).sum(), np.sqrt((d * d).sum())])
            rec['%s/din0_samp' % prefix] = a.reshape(-1)[::STRIDE].copy()
            for k, p in net.named_parameters():
                key = '%s/dparam/samp/%s' % (prefix, k)
                if k.startswith(('psi', 'l_y')):
                    del rec[key]
                    rec['%s/dparam/full/%s' % (prefix, k)] = G.t2n(p.grad)
                else:
                    rec[key] = G.t2n(p.grad).reshape(-1)[::STRIDE].copy()
        out.update(rec)
    path = os.path.join(ROOT, 'tests', 'golden', 'projection_d.npz')
    np.savez(path, **out)
    print('wrote %s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == '__main__':
    main()
