#!/usr/bin/env python
"""Image sampler for the evaluation tools -- the `generate_images.py` the reference's eval_emb.py shells out to (eval_emb.py:70-93) but
does not ship.  Its command line is the one eval_emb.py builds; its flags already live in the reference's
test options (options/test_options.py:20-22: --how_to_sample, --sample_label_file, --output_dir).

    python generate_images.py --model wsgan_emb --how_to_sample label --dataset_mode single --sourcefile_A list.txt --dataroot imgs \\
        --embedding_bins "[-1.2, 0.1, 1.4]" --embedding_mean 0.0 --embedding_std 1.0 --name run --which_epoch latest \\
        --which_model_netG resnet_9blocks --output_dir out --how_many 1000 [--sample_label_file labels.txt]

  --how_to_sample label   every source image A is turned into the class drawn for it: `model.sample_from_label(l)` = G(A, the
                          normalised bin centre embedding_bins[l]) (reference models/wsgan_emb_model.py:294-298).  The class of
                          image i is line i of --sample_label_file (cycled) or, without a file, uniform over the bins under --seed.
  --how_to_sample prior   needs a pair dataset (--dataset_mode wsgan_emb): `model.sample_from_prior()` = G(A, E(B)) (:279-292).
                          Refused for --model wsgan_bigan, which is sampled by class only (its classes are --attr_bins).

Files: <output_dir>/<label>_<index>_<stem>.png -- the class first, so that the attribute parsers of the evaluation scripts
(`float(name.split('_')[0])`, siamese.py:299-303) read it back.  compute_fid_score.py then takes <output_dir> as its first path."""
import ntpath
import os
import random

from pcgan_amd.data import CreateDataLoader
from pcgan_amd.models import create_model
from pcgan_amd.options.test_options import TestOptions
from pcgan_amd.util import util


def main(argv=None):
    import sys
    import torch
    if argv is not None:
        sys.argv = ['generate_images.py'] + list(argv)
    opt = TestOptions().parse()
    opt.nThreads, opt.batchSize, opt.serial_batches, opt.no_flip, opt.display_id, opt.sorted = 1, 1, True, True, -1, True
    if not opt.output_dir:
        raise ValueError('generate_images.py needs --output_dir')
    if not hasattr(opt, 'embedding_bins') and opt.model not in ('wsgan_cont', 'wsgan_disc', 'wsgan_bigan'):
        raise ValueError('generate_images.py drives wsgan_emb, wsgan_cont and wsgan_disc, and wsgan_bigan by class '
                         '(--model wsgan_emb / wsgan_cont / wsgan_disc / wsgan_bigan)')
    if opt.model == 'wsgan_bigan' and opt.how_to_sample != 'label':
        raise ValueError('generate_images.py samples --model wsgan_bigan by class only (--how_to_sample label); '
                         '--how_to_sample prior is not supported for it')
    dataset = CreateDataLoader(opt).load_data()
    model = create_model(opt)
    model.setup(opt)
    util.mkdirs([opt.output_dir])
    # the classes: rating bins of wsgan_emb, attribute bins (--attr_bins) of wsgan_cont and wsgan_bigan, --num_classes of wsgan_disc
    if opt.model == 'wsgan_disc':
        n_bins = opt.num_classes
    else:
        n_bins = len(model.embedding_bins if hasattr(model, 'embedding_bins') else model.attr_bins)
    labels = None
    if opt.how_to_sample == 'label':
        if opt.sample_label_file:
            with open(opt.sample_label_file) as f:
                labels = [int(float(line.split()[-1])) for line in f if line.strip()]
            if not labels or min(labels) < 0 or max(labels) >= n_bins:
                raise ValueError('--sample_label_file: labels must lie in [0, %d)' % n_bins)
        rng = random.Random(opt.seed if opt.seed is not None else 0)
    written = []
    with torch.no_grad():
        for i, data in enumerate(dataset):
            if i >= opt.how_many:
                break
            model.set_input(data)
            if opt.how_to_sample == 'label':
                label = labels[i % len(labels)] if labels else rng.randrange(n_bins)
                image = model.sample_from_label(label)
            else:
                if not (hasattr(model, 'real_B') or hasattr(model, 'attr_B')):
                    raise ValueError('--how_to_sample prior needs a pair dataset (--dataset_mode wsgan_emb / wsgan_cont): the rating or attribute comes from B')
                image = model.sample_from_prior()
                label = int(data['label'][0]) if 'label' in data else 0
            stem = os.path.splitext(ntpath.basename(model.get_image_paths()[0]))[0]
            name = '%d_%05d_%s.png' % (label, i, stem)
            util.save_image(util.tensor2im(image), os.path.join(opt.output_dir, name))
            written.append(name)
            if i % 100 == 0:
                print('generated (%05d) %s' % (i, name))
    print('%d images -> %s' % (len(written), opt.output_dir))
    return written


if __name__ == '__main__':
    main()
