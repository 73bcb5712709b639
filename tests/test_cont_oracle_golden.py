"""wsgan_cont, the continuous-label CGAN baseline, on the CPU: the plain-torch twin of its step (tests/cont_ref.py) against the vectors
captured from the reference itself (scripts/make_cont_golden.py -> tests/golden/cont_step*.npz, tolerances of
test_cycle_oracle_golden.py), the plugin registry, the parsed defaults, the pair data set with attributes, and the argument checks of
pcgan_add_n that need no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import cont_ref as C
from util_cmp import assert_close


def check_against_golden(gold, p, losses, tensors, grads, nets, zero, steps, tol_loss=2e-5, tol_t=2e-5, tol_g=2e-3, tol_after=1e-4):
    """test_cycle_oracle_golden.check_against_golden for the packed statistics of the cont fixtures.  `zero` names, per net, the
    tensors whose TRUE gradient is 0 -- a bias in front of an InstanceNorm without affine parameters; found as |g| < 1e-9 in the float64
    twin, not by looking at the values under test.  What two fp32 runs hold there is rounding noise of the five-way gradient sum, which
    need not agree to 2e-3 of itself: both must stay below the 1e-4 that test_gpu_cycle.py allows such tensors.  Adam turns that noise
    into a move of lr * m^ / sqrt(v^) per entry, whose sign is the noise's; over the first two steps |m^ / sqrt(v^)| <= 1.06 (beta1 0.5,
    beta2 0.999), so after `steps` steps two correct runs differ there by at most 2 * 1.06 * lr * steps per entry, and no more is
    allowed (test_gpu_cycle.py: the same slack for one step)."""
    for i, n in enumerate(list(gold['loss_names'])):
        ref = gold[p + '/losses'][i]
        assert abs(losses[n] - ref) <= tol_loss * max(1.0, abs(ref)), 'loss %s: %r vs %r' % (n, losses[n], ref)
    for k, t in tensors.items():
        if '%s/%s' % (p, k) in gold:
            assert_close(t, torch.from_numpy(gold['%s/%s' % (p, k)]), tol_t, k)
        else:       # the U-Net variant's second iteration: every 16th pixel
            assert_close(t.reshape(-1)[::16], torch.from_numpy(gold['%s/samp16/%s' % (p, k)]), tol_t, k)
    for tag, gd in grads.items():
        keys = list(gold['grad%s/keys' % tag])
        assert keys == [k for k, g in gd.items() if g is not None], 'grad%s: tensors that received a gradient' % tag
        for k, st in zip(keys, gold['%s/grad%s/stat' % (p, tag)]):
            l2 = float(gd[k].double().pow(2).sum().sqrt())
            if k in zero[tag]:
                assert l2 <= 1e-4 and st[2] <= 1e-4, 'grad%s %s: true gradient 0, l2 %g and %g' % (tag, k, l2, st[2])
                continue
            assert abs(l2 - st[2]) <= tol_g * st[2] + 1e-6, 'grad%s %s l2 %g vs %g' % (tag, k, l2, st[2])
    for tag, net in nets.items():
        sd = net.state_dict()
        keys = list(gold['after%s/keys' % tag])
        assert keys == list(sd.keys())
        for k, ref in zip(keys, gold['%s/after%s' % (p, tag)]):
            slack = 2.12 * 2e-4 * steps * sd[k].numel() if k in zero[tag] else 0.0
            assert abs(float(sd[k].double().abs().sum()) - ref[1]) <= tol_after * (ref[1] + 1e-3) + slack, 'after-step %s %s' % (tag, k)


@pytest.mark.parametrize('name', list(C.VARIANTS))
def test_cont_step_matches_reference(name):
    torch.set_num_threads(4)
    gold = np.load(C.fixture_path(name))
    assert list(gold['loss_names']) == C.LOSS_NAMES
    m, m64 = C.build_twin(name), C.build_twin(name, torch.float64)
    for it in range(2):
        for twin in (m64, m):
            torch.manual_seed(1234 + it)
            np.random.seed(C.NP_SEED + it)
            twin.set_input(C.batch(name, it))
            twin.optimize_parameters()
        zero = {tag: set(k for k, g in gd.items() if g is not None and float(g.norm()) < 1e-9) for tag, gd in m64.grads.items()}
        assert m.label_AB == [int(v) for v in gold['it%d/label_AB' % it]]
        check_against_golden(gold, 'it%d' % it, m.losses(), {'fake_B': m.fake_B, 'rec_A': m.rec_A}, m.grads,
                             {'G': m.netG, 'D': m.netD, 'E': m.netE}, zero, it + 1)


def _parse(argv):
    from pcgan_amd.options.train_options import TrainOptions
    old, sys.argv = sys.argv, argv
    try:
        options = TrainOptions()
        return options, options.parse()
    finally:
        sys.argv = old


def test_registry_resolves_wsgan_cont():
    from pcgan_amd.data import find_dataset_using_name
    from pcgan_amd.models import find_model_using_name
    assert find_model_using_name('wsgan_cont').__name__ == 'WSGANContModel'
    assert find_dataset_using_name('wsgan_cont').__name__ == 'WSGANContDataset'


def test_parsed_defaults_equal_the_reference(tmp_path):
    gold = np.load(C.fixture_path('default'))
    options, opt = _parse(C.argv('default', str(tmp_path), 'E.pth', 'IP.pth', '-1'))
    recorded = dict(zip(gold['option_names'], gold['option_defaults']))
    mine = {k: str(options.parser.get_default(k)) for k in vars(opt)}
    for k, v in recorded.items():       # every option of the reference, with its default
        assert k in mine, 'option --%s of the reference is missing' % k
        assert mine[k] == v, '--%s: default %s, the reference has %s' % (k, mine[k], v)
    from pcgan_amd.models import find_model_using_name
    model = find_model_using_name('wsgan_cont')
    for key in ('n_layers_D', 'batchSize', 'loadSize', 'fineSize', 'no_lsgan', 'pool_size', 'dataset_mode', 'which_model_netG'):
        assert key in recorded
    assert recorded['dataset_mode'] == 'wsgan_cont' and recorded['n_layers_D'] == '4' and recorded['batchSize'] == '10'
    assert model is not None


def _pair_folder(tmp_path):
    from PIL import Image
    rs = np.random.RandomState(3)
    names = ['%d_x%d.png' % (attr, i) for i, attr in enumerate((12, 25, 31, 40, 44, 52, 18, 7))]
    for n in names:
        Image.fromarray(rs.randint(0, 256, size=(40, 40, 3), dtype=np.uint8)).save(str(tmp_path / n))
    pairs = [(0, 1, 0), (1, 0, 2), (2, 2, 1), (3, 4, 0), (5, 4, 2), (6, 7, 2), (7, 6, 0), (1, 3, 0)]
    lines = ['%s %s %d' % (names[a], names[b], lab) for a, b, lab in pairs]
    (tmp_path / 'pairs.txt').write_text('\n'.join(lines) + '\n')
    return names, pairs, lines


def _dataset(tmp_path, extra=()):
    from pcgan_amd.data import create_dataset
    argv = ['train.py', '--dataroot', str(tmp_path), '--model', 'wsgan_cont', '--gpu_ids', '-1', '--checkpoints_dir', str(tmp_path / 'ck'),
            '--sourcefile_A', str(tmp_path / 'pairs.txt'), '--loadSize', '40', '--fineSize', '32', '--serial_batches', '--no_flip',
            '--display_id', '-1'] + list(extra)
    _, opt = _parse(argv)
    ds = create_dataset(opt)
    ds.external_shuffle = True          # keep the list order: the reshuffle is tested on its own
    return ds, opt


def test_dataset_mixed_labels(tmp_path):
    names, pairs, lines = _pair_folder(tmp_path)
    ds, opt = _dataset(tmp_path)
    assert ds.name() == 'WSGANContDataset' and len(ds) == 8
    for i, (a, b, lab) in enumerate(pairs):
        item = ds[i]
        assert sorted(item) == ['A', 'A_attr', 'A_paths', 'B', 'B_attr', 'B_paths', 'label']
        assert tuple(item['A'].shape) == (3, 32, 32) and tuple(item['B'].shape) == (3, 32, 32)
        assert tuple(item['A_attr'].shape) == (1, 1, 1) and item['A_attr'].dtype == torch.float32
        assert float(item['A_attr']) == float(names[a].split('_')[0]) and float(item['B_attr']) == float(names[b].split('_')[0])
        assert item['label'] == lab and item['A_paths'] == os.path.join(str(tmp_path), names[a]) and item['B_paths'].endswith(names[b])
        assert float(item['A'].min()) >= -1.0 and float(item['A'].max()) <= 1.0
    # the reference reshuffles whenever the length is taken; the loader takes that over under `external_shuffle`
    ds.external_shuffle = False
    import random
    random.seed(5)
    assert len(ds) == 8 and sorted(ds.sourcefile) == sorted(lines) and ds.sourcefile != lines


def test_dataset_gray_mix(tmp_path):
    _pair_folder(tmp_path)
    ds, _ = _dataset(tmp_path, ['--input_nc', '1', '--output_nc', '1', '--loadSize', '32'])      # (no room for a random crop offset)
    rgb, _ = _dataset(tmp_path, ['--loadSize', '32'])
    g, c = ds[2], rgb[2]
    assert tuple(g['A'].shape) == (1, 32, 32) and tuple(g['B'].shape) == (1, 32, 32)
    assert torch.equal(g['B'][0], c['B'][0] * 0.299 + c['B'][1] * 0.587 + c['B'][2] * 0.114)


def test_dataset_one_label_per_batch(tmp_path):
    names, pairs, lines = _pair_folder(tmp_path)
    ds, opt = _dataset(tmp_path, ['--no_mixed_label_D'])
    per = {L: [ln for ln in lines if int(ln.split()[2]) == L] for L in (0, 1, 2)}
    assert len(ds) == max(len(v) for v in per.values()) == 4           # the longest list; the single label-1 pair wraps around
    for i in range(4):
        item = ds[i]
        assert sorted(item) == sorted('%d_%s' % (L, k) for L in (0, 1, 2) for k in ('A', 'B', 'A_attr', 'B_attr', 'A_paths', 'B_paths'))
        for L in (0, 1, 2):
            fa, fb = per[L][i % len(per[L])].split()[:2]
            assert item['%d_A_paths' % L].endswith(fa) and item['%d_B_paths' % L].endswith(fb)
            assert float(item['%d_A_attr' % L]) == float(fa.split('_')[0]) and float(item['%d_B_attr' % L]) == float(fb.split('_')[0])
            assert tuple(item['%d_A' % L].shape) == (3, 32, 32)


def test_dataset_raw_form_and_synthetic(tmp_path):
    _pair_folder(tmp_path)
    ds, _ = _dataset(tmp_path, ['--gpu_transform'])
    item = ds[0]
    assert sorted(item) == ['A_attr', 'A_aug', 'A_paths', 'A_raw', 'B_attr', 'B_aug', 'B_paths', 'B_raw', 'label']
    from pcgan_amd.data import create_dataset
    _, opt = _parse(['train.py', '--dataroot', 'synthetic', '--model', 'wsgan_cont', '--gpu_ids', '-1', '--checkpoints_dir', str(tmp_path / 'ck'),
                     '--fineSize', '16', '--batchSize', '2', '--display_id', '-1'])
    syn = create_dataset(opt)
    assert len(syn) == 128
    items = [syn[i] for i in range(40)]
    assert all(tuple(it['A'].shape) == (3, 16, 16) and tuple(it['B_attr'].shape) == (1, 1, 1) for it in items)
    assert all(0.0 <= float(it[k]) < 60.0 for it in items for k in ('A_attr', 'B_attr'))
    assert set(it['label'] for it in items) == {0, 1, 2}
    assert torch.equal(syn[3]['A'], items[3]['A'])         # seeded by the index


def test_add_n_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with another message (or crash)"""
    from pcgan_amd.hip import lib
    h = lib.load()
    vp = ctypes.c_void_p
    two = (vp * 2)(4096, 8192)
    nine = (vp * 9)(*[4096 * (i + 1) for i in range(9)])
    assert h.pcgan_add_n(two, 0, 65536, 16, lib.F32, None) != 0 and b'add_n' in h.pcgan_last_error() and b'n_src' in h.pcgan_last_error()
    assert h.pcgan_add_n(nine, 9, 65536, 16, lib.F32, None) != 0 and b'n_src' in h.pcgan_last_error()
    assert h.pcgan_add_n(two, 2, None, 16, lib.F32, None) != 0 and b'null' in h.pcgan_last_error()
    assert h.pcgan_add_n(None, 2, 65536, 16, lib.F32, None) != 0 and b'null' in h.pcgan_last_error()
    assert h.pcgan_add_n((vp * 2)(4096, None), 2, 65536, 16, lib.F32, None) != 0 and b'null' in h.pcgan_last_error()
    assert h.pcgan_add_n(two, 2, 8192, 16, lib.F32, None) != 0 and b'alias' in h.pcgan_last_error()
    assert h.pcgan_add_n(two, 2, 8192 + 32, 16, lib.F32, None) != 0 and b'alias' in h.pcgan_last_error()       # partial overlap
    assert h.pcgan_add_n(two, 2, 65536, 0, lib.F32, None) != 0 and b'n == 0' in h.pcgan_last_error()
    assert h.pcgan_add_n(two, 2, 65536, 16, 7, None) != 0 and b'dtype' in h.pcgan_last_error()
    assert lib.ADD_N_MAX == 8


def test_fan_out_limits():
    from pcgan_amd.hip import functional as HF
    x = torch.zeros(3, requires_grad=True)
    with pytest.raises(ValueError):
        HF.fan_out(x, 9)
    with pytest.raises(ValueError):
        HF.fan_out(x, 0)
    outs = HF.fan_out(x, 3)       # forward: aliases, no copy, no launch (so it works without a GPU)
    assert len(outs) == 3 and all(o.data_ptr() == x.data_ptr() for o in outs)
    outs[1].sum().backward()      # one live gradient: handed on as it is, still no launch
    assert torch.equal(x.grad, torch.ones(3))
