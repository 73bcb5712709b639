"""CPU: what the stand-alone scripts share (pcgan_amd/util/script.py), held to the code it replaced.

* the option report of classification.py, regression.py, siamese_online.py and BaseOptions.print_options: stdout and the file, byte for
  byte, against the reference's dump loop restated here;
* init_like_reference against the two loops it replaced (siamese.py's: convolutions and BatchNorm; classification.py's: also Linear),
  the same draws out of torch's generator;
* first_gpu's refusal, checkpoint_file against the old join, normalized_transform's refusal and its arithmetic.
"""
import argparse
import os
import types

import numpy as np
import pytest
import torch

from pcgan_amd.util import script

SCRIPT_HEADER = '--------------- Options -----------------'
BASE_HEADER = '----------------- Options ---------------'


def reference_dump(opt, parser, header):
    """the reference's print_options loop (siamese_online.py:105-124, options/base_options.py), restated"""
    message = header + '\n'
    for k, v in sorted(vars(opt).items()):
        comment = ''
        default = parser.get_default(k)
        if v != default:
            comment = '\t[default: %s]' % str(default)
        message += '{:>25}: {:<30}{}\n'.format(str(k), str(v), comment)
    message += '----------------- End -------------------'
    return message


@pytest.mark.parametrize('module, argv, later', [
    ('classification', ['--dataroot', 'some/where', '--attr_bins', '[1, 21, 41]', '--num_classes', '3', '--weight', '1', '2', '0.5'], ()),
    ('regression', ['--dataroot', 'some/where', '--embedding_mean', '33', '--cnn_dim', '32', '1', '--no_flip'], ('embedding_normalize',)),
    ('siamese_online', ['--dataroot', 'synthetic', '--pair_selector_type', 'hard', '--max_kept', '5', '--affineScale', '0.9', '1.1'], ()),
])
def test_report_bytes_of_the_scripts(module, argv, later, tmp_path, capsys):
    S = __import__(module)
    opt = S.get_options(argv + ['--checkpoint_dir', str(tmp_path), '--name', 'run'])
    out = capsys.readouterr().out
    shown = argparse.Namespace(**{k: v for k, v in vars(opt).items() if k not in later})      # (set after the report was made)
    want = reference_dump(shown, S.build_parser(), SCRIPT_HEADER)
    assert '\t[default: ' in want and out == want + '\n'
    with open(tmp_path / 'run' / 'opt.txt') as f:
        assert f.read() == want + '\n'
    assert script.options_report(S.build_parser(), shown) == want


def test_report_bytes_of_base_options(tmp_path, capsys, monkeypatch):
    from pcgan_amd.options.base_options import BaseOptions
    monkeypatch.delenv('RANK', raising=False)
    o = BaseOptions()
    o.parser = o.initialize(argparse.ArgumentParser())
    opt = o.parser.parse_args(['--dataroot', 'd', '--checkpoints_dir', str(tmp_path), '--name', 'run', '--fineSize', '64', '--no_flip'])
    opt.phase = 'train'
    o.print_options(opt)
    want = reference_dump(opt, o.parser, BASE_HEADER)
    assert capsys.readouterr().out == want + '\n'
    with open(tmp_path / 'run' / 'opt_train.txt') as f:
        assert f.read() == want + '\n'
    assert os.path.exists(tmp_path / 'run' / 'cmd_train.txt')
    monkeypatch.setenv('RANK', '1')                       # another rank prints, and writes nothing
    opt.name = 'other'
    o.print_options(opt)
    assert capsys.readouterr().out == reference_dump(opt, o.parser, BASE_HEADER) + '\n' and not os.path.exists(tmp_path / 'other')


def toy_net():
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.ConvTranspose2d(4, 2, 2), torch.nn.Flatten(),
                               torch.nn.Linear(8, 3))


def old_siamese_init(net):
    for m in net.modules():
        kind = m.__class__.__name__
        if 'Conv' in kind:
            m.weight.data.normal_(0.0, 0.02)
        elif 'BatchNorm2d' in kind:
            m.weight.data.normal_(1.0, 0.02)
            m.bias.data.fill_(0)


def old_classification_init(net):
    with torch.no_grad():
        for m in net.modules():
            kind = type(m).__name__
            if 'Conv' in kind or 'Linear' in kind:
                m.weight.normal_(0.0, 0.02)
            elif 'BatchNorm2d' in kind:
                m.weight.normal_(1.0, 0.02)
                m.bias.zero_()


@pytest.mark.parametrize('linear, old', [(False, old_siamese_init), (True, old_classification_init)])
def test_initialisation_takes_the_same_draws(linear, old):
    torch.manual_seed(11)
    got, want = toy_net(), toy_net()
    want.load_state_dict(got.state_dict())
    with torch.no_grad():
        got[1].bias.fill_(0.5)
        want[1].bias.fill_(0.5)
    before = {k: v.clone() for k, v in got.state_dict().items()}
    torch.manual_seed(5)
    script.init_like_reference(got, linear)
    after_got = torch.rand(3)
    torch.manual_seed(5)
    old(want)
    after_want = torch.rand(3)
    for (k, a), b in zip(got.state_dict().items(), want.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(after_got, after_want)                     # the generator stands where it stood
    sd = got.state_dict()
    for k in ('0.weight', '1.weight', '2.weight'):
        assert not torch.equal(sd[k], before[k]), k
    assert float(sd['1.bias'].abs().max()) == 0
    for k in ('0.bias', '2.bias', '4.bias'):
        assert torch.equal(sd[k], before[k]), k
    assert torch.equal(sd['4.weight'], before['4.weight']) != linear
    assert all(p.requires_grad and p.grad is None for p in got.parameters())


@pytest.mark.parametrize('gpu_ids', ['0', '-1', ''])
def test_first_gpu_refuses_without_a_device(gpu_ids, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for name in ('siamese.py', 'classification.py'):
        with pytest.raises(RuntimeError) as e:
            script.first_gpu(types.SimpleNamespace(gpu_ids=gpu_ids), name, index=3)
        assert str(e.value) == 'pcgan_amd: %s needs an MI355X (no CPU fallback)' % name


def test_checkpoint_file_is_the_old_join():
    opt = types.SimpleNamespace(checkpoint_dir=os.path.join('some', 'dir'), name='exp')
    assert script.checkpoint_file(opt, 'latest') == os.path.join(opt.checkpoint_dir, opt.name, '{}_net.pth'.format('latest'))
    assert script.checkpoint_file(opt, 15) == os.path.join(os.path.join(opt.checkpoint_dir, opt.name), '%d_net.pth' % 15)
    assert script.checkpoint_file(opt, 'init') == os.path.join(opt.checkpoint_dir, opt.name, 'init_net.pth')


def test_normalized_transform():
    from PIL import Image
    from pcgan_amd.data.base_dataset import to_tensor
    opt = types.SimpleNamespace(transforms='none', loadSize=36, fineSize=32, no_flip=True, isTrain=False, use_color_jitter=False,
                                affineScale=[0.95, 1.05], affineDegrees=5)
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (40, 40, 3), dtype=np.uint8))
    got = script.normalized_transform(opt, ('crop', 'none'))(img)
    mean, std = torch.tensor(script.MEAN).view(3, 1, 1), torch.tensor(script.STD).view(3, 1, 1)
    assert got.dtype == torch.float32 and torch.equal(got, (to_tensor(img) - mean) / std)
    assert script.MEAN == (0.4914, 0.4822, 0.4465) and script.STD == (0.2023, 0.1994, 0.2010)
    with pytest.raises(ValueError) as e:
        script.normalized_transform(opt, ('crop', 'resize_and_crop'))          # a mode of the loader's, outside the caller's list
    assert str(e.value) == '--resize_or_crop none is not a valid option.'
