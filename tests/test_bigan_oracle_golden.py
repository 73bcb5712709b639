"""wsgan_bigan, the BiGAN-style model, on the CPU: the plain-torch twin of its step (tests/bigan_ref.py) against the vectors captured from
the reference itself (scripts/make_bigan_golden.py -> tests/golden/bigan_step*.npz, bounds of test_cont_oracle_golden.py), the plugin
registry, the parsed defaults, the refusals of the model and of generate_images.py, the fused_concat_bwd switch, and the argument checks
of pcgan_concat_z_bwd that need no GPU."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import bigan_ref as C
from test_cont_oracle_golden import check_against_golden as check_packed
from util_cmp import assert_close


def check_against_golden(gold, p, twin, zero, steps):
    """test_cont_oracle_golden.check_against_golden (losses 2e-5, images 2e-5, gradient norms 2e-3, post-step state 1e-4) plus every
    GRAD_STRIDE-th element of every gradient tensor to 2e-3 of the tensor's largest recorded magnitude"""
    tensors = {}
    for k in C.IMAGES:
        if '%s/%s' % (p, k) in gold:
            tensors[k] = getattr(twin, k)
        else:       # the U-Net variant's second iteration: every UNET_IT1_STRIDE-th pixel
            assert_close(getattr(twin, k).reshape(-1)[::C.UNET_IT1_STRIDE], torch.from_numpy(gold['%s/samp/%s' % (p, k)]), 2e-5, k)
    check_packed(gold, p, twin.losses(), tensors, twin.grads, {'G': twin.netG, 'D': twin.netD, 'E': twin.netE}, zero, steps)
    for tag, gd in twin.grads.items():
        for k in gold['grad%s/keys' % tag]:
            if k in zero[tag]:
                continue
            ref = gold['%s/grad%s/samp/%s' % (p, tag, k)].astype(np.float64)
            got = gd[k].detach().reshape(-1)[::C.GRAD_STRIDE].double().numpy()
            scale = float(gd[k].detach().abs().max())
            assert np.abs(got - ref).max() <= 2e-3 * scale + 1e-7, 'grad%s %s samples: %g of %g' % (tag, k, np.abs(got - ref).max(), scale)


@pytest.mark.parametrize('name', list(C.VARIANTS))
def test_bigan_step_matches_reference(name):
    torch.set_num_threads(4)
    gold = np.load(C.fixture_path(name))
    assert list(gold['loss_names']) == C.LOSS_NAMES
    m, m64 = C.build_twin(name), C.build_twin(name, torch.float64)
    for it in range(2):
        for twin in (m64, m):
            torch.manual_seed(1234 + it)
            twin.set_input(C.batch(name, it))
            twin.optimize_parameters()
        zero = {tag: set(k for k, g in gd.items() if g is not None and float(g.norm()) < 1e-9) for tag, gd in m64.grads.items()}
        check_against_golden(gold, 'it%d' % it, m, zero, it + 1)


def _parse(argv):
    from pcgan_amd.options.train_options import TrainOptions
    old, sys.argv = sys.argv, argv
    try:
        options = TrainOptions()
        return options, options.parse()
    finally:
        sys.argv = old


def test_registry_resolves_wsgan_bigan():
    from pcgan_amd.models import find_model_using_name
    assert find_model_using_name('wsgan_bigan').__name__ == 'WSGANBiGANModel'


def test_parsed_defaults_equal_the_reference(tmp_path):
    gold = np.load(C.fixture_path('default'))
    options, opt = _parse(C.argv('default', str(tmp_path), 'E.pth', 'IP.pth', '-1'))
    recorded = dict(zip(gold['option_names'], gold['option_defaults']))
    mine = {k: str(options.parser.get_default(k)) for k in vars(opt)}
    for k, v in recorded.items():       # every option of the reference, with its default
        assert k in mine, 'option --%s of the reference is missing' % k
        assert mine[k] == v, '--%s: default %s, the reference has %s' % (k, mine[k], v)
    assert recorded['dataset_mode'] == 'wsgan_cycle' and recorded['loadSize'] == '128' and recorded['fineSize'] == '128'
    assert recorded['n_layers_D'] == '4' and recorded['batchSize'] == '10' and recorded['which_model_netG'] == 'unet_128'


def _model(tmp_path, extra=(), name='default'):
    """the model on the CPU, up to the point where it would need the GPU library: construction only"""
    from pcgan_amd.models import create_model
    _, opt = _parse(C.argv(name, str(tmp_path), str(tmp_path / 'E.pth'), str(tmp_path / 'IP.pth'), '-1') + list(extra))
    return create_model(opt)


def _checkpoints(tmp_path):
    from oracle import networks_ref as N
    from oracle import weights as W
    torch.save(C.encoder_base_weights(N.ResNetFeatureRef('resnet18').model.state_dict()), str(tmp_path / 'E.pth'))
    ip = N.AlexNetFeatureRef(3, 'None')
    torch.save(W.fill_state_dict(ip.state_dict(), C.SEED_IP), str(tmp_path / 'IP.pth'))


def test_names_match_the_fixture(tmp_path):
    gold = np.load(C.fixture_path('default'))
    _checkpoints(tmp_path)
    model = _model(tmp_path)
    assert model.name() == 'WSGANBiGANModel'
    assert model.loss_names == list(gold['loss_names']) == C.LOSS_NAMES
    assert model.visual_names == list(gold['visual_names']) and model.model_names == list(gold['model_names'])
    assert list(gold['current_visuals']) == ['real_x', 'fake_x', 'rec_x', 'attr_0', 'attr_1', 'attr_2']
    assert len(model.fixed_embeddings) == 3 and tuple(model.fixed_embeddings[0].shape) == (1, 1, 1, 1)
    assert [type(o).__name__ for o in model.optimizers] == ['FusedAdam'] * 3
    assert model.optimizers == [model.optimizer_G, model.optimizer_D, model.optimizer_E]       # the reference's list order
    first = [m for m in model.netD.modules() if isinstance(m, torch.nn.Conv2d)][0]
    assert first.weight.shape[1] == 3 + 1           # D reads the image and the rating
    assert list(model.netE.state_dict().keys()) == list(gold['afterE/keys'])
    assert list(model.netD.state_dict().keys()) == list(gold['afterD/keys'])
    assert model.test() is None


def test_refusals(tmp_path, monkeypatch):
    _checkpoints(tmp_path)
    with pytest.raises(NotImplementedError, match=r'\[unet_128\] is not a name of the MI355X hot path'):
        _model(tmp_path, ['--which_model_netG', 'unet_128'])
    with pytest.raises(NotImplementedError, match='--use_bicycle_E'):
        _model(tmp_path, ['--use_bicycle_E'])
    from pcgan_amd.hip import parallel
    monkeypatch.setattr(parallel, 'is_distributed', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match='a run of 2 ranks is not supported'):
        _model(tmp_path)


def test_generate_images_refuses_the_prior(tmp_path):
    import generate_images
    old = sys.argv
    try:
        with pytest.raises(ValueError, match='wsgan_bigan.*--how_to_sample prior'):
            generate_images.main(['--model', 'wsgan_bigan', '--how_to_sample', 'prior', '--dataroot', str(tmp_path), '--gpu_ids', '-1',
                                  '--output_dir', str(tmp_path / 'out'), '--checkpoints_dir', str(tmp_path), '--attr_bins', '[10, 30, 50]',
                                  '--which_model_netG', 'resnet_9blocks'])
    finally:
        sys.argv = old


def test_fused_concat_bwd_switch(monkeypatch):
    """the context is read when concat_z runs; it nests and restores; PCGAN_CONCATZ_FUSED=0 wins; a shared rating that needs a gradient
    keeps the chain outside the measured winning region (one workgroup walks all its planes), and so does a rating without a gradient.  (No launch: apply() is
    replaced, the tensors carry shapes only.)"""
    from pcgan_amd.hip import functional as HF
    import os
    assert HF._CONCATZ_FUSED_ENV is (os.environ.get('PCGAN_CONCATZ_FUSED', '1') != '0')
    taken = []
    monkeypatch.setattr(HF._ConcatZFn, 'apply', staticmethod(lambda img, z: taken.append('chain')))
    monkeypatch.setattr(HF._ConcatZFusedFn, 'apply', staticmethod(lambda img, z: taken.append('fused')))
    monkeypatch.setattr(HF, '_CONCATZ_FUSED_ENV', True)
    img, z = torch.empty(2, 3, 4, 4, device='meta'), torch.zeros(2, 1, 1, 1, requires_grad=True)
    HF.concat_z(img, z)
    with HF.fused_concat_bwd():
        HF.concat_z(img, z)
        with HF.fused_concat_bwd(False):
            HF.concat_z(img, z)
        HF.concat_z(img, z)
    HF.concat_z(img, z)
    with pytest.raises(KeyError):
        with HF.fused_concat_bwd():
            raise KeyError('x')
    HF.concat_z(img, z)
    assert taken == ['chain', 'fused', 'chain', 'fused', 'chain', 'chain']
    del taken[:]
    big32 = torch.empty(32, 3, 256, 256, device='meta')
    shared = torch.zeros(1, 1, 1, 1, requires_grad=True)
    assert (HF.FUSED_SHARED_MAX_PLANES, HF.FUSED_SHARED_MAX_BYTES) == (16, 640 << 10)
    cases = [(big32, shared, 'chain'),                                                  # 8 MiB of rating planes for one workgroup
             (big32, torch.zeros(32, 1, 1, 1, requires_grad=True), 'fused'),            # a rating per sample: one workgroup per plane
             (big32, torch.zeros(32, 1, 1, 1), 'chain'),                                # no gradient for the rating: one copy either way
             (img, z.detach(), 'chain'),
             (torch.empty(10, 3, 128, 128, device='meta'), shared, 'fused'),            # 640 KiB: measured, wins
             (torch.empty(11, 3, 128, 128, device='meta'), shared, 'chain'),
             (torch.empty(16, 3, 128, 128, device='meta', dtype=torch.bfloat16), shared, 'fused'),      # 512 KiB: measured, wins
             (torch.empty(16, 3, 128, 128, device='meta'), shared, 'chain'),            # 1 MiB: measured, loses
             (torch.empty(24, 3, 128, 128, device='meta', dtype=torch.bfloat16), shared, 'chain'),      # 768 KiB: measured, loses
             (torch.empty(17, 3, 8, 8, device='meta'), shared, 'chain'),                # few bytes, but 17 planes for one workgroup
             (torch.empty(1, 3, 512, 512, device='meta'), shared, 'fused')]             # batch 1: z_batch == N
    with HF.fused_concat_bwd():
        for a, b, _ in cases:
            HF.concat_z(a, b)
    assert taken == [want for _, _, want in cases]
    del taken[:]
    monkeypatch.setattr(HF, '_CONCATZ_FUSED_ENV', False)
    with HF.fused_concat_bwd():
        HF.concat_z(img, z)
    assert taken == ['chain']


def test_concat_z_bwd_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with another message (or crash)"""
    from pcgan_amd.hip import lib
    h = lib.load()
    dy, dimg, dz = 4096, 65536, 131072

    def call(*a):
        st = h.pcgan_concat_z_bwd(*a)
        return st, h.pcgan_last_error()
    for args, word in (((None, dimg, dz, 2, 3, 1, 16, 2, lib.F32, None), b'null pointer (dy)'),
                       ((dy, None, None, 2, 3, 1, 16, 2, lib.F32, None), b'no output wanted'),
                       ((dy, dimg, dz, 0, 3, 1, 16, 0, lib.F32, None), b'must be positive'),
                       ((dy, dimg, dz, 2, 0, 1, 16, 2, lib.F32, None), b'must be positive'),
                       ((dy, dimg, dz, 2, 3, 1, 0, 2, lib.F32, None), b'must be positive'),
                       ((dy, dimg, dz, -1, 3, 1, 16, -1, lib.F32, None), b'must be positive'),
                       ((dy, dimg, dz, 2, 3, 0, 16, 2, lib.F32, None), b'nz = 0'),
                       ((dy, dimg, dz, 2, 3, -2, 16, 2, lib.F32, None), b'nz = -2'),
                       ((dy, dimg, dz, 4, 3, 1, 16, 2, lib.F32, None), b'z batch 2 must be 1 or N = 4'),
                       ((dy, dimg, dz, 4, 3, 1, 16, 0, lib.F32, None), b'z batch 0'),
                       ((dy, dimg, dz, 2, 3, 1, 16, 2, 7, None), b'dtype'),
                       ((dy, dimg, dz, 1 << 15, 3, 1, 1 << 16, 1 << 15, lib.F32, None), b'overflow int'),        # 2^15 * 4 * 2^16 = 2^33
                       ((dy, None, dz, 4, 2147483647, 1, 1, 4, lib.BF16, None), b'overflow int'),                # C + nz
                       ((dy, dimg, None, 1 << 20, 1 << 10, 1, 2, 1, lib.F32, None), b'overflow int')):           # elements AND workgroups
        st, msg = call(*args)
        assert st != 0 and b'concat_z_bwd' in msg and word in msg, (args, msg)
