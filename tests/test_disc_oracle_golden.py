"""wsgan_disc, the class-label CGAN baseline, on the CPU: the plain-torch twin of its step (tests/disc_ref.py) against the vectors
captured from the reference itself (scripts/make_disc_golden.py -> tests/golden/disc_step*.npz, tolerances of
test_cont_oracle_golden.py), the label draws, the plugin registry, the parsed defaults, define_AC, the class-grouped data set, the image
pool's draws and a plain-torch restatement of its data path against the reference's pool (tests/golden/disc_pool.npz), and the argument
checks of pcgan_pool_exchange that need no GPU.

Draws: the fixtures hold what the reference drew under Python <= 3.10.  On such an interpreter (disc_ref.REFERENCE_DRAWS) the twin
draws for itself and the draws are ASSERTED equal to the recorded ones; on a newer one, whose random.sample may pick differently for the
same seed, the label triple and the pool's plan are set from the fixture and that one assertion is skipped over."""
import ctypes
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import disc_ref as C
from test_cont_oracle_golden import check_against_golden, _parse


@pytest.mark.parametrize('name', list(C.VARIANTS))
def test_disc_step_matches_reference(name):
    torch.set_num_threads(4)
    gold = np.load(C.fixture_path(name))
    assert list(gold['loss_names']) == C.LOSS_NAMES
    assert list(gold['visual_names']) == ['real_A', 'fake_B', 'real_B', 'rec_A'] and list(gold['model_names']) == ['G', 'D', 'AC']
    m, m64 = C.build_twin(name), C.build_twin(name, torch.float64)
    for it in range(C.iterations(name)):
        for twin in (m64, m):
            C.step(twin, name, it, gold)
        zero = {tag: set(k for k, g in gd.items() if g is not None and float(g.norm()) < 1e-9) for tag, gd in m64.grads.items()}
        if C.REFERENCE_DRAWS:
            assert [m.label_A, m.label_B, m.label_B_not] == [int(v) for v in gold['it%d/labels' % it]]
        if name == 'pool':
            assert m.pool_plan == [int(v) for v in gold['it%d/pool_plan' % it]]
            ref = float(gold['it%d/pool_sum' % it])
            assert abs(float(m.fake_B_from_pool.double().sum()) - ref) <= 2e-5 * m.fake_B.numel(), 'the batch D saw, iteration %d' % it
        check_against_golden(gold, 'it%d' % it, m.losses(), {'fake_B': m.fake_B, 'rec_A': m.rec_A}, m.grads,
                             {'G': m.netG, 'D': m.netD, 'AC': m.netAC}, zero, it + 1)


def test_pool_variant_fills_then_exchanges():
    """what makes the `pool` fixture worth having: label_B is 1 in every step, so ONE pool fills inside the first batch, and a later
    query both exchanges and passes"""
    gold = np.load(C.fixture_path('pool'))
    plans = [[int(v) for v in gold['it%d/pool_plan' % it]] for it in range(3)]
    assert all(int(gold['it%d/labels' % it][1]) == 1 for it in range(3))
    assert plans[0][:3] == [0, 2, 4] and len(plans[0]) == 4
    later = plans[0][3:] + plans[1] + plans[2]
    assert any(p >= 0 and p % 2 == 1 for p in later), plans
    assert all(p < 0 or p % 2 == 1 for p in later), plans


def test_registry_resolves_wsgan_disc():
    from pcgan_amd.data import find_dataset_using_name
    from pcgan_amd.models import find_model_using_name
    assert find_model_using_name('wsgan_disc').__name__ == 'WSGANDiscModel'
    assert find_dataset_using_name('wsgan_disc').__name__ == 'WSGANDiscDataset'


def test_parsed_defaults_equal_the_reference(tmp_path):
    gold = np.load(C.fixture_path('default'))
    options, opt = _parse(C.argv('default', str(tmp_path), 'AC.pth', 'IP.pth', '-1'))
    recorded = dict(zip(gold['option_names'], gold['option_defaults']))
    mine = {k: str(options.parser.get_default(k)) for k in vars(opt)}
    for k, v in recorded.items():       # every option of the reference, with its default
        assert k in mine, 'option --%s of the reference is missing' % k
        assert mine[k] == v, '--%s: default %s, the reference has %s' % (k, mine[k], v)
    for key, v in (('dataset_mode', 'wsgan_disc'), ('n_layers_D', '4'), ('batchSize', '10'), ('pool_size', '0'), ('which_model_netG', 'unet_128'),
                   ('embedding_nc', '5'), ('which_model_netAC', 'resnet18'), ('lambda_AC', '1'), ('label_as_group', 'False')):
        assert recorded[key] == v, key


def test_define_AC_names_and_refusals():
    from pcgan_amd.models import networks
    torch.manual_seed(0)
    net = networks.define_AC('resnet18', 3, 'normal', 4, pooling='max', dropout=0.1, gpu_ids=[])
    assert isinstance(net, networks.ResNet) and tuple(net.model.fc.weight.shape) == (4, 512)
    assert list(net.state_dict())[0] == 'model.conv1.weight' and list(net.state_dict())[-1] == 'model.fc.bias'
    assert tuple(networks.define_AC('resnet50', 3, 'normal', 3).model.fc.weight.shape) == (3, 2048)
    assert isinstance(networks.define_AC('resnet34', 3, 'normal', 3), networks.ResNet)
    for which in ('alexnet', 'alexnet_lite', 'resnet101', 'resnet152'):
        with pytest.raises(NotImplementedError, match='hot path'):
            networks.define_AC(which, 3, 'normal', 3)
    with pytest.raises(NotImplementedError, match='not recognized'):
        networks.define_AC('vgg16', 3, 'normal', 3)


# ---- the data set ----------------------------------------------------------------------------------------------------------------------
ATTRS = (12, 25, 31, 40, 44, 52, 18, 7)            # bins [10, 30, 50, inf): 7 matches no bin and falls to the LAST class (reference quirk)
GROUPS = [[0, 1, 6], [2, 3, 4], [5, 7]]


def _folder(tmp_path, second_column=None):
    from PIL import Image
    rs = np.random.RandomState(3)
    names = ['%d_x%d.png' % (attr, i) for i, attr in enumerate(ATTRS)]
    for n in names:
        Image.fromarray(rs.randint(0, 256, size=(40, 40, 3), dtype=np.uint8)).save(str(tmp_path / n))
    lines = [n if second_column is None else '%s %s' % (n, second_column[i]) for i, n in enumerate(names)]
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    return names


def _dataset(tmp_path, extra=()):
    from pcgan_amd.data import create_dataset
    argv = ['train.py', '--dataroot', str(tmp_path), '--model', 'wsgan_disc', '--gpu_ids', '-1', '--checkpoints_dir', str(tmp_path / 'ck'),
            '--sourcefile_A', str(tmp_path / 'list.txt'), '--loadSize', '40', '--fineSize', '32', '--serial_batches', '--no_flip',
            '--display_id', '-1', '--num_classes', '3', '--embedding_nc', '3', '--attr_bins', '[10, 30, 50]'] + list(extra)
    _, opt = _parse(argv)
    ds = create_dataset(opt)
    ds.external_shuffle = True          # keep the list order: the reshuffle is tested on its own
    return ds, opt


def test_dataset_group_lists_and_modulo_indexing(tmp_path):
    names = _folder(tmp_path)
    ds, opt = _dataset(tmp_path)
    assert ds.name() == 'WSGANDiscDataset' and ds.attr_group_list == GROUPS and ds.attr_group_list_len == [3, 3, 2]
    assert len(ds) == 3 and ds.attrs == [float(a) for a in ATTRS]
    for i in range(5):          # past the length: the index is taken modulo each list
        item = ds[i]
        assert sorted(item, key=str) == [0, 1, 2, 'path_0', 'path_1', 'path_2']
        for L in range(3):
            assert item['path_%d' % L] == os.path.join(str(tmp_path), names[GROUPS[L][i % len(GROUPS[L])]])
            assert tuple(item[L].shape) == (3, 32, 32) and float(item[L].min()) >= -1.0 and float(item[L].max()) <= 1.0
    batch = torch.utils.data.default_collate([ds[0], ds[1]])
    assert tuple(batch[2].shape) == (2, 3, 32, 32) and len(batch['path_2']) == 2
    # the reference reshuffles every class list whenever the length is taken; a generator can be handed in
    ds.external_shuffle = False
    random.seed(5)
    assert len(ds) == 3 and [sorted(g) for g in ds.attr_group_list] == GROUPS and ds.attr_group_list != GROUPS
    a, _ = _dataset(tmp_path)
    b, _ = _dataset(tmp_path)
    a.reshuffle(random.Random(9))
    b.reshuffle(random.Random(9))
    assert a.attr_group_list == b.attr_group_list and a.attr_group_list != GROUPS


def test_dataset_label_as_group(tmp_path):
    _folder(tmp_path, second_column=[2, 2, 0, 1, 1, 0, 2, 1])
    ds, opt = _dataset(tmp_path, ['--label_as_group'])
    assert opt.label_as_group is True
    assert ds.attr_group_list == [[2, 5], [3, 4, 7], [0, 1, 6]] and len(ds) == 3 and ds.attrs[:3] == [2.0, 2.0, 0.0]
    # without the flag the second column is the ATTRIBUTE, binned like any other: all below 10 -> the last class
    plain, _ = _dataset(tmp_path)
    assert plain.attr_group_list == [[], [], list(range(8))]
    # the flag belongs to the model's TRAINING options: a test-time option set has none, and the data set reads it as False
    from pcgan_amd.data.wsgan_disc_dataset import WSGANDiscDataset
    o = SimpleNamespace(**{k: v for k, v in vars(opt).items() if k != 'label_as_group'})
    t = WSGANDiscDataset()
    t.initialize(o)
    assert t.attr_group_list == plain.attr_group_list


def test_dataset_gray_mix(tmp_path):
    _folder(tmp_path)
    ds, _ = _dataset(tmp_path, ['--input_nc', '1', '--output_nc', '1', '--loadSize', '32'])      # (no room for a random crop offset)
    rgb, _ = _dataset(tmp_path, ['--loadSize', '32'])
    g, c = ds[1], rgb[1]
    for L in range(3):
        assert tuple(g[L].shape) == (1, 32, 32)
        assert torch.equal(g[L][0], c[L][0] * 0.299 + c[L][1] * 0.587 + c[L][2] * 0.114)


def test_dataset_raw_form_synthetic_and_int_key_filing(tmp_path):
    from pcgan_amd.data import create_dataset, CustomDatasetDataLoader, _collate_keep_raw
    _folder(tmp_path)
    ds, _ = _dataset(tmp_path, ['--gpu_transform'])
    item = ds[0]
    assert sorted(item) == ['0_aug', '0_raw', '1_aug', '1_raw', '2_aug', '2_raw', 'path_0', 'path_1', 'path_2']
    batch = _collate_keep_raw([ds[0], ds[1]])
    assert isinstance(batch['1_raw'], list) and len(batch['1_raw']) == 2 and batch['1_aug'].shape[0] == 2
    # the loader files a finished image under the int key when the stem is all digits, with input_nc channels; other stems as before
    loader = CustomDatasetDataLoader()
    loader.opt = SimpleNamespace(input_nc=1, output_nc=3)
    loader.gpu_transform = lambda raw, aug, out_channels: ('finished', len(raw), tuple(aug.shape), out_channels)
    batch.update({'A_raw': [0], 'A_aug': torch.zeros(1, 3), 'B_raw': [0], 'B_aug': torch.zeros(1, 3), '12_raw': [0, 0, 0], '12_aug': torch.zeros(3, 3)})
    done = loader._finish_on_gpu(batch)
    assert sorted(done, key=str) == [0, 1, 12, 2, 'A', 'B', 'path_0', 'path_1', 'path_2']
    assert done[1][:2] == ('finished', 2) and done[1][2][0] == 2 and done[1][3] == 1
    assert done[12][3] == 1 and done['A'][3] == 1 and done['B'][3] == 3
    _, opt = _parse(['train.py', '--dataroot', 'synthetic', '--model', 'wsgan_disc', '--gpu_ids', '-1', '--checkpoints_dir', str(tmp_path / 'ck'),
                     '--fineSize', '16', '--batchSize', '2', '--display_id', '-1', '--num_classes', '3', '--embedding_nc', '3',
                     '--attr_bins', '[10, 30, 50]'])
    syn = create_dataset(opt)
    assert len(syn) == 128
    items = [syn[i] for i in range(4)]
    assert all(sorted(it, key=str) == [0, 1, 2, 'path_0', 'path_1', 'path_2'] for it in items)
    assert all(tuple(it[L].shape) == (3, 16, 16) and float(it[L].min()) >= -1.0 and float(it[L].max()) < 1.0 for it in items for L in range(3))
    assert torch.equal(syn[3][2], items[3][2]) and not torch.equal(items[3][2], items[3][1]) and not torch.equal(items[2][2], items[3][2])


# ---- the image pool --------------------------------------------------------------------------------------------------------------------
def test_plan_encoding_is_the_librarys():
    from pcgan_amd.hip import lib
    assert lib.POOL_PASS == C.POOL_PASS == -1 and lib.POOL_PLAN_MAX == 64
    assert [lib.pool_store(s) for s in (0, 1, 5)] == [0, 2, 10] and [lib.pool_swap(s) for s in (0, 1, 5)] == [1, 3, 11]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pcgan_hip.h')).read()
    assert '#define PCGAN_POOL_PLAN_MAX 64' in header and 'util/image_pool.py:12-32' in header


@pytest.mark.parametrize('size', [3, 1])
def test_pool_restatement_and_plans_against_the_reference(size):
    """the reference's ImagePool over six seeded queries: the restatement returns its batches bit for bit under the recorded plans,
    and after random.seed(k) both the restatement and ImagePool.plan_for make the recorded decisions (randint, not random.sample: the
    same under every Python)"""
    from pcgan_amd.util.image_pool import ImagePool
    gold = np.load(os.path.join(C.GOLD, 'disc_pool.npz'))
    pool = torch.zeros(size, 2, 3, 5)
    for q in range(6):
        x, plan = torch.from_numpy(gold['size%d/q%d/x' % (size, q)]), [int(v) for v in gold['size%d/q%d/plan' % (size, q)]]
        y = C.pool_apply(pool, x, plan)
        assert torch.equal(y.view(torch.int32), torch.from_numpy(gold['size%d/q%d/y' % (size, q)]).view(torch.int32)), q
    recorded = [[int(v) for v in gold['size%d/q%d/plan' % (size, q)]] for q in range(6)]
    assert recorded[0][:size] == [2 * s for s in range(size)]                 # the fill phase, in slot order, no draw
    flat = [p for plan in recorded for p in plan][size:]
    assert any(p < 0 for p in flat) and any(p >= 0 for p in flat) and all(p < 0 or (p % 2 == 1 and p // 2 < size) for p in flat)
    for make in (C.PoolRef, ImagePool):
        random.seed(int(gold['seed']))
        p = make(size)
        assert [p.plan_for(4) for _ in range(6)] == recorded, make.__name__
    # the draws come only once the pool is full, uniform first and randint only above 0.5: the generator ends where the reference's does
    random.seed(int(gold['seed']))
    ref_state = random.getstate()
    p = ImagePool(size)
    p.plan_for(size)
    assert random.getstate() == ref_state and p.num_imgs == size


def test_image_pool_size_zero_and_shape_change():
    from pcgan_amd.util.image_pool import ImagePool
    x = torch.zeros(2, 1, 2, 2)
    state = random.getstate()
    assert ImagePool(0).query(x) is x and random.getstate() == state
    p = ImagePool(2)
    p.images = torch.zeros(2, 1, 2, 2)          # as after a first query
    p.num_imgs = 2
    state = random.getstate()
    for bad in (torch.zeros(2, 1, 2, 3), torch.zeros(2, 1, 2, 2, dtype=torch.bfloat16)):
        with pytest.raises(RuntimeError, match='ImagePool holds'):
            p.query(bad)
    assert random.getstate() == state           # refused before any draw


def test_pool_exchange_refuses_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail with another message (or crash)"""
    from pcgan_amd.hip import lib
    h = lib.load()
    before = lib.pool_exchange_launches()
    plan = (ctypes.c_int * 4)(0, 3, -1, 5)
    POOL, X, Y, n = 1 << 20, 2 << 20, 3 << 20, 16       # pool of 3 slots, 4 images of 16 fp32: 192 / 256 bytes

    def refused(*args):
        assert h.pcgan_pool_exchange(*args) != 0
        msg = h.pcgan_last_error()
        assert b'pool_exchange' in msg
        return msg
    assert b'null' in refused(None, 3, X, Y, plan, 4, n, lib.F32, None)
    assert b'null' in refused(POOL, 3, None, Y, plan, 4, n, lib.F32, None)
    assert b'null' in refused(POOL, 3, X, None, plan, 4, n, lib.F32, None)
    assert b'null' in refused(POOL, 3, X, Y, None, 4, n, lib.F32, None)
    assert b'n == 0' in refused(POOL, 3, X, Y, plan, 4, 0, lib.F32, None)
    assert b'n_img' in refused(POOL, 3, X, Y, plan, 0, n, lib.F32, None)
    assert b'n_img' in refused(POOL, 3, X, Y, plan, -2, n, lib.F32, None)
    assert b'pool_size' in refused(POOL, 0, X, Y, (ctypes.c_int * 4)(-1, -1, -1, -1), 4, n, lib.F32, None)
    assert b'slot 2 outside [0, 2)' in refused(POOL, 2, X, Y, plan, 4, n, lib.F32, None)          # 5 = exchange with slot 2
    assert b'slot' in refused(POOL, 3, X, Y, (ctypes.c_int * 4)(0, 6, -1, -1), 4, n, lib.F32, None)   # 6 = store into slot 3
    assert b'dtype' in refused(POOL, 3, X, Y, plan, 4, n, 7, None)
    assert b'x and y overlap' in refused(POOL, 3, X, X, plan, 4, n, lib.F32, None)
    assert b'x and y overlap' in refused(POOL, 3, X, X + 4 * n * 4 - 4, plan, 4, n, lib.F32, None)       # the last element of x
    assert b'x and pool overlap' in refused(X + 3 * n * 4, 3, X, Y, plan, 4, n, lib.F32, None)           # pool starts inside x
    assert b'y and pool overlap' in refused(Y - 3 * n * 4 + 4, 3, X, Y, plan, 4, n, lib.F32, None)       # pool ends inside y
    assert b'y and pool overlap' in refused(Y + 4 * n * 2 - 2, 3, X, Y, plan, 4, n, lib.BF16, None)      # bf16: the ranges are half as long
    assert lib.pool_exchange_launches() == before


def test_ops_pool_exchange_checks_shapes_and_types():
    from pcgan_amd.hip import ops
    with pytest.raises(RuntimeError, match='GPU tensors'):
        ops.pool_exchange(torch.zeros(2, 3), torch.zeros(1, 3), [-1])


def test_generate_images_accepts_wsgan_disc(tmp_path):
    """past the model guard: the run gets as far as loading the generator's checkpoint, which is not there"""
    import generate_images
    _folder(tmp_path)
    argv = ['--model', 'wsgan_disc', '--how_to_sample', 'label', '--dataset_mode', 'single', '--sourcefile_A', str(tmp_path / 'list.txt'),
            '--dataroot', str(tmp_path), '--name', 'none', '--checkpoints_dir', str(tmp_path / 'ck'), '--which_model_netG', 'resnet_2blocks',
            '--ngf', '8', '--loadSize', '32', '--fineSize', '32', '--num_classes', '3', '--embedding_nc', '3', '--attr_bins', '[10, 30, 50]',
            '--output_dir', str(tmp_path / 'out'), '--gpu_ids', '-1']
    old = sys.argv
    try:
        with pytest.raises(FileNotFoundError, match='latest_net_G.pth'):
            generate_images.main(argv)
        with pytest.raises(ValueError, match='wsgan_emb, wsgan_cont and wsgan_disc'):
            generate_images.main(['--model', 'wsgan_cycle'] + argv[2:])
    finally:
        sys.argv = old
