"""CPU: the online pair selection -- the float64 restatement (tests/online_ref.py) against what the reference's own classes computed
(tests/golden/online_select.npz, written by scripts/make_online_golden.py), its tie rule, the C entry's argument validation (before
any launch, so it runs without a GPU), the checks of ops.online_pair_bce, and siamese_online.py's parser, refusals and data set.

Bounds against the golden file (the reference computes in fp32): each fp32 logsigmoid term of the reference is off by at most about
4 ulp and the pairwise mean over up to 4096 terms adds at most log2(4096) = 12 more, so |loss - golden| <= 16 * 2^-24 * mean|term|
(observed worst case over these shapes: 2.6 such units); |grad - golden| <= 4 * 2^-24 / k (observed 1.74); the regularization terms
are held to the same 16 units relative to their own value.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import online_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'online_select.npz')
U24 = 2.0 ** -24
CASES = [(1, 1), (2, 5), (12, 5), (100, 100), (100, 37), (1024, 300), (4096, 4096)]


def golden_case(gold, N, max_kept, hard):
    tag = '%d_%d_%s' % (N, max_kept, 'hard' if hard else 'easy')
    return {k: gold['%s/%s' % (tag, k)] for k in ('f1', 'f2', 'label', 'sel', 'pseudo', 'loss', 'df1', 'df2', 'reg')}


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def test_golden_holds_every_case(gold):
    assert [tuple(c) for c in gold['cases'].tolist()] == CASES


@pytest.mark.parametrize('hard', [True, False], ids=['hard', 'easy'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%d' % c)
def test_restatement_against_the_reference(gold, case, hard):
    N, max_kept = case
    g = golden_case(gold, N, max_kept, hard)
    k = min(N, max_kept)
    lam = float(gold['lambda_reg'])
    ref = R.online_pair_bce(g['f1'], g['f2'], g['label'], k, not hard, 0.16, 0.0)
    assert np.array_equal(ref['sel'], g['sel'].astype(np.int32)) and np.array_equal(ref['pseudo'], g['pseudo'].astype(np.int32))
    assert ref['min_key_gap'] > 0 or N == 1, 'the golden keys are pairwise distinct'
    unit = U24 * ref['mean_abs_term']
    err = abs(ref['loss'][0] - float(g['loss']))
    print('N %d k %d %s: loss error %.2f units' % (N, k, 'hard' if hard else 'easy', err / unit))
    assert err <= 16 * unit
    assert ref['loss'][1] == 0.0 and ref['loss'][2] == ref['loss'][0]
    gerr = max(np.abs(ref['df1'] - g['df1']).max(), np.abs(ref['df2'] - g['df2']).max())
    print('gradient error %.2f units' % (gerr / (U24 / k)))
    assert gerr <= 4 * U24 / k
    # the regularizer: (mean(f1^2), mean(f2^2), lambda (sum)) of the two torch fp32 expressions
    reg = R.online_pair_bce(g['f1'], g['f2'], g['label'], k, not hard, 0.16, lam)
    lam32 = float(np.float32(lam))
    m1 = float(np.mean(g['f1'].astype(np.float64) ** 2))
    m2 = float(np.mean(g['f2'].astype(np.float64) ** 2))
    for mine, theirs in ((m1, g['reg'][0]), (m2, g['reg'][1]), (reg['loss'][1], g['reg'][2])):
        assert abs(mine - float(theirs)) <= 16 * U24 * abs(mine)
    assert abs(reg['loss'][1] - lam32 * (m1 + m2)) <= 1e-15 * abs(reg['loss'][1]) and reg['loss'][0] == ref['loss'][0]
    assert np.array_equal(reg['sel'], ref['sel']) and np.array_equal(reg['pred'], ref['pred'])
    # d (lambda mean(f^2)) / d f on top of the selection's gradient
    assert np.allclose(reg['df1'] - ref['df1'], lam32 * 2.0 * g['f1'].astype(np.float64) / N, rtol=0, atol=1e-15 * (1 + np.abs(g['f1']).max()))


@pytest.mark.parametrize('N', [2, 64, 1025])
def test_tie_rule_of_the_restatement(N):
    """+-d pairs give exactly equal keys: ascending takes the lower index first, descending is the exact reverse; an all-equal key
    array gives 0 .. N - 1 or its reverse"""
    half = N // 2
    d = (1.0 + np.arange(half, dtype=np.float32) % 7)                 # 7 distinct distances, each many times, +d and -d
    s = np.concatenate([d, -d, np.full(N - 2 * half, 0.5, dtype=np.float32)])
    f2 = np.linspace(-1, 1, N).astype(np.float32) * 0                # s = f1 - f2 exactly
    f1 = s + f2
    label = np.arange(N) % 3
    up = R.online_pair_bce(f1, f2, label, N, False, 0.16, 0.0)['order']
    down = R.online_pair_bce(f1, f2, label, N, True, 0.16, 0.0)['order']
    key = (s * s).astype(np.float32)
    for a, b in zip(up[:-1], up[1:]):
        assert key[a] < key[b] or (key[a] == key[b] and a < b)
    assert np.array_equal(down, up[::-1])
    same = np.full(N, 2.0, dtype=np.float32)
    assert np.array_equal(R.online_pair_bce(same, f2, label, 1, False, 0.16, 0.0)['order'], np.arange(N))
    assert np.array_equal(R.online_pair_bce(same, f2, label, 1, True, 0.16, 0.0)['order'], np.arange(N)[::-1])
    # an explicit key: -0 == +0, inf before NaN, NaN last
    if N >= 6:
        k6 = np.array([np.nan, np.inf, 0.0, -0.0, -np.inf, 3.0], dtype=np.float32)
        assert R.order_of(k6, False).tolist() == [4, 2, 3, 5, 1, 0] and R.order_of(k6, True).tolist() == [0, 1, 5, 3, 2, 4]


def test_entry_validates_before_any_launch():
    from pcgan_amd.hip import lib
    h = lib.load()
    buf = (ctypes.c_float * 8)()
    lab = (ctypes.c_int64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    lp = ctypes.cast(lab, ctypes.c_void_p)

    def call(f1, f2, label, N, k):
        return h.pcgan_online_pair_bce(f1, f2, label, None, None, None, None, None, N, k, 0, 0.16, 0.0, 1.0, None)
    for N, k, the_range in ((0, 1, b'1 <= N <= 4096'), (4097, 1, b'1 <= N <= 4096'), (8, 0, b'1 <= k <= N'), (8, 9, b'1 <= k <= N')):
        assert call(p, p, lp, N, k) != 0
        msg = h.pcgan_last_error()
        assert b'online_pair_bce' in msg and the_range in msg, msg
    for args in ((None, p, lp), (p, None, lp), (p, p, None)):
        assert call(*args, 8, 4) != 0
        assert b'online_pair_bce' in h.pcgan_last_error() and b'null' in h.pcgan_last_error()


def test_op_refuses_cpu_tensors_and_mismatched_sizes():
    from pcgan_amd.hip import ops
    f = torch.zeros(8)
    lab = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='GPU tensors'):
        ops.online_pair_bce(f, f.clone(), lab, 4, False, 0.16, 0.0)
    with pytest.raises(RuntimeError, match='online_pair_bce: f2 of shape'):
        ops.online_pair_bce(f, torch.zeros(7), lab, 4, False, 0.16, 0.0)
    with pytest.raises(RuntimeError, match='online_pair_bce: label of shape'):
        ops.online_pair_bce(f, f.clone(), lab[:5], 4, False, 0.16, 0.0)
    with pytest.raises(RuntimeError, match='online_pair_bce: key of shape'):
        ops.online_pair_bce(f, f.clone(), lab, 4, False, 0.16, 0.0, key=torch.zeros(9))


# ---- siamese_online.py: parser, refusals, data set -------------------------------------------------------------------------------------
# the reference's defaults (siamese_online.py:28-80); display_id is this project's -1
DEFAULTS = dict(mode='train', name='exp', datafile='', pretrained_model_path='', checkpoint_dir='checkpoints', save_epoch_freq=5,
                num_workers=4, num_epochs=1, batch_size=100, lr=2e-4, which_epoch='latest', which_model='resnet18', pooling='avg',
                loadSize=224, fineSize=224, gpu_ids='0', weight=[], dropout=0.05, finetune_fc_only=False, fc_dim=[], fc_relu_slope=0.3,
                cnn_dim=[64, 1], cnn_pad=1, cnn_relu_slope=0.7, use_cxn=False, lambda_regularization=0.0, lambda_contrastive=0.0,
                print_freq=50, display_id=-1, transforms='resize_affine_crop', affineScale=[0.95, 1.05], affineDegrees=5,
                use_color_jitter=False, no_flip=False, continue_train=False, epoch_count=1, min_kept=1, max_kept=-1, save_latest_freq=10,
                pair_selector_type='random', serial_batches=False, draw_prob_thresh=0.16, a=1.0, use_pseudo_label=False)


def test_parser_defaults_are_the_references():
    import siamese_online as SO
    opt = SO.build_parser().parse_args(['--dataroot', 'synthetic'])
    for k, v in DEFAULTS.items():
        assert getattr(opt, k) == v, k
    opt = SO.get_options(['--dataroot', 'synthetic', '--pair_selector_type', 'hard', '--batch_size', '24', '--num_epochs', '7'], save=False)
    assert opt.max_kept == 24 and opt.num_epochs == 1
    assert SO.get_options(['--dataroot', 'synthetic', '--pair_selector_type', 'easy', '--max_kept', '5'], save=False).max_kept == 5


@pytest.mark.parametrize('argv', [[], ['--pair_selector_type', 'random'], ['--pair_selector_type', 'softmax_hard'],
                                  ['--pair_selector_type', 'softmax_easy'], ['--pair_selector_type', 'hard', '--mode', 'test'],
                                  ['--pair_selector_type', 'hard', '--which_model', 'alexnet'],
                                  ['--pair_selector_type', 'hard', '--finetune_fc_only'], ['--pair_selector_type', 'hard', '--fc_dim', '8'],
                                  ['--pair_selector_type', 'hard', '--use_cxn'], ['--pair_selector_type', 'hard', '--pooling', ''],
                                  ['--pair_selector_type', 'hard', '--cnn_dim', '64', '2']], ids=lambda a: ' '.join(a) or 'defaults')
def test_what_the_reference_cannot_run_is_refused(argv):
    import siamese_online as SO
    with pytest.raises(NotImplementedError, match='pcgan_amd'):
        SO.get_options(['--dataroot', 'synthetic'] + argv, save=False)


def test_selector_refusal_says_why():
    import siamese_online as SO
    with pytest.raises(NotImplementedError, match="reference's own loop cannot run"):
        SO.get_options(['--dataroot', 'synthetic'], save=False)


def test_more_than_one_process_is_refused(monkeypatch):
    import siamese_online as SO
    monkeypatch.setenv('WORLD_SIZE', '2')
    monkeypatch.setenv('RANK', '0')
    monkeypatch.setenv('LOCAL_RANK', '0')
    with pytest.raises(NotImplementedError, match='ONE process'):
        SO.get_options(['--dataroot', 'synthetic', '--pair_selector_type', 'hard'], save=False)


def test_datafile_label_out_of_range_names_the_line(tmp_path):
    import siamese_online as SO
    path = tmp_path / 'pairs.txt'
    path.write_text('a.png b.png 0\n\nc.png d.png 2\ne.png f.png 3\n')
    with pytest.raises(ValueError, match='line 4'):
        SO.parse_pair_lines(str(path), 1 << 30)
    path.write_text('a.png b.png 0\n\nc.png d.png 2\ne.png f.png 1')
    assert SO.parse_pair_lines(str(path), 1 << 30) == ['a.png b.png 0\n', 'c.png d.png 2\n', 'e.png f.png 1\n']
    assert SO.parse_pair_lines(str(path), 2) == ['a.png b.png 0\n', 'c.png d.png 2\n']


def test_synthetic_labels_follow_the_reversed_convention():
    """label 0 when the FIRST hidden score is higher: siamese.py's synthetic labels with 0 and 2 exchanged; items end in (label, index)"""
    import siamese as S
    import siamese_online as SO
    opt = SO.get_options(['--dataroot', 'synthetic', '--pair_selector_type', 'hard', '--fineSize', '8', '--batch_size', '4',
                          '--max_dataset_size', '40'], save=False)
    mine, theirs = SO.OnlinePairDataset(opt, 'synthetic', ''), S.PairDataset(opt, 'synthetic', '')
    assert len(mine) == len(theirs) == 40 and len(mine.text) == 40
    seen = set()
    for i in range(40):
        a0, b0, lab, idx = mine[i]
        a1, b1, other = theirs[i]
        assert torch.equal(a0, a1) and torch.equal(b0, b1) and int(idx) == i
        assert int(lab) == 2 - int(other)
        brighter_first = float(a0.mean()) > float(b0.mean())
        if int(lab) != 1:
            assert (int(lab) == 0) == brighter_first
        assert mine.text[i] == 'syn_%05d_A.png syn_%05d_B.png %d\n' % (i, i, int(lab))
        seen.add(int(lab))
    assert seen == {0, 1, 2}


def test_log_writes_kept_then_pseudo_lines(tmp_path):
    """OnlineLog.record on a hand-made picks buffer: the original lines of sel, "<a> <b> <pred>" for pseudo, the reference's counters"""
    import siamese_online as SO
    opt = SO.get_options(['--dataroot', 'synthetic', '--pair_selector_type', 'hard', '--use_pseudo_label', '--checkpoint_dir', str(tmp_path),
                          '--name', 'x'], save=False)
    os.makedirs(tmp_path / 'x')
    text = ['a%d b%d %d\n' % (i, i, i % 3) for i in range(10)]
    log = SO.OnlineLog(opt, text)
    index = np.array([7, 3, 9, 0])                                    # the batch's dataset indices
    label = np.array([1, 0, 0, 0])                                    # = text labels of 7, 3, 9, 0
    picks = np.array([2, 0, 1, 3, 0, 1, 2, 1], dtype=np.int32)        # sel (2, 0), pseudo (1, 3), pred (0, 1, 2, 1)
    log.record(picks, label, index)
    assert open(log.path).read() == 'a9 b9 0\na7 b7 1\na3 b3 1\na0 b0 1\n'
    assert (log.cnt_online, log.cnt_online_diff, log.wrong) == (2, 1, 4)
