"""The case table of tests/test_gpu_conv_f32.py (tests/conv_f32_cases.py), checked without a GPU: every case satisfies the condition that
makes its gate bite, is ragged the way it claims, and names a launch record that the host's routing -- restated in conv_f32_cases.plan --
gives for it.  The GPU test then holds the same record against what the library says it launched."""
import pytest

import conv_f32_cases as T

NAMES = list(T.BY_NAME)


@pytest.mark.parametrize('name', NAMES)
def test_case(name):
    c = T.BY_NAME[name]
    pl = T.plan(c)
    # the expected record is self-consistent: legal values, and what the routing gives
    form, mode, bm, bp, ks, nphase = c.want
    assert T.record(pl) == c.want, 'the routing gives %r, the case expects %r' % (T.record(pl), c.want)
    assert mode == ('fwd_reflect' if c.geom[9] else 'fwd_zero') if c.pass_ == 'fwd' else mode in ('dgrad', 'dgrad_reflect')
    assert 1 <= ks <= 8 and 1 <= nphase <= 16
    if form == 'smallm':
        assert pl.M <= 4 and ((bm == 1 and bp in (43, 44, 73, 74) and (bp % 10 == 3) == (pl.M <= 3)) or (bm in (2, 3) and bp == 0 and ks == 1))
        assert mode != 'dgrad_reflect'
    else:
        assert pl.M > 4 and (bm, bp) in ((128, 128), (128, 64), (64, 128), (64, 64), (32, 128)) and (bm == 32) == (pl.M <= 32)
        assert (form == 'igemm2_cg16') == (pl.Cg % 16 == 0 and c.geom[5] * c.geom[6] <= T.NTAP_FWD)
        assert (form == 'igemm2_cg4') == (pl.Cg <= 4 and c.geom[5] * c.geom[6] <= T.NTAP_CG4)
        assert mode != 'dgrad_reflect' or form == 'igemm2_cg16'
        assert pl.M > 32 or (c.tile == 0 and c.ks == 0), 'the forcing options do not reach layers of <= 32 rows'
    assert T.instantiation(c, c.want) in T.all_instantiations()
    # ragged in the way the case claims
    for claim in c.claims:
        assert T.CLAIMS[claim](pl), 'the case claims %r: %r' % (claim, pl)
    # the condition: the bound is under half the smallest term, in every element
    d = T.data(c)
    terms = float(d.A.max()) / T.TERM_MIN
    worst = T.condition(c, pl)
    assert worst < T.TERM_MIN / 2, 'the largest bound %.4f (up to %d terms, max |ref| %.1f) would not catch one lost term' % (
        worst, terms, float(d.ref.abs().max()))
    assert d.ref.shape == d.A.shape and bool((d.A >= d.ref.abs() - 1e-9).all())
    if c.bias and not pl.need_zero:
        assert float(d.A.min()) >= T.TERM_MIN, 'every element sums at least one term'


def test_table_covers_every_instantiation():
    """100 fp32-MFMA and 36 small-M instantiations, each named by at least one case's expected record"""
    want = {T.instantiation(c, c.want) for c in T.CASES}
    every = T.all_instantiations()
    assert len(every) == 136 and len(set(every)) == 136
    assert sorted(set(every) - want) == [] and want <= set(every)


def test_sections_hold_what_they_name():
    by = lambda sect: [c for c in T.CASES if c.sect == sect]
    assert {c.want[0] for c in by('A')} == {'igemm2_cg16'} and {c.want[0] for c in by('B')} == {'igemm2_cg4'}
    assert {c.want[0] for c in by('D')} == {'smallm'}
    plans = [(c, T.plan(c)) for c in T.CASES]
    assert {pl.Cg for c, pl in plans if c.want[0] == 'igemm'} >= {5, 8, 12, 20, 24}
    assert any(T.CLAIMS['empty_slice'](pl) for c, pl in plans if c.want[0] == 'igemm2_cg16')
    for half in (False, True):      # the padded reflect fallback, a plane under 2 pad + 2, a reflect gradient with a bias: both storage types
        assert any(pl.padded and c.half == half for c, pl in plans)
        assert any(pl.padded and pl.small_plane and c.half == half and c.want[0] == 'igemm' and pl.Cg % 16 != 0 for c, pl in plans)
        assert any(pl.padded and c.bias and c.half == half for c, pl in plans) and any(pl.padded and not c.bias and c.half == half for c, pl in plans)
        assert any(c.want[1] == 'dgrad_reflect' and c.bias and c.half == half for c, pl in plans)
    assert {c.act for c in by('E')} == {0, 1, 2, 3, 4}
