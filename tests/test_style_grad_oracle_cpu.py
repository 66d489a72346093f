"""The style-gradient oracle (tests/style_grad_oracle.py) against itself, on the CPU: every emulation stays inside the bar its kernel
family is held to, and each seeded defect breaks the criterion named for it -- so the bars of tests/test_gpu_style_grad.py are neither
out of a correct kernel's reach nor blind to these defects."""
import numpy as np
import pytest

import style_grad_oracle as so

F32 = np.float32
SHAPES = [(48, 33), (64, 35), (128, 36), (200, 165), (512, 630)]
_cache = {}


def case(C, hw):
    """D, F, the bf16 copy of F, c2 and both references -- computed once per shape and shared (never modified)."""
    if (C, hw) not in _cache:
        D, F = so.make_data(C, hw)
        F16 = so.bf16_nearest(F)
        c2 = so.c2_of(C, C * hw)
        d = dict(D=D, F=F, F16=F16, c2=c2, ref=so.reference(D, F, c2), ref16=so.reference(D, F16, c2))
        for a in (D, F, F16) + d['ref'] + d['ref16']:
            a.setflags(write=False)
        _cache[(C, hw)] = d
    return _cache[(C, hw)]


def operands(d, family):
    return (d['F16'], d['ref16']) if family == 'bf16' else (d['F'], d['ref'])


@pytest.mark.parametrize('C,hw', SHAPES)
@pytest.mark.parametrize('family', so.FAMILIES)
def test_emulation_stays_inside_its_per_element_bar(family, C, hw):
    d = case(C, hw)
    F, (S_ref, B) = operands(d, family)
    S = so.EMULATE[family](d['D'], F, d['c2'])
    r = so.worst_ratio(S, S_ref, so.bar(family, C) * B)
    print('%s C %d hw %d: worst |S - S_ref| / (bar B) = %.3g, rel-L2 %.3g' % (family, C, hw, r, so.rel_l2(S, S_ref)))
    assert r <= 1.0


@pytest.mark.parametrize('C,hw', SHAPES)
@pytest.mark.parametrize('family', so.FAMILIES)
def test_scaled_epilogue_of_the_emulation_stays_inside_its_bound(family, C, hw):
    """dst = coef * S + b in float32 (one rounding each), against the float64 value: the bound of the scaled epilogues."""
    d = case(C, hw)
    F, (S_ref, B) = operands(d, family)
    S = so.EMULATE[family](d['D'], F, d['c2'])
    coef = F32(1.0) / F32(np.sqrt(np.mean(S.astype(np.float64) ** 2)))
    base = (np.random.RandomState(C + hw).randn(*S.shape) * 0.7).astype(F32)
    for b in (None, base):
        dst = coef * S if b is None else (coef * S + b).astype(F32)
        want = float(coef) * S_ref + (0.0 if b is None else b.astype(np.float64))
        assert so.worst_ratio(dst, want, so.scaled_bound(family, C, coef, S_ref, B, b)) <= 1.0


@pytest.mark.parametrize('C,hw', SHAPES)
def test_one_dropped_product_breaks_the_per_element_bar(C, hw):
    d = case(C, hw)
    S_ref, B = d['ref']
    # a product that is not zero (the features are ReLU'd: half of them are)
    m, p = C // 3, hw // 2
    j = int(np.argmax(np.abs(d['D'][m]) * d['F'][:, p]))
    assert d['D'][m, j] != 0 and d['F'][j, p] != 0
    S = so.emulate_fp32(d['D'], d['F'], d['c2'], drop_product=(m, j, p))
    bound = so.bar('fp32', C) * B
    err = np.abs(S.astype(np.float64) - S_ref)
    print('C %d hw %d: dropped product at %.3g x the bar' % (C, hw, err[m, p] / bound[m, p]))
    assert err[m, p] > bound[m, p]
    mask = np.ones_like(err, bool)
    mask[m, p] = False
    assert np.all(err[mask] <= bound[mask])          # ... and nothing else moved


@pytest.mark.parametrize('C,hw', SHAPES)
def test_the_lo_term_of_d_dropped_breaks_the_bf16_per_element_bar(C, hw):
    d = case(C, hw)
    S_ref, B = d['ref16']
    S = so.emulate_bf16(d['D'], d['F16'], d['c2'], drop_lo=True)
    err, bound = np.abs(S.astype(np.float64) - S_ref), so.bar('bf16', C) * B
    print('C %d hw %d: without lo, worst %.3g x the bar, %.0f %% of the elements over it' % (C, hw, so.worst_ratio(S, S_ref, bound), 100 * np.mean(err > bound)))
    assert so.worst_ratio(S, S_ref, bound) > 1.0


@pytest.mark.parametrize('C,hw', SHAPES)
@pytest.mark.parametrize('dropped', ['mm', 'hl'])
def test_a_dropped_low_order_product_breaks_the_split_aggregate_criterion(dropped, C, hw):
    """The aggregate criterion of the split family is two inequalities (style_grad_oracle.aggregate_ok): the rel-L2 one and the
    presence of every kept partial product.  With the kernels' split (head term rounded to nearest: the lower terms have random
    signs, a missing product is an incoherent error) the rel-L2 half alone sees a dropped product only at the small channel counts.
    Measured here, rel-L2 of the chain / without mm / without hl, and the factor the criterion needs above 3:
        (48, 33)    1.59e-7   1.22e-6 (7.6 x)   2.50e-6 (15.7 x)
        (64, 35)    1.81e-7   1.07e-6 (5.9 x)   1.77e-6 (9.8 x)
        (128, 36)   2.57e-7   8.19e-7 (3.2 x)   1.37e-6 (5.3 x)
        (200, 165)  3.00e-7   7.26e-7 (2.4 x)   1.22e-6 (4.1 x)
        (512, 630)  4.45e-7   6.01e-7 (1.3 x)   8.54e-7 (1.9 x)
    so it is asserted where the arithmetic supports it (defect above 3 x the chain) and the presence half at every shape: its
    coefficient is -1 for the dropped product and within 0.06 of 0 for the five others (the products are weakly correlated)."""
    d = case(C, hw)
    S_ref, _ = d['ref']
    emu = so.emulate_split(d['D'], d['F'], d['c2'])
    ok, fig = so.aggregate_ok('split', emu, S_ref, emu, d['D'], d['F'], d['c2'])
    assert ok, fig
    bad = so.emulate_split(d['D'], d['F'], d['c2'], drop=(dropped,))
    ok, fig = so.aggregate_ok('split', bad, S_ref, emu, d['D'], d['F'], d['c2'])
    print('C %d hw %d without %s: rel-L2 %.3g against %.3g (%.1f x), presence %s' % (
        C, hw, dropped, fig['rel_l2'], fig['rel_l2_emulation'], fig['rel_l2'] / fig['rel_l2_emulation'],
        {k: round(v, 4) for k, v in fig['presence'].items()}))
    assert not ok
    assert abs(fig['presence'][dropped] + 1) <= 0.2
    assert all(abs(v) <= 0.2 for k, v in fig['presence'].items() if k != dropped)
    # the rel-L2 half on its own, wherever the defect is more than 3 x the chain's own error
    if C <= 128 or (dropped == 'hl' and C == 200):
        assert fig['rel_l2'] > so.AGG_MARGIN * fig['rel_l2_emulation']
