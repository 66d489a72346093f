"""tests/fused_style_oracle.py on the CPU, before anything runs on a GPU: the float64 conv backward-data is the oracle's; the exactly
rounded float32 chain stays inside the per-element bound and the aggregate criterion (so the bars are reachable); every seeded defect of
that chain fails at least one half of the criterion at every shape where the fused launch exists (so they are sharp).

Which half catches which defect (asserted below):
    lo_dropped        the presence coefficient of 'lo' (-1).  Per element it shows on masked elements, and on unmasked ones only while
                      the conv sum does not outweigh the style sum (test_a_dropped_lo_half_under_a_heavy_conv_sum_...)
    chunk_dropped     the presence coefficient of that chunk (-1), and per element
    left_pixel        per element; so is left_pixel_clipped_tile, the same defect in the pixels of the clipped last tile column only
                      (the shapes of CLIPPED whose width is no multiple of the 32-pixel tile)
    mask_after        per element (a masked element loses its style term: its bound has no conv part)
    no_coef           per element
    base_overwritten  per element
Shapes: the two smallest and the two largest of the GPU test and its fused shapes with clipped tiles, the fp32 form everywhere; the bf16-only form with its defects where the
fused launch exists (hw % 64 == 0) -- at one pixel the rounding of C elements leaves a presence coefficient no meaning."""
import numpy as np
import pytest

from oracle.caffe_net import conv3x3_backward_data

import fused_style_oracle as fo

SHAPES = ((1, 1), (5, 7), (16, 64), (17, 70))
# where the fused launch exists with a tile clipped at the blob's edge: in x and y; in x inside one tile; in y only
CLIPPED = ((12, 48), (16, 20), (10, 32))
CASES = ([(C, 64, s) for C in (64, 96, 128, 256) for s in SHAPES] + [(512, 64, s) for s in SHAPES[:2]] + [(64, 128, s) for s in SHAPES] +
         [(128, 128, (8, 32))] + [(C, 64, s) for C in (64, 256) for s in CLIPPED] + [(128, 128, s) for s in CLIPPED] +
         [(512, 128, (8, 32))])
ELEMENT_DEFECTS = ('chunk_dropped', 'left_pixel', fo.CLIPPED_DEFECT, 'mask_after', 'no_coef', 'base_overwritten')


def test_conv_t_is_the_oracles_backward_data():
    rs = np.random.RandomState(0)
    for K, C, h, w in ((3, 5, 1, 1), (4, 2, 5, 7), (8, 16, 9, 33)):
        wt = rs.randint(-4, 5, (K, C, 3, 3)).astype(np.float32)          # small integers: the float32 oracle is exact
        d = rs.randint(-8, 9, (K, h, w)).astype(np.float32)
        assert np.array_equal(fo.conv_t(wt, d), conv3x3_backward_data(d, wt).astype(np.float64))


def test_the_bf16_rounding_term_is_two_to_the_minus_eight():
    """One round-to-nearest to bf16 errs by up to 2^-8 of the value (just above a power of two), not 2^-9."""
    x = np.float32(1.0 + 2.0 ** -8)                                      # a tie: rounds to even, 1.0
    assert abs(float(fo.bf16_nearest(np.array([x]))[0]) - float(x)) / float(x) > 2.0 ** -9
    v = np.linspace(1, 2, 100001).astype(np.float32)
    assert np.max(np.abs(fo.bf16_nearest(v).astype(np.float64) - v) / v) <= fo.U16


@pytest.mark.parametrize('C,K,shape', CASES, ids=['C%d-K%d-%dx%d' % (c, k, s[0], s[1]) for c, k, s in CASES])
def test_emulation_inside_the_bars_and_every_seeded_defect_outside(C, K, shape):
    h, w = shape
    for with_base in (False, True):
        op, _ = fo.make_operands(C, K, h, w, with_base=with_base)
        R = fo.Reference(**op)
        masked, s_over_c, c_over_s = R.branches()
        assert 0.25 <= masked <= 0.75 and s_over_c >= 0.05 and c_over_s >= 0.05, (masked, s_over_c, c_over_s)
        conv = fo.emulate_conv(op['w16'], op['d16'])
        args = (op['D'], op['F16'], op['coef'], op['c2'])
        for bf16_only in (False, True):
            presence = not bf16_only or fo.fused_shape(C, h, w)
            emu = fo.emulate(**op, bf16_only=bf16_only, conv_sum=conv)
            v = fo.verdict(emu, R, emu, *args, bf16_only=bf16_only, with_presence=presence)
            print('C %d K %d %dx%d base %d bf16-only %d: emulation worst ratio %.3f at %s, rel-L2 %.3g' %
                  (C, K, h, w, with_base, bf16_only, v['element'], v['where'], v['figures']['rel_l2']))
            assert v['element'] <= 1.0 and v['aggregate'], v
            if not presence:
                continue
            for defect in fo.DEFECTS + (fo.CLIPPED_DEFECT,):
                if (defect == 'base_overwritten' and not with_base) or (defect == fo.CLIPPED_DEFECT and fo.clipped_column(w) is None):
                    continue
                out = fo.emulate(**op, bf16_only=bf16_only, defect=defect, conv_sum=conv)
                v = fo.verdict(out, R, emu, *args, bf16_only=bf16_only)
                assert v['element'] > 1.0 or not v['aggregate'], (defect, v)
                p = v['figures']['presence']
                if defect == 'lo_dropped':
                    assert p['lo'] < -fo.PRESENCE_BAR, (defect, p['lo'])
                elif defect == 'chunk_dropped':
                    assert p['chunk%d' % (C // 16 - 1)] < -fo.PRESENCE_BAR and v['element'] > 1.0, (defect, v['element'], p)
                elif defect in ELEMENT_DEFECTS:
                    assert v['element'] > 1.0, (defect, v['element'])


def test_the_last_chunk_is_the_last_of_a_ragged_group_of_three():
    assert fo.chunk_groups(64) == [[0, 1, 2], [3]] and fo.chunk_groups(96) == [[0, 1, 2], [3, 4, 5]]
    assert fo.chunk_groups(128)[-1] == [6, 7] and fo.chunk_groups(256)[-1] == [15] and fo.chunk_groups(512)[-1] == [30, 31]


@pytest.mark.parametrize('bf16_only', [False, True], ids=['fp32', 'bf16-only'])
def test_a_dropped_lo_half_under_a_heavy_conv_sum_is_seen_by_its_presence_coefficient(bf16_only):
    """Once 9 K u A_c dominates the bound, every UNMASKED element of a launch without the lo half passes (a masked one has no conv part
    in its bound and still shows it); the presence coefficient does not depend on the mask."""
    C, K, h, w = 64, 128, 8, 32
    op, _ = fo.make_operands(C, K, h, w, conv_weight=256.0)
    R = fo.Reference(**op)
    conv = fo.emulate_conv(op['w16'], op['d16'])
    args = (op['D'], op['F16'], op['coef'], op['c2'])
    emu = fo.emulate(**op, bf16_only=bf16_only, conv_sum=conv)
    good = fo.verdict(emu, R, emu, *args, bf16_only=bf16_only)
    assert good['element'] <= 1.0 and good['aggregate'], good
    out = fo.emulate(**op, bf16_only=bf16_only, defect='lo_dropped', conv_sum=conv)
    bad = fo.verdict(out, R, emu, *args, bf16_only=bf16_only)
    unmasked = fo.worst_ratio(out[R.m], R.ref[R.m], R.bound(bf16_only)[R.m])
    print('lo dropped: worst ratio %.3f (unmasked elements %.3f), presence of lo %.3f' % (bad['element'], unmasked, bad['figures']['presence']['lo']))
    assert unmasked <= 1.0 and bad['figures']['presence']['lo'] < -fo.PRESENCE_BAR and not bad['aggregate'], bad


def test_trace_formula_is_the_squared_norm_of_the_style_gradient():
    """c2^2 n <D (D + A), D> == || c2 D F ||^2 when D + A is the Gram of F."""
    rs = np.random.RandomState(1)
    C, hw = 32, 64
    F = fo.bf16_nearest(np.maximum(rs.randn(C, hw) * 40, 0).astype(np.float32)).astype(np.float64)
    n = C * hw
    G = F @ F.T / n
    A = rs.randn(C, C); A = A + A.T
    D, c2 = G - A, 2.0 / (C * C * n)
    value, bound = fo.trace_reference(D, A, c2, n)
    assert np.isclose(value, np.sum((c2 * (D @ F)) ** 2), rtol=1e-12) and bound > 0
    assert fo.trace_distance(D, A, c2, n, F.reshape(C, 8, 8)) < 1e-12
