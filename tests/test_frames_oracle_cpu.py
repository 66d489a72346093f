"""tests/frames_oracle.py (the reliability and the long-term composition of include/st2.h in NumPy) held to cases worked out by hand: a
translation with its exact inverse, an occluder over a static background, a one-pixel step in the flow, inputs two float32 steps on
either side of each threshold, the "outside" rule on all four sides, and the disjointness of the composed maps.  No GPU."""
import numpy as np
import pytest

import frames_oracle as fo

F32, F64 = np.float32, np.float64


def const_flow(h, w, dx, dy):
    f = np.empty((h, w, 2), F32)
    f[..., 0], f[..., 1] = dx, dy
    return f


def test_a_translation_with_its_exact_inverse_is_reliable_except_where_the_sample_leaves_the_image():
    h, w = 9, 12
    bwd, fwd = const_flow(h, w, 2.5, -1.25), const_flow(h, w, -2.5, 1.25)
    outside, disoccluded, boundary = fo.parts(bwd, fwd)
    assert not disoccluded.any() and not boundary.any()
    want = np.zeros((h, w), bool)
    want[:2, :] = True                                     # y - 1.25 < 0 for y = 0, 1
    want[:, w - 3:] = True                                 # x + 2.5 > w - 1 for the last three columns
    assert np.array_equal(outside, want)
    c = fo.reliability(bwd, fwd)
    assert c.dtype == F32 and np.array_equal(c, (~want).astype(F32))
    assert np.array_equal(fo.reliability(bwd, None), np.ones((h, w), F32))


def test_an_occluder_over_a_static_background_leaves_a_zero_band_as_wide_as_its_motion():
    h, w, a, b, d = 6, 40, 10, 22, 4                        # the object covers columns [a, b) of the earlier frame and moves d to the right
    fwd, bwd = np.zeros((h, w, 2), F32), np.zeros((h, w, 2), F32)
    fwd[:, a:b, 0] = d                                     # on the earlier frame: the object moves, the background rests
    bwd[:, a + d:b + d, 0] = -d                            # on the later frame: the object points back to where it was
    outside, disoccluded, boundary = fo.parts(bwd, fwd)
    assert not outside.any()
    cols = np.zeros(w, bool); cols[a:a + d] = True         # the background the object uncovered: it samples the object, whose flow does not return
    assert np.array_equal(disoccluded, np.broadcast_to(cols, (h, w)))
    edge = np.zeros(w, bool); edge[[a + d - 1, b + d - 1]] = True       # the two columns whose right neighbour has another flow
    assert np.array_equal(boundary, np.broadcast_to(edge, (h, w)))
    c = fo.reliability(bwd, fwd)
    assert np.array_equal(c == 0, np.broadcast_to(cols | edge, (h, w))) and int((c[0] == 0).sum()) == d + 1


def test_a_one_pixel_step_in_the_flow_is_one_boundary_column_and_nothing_else():
    h, w, k = 5, 16, 7
    bwd, fwd = np.zeros((h, w, 2), F32), np.zeros((h, w, 2), F32)
    bwd[:, k:, 0] = 1                                      # columns from k on sample one pixel to the right ...
    fwd[:, k + 1:, 0] = -1                                 # ... where the earlier frame's flow leads back
    outside, disoccluded, boundary = fo.parts(bwd, fwd)
    col = np.zeros(w, bool); col[k - 1] = True
    assert np.array_equal(boundary, np.broadcast_to(col, (h, w)))
    assert not disoccluded.any()
    last = np.zeros(w, bool); last[w - 1] = True           # (the last column samples x = w: outside)
    assert np.array_equal(outside, np.broadcast_to(last, (h, w)))
    assert np.array_equal(fo.reliability(bwd, fwd) == 0, np.broadcast_to(col | last, (h, w)))
    # a vertical step: one row
    bwd, fwd = np.zeros((h, w, 2), F32), np.zeros((h, w, 2), F32)
    bwd[2:, :, 1] = -1
    assert np.array_equal(fo.parts(bwd, fwd)[2], np.broadcast_to((np.arange(h) == 1)[:, None], (h, w)))


def two_steps(x):
    x = F32(x)
    lo = np.nextafter(np.nextafter(x, F32(-np.inf)), F32(-np.inf))
    hi = np.nextafter(np.nextafter(x, F32(np.inf)), F32(np.inf))
    return lo, hi


def test_a_hair_on_either_side_of_the_disocclusion_threshold():
    # no backward flow, a forward flow (e, 0): e^2 > 0.01 e^2 + 0.5, i.e. e > sqrt(0.5 / 0.99)
    lo, hi = two_steps(np.sqrt(0.5 / 0.99))
    h, w = 3, 4
    zero = np.zeros((h, w, 2), F32)
    assert np.array_equal(fo.reliability(zero, const_flow(h, w, lo, 0)), np.ones((h, w), F32))
    assert np.array_equal(fo.reliability(zero, const_flow(h, w, hi, 0)), np.zeros((h, w), F32))
    assert np.array_equal(fo.reliability(zero, const_flow(h, w, 0, -lo)), np.ones((h, w), F32))
    assert np.array_equal(fo.reliability(zero, const_flow(h, w, 0, -hi)), np.zeros((h, w), F32))
    assert np.array_equal(fo.reliability(None, const_flow(h, w, hi, 0)), np.zeros((h, w), F32))       # no backward flow at all: (0, 0)
    # with a backward flow of (3, 0) that stays inside and a forward flow (-3 + e, 0): e^2 > 0.01 ((3 - e)^2 + 9) + 0.5
    e = (-0.06 + np.sqrt(0.0036 + 4 * 0.99 * 0.68)) / (2 * 0.99)
    for f, want in zip(two_steps(-3 + e), (1, 0)):
        c = fo.reliability(const_flow(h, 8, 3, 0), const_flow(h, 8, f, 0))
        assert np.array_equal(c[:, :5], np.full((h, 5), want, F32)) and not c[:, 5:].any()         # (the last three columns sample outside)


def test_a_hair_on_either_side_of_the_boundary_threshold():
    # flow 0 left of a step of s: s^2 > 0.002
    h, w, k = 3, 8, 4
    for s, want in zip(two_steps(np.sqrt(0.002)), (False, True)):
        bwd = np.zeros((h, w, 2), F32)
        bwd[:, k:, 0] = s
        got = fo.parts(bwd, np.zeros_like(bwd))[2]
        assert got[:, k - 1].all() == want and got[:, k - 1].any() == want and not np.delete(got, k - 1, axis=1).any()
    # a flow of (10, 0) left of the step: s^2 > 0.01 * 100 + 0.002
    for right, want in zip(two_steps(10 + np.sqrt(1.002)), (False, True)):
        bwd = const_flow(h, w, 10, 0)
        bwd[:, k:, 0] = right
        diff = F64(right) - 10.0                            # (exact in float64)
        assert (diff * diff > 0.01 * 100 + 0.002) == want
        got = fo.parts(bwd, np.zeros_like(bwd))[2]
        assert got[:, k - 1].all() == want and got[:, k - 1].any() == want


@pytest.mark.parametrize('h,w', [(6, 9), (1, 1)], ids=['6x9', '1x1'])
def test_the_outside_rule_on_all_four_sides_and_exactly_on_the_last_row_and_column(h, w):
    yy, xx = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing='ij')
    tiny = F32(1e-3)

    def outside(dx, dy):
        bwd = np.stack([np.broadcast_to(dx, (h, w)), np.broadcast_to(dy, (h, w))], axis=-1).astype(F32)
        return fo.parts(bwd, np.zeros_like(bwd))[0]
    assert not outside(w - 1 - xx, 0).any() and outside(w - 1 - xx + tiny, 0).all()        # exactly on the last column; a hair beyond it
    assert not outside(0, h - 1 - yy).any() and outside(0, h - 1 - yy + tiny).all()
    assert not outside(-xx, 0).any() and outside(-xx - tiny, 0).all()                       # exactly on column 0; a hair before it
    assert not outside(0, -yy).any() and outside(0, -yy - tiny).all()
    c = fo.reliability(const_flow(h, w, 0, 0) + np.stack([w - 1 - xx + tiny, 0 * yy], axis=-1), np.zeros((h, w, 2), F32))
    assert not c.any()


def test_the_composed_maps_of_binary_inputs_are_disjoint_and_add_up_to_their_union():
    rng = np.random.RandomState(0)
    h, w = 11, 13
    cs = [(rng.rand(h, w) < 0.4).astype(F32) for _ in range(3)]
    planes = [rng.randn(3, h, w).astype(F32) for _ in range(3)]
    ax, M = planes[0].copy(), cs[0].copy()                  # the first call sets
    ms = [cs[0]]
    for a_j, c in zip(planes[1:], cs[1:]):
        ax, M, m = fo.compose(ax, M, a_j, c)
        assert ax.dtype == F32 and M.dtype == F32
        ms.append(m)
    for i in range(3):
        assert set(np.unique(ms[i])) <= {0.0, 1.0} and (ms[i] <= cs[i]).all()
        for k in range(i):
            assert not (ms[i] * ms[k]).any()               # c_long: disjoint by construction
    assert np.array_equal(M, np.maximum(np.maximum(cs[0], cs[1]), cs[2])) and np.array_equal(M, ms[0] + ms[1] + ms[2])
    for m, a_j in zip(ms[1:], planes[1:]):                  # each pixel holds the first frame whose map shows it
        assert np.array_equal(ax[:, m > 0], a_j[:, m > 0])
    assert np.array_equal(ax[:, ms[1] + ms[2] == 0], planes[0][:, ms[1] + ms[2] == 0])
    # a mask scales the reliability in float64, rounded once
    mask = rng.rand(h, w).astype(F32)
    assert np.array_equal(fo.reliability(None, None, mask), mask)
    bwd = const_flow(h, w, 20, 0)                           # every sample outside
    assert not fo.reliability(bwd, np.zeros_like(bwd), mask).any()
