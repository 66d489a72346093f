"""tests/laplacian_oracle.py checked against itself: its gradient is the derivative of its loss, a float32 emulation of the documented
operation order meets every derived bar, and each seeded defect breaks one at the sizes the GPU test runs."""
import numpy as np
import pytest

import laplacian_oracle as lo

SIZES = ((16, 16), (17, 33), (37, 50), (20, 260), (64, 64))
LEVEL_SETS = (((1, 0.7),), ((4, 1.5),), ((16, 2.0),), ((32, 3.0),), ((2, 0.8), (4, -1.3), (16, 2.5)))
THREE = LEVEL_SETS[-1]


def test_gradient_is_the_central_difference_of_the_loss():
    rng = np.random.RandomState(0)
    u, uc = rng.rand(3, 9, 11), rng.rand(3, 9, 11)
    levels = ((1, 0.6), (4, -1.7))
    _, g = lo.loss_and_grad_u(u, uc, levels)
    h = 1e-4                                                  # the loss is quadratic in u: the central difference is exact up to rounding
    fd = np.zeros_like(u)
    for idx in np.ndindex(*u.shape):
        up, dn = u.copy(), u.copy()
        up[idx] += h; dn[idx] -= h
        fd[idx] = (lo.loss_and_grad_u(up, uc, levels)[0] - lo.loss_and_grad_u(dn, uc, levels)[0]) / (2 * h)
    assert np.max(np.abs(fd - g)) <= 1e-6 * np.max(np.abs(g))


def test_evaluate_is_the_loss_and_gradient_of_u():
    x, cx = lo.images(9, 11, 1)
    levels = ((1, 0.6), (4, -1.7))
    ref = lo.evaluate(x, cx, levels)
    loss, g = lo.loss_and_grad_u(x.astype(np.float64) / 255, cx.astype(np.float64) / 255, levels)
    assert np.isclose(ref['loss'], loss, rtol=1e-13) and np.allclose(ref['g'], g, rtol=1e-13, atol=0)


def test_stencil_properties():
    rng = np.random.RandomState(2)
    assert not lo.stencil(np.full((3, 5, 7), 2.5)).any()                         # a constant gives 0
    assert not lo.stencil(rng.rand(3, 1, 1)).any()                               # a 1 x 1 grid gives 0
    a, b = rng.rand(1, 4, 6), rng.rand(1, 4, 6)
    assert np.isclose(np.sum(a * lo.stencil(b)), np.sum(lo.stencil(a) * b))      # D is symmetric
    q = np.zeros((1, 4, 6)); q[0, 0, 0] = 1
    assert lo.stencil(q)[0, 0, 0] == 2 and lo.stencil(q)[0, 0, -1] == 0          # a corner has two neighbours, nothing wraps
    assert np.array_equal(lo.pool(rng.rand(3, 5, 7), 1).shape, (3, 5, 7))
    assert np.array_equal(lo.counts(5, 7, 4), [[16, 12], [4, 3]])


@pytest.mark.parametrize('levels', LEVEL_SETS, ids=lambda lv: '+'.join(str(p) for p, _ in lv))
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_float32_emulation_meets_every_bar(size, levels):
    x, cx = lo.images(size[0], size[1], 3)
    ref = lo.evaluate(x, cx, levels)
    assert lo.misses(lo.emulate32(x, cx, levels), ref) == []


@pytest.mark.parametrize('defect', lo.DEFECTS)
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_seeded_defects_break_a_bar(size, defect):
    H, W = size
    x, cx = lo.images(H, W, 4)
    ref = lo.evaluate(x, cx, THREE)
    bad = lo.misses(lo.emulate32(x, cx, THREE, defect), ref)
    if defect == 'divisor' and all(H % p == 0 and W % p == 0 for p, _ in THREE):
        assert bad == []                                      # no clipped cell at this size: the defect cannot show
    else:
        assert bad, (size, defect)


def test_validation():
    for levels in (((3, 1.0),), ((4, 1.0), (4, 2.0)), ((4, 0.0),), ((4, float('nan')),), ((4, float('inf')),),
                   ((1, 1.0), (2, 1.0), (4, 1.0), (8, 1.0))):
        with pytest.raises(ValueError):
            lo.validate(levels)
    assert lo.validate(()) == []
