"""tests/anchor_oracle.py against itself, on the CPU: the float64 restatement of the anchor term has the gradient of its own loss (central
differences), the float32 emulation of the documented operation order stays inside every derived bar at the sizes, weights and maps the
GPU tests use, and every seeded defect exceeds a bar by three orders of magnitude or more.  No GPU."""
import numpy as np
import pytest

import anchor_oracle as ao

MAPS = ('none', 'mixed')
size_id = lambda s: '%dx%d' % s                                           # noqa: E731


def case(size, kind):
    h, w = size
    x, ax = ao.images(h, w, 1000 * h + w)
    return x, ax, (ao.mixed_map(h, w, 5) if kind == 'mixed' else None)


def test_the_map_has_zeros_and_large_values():
    m = ao.mixed_map(64, 64, 5)
    assert 0.15 < np.mean(m == 0) < 0.25 and 0.05 < np.mean(m > 1) < 0.15 and m.min() == 0 and m.max() > 5 and m.dtype == np.float32


@pytest.mark.parametrize('kind', MAPS)
@pytest.mark.parametrize('weight', ao.WEIGHTS)
@pytest.mark.parametrize('size', ao.SIZES, ids=size_id)
def test_float32_emulation_is_inside_every_bar(size, weight, kind):
    x, ax, m = case(size, kind)
    ref = ao.evaluate(x, ax, m, weight)
    r = ao.ratios(ao.emulate32(x, ax, m, weight), ref)
    print('[%s w %g map %s] of the bars: g %.3f, loss %.3f, a_grad %.3f' % (size_id(size), weight, kind, r['g'], r['loss'], r['a_grad']))
    assert r['g'] <= 1 and r['loss'] <= 1 and r['a_grad'] <= 1, r
    if m is not None:                                                     # where the map is 0 the gradient is 0, exactly, and so is its bar
        assert not ref['g_bar'][:, m == 0].any() and not ao.emulate32(x, ax, m, weight)['g'][:, m == 0].any()


@pytest.mark.parametrize('defect', ao.DEFECTS)
@pytest.mark.parametrize('weight', ao.WEIGHTS)
@pytest.mark.parametrize('size', ao.SIZES, ids=size_id)
def test_every_seeded_defect_exceeds_a_bar_a_thousandfold(size, weight, defect):
    x, ax, m = case(size, 'mixed')
    ref = ao.evaluate(x, ax, m, weight)
    r = ao.ratios(ao.emulate32(x, ax, m, weight, defect), ref)
    assert max(r.values()) >= 1e3, (defect, r)


def test_the_factor_2_defect_shows_without_a_map_too():
    x, ax, _ = case((17, 33), 'none')
    ref = ao.evaluate(x, ax, None, 0.7)
    assert ao.ratios(ao.emulate32(x, ax, None, 0.7, 'no2'), ref)['g'] >= 1e3


@pytest.mark.parametrize('kind', MAPS)
def test_gradient_is_the_central_difference_of_the_loss(kind):
    x, ax, m = case((17, 33), kind)
    u, ua = x.astype(np.float64) / 255, ax.astype(np.float64) / 255
    w = -1.3
    _, g = ao.loss_and_grad_u(u, ua, m, w)
    rng = np.random.RandomState(0)
    h = 1e-5
    for _ in range(40):
        at = (rng.randint(3), rng.randint(17), rng.randint(33))
        up, dn = u.copy(), u.copy()
        up[at] += h; dn[at] -= h
        fd = (ao.loss_and_grad_u(up, ua, m, w)[0] - ao.loss_and_grad_u(dn, ua, m, w)[0]) / (2 * h)
        # the loss is quadratic in u: the central difference is exact but for the float64 rounding of two sums of size |loss|
        assert abs(fd - g[at]) <= 1e-6 * max(1.0, abs(g[at])), (at, fd, g[at])
    ref = ao.evaluate(x, ax, m, w)                                        # evaluate() is the same function of x / 255
    assert np.array_equal(ref['g'], g) and ref['a_grad'] == np.sqrt(np.sum(g * g) / g.size)


def test_evaluate_refuses_what_the_engine_refuses():
    x, ax, m = case((16, 16), 'mixed')
    for w in (0.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            ao.evaluate(x, ax, m, w)
    for bad in (-1.0, float('nan'), float('inf')):
        mm = m.copy(); mm[3, 4] = bad
        with pytest.raises(ValueError):
            ao.evaluate(x, ax, mm, 1.0)
