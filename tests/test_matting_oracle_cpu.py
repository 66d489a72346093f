"""tests/matting_oracle.py held to itself on the CPU: the matrix-free float64 form against the dense matting Laplacian, the properties
of L, and the fp32 restatement of st2.h's operation order against float64.

The fp32 figures are measured, not derived: per case (kind of image, eps, size) the worst |g32 - g64| / rms(g64) over the gradient
and the relative error of the loss.  ``python tests/test_matting_oracle_cpu.py`` writes them to profiles/matting_errors.txt, the
committed file is the record, and the test asserts today's figures at 4 x the recorded ones.  Ramps at eps <= 1e-7 are the
ill-conditioned end: content and iterate are both nearly affine, the true gradient is ~1e-7 and the fp32 rounding of I itself
dominates it, so the figure relative to rms(g64) is large there (about 90 at eps = 1e-9); it is recorded as it is.

Seeded defects.  Every defect must change bits of the restatement AND exceed the 4 x bar of at least one input.  Five of them change
the mathematics or lose bits wholesale and show on the plain cases (eps_not_over_9, clipped_windows, no_eps_a2 through the loss,
mu_double) or on two earlier planes that cancel (prev_second, the input `cancelling_prev`).  Two are other roundings of the same
mathematics, as accurate as the definition on any generic input (measured on the plain cases: column_major at most 1.78 x a recorded
figure, two_after_w the same bits), so each has an input built for it, on which the definition's order is exact where the other is not:
    exact_row_major    one 3 x 3 window.  The content's colours are small integers with the window mean at pixels 0, 1 and 8, so dI = 0
                       there; the iterate is [A, -A, a, -a, b, -b, c, -c, 0] row-major with A = 2^22.  Visited row-major every pair
                       cancels exactly: pb = 0, and the big pixels meet only dI = 0, so the restatement errs at the scale of a, b, c
                       alone.  Visited column-major, A swallows -a and c before -A arrives, and pb is wrong by about (a - c) / 9.
    half_unit_weight   2 * x is exact, so w * (2 Lu) and 2 * (w Lu) differ only where w Lu is subnormal.  w = 2^-149, the smallest
                       float, and residuals of exactly 0.5, 0.5 and -1 (the same content; the fit is a = 0, pb = 0 exactly): w * (2 * 0.5)
                       is one unit, exactly, while w * 0.5 is a tie that rounds to 0.  The restatement's error is 0 there, and so is the
                       recorded figure: the bar there is the float64 reference's own floor (REF_FLOOR).
    tiny_weight        (w = 3e-44 on noise: both orders are off by about 1e-2 of the rms there; kept as a record of that)."""
import os

import numpy as np
import pytest

import matting_oracle as mo

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(os.path.dirname(HERE), 'profiles', 'matting_errors.txt')
KINDS, EPS, SIZES = ('noise', 'ramp', 'flat'), (1e-9, 1e-7, 1e-2), ((7, 9), (9, 11))
MARGIN = 4.0
REF_FLOOR = 2.0 ** -46      # 64 ulps of float64: what loss_grad64 itself (LAPACK's inverse, BLAS's dot products) may differ by between machines;
                           # it only matters where a recorded figure is 0 or nearly so


def bar_of(recorded):
    return MARGIN * recorded + REF_FLOOR


def unit(planes):
    return (planes / F32(255)).astype(F64)


def case_inputs(kind, h, w):
    return mo.planes(kind, h, w, 1), mo.planes(kind, h, w, 2)


def figures(x, cx, weight, eps, prev=(), defect=None):
    """(worst |extra32 - extra64| / rms(extra64), relative error of sum J) of the restatement, the defect seeded where one is named."""
    loss64, g64 = mo.loss_grad64(unit(x), unit(cx), eps)
    want = F64(F32(weight)) * g64
    for p in prev:
        want = want + np.asarray(p, F64)
    got = mo.evaluate(x, cx, weight, eps, prev=prev, defect=defect)
    rms = np.sqrt((want ** 2).mean())
    return float(np.abs(got['extra'].astype(F64) - want).max() / rms), float(abs(got['sum_j'] - loss64) / loss64)


def special_inputs():
    """Inputs beyond the grid of cases, for the defects no plain input can show: weights so small that w Lu is subnormal, two earlier
    planes that cancel (g_lap = -g_anc to within 1e-3 at a magnitude of 1e5), and a window on which row-major sums are exact (the
    module's docstring has the construction)."""
    x, cx = case_inputs('noise', 7, 9)
    big = (mo.planes('noise', 7, 9, 5) * F32(1e3)).astype(F32)
    small = (mo.planes('noise', 7, 9, 6) * F32(1e-3)).astype(F32)
    # one 3 x 3 window whose content has dI = 0 at pixels 0, 1 and 8 (integers, the mean among them)
    pairs = np.array([[-3, -2, -1], [1, 3, -2], [1, 1, 1]], F64)          # dI of pixels 2 .. 7 is (a, -a, b, -b, c, -c) per channel
    content = np.zeros((3, 9), F64)
    for ch in range(3):
        content[ch, 2:8] = np.repeat(pairs[ch], 2) * np.tile([1, -1], 3)
    content = ((content + np.array([[5.0], [7.0], [9.0]])) * 255).astype(F32).reshape(3, 3, 3)
    rng = np.random.RandomState(11)
    cancel = np.zeros((3, 9), F64)
    for ch in range(3):
        a, b, c = rng.rand(3) * 90 + 10
        cancel[ch] = [255.0 * 2 ** 22, -255.0 * 2 ** 22, a, -a, b, -b, c, -c, 0]
    halves = np.tile(np.array([127.5, 127.5, 0, 0, 0, 0, 0, 0, -255.0]), (3, 1))
    return {'tiny_weight': (x, cx, 3e-44, 1e-7, ()), 'cancelling_prev': (x, cx, 1.0, 1e-7, (big, -big + small)),
            'exact_row_major': (cancel.astype(F32).reshape(3, 3, 3), content, 1.0, 1e-7, ()),
            'half_unit_weight': (halves.astype(F32).reshape(3, 3, 3), content, 2.0 ** -149, 1e-7, ())}


def all_cases():
    cases = {}
    for kind in KINDS:
        for eps in EPS:
            for h, w in SIZES:
                cases['%s eps=%g %dx%d' % (kind, eps, h, w)] = case_inputs(kind, h, w) + (1.0, eps, ())
    cases.update(special_inputs())
    return cases


def measure():
    return {name: figures(*args) for name, args in all_cases().items()}


def read_record():
    out = {}
    for line in open(RECORD):
        if line.startswith('#') or not line.strip():
            continue
        name, g, loss = line.rstrip('\n').split(' | ')
        out[name.strip()] = (float(g), float(loss))
    return out


# ---- float64: matrix-free against dense ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eps', (1e-7, 1e-4))
@pytest.mark.parametrize('kind', KINDS)
def test_matrix_free_agrees_with_the_dense_laplacian(kind, eps):
    h, w = 7, 9
    x, cx = case_inputs(kind, h, w)
    u, I = unit(x), unit(cx)
    L = mo.dense_laplacian(I, eps)
    loss, g = mo.loss_grad64(u, I, eps)
    dense_loss = sum(u[c].ravel() @ L @ u[c].ravel() for c in range(3))
    dense_g = np.stack([2 * (L @ u[c].ravel()).reshape(h, w) for c in range(3)])
    assert np.abs(L - L.T).max() <= 1e-9 * np.abs(L).max()                # symmetric
    assert np.abs(L @ np.ones(h * w)).max() <= 1e-9 * np.abs(L).max()     # constants are in the null space
    assert np.abs(dense_g - g).max() <= 1e-9 * max(np.abs(g).max(), 1e-12 * np.abs(L).max())
    assert abs(dense_loss - loss) <= 1e-7 * abs(loss)
    assert loss >= 0


def test_an_affine_function_of_the_content_costs_at_most_eps_alpha_squared_per_window():
    h, w, eps = 9, 11, 1e-4
    I = unit(mo.planes('noise', h, w, 2))
    alpha, beta = np.array([0.3, -1.2, 0.7]), 0.25
    p = np.tensordot(alpha, I, 1) + beta
    loss, g = mo.loss_grad64(np.stack([p, p, p]), I, eps)
    bound = 3 * eps * (alpha @ alpha) * (h - 2) * (w - 2)
    assert 0 <= loss <= bound * (1 + 1e-9), (loss, bound)
    noise, _ = mo.loss_grad64(unit(mo.planes('noise', h, w, 1)), I, eps)
    assert noise > 1e3 * loss                                             # (and anything else costs far more)


def test_central_differences_of_the_float64_loss_match_the_gradient():
    h, w, eps = 6, 7, 1e-4
    u, I = unit(mo.planes('noise', h, w, 1)), unit(mo.planes('noise', h, w, 2))
    _, g = mo.loss_grad64(u, I, eps)
    rng, step = np.random.RandomState(0), 1e-5
    for _ in range(12):
        c, y, x = rng.randint(3), rng.randint(h), rng.randint(w)
        up, dn = u.copy(), u.copy()
        up[c, y, x] += step
        dn[c, y, x] -= step
        fd = (mo.loss_grad64(up, I, eps)[0] - mo.loss_grad64(dn, I, eps)[0]) / (2 * step)
        assert abs(fd - g[c, y, x]) <= 1e-6 * max(abs(g[c, y, x]), 1.0), (c, y, x, fd, g[c, y, x])


def test_the_device_sum_is_the_plain_sum_to_fp32_partials():
    cells = np.random.RandomState(3).rand(3, 9, 131)                      # three tiles across, three down
    assert abs(mo.device_sum(cells) - cells.sum()) <= 4 * 2.0 ** -24 * cells.sum()
    one = np.zeros((3, 1, 1))
    one[1, 0, 0] = 0.3
    assert mo.device_sum(one) == F64(F32(0.3))


# ---- fp32 against float64 ------------------------------------------------------------------------------------------------------------
def test_the_fp32_restatement_stays_within_four_times_its_recorded_error():
    record, now = read_record(), measure()
    assert sorted(record) == sorted(now)
    for name, (g, loss) in now.items():
        print('%-28s g %.3e (recorded %.3e)  loss %.3e (recorded %.3e)' % (name, g, record[name][0], loss, record[name][1]))
        assert g <= bar_of(record[name][0]) and loss <= bar_of(record[name][1]), name


@pytest.mark.parametrize('defect', mo.DEFECTS)
def test_every_seeded_defect_changes_bits_and_exceeds_the_bar(defect):
    record = read_record()
    changed, exceeded, worst, where = False, False, 0.0, None
    for name, (x, cx, weight, eps, prev) in all_cases().items():
        if defect == 'clipped_windows' and name.split()[-1] != '7x9':
            continue                                                      # (the loop form: the small size of every kind and eps)
        right, wrong = mo.evaluate(x, cx, weight, eps, prev=prev), mo.evaluate(x, cx, weight, eps, prev=prev, defect=defect)
        changed |= right['extra'].tobytes() != wrong['extra'].tobytes() or F64(right['sum_j']).tobytes() != F64(wrong['sum_j']).tobytes()
        g, loss = figures(x, cx, weight, eps, prev, defect)
        for got, bar in ((g, record[name][0]), (loss, record[name][1])):
            exceeded |= got > bar_of(bar)
            ratio = got / bar if bar > 0 else (np.inf if got > 0 else 0.0)      # (a recorded 0: the restatement is exact on that input)
            if ratio > worst:
                worst, where = ratio, name
    print('%s: bits %s; worst %.3g x a recorded figure (%s); the bar is %g x' % (defect, 'change' if changed else 'THE SAME', worst, where, MARGIN))
    assert changed, '%s leaves every bit of the restatement as it was' % defect
    assert exceeded and worst > MARGIN, '%s stays within the bar: worst %.3g x a recorded figure, at %s' % (defect, worst, where)


def write_record():
    rows = measure()
    with open(RECORD, 'w') as f:
        f.write('# The fp32 restatement of the photorealism term (tests/matting_oracle.py: evaluate) against float64 (loss_grad64); weight 1 but for\n'
                '# tiny_weight (3e-44) and half_unit_weight (2^-149).\n'
                '# Written by `python tests/test_matting_oracle_cpu.py`; tests/test_matting_oracle_cpu.py asserts 4 x these figures.\n'
                '# case | worst |extra32 - extra64| / rms(extra64) | |sum J 32 - loss64| / loss64\n')
        for name, (g, loss) in rows.items():
            f.write('%-28s | %.3e | %.3e\n' % (name, g, loss))
    return rows


if __name__ == '__main__':
    for name, (g, loss) in write_record().items():
        print('%-28s %.3e %.3e' % (name, g, loss))
