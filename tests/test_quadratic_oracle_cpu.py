"""The quadratic job of tests/quadratic_oracle.py on the CPU: the fp32 oracles against their float64 restatements, the events the
schedule is meant to produce (ten pairs from step 9 on, rejections exactly where the step is 1e-9, no gate decision near 1e-10), and
the mutants of the float64 L-BFGS against the bar the GPU tests put on the device (tests/test_gpu_quadratic_descent.py)."""
import numpy as np
import pytest

import quadratic_oracle as q

SCHED = q.SCHEDULE['lbfgs']


@pytest.mark.parametrize('h,w', q.SIZES)
def test_fp32_lbfgs_oracle_follows_float64_and_the_schedule_produces_its_events(h, w):
    ref, log64 = q.reference('lbfgs', h, w)
    f32, log32 = q.lbfgs_fp32(h, w)
    dx = [q.max_abs(a[0], b[0]) for a, b in zip(f32, ref)]
    dl = [abs(a[1] / b[1] - 1) for a, b in zip(f32, ref)]
    print('[lbfgs %dx%d] fp32 oracle: worst max|x32 - x64| %.3g (step %d), worst relative loss deviation %.3g (step %d)'
          % (h, w, max(dx), int(np.argmax(dx)), max(dl), int(np.argmax(dl))))
    assert max(dx) <= 5e-3, max(dx)
    # LOSS_RTOL is ten times the worst of these over the sizes: every size has at least that factor (5 here: another BLAS may round
    # the oracle's dot products differently)
    assert max(dl) <= q.LOSS_RTOL / 5, max(dl)
    q.assert_events(log64, SCHED, q.SY_REJECTED_MAX, 'float64 %dx%d' % (h, w))
    q.assert_events(log32, SCHED, q.SY_REJECTED_MAX, 'fp32 %dx%d' % (h, w))
    # a rejected step leaves an fp32 iterate alone except where a pixel is nearly zero; where the float64 run says none can move, none does
    for k in SCHED['tiny_at']:
        smax, may_move = q.tiny_step_effect(ref, k)
        moved = q.max_abs(f32[k][0], f32[k - 1][0])
        print('[lbfgs %dx%d] step %d: max|s| %.3g, fp32 iterate moved by %.3g%s' % (h, w, k, smax, moved, '' if may_move else ' (must not move)'))
        assert moved <= 4 * smax
        if not may_move:
            assert np.array_equal(f32[k][0], f32[k - 1][0])
    if (h, w) == q.SIZES[0]:
        assert [q.tiny_step_effect(ref, k)[1] for k in SCHED['tiny_at']] == [False, False, True]


@pytest.mark.parametrize('h,w', q.SIZES)
@pytest.mark.parametrize('name', list(q.MUTANTS))
def test_every_mutant_of_the_float64_lbfgs_leaves_the_trajectory_by_far_more_than_the_bar(name, h, w):
    ref, _ = q.reference('lbfgs', h, w)
    mut, _ = q.lbfgs_reference(h, w, **q.MUTANTS[name])
    worst = max(q.max_abs(a[0], b[0]) for a, b in zip(mut, ref))
    print('[mutant %dx%d] %s: worst max|x_mut - x64| %.3g' % (h, w, name, worst))
    assert worst >= 0.1 >= 5 * q.X_ATOL, worst


def test_the_run_at_the_second_grid_sweep_size_has_its_events_too():
    """592 x 600, 14 steps: ten pairs by step 9, the first eviction at step 10, one rejection at step 12.  Its rejected s.y is 2.3e-13
    in float64 (s.y grows with the pixel count), which no choice of step inside 14 brings below the 1e-14 of the small sizes: the bar is
    SY_REJECTED_MAX_BIG = 1e-12 here, two orders from the gate, and the rejection stays at step 12."""
    h, w = q.BIG_SIZE
    sched = q.SCHEDULE['lbfgs_big']
    ref, log64 = q.reference('lbfgs_big', h, w)
    f32, log32 = q.lbfgs_fp32(h, w, sched)
    dx = max(q.max_abs(a[0], b[0]) for a, b in zip(f32, ref))
    dl = max(abs(a[1] / b[1] - 1) for a, b in zip(f32, ref))
    print('[lbfgs %dx%d] fp32 oracle: worst max|x32 - x64| %.3g, worst relative loss deviation %.3g' % (h, w, dx, dl))
    assert dx <= 5e-3 and dl <= q.LOSS_RTOL / 5, (dx, dl)
    q.assert_events(log64, sched, q.SY_REJECTED_MAX_BIG, 'float64 %dx%d' % (h, w))
    q.assert_events(log32, sched, q.SY_REJECTED_MAX_BIG, 'fp32 %dx%d' % (h, w))


def test_the_cleared_run_restarts_its_history_and_keeps_its_margins():
    """A replacement input and objective_changed after step 20: the pair count restarts at 1, the rejection at step 25 remains.  It
    now comes four steps after a fresh start, where s.y is still large (3.2e-13 in float64): held to the 1e-12 of the large size."""
    h, w = q.SIZES[1]
    ref, log = q.reference('lbfgs_cleared', h, w)
    at = q.CLEARED['at']
    assert len(ref) == at + q.CLEARED['more']
    assert [n for _, _, n in log[at:at + 4]] == [1, 2, 3, 4] and log[-1][2] == 10
    assert q.rejected_steps(log) == SCHED['tiny_at']
    assert min(sy for sy, k, _ in log if k) > q.SY_KEPT_MIN and max(sy for sy, k, _ in log if not k) < q.SY_REJECTED_MAX_BIG
    plain, _ = q.reference('lbfgs', h, w)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(ref[:at], plain[:at]))
    assert q.max_abs(ref[at][0], plain[at][0]) > 10.0          # (the new input took effect)


@pytest.mark.parametrize('h,w', q.SIZES)
def test_fp32_adam_oracle_follows_float64_through_a_new_input_and_a_new_step_size(h, w):
    (ref, states64), (f32, states32) = q.reference('adam', h, w), q.adam_fp32(h, w)
    dx = max(q.max_abs(a[0], b[0]) for a, b in zip(f32, ref))
    dl = max(abs(a[1] / b[1] - 1) for a, b in zip(f32, ref))
    print('[adam %dx%d] fp32 oracle: worst max|x32 - x64| %.3g, worst relative loss deviation %.3g' % (h, w, dx, dl))
    assert dx <= 1e-2 and 10 * dl <= q.LOSS_RTOL, (dx, dl)
    want_items = {11: (12, 12), 12: (1, 13), 19: (8, 20), 29: (18, 30)}      # items1 restarts at objective_changed, items2 does not
    for k in q.ADAM_STATE_STEPS:
        m32, v32, i1, i2 = states32[k]
        m64, v64, j1, j2 = states64[k]
        assert (i1, i2) == (j1, j2) == want_items[k]
        dm, dv = q.max_rel(m32, m64), q.max_rel(v32, v64)
        print('[adam %dx%d] after step %d: m within %.3g, v within %.3g (relative to their max)' % (h, w, k, dm, dv))
        assert 10 * dm <= q.ADAM_M_RTOL and 10 * dv <= q.ADAM_V_RTOL, (dm, dv)
    # the replacement input and the new step size are visible in the trajectory
    assert q.max_abs(ref[12][0], ref[11][0]) > 50.0
    step = [q.max_abs(ref[k][0], ref[k - 1][0]) for k in (19, 20)]
    assert step[1] < 0.5 * step[0], step


def test_objective_is_the_image_terms_of_the_transfer_oracle():
    """objective() against TransferOracle.opfunc with an empty weight table (fp32), and its gradient against a central difference of
    its own float64 loss along a random direction (the objective is a quadratic: exact up to rounding).  The reference applies no
    1/255 chain factor (worker.py:296-297), so what the optimisers are handed is 255 times the derivative."""
    import oracle
    h, w = 9, 11
    topo = oracle.tiny_topology((8,), (1,))
    ora = oracle.TransferOracle(oracle.NetOracle(topo, oracle.he_init_weights(topo, seed=0, bias_std=0.1)))
    ora.rows, ora.cells = [], {k: {} for k in ('content', 'style', 'deepdream')}
    ora.params = {k: q.JOB[k] for k in ('tv', 'tv_power', 'p', 'p_power')}
    x = q.x0(h, w)
    want_loss, want_grad = ora.opfunc(x.copy())
    loss, grad = q.objective(x, dtype=q.F32)
    assert np.isclose(loss, want_loss, rtol=1e-6) and np.allclose(grad, want_grad, rtol=1e-6, atol=1e-9)
    d = np.random.RandomState(1).randn(*x.shape)
    x64 = x.astype(q.F64)
    l1, l0 = q.objective(x64 + d)[0], q.objective(x64 - d)[0]
    assert np.isclose(255 * (l1 - l0) / 2, np.vdot(q.objective(x64)[1], d), rtol=1e-10)
