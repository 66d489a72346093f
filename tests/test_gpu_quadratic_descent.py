"""Both device optimisers held to float64 trajectories on the quadratic job of tests/quadratic_oracle.py.

With an empty weight table and tv_power = p_power = 2 the engine's objective is an exact quadratic, a fixed-step L-BFGS contracts on it
and rounding is not amplified, so EVERY iterate of the running device state machine (lbfgs.hip: the chain form, the Gram form with its
carried matrix of inner products, the tile-sharded Gram form of engine_comm.cpp) can be compared with a float64 run of the same
algorithm -- through 23 evictions, three gate rejections inside a running history, a cleared history and the second sweep of the
grid-stride loops.  The bar on the iterate, X_ATOL = 0.02 in preprocessed pixel units, lies ten times above the fp32 CPU oracle's own
distance from float64 and ten times below the mildest mutant of the recursion (evicting the wrong pair, nine or eleven pairs, a gate at
zero, H0 from the wrong pair): tests/test_quadratic_oracle_cpu.py asserts both.  Adam (fused into image_pass_k) runs the other half of
the job: a replacement input with objective_changed and a new step size in mid-run, iterate, m, v and the two item counts.

A step of 1e-9 is what the schedule rejects pairs with.  It moves an fp32 iterate only at the few pixels that are nearly zero
(quadratic_oracle.tiny_step_effect); where the float64 run shows that no pixel can move (15x17, steps 13 and 14) the device iterate
must stay bit-identical, everywhere else it may move by no more than a few |s|.  For the same reason the gate itself is guarded by
the 64x96 cases and the tile grid only: at 15x17 y = 0 exactly at steps 13 and 14, so a gate of `sy > 0` rejects those pairs too (seeded
into lbfgs.hip it passes at 15x17 and leaves float64 by 4.5 to 86 at the larger sizes).
"""
import numpy as np
import pytest

import oracle
import quadratic_oracle as q
import style_transfer2_amd as st2
from helpers import rel_l2
from style_transfer2_amd.engine import OPT_ADAM, OPT_LBFGS

pytestmark = pytest.mark.gpu
F32 = np.float32
TOPO = oracle.tiny_topology((8,), (1,))
PARAMS4 = [q.JOB[k] for k in ('tv', 'tv_power', 'p', 'p_power')]
SCHED = q.SCHEDULE['lbfgs']
_runs = {}          # (form, h, w) -> (iterates, losses) of the plain scheduled run, shared by the cases that must reproduce it bit for bit


def _set_form(monkeypatch, form):
    """ST2_LBFGS_FORM for the engines built from here on (read while the history is empty); None: unset, the engine's own choice."""
    if form is None:
        monkeypatch.delenv('ST2_LBFGS_FORM', raising=False)
    else:
        monkeypatch.setenv('ST2_LBFGS_FORM', form)


def _engine(h, w, kind, step, precision='fp32'):
    eng = st2.Engine(TOPO, precision=precision)
    eng.load_weights(oracle.he_init_weights(TOPO, seed=0, bias_std=0.1))
    rs = np.random.RandomState(h + w)
    eng.set_content(rs.randint(0, 256, (h, w, 3)).astype(np.uint8))
    eng.set_style(rs.randint(0, 256, (12, 10, 3)).astype(np.uint8))
    eng.set_input_nchw(q.x0(h, w))
    eng.set_weights([], [], [], [], PARAMS4)            # image terms only: no layer is visited
    eng.optimizer_reset(kind, step)
    assert eng.trace_len() == 8
    return eng


def _run_lbfgs(eng, sched, events=None):
    """The scheduled run, every iterate read back: ([x], [loss])."""
    xs, losses = [], []
    for k in range(sched['steps']):
        if events and k in events:
            events[k](eng)
        eng.optimizer_set_step(q.lbfgs_step_size(k, sched))
        _, trace, loss = eng.step()
        assert trace[-2] == loss
        xs.append(eng.get_input_nchw())
        losses.append(float(loss))
    return xs, losses


def _hold(xs, losses, ref, tag, x_atol=q.X_ATOL):
    dx = [q.max_abs(x, r[0]) for x, r in zip(xs, ref)]
    dl = [abs(l / r[1] - 1) for l, r in zip(losses, ref)]
    print('[%s] worst max|x_dev - x64| %.3g (step %d), worst relative loss deviation %.3g (step %d); bars %g and %g'
          % (tag, max(dx), int(np.argmax(dx)), max(dl), int(np.argmax(dl)), x_atol, q.LOSS_RTOL))
    assert len(xs) == len(ref)
    assert max(dx) <= x_atol, (tag, dx)
    assert max(dl) <= q.LOSS_RTOL, (tag, dl)


def _rejected_steps_leave_the_iterate(xs, ref, sched, tag):
    for k in sched['tiny_at']:
        smax, may_move = q.tiny_step_effect(ref, k)
        moved = q.max_abs(xs[k], xs[k - 1])
        print('[%s] rejected step %d: max|s| %.3g, iterate moved by %.3g%s' % (tag, k, smax, moved, '' if may_move else ' (must not move)'))
        assert moved <= 4 * smax, (tag, k, moved, smax)
        if not may_move:
            assert np.array_equal(xs[k], xs[k - 1]), (tag, k)
        if k + 1 not in sched['tiny_at']:
            assert q.max_abs(xs[k + 1], xs[k]) > 1e3 * smax, (tag, k)     # ... and the next full step moves it again


# ---------------------------------------------------------------------------------------------------------------- a. trajectory
@pytest.mark.parametrize('h,w', q.SIZES)
@pytest.mark.parametrize('form', ['chain', 'gram'])
def test_lbfgs_follows_float64_through_evictions_and_rejections(form, h, w, monkeypatch):
    ref, log = q.reference('lbfgs', h, w)
    tag = 'lbfgs %s %dx%d' % (form, h, w)
    xs, losses = _plain_run(monkeypatch, form, h, w)
    _hold(xs, losses, ref, tag)
    _rejected_steps_leave_the_iterate(xs, ref, SCHED, tag)
    eng = _engine(h, w, OPT_LBFGS, SCHED['step'])
    again, losses2 = _run_lbfgs(eng, SCHED)
    eng.close()
    assert all(np.array_equal(a, b) for a, b in zip(xs, again)) and losses == losses2        # fixed-order reductions


def _plain_run(monkeypatch, form, h, w):
    """(iterates, losses) of the scheduled run under ST2_LBFGS_FORM=form, which stays set for the caller's own engines."""
    _set_form(monkeypatch, form)
    if (form, h, w) not in _runs:
        eng = _engine(h, w, OPT_LBFGS, SCHED['step'])
        _runs[form, h, w] = _run_lbfgs(eng, SCHED)
        eng.close()
    return _runs[form, h, w]


# ------------------------------------------------------------------------------------------------------------------ b. queueing
@pytest.mark.parametrize('form', ['chain', 'gram'])
def test_lbfgs_steps_queued_without_a_read_back_end_where_the_plain_run_ends(form, monkeypatch):
    """The ring, the pair count and the gate live on the device: 36 steps queued with nothing read back, and 36 steps through
    step_begin / step_end with two iterations in flight, leave the iterate of the step-by-step run, bit for bit."""
    h, w = q.SIZES[1]
    want = _plain_run(monkeypatch, form, h, w)[0]
    eng = _engine(h, w, OPT_LBFGS, SCHED['step'])
    for k in range(SCHED['steps']):
        eng.optimizer_set_step(q.lbfgs_step_size(k, SCHED))
        eng.step(want_image=False, want_trace=False)
    assert np.array_equal(eng.get_input_nchw(), want[-1])
    eng.close()
    eng = _engine(h, w, OPT_LBFGS, SCHED['step'])
    collected = 0
    for k in range(SCHED['steps']):
        eng.optimizer_set_step(q.lbfgs_step_size(k, SCHED))
        eng.step_begin()
        if eng.steps_pending() == 2:
            eng.step_end()
            collected += 1
    eng.step_end()
    assert eng.steps_pending() == 0 and collected + 1 == SCHED['steps']
    assert np.array_equal(eng.get_input_nchw(), want[-1])
    eng.close()


# -------------------------------------------------------------------------------------------------------- c. default form (bf16)
def test_bf16_engine_picks_the_gram_form_and_follows_float64(monkeypatch):
    _set_form(monkeypatch, None)
    h, w = q.SIZES[1]
    ref, _ = q.reference('lbfgs', h, w)
    eng = _engine(h, w, OPT_LBFGS, SCHED['step'], precision='bf16')
    xs, losses = _run_lbfgs(eng, SCHED)
    eng.close()
    _hold(xs, losses, ref, 'lbfgs bf16 engine, form unset, %dx%d' % (h, w))
    _rejected_steps_leave_the_iterate(xs, ref, SCHED, 'lbfgs bf16 engine')
    gram = _plain_run(monkeypatch, 'gram', h, w)[0]
    same = all(np.array_equal(a, b) for a, b in zip(xs, gram))
    print('[lbfgs bf16 engine] bit-identical to the fp32 engine under ST2_LBFGS_FORM=gram: %s' % same)
    # no layer is visited, so the precision of the feature path changes nothing: the default of a bf16 engine IS the Gram form
    assert same


# ------------------------------------------------------------------------------------------------------ d. history cleared mid-run
@pytest.mark.parametrize('form', ['chain', 'gram'])
def test_lbfgs_history_cleared_in_mid_run(form, monkeypatch):
    """A replacement input and objective_changed after step 20 (ten live pairs, the ring wrapped): the history and the cached gradient
    are dropped (optimizers.py:121-125), the Gram form's matrix and coefficients with them; 16 more steps, one of them rejected."""
    _set_form(monkeypatch, form)
    h, w = q.SIZES[1]
    ref, _ = q.reference('lbfgs_cleared', h, w)
    sched = dict(SCHED, steps=len(ref))

    def replace(eng):
        eng.set_input_nchw(q.x0(h, w, q.CLEARED['seed']))
        eng.objective_changed()
    eng = _engine(h, w, OPT_LBFGS, SCHED['step'])
    xs, losses = _run_lbfgs(eng, sched, {q.CLEARED['at']: replace})
    eng.close()
    _hold(xs, losses, ref, 'lbfgs %s %dx%d, cleared after step %d' % (form, h, w, q.CLEARED['at'] - 1))
    _rejected_steps_leave_the_iterate(xs, ref, sched, 'lbfgs %s cleared' % form)


# ------------------------------------------------------------------------------------------------------------ e. second grid sweep
def _history(rng, shape, n_pairs):
    """(s, y, s.y) triples with positive curvature: y = D s + noise for a positive diagonal D (as tests/test_gpu_lbfgs.py)."""
    d = (0.5 + rng.rand(*shape)).astype(F32)
    pairs = []
    for _ in range(n_pairs):
        s = rng.randn(*shape).astype(F32)
        y = (d * s + 0.05 * rng.randn(*shape)).astype(F32)
        pairs.append((s, y, oracle.descent.sdot(s, y)))
    return pairs


@pytest.mark.parametrize('n_pairs', [3, 10])
@pytest.mark.parametrize('form', ['chain', 'gram'])
def test_two_loop_at_a_length_that_needs_a_second_grid_sweep(form, n_pairs, monkeypatch):
    """Every link launches 1024 x 256 threads, one float4 each per sweep: 3 x 592 x 600 / 4 = 266 400 > 262 144, so the grid-stride
    loops run a second, partly filled sweep.  H g element by element against LBFGSOracle.inv_hessian_times, the bar of
    test_device_two_loop_matches_oracle_inv_hessian_times."""
    _set_form(monkeypatch, form)
    h, w = q.BIG_SIZE
    assert 3 * h * w // 4 > 1024 * 256
    rng = np.random.RandomState(100 * n_pairs + h)
    shape = (1, 3, h, w)
    pairs = _history(rng, shape, n_pairs)
    g = (rng.randn(*shape) * 3).astype(F32)
    ora = oracle.LBFGSOracle(np.zeros(shape, F32), None)
    ora.pairs = list(pairs)
    want = ora.inv_hessian_times(g)
    eng = st2.Engine(TOPO)
    eng.set_input(np.zeros((h, w, 3), np.uint8))
    got = eng.lbfgs_inv_hv([(s, y) for s, y, _ in pairs], g)
    err = rel_l2(got, want)
    tail = rel_l2(got.ravel()[4 * 1024 * 256:], want.ravel()[4 * 1024 * 256:])
    print('[inv_hv %s] %dx%d, %d pairs: rel-L2 %.2e (elements of the second sweep alone: %.2e)' % (form, h, w, n_pairs, err, tail))
    assert got.shape == want.shape and err <= 1e-5 and tail <= 1e-5, (err, tail)
    assert np.array_equal(eng.lbfgs_inv_hv([(s, y) for s, y, _ in pairs], g), got)
    eng.close()


@pytest.mark.parametrize('form', ['chain', 'gram'])
def test_lbfgs_follows_float64_at_a_length_that_needs_a_second_grid_sweep(form, monkeypatch):
    """14 steps at 592 x 600: ten pairs by step 9, evictions from step 10, a rejection at step 12 (its s.y is 2.3e-13 in float64, the
    events and margins of this size are asserted by tests/test_quadratic_oracle_cpu.py)."""
    _set_form(monkeypatch, form)
    h, w = q.BIG_SIZE
    sched = q.SCHEDULE['lbfgs_big']
    ref, _ = q.reference('lbfgs_big', h, w)
    eng = _engine(h, w, OPT_LBFGS, sched['step'])
    xs, losses = _run_lbfgs(eng, sched)
    eng.close()
    _hold(xs, losses, ref, 'lbfgs %s %dx%d' % (form, h, w))
    _rejected_steps_leave_the_iterate(xs, ref, sched, 'lbfgs %s %dx%d' % (form, h, w))


# ----------------------------------------------------------------------------------------------------------- f. tile-sharded form
class _ScheduledRank:
    """A FusedTiledTransfer whose step size follows the schedule."""
    def __init__(self, ft, sched):
        self.ft, self.sched, self.k = ft, sched, 0

    def step(self):
        self.ft.backend.engine.optimizer_set_step(q.lbfgs_step_size(self.k, self.sched))
        self.k += 1
        return self.ft.step()

    def tile_x(self):
        """This rank's tile of the iterate, (1, 3, th, tw), as it lies in the window."""
        t, wd = self.ft.grid.tiles[self.ft.rank], self.ft.grid.windows[self.ft.rank]
        return self.ft.backend.engine.get_input_nchw()[:, :, t.y0 - wd.y0:t.y1 - wd.y0, t.x0 - wd.x0:t.x1 - wd.x0].copy()


def test_tile_sharded_lbfgs_follows_float64_on_a_1x2_grid():
    """The third implementation of the recursion (lbfgs_gram_commit_k modes 3-5 around one all-reduce of the new inner products) on two
    ranks.  The whole gradient is TV plus p-norm here, and TV couples the pixels across the tile border and, periodically, across the
    image edge: the 1-px ring and the apron refresh are exercised by every step.

    Tile mode has never run with an empty active list (st_tile_backward would start from layer -1), so the table is
    {'content': {'conv1_1': 1e-12}}: the layer's gradient is normalised to unit RMS before it is weighted, so it adds 1e-12 to a
    gradient of order 1e-3 to 1e-1 -- below fp32 resolution -- and the float64 reference ignores it.  Its loss term is not negligible
    beside a loss that falls to 1e-2, so the loss compared is t_loss + p_loss of the trace, which is the quadratic itself."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    h, w, world = 64, 128, 2
    topo = oracle.tiny_topology((8, 16), (2, 2))
    ref, log = q.reference('lbfgs', h, w)
    q.assert_events(log, SCHED, tag='float64 %dx%d' % (h, w))
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (20, 28, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))
    net_params = oracle.he_init_weights(topo, 0, 0.1)
    weights = {'content': {'conv1_1': 1e-12}, 'style': {}, 'deepdream': {}}
    params = {k: q.JOB[k] for k in ('tv', 'tv_power', 'p', 'p_power')}
    grid = tiling.TileGrid(h, w, 1, world, topo, 5)
    fabric = tiled.InProcessFabric(world, 120.0)
    x_start = q.x0(h, w)
    ranks = []
    for r in range(world):
        backend = HipTileBackend(net_params, grid, r, content, style, init, weights, params, step_size=SCHED['step'], topology=topo,
                                 optimizer='lbfgs')
        backend.comm_init_local(r, world, fabric)
        wd = grid.windows[r]
        backend.engine.set_input_nchw(x_start[:, :, wd.y0:wd.y1, wd.x0:wd.x1])       # the job's x0 itself, not an image rounded to it
        ranks.append(_ScheduledRank(tiled.FusedTiledTransfer(grid, r, backend), SCHED))
    out = tiled.run_in_process(ranks, SCHED['steps'], fabric, on_step=lambda r, k, rank, vals: (rank.tile_x(), np.asarray(vals)))
    xs, losses = [], []
    for k in range(SCHED['steps']):
        full = np.zeros((1, 3, h, w), F32)
        for r in range(world):
            t = grid.tiles[r]
            full[:, :, t.y0:t.y1, t.x0:t.x1] = out[r][k][0]
            assert np.array_equal(out[r][k][1], out[0][k][1]), (k, r)                 # every rank derives the same trace
        vals = out[0][k][1]
        assert len(vals) == 14
        xs.append(full)
        losses.append(float(vals[-7] + vals[-6]))                                     # t_loss + p_loss
    for rank in ranks:
        rank.ft.backend.engine.close()
    _hold(xs, losses, ref, 'lbfgs tile-sharded 1x2, %dx%d' % (h, w))
    _rejected_steps_leave_the_iterate(xs, ref, SCHED, 'lbfgs tile-sharded 1x2')


# ------------------------------------------------------------------------------------------------------------------------ g. Adam
@pytest.mark.parametrize('h,w', q.SIZES)
def test_adam_follows_float64_through_a_new_input_and_a_new_step_size(h, w):
    sched = q.SCHEDULE['adam']
    ref, states = q.reference('adam', h, w)
    eng = _engine(h, w, OPT_ADAM, sched['step'])
    xs, losses, worst_m, worst_v = [], [], 0.0, 0.0
    for k in range(sched['steps']):
        if k == sched['new_input_at']:
            eng.set_input_nchw(q.x0(h, w, sched['new_input_seed']))
            eng.objective_changed()
        eng.optimizer_set_step(sched['late_step'] if k >= sched['late_from'] else sched['step'])
        _, trace, loss = eng.step()
        xs.append(eng.get_input_nchw())
        losses.append(float(loss))
        if k in q.ADAM_STATE_STEPS:
            m, v, i1, i2 = eng.adam_get_state()
            m64, v64, j1, j2 = states[k]
            assert (i1, i2) == (j1, j2), (k, i1, i2, j1, j2)          # items1 restarts at objective_changed, items2 does not
            dm, dv = q.max_rel(m, m64), q.max_rel(v, v64)
            worst_m, worst_v = max(worst_m, dm), max(worst_v, dv)
            assert dm <= q.ADAM_M_RTOL and dv <= q.ADAM_V_RTOL, (k, dm, dv)
    eng.close()
    print('[adam %dx%d] m within %.3g, v within %.3g of float64 (relative to their max); bars %g and %g'
          % (h, w, worst_m, worst_v, q.ADAM_M_RTOL, q.ADAM_V_RTOL))
    _hold(xs, losses, ref, 'adam %dx%d' % (h, w), x_atol=q.ADAM_X_ATOL)
