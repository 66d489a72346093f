"""The seams of the tile-sharded mode on the GPU, per pixel: HipTileBackend ranks (threads of this process over tiled.InProcessFabric,
at most nine engine contexts) against the CPU oracle on the WHOLE image (seam_oracle.WholeReference) -- the stitched network-side and
combined gradients under max |got - want| / rms(want) over all pixels, every rank's whole window and its gathered ring bit for bit.

  driver P        tiled.TiledTransfer phase by phase (strip_copy_k through st_tile_strips), L-BFGS: evaluation 1, one step, evaluation 2
  driver F-lbfgs  tiled.FusedTiledTransfer, st_tile_step with the Gram-form L-BFGS: the gradient buffer after each of two steps
  driver F-adam   the same with Adam: m after the first step is (1 - 0.9) g; windows after each of three steps
  re-cut plans    more than kMaxStripRects rectangles per peer (the chunked strips() of engine_comm.cpp, the torch path of
                  TiledTransfer._pack / _unpack): bit-identical to the uncut plans
  bf16            the rounded-operand oracle as reference, its own bar

The bars and how they were measured: seam_oracle.py; the figures: profiles/tile_seam_errors.txt."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import seam_oracle as so                                          # noqa: E402
from style_transfer2_amd import tiled                             # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
OPERANDS = {'fp32': 'fp32', 'bf16': 'bf16'}
# 1 x 2, 2 x 2 ragged (every parameter set the table gives them) and the stride-4 2 x 2 ragged
BF16_CASES = [i for i in so.CASE_IDS if i.startswith(('T2-1x2-16x24-', 'T2-2x2-37x50-', 'T4-2x2-37x50-'))]
RECUT_CASES = ['T2-2x2-37x50-std', 'T2-3x3-36x44-std']


def hip_ranks(c, grid, precision='fp32', optimizer='adam', step_size=10):
    from style_transfer2_amd.tile_backend import HipTileBackend
    topo = so.TOPOLOGIES[c.topo][0]
    return [HipTileBackend(so.net_params(c.topo), grid, r, *so.backend_args(c), step_size=step_size, topology=topo, precision=precision,
                           optimizer=optimizer) for r in range(grid.world)]


def halves_for(grid):
    """Tiles of no more than MAX_RECTS rows: single-row rectangles alone would not exceed one launch's table."""
    return max(t.y1 - t.y0 for t in grid.tiles) <= tiled.TiledTransfer.MAX_RECTS


# ---------------------------------------------------------------------------------------------------------------- the plain engine
def _plain_cases(case_ids):
    seen, out = set(), []
    for case_id in case_ids:
        c = so.case(case_id)
        key = (c.topo, c.h, c.w, c.params)
        if key not in seen:
            seen.add(key)
            out.append(case_id)
    return out


@pytest.mark.parametrize('precision,case_id', [('fp32', i) for i in _plain_cases(so.CASE_IDS)] + [('bf16', i) for i in _plain_cases(BF16_CASES)])
def test_plain_engine_on_the_whole_image_meets_the_bar_it_sets(precision, case_id):
    """What the bars are measured with: StyleTransfer.opfunc (the single engine, no tile code) against the same reference under the same
    metric -- the combined gradient with the case's scalar parameters and the network-side gradient alone (the same job with p = tv = 0,
    where opfunc returns it) -- at evaluation 1 (norms captured) and evaluation 2 (norms frozen, one signed step of 10 away).  The bar is
    four times the largest figure printed here, so the engine itself stays inside it."""
    import style_transfer2_amd as st2
    c = so.case(case_id)
    for tensor, job in [('grad', c)] + ([('scd', c._replace(params='scd'))] if c.params != 'scd' else []):
        content, style, init, weights, params = so.backend_args(job)
        st = st2.StyleTransfer(st2.HipModel(so.net_params(c.topo), topology=so.TOPOLOGIES[c.topo][0], precision=precision))
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(weights, params)
        st.optimizer_cls = st2.AdamOptimizer; st.set_step_size(10); st.reset()
        assert st.start()
        ref = so.WholeReference(job, OPERANDS[precision])
        whole = so.grid_of(c, 1, 1)
        x = ref.x()
        for k in (1, 2):
            _, grad_ref = ref.evaluate(x)
            _, grad = st.opfunc(x[None])
            so.hold(whole, np.asarray(grad, F32)[0], grad_ref, so.BAR[precision], '%s plain engine %s evaluation %d %s' % (c.id, precision, k, tensor))
            x = (x - F32(10) * np.sign(grad_ref)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- driver P
@pytest.mark.parametrize('case_id', so.CASE_IDS)
def test_phase_driver_holds_gradients_windows_and_rings_per_pixel(case_id):
    c = so.case(case_id)
    grid = so.grid_of(c)
    ranks = so.run_phase_driver(c, grid, hip_ranks(c, grid, step_size=1), 'lbfgs', 1)
    assert len(ranks[0].evals) == 2
    so.check_phase_driver(c, grid, ranks, so.WholeReference(c), so.BAR['fp32'], 'driver P fp32')


@pytest.mark.parametrize('case_id', BF16_CASES)
def test_phase_driver_with_bf16_operands_against_the_rounded_operand_oracle(case_id):
    c = so.case(case_id)
    grid = so.grid_of(c)
    ranks = so.run_phase_driver(c, grid, hip_ranks(c, grid, 'bf16', step_size=1), 'lbfgs', 1)
    so.check_phase_driver(c, grid, ranks, so.WholeReference(c, 'bf16'), so.BAR['bf16'], 'driver P bf16')


@pytest.mark.parametrize('case_id', RECUT_CASES)
def test_phase_driver_with_rectangle_lists_beyond_one_launch_matches_bit_for_bit(case_id):
    """More than MAX_RECTS rectangles per peer: TiledTransfer._pack / _unpack leave strip_copy_k for their torch form."""
    c = so.case(case_id)
    grid = so.grid_of(c)
    runs = [so.run_phase_driver(c, grid, hip_ranks(c, grid, step_size=1), 'lbfgs', 1, prepare=prep)
            for prep in (None, lambda ranks: [so.recut_driver(tt, halves_for(grid)) for tt in ranks])]
    assert max(so.driver_rects_per_peer(tt) for tt in runs[0]) <= tiled.TiledTransfer.MAX_RECTS
    assert min(so.driver_rects_per_peer(tt) for tt in runs[1]) > tiled.TiledTransfer.MAX_RECTS
    for a, b in zip(*runs):
        assert np.array_equal(a.window_now(), b.window_now()), a.rank
        for k, (ea, eb) in enumerate(zip(a.evals, b.evals)):
            for key in ('scd', 'grad', 'ring', 'window', 'trace'):
                assert np.array_equal(ea[key], eb[key]), (a.rank, k, key)


# ---------------------------------------------------------------------------------------------------------------- the fused drivers
def run_fused(c, grid, optimizer, precision, steps, transport, cut=False):
    """`steps` st_tile_step calls per rank, ranks as threads.  Returns (the windows before the first step, per rank and step a dict with
    the whole window of x, the trace, and the tile part of the gradient buffer (L-BFGS) or of Adam's m)."""
    world = grid.world
    fabric = tiled.InProcessFabric(world, 120.0)
    backends = hip_ranks(c, grid, precision, optimizer, {'lbfgs': 1, 'adam': 10}[optimizer])
    ranks = []
    for r, b in enumerate(backends):
        if transport == 'host':
            b.comm_init_host(r, world, lambda v, r=r: fabric.allreduce(r, v), lambda s, rc, r=r: fabric.exchange(r, s, rc))
        else:
            b.comm_init_local(r, world, fabric)
        ranks.append(tiled.FusedTiledTransfer(grid, r, b))
        if cut:
            plans = so.recut(tiled.fused_plans(grid, r), halves_for(grid))
            assert so.max_rects_per_peer(plans) > tiled.TiledTransfer.MAX_RECTS
            for phase, peers in plans.items():
                b.set_plan(phase, peers)
    before = [so.host(b.x_cur()) for b in backends]

    def on_step(r, k, ft, vals):
        b = ft.backend
        rec = {'trace': np.asarray(vals, np.float64), 'window': so.host(b.x_cur())}
        if optimizer == 'lbfgs':            # (the gradient buffer exists only where the image pass runs without an optimizer)
            rec['grad'] = so.host(so.tile_part(grid, r, b._buf(4, (3, b.wh, b.ww))))
        else:
            rec['m'] = so.tile_part(grid, r, b.engine.adam_get_state()[0][0]).copy()
        return rec
    return before, tiled.run_in_process(ranks, steps, fabric, on_step=on_step)


def check_fused_lbfgs(c, grid, precision, transport):
    before, out = run_fused(c, grid, 'lbfgs', precision, 2, transport)
    ref = so.WholeReference(c, OPERANDS[precision])
    ref.evaluate(so.exact_windows(grid, before, '%s F-lbfgs before the first step' % c.id))          # the norms of the first evaluation
    for k in range(2):
        ev = [out[r][k] for r in range(grid.world)]
        tag = '%s driver F-lbfgs %s step %d' % (c.id, precision, k + 1)
        x = so.exact_windows(grid, [e['window'] for e in ev], tag)
        _, grad_ref = ref.evaluate(x)
        so.hold(grid, so.stitch(grid, [e['grad'] for e in ev]), grad_ref, so.BAR[precision], tag + ' grad')
        for e in ev:
            assert np.array_equal(e['trace'], ev[0]['trace']), tag
    return out


def check_fused_adam(c, grid, precision, transport):
    before, out = run_fused(c, grid, 'adam', precision, 3, transport)
    ref = so.WholeReference(c, OPERANDS[precision])
    _, grad_ref = ref.evaluate(so.exact_windows(grid, before, '%s F-adam before the first step' % c.id))
    m = so.stitch(grid, [out[r][0]['m'] for r in range(grid.world)])
    so.hold(grid, m, F32(0.1) * grad_ref, so.BAR[precision], '%s driver F-adam %s step 1 m' % (c.id, precision))
    for k in range(3):
        ev = [out[r][k] for r in range(grid.world)]
        so.exact_windows(grid, [e['window'] for e in ev], '%s driver F-adam %s step %d' % (c.id, precision, k + 1))
        for e in ev:
            assert np.array_equal(e['trace'], ev[0]['trace']), (c.id, k)
    return out


@pytest.mark.parametrize('case_id', so.CASE_IDS)
def test_fused_lbfgs_steps_hold_the_gradient_and_the_windows_per_pixel(case_id):
    c = so.case(case_id)
    check_fused_lbfgs(c, so.grid_of(c), 'fp32', 'local')


@pytest.mark.parametrize('case_id', so.CASE_IDS)
def test_fused_adam_first_moment_is_a_tenth_of_the_gradient_per_pixel(case_id):
    c = so.case(case_id)
    check_fused_adam(c, so.grid_of(c), 'fp32', 'host')


@pytest.mark.parametrize('case_id', BF16_CASES)
def test_fused_adam_with_bf16_operands_against_the_rounded_operand_oracle(case_id):
    c = so.case(case_id)
    check_fused_adam(c, so.grid_of(c), 'bf16', 'local')


@pytest.mark.parametrize('optimizer', ['lbfgs', 'adam'])
@pytest.mark.parametrize('case_id', RECUT_CASES)
def test_fused_steps_with_recut_plans_match_bit_for_bit(case_id, optimizer):
    """st_tile_plan with more than kMaxStripRects rectangles per peer: engine_comm.cpp's strips() launches strip_copy_k in chunks."""
    c = so.case(case_id)
    grid = so.grid_of(c)
    runs = [run_fused(c, grid, optimizer, 'fp32', 2, 'local', cut=cut)[1] for cut in (False, True)]
    for r in range(grid.world):
        for k in range(2):
            for key in ('window', 'trace', 'grad' if optimizer == 'lbfgs' else 'm'):
                assert np.array_equal(runs[0][r][k][key], runs[1][r][k][key]), (r, k, key)
