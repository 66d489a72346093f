"""The per-pixel seam check of the tile-sharded mode, on the CPU: the reference alone meets the bar (oracle tiles against the oracle on
the whole image), the check has teeth (planted defects in the CPU driver's plans are caught with a margin), and plans cut into
single-row rectangles move the same pixels.  test_gpu_seams.py holds the HIP path to the same reference with the same bars."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import seam_oracle as so                                          # noqa: E402
from style_transfer2_amd import tiled, tiling                     # noqa: E402

F32 = np.float32


def oracle_ranks(c, grid):
    return [so.oracle_rank(c, grid, r) for r in range(grid.world)]


# ------------------------------------------------------------------------------------------------ a. the reference alone meets the bar
@pytest.mark.parametrize('case_id', so.CASE_IDS)
def test_oracle_tiles_match_the_oracle_on_the_whole_image_per_pixel(case_id):
    """L-BFGS, one step: evaluation 1 (norms captured), the step, the apron refresh, evaluation 2 (norms frozen).  Stitched scd and
    combined gradients within the fp32 bar of the 1 x 1 reference at the same x; windows and rings exact."""
    c = so.case(case_id)
    grid = so.grid_of(c)
    ranks = so.run_phase_driver(c, grid, oracle_ranks(c, grid), 'lbfgs', 1)
    assert len(ranks[0].evals) == 2
    errors = {}
    so.check_phase_driver(c, grid, ranks, so.WholeReference(c), so.BAR['fp32'], 'oracle tiles, L-BFGS', errors)
    print('[seam-cpu] %s: oracle tiles vs oracle whole: scd %.3g, combined %.3g' % (c.id, errors['scd'], errors['grad']))


@pytest.mark.parametrize('case_id', so.CASE_IDS)
def test_oracle_tiles_adam_steps_keep_windows_rings_and_gradients(case_id):
    """Adam, three steps: the other driver loop (update -> refresh of x_next -> swap).  Same checks after every step."""
    c = so.case(case_id)
    grid = so.grid_of(c)
    ranks = so.run_phase_driver(c, grid, oracle_ranks(c, grid), 'adam', 3)
    assert len(ranks[0].evals) == 3
    so.check_phase_driver(c, grid, ranks, so.WholeReference(c), so.BAR['fp32'], 'oracle tiles, Adam')


@pytest.mark.parametrize('case_id', ['T2-1x2-16x24-std', 'T2-2x2-37x50-scd', 'T4-2x2-37x50-std'])
def test_bf16_oracle_tiles_round_partial_diffs_in_the_seam_band(case_id):
    """With bf16 operands the sharded algorithm itself differs from the whole image beyond fp32 rounding: a conv's data gradient rounds
    its incoming diff to bf16, and near a seam each window holds only its own ranks' part of that diff -- parts are rounded where the
    whole image rounds their sum.  The oracle's tiles show it against the oracle's whole image: beyond the fp32 bar, inside the bf16
    bar, the worst pixel in a seam band.  (The HIP tiles show the same figures at the same pixels: profiles/tile_seam_errors.txt.)"""
    c = so.case(case_id)
    grid = so.grid_of(c)
    ranks = so.run_phase_driver(c, grid, [so.oracle_rank(c, grid, r, 'bf16') for r in range(grid.world)], 'lbfgs', 1)
    errors = {}
    so.check_phase_driver(c, grid, ranks, so.WholeReference(c, 'bf16'), so.BAR['bf16'], 'oracle tiles, bf16 operands', errors)
    assert errors['scd'] > so.BAR['fp32']
    ev = [tt.evals[0] for tt in ranks]
    x = so.stitch(grid, [so.tile_part(grid, r, e['window']) for r, e in enumerate(ev)])
    scd_ref, _ = so.WholeReference(c, 'bf16').evaluate(x)
    _, (_, y, xx) = so.seam_error(so.stitch(grid, [e['scd'] for e in ev]), scd_ref)
    assert 'seam band' in so.locate(grid, y, xx)[3]


# ------------------------------------------------------------------------------------------------ b. planted defects
# Each defect changes CPU objects of the phase driver only (its plan lists, its unpack, the grid's region of interest).  `ranks` are the
# RecordingTransfers of one run, before they start.
def _shift_one_overlap_receive(ranks):
    """One overlap receive rectangle of one rank (the first the grid plans for it) lands one column off (the sender packs what it always
    packed)."""
    tt = ranks[-1]
    src = next(s for s, d, _ in tt.grid.grad_overlap_plan() if d == tt.rank)
    recv = tt.plans[tiled.PLAN_OVERLAP][src][1]
    y, x, h, w = recv[0]
    recv[0] = (y, x + (1 if x + w + 1 <= tt.window.x1 - tt.window.x0 else -1), h, w)


def _drop_the_corner_rectangle(ranks):
    """2 x 2: what the diagonal neighbour owes rank 0 (the four-corner rectangle) is in nobody's plan."""
    assert len(ranks) == 4
    send, recv = ranks[3].plans[tiled.PLAN_OVERLAP][0][0], ranks[0].plans[tiled.PLAN_OVERLAP][3][1]
    assert len(send) == 1 and len(recv) == 1
    del send[0], recv[0]


def _assign_in_place_of_add(ranks):
    for tt in ranks:
        unpack = tt._unpack
        tt._unpack = lambda t, rects, buf, add, unpack=unpack: unpack(t, rects, buf, False)


def _ring_item_one_cell_off(ranks):
    """One received ring column of one rank lands one cell to the right."""
    tt = ranks[0]
    for src, r, ry, rx in tt.grid.ring_plan()[tt.rank]:         # (the first such item the grid plans: a column, before the corners)
        if src != tt.rank and r.x1 - r.x0 == 1 and rx == 0:
            recv = tt.plans[tiled.PLAN_RING][src][1]
            i = recv.index((ry, rx, r.y1 - r.y0, 1))
            recv[i] = (ry, rx + 1, r.y1 - r.y0, 1)
            return
    raise AssertionError('rank 0 receives no left ring column')


def _top_ring_row_from_the_unwrapped_neighbour(ranks):
    """The top ring row of the top tiles comes from the near side of its source rank (that rank's first row: where the neighbour would be
    without the wrap) instead of the image's last row.  (Tiles are more than one row high: a one-row rectangle sent from the image's last
    row is a top ring row or one of its corners.)"""
    grid, hit = ranks[0].grid, 0
    for tt in ranks:
        last = grid.gH - 1 - tt.window.y0
        for dst, (send, _) in tt.plans[tiled.PLAN_RING].items():
            if grid.tiles[dst].y0 != 0:
                continue
            for i, (y, x, h, w) in enumerate(send):
                if y == last and h == 1:
                    send[i] = (tt.tile.y0 - tt.window.y0, x, h, w)
                    hit += 1
    assert hit


def _roi_one_cell_off(ranks):
    """roi_in_blob of one rank starts one cell late in x in every pooled blob (the grid object of this run only)."""
    grid = ranks[0].grid
    target = grid.world - 1
    plain = grid.roi_in_blob

    def roi(rank, blob_hw, blob_stride):
        r = plain(rank, blob_hw, blob_stride)
        return tiling.Rect(r.y0, r.x0 + 1, r.y1, r.x1) if rank == target and blob_stride > 1 else r
    grid.roi_in_blob = roi


def _drop_one_refresh_rectangle(ranks):
    src, dst, _ = ranks[0].grid.apron_refresh_plan()[0]
    send, recv = ranks[src].plans[tiled.PLAN_REFRESH][dst][0], ranks[dst].plans[tiled.PLAN_REFRESH][src][1]
    assert send and len(send) == len(recv)
    del send[0], recv[0]


# (defect, the cases it is tried on): the largest figure over those cases counts
_SMALL = ['T2-1x2-16x24-%s', 'T2-2x1-24x16-%s', 'T2-2x2-37x50-%s', 'T2-3x3-36x44-%s']
DEFECTS = {
    'overlap receive shifted by one column': (_shift_one_overlap_receive, [s % 'scd' for s in _SMALL if '2x1' not in s]),
    'four-corner rectangle dropped': (_drop_the_corner_rectangle, ['T2-2x2-37x50-scd', 'T2-2x2-32x48-std', 'T4-2x2-40x52-std']),
    'overlap assigned, not added': (_assign_in_place_of_add, [s % 'scd' for s in _SMALL]),
    'ring item one cell off': (_ring_item_one_cell_off, [s % 'tv' for s in _SMALL]),
    'top ring row from the unwrapped neighbour': (_top_ring_row_from_the_unwrapped_neighbour, [s % 'tv' for s in _SMALL]),
    'region of interest one cell off in pooled blobs': (_roi_one_cell_off, [s % 'scd' for s in _SMALL] + ['T4-2x2-37x50-std']),
}


def _planted_run(c, plant):
    grid = so.grid_of(c)
    ranks = so.run_phase_driver(c, grid, oracle_ranks(c, grid), 'lbfgs', 1, prepare=plant)
    return grid, ranks


@pytest.mark.parametrize('name', sorted(DEFECTS))
def test_a_planted_seam_defect_is_caught_with_a_margin(name):
    """The per-pixel metric of a run with the defect, over the defect's cases and both evaluations and both tensors: past ten times the
    fp32 bar and past the bf16 bar."""
    plant, case_ids = DEFECTS[name]
    worst = 0.0
    for case_id in case_ids:
        c = so.case(case_id)
        grid, ranks = _planted_run(c, plant)
        ref = so.WholeReference(c)
        for k in range(2):
            ev = [tt.evals[k] for tt in ranks]
            x = so.stitch(grid, [so.tile_part(grid, r, e['window']) for r, e in enumerate(ev)])
            scd_ref, grad_ref = ref.evaluate(x)
            for tensor, want in (('scd', scd_ref), ('grad', grad_ref)):
                err, (ch, y, xx) = so.seam_error(so.stitch(grid, [e[tensor] for e in ev]), want)
                print('[planted] %s on %s, evaluation %d, %s: %.3g at pixel (%d, %d): rank %d, %d px from its tile edge, %d px from the border, %s'
                      % ((name, c.id, k + 1, tensor, err, y, xx) + so.locate(grid, y, xx)))
                worst = max(worst, err)
    f32, b16 = worst / so.BAR['fp32'], worst / so.BAR['bf16']
    print('[planted] %s: metric %.3g = %.3g x the fp32 bar, %.3g x the bf16 bar' % (name, worst, f32, b16))
    assert f32 > 10.0 and b16 > 1.0, (name, worst)
    assert np.isclose(worst, so.PLANTED_METRIC[name], rtol=0.05), (name, worst)        # the recorded figure is this one


def test_a_dropped_refresh_rectangle_breaks_the_exact_window_check():
    c = so.case('T2-2x2-37x50-std')
    grid, ranks = _planted_run(c, _drop_one_refresh_rectangle)
    with pytest.raises(AssertionError, match='differs from the stitched image'):
        so.exact_windows(grid, [tt.window_now() for tt in ranks], 'planted')
    so.exact_windows(grid, [tt.evals[0]['window'] for tt in ranks], 'before the step')        # (and only after the step)


# ------------------------------------------------------------------------------------------------ c. re-cut plans
def _play(grid, plans, phase, src, dst, add):
    """The exchange of one phase on numpy arrays, messages = concatenated rectangles, as the engine packs them."""
    for a in range(grid.world):
        for b, (send, _) in sorted(plans[a][phase].items()):
            msg = np.concatenate([src[a][:, y:y + h, x:x + w].ravel() for y, x, h, w in send])
            pos = 0
            for y, x, h, w in plans[b][phase][a][1]:
                piece = msg[pos:pos + 3 * h * w].reshape(3, h, w)
                pos += 3 * h * w
                if add:
                    dst[b][:, y:y + h, x:x + w] += piece
                else:
                    dst[b][:, y:y + h, x:x + w] = piece
            assert pos == msg.size


def test_rectangle_counts_of_the_case_table_are_the_recorded_ones():
    """The uncut plans of the table stay within one strip_copy_k launch per peer (kMaxStripRects = 12); the re-cut ones do not."""
    uncut = recut = 0
    for c in so.CASES:
        grid = so.grid_of(c)
        for r in range(grid.world):
            plans = tiled.fused_plans(grid, r)
            uncut = max(uncut, so.max_rects_per_peer(plans))
            recut = max(recut, so.max_rects_per_peer(so.recut(plans)))
    print('[seam-cpu] largest rectangle count per peer: %d uncut, %d re-cut' % (uncut, recut))
    assert (uncut, recut) == (so.MAX_RECTS_UNCUT, so.MAX_RECTS_RECUT)
    assert uncut <= tiled.TiledTransfer.MAX_RECTS < recut


@pytest.mark.parametrize('case_id', ['T2-2x2-37x50-std', 'T2-3x3-36x44-std', 'T2-1x2-16x24-std', 'T4-2x2-37x50-std'])
def test_recut_plans_move_the_same_pixels_bit_for_bit(case_id):
    """A rectangle-list property: plans cut into single-row rectangles give the same windows, rings and sums -- played on arrays for
    tiled.fused_plans, and through the CPU driver, which executes the same lists."""
    c = so.case(case_id)
    grid = so.grid_of(c)
    rng = np.random.RandomState(5)
    image = rng.randn(3, c.h, c.w).astype(F32)
    plans = [tiled.fused_plans(grid, r) for r in range(grid.world)]
    outs = []
    for p in (plans, [so.recut(q) for q in plans], [so.recut(q, halves=True) for q in plans]):
        wins = [np.full(so.crop(image, w).shape, np.nan, F32) for w in grid.windows]
        for r in range(grid.world):
            so.tile_part(grid, r, wins[r])[...] = so.crop(image, grid.tiles[r])
        _play(grid, p, tiled.PLAN_REFRESH, wins, wins, False)
        grads = [np.sin(so.crop(image, w) * (r + 1)).astype(F32) for r, w in enumerate(grid.windows)]
        _play(grid, p, tiled.PLAN_OVERLAP, [g.copy() for g in grads], grads, True)
        rings = [np.zeros((3, t.y1 - t.y0 + 2, t.x1 - t.x0 + 2), F32) for t in grid.tiles]
        _play(grid, p, tiled.PLAN_RING, wins, rings, False)
        outs.append((wins, grads, rings))
    for r in range(grid.world):
        assert np.array_equal(outs[0][0][r], so.crop(image, grid.windows[r]))
        for k in range(3):
            assert np.array_equal(outs[0][k][r], outs[1][k][r]) and np.array_equal(outs[0][k][r], outs[2][k][r]), (k, r)
    so.exact_rings(grid, image, outs[1][2], 'recut, played')
    halves = max(t.y1 - t.y0 for t in grid.tiles) <= tiled.TiledTransfer.MAX_RECTS
    runs = [so.run_phase_driver(c, grid, oracle_ranks(c, grid), 'lbfgs', 1, prepare=prep)
            for prep in (None, lambda ranks: [so.recut_driver(tt, halves) for tt in ranks])]
    assert max(so.driver_rects_per_peer(tt) for tt in runs[0]) <= tiled.TiledTransfer.MAX_RECTS
    assert min(so.driver_rects_per_peer(tt) for tt in runs[1]) > tiled.TiledTransfer.MAX_RECTS
    for a, b in zip(*runs):
        assert np.array_equal(a.window_now(), b.window_now())
        for ea, eb in zip(a.evals, b.evals):
            for key in ('scd', 'grad', 'ring', 'window', 'trace'):
                assert np.array_equal(ea[key], eb[key]), (a.rank, key)


def test_locate_names_seam_band_torus_border_and_interior():
    grid = so.grid_of(so.case('T2-3x3-36x44-std'))
    assert so.locate(grid, 0, 0) == (0, 0, 0, 'torus border')
    assert so.locate(grid, 12, 20) == (4, 0, 12, 'seam band')
    assert so.locate(grid, 35, 14)[3] == 'seam band + torus border'
    big = tiling.TileGrid(64, 96, 1, 2, so.T2, 5)
    assert so.locate(big, 30, 20) == (0, 20, 20, 'tile interior')
    err, at = so.seam_error(np.array([[[1.0, 2.0], [3.0, 5.0]]]), np.array([[[1.0, 2.0], [3.0, 4.0]]]))
    assert at == (0, 1, 1) and np.isclose(err, 1.0 / np.sqrt(7.5))
