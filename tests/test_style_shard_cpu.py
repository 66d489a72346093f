"""The style targets of a tile-sharded job, sharded as well -- on the CPU: the geometry of the style image's own grid
(tiling.style_grid), the numpy restatement of the pass over the oracle (window forward -> raw Gram sums over the tile's region ->
sum over the ranks -> division by the global element count, worker.py:109-114), and the same through tiled.TiledTransfer's phase
driver with the ranks as threads (tiled.LocalComm)."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import oracle                                                     # noqa: E402
from style_transfer2_amd import tiled, tiling                     # noqa: E402
from style_transfer2_amd.engine import VGG19_TOPOLOGY             # noqa: E402
from tile_oracle import OracleTileBackend                         # noqa: E402

F32 = np.float32
TOPO = oracle.tiny_topology((8, 16, 16), (2, 2, 1), final_pool=True)          # 8 layers, three pools: stride 8 at pool3
LAST = len(TOPO)
# (style image, cut): even cuts, a ragged image (clipped ceil-mode pooling windows at the far edges), a thin one cut four ways
SHAPES = [((96, 128), (1, 2)), ((96, 128), (2, 2)), ((75, 101), (2, 2)), ((43, 150), (1, 4))]
# The Gram of every blob against the whole-image Gram, relative to its largest entry.  Two correct fp32 forwards differ by ulps (BLAS
# blocks by width) and the per-tile sums associate differently: 6e-8 per rounding times a random walk over the few thousand terms of
# an entry stays far below 1e-6 (observed on these shapes: 4.3e-9).
GRAM_TOL = 1e-6


def style_image(h, w, seed=2):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def raw_style_sums(net, style, grid, rank, last_blob):
    """One rank's share: the window of the style image forwarded on its own, F F^T over the tile's region of blobs 0 .. last_blob,
    un-normalised, back to back in one flat float32 array (zeros for a rank beyond the grid) -- the buffer of st_tile_style_partials."""
    names = net.layers()[:last_blob + 1]
    chans = [net.blob_shape(n, 16, 16)[0] for n in names]
    if rank >= grid.world:
        return np.zeros(sum(c * c for c in chans), F32)
    w = grid.windows[rank]
    feats = net.forward(net.preprocess(np.ascontiguousarray(style[w.y0:w.y1, w.x0:w.x1])), names)
    geo = tiling.blob_geometry(net.topology, w.y1 - w.y0, w.x1 - w.x0)
    parts = []
    for i, name in enumerate(names):
        c, h, wd, s = geo[i]
        r = grid.roi_in_blob(rank, (h, wd), s)
        f = feats[name][0][:, r.y0:r.y1, r.x0:r.x1].reshape(c, -1)
        parts.append(np.dot(f, f.T).ravel())
    return np.concatenate(parts).astype(F32)


def commit_style_sums(net, sums, grid, last_blob):
    """{blob name: target} from the reduced sums: division by the blob's GLOBAL C h w as a float32 (oracle.gram)."""
    geo = tiling.blob_geometry(net.topology, grid.gH, grid.gW)
    out, pos = {}, 0
    for i, name in enumerate(net.layers()[:last_blob + 1]):
        c, h, w, _ = geo[i]
        out[name] = sums[pos:pos + c * c].reshape(c, c) / F32(c * h * w)
        pos += c * c
    return out


def whole_grams(net, style):
    return {k: oracle.gram(v) for k, v in net.forward(net.preprocess(style)).items()}


# ------------------------------------------------------------------------------------------------------------ geometry
def test_style_grid_edges_sit_on_stride_multiples_and_cover_the_image():
    for (h, w), world in (((96, 128), 4), ((75, 101), 4), ((43, 150), 4), ((640, 1000), 8)):
        for topo, last in ((TOPO, LAST), (TOPO, 4), (VGG19_TOPOLOGY, 17)):
            g = tiling.style_grid(h, w, world, topo, last)
            s = tiling.total_stride(topo, last)
            assert g.world == g.rows * g.cols <= world and (g.gH, g.gW) == (h, w) and g.last_blob == last
            assert g.stride == s and g.apron == tiling.receptive_apron(topo, last)
            cover = np.zeros((h, w), int)
            for t, win in zip(g.tiles, g.windows):
                assert t.y0 % s == 0 and t.x0 % s == 0 and win.y0 % s == 0 and win.x0 % s == 0
                assert (t.y1 % s == 0 or t.y1 == h) and (t.x1 % s == 0 or t.x1 == w)
                assert tiling.rect_and(win, t) == t
                cover[t.y0:t.y1, t.x0:t.x1] += 1
            assert np.all(cover == 1)


def test_style_grid_prefers_the_smallest_peak_window_then_the_smallest_summed_area():
    def areas(g):
        return [(w.y1 - w.y0) * (w.x1 - w.x0) for w in g.windows]
    # every admissible cut is no better than the chosen one
    for (h, w), world, topo, last in (((96, 128), 4, TOPO, LAST), ((512, 640), 8, VGG19_TOPOLOGY, 17), ((43, 150), 4, TOPO, LAST)):
        g = tiling.style_grid(h, w, world, topo, last)
        best = (max(areas(g)), sum(areas(g)))
        for rows in range(1, world + 1):
            for cols in range(1, world // rows + 1):
                try:
                    other = tiling.TileGrid(h, w, rows, cols, topo, last)
                except ValueError:
                    continue
                assert best <= (max(areas(other)), sum(areas(other))), (rows, cols)
    # a real job: the 8192 x 5120 style image of the example pair over the eight ranks of the 2 x 4 layout is cut eight ways
    g = tiling.style_grid(5120, 8192, 8, VGG19_TOPOLOGY, 17)
    assert g.world == 8 and max(areas(g)) < 5120 * 8192 / 6


def test_style_grid_leaves_ranks_without_a_tile_where_cutting_further_does_not_help():
    # 16 x 40 under an 8-px apron, stride 4: the rows cannot be cut to any gain (a half plus its apron is the whole height), five
    # columns of 8 px give windows of at most 16 x 24, and no finer cut has a smaller one -- eight ranks, five tiles
    topo = (('conv', 'a', 3, 4), ('conv', 'b', 4, 4), ('pool', 'p1'), ('conv', 'c', 4, 4), ('pool', 'p2'), ('conv', 'd', 4, 4))
    assert tiling.total_stride(topo, 6) == 4 and tiling.receptive_apron(topo, 6) == 8
    g = tiling.style_grid(16, 40, 8, topo, 6)
    assert (g.rows, g.cols) == (1, 5) and g.world == 5 < 8
    assert g.windows == [tiling.Rect(0, 0, 16, 16), tiling.Rect(0, 0, 16, 24), tiling.Rect(0, 8, 16, 32), tiling.Rect(0, 16, 16, 40),
                         tiling.Rect(0, 24, 16, 40)]


def test_style_grid_of_an_image_too_small_for_any_cut_is_the_image():
    g = tiling.style_grid(20, 24, 8, VGG19_TOPOLOGY, 17)               # stride 16: neither edge takes two tiles
    assert (g.rows, g.cols, g.world) == (1, 1, 1) and g.tiles == g.windows == [tiling.Rect(0, 0, 20, 24)]
    g = tiling.style_grid(7, 5, 4, TOPO, LAST)
    assert g.world == 1 and g.windows == [tiling.Rect(0, 0, 7, 5)]
    with pytest.raises(ValueError):
        tiling.style_grid(64, 64, 0, TOPO, LAST)
    with pytest.raises(ValueError, match='average pools'):
        tiling.style_grid(64, 64, 2, (('conv', 'a', 3, 4), ('pool', 'p', 'ave')), 2)


# ------------------------------------------------------------------------------------- the pass, restated on the oracle
@pytest.fixture(scope='module')
def net():
    return oracle.NetOracle(TOPO, oracle.he_init_weights(TOPO, 3, 0.1))


@pytest.fixture(scope='module')
def references(net):
    """Whole-image Grams per style shape, computed once."""
    return {hw: whole_grams(net, style_image(*hw)) for hw in sorted({s for s, _ in SHAPES})}


@pytest.mark.parametrize('hw,cut', SHAPES)
def test_region_features_and_sharded_grams_match_the_whole_image(net, references, hw, cut):
    style = style_image(*hw)
    grid = tiling.TileGrid(hw[0], hw[1], cut[0], cut[1], TOPO, LAST)
    whole = net.forward(net.preprocess(style))
    whole = {k: v.copy() for k, v in whole.items()}
    ggeo = tiling.blob_geometry(TOPO, *hw)
    for rank, (w, t) in enumerate(zip(grid.windows, grid.tiles)):
        feats = net.forward(net.preprocess(np.ascontiguousarray(style[w.y0:w.y1, w.x0:w.x1])))
        geo = tiling.blob_geometry(TOPO, w.y1 - w.y0, w.x1 - w.x0)
        for i, name in enumerate(net.layers()):
            c, h, wd, s = geo[i]
            r = grid.roi_in_blob(rank, (h, wd), s)
            y0, x0 = t.y0 // s, t.x0 // s
            mine = feats[name][0][:, r.y0:r.y1, r.x0:r.x1]
            theirs = whole[name][0][:, y0:y0 + r.y1 - r.y0, x0:x0 + r.x1 - r.x0]
            assert mine.shape == theirs.shape and (t.y1 != hw[0] or y0 + r.y1 - r.y0 == ggeo[i][1])
            assert np.allclose(mine, theirs, rtol=1e-5, atol=1e-5 * np.abs(theirs).max()), (rank, name)   # ulps, not bits
    sums = sum(raw_style_sums(net, style, grid, r, LAST) for r in range(grid.world))
    got = commit_style_sums(net, sums, grid, LAST)
    assert sorted(got) == sorted(references[hw])
    for name, ref in references[hw].items():
        err = np.abs(got[name] - ref).max() / np.abs(ref).max()
        assert err <= GRAM_TOL, (name, err)


# ------------------------------------------------------------------------------- through the phase driver, ranks as threads
class ShardedStyleOracleBackend(OracleTileBackend):
    """OracleTileBackend whose style targets come from the sharded pass: the two halves tiled.TiledTransfer.shard_style drives."""

    oracle_lock = threading.Lock()           # the oracle's conv layers share module-level scratch arrays: one forward at a time

    count_lock, inside, most_inside = threading.Lock(), 0, 0     # ranks between the start of their pass and their all-reduce

    def style_partials(self, style, style_grid):
        cls = ShardedStyleOracleBackend
        with cls.count_lock:
            cls.inside += 1
            cls.most_inside = max(cls.most_inside, cls.inside)
        try:
            self._style_grid = style_grid
            with self.oracle_lock:
                self._sp = raw_style_sums(self.net, style, style_grid, self.rank, style_grid.last_blob)
        finally:
            with cls.count_lock:
                cls.inside -= 1
        return torch.from_numpy(self._sp)

    def style_commit(self):
        self.grams = commit_style_sums(self.net, self._sp, self._style_grid, self._style_grid.last_blob)


CONTENT_WEIGHTS = {'content': {'conv2_1': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1}, 'deepdream': {}}
PARAMS = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}


@pytest.mark.parametrize('world,hw,cut', [(2, (96, 128), (1, 2)), (4, (75, 101), (2, 2)), (4, (43, 150), (1, 4)), (4, (96, 128), (1, 2))])
def test_phase_driver_shards_the_style_pass_over_local_comm_threads(net, references, world, hw, cut):
    """tiled.TiledTransfer.shard_style on every rank of a 1 x world content grid, one thread each: partials -> Comm.all_reduce ->
    commit.  The last case has four ranks and two style tiles: ranks 2 and 3 contribute zeros."""
    style = style_image(*hw)
    sgrid = tiling.TileGrid(hw[0], hw[1], cut[0], cut[1], TOPO, LAST)
    rs = np.random.RandomState
    content, init = rs(1).randint(0, 256, (32, 64, 3)).astype(np.uint8), rs(3).randint(0, 256, (32, 64, 3)).astype(np.uint8)
    grid = tiling.TileGrid(32, 64, 1, world, TOPO, 4)
    fabric = tiled.InProcessFabric(world, timeout=60.0)
    small = style_image(16, 16)                            # the constructor's whole-image targets: replaced by the pass
    backends = [ShardedStyleOracleBackend(TOPO, net.params, grid, r, content, small, init, CONTENT_WEIGHTS, PARAMS) for r in range(world)]
    drivers = [tiled.TiledTransfer(grid, r, backends[r], tiled.LocalComm(fabric, r)) for r in range(world)]
    tiled.run_collective([lambda d=d: d.shard_style(style, sgrid) for d in drivers], fabric)
    assert fabric.reduces == 1
    for name, ref in references[hw].items():
        for r in range(world):
            assert np.array_equal(backends[r].grams[name], backends[0].grams[name]), (name, r)    # one reduced buffer, one division
        err = np.abs(backends[0].grams[name] - ref).max() / np.abs(ref).max()
        assert err <= GRAM_TOL, (name, err)


def test_ranks_take_turns_through_the_style_pass(net, references):
    """run_collective(in_turns=True), as jobs.run_tiled_job runs the pass on one GPU: a rank starts its window when the one before it
    has arrived at the all-reduce, so only one rank's transient activation set is alive at a time; same targets."""
    hw, world = (75, 101), 4
    style = style_image(*hw)
    sgrid = tiling.TileGrid(hw[0], hw[1], 2, 2, TOPO, LAST)
    rs = np.random.RandomState
    content, init = rs(1).randint(0, 256, (32, 64, 3)).astype(np.uint8), rs(3).randint(0, 256, (32, 64, 3)).astype(np.uint8)
    grid = tiling.TileGrid(32, 64, 1, world, TOPO, 4)
    fabric = tiled.InProcessFabric(world, timeout=60.0)
    backends = [ShardedStyleOracleBackend(TOPO, net.params, grid, r, content, style_image(16, 16), init, CONTENT_WEIGHTS, PARAMS)
                for r in range(world)]
    drivers = [tiled.TiledTransfer(grid, r, backends[r], tiled.LocalComm(fabric, r)) for r in range(world)]
    ShardedStyleOracleBackend.most_inside = 0
    tiled.run_collective([lambda d=d: d.shard_style(style, sgrid) for d in drivers], fabric, in_turns=True)
    assert ShardedStyleOracleBackend.most_inside == 1 and fabric.reduces == 1 and fabric.turn_of is None and not fabric.turn.locked()
    for name, ref in references[hw].items():
        assert np.abs(backends[0].grams[name] - ref).max() / np.abs(ref).max() <= GRAM_TOL, name


def test_run_collective_reports_a_failing_rank_and_releases_the_others():
    fabric = tiled.InProcessFabric(2, timeout=60.0)

    def good():
        fabric.allreduce(0, np.ones(2, F32))

    def bad():
        raise ValueError('rank 1 broke')
    for in_turns in (False, True):
        fabric = tiled.InProcessFabric(2, timeout=60.0)
        with pytest.raises(RuntimeError) as info:
            tiled.run_collective([good, bad], fabric, in_turns=in_turns)
        assert 'rank 1 broke' in str(info.value) and info.value.still_running is False and not fabric.turn.locked()
