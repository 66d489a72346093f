"""Per-pixel reference, metric, case table and drivers for the seams of the tile-sharded mode.  TEST INFRASTRUCTURE.

The sharded path (tiling.py, tiled.py, tile_backend.py, engine_tile.cpp, engine_comm.cpp) is data movement around unchanged network
kernels: overlap-add of window gradients, the periodic 1-px ring of the TV stencil, the apron refresh, regions of interest in pooled
blobs.  A defect there changes a few rows or columns of the gradient and leaves every aggregate (loss, gradient norm, iterate MSE)
where it was.  This module holds the gradient of a sharded run to the gradient of the WHOLE image, pixel by pixel:

  reference   tile_oracle.OracleTileBackend on a 1 x 1 grid of the whole image (WholeReference): the network-side gradient
              (backward(), the "scd" part) and the combined gradient (grad_tile()), for the first evaluation (norms captured) and
              for later ones (norms frozen), at an x the caller supplies.  operands='bf16' for runs with bf16 conv operands.
  metric      max over ALL pixels of |got - want| / rms(want), per tensor (seam_error); the message of a miss names the pixel, its
              rank, its distance to the nearest tile edge and image border and where it lies (seam band / torus border / interior).
  cases       CASES: two topologies (stride 2 / apron 6, stride 4 / apron 8), nine grids, three scalar parameter sets.
  drivers     RecordingTransfer: tiled.TiledTransfer that keeps, per evaluation, what the checks need (the driver's own code runs).
  recut       the same exchange plans cut into single-row rectangles: more than kMaxStripRects rectangles per peer.
"""
import threading
from collections import namedtuple

import numpy as np
import torch

import oracle
from style_transfer2_amd import tiled, tiling
from tile_oracle import OracleTileBackend

F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------- the bars
# The bar of a precision is 4 x the largest per-pixel error the PLAIN single engine (StyleTransfer.opfunc on the whole image: not the
# code under test) shows against the same 1 x 1 oracle under the same metric, over CASES and both evaluations, rounded up to one
# significant digit; for fp32 the larger of that and the same rule applied to oracle-tiles-versus-oracle-whole on the CPU.  "The same
# metric" is both tensors: the combined gradient with the case's scalar parameters and the network-side gradient alone (the same job
# with p = tv = 0, where opfunc returns it).  A sharded fp32 run differs from the plain one only in the order of the all-reduced
# partial sums (up to nine ranks) and in which conv launch plan a window size selects: rounding-sized (largest sharded figure: 1.32e-5,
# driver F-lbfgs, T2-2x2-37x50-scd, step 2).  With bf16 operands there is a third difference, by design and not a defect: a conv's data
# gradient rounds its incoming diff to bf16, and in the seam band a window holds only ITS ranks' part of that diff (the injected diffs
# are zero outside the region of interest), so the windows round parts where the whole image rounds their sum.  The sharded bf16
# figures are therefore up to four times the plain engine's, always in a seam band (largest: 0.0144, T4-2x2-37x50-std, scd), and the
# oracle's own bf16 tiles show the SAME figures at the same pixels against the oracle's bf16 whole image
# (test_seam_oracle_cpu.py::test_bf16_oracle_tiles_round_partial_diffs_in_the_seam_band): the HIP windows follow the algorithm.
MEASURED = {
    'cpu_tiles_vs_whole': 5.74e-6,      # oracle tiles against the oracle on the whole image, fp32 (T2-2x2-37x50-std, scd)
    'plain_engine_fp32': 7.22e-6,       # T2-2x2-32x48-std, evaluation 2, scd
    'plain_engine_bf16': 3.74e-3,       # T2-1x2-16x24-std, evaluation 1, scd
}
BAR = {'fp32': 3e-5,                    # 4 x 7.22e-6 = 2.9e-5 (the CPU figure gives 4 x 5.74e-6 = 2.3e-5: the same digit)
       'bf16': 2e-2}                    # 4 x 3.74e-3 = 1.5e-2
# the metric each planted defect of test_seam_oracle_cpu.py reaches on its best case: the smallest is 20 000 x the fp32 bar and 30 x the
# bf16 bar
PLANTED_METRIC = {
    'four-corner rectangle dropped': 0.607,
    'overlap assigned, not added': 3.8,
    'overlap receive shifted by one column': 1.63,
    'region of interest one cell off in pooled blobs': 2.12,
    'ring item one cell off': 0.625,
    'top ring row from the unwrapped neighbour': 0.801,
}
# largest number of rectangles one peer gets in one phase (tiled.fused_plans over CASES); st2_kernels.h kMaxStripRects = 12
MAX_RECTS_UNCUT = 6
MAX_RECTS_RECUT = 40

# ---------------------------------------------------------------------------------------------------------------- the case table
T2 = oracle.tiny_topology((8, 16), (2, 2))                  # conv1_1 conv1_2 pool1 conv2_1 conv2_2: stride 2, apron 6 at blob 5
T4 = oracle.tiny_topology((8, 16, 16), (2, 1, 1))           # conv1_1 conv1_2 pool1 conv2_1 pool2 conv3_1: stride 4, apron 8 at blob 6
TOPOLOGIES = {'T2': (T2, 5), 'T4': (T4, 6)}
# content-only, style-only, pool and style + deep-dream rows (test_gpu_parity.TILED_WEIGHTS); T4 has no conv2_2: its deep content row
# sits on pool2 (a stride-4 pooled blob) and the deepest conv carries a style row
WEIGHTS = {
    'T2': {'content': {'conv2_2': 0.08, 'conv1_2': 0.5}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'pool1': 0.7},
           'deepdream': {'conv2_1': 0.02}},
    'T4': {'content': {'pool2': 0.08, 'conv1_2': 0.5}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'pool1': 0.7, 'conv3_1': 1},
           'deepdream': {'conv2_1': 0.02}},
}
PARAM_SETS = {
    'std': {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2},             # test_gpu_parity.TILED_PARAMS
    'scd': {'p': 0, 'p_power': 6, 'tv': 0, 'tv_power': 2},              # the network-side gradient alone
    'tv': {'p': 50, 'p_power': 2.5, 'tv': 500, 'tv_power': 1.7},        # the ring decides the gradient at the image border
}
Case = namedtuple('Case', 'id topo rows cols h w params')
_ALL, _STD = ('std', 'scd', 'tv'), ('std',)
_GRIDS = [('T2', 1, 2, 16, 24, _ALL),       # a peer that is both the left and the right torus neighbour
          ('T2', 2, 1, 24, 16, _ALL),       # ... the upper and the lower
          ('T2', 2, 2, 32, 48, _STD),
          ('T2', 2, 2, 37, 50, _ALL),       # ragged: ceil-mode pools at the border, odd last tile
          ('T2', 3, 3, 36, 44, _ALL),       # an interior tile with eight neighbours
          ('T2', 1, 4, 16, 32, _STD),       # tiles narrower than twice the apron: a window spans three tiles
          ('T4', 2, 2, 40, 52, _STD),
          ('T4', 2, 2, 37, 50, _STD),
          ('T2', 2, 4, 24, 64, _STD)]
CASES = [Case('%s-%dx%d-%dx%d-%s' % (t, r, c, h, w, p), t, r, c, h, w, p) for t, r, c, h, w, ps in _GRIDS for p in ps]
CASE_IDS = [c.id for c in CASES]


def case(case_id):
    return CASES[CASE_IDS.index(case_id)]


def images(h, w):
    """(content, style, init) as the tile tests draw them (test_gpu_parity._tiled_images)."""
    rs = np.random.RandomState
    return (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (20, 28, 3)).astype(np.uint8),
            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))


_net_params = {}


def net_params(topo_key):
    if topo_key not in _net_params:
        _net_params[topo_key] = oracle.he_init_weights(TOPOLOGIES[topo_key][0], 0, 0.1)
    return _net_params[topo_key]


def grid_of(c, rows=None, cols=None):
    topo, last = TOPOLOGIES[c.topo]
    return tiling.TileGrid(c.h, c.w, c.rows if rows is None else rows, c.cols if cols is None else cols, topo, last)


def backend_args(c):
    """What OracleTileBackend and HipTileBackend take between `rank` and `step_size`."""
    content, style, init = images(c.h, c.w)
    return content, style, init, WEIGHTS[c.topo], PARAM_SETS[c.params]


# ---------------------------------------------------------------------------------------------------------------- the reference
class SeamTileOracle(OracleTileBackend):
    """OracleTileBackend for ranks that are threads: the oracle's conv layers share module-level scratch arrays, so one network pass
    at a time."""
    net_lock = threading.Lock()

    def forward_partials(self):
        with self.net_lock:
            return super().forward_partials()

    def backward(self):
        with self.net_lock:
            return super().backward()


def oracle_rank(c, grid, rank, operands='fp32', step_size=10):
    return SeamTileOracle(TOPOLOGIES[c.topo][0], net_params(c.topo), grid, rank, *backend_args(c), step_size=step_size, operands=operands)


class WholeReference:
    """The 1 x 1 grid of the whole image.  evaluate(x) -> (scd gradient, combined gradient), both (3, H, W) float32; the first call
    captures the norms, later calls use them."""

    def __init__(self, c, operands='fp32'):
        self.backend = oracle_rank(c, grid_of(c, 1, 1), 0, operands)

    def x(self):
        b = self.backend
        return b.x[b.cur][0].copy()

    def evaluate(self, x=None):
        b = self.backend
        if x is not None:
            b.x[b.cur][0][...] = x
        b.forward_partials()
        b.losses_need_style_norm()
        b.finish_losses()
        scd = b.backward().numpy().copy()
        b.gradient(torch.from_numpy(wrap_ring(b.x[b.cur][0])))
        return scd, b.grad_tile().numpy().copy()


def wrap_ring(x):
    """(3, H + 2, W + 2): the image with its 1-px periodic neighbourhood."""
    return np.pad(x, ((0, 0), (1, 1), (1, 1)), mode='wrap')


# ---------------------------------------------------------------------------------------------------------------- stitching, metric
def stitch(grid, per_rank_tiles):
    """(3, H, W) from the ranks' (3, th, tw) tiles."""
    out = np.full((3, grid.gH, grid.gW), np.nan, F32)
    for t, a in zip(grid.tiles, per_rank_tiles):
        a = np.asarray(a)
        assert a.shape == (3, t.y1 - t.y0, t.x1 - t.x0), (a.shape, t)
        out[:, t.y0:t.y1, t.x0:t.x1] = a
    assert not np.isnan(out).any()
    return out


def tile_part(grid, rank, window_array):
    t, w = grid.tiles[rank], grid.windows[rank]
    return window_array[:, t.y0 - w.y0:t.y1 - w.y0, t.x0 - w.x0:t.x1 - w.x0]


def crop(image, r):
    return image[:, r.y0:r.y1, r.x0:r.x1]


def seam_error(got, want):
    """(max over all pixels of |got - want| / rms(want), (channel, y, x) of the worst one)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), got.shape
    rms = float(np.sqrt(np.mean(want ** 2)))
    assert rms > 0
    d = np.abs(got - want)
    worst = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d[worst]) / rms, tuple(int(v) for v in worst)


def locate(grid, y, x):
    """Where pixel (y, x) lies: its rank, distances, and seam band / torus border / tile interior."""
    rank = next(r for r, t in enumerate(grid.tiles) if t.y0 <= y < t.y1 and t.x0 <= x < t.x1)
    t = grid.tiles[rank]
    to_edge = min(y - t.y0, t.y1 - 1 - y, x - t.x0, t.x1 - 1 - x)
    to_border = min(y, grid.gH - 1 - y, x, grid.gW - 1 - x)
    inner_y = sorted({q.y0 for q in grid.tiles} - {0})
    inner_x = sorted({q.x0 for q in grid.tiles} - {0})
    in_band = any(e - grid.apron <= y < e + grid.apron for e in inner_y) or any(e - grid.apron <= x < e + grid.apron for e in inner_x)
    where = [name for name, on in (('seam band', in_band), ('torus border', to_border == 0)) if on] or ['tile interior']
    return rank, to_edge, to_border, ' + '.join(where)


def hold(grid, got, want, bar, label):
    """Asserts the metric; prints the figure first.  Returns it."""
    err, (ch, y, x) = seam_error(got, want)
    rank, to_edge, to_border, where = locate(grid, y, x)
    line = '[seam] %s: %.3g of the rms (bar %.3g) at channel %d pixel (%d, %d), rank %d, %d px from its tile edge, %d px from the image border, %s' \
        % (label, err, bar, ch, y, x, rank, to_edge, to_border, where)
    print(line)
    assert err <= bar, line + '; got %.9g, want %.9g' % (got[ch, y, x], want[ch, y, x])
    return err


def exact_windows(grid, windows, label):
    """Every rank's whole window equals the crop of the image stitched from the tile parts, bit for bit.  Returns that image."""
    image = stitch(grid, [tile_part(grid, r, w) for r, w in enumerate(windows)])
    for r, w in enumerate(windows):
        want = crop(image, grid.windows[r])
        if not np.array_equal(w, want):
            bad = np.argwhere(w != want)
            raise AssertionError('%s: the window of rank %d differs from the stitched image at %d pixels, first at window (c, y, x) = %s'
                                 % (label, r, len(bad), tuple(bad[0])))
    return image


def exact_rings(grid, image, rings, label):
    """Every rank's gathered ring (border cells) equals the wrap-padded image's, bit for bit."""
    padded = wrap_ring(image)
    for r, (t, ring) in enumerate(zip(grid.tiles, rings)):
        want = padded[:, t.y0:t.y1 + 2, t.x0:t.x1 + 2]
        assert ring.shape == want.shape, (label, r, ring.shape)
        for name, sl in (('top', np.s_[:, 0, :]), ('bottom', np.s_[:, -1, :]), ('left', np.s_[:, :, 0]), ('right', np.s_[:, :, -1])):
            assert np.array_equal(ring[sl], want[sl]), '%s: the %s ring line of rank %d is not the torus neighbour' % (label, name, r)


# ---------------------------------------------------------------------------------------------------------------- drivers
def host(t):
    return t.detach().cpu().numpy().copy()


class RecordingTransfer(tiled.TiledTransfer):
    """tiled.TiledTransfer that keeps per evaluation: the tile part of the window gradient after overlap_add ('scd'), the gathered ring,
    the whole window of x_cur, the combined gradient of the tile ('grad') and the trace.  The driver's own phases run."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.evals, self._rec = [], {}

    def overlap_add(self, g):
        super().overlap_add(g)
        ys, xs = tiled._local(self.tile, self.window)
        self._rec['scd'] = host(g[:, ys, xs])

    def gather_ring(self, x):
        ring = super().gather_ring(x)
        self._rec['ring'], self._rec['window'] = host(ring), host(x)
        return ring

    def _close(self, values, grad):
        self._rec['trace'] = np.asarray(values, np.float64)
        if grad:
            self._rec['grad'] = host(self.backend.grad_tile())
        self.evals.append(self._rec)
        self._rec = {}

    def _evaluate(self):
        values = super()._evaluate()
        self._close(values, True)
        return values

    def step(self):
        values = super().step()
        if self.optimizer == 'adam':        # (the oracle backend keeps the combined gradient of an Adam update too; the engine does not)
            self._close(values, hasattr(self.backend, '_grad_tile'))
        return values

    def window_now(self):
        return host(self.backend.x_cur())


def run_phase_driver(c, grid, backends, optimizer, steps, prepare=None, timeout=120.0):
    """`steps` iterations of RecordingTransfer over `backends` (one per rank), ranks as threads on tiled.InProcessFabric + LocalComm.
    prepare(ranks) may change the drivers before they run.  Returns the drivers."""
    fabric = tiled.InProcessFabric(grid.world, timeout)
    ranks = [RecordingTransfer(grid, r, backends[r], tiled.LocalComm(fabric, r), optimizer=optimizer,
                               step_size={'adam': None, 'lbfgs': 1}[optimizer]) for r in range(grid.world)]
    if prepare:
        prepare(ranks)
    tiled.run_in_process(ranks, steps, fabric)
    return ranks


def check_phase_driver(c, grid, ranks, reference, bar, label, errors=None):
    """Every recorded evaluation of every rank against `reference` (a WholeReference) at the stitched x of that evaluation; windows and
    rings exact; every rank the same trace.  errors: dict that receives the largest figure per tensor."""
    n_evals = len(ranks[0].evals)
    assert n_evals and all(len(tt.evals) == n_evals for tt in ranks)
    for k in range(n_evals):
        ev = [tt.evals[k] for tt in ranks]
        tag = '%s %s evaluation %d' % (c.id, label, k + 1)
        x = exact_windows(grid, [e['window'] for e in ev], tag)
        exact_rings(grid, x, [e['ring'] for e in ev], tag)
        scd_ref, grad_ref = reference.evaluate(x)
        for name, want in (('scd', scd_ref), ('grad', grad_ref)):
            if name in ev[0]:
                err = hold(grid, stitch(grid, [e[name] for e in ev]), want, bar, '%s %s' % (tag, name))
                if errors is not None:
                    errors[name] = max(errors.get(name, 0.0), err)
        for e in ev:
            assert np.array_equal(e['trace'], ev[0]['trace']), tag         # every rank derives the same trace from the reduced sums
    exact_windows(grid, [tt.window_now() for tt in ranks], '%s %s after the last step' % (c.id, label))


# ---------------------------------------------------------------------------------------------------------------- re-cut plans
def _pieces(x, w, halves):
    """(x offset, width) pieces of one row: the row, or its two halves."""
    return [(x, w // 2), (x + w // 2, w - w // 2)] if halves and w >= 2 else [(x, w)]


def recut(plans, halves=False):
    """What tiled.fused_plans returns with every rectangle cut into single-row rectangles, send and receive side alike, same order:
    the same exchange with more than kMaxStripRects rectangles per peer.  halves: every row in two pieces as well, for grids whose
    rectangles have no more than kMaxStripRects rows (tiles of 12 rows)."""
    def rows(rects):
        return [(y + i, px, 1, pw) for y, x, h, w in rects for i in range(h) for px, pw in _pieces(x, w, halves)]
    return {phase: {peer: (rows(send), rows(recv)) for peer, (send, recv) in peers.items()} for phase, peers in plans.items()}


def recut_driver(tt, halves=False):
    """The same for a tiled.TiledTransfer: it executes the plans it holds."""
    tt.plans = recut(tt.plans, halves)


def driver_rects_per_peer(tt):
    """Largest number of rectangles this rank of a tiled.TiledTransfer receives from one peer (not itself) in one phase."""
    return max_rects_per_peer({phase: {peer: ([], recv) for peer, (_, recv) in peers.items() if peer != tt.rank}
                               for phase, peers in tt.plans.items()})


def max_rects_per_peer(plans):
    return max([max(len(send), len(recv)) for peers in plans.values() for send, recv in peers.values()] or [0])
