"""The plain form of the emission pass on the real engine (``pytest -m gpu``): iterate averaging off, original colours off, so every
image handed out is deprocess(x), one fp32 addition per element (csrc/emit.hip: emit_k with the iterate as its source and the channel
mean added).  Held BIT FOR BIT to tests/average_oracle.py's deprocess of get_input_nchw() after every step.

Sizes: 16 x 32 (plane a multiple of 4: the 16-byte path), 18 x 34 (plane a multiple of 4, width not: the 16-byte path across row
ends), 17 x 33 (odd plane: one pixel per thread).  The launch has at most 2048 workgroups of 256 threads: a thread strides on to further
pixels from 2048 * 256 = 524288 pixels on the one-pixel path -- 725 x 725 = 525625, odd, is the smallest square beyond it -- and from
four times as many on the 16-byte path -- 1450 x 1448 = 2099600 (a multiple of 4) against 2097152.  Tiny VGG-shaped net and make() of
tests/test_gpu_iterate_average.py."""
import numpy as np
import pytest

from average_oracle import deprocess
from style_transfer2_amd import tiled, tiling
from style_transfer2_amd.tile_backend import HipTileBackend
from test_gpu_iterate_average import NET, PARAMS, TOPO, WEIGHTS, image, make, same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
SMALL = [(16, 32), (18, 34), (17, 33)]
STRIDING = [(725, 725), (1450, 1448)]


def off_by(a, b):
    return 'largest difference %g' % float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize('h,w', SMALL + STRIDING)
def test_step_hands_out_the_deprocessed_iterate(h, w):
    eng = make(h, w)
    assert eng.iterate_average()[:2] == (0.0, 0) and eng.color_modes()[0] is False
    first = None
    for _ in range(2):
        img, _, loss = eng.step()
        assert np.isfinite(loss)
        want = deprocess(eng.get_input_nchw())
        assert img.dtype == F32 and img.shape == (h, w, 3) and same_bits(img, want), off_by(img, want)
        first = img if first is None else first
    assert not np.array_equal(first, img)                       # (the iterate moved: two different images were checked)
    eng.close()


@pytest.mark.parametrize('h,w', SMALL)
def test_step_begin_and_end_hand_out_the_deprocessed_iterates_at_depth_two(h, w):
    """Two iterations in flight: every begin's iterate is read (st_get_input_nchw waits for the stream) and the image st_step_end hands
    out for it is its deprocess."""
    eng = make(h, w)
    want, got = [], []
    for _ in range(6):
        eng.step_begin()
        want.append(deprocess(eng.get_input_nchw()))
        if eng.steps_pending() == 2:
            got.append(eng.step_end()[0])
    while eng.steps_pending():
        got.append(eng.step_end()[0])
    assert len(got) == 6
    for a, b in zip(got, want):
        assert same_bits(a, b), off_by(a, b)
    eng.close()


def test_every_ranks_tile_is_the_crop_of_its_deprocessed_window():
    """1 x 2 grid over the in-process fabric, 32 x 64, two fused Adam steps: st_tile_get_tile is deprocess of the tile cut from the
    window st_get_input_nchw returns.  Tile planes are multiples of 4 in this topology: the 16-byte path."""
    h, w = 32, 64
    content, style, init = image(1, h, w), image(2, 24, 40), image(3, h, w)
    grid = tiling.TileGrid(h, w, 1, 2, TOPO, len(TOPO))
    fabric = tiled.InProcessFabric(2, timeout=120.0)
    backends = []
    for r in range(2):
        b = HipTileBackend(NET, grid, r, content, style, init, WEIGHTS, PARAMS, step_size=10, topology=TOPO)
        b.comm_init_local(r, 2, fabric)
        backends.append(b)
    ranks = [tiled.FusedTiledTransfer(grid, r, b) for r, b in enumerate(backends)]
    seen = []
    for _ in range(2):
        tiled.run_in_process(ranks, 1, fabric)
        for b, rank in zip(backends, ranks):
            t, win = grid.tiles[b.rank], grid.windows[b.rank]
            assert (t.y1 - t.y0) * (t.x1 - t.x0) % 4 == 0
            x = b.engine.get_input_nchw()[0][:, t.y0 - win.y0:t.y1 - win.y0, t.x0 - win.x0:t.x1 - win.x0]
            got, want = b.tile_image(), deprocess(x)
            assert got.dtype == F32 and same_bits(got, want), (b.rank, off_by(got, want))
            assert same_bits(rank.tile_image(), got)            # what the fused driver hands out
            seen.append(got)
    assert not np.array_equal(seen[0], seen[2])
    for b in backends:
        b.engine.close()
