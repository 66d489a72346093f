"""The style targets of a tile-sharded job, sharded as well -- on the engine (``pytest -m gpu``): st_tile_set_style /
st_tile_style_partials / st_tile_style_commit / st_get_style_gram against the CPU oracle's whole-image Grams.  Ranks are engine
contexts of this process on the one GPU, one thread each, over tiled.InProcessFabric (as the tile tests of test_gpu_parity.py)."""
import ctypes
import os

import numpy as np
import pytest

import oracle
import style_transfer2_amd as st2
from style_transfer2_amd import capi, jobs, tiled, tiling
from style_transfer2_amd.capi import StError
from style_transfer2_amd.engine import Engine
from style_transfer2_amd.tile_backend import HipTileBackend
from helpers import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
F32 = np.float32
# every C-tile shape of the region Gram kernel: 3 (the image), 64, 128, 200 (ragged 128-tiles), 512 (mirrored upper-triangular tiles);
# two pools: stride 4, apron 8 at the last blob
TOPO = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 128), ('pool', 'pool1'), ('conv', 'conv2_1', 128, 200), ('pool', 'pool2'),
        ('conv', 'conv3_1', 200, 512))
NAMES = ['data'] + [layer[1] for layer in TOPO]
LAST = len(TOPO)
WEIGHTS = {'content': {'conv2_1': 0.08}, 'style': {'conv1_1': 1, 'conv3_1': 1}, 'deepdream': {}}
PARAMS = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
GRAM_BAR = 1e-5                     # rel-L2 against oracle.gram of the whole forward: the bar of test_gram_matches_oracle

_net_params = oracle.he_init_weights(TOPO, 7, 0.1)
_refs = {}


def style_image(hw):
    return np.random.RandomState(hw[0] * 1000 + hw[1]).randint(0, 256, (hw[0], hw[1], 3)).astype(np.uint8)


def reference(hw, operands='fp32'):
    """{blob: oracle.gram of the whole-image forward}, computed once per shape and never modified."""
    key = (hw, operands)
    if key not in _refs:
        net = oracle.NetOracle(TOPO, _net_params, operands=operands)
        _refs[key] = {k: oracle.gram(v) for k, v in net.forward(net.preprocess(style_image(hw))).items()}
    return _refs[key]


def make_ranks(world, precision='fp32', weights=WEIGHTS):
    """`world` tile backends WITHOUT style targets on a 1 x world content grid of a small image, joined by an InProcessFabric."""
    h, w = 32, 16 * max(world, 2)
    rs = np.random.RandomState
    content, init = rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8)
    grid = tiling.TileGrid(h, w, 1, world, TOPO, 4)
    fabric = tiled.InProcessFabric(world, timeout=120.0)
    backends = []
    for r in range(world):
        b = HipTileBackend(_net_params, grid, r, content, None, init, weights, PARAMS, step_size=10, topology=TOPO, precision=precision)
        if world == 1:
            b.comm_init_solo(0, 1)
        else:
            b.comm_init_local(r, world, fabric)
        backends.append(b)
    return grid, fabric, backends


def shard(backends, fabric, style, sgrid):
    tiled.run_collective([lambda b=b: b.shard_style(style, sgrid) for b in backends], fabric)


def check_targets(backends, ref, bar, names=NAMES):
    worst = 0.0
    for name in names:
        g0 = backends[0].engine.style_gram(name)
        err = rel_l2(g0, ref[name])
        worst = max(worst, err)
        print('[sharded style] %-8s rel-L2 %.3g (bar %.3g)' % (name, err, bar))
        assert err <= bar, (name, err)
        for r, b in enumerate(backends[1:], start=1):
            assert np.array_equal(b.engine.style_gram(name), g0), (name, r)       # one reduced buffer, one division: bit for bit
    return worst


# 37 x 50: clipped ceil-mode pooling windows at the far edges (37 -> 19 -> 10, 50 -> 25 -> 13), ragged 200-channel tiles, the 3-channel
# blob; 16 x 40 over eight ranks: tiling.style_grid cuts five tiles, ranks 5 .. 7 contribute zeros
@pytest.mark.parametrize('hw,cut,world', [((64, 96), (1, 2), 2), ((64, 96), (2, 2), 4), ((37, 50), (2, 2), 4), ((16, 40), None, 8)])
def test_sharded_style_targets_match_the_whole_image_oracle_on_every_rank(hw, cut, world):
    style = style_image(hw)
    sgrid = tiling.TileGrid(hw[0], hw[1], cut[0], cut[1], TOPO, LAST) if cut else tiling.style_grid(hw[0], hw[1], world, TOPO, LAST)
    if cut is None:
        assert sgrid.world < world                           # some ranks have no tile
    assert sgrid.stride == 4 and sgrid.apron == 8
    grid, fabric, backends = make_ranks(world)
    shard(backends, fabric, style, sgrid)
    assert fabric.reduces == 1
    check_targets(backends, reference(hw), GRAM_BAR)
    # ... and the job runs on them: one fused iteration, finite, the same trace on every rank
    ranks = [tiled.FusedTiledTransfer(grid, r, b) for r, b in enumerate(backends)]
    out = tiled.run_in_process(ranks, 1, fabric)
    assert np.isfinite(out[0][0][-2]) and all(np.array_equal(np.asarray(o[0]), np.asarray(out[0][0])) for o in out)


def _solo_callbacks(engine):
    engine._cb = (capi.ALLREDUCE_FN(lambda user, ptr, n: 0), capi.EXCHANGE_FN(lambda *a: 0))
    capi.check(engine.lib.st_comm_callbacks(engine._ctx, 0, 1, engine._cb[0], engine._cb[1], None))


def _engine(precision='fp32'):
    e = Engine(TOPO, 0, precision)
    e.load_weights(_net_params)
    return e


@pytest.mark.parametrize('rccl', [False, True])
def test_one_rank_whose_window_is_the_image_meets_the_same_bar(rccl):
    """World 1: the tile is the image, the all-reduce sees one rank -- over the caller's transport, and over a REAL RCCL communicator
    of one rank (ncclAllReduce on the partials' buffer, on the engine's stream)."""
    hw = (37, 50)
    style = style_image(hw)
    e = _engine()
    if rccl:
        uid = ctypes.create_string_buffer(capi.COMM_ID_BYTES)
        capi.check(e.lib.st_comm_unique_id(uid))
        capi.check(e.lib.st_comm_init(e._ctx, uid.raw, 0, 1))
    else:
        _solo_callbacks(e)
    e.tile_set_style(style, hw)
    ref = reference(hw)
    for name in NAMES:
        err = rel_l2(e.style_gram(name), ref[name])
        assert err <= GRAM_BAR, (name, err)
    # the two-call form leaves the same targets
    ptr, n = e.tile_style_partials(style, hw, last='pool1')
    assert n == 3 * 3 + 64 * 64 + 128 * 128 + 128 * 128 and ptr
    e.tile_style_commit()
    assert rel_l2(e.style_gram('pool1'), ref['pool1']) <= GRAM_BAR
    if rccl:
        capi.check(e.lib.st_comm_destroy(e._ctx))


# bf16 operands.  The targets are the fp32 region Gram of the fp32 blobs the bf16 convs wrote, as st_set_style's are; the reference is
# the oracle with operands='bf16' (bf16-rounded conv operands, fp32 accumulation).  The bar is what st_set_style on ONE context under
# bf16 differs from that oracle by, times 2: a window's convs split K by its own size, so the sharded features are a second, equally
# valid bf16-operand evaluation.  Measured on MI355X per blob (data, conv1_1, conv1_2, pool1, conv2_1, pool2, conv3_1), worst blob:
BF16_SET_STYLE_MEASURED = {(64, 96): 1.227e-5, (37, 50): 4.412e-5}      # (conv3_1 both times; data .. pool1 stay below 1e-6)
BF16_BAR = {hw: 2 * v for hw, v in BF16_SET_STYLE_MEASURED.items()}        # 2.454e-5 and 8.824e-5


@pytest.mark.parametrize('hw,cut,world', [((64, 96), (1, 2), 2), ((37, 50), (2, 2), 4)])
def test_sharded_style_targets_under_bf16_operands(hw, cut, world):
    style = style_image(hw)
    ref = reference(hw, 'bf16')
    whole = _engine('bf16')
    whole.set_style(style)
    measured = max(rel_l2(whole.style_gram(name), ref[name]) for name in NAMES)
    print('[sharded style, bf16] st_set_style on one context against the bf16-operand oracle at %s: worst rel-L2 %.3g' % (hw, measured))
    sgrid = tiling.TileGrid(hw[0], hw[1], cut[0], cut[1], TOPO, LAST)
    grid, fabric, backends = make_ranks(world, precision='bf16')
    shard(backends, fabric, style, sgrid)
    for name in NAMES:
        print('[sharded style, bf16] %-8s sharded rel-L2 %.3g, st_set_style %.3g' % (
            name, rel_l2(backends[0].engine.style_gram(name), ref[name]), rel_l2(whole.style_gram(name), ref[name])))
    check_targets(backends, ref, BF16_BAR[hw])


def test_the_style_pass_of_a_rank_forwards_its_window_not_the_image():
    """Profiler: the conv FLOPs a rank reports for the style pass are the formula for ITS window (exactly), not the whole image's."""
    hw = (64, 96)
    style = style_image(hw)
    sgrid = tiling.TileGrid(hw[0], hw[1], 1, 2, TOPO, LAST)
    grid, fabric, backends = make_ranks(2)
    for b in backends:
        b.engine.profile_enable(True)
    shard(backends, fabric, style, sgrid)

    def conv_flops(h, w):
        return sum(2.0 * 9 * layer[2] * layer[3] * gh * gw
                   for layer, (_, gh, gw, _) in zip(TOPO, tiling.blob_geometry(TOPO, h, w)[1:]) if layer[0] == 'conv')
    for r, b in enumerate(backends):
        prof = b.engine.profile_read()
        got = sum(v['flops'] for k, v in prof.items() if k.startswith('conv3x3_fwd'))
        win = sgrid.windows[r]
        assert (win.y1 - win.y0, win.x1 - win.x0) == (64, 56)
        assert got == conv_flops(64, 56) and got < conv_flops(64, 96), (r, got)
        assert prof['gram_partial_mfma_f32']['launches'] == LAST + 1 and 'gram_partial_split_bf16x6' not in prof


def test_refusals():
    hw = (64, 96)
    style = style_image(hw)
    lib = capi.load_library()
    # before a communicator exists
    e = _engine()
    with pytest.raises(StError, match='st2 error 2.*st_comm_init'):
        e.tile_set_style(style, hw)
    with pytest.raises(StError, match='st2 error 2'):
        e.tile_style_commit()                                  # no partials
    with pytest.raises(StError, match='st2 error 2.*no style target'):
        e.style_gram('data')
    _solo_callbacks(e)
    # bad geometry: ST_ERR_ARG, nothing launched
    half = np.ascontiguousarray(style[:, :56])
    for kw, what in ((dict(window=(0, 48), tile=(0, 48, 64, 96)), 'window beyond the image'),
                     (dict(window=(0, 0), tile=(0, 0, 64, 60)), 'tile beyond the window'),
                     (dict(window=(0, 0), tile=(0, 8, 64, 8)), 'empty tile'),
                     (dict(window=(0, 0), tile=(0, 0, 64, 46)), 'inner edge off the stride'),
                     (dict(window=(0, 2), tile=(0, 4, 64, 48)), 'window origin off the stride'),
                     (dict(window=(0, 0), tile=(0, 0, 64, 48), last=LAST + 1), 'no such blob'),
                     (dict(window=(0, 0), tile=(0, 0, 64, 48), last=-1), 'no such blob')):
        with pytest.raises(StError, match='st2 error 1'):
            e.tile_set_style(half, hw, **kw)
    with pytest.raises(StError, match='st2 error 2'):
        e.style_gram('data')                                   # the refused calls left no target behind
    assert lib.st_tile_set_style(None, None, *([0] * 12)) == 1 and lib.st_tile_style_commit(None) == 1
    assert lib.st_get_style_gram(None, 0, None) == 1
    # targets up to conv2_1 only: the blobs above are absent, for the hook and for every evaluation that weights them
    grid, fabric, backends = make_ranks(1)
    b = backends[0]
    b.shard_style(style, tiling.TileGrid(hw[0], hw[1], 1, 1, TOPO, 4))
    assert b.engine.style_gram('conv2_1').shape == (200, 200)
    with pytest.raises(StError, match='st2 error 2.*conv3_1'):
        b.engine.style_gram('conv3_1')
    with pytest.raises(StError, match='st2 error 2.*conv3_1'):
        tiled.FusedTiledTransfer(grid, 0, b).step()            # tiled evaluation: WEIGHTS put a style weight on conv3_1
    with pytest.raises(StError, match='st2 error 2.*conv3_1'):
        b.engine.opfunc()                                      # whole-image evaluation of the same context
    b.shard_style(style, tiling.TileGrid(hw[0], hw[1], 1, 1, TOPO, LAST))
    assert np.isfinite(tiled.FusedTiledTransfer(grid, 0, b).step()[-2])
    # st_set_style gives every blob a target again
    b.engine.set_style(style)
    assert b.engine.style_gram('conv3_1').shape == (512, 512)


def test_run_tiled_job_with_a_sharded_style_pass_equals_run_job():
    """jobs.run_tiled_job(shard_style=True): the example pair at 256 px cut 2 x 2, the style image cut over the same four ranks,
    against jobs.run_job on the whole image: ten Adam iterations, at the bar of test_run_tiled_job_on_one_gpu_equals_run_job."""
    from PIL import Image
    src = np.load(os.path.join(GOLDEN, 'config1_sources.npz'))
    content, style = Image.fromarray(src['golden_gate']), Image.fromarray(src['starry_night'])
    params = oracle.he_init_weights(oracle.VGG19_TOPOLOGY, seed=0)
    whole = jobs.run_job(st2.StyleTransfer(st2.HipModel(params)), content, style, 10, size=256, optimizer='adam', seed=5)
    tiles = jobs.run_tiled_job(params, content, style, 10, (2, 2), size=256, seed=5, shard_style=True)
    mse = float(np.mean((tiles.astype(np.float64) - whole) ** 2))
    print('[tiled job 2x2 at 192x256, sharded style pass] image MSE %.3g against the whole-image job after 10 Adam iterations' % mse)
    assert tiles.shape == whole.shape == (192, 256, 3) and mse <= 0.05
