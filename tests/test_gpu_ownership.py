"""Every device and pinned buffer of the engine is owned by a DevBuf / PinBuf (csrc/devbuf.h) and allocated through one counted funnel.
Each case reads st_live_bytes, creates the engine(s), runs a scenario that makes one group of owners allocate, re-allocate and retire
buffers, checks that both counters moved while the engine lived (a dead counter cannot pass) and that close() brings both back to
the start value EXACTLY.  Other engines of the process may be alive: everything is relative to the start value.

Tiny VGG-shaped nets (oracle.tiny_topology, as helpers.tiny_setup builds them) at 32 x 48; nothing here provokes an allocation
failure -- those paths are tests/devbuf_host_main.cpp's."""
from ctypes import byref, c_longlong

import numpy as np
import pytest

import oracle
from style_transfer2_amd import capi, tiled, tiling
from style_transfer2_amd.engine import OPT_ADAM, OPT_LBFGS, Engine, _ptr
from style_transfer2_amd.tile_backend import HipTileBackend
from style_transfer2_amd.transfer import LOSS_NAMES, SCALAR_LOSS_NAMES, weight_table
from helpers import load, tiny_setup

pytestmark = pytest.mark.gpu
F32 = np.float32
H, W = 32, 48
PARAMS = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
# 64 channels: the widths at which the split-operand kernels, the bf16 style kernels and the fused style term have a build
WIDE = oracle.tiny_topology(widths=(64, 64))
WIDE_AVE = tuple(('pool', l[1], 'ave') if l[0] == 'pool' else l for l in WIDE)
_wide_params = oracle.he_init_weights(WIDE, 3, 0.1)


def image(seed, h=H, w=W):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def live():
    dev, pin = c_longlong(-1), c_longlong(-1)
    capi.check(capi.load_library().st_live_bytes(byref(dev), byref(pin)))
    return dev.value, pin.value


def tiny():
    topo, params, weights, _, _, _ = tiny_setup(load('transfer_tiny.npz'))
    return topo, params, weights


def set_weights(eng, weights):
    rows, cells = weight_table(weights)
    cols = [[cells[k][r] for r in rows] for k in LOSS_NAMES]
    eng.set_weights(rows, cols[0], cols[1], cols[2], [PARAMS[k] for k in SCALAR_LOSS_NAMES])


def make(topo, params, weights, precision='fp32', kind=OPT_ADAM, step=10, style_hw=(24, 40)):
    eng = Engine(topo, 0, precision)
    eng.load_weights(params)
    eng.set_input(image(3))
    eng.set_content(image(1))
    eng.set_style(image(2, *style_hw))        # another size than the input: the style forward has an activation set of its own
    set_weights(eng, weights)
    eng.optimizer_reset(kind, step)
    return eng


def alive(start):
    """Both counters are above the start value: the engine holds device AND pinned memory, and the funnel counts it."""
    now = live()
    assert now[0] > start[0] and now[1] > start[1], (start, now)
    return now


def test_pipelined_adam_with_frame_room_a_larger_input_and_retired_pinned_slots():
    start = live()
    topo, params, weights = tiny()
    eng = make(topo, params, weights)
    eng.set_frame_room(64, 32)

    def run(n):
        for k in range(n):                    # one begin ahead of every end, as the worker loop runs it
            eng.step_begin()
            if k:
                assert np.isfinite(eng.step_end(copy=False)[2])
        assert np.isfinite(eng.step_end()[2]) and eng.steps_pending() == 0
    run(6)
    first = alive(start)
    eng.set_input(image(4, 40, 56))
    eng.set_content(image(5, 40, 56))
    eng.set_frame_room(5000, 100)             # the slots of the first six steps are retired, not freed: their views stay valid
    run(4)
    grown = alive(start)
    assert grown[1] > first[1], (first, grown)         # larger slots AND the retired ones
    eng.close()
    assert live() == start


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_lbfgs_both_forms_the_model_hooks_and_resampling(precision):
    """fp32: the chain form; bf16: the Gram form (engine_step.cpp decides by the precision)."""
    start = live()
    topo, params, weights = tiny()
    eng = make(topo, params, weights, precision=precision, kind=OPT_LBFGS, step=1)
    for _ in range(5):
        assert np.isfinite(eng.step()[2])
    alive(start)
    x = np.random.RandomState(6).randn(1, 3, H, W).astype(F32)
    eng.forward(x)                            # the probe image's own buffer; every blob
    last = topo[-1][1]
    blob = eng.get_blob(last)
    grad = eng.backward({last: np.ones_like(blob), 'conv1_1': np.ones_like(eng.get_blob('conv1_1'))})
    assert np.isfinite(blob).all() and np.isfinite(grad).all() and np.isfinite(eng.gram(last)).all()
    eng.forward(np.zeros((1, 3, 20, 28), F32))         # a forward at another geometry re-creates the size-dependent buffers
    eng.set_input(image(3))
    eng.resample_state((24, 40))
    eng.resample_content((24, 40))
    assert eng.input_shape() == (24, 40) and eng.content_shape() == (24, 40)
    assert np.isfinite(eng.step()[2])
    alive(start)
    eng.close()
    assert live() == start


def test_conv_and_gram_algorithms_set_before_and_after_the_weights_and_a_layer_loaded_twice():
    start = live()
    weights = {'content': {'conv2_1': 0.08}, 'style': {'conv1_1': 1, 'conv1_2': 1}, 'deepdream': {}}
    eng = Engine(WIDE, 0, 'fp32')
    eng.set_conv_algo(2)                      # before the weights: load_weights makes the split packs
    eng.set_gram_algo(1)
    eng.load_weights(_wide_params)
    assert eng.algos() == (2, 1)
    loaded = alive(start)
    w, b = (np.ascontiguousarray(a, F32) for a in _wide_params['conv1_2'])
    capi.check(eng.lib.st_load_conv_weights(eng._ctx, b'conv1_2', _ptr(w), _ptr(b)))
    assert live() == loaded                   # a reload replaces every pack of the layer by one of the same size
    eng.set_conv_algo(1)
    eng.set_conv_algo(2)                      # after the weights: the packs exist already, nothing is made twice
    eng.set_gram_algo(0)
    eng.set_gram_algo(1)
    assert live() == loaded
    eng.set_input(image(3)); eng.set_content(image(1)); eng.set_style(image(2))
    set_weights(eng, weights)
    eng.optimizer_reset(OPT_ADAM, 10)
    for _ in range(3):
        assert np.isfinite(eng.step()[2])
    alive(start)
    eng.close()
    assert live() == start
    # ... and the other order: plain packs first, the split packs from the device copy of the weights
    eng = Engine(WIDE, 0, 'fp32')
    eng.load_weights(_wide_params)
    plain = alive(start)
    eng.set_conv_algo(2)
    eng.set_gram_algo(1)
    assert live() == loaded and loaded[0] > plain[0]
    eng.close()
    assert live() == start


def test_bf16_lean_flow_with_fused_average_pool_fused_style_term_and_dropped_content_features(monkeypatch):
    monkeypatch.setenv('ST2_CONV16_CFG', '0')           # the 64 x 256 tile, which has the pooling builds (the default takes it from 128 x 1024 on)
    start = live()
    weights = {'content': {'pool1': 0.1, 'conv2_1': 0.1}, 'style': {'conv1_1': 1}, 'deepdream': {}}
    eng = make(WIDE_AVE, _wide_params, weights, precision='bf16', style_hw=(H, W))
    eng.set_pool_algo(1)
    eng.profile_enable(True)
    for _ in range(3):
        assert np.isfinite(eng.step()[2])
    prof = eng.profile_read()
    eng.profile_enable(False)
    # the scenario made what it is about: the style term rode on a data-gradient conv (its operand pack, the sign maps) and the
    # average pool on the convs around it (its map buffer)
    assert prof['style_grad_fused_in_conv_dgrad_bf16']['launches'] > 0, sorted(prof)
    assert 'avepool_fwd' not in prof and 'avepool_bwd' not in prof, sorted(prof)
    full = alive(start)
    set_weights(eng, {'content': {'conv2_1': 0.1}, 'style': weights['style'], 'deepdream': {}})
    dropped = alive(start)
    assert dropped[0] < full[0]               # the content features of pool1 went
    assert np.isfinite(eng.step()[2])
    set_weights(eng, weights)
    assert np.isfinite(eng.step()[2])         # ... and came back from the kept content image
    assert alive(start)[0] >= full[0]
    eng.close()
    assert live() == start


def test_tile_sharded_adam_and_lbfgs_with_the_sharded_style_pass():
    start = live()
    topo, params, _ = tiny()
    weights = {'content': {'conv2_1': 0.08}, 'style': {'conv1_1': 1, 'conv2_2': 1}, 'deepdream': {}}
    content, style, init = image(1), image(2, 24, 40), image(3)
    last = len(topo)
    grid = tiling.TileGrid(H, W, 1, 2, topo, last)
    sgrid = tiling.TileGrid(24, 40, 1, 2, topo, last)
    fabric = tiled.InProcessFabric(2, timeout=120.0)
    backends = []
    for r in range(2):
        b = HipTileBackend(params, grid, r, content, None, init, weights, PARAMS, step_size=10, topology=topo)
        b.comm_init_local(r, 2, fabric)
        backends.append(b)
    tiled.run_collective([lambda b=b: b.shard_style(style, sgrid) for b in backends], fabric)
    ranks = [tiled.FusedTiledTransfer(grid, r, b) for r, b in enumerate(backends)]
    out = tiled.run_in_process(ranks, 2, fabric)
    assert all(np.isfinite(o[-1][-2]) for o in out)
    adam = alive(start)
    for b in backends:
        b.engine.optimizer_reset(OPT_LBFGS, 1)
    out = tiled.run_in_process(ranks, 1, fabric)
    assert all(np.isfinite(o[-1][-2]) for o in out)
    assert backends[0].tile_image().shape == (H, W // 2, 3)
    assert alive(start)[0] > adam[0]          # the L-BFGS vectors and the tile's compact copies
    backends[0].engine.close()
    alive(start)                              # rank 1 still holds its share
    backends[1].engine.close()
    assert live() == start


def test_close_twice_is_a_no_op():
    start = live()
    topo, params, weights = tiny()
    eng = make(topo, params, weights)
    assert np.isfinite(eng.step()[2])
    alive(start)
    eng.close()
    assert live() == start
    eng.close()
    assert live() == start
