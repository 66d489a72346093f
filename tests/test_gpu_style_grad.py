"""The style gradient S = c2 * D @ F of every kernel family, element by element against float64 on the operands the launch itself read,
and the content / deep-dream diffs of layer_elem_k bit for bit -- through st_get_layer_terms, the hook that hands out what the last
evaluation left in the engine's own buffers.  The bars are derived in tests/style_grad_oracle.py (and shown reachable, and sharp
against seeded defects, on the CPU in tests/test_style_grad_oracle_cpu.py); nothing here is fitted to what a kernel returns.

The style term that rides on the bf16 data-gradient conv (ST2_STYLE_FUSE) never materialises S: tests/test_gpu_fused_style.py holds it
to float64 through the diff tap.  ST2_STYLE_GRAD_REPORT=<file> appends the measured figures of every case to that file (the
record profiles/style_grad_errors.txt was made this way); they are records, not bars."""
import os
from ctypes import byref, c_float, c_int, c_void_p

import numpy as np
import pytest

import oracle
import style_transfer2_amd as st2
from oracle.caffe_net import bf16_round
from style_transfer2_amd.capi import StError, check

import style_grad_oracle as so

pytestmark = pytest.mark.gpu
F32 = np.float32
RS = np.random.RandomState
PARAMS4 = (5, 2, 50, 6)                                 # tv, tv_power, p, p_power
STYLE_HW = (13, 17)                                     # the style image: the target comes from another size
CLASS = {'fp32': 'style_grad_mfma_f32', 'split': 'style_grad_split_bf16x6', 'bf16': 'style_grad_mfma_bf16'}
TRACE_RTOL = 2e-4                                       # the suite's trace tolerance (check_trace)
# (h, w) of the blob: smallest blobs; hw odd (_w builds, unaligned split / bf16 paths); one 4 x 32 pixel tile; ragged both ways;
# W % 4 == 0 with a ragged 32-column tile (_q builds); whole tiles; several tiles with W % 4 != 0; two whole 128-pixel groups of
# style16; a ragged last group.  Grouped so that one pytest case stays at a few seconds.
SHAPE_GROUPS = (((1, 1), (1, 4), (5, 7), (4, 32), (5, 33), (12, 36)), ((8, 64), (2, 128)), ((9, 70), (3, 130)))
# (family, variant, environment, C)
CASES = ([('fp32', 'default', {}, c) for c in (48, 64, 128, 200, 512)] +
         [('fp32', 'tile128', {'ST2_STYLE_SMALL': '0'}, c) for c in (128, 200, 512)] +
         [('fp32', 'big', {'ST2_STYLE_FORCE_BIG': '1'}, c) for c in (48, 64, 128, 200, 512)] +
         [('split', 'default', {}, c) for c in (64, 128, 192, 200, 512)] +
         [('bf16', 'default', {'ST2_BF16_LEAN': '0'}, c) for c in (64, 128, 192, 512)])
SWITCHES = ('ST2_STYLE_SMALL', 'ST2_STYLE_FORCE_BIG', 'ST2_BF16_LEAN', 'ST2_TILE_STYLE16', 'ST2_STYLE_FUSE')


# ------------------------------------------------------------------------------------------ mirrors of the launch decisions
def style_tile(C, H, W, small_off=False):
    """conv3x3_mfma.hip's style_tile: (channels, pixel rows) of the fp32 style-gradient tile."""
    if C <= 64:
        return 64, 8
    mpad = -(-C // 64) * 64
    blocks = -(-W // 32) * -(-H // 4) * (mpad // 128)
    return (64 if blocks < 256 and mpad % 64 == 0 and not small_off else 128), 4


def kernel_family(family, C):
    """The family that must run: the split kernels take C % 64 == 0 from 128 up, every other shape keeps the fp32 kernels."""
    return 'fp32' if family == 'split' and not (C >= 128 and C % 64 == 0) else family


# ------------------------------------------------------------------------------------------ jobs
def two_conv(C):
    return (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, C))


def make_engine(topo, family):
    eng = st2.Engine(topo, precision='bf16' if family == 'bf16' else 'fp32')
    eng.load_weights(oracle.he_init_weights(topo, seed=1, bias_std=0.1))
    if family == 'split':
        eng.set_gram_algo(1)
    eng.set_style(RS(2).randint(0, 256, STYLE_HW + (3,)).astype(np.uint8))
    eng.profile_enable(True)
    return eng


def set_images(eng, h, w):
    eng.set_input(RS(3000 + 131 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8))
    eng.set_content(RS(1000 + 131 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8))
    eng.clear_norms()


def second_point(eng, h, w):
    """x + 2 sign(noise): the evaluation point of the steady state."""
    x = eng.get_input_nchw()
    eng.set_input_nchw(x + F32(2) * np.sign(RS(7 + h * w).randn(*x.shape)).astype(F32))


def weights(eng, layer, cw=0.0, sw=0.0, dw=0.0):
    eng.set_weights([layer], [cw], [sw], [dw], PARAMS4)


def evaluate(eng):
    eng.opfunc(return_grad=False)


def tile_evaluate(eng, first):
    """The phases of one tile-sharded evaluation up to the injected diffs, in order and without an all-reduce (one rank: its local
    sums are a valid D and a valid norm)."""
    p, n = c_void_p(), c_int()
    check(eng.lib.st_tile_forward(eng._ctx, byref(p), byref(n)))
    check(eng.lib.st_tile_losses(eng._ctx, byref(p), byref(n)))
    assert (n.value > 0) == first
    if first:
        check(eng.lib.st_tile_style_raw(eng._ctx))
    check(eng.lib.st_tile_losses_finish(eng._ctx))
    eng._fwd_hw = eng.input_shape()


def blob_of(eng, layer, family):
    """(C, h, w) operand F of the style gradient: the fp32 blob, or -- bf16 family -- the bf16 copy the kernel read (the forward rounds
    the fp32 accumulator once to each; ST2_BF16_LEAN=0 keeps the fp32 blob)."""
    f = eng.get_blob(layer)[0]
    return bf16_round(f) if family == 'bf16' else f


def report(*row):
    path = os.environ.get('ST2_STYLE_GRAD_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(' '.join(str(v) for v in row) + '\n')


_emulations = {}


def emulation(key, family, D, F, c2):
    """The CPU emulation of one (case, shape): computed once, shared by the runs with and without a content term (the style term of
    the first evaluation does not depend on it) and never modified."""
    if key not in _emulations:
        e = so.EMULATE[family](D, F, c2)
        e.setflags(write=False)
        _emulations[key] = (e, D.copy(), F.copy())
    e, D0, F0 = _emulations[key]
    assert np.array_equal(D0, D) and np.array_equal(F0, F), 'the style term of the first evaluation changed with the content weight'
    return e


class Figures:
    def __init__(self):
        self.raw = self.scaled = self.l2 = self.l2_emu = 0.0

    def row(self):
        return '%.3f %.3f %.3g %.3g' % (self.raw, self.scaled, self.l2, self.l2_emu)


def check_style_term(eng, layer, family, C, region, n_global, sw, with_content, fig, key, evaluate_fn, second_fn):
    """Both evaluations of one (shape, content weight): see the module docstring of tests/style_grad_oracle.py for the bars.
    region = (y0, x0, y1, x1) of the blob that the launch covers (None: the whole blob); outside it the diff must be exactly +0.0."""
    cw = 0.5 if with_content else 0.0
    c2 = so.c2_of(C, n_global)

    def inside(a):
        a = a.reshape(C, *a.shape[-2:])
        return (a if region is None else a[:, region[0]:region[2], region[1]:region[3]]).reshape(C, -1)

    def outside_is_zero(diff):
        if region is None:
            return
        mask = np.ones(diff.shape[-2:], bool)
        mask[region[0]:region[2], region[1]:region[3]] = False
        out = diff.reshape(C, *diff.shape[-2:])[:, mask]
        assert not np.any(out) and not np.any(np.signbit(out)), 'the diff outside the region is not +0.0'

    def base_term(first):
        """The content part of the diff as bits from the device: the same evaluation with the style weight zero (layer_elem_k is
        element-wise and deterministic; the content norm is already captured)."""
        if not with_content:
            return None
        weights(eng, layer, cw=cw)
        evaluate_fn(False)
        b = eng.layer_terms(layer, want=('diff',))['diff']
        weights(eng, layer, cw=cw, sw=sw)
        return b

    # ---- first evaluation: S unscaled, the norm from it, then coef * S (+ b)
    weights(eng, layer, cw=cw, sw=sw)
    evaluate_fn(True)
    F = inside(blob_of(eng, layer, family))
    t = eng.layer_terms(layer)
    D, norms = t['D'], t['norms']
    S_ref, B = so.reference(D, F, c2)
    raw = inside(t['raw_S'])
    r = so.worst_ratio(raw, S_ref, so.bar(family, C) * B)
    print('%s first: worst |S - S_ref| / (bar B) = %.3g' % (key, r))
    fig.raw = max(fig.raw, r)
    assert r <= 1.0, (key, r)
    emu = emulation(key, family, D, F, c2)
    ok, agg = so.aggregate_ok(family, raw, S_ref, emu, D, F, c2)
    print('%s first: rel-L2 %.3g, emulation %.3g%s' % (key, agg['rel_l2'], agg['rel_l2_emulation'],
                                                       ''.join(' %s %.3g' % kv for kv in agg.get('presence', {}).items())))
    fig.l2, fig.l2_emu = max(fig.l2, agg['rel_l2']), max(fig.l2_emu, agg['rel_l2_emulation'])
    assert ok, (key, agg)
    want_norm = np.sqrt(np.sum(raw.astype(np.float64) ** 2) / n_global)
    assert np.isclose(norms[1], want_norm, rtol=TRACE_RTOL, atol=0), (key, norms, want_norm)
    assert (norms[0] > 0) == with_content and norms[2] == 0
    coef = F32(sw) / norms[1]                            # one IEEE float32 division, as the kernels form it
    b = base_term(True)
    diff = t['diff']
    outside_is_zero(diff)
    if region is None:
        # scaled_accumulate_k: coef * S + base with one rounding each (passes.hip is built without contraction): exact bits
        want = (coef * t['raw_S']).astype(F32) + (b if b is not None else F32(0))
        assert np.array_equal(diff, want), (key, 'scaled_accumulate')
    else:
        # tile-sharded: the norm is known before the diffs are made, so the first evaluation runs the fused epilogue too
        bi = None if b is None else inside(b)
        want = float(coef) * S_ref + (0.0 if bi is None else bi.astype(np.float64))
        r = so.worst_ratio(inside(diff), want, so.scaled_bound(family, C, coef, S_ref, B, bi))
        fig.scaled = max(fig.scaled, r)
        assert r <= 1.0, (key, 'first, fused epilogue', r)

    # ---- second evaluation, elsewhere: the fused epilogue dst = coef * S (+ b)
    second_fn()
    evaluate_fn(False)
    F = inside(blob_of(eng, layer, family))
    t = eng.layer_terms(layer, want=('D', 'diff', 'norms'))
    assert np.array_equal(t['norms'], norms), 'the norms moved after their capture'
    with pytest.raises(StError, match='unscaled'):
        eng.layer_terms(layer, want=('raw_S',))
    S_ref, B = so.reference(t['D'], F, c2)
    b = base_term(False)
    bi = None if b is None else inside(b)
    outside_is_zero(t['diff'])
    want = float(coef) * S_ref + (0.0 if bi is None else bi.astype(np.float64))
    r = so.worst_ratio(inside(t['diff']), want, so.scaled_bound(family, C, coef, S_ref, B, bi))
    print('%s second: worst |diff - (coef S_ref + b)| / bound = %.3g' % (key, r))
    fig.scaled = max(fig.scaled, r)
    assert r <= 1.0, (key, 'second', r)


# ------------------------------------------------------------------------------------------ whole blobs, every family
def case_shapes(variant, group):
    """ST2_STYLE_FORCE_BIG takes the shapes with hw % 4 == 0 only."""
    return [s for s in SHAPE_GROUPS[group] if variant != 'big' or (s[0] * s[1]) % 4 == 0]


GROUPED = [(f, v, env, c, g) for f, v, env, c in CASES for g in range(len(SHAPE_GROUPS)) if case_shapes(v, g)]


@pytest.mark.parametrize('family,variant,env,C,group', GROUPED, ids=['%s-%s-%d-g%d' % (f, v, c, g) for f, v, _, c, g in GROUPED])
def test_style_gradient_per_element_against_float64(family, variant, env, C, group, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    shapes = case_shapes(variant, group)
    ran = kernel_family(family, C)
    eng = make_engine(two_conv(C), family)
    eng.profile_read()
    fig, evaluations = Figures(), 0
    for h, w in shapes:
        # the case is what its name says: the tile the fp32 launch must choose here (a changed threshold cannot empty a case silently)
        if family == 'fp32' and variant != 'big':
            want_tile = (64, 8) if C <= 64 else ((128, 4) if variant == 'tile128' else (64, 4))
            assert style_tile(C, h, w, small_off=variant == 'tile128') == want_tile, (C, h, w)
        for with_content in (False, True):
            set_images(eng, h, w)
            check_style_term(eng, 'conv1_2', ran, C, None, C * h * w, 1.0, with_content, fig,
                             (family, variant, C, h, w), lambda first: evaluate(eng), lambda: second_point(eng, h, w))
            evaluations += 2
    n = {k: v['launches'] for k, v in eng.profile_read().items() if k.startswith('style_grad')}
    assert n == {CLASS[ran]: evaluations}, n
    report(family, variant, C, 'group%d' % group, fig.row())
    eng.close()


def test_d_is_one_float32_subtraction_of_the_two_grams():
    eng = make_engine(two_conv(128), 'fp32')
    set_images(eng, 9, 70)
    weights(eng, 'conv1_2', sw=1.0)
    evaluate(eng)
    D = eng.layer_terms('conv1_2', want=('D',))['D']
    assert np.array_equal(D, eng.gram('conv1_2') - eng.style_gram('conv1_2'))
    eng.close()


# ------------------------------------------------------------------------------------------ regions (tile-sharded mode)
WINDOW = (20, 45)
TILES = ((4, 8, 16, 40), (3, 5, 17, 42))               # aligned; unaligned: the 4-byte stores and the ragged last step
REGION_CASES = [('fp32', 64), ('fp32', 128), ('fp32', 200), ('bf16', 64), ('bf16', 128)]


def tile_engine(topo, family, tile):
    eng = make_engine(topo, family)
    set_images(eng, *WINDOW)
    check(eng.lib.st_tile_configure(eng._ctx, WINDOW[0], WINDOW[1], 0, 0, *tile))
    return eng


@pytest.mark.parametrize('tile', TILES, ids=['aligned', 'unaligned'])
@pytest.mark.parametrize('family,C', REGION_CASES)
def test_region_style_gradient_per_element_and_zero_outside(family, C, tile, monkeypatch):
    """The window is the image, the tile strictly inside it.  The bf16 family is told from the fp32 one by its operand: against the
    bf16 copy of the blob an fp32-kernel result would miss the bar by 2^7 (the phases of a tile-sharded evaluation are not booked
    with the profiler)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if family == 'bf16':
        monkeypatch.setenv('ST2_BF16_LEAN', '0')
    fig = Figures()
    for with_content in (False, True):
        eng = tile_engine(two_conv(C), family, tile)
        check_style_term(eng, 'conv1_2', family, C, tile, C * WINDOW[0] * WINDOW[1], 1.0, with_content, fig,
                         (family, 'region', C) + tile, lambda first: tile_evaluate(eng, first), lambda: second_point(eng, *WINDOW))
        eng.close()
    report(family, 'region', C, 'tile%d,%d,%d,%d' % tile, fig.row())


@pytest.mark.parametrize('tile', [(4, 8, 16, 40), (2, 6, 18, 42)], ids=['aligned', 'unaligned'])
def test_region_style_gradient_below_a_pool(tile):
    """conv1_1, conv1_2, pool1, conv2_1 with the style weight on conv2_1: the region is the tile halved."""
    C = 128
    topo = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 64), ('pool', 'pool1'), ('conv', 'conv2_1', 64, C))
    region = tuple(v // 2 for v in tile)
    gh, gw = -(-WINDOW[0] // 2), -(-WINDOW[1] // 2)
    fig = Figures()
    for with_content in (False, True):
        eng = tile_engine(topo, 'fp32', tile)
        assert eng.blob_shape('conv2_1', *WINDOW) == (C, gh, gw)
        check_style_term(eng, 'conv2_1', 'fp32', C, region, C * gh * gw, 1.0, with_content, fig,
                         ('fp32', 'halved', C) + tile, lambda first: tile_evaluate(eng, first), lambda: second_point(eng, *WINDOW))
        eng.close()
    report('fp32', 'halved-region', C, 'tile%d,%d,%d,%d' % tile, fig.row())


# ------------------------------------------------------------------------------------------ content and deep-dream diffs
def replay_layer_elem(f, target, n_norm, cw, dw, norms):
    """layer_elem_k in numpy float32, one rounding per operation: d = f - t, gc = cn_coef d, out = (cw gc) / norm_c, then likewise
    (dw gd) / norm_d added (gd = dn_coef f)."""
    cn, dn = F32(2.0 / n_norm), F32(-2.0 / n_norm)
    out = np.zeros_like(f)
    if cw:
        out = out + (F32(cw) * (cn * (f - target))) / norms[0]
    if dw:
        out = out + (F32(dw) * (dn * f)) / norms[2]
    return out


def layer_operands(eng, layer):
    """(content features, iterate features or None) of a layer: the content image's through this engine's own forward."""
    if layer == 'data':
        return eng.get_content_nchw()[0], eng.get_input_nchw()[0]
    eng.forward(eng.get_content_nchw(), layer)
    return eng.get_blob(layer)[0], None


@pytest.mark.parametrize('layer,hw', [('data', (5, 7)), ('conv1_1', (5, 7)), ('conv1_1', (8, 64))], ids=['data-5x7', 'conv1_1-5x7', 'conv1_1-8x64'])
@pytest.mark.parametrize('cw,dw', [(0.5, 0.0), (0.0, 0.02), (0.5, 0.02)], ids=['content', 'deepdream', 'both'])
def test_content_and_deepdream_diffs_are_a_float32_replay(layer, hw, cw, dw):
    """Bit for bit, on the 16-byte path (n % 4 == 0: conv1_1) and on the scalar path (data at 5 x 7: n = 105)."""
    eng = make_engine(two_conv(64), 'fp32')
    set_images(eng, *hw)
    target, f = layer_operands(eng, layer)
    weights(eng, layer, cw=cw, dw=dw)
    evaluate(eng)
    if f is None:
        f = eng.get_blob(layer)[0]
    t = eng.layer_terms(layer, want=('diff', 'norms'))
    assert (t['norms'][0] > 0) == bool(cw) and t['norms'][1] == 0 and (t['norms'][2] > 0) == bool(dw)
    assert (f.size % 4 == 0) == (layer != 'data')
    assert np.array_equal(t['diff'][0], replay_layer_elem(f, target, f.size, cw, dw, t['norms']))
    for k in ('D', 'raw_S'):                             # no style term: nothing of one is handed out
        with pytest.raises(StError, match='no style term'):
            eng.layer_terms(layer, want=(k,))
    eng.close()


@pytest.mark.parametrize('cw,dw', [(0.5, 0.0), (0.0, 0.02), (0.5, 0.02)], ids=['content', 'deepdream', 'both'])
def test_region_content_and_deepdream_diffs_replay_and_zero_outside(cw, dw):
    tile = TILES[1]
    eng = tile_engine(two_conv(64), 'fp32', tile)
    target, _ = layer_operands(eng, 'conv1_1')
    weights(eng, 'conv1_1', cw=cw, dw=dw)
    tile_evaluate(eng, False)
    f = eng.get_blob('conv1_1')[0]
    t = eng.layer_terms('conv1_1', want=('diff', 'norms'))
    want = replay_layer_elem(f, target, f.size, cw, dw, t['norms'])
    mask = np.zeros(WINDOW, bool)
    mask[tile[0]:tile[2], tile[1]:tile[3]] = True
    want[:, ~mask] = 0
    assert np.array_equal(t['diff'][0], want)
    assert not np.any(np.signbit(t['diff'][0][:, ~mask]))
    eng.close()


# ------------------------------------------------------------------------------------------ the hook's refusals
def refused(eng, layer, want, match):
    """ST_ERR_STATE, the message names the reason, and nothing was written into the caller's buffers."""
    c, h, w = eng.blob_shape(layer, *eng.input_shape())
    bufs = {'D': np.full((c, c), 12345, F32), 'raw_S': np.full((c, h, w), 12345, F32), 'diff': np.full((c, h, w), 12345, F32)}
    norms = (c_float * 3)(12345, 12345, 12345)
    ptr = lambda k: bufs[k].ctypes.data_as(c_void_p) if k in want else None
    rc = eng.lib.st_get_layer_terms(eng._ctx, eng.blob_index(layer), ptr('D'), ptr('raw_S'), ptr('diff'), norms if 'norms' in want else None)
    msg = eng.lib.st_last_error().decode()
    assert rc == 2 and match in msg, (rc, msg)
    assert all(np.all(b == 12345) for b in bufs.values()) and list(norms) == [12345] * 3


def test_the_hook_refuses_every_stale_read(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    eng = make_engine(two_conv(128), 'fp32')
    set_images(eng, 8, 64)
    eng.set_weights(['conv1_1', 'conv1_2'], [0.5, 0], [1, 1], [0, 0], PARAMS4)
    for want in (('D',), ('raw_S',), ('diff',), ('norms',)):
        refused(eng, 'conv1_2', want, 'no objective evaluation')               # before any evaluation
    evaluate(eng)
    for want in (('D',), ('raw_S',), ('D', 'diff')):
        refused(eng, 'conv1_1', want, 'the style layer evaluated last')        # dbuf / stmp hold conv1_2's
    refused(eng, 'data', ('norms',), 'carried no weight')
    a = eng.layer_terms('conv1_1', want=('diff', 'norms'))                      # ... its diff and norms are its own
    assert np.any(a['diff']) and a['norms'][0] > 0 and a['norms'][1] > 0
    assert set(eng.layer_terms('conv1_2')) == {'D', 'raw_S', 'diff', 'norms'}
    evaluate(eng)                                                               # a second evaluation: the norm is known
    refused(eng, 'conv1_2', ('raw_S',), 'unscaled')
    eng.layer_terms('conv1_2', want=('D', 'diff', 'norms'))
    # st_backward writes the caller's diffs into the same buffers
    eng.backward({'conv1_2': np.zeros((1,) + eng.blob_shape('conv1_2', 8, 64), F32)})
    refused(eng, 'conv1_2', ('diff',), 'st_backward')
    eng.layer_terms('conv1_2', want=('D',))
    eng.layer_terms('conv1_1', want=('diff',))
    # a resized iterate: the work buffers are gone
    eng.set_input(np.zeros((8, 68, 3), np.uint8))
    for want in (('D',), ('diff',), ('norms',)):
        refused(eng, 'conv1_2', want, 'resized')
    eng.close()
    assert eng.lib.st_get_layer_terms(None, 0, None, None, None, None) == 1


def test_the_hook_refuses_a_diff_whose_style_term_rode_on_the_conv(monkeypatch):
    """bf16 flow with a gradient wanted, norm known: the style gradient of conv1_1 is extra K chunks of conv1_2's data gradient and
    nothing is written into its diff.  Without the gradient (out_grad == NULL) the same evaluation materialises it."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    eng = make_engine(two_conv(64), 'bf16')
    set_images(eng, 8, 64)
    eng.set_weights(['conv1_1', 'conv1_2'], [0, 0.5], [1, 0], [0, 0], PARAMS4)
    eng.opfunc(return_grad=True)                                                # first evaluation: unfused, the norm is captured
    assert np.any(eng.layer_terms('conv1_1', want=('diff',))['diff'])
    eng.profile_read()
    eng.opfunc(return_grad=True)
    assert eng.profile_read().get('style_grad_fused_in_conv_dgrad_bf16', {}).get('launches', 0) == 1
    refused(eng, 'conv1_1', ('diff',), 'rode on the data-gradient conv')
    eng.layer_terms('conv1_1', want=('D', 'norms'))
    eng.layer_terms('conv1_2', want=('diff',))
    eng.opfunc(return_grad=False)
    assert np.any(eng.layer_terms('conv1_1', want=('diff',))['diff'])
    eng.close()
