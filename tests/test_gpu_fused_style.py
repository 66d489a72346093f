"""The style term that rides on the bf16 data-gradient conv (ST2_STYLE_FUSE: out = mask(conv) + D' @ F (+ inject)), element by element
against float64 on the operands the launch itself read.  The launch writes into the backward's ping-pong buffers, so its output is
observed through the tap (Engine.tap_diff / tapped_diff: a device-to-device copy right after the launch).  Reference, bound, emulation and
presence coefficients are derived in tests/fused_style_oracle.py and shown reachable and sharp on the CPU in
tests/test_fused_style_oracle_cpu.py; nothing here is fitted to what a kernel returns.

Topology: conv(3 -> 64), conv(64 -> C) [style, optionally content: the tapped blob], conv(C -> K) [content: the top].  Operands are read in
the full data flow ('bf16-full', the flow ST2_BF16_LEAN=0 forces), where every one of them can be read back; the lean flow's tapped diff at
the same point is held to the same reference.  The fused launch exists for C % 64 == 0 and h w % 64 == 0 (the Gram and the gradient on the
bf16 copy), whatever h and w are: its tiles may be clipped at the blob's edge in x and in y, and shapes that do so are in the lists.  At
every other blob of the lists -- C = 96, C = 48, h w % 64 != 0 -- the separate style-gradient kernel must run, and the tapped diff is held
to the same reference within the bound of that route.  ST2_FUSED_STYLE_REPORT=<file> appends the
measured figures of every case (profiles/fused_style_errors.txt was made this way): records, not bars."""
import os

import numpy as np
import pytest

import oracle
import style_transfer2_amd as st2
from oracle.caffe_net import bf16_round
from style_transfer2_amd.capi import StError, check

import fused_style_oracle as fo
import style_grad_oracle as so

pytestmark = pytest.mark.gpu
F32 = np.float32
RS = np.random.RandomState
PARAMS4 = (5, 2, 50, 6)                                 # tv, tv_power, p, p_power
STYLE_HW = (13, 17)                                     # the style image: the target comes from another size
SW, CW_TOP, CW_BLOB = 1.0, 0.125, 0.5                   # so that conv sum and style sum weigh alike (checked per case: Reference.branches)
TRACE_RTOL = 2e-4                                       # the suite's trace tolerance
FUSED, SEP16, SEP32 = 'style_grad_fused_in_conv_dgrad_bf16', 'style_grad_mfma_bf16', 'style_grad_mfma_f32'
# (h, w) of the blob.  Group 0, where the fused launch does not exist (h w % 64 != 0): one pixel, a tiny blob, ragged both ways around one
# 64 x 256-pixel tile and around 64 x 512 tiles.  Group 1, where it does (h w % 64 == 0; the conv tile is 32 pixels wide and 4, 8 or 16
# rows high): one whole 64 x 256-pixel tile, whole 64 x 512 tiles, then tiles clipped at the blob's edge -- in x and y (12, 48), in x
# inside a single tile column (16, 20), in y only (10, 32).  Group 2, the same for C = 512 (32 style chunks: ten groups of three and a
# ragged one): a whole tile and one clipped both ways.
SHAPE_GROUPS = (((1, 1), (5, 7), (9, 33), (17, 70)), ((8, 32), (16, 64), (12, 48), (16, 20), (10, 32)), ((8, 32), (12, 48)))
SWITCHES = ('ST2_STYLE_FUSE', 'ST2_BF16_LEAN', 'ST2_CONV16_CFG', 'ST2_CONV16_SB_MAXK', 'ST2_CONV16_EPI', 'ST2_MASK_BITS', 'ST2_CONV16_UNPOOL',
            'ST2_CONV16_BIG_MIN', 'ST2_CONV16_EPI_KINDS', 'ST2_CONV16_UNPOOL_MAXK')
TILES = {0: '64x256', 1: '128x128', 2: '64x128', 3: '64x512'}      # ST2_CONV16_CFG -> channels x pixels of the tile


def conv16_build(env, K, C):
    """Mirror of conv16_resolve (conv3x3_mfma_bf16.hip) for the tapped data gradient -- reduction depth K, C output channels -- at the
    sizes of this file: (tile, single-buffered staging).  Unforced, a launch of fewer than 512 workgroups takes the 64 x 128 tile; the
    128-channel tile needs MPad % 128 == 0; a wide tile (64 x 256, 64 x 512) with K <= ST2_CONV16_SB_MAXK (64) becomes the
    single-buffered 64 x 256 build.  A mirror, not an observation: it keeps a case's name honest when a threshold moves."""
    cfg = int(env.get('ST2_CONV16_CFG', 2))
    if cfg == 1 and (-(-C // 64) * 64) % 128 != 0:
        cfg = 0
    sb = cfg in (0, 3) and K <= int(env.get('ST2_CONV16_SB_MAXK', 64))
    return (0 if sb else cfg), sb


def _case(env, C, K, group, extra=''):
    tile, sb = conv16_build(env, K, C)
    forced = '' if 'ST2_CONV16_CFG' in env else 'unforced-'
    name = '%s%s%s%s' % (forced, TILES[tile], '-single-buffered' if sb else '', extra)
    return name, env, (tile, sb), C, K, group


def _cfg(n, **more):
    return dict({'ST2_CONV16_CFG': str(n)}, **more)


# Every case is named for the build its tapped launch runs.  Unforced, these sizes always get the 64 x 128 tile, which has neither the
# single-buffered staging nor the specialised epilogues; every other build is forced: the 64 x 256 tile single-buffered (K = 64) and
# double-buffered (K = 128, and K = 64 under ST2_CONV16_SB_MAXK=0), the 128 x 128 tile (MPad % 128 == 0), the 64 x 512 tile (K = 128, and
# K = 64 under ST2_CONV16_SB_MAXK=0: with K = 64 alone it would be the single-buffered 64 x 256 build again); the general epilogue and
# the bf16-copy mask on the single-buffered and on the 64 x 512 build.
CASES = ([_case({}, c, k, g) for c in (64, 96, 128, 256) for k in (64, 128) for g in (0, 1)] +
         [_case({}, 512, k, g) for k in (64, 128) for g in (0, 2)] +
         [_case(_cfg(0), c, k, 1) for c in (64, 128, 256) for k in (64, 128)] +
         [_case(_cfg(1), c, k, 1) for c in (128, 256) for k in (64, 128)] +
         [_case(_cfg(3), c, 128, 1) for c in (64, 128, 256)] +
         [_case(_cfg(n, ST2_CONV16_SB_MAXK='0'), c, 64, 1, '-sb-off') for n in (0, 3) for c in (64, 128, 256)] +
         [_case(_cfg(n, **{sw: '0'}), c, k, 1, tag) for n, k in ((0, 64), (3, 128))
          for sw, tag in (('ST2_CONV16_EPI', '-general-epilogue'), ('ST2_MASK_BITS', '-mask-copies')) for c in (64, 128, 256)] +
         [_case(_cfg(0), 512, 64, 2), _case(_cfg(3), 512, 128, 2)])
BUILDS_RUN = {c[2] for c in CASES}
assert BUILDS_RUN == {(0, True), (0, False), (1, False), (2, False), (3, False)}, BUILDS_RUN


def topo3(C, K, pool=None):
    t = (('conv', 'c1', 3, 64), ('conv', 'c2', 64, C), ('conv', 'c3', C, K))
    return t if pool is None else t + ((('pool', 'p'),) if pool == 'max' else (('pool', 'p', 'ave'),))


def make_engine(topo, params):
    eng = st2.Engine(topo, precision='bf16-full')
    eng.load_weights(params)
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


def weights(eng, top, cw_blob, sw=SW):
    eng.set_weights(['c2', top], [cw_blob, CW_TOP], [sw, 0], [0, 0], PARAMS4)


def tapped_eval(eng):
    """One evaluation with a gradient: (gradient, trace, {class: launches}, tapped diff)."""
    eng.profile_read()
    _, grad, trace = eng.opfunc(return_grad=True)
    prof = {k: v['launches'] for k, v in eng.profile_read().items()}
    return grad, trace, prof, eng.tapped_diff()


def report(*row):
    path = os.environ.get('ST2_FUSED_STYLE_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(' '.join(str(v) for v in row) + '\n')


class Figures:
    """The largest measured ratio to each bar of one case."""

    def __init__(self):
        self.element = self.l2_over_emu = self.presence = self.trace = self.trace_dist = 0.0
        self.emu = {}                                   # this case's CPU emulations, per (shape, content weight)

    def row(self):
        return 'element %.3f rel-L2/(%g emulation) %.3f presence/%g %.3f trace %.3f trace-formula-distance %.3g' % (
            self.element, so.AGG_MARGIN, self.l2_over_emu, so.PRESENCE_BAR, self.presence, self.trace, self.trace_dist)


def emulation(fig, key, op, bf16_only):
    """The CPU emulation of one (shape, content weight) of the case: the full flow's two forms and the lean flow's read the same
    operands, so it is computed once per case and shape (the bf16-only form is the fp32 form rounded once)."""
    if key not in fig.emu:
        fig.emu[key] = fo.emulate(**op)
    return fo.bf16_nearest(fig.emu[key]) if bf16_only else fig.emu[key]


def held(fig, key, what, out, R, op, bf16_only, separate):
    """Both halves of the criterion for one tapped diff."""
    assert out is not None, (key, what, 'the launch wrote no such form')
    out = out[0]
    r = so.worst_ratio(out, R.ref, R.bound(bf16_only, separate))
    fig.element = max(fig.element, r)
    fused = separate is None
    ok, agg = True, {}
    if fused:             # (a separate kernel's own chain is not this emulation's: its diff is held per element)
        ok, agg = fo.aggregate_ok(out, R, emulation(fig, key, op, bf16_only), op['D'], op['F16'], op['coef'], op['c2'])
        worst_p = max(abs(v) for v in agg['presence'].values())
        fig.l2_over_emu = max(fig.l2_over_emu, agg['rel_l2'] / (so.AGG_MARGIN * agg['rel_l2_emulation']))
        fig.presence = max(fig.presence, worst_p / so.PRESENCE_BAR)
    print('%s %s: worst |out - ref| / bound = %.3g%s' % (key, what, r, '' if not fused else ', rel-L2 %.3g (emulation %.3g), worst presence coefficient %.3g' %
                                                       (agg['rel_l2'], agg['rel_l2_emulation'], worst_p)))
    if r > 1.0:
        err = np.abs(out.astype(np.float64) - R.ref) / np.where(R.bound(bf16_only, separate) > 0, R.bound(bf16_only, separate), 1e-300)
        assert False, (key, what, 'element (c, y, x) = %s misses its bound by %.3g' % (np.unravel_index(np.argmax(err), err.shape), r))
    assert ok, (key, what, agg)


def read_operands(eng, top, C, K, h, w, params, cw_blob, separate, d16=None):
    """What the tapped launch of the last (full-flow) evaluation read, from the device; leaves the weights as they were."""
    f32 = eng.get_blob('c2')[0]
    t = eng.layer_terms('c2', want=('D', 'norms'))
    if d16 is None:
        d16 = bf16_round(eng.layer_terms(top, want=('diff',))['diff'][0])
    base = None
    if cw_blob:           # the content part as bits from the device: the same evaluation with the style weight zero
        weights(eng, top, cw_blob, sw=0.0)
        eng.opfunc(return_grad=False)
        base = eng.layer_terms('c2', want=('diff',))['diff'][0]
        weights(eng, top, cw_blob)
    op = dict(w16=bf16_round(params['c3'][0]), d16=d16, F16=bf16_round(f32), D=t['D'], coef=fo.coef_of(SW, t['norms'][1]),
              c2=so.c2_of(C, C * h * w), base=base)
    return op, fo.Reference(**op, style_operand=f32 if separate == 'fp32' else None), eng.style_gram('c2')


def check_branches(key, R):
    masked, s_over_c, c_over_s = R.branches()
    print('%s: %.2f of the elements masked; unmasked median A_s / A_c %.3g, A_c / A_s %.3g' % (key, masked, s_over_c, c_over_s))
    if R.ref.size >= 1024:            # (a blob of a few pixels has no quarter of anything)
        assert 0.25 <= masked <= 0.75 and s_over_c >= 0.05 and c_over_s >= 0.05, (key, masked, s_over_c, c_over_s)


def expected_route(C, h, w):
    """(fused, the separate class that must run otherwise, its family)."""
    if fo.fused_shape(C, h, w):
        return True, None, None
    return (False, SEP16, 'bf16') if C % 64 == 0 else (False, SEP32, 'fp32')


def style_launches(prof, fused, sep_cls):
    """The launch is what the case names: the fused class once and no separate bf16 style gradient, or the separate class once."""
    got = {k: prof.get(k, 0) for k in (FUSED, SEP16)}
    if fused:
        assert got == {FUSED: 1, SEP16: 0}, prof
    else:
        assert got[FUSED] == 0 and prof.get(sep_cls, 0) == 1, prof


def trace_checks(fig, key, trace, op, A, C, n):
    """The trace value of style_s2_trace_k against its float64 restatement: trace[3] = |sw / norm| sqrt(S2 / n) of the first row."""
    s2 = (float(trace[3]) / abs(float(op['coef']))) ** 2 * n
    ref, bound = fo.trace_reference(op['D'], A, op['c2'], n)
    dist = fo.trace_distance(op['D'], A, op['c2'], n, op['F16'])
    r = abs(s2 - ref) / bound
    print('%s: trace |S2 - ref| / bound = %.3g; the formula is %.3g from || c2 D F16 ||^2' % (key, r, dist))
    fig.trace, fig.trace_dist = max(fig.trace, r), max(fig.trace_dist, dist)
    assert r <= 1.0, (key, 'trace', s2, ref, bound)


# ------------------------------------------------------------------------------------------ the fused launch, every build
@pytest.mark.parametrize('variant,env,build,C,K,group', CASES, ids=['%s-C%d-K%d-g%d' % (c[0], c[3], c[4], c[5]) for c in CASES])
def test_fused_style_term_per_element_against_float64(variant, env, build, C, K, group, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert conv16_build(env, K, C) == build
    topo = topo3(C, K)
    params = oracle.he_init_weights(topo, seed=1, bias_std=0.1)
    eng = make_engine(topo, params)
    fig = Figures()
    for h, w in SHAPE_GROUPS[group]:
        fused, sep_cls, sep = expected_route(C, h, w)
        n = C * h * w
        for cw_blob in (0.0, CW_BLOB):
            key = (variant, C, K, h, w, bool(cw_blob))
            eng.set_precision('bf16-full')
            eng.tap_diff(None)
            set_images(eng, h, w)
            weights(eng, 'c3', cw_blob)
            eng.opfunc(return_grad=True)                    # first evaluation: the norms are captured, nothing is fused
            second_point(eng, h, w)
            # ---- the full data flow, tapped: fp32 and bf16 forms of one accumulator
            eng.tap_diff('c2')
            g_full, tr_full, prof_full, tap_full = tapped_eval(eng)
            style_launches(prof_full, fused, sep_cls)
            op, R, A = read_operands(eng, 'c3', C, K, h, w, params, cw_blob, sep)
            check_branches(key, R)
            held(fig, key, 'full flow, fp32 form', tap_full['f32'], R, op, False, sep)
            held(fig, key, 'full flow, bf16 form', tap_full['bf16'], R, op, True, sep)
            if fused:
                trace_checks(fig, key, tr_full, op, A, C, n)
            # ---- the lean flow at the same point: bf16 only, the same reference, the same image gradient
            eng.set_precision('bf16')
            g_lean, tr_lean, prof_lean, tap_lean = tapped_eval(eng)
            style_launches(prof_lean, fused, sep_cls)
            assert tap_lean['f32'] is None, (key, 'the lean flow wrote an fp32 diff')
            held(fig, key, 'lean flow', tap_lean['bf16'], R, op, True, sep)
            assert np.array_equal(g_lean, g_full), (key, 'lean and full image gradients differ')
            if env:
                continue
            # ---- tap on versus tap off: the same bits, the same launches in every class
            eng.tap_diff(None)
            eng.profile_read()
            _, g_off, tr_off = eng.opfunc(return_grad=True)
            prof_off = {k: v['launches'] for k, v in eng.profile_read().items()}
            assert np.array_equal(g_off, g_lean) and np.array_equal(tr_off, tr_lean) and prof_off == prof_lean, (key, prof_off, prof_lean)
            with pytest.raises(StError, match='no diff is tapped'):
                eng.tapped_diff()
            # ---- ST2_STYLE_FUSE=0 at the same point: the separate kernel through the inject buffer, this bound plus that kernel's
            if fused:
                monkeypatch.setenv('ST2_STYLE_FUSE', '0')
                eng.set_precision('bf16-full')
                eng.tap_diff('c2')
                _, tr_sep, prof_sep, tap_sep = tapped_eval(eng)
                monkeypatch.delenv('ST2_STYLE_FUSE')
                style_launches(prof_sep, False, SEP16)
                for form, b16 in (('f32', False), ('bf16', True)):
                    r = so.worst_ratio(tap_sep[form][0], R.ref, R.bound(b16, 'bf16'))
                    print('%s unfused, %s form: worst ratio %.3g' % (key, form, r))
                    assert r <= 1.0, (key, 'unfused', form, r)
                assert np.isclose(tr_full[3], tr_sep[3], rtol=TRACE_RTOL, atol=0), (key, tr_full[3], tr_sep[3])
    report(variant, C, K, 'group%d' % group, fig.row())
    eng.close()


def test_forty_eight_channels_do_not_fuse_and_the_switch_changes_nothing(monkeypatch):
    """C = 48: the separate class runs, and the tapped diff equals the ST2_STYLE_FUSE=0 one bit for bit."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    C, K = 48, 64
    topo = topo3(C, K)
    params = oracle.he_init_weights(topo, seed=1, bias_std=0.1)
    eng = make_engine(topo, params)
    fig = Figures()
    for h, w in ((8, 32), (9, 33)):
        key = ('C48', C, K, h, w, True)
        set_images(eng, h, w)
        weights(eng, 'c3', CW_BLOB)
        eng.opfunc(return_grad=True)
        second_point(eng, h, w)
        eng.tap_diff('c2')
        g1, _, prof1, tap1 = tapped_eval(eng)
        style_launches(prof1, False, SEP32)
        op, R, _ = read_operands(eng, 'c3', C, K, h, w, params, CW_BLOB, 'fp32')
        held(fig, key, 'full flow, fp32 form', tap1['f32'], R, op, False, 'fp32')
        monkeypatch.setenv('ST2_STYLE_FUSE', '0')
        g0, _, prof0, tap0 = tapped_eval(eng)
        monkeypatch.delenv('ST2_STYLE_FUSE')
        assert prof0 == prof1 and np.array_equal(g0, g1)
        for form in ('f32', 'bf16'):
            assert (tap0[form] is None) == (tap1[form] is None) and (tap0[form] is None or np.array_equal(tap0[form], tap1[form])), form
        eng.tap_diff(None)
    report('unforced-64x128', C, K, 'no-fuse', fig.row())
    eng.close()


# ------------------------------------------------------------------------------------------ the unpooling builds
# even sizes: the smallest, whole tiles, a ragged one where the separate kernel runs, and the fused shapes with clipped tiles
UNPOOL_SHAPES = ((2, 2), (8, 32), (16, 64), (18, 66), (12, 48), (16, 20), (10, 32))
UNPOOL_CASES = [(pool, cfg, c, k) for pool in ('max', 'ave') for cfg in (0, 3) for c, k in ((64, 64), (128, 128), (256, 64))]


@pytest.mark.parametrize('pool,cfg,C,K', UNPOOL_CASES, ids=['%s-cfg%d-C%d-K%d' % c for c in UNPOOL_CASES])
def test_fused_style_term_under_the_unpooling_builds(pool, cfg, C, K, monkeypatch):
    """A pool on top (content on the pool): in the lean flow the conv's full-resolution output is never materialised and its data
    gradient expands the pooled diff itself.  With ST2_CONV16_UNPOOL=0 the separate pool backward writes the full-resolution bf16 diff:
    tapped, it is the d16 the float64 reference takes; the unpooling launch must then give the same bits (routing only places values)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('ST2_CONV16_CFG', str(cfg))          # (a wide tile: the only ones with the pooling and unpooling builds)
    topo = topo3(C, K, pool)
    params = oracle.he_init_weights(topo, seed=1, bias_std=0.1)
    eng = make_engine(topo, params)
    if pool == 'ave':
        eng.set_pool_algo(1)
    fig = Figures()
    for h, w in UNPOOL_SHAPES:
        fused, sep_cls, sep = expected_route(C, h, w)
        key = ('unpool-%s-cfg%d' % (pool, cfg), C, K, h, w, False)
        eng.set_precision('bf16-full')
        eng.tap_diff(None)
        set_images(eng, h, w)
        weights(eng, 'p', 0.0)
        eng.opfunc(return_grad=True)
        second_point(eng, h, w)
        eng.opfunc(return_grad=True)                        # the full flow at the point: F, D and the norms can be read back
        f32 = eng.get_blob('c2')[0]
        t = eng.layer_terms('c2', want=('D', 'norms'))
        # ---- lean flow, the separate pool backward: the full-resolution diff above, then the diff of the style blob
        eng.set_precision('bf16')
        monkeypatch.setenv('ST2_CONV16_UNPOOL', '0')
        eng.tap_diff('c3')
        _, _, prof_a, above = tapped_eval(eng)
        assert above['f32'] is None and above['bf16'] is not None, (key, 'the pool backward writes bf16 only')
        eng.tap_diff('c2')
        g0, _, prof0, tap0 = tapped_eval(eng)
        style_launches(prof0, fused, sep_cls)
        op = dict(w16=bf16_round(params['c3'][0]), d16=above['bf16'][0], F16=bf16_round(f32), D=t['D'], coef=fo.coef_of(SW, t['norms'][1]),
                  c2=so.c2_of(C, C * h * w), base=None)
        R = fo.Reference(**op)
        held(fig, key, 'separate pool backward', tap0['bf16'], R, op, True, sep)
        # ---- the unpooling build: the same values
        monkeypatch.delenv('ST2_CONV16_UNPOOL')
        g1, _, prof1, tap1 = tapped_eval(eng)
        style_launches(prof1, fused, sep_cls)
        pool_cls = 'maxpool_bwd' if pool == 'max' else 'avepool_bwd_map16'
        assert prof0.get(pool_cls, 0) == 1 and prof1.get(pool_cls, 0) == 0, (key, 'the unpooling build did not run', prof0, prof1)
        assert tap1['f32'] is None and np.array_equal(tap1['bf16'], tap0['bf16']), (key, 'the unpooling launch differs from the separate pool backward')
        assert np.array_equal(g1, g0)
        eng.tap_diff('c3')                                  # ... and no launch writes the full-resolution diff above any more
        eng.opfunc(return_grad=True)
        with pytest.raises(StError, match='c3'):
            eng.tapped_diff()
    report('unpool-%s-cfg%d' % (pool, cfg), C, K, 'all', fig.row())
    eng.close()


# ------------------------------------------------------------------------------------------ the tap's refusals
def test_the_tap_refuses_what_it_cannot_answer(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    topo = topo3(64, 64)
    eng = make_engine(topo, oracle.he_init_weights(topo, seed=1, bias_std=0.1))
    set_images(eng, 8, 32)
    weights(eng, 'c3', 0.0)
    with pytest.raises(StError, match='no diff is tapped'):
        eng.tapped_diff()
    eng.tap_diff('c2')
    with pytest.raises(StError, match='c2'):                # read-back before an evaluation
        eng.tapped_diff()
    eng.opfunc(return_grad=False)                           # ... and an evaluation without a gradient has no backward
    with pytest.raises(StError, match='no evaluation with a gradient'):
        eng.tapped_diff()
    with pytest.raises(StError, match='only st_opfunc'):    # st_step with a tap: refused before anything is enqueued
        eng.step()
    with pytest.raises(StError, match='only st_opfunc'):
        eng.step_begin()
    assert eng.steps_pending() == 0
    eng.opfunc(return_grad=True)
    assert eng.tapped_diff()['f32'] is not None
    eng.set_input(np.zeros((8, 36, 3), np.uint8))           # a resized iterate
    with pytest.raises(StError, match='resized'):
        eng.tapped_diff()
    eng.set_content(np.zeros((8, 36, 3), np.uint8))
    eng.opfunc(return_grad=True)
    assert eng.tapped_diff()['f32'].shape == (1, 64, 8, 36)
    # tile-sharded: the tap is refused on a tile-configured context, and the configuration under a tap
    rc = eng.lib.st_tile_configure(eng._ctx, 8, 36, 0, 0, 0, 0, 8, 36)
    assert rc == 2 and 'diff tap' in eng.lib.st_last_error().decode()
    eng.tap_diff(None)
    check(eng.lib.st_tile_configure(eng._ctx, 8, 36, 0, 0, 0, 0, 8, 36))
    with pytest.raises(StError, match='tile-configured'):
        eng.tap_diff('c2')
    eng.close()
    assert eng.lib.st_tap_diff(None, 0) == 1 and eng.lib.st_get_tapped_diff(None, None, None, None, None) == 1
