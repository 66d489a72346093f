"""Convs, pools and Grams held to EXACT integer references, ties included (``pytest -m gpu``).

The operands are small integers (tests/exact_oracle.py has the recipes, the float64 references and the derivation of why every
kernel must then reproduce them bit for bit): every comparison is np.array_equal, every case asserts through
engine.profile_read() which kernel class ran, and every recipe passes exact_oracle.assert_exact_domain before anything is launched.

  A  one conv layer, forward and data gradient, on every kernel family and tile configuration; conv1_1's own kernels
  B  the VGG head (two pools) on data full of tied pooling windows and pre-activations of exactly zero, on every pool route:
     the first-maximum rule and the `> 0` mask, blob by blob and through the ranged backward with injected diffs
  C  the Gram on every launch plan, the style targets, and the raw sums of a tile-sharded style pass

What these tests reach is what the model hooks (st_forward / st_backward / st_gram / st_set_style) run.  The hooks never run the
LEAN data flow of an iteration: under bf16 a pool is then a stand-alone kernel on the fp32 blob, so the bf16 epilogues' fused pool
with its arg-max map, maxpool_bwd_idx16_k, the unpooling bf16 data gradient and the sign-map masks stay with the bit-for-bit A/B
tests of tests/test_gpu_bf16.py (their switches are still run here: they change tile configurations and epilogues of the convs).
Style gradients, norms, losses and the optimizer passes are out of scope: their scalars are not dyadic."""

import collections

import numpy as np
import pytest

import style_transfer2_amd as st2
from style_transfer2_amd import tiling
from style_transfer2_amd.tile_backend import dev_tensor
import exact_oracle as eo
from test_gpu_edge_sizes import FAMILIES, conv_launches, dgrad_class, fwd_class, make_model
from test_gpu_edge_sizes import DG_BF16, DG_F32, DG_SPLIT, DG_WINO, FWD_BF16, FWD_F32, FWD_SPLIT, FWD_WINO

pytestmark = pytest.mark.gpu
F32 = np.float32
DOMAIN = {FWD_F32: 'direct', FWD_WINO: 'wino', FWD_SPLIT: 'split', FWD_BF16: 'bf16',
          DG_F32: 'direct', DG_WINO: 'wino', DG_SPLIT: 'split', DG_BF16: 'bf16'}


def launches(engine, prefix=''):
    return collections.Counter({k: v['launches'] for k, v in engine.profile_read().items() if k.startswith(prefix)})


def x4(a):
    """(C, h, w) float64 integers -> the (1, C, h, w) float32 array the hooks take (exact)."""
    return np.ascontiguousarray(np.asarray(a, F32)[None])


def assert_equal(got, want, what):
    got = np.asarray(got, np.float64).reshape(np.shape(want))
    bad = got != want
    assert not bad.any(), '%s: %d of %d elements differ from the exact reference, first at %s: got %r, exact %r' % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), float(got[bad][0]), float(np.asarray(want)[bad][0]))


# ------------------------------------------------------------------------------------------ A. one conv layer, every family
EXACT_FAMILIES = dict(FAMILIES)
EXACT_FAMILIES['wino-cfg1'] = ('wino', {'ST2_WINO_CFG': '1'})
# (128, 48): 48 output channels, the smallest the Winograd kernel takes in the forward; (40, 64): 40 < 48 input channels make the
# fp32 data gradient fall back to the direct kernel, and 40 % 16 != 0 the split-operand forward to the fp32 Winograd kernel
A_PAIRS = [(64, 64), (64, 128), (256, 256), (512, 512), (128, 48), (40, 64)]
# a one-pixel tile; one past a 32-column tile; widths = 0 mod 4 (the split kernel); an any-width build; few workgroups at deep K
# (split-K)
A_SHAPES = [(1, 1), (2, 3), (5, 33), (6, 36), (8, 64), (9, 70)]


def _layer_params():
    out = []
    for f, family in enumerate(EXACT_FAMILIES):
        for i, (h, w) in enumerate(A_SHAPES):
            j = (i + f) % len(A_PAIRS)
            while A_PAIRS[j][0] * A_PAIRS[j][1] * h * w > 100e6:          # the oracle's cost, as test_gpu_edge_sizes._heavy
                j = (j + 1) % len(A_PAIRS)
            out.append(pytest.param(family, A_PAIRS[j][0], A_PAIRS[j][1], h, w, id='%s-%d-%d-%dx%d' % ((family,) + A_PAIRS[j] + (h, w))))
    return out


def _domains(path):
    """ExactNet's `paths`: the exactness conditions of the kernel class each launch of `path` must run as."""
    def of(layer, direction):
        _, _, cin, cout = layer
        if cin == 3:        # conv1_1: fp32 kernels; bf16 path: the split-operand forward, bf16 operands in the data gradient
            return ('direct', 'split') if direction == 'fwd' else ('bf16' if path == 'bf16' else 'direct')
        # (the width does not matter here: a launch the split kernel refuses is held to the `wino` conditions, which `split` includes)
        return DOMAIN[fwd_class(path, cin, cout, 4) if direction == 'fwd' else dgrad_class(path, cin, cout, 4)]
    return of


@pytest.mark.parametrize('family,cin,cout,h,w', _layer_params())
def test_conv_layer_is_exact_on_integers(family, cin, cout, h, w, monkeypatch):
    """conv1_1 (3 -> cin, sparse) then conv1_2 (cin -> cout, dense in {-1, 0, 1}, integer bias): both blobs must equal
    relu(exact conv), and the data gradient of an integer diff in [-2, 2] -- masked by the exact conv1_1 blob, through conv1_1's
    own data gradient down to the image -- the exact chain (bf16 path: the diff conv1_1's kernel reads is the exact one rounded to
    bf16, as the path stores it)."""
    path, env = EXACT_FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    topo, params, x, dy = eo.layer_recipe(cin, cout, h, w)
    net = eo.ExactNet(topo, params, paths=_domains(path), bf16=path == 'bf16')
    blobs = net.forward(x)
    want_grad = net.backward({'conv1_2': dy})                  # (every domain check has passed: nothing is launched before)
    gpu = make_model(eo.params32(params), topo, path)
    gpu.engine.profile_enable(True)
    f = gpu.forward(x4(x), ['conv1_1', 'conv1_2'])
    fwd = conv_launches(gpu.engine)
    for name in ('conv1_1', 'conv1_2'):
        assert_equal(f[name], blobs[name], '%s forward %s' % (family, name))
    assert fwd == collections.Counter([fwd_class(path, ci, co, w) for _, _, ci, co in topo]), (family, fwd)
    gpu.engine.profile_enable(True)
    got = gpu.backward({'conv1_2': x4(dy)})
    bwd = conv_launches(gpu.engine)
    assert_equal(got, want_grad, '%s data gradient' % family)
    assert bwd == collections.Counter([dgrad_class(path, ci, co, w) for _, _, ci, co in topo]), (family, bwd)
    gpu.engine.close()


@pytest.mark.parametrize('h,w', [(1, 1), (5, 33), (8, 64), (23, 132)], ids=lambda v: str(v))
@pytest.mark.parametrize('kind', ['fp32', 'bf16-split', 'bf16-nosplit'])
def test_first_conv_kernels_are_exact_on_integers(kind, h, w, monkeypatch):
    """conv1_1 alone (3 -> 64, dense): the fp32 forward kernel, the bf16 path's split-operand kernel (ST2_FIRST_SPLIT=1) and its
    stand-in (=0); the data gradient by the strip walker, the tile kernel and the VALU kernels (fp32: ST2_DGRAD_FIRST unset, 1, 0;
    bf16: ST2_DGRAD_FIRST_STRIP unset, 0), with and without an integer diff injected at the image."""
    topo, params, x, dy = eo.layer_recipe(3, 64, h, w)
    bf16 = kind != 'fp32'
    net = eo.ExactNet(topo, params, paths=_domains('bf16' if bf16 else 'direct'), bf16=bf16)
    blob = net.forward(x)['conv1_1']
    inj = eo.int_diff(np.random.RandomState(h * 7 + w), x.shape)
    cases = [({'conv1_1': dy}, net.backward({'conv1_1': dy})), ({'conv1_1': dy, 'data': inj}, net.backward({'conv1_1': dy, 'data': inj}))]
    monkeypatch.setenv('ST2_FIRST_SPLIT', '0' if kind == 'bf16-nosplit' else '1')
    gpu = st2.HipModel(eo.params32(params), topology=topo, precision='bf16' if bf16 else 'fp32')
    gpu.engine.profile_enable(True)
    f = gpu.forward(x4(x), ['conv1_1'])
    assert conv_launches(gpu.engine) == collections.Counter({FWD_F32: 1})
    assert_equal(f['conv1_1'], blob, '%s conv1_1 forward' % kind)
    variants = [('ST2_DGRAD_FIRST', None), ('ST2_DGRAD_FIRST', '1'), ('ST2_DGRAD_FIRST', '0')] if not bf16 else \
        [('ST2_DGRAD_FIRST_STRIP', None), ('ST2_DGRAD_FIRST_STRIP', '0')]
    for diffs, want in cases:
        for var, val in variants:
            if val is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, val)
            gpu.engine.profile_enable(True)
            got = gpu.backward({n: x4(v) for n, v in diffs.items()})
            assert conv_launches(gpu.engine) == collections.Counter({DG_F32: 1}), (var, val)
            assert_equal(got, want, '%s conv1_1 data gradient %s=%s %s' % (kind, var, val, sorted(diffs)))
    gpu.engine.close()


# ------------------------------------------------------------------------------------------ B. ties and zeros, every pool route
# (8, 32): W % 32 == 0, the unpooling input transform of conv1_2's data gradient; (16, 24): the map without unpooling; (9, 13):
# clipped windows, any-width builds, the scalar pool kernels; (6, 64): an odd pooled height (no map at pool2)
B_SIZES = [(8, 32), (16, 24), (9, 13), (6, 64)]
# At these sizes every Winograd launch would split K (few workgroups), and a split-K launch has no fused pool: the routes that are
# about the fused pool and its map switch split-K off (ST2_WINO_SPLITK=0), `*-splitk` run the same switches with it on.
NOSPLITK = {'ST2_WINO_SPLITK': '0'}
B_ROUTES = {        # id -> (precision, conv algorithm, environment)
    'amap-unpool': ('fp32', 1, dict(NOSPLITK, ST2_POOL_AMAP='1', ST2_WINO_UNPOOL='1')),
    'amap': ('fp32', 1, dict(NOSPLITK, ST2_POOL_AMAP='1', ST2_WINO_UNPOOL='0')),
    'no-amap': ('fp32', 1, dict(NOSPLITK, ST2_POOL_AMAP='0')),
    'no-fused-pool': ('fp32', 1, dict(NOSPLITK, ST2_WINO_POOL='0')),
    'direct': ('fp32', 1, dict(NOSPLITK, ST2_WINO='0')),
    'lean32-off': ('fp32', 1, dict(NOSPLITK, ST2_LEAN32='0')),
    'default-splitk': ('fp32', 1, {}),
    'split': ('fp32', 2, dict(NOSPLITK)),
    'split-dgrad64-off': ('fp32', 2, dict(NOSPLITK, ST2_WS_DGRAD64='0')),
    'split-splitk': ('fp32', 2, {}),
    'bf16': ('bf16', 1, {}),
    'bf16-cfg0': ('bf16', 1, {'ST2_CONV16_CFG': '0'}),
    'bf16-unpool-off': ('bf16', 1, {'ST2_CONV16_UNPOOL': '0'}),
    'bf16-mask-bits-off': ('bf16', 1, {'ST2_MASK_BITS': '0'}),
    'bf16-epi-off': ('bf16', 1, {'ST2_CONV16_EPI': '0'}),
    'bf16-full': ('bf16-full', 1, {}),
}
B_DIFF_SETS = [(n,) for n in eo.HEAD_INJECTIONS] + [('pool2', 'pool1', 'data'), eo.HEAD_INJECTIONS]
_head = {}


def head_reference(h, w):
    """The recipe and its exact references at one size, fp32 and bf16, computed once and never modified."""
    if (h, w) not in _head:
        params, x, diffs, seed = eo.head_recipe(h, w)
        ref = {}
        for bf16 in (False, True):
            net = eo.ExactNet(eo.HEAD_TOPOLOGY, params, paths=('direct', 'wino', 'split', 'bf16') if bf16 else ('direct', 'wino', 'split'), bf16=bf16)
            blobs = dict(net.forward(x))
            for name in eo.HEAD_POOLED:                       # the conditions, on the reference alone
                eo.assert_tie_conditions(net.pre[name], name)
            for name, blob in blobs.items():
                assert eo.bf16_representable(blob), name     # every blob the bf16 path stores as bf16 is stored exactly
            ref[bf16] = (blobs, {names: net.backward({n: diffs[n] for n in names}) for names in B_DIFF_SETS})
        for name in blobs:
            assert np.array_equal(ref[False][0][name], ref[True][0][name])
        _head[(h, w)] = (params, x, diffs, ref)
    return _head[(h, w)]


def _splitk(nblk, nch):
    sp = 1
    while nblk * sp * 2 <= 256 and nch % (sp * 2) == 0 and nch // (sp * 2) >= 4 and sp < 16:
        sp *= 2
    return sp


def _wino_facts(k, m, h, w, env):
    """What conv3x3_winograd.hip's wino_resolve decides for the default variant: (fused pool, its arg-max map, unpooling input
    transform)."""
    quad = w % 4 == 0
    if (m + 127) // 128 * 128 <= (m + 63) // 64 * 64:
        bm, prows, amap, full = 128, 4, True, True
    elif quad:
        bm, prows, amap, full = 64, 4, True, True              # the half tile
    else:
        bm, prows, amap, full = 64, 8, False, False
    nblk = -(-w // 32) * -(-h // prows) * -(-m // bm)
    splits = _splitk(nblk, k // 8) if (h * w) % 4 == 0 and env.get('ST2_WINO_SPLITK') != '0' else 1
    can_pool = splits == 1 and env.get('ST2_WINO_POOL') != '0'
    return can_pool, can_pool and quad and h % 2 == 0 and amap, w % 32 == 0 and h % 2 == 0 and full and env.get('ST2_WINO_UNPOOL') != '0'


def _split_facts(k, m, h, w, env):
    """conv3x3_wino_split.hip's wino_split_resolve: (takes the shape, fused pool, its map)."""
    ok = k % 16 == 0 and m % 64 == 0 and w >= 4 and w % 4 == 0
    nblk = -(-w // 32) * -(-h // 8) * (m // 64)
    splits = _splitk(nblk, k // 16) if ok and env.get('ST2_WINO_SPLITK') != '0' else 1
    can_pool = ok and splits == 1 and env.get('ST2_WINO_POOL') != '0'
    return ok, can_pool, can_pool and h % 2 == 0


def head_plan(precision, algo, env, h, w, injected):
    """The kernel classes engine_route.cpp plans for the head through the hooks (never lean): (forward conv classes, stand-alone
    forward pools, data-gradient conv classes, stand-alone backward pools) for a backward with diffs at `injected`."""
    names = ['data'] + [layer[1] for layer in eo.HEAD_TOPOLOGY]
    top = max(names.index(n) for n in injected)
    hh, ww = {}, {}
    ch, cw = h, w
    for i, layer in enumerate(eo.HEAD_TOPOLOGY, start=1):
        if layer[0] == 'pool':
            ch, cw = eo.pooled_size(ch), eo.pooled_size(cw)
        hh[i], ww[i] = ch, cw
    fwd, bwd = collections.Counter(), collections.Counter()
    pools_fwd = pools_bwd = 0
    amap, unpool_below = {}, {}
    for i, layer in enumerate(eo.HEAD_TOPOLOGY, start=1):
        if layer[0] == 'pool':
            continue
        _, name, cin, cout = layer
        pooled = i < len(eo.HEAD_TOPOLOGY) and eo.HEAD_TOPOLOGY[i][0] == 'pool'
        fused = False
        if cin == 3:
            fcls = dcls = 'direct'
        elif precision != 'fp32':
            fcls = dcls = 'bf16'
        elif env.get('ST2_WINO') == '0':
            fcls = dcls = 'direct'
        else:
            fcls = dcls = 'wino'
            fused, amap[i + 1], _ = _wino_facts(cin, cout, hh[i], ww[i], env)
            _, _, unpool_below[i] = _wino_facts(cout, cin, hh[i], ww[i], env)
            if algo == 2:
                ok, pool_s, amap_s = _split_facts(cin, cout, hh[i], ww[i], env)
                if ok:
                    fcls, fused, amap[i + 1] = 'split', pool_s, amap_s
                ok_d, _, _ = _split_facts(cout, cin, hh[i], ww[i], env)
                if ok_d and not (env.get('ST2_WS_DGRAD64') == '0' and cout <= 64 and unpool_below[i]):
                    dcls, unpool_below[i] = 'split', False
            if env.get('ST2_POOL_AMAP') == '0':
                amap[i + 1] = False
        fwd[{'direct': FWD_F32, 'wino': FWD_WINO, 'split': FWD_SPLIT, 'bf16': FWD_BF16}[fcls]] += 1
        if pooled and not fused:
            pools_fwd += 1
        if i <= top:
            bwd[{'direct': DG_F32, 'wino': DG_WINO, 'split': DG_SPLIT, 'bf16': DG_BF16}[dcls]] += 1
    for i, layer in enumerate(eo.HEAD_TOPOLOGY, start=1):
        if layer[0] == 'pool' and i <= top:
            through_map = amap.get(i, False) and names[i - 1] not in injected
            if not (through_map and unpool_below.get(i - 1, False)):
                pools_bwd += 1                                  # maxpool_bwd_amap_k or the classic kernel; else inside the conv below
    return fwd, pools_fwd, bwd, pools_bwd


@pytest.mark.parametrize('route', list(B_ROUTES))
@pytest.mark.parametrize('h,w', B_SIZES, ids=lambda v: str(v))
def test_head_with_ties_and_zeros_is_exact_on_every_pool_route(h, w, route, monkeypatch):
    """conv1_1 conv1_2 pool1 conv2_1 conv2_2 pool2 on an image constant on 4 x 4 blocks with 3-tap filters: most pooling windows
    with a positive maximum are tied and a fifth of the pre-activations is exactly 0 (asserted on the reference).  Every blob must
    equal the exact one, every pooled blob the exact Caffe pool of it, and the ranged backward the exact Caffe backward -- first
    maximum of a row-major scan, mask `> 0` -- with integer diffs injected at pool2, conv2_2, pool1, conv1_2 and data, one at a time
    and together.  Every route equals the one reference, hence every other route.  bf16: every blob of the recipe is
    bf16-representable (asserted), and the reference rounds each running diff where the path stores it as bf16, so the whole chain
    runs, not only the part below pool1."""
    precision, algo, env = B_ROUTES[route]
    params, x, diffs, ref = head_reference(h, w)
    blobs, grads = ref[precision != 'fp32']
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gpu = st2.HipModel(eo.params32(params), topology=eo.HEAD_TOPOLOGY, precision=precision)
    if algo == 2:
        gpu.engine.set_conv_algo(2)
    names = [layer[1] for layer in eo.HEAD_TOPOLOGY]
    gpu.engine.profile_enable(True)
    f = gpu.forward(x4(x), names)
    prof = launches(gpu.engine)
    want_fwd, want_pools, _, _ = head_plan(precision, algo, env, h, w, ('pool2',))
    assert collections.Counter({k: v for k, v in prof.items() if k.startswith('conv3x3_')}) == want_fwd, (route, prof)
    assert prof.get('maxpool_fwd', 0) == want_pools, (route, prof)
    for name in names:
        assert_equal(f[name], blobs[name], '%s %s' % (route, name))
    for below, name in (('conv1_2', 'pool1'), ('conv2_2', 'pool2')):
        assert_equal(f[name], eo.maxpool_exact(f[below][0])[0], '%s %s of the GPU\'s own %s' % (route, name, below))
    for inj in B_DIFF_SETS:
        _, _, want_bwd, want_pools = head_plan(precision, algo, env, h, w, inj)
        gpu.engine.profile_enable(True)
        got = gpu.backward({n: x4(diffs[n]) for n in inj})
        prof = launches(gpu.engine)
        assert_equal(got, grads[inj], '%s backward from %s' % (route, '+'.join(inj)))
        assert collections.Counter({k: v for k, v in prof.items() if k.startswith('conv3x3_')}) == want_bwd, (route, inj, prof)
        assert prof.get('maxpool_bwd', 0) == want_pools, (route, inj, prof)
    gpu.engine.close()


def test_head_routes_cover_the_map_the_unpooling_transform_and_the_classic_kernels():
    """The plan above, at the sizes above, does reach what part B is about (a change of the engine's thresholds that moved every
    case onto the classic kernels would otherwise go unnoticed): pool launches fused away forward, routed through the map
    stand-alone, and expanded inside the data gradient below."""
    p = {(s, r): head_plan(*B_ROUTES[r], s[0], s[1], ('pool2',)) for s in B_SIZES for r in B_ROUTES}
    assert p[((8, 32), 'amap-unpool')][1] == 0 and p[((8, 32), 'amap-unpool')][3] == 1       # pool1 unpooled in conv1_2's data gradient
    assert p[((8, 32), 'amap')][3] == 2 and p[((8, 32), 'no-amap')][1] == 0
    assert p[((16, 24), 'amap-unpool')][1] == 0 and p[((16, 24), 'amap-unpool')][3] == 2     # the map, no unpooling (W % 32 != 0)
    assert p[((6, 64), 'amap-unpool')][3] == 1 and p[((9, 13), 'amap-unpool')][3] == 2
    assert p[((8, 32), 'split')][0][FWD_SPLIT] == 3 and p[((8, 32), 'split')][1] == 0
    assert p[((8, 32), 'split')][2][DG_SPLIT] == 3 and p[((8, 32), 'split-dgrad64-off')][2][DG_SPLIT] == 2
    for s in B_SIZES:
        for r in ('no-fused-pool', 'direct', 'bf16', 'bf16-full'):
            assert p[(s, r)][1] == 2 and p[(s, r)][3] == 2
    assert p[((8, 32), 'default-splitk')][1] == 2 and p[((9, 13), 'default-splitk')][1] == 0  # (9 x 13: hw % 4 != 0, no split-K)


# ------------------------------------------------------------------------------------------ C. Gram, every launch plan
GRAM_C = [64, 128, 200, 512, 48]
# hw = 32; hw = 35 (hw % 32 != 0: the register-staged kernel); whole 32-pixel steps (the LDS-DMA pipeline); a ragged last step;
# (66, 64): hw = 33 x 128, the smallest at which a plan can have more than 32 splits (a slab is at least 128 pixels)
GRAM_SHAPES = [(8, 4), (5, 7), (32, 64), (37, 50), (66, 64)]
MANY = {'ST2_GRAM_BLOCKS': '8192', 'ST2_GRAM_BLOCKS64': '8192'}
GRAM_PLANS = [('default', {}, 0), ('no-dma', {'ST2_GRAM_DMA': '0'}, 0), ('one-block', {'ST2_GRAM_BLOCKS': '1', 'ST2_GRAM_BLOCKS64': '1'}, 0),
              ('many-blocks', MANY, 0), ('many-blocks-two-stage', dict(MANY, ST2_GRAM_REDUCE='2'), 0),
              ('split', {}, 1), ('split-many-blocks', MANY, 1)]
GRAM_ENV = sorted({k for _, env, _ in GRAM_PLANS for k in env})
MEAN = np.array((123.68, 116.779, 103.939), F32)


def gram_splits(c, hw, env):
    """gram.hip's gram_plan: the number of K slabs."""
    bt = 128 if c > 64 else 64
    t = -(-c // bt)
    tiles = t * (t + 1) // 2
    want = int(env.get('ST2_GRAM_BLOCKS', 512)) // tiles if bt == 128 else -(-int(env.get('ST2_GRAM_BLOCKS64', 1024)) // tiles)
    want = max(1, min(want, -(-hw // 128)))
    kslab = -(-(-(-hw // want)) // 32) * 32
    return -(-hw // kslab)


def style_image(x):
    """The HWC float32 image whose preprocessing (x - mean, float32) is EXACTLY the integer image x (3, h, w): k + mean lies in
    mean's binade [64, 128) for |k| <= 2, so the sum is representable and the kernel's subtraction exact."""
    img = (np.asarray(x, F32) + MEAN.reshape(3, 1, 1)).astype(F32)
    assert np.array_equal(img - MEAN.reshape(3, 1, 1), np.asarray(x, F32))
    return np.ascontiguousarray(img.transpose(1, 2, 0))


@pytest.mark.parametrize('h,w', GRAM_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('c', GRAM_C)
def test_gram_is_exact_on_every_launch_plan(c, h, w, monkeypatch):
    """conv1_1 (3 -> C) with an integer blob <= 13: engine.gram must equal float32(exact sum) / float32(C h w) -- one IEEE division
    of an exact integer -- and be exactly symmetric, on the default plan, without the LDS-DMA pipeline, with one slab, with as many
    slabs as the shape allows (more than 32 at 66 x 64: the one-launch wide reduction, and ST2_GRAM_REDUCE=2, the two-stage one), and
    on the split-operand kernel where it takes the shape (C % 64 == 0 and C >= 128; elsewhere the fp32 kernel must run).  The style
    targets of st_set_style, under fp32 and bf16, are the same numbers."""
    topo, params, x = eo.gram_recipe(c, h, w)
    blobs = eo.ExactNet(topo, params, paths=('direct', 'split')).forward(x)
    for blob in blobs.values():
        eo.assert_gram_domain(blob.reshape(blob.shape[0], -1))
    want = {name: eo.gram_exact(blob) for name, blob in blobs.items()}
    if (h, w) == (66, 64):
        assert gram_splits(c, h * w, MANY) > 32
    gpu = st2.HipModel(eo.params32(params), topology=topo)
    f = gpu.forward(x4(x), ['conv1_1'])
    assert_equal(f['conv1_1'], blobs['conv1_1'], 'conv1_1')
    for plan, env, algo in GRAM_PLANS:
        for k in GRAM_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        gpu.engine.set_gram_algo(algo)
        for name in ('data', 'conv1_1'):
            gpu.engine.profile_enable(True)
            g = gpu.engine.gram(name)
            prof = launches(gpu.engine, 'gram_partial')
            split = algo == 1 and name == 'conv1_1' and c % 64 == 0 and c >= 128
            assert prof == collections.Counter({'gram_partial_split_bf16x6' if split else 'gram_partial_mfma_f32': 1}), (plan, name, prof)
            assert g.dtype == F32 and np.array_equal(g, want[name]), '%s %s: %d entries differ from float32(exact sum) / float32(C h w)' % (
                plan, name, int((g != want[name]).sum()))
            assert np.array_equal(g, g.T), (plan, name)
    for k in GRAM_ENV:
        monkeypatch.delenv(k, raising=False)
    gpu.engine.set_gram_algo(0)
    gpu.engine.close()
    for precision in ('fp32', 'bf16'):
        e = st2.HipModel(eo.params32(params), topology=topo, precision=precision).engine
        e.set_style(style_image(x))
        for name in ('data', 'conv1_1'):
            assert np.array_equal(e.style_gram(name), want[name]), (precision, name)
        e.close()


@pytest.mark.parametrize('h,w', GRAM_SHAPES[:4], ids=lambda v: str(v))
@pytest.mark.parametrize('c', GRAM_C)
def test_raw_sums_of_a_tile_sharded_style_pass_are_exact(c, h, w):
    """st_tile_style_partials on a 2 x 2 grid of the style image: every rank's buffer holds the raw, un-normalised sums of F F^T over
    ITS tile's region of every blob -- exact integers, equal to the exact sums over that region of the whole-image forward -- and
    the four buffers add up to the whole-image sums."""
    topo, params, x = eo.gram_recipe(c, h, w)
    blobs = eo.ExactNet(topo, params, paths=('direct', 'split')).forward(x)
    for blob in blobs.values():
        eo.assert_gram_domain(blob.reshape(blob.shape[0], -1))
    grid = tiling.TileGrid(h, w, 2, 2, topo, 1)
    image = style_image(x)
    e = st2.HipModel(eo.params32(params), topology=topo).engine
    total = np.zeros(9 + c * c)
    for win, tile in zip(grid.windows, grid.tiles):
        e.profile_enable(True)
        ptr, n = e.tile_style_partials(np.ascontiguousarray(image[win.y0:win.y1, win.x0:win.x1]), (h, w), (win.y0, win.x0),
                                       (tile.y0, tile.x0, tile.y1, tile.x1), last='conv1_1')
        assert launches(e, 'gram_partial') == collections.Counter({'gram_partial_mfma_f32': 2})
        assert n == 9 + c * c
        got = dev_tensor(ptr, (n,), 'cuda:0').cpu().numpy().astype(np.float64)
        want = np.concatenate([eo.gram_sums_exact(blobs[name][:, tile.y0:tile.y1, tile.x0:tile.x1]).ravel() for name in ('data', 'conv1_1')])
        assert_equal(got, want, 'raw sums of tile %s' % ((tile.y0, tile.x0, tile.y1, tile.x1),))
        total += got
    assert_equal(total, np.concatenate([eo.gram_sums_exact(blobs[name]).ravel() for name in ('data', 'conv1_1')]), 'the four tiles together')
    e.close()
