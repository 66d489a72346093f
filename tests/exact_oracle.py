"""Integer-exact references for the conv, pool and Gram kernels.  TEST INFRASTRUCTURE.

Every other GPU test of the arithmetic kernels compares random floats with a float32 oracle under a bar.  Here the operands are small
INTEGERS: every product and every partial sum is then exactly representable in float32, every order of summation gives the same
float on every kernel (Winograd and split-operand kernels included), and the comparison is np.array_equal -- tolerance zero, nothing
to calibrate.  Integer data also produces in bulk what random floats never do: tied pooling windows (Caffe routes the diff to the
FIRST maximum of a row-major scan) and pre-activations of exactly zero (the ReLU mask is `> 0`).

Why the results are exact.  Let d be a layer's input and g_m the 3x3xK filter of output channel m, all integers, b the bias.

  direct   (fp32 and bf16 MFMA kernels) every term is an integer: any order of summation is exact when
           sum |g| |d| + |b| < 2^24; checked as  max|d| * max_m ||g_m||_1 + max|b| < 2^24.
  wino     (Winograd F(2x2,3x3), fp32)  U = G g G^T is formed on the host in double: its entries are multiples of 1/4 with
           |U| <= sum |g| over the 3x3.  V = B^T d B sums 4 inputs with signs; the output transform sums 9 positions.  Every
           intermediate is a multiple of 1/4 whose terms are bounded in absolute sum by 36 max|d| ||g_m||_1, so a sufficient
           condition for ANY order (split-K and its combine pass included) is  144 max|d| max_m ||g_m||_1 + max|b| < 2^24.
  split    (split-operand kernels: Winograd, conv1_1 forward, Gram)  the three-way bf16 split of an operand is exact, and the
           three dropped partial products all contain a third term, which is zero when the operand has at most 16 significant
           bits: 4 max|V| <= 16 max|d| < 2^16 and 4 max|U| <= 36 max|g| < 2^16, on top of the `wino` condition.
  bf16     (bf16 operand path)  inputs, weights and incoming diffs must be bf16-representable (integers of magnitude <= 256
           are); the fp32 accumulation is then exact under the `direct` condition.  Where the path STORES bf16 (the diff a bf16
           data-gradient conv reads) the reference applies oracle.caffe_net.bf16_round to the exact value: one rounding of an
           exact number, still bit-comparable.  Rounded integers are integers, so the sums below stay exact.
  Gram     raw sums  sum F_i F_j  are exact below 2^24; gram_reduce then does ONE IEEE division, sum / float(C h w) (the build
           uses no fast-math): the reference is np.float32(exact_sum) / np.float32(C h w), bit-equal for C h w < 2^24.

tests/test_exact_oracle_cpu.py checks the `wino` bound itself: a float32 Winograd emulation with a shuffled channel order, random
split-K parts and shuffled transform association reproduces the exact result on every recipe the GPU tests use, at their largest K.

On an MI355X every kernel reproduces these references bit for bit (tests/test_gpu_exact.py): no step was found to round inside this
domain, the matrix cores add such integers exactly.  Were a step to round legitimately, the recipe is narrowed until that step is
exact and the step is recorded here -- no tolerance is added.

assert_exact_domain asserts these conditions BEFORE anything is launched: a recipe that leaves the domain is an error of the
test, never a skip."""

import numpy as np

from oracle.caffe_net import bf16_round, maxpool_forward, pooled_size

F32 = np.float32
F64 = np.float64
LIMIT = float(2 ** 24)
PATHS = ('direct', 'wino', 'split', 'bf16')


# ------------------------------------------------------------------------------------------ data recipes
def int_image(rng, h, w, lo, hi, block=1):
    """(3, h, w) integers in [lo, hi], constant on block x block squares (block = 1: independent pixels)."""
    bh, bw = -(-h // block), -(-w // block)
    coarse = rng.randint(lo, hi + 1, (3, bh, bw))
    return np.repeat(np.repeat(coarse, block, axis=1), block, axis=2)[:, :h, :w].astype(F64)


def dense_weights(rng, cout, cin):
    """(cout, cin, 3, 3) uniform in {-1, 0, 1}."""
    return rng.randint(-1, 2, (cout, cin, 3, 3)).astype(F64)


def sparse_weights(rng, cout, cin, nz):
    """(cout, cin, 3, 3) with exactly nz taps of +-1 per filter, the rest zero."""
    w = np.zeros((cout, cin * 9), F64)
    for m in range(cout):
        w[m, rng.choice(cin * 9, nz, replace=False)] = rng.choice((-1.0, 1.0), nz)
    return w.reshape(cout, cin, 3, 3)


def int_bias(rng, cout, lo=-1, hi=1):
    return rng.randint(lo, hi + 1, cout).astype(F64)


def int_diff(rng, shape, lo=-2, hi=2):
    return rng.randint(lo, hi + 1, shape).astype(F64)


def params32(params):
    """{name: (w, b)} as the float32 arrays Engine.load_weights takes (integers: the conversion is exact)."""
    return {n: (w.astype(F32), b.astype(F32)) for n, (w, b) in params.items()}


# ------------------------------------------------------------------------------------------ the domain
def _is_integer(a):
    a = np.asarray(a, F64)
    return bool(np.all(a == np.rint(a)))


def bf16_representable(a):
    a = np.asarray(a, F32)
    return bool(np.array_equal(bf16_round(a), a))


def assert_exact_domain(path, d, g, b=None):
    """The sufficient conditions of the module docstring for one conv launch on `path`: d = its input (forward: the blob below;
    data gradient: the incoming diff), g = its filters with the OUTPUT channel first ((M, K, 3, 3); data gradient: w transposed),
    b = its bias or None.  AssertionError outside the domain."""
    assert path in PATHS, path
    d, g = np.asarray(d, F64), np.asarray(g, F64)
    bmax = float(np.abs(b).max()) if b is not None and np.size(b) else 0.0
    assert _is_integer(d) and _is_integer(g) and (b is None or _is_integer(b)), '%s: operands are not integers' % path
    dmax = float(np.abs(d).max()) if d.size else 0.0
    g1 = float(np.abs(g).reshape(g.shape[0], -1).sum(1).max())
    gmax = float(np.abs(g).max())
    direct = dmax * g1 + bmax
    wino = 144.0 * dmax * g1 + bmax
    if path in ('direct', 'bf16'):
        assert direct < LIMIT, '%s: max|d| ||g||_1 + |b| = %g >= 2^24' % (path, direct)
    if path in ('wino', 'split'):
        assert wino < LIMIT, '%s: 144 max|d| ||g||_1 + |b| = %g >= 2^24' % (path, wino)
    if path == 'split':
        assert 16.0 * dmax < 2 ** 16 and 36.0 * gmax < 2 ** 16, 'split: a transformed operand has more than 16 significant bits'
    if path == 'bf16':
        assert bf16_representable(d) and bf16_representable(g), 'bf16: an operand is not bf16-representable'


def assert_gram_domain(f):
    """Raw Gram sums of the integer features f (C, hw) stay below 2^24, and so does C hw (the divisor is then an exact float)."""
    f = np.asarray(f, F64)
    assert _is_integer(f), 'Gram operand is not integer'
    assert float(np.abs(f).max()) < 2 ** 16, 'Gram operand has more than 16 significant bits (split-operand kernel)'
    assert float((f * f).sum(1).max()) < LIMIT and f.size < LIMIT, 'Gram sums leave the exact range'


# ------------------------------------------------------------------------------------------ exact layers (float64 on integers)
def conv3x3_exact(x, w, b=None):
    """Cross-correlation, pad 1: (K, h, w) x (M, K, 3, 3) [+ (M,)] -> (M, h, w) in float64 (exact: integers far below 2^53)."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    k, h, wd = x.shape
    m = w.shape[0]
    xp = np.zeros((k, h + 2, wd + 2), F64)
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((m, h * wd), F64)
    for ky in range(3):
        for kx in range(3):
            out += w[:, :, ky, kx] @ xp[:, ky:ky + h, kx:kx + wd].reshape(k, h * wd)
    out = out.reshape(m, h, wd)
    if b is not None:
        out += np.asarray(b, F64).reshape(m, 1, 1)
    return out


def transposed_filters(w):
    """The data gradient as a forward conv: (M, K, 3, 3) -> (K, M, 3, 3), taps rotated by 180 degrees."""
    return np.ascontiguousarray(np.asarray(w, F64).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def conv3x3_dgrad_exact(dy, w):
    """dx[c, y, x] = sum_{m, ky, kx} w[m, c, ky, kx] dy[m, y - ky + 1, x - kx + 1]."""
    return conv3x3_exact(dy, transposed_filters(w))


def maxpool_exact(x):
    """Caffe MAX 2x2/2, ceil mode: (pooled float64, arg-max slot) -- the slot from oracle.caffe_net.maxpool_forward (first maximum)."""
    x = np.asarray(x, F64)
    pooled, slot = maxpool_forward(x.astype(F32))
    return pooled.astype(F64), slot


def maxpool_backward_exact(dy, slot, in_shape):
    c, h, w = in_shape
    ho, wo = dy.shape[1:]
    win = np.zeros((c, ho, wo, 4), F64)
    np.put_along_axis(win, slot[..., None], np.asarray(dy, F64)[..., None], axis=-1)
    full = win.reshape(c, ho, wo, 2, 2).transpose(0, 1, 3, 2, 4).reshape(c, 2 * ho, 2 * wo)
    return np.ascontiguousarray(full[:, :h, :w])


def gram_sums_exact(f):
    """sum over pixels of F F^T: f (C, ...) -> (C, C) float64."""
    f = np.asarray(f, F64).reshape(np.shape(f)[0], -1)
    return f @ f.T


def gram_exact(f):
    """What gram_reduce must store: float32(exact sum) / float32(C h w), one IEEE division."""
    s = gram_sums_exact(f)
    assert float(np.abs(s).max()) < LIMIT and np.size(f) < LIMIT
    return s.astype(F32) / F32(np.size(f))


# ------------------------------------------------------------------------------------------ tie / zero statistics of a pooled blob
def pool_tie_stats(pre):
    """Of the pre-activations `pre` (C, h, w) of a conv that a max pool follows: (share of the windows with a positive maximum in
    which the maximum is tied, share of ALL windows whose first and last maximiser differ, share of pre-activations exactly 0).
    Windows are those of the stored (post-ReLU) blob; clipped windows count with the elements they have."""
    pre = np.asarray(pre, F64)
    blob = np.maximum(pre, 0)
    c, h, w = blob.shape
    ho, wo = pooled_size(h), pooled_size(w)
    pad = np.full((c, 2 * ho, 2 * wo), -1.0)
    pad[:, :h, :w] = blob
    win = pad.reshape(c, ho, 2, wo, 2).transpose(0, 1, 3, 2, 4).reshape(c, ho, wo, 4)
    mx = win.max(-1)
    n_max = (win == mx[..., None]).sum(-1)
    first = np.argmax(win, -1)
    last = 3 - np.argmax(win[..., ::-1], -1)
    positive = mx > 0
    tied = float(((n_max > 1) & positive).sum()) / max(1, int(positive.sum()))
    return tied, float((first != last).mean()), float((pre == 0).mean())


def assert_tie_conditions(pre, what=''):
    """The conditions under which a pooled blob tests the first-maximum rule and the `> 0` mask at all."""
    tied, differ, zeros = pool_tie_stats(pre)
    assert tied >= 0.20, '%s: only %.1f %% of the positive-maximum windows are tied' % (what, 100 * tied)
    assert differ >= 0.10, '%s: first and last maximiser differ in only %.1f %% of the windows' % (what, 100 * differ)
    assert zeros >= 0.05, '%s: only %.1f %% of the pre-activations are exactly 0' % (what, 100 * zeros)
    return tied, differ, zeros


# ------------------------------------------------------------------------------------------ the exact network
class ExactNet:
    """oracle.NetOracle in float64 on integer data: forward (post-ReLU blobs, pre-activations, pool slots) and the ranged backward
    with per-blob diff injection, same semantics (an injected diff enters its layer unmasked; diff from above is masked by
    blob > 0).  `paths` names the kernels whose exactness conditions every conv launch must meet (assert_exact_domain, forward
    and data gradient); `bf16=True` rounds, as the bf16 path does, the diff that a data-gradient conv with cout % 8 == 0 reads."""

    def __init__(self, topology, params, paths=('direct', 'wino', 'split'), bf16=False):
        self.topology = tuple(topology)
        self.params = params
        self.paths = paths if callable(paths) else (paths,) if isinstance(paths, str) else tuple(paths)
        self.bf16 = bf16
        self.names = ['data'] + [layer[1] for layer in self.topology]
        self.blobs, self.pre, self.slots = {}, {}, {}

    def _paths_of(self, layer, direction):
        paths = self.paths(layer, direction) if callable(self.paths) else self.paths
        return (paths,) if isinstance(paths, str) else paths

    def forward(self, x):
        x = np.asarray(x, F64)
        self.blobs, self.pre, self.slots = {'data': x}, {}, {}
        for layer in self.topology:
            name = layer[1]
            if layer[0] == 'conv':
                w, b = self.params[name]
                for p in self._paths_of(layer, 'fwd'):
                    assert_exact_domain(p, x, w, b)
                self.pre[name] = conv3x3_exact(x, w, b)
                x = np.maximum(self.pre[name], 0)
            else:
                x, self.slots[name] = maxpool_exact(x)
            self.blobs[name] = x
        return self.blobs

    def backward(self, diffs):
        present = [i for i, n in enumerate(self.names) if n in diffs]
        g = None
        for i in range(max(present), 0, -1):
            layer = self.topology[i - 1]
            name = layer[1]
            if g is not None and layer[0] == 'conv':
                g = g * (self.blobs[name] > 0)
            if name in diffs:
                inj = np.asarray(diffs[name], F64).reshape(self.blobs[name].shape)
                g = inj.copy() if g is None else g + inj
            if layer[0] == 'conv':
                w = self.params[name][0]
                if self.bf16 and layer[3] % 8 == 0:
                    assert float(np.abs(g).max()) < LIMIT
                    g = bf16_round(g.astype(F32)).astype(F64)
                for p in self._paths_of(layer, 'dgrad'):
                    assert_exact_domain(p, g, transposed_filters(w))
                g = conv3x3_dgrad_exact(g, w)
            else:
                g = maxpool_backward_exact(g, self.slots[name], self.blobs[self.names[i - 1]].shape)
        if 'data' in diffs:
            inj = np.asarray(diffs['data'], F64).reshape(self.blobs['data'].shape)
            g = inj.copy() if g is None else g + inj
        assert float(np.abs(g).max()) < LIMIT
        return g


# ------------------------------------------------------------------------------------------ float32 Winograd emulation
_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], F64)
_G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], F64)
_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], F64)


def _shuffled_sum32(terms, rng):
    """float32 sum of the float32 arrays `terms` in a random order."""
    order = rng.permutation(len(terms))
    acc = terms[order[0]].astype(F32)
    for j in order[1:]:
        acc = (acc + terms[j].astype(F32)).astype(F32)
    return acc


def winograd_f32_emulation(x, w, b, rng):
    """conv3x3 (pad 1) as Winograd F(2x2,3x3) in float32: U = G g G^T formed in double and stored as float32 (as the host pack
    does), V = B^T d B and Y = A^T M A with a RANDOM association of their signed sums, the channel sum in a RANDOM order cut into
    random split-K parts that are added afterwards.  Inside the domain of assert_exact_domain('wino', ...) every such order gives
    the exact result; returns (M, h, w) float32."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    k, h, wd = x.shape
    m = w.shape[0]
    u = np.einsum('ia,mkab,jb->mkij', _G, w, _G)
    assert np.array_equal(u.astype(F32).astype(F64), u)
    u = u.astype(F32)
    th, tw = (h + 1) // 2, (wd + 1) // 2
    xp = np.zeros((k, 2 * th + 2, 2 * tw + 2), F32)
    xp[:, 1:h + 1, 1:wd + 1] = x
    # d[c, a, b, ty, tx]: the 4x4 input tile of output tile (ty, tx)
    d = np.empty((k, 4, 4, th, tw), F32)
    for a in range(4):
        for bb in range(4):
            d[:, a, bb] = xp[:, a:a + 2 * th:2, bb:bb + 2 * tw:2]
    v = np.empty((k, 4, 4, th, tw), F32)
    for i in range(4):
        for j in range(4):
            terms = [F32(_BT[i, a] * _BT[j, bb]) * d[:, a, bb] for a in range(4) for bb in range(4) if _BT[i, a] * _BT[j, bb] != 0]
            v[:, i, j] = _shuffled_sum32(terms, rng)
    order = rng.permutation(k)
    n_parts = int(rng.randint(1, 5))
    cuts = np.sort(rng.choice(np.arange(1, k), min(n_parts - 1, k - 1), replace=False)) if k > 1 and n_parts > 1 else []
    parts = []
    for chunk in np.split(order, cuts):
        acc = np.zeros((m, 4, 4, th, tw), F32)
        for c in chunk:
            acc += u[:, c, :, :, None, None] * v[c][None]
        parts.append(acc)
    mm = _shuffled_sum32(parts, rng)
    y = np.empty((m, 2 * th, 2 * tw), F32)
    for p in range(2):
        for q in range(2):
            terms = [F32(_AT[p, i] * _AT[q, j]) * mm[:, i, j] for i in range(4) for j in range(4) if _AT[p, i] * _AT[q, j] != 0]
            y[:, p::2, q::2] = _shuffled_sum32(terms, rng)
    y = y[:, :h, :wd]
    if b is not None:
        y = (y + np.asarray(b, F32).reshape(m, 1, 1)).astype(F32)
    return np.ascontiguousarray(y)


# ------------------------------------------------------------------------------------------ the recipes of the tests
HEAD_TOPOLOGY = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 64), ('pool', 'pool1'),
                 ('conv', 'conv2_1', 64, 128), ('conv', 'conv2_2', 128, 128), ('pool', 'pool2'))
HEAD_POOLED = ('conv1_2', 'conv2_2')            # the conv blobs a max pool follows
HEAD_INJECTIONS = ('pool2', 'conv2_2', 'pool1', 'conv1_2', 'data')


def layer_recipe(cin, cout, h, w):
    """One conv layer behind conv1_1: (topology, params, image (3, h, w), dy (cout, h, w)).  conv1_1 (3 -> cin) has 6 taps of +-1 per
    filter and the image values in [-2, 2], so its ReLU output stays <= 13; conv1_2 (cin -> cout) is dense in {-1, 0, 1} with a
    bias in [-3, 3]; dy in [-2, 2].  cin == 3: conv1_1 alone (3 -> cout), dense."""
    rng = np.random.RandomState((((cin * 1031 + cout) * 1031 + h) * 1031 + w) % (2 ** 32))
    if cin == 3:
        topo = (('conv', 'conv1_1', 3, cout),)
        params = {'conv1_1': (dense_weights(rng, cout, 3), int_bias(rng, cout, -3, 3))}
    else:
        topo = (('conv', 'conv1_1', 3, cin), ('conv', 'conv1_2', cin, cout))
        params = {'conv1_1': (sparse_weights(rng, cin, 3, 6), int_bias(rng, cin)),
                  'conv1_2': (dense_weights(rng, cout, cin), int_bias(rng, cout, -3, 3))}
    return topo, params, int_image(rng, h, w, -2, 2), int_diff(rng, (cout, h, w))


def head_recipe(h, w):
    """The VGG head with ties and zeros in bulk: (params, image, diffs, seed).  Every filter has 3 taps of +-1, biases in
    {-1, 0, 1}, the image values in [-1, 1] constant on 4 x 4 blocks, integer diffs in [-2, 2] at HEAD_INJECTIONS.  The seed is
    the first one whose pooled conv blobs meet assert_tie_conditions (a seed that misses them is replaced, never skipped)."""
    for seed in range(32):
        rng = np.random.RandomState(seed * 10007 + h * 101 + w)
        params = {}
        for _, name, cin, cout in (l for l in HEAD_TOPOLOGY if l[0] == 'conv'):
            params[name] = (sparse_weights(rng, cout, cin, 3), int_bias(rng, cout))
        x = int_image(rng, h, w, -1, 1, block=4)
        net = ExactNet(HEAD_TOPOLOGY, params)
        net.forward(x)
        try:
            for name in HEAD_POOLED:
                assert_tie_conditions(net.pre[name], name)
        except AssertionError:
            continue
        diffs = {n: int_diff(rng, net.blobs[n].shape) for n in HEAD_INJECTIONS}
        return params, x, diffs, seed
    raise AssertionError('no seed below 32 meets the tie conditions at %d x %d' % (h, w))


def gram_recipe(c, h, w):
    """A single conv1_1 (3 -> c) with an integer blob <= 13: (topology, params, image)."""
    rng = np.random.RandomState(((c * 1031 + h) * 1031 + w) % (2 ** 32))
    topo = (('conv', 'conv1_1', 3, c),)
    return topo, {'conv1_1': (sparse_weights(rng, c, 3, 6), int_bias(rng, c))}, int_image(rng, h, w, -2, 2)
