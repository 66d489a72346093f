"""Call sequences against the engine's test hooks, and the oracle that runs beside them.  TEST INFRASTRUCTURE.

The engine keeps ONE activation set, which every evaluation overwrites and which different evaluations leave in different states
(every fp32 blob; the lean fp32 forward of an iteration; the lean bf16 flow; a ranged forward; nothing valid).  After any state
changing call (a *preparer*) a hook -- get_blob, gram, backward, opfunc -- must either answer for the image the activations belong
to, within the bar the suite already uses for that quantity, or raise StError naming the blob or the state.

This module holds what needs no GPU (jobs, image pool, the two seeded walks, the separation of successive inputs) and the
``Runner`` that executes a walk on an engine with the CPU oracle beside every call (tests/test_gpu_call_sequences.py).

"The image the activations belong to" is the input of the evaluation that last filled them: the probe image of a forward, the
iterate an objective evaluation read (for an Adam step the iterate BEFORE the update, for an L-BFGS step the one after it, which
is where its last evaluation runs).  The opfunc hook is held to the iterate itself.
"""

import collections
import functools
import os
import sys

import numpy as np

import oracle
from avepool_oracle import AveNetOracle, avepool_forward, is_ave
from oracle.caffe_net import bf16_round, conv3x3_forward, maxpool_forward

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from make_route_fingerprints import MIXED, NETS as ROUTE_NETS, PARAMS4      # noqa: E402

F32 = np.float32
SEED = 20240917                     # of both walks

# ------------------------------------------------------------------------------------------ jobs
PATHS = (('fp32', 0), ('fp32', 1), ('fp32', 2), ('bf16', 1), ('bf16-full', 1))
# net A: the route grid's MIXED topology (max and average pools, a 64 -> 20 -> 128 conv, pooled first convs) at even levels and at
# odd levels one past a 64 edge; net B: VGG19 to conv3_3
JOBS = (('A', 20, 28), ('A', 33, 65), ('B', 24, 40))
TOPOLOGY = {'A': MIXED, 'B': tuple(oracle.VGG19_TOPOLOGY[:9])}
# the route grid's `pools` table (both nets have its blobs): content on data and a pool blob, style on a pool blob and a conv --
# conv1_2 and conv2_2 are pooled, un-weighted layers (dead in a lean evaluation), conv3_1 is live
MAIN_TABLE = dict(ROUTE_NETS['mixed'][1])['pools']
# ... and one whose deepest weighted blob is another (pool2 instead of conv3_1)
ALT_TABLE = {'content': {'conv2_2': 0.1}, 'style': {'conv1_2': 1, 'pool2': 1}, 'deepdream': {}}
MID = 'conv2_2'                                         # where the ranged forward stops
BACKWARDS = (('conv3_1', 'pool1', 'data'), ('conv2_1',))  # diffs at the deepest weighted conv, a pool blob and data; at a conv alone
OTHER_PATH = {'fp32': 'bf16', 'bf16': 'fp32', 'bf16-full': 'fp32'}


def other_size(h, w):
    return h - 4, w + 4


def split_layers(net, h, w):
    """The convs of the net whose forward conv algorithm 2 runs on the split-operand kernel at an h x w input (the predicate of
    tests/test_gpu_edge_sizes.py: K % 16 == 0, M % 64 == 0, width % 4 == 0, and what Winograd needs: K % 8 == 0, M >= 48)."""
    out = []
    for layer in TOPOLOGY[net]:
        if layer[0] != 'conv':
            h, w = oracle.caffe_net.pooled_size(h), oracle.caffe_net.pooled_size(w)
        elif layer[2] % 16 == 0 and layer[3] % 64 == 0 and w % 4 == 0:
            out.append(layer[1])
    return out


def cases():
    """(path, algo, net, h, w): algorithm 2 only where the split kernel takes at least one layer."""
    return [(p, a, n, h, w) for p, a in PATHS for n, h, w in JOBS if a != 2 or split_layers(n, h, w)]


@functools.lru_cache(None)
def net_params(net):
    return oracle.he_init_weights(TOPOLOGY[net], seed=3 if net == 'A' else 4, bias_std=0.2)


def net_oracle(net, bf16=False):
    return AveNetOracle(TOPOLOGY[net], net_params(net), operands='bf16' if bf16 else 'fp32')


# ------------------------------------------------------------------------------------------ images
N_IMAGES = 5


def image(k, h, w, target=False):
    """Image k of the pool (uint8, h x w x 3); target=True: its counterpart for the content / style slots, the same picture turned
    by 180 degrees from other noise (an iterate equal to the content image would make the content norm zero).  The five differ in their statistics, not only in their pixels, so that every blob,
    every Gram and the backward of fixed diffs differ by tenths between any two of them: two noise images of the same
    distribution have nearly the same Gram.  All carry noise: flat regions would fill the pooling windows with near-ties, which two
    correct forwards break differently."""
    k %= N_IMAGES
    rs = np.random.RandomState(100 + k + (50 if target else 0))
    yy, xx = np.mgrid[0:h, 0:w]
    if k == 0:                                              # full-range noise
        img = rs.randint(0, 256, (h, w, 3))
    elif k == 1:                                            # smooth diagonal ramp, warm tint
        ramp = (xx / max(w - 1, 1) + yy / max(h - 1, 1)) / 2
        img = np.stack([40 + 215 * ramp, 20 + 120 * ramp, 90 * ramp ** 2], -1) + rs.randint(0, 24, (h, w, 3))
    elif k == 2:                                            # noise with half its pixels dark
        img = rs.randint(0, 256, (h, w, 3)) * (rs.rand(h, w, 1) < 0.5)
    elif k == 3:                                            # bright, low contrast, blue tint, vertical stripes
        img = np.stack([150 + 20 * ((xx // 3) % 2), 200 + 0 * xx, 215 - 30 * ((xx // 3) % 2)], -1) + rs.randint(0, 40, (h, w, 3))
    else:                                                   # dark checkerboard with a bright green block
        img = np.stack([60 * ((xx + yy) % 2), 30 + 0 * xx, 90 * ((xx // 2 + yy // 2) % 2)], -1) + rs.randint(0, 40, (h, w, 3))
        img[h // 4:h // 2 + 1, w // 3:] += np.array([0, 190, 20])
    img = np.clip(img, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[::-1, ::-1]) if target else img


@functools.lru_cache(None)
def _shapes(net):
    return net_oracle(net)


def fixed_diffs(net, h, w, names):
    cpu = _shapes(net)
    return {n: np.random.RandomState(7 + len(n) + len(names)).randn(1, *cpu.blob_shape(n, h, w)).astype(F32) for n in names}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def sym_sep(a, b):
    """rel-L2 distance, by the larger of the two norms (symmetric; a stale answer is held against either as the reference)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b), 1e-30))


def snapshot(cpu, net, h, w, x):
    """Everything the act hooks may be asked for at input x: {('blob', n) / ('gram', n) / ('backward', i): array}."""
    names = cpu.layers()
    f = cpu.forward(x, names)
    out = {}
    for n in names:
        out['blob', n] = f[n].copy()
        out['gram', n] = oracle.gram(f[n])
    for i, bw in enumerate(BACKWARDS):
        out['backward', i] = cpu.backward(fixed_diffs(net, h, w, bw))
    return out


SEPARATION = 0.1


def assert_separated(s0, s1, what):
    """Every blob, Gram and backward of two successive inputs differ by at least SEPARATION: an answer from the earlier state then
    misses any bar of the suite by orders of magnitude."""
    for key in s0:
        d = sym_sep(s0[key], s1[key])
        assert d >= SEPARATION, '%s: %s of the two inputs differ by only %.3g' % (what, key, d)


# ------------------------------------------------------------------------------------------ walks
PREPARERS = ('forward_all', 'forward_mid', 'opfunc_first', 'opfunc_second', 'step_adam', 'step_lbfgs', 'step_pipelined',
             'set_input', 'set_content', 'set_style', 'set_precision', 'set_algos', 'resample_input', 'set_weights')
HOOKS = ('get_blob', 'gram', 'backward', 'opfunc')
EVALUATORS = PREPARERS[:7]


def walk(kind, case_index):
    """The steps of a walk: each a tuple of preparers, followed by every hook.  'single': every preparer once, in a seeded order
    of its own per case.  'pairs': the ordered pairs of different preparers, shuffled once with SEED and dealt over the cases in
    turn, so that all cases together run every ordered pair (state is then left by the last two calls at least)."""
    n_cases = len(cases())
    if kind == 'single':
        order = np.random.RandomState(SEED + case_index).permutation(len(PREPARERS))
        return [(PREPARERS[i],) for i in order]
    pairs = [(p, q) for p in PREPARERS for q in PREPARERS if p != q]
    order = np.random.RandomState(SEED).permutation(len(pairs))
    return [pairs[i] for i in order[case_index::n_cases]]


def case_id(case, kind):
    p, a, n, h, w = case
    return '%s-algo%d-net%s-%dx%d-%s' % (p, a, n, h, w, kind)


# ------------------------------------------------------------------------------------------ the runner (GPU)
FWD_SPLIT, DG_SPLIT = 'conv3x3_fwd_wino_split_bf16x6', 'conv3x3_dgrad_wino_split_bf16x6'


class Refused(Exception):
    pass


class Runner:
    """One job on one path: the engine (through StyleTransfer / HipModel), the oracle mirroring every evaluation (so that the
    norms are captured at the same images), and the checks after every step of a walk."""

    def __init__(self, case):
        import style_transfer2_amd as st2
        self.st2 = st2
        self.precision, self.algo, self.net, self.h, self.w = case
        self.bf16 = self.precision != 'fp32'
        self.topo = TOPOLOGY[self.net]
        self.params = net_params(self.net)
        self.names = ['data'] + [l[1] for l in self.topo]
        self.model = st2.HipModel(self.params, topology=self.topo, precision=self.precision, conv_algo=self.algo)
        self.eng = self.model.engine
        self.dev = st2.StyleTransfer(self.model)
        self.net_cpu = net_oracle(self.net, self.bf16)
        self.cpu = oracle.TransferOracle(net_oracle(self.net, self.bf16))
        self.k, self.kt = 0, 2                  # last image of the pool taken for an evaluation / for a content or style slot
        self.table = MAIN_TABLE
        self.conv_algo, self.gram_algo = self.algo, 0
        self.eval_algo = self.algo              # conv algorithm of the evaluation that filled the activations
        self.act_x = None                       # the image the activations belong to (None: nothing the oracle could answer for)
        self.act_hw = (self.h, self.w)
        self.prev_snap = None
        self.fresh = False                      # the last preparer evaluated an image of the pool that the one before had not
        self.calls = []                         # what ran, for the failure messages
        self.refusals = []                      # [(step label, hook, what was refused)]
        self.split_checked = False
        hw = (self.h, self.w)
        for st in (self.dev, self.cpu):
            st.set_input(image(0, *hw)); st.set_content(image(1, *hw, True)); st.set_style(image(2, *hw, True)); st.reset()
            st.set_weights({k: dict(v) for k, v in MAIN_TABLE.items()}, dict(PARAMS4))
        self._optimizer('adam')
        assert self.dev.start()

    def close(self):
        self.eng.close()

    # -- helpers
    def _next_image(self, hw=None, target=False):
        if target:                              # (a count of their own: successive evaluations stay neighbours in the pool)
            self.kt += 1
            return image(self.kt, *(hw or (self.h, self.w)), True)
        self.k += 1
        self.fresh = True                       # an evaluation of a new image follows
        return image(self.k, *(hw or (self.h, self.w)))

    def _optimizer(self, kind):
        cls = {'adam': self.st2.AdamOptimizer, 'lbfgs': self.st2.LBFGSOptimizer}[kind]
        self.dev.optimizer_cls = cls
        self.dev.step_size = 10 if kind == 'adam' else 1
        self.dev.optimizer = cls(self.eng, self.dev.opfunc, step_size=self.dev.step_size)       # (not reset(): the norms stay)

    def _job_size(self):
        """Back to the job's geometry (after resample_input) before anything that evaluates the objective."""
        if self.dev.input_shape != (1, 3, self.h, self.w):
            self.dev.set_input(image(self.k, self.h, self.w))

    def _evaluated(self, x):
        """The engine evaluated the objective at x: the oracle does, too (norm capture), and the activations are x's."""
        self.cpu.opfunc(x)
        self.act_x, self.act_hw, self.eval_algo = x, x.shape[2:], self.conv_algo

    def _set_input(self):
        self._job_size()
        self.dev.set_input(self._next_image())
        return self.eng.get_input_nchw()

    # -- preparers
    def forward_all(self, last=None):
        h, w = self.dev.input_shape[2:]             # (the iterate's geometry: a forward at another one re-creates its buffers)
        x = self.model.preprocess(self._next_image((h, w)))
        if self.conv_algo == 2 and not self.bf16 and (h, w) == (self.h, self.w) and last is None:
            self.eng.profile_enable(True)
            self.eng.forward(x, last)
            got = self.eng.profile_read().get(FWD_SPLIT, {}).get('launches', 0)
            self.eng.profile_enable(False)
            want = split_layers(self.net, h, w)
            assert got == len(want), 'conv algorithm 2: %d split-operand forward launches, expected %s' % (got, want)
            self.split_checked = True
        else:
            self.eng.forward(x, last)
        self.act_x, self.act_hw, self.eval_algo = x, (h, w), self.conv_algo

    def forward_mid(self):
        self.forward_all(MID)

    def opfunc_first(self):
        self._job_size()
        self.dev.reset(); self.cpu.reset()          # norms cleared on both sides
        self.opfunc_second()

    def opfunc_second(self):
        x = self._set_input()
        self._check_opfunc(x, 'the preparer itself')

    def step_adam(self):
        self._optimizer('adam')
        x = self._set_input()
        self.dev.step()
        self._evaluated(x)

    def step_lbfgs(self):
        self._optimizer('lbfgs')
        x = self._set_input()
        self.dev.step()
        self.cpu.opfunc(x)                          # (a fresh history: the step evaluates at x, moves, evaluates again)
        self._evaluated(self.eng.get_input_nchw())

    def step_pipelined(self):
        self._optimizer('adam')
        x = self._set_input()
        self.dev.step_begin()
        x1 = self.eng.get_input_nchw()              # the iterate the second iteration evaluates
        self.dev.step_begin()                       # ... begun before the first is collected
        self.dev.step_end(); self.dev.step_end()
        self.cpu.opfunc(x)
        self._evaluated(x1)

    def set_input(self):
        self._job_size()
        self.dev.set_input(self._next_image())
        self.fresh = False                          # (nothing evaluates it before the hooks)

    def set_content(self):
        img = self._next_image(target=True)
        self.dev.set_content(img); self.cpu.set_content(img)

    def set_style(self):
        img = self._next_image(target=True)
        self.dev.set_style(img); self.cpu.set_style(img)

    def set_precision(self):
        self.eng.set_precision(OTHER_PATH[self.precision])
        self.eng.set_precision(self.precision)

    def set_algos(self):
        self.conv_algo = {0: 1, 1: 0, 2: 1}[self.conv_algo]
        self.gram_algo = 1 - self.gram_algo
        self.eng.set_conv_algo(self.conv_algo); self.eng.set_gram_algo(self.gram_algo)

    def resample_input(self):
        self.dev.resample_input(other_size(self.h, self.w))

    def set_weights(self):
        self.table = ALT_TABLE if self.table is MAIN_TABLE else MAIN_TABLE
        for st in (self.dev, self.cpu):
            st.set_weights({k: dict(v) for k, v in self.table.items()}, dict(PARAMS4))

    def restore(self):
        """After the hooks of a step: the path's own algorithms, the main weight table, the job's geometry."""
        if (self.conv_algo, self.gram_algo) != (self.algo, 0):
            self.conv_algo, self.gram_algo = self.algo, 0
            self.eng.set_conv_algo(self.algo); self.eng.set_gram_algo(0)
        if self.table is not MAIN_TABLE:
            self.set_weights()
        self._job_size()

    # -- bars (each from the test the issue names)
    def _conv_bar(self, layer, width):
        """tests/test_gpu_edge_sizes.py, test_vgg19_at_tiny_and_thin_size (1): by the kernel class that ran."""
        _, name, cin, cout = layer
        if self.bf16 and cin % 8 == 0:
            return 3e-5
        if self.eval_algo == 2 and not self.bf16 and cin % 16 == 0 and cout % 64 == 0 and width % 4 == 0:
            return 2e-6
        return 1e-5

    def _backward_bar(self, adopted):
        """On the adopted forward state: fp32 3e-5, split 6e-6 (test_gpu_edge_sizes.py DG_BARS), bf16 the chain bar of
        test_bf16_chain_with_pools_and_injections.  Where the engine did not return a blob the backward passes (a lean evaluation),
        the oracle keeps its own ReLU masks and pool arg-max there and one decision taken the other way is a local O(1) difference:
        the end-to-end gradient bars of test_vgg19_at_tiny_and_thin_size (3) -- still a twentieth of SEPARATION at most."""
        if not adopted:
            return 5e-2 if self.bf16 else 5e-3
        return 2e-3 if self.bf16 else 6e-6 if self.conv_algo == 2 else 3e-5

    # -- hooks
    def _where(self, hook, what=''):
        return 'after %s: hook %s %s' % (' -> '.join(self.calls[-2:]), hook, what)

    def _try(self, fn):
        try:
            return fn()
        except self.st2.capi.StError as err:
            raise Refused(str(err))

    def hooks(self, label):
        """Every hook.  Returns nothing; the refusals are recorded, a wrong answer raises AssertionError."""
        snap = None
        if self.act_x is not None:
            snap = snapshot(self.net_cpu, self.net, *self.act_hw, self.act_x)
            # the input of this step's evaluation against that of the step before (what a stale answer would be of)
            if self.fresh and self.prev_snap is not None and self.prev_snap[0] == self.act_hw:
                assert_separated(self.prev_snap[1], snap, self._where('(oracle)'))
            self.prev_snap, self.fresh = (self.act_hw, snap), False
        self.eng._fwd_hw = self.act_hw              # (the shapes Engine.get_blob / gram / backward size their buffers by)
        refused = collections.OrderedDict((h, []) for h in HOOKS)
        got = {}
        for n in self.names:
            try:
                got[n] = self._try(lambda: self.eng.get_blob(n))
            except Refused as r:
                self._refusal_names(r, n, 'get_blob')
                refused['get_blob'].append(n)
        if got:
            assert snap is not None, self._where('get_blob', 'answers for %s although no evaluation is current' % sorted(got))
            self._check_blobs(got, snap)
        for n in self.names:
            try:
                g = self._try(lambda: self.eng.gram(n))
            except Refused as r:
                self._refusal_names(r, n, 'gram')
                refused['gram'].append(n)
                continue
            assert snap is not None, self._where('gram', 'of %s answers although no evaluation is current' % n)
            ref = oracle.gram(got[n]) if n in got else snap['gram', n]
            err = rel_l2(g, ref)
            assert err <= 1e-5, self._where('gram', 'of %s: rel-L2 %.3g against the oracle Gram of %s blob' % (n, err, 'the engine\'s' if n in got else 'the oracle\'s'))
        for i, bw in enumerate(BACKWARDS):
            diffs = fixed_diffs(self.net, *self.act_hw, bw)
            try:
                g = self._try(lambda: self.eng.backward(diffs))
            except Refused as r:
                assert any(w in str(r) for w in ('blob', 'forward')), self._where('backward', 'refuses without naming the blob or the state: %s' % r)
                refused['backward'].append('+'.join(bw))
                continue
            assert snap is not None, self._where('backward', 'of %s answers although no evaluation is current' % (bw,))
            self.net_cpu.forward(self.act_x, self.names[1:])
            self.net_cpu.adopt_forward_state(got)
            err = rel_l2(g, self.net_cpu.backward(diffs))
            top = max(self.names.index(n) for n in bw)
            bar = self._backward_bar(all(n in got for n in self.names[:top + 1]))
            assert err <= bar, self._where('backward', 'of diffs at %s: rel-L2 %.3g > %.1g' % (bw, err, bar))
        try:
            x = self._try(self.eng.get_input_nchw)
            self._check_opfunc(x, '')
        except Refused as r:
            assert any(w in str(r) for w in ('content', 'style', 'input')), self._where('opfunc', 'refuses without naming the state: %s' % r)
            refused['opfunc'].append('opfunc')
        for h, what in refused.items():
            if what:
                self.refusals.append((label, h, ' '.join(what)))

    def _refusal_names(self, r, name, hook):
        idx = self.names.index(name)
        assert ('blob %d' % idx) in str(r), self._where(hook, 'of %s refuses without naming the blob: %s' % (name, r))

    def _check_blobs(self, got, snap):
        assert 'data' in got and np.array_equal(got['data'], self.act_x), self._where('get_blob', 'of data is not the image the activations belong to')
        below, gap_bar, broken = got['data'][0], 0.0, False          # the nearest blob below that the engine returned
        for k, layer in enumerate(self.topo):
            name = layer[1]
            if layer[0] == 'conv':
                wgt, b = self.params[name]
                r16 = self.bf16 and layer[2] % 8 == 0
                ref = np.maximum(conv3x3_forward(bf16_round(below) if r16 else below, bf16_round(wgt) if r16 else wgt, b), 0)
                bar = gap_bar + self._conv_bar(layer, below.shape[2])
            else:
                ref = avepool_forward(below) if is_ave(layer) else maxpool_forward(below)[0]
                bar = gap_bar
            if name in got:
                g = got[name][0]
                if broken and self.bf16:
                    # blobs between were not returned and the bf16 roundings of two correct chains part: the forward bar of
                    # test_bf16_chain_with_pools_and_injections, against the oracle's own chain
                    err = rel_l2(g, snap['blob', name][0])
                    assert err <= 1e-3, self._where('get_blob', 'of %s: rel-L2 %.3g > 1e-3 (oracle chain)' % (name, err))
                elif bar == 0.0:
                    assert np.array_equal(g, ref), self._where('get_blob', 'of %s: not the pooling of the engine\'s own blob below, bit for bit' % name)
                else:
                    # (a blob above blobs the engine did not return: one layer's bar per layer on the way from the last returned one)
                    err = rel_l2(g, ref)
                    assert err <= bar, self._where('get_blob', 'of %s: rel-L2 %.3g > %.1g' % (name, err, bar))
                below, gap_bar, broken = g, 0.0, False
            else:
                below, gap_bar, broken = ref, bar, True

    def _check_opfunc(self, x, what):
        """tests/test_gpu_edge_sizes.py, test_vgg19_at_tiny_and_thin_size (3)."""
        from helpers import check_trace
        ld, gd = self._try(self.dev.opfunc)
        lo, go = self.cpu.opfunc(x)
        self.act_x, self.act_hw, self.eval_algo = x, x.shape[2:], self.conv_algo
        where = self._where('opfunc', what)
        tc, td = self.cpu.traces[-1].data, self.dev.traces[-1].data
        if self.bf16:
            assert np.isclose(ld, lo, rtol=1e-2), (where, ld, lo)
            assert rel_l2(gd, go) <= 5e-2, (where, rel_l2(gd, go))
            check_trace(list(tc), list(tc.values()), td, rtol=5e-2, skip=('time',) + tuple(k for k in tc if k.endswith('_grad')))
        else:
            assert np.isclose(ld, lo, rtol=1e-5), (where, ld, lo)
            assert rel_l2(gd, go) <= 5e-3, (where, rel_l2(gd, go))
            e = np.abs(gd - go)[0].max(0)
            assert np.mean(e > 1e-3 * np.abs(go).max()) <= 0.02, where
            check_trace(list(tc), list(tc.values()), td, rtol=2e-3)

    # -- a walk
    def run(self, steps):
        for i, step in enumerate(steps):
            for p in step:
                self.calls.append(p)
                getattr(self, p)()              # (act_x stays the last evaluation's image: whatever a hook still answers is held to it)
            self.hooks('%d:%s' % (i, '>'.join(step)))
            self.restore()
        return self.refusals
