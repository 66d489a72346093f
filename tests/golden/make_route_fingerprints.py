#!/usr/bin/env python3
"""Generates tests/golden/route_fingerprints.json: which kernels the engine launches for a grid of small jobs, as the profiler
reports it -- per class the number of launches and the FLOP / byte figures, whose formulas distinguish unpooling launches, mask
sources, fused style chunks and skipped outputs.  tests/test_gpu_routes.py runs the same cases (it imports this file for them) and
demands the same figures: a change that is meant to leave the routing alone is held to that.

The fixture is a record of a KNOWN-GOOD commit: run this on a checkout of that commit, on a box with an MI355X,

    python tests/golden/make_route_fingerprints.py --commit $(git rev-parse HEAD) [--out FILE]

and never on the tree a test run is about to judge.  Public Python API only.  The grid (all of it at small sizes; seconds):

  nets      VGG19 with max pools, VGG19 with `pool: AVE`, a short net that mixes both and has a conv (64 -> 20 -> 128) whose channel
            counts the Winograd and the bf16 kernels refuse
  paths     fp32 with conv algorithm 0 / 1 / 2, bf16 (lean), bf16-full
  sizes     256 x 256 (every level even), 96 x 132 (deeper levels odd), 75 x 100 (odd everywhere)
  tables    the bench's (five style layers + one content layer), one with weights on pool blobs and on `data`, one single deep layer
  calls     first opfunc (norms captured), second opfunc, an Adam step (lean fp32 inside the iteration); once per net / path / size
            the ranged hooks: forward to a middle blob, two backwards with diffs injected at two blobs, one of them a pool blob
  switches  each per-call environment switch at its non-default value, one at a time, bench table, on the paths it affects; the bf16
            ones also with the conv tile forced that pools and unpools (see SWITCHES); on the fp32 paths the split-operand Gram /
            style gradient (`gram_algo=1`: conv1_1's 64 channels and the mixed net's 20 are refused, odd sizes mix both GEMMs)
A call the engine refuses is recorded as its error and must be refused the same way.

The fixture keeps one digest per case (`digest`: of launches, FLOPs and bytes of every class; any difference in any figure changes
it), not the figures themselves: 1053 cases of a dozen classes are half a megabyte.  To see WHICH figure of a failing case moved, write
the figures of both commits with --figures FILE and compare the case in the two files.
"""
import argparse
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import style_transfer2_amd as st2                          # noqa: E402
from style_transfer2_amd.engine import VGG19_TOPOLOGY     # noqa: E402

F32 = np.float32
FIXTURE = os.path.join(HERE, 'route_fingerprints.json')


def digest(fingerprint):
    """Of one case's {class: [launches, flops, bytes]} (or {'error': ...}): exact in every figure (repr of the doubles)."""
    return hashlib.sha256(json.dumps(fingerprint, sort_keys=True, separators=(',', ':')).encode()).hexdigest()[:16]


def read_fixture(path=FIXTURE):
    """(commit, {case id: digest}); the file groups the calls of one job on one line."""
    with open(path) as f:
        d = json.load(f)
    return d['commit'], {'%s/%s' % (job, call): dg for job, calls in d['cases'].items() for call, dg in calls.items()}


def write_fixture(path, commit, cases):
    jobs = {}
    for k in sorted(cases):
        job, call = k.rsplit('/', 1)
        jobs.setdefault(job, {})[call] = digest(cases[k])
    with open(path, 'w') as f:
        f.write('{"commit": "%s",\n "cases": {\n' % commit)
        f.write(',\n'.join('  %s: %s' % (json.dumps(job), json.dumps(calls)) for job, calls in jobs.items()))
        f.write('\n }}\n')


def _ave(topo, which=None):
    return tuple(('pool', l[1], 'ave') if l[0] == 'pool' and (which is None or l[1] in which) else l for l in topo)


MIXED = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 64), ('pool', 'pool1'),
         ('conv', 'conv2_1', 64, 20), ('conv', 'conv2_2', 20, 128), ('pool', 'pool2', 'ave'),
         ('conv', 'conv3_1', 128, 256), ('conv', 'conv3_2', 256, 256), ('pool', 'pool3'),
         ('conv', 'conv4_1', 256, 256))


def _tables(style, content, deep):
    return (('bench', {'content': {content: 0.08}, 'style': {n: 1 for n in style}, 'deepdream': {}}),
            ('pools', {'content': {'data': 0.05, 'pool2': 0.1}, 'style': {'pool1': 1, 'conv3_1': 1}, 'deepdream': {}}),
            ('deep', {'content': {}, 'style': {deep: 1}, 'deepdream': {}}))


# name -> (topology, weight tables, blob of the ranged forward, the diffs of the two ranged backwards)
NETS = {
    'vgg19_max': (VGG19_TOPOLOGY, _tables(('conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1'), 'conv4_2', 'conv5_1'),
                  'conv4_2', (('conv4_2', 'pool2'), ('pool3', 'conv1_2'))),
    'vgg19_ave': (_ave(VGG19_TOPOLOGY), _tables(('conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1'), 'conv4_2', 'conv5_1'),
                  'conv4_2', (('conv4_2', 'pool2'), ('pool3', 'conv1_2'))),
    'mixed': (MIXED, _tables(('conv1_1', 'conv2_1', 'conv3_1', 'conv4_1'), 'conv3_2', 'conv4_1'),
              'conv4_1', (('conv4_1', 'pool1'), ('pool2', 'conv2_1'))),
}
PATHS = (('fp32', 0), ('fp32', 1), ('fp32', 2), ('bf16', 1), ('bf16-full', 1))
SIZES = ((256, 256), (96, 132), (75, 100))
PARAMS4 = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
# (switches at non-default values, the paths they can affect).  At these sizes the bf16 conv picks its smallest tile, which neither
# pools nor unpools: ST2_CONV16_CFG=0 forces the 64 x 256 pixel tile that does, alone and under the switches of those routes.
BF16, CFG0 = (('bf16', 1),), {'ST2_CONV16_CFG': '0'}
SWITCHES = (
    ({'ST2_POOL_AMAP': '0'}, (('fp32', 1), ('fp32', 2))),
    ({'ST2_WINO_UNPOOL': '0'}, (('fp32', 1),)),
    ({'ST2_WS_DGRAD64': '0'}, (('fp32', 2),)),
    ({'ST2_LEAN32': '0'}, (('fp32', 1), ('fp32', 2))),
    ({'ST2_MASK_BITS': '0'}, BF16),
    ({'ST2_STYLE_FUSE': '0'}, BF16),
    ({'ST2_CONV16_UNPOOL': '0'}, BF16),
    ({'ST2_CONV16_UNPOOL_MAXK': '512'}, BF16),
    (CFG0, BF16 + (('bf16-full', 1),)),
    (dict(CFG0, ST2_CONV16_UNPOOL='0'), BF16),
    (dict(CFG0, ST2_CONV16_UNPOOL_MAXK='512'), BF16),
    (dict(CFG0, ST2_MASK_BITS='0'), BF16),
    (dict(CFG0, ST2_STYLE_FUSE='0'), BF16),
)
GROUPS = [(net, prec, algo) for net in NETS for prec, algo in PATHS]

_models = {}


def _model(net):
    """One engine per net, switched between precisions and conv algorithms (the routes must not depend on what ran before)."""
    if net not in _models:
        rs = np.random.RandomState(0)
        params = {l[1]: ((rs.randn(l[3], l[2], 3, 3) * np.sqrt(2.0 / (9 * l[2]))).astype(F32), (rs.randn(l[3]) * 0.1).astype(F32))
                  for l in NETS[net][0] if l[0] == 'conv'}
        _models[net] = st2.HipModel(params, topology=NETS[net][0])
    return _models[net]


def _record(engine, call):
    """The profiler's account of one call: {class: [launches, flops, bytes]}, or {'error': message}."""
    engine.profile_enable(True)
    try:
        call()
        out = {k: [v['launches'], v['flops'], v['bytes']] for k, v in sorted(engine.profile_read().items())}
    except st2.capi.StError as err:
        out = {'error': re.sub(r'\s*\([^()]*:\d+\)$', '', str(err))}      # (without the source position of the failing call)
    engine.profile_enable(False)
    return out


def _job(model, size, weights):
    rs = np.random.RandomState
    h, w = size
    st = st2.StyleTransfer(model)
    st.set_input(rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))
    st.set_content(rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8))
    st.set_style(rs(2).randint(0, 256, (h, w, 3)).astype(np.uint8))
    st.reset()
    st.set_weights({k: dict(v) for k, v in weights.items()}, PARAMS4)
    st.optimizer_cls = st2.AdamOptimizer
    st.set_step_size(10)
    st.reset()
    assert st.start()
    return st


def _objective_calls(out, prefix, model, size, weights):
    st = _job(model, size, weights)
    out[prefix + '/opfunc1'] = _record(model.engine, st.opfunc)
    out[prefix + '/opfunc2'] = _record(model.engine, st.opfunc)
    out[prefix + '/step'] = _record(model.engine, st.step)


def run_group(net, precision, algo):
    """{case id: fingerprint} of every case of one net on one path."""
    topo, tables, mid, backs = NETS[net]
    model = _model(net)
    eng = model.engine
    eng.set_precision(precision)
    eng.set_conv_algo(algo)
    out = {}
    for h, w in SIZES:
        base = '%s/%s-algo%d/%dx%d' % (net, precision, algo, h, w)
        for tname, weights in tables:
            _objective_calls(out, '%s/%s/default' % (base, tname), model, (h, w), weights)
        for env, paths in SWITCHES:
            if (precision, algo) not in paths:
                continue
            assert not set(env) & set(os.environ), env
            os.environ.update(env)
            try:
                tag = ','.join('%s=%s' % kv for kv in sorted(env.items()))
                _objective_calls(out, '%s/bench/%s' % (base, tag), model, (h, w), tables[0][1])
            finally:
                for var in env:
                    del os.environ[var]
        if precision == 'fp32':
            eng.set_gram_algo(1)
            try:
                _objective_calls(out, '%s/bench/gram_algo=1' % base, model, (h, w), tables[0][1])
            finally:
                eng.set_gram_algo(0)
        # the ranged hooks
        x = (np.random.RandomState(h + w).randn(1, 3, h, w) * 40).astype(F32)
        out[base + '/hooks/forward_' + mid] = _record(eng, lambda: eng.forward(x, mid))
        for names in backs:
            diffs = {n: np.random.RandomState(7).randn(1, *eng.blob_shape(n, h, w)).astype(F32) for n in names}
            out[base + '/hooks/backward_' + '+'.join(names)] = _record(eng, lambda: eng.backward(diffs))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--commit', required=True, help='hash of the commit this checkout is at (recorded in the fixture)')
    ap.add_argument('--out', default=FIXTURE)
    ap.add_argument('--figures', default='', help='also write the figures themselves, per case, to this file (diagnosis; not committed)')
    args = ap.parse_args()
    cases = {}
    for group in GROUPS:
        cases.update(run_group(*group))
    write_fixture(args.out, args.commit, cases)
    if args.figures:
        with open(args.figures, 'w') as f:
            json.dump({'commit': args.commit, 'cases': cases}, f, indent=0, sort_keys=True)
    print('%d cases, %d refused -> %s' % (len(cases), sum('error' in v for v in cases.values()), args.out))


if __name__ == '__main__':
    main()
