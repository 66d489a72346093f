#!/usr/bin/env python3
"""The style statistics on the fp32 matrix cores (st_set_gram_algo 0) against the split-operand kernels (1), same process, same
device, same weights and images, on the headline job (1024^2, VGG19 to conv5_1, content + 5 style layers, Adam, bench.py's seeded
inputs): iterations per second with bench.py's timed-region contract (W untimed steps, then blocks of exactly K device-resident steps
bracketed by device synchronisation; the two contexts' blocks alternate; median over blocks), and, from a profiled run of both
afterwards, the ms per step of the Gram and style-gradient launch classes.  Once under conv algorithm 1 and once under 2.

    python tools/bench_gram_algo.py
    python tools/bench_gram_algo.py --style-layers conv1_1        # one style layer only: the per-layer A/B (C = 64 is HBM-bound)
One JSON line per conv algorithm."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CLASSES = {'gram': ('gram_partial_mfma_f32', 'gram_partial_split_bf16x6'), 'gram_reduce': ('gram_reduce',),
           'style_grad': ('style_grad_mfma_f32', 'style_grad_split_bf16x6')}


def make_job(inputs, conv_algo, gram_algo):
    import style_transfer2_amd as st2
    from style_transfer2_amd import weights as st2_weights
    import bench
    content, style, init, weights, params = inputs
    model = st2.HipModel(st2_weights.he_normal(st2.VGG19_TOPOLOGY, seed=0), conv_algo=conv_algo, gram_algo=gram_algo)
    job = st2.StyleTransfer(model)
    job.set_weights(weights, params)
    job.set_input(init)
    job.set_content(content)
    job.set_style(style)
    job.optimizer_cls = st2.AdamOptimizer
    job.set_step_size(bench.STEP_SIZES['adam'])
    job.reset()
    assert job.start()
    return job


def class_ms(job, solo, steps):
    """ms per step of the style classes over `steps` profiled steps (events around every launch: not the timed run)."""
    from style_transfer2_amd import distributed as st2_dist
    job.engine.profile_enable(True)
    job.engine.profile_read()
    st2_dist.timed_region(solo, job.step_async, steps, 0, job.engine.sync)
    prof = job.engine.profile_read()
    job.engine.profile_enable(False)
    out = {k: sum(prof.get(n, {}).get('ms', 0.0) for n in names) / steps for k, names in CLASSES.items()}
    out['gram_plus_style_grad'] = out['gram'] + out['style_grad']
    return {k: round(v, 4) for k, v in out.items()}


def leg(conv_algo, size, steps, warmup, blocks, style_layers):
    from style_transfer2_amd import distributed as st2_dist
    import bench
    weights = bench.WEIGHTS
    if style_layers:
        weights = dict(weights, style={k: v for k, v in weights['style'].items() if k in style_layers})
        assert weights['style'], 'no such style layer in the headline job'
    inputs = bench.images(size) + (weights, bench.PARAMS)
    solo = st2_dist.Group.__new__(st2_dist.Group)
    solo.rank, solo.local_rank, solo.world, solo.dist, solo.device = 0, 0, 1, None, None
    jobs = {0: make_job(inputs, conv_algo, 0), 1: make_job(inputs, conv_algo, 1)}
    try:
        for job in jobs.values():                 # warm-up of both before any timed block
            st2_dist.timed_region(solo, job.step_async, 0, warmup, job.engine.sync)
        times = {k: [] for k in jobs}
        for _ in range(blocks):
            for k, job in jobs.items():
                times[k].append(st2_dist.timed_region(solo, job.step_async, steps, 0, job.engine.sync))
        rate = {k: steps / statistics.median(v) for k, v in times.items()}
        ms = {k: class_ms(job, solo, steps) for k, job in jobs.items()}
        return {'conv_algo': conv_algo, 'size': [size, size], 'style_layers': sorted(weights['style']), 'steps': steps, 'warmup': warmup,
                'blocks': blocks, 'unit': 'it/s', 'gram_algo_0': rate[0], 'gram_algo_1': rate[1], 'algo_1_over_0': rate[1] / rate[0],
                'block_ms': {'gram_algo_%d' % k: [round(1e3 * t, 3) for t in v] for k, v in times.items()},
                'class_ms_per_step': {'gram_algo_%d' % k: v for k, v in ms.items()},
                'algos_in_force': {'gram_algo_%d' % k: list(job.engine.algos()) for k, job in jobs.items()}}
    finally:
        for job in jobs.values():
            job.engine.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--conv-algos', default='1,2')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--style-layers', default='', help='comma-separated subset of the job\'s style layers (default: all five)')
    args = ap.parse_args(argv)
    layers = [s for s in args.style_layers.split(',') if s]
    for ca in args.conv_algos.split(','):
        print(json.dumps(leg(int(ca), args.size, args.steps, args.warmup, args.blocks, layers)), flush=True)


if __name__ == '__main__':
    main()
