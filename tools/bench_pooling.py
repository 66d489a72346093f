#!/usr/bin/env python3
"""VGG19 with MAX pools against the same net with AVE pools (prototxt ``pool: AVE``), same process, same device, same weights and
images: steady-state iterations per second of both, with bench.py's timed-region contract (W untimed steps, then blocks of exactly
K device-resident steps bracketed by device synchronisation; median over blocks).  The two nets' blocks alternate, so drift of the
clock or of other work on the box falls on both.

    python tools/bench_pooling.py                       # both default legs
    python tools/bench_pooling.py --legs adam-fp32-1024 --steps 20 --blocks 3
    python tools/bench_pooling.py --pool-algo           # a third job per leg: AVE pools fused into the bf16 conv launches (st_set_pool_algo 1)
One JSON line per leg.  With --pool-algo the line also carries, per job, the milliseconds per step of every launch class over one more
block of profiled steps (events around every launch: not the timed run)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# (optimizer, precision, conv algorithm, size)
LEGS = {'adam-fp32-1024': ('adam', 'fp32', 1, 1024), 'lbfgs-bf16-2048': ('lbfgs', 'bf16', 1, 2048)}


def ave_topology(topo):
    return tuple(('pool', l[1], 'ave') if l[0] == 'pool' else l for l in topo)


def make_job(topology, inputs, optimizer, precision, conv_algo, pool_algo=None):
    import style_transfer2_amd as st2
    from style_transfer2_amd import weights as st2_weights
    import bench
    content, style, init, weights, params = inputs
    model = st2.HipModel(st2_weights.he_normal(topology, seed=0), topology=None if topology == st2.VGG19_TOPOLOGY else topology,
                         precision=precision, pool_algo=pool_algo)
    if conv_algo != 1:
        model.engine.set_conv_algo(conv_algo)
    job = st2.StyleTransfer(model)
    job.set_weights(weights, params)
    job.set_input(init)
    job.set_content(content)
    job.set_style(style)
    job.optimizer_cls = {'adam': st2.AdamOptimizer, 'lbfgs': st2.LBFGSOptimizer}[optimizer]
    job.set_step_size(bench.STEP_SIZES[optimizer])
    job.reset()
    assert job.start()
    return job


def class_ms(job, solo, steps):
    """ms per step of every launch class over `steps` profiled steps."""
    from style_transfer2_amd import distributed as st2_dist
    job.engine.profile_enable(True)
    job.engine.profile_read()
    st2_dist.timed_region(solo, job.step_async, steps, 0, job.engine.sync)
    prof = job.engine.profile_read()
    job.engine.profile_enable(False)
    return {k: round(v['ms'] / steps, 4) for k, v in sorted(prof.items())}


def leg(name, steps, warmup, blocks, pool_algo=False):
    import style_transfer2_amd as st2
    from style_transfer2_amd import distributed as st2_dist
    import bench
    optimizer, precision, algo, size = LEGS[name]
    inputs = bench.images(size) + (bench.WEIGHTS, bench.PARAMS)
    solo = st2_dist.Group.__new__(st2_dist.Group)
    solo.rank, solo.local_rank, solo.world, solo.dist, solo.device = 0, 0, 1, None, None
    jobs = {'max': make_job(st2.VGG19_TOPOLOGY, inputs, optimizer, precision, algo),
            'ave': make_job(ave_topology(st2.VGG19_TOPOLOGY), inputs, optimizer, precision, algo)}
    if pool_algo:
        jobs['ave_fused'] = make_job(ave_topology(st2.VGG19_TOPOLOGY), inputs, optimizer, precision, algo, pool_algo=1)
    try:
        for job in jobs.values():                 # warm-up of both before any timed block
            st2_dist.timed_region(solo, job.step_async, 0, warmup, job.engine.sync)
        times = {k: [] for k in jobs}
        for _ in range(blocks):
            for k, job in jobs.items():
                times[k].append(st2_dist.timed_region(solo, job.step_async, steps, 0, job.engine.sync))
        rate = {k: steps / statistics.median(v) for k, v in times.items()}
        out = {'leg': name, 'optimizer': optimizer, 'precision': precision, 'conv_algo': algo, 'size': [size, size],
               'steps': steps, 'warmup': warmup, 'blocks': blocks, 'unit': 'it/s',
               'max_pool': rate['max'], 'ave_pool': rate['ave'], 'ave_over_max': rate['ave'] / rate['max'],
               'block_ms': {k: [round(1e3 * t, 3) for t in v] for k, v in times.items()}}
        if pool_algo:
            out.update({'ave_pool_fused': rate['ave_fused'], 'ave_fused_over_ave': rate['ave_fused'] / rate['ave'],
                        'ave_fused_over_max': rate['ave_fused'] / rate['max'],
                        'pool_algo_in_force': {k: job.engine.pool_algo() for k, job in jobs.items()},
                        'class_ms_per_step': {k: class_ms(job, solo, steps) for k, job in jobs.items()}})
        return out
    finally:
        for job in jobs.values():
            job.engine.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default=','.join(LEGS))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--pool-algo', action='store_true', help='add the AVE net under st_set_pool_algo(ctx, 1) as a third job of every leg')
    args = ap.parse_args(argv)
    for name in args.legs.split(','):
        print(json.dumps(leg(name, args.steps, args.warmup, args.blocks, args.pool_algo)), flush=True)


if __name__ == '__main__':
    main()
