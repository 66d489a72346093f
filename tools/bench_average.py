#!/usr/bin/env python3
"""What iterate averaging (st_set_iterate_average) costs: ONE job -- VGG19, 1024^2, Adam, fp32, bench.py's images and weights -- timed in
alternating blocks of mode off and mode on in one process, so drift of the clock or of other work on the box falls on both.  The mode
does not touch the trajectory, so both kinds of block run the same work but for the new pass.  Two loops, bench.py's timed-region
contract (W untimed steps, then blocks of exactly K steps bracketed by device synchronisation; median over blocks):

    resident    step(want_image=False): nothing is read back; mode on adds one launch per step (x, mean in; mean out)
    pipelined   step_begin / step_end with one iteration ahead, as the worker loop runs: every iterate crosses to pinned host
                memory; mode on makes the emission launch (emit_k) update the mean on the way (x, mean in; mean, image out)

    python tools/bench_average.py
    python tools/bench_average.py --tree ../parent-checkout      # the same blocks on another (built) checkout of the project, e.g. the
                                                                 # parent commit; an engine without the mode runs the off-blocks only
One JSON line: median it/s and the spread (min, max) of the blocks per loop and mode, and, from st_profile_read over one more block
of profiled steps per loop (events around every launch: not the timed run), the mean duration of the `misc` launch of a step -- the
averaging forms of emit_k with the mode on, its plain form in the pipelined loop with it off -- and the GB/s of its algorithmic traffic where
the launch books it (the plain form of a step is booked without bytes: tests/golden/route_fingerprints.json records it so)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
DECAY = 0.9


def make_job(size):
    import style_transfer2_amd as st2
    from style_transfer2_amd import weights as st2_weights
    import bench
    content, style, init = bench.images(size)
    job = st2.StyleTransfer(st2.HipModel(st2_weights.he_normal(st2.VGG19_TOPOLOGY, seed=0)))
    job.set_weights(bench.WEIGHTS, bench.PARAMS)
    job.set_input(init)
    job.set_content(content)
    job.set_style(style)
    job.optimizer_cls = st2.AdamOptimizer
    job.set_step_size(bench.STEP_SIZES['adam'])
    job.reset()
    assert job.start()
    return job


def resident(eng, steps):
    for _ in range(steps):
        eng.step(want_image=False, want_trace=False)


def pipelined(eng, steps):
    for k in range(steps):                 # one begin ahead of every end
        eng.step_begin()
        if k:
            eng.step_end(copy=False)
    eng.step_end(copy=False)


def block(eng, loop, steps):
    eng.sync()
    t0 = time.perf_counter()
    loop(eng, steps)
    eng.sync()
    return time.perf_counter() - t0


def misc_launch(eng, loop, steps):
    """Mean microseconds and GB/s of the `misc` launches of `steps` profiled steps (one per step in both loops)."""
    eng.profile_enable(True)
    eng.profile_read()
    loop(eng, steps)
    eng.sync()
    misc = eng.profile_read().get('misc')
    eng.profile_enable(False)
    if not misc:
        return None
    out = {'launches_per_step': misc['launches'] / steps, 'mean_us': round(1e3 * misc['ms'] / misc['launches'], 2)}
    if misc['bytes']:
        out['algorithmic_MB'] = round(misc['bytes'] / misc['launches'] / 1e6, 2)
        out['GB_per_s'] = round(misc['bytes'] / (misc['ms'] * 1e-3) / 1e9, 1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--modes', default='off,on', help='off,on (default: alternating blocks) or off alone: the run an engine without the mode makes')
    ap.add_argument('--tree', default=os.path.dirname(HERE), help='the (built) checkout to measure; default: the one this tool lies in')
    args = ap.parse_args(argv)
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    job = make_job(args.size)
    eng = job.engine
    modes = {'off': 0.0, 'on': DECAY} if hasattr(eng, 'set_iterate_average') else {'off': None}
    if args.modes == 'off':
        modes = {'off': None}                      # the setter is never called
    out = {'workload': 'VGG19 %d^2 Adam fp32' % args.size, 'tree': os.path.relpath(tree, os.path.dirname(HERE)), 'decay': DECAY,
           'steps': args.steps, 'warmup': args.warmup, 'blocks': args.blocks, 'unit': 'it/s', 'modes': sorted(modes)}
    try:
        for name, loop in (('resident', resident), ('pipelined', pipelined)):
            loop(eng, args.warmup)
            times = {m: [] for m in modes}
            for _ in range(args.blocks):
                for m, decay in modes.items():
                    if decay is not None:
                        eng.set_iterate_average(decay)
                    times[m].append(block(eng, loop, args.steps))
            rates = {m: sorted(args.steps / t for t in v) for m, v in times.items()}
            out[name] = {m: {'median': round(statistics.median(r), 3), 'min': round(r[0], 3), 'max': round(r[-1], 3)} for m, r in rates.items()}
            out[name]['block_ms'] = {m: [round(1e3 * t, 3) for t in v] for m, v in times.items()}
            if 'on' in modes:
                out[name]['on_over_off'] = round(out[name]['on']['median'] / out[name]['off']['median'], 5)
            out[name]['misc_launch'] = {}
            for m, decay in modes.items():
                if decay is not None:
                    eng.set_iterate_average(decay)
                out[name]['misc_launch'][m] = misc_launch(eng, loop, args.steps)
    finally:
        eng.close()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
