#!/usr/bin/env python3
"""What the anchor term (st_set_anchor) costs: ONE job -- VGG19, 1024^2, Adam, fp32, bench.py's images and weights -- timed in alternating
blocks of the term off and on (with a map) in one process, so drift of the clock or of other work on the box falls on both.  The term
changes the trajectory (that is its purpose), but not the work of a step: every block runs the same launches but for the term's one.
Two loops, bench.py's timed-region contract (W untimed steps, then blocks of exactly K steps bracketed by device synchronisation; median
over blocks):

    resident    step(want_image=False): nothing is read back
    pipelined   step_begin / step_end with one iteration ahead, as the worker loop runs: every iterate crosses to pinned host memory

    python tools/bench_anchor.py
    python tools/bench_anchor.py --no-map                                # without the map: one stream less to read
    python tools/bench_anchor.py --tree ../parent-checkout --modes off   # the same blocks on another (built) checkout of the project,
                                                                         # e.g. the parent commit, which has no such term
One JSON line: median it/s and the spread (min, max) of the blocks per loop and mode, and, from st_profile_read over one more block of
profiled steps per loop (events around every launch: not the timed run), the mean duration and the GB/s of the algorithmic traffic of
the term's launch -- booked under a class of its own, `anchor`: x, the anchor and the map in, the plane out, 42 MB at 1024^2 -- of the
`image_pass` launch (one more stream to read with the term on) and, in the pipelined loop, of the `misc` launch, emit_k's plain form
(x in, the image out: booked without bytes, so its traffic is counted here), the yardstick the term's launch is held against."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_average import block, make_job, pipelined, resident       # noqa: E402  (the loops and the timed region are that tool's)
from bench_laplacian import per_launch                               # noqa: E402

CLASSES = ('anchor', 'image_pass', 'finalize', 'misc')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--weight', type=float, default=100.0, help='the weight of the mode on')
    ap.add_argument('--no-map', action='store_true', help='the mode on without a map')
    ap.add_argument('--modes', default='off,on', help='off,on (default: alternating blocks) or off alone: the run an engine without the term makes')
    ap.add_argument('--tree', default=os.path.dirname(HERE), help='the (built) checkout to measure; default: the one this tool lies in')
    args = ap.parse_args(argv)
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    job = make_job(args.size)
    eng = job.engine
    modes = {'off': None}                              # the setter is never called
    if args.modes != 'off' and hasattr(eng, 'set_anchor'):
        rng = np.random.RandomState(0)
        h, w = eng.input_shape()
        anchor = (rng.rand(1, 3, h, w) * 255 - 116).astype(np.float32)
        mask = None if args.no_map else rng.rand(h, w).astype(np.float32)
        modes = {'off': False, 'on': True}
    out = {'workload': 'VGG19 %d^2 Adam fp32' % args.size, 'tree': os.path.relpath(tree, os.path.dirname(HERE)), 'weight': args.weight,
           'map': not args.no_map, 'steps': args.steps, 'warmup': args.warmup, 'blocks': args.blocks, 'unit': 'it/s', 'modes': sorted(modes)}

    def switch(on):
        if on is not None:
            eng.set_anchor(anchor if on else None, mask, args.weight)
    try:
        for name, loop in (('resident', resident), ('pipelined', pipelined)):
            loop(eng, args.warmup)
            times = {m: [] for m in modes}
            for _ in range(args.blocks):
                for m, on in modes.items():
                    switch(on)
                    loop(eng, 1)                       # (untimed: the first step after the switch)
                    times[m].append(block(eng, loop, args.steps))
            rates = {m: sorted(args.steps / t for t in v) for m, v in times.items()}
            out[name] = {m: {'median': round(statistics.median(r), 3), 'min': round(r[0], 3), 'max': round(r[-1], 3)} for m, r in rates.items()}
            out[name]['block_ms'] = {m: [round(1e3 * t, 3) for t in v] for m, v in times.items()}
            if 'on' in modes:
                off_ms, on_ms = (statistics.median(times[m]) / args.steps * 1e3 for m in ('off', 'on'))
                out[name]['on_over_off'] = round(out[name]['on']['median'] / out[name]['off']['median'], 5)
                out[name]['on_minus_off_us_per_step'] = round(1e3 * (on_ms - off_ms), 2)
            out[name]['launches'] = {}
            for m, on in modes.items():
                switch(on)
                loop(eng, 1)
                out[name]['launches'][m] = per_launch(eng, loop, args.steps, args.size, CLASSES)
    finally:
        eng.close()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
