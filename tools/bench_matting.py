#!/usr/bin/env python3
"""What the photorealism term (st_set_matting) costs: ONE job -- VGG19, 1024^2, Adam, fp32, bench.py's images and weights -- timed in
alternating blocks of the term off and on in one process, so drift of the clock or of other work on the box falls on both.  The term
changes the trajectory (that is its purpose), but not the work of a step: every block runs the same launches but for the term's two.
Two loops, bench.py's timed-region contract (W untimed steps, then blocks of exactly K steps bracketed by device synchronisation; median
over blocks):

    resident    step(want_image=False): nothing is read back
    pipelined   step_begin / step_end with one iteration ahead, as the worker loop runs: every iterate crosses to pinned host memory

    python tools/bench_matting.py
    python tools/bench_matting.py --tree ../parent-checkout --modes off  # the same blocks on another (built) checkout of the project,
                                                                         # e.g. the parent commit, which has no such term
One JSON line: median it/s and the spread (min, max) of the blocks per loop and mode; from st_profile_read over one more block of
profiled steps per loop (events around every launch: not the timed run) the mean duration of the term's two launches -- booked under
classes of their own, `matting_fit` (x and I in, mu and M in, a_pb out) and `matting_apply` (x, I, a_pb and mu in, the plane out) --
their booked bytes, the GB/s of those and the time those bytes would take at the 6 TB/s a copy reaches; and the launches per step of
EVERY profile class with the term off, to hold against the parent commit's."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_average import block, make_job, pipelined, resident       # noqa: E402  (the loops and the timed region are that tool's)
from bench_laplacian import per_launch                               # noqa: E402

CLASSES = ('matting_fit', 'matting_apply', 'image_pass', 'finalize', 'misc')
COPY_GB_PER_S = 6000.0


def launch_counts(eng, loop, steps):
    """Launches per step of every profile class that launched."""
    eng.profile_enable(True)
    eng.profile_read()
    loop(eng, steps)
    eng.sync()
    prof = eng.profile_read()
    eng.profile_enable(False)
    return {name: p['launches'] / steps for name, p in sorted(prof.items()) if p['launches']}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--weight', type=float, default=1e4, help='the weight of the mode on')
    ap.add_argument('--eps', type=float, default=1e-7)
    ap.add_argument('--modes', default='off,on', help='off,on (default: alternating blocks) or off alone: the run an engine without the term makes')
    ap.add_argument('--tree', default=os.path.dirname(HERE), help='the (built) checkout to measure; default: the one this tool lies in')
    args = ap.parse_args(argv)
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    job = make_job(args.size)
    eng = job.engine
    modes = {'off': None}                              # the setter is never called
    if args.modes != 'off' and hasattr(eng, 'set_matting'):
        modes = {'off': False, 'on': True}
    out = {'workload': 'VGG19 %d^2 Adam fp32' % args.size, 'tree': os.path.relpath(tree, os.path.dirname(HERE)), 'weight': args.weight, 'eps': args.eps,
           'steps': args.steps, 'warmup': args.warmup, 'blocks': args.blocks, 'unit': 'it/s', 'modes': sorted(modes)}

    def switch(on):
        if on is not None:
            eng.set_matting(args.weight if on else 0.0, args.eps)
    try:
        for name, loop in (('resident', resident), ('pipelined', pipelined)):
            loop(eng, args.warmup)
            times = {m: [] for m in modes}
            for _ in range(args.blocks):
                for m, on in modes.items():
                    switch(on)
                    loop(eng, 1)                       # (untimed: the first step after the switch takes the per-window data)
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
                per = per_launch(eng, loop, args.steps, args.size, CLASSES)
                for p in per.values():
                    if 'algorithmic_MB' in p:
                        p['us_at_copy_rate'] = round(p['algorithmic_MB'] / COPY_GB_PER_S * 1e3, 2)
                out[name]['launches'][m] = per
            switch(False if 'on' in modes else None)
            loop(eng, 1)
            out[name]['launch_counts_off'] = launch_counts(eng, loop, args.steps)
    finally:
        eng.close()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
