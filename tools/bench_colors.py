#!/usr/bin/env python3
"""What luminance-only output (st_set_original_colors) costs: ONE job -- VGG19, 1024^2, Adam, fp32, bench.py's images and weights -- timed
in alternating blocks of mode off and mode on in one process, so drift of the clock or of other work on the box falls on both.  The mode
does not touch the trajectory, so both kinds of block run the same work but for the emission pass.  Two loops, bench.py's timed-region
contract (W untimed steps, then blocks of exactly K steps bracketed by device synchronisation; median over blocks):

    resident    step(want_image=False): nothing is read back, so no image is emitted and the mode launches nothing: the control
    pipelined   step_begin / step_end with one iteration ahead, as the worker loop runs: every iterate crosses to pinned host
                memory; mode on makes the emission launch (emit_k) the luminance form (x, content in; image out) instead of the plain one

    python tools/bench_colors.py
    python tools/bench_colors.py --tree ../parent-checkout --modes off     # the same blocks on another (built) checkout of the project,
                                                                           # e.g. the parent commit, which has no such mode
One JSON line: median it/s and the spread (min, max) of the blocks per loop and mode, and, from st_profile_read over one more block
of profiled steps per loop (events around every launch: not the timed run), the mean duration of the `misc` launch of a step -- emit_k's
luminance form with the mode on, its plain form with it off -- and the GB/s of its algorithmic traffic where the launch books it (the plain
form of a step is booked without bytes: tests/golden/route_fingerprints.json records it so)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_average import block, make_job, misc_launch, pipelined, resident       # noqa: E402  (the loops and the timed region are that tool's)


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
    modes = {'off': False, 'on': True} if hasattr(eng, 'set_original_colors') else {'off': None}
    if args.modes == 'off':
        modes = {'off': None}                      # the setter is never called
    out = {'workload': 'VGG19 %d^2 Adam fp32' % args.size, 'tree': os.path.relpath(tree, os.path.dirname(HERE)),
           'steps': args.steps, 'warmup': args.warmup, 'blocks': args.blocks, 'unit': 'it/s', 'modes': sorted(modes)}
    try:
        for name, loop in (('resident', resident), ('pipelined', pipelined)):
            loop(eng, args.warmup)
            times = {m: [] for m in modes}
            for _ in range(args.blocks):
                for m, on in modes.items():
                    if on is not None:
                        eng.set_original_colors(on)
                    times[m].append(block(eng, loop, args.steps))
            rates = {m: sorted(args.steps / t for t in v) for m, v in times.items()}
            out[name] = {m: {'median': round(statistics.median(r), 3), 'min': round(r[0], 3), 'max': round(r[-1], 3)} for m, r in rates.items()}
            out[name]['block_ms'] = {m: [round(1e3 * t, 3) for t in v] for m, v in times.items()}
            if 'on' in modes:
                out[name]['on_over_off'] = round(out[name]['on']['median'] / out[name]['off']['median'], 5)
            out[name]['misc_launch'] = {}
            for m, on in modes.items():
                if on is not None:
                    eng.set_original_colors(on)
                out[name]['misc_launch'][m] = misc_launch(eng, loop, args.steps)
    finally:
        eng.close()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
