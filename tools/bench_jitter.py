#!/usr/bin/env python3
"""What jitter (st_set_jitter) costs: ONE job -- VGG19, 1024^2, Adam, fp32, bench.py's images and weights -- timed in alternating blocks
in one process, so drift of the clock or of other work on the box falls on all of them.  The mode changes the trajectory (that is its
purpose), but not the work of an evaluation.  The blocks:

    off          the mode off, bench.py's weights (a content row at conv4_2)
    on           st_set_jitter(R, SEED) with those weights: two roll_k launches per step, and -- the shift changes with every step -- the
                 content features taken again from the rolled content image: one more forward to conv4_2
    off_style    the mode off, the style rows alone (what `on_style` is held against)
    on_style     the mode on, the style rows alone: the two roll_k launches and nothing else

bench.py's timed-region contract (W untimed steps, then blocks of exactly K steps bracketed by device synchronisation; median over
blocks), in the resident loop: step(want_image=False), nothing is read back, so the profiler's class `misc` holds the mode's launches of
roll_k and nothing else.

    python tools/bench_jitter.py
One JSON line: median it/s and the spread (min, max) of the blocks per mode, the differences per step, and, from st_profile_read over one
more block of profiled steps per mode (events around every launch: not the timed run), launches per step, the mean duration and the GB/s
of `misc` (roll_k: 25.2 MB in and out at 1024^2), `finalize` (with the mode on: one launch more, the sums of squares behind scd_grad) and
the conv classes (the extra forward)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_average import block, make_job, resident                  # noqa: E402  (the loop and the timed region are that tool's)
from bench_laplacian import per_launch                               # noqa: E402

CLASSES = ('misc', 'finalize', 'image_pass', 'conv3x3_fwd_wino_f32', 'conv3x3_fwd_mfma_f32', 'conv3x3_dgrad_wino_f32', 'conv3x3_dgrad_mfma_f32')
MODES = ('off', 'on', 'off_style', 'on_style')


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--radius', type=int, default=16)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(HERE))
    import bench
    job = make_job(args.size)
    eng = job.engine
    style_only = dict(bench.WEIGHTS, content={})
    out = {'workload': 'VGG19 %d^2 Adam fp32' % args.size, 'radius': args.radius, 'seed': args.seed, 'steps': args.steps, 'warmup': args.warmup,
           'blocks': args.blocks, 'unit': 'it/s', 'modes': list(MODES)}
    state = {'style': False}

    def switch(mode):
        style = mode.endswith('_style')
        if style != state['style']:
            job.set_weights(style_only if style else bench.WEIGHTS, bench.PARAMS)
            state['style'] = style
        eng.set_jitter(args.radius if mode.startswith('on') else 0, args.seed)
    try:
        for mode in MODES:                                 # (every lazily made buffer and every norm exists before the first timed block)
            switch(mode)
            resident(eng, args.warmup)
        times = {m: [] for m in MODES}
        for _ in range(args.blocks):
            for m in MODES:
                switch(m)
                resident(eng, 2)                           # (untimed: the first steps after the switch)
                times[m].append(block(eng, resident, args.steps))
        rates = {m: sorted(args.steps / t for t in v) for m, v in times.items()}
        out['it_per_s'] = {m: {'median': round(statistics.median(r), 3), 'min': round(r[0], 3), 'max': round(r[-1], 3)} for m, r in rates.items()}
        out['block_ms'] = {m: [round(1e3 * t, 3) for t in v] for m, v in times.items()}
        ms = {m: statistics.median(times[m]) / args.steps * 1e3 for m in MODES}
        out['ms_per_step'] = {m: round(v, 4) for m, v in ms.items()}
        out['on_minus_off_us_per_step'] = round(1e3 * (ms['on'] - ms['off']), 2)
        out['on_over_off_time'] = round(ms['on'] / ms['off'], 5)
        out['on_style_minus_off_style_us_per_step'] = round(1e3 * (ms['on_style'] - ms['off_style']), 2)
        out['on_style_over_off_style_time'] = round(ms['on_style'] / ms['off_style'], 5)
        out['launches'] = {}
        for m in MODES:
            switch(m)
            resident(eng, 2)
            out['launches'][m] = per_launch(eng, resident, args.steps, args.size, CLASSES)
    finally:
        eng.close()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
