#!/usr/bin/env python3
"""What an optical-flow estimate (st_flow_estimate; Engine.flow_estimate) costs: one process, one engine, a seeded textured pair moved
by a few pixels, the defaults (alpha 0.06, 3 warps, 40 Jacobi iterations, automatic levels).

    per size (512^2 and 1024^2) and route (0: levels of up to 4096 pixels run a warp's Jacobi iterations in one launch of one workgroup;
    1: one launch per iteration everywhere), alternating after a warm-up of both: milliseconds per estimate -- a host clock around the
    whole call, which uploads both uint8 images, waits for the stream and copies the flow out; the two routes' flows are compared bit
    for bit before anything is timed
    from st_profile_read over further estimates (events around every launch: not the timed run): launches per estimate by class, and the
    mean duration of the per-iteration Jacobi launch at level 0 against the bytes it books (u, v and the four coefficient planes in,
    u', v' out: 32 bytes per pixel) and the time those bytes take at the 6 TB/s copy rate
    the seam: the two estimates run_frames(estimate=...) makes per frame (backward and forward) beside the 200 iterations of a frame job
    -- VGG19, Adam, fp32, bench.py's images and weights at the larger size -- timed as blocks of 20 resident steps and scaled

    python tools/bench_flow.py [--sizes 512,1024] [--repeats 10] [--out profiles/flow_1024.txt]

It needs a GPU: without one the engine cannot be made and the tool fails.  The record goes to --out and to stdout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COPY_RATE = 6.0e12                                          # bytes / s: the copy rate the README holds the HBM-bound passes against


def textured_pair(h, w, seed=1, shift=(3.3, -2.1)):
    """Two uint8 HxWx3 frames of one seeded sum of sinusoids, the first displaced by `shift` pixels."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    terms = [(rng.uniform(6, 60), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 1) / 24) for _ in range(24)]

    def frame(dx, dy):
        g = np.zeros((h, w))
        for wavelength, angle, phase, amplitude in terms:
            g += amplitude * np.sin(2 * np.pi / wavelength * (np.cos(angle) * (xx + dx) + np.sin(angle) * (yy + dy)) + phase)
        grey = np.uint8(np.clip(255 * (0.5 + 0.5 * g), 0, 255))
        return np.ascontiguousarray(np.repeat(grey[..., None], 3, axis=2))
    return frame(*shift), frame(0.0, 0.0)


def spread(ms):
    ms = sorted(ms)
    return {'median': round(statistics.median(ms), 3), 'min': round(ms[0], 3), 'max': round(ms[-1], 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='512,1024')
    ap.add_argument('--repeats', type=int, default=10, help='timed estimates per size and route (at least 10)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--job-steps', type=int, default=20, help='steps per timed block of the frame job')
    ap.add_argument('--job-blocks', type=int, default=5)
    ap.add_argument('--no-job', action='store_true', help='skip the frame job (no VGG19 weights are made)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flow_1024.txt'))
    args = ap.parse_args(argv)
    if args.repeats < 10:
        ap.error('--repeats: at least 10')
    sizes = [int(s) for s in args.sizes.split(',')]
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import style_transfer2_amd as st2
    from style_transfer2_amd import flow

    out = {'workload': 'st_flow_estimate, defaults, uint8 frames, one engine', 'repeats': args.repeats, 'warmup': args.warmup, 'unit': 'ms', 'sizes': {}}
    eng = st2.Engine()                                      # (no GPU: this raises)
    try:
        for size in sizes:
            a, b = textured_pair(size, size)
            flows = {r: eng.flow_estimate(a, b, route=r) for r in (0, 1)}
            same = bool(np.array_equal(flows[0].view(np.uint32), flows[1].view(np.uint32)))
            if not same:
                raise SystemExit('the two routes differ at %d^2' % size)
            inner = flows[0][12:-12, 12:-12]
            err = float(np.sqrt((inner[..., 0] - 3.3) ** 2 + (inner[..., 1] + 2.1) ** 2).mean())
            for _ in range(args.warmup):
                for r in (0, 1):
                    eng.flow_estimate(a, b, route=r)
            times = {0: [], 1: []}
            for _ in range(args.repeats):
                for r in (0, 1):
                    eng.sync()
                    t0 = time.perf_counter()
                    eng.flow_estimate(a, b, route=r)
                    times[r].append(1e3 * (time.perf_counter() - t0))
            rec = {'levels': len(flow.level_sizes(size, size)), 'same_bits_both_routes': same, 'interior_error_px': round(err, 4),
                   'route0': spread(times[0]), 'route1': spread(times[1])}
            eng.profile_enable(True)
            for r in (0, 1):
                eng.profile_read()
                for _ in range(args.repeats):
                    eng.flow_estimate(a, b, route=r)
                prof = eng.profile_read()
                rec['route%d' % r]['launches_per_estimate'] = {k: v['launches'] / args.repeats for k, v in sorted(prof.items())}
                rec['route%d' % r]['launches_per_estimate']['all'] = sum(v['launches'] for v in prof.values()) / args.repeats
                rec['route%d' % r]['device_ms_per_estimate'] = {k: round(v['ms'] / args.repeats, 3) for k, v in sorted(prof.items())}
            eng.profile_read()
            for _ in range(args.repeats):                   # level 0 alone: every per-iteration launch is of the full size
                eng.flow_estimate(a, b, route=1, levels=1)
            jac = eng.profile_read().get('flow_jacobi')
            eng.profile_enable(False)
            per = jac['bytes'] / jac['launches']
            rec['jacobi_launch_level0'] = {'mean_us': round(1e3 * jac['ms'] / jac['launches'], 2), 'booked_MB': round(per / 1e6, 2),
                                           'GB_per_s': round(jac['bytes'] / (jac['ms'] * 1e-3) / 1e9, 1), 'us_at_6_TB_per_s': round(per / COPY_RATE * 1e6, 2)}
            out['sizes'][str(size)] = rec
        eng.flow_release()
    finally:
        eng.close()
    if not args.no_job:
        from bench_average import block, make_job, resident
        size = max(sizes)
        job = make_job(size)
        try:
            resident(job.engine, 5)
            blocks = [1e3 * block(job.engine, resident, args.job_steps) / args.job_steps for _ in range(args.job_blocks)]
        finally:
            job.engine.close()
        step = spread(blocks)
        two = 2 * out['sizes'][str(size)]['route0']['median']
        out['seam'] = {'size': size, 'step_ms': step, 'job_of_200_steps_ms': round(200 * step['median'], 1), 'two_estimates_ms': round(two, 3),
                       'estimates_over_job': round(two / (200 * step['median']), 5)}
    line = json.dumps(out)
    print(line, flush=True)
    text = 'tools/bench_flow.py --sizes %s --repeats %d: one estimate with the defaults, the two routes alternating in one process\n' % (args.sizes, args.repeats)
    for size, rec in out['sizes'].items():
        text += ('%s^2 (%d levels; both routes the same bits; interior error of the (3.3, -2.1) shift %.4f px)\n' % (size, rec['levels'], rec['interior_error_px']))
        for r, what in ((0, 'route 0 (small levels in one workgroup)'), (1, 'route 1 (one launch per iteration)   ')):
            v = rec['route%d' % r]
            text += ('  %s: median %.3f ms (min %.3f, max %.3f), %.0f launches per estimate\n'
                     % (what, v['median'], v['min'], v['max'], v['launches_per_estimate']['all']))
        j = rec['jacobi_launch_level0']
        text += ('  per-iteration Jacobi launch at level 0 (profiled in a run of its own): mean %.2f us for %.2f MB booked = %.1f GB/s; those bytes at 6 TB/s: %.2f us\n'
                 % (j['mean_us'], j['booked_MB'], j['GB_per_s'], j['us_at_6_TB_per_s']))
    if 'seam' in out:
        s = out['seam']
        text += ('seam at %d^2: two estimates %.3f ms beside a frame job of 200 steps at %.3f ms per step = %.1f ms: %.3f %% of the job\n'
                 % (s['size'], s['two_estimates_ms'], s['step_ms']['median'], s['job_of_200_steps_ms'], 100 * s['estimates_over_job']))
    text += line + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
