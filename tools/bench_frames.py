#!/usr/bin/env python3
"""What the seam between two frames of a sequence costs (jobs.run_frames): one process, one engine, a 1024^2 seeded iterate and a smooth
fractional flow, two seams timed alternately, each ending in st_sync, after a warm-up of both:

    host     what run_frames did before the frames were kept on the device: get_input_nchw -> jobs.warp_planar (NumPy float64) ->
             set_input_nchw -> set_anchor with a host map
    device   frame_push -> set_input_from_frame -> anchor_from_frame with the forward flow (the map is derived on the device)

Both leave the same iterate and the same anchor planes (checked once, bit for bit, before anything is timed).  Then, from st_profile_read
over further device seams (events around every launch: not the timed run), the mean duration of the `frames` launches against the bytes
they book and the time those bytes take at the 6 TB/s copy rate.

    python tools/bench_frames.py [--size 1024] [--seams 10] [--out profiles/frames_seam_1024.txt]

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


def smooth_flow(h, w, phase):
    yy, xx = (v.astype(np.float32) for v in np.mgrid[0:h, 0:w])
    f = np.empty((h, w, 2), np.float32)
    f[..., 0] = 3.3 * np.sin(2 * np.pi * (xx / 511 + yy / 389 + phase)) + 0.37
    f[..., 1] = 2.6 * np.cos(2 * np.pi * (xx / 433 - yy / 307 + phase)) - 0.21
    return f


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--seams', type=int, default=10, help='timed seams of each kind (at least 10)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--weight', type=float, default=40.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frames_seam_1024.txt'))
    args = ap.parse_args(argv)
    if args.seams < 10:
        ap.error('--seams: at least 10')
    sys.path.insert(0, ROOT)
    import style_transfer2_amd as st2
    from style_transfer2_amd import jobs

    h = w = args.size
    rng = np.random.RandomState(0)
    eng = st2.Engine()                                      # (no GPU: this raises)
    try:
        eng.set_input(rng.randint(0, 256, (h, w, 3)).astype(np.uint8))
        eng.frames_keep(1)
        flow = smooth_flow(h, w, 0.0)
        fwd = -smooth_flow(h, w, 0.003)
        mask = rng.rand(h, w).astype(np.float32)

        def host():
            prev = jobs.warp_planar(eng.get_input_nchw()[0], flow)
            eng.set_input_nchw(prev[None])
            eng.set_anchor(prev[None], mask, args.weight)
            eng.sync()

        def device():
            eng.frame_push()
            eng.set_input_from_frame(1, flow)
            eng.anchor_from_frame(1, flow, fwd, None, args.weight)
            eng.sync()

        # the two seams leave the same iterate and the same anchor planes
        x0 = eng.get_input_nchw()
        host()
        x_host = eng.get_input_nchw()
        eng.set_input_nchw(x0)
        device()
        same = bool(np.array_equal(eng.get_input_nchw().view(np.uint32), x_host.view(np.uint32)))
        if not same:
            raise SystemExit('the device seam does not leave the host seam\'s iterate')
        for _ in range(args.warmup):
            host(); device()
        times = {'host': [], 'device': []}
        for _ in range(args.seams):
            for name, seam in (('host', host), ('device', device)):
                eng.sync()
                t0 = time.perf_counter()
                seam()
                times[name].append(time.perf_counter() - t0)
        eng.profile_enable(True)
        eng.profile_read()
        for _ in range(args.seams):
            device()
        prof = eng.profile_read().get('frames')
        eng.profile_enable(False)
    finally:
        eng.close()
    out = {'workload': 'seam between two frames, %d^2, one engine' % args.size, 'seams': args.seams, 'warmup': args.warmup, 'unit': 'ms',
           'same_iterate_bits': same}
    for name, v in times.items():
        ms = sorted(1e3 * t for t in v)
        out[name] = {'median': round(statistics.median(ms), 3), 'min': round(ms[0], 3), 'max': round(ms[-1], 3)}
    out['host_over_device'] = round(out['host']['median'] / out['device']['median'], 2)
    if prof:
        per = prof['bytes'] / prof['launches']
        out['frames_launch'] = {'launches_per_seam': prof['launches'] / args.seams, 'mean_us': round(1e3 * prof['ms'] / prof['launches'], 2),
                                'algorithmic_MB': round(per / 1e6, 2), 'GB_per_s': round(prof['bytes'] / (prof['ms'] * 1e-3) / 1e9, 1),
                                'us_at_6_TB_per_s': round(per / COPY_RATE * 1e6, 2)}
    line = json.dumps(out)
    print(line, flush=True)
    text = ('tools/bench_frames.py --size %d --seams %d: the seam between two frames, host against device, alternating in one process\n'
            'host   (get_input_nchw -> warp_planar -> set_input_nchw -> set_anchor with a host map): median %.3f ms (min %.3f, max %.3f)\n'
            'device (frame_push -> set_input_from_frame -> anchor_from_frame with the forward flow): median %.3f ms (min %.3f, max %.3f)\n'
            % (args.size, args.seams, out['host']['median'], out['host']['min'], out['host']['max'],
               out['device']['median'], out['device']['min'], out['device']['max']))
    if prof:
        fl = out['frames_launch']
        text += ('frames launches (%.0f per seam, profiled in a run of their own): mean %.2f us for %.2f MB booked = %.1f GB/s; those bytes at 6 TB/s: %.2f us\n'
                 % (fl['launches_per_seam'], fl['mean_us'], fl['algorithmic_MB'], fl['GB_per_s'], fl['us_at_6_TB_per_s']))
    text += line + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
