#!/usr/bin/env python3
"""Headless stylisation of a frame sequence on one MI355X, with temporal consistency:
    stylize_frames.py f000.png f001.png ... --style s.jpg --out-dir out [--flows DIR] [--forward-flows DIR] [--masks DIR]
                      [--long-term 2,4] [--anchor-weight W] [--estimate-flow [--flow-alpha A] [--flow-iters N] [--flow-warps N]
                      [--flow-levels N] [--save-flows DIR]]
Frame 0 is a plain job.  Every later frame starts from the previous frame's iterate, warped by the optical flow where one is given, and
is pulled toward it by the anchor term (st_set_anchor; jobs.run_frames) with the weight W and the frame's map.  The seam between two
frames runs on the device (st_set_input_from_frame, st_anchor_from_frame).
--flows DIR: <stem>.npy per frame after the first, (H, W, 2) float (dx, dy) from that frame back to the one before, at the size the
frames are stylised at.  --masks DIR: <stem>.npy ((H, W) values >= 0) or <stem>.png (0 .. 255 -> 0 .. 1): the flow's reliability, given.
--forward-flows DIR: <stem>.npy per frame after the first, the flow from the frame before to that frame: the reliability is then derived
on the device (forward / backward consistency, motion boundaries, samples outside the image: st2.h) and multiplied by the frame's map
where --masks has one.  --long-term 2,4: pixels the map leaves free are anchored to the stylised frame 2, then 4 frames back, through
<stem>.b<j>.npy under --flows (from the frame back to the one j before; frames from the j-th on; a missing file skips that pair) and,
where it exists, <stem>.f<j>.npy under --forward-flows (the flow from the frame j before to the frame).
Flows and maps may be the caller's, or --estimate-flow estimates the flows on the device from the frames themselves (st_flow_estimate:
coarse-to-fine Horn-Schunck; --flow-alpha, --flow-iters, --flow-warps, --flow-levels are its parameters): --flows, --forward-flows and
the --long-term side files are then optional, and a file that exists still wins over the estimate.  --save-flows DIR writes the flows
the run used as <stem>.npy, <stem>.fwd.npy, <stem>.b<j>.npy and <stem>.f<j>.npy; given as both --flows and --forward-flows, that
directory reproduces the run (--forward-flows reads <stem>.fwd.npy where there is one, else <stem>.npy).  The results go to <out-dir>/<stem>.png."""
import argparse
import os
import sys

import numpy as np
from PIL import Image


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('frames', nargs='+', metavar='FRAME')
    ap.add_argument('--style', required=True)
    ap.add_argument('--out-dir', required=True)
    ap.add_argument('--flows', default='', metavar='DIR')
    ap.add_argument('--masks', default='', metavar='DIR')
    ap.add_argument('--forward-flows', default='', metavar='DIR', help='<stem>.npy: the flow from the frame before; derives the reliability on the device')
    ap.add_argument('--long-term', type=long_term_arg, default=[], metavar='J,J', help='earlier frames to anchor uncovered pixels to, e.g. 2,4 (each 2 .. 8)')
    ap.add_argument('--anchor-weight', type=float, default=1.0, metavar='W')
    ap.add_argument('--matting', default='', metavar='W[:EPS]', help='st_set_matting for every frame: the photorealism term with the weight W and the regularisation EPS (default 1e-7)')
    ap.add_argument('--estimate-flow', action='store_true', help='estimate on the device every flow no file gives (st_flow_estimate)')
    ap.add_argument('--flow-alpha', type=float, default=None, metavar='A', help='smoothness weight of the estimator (default 0.06)')
    ap.add_argument('--flow-iters', type=int, default=None, metavar='N', help='Jacobi iterations per warp (default 40)')
    ap.add_argument('--flow-warps', type=int, default=None, metavar='N', help='warps per pyramid level (default 3)')
    ap.add_argument('--flow-levels', type=int, default=None, metavar='N', help='pyramid levels; 0: while the shorter side is at least 32 (default)')
    ap.add_argument('--save-flows', default='', metavar='DIR', help='with --estimate-flow: write the flows the run used')
    ap.add_argument('--iters', type=int, default=200, help='iterations of every frame after the first')
    ap.add_argument('--first-iters', type=int, default=0, metavar='N', help='iterations of the first frame (default: --iters)')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--style-size', type=int, default=0)
    ap.add_argument('--optimizer', default='adam', choices=['adam', 'lbfgs'])
    ap.add_argument('--weights', default='', help='.npz or .caffemodel; default: seeded synthetic weights')
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--precision', default='fp32', choices=['fp32', 'bf16', 'bf16-full'], help='st_set_precision: conv operands in fp32 or bf16')
    ap.add_argument('--conv-algo', type=int, default=None, choices=[0, 1, 2], help='st_set_conv_algo (default: the engine\'s, 1)')
    ap.add_argument('--gram-algo', type=int, default=None, choices=[0, 1], help='st_set_gram_algo (default: the engine\'s, 0)')
    ap.add_argument('--pool-algo', type=int, default=None, choices=[0, 1], help='st_set_pool_algo (default: the engine\'s, 0)')
    return ap


def long_term_arg(text):
    """'2,4' -> [2, 4]: distinct integers from 2 to 8, ascending."""
    try:
        js = sorted(int(part) for part in text.split(',') if part.strip())
    except ValueError:
        raise argparse.ArgumentTypeError('--long-term: integers separated by commas, got %r' % text)
    if not js or len(set(js)) != len(js) or js[0] < 2 or js[-1] > 8:
        raise argparse.ArgumentTypeError('--long-term: distinct integers from 2 to 8, got %r' % text)
    return js


def long_term_files(flows_dir, forward_dir, stems, js):
    """{j: ([backward flow file or None per frame], [forward flow file or None per frame] or None)}: <stem>.b<j>.npy under flows_dir for
    the frames from the j-th on, <stem>.f<j>.npy under forward_dir; a file that does not exist is None."""
    def existing(directory, name):
        path = os.path.join(directory, name)
        return path if os.path.exists(path) else None
    out = {}
    for j in js:
        back = [existing(flows_dir, '%s.b%d.npy' % (stem, j)) if t >= j else None for t, stem in enumerate(stems)]
        fwd = [existing(forward_dir, '%s.f%d.npy' % (stem, j)) if t >= j and back[t] else None for t, stem in enumerate(stems)] if forward_dir else None
        out[j] = (back, fwd)
    return out


def side_file(directory, stem, endings):
    for ending in endings:
        path = os.path.join(directory, stem + ending)
        if os.path.exists(path):
            return path
    raise FileNotFoundError('%s: no %s' % (directory, ' or '.join(stem + e for e in endings)))


def optional_file(directory, name):
    """The side file where the directory is given and holds it, else None (--estimate-flow fills the gap)."""
    path = os.path.join(directory, name) if directory else ''
    return path if path and os.path.exists(path) else None


def flow_params(ap, args):
    """The estimator's parameters from the command line, checked (None without --estimate-flow); refuses what cannot work."""
    given = {key: getattr(args, 'flow_' + key) for key in ('alpha', 'iters', 'warps', 'levels') if getattr(args, 'flow_' + key) is not None}
    if not args.estimate_flow:
        if given or args.save_flows:
            ap.error('--flow-alpha, --flow-iters, --flow-warps, --flow-levels and --save-flows need --estimate-flow')
        if args.forward_flows and not args.flows:
            ap.error('--forward-flows needs --flows: the reliability takes both directions')
        if args.long_term and (not args.flows or not (args.forward_flows or args.masks)):
            ap.error('--long-term needs --flows (the <stem>.b<j>.npy files) and a map from --forward-flows or --masks')
        return None
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from style_transfer2_amd import flow
    try:
        flow.check_flow(**given)
    except ValueError as e:
        ap.error('--estimate-flow: %s' % e)
    return given


def save_flows(directory, stems, flows, forward_flows, long_term):
    """<stem>.npy, <stem>.fwd.npy, <stem>.b<j>.npy, <stem>.f<j>.npy of every flow that is there; returns the paths written."""
    os.makedirs(directory, exist_ok=True)
    named = [('%s.npy', flows), ('%s.fwd.npy', forward_flows)]
    for j, (back, forth) in sorted((long_term or {}).items()):
        named += [('%%s.b%d.npy' % j, back), ('%%s.f%d.npy' % j, forth)]
    written = []
    for pattern, seq in named:
        for stem, f in zip(stems, seq or []):
            if f is not None:
                written.append(os.path.join(directory, pattern % stem))
                np.save(written[-1], np.asarray(f, np.float32))
    return written


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    estimate = flow_params(ap, args)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import style_transfer2_amd as st2
    from style_transfer2_amd import jobs, matting as st2_matting, weights as st2_weights
    try:
        mat = st2_matting.parse_matting(args.matting) if args.matting else None
    except ValueError as err:
        ap.error('--matting %s: %s' % (args.matting, err))

    frames = [np.uint8(jobs.resize_to_fit(jobs.load_rgb(path), args.size)) for path in args.frames]
    stems = [os.path.splitext(os.path.basename(path))[0] for path in args.frames]
    hw = frames[0].shape[:2]
    flows = masks = None
    load = lambda paths: [np.load(path) if path else None for path in paths]      # noqa: E731
    if args.flows and estimate is None:
        flows = [None] + [np.load(side_file(args.flows, stem, ('.npy',))) for stem in stems[1:]]
    if args.masks:
        masks = [None] + [jobs.load_mask(side_file(args.masks, stem, ('.npy', '.png')), hw) for stem in stems[1:]]
    forward_flows = long_term = None
    if args.forward_flows and estimate is None:
        forward_flows = [None] + [np.load(side_file(args.forward_flows, stem, ('.fwd.npy', '.npy'))) for stem in stems[1:]]
    if estimate is not None:                                # the files that exist; the estimates fill the gaps below
        flows = [None] + load(optional_file(args.flows, stem + '.npy') for stem in stems[1:])
        forward_flows = [None] + load(optional_file(args.forward_flows, stem + '.fwd.npy') or optional_file(args.forward_flows, stem + '.npy')
                                      for stem in stems[1:])
    if args.long_term and estimate is not None and not args.flows:
        long_term = {j: None for j in args.long_term}       # no side files: both directions are estimated
    elif args.long_term:
        long_term = {j: (load(back), load(fwd) if fwd else None)
                     for j, (back, fwd) in long_term_files(args.flows, args.forward_flows, stems, args.long_term).items()}
    style = jobs.load_rgb(args.style)
    style = np.uint8(jobs.resize_to_fit(style, args.style_size or args.size))

    if args.weights.endswith('.npz'):
        params = st2_weights.load_npz(args.weights, st2.VGG19_TOPOLOGY)
    elif args.weights.endswith('.caffemodel'):
        from style_transfer2_amd import caffemodel
        params = caffemodel.vgg_params(caffemodel.read_caffemodel(args.weights), st2.VGG19_TOPOLOGY)
    else:
        params = st2_weights.he_normal(st2.VGG19_TOPOLOGY, seed=0)
    job = st2.StyleTransfer(st2.HipModel(params, device=args.gpu, precision=args.precision, conv_algo=args.conv_algo, gram_algo=args.gram_algo,
                                         pool_algo=args.pool_algo))
    if estimate is not None:
        flows, forward_flows, long_term = jobs.fill_flows(job.engine, frames, flows, forward_flows, long_term or {}, **estimate)
        if args.save_flows:
            for path in save_flows(args.save_flows, stems, flows, forward_flows, long_term):
                print('wrote', path)
    results = jobs.run_frames(job, frames, style, args.iters, args.anchor_weight, flows=flows, masks=masks, forward_flows=forward_flows, long_term=long_term,
                              first_iterations=args.first_iters or None, optimizer=args.optimizer, matting=mat)
    os.makedirs(args.out_dir, exist_ok=True)
    for stem, image in zip(stems, results):
        out = os.path.join(args.out_dir, stem + '.png')
        Image.fromarray(np.uint8(np.clip(image, 0, 255))).save(out)
        print('wrote', out, image.shape)


if __name__ == '__main__':
    main()
