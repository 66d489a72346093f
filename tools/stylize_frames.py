#!/usr/bin/env python3
"""Headless stylisation of a frame sequence on one MI355X, with temporal consistency:
    stylize_frames.py f000.png f001.png ... --style s.jpg --out-dir out [--flows DIR] [--masks DIR] [--anchor-weight W]
Frame 0 is a plain job.  Every later frame starts from the previous frame's iterate, warped by the optical flow where one is given, and
is pulled toward it by the anchor term (st_set_anchor; jobs.run_frames) with the weight W and the frame's map.
--flows DIR: <stem>.npy per frame after the first, (H, W, 2) float (dx, dy) from that frame back to the one before, at the size the
frames are stylised at.  --masks DIR: <stem>.npy ((H, W) values >= 0) or <stem>.png (0 .. 255 -> 0 .. 1): the flow's reliability.
Flows and maps are the caller's: nothing here estimates them.  The results go to <out-dir>/<stem>.png."""
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
    ap.add_argument('--anchor-weight', type=float, default=1.0, metavar='W')
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


def side_file(directory, stem, endings):
    for ending in endings:
        path = os.path.join(directory, stem + ending)
        if os.path.exists(path):
            return path
    raise FileNotFoundError('%s: no %s' % (directory, ' or '.join(stem + e for e in endings)))


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import style_transfer2_amd as st2
    from style_transfer2_amd import jobs, weights as st2_weights

    frames = [np.uint8(jobs.resize_to_fit(jobs.load_rgb(path), args.size)) for path in args.frames]
    stems = [os.path.splitext(os.path.basename(path))[0] for path in args.frames]
    hw = frames[0].shape[:2]
    flows = masks = None
    if args.flows:
        flows = [None] + [np.load(side_file(args.flows, stem, ('.npy',))) for stem in stems[1:]]
    if args.masks:
        masks = [None] + [jobs.load_mask(side_file(args.masks, stem, ('.npy', '.png')), hw) for stem in stems[1:]]
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
    results = jobs.run_frames(job, frames, style, args.iters, args.anchor_weight, flows=flows, masks=masks,
                              first_iterations=args.first_iters or None, optimizer=args.optimizer)
    os.makedirs(args.out_dir, exist_ok=True)
    for stem, image in zip(stems, results):
        out = os.path.join(args.out_dir, stem + '.png')
        Image.fromarray(np.uint8(np.clip(image, 0, 255))).save(out)
        print('wrote', out, image.shape)


if __name__ == '__main__':
    main()
