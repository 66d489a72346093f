#!/usr/bin/env python3
"""Headless stylisation job on one MI355X:  stylize.py content.jpg style.jpg out.png [--size 512] [--iters 500]
--grid RxC: an image too large for one engine (beyond about 4096 x 4096) is cut into R x C tiles that all live on the one GPU
(jobs.run_tiled_job; the image edges must divide into tiles of multiples of 16 pixels).
--avg-decay D: the image written is the bias-corrected exponentially weighted mean of the iterates (st_set_iterate_average), not
the last iterate.
--original-colors: the image written keeps the content image's colours (the iterate's luminance, the content's chroma).
--match-style-colors: the style image is given the content image's colour mean and covariance before the style targets are taken.
--jitter R [--jitter-seed S]: every iteration shows the network the iterate rolled by a random shift of up to R pixels per axis
(st_set_jitter), which removes the regular grid artefacts of pools and strides; not with --grid."""
import argparse
import os
import sys

import numpy as np
from PIL import Image


def avg_decay(text):
    value = float(text)
    if not 0.0 <= value < 1.0:
        raise argparse.ArgumentTypeError('a decay in [0, 1) (0: off), not %r' % text)
    return value


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('content'); ap.add_argument('style'); ap.add_argument('out')
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--style-size', type=int, default=0)
    ap.add_argument('--iters', type=int, default=500)
    ap.add_argument('--optimizer', default='adam', choices=['adam', 'lbfgs'])
    ap.add_argument('--weights', default='', help='.npz or .caffemodel; default: seeded synthetic weights')
    ap.add_argument('--gpu', type=int, default=0)
    ap.add_argument('--precision', default='fp32', choices=['fp32', 'bf16', 'bf16-full'], help='st_set_precision: conv operands in fp32 or bf16')
    ap.add_argument('--conv-algo', type=int, default=None, choices=[0, 1, 2], help='st_set_conv_algo (default: the engine\'s, 1)')
    ap.add_argument('--gram-algo', type=int, default=None, choices=[0, 1], help='st_set_gram_algo (default: the engine\'s, 0)')
    ap.add_argument('--ave-pools', action='store_true', help='VGG19 with every pool an average pool (Caffe `pool: AVE`; the pooling of vgg_normalised-style weights)')
    ap.add_argument('--pool-algo', type=int, default=None, choices=[0, 1], help='st_set_pool_algo (default: the engine\'s, 0); 1 fuses average pools into the bf16 conv launches (--precision bf16)')
    ap.add_argument('--grid', default='', help='RxC: tile-shard the image over this one GPU (large images)')
    ap.add_argument('--shard-style', action='store_true', help='with --grid: cut the style image over the ranks as well (every rank forwards one window of it)')
    ap.add_argument('--avg-decay', type=avg_decay, default=None, metavar='D',
                    help='st_set_iterate_average: write the bias-corrected running mean of the iterates with this decay, 0 < D < 1 (default: the last iterate)')
    ap.add_argument('--original-colors', action='store_true', help='st_set_original_colors: keep the content image\'s colours (luminance of the result, chroma of the content)')
    ap.add_argument('--match-style-colors', action='store_true',
                    help='st_set_style_color_match (with --grid: st_set_style_transform on every rank): linear colour transfer of the content\'s colours onto the style image')
    ap.add_argument('--laplacian', default='', metavar='P:W,...',
                    help='st_set_laplacian: the Laplacian-steered content term, levels as POOL:WEIGHT such as 4:100,16:100 (at most three; pool sizes 1, 2, 4, 8, 16, 32); not with --grid')
    ap.add_argument('--anchor', default='', metavar='IMG', help='st_set_anchor: pull the result toward this image (resized to the content\'s size); not with --grid')
    ap.add_argument('--anchor-mask', default='', metavar='M', help='with --anchor: a per-pixel map of the pull, an image (0 .. 255 -> 0 .. 1) or an .npy of (H, W) values >= 0')
    ap.add_argument('--anchor-weight', type=float, default=1.0, metavar='W', help='with --anchor: the weight of the term (default 1)')
    ap.add_argument('--jitter', type=int, default=None, metavar='R',
                    help='st_set_jitter: evaluate the network on the iterate rolled by a random shift of up to R pixels per axis in every iteration (1 .. 4096; removes the grid artefacts of pools and strides); not with --grid')
    ap.add_argument('--jitter-seed', type=int, default=None, metavar='S', help='with --jitter: the seed of the shift sequence, 0 .. 2**64 - 1 (default 0)')
    ap.add_argument('--matting', default='', metavar='W[:EPS]',
                    help='st_set_matting: the photorealism term, the matting Laplacian of the content image with the weight W such as 1e4 and the regularisation EPS in [1e-9, 1] (default 1e-7); not with --grid')
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if args.laplacian and args.grid:
        ap.error('--laplacian with --grid: tile-sharded mode does not run the Laplacian term')
    if args.anchor and args.grid:
        ap.error('--anchor with --grid: tile-sharded mode does not run the anchor term')
    if args.matting and args.grid:
        ap.error('--matting with --grid: tile-sharded mode does not run the photorealism term')
    if args.jitter and args.grid:
        ap.error('--jitter with --grid: tile-sharded mode does not run jitter')
    if args.jitter_seed is not None and args.jitter is None:
        ap.error('--jitter-seed without --jitter')
    if args.anchor_mask and not args.anchor:
        ap.error('--anchor-mask without --anchor')
    if args.ave_pools and args.grid:
        ap.error('--ave-pools with --grid: tile-sharded mode does not run average pools')

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import style_transfer2_amd as st2
    from style_transfer2_amd import jitter as st2_jitter, jobs, laplacian, matting as st2_matting, weights as st2_weights
    try:
        jit = st2_jitter.check_jitter(args.jitter, args.jitter_seed or 0) if args.jitter is not None else None
    except ValueError as err:
        ap.error('--jitter %s: %s' % (args.jitter, err))
    try:
        mat = st2_matting.parse_matting(args.matting) if args.matting else None
    except ValueError as err:
        ap.error('--matting %s: %s' % (args.matting, err))
    try:
        levels = laplacian.parse_levels(args.laplacian) if args.laplacian else None
    except ValueError as err:
        ap.error('--laplacian %s: %s' % (args.laplacian, err))

    topology = st2.VGG19_TOPOLOGY
    if args.ave_pools:
        topology = tuple(('pool', layer[1], 'ave') if layer[0] == 'pool' else layer for layer in topology)

    if args.weights.endswith('.npz'):
        params = st2_weights.load_npz(args.weights, st2.VGG19_TOPOLOGY)
    elif args.weights.endswith('.caffemodel'):
        from style_transfer2_amd import caffemodel
        params = caffemodel.vgg_params(caffemodel.read_caffemodel(args.weights), st2.VGG19_TOPOLOGY)
    else:
        params = st2_weights.he_normal(st2.VGG19_TOPOLOGY, seed=0)
    if args.grid:
        rows, cols = (int(v) for v in args.grid.split('x'))
        image = jobs.run_tiled_job(params, jobs.load_rgb(args.content), jobs.load_rgb(args.style), args.iters, (rows, cols), size=args.size,
                                   style_size=args.style_size or None, device=args.gpu, optimizer=args.optimizer, shard_style=args.shard_style,
                                   iterate_average=args.avg_decay, original_colors=args.original_colors or None,
                                   match_style_colors=args.match_style_colors or None)
    else:
        job = st2.StyleTransfer(st2.HipModel(params, topology=None if topology is st2.VGG19_TOPOLOGY else topology, device=args.gpu, precision=args.precision,
                                             conv_algo=args.conv_algo, gram_algo=args.gram_algo, pool_algo=args.pool_algo))
        content = jobs.load_rgb(args.content)
        anchor = None
        if args.anchor:                                     # the anchor and its map take the size the content image will have
            content = np.uint8(jobs.resize_to_fit(content, args.size or max(content.size)))
            hw = content.shape[:2]
            anchor = (np.uint8(jobs.load_rgb(args.anchor).resize(hw[::-1], Image.LANCZOS)),
                      jobs.load_mask(args.anchor_mask, hw) if args.anchor_mask else None, args.anchor_weight)
        image = jobs.run_job(job, content, jobs.load_rgb(args.style), args.iters, size=args.size,
                             style_size=args.style_size or None, optimizer=args.optimizer, iterate_average=args.avg_decay,
                             original_colors=args.original_colors or None, match_style_colors=args.match_style_colors or None,
                             laplacian=levels, anchor=anchor, jitter=jit[0] if jit else None, jitter_seed=jit[1] if jit else 0, matting=mat)
    Image.fromarray(np.uint8(np.clip(image, 0, 255))).save(args.out)
    print('wrote', args.out, image.shape)


if __name__ == '__main__':
    main()
