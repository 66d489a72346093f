"""What the web app does to images before they reach the worker, for headless jobs and the benchmark
(SURVEY section 8f item 4): aspect-preserving fit into a square (reference utils.py:210-229), the
uniform-noise initial image (reference app.py:82,251), and a driver that plays the app's message
sequence (app.py:244-262) against a ``StyleTransfer``."""

import numpy as np
from PIL import Image

DEFAULT_WEIGHTS = {'content': {'conv4_2': 0.08},                       # reference initial_weights.yaml:1-3
                   'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1},
                   'deepdream': {}}
DEFAULT_PARAMS = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}       # reference initial_weights.yaml:4


def fit_into_square(current_size, size, scale_up=False):
    """(w, h) scaled, aspect preserved, so that the longer side equals ``size``."""
    size = int(round(size))
    w, h = current_size
    if not scale_up and max(w, h) <= size:
        return current_size
    if w > h:
        return size, int(round(size * h / w))
    return int(round(size * w / h)), size


def resize_to_fit(image, size, scale_up=True):
    return image.resize(fit_into_square(image.size, size, scale_up), Image.LANCZOS)


def noise_image(hw, seed=None):
    """uint8 uniform noise, like ``np.uint8(np.random.uniform(0, 255, (h, w, 3)))`` in the app."""
    rng = np.random.RandomState(seed) if seed is not None else np.random
    return np.uint8(rng.uniform(0, 255, tuple(hw) + (3,)))


def load_rgb(path):
    return Image.open(path).convert('RGB')


def load_mask(path, hw):
    """A per-pixel map for the anchor term: an .npy of (H, W) values as they are, or an image read as 8-bit grey (0 .. 255, which
    Engine.set_anchor divides by 255) and resized to hw = (H, W)."""
    if str(path).endswith('.npy'):
        mask = np.load(path)
        if mask.shape != tuple(hw):
            raise ValueError('%s: a map of %s for an image of %s' % (path, mask.shape, tuple(hw)))
        return mask
    return np.uint8(Image.open(path).convert('L').resize(tuple(hw)[::-1], Image.BILINEAR))


def run_job(transfer, content, style, iterations, size=None, style_size=None, optimizer='adam', step_size=None,
            weights=None, params=None, init=None, seed=0, callback=None, iterate_average=None, original_colors=None,
            match_style_colors=None, laplacian=None, anchor=None, init_nchw=None, init_frame=None, anchor_frames=None, jitter=None,
            jitter_seed=0, matting=None):
    """One whole stylisation: content/style are PIL images or HxWx3 arrays.  Returns the final HxWx3 float32
    image.  Mirrors app.init_arrays + 'start': SetImages(reset) -> SetWeights -> SetOptimizer -> iterate.
    iterate_average: a decay in (0, 1) makes every image handed out (the callback's, the result) the bias-corrected running mean of
    the iterates (Engine.set_iterate_average); 0 turns that off; None leaves the engine as it is.
    original_colors: True makes every image handed out keep the content image's colours (the iterate's luminance, the content's chroma:
    Engine.set_original_colors); match_style_colors: True gives the style image the content image's colour mean and covariance before
    the style targets are taken (Engine.set_style_color_match).  False turns either off; None leaves the engine as it is.
    laplacian: a list of (pool, weight) pairs turns the Laplacian-steered content term on (Engine.set_laplacian: the edges and fine
    structure of the content image are held through the Laplacians of the pooled images); an empty list turns it off; None leaves
    the engine as it is.
    anchor: an (image, mask, weight) tuple turns the anchor term on (StyleTransfer.set_anchor: a per-pixel weighted pull toward the
    image, which has the content's size; HxWx3, or preprocessed planes (3, H, W)); False turns it off; None leaves the engine as it is.
    init_nchw: preprocessed planes (3, H, W) or (1, 3, H, W) to start from in place of `init` (an iterate read with
    Engine.get_input_nchw, for one).
    init_frame: (j, flow) starts from kept frame j of the engine (Engine.frame_push), warped on the device by flow (or None) in place
    of `init` (Engine.set_input_from_frame); not together with init_nchw.
    anchor_frames: (weight, [(j, flow, forward_flow, mask), ...]) turns the anchor term on from kept frames (StyleTransfer.
    anchor_from_frame): the first entry sets the anchor, the others accumulate into it; not together with anchor.
    jitter: a radius R in 1 .. 4096 makes every iteration show the network the iterate rolled by a random shift of up to R pixels per
    axis, drawn from jitter_seed (Engine.set_jitter: the grid artefacts of pools and strides go; the iterate itself never moves); 0
    turns it off; None leaves the engine as it is.
    matting: (weight, eps) or a weight alone (eps 1e-7) turns the photorealism term on (StyleTransfer.set_matting: the matting Laplacian
    of the content image keeps the result locally affine in the content's colours, so straight edges stay straight); False or 0 turns
    it off; None leaves the engine as it is."""
    from .device_optimizers import AdamOptimizer, LBFGSOptimizer
    from .matting import matting_arg
    if matting is not None:
        matting = matting_arg(matting)                      # (a ValueError before anything is set)
    if init_frame is not None and init_nchw is not None:
        raise ValueError('init_frame and init_nchw are two ways to start: give one')
    if anchor_frames is not None and anchor is not None:
        raise ValueError('anchor_frames and anchor are two ways to set the anchor term: give one')
    if anchor_frames is not None and not anchor_frames[1]:
        raise ValueError('anchor_frames: at least one (j, flow, forward_flow, mask) entry')
    if isinstance(content, Image.Image):
        content = np.uint8(resize_to_fit(content, size or max(content.size)))
    if isinstance(style, Image.Image):
        style = np.uint8(resize_to_fit(style, style_size or size or max(style.size)))
    if init_nchw is not None:
        init_nchw = np.ascontiguousarray(init_nchw, np.float32).reshape((1, 3) + tuple(content.shape[:2]))
        init = np.zeros(content.shape[:2] + (3,), np.uint8)    # (sizes the engine's buffers; the planes follow)
    elif init_frame is not None:
        init = np.zeros(content.shape[:2] + (3,), np.uint8)    # (sizes the engine's buffers; the warped frame follows)
    elif init is None:
        init = noise_image(content.shape[:2], seed)
    if original_colors is not None:
        transfer.engine.set_original_colors(original_colors)
    if match_style_colors is not None:
        transfer.engine.set_style_color_match(match_style_colors)
    transfer.set_input(init)
    if init_nchw is not None:
        transfer.engine.set_input_nchw(init_nchw)
    if init_frame is not None:
        transfer.engine.set_input_from_frame(*init_frame)
    transfer.set_content(content)
    transfer.set_style(style)
    transfer.reset()
    transfer.set_weights(weights or DEFAULT_WEIGHTS, params or DEFAULT_PARAMS)
    transfer.optimizer_cls = {'adam': AdamOptimizer, 'lbfgs': LBFGSOptimizer}[optimizer]
    transfer.set_step_size(step_size if step_size else {'adam': 10, 'lbfgs': 1}[optimizer])
    transfer.reset()
    if iterate_average is not None:
        transfer.engine.set_iterate_average(iterate_average)
    if laplacian is not None:
        transfer.set_laplacian(laplacian)
    if anchor is not None:
        if anchor is False:
            transfer.set_anchor(None)
        else:
            image, mask, weight = anchor
            transfer.set_anchor(image, mask, weight)
    if matting is not None:
        transfer.set_matting(*matting)
    if jitter is not None:
        transfer.engine.set_jitter(jitter, jitter_seed)     # (after the resets: the shift sequence starts at step 0 of this job)
    if anchor_frames is not None:
        weight, entries = anchor_frames
        for k, (j, flow, forward_flow, mask) in enumerate(entries):
            transfer.anchor_from_frame(j, flow, forward_flow, mask, weight, accumulate=k > 0)
    if not transfer.start():
        raise RuntimeError('job could not start: inconsistent images')
    image = None
    for i in range(iterations):
        last = i == iterations - 1
        if callback is None and not last:
            transfer.step_async()
        else:
            image, trace = transfer.step()
            if callback is not None:
                callback(i + 1, image, trace)
    return image


def run_tiled_job(net_params, content, style, iterations, grid, size=None, style_size=None, weights=None, params=None, init=None,
                  seed=0, device=0, precision='fp32', topology=None, callback=None, optimizer='adam', step_size=None, shard_style=False,
                  iterate_average=None, original_colors=None, match_style_colors=None, laplacian=None, anchor=None, matting=None):
    """The same job for an image no single engine holds (an 8192 x 8192 image has conv1 blobs of 17 GB each): the image is cut into
    grid = (rows, cols) tiles, every tile + apron is an engine context of THIS process on the one GPU (tiled.InProcessFabric: one
    thread per rank, the all-reduces and strip exchanges are device-to-device copies); one st_tile_step per rank and iteration, Adam or
    L-BFGS (the Gram form: one all-reduce of the new inner products per step).
    Same result as run_job where both can run (tests/test_gpu_jobs.py).  Image edges must be multiples of 16 * rows / cols
    (tiling.TileGrid).  shard_style: the style image is cut as well (tiling.style_grid over the same ranks, up to the deepest
    style-weighted blob) and every rank forwards one window of it, instead of every rank forwarding all of it.
    iterate_average: a decay in (0, 1) makes every rank keep the running mean of its window's iterates; the stitched image is then the
    bias-corrected mean, as run_job's is.
    original_colors: every rank hands out its tile with the chroma of its own window of the content image (per pixel: the stitched image
    is run_job's).  match_style_colors: the colour moments of the WHOLE content and style images are taken once, through rank 0's engine,
    and the transform derived from them goes to every rank (Engine.set_style_transform) before the style is set, plain or shard_style.
    laplacian: the Laplacian term does not run tile-sharded (st_set_laplacian refuses a tile-configured context): any levels, here or
    in params['laplacian'], are a ValueError before anything is built.
    anchor: the anchor term does not run tile-sharded either (st_set_anchor refuses a tile-configured context): a ValueError as well.
    matting: nor does the photorealism term (st_set_matting refuses a tile-configured context): a ValueError as well.
    Returns the stitched HxWx3 float32 image; callback(i, trace values) after every iteration."""
    if matting:
        raise ValueError('the photorealism term does not run tile-sharded: use run_job, or drop matting')
    if anchor:
        raise ValueError('the anchor term does not run tile-sharded: use run_job, or drop the anchor')
    if laplacian or (params and params.get('laplacian')):
        raise ValueError('the Laplacian term does not run tile-sharded: use run_job, or drop the levels')
    from . import tiled, tiling
    from .engine import VGG19_TOPOLOGY
    from .tile_backend import HipTileBackend
    topology = topology or VGG19_TOPOLOGY
    if isinstance(content, Image.Image):
        content = np.uint8(resize_to_fit(content, size or max(content.size)))
    if isinstance(style, Image.Image):
        style = np.uint8(resize_to_fit(style, style_size or size or max(style.size)))
    if init is None:
        init = noise_image(content.shape[:2], seed)
    weights, params = weights or DEFAULT_WEIGHTS, params or DEFAULT_PARAMS
    rows, cols = grid
    h, w = content.shape[:2]
    deepest = max(i for i, layer in enumerate(topology) if any(layer[1] in weights[k] and weights[k][layer[1]] for k in weights))
    tg = tiling.TileGrid(h, w, rows, cols, topology, deepest + 1)
    world = rows * cols
    fabric = tiled.InProcessFabric(world, timeout=600.0)
    ranks, backends = [], []
    # colour matching: rank 0's backend derives A, b from the whole images before it sets its style; the other ranks are given them
    transform = (content, style) if match_style_colors else None
    for r in range(world):
        b = HipTileBackend(net_params, tg, r, content, None if shard_style else style, init, weights, params, step_size=step_size or {'adam': 10, 'lbfgs': 1}[optimizer],
                           topology=topology, device=device, precision=precision, optimizer=optimizer, iterate_average=iterate_average,
                           original_colors=original_colors, style_transform=transform)
        if r == 0 and match_style_colors:
            transform = b.style_transform
        backends.append(b)
        b.comm_init_local(r, world, fabric)
        ranks.append(tiled.FusedTiledTransfer(tg, r, b))
    try:
        if shard_style:
            styled = [i for i, layer in enumerate(topology) if weights.get('style', {}).get(layer[1])]
            sg = tiling.style_grid(style.shape[0], style.shape[1], world, topology, max(styled) + 1 if styled else 0)
            tiled.run_collective([lambda b=b: b.shard_style(style, sg) for b in backends], fabric, in_turns=True)
        for i in range(iterations):
            vals = tiled.run_in_process(ranks, 1, fabric)[0][0]
            if callback is not None:
                callback(i + 1, vals)
        image = np.zeros((h, w, 3), np.float32)
        for r in range(world):
            t = tg.tiles[r]
            image[t.y0:t.y1, t.x0:t.x1] = ranks[r].tile_image()
    except RuntimeError as err:
        if getattr(err, 'still_running', False):     # a rank thread is still inside the engine: freeing its context under it would
            backends = []                            # pull device memory from running kernels -- leak the contexts and report
        raise
    finally:
        for b in backends:
            b.engine.close()
    return image


def warp_planar(x_chw, flow_hw2):
    """Backward bilinear warp of planes (C, H, W) by a flow field (H, W, 2) of (dx, dy) in pixels:
    out[:, y, x] = bilinear(x_chw, y + flow[y, x, 1], x + flow[y, x, 0]), sample coordinates clamped to the image.  Computed in float64,
    returned as float32.  Frame sequences warp the previous stylised frame onto the next one with it (run_frames)."""
    x = np.asarray(x_chw, np.float64)
    flow = np.asarray(flow_hw2, np.float64)
    if x.ndim != 3 or flow.shape != x.shape[1:] + (2,):
        raise ValueError('planes (C, H, W) and a flow (H, W, 2) of the same size, got %s and %s' % (x.shape, flow.shape))
    h, w = x.shape[1:]
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    sy = np.clip(yy + flow[..., 1], 0, h - 1)
    sx = np.clip(xx + flow[..., 0], 0, w - 1)
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    fy, fx = sy - y0, sx - x0
    top = x[:, y0, x0] * (1 - fx) + x[:, y0, x1] * fx
    bottom = x[:, y1, x0] * (1 - fx) + x[:, y1, x1] * fx
    return (top * (1 - fy) + bottom * fy).astype(np.float32)


def _long_term_keys(long_term):
    js = sorted(long_term or ())
    for j in js:
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 2 <= j <= 8:
            raise ValueError('long_term: the keys are integers from 2 to 8, got %r' % (j,))
    return [int(j) for j in js]


def estimate_flows(engine, frames, long_term=(), **params):
    """Every optical flow run_frames reads, estimated on the device from the frames themselves (Engine.flow_estimate; st2.h:
    st_flow_estimate).  frames: HxWx3 arrays of one size, as they are stylised.  long_term: the distances j (2 .. 8) to estimate as well.
    params: alpha, warps, iters, levels (flow.DEFAULTS).  Returns (flows, forward_flows, long_term) in the shapes run_frames takes:
    flows[t] = estimate(frames[t], frames[t - 1]), forward_flows[t] = estimate(frames[t - 1], frames[t]), entry 0 None;
    long_term = {j: (flows_j, forward_flows_j)} likewise against frame t - j, entries below j None."""
    frames = [np.asarray(f) for f in frames]
    if len({f.shape for f in frames}) > 1:
        raise ValueError('the frames differ in size: %s' % sorted({f.shape[:2] for f in frames}))

    def pair(j):
        back = [None if t < j else engine.flow_estimate(frames[t], frames[t - j], **params) for t in range(len(frames))]
        forth = [None if t < j else engine.flow_estimate(frames[t - j], frames[t], **params) for t in range(len(frames))]
        return back, forth
    flows, forward_flows = pair(1)
    return flows, forward_flows, {j: pair(j) for j in _long_term_keys(long_term)}


def _filled(given, estimated):
    """Per frame the caller's entry where there is one, else the estimated one."""
    if given is None:
        return estimated
    if len(given) != len(estimated):
        return given                                       # (run_frames' own checks name the sequence)
    return [e if g is None else g for g, e in zip(given, estimated)]


def fill_flows(engine, frames, flows=None, forward_flows=None, long_term=None, **params):
    """run_frames' (flows, forward_flows, long_term) with every flow the caller did not give estimated from the frames (estimate_flows
    with params); what is given wins, entry by entry.  long_term: a dict {j: (flows_j, forward_flows_j or None) or None}, or a plain
    sequence of distances.  The estimates' scratch on the device is released before returning."""
    given = long_term if isinstance(long_term, dict) else {j: None for j in (long_term or ())}
    for j in _long_term_keys(given):
        pair = given[j]
        if pair is not None and (not isinstance(pair, (tuple, list)) or len(pair) != 2):
            raise ValueError('long_term[%d]: a (flows, forward_flows or None) pair, or None to estimate both' % j)
    est_flows, est_forward, est_long = estimate_flows(engine, frames, long_term=given, **params)
    engine.flow_release()                                  # (the jobs run with the memory they have without the estimates)
    out = {}
    for j, (back, forth) in est_long.items():
        pair = given[j]
        out[j] = (_filled(pair[0], back), _filled(pair[1], forth)) if pair is not None else (back, forth)
    return _filled(flows, est_flows), _filled(forward_flows, est_forward), out


def run_frames(transfer, frames, style, iterations, anchor_weight, flows=None, masks=None, first_iterations=None, forward_flows=None,
               long_term=None, jitter=None, jitter_seed=0, estimate=None, **job_kwargs):
    """A frame sequence with temporal consistency (Ruder et al.): frame 0 is a plain run_job (first_iterations of them where given);
    frame t > 0 starts from the raw iterate of frame t - 1 (kept on the device, Engine.frame_push: never the averaged or recoloured
    image handed out), warped by flows[t] ((H, W, 2), from frame t back to frame t - 1; the arithmetic of warp_planar) where one is
    given, and is pulled toward that same image by the anchor term with anchor_weight and a map.  The seam between two frames runs on
    the device (Engine.set_input_from_frame, Engine.anchor_from_frame): no iterate crosses to the host.
    masks[t]: the caller's map (the flow's reliability; None: 1 everywhere).  forward_flows[t] ((H, W, 2), from frame t - 1 to frame t)
    turns the derived reliability on (st2.h: forward / backward consistency, motion boundaries, samples outside the image), which
    masks[t] multiplies where given; it needs flows[t].
    long_term: {j: (flows_j, forward_flows_j or None)} with integer 2 <= j <= 8: flows_j[t] goes from frame t back to frame t - j and is
    read for t >= j (a None entry skips that pair).  Pixels the map of frame t - 1 leaves free are then anchored to the newest of those
    older stylised frames that reliably shows them (the j in ascending order): Ruder's long-term consistency as one anchor term.  It
    needs a map from forward_flows or masks at every frame it applies to.
    frames: HxWx3 arrays of one size; flows, masks, forward_flows, flows_j: sequences as long as frames (entry 0 is not read) or None.
    jitter, jitter_seed: run_job's, for every frame: each frame's job draws the same shift sequence from step 0.
    estimate: None, or a dict of estimate_flows' parameters (possibly empty): every flow the caller did not give -- flows, forward_flows
    and, for every key of long_term (then also a plain sequence of distances, or a dict with None in place of a pair), both of its
    sequences -- is estimated on the device from the frames (estimate_flows) before the first job; entries that are given win.  With
    estimate=None nothing is estimated, and flows=None still means "no warp".
    job_kwargs go to every run_job.  Returns the list of results."""
    frames = [np.asarray(f) for f in frames]
    if len({f.shape for f in frames}) > 1:
        raise ValueError('the frames differ in size: %s' % sorted({f.shape[:2] for f in frames}))
    hw = frames[0].shape[:2] if frames else (0, 0)
    if estimate is not None:
        flows, forward_flows, long_term = fill_flows(transfer.engine, frames, flows, forward_flows, long_term, **dict(estimate))
    older = []                                             # (j, flows_j, forward_flows_j), ascending
    for j, pair in (long_term or {}).items():
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 2 <= j <= 8:
            raise ValueError('long_term: the keys are integers from 2 to 8, got %r' % (j,))
        if not isinstance(pair, (tuple, list)) or len(pair) != 2 or pair[0] is None:
            raise ValueError('long_term[%d]: a (flows, forward_flows or None) pair' % j)
        older.append((int(j), pair[0], pair[1]))
    older.sort(key=lambda e: e[0])
    named = [('flows', flows, 1, 2), ('masks', masks, 1, 0), ('forward_flows', forward_flows, 1, 2)]
    for j, fl, ff in older:
        named += [('long_term[%d] flows' % j, fl, j, 2), ('long_term[%d] forward_flows' % j, ff, j, 2)]
    for name, seq, first, last_axis in named:
        if seq is None:
            continue
        if len(seq) != len(frames):
            raise ValueError('%s: one entry per frame (entry 0 is not read), got %d for %d frames' % (name, len(seq), len(frames)))
        want = tuple(hw) + ((last_axis,) if last_axis else ())
        for t in range(first, len(frames)):
            if seq[t] is not None and np.shape(seq[t]) != want:
                raise ValueError('%s[%d]: %s for frames of %s, expected %s' % (name, t, np.shape(seq[t]), tuple(hw), want))
    for t in range(1, len(frames)):
        if forward_flows is not None and forward_flows[t] is not None and (flows is None or flows[t] is None):
            raise ValueError('forward_flows[%d] without flows[%d]: the reliability needs both directions' % (t, t))
        for j, fl, ff in older:
            if t < j or fl[t] is None:
                if t >= j and ff is not None and ff[t] is not None:
                    raise ValueError('long_term[%d] forward_flows[%d] without its flows[%d]' % (j, t, t))
                continue
            if (forward_flows is None or forward_flows[t] is None) and (masks is None or masks[t] is None):
                raise ValueError('long_term at frame %d needs a map of frame %d: give forward_flows[%d] or masks[%d]' % (t, t - 1, t, t))
    transfer.engine.frames_keep(max([1] + [j for j, _, _ in older]))
    results = []
    for t, frame in enumerate(frames):
        if t == 0:
            results.append(run_job(transfer, frame, style, first_iterations or iterations, anchor=False, jitter=jitter, jitter_seed=jitter_seed, **job_kwargs))
        else:
            flow = flows[t] if flows is not None else None
            entries = [(1, flow, forward_flows[t] if forward_flows is not None else None, masks[t] if masks is not None else None)]
            entries += [(j, fl[t], ff[t] if ff is not None else None, None) for j, fl, ff in older if t >= j and fl[t] is not None]
            results.append(run_job(transfer, frame, style, iterations, init_frame=(1, flow), anchor_frames=(anchor_weight, entries), jitter=jitter,
                                   jitter_seed=jitter_seed, **job_kwargs))
        transfer.engine.frame_push()
    return results
