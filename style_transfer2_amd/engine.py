"""Thin object view of the C ABI: one ``Engine`` == one ``st_ctx`` == one reference worker's
model + objective + optimizer, resident on one MI355X."""

import ctypes
from ctypes import POINTER, byref, c_double, c_float, c_int, c_longlong, c_ulonglong, c_void_p

import numpy as np

from . import capi, prototxt
from . import flow as flow_mod
from .capi import check

F32 = np.float32
OPT_ADAM, OPT_LBFGS = 1, 2

# reference models/vgg19.prototxt:1-337
VGG19_TOPOLOGY = (
    ('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 64), ('pool', 'pool1'),
    ('conv', 'conv2_1', 64, 128), ('conv', 'conv2_2', 128, 128), ('pool', 'pool2'),
    ('conv', 'conv3_1', 128, 256), ('conv', 'conv3_2', 256, 256),
    ('conv', 'conv3_3', 256, 256), ('conv', 'conv3_4', 256, 256), ('pool', 'pool3'),
    ('conv', 'conv4_1', 256, 512), ('conv', 'conv4_2', 512, 512),
    ('conv', 'conv4_3', 512, 512), ('conv', 'conv4_4', 512, 512), ('pool', 'pool4'),
    ('conv', 'conv5_1', 512, 512), ('conv', 'conv5_2', 512, 512),
    ('conv', 'conv5_3', 512, 512), ('conv', 'conv5_4', 512, 512), ('pool', 'pool5'),
)


def _ptr(a):
    return a.ctypes.data_as(c_void_p) if a is not None else None


def _image_arg(image):
    """HxWx3 uint8 or anything float-convertible -> (contiguous array, is_u8)."""
    arr = np.asarray(image)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError('image must be HxWx3, got %s' % (arr.shape,))
    if arr.dtype == np.uint8:
        return np.ascontiguousarray(arr), 1
    return np.ascontiguousarray(arr, F32), 0


def _map_arg(mask, h, w):
    """A per-pixel map of the anchor term -> contiguous float32 (h, w): float as it is, uint8 divided by 255, bool as 0 / 1; None stays."""
    if mask is None:
        return None
    mask = np.asarray(mask)
    if mask.shape != (h, w):
        raise ValueError('the map must be (%d, %d), got %s' % (h, w, mask.shape))
    if mask.dtype == np.uint8:
        mask = mask.astype(F32) / F32(255)
    return np.ascontiguousarray(mask, F32)                  # (bool: 0 / 1)


def _flow_arg(flow, h, w, name='flow'):
    """An optical flow (h, w, 2) of (dx, dy) in pixels -> contiguous float32; None stays."""
    if flow is None:
        return None
    flow = np.asarray(flow)
    if flow.shape != (h, w, 2):
        raise ValueError('the %s must be (%d, %d, 2), got %s' % (name, h, w, flow.shape))
    return np.ascontiguousarray(flow, F32)


def cov_full(upper):
    """The six values RR, RG, RB, GG, GB, BB of the C ABI -> symmetric (3, 3) float64."""
    rr, rg, rb, gg, gb, bb = (float(v) for v in upper)
    return np.array(((rr, rg, rb), (rg, gg, gb), (rb, gb, bb)), np.float64)


def color_transform(mean_c, cov_c, mean_s, cov_s):
    """Linear colour transfer (st_color_transform; host only, no engine): (A (3, 3), b (3,)) float32 such that s' = A s + b, in
    preprocessed coordinates, gives pixels with colour mean mean_s and covariance cov_s (3, 3) the mean mean_c and covariance cov_c."""
    def upper(cov):
        cov = np.asarray(cov, np.float64).reshape(3, 3)
        return (c_double * 6)(cov[0, 0], cov[0, 1], cov[0, 2], cov[1, 1], cov[1, 2], cov[2, 2])
    mc = (c_double * 3)(*[float(v) for v in mean_c])
    ms = (c_double * 3)(*[float(v) for v in mean_s])
    A, b = (c_float * 9)(), (c_float * 3)()
    check(capi.load_library().st_color_transform(mc, upper(cov_c), ms, upper(cov_s), A, b))
    return np.array(A[:], F32).reshape(3, 3), np.array(b[:], F32)


class Engine:
    def __init__(self, topology=None, device=0, precision='fp32'):
        self.lib = capi.load_library()
        self.precision = precision
        self._ctx = c_void_p()
        self.topology = tuple(topology) if topology is not None else VGG19_TOPOLOGY
        if topology is None:
            check(self.lib.st_create(byref(self._ctx), int(device), None, 0))
        else:
            descs = (capi.LayerDesc * len(self.topology))()
            self._names = []          # keep the byte strings alive
            for d, layer in zip(descs, self.topology):
                name = layer[1].encode()
                self._names.append(name)
                # ST_LAYER_CONV / ST_LAYER_POOL / ST_LAYER_AVEPOOL ('pool', name, 'ave': prototxt `pool: AVE`)
                d.kind = 0 if layer[0] == 'conv' else (2 if prototxt.pool_method(layer) == 'ave' else 1)
                d.name = name
                d.cin, d.cout = (layer[2], layer[3]) if layer[0] == 'conv' else (0, 0)
            check(self.lib.st_create(byref(self._ctx), int(device), descs, len(self.topology)))
        # 'bf16-full' = the bf16 feature path with every fp32 blob / diff materialised (A/B reference of the lean data flow)
        self.set_precision(precision)
        n = self.lib.st_num_blobs(self._ctx)
        self.blob_names = [self.lib.st_blob_name(self._ctx, i).decode() for i in range(n)]
        self._index = {name: i for i, name in enumerate(self.blob_names)}

    PRECISIONS = {'fp32': 0, 'bf16': 1, 'bf16-full': 2}

    def set_precision(self, precision):
        """'fp32', 'bf16' (lean data flow: blobs only bf16 convs read are not materialised in fp32) or 'bf16-full' (same arithmetic,
        every blob / diff written in fp32 as well).  Takes effect from the next evaluation."""
        if precision not in self.PRECISIONS:
            raise ValueError('precision must be one of %s' % sorted(self.PRECISIONS))
        check(self.lib.st_set_precision(self._ctx, self.PRECISIONS[precision]))
        self.precision = precision

    def graph_replays(self):
        """Number of steps that ran as a hipGraph replay (steady-state Adam steps at small image sizes)."""
        n = c_longlong()
        check(self.lib.st_graph_replays(self._ctx, byref(n)))
        return n.value

    def set_conv_algo(self, winograd):
        """True / 1 (default): eligible fp32 convs run as Winograd F(2x2,3x3) on the fp32 matrix cores; False / 0: direct kernel only;
        2: Winograd with the transform-domain products as six bf16 partial products of split operands (fp32 results) where the shape allows."""
        if winograd not in (0, 1, 2):         # (False == 0 and True == 1)
            raise ValueError('conv_algo must be 0 (direct), 1 (Winograd, fp32 matrix cores) or 2 (split-operand Winograd), not %r' % (winograd,))
        check(self.lib.st_set_conv_algo(self._ctx, int(winograd)))

    def set_gram_algo(self, algo):
        """0 (default): Gram partials and style gradients of fp32 features on the fp32 matrix cores; 1: as six bf16 partial products of
        three-way split operands on the bf16 matrix cores (fp32 results) where the shape allows.  Applies to every Gram computed afterwards
        (style targets included); no effect on the bf16 feature path or in tile-sharded mode."""
        if algo not in (0, 1):
            raise ValueError('gram_algo must be 0 (fp32 matrix cores) or 1 (split operands), not %r' % (algo,))
        check(self.lib.st_set_gram_algo(self._ctx, int(algo)))

    def algos(self):
        """(conv_algo, gram_algo) in force."""
        conv, gram = c_int(), c_int()
        check(self.lib.st_get_algos(self._ctx, byref(conv), byref(gram)))
        return conv.value, gram.value

    def set_pool_algo(self, algo):
        """0 (default): every average pool is a stand-alone pass; 1: an average pool rides on the bf16 conv launches around it in the lean
        'bf16' flow (same results bit for bit; every other precision and evaluation routes as under 0).  Takes effect from the next
        evaluation."""
        if algo not in (0, 1):
            raise ValueError('pool_algo must be 0 (stand-alone passes) or 1 (fused into the bf16 conv launches), not %r' % (algo,))
        check(self.lib.st_set_pool_algo(self._ctx, int(algo)))

    def pool_algo(self):
        """The pool_algo in force."""
        algo = c_int()
        check(self.lib.st_get_pool_algo(self._ctx, byref(algo)))
        return algo.value

    # -- lifecycle -------------------------------------------------------------------------------
    def close(self):
        if self._ctx:
            self.lib.st_destroy(self._ctx)
            self._ctx = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- model -----------------------------------------------------------------------------------
    def load_weights(self, params):
        """params: {conv name: (w (Cout,Cin,3,3), b (Cout,))}"""
        for layer in self.topology:
            if layer[0] != 'conv':
                continue
            w, b = params[layer[1]]
            w = np.ascontiguousarray(w, F32)
            b = np.ascontiguousarray(b, F32)
            if w.shape != (layer[3], layer[2], 3, 3) or b.shape != (layer[3],):
                raise ValueError('%s: bad weight shapes %s %s' % (layer[1], w.shape, b.shape))
            check(self.lib.st_load_conv_weights(self._ctx, layer[1].encode(), _ptr(w), _ptr(b)))

    def blob_index(self, name):
        return self._index[name]

    def blob_shape(self, name, h, w):
        c, bh, bw = c_int(), c_int(), c_int()
        check(self.lib.st_blob_shape(self._ctx, self._index[name], h, w, byref(c), byref(bh), byref(bw)))
        return c.value, bh.value, bw.value

    def forward(self, x_nchw, last=None):
        x = np.ascontiguousarray(x_nchw, F32)
        assert x.ndim == 4 and x.shape[:2] == (1, 3)
        self._fwd_hw = x.shape[2:]
        last_i = -1 if last is None else self._index[last]
        check(self.lib.st_forward(self._ctx, _ptr(x), x.shape[2], x.shape[3], last_i))

    def get_blob(self, name):
        """Host copy of a blob of the last forward (st_forward, or the forward inside the last opfunc / step)."""
        h, w = getattr(self, '_fwd_hw', None) or self.input_shape()
        out = np.empty((1,) + self.blob_shape(name, h, w), F32)
        check(self.lib.st_get_blob(self._ctx, self._index[name], _ptr(out)))
        return out

    def backward(self, diffs):
        h, w = self._fwd_hw
        names = list(diffs)
        arrs = [np.ascontiguousarray(diffs[n], F32) for n in names]
        for n, a in zip(names, arrs):
            if a.shape != (1,) + self.blob_shape(n, h, w):
                raise ValueError('diff for %s has shape %s' % (n, a.shape))
        idx = (c_int * len(names))(*[self._index[n] for n in names])
        ptrs = (c_void_p * len(names))(*[a.ctypes.data for a in arrs])
        out = np.empty((1, 3, h, w), F32)
        check(self.lib.st_backward(self._ctx, len(names), idx, ptrs, _ptr(out)))
        return out

    def gram(self, name):
        c = self.blob_shape(name, *self._fwd_hw)[0]
        out = np.empty((c, c), F32)
        check(self.lib.st_gram(self._ctx, self._index[name], _ptr(out)))
        return out

    def layer_terms(self, name, want=('D', 'raw_S', 'diff', 'norms')):
        """Test hook (st_get_layer_terms): what the last objective evaluation left for a blob -- a dict with the entries of `want`:
        'D' (C, C) = G - G_style as the style-gradient launch read it, 'raw_S' (1, C, h, w) the unscaled style gradient (first
        evaluation after reset() only), 'diff' (1, C, h, w) the injected layer diff, 'norms' (3,) = c, s, d.  StError where the shared
        buffers no longer (or never did) hold that blob's data."""
        unknown = set(want) - {'D', 'raw_S', 'diff', 'norms'}
        if unknown:
            raise ValueError('unknown layer term(s) %s' % sorted(unknown))
        shape = self.blob_shape(name, *self.input_shape())
        out = {}
        if 'D' in want:
            out['D'] = np.empty((shape[0], shape[0]), F32)
        for k in ('raw_S', 'diff'):
            if k in want:
                out[k] = np.empty((1,) + shape, F32)
        norms = (c_float * 3)()
        check(self.lib.st_get_layer_terms(self._ctx, self._index[name], _ptr(out.get('D')), _ptr(out.get('raw_S')),
                                          _ptr(out.get('diff')), norms if 'norms' in want else None))
        if 'norms' in want:
            out['norms'] = np.array(norms[:], F32)
        return out

    def tap_diff(self, name):
        """Test hook (st_tap_diff): from now on every opfunc(return_grad=True) copies the running diff of blob `name` right after the
        launch that wrote it; None turns the tap off.  step() / step_begin() are refused while a tap is set."""
        check(self.lib.st_tap_diff(self._ctx, -1 if name is None else self._index[name]))
        self._tapped = name

    def tapped_diff(self):
        """Test hook (st_get_tapped_diff): {'f32': (1, C, h, w) or None, 'bf16': (1, C, h, w) float32 holding bf16 values or None} --
        the forms the tapped launch of the last opfunc(return_grad=True) wrote.  StError before such an evaluation has completed
        and after the iterate was resized."""
        name = getattr(self, '_tapped', None)
        if name is None:
            check(self.lib.st_get_tapped_diff(self._ctx, None, None, None, None))        # (refuses: no diff is tapped)
        C, h, w = self.blob_shape(name, *self.input_shape())
        cb = (C + 7) // 8
        o32, o16 = np.empty((1, C, h, w), F32), np.empty((cb, h * w, 8), np.uint16)
        h32, h16 = c_int(), c_int()
        check(self.lib.st_get_tapped_diff(self._ctx, _ptr(o32), _ptr(o16), byref(h32), byref(h16)))
        out = {'f32': o32 if h32.value else None, 'bf16': None}
        if h16.value:           # channel-blocked [C/8][hw][8] -> (C, h, w); a bf16 value is the upper half of a float32
            bits = o16.transpose(0, 2, 1).reshape(cb * 8, h * w)[:C].astype(np.uint32) << 16
            out['bf16'] = np.ascontiguousarray(bits).view(F32).reshape(1, C, h, w)
        return out

    # -- image slots -------------------------------------------------------------------------------
    def set_input(self, image):
        arr, u8 = _image_arg(image)
        check(self.lib.st_set_input(self._ctx, _ptr(arr), arr.shape[0], arr.shape[1], u8))

    def set_content(self, image):
        arr, u8 = _image_arg(image)
        check(self.lib.st_set_content(self._ctx, _ptr(arr), arr.shape[0], arr.shape[1], u8))

    def set_style(self, image):
        arr, u8 = _image_arg(image)
        check(self.lib.st_set_style(self._ctx, _ptr(arr), arr.shape[0], arr.shape[1], u8))

    # -- the style targets of a tile-sharded job, sharded as well (st_tile_set_style; tiling.style_grid has the geometry) ------
    def _style_tile_args(self, window_image, grid_hw, window, tile, last):
        """(image pointer or NULL, the 12 integers of the C ABI, the array kept alive).  window_image None: this rank has no style tile."""
        last_i = self._index[last] if isinstance(last, str) else int(last)
        if window_image is None:
            return None, [0, 0, 0, int(grid_hw[0]), int(grid_hw[1]), 0, 0, 0, 0, 0, 0, last_i], None
        arr, u8 = _image_arg(window_image)
        geo = [arr.shape[0], arr.shape[1], u8, int(grid_hw[0]), int(grid_hw[1]), int(window[0]), int(window[1])] + [int(v) for v in tile]
        return _ptr(arr), geo + [last_i], arr

    def tile_set_style(self, window_image, grid_hw, window=(0, 0), tile=None, last=None):
        """Collective over the communicator of this context (every rank calls it, after st_comm_init / st_comm_callbacks): the style
        targets of blobs 0 .. `last` from the raw Gram sums of every rank's tile of the style image, all-reduced.  window_image is this
        rank's window (tile + apron) of the grid_hw = (gH, gW) style image, window = (wy0, wx0) its origin, tile = (ty0, tx0, ty1, tx1)
        in global pixels (default: the window is the whole image); None: this rank has no tile and contributes zeros."""
        last = len(self.blob_names) - 1 if last is None else last
        if tile is None and window_image is not None:
            tile = (0, 0, int(grid_hw[0]), int(grid_hw[1]))
        p, ints, keep = self._style_tile_args(window_image, grid_hw, window, tile, last)
        check(self.lib.st_tile_set_style(self._ctx, p, *ints))

    def tile_style_partials(self, window_image, grid_hw, window=(0, 0), tile=None, last=None):
        """The first half of tile_set_style for a caller that all-reduces itself: (device pointer, number of floats) of this rank's
        raw Gram sums, blobs 0 .. `last` back to back; tile_style_commit() after the all-reduce."""
        last = len(self.blob_names) - 1 if last is None else last
        if tile is None and window_image is not None:
            tile = (0, 0, int(grid_hw[0]), int(grid_hw[1]))
        p, ints, keep = self._style_tile_args(window_image, grid_hw, window, tile, last)
        dev, n = c_void_p(), c_int()
        check(self.lib.st_tile_style_partials(self._ctx, p, *ints, byref(dev), byref(n)))
        return dev.value, n.value

    def tile_style_commit(self):
        check(self.lib.st_tile_style_commit(self._ctx))

    def style_gram(self, name):
        """Host copy of the style target (C x C) of a blob; an error if the context holds none for it."""
        i = self._index[name]
        c = self.blob_shape(name, 16, 16)[0]
        out = np.empty((c, c), F32)
        check(self.lib.st_get_style_gram(self._ctx, i, _ptr(out)))
        return out

    def set_input_nchw(self, x):
        x = np.ascontiguousarray(x, F32)
        check(self.lib.st_set_input_nchw(self._ctx, _ptr(x), x.shape[2], x.shape[3]))

    def set_content_nchw(self, x):
        x = np.ascontiguousarray(x, F32)
        check(self.lib.st_set_content_nchw(self._ctx, _ptr(x), x.shape[2], x.shape[3]))

    def input_shape(self):
        h, w = c_int(), c_int()
        check(self.lib.st_input_shape(self._ctx, byref(h), byref(w)))
        return h.value, w.value

    def get_input_nchw(self):
        h, w = self.input_shape()
        out = np.empty((1, 3, h, w), F32)
        check(self.lib.st_get_input_nchw(self._ctx, _ptr(out)))
        return out

    # -- objective -----------------------------------------------------------------------------------
    def set_weights(self, rows, content, style, deepdream, params4):
        n = len(rows)
        idx = (c_int * n)(*[self._index[r] for r in rows])
        cw = (c_float * n)(*[float(v) for v in content])
        sw = (c_float * n)(*[float(v) for v in style])
        dw = (c_float * n)(*[float(v) for v in deepdream])
        pr = (c_double * 4)(*[float(v) for v in params4])
        check(self.lib.st_set_weights(self._ctx, n, idx, cw, sw, dw, pr))

    def clear_norms(self):
        check(self.lib.st_clear_norms(self._ctx))

    def trace_len(self):
        return self.lib.st_trace_len(self._ctx)

    def opfunc(self, return_grad=True):
        h, w = self.input_shape()
        loss = c_float()
        trace = np.zeros(self.trace_len(), np.float64)
        grad = np.empty((1, 3, h, w), F32) if return_grad else None
        check(self.lib.st_opfunc(self._ctx, byref(loss), _ptr(grad), _ptr(trace)))
        self._fwd_hw = (h, w)           # the blobs up to the deepest weighted layer are those of this evaluation
        return F32(loss.value), grad, trace

    # -- optimizer -----------------------------------------------------------------------------------
    def optimizer_reset(self, kind, step_size):
        check(self.lib.st_optimizer_reset(self._ctx, kind, float(step_size)))

    def optimizer_set_step(self, step_size):
        check(self.lib.st_optimizer_set_step(self._ctx, float(step_size)))

    def objective_changed(self):
        check(self.lib.st_objective_changed(self._ctx))

    def adam_get_state(self):
        h, w = self.input_shape()
        m = np.empty((1, 3, h, w), F32)
        v = np.empty((1, 3, h, w), F32)
        i1, i2 = c_int(), c_int()
        check(self.lib.st_adam_get_state(self._ctx, _ptr(m), _ptr(v), byref(i1), byref(i2)))
        return m, v, i1.value, i2.value

    def adam_set_state(self, m, v, items1, items2):
        m = np.ascontiguousarray(m, F32)
        v = np.ascontiguousarray(v, F32)
        check(self.lib.st_adam_set_state(self._ctx, _ptr(m), _ptr(v), int(items1), int(items2)))

    # -- device-resident resampling (Pillow-exact) -------------------------------------------------------
    @staticmethod
    def _table(in_size, out_size, method):
        from . import resample
        lo, n, k = resample.pillow_coeffs(in_size, out_size, method)
        t = capi.ResampleTable()
        t._keep = (np.ascontiguousarray(lo), np.ascontiguousarray(n), np.ascontiguousarray(k))
        t.lo = t._keep[0].ctypes.data_as(ctypes.POINTER(c_int))
        t.n = t._keep[1].ctypes.data_as(ctypes.POINTER(c_int))
        t.k = t._keep[2].ctypes.data_as(ctypes.POINTER(c_double))
        t.kmax, t.out_size = k.shape[1], out_size
        return t

    def resample_state(self, size, new_x=None):
        """optimizer.resample (optimizers.py:29-40,110-119) on the device: x (Lanczos, or replaced by new_x),
        Adam m (Lanczos), Adam v (bilinear, clipped at 0)."""
        from . import resample
        h, w = self.input_shape()
        if new_x is not None:
            new_x = np.ascontiguousarray(new_x, F32)
            size = new_x.shape[2:]
        size = tuple(int(v) for v in size)
        lx, ly = self._table(w, size[1], resample.LANCZOS), self._table(h, size[0], resample.LANCZOS)
        bx, by = self._table(w, size[1], resample.BILINEAR), self._table(h, size[0], resample.BILINEAR)
        check(self.lib.st_resample_state(self._ctx, byref(lx), byref(ly), byref(bx), byref(by), _ptr(new_x)))

    def resample_content(self, size):
        from . import resample
        h, w = self.content_shape()
        size = tuple(int(v) for v in size)
        lx, ly = self._table(w, size[1], resample.LANCZOS), self._table(h, size[0], resample.LANCZOS)
        check(self.lib.st_resample_content(self._ctx, byref(lx), byref(ly)))

    def content_shape(self):
        h, w = c_int(), c_int()
        check(self.lib.st_get_content_nchw(self._ctx, None, byref(h), byref(w)))
        return h.value, w.value

    def get_content_nchw(self):
        h, w = self.content_shape()
        out = np.empty((1, 3, h, w), F32)
        check(self.lib.st_get_content_nchw(self._ctx, _ptr(out), None, None))
        return out

    def step(self, want_image=True, want_trace=True):
        """One iteration.  With both flags False nothing is read back and the call is asynchronous."""
        h, w = self.input_shape()
        img = np.empty((h, w, 3), F32) if want_image else None
        trace = np.zeros(self.trace_len(), np.float64) if want_trace else None
        loss = c_float()
        check(self.lib.st_step(self._ctx, _ptr(img), _ptr(trace),
                               byref(loss) if (want_image or want_trace) else None))
        return img, trace, F32(loss.value)

    def step_begin(self):
        """Queue one iteration and the copy of its iterate / trace to the host (st_step_begin); at most two may be in flight."""
        check(self.lib.st_step_begin(self._ctx))

    STEP_VIEW_LIFETIME = 5      # st2.h: a view returned by step_end(copy=False) survives this many further step_begin calls

    def set_frame_room(self, head_bytes, tail_bytes):
        """Reserve room in front of / behind the iterates step_end hands out (st_step_frame_room), from the next step_begin on."""
        check(self.lib.st_step_frame_room(self._ctx, int(head_bytes), int(tail_bytes)))
        self._frame_room = ((int(head_bytes) + 4095) // 4096 * 4096, int(tail_bytes))

    def step_end(self, copy=True, room=False):
        """Results of the OLDEST queued iteration, as step() returns them.  copy=False returns a read-only view of the context's
        pinned buffer instead of an owned array: valid for the next STEP_VIEW_LIFETIME calls of step_begin (the worker's bounded
        sender queue stays inside that; a 12.6 MB host copy per iterate is what it saves).  room=True (with copy=False, after
        set_frame_room): a fourth result, the writable buffer [head room | image | tail room] the view lies in (iterate_frame.py)."""
        ptr, h, w, loss = c_void_p(), c_int(), c_int(), c_float()
        trace = np.zeros(self.trace_len(), np.float64)
        check(self.lib.st_step_end(self._ctx, byref(ptr), byref(h), byref(w), _ptr(trace), byref(loss)))
        view = np.ctypeslib.as_array(ctypes.cast(ptr, POINTER(c_float)), shape=(h.value, w.value, 3))
        if copy:
            return view.copy(), trace, F32(loss.value)
        view.flags.writeable = False
        if room:
            head, tail = getattr(self, '_frame_room', (0, 0))
            buf = (ctypes.c_char * (head + view.nbytes + tail)).from_address(ptr.value - head)
            return view, trace, F32(loss.value), buf
        return view, trace, F32(loss.value)

    def set_iterate_average(self, decay):
        """0 (default): step() / step_end() hand out the raw iterate.  0 < decay < 1: they hand out the bias-corrected exponentially
        weighted mean of the iterates (utils.DecayingMean over x after every optimizer step); the mean starts empty.  The trajectory,
        the trace and get_input_nchw() are unchanged.  Refused while a pipelined iteration is in flight."""
        check(self.lib.st_set_iterate_average(self._ctx, float(decay)))

    def iterate_average(self, want_mean=True):
        """(decay, items, mean): the decay in force (0.0: off), the number of iterates averaged, and the raw, uncorrected mean as a
        (1, 3, H, W) array -- None while it is empty, or when want_mean is False."""
        decay, items = c_double(), c_int()
        check(self.lib.st_get_iterate_average(self._ctx, byref(decay), byref(items), None))
        if not items.value or not want_mean:
            return decay.value, items.value, None
        h, w = self.input_shape()
        mean = np.empty((1, 3, h, w), F32)
        check(self.lib.st_get_iterate_average(self._ctx, None, None, _ptr(mean)))
        return decay.value, items.value, mean

    # -- the content's colours (st2.h: luminance-only output, colour-matched style) ----------------------------------
    def set_original_colors(self, on):
        """True: step() / step_end() (tile-sharded: the tile readers) hand out the luminance of the iterate with the chroma of the content
        image; the optimisation, get_input_nchw() and the running mean are untouched.  Refused while a pipelined iteration is in flight;
        while on, a step that wants an image is refused without a content image of the input's size."""
        check(self.lib.st_set_original_colors(self._ctx, 1 if on else 0))

    def image_moments(self, image):
        """(mean (3,), cov (3, 3)) of an HxWx3 image in float64: the colour mean in image scale and the population covariance, from sums
        taken on the device in double in a fixed order (st_image_moments)."""
        arr, u8 = _image_arg(image)
        mean, cov = (c_double * 3)(), (c_double * 6)()
        check(self.lib.st_image_moments(self._ctx, _ptr(arr), arr.shape[0], arr.shape[1], u8, mean, cov))
        return np.array(mean[:], np.float64), cov_full(cov[:])

    def set_style_transform(self, A, b):
        """The affine colour map s' = A s + b (preprocessed coordinates) every later set_style / tile_set_style / tile_style_partials applies
        to the style image; A = b = None turns it off."""
        if A is None and b is None:
            check(self.lib.st_set_style_transform(self._ctx, None, None))
            return
        A, b = np.ascontiguousarray(A, F32).reshape(9), np.ascontiguousarray(b, F32).reshape(3)
        check(self.lib.st_set_style_transform(self._ctx, A.ctypes.data_as(POINTER(c_float)), b.ctypes.data_as(POINTER(c_float))))

    def set_style_color_match(self, on):
        """True: set_style gives the style image the content image's colour mean and covariance first (linear colour transfer, derived from
        the two images' moments when the style is set).  Refused on a tile-sharded context: set_style_transform there."""
        check(self.lib.st_set_style_color_match(self._ctx, 1 if on else 0))

    def color_modes(self):
        """(original_colors, style_match, A (3, 3), b (3,)): style_match 0 off, 1 colour matching, 2 a given transform; A, b the transform
        last applied (or given and waiting), the identity before either."""
        oc, sm = c_int(), c_int()
        A, b = np.empty(9, F32), np.empty(3, F32)
        check(self.lib.st_get_color_modes(self._ctx, byref(oc), byref(sm), A.ctypes.data_as(POINTER(c_float)), b.ctypes.data_as(POINTER(c_float))))
        return bool(oc.value), sm.value, A.reshape(3, 3), b

    # -- the Laplacian-steered content term (st2.h: st_set_laplacian) ---------------------------------------------------
    def set_laplacian(self, levels):
        """levels: a sequence of (pool, weight) pairs -- at most three, pool sizes distinct and from {1, 2, 4, 8, 16, 32}, weights finite
        and non-zero; empty or None turns the term off (the default).  While on, every evaluation adds sum over levels of
        w * sum (D(P(x / 255)) - D(P(content / 255))) ** 2 to the loss and its gradient to the image gradient, and the trace has two more
        scalars.  Refused while a pipelined iteration is in flight and on a tile-configured context."""
        levels = [tuple(lv) for lv in (levels or ())]
        if any(len(lv) != 2 for lv in levels):
            raise ValueError('a Laplacian level is a (pool, weight) pair')
        n = len(levels)
        pool = (c_int * max(n, 1))(*[int(p) for p, _ in levels])
        weight = (c_double * max(n, 1))(*[float(w) for _, w in levels])
        check(self.lib.st_set_laplacian(self._ctx, n, pool, weight))

    def laplacian(self):
        """The levels in force as a list of (pool, weight) pairs; empty: the term is off."""
        n, pool, weight = c_int(), (c_int * 3)(), (c_double * 3)()
        check(self.lib.st_get_laplacian(self._ctx, byref(n), pool, weight))
        return [(int(pool[i]), float(weight[i])) for i in range(n.value)]

    def laplacian_terms(self, level, want_grad=True):
        """Test hook: (T, E, g_lap) of the last evaluation -- the target and the difference of `level` (an index into laplacian()), each
        (3, hp, wp), and the summed gradient term (1, 3, H, W), None when want_grad is False."""
        levels = self.laplacian()
        h, w = self.input_shape()
        if not 0 <= level < max(len(levels), 1):
            raise ValueError('level %d of %d' % (level, len(levels)))
        p = levels[level][0] if levels else 1
        hp, wp = -(-h // p), -(-w // p)
        target, diff = np.empty((3, hp, wp), F32), np.empty((3, hp, wp), F32)
        grad = np.empty((1, 3, h, w), F32) if want_grad else None
        check(self.lib.st_get_laplacian_terms(self._ctx, level, _ptr(target), _ptr(diff), _ptr(grad)))
        return target, diff, grad

    # -- the anchor term (st2.h: st_set_anchor) ------------------------------------------------------------------------------
    def set_anchor(self, image, mask=None, weight=1.0):
        """A per-pixel weighted pull toward `image`: every evaluation adds weight * sum mask * (x / 255 - anchor / 255) ** 2 to the loss
        and its gradient to the image gradient, and the trace has two more scalars (a_loss, a_grad).  image: HxWx3 (uint8 or float,
        preprocessed on the device like a content image), or already preprocessed planes of shape (3, H, W) or (1, 3, H, W); None turns
        the term off (the default).  mask: an optional (H, W) map of finite values >= 0 shared by the channels -- float as it is, uint8
        divided by 255, bool as 0 / 1.  The anchor does not follow the input: after a resize every evaluation is refused until an
        anchor of the new size is set or the term is turned off.  Refused while a pipelined iteration is in flight and on a
        tile-configured context."""
        if image is None:
            check(self.lib.st_set_anchor(self._ctx, None, 0, 0, 0, None, 1.0))
            return
        arr = np.asarray(image)
        if arr.ndim == 4:
            if arr.shape[:2] != (1, 3):
                raise ValueError('planar anchor must be (3, H, W) or (1, 3, H, W), got %s' % (arr.shape,))
            arr = arr[0]
        planar = arr.ndim == 3 and arr.shape[0] == 3 and (np.ndim(image) == 4 or arr.shape[2] != 3)
        if planar:
            arr = np.ascontiguousarray(arr, F32)
            h, w = arr.shape[1:]
        else:
            arr, u8 = _image_arg(arr)
            h, w = arr.shape[:2]
        mask = _map_arg(mask, h, w)
        if planar:
            check(self.lib.st_set_anchor_nchw(self._ctx, _ptr(arr), h, w, _ptr(mask), float(weight)))
        else:
            check(self.lib.st_set_anchor(self._ctx, _ptr(arr), h, w, u8, _ptr(mask), float(weight)))

    def anchor(self):
        """The term in force: None while it is off, else a dict with 'size' (H, W), 'has_mask' and 'weight'."""
        on, h, w, has_mask, weight = c_int(), c_int(), c_int(), c_int(), c_double()
        check(self.lib.st_get_anchor(self._ctx, byref(on), byref(h), byref(w), byref(has_mask), byref(weight)))
        if not on.value:
            return None
        return {'size': (h.value, w.value), 'has_mask': bool(has_mask.value), 'weight': weight.value}

    def anchor_terms(self, want_extra=True):
        """Test hook: (anchor, mask, extra) of the last evaluation -- the preprocessed anchor (1, 3, H, W), the map (H, W) or None
        without one, and the plane the image pass added after the p-norm term (1, 3, H, W): g_lap + g_anc with the Laplacian term
        on, else g_anc; None when want_extra is False."""
        info = self.anchor()
        h, w = info['size'] if info else (1, 1)
        ax = np.empty((1, 3, h, w), F32)
        mask = np.empty((h, w), F32) if info and info['has_mask'] else None
        extra = np.empty((1, 3, h, w), F32) if want_extra else None
        check(self.lib.st_get_anchor_terms(self._ctx, _ptr(ax), _ptr(mask), _ptr(extra)))
        return ax, mask, extra

    # -- the photorealism term (st2.h: st_set_matting) ------------------------------------------------------------------------------
    def set_matting(self, weight, eps=1e-7):
        """The matting-Laplacian regulariser of Luan et al.: every evaluation adds weight * sum_c u_c' L u_c (u = x / 255, L the matting
        Laplacian of the content image with regularisation eps in [1e-9, 1]) to the loss and its gradient to the image gradient, and the
        trace has two more scalars (m_loss, m_grad).  The term is zero where the result is locally an affine function of the content's
        colours.  weight 0, None or False turns it off (the default).  It follows the content image; evaluations are refused without
        one of the input's size and under 3 x 3.  Refused while a pipelined iteration is in flight and on a tile-configured context."""
        check(self.lib.st_set_matting(self._ctx, float(weight or 0.0), float(eps)))

    def matting(self):
        """The term in force: None while it is off, else a dict with 'weight' and 'eps'."""
        on, weight, eps = c_int(), c_double(), c_double()
        check(self.lib.st_get_matting(self._ctx, byref(on), byref(weight), byref(eps)))
        if not on.value:
            return None
        return {'weight': weight.value, 'eps': eps.value}

    def matting_terms(self, want_extra=True):
        """Test hook: (mu, M, a_pb, extra) of the last evaluation -- the window means (3, H - 2, W - 2), the inverse covariances
        (6, H - 2, W - 2) in the order 00 01 02 11 12 22, the fits (3, 4, H - 2, W - 2) (a0 a1 a2 pb per channel of the iterate) and the
        plane the image pass added after the p-norm term (1, 3, H, W); None for it when want_extra is False."""
        h, w = self.input_shape()
        hw, ww = max(h - 2, 1), max(w - 2, 1)
        mu, m, ab = np.empty((3, hw, ww), F32), np.empty((6, hw, ww), F32), np.empty((3, 4, hw, ww), F32)
        extra = np.empty((1, 3, h, w), F32) if want_extra else None
        check(self.lib.st_get_matting_terms(self._ctx, _ptr(mu), _ptr(m), _ptr(ab), _ptr(extra)))
        return mu, m, ab, extra

    def trace_terms(self):
        """Which optional image-space terms are on, as the trace orders them: (laplacian, anchor, matting)."""
        lap, anchor, mat = c_int(), c_int(), c_int()
        check(self.lib.st_get_trace_terms(self._ctx, byref(lap), byref(anchor), byref(mat)))
        return bool(lap.value), bool(anchor.value), bool(mat.value)

    # -- jitter (st2.h: st_set_jitter) ------------------------------------------------------------------------------------------------
    def set_jitter(self, radius, seed=0):
        """Evaluate the network terms on the iterate rolled by a random shift of up to `radius` pixels per axis (1 .. 4096), one shift per
        optimizer step drawn from splitmix64 of `seed`; the gradient is rolled back, the iterate itself never moves.  0 or None turns
        the mode off (the default).  Refused while a pipelined iteration is in flight and on a tile-configured context."""
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError('the jitter seed must fit 64 unsigned bits, got %d' % seed)
        check(self.lib.st_set_jitter(self._ctx, int(radius or 0), seed))

    def set_jitter_shift(self, dy, dx):
        """The mode on with the shift (dy, dx) -- any integers -- held for every evaluation; the step counter still counts."""
        check(self.lib.st_set_jitter_shift(self._ctx, int(dy), int(dx)))

    def jitter(self):
        """The mode in force: None while it is off, else a dict with 'radius', 'seed', 'k' (optimizer steps begun since it was set),
        'pinned' and 'shift', the (dy, dx) the next evaluation will use."""
        radius, seed, k, pinned, dy, dx = c_int(), c_ulonglong(), c_longlong(), c_int(), c_int(), c_int()
        check(self.lib.st_get_jitter(self._ctx, byref(radius), byref(seed), byref(k), byref(pinned), byref(dy), byref(dx)))
        if not radius.value and not pinned.value:
            return None
        return {'radius': radius.value, 'seed': seed.value, 'k': k.value, 'pinned': bool(pinned.value), 'shift': (dy.value, dx.value)}

    def jitter_terms(self, want_scd=True):
        """Test hook: (xs, scd, (dy, dx)) of the last evaluation -- the planes its forward read (1, 3, H, W), the un-rolled network
        gradient it handed to the image pass (None when want_scd is False), and the shift it used."""
        h, w = self.input_shape()
        xs = np.empty((1, 3, max(h, 1), max(w, 1)), F32)
        scd = np.empty_like(xs) if want_scd else None
        dy, dx = c_int(), c_int()
        check(self.lib.st_get_jitter_terms(self._ctx, _ptr(xs), _ptr(scd), byref(dy), byref(dx)))
        return xs, scd, (dy.value, dx.value)

    # -- optical flow (st2.h: st_flow_estimate .. st_get_flow_level) ----------------------------------------------------------------
    def flow_estimate(self, from_image, to_image, **params):
        """The dense optical flow (H, W, 2) float32 of (dx, dy) with from_image(p) ~ to_image(p + flow(p)), estimated on the device
        (st2.h: coarse-to-fine Horn-Schunck; tests/flow_oracle.py restates it bit for bit).  The images are HxWx3 of one size, uint8
        or float on the 0 .. 255 scale.  params: alpha, warps, iters, levels, route (flow.check_flow; the defaults of flow.DEFAULTS).
        With from = frame t and to = frame t - 1 this is flows[t] of jobs.run_frames; the other way round, forward_flows[t].  Nothing
        of the job's state is read or written."""
        par = flow_mod.check_flow(**params)
        a, a_u8 = _image_arg(from_image)
        b, b_u8 = _image_arg(to_image)
        if a.shape != b.shape:
            raise ValueError('the two images differ in size: %s and %s' % (a.shape[:2], b.shape[:2]))
        if a_u8 != b_u8:                                   # one upload format for both
            a, b, a_u8 = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32), 0
        h, w = a.shape[:2]
        out = np.empty((h, w, 2), F32)
        cpar = capi.FlowParams(par['levels'], par['warps'], par['iters'], par['alpha'], par['route'])
        check(self.lib.st_flow_estimate(self._ctx, _ptr(a), _ptr(b), h, w, a_u8, byref(cpar), _ptr(out)))
        return out

    def flow_release(self):
        """Free the scratch buffer the estimates keep on the device (the next estimate makes it again)."""
        check(self.lib.st_flow_release(self._ctx))

    def flow_level(self, level):
        """Test hook: (from_l, to_l, flow_l) of one level of the last estimate: the smoothed luma planes (h, w) and the level's
        finished flow (h, w, 2)."""
        h, w = c_int(), c_int()
        check(self.lib.st_get_flow_level(self._ctx, int(level), byref(h), byref(w), None, None, None))
        a, b, f = np.empty((h.value, w.value), F32), np.empty((h.value, w.value), F32), np.empty((h.value, w.value, 2), F32)
        check(self.lib.st_get_flow_level(self._ctx, int(level), byref(h), byref(w), _ptr(a), _ptr(b), _ptr(f)))
        return a, b, f

    # -- frame sequences (st2.h: st_frames_keep .. st_anchor_from_frame) ------------------------------------------------------------
    def frames_keep(self, depth):
        """Keep up to `depth` (0 .. 8) earlier iterates on the device; a smaller depth drops the oldest beyond it, 0 frees them."""
        check(self.lib.st_frames_keep(self._ctx, int(depth)))

    def frame_push(self):
        """The current raw iterate (get_input_nchw: never the averaged or recoloured image) becomes frame 1, frames 1.. become 2..,
        the oldest beyond the depth is dropped.  A push at another size than the kept frames' drops those first."""
        check(self.lib.st_frame_push(self._ctx))

    def frames(self):
        """A dict with 'depth', 'count' (frames held) and 'size' (H, W) of the kept frames, (0, 0) while none is held."""
        depth, count, h, w = c_int(), c_int(), c_int(), c_int()
        check(self.lib.st_get_frames(self._ctx, byref(depth), byref(count), byref(h), byref(w)))
        return {'depth': depth.value, 'count': count.value, 'size': (h.value, w.value)}

    def set_input_from_frame(self, j, flow=None):
        """The iterate becomes kept frame j, warped on the device by `flow` ((H, W, 2) of (dx, dy), from the frame being stylised back to
        frame j; the arithmetic of jobs.warp_planar, bit for bit); None: a copy.  The rest of the state as after set_input_nchw."""
        h, w = self.input_shape()
        check(self.lib.st_set_input_from_frame(self._ctx, int(j), _ptr(_flow_arg(flow, h, w))))

    def anchor_from_frame(self, j, flow=None, forward_flow=None, mask=None, weight=1.0, accumulate=False):
        """The anchor term from kept frame j, in one launch on the device: the anchor is the frame warped by `flow` (None: as it is); with
        forward_flow (from frame j to the frame being stylised) the map is the flow's reliability (st2.h: 0 where the sample leaves the
        image, at disocclusions and at motion boundaries, else 1), times `mask` where one is given (set_anchor's conversions); without
        either there is no map.  accumulate=True composes into the anchor that is there (it needs one with a map, of the same weight):
        pixels its map leaves free take this frame's sample and reliability -- the long-term term, called for j = 1, 2, 4, .. in turn."""
        h, w = self.input_shape()
        check(self.lib.st_anchor_from_frame(self._ctx, int(j), _ptr(_flow_arg(flow, h, w)), _ptr(_flow_arg(forward_flow, h, w, 'forward flow')),
                                            _ptr(_map_arg(mask, h, w)), float(weight), 1 if accumulate else 0))

    def set_style_nchw(self, x):
        """set_style for an already-preprocessed (1, 3, H, W) image; no colour transform is applied."""
        x = np.ascontiguousarray(x, F32)
        check(self.lib.st_set_style_nchw(self._ctx, _ptr(x), x.shape[2], x.shape[3]))

    def style_recolor(self, image):
        """Test hook: the preprocessed, recoloured (1, 3, H, W) image exactly as set_style would forward it under the modes in force."""
        arr, u8 = _image_arg(image)
        out = np.empty((1, 3, arr.shape[0], arr.shape[1]), F32)
        check(self.lib.st_style_recolor(self._ctx, _ptr(arr), arr.shape[0], arr.shape[1], u8, _ptr(out)))
        return out

    def steps_pending(self):
        return int(self.lib.st_step_pending(self._ctx))

    def lbfgs_inv_hv(self, pairs, g):
        """Test hook: H g of optimizers.py:89-108 for the given [(s, y), ...] history (oldest first) on the device."""
        g = np.ascontiguousarray(g, F32)
        ss = [np.ascontiguousarray(s, F32) for s, _ in pairs]
        ys = [np.ascontiguousarray(y, F32) for _, y in pairs]
        sp = (c_void_p * len(pairs))(*[a.ctypes.data for a in ss])
        yp = (c_void_p * len(pairs))(*[a.ctypes.data for a in ys])
        out = np.empty_like(g)
        check(self.lib.st_lbfgs_inv_hv(self._ctx, len(pairs), sp, yp, _ptr(g), _ptr(out)))
        return out

    def sync(self):
        check(self.lib.st_sync(self._ctx))

    # -- measurement -----------------------------------------------------------------------------------
    def profile_enable(self, on=True):
        check(self.lib.st_profile_enable(self._ctx, 1 if on else 0))

    def profile_read(self):
        n = self.lib.st_profile_num_classes()
        launches = (c_longlong * n)()
        ms, flops, nbytes = (c_double * n)(), (c_double * n)(), (c_double * n)()
        check(self.lib.st_profile_read(self._ctx, launches, ms, flops, nbytes))
        out = {}
        for i in range(n):
            if launches[i]:
                out[self.lib.st_profile_class_name(i).decode()] = dict(
                    launches=int(launches[i]), ms=float(ms[i]), flops=float(flops[i]), bytes=float(nbytes[i]))
        return out
