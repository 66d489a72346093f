"""HIP tile backend of the tile-sharded mode: one ``Engine`` per rank holding that rank's window in HBM;
the phases of tiled.TiledTransfer map 1:1 onto the ``st_tile_*`` entry points of the C ABI.  Device buffers
are handed to torch (for RCCL) as zero-copy views through ``__cuda_array_interface__``."""

import ctypes
from ctypes import byref, c_int, c_void_p

import numpy as np

from . import capi
from .capi import check
from .engine import Engine, OPT_ADAM, OPT_LBFGS, color_transform
from .tiled import crop, local_rect, torch          # (torch: tiled's lazy import -- nothing here loads it at import time)
from .transfer import weight_table, LOSS_NAMES, SCALAR_LOSS_NAMES

F32 = np.float32


class _DevArray:
    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {'shape': tuple(shape), 'typestr': '<f4', 'data': (int(ptr), False),
                                         'version': 2, 'strides': None}


def dev_tensor(ptr, shape, device):
    import torch
    return torch.as_tensor(_DevArray(ptr, shape), device=device)


class HipTileBackend:
    def __init__(self, net_params, grid, rank, content, style, init, weights, params, step_size=10,
                 topology=None, device=0, precision='fp32', use_torch=True, optimizer='adam', iterate_average=None,
                 original_colors=None, style_transform=None):
        # torch bundles its own copy of the HIP runtime; when both live in one process torch's must come up FIRST.
        # The phase-by-phase driver and the host-staged test transport need torch; the in-engine iteration over RCCL
        # (comm_init_rccl + tiled.FusedTiledTransfer) does not: pass use_torch=False and the process never loads it.
        if use_torch:
            import torch as _torch
            if _torch.cuda.is_available():
                _torch.cuda.init()
        # precision='bf16': the convs of the window run on the bf16 matrix cores (fp32 accumulation) with the lean data flow (fp32 blobs /
        # diffs only where something reads fp32); the Gram / style / loss kernels of the tile phases stay fp32 on the fp32 blobs of the
        # weighted layers (the region-of-interest forms exist for those only).  'bf16-full' writes every fp32 tensor: same results.
        self.engine = Engine(topology, device, precision)
        self.engine.load_weights(net_params)
        self.lib, self.ctx = self.engine.lib, self.engine._ctx
        self.device_index = device
        self.grid, self.rank = grid, rank
        w, t = grid.windows[rank], grid.tiles[rank]
        # the content's colours.  original_colors: the tile readers hand out the chroma of this window's own content (per pixel, so the
        # stitched image is the whole-image job's).  style_transform: (A, b) for Engine.set_style_transform, in force before the style is
        # set here or by shard_style -- or (content image, style image), WHOLE images, to derive it from through this engine (colour
        # matching itself is refused on a tile-sharded context: a window's content is not the image's)
        if original_colors is not None:
            self.engine.set_original_colors(original_colors)
        self.style_transform = None
        if style_transform is not None:
            first, second = style_transform
            if np.ndim(first) == 3:
                mean_c, cov_c = self.engine.image_moments(first)
                mean_s, cov_s = self.engine.image_moments(second)
                first, second = color_transform(mean_c, cov_c, mean_s, cov_s)
            self.style_transform = (first, second)
            self.engine.set_style_transform(first, second)
        self.engine.set_input(crop(init, w))
        self.engine.set_content(crop(content, w))
        if style is not None:            # None: the targets come from the sharded style pass (shard_style, after comm_init_*)
            self.engine.set_style(style)
        rows, cells = weight_table(weights)
        cols = [[cells[k][r] for r in rows] for k in LOSS_NAMES]
        self.engine.set_weights(rows, cols[0], cols[1], cols[2], [params[k] for k in SCALAR_LOSS_NAMES])
        # optimizer: what the fused iteration (st_tile_step) runs -- Adam, or L-BFGS in its Gram form with one all-reduce of the new inner
        # products per step; the phase-by-phase driver (tiled.TiledTransfer) brings its own L-BFGS and only uses Adam's fused update
        if optimizer not in ('adam', 'lbfgs'):
            raise ValueError('optimizer must be adam or lbfgs')
        self.engine.optimizer_reset(OPT_LBFGS if optimizer == 'lbfgs' else OPT_ADAM, step_size)
        self.engine.clear_norms()
        # iterate averaging (Engine.set_iterate_average): st_tile_step keeps the running mean of the window; averaged_image() reads the tile
        if iterate_average:
            self.engine.set_iterate_average(iterate_average)
        check(self.lib.st_tile_configure(self.ctx, grid.gH, grid.gW, w.y0, w.x0, t.y0, t.x0, t.y1, t.x1))
        self.wh, self.ww = w.y1 - w.y0, w.x1 - w.x0

    @property
    def device(self):
        return torch.device('cuda', self.device_index)

    def _sync(self):
        self.engine.sync()

    # ---- the iteration with its communication inside the engine (st_tile_step; engine_comm.cpp) -------------------------------
    def comm_init_rccl(self, unique_id, rank, world):
        """One RCCL communicator for this context (unique_id: the 128 bytes of st_comm_unique_id from rank 0)."""
        check(self.lib.st_comm_init(self.ctx, bytes(unique_id), int(rank), int(world)))

    def comm_init_host(self, rank, world, allreduce, exchange):
        """Host-staged transport in place of RCCL (tests: several ranks share one GPU).  `allreduce(values)` sums a float32 numpy
        array over the ranks in place; `exchange(sends, recvs)` delivers sends = [(peer, float32 array)] and fills
        recvs = [(peer, float32 array to fill)].  The engine calls them from st_tile_step with its stream drained."""
        device = self.device

        def on_allreduce(ptr, n):
            t = dev_tensor(ptr, (n,), device)
            h = t.cpu().numpy()
            allreduce(h)
            t.copy_(torch.from_numpy(h))
            torch.cuda.synchronize(device)

        def on_exchange(ns, speer, sbuf, scount, nr, rpeer, rbuf, rcount):
            sends = [(int(speer[i]), dev_tensor(sbuf[i], (scount[i],), device).cpu().numpy()) for i in range(ns)]
            recvs = [(int(rpeer[j]), np.empty(rcount[j], F32)) for j in range(nr)]
            exchange(sends, recvs)
            for j, (_, h) in enumerate(recvs):
                dev_tensor(rbuf[j], (rcount[j],), device).copy_(torch.from_numpy(h))
            torch.cuda.synchronize(device)
        self._install_callbacks(rank, world, on_allreduce, on_exchange)

    def comm_init_local(self, rank, world, fabric):
        """Ranks that are threads of this process on this GPU (tiled.InProcessFabric): the engine's all-reduces and strip exchanges
        become device-to-device copies between the contexts' buffers -- no host staging."""
        device = self.device

        def on_allreduce(ptr, n):
            fabric.allreduce(rank, dev_tensor(ptr, (n,), device))
            torch.cuda.synchronize(device)

        def on_exchange(ns, speer, sbuf, scount, nr, rpeer, rbuf, rcount):
            sends = [(int(speer[i]), dev_tensor(sbuf[i], (scount[i],), device)) for i in range(ns)]
            recvs = [(int(rpeer[j]), dev_tensor(rbuf[j], (rcount[j],), device)) for j in range(nr)]
            fabric.exchange(rank, sends, recvs)
        self._install_callbacks(rank, world, on_allreduce, on_exchange)

    def _install_callbacks(self, rank, world, on_allreduce, on_exchange):
        """The transport st_tile_step calls with its stream drained: on_allreduce(ptr, n) sums n floats at the device pointer over the
        ranks in place; on_exchange(n_send, peers, buffers, counts, n_recv, peers, buffers, counts) delivers the packed strips.  An
        exception in either is printed and reported to the engine through the status code."""
        def guarded(body):
            def thunk(_user, *args):
                try:
                    body(*args)
                    return 0
                except Exception:           # noqa: BLE001 (reported through the status code)
                    import traceback
                    traceback.print_exc()
                    return 1
            return thunk
        self._callbacks = (capi.ALLREDUCE_FN(guarded(on_allreduce)), capi.EXCHANGE_FN(guarded(on_exchange)))     # keep the thunks alive
        check(self.lib.st_comm_callbacks(self.ctx, int(rank), int(world), self._callbacks[0], self._callbacks[1], None))

    def comm_init_callbacks(self, dist, rank, world):
        """comm_init_host over a torch.distributed (gloo) group: one process per rank."""
        def allreduce(values):
            t = torch.from_numpy(values)
            dist.all_reduce(t)

        def exchange(sends, recvs):
            ops = [dist.P2POp(dist.isend, torch.from_numpy(h), peer) for peer, h in sends]
            ops += [dist.P2POp(dist.irecv, torch.from_numpy(h), peer) for peer, h in recvs]
            if ops:
                for req in dist.batch_isend_irecv(ops):
                    req.wait()
        self.comm_init_host(rank, world, allreduce, exchange)

    def comm_init_solo(self, rank, world):
        """ONE rank of a larger grid alone on a GPU (timing the per-rank compute of a multi-GPU run): the all-reduces see one rank,
        what the neighbours would send never arrives -- the receive buffers hold the zeros st_tile_plan initialised them with, so the
        timed update runs on finite data."""
        self._install_callbacks(rank, world, lambda ptr, n: None, lambda *a: None)

    # ---- the style targets from the sharded style image (st_tile_set_style; tiling.style_grid) ---------------------------------
    def _style_share(self, style, style_grid):
        """(this rank's window of the style image or None, window origin, tile) for the C ABI."""
        style = np.asarray(style)
        if style.shape[:2] != (style_grid.gH, style_grid.gW):
            raise ValueError('the style grid is cut for %d x %d, the image is %d x %d' % ((style_grid.gH, style_grid.gW) + style.shape[:2]))
        if self.rank >= style_grid.world:
            return None, (0, 0), None
        w, t = style_grid.windows[self.rank], style_grid.tiles[self.rank]
        return np.ascontiguousarray(style[w.y0:w.y1, w.x0:w.x1]), (w.y0, w.x0), (t.y0, t.x0, t.y1, t.x1)

    def shard_style(self, style, style_grid):
        """Collective (every rank calls it, after comm_init_*): the style targets of blobs 0 .. style_grid.last_blob from the ranks'
        tiles of the style image; a rank beyond the style grid contributes nothing but takes part in the all-reduce."""
        image, origin, tile = self._style_share(style, style_grid)
        self.engine.tile_set_style(image, (style_grid.gH, style_grid.gW), origin, tile, style_grid.last_blob)

    def style_partials(self, style, style_grid):
        """The same in two halves for the phase-by-phase driver (tiled.TiledTransfer.shard_style): this rank's raw Gram sums as a 1-D
        device tensor, to be all-reduced; then style_commit()."""
        image, origin, tile = self._style_share(style, style_grid)
        torch.cuda.synchronize(self.device)
        ptr, n = self.engine.tile_style_partials(image, (style_grid.gH, style_grid.gW), origin, tile, style_grid.last_blob)
        return dev_tensor(ptr, (n,), self.device)

    def style_commit(self):
        torch.cuda.synchronize(self.device)
        self.engine.tile_style_commit()

    def set_plan(self, phase, peers):
        """peers: {peer rank: (send rects, recv rects)}, rects = [(y0, x0, h, w), ...] (tiled.fused_plans)."""
        keep = []
        arr = (capi.TilePeer * max(len(peers), 1))()
        for k, peer in enumerate(sorted(peers)):
            send, recv = peers[peer]
            sa = (c_int * max(4 * len(send), 1))(*[int(v) for r in send for v in r])
            ra = (c_int * max(4 * len(recv), 1))(*[int(v) for r in recv for v in r])
            keep += [sa, ra]
            arr[k].peer, arr[k].n_send, arr[k].n_recv = int(peer), len(send), len(recv)
            arr[k].send_rects = ctypes.cast(sa, ctypes.POINTER(c_int))
            arr[k].recv_rects = ctypes.cast(ra, ctypes.POINTER(c_int))
        check(self.lib.st_tile_plan(self.ctx, int(phase), len(peers), arr))

    def step_fused(self):
        """One iteration (Adam or L-BFGS, as the backend was built), every phase and collective enqueued by the engine; returns the
        trace values."""
        trace = np.zeros(self.engine.trace_len(), np.float64)
        check(self.lib.st_tile_step(self.ctx, trace.ctypes.data_as(c_void_p)))
        return trace

    def step_fused_async(self):
        """The same iteration without its trace: nothing is read back, so the call returns as soon as the launches and collectives
        are enqueued (over RCCL the host then runs ahead of the GPU, as Engine.step(want_trace=False) does on one GPU); the
        reduced sums stay on the device."""
        check(self.lib.st_tile_step(self.ctx, None))

    def barrier(self):
        check(self.lib.st_comm_barrier(self.ctx))

    def _tile_rect(self):
        """[(y0, x0, h, w)] of this rank's tile in its window: a rectangle list for strips()."""
        return [local_rect(self.grid.tiles[self.rank], self.grid.windows[self.rank])]

    def _read_tile(self, entry):
        _, _, th, tw = self._tile_rect()[0]
        out = np.empty((th, tw, 3), F32)
        check(entry(self.ctx, out.ctypes.data_as(c_void_p)))
        return out

    def tile_image(self):
        return self._read_tile(self.lib.st_tile_get_tile)

    def averaging(self):
        """True once the engine holds a running mean of this window's iterates (the mode is on and a fused step has run)."""
        decay, items, _ = self.engine.iterate_average(want_mean=False)
        return bool(decay and items)

    def averaged_image(self):
        """This rank's tile of the corrected, deprocessed iterate average (st_tile_get_tile_average): an error while the mode is off or
        no fused step has run since the mean was cleared."""
        return self._read_tile(self.lib.st_tile_get_tile_average)

    def _buf(self, which, shape):
        p = c_void_p()
        check(self.lib.st_tile_buffer(self.ctx, which, byref(p)))
        return dev_tensor(p.value, shape, self.device)

    def x_cur(self):
        return self._buf(0, (3, self.wh, self.ww))

    def x_next(self):
        return self._buf(1, (3, self.wh, self.ww))

    def swap(self):
        torch.cuda.synchronize(self.device)
        check(self.lib.st_tile_swap(self.ctx))

    def strips(self, tensor, rects, buf, mode):
        """One kernel per neighbour and phase: pack (mode 0) the rects [(y0, x0, h, w)] of the (3, wh, ww) device tensor into
        the 1-D device buffer `buf`, or unpack them from it (1 assign, 2 add)."""
        torch.cuda.synchronize(self.device)
        flat = (c_int * (4 * len(rects)))(*[int(v) for r in rects for v in r])
        check(self.lib.st_tile_strips(self.ctx, c_void_p(tensor.data_ptr()), tensor.shape[0], tensor.shape[1], tensor.shape[2],
                                      len(rects), flat, c_void_p(buf.data_ptr()), mode))

    # ---- phases -------------------------------------------------------------------------------------------
    def forward_partials(self):
        torch.cuda.synchronize(self.device)
        p, n = c_void_p(), c_int()
        check(self.lib.st_tile_forward(self.ctx, byref(p), byref(n)))
        self._sync()
        self.p1 = dev_tensor(p.value, (n.value,), self.device) if n.value else None
        return self.p1

    def losses_need_style_norm(self):
        torch.cuda.synchronize(self.device)
        p, n = c_void_p(), c_int()
        check(self.lib.st_tile_losses(self.ctx, byref(p), byref(n)))
        self.p2 = None
        if n.value:
            check(self.lib.st_tile_style_raw(self.ctx))
            self._sync()
            self.p2 = dev_tensor(p.value, (n.value,), self.device)
        return self.p2

    def finish_losses(self):
        torch.cuda.synchronize(self.device)
        check(self.lib.st_tile_losses_finish(self.ctx))
        self._sync()

    def backward(self):
        p = c_void_p()
        check(self.lib.st_tile_backward(self.ctx, byref(p)))
        return dev_tensor(p.value, (3, self.wh, self.ww), self.device)

    def _image_pass(self, entry, ring):
        ring = ring.contiguous()
        torch.cuda.synchronize(self.device)
        self._ring = ring                                    # keep alive until the kernel has run
        p, n = c_void_p(), c_int()
        check(entry(self.ctx, c_void_p(ring.data_ptr()), byref(p), byref(n)))
        self.p3 = dev_tensor(p.value, (n.value,), self.device)
        return self.p3

    def update(self, ring):
        return self._image_pass(self.lib.st_tile_update, ring)

    def gradient(self, ring):
        """The image-space pass without an optimizer (st_tile_gradient): partial sums as update() returns them; the combined
        gradient of the tile is then available from grad_tile()."""
        return self._image_pass(self.lib.st_tile_gradient, ring)

    # ---- L-BFGS pieces (tiled.TiledTransfer, optimizer='lbfgs'): vectors are compact (3, th, tw) tile tensors ----------------
    def vnew(self):
        _, _, th, tw = self._tile_rect()[0]
        return torch.empty((3, th, tw), dtype=torch.float32, device=self.device)

    def grad_tile(self):
        out = self.vnew()
        self.strips(self._buf(4, (3, self.wh, self.ww)), self._tile_rect(), out.reshape(-1), 0)
        return out

    def vcopy(self, v):
        out = self.vnew()
        out.copy_(v)                                    # (device-to-device copy: memory plumbing)
        torch.cuda.synchronize(self.device)
        return out

    def vdot(self, a, b):
        """This rank's partial sum of <a, b> as a 1-element device tensor (utils.dot, utils.py:29-36)."""
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        check(self.lib.st_vec_dot(self.ctx, c_void_p(a.data_ptr()), c_void_p(b.data_ptr()), a.numel(), c_void_p(out.data_ptr())))
        return out

    def vaxpy(self, alpha, x, y):
        """y += alpha x (utils.axpy, utils.py:38-47)."""
        torch.cuda.synchronize(self.device)
        check(self.lib.st_vec_axpy(self.ctx, float(F32(alpha)), c_void_p(x.data_ptr()), c_void_p(y.data_ptr()), x.numel()))

    def vscale(self, alpha, y):
        """y *= alpha, as y = (alpha - 1) y + y would not round the same way: axpy onto a zeroed vector."""
        src = self.vcopy(y)
        y.zero_()
        self.vaxpy(alpha, src, y)

    def vdiv(self, divisor, y):
        """y /= divisor with the quotient formed in double and rounded once (optimizers.py:99: p /= np.sqrt(...), a float64)."""
        torch.cuda.synchronize(self.device)
        check(self.lib.st_vec_div(self.ctx, float(divisor), c_void_p(y.data_ptr()), y.numel()))

    def apply_step(self, s):
        """x_next[tile] = x_cur[tile] + s; the rest of x_next starts as a copy of x_cur (its apron is refreshed by the caller)."""
        xt = self.vnew()
        rect = self._tile_rect()
        self.strips(self.x_cur(), rect, xt.reshape(-1), 0)
        self.vaxpy(1.0, s, xt)
        nxt = self.x_next()
        nxt.copy_(self.x_cur())
        torch.cuda.synchronize(self.device)
        self.strips(nxt, rect, xt.reshape(-1), 1)

    def finish_trace(self):
        """The trace of the evaluation whose phase buffers the caller has all-reduced in place (st_tile_trace: the finisher st_tile_step
        uses); same layout as the single-GPU engine: 6 per active layer + 8."""
        torch.cuda.synchronize(self.device)
        trace = np.zeros(self.engine.trace_len(), np.float64)
        check(self.lib.st_tile_trace(self.ctx, trace.ctypes.data_as(c_void_p)))
        return trace
