"""CPU restatement of Caffe's average pooling (``pool: AVE``, kernel 2, stride 2, pad 0) for the tests.  TEST INFRASTRUCTURE.

Caffe PoolingLayer::Forward_cpu / Backward_cpu, AVE, as Caffe's own CPU / CUDA layer computes it:
  * output size ceil((n - 2) / 2) + 1 per axis, as for MAX (oracle.caffe_net.pooled_size);
  * forward: top = 0 + x[r0, c0] + x[r0, c0 + 1] + x[r0 + 1, c0] + x[r0 + 1, c0 + 1] over the in-image elements of the window,
    in that (row-major) order, then divided by the clipped window size (4, 2 or 1);
  * backward: every in-image element of a window receives top_diff / window size (windows do not overlap).
``AveNetOracle`` runs the topologies' ``('pool', name, 'ave')`` layers that way and everything else as ``NetOracle`` does, the bf16
operand rounding included (pooling stays fp32; the next conv rounds its input), so ``oracle.TransferOracle`` drives it unchanged.
"""

from collections import OrderedDict

import numpy as np

from oracle.caffe_net import NetOracle, _tick, bf16_round, conv3x3_backward_data, conv3x3_forward, maxpool_backward, \
    maxpool_forward, pooled_size

F32 = np.float32


def is_ave(layer):
    return layer[0] == 'pool' and len(layer) > 2 and layer[2] == 'ave'


def window_sizes(h, w):
    """(ho, wo) float32 array of the clipped window sizes."""
    ho, wo = pooled_size(h), pooled_size(w)
    rows = np.minimum(2 * np.arange(ho) + 2, h) - 2 * np.arange(ho)
    cols = np.minimum(2 * np.arange(wo) + 2, w) - 2 * np.arange(wo)
    return (rows[:, None] * cols[None, :]).astype(F32)


def avepool_forward(x):
    """(C, h, w) -> (C, ho, wo), Caffe's summation order, one IEEE operation per step."""
    c, h, w = x.shape
    ho, wo = pooled_size(h), pooled_size(w)
    pad = np.zeros((c, 2 * ho, 2 * wo), F32)
    pad[:, :h, :w] = x
    top = np.zeros((c, ho, wo), F32)
    # a clipped window skips the terms outside the blob, as Caffe's loop bounds do (adding the padding's zeros instead would turn a
    # -0 sum into +0)
    for dr in (0, 1):
        for dc in (0, 1):
            term = pad[:, dr::2, dc::2]
            inside = ((2 * np.arange(ho) + dr) < h)[:, None] & ((2 * np.arange(wo) + dc) < w)[None, :]
            top = np.where(inside, top + term, top).astype(F32)
    return (top / window_sizes(h, w)).astype(F32)


def avepool_backward(dy, in_shape):
    """(C, ho, wo) pooled diff -> (C, h, w): every element of a window gets dy / window size."""
    c, h, w = in_shape
    share = (dy / window_sizes(h, w)).astype(F32)
    full = np.repeat(np.repeat(share, 2, axis=1), 2, axis=2)
    return np.ascontiguousarray(full[:, :h, :w])


class AveNetOracle(NetOracle):
    """NetOracle with average pools (topology layers ``('pool', name, 'ave')``)."""

    def forward(self, image, layers=None):
        wanted = self.layers() if layers is None else list(layers)
        last = len(self.topology)
        if not self.full_forward and wanted:
            last = max(self.blob_names.index(n) for n in wanted)
        x = np.ascontiguousarray(image[0], F32)
        self._blobs = {'data': x}
        self._slots = {}
        for layer in self.topology[:last]:
            if layer[0] == 'conv':
                w, b = self.params[layer[1]]
                if self.operands == 'bf16' and layer[2] % 8 == 0:
                    x = conv3x3_forward(bf16_round(x), self._weights16(layer[1]), b)
                else:
                    x = conv3x3_forward(x, w, b)
                np.maximum(x, 0, out=x)
            elif is_ave(layer):
                x = avepool_forward(x)
            else:
                x, self._slots[layer[1]] = maxpool_forward(x)
            self._blobs[layer[1]] = x
            _tick()
        return OrderedDict((n, self._blobs[n][None]) for n in wanted)

    def adopt_forward_state(self, blobs):
        """As NetOracle's; an average pool has no arg-max to adopt (only the ReLU masks of the conv blobs matter)."""
        for name, arr in blobs.items():
            self._blobs[name] = np.ascontiguousarray(np.asarray(arr, F32)[0])
        for i, layer in enumerate(self.topology):
            if layer[0] == 'pool' and not is_ave(layer) and self.blob_names[i] in self._blobs and layer[1] in self._slots:
                _, self._slots[layer[1]] = maxpool_forward(self._blobs[self.blob_names[i]])

    def backward(self, diffs):
        """NetOracle.backward's rules (ReLU mask on the diff arriving at a conv blob, injected diff added unmasked) with average
        pools: the pool's bottom diff is its top diff spread over the window, divided by the window size."""
        present = [i for i, n in enumerate(self.blob_names) if n in diffs]
        c, h, w = self._blobs['data'].shape
        if not present:
            return np.zeros((1, c, h, w), F32)
        top = max(present)
        g = None
        for i in range(top, 0, -1):
            layer = self.topology[i - 1]
            name = layer[1]
            if g is not None and layer[0] == 'conv':
                g = g * (self._blobs[name] > 0)
            if name in diffs:
                inj = np.asarray(diffs[name], F32)[0]
                g = inj.copy() if g is None else g + inj
            if layer[0] == 'conv':
                if self.operands == 'bf16' and layer[3] % 8 == 0:
                    g = conv3x3_backward_data(bf16_round(g), self._weights16(name))
                else:
                    g = conv3x3_backward_data(g, self.params[name][0])
            elif is_ave(layer):
                g = avepool_backward(g, self._blobs[self.blob_names[i - 1]].shape)
            else:
                below = self.blob_names[i - 1]
                g = maxpool_backward(g, self._slots[name], self._blobs[below].shape)
            _tick()
        if 'data' in diffs:
            inj = np.asarray(diffs['data'], F32)[0]
            g = inj.copy() if g is None else g + inj
        return g[None]
