"""CPU side of the anchor term's plumbing: the trace names for every layout of the image part (8; 10 with the Laplacian term; 10 with the
anchor term; 12 with both), the refusals of the tile-sharded paths (jobs.run_tiled_job, tools/stylize.py --anchor with --grid),
jobs.warp_planar, and run_frames' refusal of frames that differ in size.  No GPU."""
import importlib.util
import inspect
import os

import numpy as np
import pytest

from style_transfer2_amd import jobs
from style_transfer2_amd.transfer import StyleTransfer

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def set_anchor(self, image, mask, weight):
        self.calls.append((image is not None, mask is not None, weight))

    def set_laplacian(self, levels):
        pass

    def set_weights(self, *args):
        pass


class _Model:
    def __init__(self):
        self.engine = _FakeEngine()

    def layers(self):
        return ['data', 'conv1_1']


def test_trace_names_for_the_four_layouts_of_the_image_part():
    st = StyleTransfer(_Model())
    st.set_weights({'content': {'conv1_1': 1}, 'style': {}, 'deepdream': {}}, {'p': 1, 'p_power': 6, 'tv': 1, 'tv_power': 2})
    layer = ['conv1_1_c_loss', 'conv1_1_c_grad']
    plain = layer + ['scd_loss', 't_loss', 'p_loss', 'scd_grad', 't_grad', 'p_grad', 'time', 'loss', 'grad']
    lap = layer + ['scd_loss', 't_loss', 'p_loss', 'l_loss', 'scd_grad', 't_grad', 'p_grad', 'l_grad', 'time', 'loss', 'grad']
    anchor = [k.replace('l_', 'a_') if k in ('l_loss', 'l_grad') else k for k in lap]
    both = layer + ['scd_loss', 't_loss', 'p_loss', 'l_loss', 'a_loss', 'scd_grad', 't_grad', 'p_grad', 'l_grad', 'a_grad', 'time', 'loss', 'grad']
    v8, v10, v12 = (np.arange(6 + n, dtype=np.float64) for n in (8, 10, 12))
    # this object never turned the term on: 10 values are the Laplacian term's
    assert list(st._make_trace(v8, True).data) == plain and list(st._make_trace(v10, True).data) == lap
    assert list(st._make_trace(v12, True).data) == both                   # (12 can only be both)
    st.set_anchor(np.zeros((4, 4, 3), np.uint8), None, 2.0)
    assert st.engine.calls == [(True, False, 2.0)]
    assert list(st._make_trace(v10, True).data) == anchor and list(st._make_trace(v12, True).data) == both
    t = st._make_trace(v10, True).data
    assert (t['p_loss'], t['a_loss'], t['scd_grad'], t['p_grad'], t['a_grad'], t['loss'], t['grad']) == (8, 9, 10, 12, 13, 14, 15)
    t = st._make_trace(v12, True).data
    assert (t['l_loss'], t['a_loss'], t['scd_grad'], t['l_grad'], t['a_grad'], t['loss'], t['grad']) == (9, 10, 11, 14, 15, 16, 17)
    assert list(st._make_trace(v12, False).data) == layer + ['scd_loss', 't_loss', 'p_loss', 'l_loss', 'a_loss', 'loss']
    assert st._make_trace(v12, False).data['loss'] == 16
    assert list(st._make_trace(v10, False).data) == layer + ['scd_loss', 't_loss', 'p_loss', 'a_loss', 'loss']
    st.set_anchor(None)
    assert st.engine.calls[-1] == (False, False, 1.0)
    assert list(st._make_trace(v10, True).data) == lap and list(st._make_trace(v8, True).data) == plain


def test_tile_sharded_jobs_refuse_the_term_before_anything_is_built():
    img = np.zeros((32, 32, 3), np.uint8)
    with pytest.raises(ValueError, match='tile-sharded'):
        jobs.run_tiled_job({}, img, img, 1, (1, 2), anchor=(img, None, 1.0))
    assert inspect.signature(jobs.run_job).parameters['anchor'].default is None


def _stylize():
    spec = importlib.util.spec_from_file_location('stylize_tool', os.path.join(ROOT, 'tools', 'stylize.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stylize_refuses_the_term_with_a_grid(capsys):
    tool = _stylize()
    args = tool.parser().parse_args(['c.jpg', 's.jpg', 'o.png', '--anchor', 'a.png', '--anchor-mask', 'm.png', '--anchor-weight', '3'])
    assert (args.anchor, args.anchor_mask, args.anchor_weight) == ('a.png', 'm.png', 3.0)
    with pytest.raises(SystemExit) as e:
        tool.main(['c.jpg', 's.jpg', 'o.png', '--anchor', 'a.png', '--grid', '1x2'])
    assert e.value.code == 2 and '--anchor with --grid' in capsys.readouterr().err


def test_frames_tool_parses_its_flags():
    spec = importlib.util.spec_from_file_location('stylize_frames_tool', os.path.join(ROOT, 'tools', 'stylize_frames.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    args = tool.parser().parse_args(['a.png', 'b.png', '--style', 's.jpg', '--out-dir', 'out', '--flows', 'f', '--masks', 'm', '--anchor-weight', '40',
                                     '--first-iters', '300', '--iters', '100', '--precision', 'bf16'])
    assert (args.frames, args.flows, args.masks, args.anchor_weight, args.first_iters, args.iters) == (['a.png', 'b.png'], 'f', 'm', 40.0, 300, 100)


# ---- warp_planar ---------------------------------------------------------------------------------------------------------------------
def planes(h, w, seed=0):
    return (np.random.RandomState(seed).rand(3, h, w) * 255 - 116).astype(F32)


@pytest.mark.parametrize('shift', [(0, 0), (1, 0), (0, 1), (-2, 3), (5, -4)], ids=str)
def test_integer_flows_reproduce_the_clamped_shift_bit_for_bit(shift):
    h, w = 7, 9
    x = planes(h, w)
    dx, dy = shift
    flow = np.empty((h, w, 2), F32)
    flow[..., 0], flow[..., 1] = dx, dy
    ys, xs = np.clip(np.arange(h) + dy, 0, h - 1), np.clip(np.arange(w) + dx, 0, w - 1)
    out = jobs.warp_planar(x, flow)
    assert out.dtype == F32 and out.shape == x.shape
    assert np.array_equal(out.view(np.uint32), x[:, ys][:, :, xs].view(np.uint32))


def test_a_half_pixel_flow_is_the_float32_of_the_float64_mean_of_two_neighbours():
    h, w = 5, 6
    x = planes(h, w, 1)
    flow = np.zeros((h, w, 2), F32)
    flow[..., 0] = 0.5
    out = jobs.warp_planar(x, flow)
    x64 = x.astype(np.float64)
    want = np.concatenate([(x64[:, :, :-1] + x64[:, :, 1:]) / 2, x64[:, :, -1:]], axis=2).astype(F32)      # the last column clamps
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_flows_pointing_outside_the_image_clamp():
    h, w = 4, 5
    x = planes(h, w, 2)
    flow = np.zeros((h, w, 2), F32)
    flow[..., 0], flow[..., 1] = -100.25, 1e6
    out = jobs.warp_planar(x, flow)
    assert np.array_equal(out, np.broadcast_to(x[:, -1:, :1], x.shape))   # every pixel samples the bottom-left corner
    flow[..., 0], flow[..., 1] = 100.75, -3.5
    assert np.array_equal(jobs.warp_planar(x, flow), np.broadcast_to(x[:, :1, -1:], x.shape))
    with pytest.raises(ValueError):
        jobs.warp_planar(x, np.zeros((h, w + 1, 2), F32))


def test_run_frames_refuses_frames_of_different_sizes_before_anything_runs():
    class Untouched:
        def __getattr__(self, name):
            raise AssertionError('run_frames touched the transfer (%s) before it refused' % name)
    a, b = np.zeros((24, 32, 3), np.uint8), np.zeros((24, 36, 3), np.uint8)
    with pytest.raises(ValueError, match='differ in size'):
        jobs.run_frames(Untouched(), [a, a, b], a, 2, 10.0)
    with pytest.raises(ValueError, match='one entry per frame'):
        jobs.run_frames(Untouched(), [a, a], a, 2, 10.0, flows=[None])
