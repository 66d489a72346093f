"""Drop-in boundary on the CPU: wire compatibility of messages.py with the reference's pickles, the
worker's message loop and ordering guarantees, the C ABI surface, and the "no CPU fallback" rule."""
import json
import os
import pickle
import re
import subprocess
import sys
from collections import OrderedDict, deque

import numpy as np
import pytest

import messages
import worker as worker_mod
from helpers import GOLDEN, load_json
from style_transfer2_amd import capi, transfer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ------------------------------------------------------------------------------------- messages
def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    return type(a) == type(b) and a == b


def _ours():
    m = messages
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    weights = {'content': {'conv2_2': 0.08, 'conv1_2': 0.5},
               'style': {'conv1_1': 1, 'conv2_1': 1, 'conv1_2': 0.3, 'pool1': 0.7}, 'deepdream': {'conv2_1': 0.02}}
    params = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
    return OrderedDict([
        ('SetImages', m.SetImages(None, img, img, m.SetImages.RESAMPLE, True)),
        ('SetImagesResample', m.SetImages((4, 6), m.SetImages.RESAMPLE, m.SetImages.RESAMPLE)),
        ('SetOptimizer', m.SetOptimizer('adam')),
        ('SetOptimizerStep', m.SetOptimizer('lbfgs', 0.5)),
        ('SetWeights', m.SetWeights(weights, params)),
        ('StartIteration', m.StartIteration()), ('PauseIteration', m.PauseIteration()),
        ('Shutdown', m.Shutdown()), ('WorkerReady', m.WorkerReady(['data', 'conv1_1'])),
        ('Iterate', m.Iterate(img.astype(F32), 3, OrderedDict(loss=1.5, fevals=3))),
        ('GetImages', m.GetImages()),
    ])


def test_messages_are_byte_compatible_with_the_reference_pickles():
    """Reference pickles load into our classes with identical state, and our pickles are the same
    BYTES as the reference's (same module path, class names, attribute names and order)."""
    golden = load_json('message_pickles.json')
    for name, obj in _ours().items():
        ref_bytes = bytes.fromhex(golden[name])
        theirs = pickle.loads(ref_bytes)
        assert type(theirs) is type(obj) and type(theirs).__module__ == 'messages'
        assert _same(vars(theirs), vars(obj)), name
        assert pickle.dumps(obj, protocol=pickle.DEFAULT_PROTOCOL) == ref_bytes, name


def test_message_constants_and_validation():
    assert messages.SetImages.RESAMPLE == 1
    assert messages.SetOptimizer.step_sizes == {'adam': 10, 'lbfgs': 1}
    assert messages.SetWeights.loss_names == ('content', 'style', 'deepdream')
    assert messages.SetWeights.scalar_loss_names == ('tv', 'tv_power', 'p', 'p_power')
    assert messages.SetOptimizer('adam').step_size == 10 and messages.SetOptimizer('lbfgs', 3).step_size == 3
    with pytest.raises(ValueError):
        messages.SetOptimizer('sgd')
    assert messages.WorkerReady().layers == []
    assert 'ndarray, shape: (2, 2, 3)' in repr(messages.Iterate(np.zeros((2, 2, 3), F32), 1, {}))
    for extra in ('AppUp', 'AppDown', 'Reset'):
        assert hasattr(messages, extra)


# --------------------------------------------------------------------------------------- worker
class FakeSockets:
    """In-process stand-in for the PULL/PUSH pair (pyzmq is not installed in the build container)."""
    class Again(Exception):
        pass

    def __init__(self, inbound):
        self.inbound = deque(inbound)
        self.sent = []

    def recv_pyobj(self, flags=0):
        if not self.inbound:
            if flags:
                raise self.Again()
            return messages.Shutdown()
        return pickle.loads(pickle.dumps(self.inbound.popleft()))

    def send_pyobj(self, obj):
        self.sent.append(pickle.loads(pickle.dumps(obj)))


class FakeTransfer:
    """Records calls; becomes runnable once all three images are set (reference worker.py:140-189)."""
    def __init__(self, max_steps=3):
        self.calls, self.is_running, self.t, self.max_steps = [], False, 0, max_steps
        self.have = set()
        self.optimizer, self.optimizer_cls, self.step_size = None, None, None
        self.model = type('M', (), {'layers': staticmethod(lambda: ['data', 'conv1_1'])})()

    def __getattr__(self, name):
        if name.startswith('set_') or name.startswith('resample_') or name in ('reset', 'pause'):
            def call(*a):
                self.calls.append(name)
                if name in ('set_input', 'set_content', 'set_style'):
                    self.have.add(name)
                if name == 'pause':
                    self.is_running = False
            return call
        raise AttributeError(name)

    def check_consistency(self):
        return len(self.have) == 3

    def start(self):
        self.calls.append('start')
        self.is_running = self.check_consistency()
        return self.is_running

    def step(self):
        self.t += 1
        if self.t >= self.max_steps:
            self.is_running = False
        return np.full((2, 2, 3), self.t, F32), OrderedDict(loss=float(self.t), fevals=self.t)


def run_worker(inbound, transfer_obj):
    socks = FakeSockets(inbound)
    wk = worker_mod.Worker({}, sock_in=socks, sock_out=socks, transfer=transfer_obj)
    wk.run()
    return socks.sent, transfer_obj


def test_worker_protocol_order_and_iterates():
    img = np.zeros((4, 4, 3), np.uint8)
    sent, tr = run_worker([messages.SetImages(None, img, img, img, True),
                           messages.SetWeights({'content': {}, 'style': {}, 'deepdream': {}}, {}),
                           messages.SetOptimizer('adam', 10), messages.StartIteration()], FakeTransfer(3))
    kinds = [type(m).__name__ for m in sent]
    assert kinds == ['WorkerReady', 'Iterate', 'Iterate', 'Iterate', 'Shutdown']
    assert sent[0].layers == ['data', 'conv1_1']
    assert [m.i for m in sent[1:4]] == [1, 2, 3] and sent[3].trace['fevals'] == 3
    assert sent[1].image.dtype == F32 and sent[1].image.shape == (2, 2, 3)
    assert tr.calls[:4] == ['set_input', 'set_content', 'set_style', 'reset']
    assert 'set_weights' in tr.calls and 'set_step_size' in tr.calls and tr.calls[-1] == 'start'


class FakePipelinedTransfer(FakeTransfer):
    """A backend with the two-half iteration (st_step_begin / st_step_end): at most two in flight, results in begin order."""
    def __init__(self, max_steps=5, on_begin=None):
        super().__init__(max_steps)
        self.inflight, self.on_begin = [], on_begin

    def step(self):
        raise AssertionError('the pipelined loop never calls step()')

    def step_begin(self):
        assert len(self.inflight) < 2, 'more than two iterations in flight'
        self.t += 1
        self.inflight.append(self.t)
        self.calls.append('begin%d' % self.t)
        if self.t >= self.max_steps:
            self.is_running = False
        if self.on_begin:
            self.on_begin(self.t)

    def step_end(self):
        i = self.inflight.pop(0)
        self.calls.append('end%d' % i)
        return np.full((2, 2, 3), i, F32), OrderedDict(loss=float(i), fevals=i), i

    @property
    def steps_pending(self):
        return len(self.inflight)


@pytest.mark.parametrize('async_iterate', ['0', '1'])
def test_worker_pipelined_iterations_keep_the_wire_and_the_message_order(async_iterate):
    """Pipelined loop (worker.py: iteration k + 1 is begun before iterate k is collected): the wire carries what the plain loop
    sends -- one Iterate per step, in order, Shutdown last -- and a message that arrives mid-run is acted on only after every
    iteration begun before it has been collected and sent (reference worker.py:380-395 polls between steps)."""
    img = np.zeros((4, 4, 3), np.uint8)
    socks = FakeSockets([messages.SetImages(None, img, img, img, True), messages.StartIteration()])
    tr = FakePipelinedTransfer(5, on_begin=lambda t: socks.inbound.append(messages.SetWeights({'content': {}, 'style': {}, 'deepdream': {}}, {}))
                               if t == 3 else None)
    wk = worker_mod.Worker({'async_iterate': async_iterate}, sock_in=socks, sock_out=socks, transfer=tr)
    assert wk.pipelined
    wk.run()
    kinds = [type(m).__name__ for m in socks.sent]
    assert kinds == ['WorkerReady'] + ['Iterate'] * 5 + ['Shutdown']
    its = [m for m in socks.sent if isinstance(m, messages.Iterate)]
    assert [m.i for m in its] == [1, 2, 3, 4, 5] and [m.trace['fevals'] for m in its] == [1, 2, 3, 4, 5]
    assert [float(m.image[0, 0, 0]) for m in its] == [1, 2, 3, 4, 5]
    steps = [c for c in tr.calls if c.startswith(('begin', 'end', 'set_weights'))]
    # one iteration ahead in steady state; everything begun before the message is collected before the message is handled
    assert steps == ['begin1', 'begin2', 'end1', 'begin3', 'end2', 'end3', 'set_weights', 'begin4', 'begin5', 'end4', 'end5']
    # the plain loop on a backend without the two halves, or when switched off
    plain = worker_mod.Worker({'pipeline_iterate': '0'}, sock_in=FakeSockets([]), sock_out=FakeSockets([]), transfer=FakePipelinedTransfer())
    assert not plain.pipelined
    plain.close()
    assert not worker_mod.Worker({}, sock_in=FakeSockets([]), sock_out=FakeSockets([]), transfer=FakeTransfer()).pipelined


def zmq_module(monkeypatch):
    """pyzmq where it is installed; otherwise tests/minizmq.py (ZMTP 3.0 PUSH / PULL on real TCP sockets) stands in as `zmq`."""
    try:
        import zmq
        return zmq, 'pyzmq'
    except ImportError:
        import minizmq
        monkeypatch.setitem(sys.modules, 'zmq', minizmq)
        return minizmq, 'minizmq (ZMTP 3.0 over TCP; pyzmq is not installed)'


def run_worker_over_tcp(zmq, transfer_obj, n_iterates, extra_config=None):
    """The reference's deployment (worker.py:321-324): the worker creates its own PULL (bind) / PUSH (connect) sockets from the config;
    an "app" on the other side of two TCP connections sends SetImages + StartIteration, collects, then sends Shutdown."""
    import threading
    ctx = zmq.Context()
    app_in = ctx.socket(zmq.PULL)
    port_app = app_in.bind_to_random_port('tcp://127.0.0.1')
    probe = ctx.socket(zmq.PULL)
    port_worker = probe.bind_to_random_port('tcp://127.0.0.1')
    probe.close(0)
    config = {'worker_socket': 'tcp://127.0.0.1:%d' % port_worker, 'app_socket': 'tcp://127.0.0.1:%d' % port_app, 'async_iterate': '1'}
    config.update(extra_config or {})
    img = np.zeros((4, 4, 3), np.uint8)
    wk = worker_mod.Worker(config, transfer=transfer_obj)
    t = threading.Thread(target=wk.run, daemon=True)
    t.start()
    app_out = ctx.socket(zmq.PUSH)
    app_out.connect(config['worker_socket'])
    for m in (messages.SetImages(None, img, img, img, True), messages.StartIteration()):
        app_out.send_pyobj(m)
    got = []
    poller = zmq.Poller()
    poller.register(app_in, zmq.POLLIN)
    while len(got) < 1 + n_iterates and poller.poll(10000):
        got.append(app_in.recv_pyobj())
    app_out.send_pyobj(messages.Shutdown())
    while poller.poll(10000):
        got.append(app_in.recv_pyobj())
        if isinstance(got[-1], messages.Shutdown):
            break
    t.join(20)
    wk.close()
    app_out.close(0); app_in.close(0); ctx.destroy(0)
    return wk, got


def test_worker_over_its_own_tcp_sockets_loopback(monkeypatch):
    """The transport the reference uses (worker.py:321-324: PULL bind / PUSH connect, send_pyobj / recv_pyobj) with the sender
    thread on: WorkerReady -> Iterates in order -> Shutdown last, over real TCP connections.  With pyzmq where it exists; in this
    image through tests/minizmq.py, which frames the same pickles per ZMTP 3.0."""
    zmq, which = zmq_module(monkeypatch)
    wk, got = run_worker_over_tcp(zmq, FakePipelinedTransfer(4), 4)
    print('[transport] worker loopback ran over', which)
    kinds = [type(m).__name__ for m in got]
    assert kinds == ['WorkerReady'] + ['Iterate'] * 4 + ['Shutdown']
    assert [m.i for m in got[1:5]] == [1, 2, 3, 4]
    assert not wk.zero_copy                                  # this backend offers no frames: owned copies through send_pyobj


def test_minizmq_frames_follow_zmtp_3(monkeypatch):
    """What tests/minizmq.py puts on the wire, read back byte by byte: 64-byte greeting (signature, version 3.0, NULL mechanism),
    a READY command naming the socket type, then one frame per message -- short (1-byte size) or long (flag 0x02, 8-byte size)."""
    import socket as socket_mod
    import minizmq
    srv = socket_mod.socket()
    srv.bind(('127.0.0.1', 0))
    srv.listen(1)
    ctx = minizmq.Context()
    push = ctx.socket(minizmq.PUSH)
    push.connect('tcp://127.0.0.1:%d' % srv.getsockname()[1])
    import threading
    big = bytes(range(256)) * 5
    th = threading.Thread(target=lambda: (push.send(b'abc'), push.send(big, copy=False, track=True).wait()), daemon=True)
    th.start()
    conn, _ = srv.accept()
    conn.sendall(minizmq._greeting() + minizmq._ready(minizmq.PULL))

    def exact(n):
        out = b''
        while len(out) < n:
            out += conn.recv(n - len(out))
        return out
    g = exact(64)
    assert g[0] == 0xff and g[9] == 0x7f and g[10:12] == b'\x03\x00' and g[12:16] == b'NULL' and not any(g[16:32]) and g[32] == 0
    flags, size = exact(2)
    ready = exact(size)
    assert flags == 0x04 and ready.startswith(b'\x05READY\x0bSocket-Type\x00\x00\x00\x04PUSH')
    assert exact(2) == b'\x00\x03' and exact(3) == b'abc'                            # short frame
    assert exact(1) == b'\x02' and int.from_bytes(exact(8), 'big') == len(big) and exact(len(big)) == big     # long frame
    th.join(5)
    conn.close(); srv.close(); ctx.destroy(0)


def test_worker_asks_for_images_when_it_cannot_start_and_survives_garbage():
    sent, tr = run_worker([messages.StartIteration(), 'not a message', messages.PauseIteration()], FakeTransfer())
    assert [type(m).__name__ for m in sent] == ['WorkerReady', 'GetImages', 'Shutdown']
    assert tr.calls == ['start', 'pause']


def test_worker_resample_sentinels_route_to_resample_methods():
    sent, tr = run_worker([messages.SetImages((6, 8), messages.SetImages.RESAMPLE, messages.SetImages.RESAMPLE)],
                          FakeTransfer())
    assert tr.calls == ['resample_input', 'resample_content']


def test_worker_exits_with_code_2_without_backend(tmp_path):
    """reference worker.py:51-53: missing compute backend -> message on stderr + exit code 2."""
    cfg = tmp_path / 'c.ini'
    cfg.write_text('[DEFAULT]\nweights = synthetic\ngpu = 0\nworker_socket = inproc://a\napp_socket = inproc://b\n')
    code = ("import sys, types; sys.argv=['worker.py', %r];"
            "z=types.ModuleType('zmq'); z.Context=lambda: types.SimpleNamespace(socket=lambda k: types.SimpleNamespace("
            "bind=lambda a: None, connect=lambda a: None, send_pyobj=lambda o: None), destroy=lambda l: None);"
            "z.PULL=z.PUSH=z.NOBLOCK=1; z.ZMQError=Exception; sys.modules['zmq']=z;"
            "import worker; worker.main()") % str(cfg)
    r = subprocess.run([sys.executable, '-c', code], cwd=REPO, capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES='-1'))
    assert r.returncode == 2, r.stderr
    assert 'compute backend is unavailable' in r.stderr


# --------------------------------------------------------------------------------------- C ABI
def test_every_header_symbol_is_exported_and_bound():
    header = open(os.path.join(REPO, 'include', 'st2.h')).read()
    declared = set(re.findall(r'\b(st_[a-z0-9_]+)\s*\(', header))
    assert len(declared) >= 35
    lib = capi.load_library()                      # loads without a GPU
    for name in declared:
        assert hasattr(lib, name), 'header declares %s but the library does not export it' % name
    assert declared == set(capi.PROTOTYPES), declared ^ set(capi.PROTOTYPES)
    for line in re.findall(r'/\*.*?\*/', header, re.S)[:1]:
        assert 'worker.py' in line                 # the header cites the reference interfaces it replaces


def test_engine_fails_loudly_without_a_gpu():
    import style_transfer2_amd as st2
    r = subprocess.run([sys.executable, '-c',
                        'import style_transfer2_amd as s\ntry:\n s.Engine()\nexcept s.StError as e:\n print("ERR", e)'],
                       cwd=REPO, capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES='-1'))
    assert 'ERR st2 error 3' in r.stdout, r.stdout + r.stderr
    os.environ['ST2_HIP_LIB'] = '/nonexistent/libst2_hip.so'
    try:
        capi._lib = None
        with pytest.raises(st2.HipUnavailable):
            capi.load_library()
    finally:
        del os.environ['ST2_HIP_LIB']
        capi._lib = None


def test_product_code_never_imports_the_oracle():
    """oracle/ is test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may use it."""
    offenders = []
    for root, dirs, files in os.walk(os.path.join(REPO, 'style_transfer2_amd')):
        for f in files:
            if f.endswith(('.py', '.cpp', '.hip', '.h')):
                text = open(os.path.join(root, f)).read()
                if re.search(r'^\s*(import|from)\s+oracle\b', text, re.M) or 'oracle/' in text and f.endswith('.py'):
                    offenders.append(f)
    for f in ('worker.py', 'messages.py'):
        if re.search(r'^\s*(import|from)\s+oracle\b', open(os.path.join(REPO, f)).read(), re.M):
            offenders.append(f)
    assert not offenders, offenders
    bench = open(os.path.join(REPO, 'bench.py')).read()
    assert bench.count('import oracle') == 1
    assert bench.split('import oracle')[0].rsplit('\ndef ', 1)[1].startswith('cpu_baseline_and_parity(')   # only inside that leg
    assert 'oracle' not in open(os.path.join(REPO, 'tools', 'probes', 'probes.hip')).read()


def test_every_environment_switch_the_engine_reads_is_in_the_readme_table():
    """Every ST2_* switch of style_transfer2_amd/csrc is read through env.h's helpers (no getenv anywhere else), and the set of names
    handed to them equals the set in README.md's environment table, bar the names only Python reads."""
    python_only = {'ST2_HIP_LIB', 'ST2_WS_VAR'}        # capi.load_library, build.py
    csrc = os.path.join(REPO, 'style_transfer2_amd', 'csrc')
    read = set()
    for f in sorted(os.listdir(csrc)):
        if not f.endswith(('.cpp', '.hip', '.h')):
            continue
        text = open(os.path.join(csrc, f)).read()
        if f != 'env.h':
            assert 'getenv' not in text, f
        calls = re.findall(r'\benv_(?:off|on|int|get)\(\s*([^,)]*)', text)
        for arg in calls:
            if f == 'env.h' and arg.strip() in ('const char* name', 'name'):
                continue                                # the helpers' own definitions
            m = re.fullmatch(r'"(ST2_[A-Z0-9_]+)"', arg.strip())
            assert m, '%s: %s is not a literal switch name' % (f, arg)
            read.add(m.group(1))
    table = set()
    for line in open(os.path.join(REPO, 'README.md')):
        if line.startswith('|'):
            table |= set(re.findall(r'ST2_[A-Z0-9_]+', line))
    assert len(read) > 40
    assert read | python_only == table, (sorted(read - table), sorted(table - read - python_only))


def _code_object_kernels(lib):
    """{kernel name: metadata dict} of every gfx950 code object bundled in a shared library (llvm-objdump --offloading
    + llvm-readelf --notes on a scratch copy)."""
    import shutil
    import tempfile
    llvm = '/opt/rocm/lib/llvm/bin'
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = shutil.copy(lib, tmp)
        subprocess.run([os.path.join(llvm, 'llvm-objdump'), '--offloading', copy], check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if 'amdgcn' not in f:
                continue
            notes = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '--notes', os.path.join(tmp, f)], check=True,
                                   capture_output=True, text=True).stdout
            cur = None
            for line in notes.splitlines():
                m = re.match(r'\s*-?\s*\.(\w+):\s+(\S+)', line)
                if not m:
                    continue
                key, val = m.groups()
                if key == 'name' and val.startswith('_Z'):
                    cur = kernels.setdefault(val, {})
                elif cur is not None and key in ('private_segment_fixed_size', 'vgpr_spill_count', 'vgpr_count', 'sgpr_spill_count'):
                    cur[key] = int(val)
    return kernels


def test_no_product_kernel_uses_scratch():
    """Every kernel of libst2_hip.so keeps its state in registers / LDS: no private segment, no VGPR spills (a
    512-register kernel that spills is what faulted in round 1's operand-feed probe, now in tools/probes/)."""
    if not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-readelf'):
        pytest.skip('ROCm llvm tools absent')
    kernels = _code_object_kernels(capi.lib_path())
    assert len(kernels) >= 40, len(kernels)
    bad = {k: v for k, v in kernels.items() if v.get('private_segment_fixed_size', 0) or v.get('vgpr_spill_count', 0)}
    assert not bad, bad
    assert not [k for k in kernels if 'probe' in k], 'development probes belong to tools/probes/, not the product library'


def test_no_product_kernel_stores_16_bytes_at_an_sgpr_offset():
    """A buffer store of more than 64 bits whose soffset is an SGPR may be followed at once by a VALU write of its data registers
    (hipcc guards that hazard only for a constant soffset), and gfx950 then stores the NEW value in some lanes -- measured in round 5
    (conv3x3_mfma_bf16.hip, kOOBStore).  The kernels fold the wave-uniform offset into the vector offset instead; this keeps it so."""
    llvm = '/opt/rocm/lib/llvm/bin'
    if not os.path.exists(os.path.join(llvm, 'llvm-objdump')):
        pytest.skip('ROCm llvm tools absent')
    import shutil
    import tempfile
    wide, bad = 0, []
    with tempfile.TemporaryDirectory() as tmp:
        copy = shutil.copy(capi.lib_path(), tmp)
        subprocess.run([os.path.join(llvm, 'llvm-objdump'), '--offloading', copy], check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if 'amdgcn' not in f:
                continue
            asm = subprocess.run([os.path.join(llvm, 'llvm-objdump'), '-d', '--no-show-raw-insn', os.path.join(tmp, f)], check=True,
                                 capture_output=True, text=True).stdout
            for line in asm.splitlines():
                m = re.search(r'buffer_store_dwordx[34]\s+v\[\d+:\d+\],\s*(?:v\d+|off),\s*s\[\d+:\d+\],\s*(\S+)', line)
                if m:
                    wide += 1
                    if re.match(r'(s\d+|m0|ttmp\d+)', m.group(1)):
                        bad.append(line.strip())
    assert wide >= 100, wide                      # (the pattern still matches this disassembler's output)
    assert not bad, bad[:5]


# --------------------------------------------------------------------------- host-side mirrors
def test_package_weight_table_matches_pandas_vectors():
    for name, case in load_json('weight_order.json').items():
        rows, cells = transfer.weight_table(case['weights'])
        assert rows == case['rows'], name
        for kind, col in case['cells'].items():
            for layer, v in col.items():
                got = cells[kind][layer]
                assert (np.isnan(got) if v is None else float(got) == v), (name, kind, layer)


def test_config1_inputs_fixture_geometry():
    g = np.load(os.path.join(GOLDEN, 'config1_inputs.npz'))
    assert g['golden_gate'].shape == (192, 256, 3) and g['starry_night'].shape == (160, 256, 3)
    assert g['golden_gate'].dtype == np.uint8


def test_async_sender_keeps_order_and_flushes_before_close():
    import time

    class SlowSock:
        def __init__(self):
            self.sent = []

        def send_pyobj(self, obj):
            time.sleep(0.01)
            self.sent.append(obj)

    sock = SlowSock()
    sender = worker_mod.AsyncSender(sock, depth=2)
    t0 = time.perf_counter()
    for i in range(8):
        sender.send_pyobj(i)
    queued_in = time.perf_counter() - t0
    sender.close()
    assert sock.sent == list(range(8))
    assert queued_in >= 0.04            # bounded queue: the producer was held back, not 8 sends deep

    class BadSock:
        def send_pyobj(self, obj):
            raise OSError('peer gone')

    sender = worker_mod.AsyncSender(BadSock())
    sender.send_pyobj(1)
    time.sleep(0.05)
    with pytest.raises(OSError):
        sender.send_pyobj(2)
    with pytest.raises(OSError):
        sender.close()


def test_worker_synchronous_send_option():
    socks = FakeSockets([messages.StartIteration()])
    wk = worker_mod.Worker({'async_iterate': '0'}, sock_in=socks, sock_out=socks, transfer=FakeTransfer())
    assert wk.sock_out is socks
    wk.run()
    assert [type(m).__name__ for m in socks.sent] == ['WorkerReady', 'GetImages', 'Shutdown']


def test_new_entry_points_refuse_null_handles_without_a_gpu():
    """The round-3 additions to the C ABI (frame room, communicator, exchange plans, the in-engine tile step) check their arguments
    before they touch the device: a NULL context is ST_ERR_ARG / ST_ERR_STATE with a message, here, without a GPU."""
    lib = capi.load_library()
    assert lib.st_step_frame_room(None, 4096, 65536) == 1 and b'NULL' in lib.st_last_error()
    assert lib.st_comm_unique_id(None) == 1
    assert lib.st_comm_init(None, b'\0' * capi.COMM_ID_BYTES, 0, 1) == 1
    assert lib.st_comm_destroy(None) == 1 and lib.st_comm_barrier(None) == 1
    assert lib.st_tile_plan(None, 0, 0, None) == 1
    assert lib.st_tile_step(None, None) == 2 and lib.st_tile_get_tile(None, None) == 2
    assert lib.st_tile_trace(None, None) == 1
    assert lib.st_vec_div(None, 1.0, None, 0) == 1
    # the layer-terms hook: bound with the header's six arguments, and a NULL context is an argument error with a message
    assert 'st_get_layer_terms' in capi.PROTOTYPES and len(capi.PROTOTYPES['st_get_layer_terms'][1]) == 6
    assert lib.st_get_layer_terms(None, 0, None, None, None, None) == 1 and b'bad argument' in lib.st_last_error()
