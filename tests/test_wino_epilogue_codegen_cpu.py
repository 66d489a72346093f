"""Compile-only check of the twelve specialised-epilogue builds of csrc/conv3x3_winograd.hip (no GPU): the kernel is compiled for
gfx950 with the library's flags to assembly, and for each build
  * no scratch, the LDS it always had, and the occupancy it always had: one workgroup per CU for the 128-channel builds (more than 256
    of the 512 registers of a SIMD lane), two for the half-tile builds (at most 256);
  * after the last MFMA the vector-memory accesses are ordered loads first: no operand load behind the first store.  vmcnt counts
    loads and stores together in issue order, so a load behind a store makes its consumer wait for that store's acknowledgement too."""

import os
import re
import subprocess

import pytest

from style_transfer2_amd import build

KINDS = ('fwd', 'pool', 'poolonly', 'dgm', 'dg', 'unpool_dgm')
BUILDS = [('128x128', k) for k in KINDS] + [('h4_64x128', k) for k in KINDS]


@pytest.fixture(scope='module')
def assembly(tmp_path_factory):
    out = tmp_path_factory.mktemp('wino_asm') / 'conv3x3_winograd.s'
    cmd = [build._hipcc(), '-O3', '-std=c++17', '--offload-arch=' + build.ARCH, '-fPIC', '-Wall', '-Wno-unused-result',
           '--cuda-device-only', '-S', os.path.join(build.CSRC, 'conv3x3_winograd.hip'), '-o', str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out.read_text()


def _kernel(text, tile, kind):
    """(instruction lines, {.amdhsa_ directive: value}) of one build"""
    name = r'_ZN3st2\d+conv3x3_wino_f32_%s_%sENS_9WinoKArgsE' % (tile, kind)
    body = re.search(r'^%s:[^\n]*\n(.*?)^\s*s_endpgm' % name, text, re.S | re.M)
    desc = re.search(r'\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel' % name, text, re.S)
    assert body and desc, (tile, kind)
    lines = [l.split() for l in body.group(1).splitlines()]
    return [l for l in lines if l and not l[0].startswith((';', '.'))], dict(re.findall(r'\.amdhsa_(\w+) (\d+)', desc.group(1)))


@pytest.mark.parametrize('tile,kind', BUILDS)
def test_specialised_build_resources(assembly, tile, kind):
    _, d = _kernel(assembly, tile, kind)
    assert int(d['private_segment_fixed_size']) == 0                    # no scratch
    assert int(d['group_segment_fixed_size']) == (40960 if kind == 'unpool_dgm' else 49152)
    regs = (int(d['next_free_vgpr']) + 7) // 8 * 8                      # VGPRs + AGPRs, allocated in eights, 512 per SIMD lane
    assert 512 // regs == (1 if tile == '128x128' else 2), regs


@pytest.mark.parametrize('tile,kind', BUILDS)
def test_no_operand_load_behind_the_first_store(assembly, tile, kind):
    ins, _ = _kernel(assembly, tile, kind)
    last_mfma = max(i for i, l in enumerate(ins) if l[0].startswith('v_mfma'))
    seq = ['L' if l[0].startswith('buffer_load') else 'S' for l in ins[last_mfma + 1:] if l[0].startswith(('buffer_load', 'buffer_store'))]
    assert 'S' in seq                                                   # the epilogue is where the text says it is
    assert 'L' not in seq[seq.index('S'):], ''.join(seq)
    # ... and the operands are loaded at all, under the last chunk or behind it (16-byte loads; the compiler merges four bias dwords)
    loads = [l for l in ins if l[0].startswith('buffer_load') and 'lds' not in l]
    rows = 8 if tile == 'h4_64x128' else 16
    want = {'fwd': rows // 4, 'pool': rows // 4, 'poolonly': rows // 4, 'dgm': 2 * rows, 'dg': rows, 'unpool_dgm': 2 * rows}[kind]
    assert len(loads) >= want, (len(loads), want)
