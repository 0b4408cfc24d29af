"""CPU test on the ISA of the render step's kernels: the single-kernel compile of csrc/nfi_kernels.hip (NFI_SINGLE_KERNEL:
the headline render kernel render_fwd_kernel<0,true,2,0,1,false> and every non-render kernel of the unit, ~15 s) is read
as text.

* raygen_kernel holds no atomic: it stores one partial per block, which raygen_finish_kernel reduces (before: three
  global atomics at the end of every block, on three cells a memset had to clear).  slab_kernel (nfi_near_far, whose
  caller supplies the cells) keeps its three.
* The register budget of the headline kernel: no scratch, at most 224 vector registers (218 with this toolchain, before
  and after).

Two more ISA checks belong to the two parts of this round that did NOT show on the GPU and are not in the tree - the
split-phase work fetch (>= 500 instructions and no vmcnt wait between the hand-out atomic and the first read of its
result; before: 1) and the softplus by accumulator quads (<= 8 s_nop directly behind a v_exp_f32 / v_log_f32 per field
loop; before: 39 and 28).  They are kept, with the code they test, in tools/probes/patches/r7_*.patch (profiles/r7)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nerf_from_image_amd', 'csrc')
KERNEL = '_Z17render_fwd_kernelILi0ELb1ELi2ELi0ELi1ELb0EEv18RenderKernelParams'


@pytest.fixture(scope='module')
def listing(tmp_path_factory):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.fail('no hipcc at %s (set HIPCC)' % hipcc, pytrace=False)
    out = str(tmp_path_factory.mktemp('isa') / 'render_single.s')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-S', '--cuda-device-only',
           '-DNFI_SINGLE_KERNEL=0', '-DNFI_SINGLE_MODE=0', '-DNFI_RENDER_OCC=2', 'nfi_kernels.hip', '-o', out]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read()


def kernel_body(listing, name):
    """labels and instructions of the kernel whose mangled name starts with `name`; comments and directives dropped"""
    lines = listing.splitlines()
    start = next(i for i, ln in enumerate(lines) if re.match(r'%s\w*:' % re.escape(name), ln))
    out = []
    for ln in lines[start + 1:]:
        s = ln.strip()
        if s.startswith('.end_amdhsa_kernel') or s.startswith('.section') or s.startswith('.Lfunc_end'):
            break
        s = s.split(';')[0].strip()
        if not s or (s.startswith('.') and not s.endswith(':')):
            continue
        out.append(s)
    assert any(s.startswith('s_endpgm') for s in out), name
    return out


def test_register_budget(listing):
    # the kernel's entry in the code object metadata (keys in alphabetical order: .name ... .private_segment_fixed_size
    # ... .vgpr_count)
    meta = listing[re.search(r'\.name:\s+%s\n' % re.escape(KERNEL), listing).end():]
    scratch = int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', meta).group(1))
    vgprs = int(re.search(r'\.vgpr_count:\s+(\d+)', meta).group(1))
    print('vector registers %d, scratch %d bytes' % (vgprs, scratch))
    assert scratch == 0
    assert vgprs <= 224


def test_ray_setup_has_no_atomics(listing):
    counts = {}
    # (raygen_finish_kernel lives with the host code, outside the single-kernel compile: tests/test_render_setup_split_gpu.py
    #  runs it on a workspace filled with 0xff)
    for name in ('_Z13raygen_kernel', '_Z11slab_kernel'):
        body = kernel_body(listing, name)
        counts[name] = sum('atomic' in s for s in body)
        assert any(s.startswith('global_store') for s in body), name
    print(counts)
    assert counts['_Z13raygen_kernel'] == 0
    assert counts['_Z11slab_kernel'] == 3
