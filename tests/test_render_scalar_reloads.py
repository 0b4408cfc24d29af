"""CPU test on the ISA of the headline render kernel render_fwd_kernel<0,true,2,0,1,false>: how many loop-invariant scalars
it fetches back from lanes of vector registers while it marches a ray.  The single-kernel compile of
tests/test_render_isa_stalls.py (~20 s) is read as text.

The kernel has no scalar register to spare (106 of them), and what does not fit is kept in lanes of a vector register
(v_writelane_b32 in the prologue) and fetched back with v_readlane_b32 - a VECTOR instruction, in a kernel bound by vector
issue, for a value that never changes during the launch.  Before round 19 the kernel kept 121 scalars that way in two
registers and the marched path of the ray loop held 216 such reloads of 110 slots (profiles/r19): the eighteen conditions
on the number of attention rows of sample_epilogue as 64-bit lane masks, the pointers and strides of the next ray's input
loads, the output pointers, the conditions on S / 2 S of the resampling, the merge and the composite.  Now the arguments
are read again from the argument segment at their use (kernel_args_here: scalar loads) and the conditions are scalar
compares at their use (scalar_here); 27 scalars are left in lanes of one register and the marched path reloads 22.

Definitions (all textual, on the listing):
  carriers      the destination registers of v_writelane_b32
  reload        v_readlane_b32 from a carrier
  field loops   the innermost backward-branch regions that hold MFMAs (coarse and fine pass: two)
  ray loop      the widest backward-branch region that holds both field loops
  marched path  the ray loop from its head to the first atomic behind the second field loop - the hand-out of the next
                position; from there on the loop is the work fetch, ray_at, the pixel store and skip_miss_run
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nerf_from_image_amd', 'csrc')
KERNEL = '_Z17render_fwd_kernelILi0ELb1ELi2ELi0ELi1ELb0EEv18RenderKernelParams'

# the parent of round 19, same toolchain, same definitions (profiles/r19/README.md)
PARENT_MARCHED_RELOADS = 216
PARENT_READFIRSTLANE = 95
# what the tree reaches (22) plus a tenth, and in no case more than 91: half the 182 the issue counted in the parent, on a
# narrower marched path (this one runs on through the pixel store to the hand-out's atomic)
TREE_MARCHED_RELOADS = 22
LIMIT = min(TREE_MARCHED_RELOADS + (TREE_MARCHED_RELOADS + 9) // 10, 91)


@pytest.fixture(scope='module')
def body(tmp_path_factory):
    """labels and instructions of the headline kernel; comments and directives dropped"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.fail('no hipcc at %s (set HIPCC)' % hipcc, pytrace=False)
    out = str(tmp_path_factory.mktemp('isa') / 'render_single.s')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-S', '--cuda-device-only',
           '-DNFI_SINGLE_KERNEL=0', '-DNFI_SINGLE_MODE=0', '-DNFI_RENDER_OCC=2', 'nfi_kernels.hip', '-o', out]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = open(out).read().splitlines()
    start = next(i for i, ln in enumerate(lines) if re.match(r'%s\w*:' % re.escape(KERNEL), ln))
    res = []
    for ln in lines[start + 1:]:
        s = ln.strip()
        if s.startswith('.end_amdhsa_kernel') or s.startswith('.section') or s.startswith('.Lfunc_end'):
            break
        s = s.split(';')[0].strip()
        if not s or (s.startswith('.') and not s.endswith(':')):
            continue
        res.append(s)
    assert any(s.startswith('s_endpgm') for s in res)
    return res


def regions(body):
    """(carriers, field loops, ray loop, end of the marched path, indices of the reloads)"""
    carriers = {re.match(r'v_writelane_b32\s+(v\d+)', s).group(1) for s in body if s.startswith('v_writelane_b32')}
    labels = {s[:-1]: i for i, s in enumerate(body) if s.endswith(':')}
    loops = []
    for i, s in enumerate(body):
        m = re.match(r's_c?branch\w*\s+(\S+)', s)
        if m and labels.get(m.group(1), i) < i:
            loops.append((labels[m.group(1)], i))
    mfma = [i for i, s in enumerate(body) if s.startswith('v_mfma')]

    def holds_mfma(a, b):
        return any(a <= i <= b for i in mfma)
    with_mfma = [r for r in loops if holds_mfma(*r)]
    field = sorted(r for r in with_mfma
                   if not any(o != r and r[0] <= o[0] and o[1] <= r[1] for o in with_mfma))
    assert len(field) == 2, field
    ray = max((r for r in loops if all(r[0] <= a and b <= r[1] for a, b in field)), key=lambda r: r[1] - r[0])
    hand_out = next(i for i in range(field[1][1], ray[1] + 1) if 'atomic' in body[i])
    reloads = []
    for i, s in enumerate(body):
        m = re.match(r'v_readlane_b32\s+s\d+,\s*(v\d+)', s)
        if m and m.group(1) in carriers:
            reloads.append(i)
    return carriers, field, ray, hand_out, reloads


def test_marched_path_reloads(body):
    carriers, field, ray, hand_out, reloads = regions(body)
    marched = [i for i in reloads if ray[0] <= i < hand_out]
    behind = [i for i in reloads if hand_out <= i <= ray[1]]
    in_field = [i for i in reloads if any(a <= i <= b for a, b in field)]
    spilled = sum(s.startswith('v_writelane_b32') for s in body)
    print('carriers %s, v_writelane %d; ray loop %s, field loops %s, hand-out at %d' % (sorted(carriers), spilled, ray, field, hand_out))
    print('reloads: marched path %d (parent %d), hand-out / miss-run code %d, field loops %d, whole kernel %d'
          % (len(marched), PARENT_MARCHED_RELOADS, len(behind), len(in_field), len(reloads)))
    assert hand_out - ray[0] > 3000          # the marched path is there: two field loops of ~620 and the stages between them
    assert len(in_field) == 0
    assert len(marched) <= LIMIT, (len(marched), LIMIT)


def test_no_waterfall_loops(body):
    # a value the compiler takes for divergent on its way to a scalar operand (a buffer descriptor, a scalar load's
    # address) is walked lane group by lane group: v_readfirstlane in a loop.  None before, none now: the count is the
    # parent's
    n = sum(s.startswith('v_readfirstlane') for s in body)
    print('v_readfirstlane %d (parent %d)' % (n, PARENT_READFIRSTLANE))
    assert n <= PARENT_READFIRSTLANE
