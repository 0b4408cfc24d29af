"""CPU test on the ISA of the field loops of the headline render kernel render_fwd_kernel<0,true,2,0,1,false>: the dependent
LDS round trips of one turn (two tiles: gather half, decoder half).  The single-kernel compile of
tests/test_render_isa_stalls.py (~20 s) is read as text.

Definitions (all textual, on the listing):
  field loops   the innermost backward-branch regions that hold MFMAs (coarse and fine pass: two), as in
                tests/test_render_scalar_reloads.py
  tight wait    an s_waitcnt on lgkmcnt that has to wait for a ds_read / ds_bpermute issued fewer than D = 8 instructions
                earlier.  LDS operations of a wave return in issue order, so lgkmcnt(N) leaves the N youngest LDS
                operations outstanding and waits for the rest: the wait is tight when the youngest operation it does
                wait for is such a read.  (Counting every wait behind a recent read, whether or not it waits for it,
                calls the waits of a read-ahead schedule tight too - `s_waitcnt lgkmcnt(3)` right behind the two reads of
                the NEXT group waits for reads issued a whole MFMA group earlier - and cannot tell the schedules apart:
                15 in the parent, 14 in the tree.)  The loop is read in program order, the unpaired last turn's
                branch included.

The parent of round 21 (profiles/r21), same toolchain, same definitions: 13 tight waits in the coarse loop and 14 in the
fine loop - per tile the permutes of the gather operands (2) and, behind the second tile, the transpose (1); in the
decoder the first wait in front of the first MFMA and one or two per operand group of layer 1 (6), three in layer 2.
The tree fetches both tiles' gather operands in front of one wait, sends tile a's features through the transpose under
tile b's loads, and reads every decoder operand one MFMA group ahead (the first group together with the last transpose
read): no tight wait is left in either loop.  The bound is a third of the parent's count."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nerf_from_image_amd', 'csrc')
KERNEL = '_Z17render_fwd_kernelILi0ELb1ELi2ELi0ELi1ELb0EEv18RenderKernelParams'
D = 8
PARENT_TIGHT = 13          # the smaller of the parent's two loops (13 and 14)
PARENT_VALU = 387
LIMIT = PARENT_TIGHT // 3


@pytest.fixture(scope='module')
def loops(tmp_path_factory):
    """the instructions of the two field loops of the headline kernel (labels, comments and directives dropped)"""
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
    body = []
    for ln in lines[start + 1:]:
        s = ln.strip()
        if s.startswith('.end_amdhsa_kernel') or s.startswith('.section') or s.startswith('.Lfunc_end'):
            break
        s = s.split(';')[0].strip()
        if not s or (s.startswith('.') and not s.endswith(':')):
            continue
        body.append(s)
    assert any(s.startswith('s_endpgm') for s in body)
    labels = {s[:-1]: i for i, s in enumerate(body) if s.endswith(':')}
    back = []
    for i, s in enumerate(body):
        m = re.match(r's_c?branch\w*\s+(\S+)', s)
        if m and labels.get(m.group(1), i) < i:
            back.append((labels[m.group(1)], i))
    mfma = [i for i, s in enumerate(body) if s.startswith('v_mfma')]
    with_mfma = [r for r in back if any(r[0] <= i <= r[1] for i in mfma)]
    field = sorted(r for r in with_mfma if not any(o != r and r[0] <= o[0] and o[1] <= r[1] for o in with_mfma))
    assert len(field) == 2, field
    return [[s for s in body[a:b + 1] if not s.endswith(':')] for a, b in field]


def tight_waits(ins):
    """indices of the tight waits of an instruction list (see the module's docstring)"""
    outstanding = []          # (index, is a read) of the LDS operations not yet waited for, oldest first
    tight = []
    for i, s in enumerate(ins):
        if s.startswith('ds_'):
            outstanding.append((i, s.startswith('ds_read') or s.startswith('ds_bpermute')))
        m = re.match(r's_waitcnt\b.*lgkmcnt\((\d+)\)', s)
        if m:
            keep = int(m.group(1))
            waited = outstanding[:max(len(outstanding) - keep, 0)]
            outstanding = outstanding[len(waited):]
            reads = [k for k, is_read in waited if is_read]
            if reads and i - reads[-1] < D:
                tight.append(i)
    return tight


def count(ins, pattern):
    return sum(bool(re.match(pattern, s)) for s in ins)


def test_tight_waits_of_a_turn(loops):
    for name, ins in zip(('coarse', 'fine'), loops):
        tight = tight_waits(ins)
        print('%s field loop: %d instructions, tight waits at %s (parent: %d)' % (name, len(ins), tight, PARENT_TIGHT))
        assert len(tight) <= LIMIT, (name, [(i, ins[max(i - 3, 0):i + 1]) for i in tight])


def test_decoder_half_opens_on_mfmas(loops):
    for name, ins in zip(('coarse', 'fine'), loops):
        first = next(i for i, s in enumerate(ins) if s.startswith('v_mfma'))
        waits = [i for i in range(first) if re.match(r's_waitcnt\b.*lgkmcnt', ins[i])]
        tight = tight_waits(ins)
        print('%s field loop: first MFMA at %d, the wait in front of it at %d: %s' % (name, first, waits[-1], ins[waits[-1]]))
        assert waits[-1] not in tight, (name, ins[waits[-1] - 4:first + 1])
        # ... and nothing is read between the head of the half (s_setprio 0) and that MFMA but the NEXT group's three
        # fragments (bias, W1' hi, W1' lo)
        head = max(i for i in range(first) if ins[i].startswith('s_setprio'))
        assert count(ins[head:first], r'ds_read') <= 3, (name, ins[head:first])


def test_the_turn_keeps_its_work(loops):
    for name, ins in zip(('coarse', 'fine'), loops):
        c = dict(loads=count(ins, r'buffer_load_dwordx4'), mfma=count(ins, r'v_mfma'), valu=count(ins, r'v_(?!mfma)'),
                 permutes=count(ins, r'ds_bpermute_b32'), reads=count(ins, r'ds_read_b128'))
        print('%s field loop: %s' % (name, c))
        assert c['loads'] == 48 and c['mfma'] == 36
        assert c['valu'] <= PARENT_VALU + 8
        assert c['permutes'] == 8
