"""CPU tests of the measurement tooling: tools/phase_split.py on a synthetic kernel trace (the renderer / producer / other
split of profiles/r6/e2e is only as good as this parser), tools/isa_diff.py on synthetic device assembly, and the limits
DESIGN.md is held to."""
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trace(path, steps):
    """A kernel trace in rocprofv3's CSV form: per step  marker, zero_grad fill, raygen (own), model_begin, conv, synth_end,
    planes_to_texels (own, inside Generator.forward), model_end, render (own), render_end, loss, loss_bwd_end x2,
    field backward (own), producer_bwd_begin, conv backward, bwd_end, Adam."""
    t = [1000]
    rows = []

    def k(name, dur):
        rows.append({'Kind': 'KERNEL_DISPATCH', 'Kernel_Name': name, 'Start_Timestamp': t[0], 'End_Timestamp': t[0] + dur})
        t[0] += dur + 50
    mk = {'step_begin': 'erfinv_kernel_vectorized4_kernel', 'model_begin': 'digamma_vectorized4_kernel',
          'synth_end': 'lgamma_kernel_vectorized4_kernel', 'model_end': 'erfc_kernel_vectorized4_kernel',
          'render_end': 'sinc_vectorized4_kernel',
          'loss_bwd_end': 'void at::native::vectorized_elementwise_kernel<4, at::native::frac_kernel_cuda(at::TensorIteratorBase&)::{lambda()#1}>',
          'producer_bwd_begin': 'void at::native::vectorized_elementwise_kernel<4, at::native::asinh_kernel_cuda(at::TensorIteratorBase&)>',
          'bwd_end': 'void at::native::vectorized_elementwise_kernel<4, at::native::atanh_kernel_cuda(at::TensorIteratorBase&)>'}
    for _ in range(steps):
        k(mk['step_begin'], 10)
        k('raygen_kernel(nfi::CameraParams, int, RaygenOut)', 100_000)
        k(mk['model_begin'], 10)
        k('miopenSp3AsmConv_v30_3_1_gfx9_fp32_f2x3_stride1', 3_000_000)
        k(mk['synth_end'], 10)
        k('void planes_to_texels_kernel<0>(float const*, void*, int)', 200_000)
        k(mk['model_end'], 10)
        k('void render_fwd_kernel<0, true, 2, 1, 1, false>(RenderKernelParams)', 700_000)
        k(mk['render_end'], 10)
        k('void at::native::reduce_kernel<512, 1, at::native::ReduceOp<float, at::native::MeanOps<float> > >', 40_000)
        k(mk['loss_bwd_end'], 10)
        k(mk['loss_bwd_end'], 10)                      # (rgb and mask both carry the boundary: the first one counts)
        k('void field_query_bwd_kernel<true, false, false, 0>(FieldBwdParams)', 1_700_000)
        k(mk['producer_bwd_begin'], 10)
        k('igemm_wrw_gtcx35_nhwc_fp32_bx0_ex1', 5_000_000)
        k(mk['bwd_end'], 10)
        k('void at::native::(anonymous namespace)::multi_tensor_apply_kernel<FusedAdamMathFunctor<float> >', 600_000)
    with open(path, 'w', newline='') as f:
        w = csv.DictWriter(f, fieldnames=['Kind', 'Kernel_Name', 'Start_Timestamp', 'End_Timestamp'], quoting=csv.QUOTE_ALL)
        w.writeheader()
        w.writerows(rows)


def test_phase_split_on_a_synthetic_trace(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import end_to_end                      # (module level imports torch only; the marker table is what is needed)
    _trace(str(tmp_path / 't_kernel_trace.csv'), steps=5)
    sidecar = {'markers': end_to_end.MARKER_OPS, 'iters': 3, 'warmup': 2, 'result': {'leg': 'gstep', 'impl': 'hip', 'ms_median': 11.5}}
    json.dump(sidecar, open(tmp_path / 'side.json', 'w'))
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'phase_split.py'), str(tmp_path), str(tmp_path / 'side.json')],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout)
    g = d['group_ms_per_step']
    # renderer: raygen 0.1 + planes_to_texels 0.2 (own kernel inside Generator.forward) + render 0.7 + field backward 1.7
    assert abs(g['renderer'] - 2.7) < 1e-6, g
    assert abs(g['producer'] - 8.0) < 1e-6, g               # conv 3.0 + weight-gradient conv 5.0
    assert abs(g['other'] - 0.64) < 1e-6, g                 # loss 0.04 + Adam 0.6
    assert g['forward_rest'] == 0.0
    assert abs(d['libnfi_kernels_ms_per_step'] - 2.7) < 1e-6 and d['steps'] == 3
    assert abs(sum(d['group_share_of_gpu_time'].values()) - 1.0) < 1e-9


def _asm(kernels, first=0):
    """Device assembly in the compiler's form: per (name, operand) one kernel with a branch label, a .Ltmp, a comment, its
    descriptor block and .Lfunc_end; the label counters start at `first`, as they would further down a larger file."""
    out = ['\t.text', '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"']
    for i, (name, operand) in enumerate(kernels, first):
        out += ['\t.protected\t%s ; -- Begin function %s' % (name, name), '\t.globl\t%s' % name, '\t.p2align\t8',
                '\t.type\t%s,@function' % name, '%s:   ; @%s' % (name, name), '; %%bb.0:',
                '\ts_load_dwordx2 s[0:1], s[0:1], 0x0', '.Ltmp%d:' % (7 * i), '\tv_mov_b32_e32 v1, %s' % operand,
                '\ts_cbranch_execz .LBB%d_2' % i, '.LBB%d_2:        ;   in Loop: Header=BB%d_1 Depth=1' % (i, i), '\ts_endpgm',
                '\t.section\t.rodata,"a",@progbits', '\t.amdhsa_kernel %s' % name, '\t\t.amdhsa_next_free_vgpr 10',
                '\t.end_amdhsa_kernel', '\t.text', '.Lfunc_end%d:' % i,
                '\t.size\t%s, .Lfunc_end%d-%s' % (name, i, name), '; codeLenInByte = %d' % (512 + i)]
    return '\n'.join(out) + '\n'


def test_isa_diff_compares_kernels_by_name_whatever_their_place(tmp_path):
    """tools/isa_diff.py: label renumbering and comments are no difference; a changed operand, a changed descriptor and a
    kernel on one side only are each reported by name, with exit status 1."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import isa_diff
    a, b, c = ('_Z1aPf', '0x3e000000'), ('_Z1bPf', 'v7'), ('_Z1cPf', 'v9')
    old = isa_diff.functions(_asm([a, b, c]))
    assert sorted(old) == ['_Z1aPf', '_Z1bPf', '_Z1cPf'] and all(kernel for _, kernel in old.values())
    assert ';' not in old['_Z1bPf'][0] and '.amdhsa_next_free_vgpr 10' in old['_Z1bPf'][0]
    # the same kernels in another order and from another place in their file, an extra comment line: nothing to report
    moved = isa_diff.functions(_asm([c, a, b], first=40).replace('\ts_endpgm', '; a remark\n\ts_endpgm'))
    assert isa_diff.diff(old, moved) == []
    assert isa_diff.diff(old, isa_diff.functions(_asm([a, ('_Z1bPf', 'v8'), c]))) == ['differs: _Z1bPf']
    assert isa_diff.diff(old, isa_diff.functions(_asm([a, b, c]).replace('vgpr 10', 'vgpr 12', 1))) == ['differs: _Z1aPf']
    assert isa_diff.diff(old, isa_diff.functions(_asm([a, b]))) == ['missing (old side only): _Z1cPf']
    assert isa_diff.diff(isa_diff.functions(_asm([a, b])), old) == ['extra (new side only): _Z1cPf']
    # the command line: two files against one, counts printed, exit status
    for name, text in (('ab.s', _asm([a, b])), ('c.s', _asm([c])), ('all.s', _asm([c, b, a], first=3)), ('short.s', _asm([a, b]))):
        (tmp_path / name).write_text(text)
    run = lambda *args: subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'isa_diff.py')] + [str(tmp_path / x) if x != '--' else x for x in args],
                                       capture_output=True, text=True, timeout=60)
    p = run('ab.s', 'c.s', '--', 'all.s')
    assert p.returncode == 0 and p.stdout.splitlines()[:2] == ['old: 3 kernels, 3 functions in all', 'new: 3 kernels, 3 functions in all'], p.stdout + p.stderr
    p = run('ab.s', 'c.s', '--', 'short.s')
    assert p.returncode == 1 and 'missing (old side only): _Z1cPf' in p.stdout and 'new: 2 kernels' in p.stdout, p.stdout + p.stderr


def test_design_md_stays_a_current_state_document():
    """The review of round 5 asked for DESIGN.md <= 400 lines of <= 120 columns (history lives in HISTORY.md)."""
    lines = open(os.path.join(ROOT, 'DESIGN.md')).read().split('\n')
    assert len(lines) <= 400, len(lines)
    too_long = [(i + 1, len(l)) for i, l in enumerate(lines) if len(l) > 120]
    assert not too_long, too_long[:5]
    assert os.path.exists(os.path.join(ROOT, 'HISTORY.md'))


def test_bench_dump_outputs_writes_float32_and_samples_whole_images_above_the_cap(tmp_path, monkeypatch):
    """bench.py --dump-outputs: one float32 .npy per returned array; above the byte cap the same seeded sample of whole
    images from every array, the same sample every time."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(5)
    out = {'rgb': torch.rand(6, 4, 4, 3, generator=g), 'depth': torch.rand(6, 4, 4, generator=g),
           'mask': torch.rand(6, 4, 4, generator=g)}
    info = bench.dump_outputs(out, str(tmp_path / 'all'))
    assert info['images'] == 'all' and info['arrays']['rgb'] == [6, 4, 4, 3]
    for k in ('rgb', 'depth', 'mask'):
        a = np.load(str(tmp_path / 'all' / (k + '.npy')))
        assert a.dtype == np.float32 and np.array_equal(a, out[k].numpy())
    monkeypatch.setattr(bench, 'DUMP_BYTES_MAX', 3 * 4 * 4 * 5 * 4)          # room for three images
    a = bench.dump_outputs(out, str(tmp_path / 'a'))
    b = bench.dump_outputs(out, str(tmp_path / 'b'))
    assert len(a['images']) == 3 and a['images'] == sorted(a['images']) and a['images'] == b['images']
    assert sum(os.path.getsize(str(tmp_path / 'a' / (k + '.npy'))) - 128 for k in ('rgb', 'depth', 'mask')) <= bench.DUMP_BYTES_MAX
    for k in ('rgb', 'depth', 'mask'):
        assert np.array_equal(np.load(str(tmp_path / 'a' / (k + '.npy'))), out[k][a['images']].numpy())
