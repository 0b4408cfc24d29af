"""CPU tests of the measurement tooling: tools/phase_split.py on a synthetic kernel trace (the renderer / producer / other
split of profiles/r6/e2e is only as good as this parser), and the limits DESIGN.md is held to."""
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
