"""nerf_from_image_amd.pose_utils against the reference's lib/pose_utils.py (the staged copy, PyTorch-ROCm) on the same GPU:
    python tools/bench_pose.py [--iters 50] [--out profiles/rNN/pose_utils.json]
For B = 1, 4, 16, perspective and orthographic, per leg and contender the number of device launches of ONE call (kernels,
copies and memsets the profiler sees on the device) and the median wall time (host clock, synchronised at the end) and GPU
time (HIP events on the stream around the call: in a launch-bound leg mostly the gaps between the launches):
  (a) step:    normalise + pose_to_matrix + backward of a random cotangent + the fix-ups after the optimiser step
               (run.py:2257-2262, 2299, 2307-2310); here: pose_to_matrix(normalize=True), its backward, project_pose_
  (b) inverse: matrix_to_pose (run.py:1986); the reference copies to the host and loops in numpy
  (c) perturb: perturb_poses at N = 2048 with two extra arguments (run.py:162,171), once per contender and branch
The two contenders alternate inside one process.  The reference's numpy loop is written for numpy 1 (np.array(copy=False));
under numpy 2 it gets that call's old meaning back, nothing else is changed."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402
from nerf_from_image_amd import pose_utils as ours  # noqa: E402
from oracle import reference  # noqa: E402


class NumpyOneCopyRule:
    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, dtype=None, copy=True):
        return np.array(obj, dtype=dtype) if copy else np.asarray(obj, dtype=dtype)


def device_launches(fn):
    """(count, {name: count}, summed device time in ms) of the device-side events of one call of fn."""
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names, busy = {}, 0.0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            name = e.name if len(e.name) <= 96 else e.name[:93] + '...'
            names[name] = names.get(name, 0) + 1
            busy += e.time_range.elapsed_us() / 1e3
    return sum(names.values()), names, busy


def timed(fns, n, warm=3):
    """Per fn, called in turn: (median wall ms, median GPU ms)."""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    wall, gpu = [[] for _ in fns], [[] for _ in fns]
    for _ in range(n):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            wall[i].append((time.perf_counter() - t0) * 1e3)
            gpu[i].append(a.elapsed_time(b))
    return [(sorted(w)[n // 2], sorted(g)[n // 2]) for w, g in zip(wall, gpu)]


def leg(name, fns, n):
    out = {}
    times = timed([fns['hip'], fns['reference']], n)
    for (who, f), (wall, gpu) in zip(fns.items(), times):
        count, names, busy = device_launches(f)
        out[who] = dict(launches=count, wall_ms=round(wall, 4), gpu_ms=round(gpu, 4), device_busy_ms=round(busy, 4), launches_by_name=names)
    print('%-28s HIP %3d launches %8.3f ms wall %8.3f ms GPU | reference %5d launches %8.3f ms wall %8.3f ms GPU' % (
        name, out['hip']['launches'], out['hip']['wall_ms'], out['hip']['gpu_ms'], out['reference']['launches'],
        out['reference']['wall_ms'], out['reference']['gpu_ms']))
    return out


def parameters(b, persp, g, dev):
    q = torch.randn(b, 4, generator=g)
    t2, s = torch.rand(b, 2, generator=g) - 0.5, 0.5 + 1.5 * torch.rand(b, generator=g)
    z0 = torch.rand(b, generator=g) * 2 - 1 if persp else None
    return [None if t is None else t.to(dev).requires_grad_() for t in (z0, t2, s, q)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    ref = reference.modules().pose_utils
    ref.np = NumpyOneCopyRule()
    g = torch.Generator().manual_seed(0)
    flipped = True
    result = {'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'iters': a.iters, 'legs': {}}
    for persp in (True, False):
        branch = 'perspective' if persp else 'orthographic'
        for b in (1, 4, 16):
            z0, t2, s, q = parameters(b, persp, g, dev)
            leaves = [t for t in (z0, t2, s, q) if t is not None]
            g_mat, g_focal = torch.randn(b, 4, 4, generator=g).to(dev), torch.randn(b, generator=g).to(dev)

            def step_hip():
                mat, focal = ours.pose_to_matrix(z0, t2, s, q, flipped, normalize=True)
                grads = torch.autograd.grad([mat] + ([focal] if persp else []), leaves, [g_mat] + ([g_focal] if persp else []))
                ours.project_pose_(q, s, z0)
                return grads

            def step_reference():
                mat, focal = ref.pose_to_matrix(z0, t2, s, F.normalize(q, dim=-1), flipped)
                grads = torch.autograd.grad([mat] + ([focal] if persp else []), leaves, [g_mat] + ([g_focal] if persp else []))
                q.data[:] = F.normalize(q.data, dim=-1)
                if z0 is not None:
                    z0.data.clamp_(-4, 4)
                s.data.abs_()
                return grads
            result['legs']['step %s B=%d' % (branch, b)] = leg('step %s B=%d' % (branch, b), {'hip': step_hip, 'reference': step_reference}, a.iters)
            with torch.no_grad():
                cam, focal = ours.pose_to_matrix(z0, t2, s, q, flipped, normalize=True)
            result['legs']['inverse %s B=%d' % (branch, b)] = leg(
                'inverse %s B=%d' % (branch, b), {'hip': lambda: ours.matrix_to_pose(cam, focal, flipped),
                                                  'reference': lambda: ref.matrix_to_pose(cam, focal, flipped)}, a.iters)
        n = 2048
        z0, t2, s, q = parameters(n, persp, g, dev)
        with torch.no_grad():
            cams, focals = ours.pose_to_matrix(z0, t2, s, q, flipped, normalize=True)
        bbox = torch.rand(n, 4, generator=g).to(dev)
        fns = {'hip': lambda: ours.perturb_poses(cams, 15.0, focals, bbox), 'reference': lambda: ref.perturb_poses(cams, 15.0, focals, bbox)}
        result['legs']['perturb %s N=%d' % (branch, n)] = leg('perturb %s N=%d' % (branch, n), fns, 3)
        mine, theirs = fns['hip'](), fns['reference']()
        result['legs']['perturb %s N=%d' % (branch, n)]['poses_chosen_differently'] = int((mine[0] != theirs[0]).flatten(1).any(1).sum())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)
    print(json.dumps({k: {w: {m: v[w][m] for m in ('launches', 'wall_ms', 'gpu_ms')} for w in ('hip', 'reference')} for k, v in result['legs'].items()}))


if __name__ == '__main__':
    main()
