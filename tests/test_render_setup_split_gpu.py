"""GPU checks of the ray set-up without atomics or memset (raygen_kernel's per-block partials + raygen_finish_kernel) and of
the split-phase work hand-out, on the BASELINE cfg2 batch (8 x 128 x 128 rays, 64 + 64 samples, fp32 texels):

* render_setup + render_fwd(rays_ready=True) gives the image of the one-call render_fwd bit for bit - from a workspace
  whose every byte was set to 0xff first, so a header cell that the set-up left unwritten would show (the work counters
  would start beyond every queue's end and no ray would be rendered);
* the three reduction cells of the workspace equal what nfi_near_far (the atomic form, slab_kernel) computes for the same
  rays, and agree with ops.near_far's hit mask and miss-fill."""
import numpy as np
import pytest
import torch

from nerf_from_image_amd import _lib, ops
from stand_in import look_at_cameras
from test_hip_full_size import A, R, S, make_inputs

pytestmark = pytest.mark.gpu
HEADER_BYTES = 64 + 8 * 64


def _render(d, **kw):
    texels = ops.planes_to_texels(d['planes'].contiguous())
    image = ops.decoder_pack(d['w1'], d['b1'], d['w2'], d['b2'], A)
    return ops.render_fwd(d['cam'].contiguous(), d['focal'].contiguous(), R, R, S, texels, image, 0.55, A, d['att'].contiguous(),
                          True, d['beta'], d['alpha'], noise_coarse=d['noise_c'].contiguous(), noise_fine=d['noise_f'],
                          white_background=True, skip_missed_rays=True, **kw)


def _dirty_workspace(n, dev):
    return torch.full((_lib.load().nfi_render_workspace_bytes(n),), 0xff, dtype=torch.uint8, device=dev)


def test_two_call_render_equals_one_call_render(gpu_device):
    d = make_inputs(8, gpu_device)
    n = 8 * R * R
    one = _render(d, workspace=_dirty_workspace(n, gpu_device))
    ws = ops.render_setup(d['cam'].contiguous(), d['focal'].contiguous(), R, R, 0.55, workspace=_dirty_workspace(n, gpu_device))
    head = ws[:HEADER_BYTES].view(torch.int32).cpu()
    assert int(head[2]) > 0                                          # rays hit the cube
    assert not head[3:].any(), 'the work counters (and the padding) are zero after the set-up'
    two = _render(d, workspace=ws, rays_ready=True)
    assert float(one['mask'].mean()) > 0.05, 'scene should not be empty'
    for k in ('rgb', 'depth', 'mask'):
        assert torch.equal(one[k], two[k]), k
    # the one-call path left the same reduction cells behind
    assert torch.equal(one['_workspace'][:12].cpu(), ws[:12].cpu())


@pytest.mark.parametrize('B', [1, 8, 20])        # 20 x 128 x 128 = 327 680 rays: beyond one thread per ray (grid-stride loop)
def test_reduction_cells_equal_near_far(gpu_device, B):
    g = torch.Generator().manual_seed(1234)
    d = dict(cam=look_at_cameras(B, 2.0, g).to(gpu_device), focal=torch.full((B,), 1.0254, device=gpu_device))
    n = B * R * R
    ws = ops.render_setup(d['cam'].contiguous(), d['focal'].contiguous(), R, R, 0.55, workspace=_dirty_workspace(n, gpu_device))
    cells = ws[:12].view(torch.int32).cpu().numpy().view(np.uint32)
    rays = ws[HEADER_BYTES:HEADER_BYTES + 24 * n].view(torch.float32)
    ro, rd = rays[:3 * n].view(n, 3).clone(), rays[3 * n:].view(n, 3).clone()
    # the atomic form on the same rays
    near_raw, far_raw = torch.empty(n, device=gpu_device), torch.empty(n, device=gpu_device)
    hit = torch.empty(n, dtype=torch.uint8, device=gpu_device)
    red = torch.empty(4, dtype=torch.int32, device=gpu_device)
    with torch.cuda.device(gpu_device):
        _lib.call_struct('nfi_near_far', 'nfi_near_far_args', ops._stream(ro), n_rays=n, ray_origins=ro, ray_directions=rd,
                         scene_range=0.55, near_raw=near_raw, far_raw=far_raw, hit=hit, reduce=red)
    ref = red[:3].cpu().numpy().view(np.uint32)
    print('B = %d: cells %s, nfi_near_far %s' % (B, cells.tolist(), ref.tolist()))
    assert cells.tolist() == ref.tolist()
    # and ops.near_far: the hit count, and the miss-fill (min near / max far over the rays that hit) in the finished planes
    near, far, hit_mask = ops.near_far(ro, rd, 0.55)
    assert int(cells[2]) == int(hit_mask.sum())
    assert 0 < int(cells[2]) < n

    def key_inv(k):
        k = int(k)
        b = (k ^ 0x80000000) if (k >> 31) else (~k & 0xffffffff)
        return float(np.array([b], dtype=np.uint32).view(np.float32)[0])
    fill_near, fill_far = key_inv(~int(cells[0]) & 0xffffffff), key_inv(cells[1])
    assert fill_near == float(near_raw[hit_mask].min()) and fill_far == float(far_raw[hit_mask].max())
    miss = ~hit_mask
    assert torch.all(near[miss] == max(fill_near, 0.1))
