"""GPU checks of the block table of the render kernels' per-XCD queues.

The ray set-up (raygen_finish_kernel) writes, behind the per-block partials of the render workspace, which pixel block
sits in which queue slot: every complete aligned group of 16 slots is a permutation of itself that gives each XCD a heavy
and a light block by the number of rays whose hit byte has bit 1 set; everything else is the identity.  The render
kernels read it (RayQueue::block_at) unless tuning bit 5 (NFI_TUNING_XCD_BLOCKS_IN_ORDER) asks for today's order.

1. the table equals its definition, recomputed here from the hit bytes of the same workspace;
2. the images are the same with the table (tuning 0), in order (32) and from the single counter (16), and every pixel is
   written (the outputs start as NaN);
3. a table that no longer matches the hit bytes changes nothing;
4. on the benchmark's cameras the table balances the XCDs (max/mean <= 1.10 where the identity has >= 1.35).

Tolerances: none - tables are compared exactly, images with torch.equal."""
import pytest
import torch

import bench
from nerf_from_image_amd import _lib, ops
from stand_in import look_at_cameras
from test_hip_edge_cases import scene

pytestmark = pytest.mark.gpu
A = 10
PLANE_RES = 16
RANGE = 0.55
HIT_OFFSET = lambda n: 576 + 32 * n
TABLE_OFFSET = lambda n: 576 + 32 * n + ((n + 63) & ~63) + 16384      # behind 1024 partials of 16 bytes


class Shape:
    def __init__(self, name, B, H, W, radii, focal=1.0, views=1, row_window=None):
        self.name, self.B, self.H, self.W, self.radii, self.focal, self.views, self.row_window = name, B, H, W, radii, focal, views, row_window
        self.n = B * H * W
        both = H | W
        self.side = 32 if both % 32 == 0 else (16 if both % 16 == 0 else 8)
        self.n_blocks = self.n // (self.side * self.side)

    def __repr__(self):
        return self.name


# cameras near the cube (most blocks full: counts tie at side^2) and far from it (the corner blocks empty: counts tie at 0,
# the blocks at the silhouette differ)
SHAPES = [Shape('1x32x32', 1, 32, 32, [2.0]),                                   # 1 block
          Shape('1x64x64', 1, 64, 64, [2.0]),                                   # 4 blocks, fewer than 16: identity
          Shape('2x128x128', 2, 128, 128, [1.4, 3.0]),                          # two complete groups
          Shape('3x96x96', 3, 96, 96, [2.0, 3.0, 1.4]),                         # 27 blocks: one group + identity tail
          Shape('1x128x64', 1, 128, 64, [2.0]),                                 # not square
          Shape('2x48x48', 2, 48, 48, [2.0, 3.0]),                              # 16-pixel blocks, 18 of them
          Shape('2x40x40', 2, 40, 40, [1.4, 3.0]),                              # 8-pixel blocks, 50 of them
          Shape('4x64x64_views2', 4, 64, 64, [2.0, 3.0, 1.4, 2.0], views=2),    # 16 blocks over 4 images of 2 scenes
          Shape('4x32of128x128', 4, 32, 128, [2.0, 3.0, 1.4, 2.0], row_window=(48, 128)),   # a row window: 16 blocks
          Shape('1x128x128_all_hit', 1, 128, 128, [0.9], focal=4.0)]            # every count ties
BY_NAME = {s.name: s for s in SHAPES}


def cameras_of(shape, dev):
    g = torch.Generator().manual_seed(17 + shape.n)
    cam = look_at_cameras(shape.B, 1.0, g)
    cam[:, :3, 3] *= torch.tensor(shape.radii).view(-1, 1)
    return cam.to(dev), torch.full((shape.B,), shape.focal, device=dev)


def dirty_workspace(n, dev):
    return torch.full((_lib.load().nfi_render_workspace_bytes(n),), 0xff, dtype=torch.uint8, device=dev)


def setup(shape, dev):
    cam, focal = cameras_of(shape, dev)
    ws = ops.render_setup(cam, focal, shape.H, shape.W, RANGE, workspace=dirty_workspace(shape.n, dev), row_window=shape.row_window)
    return cam, focal, ws


def wide_hit_counts(ws, shape):
    """int64 [n_blocks] on the CPU: rays with hit bit 1 per pixel block, blocks image-major and row-major"""
    s = shape.side
    hit = ws[HIT_OFFSET(shape.n):HIT_OFFSET(shape.n) + shape.n].cpu()
    wide = ((hit & 2) != 0).view(shape.B, shape.H // s, s, shape.W // s, s)
    return wide.sum(dim=(2, 4)).reshape(-1).to(torch.int64)


def table_of(ws, shape):
    off = TABLE_OFFSET(shape.n)
    return ws[off:off + 4 * shape.n_blocks].view(torch.int32).cpu().to(torch.int64)


def table_by_rule(counts):
    n = counts.numel()
    table = torch.arange(n)
    for G in range(n // 16):
        order = torch.argsort(-counts[16 * G:16 * G + 16], stable=True)       # count descending, index ascending
        for r in range(16):
            x = (min(r, 15 - r) + G) % 8
            table[16 * G + (0 if r < 8 else 8) + x] = 16 * G + int(order[r])
    return table


def xcd_sums(counts, table):
    return [int(counts[table[q::8]].sum()) for q in range(8)]


# ---- 1. the table against its definition --------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=repr)
def test_table_is_its_definition(gpu_device, shape):
    _, _, ws = setup(shape, gpu_device)
    counts, got = wide_hit_counts(ws, shape), table_of(ws, shape)
    want = table_by_rule(counts)
    print(shape, 'counts', counts.tolist(), 'table', got.tolist())
    assert torch.equal(got, want)
    groups = shape.n_blocks // 16
    for G in range(groups):
        assert sorted(got[16 * G:16 * G + 16].tolist()) == list(range(16 * G, 16 * G + 16))
    assert got[16 * groups:].tolist() == list(range(16 * groups, shape.n_blocks))
    if shape.name == '2x128x128':         # the cameras do what the comment at SHAPES says: counts that tie and counts that differ
        c = counts[16:32]
        assert int((c == 0).sum()) >= 2 and c.unique().numel() >= 4 and int((counts[:16] == 1024).sum()) >= 2
    if shape.name == '1x128x128_all_hit':
        assert bool((counts == 1024).all())
        assert got.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 15, 14, 13, 12, 11, 10, 9, 8]     # the index-order pairing


# ---- 2. the images are the same, every pixel is written -----------------------------------------------------------------
_fields = {}


def field_of(n_scenes, dev):
    if n_scenes not in _fields:
        d, _ = scene(n_scenes, A, PLANE_RES, 900 + n_scenes)
        mv = lambda t: t.to(dev)
        _fields[n_scenes] = dict(texels=ops.planes_to_texels(mv(d['planes'])), att=mv(d['att']), beta=mv(d['beta']), alpha=mv(d['alpha']),
                                 image=ops.decoder_pack(mv(d['w1']), mv(d['b1']), mv(d['w2']), mv(d['b2']), A))
    return _fields[n_scenes]


def nan_empty(real_empty):
    """torch.empty whose float tensors start as NaN and byte tensors as 0xff: render_fwd allocates its outputs (and the
    workspace) with torch.empty, and a pixel nobody writes must show"""
    def empty(*a, **kw):
        t = real_empty(*a, **kw)
        if t.dtype == torch.float32:
            t.fill_(float('nan'))
        elif t.dtype == torch.uint8:
            t.fill_(0xff)
        return t
    return empty


def render(shape, dev, S, fine, tuning, monkeypatch, workspace=None, rays_ready=False):
    f = field_of(shape.B // shape.views, dev)
    cam, focal = cameras_of(shape, dev)
    g = torch.Generator().manual_seed(5)
    noise_c = torch.rand(shape.B, shape.H, shape.W, S, generator=g).to(dev)
    noise_f = torch.rand(shape.n, S, generator=g).to(dev) if fine else None
    with monkeypatch.context() as m:
        m.setattr(torch, 'empty', nan_empty(torch.empty))
        out = ops.render_fwd(cam, focal, shape.H, shape.W, S, f['texels'], f['image'], RANGE, A, f['att'], True, f['beta'], f['alpha'],
                             noise_coarse=noise_c, noise_fine=noise_f, fine_sampling=fine, white_background=True,
                             skip_missed_rays=True, tuning=tuning, views_per_scene=shape.views, row_window=shape.row_window,
                             workspace=workspace, rays_ready=rays_ready)
    torch.cuda.synchronize(dev)
    return out


def same_images(shape, dev, S, fine, monkeypatch):
    ref = render(shape, dev, S, fine, 16, monkeypatch)          # the single counter: no blocks, no table
    assert float(ref['mask'].max()) > 0.1, 'scene should not be empty'
    for k in ('rgb', 'depth', 'mask'):
        assert not bool(torch.isnan(ref[k]).any()), k
    for tuning in (0, 32):
        out = render(shape, dev, S, fine, tuning, monkeypatch)
        for k in ('rgb', 'depth', 'mask'):
            assert torch.equal(out[k], ref[k]), (shape, tuning, k)      # (NaN != NaN: an unwritten pixel fails here too)


@pytest.mark.parametrize('shape', SHAPES, ids=repr)
def test_images_unchanged(gpu_device, shape, monkeypatch):
    same_images(shape, gpu_device, 8, True, monkeypatch)


def test_images_unchanged_wide_kernel(gpu_device, monkeypatch):
    """render_fwd_wide_kernel, 96 + 96 samples, on 18 blocks of 16 pixels (one complete group and a tail)"""
    same_images(BY_NAME['2x48x48'], gpu_device, 96, True, monkeypatch)


def test_images_unchanged_long_kernel(gpu_device, monkeypatch):
    """render_fwd_long_kernel, one pass of 256 samples"""
    same_images(BY_NAME['2x48x48'], gpu_device, 256, False, monkeypatch)


# ---- 3. a stale table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pattern', ['block', 'checkerboard', 'everything'])
def test_stale_table(gpu_device, pattern, monkeypatch):
    """bit 1 of chosen hit bytes cleared between the set-up and the render: the table's counts are no longer the kernel's"""
    shape, dev = BY_NAME['2x128x128'], gpu_device
    _, _, ws = setup(shape, dev)
    y, x = torch.meshgrid(torch.arange(shape.H), torch.arange(shape.W), indexing='ij')
    cleared = torch.zeros(shape.B, shape.H, shape.W, dtype=torch.bool)
    if pattern == 'block':
        cleared[0, 32:64, 32:64] = True                     # a whole block at the centre of the near image
    elif pattern == 'checkerboard':
        cleared[:] = (((x >> 3) + (y >> 3)) & 1) == 1      # every second 8x8 sub-tile
    else:
        cleared[:] = True
    hit = ws[HIT_OFFSET(shape.n):HIT_OFFSET(shape.n) + shape.n]
    assert int(((hit.cpu() & 2) != 0).view_as(cleared)[cleared].sum()) > 0, 'the pattern clears bits that were set'
    hit[cleared.reshape(-1).to(dev)] &= 0xfd
    ref = render(shape, dev, 8, True, 16, monkeypatch, workspace=ws.clone(), rays_ready=True)
    out = render(shape, dev, 8, True, 0, monkeypatch, workspace=ws.clone(), rays_ready=True)
    c = cleared.to(dev)
    for k, bg in (('rgb', 1.0), ('depth', 0.0), ('mask', 0.0)):
        assert torch.equal(out[k], ref[k]), (pattern, k)
        assert bool((out[k][c] == bg).all()), (pattern, k)


# ---- 4. balance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_balance_on_bench_cameras(gpu_device, seed):
    """8 x 128 x 128 from the benchmark's camera distribution: marched rays per XCD through the table, max / mean.  On the
    CPU the rule gives 1.040 / 1.016 / 1.012 and the identity 1.45 / 1.40 / 1.42 (tools/xcd_balance.py)."""
    shape, dev = Shape('bench', 8, 128, 128, None), gpu_device
    cam = bench.cameras(8, 2.0, torch.Generator().manual_seed(seed)).to(dev)
    focal = torch.full((8,), bench.FOCAL, device=dev)
    ws = ops.render_setup(cam, focal, 128, 128, bench.SCENE_RANGE, workspace=dirty_workspace(shape.n, dev))
    counts, table = wide_hit_counts(ws, shape), table_of(ws, shape)
    assert sorted(table.tolist()) == list(range(shape.n_blocks))
    spread = lambda sums: max(sums) / (sum(sums) / 8.0)
    paired, in_order = xcd_sums(counts, table), xcd_sums(counts, torch.arange(shape.n_blocks))
    print('seed %d: paired %s %.3f, in order %s %.3f' % (seed, paired, spread(paired), in_order, spread(in_order)))
    assert spread(paired) <= 1.10
    assert spread(in_order) >= 1.35
