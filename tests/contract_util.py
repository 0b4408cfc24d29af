"""The contract between a caller's tensors and the raw pointers a kernel gets, as one table: a row per core wrapper of
nerf_from_image_amd/ops.py (+ field_backward.field_query_bwd; the synthesis layer's tail, head and modulation) with the
smallest valid arguments, the way to call it, its
tensor arguments, the element count the wrapper must insist on for each, and the widest access a kernel makes through each
pointer.  tests/test_wrapper_contract.py (CPU) and tests/test_wrapper_contract_gpu.py run every row through the same
cases: views of the same values, refused arguments, unaligned views.

Also the three view helpers those cases (and the pose tests) use: strided, permuted, offset."""
import inspect
import re

import torch

from nerf_from_image_amd import _lib, ops
from nerf_from_image_amd import field_backward

# smallest shapes at which these kernels can still go wrong: two scenes, plane resolution 8 (the layouts need R > 3), 70
# points per scene (one wave + a tail), rays 2 x 6 x 8 with 16 samples and the fine pass, A = 0 and 10, the hand-off at
# Cin = 16, R = 8, images 2 x 3 x 9 x 11
B, R, P, H, W, S = 2, 8, 70, 6, 8, 16
N = B * H * W
CIN = 16
IMG = (2, 3, 9, 11)
RANGE = 0.55
VD_RAYS, VD_SAMPLES = 7, 10            # P = 70 points as 7 rays of 10 samples (the view-direction decoder)

# Bytes of the widest load or store a kernel makes through a caller's pointer.  READ_AS_16 lists what was read in the
# kernels (csrc/nfi_layout.inc: planes, texels; nfi_handoff.inc: x, g_out, the texel image; nfi_regulariser.inc, nfi_device.hpp
# and nfi_backward_field.inc: the texel gathers).  Every other argument was NOT traced through its kernel and is treated as
# 16 as well: the wrappers copy any argument whose first byte is not on a multiple of ops.POINTER_ALIGN.
WIDEST_ACCESS = 16
READ_AS_16 = {'planes', 'texels', 'x', 'g_out', 'previous_image'}


# --------------------------------------------------------------------------- views
def strided(t):
    """The same values behind a non-contiguous view (every other element of the last axis of a wider buffer; a 1-D tensor:
    every other element)."""
    if t is None:
        return None
    wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    view = wide[..., ::2]
    view.copy_(t)
    assert not view.is_contiguous() or t.numel() <= 1
    return view


def permuted(t):
    """The same values and shape behind a permute of a dense buffer of the reversed shape (1-D: strided)."""
    if t is None:
        return None
    if t.dim() < 2:
        return strided(t)
    order = tuple(reversed(range(t.dim())))
    view = torch.zeros(tuple(t.shape[i] for i in order), dtype=t.dtype, device=t.device).permute(order)
    view.copy_(t)
    assert view.shape == t.shape
    return view


def offset(t):
    """A contiguous view of the same values that starts one element into a buffer one element longer."""
    if t is None:
        return None
    view = torch.zeros((t.numel() + 1,), dtype=t.dtype, device=t.device)[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() == 1
    return view


def other_layout_view(texels):
    """texels' values and SHAPE over the storage of the other layout: planar [B,3,R,R,32] seen through a permute of a dense
    interleaved buffer, interleaved [B,R,R,3,32] through a permute of a dense planar one - what a shape alone cannot tell
    from a dense tensor."""
    if ops.texel_layout_of(texels) == ops.TEXELS_PLANAR:
        return texels.permute(0, 2, 3, 1, 4).contiguous().permute(0, 3, 1, 2, 4)
    return texels.permute(0, 3, 1, 2, 4).contiguous().permute(0, 2, 3, 1, 4)


VIEWS = {'strided': strided, 'permuted': permuted}


def bit_equal(a, b):
    """Same shape, dtype and bits (NaNs compare by their bits)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    if a.is_floating_point():
        ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        a, b = a.view(ints), b.view(ints)
    return bool(torch.equal(a, b))


# --------------------------------------------------------------------------- the library behind a proxy
def stream_entries(header=_lib.HEADER):
    """Names of the C entries whose declaration has an nfi_stream_t parameter: the ones that launch."""
    src = _lib._strip_comments(open(header).read())
    return {m.group(1) for m in re.finditer(r'\b(nfi_\w+)\s*\(([^)]*)\)\s*;', src) if 'nfi_stream_t' in m.group(2)}


class ReachedLibrary(BaseException):
    """A call got as far as an entry that launches.  (Not an Exception: no handler of a wrapper may swallow it.)"""


class LibraryProxy:
    """The real library for the pure size queries (no nfi_stream_t in the declaration); any entry that takes a stream
    raises ReachedLibrary with its name instead of running."""

    def __init__(self, real):
        self._real = real
        self._launching = stream_entries()
        self.reached = []

    def __getattr__(self, name):
        if name in self._launching:
            def refuse(*args, **kw):
                self.reached.append(name)
                raise ReachedLibrary(name)
            return refuse
        return getattr(self._real, name)


def install_proxy(monkeypatch):
    proxy = LibraryProxy(_lib.load())
    monkeypatch.setattr(_lib, 'load', lambda: proxy)
    return proxy


# --------------------------------------------------------------------------- rows
class Row:
    def __init__(self, rid, fn, build, call, counts, exact=True, tolerance=None, f16_ok=(), g_texels=False):
        """rid: test id; fn: the wrapper's name; build(dev) -> dict of arguments (seeded); call(args) -> the wrapper's
        result; counts: {tensor argument: None (it sets the sizes) or f(args) -> the element count the wrapper must insist
        on}, whose keys are the row's tensor arguments; exact: the result is bit-reproducible (backwards: in their ordered
        mode); tolerance: else |a - b| <= tolerance x max |b|; f16_ok: arguments that may be float16; g_texels: the result
        has a 'g_texels' gradient image."""
        self.id, self.fn, self.build, self._call, self.counts = rid, fn, build, call, counts
        self.exact, self.tolerance, self.f16_ok, self.g_texels = exact, tolerance, set(f16_ok), g_texels
        self.tensors = tuple(counts)
        self.widest = {name: WIDEST_ACCESS for name in counts}

    def call(self, args):
        return self._call(args)

    def outputs(self, args):
        """The result as a tuple of tensors in a fixed order."""
        return flatten(self._call(args))


def flatten(res):
    if res is None:
        return ()
    if torch.is_tensor(res):
        return (res,)
    if isinstance(res, dict):
        return tuple(t for k in sorted(res) if not k.startswith('_') for t in flatten(res[k]))
    return tuple(t for r in res for t in flatten(r))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _scene(dev, seed, A, layout, dtype=torch.float32, viewdir=False):
    g = _gen(seed)
    planes = 0.5 * torch.randn(B, 3, 32, R, R, generator=g)
    texels = planes.permute(0, 1, 3, 4, 2) if layout == ops.TEXELS_PLANAR else planes.permute(0, 3, 4, 1, 2)
    n_out = 33 if viewdir else (1 + A if A > 0 else 4)
    n3 = A if A > 0 else 3
    a = dict(points=(torch.rand(B, P, 3, generator=g) * 2 - 1) * RANGE * 0.95, texels=texels.contiguous().to(dtype),
             w1=torch.randn(64, 32, generator=g), b1=0.3 * torch.randn(64, generator=g),
             w2=torch.randn(n_out, 64, generator=g), b2=0.3 * torch.randn(n_out, generator=g),
             attention_values=torch.rand(B, A, 3, generator=g) * 2 - 1 if A > 0 else None,
             beta=torch.tensor([0.12]), alpha=torch.tensor([0.3]), n_attention=A)
    if viewdir:
        a.update(w3=torch.randn(n3, 32, generator=g), b3=0.3 * torch.randn(n3, generator=g))
    a = {k: v.to(dev) if torch.is_tensor(v) else v for k, v in a.items()}
    tdt = ops.texel_dtype_of(a['texels'])
    if torch.device(dev).type == 'cuda':
        a['decoder_image'] = (ops.decoder_pack_viewdir(*(a[k] for k in ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')), A, tdt) if viewdir
                              else ops.decoder_pack(a['w1'], a['b1'], a['w2'], a['b2'], A, tdt))
    else:           # (the host-tensor cases never get as far as reading it)
        a['decoder_image'] = torch.zeros(ops._decoder_image_floats(viewdir))
    return a, g


def _image_floats(viewdir):
    return lambda a: ops._decoder_image_floats(viewdir)


def _rows():
    rows = []

    def add(rid, fn, build, call, counts, **kw):
        rows.append(Row(rid, fn, build, call, counts, **kw))

    # ---- layout, decoder image
    add('planes_to_texels', 'planes_to_texels',
        lambda dev: dict(planes=torch.randn(B, 3, 32, R, R, generator=_gen(1)).to(dev)),
        lambda a: ops.planes_to_texels(a['planes']), {'planes': None})
    add('planes_to_texels[bf16]', 'planes_to_texels',
        lambda dev: dict(planes=torch.randn(B, 3, 32, R, R, generator=_gen(2)).to(dev)),
        lambda a: ops.planes_to_texels(a['planes'], ops.TEXEL_BF16), {'planes': None})
    add('texels_to_planes', 'texels_to_planes',
        lambda dev: dict(texels=torch.randn(B, 3, R, R, 32, generator=_gen(3)).to(dev)),
        lambda a: ops.texels_to_planes(a['texels']), {'texels': None})
    for A in (0, 10):
        n_out = 1 + A if A else 4
        add('decoder_pack[A%d]' % A, 'decoder_pack', lambda dev, A=A: _scene(dev, 4, A, 0)[0],
            lambda a: ops.decoder_pack(a['w1'], a['b1'], a['w2'], a['b2'], a['n_attention']),
            {'w1': lambda a: 2048, 'b1': lambda a: 64, 'w2': lambda a, n=n_out: 64 * n, 'b2': lambda a, n=n_out: n})
        n3 = A if A else 3
        add('decoder_pack_viewdir[A%d]' % A, 'decoder_pack_viewdir', lambda dev, A=A: _scene(dev, 5, A, 0, viewdir=True)[0],
            lambda a: ops.decoder_pack_viewdir(a['w1'], a['b1'], a['w2'], a['b2'], a['w3'], a['b3'], a['n_attention']),
            {'w1': lambda a: 2048, 'b1': lambda a: 64, 'w2': lambda a: 64 * 33, 'b2': lambda a: 33,
             'w3': lambda a, n=n3: 32 * n, 'b3': lambda a, n=n3: n})

    # ---- ray stages
    def cameras(dev, seed=6):
        from stand_in import look_at_cameras
        g = _gen(seed)
        cam = look_at_cameras(B, 2.0, g)
        a = dict(cam2world=cam, focal=1.0 + 0.05 * torch.rand(B, generator=g),
                 bbox=torch.tensor([[-1.0, -1.0], [2.0, 2.0]]).repeat(B, 1, 1) + 0.01 * torch.rand(B, 2, 2, generator=g),
                 center=0.02 * (torch.rand(B, 2, generator=g) - 0.5))
        return {k: v.to(dev) for k, v in a.items()}, g
    cam_counts = {'cam2world': None, 'focal': lambda a: B, 'bbox': lambda a: 4 * B, 'center': lambda a: 2 * B}
    add('raygen', 'raygen', lambda dev: cameras(dev)[0],
        lambda a: ops.raygen(H, W, a['focal'], a['cam2world'], a['bbox'], a['center'], normalize=True), cam_counts)

    def rays(dev, seed=7):
        g = _gen(seed)
        ro = torch.randn(B, H, W, 3, generator=g)
        ro = 2.0 * ro / ro.norm(dim=-1, keepdim=True)
        rd = -ro / 2.0 + 0.1 * torch.randn(B, H, W, 3, generator=g)
        near = 1.2 + 0.1 * torch.rand(B, H, W, generator=g)
        depth = (near[..., None] + torch.sort(torch.rand(B, H, W, S, generator=g), dim=-1).values * 1.5).contiguous()
        a = dict(ray_origins=ro, ray_directions=rd, near=near, far=near + 1.5, noise=torch.rand(B, H, W, S, generator=g),
                 depth=depth, sigma=3 * torch.rand(B, H, W, S, generator=g), rgb=torch.rand(B, H, W, S, 3, generator=g),
                 u=torch.rand(N, S, generator=g))
        return {k: v.to(dev) for k, v in a.items()}, g
    add('near_far', 'near_far', lambda dev: rays(dev)[0],
        lambda a: ops.near_far(a['ray_origins'], a['ray_directions'], RANGE, strict=False),
        {'ray_origins': None, 'ray_directions': lambda a: 3 * N})
    add('stratified_points', 'stratified_points', lambda dev: rays(dev)[0],
        lambda a: ops.stratified_points(a['ray_origins'], a['ray_directions'], a['near'], a['far'], S, a['noise']),
        {'ray_origins': None, 'ray_directions': lambda a: 3 * N, 'near': lambda a: N, 'far': lambda a: N, 'noise': lambda a: N * S})
    add('points_on_rays', 'points_on_rays', lambda dev: rays(dev)[0],
        lambda a: ops.points_on_rays(a['ray_origins'], a['ray_directions'], a['depth']),
        {'depth': None, 'ray_origins': lambda a: 3 * N, 'ray_directions': lambda a: 3 * N})
    add('ray_weights', 'ray_weights', lambda dev: rays(dev)[0],
        lambda a: ops.ray_weights(a['sigma'], a['ray_directions'], a['depth']),
        {'depth': None, 'sigma': lambda a: N * S, 'ray_directions': lambda a: 3 * N})

    def pdf(dev):
        g = _gen(8)
        bins = torch.sort(torch.rand(N, S, generator=g), dim=-1).values
        a = dict(bins=bins, weights=torch.rand(N, S - 1, generator=g) + 1e-3, u=torch.rand(N, 11, generator=g))
        return {k: v.to(dev) for k, v in a.items()}
    add('sample_pdf', 'sample_pdf', pdf, lambda a: ops.sample_pdf(a['bins'], a['weights'], a['u'], want_inds=True, want_cdf=True),
        {'bins': None, 'weights': lambda a: N * (S - 1), 'u': lambda a: N * 11})
    add('resample', 'resample', lambda dev: rays(dev)[0],
        lambda a: ops.resample(a['sigma'], a['ray_directions'], a['depth'], a['u'], want_taps=True),
        {'depth': None, 'sigma': lambda a: N * S, 'ray_directions': lambda a: 3 * N, 'u': lambda a: N * S})

    def lists(dev):
        a, g = rays(dev, 9)
        nb, e = 5, 4
        b = dict(depth_b=(1.2 + 1.5 * torch.rand(B, H, W, nb, generator=g)), sigma_b=3 * torch.rand(B, H, W, nb, generator=g),
                 rgb_b=torch.rand(B, H, W, nb, 3, generator=g), extra_a=torch.randn(B, H, W, S, e, generator=g),
                 extra_b=torch.randn(B, H, W, nb, e, generator=g), g_rgb_map=torch.randn(B, H, W, 3, generator=g),
                 g_mask=torch.randn(B, H, W, generator=g), g_extra_map=torch.randn(B, H, W, e, generator=g),
                 g_points=torch.randn(B, H, W, S, 3, generator=g))
        a.update({k: v.to(dev) for k, v in b.items()})
        return a
    list_counts = {'depth': None, 'ray_directions': lambda a: 3 * N, 'sigma': lambda a: N * S, 'rgb': lambda a: 3 * N * S,
                   'depth_b': lambda a: 5 * N, 'sigma_b': lambda a: 5 * N, 'rgb_b': lambda a: 15 * N,
                   'extra_a': lambda a: 4 * N * S, 'extra_b': lambda a: 20 * N}
    add('composite', 'composite', lists,
        lambda a: ops.composite(a['ray_directions'], a['depth'], a['sigma'], a['rgb'], a['depth_b'], a['sigma_b'], a['rgb_b'],
                                a['extra_a'], a['extra_b'], want_taps=True), list_counts)
    add('composite_bwd', 'composite_bwd', lists,
        lambda a: ops.composite_bwd(a['ray_directions'], a['depth'], a['sigma'], a['rgb'], a['g_rgb_map'], a['g_mask'], a['depth_b'],
                                    a['sigma_b'], a['rgb_b'], a['extra_a'], a['extra_b'], a['g_extra_map']),
        dict(list_counts, g_rgb_map=lambda a: 3 * N, g_mask=lambda a: N, g_extra_map=lambda a: 4 * N))
    add('composite_bwd_stash', 'composite_bwd_stash', lists,
        lambda a: ops.composite_bwd_stash(a['ray_directions'], a['depth'], a['sigma'], a['rgb'], a['g_rgb_map'], a['g_mask']),
        {'depth': None, 'ray_directions': lambda a: 3 * N, 'sigma': lambda a: N * S, 'rgb': lambda a: 3 * N * S,
         'g_rgb_map': lambda a: 3 * N, 'g_mask': lambda a: N})
    add('points_bwd', 'points_bwd', lists, lambda a: ops.points_bwd(a['g_points'], a['depth']),
        {'depth': None, 'g_points': lambda a: 3 * N * S})

    def cam_grads(dev):
        a, g = cameras(dev, 10)
        a.update(g_ro=torch.randn(B, H, W, 3, generator=g).to(dev), g_rd=torch.randn(B, H, W, 3, generator=g).to(dev))
        return a
    add('raygen_bwd', 'raygen_bwd', cam_grads,
        lambda a: ops.raygen_bwd(H, W, a['focal'], a['cam2world'], a['bbox'], a['center'], True, a['g_ro'], a['g_rd'], ordered=True),
        dict(cam_counts, g_ro=lambda a: 3 * N, g_rd=lambda a: 3 * N))

    # ---- field query, fused render, their backwards
    def field(dev, seed, A, layout, dtype=torch.float32, viewdir=False):
        a, g = _scene(dev, seed, A, layout, dtype, viewdir)
        b = dict(g_sigma=torch.randn(B, P, generator=g), g_rgb=torch.randn(B, P, 3, generator=g), g_sdf=torch.randn(B, P, generator=g),
                 g_semantics=torch.randn(B, P, A, generator=g) if A else None,
                 ray_features=torch.randn(B, VD_RAYS, 32, generator=g) if viewdir else None)
        a.update({k: v.to(dev) if v is not None else None for k, v in b.items()})
        if viewdir:
            a['ray_features'] = torch.nn.functional.pad(a['ray_features'], (1, ops.RAY_FEATURE_PITCH - 33)).contiguous()
        return a
    variants = [('A10-planar-f32', 10, ops.TEXELS_PLANAR, torch.float32, False),
                ('A0-interleaved-bf16', 0, ops.TEXELS_INTERLEAVED, torch.bfloat16, False),
                ('A10-interleaved-f16', 10, ops.TEXELS_INTERLEAVED, torch.float16, False),
                ('viewdir-A0-planar-f32', 0, ops.TEXELS_PLANAR, torch.float32, True)]
    for tag, A, layout, dtype, vd in variants:
        n_out = 33 if vd else (1 + A if A else 4)
        fq = {'points': None, 'texels': lambda a: B * 3 * R * R * 32, 'decoder_image': _image_floats(vd),
              'beta': lambda a: 1, 'alpha': lambda a: 1}
        if A:
            fq['attention_values'] = lambda a, A=A: B * A * 3
        if vd:
            fq['ray_features'] = lambda a: B * VD_RAYS * ops.RAY_FEATURE_PITCH
        add('field_query[%s]' % tag, 'field_query', lambda dev, A=A, layout=layout, dtype=dtype, vd=vd: field(dev, 11, A, layout, dtype, vd),
            lambda a, vd=vd: ops.field_query(a['points'], a['texels'], a['decoder_image'], RANGE, a['n_attention'], a['attention_values'], True,
                                             a['beta'], a['alpha'], want_sdf=True, want_semantics=a['n_attention'] > 0, want_outside=True,
                                             ray_features=a['ray_features'], samples_per_ray=VD_SAMPLES if vd else 0),
            fq, f16_ok=('texels',))
        fb = dict(fq, w1=lambda a: 2048, w2=lambda a, n=n_out: 64 * n, g_sigma=lambda a: B * P, g_rgb=lambda a: 3 * B * P,
                  g_sdf=lambda a: B * P)
        if A:
            fb['g_semantics'] = lambda a, A=A: B * P * A
        if vd:
            fb['w3'] = lambda a, A=A: 32 * (A if A else 3)
        # ordered (scatter_mode 2) where it exists: the plain decoder.  The view-direction decoder has none (its ray-feature
        # gradients are atomics): compared at the bound of its float64 parity test, tests/test_hip_backward.py
        # test_field_query_backward_viewdir (5e-4 of the largest entry)
        add('field_query_bwd[%s]' % tag, 'field_query_bwd', lambda dev, A=A, layout=layout, dtype=dtype, vd=vd: field(dev, 12, A, layout, dtype, vd),
            lambda a, vd=vd: field_backward.field_query_bwd(
                a['points'], a['texels'], a['decoder_image'], a['w1'], a['w2'], RANGE, a['n_attention'], a['attention_values'], True,
                a['beta'], a['alpha'], a['g_sigma'], a['g_rgb'], a['g_sdf'], a['g_semantics'], want_points=True,
                viewdir=dict(ray_features=a['ray_features'], samples_per_ray=VD_SAMPLES, w3=a['w3']) if vd else None,
                scatter_mode=0 if vd else 2),
            fb, exact=not vd, tolerance=5e-4 if vd else None, f16_ok=('texels',), g_texels=True)

    def render(dev, A, layout, dtype, vd):
        a = field(dev, 13, A, layout, dtype, vd)
        c, g = cameras(dev, 14)
        a.update(c)
        a.update(noise_coarse=torch.rand(B, H, W, S, generator=g).to(dev), noise_fine=torch.rand(N, S, generator=g).to(dev))
        if vd:
            x = torch.randn(B, H, W, 32, generator=g).to(dev)
            a['ray_features'] = torch.nn.functional.pad(x, (1, ops.RAY_FEATURE_PITCH - 33)).contiguous()
        return a
    for tag, A, layout, dtype, vd in variants:
        rc = dict(cam_counts, texels=lambda a: B * 3 * R * R * 32, decoder_image=_image_floats(vd), beta=lambda a: 1, alpha=lambda a: 1,
                  noise_coarse=lambda a: N * S, noise_fine=lambda a: N * S)
        if A:
            rc['attention_values'] = lambda a, A=A: B * A * 3
        if vd:
            rc['ray_features'] = lambda a: N * ops.RAY_FEATURE_PITCH
        add('render_fwd[%s]' % tag, 'render_fwd', lambda dev, A=A, layout=layout, dtype=dtype, vd=vd: render(dev, A, layout, dtype, vd),
            lambda a: ops.render_fwd(a['cam2world'], a['focal'], H, W, S, a['texels'], a['decoder_image'], RANGE, a['n_attention'],
                                     a['attention_values'], True, a['beta'], a['alpha'], a['bbox'], a['center'], a['noise_coarse'],
                                     a['noise_fine'], ray_features=a['ray_features'], want_semantics=a['n_attention'] > 0),
            rc, f16_ok=('texels',))

    def setup_then_render(a):
        ws = ops.render_setup(a['cam2world'], a['focal'], H, W, RANGE, a['bbox'], a['center'])
        return ops.render_fwd(a['cam2world'], a['focal'], H, W, S, a['texels'], a['decoder_image'], RANGE, a['n_attention'],
                              a['attention_values'], True, a['beta'], a['alpha'], a['bbox'], a['center'], a['noise_coarse'], a['noise_fine'],
                              workspace=ws, rays_ready=True)
    # (the workspace render_setup returns holds scratch besides the rays: it is compared through the render that marches it)
    add('render_setup', 'render_setup', lambda dev: render(dev, 10, ops.TEXELS_PLANAR, torch.float32, False), setup_then_render, cam_counts)

    # ---- regulariser
    def sdf(dev, layout):
        a, g = _scene(dev, 15, 0, layout)
        a.update(g_sdf=torch.randn(B, P, generator=g).to(dev), g_gradient=torch.randn(B, P, 3, generator=g).to(dev))
        return a
    sc = {'points': None, 'texels': lambda a: B * 3 * R * R * 32, 'w1': lambda a: 2048, 'b1': lambda a: 64, 'w2': None, 'b2': lambda a: 4}
    for tag, layout in (('planar', ops.TEXELS_PLANAR), ('interleaved', ops.TEXELS_INTERLEAVED)):
        add('sdf_gradient_fwd[%s]' % tag, 'sdf_gradient_fwd', lambda dev, layout=layout: sdf(dev, layout),
            lambda a: ops.sdf_gradient_fwd(a['points'], a['texels'], a['w1'], a['b1'], a['w2'], a['b2'], RANGE), sc)
        add('sdf_gradient_bwd[%s]' % tag, 'sdf_gradient_bwd', lambda dev, layout=layout: sdf(dev, layout),
            lambda a: ops.sdf_gradient_bwd(a['points'], a['texels'], a['w1'], a['b1'], a['w2'], a['b2'], RANGE, a['g_sdf'], a['g_gradient'],
                                           ordered=True),
            dict(sc, g_sdf=lambda a: B * P, g_gradient=lambda a: 3 * B * P), g_texels=True)

    def overlay(dev):
        g = _gen(16)
        return dict(points=((torch.rand(B, P, 3, generator=g) * 2 - 1) * RANGE * 1.1).to(dev), sigma=torch.rand(B, P, generator=g).to(dev))
    add('bbox_overlay', 'bbox_overlay', overlay, lambda a: ops.bbox_overlay(a['points'], a['sigma'], RANGE),
        {'sigma': None, 'points': lambda a: 3 * B * P})

    # ---- warp, metrics, hand-off
    def images(dev):
        g = _gen(17)
        n = IMG[0]
        a = dict(img=torch.rand(*IMG, generator=g), g_out=torch.randn(*IMG, generator=g), rot=0.5 * torch.randn(n, generator=g),
                 scale=1.0 + 0.2 * torch.rand(n, generator=g), translation=0.2 * torch.randn(n, 2, generator=g),
                 pred=torch.rand(*IMG, generator=g), target=torch.rand(*IMG, generator=g),
                 mask_pred=torch.rand(n, 1, IMG[2], IMG[3], generator=g), mask_real=(torch.rand(n, 1, IMG[2], IMG[3], generator=g) > 0.5).float())
        return {k: v.to(dev) for k, v in a.items()}
    wc = {'rot': lambda a: IMG[0], 'scale': lambda a: IMG[0], 'translation': lambda a: 2 * IMG[0]}
    add('affine_warp', 'affine_warp', images, lambda a: ops.affine_warp(a['img'], a['rot'], a['scale'], a['translation'], True), dict(wc, img=None))
    add('affine_warp_bwd', 'affine_warp_bwd', images,
        lambda a: ops.affine_warp_bwd(a['g_out'], a['rot'], a['scale'], a['translation'], True, ordered=True), dict(wc, g_out=None))
    n_img = IMG[0] * IMG[1] * IMG[2] * IMG[3]
    add('image_metrics', 'image_metrics', images, lambda a: ops.image_metrics(a['pred'], a['target'], a['mask_pred'], a['mask_real']),
        {'pred': None, 'target': lambda a: n_img, 'mask_pred': lambda a: n_img // 3, 'mask_real': lambda a: n_img // 3})

    def handoff(dev):
        g = _gen(18)
        a = dict(x=torch.randn(B, CIN, R, R, generator=g), styles=torch.randn(B, CIN, generator=g), weight=torch.randn(96, CIN, generator=g),
                 bias=0.3 * torch.randn(96, generator=g), previous_image=torch.randn(B, 96, R // 2, R // 2, generator=g),
                 g_out=torch.randn(B, 96, R, R, generator=g))
        return {k: v.to(dev) for k, v in a.items()}
    hc = {'x': None, 'styles': lambda a: B * CIN, 'weight': lambda a: 96 * CIN, 'previous_image': lambda a: B * 96 * (R // 2) ** 2}
    add('torgb_texels', 'torgb_texels', handoff,
        lambda a: ops.torgb_texels(a['x'], a['styles'], a['weight'], a['bias'], a['previous_image']), dict(hc, bias=lambda a: 96))
    add('torgb_texels_bwd', 'torgb_texels_bwd', handoff,
        lambda a: ops.torgb_texels_bwd(a['g_out'], a['x'], a['styles'], a['weight'], a['previous_image'], ordered=True),
        dict(hc, g_out=lambda a: B * 96 * R * R))

    # ---- synthesis layer: tail, head, modulation.  The families' own smallest shapes (tests/test_synth_tail_gpu.py,
    # tests/synth_head_util.py): the tail at B = 2, C = 3, R = 4, once with `up` (y one wider, the 4x4 filter, noise per image)
    # and once without (one noise plane for the batch); the head at D = 70 (one wave and a tail), I = 5, O = 3, K = 9 with
    # demodulation and a bias; the modulation on x [2,5,4,4].  What a backward reads of its forward comes from the forward
    # (on the CPU, where no row gets as far as reading it: zeros of that shape).
    TB, TC, TR = 2, 3, 4
    GAIN = 2.0 ** 0.5

    def tail(dev, up):
        g = _gen(19 + int(up))
        n = TR + 1 if up else TR
        a = dict(y=torch.randn(TB, TC, n, n, generator=g), dcoefs=0.5 + torch.rand(TB, TC, generator=g),
                 noise=0.1 * (torch.randn(TB, 1, TR, TR, generator=g) if up else torch.randn(TR, TR, generator=g)),
                 bias=0.3 * torch.randn(TC, generator=g), taps=torch.rand(4, 4, generator=g) / 8 if up else None,
                 g_out=torch.randn(TB, TC, TR, TR, generator=g))
        a = {k: v if v is None else v.to(dev) for k, v in a.items()}
        a['out'] = (ops.synth_tail(a['y'], a['dcoefs'], a['noise'], a['bias'], a['taps'], GAIN, up) if torch.device(dev).type == 'cuda'
                    else torch.zeros(TB, TC, TR, TR))
        return a
    for up in (True, False):
        tc = {'y': None, 'dcoefs': lambda a: TB * TC, 'noise': lambda a, up=up: (TB if up else 1) * TR * TR, 'bias': lambda a: TC}
        if up:
            tc['taps'] = lambda a: 16
        tag = 'up' if up else 'shared-noise'
        add('synth_tail[%s]' % tag, 'synth_tail', lambda dev, up=up: tail(dev, up),
            lambda a, up=up: ops.synth_tail(a['y'], a['dcoefs'], a['noise'], a['bias'], a['taps'], GAIN, up), tc)
        add('synth_tail_bwd[%s]' % tag, 'synth_tail_bwd', lambda dev, up=up: tail(dev, up),
            lambda a, up=up: ops.synth_tail_bwd(a['g_out'], a['out'], a['y'], a['dcoefs'], a['noise'], a['bias'], a['taps'], GAIN, up,
                                                need_noise=True),
            dict(tc, g_out=lambda a: TB * TC * TR * TR, out=lambda a: TB * TC * TR * TR))

    HB, HD, HI, HO, HK = 2, 70, 5, 3, 9

    def head(dev):
        g = _gen(21)
        a = dict(latent=torch.randn(HB, HD, generator=g), affine_weight=torch.randn(HI, HD, generator=g),
                 affine_bias=1.0 + 0.5 * torch.randn(HI, generator=g), conv_weight=torch.randn(HO, HI, 3, 3, generator=g),
                 g_styles=torch.randn(HB, HI, generator=g), g_dcoefs=torch.randn(HB, HO, generator=g))
        a = {k: v.to(dev) for k, v in a.items()}
        a['styles'], a['dcoefs'] = (head_fwd(a) if torch.device(dev).type == 'cuda' else (torch.zeros(HB, HI), torch.zeros(HB, HO)))
        return a

    def head_fwd(a):
        return ops.synth_head(a['latent'], a['affine_weight'], a['affine_bias'], HD ** -0.5, 1.0, a['conv_weight'])
    # conv_weight sets O for the forward; the backward has dcoefs [B,O] to hold it to
    add('synth_head', 'synth_head', head, head_fwd,
        {'latent': None, 'affine_weight': lambda a: HI * HD, 'affine_bias': lambda a: HI, 'conv_weight': None})
    add('synth_head_bwd', 'synth_head_bwd', head,
        lambda a: ops.synth_head_bwd(a['g_styles'], a['g_dcoefs'], a['styles'], a['dcoefs'], a['latent'], a['affine_weight'], a['affine_bias'],
                                     HD ** -0.5, 1.0, a['conv_weight']),
        {'latent': None, 'affine_weight': lambda a: HI * HD, 'affine_bias': lambda a: HI, 'conv_weight': lambda a: HO * HI * HK,
         'g_styles': lambda a: HB * HI, 'g_dcoefs': lambda a: HB * HO, 'styles': lambda a: HB * HI, 'dcoefs': lambda a: HB * HO})

    def modulation(dev):
        g = _gen(22)
        a = dict(x=torch.randn(2, 5, 4, 4, generator=g), styles=torch.randn(2, 5, generator=g), g_out=torch.randn(2, 5, 4, 4, generator=g))
        return {k: v.to(dev) for k, v in a.items()}
    add('synth_modulate', 'synth_modulate', modulation, lambda a: ops.synth_modulate(a['x'], a['styles']),
        {'x': None, 'styles': lambda a: 10})
    # a dense x or g_out one float off 16-byte alignment is read in place on the scalar path, which adds a plane's products in
    # another order than the 16-byte path: g_styles within one unit in the last place of its largest entry, the bound of
    # tests/test_synth_head_gpu.py test_modulate_views_and_unaligned_planes (which also holds the copied views to the same bits)
    add('synth_modulate_bwd', 'synth_modulate_bwd', modulation, lambda a: ops.synth_modulate_bwd(a['g_out'], a['x'], a['styles']),
        {'x': None, 'styles': lambda a: 10, 'g_out': lambda a: 160}, exact=False, tolerance=2.0 ** -23)
    return rows


ROWS = _rows()
ROW_IDS = [r.id for r in ROWS]

# public callables of ops.py that reach the library and have no row, each with the reason
EXEMPT = {
    'texel_grad_to_planes': 'a permute, or texels_to_planes, which has a row',
    'synth_tail_launch': 'takes the dict synth_tail_args has checked: covered through synth_tail',
    'synth_tail_bwd_launch': 'takes the dict synth_tail_args has checked: covered through synth_tail_bwd',
    'synth_head_launch': 'takes the dict synth_head_args has checked: covered through synth_head',
    'synth_head_bwd_launch': 'takes the dict synth_head_args has checked: covered through synth_head_bwd',
    'synth_modulate_launch': 'takes the dict synth_modulate_args has checked: covered through synth_modulate',
    'synth_modulate_bwd_launch': 'takes the dict synth_modulate_args has checked: covered through synth_modulate_bwd',
    'image_ssim': 'dense in either layout, else copied: tests/test_ssim_gpu.py',
    'separable_filter': 'dense in either layout, else copied: tests/test_blur_gpu.py',
    'lpips_head': '_lpips_inputs: tests/test_lpips_gpu.py',
    'lpips_head_bwd': '_lpips_inputs: tests/test_lpips_gpu.py',
    'viewdir_mapper_fwd': 'views and the shifted gradient: tests/test_viewdir_mapper.py',
    'viewdir_mapper_bwd': 'views and the shifted gradient: tests/test_viewdir_mapper.py',
    'pose_to_matrix': 'strided views: tests/test_pose_utils_gpu.py',
    'pose_to_matrix_bwd': 'strided views: tests/test_pose_utils_gpu.py',
    'matrix_to_pose': 'strided views: tests/test_pose_utils_gpu.py',
    'rotation_distance': 'strided views: tests/test_pose_utils_gpu.py',
    'pose_nearest_by_angle': 'strided views: tests/test_pose_utils_gpu.py',
    'pose_project_': 'in place: refuses what it cannot change in place, tests/test_pose_utils_gpu.py',
}


def wrappers_that_reach_the_library(module=ops):
    """Public functions of `module` whose body hands something to _lib.ptr / call_struct / make_args / struct_query (or to
    the module's launch and workspace helpers, which do), directly or through another function of the module - a private
    one as well: a public wrapper whose only way to the library is `_something(...)` is found."""
    direct = re.compile(r'_lib\.(ptr|call_struct|make_args|struct_query)\(|\b_(launch|launch_positional|workspace|call_ordered)\(')
    own = {n: inspect.getsource(f) for n, f in vars(module).items() if inspect.isfunction(f) and f.__module__ == module.__name__}
    found = {n for n, src in own.items() if direct.search(src)}
    grew = True
    while grew:
        grew = False
        for n, src in own.items():
            if n not in found and any(re.search(r'\b%s\(' % re.escape(m), src) for m in found):
                found.add(n)
                grew = True
    return {n for n in found if not n.startswith('_')}
