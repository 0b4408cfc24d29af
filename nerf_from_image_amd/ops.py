"""Tensor-level wrappers over the C ABI (one function per entry point of include/nfi_hip.h).

PyTorch is used here for device memory and streams only: every function checks
its inputs, allocates the outputs as torch tensors, and passes raw device
pointers plus ``torch.cuda.current_stream()`` to libnfi_hip.so.  Nothing here
computes on the CPU and nothing falls back to ATen ops.

The argument contract (tests/contract_util.py has a row per wrapper, tests/test_wrapper_contract*.py run them): the C ABI
sees pointers and a few integers, so this layer is the only one that can know a tensor's strides, dtype, device and
length.  Every tensor argument is therefore
  - refused when it is not on the GPU (RuntimeError), has the wrong dtype (TypeError), lives on another device than the
    tensor whose stream the call uses, or does not hold the element count the kernel indexes (ValueError) - _refuse, the
    one place that says so; _f32c (with `on` / `n`) is its common front, and _texels, _u_and_stride, _latent_rows,
    _range_flag and the tensors a caller hands in to be written rest on it too; _need checks shapes by rows;
  - copied when it is not dense in the layout its shape claims, or when its first byte is not on a multiple of
    POINTER_ALIGN (a contiguous view at an odd offset into a flat buffer): kernels read texels, planes and the hand-off's
    activations as 16-byte vectors, and no other alignment is tested for the rest - _dense, _dense_channels_last, and
    _nchw_or_nhwc for the images that are read in place in either layout.
All of it is attribute reads on the host: a dense, aligned argument costs no launch and no device-to-host read.

Every launch goes through _launch (the entries that take a struct) or _launch_positional (the rest): they enter the device
of the tensor whose stream the call uses and pass that device's current stream.  _workspace allocates a call's scratch
buffer, or raises for a shape the library reports as unsupported (a size of 0).
"""
import functools
import math

import torch

from . import _lib

TEXEL_F32 = 0
TEXEL_BF16 = 1
TEXEL_F16 = 2
_TEXEL_TORCH = {TEXEL_F32: torch.float32, TEXEL_BF16: torch.bfloat16, TEXEL_F16: torch.float16}


def texel_dtype_of(texels):
    for k, v in _TEXEL_TORCH.items():
        if texels.dtype == v:
            return k
    raise TypeError('texels must be float32, bfloat16 or float16, got %s' % texels.dtype)


TEXELS_PLANAR = 0          # [B,3,R,R,32]
TEXELS_INTERLEAVED = 1     # [B,R,R,3,32] = channels-last [B,96,R,R]


def texel_layout_of(texels):
    """Layout of a texel tensor from its shape: [B,3,R,R,32] planar, [B,R,R,3,32] interleaved (R > 3)."""
    if texels.dim() != 5 or texels.shape[4] != 32:
        raise ValueError('texels must be [B,3,R,R,32] or [B,R,R,3,32], got %s' % (tuple(texels.shape),))
    if texels.shape[1] == 3 and texels.shape[2] == texels.shape[3]:
        return TEXELS_PLANAR
    if texels.shape[3] == 3 and texels.shape[1] == texels.shape[2]:
        return TEXELS_INTERLEAVED
    raise ValueError('texels must be [B,3,R,R,32] or [B,R,R,3,32], got %s' % (tuple(texels.shape),))


def texel_res(texels):
    return texels.shape[2]          # R sits at index 2 in both layouts


def planes_view_as_texels(planes):
    """planes [B,3,32,R,R] (a view of the producer's [B,96,R,R] output): if that output is channels-last in memory
    (torch.channels_last, or written by torgb_texels), returns the zero-copy interleaved texel view [B,R,R,3,32];
    otherwise None (the caller then runs planes_to_texels)."""
    if planes.dim() != 5 or planes.shape[1] != 3 or planes.shape[2] != 32 or planes.shape[3] <= 3:
        return None
    v = planes.permute(0, 3, 4, 1, 2)
    return v if v.is_contiguous() else None


def texel_grad_to_planes(g_texels):
    """Gradient image in texel layout -> gradient of the [B,3,32,R,R] planes view (a kernel for the planar layout,
    a zero-copy strided view for the interleaved one)."""
    if texel_layout_of(g_texels) == TEXELS_INTERLEAVED:
        return g_texels.permute(0, 3, 4, 1, 2)
    return texels_to_planes(g_texels)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _launch(entry, struct, on, *extra, **fields):
    """One entry that takes a struct, on the current stream of the device of `on`, with that device entered for the call.
    extra: the entry's arguments between the struct and the stream (a tensor stands for its device pointer).  (The device
    goes to torch as its index: that spares both calls the parsing of a torch.device, on a path a host-bound layer runs
    several times.)"""
    index = on.get_device()
    with torch.cuda.device(index):
        _lib.call_struct(entry, struct, torch.cuda.current_stream(index).cuda_stream, *extra, **fields)


def _launch_positional(entry, on, *args):
    """The same for an entry that takes its arguments one by one; args: all of them but the stream (a tensor stands for
    its device pointer, None for a null pointer)."""
    fn = getattr(_lib.load(), entry)
    index = on.get_device()
    with torch.cuda.device(index):
        _lib.check(fn(*[_lib.ptr(a) if torch.is_tensor(a) else a for a in args], torch.cuda.current_stream(index).cuda_stream), entry)


def _workspace(n_bytes, on, where, shape, dtype=torch.uint8):
    """A call's scratch buffer of at least n_bytes on the device of `on`, as whole elements of `dtype` (the type whose
    alignment the kernel counts on).  A size of 0 is the library's answer for a shape it does not support: RuntimeError
    naming `where` and `shape`."""
    if n_bytes == 0:
        raise RuntimeError('%s: shape not supported: %s' % (where, shape))
    size = dtype.itemsize
    return torch.empty(((n_bytes + size - 1) // size,), dtype=dtype, device=on.device)


def _call_ordered(entry, struct, on, where, shape, args):
    """An ordered entry with a workspace: the size from `entry`_workspace_bytes, allocated per call."""
    ws = _workspace(_lib.struct_query(entry + '_workspace_bytes', struct, **args), on, where, shape)
    _launch(entry, struct, on, ws, ws.numel(), **args)


POINTER_ALIGN = 16         # bytes: the widest vector a kernel reads or writes through a caller's pointer


def _dense(t, align=POINTER_ALIGN):
    """t itself if it is contiguous and its first byte sits on a multiple of `align`, else a copy in fresh storage (a
    contiguous view at an odd offset into a flat buffer is a copy too: kernels read rows as 8- and 16-byte vectors)."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % align else t


def _dense_channels_last(t, align=POINTER_ALIGN):
    """_dense for a [B,C,H,W] tensor the kernel reads as [B,H,W,C]."""
    t = t.contiguous(memory_format=torch.channels_last)
    return t.clone(memory_format=torch.preserve_format) if t.data_ptr() % align else t


def _refuse(t, name, on=None, n=None, where=None, dtypes=(torch.float32,)):
    """The refusal rule of every tensor argument, in one place; returns t itself (whether it is copied is the caller's
    business).  Not on the GPU: RuntimeError; a dtype outside `dtypes` (None: any): TypeError; on another device than `on`,
    the tensor whose device and stream the call uses, or another element count than n, the one the kernel indexes:
    ValueError.  Attribute reads on the host only."""
    if not t.is_cuda:
        raise RuntimeError('%s must live on the GPU (no CPU path in nerf_from_image_amd)' % name)
    if dtypes is not None and t.dtype not in dtypes:
        raise TypeError('%s must be %s, got %s' % (name, ' / '.join(str(d)[len('torch.'):] for d in dtypes), t.dtype))
    if on is not None and t.device != on.device:
        raise ValueError('%s: %s lives on %s, the call runs on %s' % (where or name, name, t.device, on.device))
    if n is not None and t.numel() != n:
        raise ValueError('%s: %s must hold %d elements, got %s' % (where or name, name, n, list(t.shape)))
    return t


def _f32c(t, name, on=None, n=None, where=None, align=POINTER_ALIGN):
    """t as a dense, `align`-byte aligned float32 tensor on the GPU (refused by _refuse's rule, copied if it is not dense
    and aligned; None stays None).  No launch for a dense, aligned argument."""
    if t is None:
        return None
    t = _refuse(t, name, on, n, where).contiguous()            # (_dense, written out: a call comes through here per argument)
    return t.clone() if t.data_ptr() % align else t


def _nchw_or_nhwc(t):
    """(the tensor a kernel reads, its layout code) for an image [B,C,H,W] that is read in place in either layout: t
    itself and 0 (SSIM_BCHW, FILTER_BCHW) if it is dense, t itself and 1 (SSIM_BHWC, FILTER_BHWC) if it is dense as
    [B,H,W,C] behind a permute, else a contiguous copy and 0."""
    if t.is_contiguous():
        return t, 0
    if t.permute(0, 2, 3, 1).is_contiguous():
        return t, 1
    return t.contiguous(), 0


def _texels(texels, n_scenes, on, where, fp32_only=False):
    """(texels, dtype code, layout code) for a kernel: on the device of `on`, float32 / bfloat16 / float16 (fp32_only:
    float32), at least n_scenes scenes, and DENSE in the layout its shape claims - a view of the right shape over other
    strides (a permute of the other layout, a slice of a wider buffer) or at an unaligned offset is copied, as every other
    argument is, never read as if it were dense."""
    _refuse(texels, 'texels', on, where=where, dtypes=(torch.float32,) if fp32_only else tuple(_TEXEL_TORCH.values()))
    tdt = texel_dtype_of(texels)
    layout = texel_layout_of(texels)
    if texels.shape[0] < n_scenes:
        raise ValueError('%s: texels of %d scene(s) where %d are indexed' % (where, texels.shape[0], n_scenes))
    return _dense(texels), tdt, layout


@functools.lru_cache(maxsize=None)
def _decoder_image_floats(viewdir):
    lib = _lib.load()
    return int(lib.nfi_decoder_image_floats_viewdir() if viewdir else lib.nfi_decoder_image_floats())


def _decoder_image(image, viewdir, on, where):
    """The operand image of decoder_pack (viewdir: of decoder_pack_viewdir): dense float32 on the device of `on`, exactly as
    long as the kernels read it - the image of the other decoder kind is refused, not read past its end."""
    if image is None:
        raise ValueError('%s: decoder_image is missing' % where)
    try:
        return _f32c(image, 'decoder_image', on, _decoder_image_floats(bool(viewdir)), where)
    except ValueError as e:
        raise ValueError('%s (the image of %s is expected)' % (e, 'decoder_pack_viewdir' if viewdir else 'decoder_pack')) from None


def _need(t, n, tail, name, where):
    """Refuse (ValueError, before any launch) a tensor that does not hold n rows of trailing shape `tail`: the kernels index
    by the shapes of depth / bins alone, so a shorter argument would be read past its end."""
    tail = tuple(tail)
    rows = 1
    for d in t.shape[:t.dim() - len(tail)]:
        rows *= d
    if t.dim() < len(tail) or tuple(t.shape[t.dim() - len(tail):]) != tail or rows != n:
        raise ValueError('%s: %s must be %d rows of %s, got %s' % (where, name, n, list(tail), list(t.shape)))


def _one_device(where, on, *tensors):
    """Refuse (ValueError) a call whose tensors do not all live on the device of `on`, the tensor whose stream is used."""
    for t in tensors:
        if torch.is_tensor(t) and t.device != on.device:        # (the name is put together for a refusal only)
            _refuse(t, 'an argument of shape %s' % list(t.shape), on, where=where, dtypes=None)


def _points(points, where):
    points = _f32c(points, 'points')
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError('%s: points must be [B,P,3], got %s' % (where, tuple(points.shape)))
    return points


def _attention(attention_values, n_attention, n_scenes, on, where):
    """attention_values [>= n_scenes, A, 3] for A = n_attention > 0, else None (the argument is then not looked at)."""
    if n_attention <= 0:
        return None
    att = _f32c(attention_values, 'attention_values', on, where=where)
    if att is None or att.dim() != 3 or att.shape[0] < n_scenes or tuple(att.shape[1:]) != (n_attention, 3):
        raise ValueError('%s: attention_values must be [%d or more, %d, 3], got %s' % (
            where, n_scenes, n_attention, None if att is None else tuple(att.shape)))
    return att


def _need_rays(rd, n, where):
    if rd.shape[-1] != 3 or rd.numel() != 3 * n:
        raise ValueError('%s: ray_directions must hold %d rays of 3 components, got %s' % (where, n, list(rd.shape)))


# --------------------------------------------------------------------------- #
def planes_to_texels(planes, texel_dtype=TEXEL_F32):
    """planes [B,3,32,R,R] fp32 -> texels [B,3,R,R,32] (fp32 or bf16)."""
    planes = _f32c(planes, 'planes')
    if planes.dim() != 5:
        raise ValueError('planes must be [B,3,32,R,R], got %s' % (tuple(planes.shape),))
    B, three, C, R, R2 = planes.shape
    if three != 3 or C != 32 or R != R2:
        raise ValueError('planes must be [B,3,32,R,R], got %s' % (tuple(planes.shape),))
    dt = _TEXEL_TORCH[texel_dtype]
    texels = torch.empty((B, 3, R, R, 32), dtype=dt, device=planes.device)
    _launch_positional('nfi_planes_to_texels', planes, planes, texels, B, R, texel_dtype)
    return texels


def texels_to_planes(texels):
    """fp32 texels [B,3,R,R,32] -> planes [B,3,32,R,R] (adjoint layout change for gradients)."""
    texels = _f32c(texels, 'texels')
    if texel_layout_of(texels) != TEXELS_PLANAR:
        raise ValueError('texels_to_planes: planar texels [B,3,R,R,32] expected, got %s' % (tuple(texels.shape),))
    B, three, R, R2, C = texels.shape
    planes = torch.empty((B, 3, C, R, R), dtype=torch.float32, device=texels.device)
    _launch_positional('nfi_texels_to_planes', texels, texels, planes, B, R)
    return planes


def decoder_pack(w1, b1, w2, b2, n_attention, texel_dtype=TEXEL_F32):
    """Raw TriplanarDecoder parameters -> lane-ordered MFMA operand image (fp32 [3152])."""
    w1 = _f32c(w1, 'w1')
    b1, w2, b2 = (_f32c(t, n, w1, where='decoder_pack') for t, n in ((b1, 'b1'), (w2, 'w2'), (b2, 'b2')))
    n_out = 1 + n_attention if n_attention > 0 else 4
    if tuple(w1.shape) != (64, 32) or tuple(b1.shape) != (64,) or tuple(w2.shape) != (n_out, 64) \
            or tuple(b2.shape) != (n_out,):
        raise ValueError('decoder shapes must be [64,32],[64],[%d,64],[%d]; got %s %s %s %s' % (
            n_out, n_out, tuple(w1.shape), tuple(b1.shape), tuple(w2.shape), tuple(b2.shape)))
    image = torch.empty((_decoder_image_floats(False),), dtype=torch.float32, device=w1.device)
    _launch_positional('nfi_decoder_pack', w1, w1, b1, w2, b2, n_attention, texel_dtype, image)
    return image


RAY_FEATURE_PITCH = 48


def decoder_pack_viewdir(w1, b1, w2, b2, w3, b3, n_attention, texel_dtype=TEXEL_F32):
    """--use_viewdir decoder (33 outputs) + ViewDirectionMapper.output (w3, b3) -> operand image (fp32 [6016])."""
    w1 = _f32c(w1, 'w1')
    ts = [w1] + [_f32c(t, n, w1, where='decoder_pack_viewdir') for t, n in ((b1, 'b1'), (w2, 'w2'), (b2, 'b2'), (w3, 'w3'), (b3, 'b3'))]
    n3 = n_attention if n_attention > 0 else 3
    want = [(64, 32), (64,), (33, 64), (33,), (n3, 32), (n3,)]
    if [tuple(t.shape) for t in ts] != want:
        raise ValueError('view-direction decoder shapes must be %s; got %s' % (want, [tuple(t.shape) for t in ts]))
    image = torch.empty((_decoder_image_floats(True),), dtype=torch.float32, device=w1.device)
    _launch_positional('nfi_decoder_pack_viewdir', w1, *ts, n_attention, texel_dtype, image)
    return image


def pad_ray_features(x):
    """ViewDirectionMapper.fc6 output [..., 32] -> [..., 48] rows [0, x, 0 x 15] (the kernels' accumulator-row order)."""
    x = _f32c(x, 'ray_features')
    if x.shape[-1] != 32:
        raise ValueError('ray features must have 32 channels, got %s' % (tuple(x.shape),))
    return torch.nn.functional.pad(x, (1, RAY_FEATURE_PITCH - 33)).contiguous()


# --------------------------------------------------------------------------- #
def raygen(height, width, focal, cam2world, bbox=None, center=None, normalize=False):
    cam2world = _cameras(cam2world, 'raygen')
    B = cam2world.shape[0]
    dev = cam2world.device
    focal, bbox, center = _camera_extras(focal, bbox, center, cam2world, 'raygen')
    ro = torch.empty((B, height, width, 3), dtype=torch.float32, device=dev)
    rd = torch.empty_like(ro)
    _launch('nfi_raygen', 'nfi_raygen_args', cam2world, n_scenes=B, height=height, width=width, cam2world=cam2world,
            focal=focal, bbox=bbox, center=center, normalize=int(normalize), ray_origins=ro, ray_directions=rd)
    return ro, rd


def near_far(ray_origins, ray_directions, scene_range, strict=True):
    """Returns near, far (finished planes), hit (bool).  strict: True - raise when no ray hits, as the reference does
    (costs a device->host read of one counter); 'deferred' - no synchronisation, the counter is looked at by the next
    strict call on the device / flush_strict() (as in render_fwd); False - never raises."""
    ro = _f32c(ray_origins, 'ray_origins')
    if ro.dim() < 1 or ro.shape[-1] != 3:
        raise ValueError('near_far: ray_origins must be [...,3], got %s' % (tuple(ro.shape),))
    shape = ro.shape[:-1]
    n = ro.numel() // 3
    rd = _f32c(ray_directions, 'ray_directions', ro, 3 * n, 'near_far')
    dev = ro.device
    near_raw = torch.empty((n,), dtype=torch.float32, device=dev)
    far_raw = torch.empty_like(near_raw)
    near, far = torch.empty_like(near_raw), torch.empty_like(near_raw)
    hit = torch.empty((n,), dtype=torch.uint8, device=dev)
    red = torch.empty((4,), dtype=torch.int32, device=dev)
    _launch('nfi_near_far', 'nfi_near_far_args', ro, n_rays=n, ray_origins=ro, ray_directions=rd,
            scene_range=float(scene_range), near_raw=near_raw, far_raw=far_raw, hit=hit, reduce=red, near_plane=near,
            far_plane=far)
    if strict == 'deferred':
        _raise_pending(dev)
        _defer_hit_count(red[2:3], dev)
    elif strict and int(red[2].item()) == 0:
        raise RuntimeError(_NO_HIT)
    return near.view(shape), far.view(shape), (hit & 1).bool().view(shape)


def stratified_points(ray_origins, ray_directions, near, far, num_samples, noise=None, want_points=True):
    where = 'stratified_points'
    ro = _f32c(ray_origins, 'ray_origins')
    if ro.dim() < 1 or ro.shape[-1] != 3:
        raise ValueError('stratified_points: ray_origins must be [...,3], got %s' % (tuple(ro.shape),))
    shape = ro.shape[:-1]
    n = ro.numel() // 3
    rd = _f32c(ray_directions, 'ray_directions', ro, 3 * n, where)
    near, far = _f32c(near, 'near', ro, n, where), _f32c(far, 'far', ro, n, where)
    noise = _f32c(noise, 'noise', ro, n * num_samples, where)
    depth = torch.empty((*shape, num_samples), dtype=torch.float32, device=ro.device)
    points = torch.empty((*shape, num_samples, 3), dtype=torch.float32, device=ro.device) if want_points else None
    _launch('nfi_stratified_points', 'nfi_stratified_args', ro, n_rays=n, n_samples=num_samples, ray_origins=ro,
            ray_directions=rd, near_plane=near, far_plane=far, noise=noise, depth=depth, points=points)
    return points, depth


def points_on_rays(ray_origins, ray_directions, depth):
    depth = _f32c(depth, 'depth')
    S = depth.shape[-1]
    n = depth.numel() // S
    ro = _f32c(ray_origins, 'ray_origins', depth, 3 * n, 'points_on_rays')
    rd = _f32c(ray_directions, 'ray_directions', depth, 3 * n, 'points_on_rays')
    points = torch.empty((*depth.shape, 3), dtype=torch.float32, device=depth.device)
    _launch_positional('nfi_points_on_rays', depth, ro, rd, depth, n, S, points)
    return points


# --------------------------------------------------------------------------- #
def field_query(points, texels, decoder_image, scene_range, n_attention, attention_values=None, use_sdf=True,
                beta=None, alpha=None, want_sdf=False, want_semantics=False, want_outside=False,
                ray_features=None, samples_per_ray=0, mlp_precision=0):
    """points [B,P,3] -> dict(sigma [B,P], rgb [B,P,3], sdf?, semantics?, outside?).
    mlp_precision: 0 exact fp32 MFMA, 1 split-fp16 operands (the fused renderer's arithmetic; not with ray_features).
    ray_features: padded [B, P/samples_per_ray, 48] (pad_ray_features) with a decoder_pack_viewdir image."""
    where = 'field_query'
    points = _points(points, where)
    B, P = points.shape[0], points.shape[1]
    if ray_features is not None:
        ray_features = _f32c(ray_features, 'ray_features', points, where=where)
        if samples_per_ray <= 0 or P % samples_per_ray or \
                tuple(ray_features.shape) != (B, P // samples_per_ray, RAY_FEATURE_PITCH):
            raise ValueError('ray_features must be [B, P/samples_per_ray, 48]; got %s for P=%d, S=%d' % (
                tuple(ray_features.shape), P, samples_per_ray))
    dev = points.device
    texels, tdt, layout = _texels(texels, B, points, where)
    decoder_image = _decoder_image(decoder_image, ray_features is not None, points, where)
    att = _attention(attention_values, n_attention, B, points, where)
    beta, alpha = _f32c(beta if use_sdf else None, 'beta', points, 1, where), _f32c(alpha if use_sdf else None, 'alpha', points, 1, where)
    out = {'sigma': torch.empty((B, P), dtype=torch.float32, device=dev),
           'rgb': torch.empty((B, P, 3), dtype=torch.float32, device=dev)}
    if want_sdf:
        out['sdf'] = torch.empty((B, P), dtype=torch.float32, device=dev)
    if want_semantics:
        out['semantics'] = torch.empty((B, P, n_attention), dtype=torch.float32, device=dev)
    if want_outside:
        out['outside'] = torch.empty((B, P), dtype=torch.uint8, device=dev)
    _launch('nfi_field_query_fwd', 'nfi_field_args', points, n_scenes=B, points_per_scene=P, points=points, texels=texels,
            plane_res=texel_res(texels), texel_dtype=tdt, texel_layout=layout, decoder_image=decoder_image,
            n_attention=n_attention, attention_values=att, use_sdf=int(use_sdf), beta=beta, alpha=alpha,
            scene_range=float(scene_range), sigma=out['sigma'], rgb=out['rgb'], sdf=out.get('sdf'),
            semantics=out.get('semantics'), outside=out.get('outside'), ray_features=ray_features,
            samples_per_ray=int(samples_per_ray), mlp_precision=int(mlp_precision))
    return out


def bbox_overlay(points, sigma, scene_range):
    """sigma + 100 on the wire frame of the scene cube (generator.py:645-659)."""
    import numpy as np
    sigma = _f32c(sigma, 'sigma')
    points = _f32c(points, 'points', sigma, where='bbox_overlay')
    n = sigma.numel()
    if points.numel() != 3 * n:
        raise ValueError('bbox_overlay: points %s do not match sigma %s' % (tuple(points.shape), tuple(sigma.shape)))
    out = torch.empty_like(sigma)
    thr = float(np.float32(scene_range - 5e-2))          # `x < scene_range - eps` against an fp32 tensor
    _launch_positional('nfi_bbox_overlay', sigma, points, n, float(scene_range), thr, sigma, out)
    return out


# --------------------------------------------------------------------------- #
def ray_weights(sigma, ray_directions, depth):
    depth = _f32c(depth, 'depth')
    sigma, rd = _f32c(sigma, 'sigma', depth, where='ray_weights'), _f32c(ray_directions, 'ray_directions', depth, where='ray_weights')
    S = depth.shape[-1]
    n = depth.numel() // S
    _need(sigma, n, (S,), 'sigma', 'ray_weights')
    _need_rays(rd, n, 'ray_weights')
    w = torch.empty_like(depth)
    _launch('nfi_ray_weights', 'nfi_weights_args', depth, n_rays=n, n_samples=S, sigma=sigma, ray_directions=rd,
            depth=depth, weights=w)
    return w


def _u_and_stride(u, n, k, where, on):
    """(u, its row stride) for u [n,k] dense (copied if not), or a stride-0 broadcast of one row, read in place; float32
    on the device of `on`."""
    _refuse(u, 'u', on, where=where)
    if u.shape[-1] != k:
        raise ValueError('%s: u must have %d entries per ray, got %s' % (where, k, list(u.shape)))
    if u.dim() == 2 and u.stride(0) == 0 and u.stride(1) == 1 and u.data_ptr() % POINTER_ALIGN == 0:
        return u, 0
    if u.numel() != n * k:
        raise ValueError('%s: u must hold one row per ray ([%d,%d]) or broadcast one row with stride 0, got %s' % (
            where, n, k, list(u.shape)))
    return _dense(u), k


def sample_pdf(bins, weights, u, want_inds=False, want_cdf=False):
    bins = _f32c(bins, 'bins')
    weights = _f32c(weights, 'weights', bins, where='sample_pdf')
    if bins.dim() != 2:
        raise ValueError('sample_pdf: bins must be [n,M], got %s' % (list(bins.shape),))
    n, M = bins.shape
    _need(weights, n, (M - 1,), 'weights', 'sample_pdf')
    K = u.shape[-1]
    u, stride = _u_and_stride(u, n, K, 'sample_pdf', bins)
    dev = bins.device
    samples = torch.empty((n, K), dtype=torch.float32, device=dev)
    inds = torch.empty((n, K), dtype=torch.int64, device=dev) if want_inds else None
    cdf = torch.empty((n, M), dtype=torch.float32, device=dev) if want_cdf else None
    _launch('nfi_sample_pdf', 'nfi_sample_pdf_args', bins, n_rays=n, n_bins=M, n_samples=K, bins=bins, weights=weights,
            u=u, u_row_stride=stride, samples=samples, inds=inds, cdf=cdf)
    return samples, inds, cdf


def resample(sigma, ray_directions, depth, u, want_taps=False):
    depth = _f32c(depth, 'depth')
    sigma, rd = _f32c(sigma, 'sigma', depth, where='resample'), _f32c(ray_directions, 'ray_directions', depth, where='resample')
    S = depth.shape[-1]
    n = depth.numel() // S
    _need(sigma, n, (S,), 'sigma', 'resample')
    _need_rays(rd, n, 'resample')
    if u.shape[-1] != S:
        raise ValueError('resample: u must have %d entries per ray, got %s' % (S, list(u.shape)))
    u, stride = _u_and_stride(u.reshape(-1, S) if u.stride(0) != 0 else u, n, S, 'resample', depth)
    dev = depth.device
    fine = torch.empty((n, S), dtype=torch.float32, device=dev)
    taps = {}
    if want_taps:
        taps = dict(weights=torch.empty((n, S), dtype=torch.float32, device=dev),
                    smooth=torch.empty((n, S), dtype=torch.float32, device=dev),
                    cdf=torch.empty((n, S - 1), dtype=torch.float32, device=dev),
                    inds=torch.empty((n, S), dtype=torch.int64, device=dev))
    _launch('nfi_resample', 'nfi_resample_args', depth, n_rays=n, n_samples=S, sigma=sigma, ray_directions=rd, depth=depth,
            u=u, u_row_stride=stride, fine_depth=fine, **taps)
    return fine, taps


def _check_lists(where, rd, depth_a, sigma_a, rgb_a, depth_b, sigma_b, rgb_b, extra_a, extra_b):
    """The shape rules of composite / composite_bwd (ValueError before any launch): every per-sample argument follows its
    depth list, both lists and the directions hold the same rays, an extra attribute comes for every list."""
    na = depth_a.shape[-1]
    n = depth_a.numel() // na
    _one_device(where, rd, depth_a, sigma_a, rgb_a, depth_b, sigma_b, rgb_b, extra_a, extra_b)
    _need_rays(rd, n, where)
    _need(sigma_a, n, (na,), 'sigma_a', where)
    _need(rgb_a, n, (na, 3), 'rgb_a', where)
    if depth_b is not None:
        if sigma_b is None or rgb_b is None:
            raise ValueError('%s: list b needs depth_b, sigma_b and rgb_b' % where)
        nb = depth_b.shape[-1]
        _need(depth_b, n, (nb,), 'depth_b', where)
        _need(sigma_b, n, (nb,), 'sigma_b', where)
        _need(rgb_b, n, (nb, 3), 'rgb_b', where)
    if extra_a is not None:
        _need(extra_a, n, (na, extra_a.shape[-1]), 'extra_a', where)
        if depth_b is not None:
            if extra_b is None:
                raise ValueError('%s: extra_a comes with a list b, but extra_b is missing' % where)
            _need(extra_b, n, (nb, extra_a.shape[-1]), 'extra_b', where)
    return n


def _lists(where, ray_directions, depth_a, sigma_a, rgb_a, depth_b, sigma_b, rgb_b, extra_a, extra_b):
    """The directions and the sample lists of composite / composite_bwd as dense float32, checked by _check_lists:
    (rays, samples of list a, of list b, extra channels), (ray_directions, depth_a, sigma_a, rgb_a, depth_b, sigma_b, rgb_b,
    extra_a, extra_b).  Without depth_b there is no list b, without extra_a no extras: those come back None."""
    rd = _f32c(ray_directions, 'ray_directions')
    depth_a, sigma_a, rgb_a = _f32c(depth_a, 'depth'), _f32c(sigma_a, 'sigma'), _f32c(rgb_a, 'rgb')
    if depth_b is None:
        sigma_b = rgb_b = None
    depth_b, sigma_b, rgb_b = _f32c(depth_b, 'depth_b'), _f32c(sigma_b, 'sigma_b'), _f32c(rgb_b, 'rgb_b')
    extra_a = _f32c(extra_a, 'extra_a')
    extra_b = _f32c(extra_b, 'extra_b') if extra_a is not None and depth_b is not None else None
    tensors = (rd, depth_a, sigma_a, rgb_a, depth_b, sigma_b, rgb_b, extra_a, extra_b)
    n = _check_lists(where, *tensors)
    return (n, depth_a.shape[-1], 0 if depth_b is None else depth_b.shape[-1], 0 if extra_a is None else extra_a.shape[-1]), tensors


def composite(ray_directions, depth_a, sigma_a, rgb_a, depth_b=None, sigma_b=None, rgb_b=None, extra_a=None,
              extra_b=None, white_background=True, want_taps=False):
    (n, na, nb, n_extra), (rd, depth_a, sigma_a, rgb_a, depth_b, sigma_b, rgb_b, extra_a, extra_b) = _lists(
        'composite', ray_directions, depth_a, sigma_a, rgb_a, depth_b, sigma_b, rgb_b, extra_a, extra_b)
    dev = depth_a.device
    shape = depth_a.shape[:-1]
    rgb_map = torch.empty((*shape, 3), dtype=torch.float32, device=dev)
    depth_map = torch.empty(shape, dtype=torch.float32, device=dev)
    mask = torch.empty(shape, dtype=torch.float32, device=dev)
    extra_map = torch.empty((*shape, n_extra), dtype=torch.float32, device=dev) if n_extra else None
    taps = {}
    if want_taps:
        taps = dict(weights=torch.empty((*shape, na + nb), dtype=torch.float32, device=dev),
                    depth_sorted=torch.empty((*shape, na + nb), dtype=torch.float32, device=dev),
                    perm=torch.empty((*shape, na + nb), dtype=torch.int64, device=dev))
    _launch('nfi_composite_fwd', 'nfi_composite_args', depth_a, n_rays=n, n_a=na, n_b=nb, ray_directions=rd, depth_a=depth_a,
            sigma_a=sigma_a, rgb_a=rgb_a, depth_b=depth_b, sigma_b=sigma_b, rgb_b=rgb_b, n_extra=n_extra, extra_a=extra_a,
            extra_b=extra_b, white_background=int(white_background), rgb_map=rgb_map, depth_map=depth_map, mask=mask,
            extra_map=extra_map, **taps)
    return rgb_map, depth_map, mask, extra_map, taps


# --------------------------------------------------------------------------- #
def _cameras(cam2world, where):
    cam2world = _f32c(cam2world, 'tform_cam2world')
    if cam2world.dim() != 3 or tuple(cam2world.shape[1:]) != (4, 4):
        raise ValueError('%s: tform_cam2world must be [B,4,4], got %s' % (where, tuple(cam2world.shape)))
    return cam2world


def _camera_extras(focal, bbox, center, cam2world, where):
    """focal [B], bbox [B,2,2], center [B,2] (each may be None) on the cameras' device."""
    B = cam2world.shape[0]
    return (_f32c(focal, 'focal_length', cam2world, B, where), _f32c(bbox, 'bbox', cam2world, 4 * B, where),
            _f32c(center, 'center', cam2world, 2 * B, where))


TAP_NAMES = ('ray_origins', 'ray_directions', 'near_plane', 'far_plane', 'hit', 't_coarse', 'sigma_coarse',
             'rgb_coarse', 't_fine', 'sigma_fine', 'rgb_fine', 't_sorted', 'weights', 'perm')


def render_setup(cam2world, focal, height, width, scene_range, bbox=None, center=None, workspace=None, row_window=None):
    """The ray set-up of render_fwd alone (nfi_render_setup) into `workspace` (allocated when None; returned).  A
    render_fwd(..., workspace=that, rays_ready=True) with the same cameras / shape / scene_range / row_window then launches
    the render kernel only - e.g. with the set-up of the next batch running on another stream meanwhile.  (Not for calls
    that ask for the ray_origins / ray_directions taps or the training stash: those write rays to their own tensors.)"""
    lib = _lib.load()
    cam2world = _cameras(cam2world, 'render_setup')
    dev = cam2world.device
    B = cam2world.shape[0]
    n = B * height * width
    focal, bbox, center = _camera_extras(focal, bbox, center, cam2world, 'render_setup')
    ws_bytes = lib.nfi_render_workspace_bytes(n)
    if workspace is None or workspace.numel() < ws_bytes:
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    _one_device('render_setup', cam2world, workspace)
    _launch('nfi_render_setup', 'nfi_render_args', cam2world, n_scenes=B, height=height, width=width,
            scene_range=float(scene_range), cam2world=cam2world, focal=focal, bbox=bbox, center=center, workspace=workspace,
            workspace_bytes=workspace.numel(), row_offset=0 if row_window is None else int(row_window[0]),
            full_height=0 if row_window is None else int(row_window[1]))
    return workspace


def render_fwd(cam2world, focal, height, width, num_samples, texels, decoder_image, scene_range, n_attention,
               attention_values=None, use_sdf=True, beta=None, alpha=None, bbox=None, center=None,
               noise_coarse=None, noise_fine=None, fine_sampling=True, white_background=True, taps=(),
               skip_missed_rays=True, workspace=None, events=None, tuning=0, profile_cycles=None, ray_features=None,
               termination_eps=0.0, row_window=None, clock_probe=None, stash=False, rays_ready=False,
               want_semantics=False, want_coords=False, want_normals=False, strict=False, views_per_scene=1):
    """Fused forward render.  Returns dict(rgb [B,H,W,3], depth, mask [B,H,W], + requested taps).
    views_per_scene: V >= 1 images per scene, scene-major: image i (camera i, noise rows i, output rows i; B of them, a
    multiple of V) reads the texels and attention rows of scene i // V, so `texels` / `attention_values` hold B / V
    scenes - bit for bit the result of V = 1 with both repeat_interleave(V, 0).  Whatever V, a call whose texels or
    attention values hold fewer scenes than its cameras need is refused (ValueError) before any launch.
    row_window: None, or (row_offset, full_height): `height` rows starting at row_offset of an image full_height rows tall
    (bit-identical to those rows of the full render; noise / outputs / taps are sized for the window).
    clock_probe: None or a uint64 / int64 [2] device tensor receiving {shader cycles, 100 MHz ticks} of the render kernel.
    stash: also return the training stash 'stash_t' [B,H,W,2S], 'stash_sigma' [B,H,W,2S], 'stash_rgb' [B,H,W,2S,3]
    (coarse samples in [..., :S], fine in [..., S:], source order; skipped rays hold zeros; without fine sampling the
    rows hold the S samples of the single pass) and 'ray_origins' /
    'ray_directions' - what composite_bwd(list_row_stride=2S) + field_query_bwd need for the backward of the render.
    ray_features: padded [B,H,W,48] per-ray view-direction features (decoder_pack_viewdir image).
    termination_eps: 0 = off; eps in (0,1): fine samples behind the depth at which the COARSE transmittance has fallen
    below eps are not evaluated and the rest is compacted by wave ballot (the coarse pass, the pdf and every sample index
    are untouched; |d rgb| <= ~eps, see include/nfi_hip.h).
    strict: True - raise when no ray of the batch meets the scene cube, as the reference does (lib/nerf_utils.py:258 fails
    on min() of an empty selection): the ray set-up runs as its own launch and its hit counter is read back before the
    render kernel is launched (one host synchronisation, on the set-up only - the reference synchronises at the same
    place, its boolean indexing at nerf_utils.py:258; the device idles for that host round trip, and `events` /
    `clock_probe` then bracket the render kernel WITHOUT the ray set-up); 'after' - one launch, the counter is read
    back behind the render kernel (no gap between set-up and render; the host waits for the whole render);
    'deferred' - no synchronisation: the counter is copied to pinned memory behind the render and checked by the next
    strict call / flush_strict().
    want_semantics / want_coords: also return 'semantics' [B,H,W,A] (composited softmax probabilities, run.py:312-335)
    / 'coords' [B,H,W,3] (composited query points, run.py:337-338) / 'normals' [B,H,W,3] (composited unit normals of the
    SDF, + 1 - mask on a white background, lib/nerf_utils.py:149-151, 159; any texel storage; with ray_features: fp32
    texels) from the SAME launch.
    Precision of 'semantics': with num_samples <= 64 the per-sample probabilities wait for the compositing in fp32; the
    64 < num_samples <= 128 kernel parks them as unorm16 (|error| <= 2^-17 = 7.7e-6 per sample, values below that become
    0) and scales the composited map to sum to the mask, so its map is within 1e-5 of the reference's instead of 1e-6
    (tests/test_hip_parity.py, test_wide_kernel_semantics_table_precision; tests/test_kernel_matrix.py for A = 14)."""
    where = 'render_fwd'
    cam2world = _cameras(cam2world, where)
    B = cam2world.shape[0]
    dev = cam2world.device
    n = B * height * width
    S = num_samples
    V = int(views_per_scene)
    if V < 1 or B % V != 0:
        raise ValueError('render_fwd: %d cameras are not a multiple of views_per_scene = %d (>= 1)' % (B, V))
    if texels.shape[0] * V < B:
        raise ValueError('render_fwd: texels of %d scene(s) x views_per_scene %d do not cover %d cameras' % (
            texels.shape[0], V, B))
    if n_attention > 0 and (attention_values is None or attention_values.shape[0] * V < B):
        raise ValueError('render_fwd: attention_values of %d scene(s) x views_per_scene %d do not cover %d cameras' % (
            0 if attention_values is None else attention_values.shape[0], V, B))
    lib = _lib.load()
    texels, tdt, layout = _texels(texels, B // V, cam2world, where)
    decoder_image = _decoder_image(decoder_image, ray_features is not None, cam2world, where)
    att = _attention(attention_values, n_attention, B // V, cam2world, where)
    focal, bbox, center = _camera_extras(focal, bbox, center, cam2world, where)
    beta, alpha = _f32c(beta if use_sdf else None, 'beta', cam2world, 1, where), _f32c(alpha if use_sdf else None, 'alpha', cam2world, 1, where)
    noise_coarse = _f32c(noise_coarse, 'noise_coarse', cam2world, n * S, where)
    out = {'rgb': torch.empty((B, height, width, 3), dtype=torch.float32, device=dev),
           'depth': torch.empty((B, height, width), dtype=torch.float32, device=dev),
           'mask': torch.empty((B, height, width), dtype=torch.float32, device=dev)}
    n2 = 2 * S if fine_sampling else S
    shapes = {'ray_origins': ((B, height, width, 3), torch.float32), 'ray_directions': ((B, height, width, 3), torch.float32),
              'near_plane': ((B, height, width), torch.float32), 'far_plane': ((B, height, width), torch.float32),
              'hit': ((B, height, width), torch.uint8),
              't_coarse': ((B, height, width, S), torch.float32), 'sigma_coarse': ((B, height, width, S), torch.float32),
              'rgb_coarse': ((B, height, width, S, 3), torch.float32),
              't_fine': ((B, height, width, S), torch.float32), 'sigma_fine': ((B, height, width, S), torch.float32),
              'rgb_fine': ((B, height, width, S, 3), torch.float32),
              't_sorted': ((B, height, width, n2), torch.float32), 'weights': ((B, height, width, n2), torch.float32),
              'perm': ((B, height, width, n2), torch.int32)}
    tap_t = {}
    for name in taps:
        if name not in shapes:
            raise KeyError('unknown tap %s' % name)
        if not fine_sampling and name in ('t_fine', 'sigma_fine', 'rgb_fine', 'perm'):
            continue
        shp, dt = shapes[name]
        tap_t[name] = torch.zeros(shp, dtype=dt, device=dev)
    if stash:
        for name in ('ray_origins', 'ray_directions'):
            tap_t.setdefault(name, torch.empty(shapes[name][0], dtype=torch.float32, device=dev))
        tap_t['stash_t'] = torch.empty((B, height, width, n2), dtype=torch.float32, device=dev)
        tap_t['stash_sigma'] = torch.empty((B, height, width, n2), dtype=torch.float32, device=dev)
        tap_t['stash_rgb'] = torch.empty((B, height, width, n2, 3), dtype=torch.float32, device=dev)
    if want_semantics:
        if n_attention <= 0:
            raise ValueError('render_fwd: semantics need attention values (n_attention > 0)')
        tap_t['semantics'] = torch.empty((B, height, width, n_attention), dtype=torch.float32, device=dev)
    if want_coords:
        tap_t['coords'] = torch.empty((B, height, width, 3), dtype=torch.float32, device=dev)
    if want_normals:
        if not use_sdf:
            raise ValueError('render_fwd: the normals map needs the SDF decoder (use_sdf)')
        tap_t['normals'] = torch.empty((B, height, width, 3), dtype=torch.float32, device=dev)
    ws_bytes = lib.nfi_render_workspace_bytes(n)
    check_after = False
    if strict == 'deferred':
        _raise_pending(dev)                      # an EARLIER batch of this device that met no ray
    elif strict == 'after':
        check_after = True
    elif strict:
        if not rays_ready and not stash and not any(name in tap_t for name in ('ray_origins', 'ray_directions', 'hit')):
            # the ray set-up as its own launch, its hit count read back BEFORE the render kernel goes out: the host waits
            # for the set-up only, and a batch without a hit never pays for a render
            workspace = render_setup(cam2world, focal, height, width, scene_range, bbox=bbox, center=center,
                                     workspace=workspace, row_window=row_window)
            rays_ready = True
        if rays_ready and workspace is not None and workspace.numel() >= ws_bytes:
            _raise_if_no_hit(workspace)
        else:
            check_after = True                   # (stash / ray taps: the set-up writes rays to the caller's tensors)
    if rays_ready:
        # the kernel would march whatever the workspace holds: refuse anything that is not nfi_render_setup's own result
        if workspace is None or workspace.numel() < ws_bytes:
            raise ValueError('render_fwd(rays_ready=True) needs the workspace render_setup filled (%d bytes)' % ws_bytes)
        if stash or any(name in tap_t for name in ('ray_origins', 'ray_directions', 'hit')):
            raise ValueError('render_fwd(rays_ready=True) cannot be combined with the stash or the ray_origins / '
                             'ray_directions / hit taps (they redirect the ray set-up away from the workspace)')
    if workspace is None or workspace.numel() < ws_bytes:
        workspace = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    if fine_sampling:
        if noise_fine is None:
            noise_fine = torch.linspace(0.0, 1.0, steps=S, dtype=torch.float32, device=dev).expand(n, S)
        u, ustride = _u_and_stride(noise_fine if noise_fine.dim() == 2 else noise_fine.reshape(-1, S), n, S, where, cam2world)
    else:
        u, ustride = None, 0
    if ray_features is not None:
        ray_features = _f32c(ray_features, 'ray_features', cam2world, where=where)
        if ray_features.numel() != n * RAY_FEATURE_PITCH:
            raise ValueError('ray_features must be [B,H,W,48], got %s' % (tuple(ray_features.shape),))
    _one_device(where, cam2world, workspace, profile_cycles, clock_probe)
    _launch('nfi_render_fwd', 'nfi_render_args', cam2world, n_scenes=B, height=height, width=width,
            n_samples=S, fine_sampling=int(fine_sampling), white_background=int(white_background),
            scene_range=float(scene_range), views_per_scene=V, cam2world=cam2world, focal=focal,
            bbox=bbox, center=center, texels=texels, plane_res=texel_res(texels),
            texel_layout=layout, texel_dtype=tdt, decoder_image=decoder_image, n_attention=n_attention,
            attention_values=att, use_sdf=int(use_sdf), beta=beta, alpha=alpha, noise_coarse=noise_coarse,
            noise_fine=u, noise_fine_row_stride=ustride, rgb=out['rgb'], depth=out['depth'], mask=out['mask'],
            workspace=workspace, workspace_bytes=workspace.numel(), skip_missed_rays=int(skip_missed_rays),
            event_start=None if events is None else events[0], event_stop=None if events is None else events[1],
            tuning=int(tuning), profile_cycles=profile_cycles, ray_features=ray_features,
            termination_eps=float(termination_eps), clock_probe=clock_probe,
            row_offset=0 if row_window is None else int(row_window[0]),
            full_height=0 if row_window is None else int(row_window[1]), rays_ready=int(bool(rays_ready)), **tap_t)
    out.update(tap_t)
    out['_workspace'] = workspace
    if strict == 'deferred':
        _defer_hit_count(workspace, dev)
    elif check_after:
        _raise_if_no_hit(workspace)
    return out


_NO_HIT = ('compute_near_far_planes: no ray intersects the scene cube (the reference fails on min() of an empty '
           'selection here)')
_PENDING = {}          # device index -> dict(host=pinned int32 ring, slot, queue=[(event, slot)]); one thread per device


def _raise_if_no_hit(workspace):
    if int(workspace[8:12].view(torch.int32).item()) == 0:      # the hit count of the ray set-up (csrc: reduce[2])
        raise RuntimeError(_NO_HIT)


def _dev_key(dev):
    """The device's index; torch.device('cuda') (index None) is the current device - the key the tensors' own device has."""
    return torch.cuda.current_device() if dev.index is None else dev.index


def _defer_hit_count(source, dev):
    """strict='deferred': the hit count goes to pinned host memory behind the render (async copy + event), no wait.
    source: the render workspace (uint8; the count is its third int32) or the int32 [1] count itself."""
    st = _PENDING.setdefault(_dev_key(dev), {'host': torch.zeros(64, dtype=torch.int32).pin_memory(), 'slot': 0, 'queue': []})
    if len(st['queue']) >= 64:
        _raise_pending(dev, wait=True)
    slot = st['slot']
    st['slot'] = (slot + 1) % 64
    count = source[8:12].view(torch.int32) if source.dtype == torch.uint8 else source
    st['host'][slot:slot + 1].copy_(count, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    st['queue'].append((ev, slot))


def _raise_pending(dev, wait=False):
    st = _PENDING.get(_dev_key(dev))
    while st and st['queue']:
        ev, slot = st['queue'][0]
        if not ev.query():
            if not wait:
                return
            ev.synchronize()
        st['queue'].pop(0)
        if int(st['host'][slot]) == 0:
            st['queue'].clear()
            raise RuntimeError(_NO_HIT + ' [an earlier batch, strict_near_far="deferred"]')


def flush_strict(device=None):
    """strict='deferred': waits for the hit counts still in flight on `device` (default: the current one) and raises if
    one of those batches met no ray.  Call it where a loop synchronises anyway (end of an epoch, before a report)."""
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    _raise_pending(dev, wait=True)


# --------------------------------------------------------------------------- #
# regulariser branch: distance + spatial gradient as one operator
# --------------------------------------------------------------------------- #
def sdf_gradient_fwd(points, texels, w1, b1, w2, b2, scene_range):
    """points [B,P,3] (inside the cube) -> (sdf [B,P], d sdf / d points [B,P,3])."""
    where = 'sdf_gradient_fwd'
    points = _points(points, where)
    B, P = points.shape[0], points.shape[1]
    texels, _, layout = _texels(texels, B, points, where, fp32_only=True)
    w1, b1, w2, b2 = _distance_head(w1, b1, w2, b2, points, where)
    sdf = torch.empty((B, P), dtype=torch.float32, device=points.device)
    grad = torch.empty((B, P, 3), dtype=torch.float32, device=points.device)
    _launch('nfi_sdf_gradient_fwd', 'nfi_sdf_gradient_args', points, n_scenes=B, points_per_scene=P, points=points,
            texels=texels, plane_res=texel_res(texels), texel_layout=layout, scene_range=float(scene_range), w1=w1, b1=b1,
            w2=w2, b2=b2, sdf=sdf, gradient=grad)
    return sdf, grad


def _distance_head(w1, b1, w2, b2, on, where):
    """Raw decoder parameters of the regulariser: w1 [64,32], b1 [64], w2 [n_out,64], b2 [n_out] (row 0 is the distance)."""
    w1, b1 = _f32c(w1, 'w1', on, 64 * 32, where), _f32c(b1, 'b1', on, 64, where)
    w2, b2 = _f32c(w2, 'w2', on, where=where), _f32c(b2, 'b2', on, where=where)
    if w2.dim() != 2 or w2.shape[0] < 1 or w2.shape[1] != 64 or b2.numel() != w2.shape[0]:
        raise ValueError('%s: w2 must be [n_out,64] and b2 [n_out], got %s and %s' % (where, tuple(w2.shape), tuple(b2.shape)))
    return w1, b1, w2, b2


def sdf_gradient_bwd(points, texels, w1, b1, w2, b2, scene_range, g_sdf, g_gradient, ordered=False):
    """Backward (= the reference's double backward) of sdf_gradient_fwd.  Returns dict(g_texels, g_w1, g_b1, g_w2
    [n_out,64] with row 0 filled, g_b2 [n_out] with entry 0 filled).  ordered=True: nfi_sdf_gradient_bwd_ordered - the same
    contributions summed in a fixed order, every output bit-identical from launch to launch (a workspace is allocated
    per call)."""
    where = 'sdf_gradient_bwd'
    points = _points(points, where)
    B, P = points.shape[0], points.shape[1]
    dev = points.device
    texels, _, layout = _texels(texels, B, points, where, fp32_only=True)
    w1, b1, w2, b2 = _distance_head(w1, b1, w2, b2, points, where)
    # the gradient image is dense in the texels' layout whatever strides the caller's texels came with
    out = {'g_texels': torch.zeros(texels.shape, dtype=torch.float32, device=dev),
           'g_w1': torch.zeros((64, 32), dtype=torch.float32, device=dev),
           'g_b1': torch.zeros((64,), dtype=torch.float32, device=dev), 'g_w2': torch.zeros_like(w2),
           'g_b2': torch.zeros_like(b2)}
    args = dict(n_scenes=B, points_per_scene=P, points=points, texels=texels, plane_res=texel_res(texels),
                texel_layout=layout, scene_range=float(scene_range),
                w1=w1, b1=b1, w2=w2, b2=b2, g_sdf=_f32c(g_sdf, 'g_sdf', points, B * P, where),
                g_gradient=_f32c(g_gradient, 'g_gradient', points, 3 * B * P, where), **out)
    if ordered:
        _call_ordered('nfi_sdf_gradient_bwd_ordered', 'nfi_sdf_gradient_args', points,
                      'sdf_gradient_bwd(ordered=True, at most 2^25 points per scene)', (B, P, texel_res(texels)), args)
    else:
        _launch('nfi_sdf_gradient_bwd', 'nfi_sdf_gradient_args', points, **args)
    return out


# --------------------------------------------------------------------------- #
# backward wrappers
# --------------------------------------------------------------------------- #
def composite_bwd_stash(ray_directions, stash_t, stash_sigma, stash_rgb, g_rgb_map, g_mask=None, white_background=True,
                        want_rd=True, fine=True):
    """Compositing backward on the training stash of render_fwd (rows of 2S entries: coarse | fine; fine=False: rows of
    the S samples of a single pass).  Returns dict(g_sigma [..., 2S], g_rgb [..., 2S, 3], g_ray_directions?) in the
    stash's layout."""
    rd = _f32c(ray_directions, 'ray_directions')
    t, sg, col = _f32c(stash_t, 'stash_t'), _f32c(stash_sigma, 'stash_sigma'), _f32c(stash_rgb, 'stash_rgb')
    S2 = t.shape[-1]
    n = t.numel() // S2
    if not fine:
        g = composite_bwd(rd, t, sg, col, g_rgb_map, g_mask, white_background=white_background, want_rd=want_rd)
        out = dict(g_sigma=g['g_sigma_a'], g_rgb=g['g_rgb_a'])
        if want_rd:
            out['g_ray_directions'] = g['g_ray_directions']
        return out
    S = S2 // 2
    where = 'composite_bwd_stash'
    if S2 % 2:
        raise ValueError('%s: stash rows hold coarse | fine samples, an even count; got %d' % (where, S2))
    _one_device(where, rd, t, sg, col)
    _need_rays(rd, n, where)
    _need(sg, n, (S2,), 'stash_sigma', where)
    _need(col, n, (S2, 3), 'stash_rgb', where)
    g_rgb_map, g_mask = _f32c(g_rgb_map, 'g_rgb_map', rd, 3 * n, where), _f32c(g_mask, 'g_mask', rd, n, where)
    out = dict(g_sigma=torch.empty_like(sg), g_rgb=torch.empty_like(col))
    if want_rd:
        out['g_ray_directions'] = torch.empty_like(rd)
    f4 = 4              # bytes per float: list b starts S entries into every row
    _launch('nfi_composite_bwd', 'nfi_composite_bwd_args', rd, n_rays=n, n_a=S, n_b=S, list_row_stride=S2,
            ray_directions=rd, depth_a=t, sigma_a=sg, rgb_a=col, depth_b=t.data_ptr() + S * f4,
            sigma_b=sg.data_ptr() + S * f4, rgb_b=col.data_ptr() + 3 * S * f4, n_extra=0,
            white_background=int(white_background), g_rgb_map=g_rgb_map, g_mask=g_mask, g_sigma_a=out['g_sigma'],
            g_rgb_a=out['g_rgb'], g_sigma_b=out['g_sigma'].data_ptr() + S * f4,
            g_rgb_b=out['g_rgb'].data_ptr() + 3 * S * f4, g_ray_directions=out.get('g_ray_directions'))
    return out


def composite_bwd(ray_directions, depth_a, sigma_a, rgb_a, g_rgb_map, g_mask=None, depth_b=None, sigma_b=None,
                  rgb_b=None, extra_a=None, extra_b=None, g_extra_map=None, white_background=True, want_rd=True):
    # (the extras count only where their map has a gradient)
    (n, na, nb, n_extra), (rd, depth_a, sigma_a, rgb_a, depth_b, sigma_b, rgb_b, extra_a, extra_b) = _lists(
        'composite_bwd', ray_directions, depth_a, sigma_a, rgb_a, depth_b, sigma_b, rgb_b,
        extra_a if g_extra_map is not None else None, extra_b)
    g_rgb_map, g_mask = _f32c(g_rgb_map, 'g_rgb_map', rd, where='composite_bwd'), _f32c(g_mask, 'g_mask', rd, where='composite_bwd')
    g_extra_map = _f32c(g_extra_map, 'g_extra_map', rd, where='composite_bwd') if n_extra else None
    _need(g_rgb_map, n, (3,), 'g_rgb_map', 'composite_bwd')
    if g_mask is not None:
        _need(g_mask, n, (), 'g_mask', 'composite_bwd')
    if n_extra:
        _need(g_extra_map, n, (n_extra,), 'g_extra_map', 'composite_bwd')
    out = dict(g_sigma_a=torch.empty_like(sigma_a), g_rgb_a=torch.empty_like(rgb_a))
    if nb:
        out.update(g_sigma_b=torch.empty_like(sigma_b), g_rgb_b=torch.empty_like(rgb_b))
    if n_extra:
        out['g_extra_a'] = torch.empty_like(extra_a)
        if nb:
            out['g_extra_b'] = torch.empty_like(extra_b)
    if want_rd:
        out['g_ray_directions'] = torch.empty_like(rd)
    _launch('nfi_composite_bwd', 'nfi_composite_bwd_args', rd, n_rays=n, n_a=na, n_b=nb, ray_directions=rd, depth_a=depth_a,
            sigma_a=sigma_a, rgb_a=rgb_a, depth_b=depth_b, sigma_b=sigma_b, rgb_b=rgb_b, n_extra=n_extra, extra_a=extra_a,
            extra_b=extra_b, white_background=int(white_background), g_rgb_map=g_rgb_map, g_mask=g_mask,
            g_extra_map=g_extra_map, **out)
    return out


def points_bwd(g_points, depth, want_ro=True, want_rd=True):
    depth = _f32c(depth, 'depth')
    S = depth.shape[-1]
    n = depth.numel() // S
    g_points = _f32c(g_points, 'g_points', depth, 3 * n * S, 'points_bwd')
    shape = depth.shape[:-1]
    g_ro = torch.empty((*shape, 3), dtype=torch.float32, device=depth.device) if want_ro else None
    g_rd = torch.empty((*shape, 3), dtype=torch.float32, device=depth.device) if want_rd else None
    _launch_positional('nfi_points_bwd', depth, g_points, depth, n, S, g_ro, g_rd)
    return g_ro, g_rd


def raygen_bwd(height, width, focal, cam2world, bbox, center, normalize, g_ro, g_rd, ordered=False):
    """g_cam2world [B,4,4], g_focal [B] or None.  ordered: nfi_raygen_bwd_ordered - the same bits on every launch."""
    cam2world = _cameras(cam2world, 'raygen_bwd')
    B = cam2world.shape[0]
    focal, bbox, center = _camera_extras(focal, bbox, center, cam2world, 'raygen_bwd')
    n3 = 3 * B * height * width
    g_ro, g_rd = _f32c(g_ro, 'g_ro', cam2world, n3, 'raygen_bwd'), _f32c(g_rd, 'g_rd', cam2world, n3, 'raygen_bwd')
    g_cam = torch.empty((B, 4, 4), dtype=torch.float32, device=cam2world.device)
    g_focal = torch.empty((B,), dtype=torch.float32, device=cam2world.device) if focal is not None else None
    _launch('nfi_raygen_bwd_ordered' if ordered else 'nfi_raygen_bwd', 'nfi_raygen_args', cam2world, g_ro, g_rd, g_cam, g_focal,
            n_scenes=B, height=height, width=width, cam2world=cam2world, focal=focal, bbox=bbox, center=center,
            normalize=int(normalize))
    return g_cam, g_focal


# --------------------------------------------------------------------------- #
# neighbours of the renderer in the inversion loop
# --------------------------------------------------------------------------- #
def _warp_args(img, rot, scale, translation, white_background):
    n, c, h, w = img.shape
    rot, translation = _f32c(rot, 'rot', img, where='affine_warp'), _f32c(translation, 'translation', img, where='affine_warp')
    scale = _f32c(scale, 'scale', img, where='affine_warp')
    if rot.numel() != n or translation.numel() != 2 * n or (scale is not None and scale.numel() != n):
        raise ValueError('affine_warp: rot [N], scale [N] or None, translation [N,2] expected for N=%d images' % n)
    return dict(n_images=n, channels=c, height=h, width=w, rot=rot, scale=scale, translation=translation,
                white_background=int(bool(white_background)))


def affine_warp(img, rot, scale, translation, white_background=False):
    """img [N,C,H,W] warped by the per-image rotation / scale / translation of augment_impl (run.py:720-769)."""
    img = _f32c(img, 'img')
    if img.dim() != 4:
        raise ValueError('affine_warp: img must be [N,C,H,W]')
    out = torch.empty_like(img)
    _launch('nfi_affine_warp_fwd', 'nfi_warp_args', img, image=img, warped=out,
            **_warp_args(img, rot, scale, translation, white_background))
    return out


def affine_warp_bwd(g_out, rot, scale, translation, white_background=False, ordered=False):
    """Adjoint of affine_warp w.r.t. the image: g_out [N,C,H,W] -> g_img [N,C,H,W].  ordered=True:
    nfi_affine_warp_bwd_ordered - a gather per source pixel instead of a scatter of atomics, bit-identical from launch to
    launch."""
    g_out = _f32c(g_out, 'g_out')
    if g_out.dim() != 4:
        raise ValueError('affine_warp_bwd: g_out must be [N,C,H,W]')
    g_img = torch.empty_like(g_out)
    _launch('nfi_affine_warp_bwd_ordered' if ordered else 'nfi_affine_warp_bwd', 'nfi_warp_args', g_out, g_warped=g_out,
            g_image=g_img, **_warp_args(g_out, rot, scale, translation, white_background))
    return g_img


def _range_flag(check_range, flag, on, where):
    """The out_of_range word of a metrics call: None, a fresh int32 [1], or the caller's own (one element of a tensor that
    gathers the flags of several calls, so that they reach the host in one read) - written where it is, never copied."""
    if not check_range:
        return None
    if flag is None:
        return torch.empty((1,), dtype=torch.int32, device=on.device)
    return _refuse(flag, 'out_of_range', on, 1, where, dtypes=(torch.int32,))


def image_metrics(pred=None, target=None, mask_pred=None, mask_real=None, check_range=True, out_of_range=None):
    """Per-image PSNR (lib/metrics.py:30-45) of pred/target [B,...] in [0,1] and / or mask IoU (79-94) of
    mask_pred/mask_real [B,...].  Returns (psnr [B] or None, iou [B] or None, out_of_range int32 [1] or None);
    out_of_range: where to write the flag instead of a fresh tensor."""
    first = pred if pred is not None else mask_pred
    if first is None:
        raise ValueError('image_metrics: nothing to measure')
    b, dev = first.shape[0], first.device
    kw = dict(n_images=b)
    psnr = iou = flag = None
    if pred is not None:
        pred, target = _f32c(pred, 'pred', first, where='image_metrics'), _f32c(target, 'target', first, where='image_metrics')
        if pred.shape != target.shape:
            raise ValueError('image_metrics: pred %s vs target %s' % (tuple(pred.shape), tuple(target.shape)))
        psnr = torch.empty((b,), dtype=torch.float32, device=dev)
        kw.update(pred=pred, target=target, elements_per_image=pred.numel() // b, psnr=psnr)
    if mask_pred is not None:
        mask_pred, mask_real = (_f32c(mask_pred, 'mask_pred', first, where='image_metrics'),
                                _f32c(mask_real, 'mask_real', first, where='image_metrics'))
        if mask_pred.shape != mask_real.shape or mask_pred.shape[0] != b:
            raise ValueError('image_metrics: mask shapes %s vs %s' % (tuple(mask_pred.shape), tuple(mask_real.shape)))
        iou = torch.empty((b,), dtype=torch.float32, device=dev)
        kw.update(mask_pred=mask_pred, mask_real=mask_real, elements_per_mask=mask_pred.numel() // b, iou=iou)
    flag = _range_flag(check_range, out_of_range, first, 'image_metrics')
    if flag is not None:
        kw['out_of_range'] = flag
    _launch('nfi_image_metrics', 'nfi_metrics_args', first, **kw)
    return psnr, iou, flag


SSIM_BCHW = 0      # dense [B,3,H,W]
SSIM_BHWC = 1      # dense [B,H,W,3], seen as [B,3,H,W] through permute(0,3,1,2)


def image_ssim(pred, target, want_map=False, check_range=True, out_of_range=None):
    """Per-image SSIM (lib/metrics.py:48-76) of pred / target [B,3,H,W] in [0,1], each dense as [B,3,H,W] or as [B,H,W,3]
    behind a permute (read in place; anything else is copied).  Returns (ssim [B], the cropped map [B,3,H-6,W-6] or
    None, out_of_range int32 [1] or None); out_of_range: where to write the flag instead of a fresh tensor."""
    if pred.dim() != 4 or pred.shape[1] != 3 or pred.shape != target.shape:
        raise ValueError('image_ssim: pred %s and target %s must both be [B,3,H,W]' % (tuple(pred.shape), tuple(target.shape)))
    b, _, h, w = pred.shape
    if b < 1 or h < 7 or w < 7:
        raise ValueError('image_ssim: %d images of %d x %d: at least one image and one 7 x 7 window are needed' % (b, h, w))
    pred, pred_layout = _nchw_or_nhwc(_refuse(pred, 'pred'))
    target, target_layout = _nchw_or_nhwc(_refuse(target, 'target', pred, where='image_ssim'))
    dev = pred.device
    ssim = torch.empty((b,), dtype=torch.float32, device=dev)
    ssim_map = torch.empty((b, 3, h - 6, w - 6), dtype=torch.float32, device=dev) if want_map else None
    flag = _range_flag(check_range, out_of_range, pred, 'image_ssim')
    kw = dict(n_images=b, height=h, width=w)
    ws = _workspace(_lib.struct_query('nfi_image_ssim_workspace_bytes', 'nfi_ssim_args', **kw), pred, 'image_ssim', (b, h, w))
    _launch('nfi_image_ssim', 'nfi_ssim_args', pred, pred=pred, pred_layout=pred_layout, target=target,
            target_layout=target_layout, ssim=ssim, ssim_map=ssim_map, out_of_range=flag, workspace=ws,
            workspace_bytes=ws.numel(), **kw)
    return ssim, ssim_map, flag


FILTER_BCHW = 0        # dense [B,C,H,W]
FILTER_BHWC = 1        # dense [B,H,W,C], seen as [B,C,H,W] through permute(0,3,1,2)
FILTER_MAX_RADIUS = 30
FILTER_TILE = (32, 32)    # kFilterTileH, kFilterTileW of csrc/nfi_filter.inc: output pixels per block


def separable_filter(image, radius, taps=None, sigma=0.0, background=0.0, flip=False):
    """Zero-padded, same-size separable correlation of image [B,C,H,W] (lib/ops.py:29-55: filt2d with a 1-D kernel, blur):
    out = background + (f (x) f) * (image - background), dense [B,C,H,W].  taps: float32 [2 radius + 1] on the image's
    device, used as given, or None: the kernel computes blur's own from sigma.  flip=True applies the taps reversed (the
    adjoint).  image is read in place if it is dense as [B,C,H,W] or as [B,H,W,C] behind a permute; anything else is
    copied.  One launch on the current stream."""
    _refuse(image, 'image')
    if image.dim() != 4 or image.numel() == 0:
        raise ValueError('separable_filter: image must be a non-empty [B,C,H,W], got %s' % (tuple(image.shape),))
    radius = int(radius)
    if not 1 <= radius <= FILTER_MAX_RADIUS:
        raise ValueError('separable_filter: radius %d outside 1 .. %d' % (radius, FILTER_MAX_RADIUS))
    if taps is None:
        if not sigma > 0:
            raise ValueError('separable_filter: sigma must be positive when no taps are given, got %r' % (sigma,))
    else:
        taps = _f32c(taps, 'taps')
        if taps.device != image.device or tuple(taps.shape) != (2 * radius + 1,):
            raise ValueError('separable_filter: taps must be [%d] on %s, got %s on %s' % (2 * radius + 1, image.device, tuple(taps.shape), taps.device))
    image, layout = _nchw_or_nhwc(image)
    b, c, h, w = image.shape
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=image.device)
    _launch('nfi_separable_filter', 'nfi_filter_args', image, n_images=b, channels=c, height=h, width=w, layout=layout,
            image=image, out=out, radius=radius, taps=taps, sigma=float(sigma), background=float(background),
            flip=int(bool(flip)))
    return out


# --------------------------------------------------------------------------- #
# LPIPS distance head (lib/metrics.py:104-110, 130-133; csrc/nfi_lpips.inc): one layer per call
# --------------------------------------------------------------------------- #
def _lpips_inputs(x, y, weight, where):
    """x, y as dense NCHW float32 on one GPU, weight as dense [C].  Dense NCHW tensors are read in place; anything else -
    channels-last included - is copied to dense NCHW first (the kernels have no other layout)."""
    x, y, weight = _f32c(x, 'x'), _f32c(y, 'y'), _f32c(weight, 'weight')
    if x.dim() != 4 or x.numel() == 0 or x.shape != y.shape:
        raise ValueError('%s: x %s and y %s must be the same non-empty [B,C,H,W]' % (where, tuple(x.shape), tuple(y.shape)))
    if weight.numel() != x.shape[1]:
        raise ValueError('%s: weight must hold %d values, got %s' % (where, x.shape[1], tuple(weight.shape)))
    if y.device != x.device or weight.device != x.device:
        raise ValueError('%s: x, y and weight must live on one device' % where)
    b, c, h, w = x.shape
    return x, y, weight, dict(n_images=b, channels=c, height=h, width=w)


def lpips_head(x, y, weight, y_normalized=False, eps=1e-10, out=None, accumulate=False):
    """One layer of the LPIPS distance (lib/metrics.py:104-110, 130-133): x, y [B,C,H,W] feature maps, weight [C] (the lin
    layer's weight[0,:,0,0]) -> out [B] = mean_p sum_c weight[c] (x / (|x| + eps) - y / (|y| + eps))^2; y_normalized=True
    takes y as already normalised (cached features).  out: a float32 [B] to write instead of a fresh tensor;
    accumulate=True adds to it (float32), which chains the layers into one vector.  Two launches on the current stream."""
    x, y, weight, kw = _lpips_inputs(x, y, weight, 'lpips_head')
    b = kw['n_images']
    if out is None:
        if accumulate:
            raise ValueError('lpips_head: accumulate=True needs the out tensor to add to')
        out = torch.empty((b,), dtype=torch.float32, device=x.device)
    elif tuple(_refuse(out, 'out', x, b, 'lpips_head').shape) != (b,) or not out.is_contiguous():      # (written where it is)
        raise ValueError('lpips_head: out must be a dense float32 [%d] on %s' % (b, x.device))
    ws = _workspace(_lib.struct_query('nfi_lpips_head_workspace_bytes', 'nfi_lpips_head_args', **kw), x, 'lpips_head', tuple(x.shape))
    _launch('nfi_lpips_head_fwd', 'nfi_lpips_head_args', x, x=x, y=y, y_normalized=int(bool(y_normalized)), weight=weight,
            eps=float(eps), out=out, accumulate=int(bool(accumulate)), workspace=ws, workspace_bytes=ws.numel(), **kw)
    return out


def lpips_head_bwd(g_out, x, y, weight, y_normalized=False, eps=1e-10, need_x=True, need_y=False):
    """Gradients of lpips_head for the upstream g_out [B]: (g_x or None, g_y or None), each dense [B,C,H,W] and written
    whole by ONE launch (no atomics).  At a pixel of x whose channels are all zero g_x is the finite g q / eps where the
    reference's autograd has NaN."""
    x, y, weight, kw = _lpips_inputs(x, y, weight, 'lpips_head_bwd')
    g_out = _f32c(g_out, 'g_out')
    if g_out.numel() != kw['n_images'] or g_out.device != x.device:
        raise ValueError('lpips_head_bwd: g_out must hold %d values on %s, got %s' % (kw['n_images'], x.device, tuple(g_out.shape)))
    if not (need_x or need_y):
        raise ValueError('lpips_head_bwd: neither gradient is wanted')
    g_x = torch.empty_like(x) if need_x else None
    g_y = torch.empty_like(y) if need_y else None
    _launch('nfi_lpips_head_bwd', 'nfi_lpips_head_args', x, x=x, y=y, y_normalized=int(bool(y_normalized)), weight=weight,
            eps=float(eps), g_out=g_out, g_x=g_x, g_y=g_y, **kw)
    return g_x, g_y


# --------------------------------------------------------------------------- #
# tail of a synthesis layer (models/stylegan.py:101-105, 139-140, 351-355; csrc/nfi_synth_tail.inc)
# --------------------------------------------------------------------------- #
def synth_tail_args(y, dcoefs, noise, bias, taps, act_gain, up, activate=True, slope=0.2, where='synth_tail'):
    """The checked, dense arguments of nfi_synth_tail_args shared by the forward and the backward, as a dict.  A caller that
    runs both on the same tensors (synthesis.layer_tail) checks once and hands the dict to synth_tail_launch /
    synth_tail_bwd_launch."""
    y = _f32c(y, 'y')
    dcoefs, bias = _f32c(dcoefs, 'dcoefs', y, where=where), _f32c(bias, 'bias', y, where=where)
    if y.dim() != 4 or y.numel() == 0 or y.shape[2] != y.shape[3]:
        raise ValueError('%s: y must be a non-empty square [B,C,N,N], got %s' % (where, tuple(y.shape)))
    b, c, n = y.shape[0], y.shape[1], y.shape[2]
    r = n - 1 if up else n
    if r < 1:
        raise ValueError('%s: an up layer needs y of side R + 1 >= 2, got %s' % (where, tuple(y.shape)))
    if tuple(dcoefs.shape) != (b, c) or bias.numel() != c:
        raise ValueError('%s: dcoefs must be [%d,%d] and bias [%d], got %s and %s' % (where, b, c, c, tuple(dcoefs.shape), tuple(bias.shape)))
    if not act_gain > 0:
        raise ValueError('%s: act_gain must be positive, got %r' % (where, act_gain))
    if not slope >= 0:
        raise ValueError('%s: slope must not be negative, got %r' % (where, slope))
    shared = 0
    if noise is not None:
        noise = _f32c(noise, 'noise', y, where=where)
        if tuple(noise.shape) == (r, r):
            shared = 1
        elif tuple(noise.shape) != (b, 1, r, r):
            raise ValueError('%s: noise must be [%d,1,%d,%d] or [%d,%d], got %s' % (where, b, r, r, r, r, tuple(noise.shape)))
    if up:
        if taps is None:
            raise ValueError('%s: an up layer needs its resample_filter' % where)
        taps = _f32c(taps, 'resample_filter', y, where=where)
        if tuple(taps.shape) != (4, 4):
            raise ValueError('%s: resample_filter must be [4,4], got %s' % (where, tuple(taps.shape)))
    else:
        taps = None
    kw = dict(batch=b, channels=c, resolution=r, in_size=n, up=int(bool(up)), activate=int(bool(activate)), act_gain=float(act_gain),
              slope=float(slope), y=y, dcoefs=dcoefs, bias=bias, taps=taps, noise=noise, noise_shared=shared)
    return kw


@functools.lru_cache(maxsize=None)
def _synth_tail_workspace_bytes(b, c, r, up):
    return _lib.struct_query('nfi_synth_tail_bwd_workspace_bytes', 'nfi_synth_tail_args', batch=b, channels=c, resolution=r, up=up)


def synth_tail(y, dcoefs, noise, bias, resample_filter, act_gain, up, activate=True, slope=0.2):
    """Everything SynthesisLayer.forward does after its convolution (models/stylegan.py:101-105, 139-140, 351-355), one launch:
    y [B,C,R+1,R+1] with up (the transposed convolution's output; filtered by 4 * resample_filter [4,4], zero padded) or
    [B,C,R,R] without; dcoefs [B,C]; noise None, [B,1,R,R] or [R,R]; bias [C] ->
    lrelu_slope(((noise + f * dcoefs) + bias) * act_gain), dense [B,C,R,R] (no lrelu with activate=False).  The filter's
    taps are read on the device."""
    return synth_tail_launch(synth_tail_args(y, dcoefs, noise, bias, resample_filter, act_gain, up, activate, slope))


def synth_tail_launch(kw):
    """synth_tail on arguments synth_tail_args has checked."""
    r = kw['resolution']
    out = torch.empty((kw['batch'], kw['channels'], r, r), dtype=torch.float32, device=kw['y'].device)
    _launch('nfi_synth_tail_fwd', 'nfi_synth_tail_args', out, out=out, **kw)
    return out


def synth_tail_bwd(g_out, out, y, dcoefs, noise, bias, resample_filter, act_gain, up, activate=True, slope=0.2,
                   need_y=True, need_dcoefs=True, need_bias=True, need_noise=False):
    """Gradients of synth_tail for the upstream g_out [B,C,R,R]; out is the forward's result (the sign of the
    pre-activation is read from it).  Returns a dict with whichever of g_y (y's shape), g_dcoefs [B,C], g_bias [C] and
    g_noise (noise's shape) were asked for.  Every sum runs in a fixed order (no atomics): the same bits on every call."""
    kw = synth_tail_args(y, dcoefs, noise, bias, resample_filter, act_gain, up, activate, slope, 'synth_tail_bwd')
    b, c, r = kw['batch'], kw['channels'], kw['resolution']
    g_out, out = _f32c(g_out, 'g_out', kw['y'], where='synth_tail_bwd'), _f32c(out, 'out', kw['y'], where='synth_tail_bwd')
    if tuple(g_out.shape) != (b, c, r, r) or tuple(out.shape) != (b, c, r, r):
        raise ValueError('synth_tail_bwd: g_out and out must be [%d,%d,%d,%d], got %s and %s' % (
            b, c, r, r, tuple(g_out.shape), tuple(out.shape)))
    if need_noise and noise is None:
        raise ValueError('synth_tail_bwd: need_noise without a noise input')
    if not (need_y or need_dcoefs or need_bias or need_noise):
        raise ValueError('synth_tail_bwd: no gradient is wanted')
    return synth_tail_bwd_launch(kw, g_out, out, need_y, need_dcoefs, need_bias, need_noise)


def synth_tail_bwd_launch(kw, g_out, out, need_y, need_dcoefs, need_bias, need_noise):
    """synth_tail_bwd on arguments synth_tail_args has checked; g_out and out dense float32 [B,C,R,R] on their device."""
    b, c, r = kw['batch'], kw['channels'], kw['resolution']
    dev = out.device
    res = {}
    if need_y:
        res['g_y'] = torch.empty_like(kw['y'])
    if need_dcoefs:
        res['g_dcoefs'] = torch.empty((b, c), dtype=torch.float32, device=dev)
    if need_bias:
        res['g_bias'] = torch.empty((c,), dtype=torch.float32, device=dev)
    if need_noise:
        res['g_noise'] = torch.empty(kw['noise'].shape, dtype=torch.float32, device=dev)
    ws, n_ws = None, 0
    if need_dcoefs or need_bias:
        n_ws = _synth_tail_workspace_bytes(b, c, r, kw['up'])
        ws = _workspace(n_ws, out, 'synth_tail_bwd', kw['y'].shape, torch.float64)
    _launch('nfi_synth_tail_bwd', 'nfi_synth_tail_args', out, out=out, g_out=g_out, workspace=ws, workspace_bytes=n_ws,
            **dict(kw, **res))
    return res


# --------------------------------------------------------------------------- #
# head of a synthesis layer (models/stylegan.py:173-177, 127-130, 132, 373; csrc/nfi_synth_head.inc).  The kernels read
# single floats through every pointer but the modulation's planes, and those they test themselves (16-byte accesses where
# the pointers allow it): nothing here is copied for its alignment.
# --------------------------------------------------------------------------- #
def _latent_rows(latent, where):
    """latent as float32 [B,D] on the GPU whose rows the kernel can read in place: unit stride along d and rows at least D
    apart (a layer's ws.unbind(1)[k]); any other view is copied."""
    _refuse(latent, 'latent')
    if latent.dim() != 2 or latent.numel() == 0:
        raise ValueError('%s: latent must be a non-empty [B,D], got %s' % (where, tuple(latent.shape)))
    b, d = latent.shape
    in_place = (d == 1 or latent.stride(1) == 1) and (b == 1 or latent.stride(0) >= d)
    return latent if in_place else latent.contiguous()


def synth_head_args(latent, affine_weight, affine_bias, weight_gain, bias_gain, conv_weight, demodulate=True, style_gain=1.0,
                    where='synth_head'):
    """The checked arguments of nfi_synth_head_args shared by the forward and the backward, as a dict: latent [B,D] (a view
    with unit stride along d is read in place), affine_weight [I,D], affine_bias [I] or None, conv_weight [O,I,kh,kw]."""
    latent = _latent_rows(latent, where)
    b, d = latent.shape
    if affine_weight.dim() != 2 or affine_weight.shape[1] != d or affine_weight.shape[0] < 1:
        raise ValueError('%s: affine_weight must be [I,%d], got %s' % (where, d, tuple(affine_weight.shape)))
    i = affine_weight.shape[0]
    if conv_weight.dim() < 2 or conv_weight.shape[1] != i or conv_weight.numel() == 0:
        raise ValueError('%s: conv_weight must be a non-empty [O,%d,...], got %s' % (where, i, tuple(conv_weight.shape)))
    o = conv_weight.shape[0]
    k = conv_weight.numel() // (o * i)
    affine_weight = _f32c(affine_weight, 'affine_weight', latent, i * d, where, align=4)
    affine_bias = _f32c(affine_bias, 'affine_bias', latent, i, where, align=4)
    conv_weight = _f32c(conv_weight, 'conv_weight', latent, o * i * k, where, align=4)
    for name, g in (('weight_gain', weight_gain), ('bias_gain', bias_gain), ('style_gain', style_gain)):
        if not math.isfinite(g):
            raise ValueError('%s: %s must be finite, got %r' % (where, name, g))
    return dict(batch=b, latent_dim=d, in_channels=i, out_channels=o, taps=k, latent_stride=latent.stride(0) if b > 1 else d,
                demodulate=int(bool(demodulate)), weight_gain=float(weight_gain), bias_gain=float(bias_gain), style_gain=float(style_gain),
                latent=latent, affine_weight=affine_weight, affine_bias=affine_bias, weight=conv_weight)


@functools.lru_cache(maxsize=None)
def _synth_head_workspace_bytes(b, d, stride, i, o, k, demodulate):
    return _lib.struct_query('nfi_synth_head_bwd_workspace_bytes', 'nfi_synth_head_args', batch=b, latent_dim=d, latent_stride=stride,
                             in_channels=i, out_channels=o, taps=k, demodulate=demodulate)


def synth_head_launch(kw):
    """synth_head on arguments synth_head_args has checked."""
    dev = kw['latent'].device
    styles = torch.empty((kw['batch'], kw['in_channels']), dtype=torch.float32, device=dev)
    dcoefs = torch.empty((kw['batch'], kw['out_channels']), dtype=torch.float32, device=dev) if kw['demodulate'] else None
    _launch('nfi_synth_head_fwd', 'nfi_synth_head_args', styles, styles=styles, dcoefs=dcoefs, **kw)
    return styles, dcoefs


def synth_head_bwd_launch(kw, g_styles, g_dcoefs, styles, dcoefs, need_latent, need_affine_weight, need_affine_bias, need_weight):
    """synth_head_bwd on arguments synth_head_args has checked; g_styles / g_dcoefs / styles / dcoefs: dense float32 [B,I] /
    [B,O] on the device of kw['latent'], or None."""
    b, d, i, o, k = (kw[n] for n in ('batch', 'latent_dim', 'in_channels', 'out_channels', 'taps'))
    dev = kw['latent'].device
    res = {}
    if need_latent:
        res['g_latent'] = torch.empty((b, d), dtype=torch.float32, device=dev)
    if need_affine_weight:
        res['g_affine_weight'] = torch.empty((i, d), dtype=torch.float32, device=dev)
    if need_affine_bias:
        res['g_affine_bias'] = torch.empty((i,), dtype=torch.float32, device=dev)
    if need_weight:
        res['g_weight'] = torch.empty((o, i, k), dtype=torch.float32, device=dev)
    n_ws = _synth_head_workspace_bytes(b, d, kw['latent_stride'], i, o, k, kw['demodulate'])
    ws = _workspace(n_ws, kw['latent'], 'synth_head_bwd (B, D, I, O, K)', (b, d, i, o, k), torch.float64)
    _launch('nfi_synth_head_bwd', 'nfi_synth_head_args', ws, styles=styles, dcoefs=dcoefs, g_styles=g_styles, g_dcoefs=g_dcoefs,
            workspace=ws, workspace_bytes=n_ws, **dict(kw, **res))
    return res


def synth_head(latent, affine_weight, affine_bias, weight_gain, bias_gain, conv_weight, demodulate=True, style_gain=1.0):
    """What a synthesis layer does before its convolution, up to the modulation (models/stylegan.py:173-177, 127-130; 373 for
    toRGB): (styles [B,I], dcoefs [B,O] or None without demodulate).  Two launches, one without demodulate; the [B,O,I,kh,kw]
    product of the reference is never formed."""
    return synth_head_launch(synth_head_args(latent, affine_weight, affine_bias, weight_gain, bias_gain, conv_weight, demodulate, style_gain))


def synth_head_bwd(g_styles, g_dcoefs, styles, dcoefs, latent, affine_weight, affine_bias, weight_gain, bias_gain, conv_weight,
                   demodulate=True, style_gain=1.0, need_latent=True, need_affine_weight=True, need_affine_bias=True, need_weight=True):
    """Gradients of synth_head for the upstream g_styles [B,I] and g_dcoefs [B,O] (either may be None); styles and dcoefs are
    the forward's results.  Returns a dict with whichever of g_latent [B,D], g_affine_weight [I,D], g_affine_bias [I] and
    g_weight [O,I,K] (the demodulation's share only; needs g_dcoefs) were asked for.  At most four launches, every sum in
    a fixed order: the same bits on every call."""
    where = 'synth_head_bwd'
    kw = synth_head_args(latent, affine_weight, affine_bias, weight_gain, bias_gain, conv_weight, demodulate, style_gain, where)
    on, b, i, o = kw['latent'], kw['batch'], kw['in_channels'], kw['out_channels']
    styles, g_styles = _f32c(styles, 'styles', on, b * i, where, align=4), _f32c(g_styles, 'g_styles', on, b * i, where, align=4)
    dcoefs, g_dcoefs = _f32c(dcoefs, 'dcoefs', on, b * o, where, align=4), _f32c(g_dcoefs, 'g_dcoefs', on, b * o, where, align=4)
    if styles is None:
        raise ValueError('%s: styles (the forward\'s result) is needed' % where)
    if g_styles is None and g_dcoefs is None:
        raise ValueError('%s: no upstream gradient (g_styles and g_dcoefs both None)' % where)
    if g_dcoefs is not None and (dcoefs is None or not demodulate):
        raise ValueError('%s: g_dcoefs without dcoefs (the forward\'s result, with demodulate)' % where)
    need_affine_bias = bool(need_affine_bias) and kw['affine_bias'] is not None
    if need_weight and g_dcoefs is None:
        raise ValueError('%s: need_weight without g_dcoefs (g_weight is the demodulation\'s share only)' % where)
    if not (need_latent or need_affine_weight or need_affine_bias or need_weight):
        raise ValueError('%s: no gradient is wanted' % where)
    return synth_head_bwd_launch(kw, g_styles, g_dcoefs, styles, dcoefs, bool(need_latent), bool(need_affine_weight), need_affine_bias,
                                 bool(need_weight))


def synth_modulate_args(x, styles, where='synth_modulate'):
    """The checked arguments of nfi_synth_modulate_args: x [B,C,...] dense (copied if not), styles [B,C]."""
    x = _f32c(x, 'x', align=4)
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError('%s: x must be a non-empty [B,C,...], got %s' % (where, tuple(x.shape)))
    b, c = x.shape[0], x.shape[1]
    styles = _f32c(styles, 'styles', x, b * c, where, align=4)
    return dict(batch=b, channels=c, plane=x.numel() // (b * c), x=x, styles=styles)


def synth_modulate_launch(kw):
    """synth_modulate on arguments synth_modulate_args has checked."""
    out = torch.empty_like(kw['x'])
    _launch('nfi_synth_modulate_fwd', 'nfi_synth_modulate_args', out, out=out, **kw)
    return out


def synth_modulate_bwd_launch(kw, g_out, need_x, need_styles):
    """synth_modulate_bwd on arguments synth_modulate_args has checked; g_out: dense float32, x's shape and device."""
    g_x = torch.empty_like(kw['x']) if need_x else None
    g_styles = torch.empty((kw['batch'], kw['channels']), dtype=torch.float32, device=g_out.device) if need_styles else None
    _launch('nfi_synth_modulate_bwd', 'nfi_synth_modulate_args', g_out, g_out=g_out, g_x=g_x, g_styles=g_styles, **kw)
    return g_x, g_styles


def synth_modulate(x, styles):
    """x * styles.reshape(B, -1, 1, 1) (models/stylegan.py:132): x [B,C,H,W] (any trailing shape), styles [B,C] -> x's shape,
    dense.  One launch."""
    return synth_modulate_launch(synth_modulate_args(x, styles))


def synth_modulate_bwd(g_out, x, styles, need_x=True, need_styles=True):
    """(g_x = g_out * styles or None, g_styles [B,C] = sum over the plane of g_out * x or None).  One launch; the sums run
    in a fixed order: the same bits on every call."""
    where = 'synth_modulate_bwd'
    kw = synth_modulate_args(x, styles, where)
    g_out = _f32c(g_out, 'g_out', kw['x'], kw['x'].numel(), where, align=4)
    if tuple(g_out.shape) != tuple(kw['x'].shape):
        raise ValueError('%s: g_out must have x\'s shape %s, got %s' % (where, tuple(kw['x'].shape), tuple(g_out.shape)))
    if not (need_x or need_styles):
        raise ValueError('%s: no gradient is wanted' % where)
    return synth_modulate_bwd_launch(kw, g_out, bool(need_x), bool(need_styles))


# --------------------------------------------------------------------------- #
# pose algebra of the inversion loop (lib/pose_utils.py; csrc/nfi_pose.inc): thread = image, one launch per call
# --------------------------------------------------------------------------- #
def _pose_rows(t, tail, name, on=None):
    """t as dense float32 [B, *tail] on the GPU; on: the call's first tensor - t then has its B and lives on its device."""
    t = _f32c(t, name, on, align=4)          # (nfi_pose.inc: one thread per image, float loads and stores only)
    b = None if on is None else on.shape[0]
    if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail or t.shape[0] < 1 or (b is not None and t.shape[0] != b):
        raise ValueError('%s must be [%s], got %s' % (name, ', '.join(['B' if b is None else str(b)] + [str(v) for v in tail]),
                                                      tuple(t.shape)))
    return t


def _pose_params(q, t2, s, z0):
    q = _pose_rows(q, (4,), 'q')
    return q, _pose_rows(t2, (2,), 't2', q), _pose_rows(s, (), 's', q), None if z0 is None else _pose_rows(z0, (), 'z0', q)


def pose_to_matrix(q, t2, s, z0=None, camera_flipped=False, normalize_q=False):
    """lib/pose_utils.py:48-70 for q [B,4], t2 [B,2], s [B], z0 [B] or None (orthographic): (cam2world [B,4,4], focal [B]
    or None).  normalize_q: F.normalize(q, dim=-1) inside the launch."""
    q, t2, s, z0 = _pose_params(q, t2, s, z0)
    b, dev = q.shape[0], q.device
    cam2world = torch.empty((b, 4, 4), dtype=torch.float32, device=dev)
    focal = None if z0 is None else torch.empty((b,), dtype=torch.float32, device=dev)
    _launch('nfi_pose_to_matrix_fwd', 'nfi_pose_args', q, n_images=b, camera_flipped=int(bool(camera_flipped)),
            normalize_q=int(bool(normalize_q)), q=q, t2=t2, s=s, z0=z0, cam2world=cam2world, focal=focal)
    return cam2world, focal


def pose_to_matrix_bwd(g_cam2world, g_focal, q, t2, s, z0=None, camera_flipped=False, normalize_q=False,
                       needs=(True, True, True, True)):
    """Gradients (g_q, g_t2, g_s, g_z0) of the above from g_cam2world [B,4,4] and g_focal [B] or None; needs: which of the
    four to compute (the others, and g_z0 without z0, are None)."""
    q, t2, s, z0 = _pose_params(q, t2, s, z0)
    g_cam2world = _pose_rows(g_cam2world, (4, 4), 'g_cam2world', q)
    g_focal = None if g_focal is None or z0 is None else _pose_rows(g_focal, (), 'g_focal', q)
    needs = tuple(needs[:3]) + (needs[3] and z0 is not None,)
    outs = [torch.empty_like(t) if need else None for t, need in zip((q, t2, s, z0), needs)]
    if any(needs):
        _launch('nfi_pose_to_matrix_bwd', 'nfi_pose_args', q, n_images=q.shape[0], camera_flipped=int(bool(camera_flipped)),
                normalize_q=int(bool(normalize_q)), q=q, t2=t2, s=s, z0=z0, g_cam2world=g_cam2world, g_focal=g_focal,
                g_q=outs[0], g_t2=outs[1], g_s=outs[2], g_z0=outs[3])
    return tuple(outs)


def matrix_to_pose(cam2world, focal=None, camera_flipped=False, want_pose=True, want_cond=False):
    """lib/pose_utils.py:98-145 on the device: (z0 [B] or None, t2 [B,2], s [B], q [B,4], cond [B,13]); the first four are
    None without want_pose, the last without want_cond."""
    cam2world = _pose_rows(cam2world, (4, 4), 'cam2world')
    b, dev = cam2world.shape[0], cam2world.device
    focal = None if focal is None else _pose_rows(focal, (), 'focal', cam2world)

    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)
    z0 = new(b) if want_pose and focal is not None else None
    t2, s, q = (new(b, 2), new(b), new(b, 4)) if want_pose else (None, None, None)
    cond = new(b, 13) if want_cond else None
    _launch('nfi_matrix_to_pose', 'nfi_matrix_to_pose_args', cam2world, n_images=b, camera_flipped=int(bool(camera_flipped)),
            cam2world=cam2world, focal=focal, z0=z0, t2=t2, s=s, q=q, cond=cond)
    return z0, t2, s, q, cond


def rotation_distance(p, q):
    """lib/pose_utils.py:148-156: degrees [B] between p, q [B,3,3] or [B,4,4] (4 x 4: each over its element [3,3])."""
    dim = p.shape[-1]
    if dim not in (3, 4):
        raise ValueError('rotation_distance: [B,3,3] or [B,4,4] matrices, got %s' % (tuple(p.shape),))
    p = _pose_rows(p, (dim, dim), 'p')
    q = _pose_rows(q, (dim, dim), 'q', p)
    degrees = torch.empty((p.shape[0],), dtype=torch.float32, device=p.device)
    _launch('nfi_rotation_distance', 'nfi_rotation_distance_args', p, n_images=p.shape[0], dim=dim, p=p, q=q, degrees=degrees)
    return degrees


def pose_nearest_by_angle(cam2world, target):
    """The selection of lib/pose_utils.py:159-170: int32 [N], for each pose the index of the pose whose distance to it is
    closest to target [N] degrees (the lowest index on a tie)."""
    cam2world = _pose_rows(cam2world, (4, 4), 'cam2world')
    n = cam2world.shape[0]
    target = _pose_rows(target, (), 'target', cam2world)
    index = torch.empty((n,), dtype=torch.int32, device=cam2world.device)
    _launch('nfi_pose_nearest_by_angle', 'nfi_pose_nearest_args', cam2world, n_images=n, cam2world=cam2world, target=target,
            index=index)
    return index


def pose_project_(q, s, z0=None):
    """run.py:2307-2310 in place on dense float32 tensors: q [B,4] normalised, s [B] made non-negative, z0 [B] (if given)
    clamped to [-4, 4]."""
    for t, tail, name in ((q, (4,), 'q'), (s, (), 's'), (z0, (), 'z0')):
        if t is not None and _pose_rows(t, tail, name, None if t is q else q) is not t:
            raise ValueError('pose_project_: %s must be contiguous to be changed in place' % name)
    _launch('nfi_pose_project', 'nfi_pose_project_args', q, n_images=q.shape[0], q=q, s=s, z0=z0)


# --------------------------------------------------------------------------- #
# plane-producer hand-off
# --------------------------------------------------------------------------- #
def torgb_texels(x, styles, weight, bias, previous_image=None):
    """Tail of the last synthesis block (stylegan.py:383-435) written as texels: x [B,Cin,R,R], styles [B,Cin],
    weight [96,Cin], bias [96], previous_image [B,96,R/2,R/2] or None -> a [B,96,R,R] tensor in channels-last memory
    format (its storage IS the interleaved texel image [B,R,R,3,32])."""
    where = 'torgb_texels'
    x = _f32c(x, 'x')
    styles, weight, bias = _f32c(styles, 'styles', x, where=where), _f32c(weight, 'weight', x, where=where), _f32c(bias, 'bias', x, where=where)
    prev = _f32c(previous_image, 'previous_image', x, where=where)
    if x.dim() != 4:
        raise ValueError('torgb_texels: x must be [B,Cin,R,R], got %s' % (tuple(x.shape),))
    B, Cin, R, R2 = x.shape
    if R != R2 or tuple(styles.shape) != (B, Cin) or tuple(weight.shape) != (96, Cin) or tuple(bias.shape) != (96,) or \
            (prev is not None and tuple(prev.shape) != (B, 96, R // 2, R // 2)):
        raise ValueError('torgb_texels: shapes x %s styles %s weight %s bias %s prev %s' % (
            tuple(x.shape), tuple(styles.shape), tuple(weight.shape), tuple(bias.shape),
            None if prev is None else tuple(prev.shape)))
    out = torch.empty((B, 96, R, R), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    _launch('nfi_torgb_texels_fwd', 'nfi_torgb_args', x, n_scenes=B, in_channels=Cin, resolution=R, x=x, styles=styles,
            weight=weight, bias=bias, previous_image=prev, texels=out)
    return out


def torgb_texels_bwd(g_out, x, styles, weight, previous_image=None, want_weight=True, want_prev=True, ordered=False):
    """Backward of torgb_texels.  g_out: [B,96,R,R] (any strides; brought to channels-last).  Returns dict(g_x, g_styles,
    g_weight?, g_bias?, g_previous_image?).  ordered=True: nfi_torgb_texels_bwd_ordered - the style, weight and bias sums
    in a fixed order, every output bit-identical from launch to launch (a workspace is allocated per call)."""
    where = 'torgb_texels_bwd'
    x = _f32c(x, 'x')
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError('torgb_texels_bwd: x must be [B,Cin,R,R], got %s' % (tuple(x.shape),))
    B, Cin, R, _ = x.shape
    styles, weight = _f32c(styles, 'styles', x, B * Cin, where), _f32c(weight, 'weight', x, 96 * Cin, where)
    prev = _f32c(previous_image, 'previous_image', x, B * 96 * (R // 2) * (R // 2), where)
    if tuple(_refuse(g_out, 'g_out', x, where=where).shape) != (B, 96, R, R):
        raise ValueError('torgb_texels_bwd: g_out must be [%d,96,%d,%d], got %s' % (B, R, R, tuple(g_out.shape)))
    g = _dense_channels_last(g_out)
    dev = x.device
    out = {'g_x': torch.empty_like(x), 'g_styles': torch.empty((B, Cin), dtype=torch.float32, device=dev)}
    if want_weight:
        out['g_weight'] = torch.empty((96, Cin), dtype=torch.float32, device=dev)
        out['g_bias'] = torch.empty((96,), dtype=torch.float32, device=dev)
    if want_prev and prev is not None:
        out['g_previous_image'] = torch.empty_like(prev)
    args = dict(n_scenes=B, in_channels=Cin, resolution=R, x=x, styles=styles, weight=weight, previous_image=prev, g_texels=g,
                **out)
    if ordered:
        _call_ordered('nfi_torgb_texels_bwd_ordered', 'nfi_torgb_args', x, 'torgb_texels_bwd(ordered=True)', (B, Cin, R), args)
    else:
        _launch('nfi_torgb_texels_bwd', 'nfi_torgb_args', x, **args)
    return out


# --------------------------------------------------------------------------- #
# view-direction mapper: the per-ray trunk (models/generator.py:194-241)
# --------------------------------------------------------------------------- #
# the 18 parameter tensors in the order of nfi_viewdir_mapper_args, with their shapes
VIEWDIR_MAPPER_PARAMS = (('fc0_w', (64, 3)), ('fc0_b', (64,)),
                         ('fc1_w', (64, 64)), ('norm1_w', (64,)), ('norm1_b', (64,)),
                         ('fc2_w', (64, 64)), ('norm2_w', (64,)), ('norm2_b', (64,)),
                         ('fc3_w', (64, 64)), ('norm3_w', (64,)), ('norm3_b', (64,)),
                         ('fc4_w', (64, 64)), ('norm4_w', (64,)), ('norm4_b', (64,)),
                         ('fc5_w', (64, 64)), ('fc5_b', (64,)), ('fc6_w', (32, 64)), ('fc6_b', (32,)))


def _viewdir_mapper_inputs(viewdir, params):
    viewdir = _f32c(viewdir, 'viewdir')
    if viewdir.dim() < 1 or viewdir.shape[-1] != 3 or viewdir.numel() == 0:
        raise ValueError('viewdir must be a non-empty [...,3] tensor, got %s' % (tuple(viewdir.shape),))
    if len(params) != len(VIEWDIR_MAPPER_PARAMS):
        raise ValueError('viewdir_mapper: %d parameter tensors expected (%s), got %d' % (
            len(VIEWDIR_MAPPER_PARAMS), ', '.join(n for n, _ in VIEWDIR_MAPPER_PARAMS), len(params)))
    kw = {}
    for (name, shape), t in zip(VIEWDIR_MAPPER_PARAMS, params):
        t = _f32c(t, name, viewdir, where='viewdir_mapper')
        if tuple(t.shape) != shape:
            raise ValueError('viewdir_mapper: %s must be %s, got %s' % (name, list(shape), tuple(t.shape)))
        kw[name] = t
    return viewdir, kw


def viewdir_mapper_fwd(viewdir, params):
    """viewdir [...,3], params: the 18 raw tensors in VIEWDIR_MAPPER_PARAMS order -> ViewDirectionMapper.fc6's output
    [...,32], one launch."""
    viewdir, kw = _viewdir_mapper_inputs(viewdir, params)
    feature = torch.empty(viewdir.shape[:-1] + (32,), dtype=torch.float32, device=viewdir.device)
    _launch('nfi_viewdir_mapper_fwd', 'nfi_viewdir_mapper_args', viewdir, n_rays=viewdir.numel() // 3, viewdir=viewdir,
            feature=feature, **kw)
    return feature


def viewdir_mapper_bwd(viewdir, params, g_feature, want_viewdir=True, into=None, want_params=True):
    """Backward of viewdir_mapper_fwd, one launch.  Returns dict('g_' + name for the 18 parameters, shaped like them, and
    'g_viewdir' [...,3] or None).  into: such a dict from an earlier call - the parameter gradients of this call are
    then ADDED to its tensors (the accumulate contract of the C entry); otherwise fresh zeroed tensors are filled.
    want_params=False (a frozen mapper): only g_viewdir is computed, the parameter entries are None."""
    viewdir, kw = _viewdir_mapper_inputs(viewdir, params)
    where = 'viewdir_mapper_bwd'
    g_feature = _f32c(g_feature, 'g_feature', viewdir, where=where)      # (the kernel reads its rows as 16-byte vectors)
    if tuple(g_feature.shape) != tuple(viewdir.shape[:-1]) + (32,):
        raise ValueError('g_feature must be %s, got %s' % (tuple(viewdir.shape[:-1]) + (32,), tuple(g_feature.shape)))
    dev = viewdir.device
    out = {}
    if not want_params:
        if not want_viewdir or into is not None:
            raise ValueError('viewdir_mapper_bwd: want_params=False computes g_viewdir only')
        out = {'g_' + name: None for name, _ in VIEWDIR_MAPPER_PARAMS}           # (null pointers: not computed)
    elif into is None:
        # one zero-fill for the 18 buffers: they are views of one flat tensor (23 392 floats)
        sizes = [math.prod(shape) for _, shape in VIEWDIR_MAPPER_PARAMS]
        flat = torch.zeros((sum(sizes),), dtype=torch.float32, device=dev)
        for (name, shape), part in zip(VIEWDIR_MAPPER_PARAMS, flat.split(sizes)):
            out['g_' + name] = part.view(shape)
    else:
        for name, shape in VIEWDIR_MAPPER_PARAMS:
            t = _refuse(into['g_' + name], 'into[g_%s]' % name, viewdir, where=where)        # (added to where it is)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError('viewdir_mapper_bwd: into[g_%s] must be a contiguous float32 GPU tensor %s' % (name, list(shape)))
            out['g_' + name] = t
    g_viewdir = torch.empty_like(viewdir) if want_viewdir else None
    _launch('nfi_viewdir_mapper_bwd', 'nfi_viewdir_mapper_args', viewdir, n_rays=viewdir.numel() // 3, viewdir=viewdir,
            g_feature=g_feature, g_viewdir=g_viewdir, **kw, **out)
    out['g_viewdir'] = g_viewdir
    return out
