"""Drop-in for ``render`` in the reference's run.py (176-350): same 16-parameter signature, same
6-tuple, same module-level ``args`` / ``dataset_config`` globals.

    import nerf_from_image_amd.render as nfi_render
    nfi_render.configure(args, dataset_config)          # once, where run.py builds them
    render = nfi_render.render                           # replaces run.py's own def

Three execution paths, all HIP through the C ABI:
  * fused          - one persistent launch for the whole pipeline (no gradient); the composited `semantics`, `coords` and
                     `normals` maps (compute_semantics / compute_coords / compute_normals: run.py:1250-1264, 1444-1454,
                     1639-1646, 2036-2051) come out of the same launch;
  * fused + stash  - the SAME launch when a gradient is needed (training / inversion; with or without fine sampling, plain
                     or view-direction decoder): the kernel also
                     writes a per-sample stash (depths, sigma, rgb of the 2S samples of every ray, ray-major), and the
                     whole render is ONE autograd node whose backward is compositing backward on the stash -> one field
                     backward launch over the 2S points of every ray (+ its binned plane-gradient scatter) -> ray /
                     camera backward.  Replaces the ~20 launches of the staged graph;
  * staged         - one launch per stage through ``nerf_utils`` and the ``sampler`` closure: extra maps with a gradient /
                     the 'bbox' overlay / extra maps of the view-direction decoder on 16-bit texels, or over a single pass
                     of more than 128 samples.
A single pass of up to 512 samples (run.py's inversion without --fine_sampling: depth_samples_per_ray * 4, run.py:2271)
takes the fused / fused + stash paths too (render_fwd_long_kernel).
Randomness follows the reference, in its order: ``torch.rand`` of [B,H,W,S] for the stratified
jitter (nerf_utils.py:115) BEFORE the model is called (its synthesis network draws noise of its own
in training), then ``torch.rand`` of [B*H*W,S] for the inverse-CDF draws (nerf_utils.py:202), even
in eval (``randomize`` defaults to True and no caller overrides it).

Options (``configure(..., **options)`` / ``make_render(..., **options)``; per bound render function, nothing
process-wide - the reference calls render from one thread per GPU):
  termination_eps   0 = off (default).  eps in (0,1): the fused inference kernel does not evaluate fine samples behind the
                    depth at which the COARSE transmittance has fallen below eps and compacts the rest by wave ballot
                    (coarse pass, pdf and sample indices untouched; |d rgb| <= ~eps; ops.render_fwd(termination_eps=...));
                    without fine sampling, for calls that ask for extra maps and with the view-direction decoder it has
                    nothing to act on and is ignored;
  strict_near_far   True (default, the reference's behaviour): every path raises when no ray of the batch meets the scene
                    cube (lib/nerf_utils.py:258 fails on min() of an empty selection; its boolean indexing synchronises
                    the host there too).  The fused paths read the hit counter of the ray set-up back BEFORE the render
                    kernel is launched: the host waits for the set-up kernels only, and a batch without a hit does not
                    pay for a render.  'after': the fused paths launch once and read the counter back behind the render
                    (no device idle between set-up and render; the host waits for the render).  'deferred': no
                    synchronisation at all, on any path - the counter travels to pinned host memory
                    behind the render and is looked at by the NEXT strict call on that device (or ops.flush_strict()),
                    which raises for the earlier batch; for serving / pipelined loops.  False: never raises, such a
                    batch renders as background.  With row_window the check is the whole image's: it runs only when
                    row_window_sync has summed the hit count over the bands (a band of background rows is legitimate);
                    without row_window_sync a windowed call does not check;
  row_window        None, or (row_offset, rows): render only these image rows (fused inference path; one image sharded
                    over the ranks of a node, parallel.shard_rows); the outputs then have `rows` rows;
  row_window_sync   False, or True / a process group: the ranks of the group render bands of the SAME image, and the
                    batch-wide miss-fill of lib/nerf_utils.py:258-259 is reduced over them between the ray set-up and the
                    render kernel (parallel.allreduce_ray_setup), so that every band is bit-identical to the same rows
                    of the full render.  Without it the fill is the band's own: identical only where no marched ray
                    misses the exact cube (the default cameras) - stated in include/nfi_hip.h.
  views_per_scene   1 (default), or V: every scene of the model call is rendered from V cameras.  tform_cam2world is then
                    [B*V,4,4], scene-major (the V cameras of scene 0 first), focal_length / bbox / center follow the cameras,
                    model_input keeps its B rows: the plane producer runs once per scene.  Outputs are [B*V,H,W,...], bit for
                    bit those of the call with every latent repeated V times (the batch-wide miss-fill of
                    lib/nerf_utils.py:258-259 runs over all B*V images, the random draws keep their shapes and order); on
                    every path: fused (nfi_render_args.views_per_scene), fused + stash (ONE field backward launch over
                    V*H*W rays per scene sums the views' plane / attention-value / decoder gradients, camera and focal
                    gradients stay per camera; at most 2^25 points per scene, V*H*W*samples - else ValueError), staged (the V
                    views of a scene as one image V*H rows tall; so are the viewdirs a use_viewdir model receives).
  deterministic_backward  False (default), or True: every gradient the fused + stash node returns (planes, decoder, attention
                    values, beta, alpha, camera, focal) is bit-identical from call to call for identical inputs on the same
                    device and build: the field backward runs in its ordered mode (nfi_field_bwd_args.scatter_mode 2: sorted
                    plane-gradient gather, per-wave parameter slots summed in order) and the camera backward through
                    nfi_raygen_bwd_ordered, for any views_per_scene and either force_no_cam_grad.  Slower (DESIGN.md section
                    6).  The forward, its outputs and every inference path ignore it.  A use_viewdir model that needs a
                    gradient raises NotImplementedError (its per-ray feature gradient is summed with atomics); the staged
                    path's sampler closure, the regulariser branch (nfi_sdf_gradient_bwd_ordered) and the fused hand-off
                    backward (nfi_torgb_texels_bwd_ordered) take their own switch, generator.attach(...,
                    deterministic_backward=True), the augmentation warp (nfi_affine_warp_bwd_ordered) its own,
                    augment.configure(..., deterministic_backward=True); the producer and the view-direction decoder and
                    mapper are outside it, and torch.use_deterministic_algorithms is not consulted.

``render_views(fused, height, width, tform_cam2world, focal_length, depth_samples_per_ray, ...)`` renders from planes that
exist already (``generator.bake(model, model_input)``, or any sampler's ``.fused``) without calling a model: cameras
[B,V,4,4] or [B*V,4,4], V inferred; produce once, render many (turntable, viewer, the views of evaluate_inversion).
"""
import types

import torch

from . import nerf_utils, ops
from .autograd import differentiable, zeros_like_or
from .field_backward import field_query_bwd

args = None
dataset_config = None
_DEFAULTS = dict(termination_eps=0.0, strict_near_far=True, row_window=None, row_window_sync=False, views_per_scene=1,
                 deterministic_backward=False)
MAX_STASH_POINTS_PER_SCENE = 1 << 25      # nfi_field_query_bwd's binned scatter addresses a scene's points by 32-bit byte offsets
options = types.SimpleNamespace(**_DEFAULTS)


def _options(kw):
    unknown = set(kw) - set(_DEFAULTS)
    if unknown:
        raise TypeError('unknown render option(s) %s (known: %s)' % (sorted(unknown), sorted(_DEFAULTS)))
    return types.SimpleNamespace(**dict(_DEFAULTS, **kw))


def configure(new_args, new_dataset_config, **new_options):
    """Installs the globals run.py::render reads: args.{use_viewdir,use_sdf,attention_values,
    fine_sampling} and dataset_config['scene_range'|'white_background'], plus the options above."""
    global args, dataset_config, options
    args, dataset_config, options = new_args, new_dataset_config, _options(new_options)


def make_render(new_args, new_dataset_config, **new_options):
    """A render function bound to its own args / dataset_config / options (multi-config processes, one per thread)."""
    opts = _options(new_options)

    def bound(target_model, height, width, tform_cam2world, focal_length, center, bbox, model_input,
              depth_samples_per_ray, randomize=True, compute_normals=False, compute_semantics=False,
              compute_coords=False, extra_model_outputs=[], extra_model_inputs={}, force_no_cam_grad=False):
        return _render(new_args, new_dataset_config, opts, target_model, height, width, tform_cam2world, focal_length,
                       center, bbox, model_input, depth_samples_per_ray, randomize, compute_normals, compute_semantics,
                       compute_coords, extra_model_outputs, extra_model_inputs, force_no_cam_grad)
    bound.options = opts                 # (read by graphs.GraphedRender: a strict render cannot be captured)
    return bound


def render(target_model, height, width, tform_cam2world, focal_length, center, bbox, model_input,
           depth_samples_per_ray, randomize=True, compute_normals=False, compute_semantics=False,
           compute_coords=False, extra_model_outputs=[], extra_model_inputs={}, force_no_cam_grad=False):
    if args is None or dataset_config is None:
        raise RuntimeError('nerf_from_image_amd.render.configure(args, dataset_config) has not been called')
    return _render(args, dataset_config, options, target_model, height, width, tform_cam2world, focal_length, center,
                   bbox, model_input, depth_samples_per_ray, randomize, compute_normals, compute_semantics, compute_coords,
                   extra_model_outputs, extra_model_inputs, force_no_cam_grad)


def _strict(opts):
    v = opts.strict_near_far
    return v if v in ('deferred', 'after') else bool(v)


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and torch.is_tensor(t) and t.requires_grad for t in tensors)


def _render_with_stash(fused, height, width, S, cam, focal, bbox, center, noise_c, noise_f, white, cam_grad, fine=True,
                       strict=False, views_per_scene=1, deterministic=False):
    """The fused render as ONE autograd node (see the module docstring).  Gradients follow the reference's graph:
    rgb_map / mask -> sigma, rgb of every sample and (through dists * ||rd||) the ray directions; depth_map and the
    depth samples carry none; the field -> planes, decoder, colour table, beta, alpha and - unless the camera is
    detached - the query points -> rays -> tform_cam2world / focal_length.  fine=False: one pass of S samples
    (run.py without --fine_sampling).  With the view-direction decoder (fused.ray_features: --use_viewdir, carla) the
    per-ray feature of the ViewDirectionMapper and its output layer are inputs of the node too: their gradients go
    back into the PyTorch mapper and, through its view directions, into the camera.
    views_per_scene = V: `cam` holds V cameras per scene of `fused`, scene-major.  The stash is ray-major, so the V views of
    a scene are one contiguous run of points: the ONE field backward launch sees B scenes of V * H * W rays (an image
    V * H rows tall) and sums the plane, attention-value and decoder gradients of all views; camera and focal gradients
    stay per camera.
    deterministic: the backward's ordered mode (the option deterministic_backward; plain decoder only)."""
    texels, image = fused.texels, fused.decoder_image
    A, use_sdf, scene_range = fused.n_attention, fused.use_sdf, fused.scene_range
    w1, b1, w2, b2 = fused.decoder_params[:4]
    vd = fused.ray_features is not None
    B = cam.shape[0] // views_per_scene          # scenes: the batch of the field backward
    n_list = (2 if fine else 1) * S
    keep = {}

    def fwd(a_cam, a_focal, pl, a_w1, a_b1, a_w2, a_b2, att, be, al, *vd_in):
        out = ops.render_fwd(a_cam, a_focal, height, width, S, texels, image, scene_range, A, att, use_sdf, be, al,
                             bbox=bbox, center=center, noise_coarse=noise_c, noise_fine=noise_f, fine_sampling=fine,
                             white_background=bool(white), skip_missed_rays=True, stash=True,
                             ray_features=fused.ray_features, strict=strict, views_per_scene=views_per_scene)
        keep.update({k: out[k] for k in ('stash_t', 'stash_sigma', 'stash_rgb', 'ray_origins', 'ray_directions')})
        return out['rgb'], out['depth'], out['mask']

    def bwd(inputs, out_meta, grads, needs):
        a_cam, a_focal, pl, a_w1, a_b1, a_w2, a_b2, att, be, al = inputs[:10]
        g_rgb = zeros_like_or(grads[0], out_meta[0])
        g_mask = None if grads[2] is None else grads[2].contiguous()
        st_t, rd = keep['stash_t'], keep['ray_directions']
        full = cam_grad is True
        cb = ops.composite_bwd_stash(rd, st_t, keep['stash_sigma'], keep['stash_rgb'], g_rgb, g_mask,
                                     white_background=bool(white), want_rd=full, fine=fine)
        pts = ops.points_on_rays(keep['ray_origins'], rd, st_t).view(B, -1, 3)
        viewdir = dict(ray_features=fused.ray_features, samples_per_ray=n_list, w3=inputs[11]) if vd else None
        g = field_query_bwd(pts, texels, image, a_w1, a_w2, scene_range, A, att, use_sdf, be, al,
                            cb['g_sigma'].view(B, -1), cb['g_rgb'].view(B, -1, 3), want_points=bool(cam_grad),
                            viewdir=viewdir, ray_order=(n_list, width), scatter_mode=2 if deterministic else None)
        g_cam = g_focal = None
        if full:
            g_ro, g_rd = ops.points_bwd(g['g_points'].view(*st_t.shape, 3), st_t)
            g_rd = g_rd + cb['g_ray_directions']
            g_cam, g_focal = ops.raygen_bwd(height, width, a_focal, a_cam, bbox, center, True, g_ro, g_rd, ordered=deterministic)
        elif cam_grad == 'fine_origins':
            # force_no_cam_grad: only the origins of the FINE samples (stash columns S ...) are attached in the reference
            g_pts = g['g_points'].view(*st_t.shape, 3).clone()
            g_pts[..., :S, :] = 0.0
            g_ro, _ = ops.points_bwd(g_pts, st_t, want_rd=False)
            g_cam, _ = ops.raygen_bwd(height, width, a_focal, a_cam, bbox, center, True, g_ro, None, ordered=deterministic)
        g_planes = ops.texel_grad_to_planes(g['g_texels']) if needs[2] else None
        base = (g_cam, g_focal, g_planes, g['g_w1'], g['g_b1'], g['g_w2'], g['g_b2'], g.get('g_attention_values'),
                g.get('g_beta'), g.get('g_alpha'))
        if not vd:
            return base
        return base + (g['g_ray_features'].reshape(inputs[10].shape), g['g_w3'], g['g_b3'])

    cam_in = cam if cam_grad else cam.detach()
    focal_in = focal if (cam_grad is True or focal is None) else focal.detach()
    extra_in = tuple(fused.decoder_params[4:7]) if vd else ()          # (ray_feature [B,H,W,1,32], w3, b3)
    res = differentiable('render', fwd, cam_in, focal_in, fused.planes, w1, b1, w2, b2,
                         fused.attention_values if A > 0 else None, fused.beta if use_sdf else None,
                         fused.alpha if use_sdf else None, *extra_in, bwd=bwd, non_differentiable_outputs=(1,))
    return res


def _views(opts, n_images):
    """views_per_scene of the bound options, checked against the number of cameras of a call."""
    V = int(opts.views_per_scene)
    if V < 1 or n_images % V != 0:
        raise ValueError('views_per_scene = %d: %d cameras are not a whole number of scenes' % (V, n_images))
    return V


def _render(cfg, dcfg, opts, target_model, height, width, tform_cam2world, focal_length, center, bbox, model_input,
            depth_samples_per_ray, randomize=True, compute_normals=False, compute_semantics=False,
            compute_coords=False, extra_model_outputs=[], extra_model_inputs={}, force_no_cam_grad=False):
    S = depth_samples_per_ray
    if S > 512 or (S > 128 and cfg.fine_sampling):
        raise NotImplementedError('depth_samples_per_ray: at most 128 per pass with fine sampling, 512 without '
                                  '(run.py asks for 64 + 64, or 128 / 512 in one pass), got %d' % S)
    if compute_normals:
        assert cfg.use_sdf
    if compute_semantics:
        assert cfg.attention_values > 0

    B = tform_cam2world.shape[0]          # images: scenes x views_per_scene
    V = _views(opts, B)
    dev = tform_cam2world.device
    cam_grad = (not force_no_cam_grad) and _needs_grad(tform_cam2world, focal_length, bbox, center)
    if force_no_cam_grad and cfg.fine_sampling and _needs_grad(tform_cam2world, bbox, center):
        # run.py:211-214 detaches the COARSE query points, the depths and the ray directions - and then builds the fine pass's
        # points from the undetached ray origins (run.py:286-288): a camera that requires grad still receives
        # d loss / d origin of the fine samples (its translation; with an orthographic camera also its rotation).
        # Reproduced as is.
        cam_grad = "fine_origins"
    rows = height if opts.row_window is None else int(opts.row_window[1])

    # Order of the random draws as in the reference: the stratified jitter (rand_like inside
    # compute_query_points_from_rays, run.py:203-209) comes BEFORE target_model is called (whose synthesis network
    # draws its own noise in training), the inverse-CDF draw after it.
    rays = None
    viewdirs = None
    if cfg.use_viewdir:
        # run.py:192-219: the model needs the normalised ray directions before it can build the sampler
        rays = nerf_utils.get_ray_bundle_normalized(height, width, focal_length, tform_cam2world, bbox, center)
        viewdirs = (rays[1].detach() if force_no_cam_grad else rays[1]).unsqueeze(-2)
        if V > 1:
            # the V views of a scene as ONE image V * H rows tall: the model's batch is the scenes', and the per-ray MLP of
            # the ViewDirectionMapper (generator.py:223-251) returns its features in the same form
            viewdirs = viewdirs.reshape(B // V, V * height, width, 1, 3)
    noise_c = torch.rand((B, rows, width, S), dtype=torch.float32, device=dev) if randomize else None

    model_outputs = target_model(viewdirs, model_input, ['sampler'] + extra_model_outputs, extra_model_inputs)
    sampler = model_outputs['sampler']
    del model_outputs['sampler']
    fused = getattr(sampler, 'fused', None)
    if V > 1:
        first = model_input[0] if isinstance(model_input, (list, tuple)) else model_input
        scenes = fused.texels.shape[0] if fused is not None else first.shape[0]
        if B != V * scenes:
            raise ValueError('views_per_scene = %d: %d cameras for the %d scene(s) of the model call (expected %d)' % (
                V, B, scenes, V * scenes))
    out = _render_from_field(opts, fused, sampler, height, width, tform_cam2world, focal_length, center, bbox, S,
                             bool(cfg.fine_sampling), dcfg['scene_range'], dcfg['white_background'], randomize,
                             compute_normals, compute_semantics, compute_coords, noise_c, rays, cam_grad,
                             force_no_cam_grad, getattr(target_model, 'training', False))
    return out + (model_outputs,)


def render_views(fused, height, width, tform_cam2world, focal_length, depth_samples_per_ray, center=None, bbox=None,
                 randomize=True, fine_sampling=True, white_background=True, compute_normals=False,
                 compute_semantics=False, compute_coords=False, **render_options):
    """Renders views of scenes whose planes exist already: `fused` is a generator.FusedField (generator.bake(model, z), or
    the `.fused` of a sampler), no model is called.  Returns (rgb, depth, mask, normals, extra) as render() does.

    tform_cam2world: [B,V,4,4] or [B*V,4,4] (scene-major) for the B scenes of `fused`; V is inferred.  focal_length / bbox /
    center follow the cameras.  Takes the fused inference path, or the fused + stash node when the field's tensors or the
    cameras require a gradient; the random draws are render()'s, in its order.  What needs the staged path - the 'bbox'
    overlay, extra maps with a gradient, a field with ray features (the view-direction decoder: its field depends on the
    cameras) - raises NotImplementedError: call render() with the option views_per_scene for those.  `render_options` are
    render()'s options (views_per_scene is inferred, not passed)."""
    scenes = fused.texels.shape[0]
    if tform_cam2world.dim() == 4:
        if tform_cam2world.shape[0] != scenes:
            raise ValueError('render_views: cameras [%d,%d,4,4] for a field of %d scene(s): the leading dimension is the scenes\''
                             % (tform_cam2world.shape[0], tform_cam2world.shape[1], scenes))
        # [B,V,...] -> scene-major [B*V,...]: cameras [.,4,4], focal [.], bbox [.,2,2], center [.,2]
        tform_cam2world = tform_cam2world.flatten(0, 1)
        focal_length = focal_length.flatten(0, 1) if focal_length is not None and focal_length.dim() == 2 else focal_length
        bbox = bbox.flatten(0, 1) if bbox is not None and bbox.dim() == 4 else bbox
        center = center.flatten(0, 1) if center is not None and center.dim() == 3 else center
    if 'views_per_scene' in render_options:
        raise TypeError('render_views infers views_per_scene from the cameras and the field')
    B = tform_cam2world.shape[0]
    if B == 0 or B % scenes != 0:
        raise ValueError('render_views: %d cameras are not a whole number of views of the field\'s %d scene(s)' % (B, scenes))
    if getattr(fused, 'ray_features', None) is not None:
        raise NotImplementedError('render_views: a field with ray features (view-direction decoder) depends on the cameras; '
                                  'use render() with the option views_per_scene')
    opts = _options(dict(render_options, views_per_scene=B // scenes))
    S = depth_samples_per_ray
    if S > 512 or (S > 128 and fine_sampling):
        raise NotImplementedError('depth_samples_per_ray: at most 128 per pass with fine sampling, 512 without, got %d' % S)
    rows = height if opts.row_window is None else int(opts.row_window[1])
    noise_c = torch.rand((B, rows, width, S), dtype=torch.float32, device=tform_cam2world.device) if randomize else None
    cam_grad = _needs_grad(tform_cam2world, focal_length, bbox, center)
    return _render_from_field(opts, fused, None, height, width, tform_cam2world, focal_length, center, bbox, S,
                              bool(fine_sampling), fused.scene_range, white_background, randomize, compute_normals,
                              compute_semantics, compute_coords, noise_c, None, cam_grad, False, False)


def _render_from_field(opts, fused, sampler, height, width, tform_cam2world, focal_length, center, bbox, S, fine_sampling,
                       scene_range, white, randomize, compute_normals, compute_semantics, compute_coords, noise_c, rays,
                       cam_grad, force_no_cam_grad, training):
    """Everything of a render behind the model call - THE path selection, shared by render() (sampler = the model's) and
    render_views() (sampler = None: what would need the staged path raises).  noise_c: the stratified jitter, drawn by the
    caller (before its model call); rays: the normalised ray bundle if the caller needed it already.
    Returns (rgb, depth, mask, normals, extra)."""
    B = tform_cam2world.shape[0]
    V = int(opts.views_per_scene)
    dev = tform_cam2world.device
    rows = height if opts.row_window is None else int(opts.row_window[1])
    plain = not (compute_normals or compute_semantics or compute_coords)
    ray_features = getattr(fused, 'ray_features', None)

    def inverse_cdf_draws():
        if not fine_sampling:
            return None
        if randomize:
            return torch.rand([B * rows * width, S], dtype=torch.float32, device=dev)
        return None            # the kernels take linspace(0, 1, S) themselves (nerf_utils.py:196-200)

    # semantics / coords / normals are composited by the fused kernel itself (any texel storage; with the view-direction
    # decoder: fp32 texels); the 'bbox' overlay (which edits sigma, generator.py:645-659) and 16-bit texels with the
    # view-direction decoder keep the staged path
    # (with the view-direction decoder the kernel composites semantics / coords / normals on fp32 texels)
    fused_maps = plain or (not getattr(fused, 'bbox_overlay', False) and
                           (ray_features is None or fused.texels.dtype == torch.float32))
    if compute_normals and fused is not None:
        # the sampler's own condition (generator.py:599-602; torch.is_grad_enabled() is autograd's business there)
        assert fused.use_sdf and not training
    # (one pass of 129..512 samples - no fine sampling, checked above - has its own fused kernel: plain maps only)
    if fused is not None and fused_maps and not cam_grad and not fused.requires_grad and (S <= 128 or plain):
        # ---------------- fused inference path (the kernel generates the rays itself) ----------------
        window = None if opts.row_window is None else (int(opts.row_window[0]), height)
        extras = not plain
        ws = None
        if window is not None and opts.row_window_sync:
            from . import parallel
            ws = ops.render_setup(tform_cam2world.detach(), None if focal_length is None else focal_length.detach(), rows,
                                  width, scene_range, bbox=None if bbox is None else bbox.detach(),
                                  center=None if center is None else center.detach(), row_window=window)
            parallel.allreduce_ray_setup(ws, None if opts.row_window_sync is True else opts.row_window_sync)
        out = ops.render_fwd(
            tform_cam2world.detach(), None if focal_length is None else focal_length.detach(), rows, width, S,
            fused.texels, fused.decoder_image, scene_range, fused.n_attention,
            None if fused.attention_values is None else fused.attention_values.detach(), fused.use_sdf,
            None if fused.beta is None else fused.beta.detach(), None if fused.alpha is None else fused.alpha.detach(),
            bbox=None if bbox is None else bbox.detach(), center=None if center is None else center.detach(),
            noise_coarse=noise_c, noise_fine=inverse_cdf_draws(), fine_sampling=fine_sampling,
            white_background=bool(white), skip_missed_rays=True, ray_features=ray_features,
            termination_eps=opts.termination_eps if (fine_sampling and not extras and ray_features is None) else 0.0,
            row_window=window, want_semantics=compute_semantics and not compute_coords, want_coords=compute_coords,
            want_normals=compute_normals, workspace=ws, rays_ready=ws is not None,
            # a band's own hit count says nothing about the image (the top rows of a centred object are all background):
            # the check applies to the whole image - every call without a window, windowed calls only once
            # row_window_sync has summed the count over the bands
            strict=_strict(opts) if (window is None or ws is not None) else False, views_per_scene=V)
        # run.py:337-338: coords take the semantics slot of render_volume_density when both are asked for
        extra_map = out['coords'] if compute_coords else (out['semantics'] if compute_semantics else None)
        return out['rgb'], out['depth'], out['mask'], out.get('normals'), extra_map
    if opts.row_window is not None:
        raise NotImplementedError('row_window is an option of the fused inference path (no gradient, no extra maps)')
    if opts.deterministic_backward and ray_features is not None:
        raise NotImplementedError('deterministic_backward: the view-direction decoder has no ordered backward (its per-ray '
                                  'feature gradient is summed with atomics)')

    if fused is not None and plain and (ray_features is None or fused.texels.dtype == torch.float32):
        # ---------------- fused render + stash as one differentiable node ----------------
        # (with or without fine sampling, plain or view-direction decoder; the view-direction rays of run.py:216-222 were
        #  computed above for the model - the kernel regenerates the same rays, and the camera gradient of the viewdirs
        #  flows through the PyTorch mapper into that first ray op)
        points_per_scene = V * height * width * (2 if fine_sampling else 1) * S
        if points_per_scene > MAX_STASH_POINTS_PER_SCENE:
            # refused here, before the render launch and the stash: the backward of this node is ONE field backward launch
            raise ValueError('render with a gradient: %d views x %d x %d rays x %d samples = %d points per scene, above the '
                             'field backward\'s limit of 2^25 = %d points per scene (render fewer views per call)' % (
                                 V, height, width, (2 if fine_sampling else 1) * S, points_per_scene,
                                 MAX_STASH_POINTS_PER_SCENE))
        det = (lambda t: None if t is None else t.detach())
        rgb_map, depth_map, mask = _render_with_stash(
            fused, height, width, S, tform_cam2world, focal_length, det(bbox), det(center), noise_c, inverse_cdf_draws(),
            white, cam_grad, fine=fine_sampling, strict=_strict(opts), views_per_scene=V,
            deterministic=bool(opts.deterministic_backward))
        return rgb_map, depth_map, mask, None, None

    # ---------------- staged path (extra maps with a gradient or over a pass of more than 128 samples) ----------------
    if sampler is None:
        raise NotImplementedError('render_views: this call needs the staged path (the bbox overlay, extra maps with a '
                                  'gradient or over more than 128 samples); use render() with the option views_per_scene')
    ray_origins, ray_directions = rays if rays is not None else nerf_utils.get_ray_bundle_normalized(
        height, width, focal_length, tform_cam2world, bbox, center)
    if V > 1:
        # the V views of a scene are ONE image V * H rows tall: everything below is per ray or per scene
        tall = (lambda t: t.reshape(B // V, V * height, *t.shape[2:]))
        ray_origins, ray_directions = tall(ray_origins), tall(ray_directions)
        noise_c = None if noise_c is None else tall(noise_c)
    with torch.no_grad():
        # (the staged path has one place to look at the counter - behind the near / far launch: 'after' is True here)
        near, far = nerf_utils.compute_near_far_planes(ray_origins.detach(), ray_directions.detach(), scene_range,
                                                       strict=True if _strict(opts) == 'after' else _strict(opts))
    query_points, depth_values = nerf_utils.compute_query_points_from_rays(
        ray_origins, ray_directions, near, far, S, randomize=randomize, noise=noise_c)
    if force_no_cam_grad:
        query_points, depth_values = query_points.detach(), depth_values.detach()
        ray_directions = ray_directions.detach()

    req = ['sigma', 'rgb']
    if compute_normals:
        req.append('normals')
    if compute_semantics:
        req.append('semantics')
    if compute_coords:
        req.append('coords')
    shp = query_points.shape[:-1]

    def unpack(o):
        sig = o['sigma'].view(*shp)
        col = o['rgb'].view(*shp, 3)
        nor = o['normals'].view(*shp, -1) if compute_normals else None
        sem = o['semantics'].view(*shp, -1) if compute_semantics else None
        coo = o['coords'].view(*shp, -1) if compute_coords else None
        return sig, col, nor, sem, coo
    # our own closure (it carries .fused): the fused renderer's split-fp16 decoder arithmetic in this path too
    hip_kw = {'mlp_split_fp16': True} if hasattr(sampler, 'fused') else {}
    sigma, rgb, normals, semantics, coords = unpack(sampler(query_points, req, **hip_kw))

    extra = coords if coords is not None else semantics      # run.py:337-338: coords hijack the semantics slot
    if fine_sampling:
        with torch.no_grad():
            if randomize:
                u = torch.rand([B * height * width, S], dtype=torch.float32, device=dev)
            else:
                u = torch.linspace(0.0, 1.0, steps=S, dtype=torch.float32, device=dev).expand(B * height * width, S)
            z_samples, _ = ops.resample(sigma.detach(), ray_directions.detach(), depth_values.detach(), u)
            z_samples = z_samples.view(*depth_values.shape[:3], S)
        # (force_no_cam_grad: the directions are detached above, the ORIGINS are not - run.py:286-288 builds the fine points from
        #  them as they are, so their gradient reaches the camera)
        query_fine = nerf_utils.points_on_rays(ray_origins, ray_directions, z_samples)
        sigma_f, rgb_f, normals_f, semantics_f, coords_f = unpack(sampler(query_fine, req, **hip_kw))
        extra_f = coords_f if coords_f is not None else semantics_f
        maps = nerf_utils.merge_and_composite(
            ray_directions, depth_values, sigma, rgb, z_samples, sigma_f, rgb_f, normals, normals_f, extra, extra_f,
            white_background=white)
    else:
        maps = nerf_utils.render_volume_density(
            sigma, rgb, ray_origins, ray_directions, depth_values, normals, extra, white_background=white)
    if V > 1:
        # back to one image per camera: (rgb, depth, mask, normals, extra) [B/V, V*H, W, ...] -> [B, H, W, ...]
        maps = tuple(None if t is None else t.reshape(B, height, *t.shape[2:]) for t in maps)
    return tuple(maps)
