"""Autograd glue between the HIP kernels and PyTorch.

Every host-level op goes through :func:`differentiable`: the forward runs the HIP kernel(s); if
any input requires grad, the call is recorded as ONE autograd node whose backward is the ``bwd``
closure handed in by the op (it launches the HIP backward kernels).  An op without a backward
fails loudly when a gradient is actually requested; nothing ever falls back to ATen.  The nodes are
first-order only: ``torch.autograd.grad(..., create_graph=True)`` THROUGH a node raises (the one
second-order path of the reference that touches the renderer's neighbourhood, the path-length
regulariser of the plane producer, is kept off the fused hand-off node: generator.hip_forward).

Lifetime: the node keeps its INPUTS through ``save_for_backward`` and, of its outputs, only their
shape/dtype/device (:class:`OutputMeta`).  Keeping an output tensor as an attribute on ``ctx`` would
close the cycle output -> grad_fn -> ctx -> output, which the reference-counting of autograd never
frees: every step would leak its per-sample tensors.  An op whose backward reads an output (the
synthesis tail takes the sign of the pre-activation from it) names it in ``saved_outputs``: it then
goes through ``save_for_backward`` too, where autograd stores an output WITHOUT its ``grad_fn`` and
re-attaches it on unpacking, so no cycle forms; the backward closure gets those tensors as its
fifth argument.
"""
import torch


class OutputMeta:
    """What a backward closure may know about a forward output without keeping it alive."""
    __slots__ = ('shape', 'dtype', 'device')

    def __init__(self, t):
        self.shape, self.dtype, self.device = tuple(t.shape), t.dtype, t.device

    def zeros(self):
        return torch.zeros(self.shape, dtype=self.dtype, device=self.device)


class _HipNode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, name, fn, bwd, nondiff, *tensors):
        ctx.name = name
        ctx.bwd = bwd
        nondiff, keep = nondiff
        with torch.no_grad():
            out = fn(*tensors)
        outs = (out,) if not isinstance(out, tuple) else out
        # outputs in `keep` go through save_for_backward as well: autograd holds a saved OUTPUT without its grad_fn, so no
        # cycle forms (an attribute on ctx would close one, see the module docstring)
        ctx.n_inputs = len(tensors)
        ctx.save_for_backward(*tensors, *(outs[i] for i in keep))
        ctx.out_meta = tuple(None if o is None else OutputMeta(o) for o in outs)
        nd = [outs[i] for i in nondiff if i < len(outs) and outs[i] is not None]
        nd += [o for o in outs if o is not None and not o.dtype.is_floating_point]
        if nd:
            ctx.mark_non_differentiable(*nd)
        return out

    @staticmethod
    def backward(ctx, *grads):
        if torch.is_grad_enabled():
            # the engine runs backward functions with grad mode ON only under create_graph=True.  The HIP backward
            # kernels record no graph, so the node would silently act as a constant in the second-order graph
            # (once_differentiable does not catch it either when the incoming gradients carry no graph themselves)
            raise RuntimeError(
                'nerf_from_image_amd: %s is first-order only - torch.autograd.grad(..., create_graph=True) / a double '
                'backward through a HIP node is not supported (the reference needs it for the path-length output of '
                'the plane producer only; keep HIP nodes out of that graph, see handoff.unfused)' % ctx.name)
        if ctx.bwd is None:
            raise NotImplementedError(
                'nerf_from_image_amd: %s has no HIP backward (forward-only op); wrap the call in '
                'torch.no_grad() or detach its inputs' % ctx.name)
        with torch.no_grad():
            saved = ctx.saved_tensors
            kept = (saved[ctx.n_inputs:],) if len(saved) > ctx.n_inputs else ()
            gin = ctx.bwd(saved[:ctx.n_inputs], ctx.out_meta, grads, ctx.needs_input_grad[4:], *kept)
        gin = tuple(g if need else None for g, need in zip(gin, ctx.needs_input_grad[4:]))
        return (None, None, None, None) + gin


def differentiable(name, fn, *tensors, bwd=None, non_differentiable_outputs=(), saved_outputs=()):
    """Runs fn(*tensors) (HIP kernels).  Records an autograd node only when a gradient can be asked for.

    bwd(inputs, output_meta, grad_outputs, needs) -> tuple of gradients, one per input (None allowed);
    output_meta[i] is an :class:`OutputMeta` (shape / dtype / device of output i), never the tensor.
    saved_outputs: indices of outputs the backward reads (saved the way autograd saves an output, which forms no cycle);
    bwd then gets them as a fifth argument, a tuple in that order."""
    needs = torch.is_grad_enabled() and any(t is not None and torch.is_tensor(t) and t.requires_grad for t in tensors)
    if not needs:
        with torch.no_grad():
            return fn(*tensors)
    return _HipNode.apply(name, fn, bwd, (tuple(non_differentiable_outputs), tuple(saved_outputs)), *tensors)


def zeros_like_or(g, ref):
    """Autograd hands None for outputs nobody used; kernels want dense tensors.  ref: tensor or OutputMeta."""
    if g is None:
        return ref.zeros() if isinstance(ref, OutputMeta) else torch.zeros_like(ref)
    return g.contiguous()


class PoseToMatrix(torch.autograd.Function):
    """lib/pose_utils.py:48-70 as ONE node: (z0 or None, t2, s, q, camera_flipped, normalize) -> (cam2world, focal or None).
    One launch forward, one backward (ops.pose_to_matrix / pose_to_matrix_bwd: thread = image, no atomics, so the pose
    gradients repeat bit for bit); inputs that need no gradient get None.  First-order only, like every node here."""

    @staticmethod
    def forward(ctx, z0, t2, s, q, camera_flipped, normalize):
        from . import ops
        ctx.flags = (bool(camera_flipped), bool(normalize))
        ctx.perspective = z0 is not None
        ctx.save_for_backward(*(t for t in (z0, t2, s, q) if t is not None))
        cam2world, focal = ops.pose_to_matrix(q, t2, s, z0, *ctx.flags)
        return cam2world, focal

    @staticmethod
    def backward(ctx, g_cam2world, g_focal):
        from . import ops
        if torch.is_grad_enabled():
            raise RuntimeError('nerf_from_image_amd: pose_to_matrix is first-order only - torch.autograd.grad(..., '
                               'create_graph=True) / a double backward through a HIP node is not supported')
        z0, t2, s, q = ctx.saved_tensors if ctx.perspective else (None,) + tuple(ctx.saved_tensors)
        with torch.no_grad():
            if g_cam2world is None:
                g_cam2world = torch.zeros((q.shape[0], 4, 4), dtype=torch.float32, device=q.device)
            need_z0, need_t2, need_s, need_q = ctx.needs_input_grad[:4]
            g_q, g_t2, g_s, g_z0 = ops.pose_to_matrix_bwd(g_cam2world, g_focal, q, t2, s, z0, *ctx.flags,
                                                          needs=(need_q, need_t2, need_s, need_z0))
        return g_z0, g_t2, g_s, g_q, None, None


class LpipsHead(torch.autograd.Function):
    """One layer of the LPIPS distance head as ONE node (ops.lpips_head / lpips_head_bwd; lib/metrics.py:104-110, 130-133):
    (x, y [B,C,H,W], weight [C], y_normalized, eps) -> [B].  Saves x, y and weight - the forward stashes nothing else, the
    backward recomputes the norms - and returns gradients for whichever of x / y need them, in one launch.  The weight
    is frozen, as the reference freezes the net (lib/metrics.py:102): one that requires grad raises.  First-order only."""

    @staticmethod
    def forward(ctx, x, y, weight, y_normalized, eps):
        from . import ops
        if weight.requires_grad:
            raise RuntimeError('nerf_from_image_amd: lpips_head has no gradient for the lin weights (the reference freezes '
                               'the net, lib/metrics.py:102): call requires_grad_(False) on the LPIPS module')
        ctx.flags = (bool(y_normalized), float(eps))
        ctx.save_for_backward(x, y, weight)
        return ops.lpips_head(x, y, weight, *ctx.flags)

    @staticmethod
    def backward(ctx, g_out):
        from . import ops
        if torch.is_grad_enabled():
            raise RuntimeError('nerf_from_image_amd: lpips_head is first-order only - torch.autograd.grad(..., '
                               'create_graph=True) / a double backward through a HIP node is not supported')
        x, y, weight = ctx.saved_tensors
        need_x, need_y = ctx.needs_input_grad[:2]
        with torch.no_grad():
            g_x, g_y = ops.lpips_head_bwd(g_out, x, y, weight, *ctx.flags, need_x=need_x, need_y=need_y)
        return g_x, g_y, None, None, None
