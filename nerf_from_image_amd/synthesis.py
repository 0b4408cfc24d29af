"""The tail of every synthesis layer of the plane producer as one HIP node.

After its 3x3 (transposed) convolution, the reference's ``SynthesisLayer.forward`` (models/stylegan.py:325-356) runs a chain
of full-size memory passes: for ``up`` layers the 4x4 resample filter as a single-channel ``F.conv2d`` on
``[B*C,1,2n+1,2n+1]`` (filter2d, stylegan.py:58-69, 101-105), then ``addcmul(noise, x, dcoefs)`` (140), ``+ bias`` (351),
``* act_gain`` (353) and ``leaky_relu`` (355) - and autograd mirrors each in the backward.  ``layer_tail`` is that chain
as ONE launch forward (``nfi_synth_tail_fwd``: the convolution's output read once, the result written once) and at most
two launches backward plus one for the noise gradient (``nfi_synth_tail_bwd``, every sum in a fixed order: the gradients
repeat bit for bit).  The convolutions stay PyTorch / MIOpen.

The head - everything before the convolution - is opt-in on top of that (``fuse_layers(net, head=True)``): ``layer_styles`` is
the affine and the demodulation coefficients (stylegan.py:173-177, 127-130; ``nfi_synth_head_fwd``, two launches, the
``[B,O,I,3,3]`` product never formed; backward at most four launches) and ``modulate`` is ``x * styles`` (132;
``nfi_synth_modulate_fwd`` / ``_bwd``, one launch each).  With the head on, every output layer (toRGB, stylegan.py:372-380)
gets a fused forward too: the two nodes, its 1x1 ``F.conv2d`` and the bias.

    import nerf_from_image_amd.synthesis as nfi_synthesis
    nfi_synthesis.fuse_layers(model.synthesis_network)             # or attach(model, fused_synthesis_tail=True)
    nfi_synthesis.fuse_layers(model.synthesis_network, head=True)  # or attach(model, fused_synthesis_head=True)

``fuse_layers`` swaps the ``forward`` of every synthesis layer - found by its attributes, not its class - for
``fused_layer_forward``; parameters, buffers and ``state_dict`` keys are untouched, and ``handoff.fuse_last_block`` composes
with it (that block calls ``self.conv0`` / ``self.conv1`` as modules).

Limits: first-order only (a forward that asks for ``path_length`` runs under ``with unfused(net):``, as generator.py does),
float32 NCHW, 4x4 taps (any values; read from the layer's ``resample_filter`` buffer on the device at every call).
"""
import types

import torch
import torch.nn.functional as F

from . import ops
from .autograd import differentiable

OUTPUT_LAYER_ATTRS = ('affine', 'weight', 'bias', 'weight_gain')           # and no 'up': OutputLayer (stylegan.py:359-380)
LAYER_ATTRS = ('affine', 'weight', 'bias', 'resample_filter', 'up', 'use_noise', 'activate', 'act_gain', 'padding', 'resolution')


def layer_tail(y, dcoefs, noise, bias, resample_filter, act_gain, up, activate=True, slope=0.2):
    """Differentiable fused tail: y [B,C,2n+1,2n+1] with up (R = 2n) or [B,C,R,R]; dcoefs [B,C]; noise None, [B,1,R,R] or
    [R,R]; bias [C]; resample_filter [4,4] (a buffer: no gradient) ->
    lrelu_slope(((noise + filter(y) * dcoefs) + bias) * act_gain), [B,C,R,R].  act_gain must be positive."""
    # checked once: the node's forward and backward launch on these very tensors (dense float32 already, or made so here)
    kw = ops.synth_tail_args(y, dcoefs, noise, bias, resample_filter.detach() if up else None, float(act_gain), bool(up), bool(activate),
                             float(slope), 'layer_tail')
    has_noise = noise is not None

    def packed(args):
        return dict(kw, y=args[0], dcoefs=args[1], bias=args[2], noise=args[3] if has_noise else None)

    def fwd(*args):
        return ops.synth_tail_launch(packed(args))

    def bwd(inputs, out_meta, grads, needs, kept):
        if grads[0] is None or not any(needs):
            return (None,) * len(inputs)
        g = ops.synth_tail_bwd_launch(packed(inputs), grads[0].contiguous(), kept[0], bool(needs[0]), bool(needs[1]), bool(needs[2]),
                                      has_noise and bool(needs[3]))
        return (g.get('g_y'), g.get('g_dcoefs'), g.get('g_bias')) + ((g.get('g_noise'),) if has_noise else ())
    args = (kw['y'], kw['dcoefs'], kw['bias']) + ((kw['noise'],) if has_noise else ())
    return differentiable('synth_tail', fwd, *args, bwd=bwd, saved_outputs=(0,))


def layer_styles(w, affine, conv_weight, demodulate=True, style_gain=1.0):
    """Differentiable fused head: w [B,D] (a view with unit stride along D is read in place: ws.unbind(1)[k]); affine an
    EqualizedLinear-style module (weight [I,D], bias [I] or None, weight_gain, bias_gain; stylegan.py:148-180, no activation);
    conv_weight [O,I,kh,kw] -> (styles [B,I] = affine(w) * style_gain, dcoefs [B,O] = rsqrt(sum_i styles^2 sum_k weight^2 + 1e-8)
    or None without demodulate).  conv_weight's gradient is the demodulation's share only (the convolution adds its own)."""
    if getattr(affine, 'activate', False):
        raise RuntimeError('layer_styles: an affine with an activation is not supported')
    has_bias = getattr(affine, 'bias', None) is not None
    # checked once: the node's forward and backward launch on these very tensors
    kw = ops.synth_head_args(w, affine.weight, affine.bias if has_bias else None, affine.weight_gain, affine.bias_gain, conv_weight,
                             bool(demodulate), float(style_gain), 'layer_styles')
    shape = tuple(conv_weight.shape)

    def packed(args):
        return dict(kw, latent=args[0], affine_weight=args[1], weight=args[2], affine_bias=args[3] if has_bias else None)

    def fwd(*args):
        styles, dcoefs = ops.synth_head_launch(packed(args))
        return (styles, dcoefs) if demodulate else styles

    def bwd(inputs, out_meta, grads, needs, kept):
        g_styles = None if grads[0] is None else grads[0].contiguous()
        g_dcoefs = None if not demodulate or grads[1] is None else grads[1].contiguous()
        need_weight = bool(needs[2]) and g_dcoefs is not None
        need_bias = has_bias and bool(needs[3])
        if (g_styles is None and g_dcoefs is None) or not (needs[0] or needs[1] or need_weight or need_bias):
            return (None,) * len(inputs)
        g = ops.synth_head_bwd_launch(packed(inputs), g_styles, g_dcoefs, kept[0], kept[1] if demodulate else None, bool(needs[0]),
                                      bool(needs[1]), need_bias, need_weight)
        g_weight = g.get('g_weight')
        return (g.get('g_latent'), g.get('g_affine_weight'), None if g_weight is None else g_weight.view(shape)) + \
            ((g.get('g_affine_bias'),) if has_bias else ())
    args = (kw['latent'], kw['affine_weight'], kw['weight']) + ((kw['affine_bias'],) if has_bias else ())
    out = differentiable('synth_head', fwd, *args, bwd=bwd, saved_outputs=(0, 1) if demodulate else (0,))
    return out if demodulate else (out, None)


def modulate(x, styles):
    """Differentiable x * styles.reshape(B, -1, 1, 1) (stylegan.py:132): x [B,C,H,W], styles [B,C] -> dense [B,C,H,W].  One launch
    forward, one backward (g_x, and g_styles summed in a fixed order)."""
    kw = ops.synth_modulate_args(x, styles, 'modulate')

    def fwd(a_x, a_s):
        return ops.synth_modulate_launch(dict(kw, x=a_x, styles=a_s))

    def bwd(inputs, out_meta, grads, needs):
        if grads[0] is None or not any(needs):
            return (None, None)
        return ops.synth_modulate_bwd_launch(dict(kw, x=inputs[0], styles=inputs[1]), grads[0].contiguous(), bool(needs[0]), bool(needs[1]))
    return differentiable('synth_modulate', fwd, kw['x'], kw['styles'], bwd=bwd)


def fused_layer_forward(self, x, w, noise_mode='random', gain=1):
    """SynthesisLayer.forward (models/stylegan.py:325-356) with everything after the convolution on the HIP kernel - and,
    where fuse_layers was called with head=True, everything before it as well.  The affine, the noise decision and the
    torch.randn call are the reference's, in its order: a seeded run draws the same noise."""
    assert noise_mode in ['random', 'const']
    head = getattr(self, '_nfi_fused_head', False)
    if head:
        styles, dcoefs = layer_styles(w, self.affine, self.weight)
    else:
        styles = self.affine(w)

    noise = None
    if (self.use_noise and noise_mode == 'random' and (self.training or self.noise_strength != 0)):
        noise = torch.randn([x.shape[0], 1, self.resolution, self.resolution], device=x.device) * self.noise_strength
    if (self.use_noise and noise_mode == 'const' and self.noise_strength != 0):
        noise = self.noise_const * self.noise_strength

    # conv_modulated2d (stylegan.py:114-145) up to its convolution
    if head:
        x = modulate(x, styles)
    else:
        bs = x.shape[0]
        wm = self.weight.unsqueeze(0) * styles.reshape(bs, 1, -1, 1, 1)
        dcoefs = (wm.square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()
        x = x * styles.reshape(bs, -1, 1, 1)
    if self.up:
        assert self.padding == 1
        y = F.conv_transpose2d(x, self.weight.transpose(0, 1), stride=2)
    else:
        y = F.conv2d(x, self.weight, padding=self.padding)
    return layer_tail(y, dcoefs, noise, self.bias, self.resample_filter, self.act_gain * gain, self.up, self.activate)


def fused_output_forward(self, x, w):
    """OutputLayer.forward (models/stylegan.py:372-380): the styles (times weight_gain) and the modulation on the HIP nodes,
    the 1x1 convolution (conv_modulated2d without demodulation: F.conv2d, no padding) and the bias as the reference has them."""
    styles, _ = layer_styles(w, self.affine, self.weight, demodulate=False, style_gain=self.weight_gain)
    x = F.conv2d(modulate(x, styles), self.weight)
    return x + self.bias.view([-1 if dim == 1 else 1 for dim in range(x.ndim)])


def output_layers(synthesis_network):
    """The output (toRGB) layers of the network, in module order: every sub-module with ``affine``, ``weight``, ``bias`` and
    ``weight_gain`` and without ``up`` (no class is named).  May be empty."""
    return [m for m in synthesis_network.modules() if all(hasattr(m, a) for a in OUTPUT_LAYER_ATTRS) and not hasattr(m, 'up')]


def synthesis_layers(synthesis_network):
    """The synthesis layers of a StyleGAN2-style network, in module order: every sub-module with the attributes
    ``fused_layer_forward`` reads (no class is named)."""
    layers = [m for m in synthesis_network.modules() if all(hasattr(m, a) for a in LAYER_ATTRS)]
    if not layers:
        raise AttributeError('fuse_layers: the network has no StyleGAN2-style synthesis layer (a module with %s)' % (LAYER_ATTRS,))
    return layers


def fuse_layers(synthesis_network, head=False):
    """Swaps the forward of every synthesis layer for ``fused_layer_forward``.  Returns the layers.
    head=True: the layers' heads run on the HIP nodes too (``layer_styles``, ``modulate``) and every output layer gets
    ``fused_output_forward``; head=False (the default) leaves the heads PyTorch's and the output layers their own forward -
    on a network fused with head=True before, it puts both back."""
    layers = synthesis_layers(synthesis_network)
    for m in layers:
        if not hasattr(m, '_nfi_original_forward'):
            m._nfi_original_forward = m.forward
            m.forward = types.MethodType(fused_layer_forward, m)
        m._nfi_fused_head = bool(head)
    for m in output_layers(synthesis_network):
        if head and not hasattr(m, '_nfi_original_forward'):
            m._nfi_original_forward = m.forward
            m.forward = types.MethodType(fused_output_forward, m)
            m._nfi_fused_head = True
        elif not head:
            _restore(m)
    return layers


def _restore(m):
    if hasattr(m, '_nfi_original_forward'):
        m.forward = m._nfi_original_forward
        del m._nfi_original_forward
    if hasattr(m, '_nfi_fused_head'):
        del m._nfi_fused_head


def fused_layers(synthesis_network):
    """The layers ``fuse_layers`` has fused (an empty list for a network with none, fused or at all)."""
    try:
        layers = synthesis_layers(synthesis_network)
    except AttributeError:
        return []
    return [m for m in layers if hasattr(m, '_nfi_original_forward')]


def fused_output_layers(synthesis_network):
    """The output layers ``fuse_layers(net, head=True)`` has fused (an empty list without the head)."""
    return [m for m in output_layers(synthesis_network) if hasattr(m, '_nfi_original_forward')]


def head_fused(synthesis_network):
    """True where ``fuse_layers(net, head=True)`` is in effect."""
    return any(getattr(m, '_nfi_fused_head', False) for m in fused_layers(synthesis_network))


class unfused:
    """``with unfused(net):`` - the original forward of every fused layer, output layers included, for the duration of the
    block (no-op when none is fused)."""

    def __init__(self, synthesis_network):
        self.net = synthesis_network
        self.swapped = []

    def __enter__(self):
        for m in fused_layers(self.net) + fused_output_layers(self.net):
            self.swapped.append((m, m.forward))
            m.forward = m._nfi_original_forward
        return self

    def __exit__(self, *exc):
        for m, fused in self.swapped:
            m.forward = fused
        self.swapped = []
        return False


def unfuse_layers(synthesis_network):
    layers = synthesis_layers(synthesis_network)
    for m in layers + output_layers(synthesis_network):
        _restore(m)
    return layers
