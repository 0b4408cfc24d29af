"""The tail of every synthesis layer of the plane producer as one HIP node.

After its 3x3 (transposed) convolution, the reference's ``SynthesisLayer.forward`` (models/stylegan.py:325-356) runs a chain
of full-size memory passes: for ``up`` layers the 4x4 resample filter as a single-channel ``F.conv2d`` on
``[B*C,1,2n+1,2n+1]`` (filter2d, stylegan.py:58-69, 101-105), then ``addcmul(noise, x, dcoefs)`` (140), ``+ bias`` (351),
``* act_gain`` (353) and ``leaky_relu`` (355) - and autograd mirrors each in the backward.  ``layer_tail`` is that chain
as ONE launch forward (``nfi_synth_tail_fwd``: the convolution's output read once, the result written once) and at most
two launches backward plus one for the noise gradient (``nfi_synth_tail_bwd``, every sum in a fixed order: the gradients
repeat bit for bit).  The convolutions, ``x * styles`` and the ``dcoefs`` expression stay PyTorch / MIOpen.

    import nerf_from_image_amd.synthesis as nfi_synthesis
    nfi_synthesis.fuse_layers(model.synthesis_network)             # or attach(model, fused_synthesis_tail=True)

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

LAYER_ATTRS = ('affine', 'weight', 'bias', 'resample_filter', 'up', 'use_noise', 'activate', 'act_gain', 'padding', 'resolution')


def layer_tail(y, dcoefs, noise, bias, resample_filter, act_gain, up, activate=True, slope=0.2):
    """Differentiable fused tail: y [B,C,2n+1,2n+1] with up (R = 2n) or [B,C,R,R]; dcoefs [B,C]; noise None, [B,1,R,R] or
    [R,R]; bias [C]; resample_filter [4,4] (a buffer: no gradient) ->
    lrelu_slope(((noise + filter(y) * dcoefs) + bias) * act_gain), [B,C,R,R].  act_gain must be positive."""
    for t, name in ((y, 'y'), (dcoefs, 'dcoefs'), (noise, 'noise'), (bias, 'bias')):
        if t is not None and not t.is_cuda:
            raise RuntimeError('layer_tail: %s must live on the GPU (no CPU path in nerf_from_image_amd)' % name)
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


def fused_layer_forward(self, x, w, noise_mode='random', gain=1):
    """SynthesisLayer.forward (models/stylegan.py:325-356) with everything after the convolution on the HIP kernel.  The
    affine, the noise decision and the torch.randn call are the reference's, in its order: a seeded run draws the same noise."""
    assert noise_mode in ['random', 'const']
    styles = self.affine(w)

    noise = None
    if (self.use_noise and noise_mode == 'random' and (self.training or self.noise_strength != 0)):
        noise = torch.randn([x.shape[0], 1, self.resolution, self.resolution], device=x.device) * self.noise_strength
    if (self.use_noise and noise_mode == 'const' and self.noise_strength != 0):
        noise = self.noise_const * self.noise_strength

    # conv_modulated2d (stylegan.py:114-145) up to its convolution
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


def synthesis_layers(synthesis_network):
    """The synthesis layers of a StyleGAN2-style network, in module order: every sub-module with the attributes
    ``fused_layer_forward`` reads (no class is named)."""
    layers = [m for m in synthesis_network.modules() if all(hasattr(m, a) for a in LAYER_ATTRS)]
    if not layers:
        raise AttributeError('fuse_layers: the network has no StyleGAN2-style synthesis layer (a module with %s)' % (LAYER_ATTRS,))
    return layers


def fuse_layers(synthesis_network):
    """Swaps the forward of every synthesis layer for ``fused_layer_forward``.  Returns the layers."""
    layers = synthesis_layers(synthesis_network)
    for m in layers:
        if not hasattr(m, '_nfi_original_forward'):
            m._nfi_original_forward = m.forward
            m.forward = types.MethodType(fused_layer_forward, m)
    return layers


def fused_layers(synthesis_network):
    """The layers ``fuse_layers`` has fused (an empty list for a network with none, fused or at all)."""
    try:
        layers = synthesis_layers(synthesis_network)
    except AttributeError:
        return []
    return [m for m in layers if hasattr(m, '_nfi_original_forward')]


class unfused:
    """``with unfused(net):`` - every fused layer's original forward for the duration of the block (no-op when none is
    fused)."""

    def __init__(self, synthesis_network):
        self.net = synthesis_network
        self.swapped = []

    def __enter__(self):
        for m in fused_layers(self.net):
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
    for m in layers:
        if hasattr(m, '_nfi_original_forward'):
            m.forward = m._nfi_original_forward
            del m._nfi_original_forward
    return layers
