"""Drop-in for the reference's lib/metrics.py.  The three pure-tensor metrics that the inversion and evaluation loops
call side by side: ``psnr`` (30-45), ``ssim`` (48-76) and ``iou`` (79-94), same signatures, same asserts.  ``psnr`` and
``iou`` are one HIP launch (range check + clamp + reduction fused; no intermediate tensors); ``ssim`` is scikit-image's
structural_similarity(channel_axis=0, data_range=1.) at its defaults - 7 x 7 box window, sample covariance, the mean over
the window centres 3 pixels inside every edge - as a tile kernel and an ordered finish, on the device and without
scikit-image, bit-identical from launch to launch.  Limits: no Gaussian window, no other window size or data range and
no gradient (the reference calls none of them); checked against a float64 restatement pinned to scipy's uniform_filter,
not against scikit-image itself.

``LPIPSLoss`` (97-137) keeps the reference's signature and its three ``in1`` cases.  Its VGG network is dense convolution
work and stays with the library that runs it - out of scope here, and the ``lpips`` package that supplies it and its
weights must be installed for ``LPIPSLoss()``; any module with ``.net``, ``.scaling_layer``, ``.lins`` and ``.L`` can be
handed in instead.  Everything AFTER the network is HIP: per layer, the unit normalisation over the channels, the difference,
the square, the lin layer's 1x1 convolution and the spatial mean are one tile kernel and an ordered finish forward
(``lpips_distance``; ops.lpips_head) and one kernel backward, bit-identical from launch to launch.  Limits: float32 dense
NCHW features (anything else is copied), first-order gradients for the features only (the lin weights are frozen, as in
the reference), and a finite gradient where a pixel's channels are all zero (the reference has NaN there)."""
import torch
from torch import nn

from . import ops
from .autograd import LpipsHead


def _range_ok(flag):
    # lib/metrics.py:22-27 range_check: the reference asserts on device tensors (a host synchronisation), so does this
    assert int(flag.item()) == 0, 'Range check failed'


def psnr(pred, target, reduction='mean'):
    assert pred.shape == target.shape
    assert len(pred.shape) == 4
    assert pred.shape[1] == 3 or pred.shape[-1] == 3  # Ensure RGB image
    batch_psnr, _, flag = ops.image_metrics(pred=pred.detach(), target=target.detach())
    _range_ok(flag)
    if reduction == 'mean':
        return batch_psnr.mean()
    return batch_psnr


def ssim(pred, target, reduction='mean'):
    assert pred.shape == target.shape
    assert len(pred.shape) == 4
    assert pred.shape[1] == 3
    batch_ssim, _, flag = ops.image_ssim(pred.detach(), target.detach())
    _range_ok(flag)
    if reduction == 'mean':
        # the reference runs scikit-image once on the batch flattened to 3B channels: the mean of the per-image values, as [1]
        return batch_ssim.mean(dim=0, keepdim=True)
    return batch_ssim


def iou(alpha_pred, alpha_real, reduction='mean'):
    assert alpha_pred.shape == alpha_real.shape
    assert len(alpha_pred.shape) == 3 or (len(alpha_pred.shape) == 4 and alpha_pred.shape[1] == 1)
    _, batch_iou, flag = ops.image_metrics(mask_pred=alpha_pred.detach(), mask_real=alpha_real.detach())
    _range_ok(flag)
    if reduction == 'mean':
        return batch_iou.mean()
    return batch_iou.flatten()


def psnr_and_iou(pred, target, alpha_pred, alpha_real):
    """Both monitors of the inversion loop (run.py:2077-2090, 2247) in ONE launch: per-image (psnr [B], iou [B])."""
    batch_psnr, batch_iou, flag = ops.image_metrics(pred.detach(), target.detach(), alpha_pred.detach(), alpha_real.detach())
    _range_ok(flag)
    return batch_psnr, batch_iou


def psnr_ssim_iou(pred, target, alpha_pred, alpha_real):
    """The inversion report's three per-image vectors (run.py:2076-2088): (psnr [B], ssim [B], iou [B]) in two launches,
    whose two range flags share one tensor and reach the host in ONE read instead of three synchronisations."""
    assert pred.shape == target.shape
    assert len(pred.shape) == 4
    assert pred.shape[1] == 3
    pred, target = pred.detach(), target.detach()
    flags = torch.empty((2,), dtype=torch.int32, device=pred.device)
    batch_psnr, batch_iou, _ = ops.image_metrics(pred, target, alpha_pred.detach(), alpha_real.detach(), out_of_range=flags[0:1])
    batch_ssim, _, _ = ops.image_ssim(pred, target, out_of_range=flags[1:2])
    assert flags.tolist() == [0, 0], 'Range check failed'
    return batch_psnr, batch_ssim, batch_iou


def lpips_distance(features0, features1, weights, features1_normalized=False, eps=1e-10):
    """lib/metrics.py:130-133 on RAW features: sum over the layers of mean_p lin((normalize(f0) - normalize(f1))^2), [B,1].
    features0 / features1: one [B,C,H,W] per layer; weights: one [C] per layer (the lin layer's weight[0,:,0,0]);
    features1_normalized=True takes features1 as already normalised (a cached tuple).  Without a gradient the layers are
    chained into ONE output vector, left to right as the reference's sum() adds them; with one, each layer is an
    autograd node (autograd.LpipsHead) and the node outputs are summed in the same order."""
    if not (len(features0) == len(features1) == len(weights)) or len(weights) == 0:
        raise ValueError('lpips_distance: %d / %d feature maps for %d lin layers' % (len(features0), len(features1), len(weights)))
    if any(w.requires_grad for w in weights):
        raise RuntimeError('lpips_distance: the lin weights are frozen (lib/metrics.py:102); a weight that requires grad is not supported')
    if torch.is_grad_enabled() and any(f.requires_grad for f in tuple(features0) + tuple(features1)):
        total = None
        for x, y, w in zip(features0, features1, weights):
            term = LpipsHead.apply(x, y, w, features1_normalized, eps)
            total = term if total is None else total + term
    else:
        total = None
        for x, y, w in zip(features0, features1, weights):
            total = ops.lpips_head(x.detach(), y.detach(), w, features1_normalized, eps, out=total, accumulate=total is not None)
    return total.unsqueeze(1)


def lin_weight(lin):
    """The [C] weight of a lin layer: the one Conv2d in it, which must be 1x1 to one channel without a bias; an active
    Dropout (training mode, p > 0) in front of it is refused - the reference runs the net in eval()."""
    convs = [m for m in lin.modules() if isinstance(m, nn.Conv2d)]
    if len(convs) != 1:
        raise ValueError('LPIPSLoss: a lin layer must hold exactly one Conv2d, found %d' % len(convs))
    conv = convs[0]
    if conv.out_channels != 1 or tuple(conv.kernel_size) != (1, 1) or conv.bias is not None or conv.groups != 1 \
            or tuple(conv.stride) != (1, 1) or tuple(conv.padding) != (0, 0):
        raise ValueError('LPIPSLoss: a lin layer must be a 1x1 convolution to one channel without a bias, got %r' % (conv,))
    for m in lin.modules():
        if isinstance(m, nn.Dropout) and m.training and m.p > 0:
            raise ValueError('LPIPSLoss: a lin layer has an active Dropout (p = %g, training mode); call eval() first' % m.p)
    return conv.weight.reshape(-1)


def _range_check(t):
    # lib/metrics.py:22-27
    assert t.min() > -0.1, 'Range check failed'
    assert t.max() < 1.1, 'Range check failed'


class LPIPSLoss(nn.Module):
    """lib/metrics.py:97-137.  lpips_module=None builds lpips.LPIPS(net='vgg') as the reference does (an ImportError where the
    package is absent); otherwise any module with .net, .scaling_layer, .lins and .L."""

    def __init__(self, lpips_module=None):
        super().__init__()
        if lpips_module is None:
            import lpips
            lpips_module = lpips.LPIPS(net='vgg').eval()
            lpips_module.requires_grad_(False)
        for name in ('net', 'scaling_layer', 'lins', 'L'):
            if not hasattr(lpips_module, name):
                raise ValueError('LPIPSLoss: the module handed in has no .%s' % name)
        if len(lpips_module.lins) < lpips_module.L:
            raise ValueError('LPIPSLoss: %d lin layers for L = %d' % (len(lpips_module.lins), lpips_module.L))
        for lin in list(lpips_module.lins)[:lpips_module.L]:
            lin_weight(lin)
        self.lpips = lpips_module

    def _raw_features(self, im):
        features = self.lpips.net(self.lpips.scaling_layer(im))
        return tuple(features[i] for i in range(self.lpips.L))

    def _compute_features(self, im, eps=1e-10):
        # lib/metrics.py:104-110 in plain torch: only the in1=None case returns these, and no caller of run.py is hot there
        return tuple(f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps) for f in self._raw_features(im))

    def forward(self, in0, in1=None, normalize=False, reduction='none'):
        if normalize:
            _range_check(in0)
            in0 = 2 * in0 - 1
            if in1 is not None and not isinstance(in1, tuple):
                _range_check(in1)
                in1 = 2 * in1 - 1
        if in1 is None:
            return self._compute_features(in0)
        features0 = self._raw_features(in0)
        cached = isinstance(in1, tuple)
        features1 = in1 if cached else self._raw_features(in1)
        weights = [lin_weight(lin) for lin in list(self.lpips.lins)[:self.lpips.L]]
        out_features = lpips_distance(features0, features1, weights, features1_normalized=cached)       # [B,1], as lin(.).mean(dim=[2, 3])
        if reduction == 'mean':
            return out_features.mean()
        return out_features
