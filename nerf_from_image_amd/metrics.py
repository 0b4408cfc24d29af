"""Drop-in for the three pure-tensor metrics of the reference's lib/metrics.py that the inversion and evaluation loops
call side by side: ``psnr`` (30-45), ``ssim`` (48-76) and ``iou`` (79-94), same signatures, same asserts.  ``psnr`` and
``iou`` are one HIP launch (range check + clamp + reduction fused; no intermediate tensors); ``ssim`` is scikit-image's
structural_similarity(channel_axis=0, data_range=1.) at its defaults - 7 x 7 box window, sample covariance, the mean over
the window centres 3 pixels inside every edge - as a tile kernel and an ordered finish, on the device and without
scikit-image, bit-identical from launch to launch.  Limits: no Gaussian window, no other window size or data range and
no gradient (the reference calls none of them); checked against a float64 restatement pinned to scipy's uniform_filter,
not against scikit-image itself.  LPIPS is a VGG network in the reference and is out of scope."""
import torch

from . import ops


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
