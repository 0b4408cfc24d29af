"""Drop-in for ``blur`` / ``filt2d`` of the reference's lib/ops.py (29-55): same arguments, same returns.  (The name ``ops``
belongs to this package's ctypes wrappers, hence ``filters``.)

run.py blurs the real image batch of every discriminator step (1090-1093), and z_image in the L1 / MSE branch of the
generator step (998), for the first blur_warmup_iters iterations.  The reference builds the taps with some ten small
launches, shifts the image by the background, runs a dense (2r+1) x (2r+1) conv2d - 61 x 61 at iteration 0 - and shifts
back.  Here the call is ONE launch of nfi_separable_filter: the taps are computed in the kernel, the background shift
is part of the load and the store, and the filter runs as its two 1-D passes.

    import nerf_from_image_amd.filters as nfi_filters
    target_img = nfi_filters.blur(target_img.permute(0, 3, 1, 2), i, blur_warmup_iters, white_background)

Both functions are differentiable with respect to the image (first order, like every HIP node): the backward is the same
entry on the incoming gradient with the taps reversed and no background.  Limits: radius <= 30 and, for blur, i >= 0 (sigma <= 10), 1-D kernels
only, no gradient with respect to the kernel, no CPU path.
"""
import math

from . import ops
from .autograd import differentiable

MAX_RADIUS = ops.FILTER_MAX_RADIUS


def _filtered(image, radius, taps, sigma, background):
    def fwd(x):
        return ops.separable_filter(x, radius, taps, sigma, background)

    def bwd(inputs, out_meta, grads, needs):
        # the adjoint of a zero-padded correlation is the correlation with the reversed taps; the background is a constant
        return (ops.separable_filter(grads[0], radius, taps, sigma, 0.0, flip=True),)
    return differentiable('separable_filter', fwd, image, bwd=bwd)


def blur_schedule(i, blur_warmup_iters):
    """(sigma, radius) of lib/ops.py:42-55 at iteration i, in Python doubles as the reference computes them."""
    sigma = max(1 - i / blur_warmup_iters, 0) * 10
    return sigma, int(math.floor(sigma * 3))


def blur(image, i, blur_warmup_iters, white_background):
    """lib/ops.py:42-55.  image [B,C,H,W] float32 on the GPU, dense or a dense [B,H,W,C] behind permute(0,3,1,2) (read in
    place).  Returns image itself once the radius has reached 0 (i >= 12084 of 12500), else a dense [B,C,H,W]."""
    sigma, radius = blur_schedule(i, blur_warmup_iters)
    if radius == 0:
        return image
    if i < 0 or radius > MAX_RADIUS:
        # sigma <= 10 and 61 taps at most hold for i >= 0 only (the training loop counts from 0)
        raise ValueError('blur: iteration %r of %r gives sigma %g, radius %d; i >= 0 and a radius of at most %d are supported'
                         % (i, blur_warmup_iters, sigma, radius, MAX_RADIUS))
    return _filtered(image, radius, None, sigma, 1.0 if white_background else 0.0)


def filt2d(im, kernel):
    """lib/ops.py:29-39 for a 1-D kernel (the separable case, the only one the reference uses): the zero-padded
    cross-correlation of im [B,C,H,W] with kernel (x) kernel.  kernel: float32 [3 .. 61, odd] on im's device."""
    if kernel.dim() == 2:
        raise NotImplementedError('filt2d: 2-D kernels are not supported (nothing in the reference passes one); give the 1-D taps')
    if kernel.dim() != 1:
        raise ValueError('filt2d: kernel must be 1-D, got %s' % (tuple(kernel.shape),))
    n = kernel.shape[0]
    if n % 2 == 0:
        raise ValueError('filt2d: a kernel of even length %d changes the output size; odd lengths only' % n)
    if not 3 <= n <= 2 * MAX_RADIUS + 1:
        raise ValueError('filt2d: kernel length %d outside 3 .. %d' % (n, 2 * MAX_RADIUS + 1))
    return _filtered(im, n // 2, kernel.detach(), 0.0, 0.0)
