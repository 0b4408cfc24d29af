"""The layer between a caller's tensor and the pointer a kernel gets, for every core wrapper (the rows of
tests/contract_util.py): a view of the same values gives the same answer, a bad argument is refused before the library
is reached, and no unaligned view reaches a kernel.

Views are compared with the dense call of the SAME wrapper: bit for bit where the entry is bit-reproducible (the backwards
run in their ordered mode), else at the bound of that entry's float64 parity test (named in the row).  A misread layout
is wrong by O(1), not by rounding.  Refusals run with _lib.load replaced by a proxy whose launching entries raise
instead of running: a missing check is a failed assertion, never a launch on a short or foreign buffer."""
import pytest
import torch

import contract_util as cu
from nerf_from_image_amd import ops

pytestmark = pytest.mark.gpu

_CACHE = {}


def dense_case(row, dev):
    """(arguments, outputs of the dense call): computed once per row, shared by its tests, never modified."""
    if row.id not in _CACHE:
        args = row.build(dev)
        _CACHE[row.id] = (args, row.outputs(args))
    return _CACHE[row.id]


def row_of(rid):
    return cu.ROWS[cu.ROW_IDS.index(rid)]


def same(row, got, want):
    """None, or what differs between two results of the row."""
    if len(got) != len(want):
        return 'number of outputs %d vs %d' % (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        if a.shape != b.shape or a.dtype != b.dtype:
            return 'output %d: %s %s vs %s %s' % (i, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
        if row.exact:
            if not cu.bit_equal(a, b):
                d = (a.double() - b.double()).abs()
                return 'output %d %s: not bit-equal (max |diff| %.3e)' % (i, tuple(a.shape), float(d[torch.isfinite(d)].max()) if torch.isfinite(d).any() else float('nan'))
        elif a.is_floating_point():
            scale = float(b.double().abs().max().clamp_min(1e-12))
            e = float((a.double() - b.double()).abs().max()) / scale
            if not e <= row.tolerance:
                return 'output %d %s: rel %.3e > %.1e' % (i, tuple(a.shape), e, row.tolerance)
        elif not torch.equal(a, b):
            return 'output %d %s: integer outputs differ' % (i, tuple(a.shape))
    return None


def view_cases(row, args):
    """(label, argument, replacement) for every tensor argument: strided, permuted, one element off alignment; texels also
    over the storage of the other layout."""
    for name in row.tensors:
        for label, make in list(cu.VIEWS.items()) + [('offset', cu.offset)]:
            yield '%s %s' % (label, name), name, make(args[name])
        if name == 'texels' and args[name].shape[1] != args[name].shape[3]:
            yield 'other-layout texels', name, cu.other_layout_view(args[name])


@pytest.mark.parametrize('rid', cu.ROW_IDS)
def test_views_give_the_same_answer(gpu_device, rid):
    row = row_of(rid)
    args, want = dense_case(row, gpu_device)
    again = row.outputs(args)
    assert same(row, again, want) is None, 'the dense call does not repeat itself: %s' % same(row, again, want)
    bad = []
    for label, name, view in view_cases(row, args):
        assert view.shape == args[name].shape and cu.bit_equal(view, args[name])
        if label.startswith('offset'):
            # an unaligned view must not reach a kernel that reads wider than an element: the wrappers copy it (the row's
            # widest access is 16 for every argument)
            assert view.is_contiguous() and view.data_ptr() % row.widest[name] == view.element_size()
        elif args[name].numel() > 1:
            assert not view.is_contiguous(), label
        diff = same(row, row.outputs(dict(args, **{name: view})), want)
        if diff is not None:
            bad.append('%s: %s' % (label, diff))
    torch.cuda.synchronize()
    assert not bad, '%s: %d view case(s) differ from the dense call:\n  %s' % (rid, len(bad), '\n  '.join(bad))


@pytest.mark.parametrize('rid', [r.id for r in cu.ROWS if r.g_texels])
def test_the_texel_gradient_is_dense_whatever_the_texels_strides(gpu_device, rid):
    row = row_of(rid)
    args, _ = dense_case(row, gpu_device)
    want = row.call(args)['g_texels']
    assert want.is_contiguous() and want.shape == args['texels'].shape and want.dtype == torch.float32
    want_planes = ops.texel_grad_to_planes(want)
    bad = []
    for label, make in (('strided', cu.strided), ('permuted', cu.permuted), ('offset', cu.offset), ('other layout', cu.other_layout_view)):
        got = row.call(dict(args, texels=make(args['texels'])))['g_texels']
        if not got.is_contiguous():
            bad.append('%s texels: g_texels is not contiguous, strides %s' % (label, got.stride()))
        assert got.shape == want.shape and ops.texel_layout_of(got) == ops.texel_layout_of(args['texels'])
        got_planes = ops.texel_grad_to_planes(got)
        if row.exact:
            if not cu.bit_equal(got_planes.contiguous(), want_planes.contiguous()):
                bad.append('%s texels: the plane gradient is not bit-equal to the dense call\'s' % label)
        else:
            e = float((got_planes - want_planes).abs().max()) / float(want_planes.abs().max())
            if not e <= row.tolerance:
                bad.append('%s texels: plane gradient rel %.3e > %.1e' % (label, e, row.tolerance))
    assert not bad, '%s:\n  %s' % (rid, '\n  '.join(bad))


def bad_values(row, args, name):
    """(label, value) a wrapper must refuse for argument `name`."""
    t = args[name]
    yield 'float64', t.double()
    if name not in row.f16_ok and t.dtype != torch.float16:
        yield 'float16', t.half()
    yield 'pinned host', t.cpu().pin_memory()
    if row.counts[name] is not None:
        yield 'one row too few', t[:-1]
    if name == 'decoder_image':
        other = ops._decoder_image_floats(t.numel() == ops._decoder_image_floats(False))
        yield 'the image of the other decoder', torch.zeros((other,), dtype=torch.float32, device=t.device)


@pytest.mark.parametrize('rid', cu.ROW_IDS)
def test_bad_arguments_are_refused_before_the_library(gpu_device, rid, monkeypatch):
    row = row_of(rid)
    args, _ = dense_case(row, gpu_device)
    cases = [(name, label, value) for name in row.tensors for label, value in bad_values(row, args, name)]
    proxy = cu.install_proxy(monkeypatch)
    missed = []
    for name, label, value in cases:
        try:
            row.call(dict(args, **{name: value}))
            missed.append('%s as %s: accepted' % (name, label))
        except (TypeError, ValueError, RuntimeError):
            pass
        except cu.ReachedLibrary as e:
            missed.append('%s as %s: reached %s' % (name, label, e))
    assert not missed, '%s: %d bad argument(s) not refused:\n  %s' % (rid, len(missed), '\n  '.join(missed))
    assert proxy.reached == []
    # ... and the proxy is what stands between the good arguments and the kernels
    with pytest.raises(cu.ReachedLibrary):
        row.call(args)
