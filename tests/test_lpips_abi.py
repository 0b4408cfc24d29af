"""CPU-side checks of the LPIPS distance head at the C ABI and of the tests' own reference: the three entries are exported
with the header's prototypes, the argument struct keeps its field order and kinds, the workspace size behaves, the calls refuse
what the header comment says they refuse - before any launch - the Python entries have no CPU path, LPIPSLoss() without the
lpips package is an ImportError, a lin layer that is not a bias-free 1x1 convolution to one channel is refused, and the
float64 restatement the GPU tests compare against equals the formulas written out as loops."""
import ctypes
import re

import pytest
import torch

from nerf_from_image_amd import _lib
import lpips_util as lu

STRUCT = 'nfi_lpips_head_args'
SIZE, FWD, BWD = 'nfi_lpips_head_workspace_bytes', 'nfi_lpips_head_fwd', 'nfi_lpips_head_bwd'


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def size(**kw):
    return _lib.struct_query(SIZE, STRUCT, **kw)


def test_entries_are_exported_with_the_header_prototypes(lib):
    src = _lib._strip_comments(open(_lib.HEADER).read())
    proto = {m.group(2): (m.group(1), [p.strip() for p in m.group(3).split(',')])
             for m in re.finditer(r'(\w+)\s+(nfi_lpips_head\w*)\s*\(([^)]*)\)\s*;', src)}
    one, two = ['const nfi_lpips_head_args* a'], ['const nfi_lpips_head_args* a', 'nfi_stream_t stream']
    assert proto == {SIZE: ('size_t', one), FWD: ('int', two), BWD: ('int', two)}
    assert _lib.FUNCTIONS[SIZE] == (ctypes.c_size_t, [ctypes.c_void_p])
    for name in (FWD, BWD):
        assert _lib.FUNCTIONS[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    for name in (SIZE, FWD, BWD):
        fn = getattr(lib, name)
        assert fn.restype is _lib.FUNCTIONS[name][0] and list(fn.argtypes) == _lib.FUNCTIONS[name][1]
    assert lib.nfi_version() >= 105


def test_header_comment_cites_the_reference():
    src = open(_lib.HEADER).read()
    comment = src[:src.index('typedef struct nfi_lpips_head_args')].rsplit('/*', 1)[1]
    assert 'lib/metrics.py:104-110, 130-133' in comment


def test_struct_field_order_and_kinds():
    assert [n for n, _ in _lib.STRUCT_FIELDS[STRUCT]] == [
        'n_images', 'channels', 'height', 'width', 'x', 'y', 'y_normalized', 'weight', 'eps', 'out', 'accumulate', 'g_out', 'g_x',
        'g_y', 'workspace', 'workspace_bytes']
    kinds = dict(_lib.STRUCT_FIELDS[STRUCT])
    assert all(kinds[k] is ctypes.c_int for k in ('n_images', 'channels', 'height', 'width', 'y_normalized', 'accumulate'))
    assert all(kinds[k] is ctypes.c_void_p for k in ('x', 'y', 'weight', 'out', 'g_out', 'g_x', 'g_y', 'workspace'))
    assert kinds['eps'] is ctypes.c_float and kinds['workspace_bytes'] is ctypes.c_size_t


def test_workspace_bytes(lib):
    """Positive, a multiple of 8, non-decreasing in B and in H * W, independent of C, and 0 for a shape the calls refuse."""
    pixels = (1, 5, 63, 64, 65, 127, 128, 129, 131, 256, 1000, 16384)
    for B in (1, 2, 5, 64):
        last = 0
        for hw in pixels:
            for H, W in ((1, hw), (hw, 1)):
                n = size(n_images=B, channels=64, height=H, width=W)
                assert n > 0 and n % 8 == 0 and n >= last, (B, H, W, n, last)
                assert n == size(n_images=B, channels=513, height=H, width=W)
            last = n
    for H, W in ((1, 1), (7, 9), (16, 16), (128, 128)):
        last = 0
        for B in (1, 2, 3, 5, 16, 17, 64, 130):
            n = size(n_images=B, channels=3, height=H, width=W)
            assert n > 0 and n % 8 == 0 and n >= last, (B, H, W, n, last)
            last = n
    assert size(n_images=130, channels=64, height=128, width=128) == 130 * 256 * 8          # one double per block of 64 pixels
    ok = dict(n_images=2, channels=3, height=4, width=5)
    for name in ok:
        for bad in (0, -1):
            assert size(**dict(ok, **{name: bad})) == 0, (name, bad)
    assert size(n_images=2 ** 31 - 1, channels=1, height=1, width=65) == 0                  # 2^32 - 2 blocks
    assert size(n_images=1, channels=1, height=2 ** 31 - 1, width=2 ** 8) == 0              # 2^33 blocks
    assert lib.nfi_lpips_head_workspace_bytes(None) == 0


def test_refusals_come_with_a_message_and_before_any_launch(lib):
    """Every pointer below is a small integer no kernel could read: a call that got past its checks would fault, not return -1."""
    n = 2 * 3 * 4 * 5 * 4                                         # bytes of x
    base = dict(n_images=2, channels=3, height=4, width=5, x=0x10000, y=0x20000, y_normalized=0, weight=0x30000, eps=1e-10, out=0x40000,
                accumulate=0, g_out=0x50000, g_x=0x60000, g_y=0x70000)
    need = size(**base)
    assert need == 2 * 8

    def refused(entry, word, workspace=256, n_bytes=need, **kw):
        a = _lib.make_args(STRUCT, workspace=workspace, workspace_bytes=n_bytes, **dict(base, **kw))
        rc, msg = getattr(lib, entry)(ctypes.byref(a), None), lib.nfi_last_error()
        assert rc == -1 and word in msg, (entry, word, rc, msg)

    for entry in (FWD, BWD):
        assert getattr(lib, entry)(None, None) == -1 and b'null' in lib.nfi_last_error()
        for missing in ('x', 'y', 'weight'):
            refused(entry, b'null', **{missing: None})
        for name in ('n_images', 'channels', 'height', 'width'):
            for bad in (0, -2):
                refused(entry, b'at least 1', **{name: bad})
        for eps in (-1e-10, -1.0, float('nan')):
            refused(entry, b'eps', eps=eps)
        refused(entry, b'grid too large', n_images=2 ** 31 - 1, height=1, width=65)
    refused(FWD, b'null out', out=None)
    refused(FWD, b'workspace missing', workspace=None)
    refused(FWD, b'workspace too small', n_bytes=need - 1)
    refused(FWD, b'workspace too small', n_bytes=0)
    refused(FWD, b'aligned', workspace=260)
    refused(BWD, b'null g_out', g_out=None)
    refused(BWD, b'both null', g_x=None, g_y=None)
    for grad in ('g_x', 'g_y'):
        for where in (base['x'], base['x'] + n - 4, base['x'] - n + 4, base['y'], base['y'] + 8):
            refused(BWD, b'overlaps', **{grad: where})
    refused(BWD, b'g_x overlaps g_y', g_y=base['g_x'] + n - 4)
    # the backward needs no workspace and the forward no gradient fields: the next refusal in line is reached
    refused(BWD, b'both null', workspace=None, n_bytes=0, out=None, g_x=None, g_y=None)
    refused(FWD, b'workspace missing', workspace=None, g_out=None, g_x=None, g_y=None)
    with pytest.raises(RuntimeError, match='workspace missing'):
        _lib.call_struct(FWD, STRUCT, 0, workspace=None, workspace_bytes=need, **base)


def test_no_cpu_path():
    from nerf_from_image_amd import metrics, ops
    x, w = torch.rand(2, 3, 4, 5), torch.rand(3)
    for call in (lambda: ops.lpips_head(x, x, w), lambda: ops.lpips_head_bwd(torch.ones(2), x, x, w),
                 lambda: metrics.lpips_distance([x], [x], [w]), lambda: metrics.lpips_distance([x.clone().requires_grad_()], [x], [w]),
                 lambda: metrics.LPIPSLoss(lu.StandInLpips())(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16))):
        with pytest.raises(RuntimeError, match='GPU'):
            call()


def test_lpips_loss_without_the_package_is_an_import_error():
    from nerf_from_image_amd import metrics
    try:
        import lpips  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            metrics.LPIPSLoss()
    else:
        pytest.skip('the lpips package is installed here')


def test_lin_layers_that_are_not_a_plain_1x1_convolution_are_refused():
    from nerf_from_image_amd import metrics
    assert tuple(metrics.lin_weight(lu.StandInLin(8).eval()).shape) == (8,)
    for bad in (lu.StandInLin(8, bias=True), lu.StandInLin(8, out_channels=2), lu.StandInLin(8, kernel=3)):
        with pytest.raises(ValueError, match='1x1 convolution'):
            metrics.lin_weight(bad.eval())
        net = lu.StandInLpips()
        net.lins[2] = bad.eval()
        with pytest.raises(ValueError, match='1x1 convolution'):
            metrics.LPIPSLoss(net)
    training = lu.StandInLin(8).train()
    with pytest.raises(ValueError, match='Dropout'):
        metrics.lin_weight(training)
    training.model[0].p = 0.0
    assert tuple(metrics.lin_weight(training).shape) == (8,)
    with pytest.raises(ValueError, match='no .net'):
        metrics.LPIPSLoss(torch.nn.Identity())
    net = lu.StandInLpips()
    net.requires_grad_(True)
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match='frozen'):
        metrics.LPIPSLoss(net)(x, x)


def test_the_float64_restatement_is_the_formulas_written_out():
    """2 x 3 x 2 x 2, both ways of reading y, to 1e-14 relative; an all-zero pixel has a NaN gradient in the restatement,
    as in the reference's autograd - the stated deviation of the kernel is from exactly this."""
    g = torch.Generator().manual_seed(11)
    x, y, w = torch.rand(2, 3, 2, 2, generator=g), torch.rand(2, 3, 2, 2, generator=g), torch.rand(3, generator=g)
    for yn in (False, True):
        want = lu.head_loops(x, y, w, yn)
        got = lu.head_ref(x, y, w, torch.float64, yn)
        assert float(((got - want).abs() / want.abs()).max()) <= 1e-14, yn
    x0 = x.clone()
    x0[0, :, 1, 0] = 0.0
    _, g_x, _ = lu.head_grads(x0, y, w, torch.ones(2), torch.float64)
    assert bool(torch.isnan(g_x[0, :, 1, 0]).all()) and bool(torch.isfinite(g_x[1]).all())


def test_yardsticks_are_not_vacuous():
    """The bounds the GPU file uses, from the float32 restatement on the CPU: within a factor 4 of the floor for every content
    but the cancellation case, whose float32 restatement loses three digits."""
    for content in lu.PARITY_CONTENTS:
        v, g = lu.yardsticks(content)
        bv, bg = lu.bounds(content)
        print('float32 restatement against float64, %s: value %.3e, gradient %.3e; bounds %.3e, %.3e' % (content, v, g, bv, bg))
        top = 1e-3 if content == 'near' else 4 * lu.FLOOR
        assert lu.FLOOR <= bv <= top and lu.FLOOR <= bg <= top
