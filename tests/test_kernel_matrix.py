"""Every kernel the render and field selectors can pick, enumerated and compared with the oracle.

The library says which kernel a call gets (nfi_render_kernel_name, nfi_field_kernel_name, nfi_field_bwd_kernel_name: the
launch's own argument rules and selection code, no GPU needed).  The MATRIX below is the plain product of the axes those
selectors read.  Without a GPU: the set of names the matrix reaches must EQUAL the set of instantiations in the built
library (read from the mangled names), the rows the rules refuse are counted, and the seeded scenes are shown to be well
conditioned for the REFERENCE (float32 oracle within 1e-5 of the float64 oracle, no ray left out).  On the GPU: one test
per legal row, against the float32 CPU oracle (for 16-bit texel storage: on the planes rounded to the storage type), with
the bounds the suite already uses for that kind of output (imported where they have a name)."""
import collections
import contextlib
import ctypes
import itertools
import re

import pytest
import torch

from parity_util import err, grad_close, hip_field_setup, hip_render, oracle_normal_map, oracle_render
from stand_in import look_at_cameras
from test_hip_parity import ATOL, sigma_close
from nerf_from_image_amd import _lib, ops
from oracle import nfi_oracle as orc

# ------------------------------------------------------------------------------------------------
# the matrix
# ------------------------------------------------------------------------------------------------
TEXELS = ('fp32', 'bf16', 'fp16')
TEXEL_ID = {'fp32': ops.TEXEL_F32, 'bf16': ops.TEXEL_BF16, 'fp16': ops.TEXEL_F16}
TEXEL_TORCH = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
ATTENTION = (0, 10)
A_MAX = 14                      # NFI_MAX_ATTENTION: the size the per-wave semantics tables in dynamic LDS are raised for
SAMPLES = (24, 100, 200)        # render_fwd_kernel (<= 64), render_fwd_wide_kernel (<= 128), render_fwd_long_kernel (<= 512)
MODES = ('plain', 'taps', 'stash', 'term', 'semantics', 'coords', 'semantics+coords', 'normals', 'strict', 'strict+taps',
         'profile')
MAP_MODES = ('semantics', 'semantics+coords', 'normals')            # the rows that get A = 14 as well
SHAPES = ((9, 7), (16, 8))      # 126 rays: ragged last workgroup, scanline order; 256 rays: tile order, per-XCD queues
B, PR, SCENE_RANGE = 2, 32, 0.55
TERM_EPS = 1e-5
FAMILIES = collections.OrderedDict((('render_fwd_kernel', 46), ('render_fwd_wide_kernel', 44), ('render_fwd_long_kernel', 14),
                                    ('field_query_kernel', 18), ('field_query_bwd_kernel', 16)))

Row = collections.namedtuple('Row', 'tex A S fine vd mode')
Config = collections.namedtuple('Config', 'tex A S fine vd sdf white shape')        # what the oracle's result depends on
FieldRow = collections.namedtuple('FieldRow', 'tex A vd prec')
FieldBwdRow = collections.namedtuple('FieldBwdRow', 'tex A vd coord')


def render_rows():
    rows = []
    for tex, A, S, fine, vd, mode in itertools.product(TEXELS, ATTENTION, SAMPLES, (True, False), (False, True), MODES):
        rows.append(Row(tex, A, S, fine, vd, mode))
        if A == ATTENTION[-1] and mode in MAP_MODES:
            rows.append(Row(tex, A_MAX, S, fine, vd, mode))
    return rows


RENDER_ROWS = render_rows()
FIELD_ROWS = [FieldRow(*r) for r in itertools.product(TEXELS, ATTENTION, (False, True), (0, 1))]
FIELD_BWD_ROWS = [FieldBwdRow(*r) for r in itertools.product(TEXELS, ATTENTION, (False, True), (True, False))]


def row_id(row):
    return '-'.join('%s=%s' % (k, int(v) if isinstance(v, bool) else v) for k, v in row._asdict().items())


def config_of(row):
    """The run-time switches of a row - decoder branch, background, image shape - alternate over the axes instead of
    multiplying the matrix; the normal map exists for the SDF decoder only."""
    ti, si, ai = TEXELS.index(row.tex), SAMPLES.index(row.S), int(row.A > 0)
    sdf = row.mode == 'normals' or (ti + si + ai + int(row.vd) + int(row.fine)) % 3 != 0
    white = (ti + ai + si + int(row.fine)) % 2 == 0
    shape = SHAPES[(ti + si + int(row.vd) + int(row.fine)) % 2]
    return Config(row.tex, row.A, row.S, row.fine, row.vd, sdf, white, shape)


def skip_missed_of(row):
    return row.mode == 'stash' or (MODES.index(row.mode) + TEXELS.index(row.tex) + SAMPLES.index(row.S)) % 2 == 0


# The draw of a configuration's scene, keyed by the configuration itself.  A configuration is listed here when its first
# draws do not meet test_scenes_are_well_conditioned_for_the_reference - a ray whose float32 and float64 resampling fall on
# different sides of a cdf break, a sample whose normal is the direction of a vanishing gradient: such a ray says nothing
# about a kernel, so the scene is drawn again instead of allowing for outliers on the GPU.  The draws were chosen with the
# float32 - float64 difference under 5e-6, half the 1e-5 the test asserts, to leave room for another CPU build of torch.
RESEED = {
    Config(tex='bf16', A=0, S=24, fine=False, vd=False, sdf=True, white=False, shape=(16, 8)): 2,
    Config(tex='bf16', A=0, S=24, fine=False, vd=True, sdf=True, white=False, shape=(9, 7)): 1,
    Config(tex='bf16', A=0, S=100, fine=True, vd=False, sdf=True, white=False, shape=(16, 8)): 1,
    Config(tex='bf16', A=0, S=100, fine=True, vd=True, sdf=True, white=False, shape=(9, 7)): 2,
    Config(tex='bf16', A=10, S=24, fine=False, vd=False, sdf=True, white=True, shape=(16, 8)): 1,
    Config(tex='bf16', A=10, S=100, fine=False, vd=False, sdf=True, white=False, shape=(9, 7)): 2,
    Config(tex='bf16', A=10, S=100, fine=True, vd=False, sdf=True, white=True, shape=(16, 8)): 5,
    Config(tex='bf16', A=10, S=100, fine=True, vd=True, sdf=True, white=True, shape=(9, 7)): 1,
    Config(tex='bf16', A=14, S=24, fine=False, vd=False, sdf=True, white=True, shape=(16, 8)): 3,
    Config(tex='bf16', A=14, S=100, fine=True, vd=False, sdf=True, white=True, shape=(16, 8)): 5,
    Config(tex='fp16', A=0, S=24, fine=False, vd=False, sdf=True, white=True, shape=(9, 7)): 1,
    Config(tex='fp16', A=0, S=100, fine=False, vd=False, sdf=True, white=False, shape=(16, 8)): 1,
    Config(tex='fp16', A=0, S=100, fine=True, vd=False, sdf=True, white=True, shape=(9, 7)): 1,
    Config(tex='fp16', A=0, S=100, fine=True, vd=True, sdf=True, white=True, shape=(16, 8)): 1,
    Config(tex='fp16', A=10, S=24, fine=False, vd=False, sdf=True, white=False, shape=(9, 7)): 1,
    Config(tex='fp16', A=10, S=24, fine=True, vd=False, sdf=True, white=True, shape=(16, 8)): 1,
    Config(tex='fp16', A=14, S=24, fine=False, vd=False, sdf=True, white=False, shape=(9, 7)): 1,
    Config(tex='fp16', A=14, S=24, fine=True, vd=False, sdf=True, white=True, shape=(16, 8)): 10,
    Config(tex='fp16', A=14, S=100, fine=True, vd=False, sdf=True, white=False, shape=(9, 7)): 2,
    Config(tex='fp32', A=0, S=24, fine=False, vd=False, sdf=True, white=True, shape=(9, 7)): 1,
    Config(tex='fp32', A=0, S=100, fine=True, vd=False, sdf=True, white=True, shape=(9, 7)): 1,
    Config(tex='fp32', A=0, S=100, fine=True, vd=True, sdf=True, white=True, shape=(16, 8)): 1,
    Config(tex='fp32', A=10, S=24, fine=False, vd=True, sdf=True, white=False, shape=(16, 8)): 2,
    Config(tex='fp32', A=10, S=100, fine=False, vd=False, sdf=True, white=True, shape=(16, 8)): 1,
    Config(tex='fp32', A=10, S=100, fine=True, vd=False, sdf=True, white=False, shape=(9, 7)): 1,
    Config(tex='fp32', A=10, S=100, fine=True, vd=True, sdf=True, white=False, shape=(16, 8)): 1,
    Config(tex='fp32', A=14, S=24, fine=False, vd=True, sdf=True, white=False, shape=(16, 8)): 2,
    Config(tex='fp32', A=14, S=24, fine=True, vd=False, sdf=True, white=True, shape=(16, 8)): 2,
    Config(tex='fp32', A=14, S=24, fine=True, vd=True, sdf=True, white=True, shape=(9, 7)): 2,
}


def seed_of(cfg):
    """A seed from the VALUES of the axes (and the draw), independent of how rows and configurations are printed."""
    h = RESEED.get(cfg, 0)
    for v in (TEXELS.index(cfg.tex), cfg.A, cfg.S, int(cfg.fine), int(cfg.vd), int(cfg.sdf), int(cfg.white)) + tuple(cfg.shape):
        h = (h * 1000003 + v + 1) % 2147483647
    return h


def make_scene(cfg):
    """(meta, t) in the form of a golden case (parity_util.hip_render / oracle_render / oracle_normal_map take it): two
    scenes of band-limited 32^2 planes, a random decoder whose distance output is centred on its median, cameras on a
    sphere of radius 1.6, redrawn until part of each image's rays miss the cube."""
    g = torch.Generator().manual_seed(seed_of(cfg))
    H, W = cfg.shape
    A, S = cfg.A, cfg.S
    n_out = 33 if cfg.vd else (1 + A if A > 0 else 4)
    low = torch.randn(B * 3, 32, 16, 16, generator=g)
    planes = torch.nn.functional.interpolate(low, size=(PR, PR), mode='bilinear', align_corners=True).view(B, 3, 32, PR, PR) \
        + 0.05 * torch.randn(B, 3, 32, PR, PR, generator=g)
    t = dict(planes=planes, w1=torch.randn(64, 32, generator=g), b1=0.3 * torch.randn(64, generator=g),
             w2=torch.randn(n_out, 64, generator=g), b2=0.3 * torch.randn(n_out, generator=g),
             beta=torch.tensor([0.1]), alpha=torch.tensor([0.05]),
             focal=torch.full((B,), 1.0254),
             noise_coarse=torch.rand(B, H, W, S, generator=g))
    if A > 0:
        t['attention_values'] = torch.rand(B, A, 3, generator=g) * 2 - 1
    if cfg.fine:
        t['noise_fine'] = torch.rand(B * H * W, S, generator=g)
    if cfg.vd:
        n3 = A if A > 0 else 3
        t.update(viewdir_x=torch.randn(B, H, W, 32, generator=g), w3=torch.randn(n3, 32, generator=g),
                 b3=0.3 * torch.randn(n3, generator=g))
    x = (torch.rand(B, 2048, 3, generator=g) * 2 - 1) * SCENE_RANGE
    t['b2'][0] -= orc.field_query(planes, t['w1'], t['b1'], t['w2'], t['b2'], x, SCENE_RANGE, use_sdf=False)['sdf'].median()
    while True:         # cameras from which at least 10 % of each image's rays miss the cube (drawn last: nothing else moves)
        t['cam2world'] = look_at_cameras(B, 1.6, g)
        ro, rd = orc.ray_bundle(H, W, t['focal'], t['cam2world'])
        if float(orc.near_far(ro, orc.unit_dirs(rd), SCENE_RANGE)[2].float().flatten(1).mean(1).max()) <= 0.9:
            break
    meta = dict(B=B, H=H, W=W, S=S, A=A, scene_range=SCENE_RANGE, white=cfg.white, fine=cfg.fine, sdf=cfg.sdf)
    return meta, t


def rounded(t, tex, dtype=torch.float32):
    """The inputs the comparison of a row uses: the planes rounded to the texel storage type, every tensor as `dtype`."""
    t = dict(t, planes=t['planes'].to(TEXEL_TORCH[tex]).to(torch.float32))
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in t.items()}


def coords_map(o, meta):
    ts = o['t_sorted'] if meta['fine'] else o['t_coarse']
    pts = o['ro'].unsqueeze(-2) + o['rd'].unsqueeze(-2) * ts.unsqueeze(-1)
    return (o['weights'].unsqueeze(-1) * pts).sum(-2)


_scenes, _oracles, _normal_maps = {}, {}, {}


def scene_of(cfg):
    if cfg not in _scenes:
        _scenes[cfg] = make_scene(cfg)
    return _scenes[cfg]


def oracle_of(cfg, dtype=torch.float32):
    """(meta, inputs of the comparison, oracle result) of a configuration, computed once per module."""
    if (cfg, dtype) not in _oracles:
        meta, t = scene_of(cfg)
        tr = rounded(t, cfg.tex, dtype)
        _oracles[cfg, dtype] = (meta, tr, oracle_render(meta, tr, 'cpu'))
    return _oracles[cfg, dtype]


def normal_map_of(cfg, dtype=torch.float32):
    if (cfg, dtype) not in _normal_maps:
        meta, tr, o = oracle_of(cfg, dtype)
        _normal_maps[cfg, dtype] = oracle_normal_map(meta, tr, o)
    return _normal_maps[cfg, dtype]


# ------------------------------------------------------------------------------------------------
# asking the library (placeholder pointers: the queries dereference nothing)
# ------------------------------------------------------------------------------------------------
PTR = 16
FINE_TAPS = ('t_fine', 'sigma_fine', 'rgb_fine', 'perm')


def render_query_fields(row):
    """nfi_render_args of a row as ops.render_fwd fills it, with a placeholder for every device pointer."""
    cfg = config_of(row)
    H, W = cfg.shape
    f = dict(n_scenes=B, height=H, width=W, n_samples=row.S, fine_sampling=int(row.fine), white_background=int(cfg.white),
             scene_range=SCENE_RANGE, cam2world=PTR, focal=PTR, texels=PTR, plane_res=PR, texel_dtype=TEXEL_ID[row.tex],
             decoder_image=PTR, n_attention=row.A, attention_values=PTR if row.A > 0 else None, use_sdf=int(cfg.sdf),
             beta=PTR if cfg.sdf else None, alpha=PTR if cfg.sdf else None, noise_coarse=PTR,
             noise_fine=PTR if row.fine else None, noise_fine_row_stride=row.S if row.fine else 0, rgb=PTR, depth=PTR,
             mask=PTR, workspace=PTR, workspace_bytes=1 << 30, skip_missed_rays=int(skip_missed_of(row)),
             ray_features=PTR if row.vd else None)
    mode = row.mode
    if mode in ('taps', 'strict+taps'):
        f.update({k: PTR for k in ops.TAP_NAMES if row.fine or k not in FINE_TAPS})
    if mode == 'stash':
        f.update(stash_t=PTR, stash_sigma=PTR, stash_rgb=PTR, ray_origins=PTR, ray_directions=PTR)
    if mode == 'term':
        f['termination_eps'] = TERM_EPS
    if mode in ('semantics', 'semantics+coords'):
        f['semantics'] = PTR
    if mode in ('coords', 'semantics+coords'):
        f['coords'] = PTR
    if mode == 'normals':
        f['normals'] = PTR
    if mode in ('strict', 'strict+taps'):
        f['tuning'] = 8             # NFI_TUNING_EXACT_FP32_MLP
    if mode == 'profile':
        f['profile_cycles'] = PTR
    return f


def field_query_fields(row):
    return dict(n_scenes=B, points_per_scene=77, points=PTR, texels=PTR, plane_res=PR, texel_dtype=TEXEL_ID[row.tex],
                decoder_image=PTR, n_attention=row.A, attention_values=PTR if row.A > 0 else None, use_sdf=1, beta=PTR,
                alpha=PTR, scene_range=SCENE_RANGE, sigma=PTR, rgb=PTR, sdf=PTR, outside=PTR,
                ray_features=PTR if row.vd else None, samples_per_ray=7 if row.vd else 0, mlp_precision=row.prec)


def field_bwd_query_fields(row):
    out = dict(g_texels=PTR, g_w1=PTR, g_b1=PTR, g_w2=PTR, g_b2=PTR, g_beta=PTR, g_alpha=PTR)
    if row.A > 0:
        out['g_attention_values'] = PTR
    if row.coord:
        out['g_points'] = PTR
    if row.vd:
        out.update(ray_features=PTR, samples_per_ray=8, w3=PTR, g_ray_features=PTR, g_w3=PTR, g_b3=PTR)
    return dict(n_scenes=B, points_per_scene=200, points=PTR, texels=PTR, plane_res=24, texel_dtype=TEXEL_ID[row.tex],
                decoder_image=PTR, w1=PTR, w2=PTR, n_attention=row.A, attention_values=PTR if row.A > 0 else None, use_sdf=1,
                beta=PTR, alpha=PTR, scene_range=SCENE_RANGE, g_sigma=PTR, g_rgb=PTR, g_sdf=PTR,
                g_semantics=PTR if row.A > 0 else None, workspace=PTR, workspace_bytes=1 << 30, **out)


QUERIES = {'nfi_render_args': 'nfi_render_kernel_name', 'nfi_field_args': 'nfi_field_kernel_name',
           'nfi_field_bwd_args': 'nfi_field_bwd_kernel_name'}
_names = {}


def _library():
    """The built library.  NOTE: the parametrisation of the GPU tests asks it for every row's kernel, so COLLECTING this
    module builds the library if it is stale (build() is a no-op otherwise) and makes the ~950 host-only queries; a build
    failure shows as a collection error of this module."""
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def kernel_name(struct_name, fields):
    """(name, None) for a call the argument rules accept, (None, message) for one they refuse."""
    lib = _library()
    a = _lib.make_args(struct_name, **{k: v for k, v in fields.items() if v is not None})
    name = getattr(lib, QUERIES[struct_name])(ctypes.byref(a))
    if name is None:
        msg = lib.nfi_last_error().decode()
        assert msg, 'a refused call leaves a message'
        return None, msg
    return name.decode(), None


def name_of(row):
    key = (type(row).__name__, row)             # (namedtuples of different types compare equal as tuples)
    if key not in _names:
        if isinstance(row, Row):
            _names[key] = kernel_name('nfi_render_args', render_query_fields(row))
        elif isinstance(row, FieldRow):
            _names[key] = kernel_name('nfi_field_args', field_query_fields(row))
        else:
            _names[key] = kernel_name('nfi_field_bwd_args', field_bwd_query_fields(row))
    return _names[key]


def legal(rows):
    return [r for r in rows if name_of(r)[0] is not None]


def library_instantiations():
    """{family: set of canonical names} read from the mangled names in the shared object (host stubs and device symbols
    alike: _Z<len><family>I(L[ib]<value>E)+E)."""
    blob = open(_lib.LIBRARY, 'rb').read()
    found = {}
    for family in FAMILIES:
        pat = re.compile(rb'_Z%d%sI((?:L[ib]\d+E)+)E' % (len(family), family.encode()))
        found[family] = {'%s<%s>' % (family, ','.join(v.decode() for v in re.findall(rb'L[ib](\d+)E', m.group(1))))
                         for m in pat.finditer(blob)}
    return found


# ------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------
def test_matrix_reaches_every_instantiation_and_nothing_else():
    """Completeness, both ways: a kernel in the library that no row of the matrix reaches (a missing row, or dead code in
    a selector), and a row whose kernel is not in the library, both fail.  The counts are the library's at this commit: a
    new kernel forces an edit here."""
    _library()
    in_lib = library_instantiations()
    assert {f: len(s) for f, s in in_lib.items()} == dict(FAMILIES), {f: len(s) for f, s in in_lib.items()}
    reached = {f: set() for f in FAMILIES}
    for row in RENDER_ROWS + FIELD_ROWS + FIELD_BWD_ROWS:
        name = name_of(row)[0]
        if name is not None:
            family = name[:name.index('<')]
            assert family in reached, (row, name)
            reached[family].add(name)
    for family in FAMILIES:
        assert reached[family] == in_lib[family], (family, 'in the library, reached by no row: %s' % sorted(in_lib[family] - reached[family]),
                                                   'named by a row, not in the library: %s' % sorted(reached[family] - in_lib[family]))
    assert sum(len(s) for s in reached.values()) == 138


def test_names_follow_the_axes():
    """Spot checks of the canonical names against the selectors' documented rules (the template arguments in order)."""
    assert name_of(Row('fp32', 10, 24, True, False, 'plain'))[0] == 'render_fwd_kernel<0,1,2,0,1,0>'
    assert name_of(Row('fp16', 0, 24, True, False, 'plain'))[0] == 'render_fwd_kernel<2,0,3,0,1,0>'       # three workgroups per CU
    assert name_of(Row('bf16', 10, 100, True, False, 'term'))[0] == 'render_fwd_wide_kernel<1,1,3,1,0,2>'
    assert name_of(Row('fp32', 14, 100, False, True, 'normals'))[0] == 'render_fwd_wide_kernel<0,1,5,0,1,2>'
    assert name_of(Row('fp32', 0, 100, True, True, 'coords'))[0] == 'render_fwd_wide_kernel<0,0,4,0,1,2>'
    assert name_of(Row('fp16', 10, 200, False, True, 'taps'))[0] == 'render_fwd_long_kernel<2,1,0,1>'
    assert name_of(Row('fp32', 0, 200, False, False, 'strict'))[0] == 'render_fwd_long_kernel<0,0,0,0>'
    assert name_of(FieldRow('bf16', 0, False, 1))[0] == 'field_query_kernel<1,0,0,1>'
    assert name_of(FieldBwdRow('fp16', 10, False, False))[0] == 'field_query_bwd_kernel<1,0,0,2>'
    assert name_of(FieldBwdRow('fp32', 0, True, True))[0] == 'field_query_bwd_kernel<0,1,1,0>'


RENDER_LEGAL_REFUSED = (380, 520)        # of the 900 rows of the render matrix


def test_refused_rows_are_refused_with_a_message():
    """Every row the argument rules refuse returns NULL and says why; the counts of legal and refused rows are pinned so
    that a rule that starts to accept more (or less) is seen."""
    counts = {}
    for what, rows in (('render', RENDER_ROWS), ('field', FIELD_ROWS), ('field_bwd', FIELD_BWD_ROWS)):
        refused = [r for r in rows if name_of(r)[0] is None]
        for r in refused:
            assert name_of(r)[1].startswith(('render:', 'field')), (r, name_of(r)[1])
        counts[what] = (len(rows) - len(refused), len(refused))
    assert counts == {'render': RENDER_LEGAL_REFUSED, 'field': (18, 6), 'field_bwd': (16, 8)}, counts
    # the rules, one by one, on rows of the matrix
    why = lambda *row: name_of(Row(*row))[1] or ''
    assert 'n_samples' in why('fp32', 10, 200, True, False, 'plain')                    # 128 per pass with a fine pass
    assert 'cycle profile' in why('fp32', 10, 100, True, False, 'profile')
    assert 'n_samples <= 128' in why('fp32', 10, 200, False, False, 'coords')
    assert 'attention values' in why('fp32', 0, 24, True, False, 'semantics')
    assert 'fine pass' in why('fp32', 10, 24, False, False, 'term')
    assert 'termination_eps cannot' in why('fp32', 10, 24, True, True, 'term')
    assert 'fp32 texels' in why('fp16', 10, 24, True, True, 'coords')
    assert 'fp32 texels' in why('bf16', 10, 24, True, False, 'strict')
    assert 'fp32 texels' in why('fp16', 10, 24, True, False, 'profile')
    assert 'no cycle profile' in why('fp32', 10, 24, True, True, 'profile')
    assert 'mlp_precision' in name_of(FieldRow('fp32', 10, True, 1))[1]
    assert 'fp32 texels' in name_of(FieldBwdRow('fp16', 10, True, True))[1]


def render_configs():
    return sorted({config_of(r) for r in legal(RENDER_ROWS)})


def test_scenes_are_well_conditioned_for_the_reference():
    """A condition on the INPUTS, so that a row over its bound on the GPU is the kernel's doing: for every oracle
    configuration of the matrix the float32 oracle is within 1e-5 of the float64 oracle on the same (rounded) inputs - rgb,
    depth and mask of every ray, and the composited normal map where a row asks for it - and in every scene at least 10 % of
    the rays miss the cube while the mean mask is at least 0.1 (the skip path and the marching path both run)."""
    bad = []
    worst = 0.0
    normal_cfgs = {config_of(r) for r in legal(RENDER_ROWS) if r.mode == 'normals'}
    for cfg in render_configs():
        meta, t32, o32 = oracle_of(cfg)
        _, t64, o64 = oracle_of(cfg, torch.float64)
        d = max(float((o32[k].double() - o64[k]).abs().max()) for k in ('rgb', 'depth', 'mask'))
        if cfg in normal_cfgs:
            d = max(d, float((normal_map_of(cfg).double() - normal_map_of(cfg, torch.float64)).abs().max()))
        worst = max(worst, d)
        if not d <= 1e-5:
            bad.append((row_id(cfg), 'float32 vs float64 oracle', d))
        for b in range(B):
            miss, mask = 1.0 - float(o32['hit'][b].float().mean()), float(o32['mask'][b].mean())
            if miss < 0.1 or mask < 0.1:
                bad.append((row_id(cfg), 'scene %d: %.3f of the rays miss the cube, mean mask %.3f' % (b, miss, mask)))
    print('%d oracle configurations, largest float32 - float64 difference %.2e' % (len(render_configs()), worst))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def launches_recorded(struct_name, entry):
    """Asks the library, for every call of `entry` made inside, which kernel that very argument struct gets."""
    seen, real = [], _lib.call_struct

    def recording(fname, sname, stream, **kw):
        if fname == entry:
            a = _lib.make_args(sname, **kw)
            name = getattr(_lib.load(), QUERIES[struct_name])(ctypes.byref(a))
            seen.append(None if name is None else name.decode())
        return real(fname, sname, stream, **kw)
    _lib.call_struct = recording
    try:
        yield seen
    finally:
        _lib.call_struct = real


def close(a, b, tol, what):
    e = err(a, b)
    print('%-60s max %.3e (bound %.1e)' % (what, e['max'], tol))
    assert e['nonfinite'] == 0 and e['max'] <= tol, (what, e)


def exact(a, b, what):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape and torch.equal(a, b), (what, err(a.float(), b.float()))


def image_close(r, o, tol, what):
    for k in ('rgb', 'depth', 'mask'):
        close(r[k], o[k], tol, '%s: %s' % (what, k))


def image_exact(r, base, what):
    for k in ('rgb', 'depth', 'mask'):
        exact(r[k], base[k], '%s: %s' % (what, k))


def check_taps(r, o, meta, what):
    close(r['t_coarse'], o['t_coarse'], 1e-5, what + ': t_coarse')
    sigma_close(r['sigma_coarse'], o['sigma_coarse'], what + ': sigma_coarse')
    exact((r['hit'] & 1).bool(), o['hit'], what + ': hit mask')
    if meta['fine']:
        close(r['t_fine'], o['t_fine'], 1e-4, what + ': t_fine')
        close(r['t_sorted'], o['t_sorted'], 1e-4, what + ': t_sorted')
        flips = (r['perm'].cpu().long() != o['perm']).float().mean().item()
        assert flips <= 2e-4, (what, 'sort permutation flips', flips)


@pytest.mark.gpu
@pytest.mark.parametrize('row', legal(RENDER_ROWS), ids=row_id)
def test_render_row(gpu_device, row):
    dev = gpu_device
    cfg = config_of(row)
    kernel = name_of(row)[0]
    meta, tr, o = oracle_of(cfg)
    _, t = scene_of(cfg)
    what = '%s [%s]' % (row_id(row), kernel)
    tol = ATOL if row.tex == 'fp32' else 2e-4       # 16-bit storage: against the oracle on the rounded planes
    skip = skip_missed_of(row)
    tdt = TEXEL_ID[row.tex]
    mode = row.mode

    def run(**kw):
        kw.setdefault('skip_missed_rays', skip)
        return hip_render(meta, t, dev, texel_dtype=tdt, **kw)

    def run_row(**kw):
        """the launch of the row: its kernel must be the one the matrix names"""
        with launches_recorded('nfi_render_args', 'nfi_render_fwd') as seen:
            r = run(**kw)
        assert seen == [kernel], (what, seen)
        return r

    if mode == 'plain':
        image_close(run_row(), o, tol, what)
    elif mode in ('taps', 'strict+taps'):
        tuning = 8 if mode == 'strict+taps' else 0
        r = run_row(taps=ops.TAP_NAMES, tuning=tuning)
        image_close(r, o, tol, what)
        check_taps(r, o, meta, what)
        if tuning:
            split = run(taps=ops.TAP_NAMES)
            for k in ('rgb', 'depth', 'mask'):
                close(r[k], split[k], 3e-5, what + ': exact-fp32 vs split-fp16 MLP, ' + k)
    elif mode == 'stash':
        st = run_row(stash=True)
        plain = run()
        tp = run(taps=('t_coarse', 'sigma_coarse', 'rgb_coarse', 't_fine', 'sigma_fine', 'rgb_fine', 'hit'))
        image_exact(st, plain, what + ': stash launch vs plain launch')
        image_close(st, o, tol, what)
        marched = (tp['hit'] & 2) != 0
        assert 0 < int(marched.sum()) < marched.numel(), what
        for name in ('t', 'sigma', 'rgb'):
            both = torch.cat((tp[name + '_coarse'], tp[name + '_fine']), dim=3) if row.fine else tp[name + '_coarse']
            got = st['stash_' + name]
            assert got.shape == both.shape, (what, name)
            exact(got[marched], both[marched], what + ': stash ' + name)
            assert float(got[~marched].abs().max()) == 0.0, (what, name)
    elif mode == 'term':
        f = run_row(termination_eps=TERM_EPS)
        e0, plain = run(termination_eps=0.0), run()
        image_exact(e0, plain, what + ': eps = 0 vs plain')
        image_close(f, o, tol, what)
        image_close(f, e0, 6 * TERM_EPS, what + ': eps = 1e-5 vs eps = 0')
    elif mode in ('semantics', 'coords', 'semantics+coords'):
        sem, crd = 'semantics' in mode, 'coords' in mode
        r = run_row(want_semantics=sem, want_coords=crd)
        image_exact(r, run(), what + ': extra-map launch vs plain launch')
        image_close(r, o, tol, what)
        if sem:
            assert r['semantics'].shape == (B,) + cfg.shape + (row.A,)
            close(r['semantics'], o['semantics'], 1e-5, what + ': semantic map')
            # (64 < S <= 128: the kernel scales its map to the mask, so there this holds by construction and says nothing
            #  about the unorm16 table the probabilities wait in - the comparison with the oracle above is what tests it)
            close(r['semantics'].sum(-1), r['mask'], 2e-5, what + ': sum of the semantic map = mask')
            assert float(r['semantics'].min()) >= 0.0
        if crd:
            close(r['coords'], coords_map(o, meta), 1e-5, what + ': coords map')
    elif mode == 'normals':
        r = run_row(want_normals=True)
        image_exact(r, run(), what + ': normal-map launch vs plain launch')
        image_close(r, o, tol, what)
        close(r['normals'], normal_map_of(cfg), 3e-5 if row.tex == 'fp32' else 6e-5, what + ': normal map')
    elif mode == 'strict':
        r = run_row(tuning=8)
        image_close(r, o, tol, what)
        split = run()
        for k in ('rgb', 'depth', 'mask'):
            close(r[k], split[k], 3e-5, what + ': exact-fp32 vs split-fp16 MLP, ' + k)
    elif mode == 'profile':
        prof = torch.zeros(12, dtype=torch.int64, device=dev)
        r = run_row(profile_cycles=prof)
        image_close(r, o, tol, what)
        p = prof.cpu().tolist()
        # field tile {gather + interpolation, mlp, count} in [1..3] ([0], the gather's issue half, is counted in [1]), ray
        # set-up, coarse field, resample, fine field, merge, composite, rays marched, wave lifetime
        live = [1, 2, 3, 4, 5, 9, 10, 11] + ([6, 7, 8] if row.fine else [])
        assert all(p[i] > 0 for i in live), (what, p)
        assert p[10] <= B * cfg.shape[0] * cfg.shape[1], (what, p)
    else:
        raise AssertionError(mode)


def field_scene(row, seed, P, spr, R=PR):
    g = torch.Generator().manual_seed(seed)
    A = row.A
    n_out = 33 if row.vd else (1 + A if A > 0 else 4)
    low = torch.randn(B * 3, 32, 8, 8, generator=g)
    planes = torch.nn.functional.interpolate(low, size=(R, R), mode='bilinear', align_corners=True).view(B, 3, 32, R, R) \
        + 0.1 * torch.randn(B, 3, 32, R, R, generator=g)
    t = dict(planes=planes.to(TEXEL_TORCH[row.tex]).float(), w1=torch.randn(64, 32, generator=g), b1=0.3 * torch.randn(64, generator=g),
             w2=torch.randn(n_out, 64, generator=g), b2=0.3 * torch.randn(n_out, generator=g),
             beta=torch.tensor([0.12]), alpha=torch.tensor([0.3]))
    if A > 0:
        t['attention_values'] = torch.rand(B, A, 3, generator=g) * 2 - 1
    if row.vd:
        n3 = A if A > 0 else 3
        t.update(viewdir_x=torch.randn(B, P // spr, 32, generator=g), w3=torch.randn(n3, 32, generator=g),
                 b3=0.3 * torch.randn(n3, generator=g))
    return t, g


@pytest.mark.gpu
@pytest.mark.parametrize('row', legal(FIELD_ROWS), ids=row_id)
def test_field_row(gpu_device, row):
    """Points inside and outside the cube, on its faces and far away, P = 77 (no multiple of 64)."""
    dev = gpu_device
    kernel = name_of(row)[0]
    what = '%s [%s]' % (row_id(row), kernel)
    P, spr = 77, 7
    t, g = field_scene(row, 4000 + FIELD_ROWS.index(row), P, spr)
    use_sdf = FIELD_ROWS.index(row) % 3 != 1
    r = float(torch.tensor(SCENE_RANGE, dtype=torch.float32))
    x = (torch.rand(B, P, 3, generator=g) * 2 - 1) * r * 1.5
    x[0, :3] = torch.tensor([[r, -r, r], [r, 0.0, 0.0], [-r, -r, -r]])
    x[1, 5] = torch.tensor([1e6, -1e6, 3.0])
    meta = dict(A=row.A)
    texels, image = hip_field_setup(meta, t, dev, TEXEL_ID[row.tex])
    att = t['attention_values'] if row.A > 0 else None
    with launches_recorded('nfi_field_args', 'nfi_field_query_fwd') as seen:
        q = ops.field_query(x.to(dev), texels, image, r, row.A, None if att is None else att.to(dev), use_sdf,
                            t['beta'].to(dev), t['alpha'].to(dev), want_sdf=True, want_semantics=row.A > 0, want_outside=True,
                            ray_features=ops.pad_ray_features(t['viewdir_x'].to(dev)) if row.vd else None,
                            samples_per_ray=spr if row.vd else 0, mlp_precision=row.prec)
    assert seen == [kernel], (what, seen)
    ref = orc.field_query(t['planes'], t['w1'], t['b1'], t['w2'], t['b2'], x.view(B, P // spr, spr, 3), r, use_sdf, t['beta'],
                          t['alpha'], att, dict(x=t['viewdir_x'], w3=t['w3'], b3=t['b3']) if row.vd else None)
    assert 0.2 < float(ref['outside'].mean()) < 0.9
    exact(q['outside'].float(), ref['outside'], what + ': outside')
    close(q['sdf'], ref['sdf'], 1e-5, what + ': sdf')
    sigma_close(q['sigma'], ref['sigma'], what + ': sigma')
    close(q['rgb'], ref['rgb'], ATOL, what + ': rgb')
    if row.A > 0:
        close(q['semantics'], ref['semantics'], 1e-5, what + ': semantics')


def field_grads(t, x, ups, use_sdf, A, vd, spr, dtype):
    """autograd of orc.field_query in `dtype`: {name: gradient}"""
    leaf = lambda v: v.detach().to(dtype).requires_grad_()
    names = ['planes', 'w1', 'b1', 'w2', 'b2'] + (['attention_values'] if A > 0 else []) + (['beta', 'alpha'] if use_sdf else []) + \
        (['viewdir_x', 'w3', 'b3'] if vd else [])
    L = {k: leaf(t[k]) for k in names}
    L['points'] = leaf(x)
    q = orc.field_query(L['planes'], L['w1'], L['b1'], L['w2'], L['b2'], L['points'].view(B, -1, spr, 3), float(torch.tensor(SCENE_RANGE)),
                        use_sdf, L.get('beta'), L.get('alpha'), L.get('attention_values'),
                        dict(x=L['viewdir_x'], w3=L['w3'], b3=L['b3']) if vd else None)
    loss = sum((q[k].view(ups[k].shape) * ups[k].to(dtype)).sum() for k in ups)
    keys = list(L)
    return dict(zip(keys, torch.autograd.grad(loss, [L[k] for k in keys])))


@pytest.mark.gpu
@pytest.mark.parametrize('row', legal(FIELD_BWD_ROWS), ids=row_id)
def test_field_bwd_row(gpu_device, row):
    """Every gradient of nfi_field_query_bwd against float64 autograd of the oracle's field query (16-bit texels: on the
    rounded planes, straight through), each within 5e-4 of its own largest entry; without g_points the other gradients
    are the ones of the launch that wants it, up to the summation order of the atomics."""
    from nerf_from_image_amd import field_backward as fb
    dev = gpu_device
    kernel = name_of(row)[0]
    what = '%s [%s]' % (row_id(row), kernel)
    i = FIELD_BWD_ROWS.index(row)
    P, spr, R, A = 200, 8, 24, row.A
    use_sdf = (i // 2) % 3 != 1
    scatter = (i // 2) % 2
    t, g = field_scene(row, 5000 + i // 2, P, spr, R)              # (the two rows of a pair share their inputs)
    r = float(torch.tensor(SCENE_RANGE, dtype=torch.float32))
    x = (torch.rand(B, P, 3, generator=g) * 2 - 1) * r * 1.1
    x[0, 0] = torch.tensor([r, 0.1, -r])
    ups = dict(sigma=torch.randn(B, P, generator=g), rgb=torch.randn(B, P, 3, generator=g), sdf=torch.randn(B, P, generator=g))
    if A > 0:
        ups['semantics'] = torch.randn(B, P, A, generator=g)
    ref = field_grads(t, x, ups, use_sdf, A, row.vd, spr, torch.float64)
    ref32 = field_grads(t, x, ups, use_sdf, A, row.vd, spr, torch.float32)

    mv = lambda v: None if v is None else v.to(dev)
    texels, image = hip_field_setup(dict(A=A), t, dev, TEXEL_ID[row.tex])
    vd = dict(ray_features=ops.pad_ray_features(mv(t['viewdir_x'])), samples_per_ray=spr, w3=mv(t['w3'])) if row.vd else None

    def run(**kw):
        return fb.field_query_bwd(mv(x), texels, image, mv(t['w1']), mv(t['w2']), r, A, mv(t.get('attention_values')), use_sdf,
                                  mv(t['beta']), mv(t['alpha']), mv(ups['sigma']), mv(ups['rgb']), g_sdf=mv(ups['sdf']),
                                  g_semantics=mv(ups.get('semantics')), viewdir=vd, scatter_mode=scatter, **kw)

    with launches_recorded('nfi_field_bwd_args', 'nfi_field_query_bwd') as seen:
        got = run(want_points=row.coord)
    assert seen == [kernel], (what, seen)
    pairs = {'planes': ops.texel_grad_to_planes(got['g_texels']), 'w1': got['g_w1'], 'b1': got['g_b1'], 'w2': got['g_w2'],
             'b2': got['g_b2']}
    if A > 0:
        pairs['attention_values'] = got['g_attention_values']
    if use_sdf:
        pairs.update(beta=got['g_beta'], alpha=got['g_alpha'])
    if row.vd:
        pairs.update(viewdir_x=got['g_ray_features'], w3=got['g_w3'], b3=got['g_b3'])
    if row.coord:
        pairs['points'] = got['g_points']
    assert float(pairs['planes'].abs().max()) > 0
    for k, v in pairs.items():
        grad_close(v, ref[k], 5e-4, '%s: grad %s' % (what, k), ref32[k])
    if row.coord:
        # points_only: the coordinate gradient alone, from the same kernel; normalised: unit rows of the same vectors
        po = run(points_only=True)
        grad_close(po['g_points'], ref['points'], 5e-4, what + ': points_only grad points', ref32['points'])
        pn = run(points_only=True, normalize_points=True)['g_points']
        unit = torch.nn.functional.normalize(po['g_points'], dim=-1, eps=1e-12)
        close(pn, unit, 1e-6, what + ': normalize_g_points')         # the same fp32 vector divided by its own norm
    else:
        full = run(want_points=True)
        for k in got:
            grad_close(got[k], full[k], 1e-3 if k in ('g_beta', 'g_alpha') else 2e-5, '%s: %s without vs with g_points' % (what, k))
