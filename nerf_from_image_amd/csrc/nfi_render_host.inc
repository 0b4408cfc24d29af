// nfi_render_host.inc — the host side of the fused render: the workspace and its layout, the ray set-up with its finish
// kernel and block table (nfi_render_workspace_bytes, nfi_render_setup), the argument checks, select_render_kernel
// (nfi_render_kernel_name) and the launch (nfi_render_fwd) (included by nfi_kernels.hip; left out of the
// NFI_SINGLE_KERNEL compiles).  Expects the three render kernels (nfi_render_kernels.inc, nfi_render_long.inc) and
// nfi_rays.inc (raygen_kernel, RayPartial, kRayBlocks, block_reduce_keys).

// The render workspace: [RenderWorkspaceHeader][ro, rd: 3n floats each][near_raw, far_raw: n floats each][hit: n bytes,
// padded to 64][kRayBlocks RayPartial: the per-block partials of the ray set-up's reduction][block_table: n / 64
// uint32, at byte 576 + 32 n + pad64(n) + 16 384].  The header is what raygen_finish_kernel writes, every cell of it;
// callers read reduce[] from it (the first three cells of the workspace).
struct RenderWorkspaceHeader {
  uint32_t reduce[3];            // the batch-wide miss-fill of the ray set-up: ~key(min near), key(max far), hit count
  uint32_t counter;              // the device-wide work counter (RenderKernelParams::counter)
  uint32_t pad[12];
  uint32_t xcd_counter[8][16];   // the per-XCD work counters, 64 bytes apart (RenderKernelParams::xcd_counter)
};
static_assert(sizeof(RenderWorkspaceHeader) == 64 + 8 * 64 && offsetof(RenderWorkspaceHeader, xcd_counter) == 64,
              "the render workspace header is read from Python and by the kernels' 16-dword counter stride");

// the documented prefix of the workspace: header and ray arrays
static size_t render_workspace_prefix_bytes(int64_t n_rays) {
  size_t n = (size_t)n_rays;
  return sizeof(RenderWorkspaceHeader) + n * 8 * sizeof(float) + ((n + 63) & ~(size_t)63);
}

static size_t render_workspace_table_offset(int64_t n_rays) {
  return render_workspace_prefix_bytes(n_rays) + kRayBlocks * sizeof(RayPartial);
}

extern "C" size_t nfi_render_workspace_bytes(int64_t n_rays) {
  return render_workspace_table_offset(n_rays) + ((size_t)n_rays / 64) * sizeof(uint32_t);
}

// The square pixel blocks of the per-XCD queues: the largest of 32 / 16 / 8 pixels that divides both image sides (shift:
// log2 of the side; ok: at least 8 does).  One copy for the set-up, which writes the block table, and the render kernel.
struct BlockGeometry { int shift, ok; uint32_t bw, bh, n_blocks; };
static BlockGeometry render_block_geometry(const nfi_render_args* a) {
  BlockGeometry g;
  const int both = a->width | a->height;
  g.shift = (both & 31) == 0 ? 5 : ((both & 15) == 0 ? 4 : 3);
  const int side = 1 << g.shift;
  g.ok = (a->width % side == 0) && (a->height % side == 0) ? 1 : 0;
  g.bw = (uint32_t)a->width >> g.shift; g.bh = (uint32_t)a->height >> g.shift;
  g.n_blocks = g.bw * g.bh * (uint32_t)a->n_scenes;
  return g;
}

// rays of p[0..bytes) whose hit byte has bit 1 set (the inflated test); bytes: 8 or 16
__device__ __forceinline__ uint32_t count_wide_hits(const uint8_t* p, int bytes) {
  uint32_t c = 0;
  if (bytes == 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    c = __popc(v.x & 0x02020202u) + __popc(v.y & 0x02020202u) + __popc(v.z & 0x02020202u) + __popc(v.w & 0x02020202u);
  } else if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    for (int i = 0; i < bytes; i += 4) c += __popc(*reinterpret_cast<const uint32_t*>(p + i) & 0x02020202u);
  } else {
    for (int i = 0; i < bytes; ++i) c += (p[i] >> 1) & 1u;
  }
  return c;
}

// The tail of the ray set-up, behind raygen_kernel in the stream.  Block 0: reduce[0..2] from the blocks' partials (max,
// max, sum: any order gives the same cells), zeros in the work counters and the identity part of the block table (every
// slot outside a complete group of 16) - plain stores to every cell, so a workspace straight from the allocator needs no
// clearing.  Block 1 + G: group G of the block table.  Slot g = 8 * slot + q belongs to XCD q, so an aligned group of 16
// slots gives every XCD two blocks; the group's 16 pixel blocks are ranked by their rays with hit bit 1 (count descending,
// index ascending; 16 threads count one block along its rows, the counts meet in LDS, 16 lanes rank by counting), rank r
// and rank 15 - r share XCD (min(r, 15 - r) + G) % 8, the heavier of the two first.  No atomics, no block waits for
// another; the render kernels read the table as a hint for balance only (any permutation of a group renders the same).
struct BlockTableParams { const uint8_t* hit; uint32_t* table; int shift, width, hw; uint32_t bw, bps, n_blocks, groups; };

__global__ __launch_bounds__(256) void raygen_finish_kernel(const RayPartial* __restrict__ partial, int n_partials,
                                                            RenderWorkspaceHeader* __restrict__ head, BlockTableParams t) {
  if (blockIdx.x != 0) {
    __shared__ uint32_t s_part[256], s_count[16];
    const uint32_t G = blockIdx.x - 1, i = threadIdx.x >> 4, sub = threadIdx.x & 15u;
    const uint32_t b = 16u * G + i, scene = b / t.bps, bb = b - scene * t.bps, by = bb / t.bw, bx = bb - by * t.bw;
    const uint8_t* base = t.hit + (size_t)scene * (size_t)t.hw + (size_t)(by << t.shift) * (size_t)t.width + (bx << t.shift);
    const int side = 1 << t.shift, cw = side < 16 ? side : 16, per_row = side / cw;     // a row in chunks of cw bytes
    uint32_t c = 0;
    for (int ch = (int)sub; ch < side * per_row; ch += 16)
      c += count_wide_hits(base + (size_t)(ch / per_row) * (size_t)t.width + (ch % per_row) * cw, cw);
    s_part[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x < 16) {
      uint32_t sum = 0;
      for (int j = 0; j < 16; ++j) sum += s_part[threadIdx.x * 16 + j];
      s_count[threadIdx.x] = sum;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
      const uint32_t me = threadIdx.x, mine = s_count[me];
      uint32_t r = 0;
      for (uint32_t j = 0; j < 16; ++j) r += (s_count[j] > mine || (s_count[j] == mine && j < me)) ? 1u : 0u;
      const uint32_t pair = r < 8 ? r : 15u - r, x = (pair + G) & 7u;
      t.table[16u * G + (r < 8 ? 0u : 8u) + x] = 16u * G + me;
    }
    return;
  }
  uint32_t kmin = 0u, kmax = 0u, cnt = 0u;
  for (int i = threadIdx.x; i < n_partials; i += blockDim.x) {
    const RayPartial p = partial[i];
    kmin = p.kmin > kmin ? p.kmin : kmin;
    kmax = p.kmax > kmax ? p.kmax : kmax;
    cnt += p.cnt;
  }
  block_reduce_keys(kmin, kmax, cnt);
  uint32_t* cells = reinterpret_cast<uint32_t*>(head);
  for (int i = 3 + threadIdx.x; i < (int)(sizeof(RenderWorkspaceHeader) / sizeof(uint32_t)); i += blockDim.x) cells[i] = 0u;
  if (threadIdx.x == 0) { head->reduce[0] = kmin; head->reduce[1] = kmax; head->reduce[2] = cnt; }
  for (uint32_t g = 16u * t.groups + threadIdx.x; g < t.n_blocks; g += blockDim.x) t.table[g] = g;
}

// workspace carve + ray set-up shared by nfi_render_setup and nfi_render_fwd
struct RenderWorkspace {
  RenderWorkspaceHeader* head; float* ro; float* rd; float* near_raw; float* far_raw; uint8_t* hit; RayPartial* partial; uint32_t* block_table; int64_t n;
};

static int render_carve(const nfi_render_args* a, RenderWorkspace& w) {
  REQUIRE(a && a->cam2world && a->workspace, "render: null pointer");
  REQUIRE(a->n_scenes > 0 && a->height > 0 && a->width > 0, "render: bad image shape");
  const int64_t n = (int64_t)a->n_scenes * a->height * a->width;
  if (a->workspace_bytes < nfi_render_workspace_bytes(n)) return fail(NFI_ERR_WORKSPACE_TOO_SMALL, "render: workspace too small");
  w.n = n;
  w.head = reinterpret_cast<RenderWorkspaceHeader*>(a->workspace);
  float* rays = reinterpret_cast<float*>(w.head + 1);
  w.ro = a->ray_origins ? a->ray_origins : rays;
  w.rd = a->ray_directions ? a->ray_directions : rays + 3 * n;
  w.near_raw = rays + 6 * n;
  w.far_raw = rays + 7 * n;
  w.hit = a->hit ? a->hit : reinterpret_cast<uint8_t*>(rays + 8 * n);
  w.partial = reinterpret_cast<RayPartial*>(reinterpret_cast<char*>(a->workspace) + render_workspace_prefix_bytes(n));
  w.block_table = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a->workspace) + render_workspace_table_offset(n));
  return NFI_OK;
}

static int render_setup(const nfi_render_args* a, const RenderWorkspace& w, hipStream_t s) {
  const int full_h = a->full_height > 0 ? a->full_height : a->height;
  REQUIRE(a->row_offset >= 0 && a->row_offset + a->height <= full_h, "render: row window outside the image");
  CameraParams cam{a->cam2world, a->focal, a->bbox, a->focal ? a->center : nullptr, full_h, a->width, 1, a->height, a->row_offset};
  RaygenOut rout{w.ro, w.rd, w.near_raw, w.far_raw, w.hit, w.partial, a->scene_range};
  const int blocks = (int)std::min<int64_t>((w.n + 255) / 256, kRayBlocks);
  hipLaunchKernelGGL(raygen_kernel, dim3((unsigned)blocks), dim3(256), 0, s, cam, a->n_scenes, rout);
  // the block table: complete groups of 16 blocks are paired by hit count, the rest (and everything when the per-XCD
  // queues cannot be used, or there are fewer than 16 blocks) is the identity
  const BlockGeometry g = render_block_geometry(a);
  const uint32_t n_table = g.ok ? g.n_blocks : (uint32_t)(w.n / 64), groups = g.ok ? g.n_blocks / 16 : 0u;
  const BlockTableParams t{w.hit, w.block_table, g.shift, a->width, a->height * a->width, g.bw, g.bw * g.bh, n_table, groups};
  hipLaunchKernelGGL(raygen_finish_kernel, dim3(1 + groups), dim3(256), 0, s, w.partial, blocks, w.head, t);
  return NFI_OK;
}

extern "C" int nfi_render_setup(const nfi_render_args* a, nfi_stream_t stream) {
  RenderWorkspace w;
  int rc = render_carve(a, w);
  if (rc) return rc;
  rc = render_setup(a, w, (hipStream_t)stream);
  if (rc) return rc;
  return check_launch("render_setup");
}

// What of a render call picks the kernel variant, besides the texel type and the sample count: the training stash, any
// per-sample / per-ray debug tap (these switch the missed-ray skip off), either of the two (the kRenderTaps kernels), the
// exact-fp32 MLP instead of the split-fp16 one, ray termination in the fine pass, a semantics / coords / normals map
struct RenderFlags { bool stash, debug_tap, any_tap, strict, term, extra; };

static RenderFlags render_flags(const nfi_render_args* a) {
  RenderFlags f;
  f.stash = a->stash_t || a->stash_sigma || a->stash_rgb;
  f.debug_tap = a->t_coarse || a->sigma_coarse || a->rgb_coarse || a->t_fine || a->sigma_fine || a->rgb_fine ||
                a->t_sorted || a->weights || a->perm || a->near_plane || a->far_plane;
  f.any_tap = f.debug_tap || f.stash;
  f.strict = (a->tuning & NFI_TUNING_EXACT_FP32_MLP) != 0;
  f.term = a->termination_eps > 0.0f;
  f.extra = a->semantics || a->coords || a->normals;
  return f;
}

// The argument rules of nfi_render_fwd, in two parts: the ray set-up runs between them (rules are reported in this order)
static int render_check_call(const nfi_render_args* a) {
  REQUIRE(a && a->cam2world && a->rgb && a->depth && a->mask && a->workspace, "render: null pointer");
  REQUIRE(a->n_scenes > 0 && a->height > 0 && a->width > 0, "render: bad image shape");
  REQUIRE(a->views_per_scene >= 0, "render: views_per_scene must not be negative (0 and 1 both mean one view)");
  REQUIRE(a->n_scenes % std::max(a->views_per_scene, 1) == 0, "render: n_scenes (the number of images) must be a multiple of views_per_scene");
  REQUIRE(a->n_samples >= 4 && a->n_samples <= (a->fine_sampling ? NFI_MAX_SAMPLES : NFI_MAX_SAMPLES_SINGLE_PASS),
          "render: n_samples must be in [4,128] per pass with fine sampling, [4,512] for a single pass");
  REQUIRE(a->n_samples <= 64 || !a->profile_cycles, "render: the cycle profile exists for n_samples <= 64 only");
  REQUIRE(a->n_samples <= NFI_MAX_SAMPLES || !(a->semantics || a->coords || a->normals),
          "render: semantics / coords / normals maps exist for n_samples <= 128");
  REQUIRE(!a->fine_sampling || a->noise_fine, "render: fine sampling needs u (noise_fine)");
  REQUIRE(!a->semantics || a->n_attention > 0, "render: composited semantics need attention values (A > 0)");
  return check_field_common(a->texels, a->plane_res, a->texel_dtype, a->decoder_image, a->n_attention,
                            a->attention_values, a->use_sdf, a->beta, a->alpha, a->texel_layout);
}

static int render_check_variant(const nfi_render_args* a, const RenderFlags& f) {
  REQUIRE(!f.stash || (a->stash_t && a->stash_sigma && a->stash_rgb), "render: the training stash needs stash_t, stash_sigma and stash_rgb");
  REQUIRE(!f.stash || !(a->t_coarse || a->sigma_coarse || a->rgb_coarse || a->t_fine || a->sigma_fine || a->rgb_fine),
          "render: the training stash and the per-sample debug taps are mutually exclusive");
  REQUIRE(!a->normals || a->use_sdf, "render: the normals map needs the SDF decoder (use_sdf)");
  REQUIRE(a->termination_eps >= 0.0f && a->termination_eps < 1.0f, "render: termination_eps must be in [0,1)");
  REQUIRE(!f.term || a->fine_sampling, "render: termination_eps acts on the fine pass (fine_sampling)");
  REQUIRE(!f.term || !(f.any_tap || f.extra || a->profile_cycles || a->ray_features || f.strict),
          "render: termination_eps cannot be combined with stage taps, extra maps, the cycle profile, the view-direction decoder or the exact-fp32 MLP");
  REQUIRE(!f.extra || !(f.any_tap || a->profile_cycles || f.strict),
          "render: semantics / coords / normals maps cannot be combined with stage taps, the cycle profile or the exact-fp32 MLP");
  REQUIRE(!(f.extra && a->ray_features) || a->texel_dtype == NFI_TEXEL_F32,
          "render: with the view-direction decoder the semantics / coords / normals maps exist for fp32 texels");
  // the exact-fp32 MLP (a diagnostic of the split-fp16 arithmetic) and the cycle profile are built for fp32 texels only:
  // with 16-bit texel storage the texels, not the MLP operands, set the precision
  REQUIRE(!(f.strict || a->profile_cycles) || a->texel_dtype == NFI_TEXEL_F32,
          "render: the exact-fp32 MLP (tuning bit 3) and the cycle profile exist for fp32 texels");
  REQUIRE(!(a->ray_features && a->profile_cycles), "render: no cycle profile with the view-direction decoder");
  return NFI_OK;
}

static RenderKernelParams render_kernel_params(const nfi_render_args* a, const RenderWorkspace& w, const RenderFlags& f) {
  RenderKernelParams k;
  memset(&k, 0, sizeof(k));
  k.n_scenes = a->n_scenes; k.hw = a->height * a->width; k.S = a->n_samples;
  k.fine = a->fine_sampling; k.white = a->white_background; k.scene_range = a->scene_range;
  k.ro = w.ro; k.rd = w.rd; k.near_raw = w.near_raw; k.far_raw = w.far_raw; k.hit = w.hit; k.reduce = w.head->reduce;
  k.texels = a->texels; k.res = a->plane_res; k.layout = a->texel_layout; k.image = a->decoder_image; k.A = a->n_attention; k.att = a->attention_values;
  k.use_sdf = a->use_sdf; k.beta = a->beta; k.alpha = a->alpha;
  k.noise_c = a->noise_coarse; k.noise_f = a->noise_fine; k.noise_f_stride = a->noise_fine_row_stride;
  k.rgb = a->rgb; k.depth = a->depth; k.mask = a->mask;
  k.near_plane = a->near_plane; k.far_plane = a->far_plane;
  k.t_coarse = a->t_coarse; k.sigma_coarse = a->sigma_coarse; k.rgb_coarse = a->rgb_coarse;
  k.t_fine = a->t_fine; k.sigma_fine = a->sigma_fine; k.rgb_fine = a->rgb_fine;
  k.tap_stride = a->n_samples;
  if (f.stash) {
    // the stash rows hold the coarse samples in [0,S) and - with fine sampling - the fine samples in [S,2S)
    k.tap_stride = (a->fine_sampling ? 2 : 1) * a->n_samples; k.stash = 1;
    k.t_coarse = a->stash_t; k.sigma_coarse = a->stash_sigma; k.rgb_coarse = a->stash_rgb;
    if (a->fine_sampling) {
      k.t_fine = a->stash_t + a->n_samples;
      k.sigma_fine = a->stash_sigma + a->n_samples;
      k.rgb_fine = a->stash_rgb + 3 * (size_t)a->n_samples;
    }
  }
  k.t_sorted = a->t_sorted; k.weights = a->weights; k.perm = a->perm;
  k.skip_missed = (a->skip_missed_rays && !f.debug_tap) ? 1 : 0;

  k.counter = &w.head->counter;
  k.xcd_counter = &w.head->xcd_counter[0][0];
  k.width = a->width;
  // per-XCD queues (NFI_TUNING_SINGLE_WORK_COUNTER switches them off): square pixel blocks, needs image sides that are
  // multiples of 8: the largest of 32 / 16 / 8-pixel blocks that divides both image sides, TWO positions per atomic.
  // MI355X, 8 x 128^2 x (64+64), ms per launch chairs-like / every ray hits / one image (round 3, build-time variants):
  // 32x32 + 2: 0.854 / 1.299 / 0.164; 8x8 + 2: 0.848 / 1.328 / 0.167; 16x16 + 2: 0.891 / 1.301 / 0.170; 16x16 + 1 (the
  // round-1 default): 0.933 / 1.311 / 0.185; 32x32 + 1: 0.882 / 1.317 / 0.174; 4 per atomic: 0.88-0.90 / 1.33-1.38; one
  // device-wide counter 1.82 / 2.10.  Halving the atomics matters on every workload (the wave waits for each one's
  // result); the block side mostly through the balance of the chairs-like images, whose rays that cross the cube are
  // clustered.
  k.fetch_batch = 2;
  const BlockGeometry geo = render_block_geometry(a);
  k.xcd_block_shift = geo.shift;
  k.xcd_blocks = (!(a->tuning & NFI_TUNING_SINGLE_WORK_COUNTER) && geo.ok) ? 1 : 0;
  // which block sits in which queue slot: the set-up's pairing of heavy and light blocks (tuning bit 5: in order)
  k.block_table = (k.xcd_blocks && !(a->tuning & NFI_TUNING_XCD_BLOCKS_IN_ORDER)) ? w.block_table : nullptr;
  const uint32_t bw = geo.bw, bh = geo.bh;
  // the scene of a ray: its image / views_per_scene (the images of a call are scene-major); hw * V <= rays of the call < 2^32
  k.div_scene_rays = make_fastdiv((uint32_t)k.hw * (uint32_t)std::max(a->views_per_scene, 1));
  k.div_bw = make_fastdiv(bw > 0 ? bw : 1u);
  k.div_bps = make_fastdiv(bw * bh > 0 ? bw * bh : 1u);
  k.tile_order = (!(a->tuning & NFI_TUNING_SCANLINE_ORDER) && (a->width % 8 == 0) && (a->height % 8 == 0)) ? 1 : 0;
  k.prof = (unsigned long long*)a->profile_cycles;
  k.xray = a->ray_features;
  k.clock_probe = reinterpret_cast<unsigned long long*>(a->clock_probe);
  k.term_eps = a->termination_eps;
  k.semantics = a->semantics; k.coords = a->coords; k.normals = a->normals;
  return k;
}

// One launch of a render kernel: which of the render_fwd* instantiations, and what its launch needs to know about it
using RenderKernel = void (*)(RenderKernelParams);
struct RenderLaunch {
  RenderKernel kernel;
  const char* name;                           // canonical name of the instantiation (nfi_render_kernel_name)
  int occ;                                    // workgroups of 4 waves per CU it is compiled for: the persistent grid is 256 CUs x occ
  size_t max_lds;                             // the largest dynamic LDS it is ever launched with (0: it uses none)
  int (*raise_lds)(size_t, const char*);      // ensure_dynamic_lds of this kernel
};
// one maker per kernel family: the kernel pointer and its name come from the SAME template arguments
static constexpr char kFwdFamily[] = "render_fwd_kernel", kWideFamily[] = "render_fwd_wide_kernel", kLongFamily[] = "render_fwd_long_kernel";
template <int TEX, bool ATT, int OCC, int MODE, int PREC, bool VD = false>
static RenderLaunch fwd_launch(size_t max_lds = 0) {
  constexpr auto kernel = &render_fwd_kernel<TEX, ATT, OCC, MODE, PREC, VD>;
  return {kernel, KernelName<kFwdFamily, TEX, ATT, OCC, MODE, PREC, VD>::value.s, OCC, max_lds, &ensure_dynamic_lds<kernel>};
}
template <int TEX, bool ATT, int MODE, int PREC, bool VD = false>
static RenderLaunch wide_launch(size_t max_lds = 0) {
  constexpr auto kernel = &render_fwd_wide_kernel<TEX, ATT, MODE, PREC, VD, NFI_RENDER_OCC>;
  return {kernel, KernelName<kWideFamily, TEX, ATT, MODE, PREC, VD, NFI_RENDER_OCC>::value.s, NFI_RENDER_OCC, max_lds, &ensure_dynamic_lds<kernel>};
}
template <int TEX, bool ATT, int PREC, bool VD = false>
static RenderLaunch long_launch() {
  constexpr auto kernel = &render_fwd_long_kernel<TEX, ATT, PREC, VD>;
  return {kernel, KernelName<kLongFamily, TEX, ATT, PREC, VD>::value.s, NFI_RENDER_OCC, 0, &ensure_dynamic_lds<kernel>};
}

// THE rule "which kernel does a (validated) render call get": first match wins.  Every condition that is a template
// argument is an `if constexpr`, so only kernels that some call can reach are instantiated.
static RenderLaunch select_render_kernel(const nfi_render_args* a, const RenderFlags& f) {
  const bool wide = a->n_samples > 64;
  const bool lng = a->n_samples > NFI_MAX_SAMPLES;     // single pass of up to 512 samples (no fine sampling: checked)
  const bool vd = a->ray_features != nullptr, normals = a->normals != nullptr, prof = a->profile_cycles != nullptr;
  // persistent 1-D grid: OCC blocks of 4 waves per CU
  // 2 blocks (8 waves) per CU: with the whole 256-VGPR budget the field tile keeps more loads and MFMA chains in
  // flight than at 3 blocks/CU (MI355X, 8 x 128^2: 0.96 vs 1.01-1.08 ms; 4 blocks/CU spill: 1.52 ms)
  constexpr int OCC = NFI_RENDER_OCC;
  // kRenderExtra / kRenderNormals: the per-wave semantics tables [A][pitch] and the normal operands in dynamic LDS
  constexpr size_t kSemLdsMax = ((size_t)4 * NFI_MAX_ATTENTION * kSemPitch + kNrmLdsFloats) * sizeof(float);
  constexpr size_t kSemLdsMaxWide = (size_t)4 * NFI_MAX_ATTENTION * kSemPitchWide * sizeof(unsigned short) + kNrmLdsFloats * sizeof(float);
  return dispatch_texel_att(a->texel_dtype, a->n_attention > 0, [&](auto tex, auto att) -> RenderLaunch {
    constexpr int TEX = decltype(tex)::value;
    constexpr bool ATT = decltype(att)::value;
    if (lng) {     // 128 < S <= 512: taps and stash are run-time switches of this kernel
      if (vd) return long_launch<TEX, ATT, 0, true>();
      if (f.strict) return long_launch<0, ATT, 0>();
      return long_launch<TEX, ATT, 1>();
    }
    if (vd) {      // the view-direction decoder runs in exact fp32 (PREC 0); its one kernel without maps has the taps, used or not
      if constexpr (TEX == 0) {      // the maps exist for fp32 texels (checked); the distance of the normals is row 0 of the second layer here too
        if (normals) return wide ? wide_launch<0, ATT, kRenderNormals, 0, true>(kSemLdsMaxWide)
                                 : fwd_launch<0, ATT, OCC, kRenderNormals, 0, true>(kSemLdsMax);
        if (f.extra) return wide ? wide_launch<0, ATT, kRenderExtra, 0, true>(kSemLdsMaxWide)
                                 : fwd_launch<0, ATT, OCC, kRenderExtra, 0, true>(kSemLdsMax);
      }
      return wide ? wide_launch<TEX, ATT, kRenderTaps, 0, true>()
                  : fwd_launch<TEX, ATT, OCC, kRenderTaps, 0, true>();
    }
    if (wide) {    // 64 < S <= 128 per pass
      if (normals) return wide_launch<TEX, ATT, kRenderNormals, 1>(kSemLdsMaxWide);
      if (f.extra) return wide_launch<TEX, ATT, kRenderExtra, 1>(kSemLdsMaxWide);
      if (f.term) return wide_launch<TEX, ATT, kRenderTerm, 1>();
      if (f.any_tap && f.strict) return wide_launch<0, ATT, kRenderTaps, 0>();
      if (f.any_tap) return wide_launch<TEX, ATT, kRenderTaps, 1>();
      if (f.strict) return wide_launch<0, ATT, kRenderPlain, 0>();
      // (fp16 texels, 128 + 128, at THREE workgroups per CU - 168 registers, ~40 scratch reloads per ray outside the field
      //  tiles - was measured in round 4 and is slower: 1.387 vs 1.300 ms chairs-like, 2.249 vs 2.156 ms every ray hits, images
      //  identical (profiles/r4/wide_fp16_three_workgroups.log); unlike the 64 + 64 kernel, whose fp16 form gains 8 % from the
      //  third workgroup, a 256-sample ray's texel footprint makes 50 % more rays in flight cost more in the L2 than they hide)
      return wide_launch<TEX, ATT, kRenderPlain, 1>();
    }
    if (normals) return fwd_launch<TEX, ATT, OCC, kRenderNormals, 1>(kSemLdsMax);
    if (f.extra) return fwd_launch<TEX, ATT, OCC, kRenderExtra, 1>(kSemLdsMax);
    if (f.term) return fwd_launch<TEX, ATT, OCC, kRenderTerm, 1>();
    if (prof) return fwd_launch<0, ATT, OCC, kRenderProf, 1>();
    if (f.any_tap && f.strict) return fwd_launch<0, ATT, OCC, kRenderTaps, 0>();
    if (f.any_tap) return fwd_launch<TEX, ATT, OCC, kRenderTaps, 1>();
    if (f.strict) return fwd_launch<0, ATT, OCC, kRenderPlain, 0>();
    // (16-bit texel storage, plain inference: the texels stay packed - 168 registers - and THREE blocks per CU fit without a
    //  spill: 0.705 vs 0.756 ms at 8 x 128^2, every ray hits 1.040 vs 1.174 ms)
    if constexpr (TEX != 0) return fwd_launch<TEX, ATT, 3, kRenderPlain, 1>();
    else return fwd_launch<TEX, ATT, OCC, kRenderPlain, 1>();
  });
}

// which kernel nfi_render_fwd launches for *a: the same rules, the same selector, no HIP call (nothing is dereferenced)
extern "C" const char* nfi_render_kernel_name(const nfi_render_args* a) {
  if (render_check_call(a)) return nullptr;
  const RenderFlags f = render_flags(a);
  if (render_check_variant(a, f)) return nullptr;
  return select_render_kernel(a, f).name;
}

extern "C" int nfi_render_fwd(const nfi_render_args* a, nfi_stream_t stream) {
  int rc = render_check_call(a);
  if (rc) return rc;
  RenderWorkspace w;
  rc = render_carve(a, w);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  REQUIRE(!(a->rays_ready && (a->ray_origins || a->ray_directions || a->hit || a->stash_t)),
          "render: rays_ready needs the ray set-up in the workspace (no ray_origins / ray_directions / hit taps, no stash)");
  if (!a->rays_ready) {
    rc = render_setup(a, w, s);
    if (rc) return rc;
  }
  const RenderFlags f = render_flags(a);
  rc = render_check_variant(a, f);
  if (rc) return rc;
  const RenderKernelParams k = render_kernel_params(a, w, f);
  const RenderLaunch launch = select_render_kernel(a, f);
  // kRenderExtra with semantics: the per-wave tables [A][pitch] in dynamic LDS; kRenderNormals: + the normal operands
  const size_t lds = (a->semantics ? (size_t)4 * a->n_attention * (a->n_samples > 64 ? kSemPitchWide * sizeof(unsigned short) : kSemPitch * sizeof(float)) : 0) +
                     (a->normals ? (size_t)kNrmLdsFloats * sizeof(float) : 0);
  if (launch.max_lds) {
    rc = launch.raise_lds(launch.max_lds, "render");
    if (rc) return rc;
  }
  // persistent grid: never more blocks than the rays need (4 per block: one wave per ray)
  const int64_t blocks = std::min<int64_t>((int64_t)256 * launch.occ, (w.n + 3) / 4);
  if (a->event_start) (void)hipEventRecord((hipEvent_t)a->event_start, s);
  hipLaunchKernelGGL(launch.kernel, dim3((unsigned)blocks), dim3(256), lds, s, k);
  if (a->event_stop) (void)hipEventRecord((hipEvent_t)a->event_stop, s);
  return check_launch("render_fwd");
}
