// nfi_render_kernels.inc — the fused forward render on the device: RenderKernelParams, the work queues (RayQueue), what
// the persistent kernels share around their per-ray pipelines, and the two hierarchical kernels - render_fwd_kernel (up to
// 64 + 64 samples per ray) and render_fwd_wide_kernel (up to 128 + 128) - each with its NFI_SINGLE_* instantiation
// (included by nfi_kernels.hip, which explains that frame).  Expects nfi_wave_slab.inc (resampling, merge, composite),
// nfi_rays.inc (finish_planes, stratified_depth), nfi_host.hpp and `using namespace nfi`.  The third kernel is
// nfi_render_long.inc; the host side of all three is nfi_render_host.inc.

// ------------------------------------------------------------------------------------------------
// fused forward render
// ------------------------------------------------------------------------------------------------
struct RenderKernelParams {
  int n_scenes, hw, S;
  int fine, white;
  float scene_range;
  // ray set-up results
  const float* ro; const float* rd; const float* near_raw; const float* far_raw; const uint8_t* hit;
  const uint32_t* reduce;
  uint32_t* counter;   // work counter (zeroed with reduce[])
  int width;           // image width (tile order of the work queue)
  int tile_order;      // 1: hand rays out in 8x8 pixel tiles instead of scanlines
  int xcd_blocks;      // 1: every XCD marches its own square pixel blocks (own queue, steals when it runs dry)
  uint32_t* xcd_counter;   // 8 counters, 64 bytes apart
  int xcd_block_shift;     // log2 of the block side: 3, 4 or 5
  int fetch_batch;         // positions taken per atomic
  const uint32_t* block_table;   // queue slot g = 8 * slot + q -> pixel block (the set-up's pairing by hit count); null: g
  // field
  const void* texels; int res; int layout;
  const float* image; int A; const float* att;
  int use_sdf; const float* beta; const float* alpha;
  // noise
  const float* noise_c; const float* noise_f; int64_t noise_f_stride;
  // outputs
  float* rgb; float* depth; float* mask;
  // taps
  float* near_plane; float* far_plane;
  float* t_coarse; float* sigma_coarse; float* rgb_coarse;
  float* t_fine; float* sigma_fine; float* rgb_fine;
  float* t_sorted; float* weights; int32_t* perm;
  int skip_missed;
  unsigned long long* prof;
  const float* xray;   // view-direction decoder: padded per-ray features [N][kRayFeatPad], or null
  float term_eps;      // kRenderTerm kernels: coarse transmittance below which fine samples are no longer evaluated
  float* semantics;    // kRenderExtra kernels: composited softmax probabilities [N][A], or null
  float* coords;       // kRenderExtra kernels: composited query points [N][3], or null
  float* normals;      // kRenderNormals kernels: composited unit normals [N][3]
  unsigned long long* clock_probe;   // null, or {shader cycles, 100 MHz ticks} lived by workgroup 0 / wave 0
  FastDiv div_scene_rays, div_bps, div_bw;   // division by rays per scene (rays per image x views per scene), blocks per image, blocks per image row (nfi_device.hpp)
  int tap_stride;      // entries per ray in the per-sample tap arrays: S, or 2S for the training stash (fine half at +S)
  int stash;           // 1: the taps are the training stash: missed rays keep being skipped and get an all-zero row
};

// start / end of the clock probe (nfi_render_args.clock_probe): one wave of the persistent grid lives as long as the launch
struct ClockProbe {
  unsigned long long c0 = 0, r0 = 0;
  bool on = false;
  __device__ __forceinline__ void start(const RenderKernelParams& k) {
    on = k.clock_probe && blockIdx.x == 0 && threadIdx.x == 0;
    if (on) { c0 = __builtin_readcyclecounter(); r0 = __builtin_amdgcn_s_memrealtime(); }
  }
  __device__ __forceinline__ void stop(const RenderKernelParams& k) const {
    if (on) {
      k.clock_probe[0] = __builtin_readcyclecounter() - c0;
      k.clock_probe[1] = __builtin_amdgcn_s_memrealtime() - r0;
    }
  }
};

// The kernel's argument block, read again where it is used.  Every argument the compiler keeps live through the ray loop is
// a scalar register (two for a pointer) of a kernel that has none to spare: the plain S <= 64 kernel held 121 of them in
// lanes of two vector registers and fetched them back with v_readlane - vector instructions, ~190 per marched ray, for
// values that never change.  A scalar load from the argument segment (which a kernel's only by-value parameter starts)
// costs the vector pipe nothing and the scalar cache always has the line.  The pointer is opaque to the compiler, or it
// would hoist the loads back out of the loop; call this AT the use, once per group of loads that may wait together.
typedef __attribute__((address_space(4))) const RenderKernelParams RenderKernelArgs;
__device__ __forceinline__ RenderKernelArgs* kernel_args_here() {
  auto* p = reinterpret_cast<RenderKernelArgs*>(reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr()));
  asm volatile("" : "+s"(p));
  return p;
}

__device__ __forceinline__ float uniform_f32(float v) {
  return bits2f((uint32_t)__builtin_amdgcn_readfirstlane((int)f2bits(v)));
}

// one ray's inputs, as render_fwd_kernel loads them one ray ahead
struct RayInputs {
  float ox, oy, oz, dx, dy, dz, near, far, noise, u;
  uint32_t hit;
};

// Work hand-out of the persistent render kernels.  One device-scope counter for all waves serialises at ~12 ns per
// fetch on this chip (131 k rays -> 1.6 ms: with it the counter, not the field, set the kernel time), so every XCD
// has its own counter, served by its own L2: the image is cut into square pixel blocks, block b belongs to XCD b % 8
// (all XCDs stay on the same scene), positions inside a block walk 8x8 sub-tiles, and an XCD that runs dry steals
// from the next one's queue.  fetch() is wave-uniform and returns a RAY ID (n_rays: no work left); without the
// per-XCD queues (image sides not multiples of the block side, or tuning bit 4) it returns a position of the single
// queue, which ray_of() maps to a ray.
// WHICH block sits in slot g = 8 * slot + q of the queues is the set-up's block table (raygen_finish_kernel: every
// aligned group of 16 slots permuted so that each XCD gets a heavy and a light block by hit count; null or tuning bit 5:
// block g).  The entry is wave-uniform and changes once per block: (tab_g, tab_b) keep the last look-up.  A look-up
// behind the claim's atomic would be a second dependent round trip every fourth ray (256 waves x 2 positions turn a block
// over in two rounds), so the entry of the queue's NEXT block (nxt_g = tab_g + 8) is loaded in front of the atomic, by a
// scalar load that is under way together with it; only a claim that lands elsewhere (a steal, a block skipped) loads
// behind it.
struct RayQueue {
  const RenderKernelParams& k;
  int lane;
  uint32_t n_rays, xcd, bsh, bw, bps, n_blocks, q_cur, pos_next, pos_end, batch, tiles_x;
  uint32_t tab_g, tab_b = 0u, nxt_g = 0xffffffffu, nxt_b = 0u;
  bool dry;
  __device__ __forceinline__ RayQueue(const RenderKernelParams& kk, int l) : k(kk), lane(l) {
    n_rays = (uint32_t)k.n_scenes * (uint32_t)k.hw;
    xcd = k.xcd_blocks ? (__builtin_amdgcn_s_getreg(6164) & 7u) : 0u;     // hwreg(HW_REG_XCC_ID, 0, 4)
    bsh = (uint32_t)k.xcd_block_shift;                                   // log2 of the block side (3..5)
    bw = (uint32_t)k.width >> bsh;
    bps = bw * (((uint32_t)k.hw / (uint32_t)k.width) >> bsh);
    n_blocks = bps * (uint32_t)k.n_scenes;
    q_cur = xcd; pos_next = 0; pos_end = 0; dry = false;
    tab_g = xcd - 8u;                    // no entry yet; the first prefetch is for block `xcd`, the wave's first
    batch = (uint32_t)k.fetch_batch;
    tiles_x = (uint32_t)k.width >> 3;
  }
  // The table lists an XCD's pair of a complete group heavy block first (entries 16 G + x and 16 G + 8 + x); the queues
  // take the LIGHT one first (g ^ 8): a launch then ends on heavy blocks, which keep every wave of the XCD busy to the
  // end, and not on a few hits among misses (measured: profiles/r18, 9-20 us per launch whatever its size).
  __device__ __forceinline__ uint32_t table_entry(uint32_t g) const {         // g < n_blocks
    typedef __attribute__((address_space(4))) const uint32_t const_u32;       // written by the set-up, never by this kernel
    const uint32_t e = (g | 15u) < n_blocks ? g ^ 8u : g;                     // (an incomplete last group is the identity)
    return *reinterpret_cast<const_u32*>(reinterpret_cast<uintptr_t>(k.block_table) + (uintptr_t)e * 4u);
  }
  // in front of a claim's atomic / behind its issue: start the load of the next block's entry / keep it in front of the
  // atomic's wait (the compiler would sink the load to its use, behind that wait)
  __device__ __forceinline__ void table_prefetch() {
    if (!k.block_table) return;
    const uint32_t g = tab_g + 8u;
    if (g < n_blocks && g != nxt_g) { nxt_g = g; nxt_b = table_entry(g); }
  }
  __device__ __forceinline__ void table_pin() {
    if (k.block_table) asm volatile("" : "+s"(nxt_b));
  }
  __device__ __forceinline__ uint32_t block_at(uint32_t g) {
    if (!k.block_table) return g;
    if (g != tab_g) {        // g < n_blocks: fetch() / claim_finish() test it before they take a claim over
      tab_b = g == nxt_g ? nxt_b : table_entry(g);
      tab_g = g;
    }
    return tab_b;
  }
  __device__ __forceinline__ uint32_t ray_at(uint32_t q, uint32_t pos) {
    // (readfirstlane: q and pos are uniform by construction only; see hit_bytes_scalar)
    const uint32_t b = block_at((uint32_t)__builtin_amdgcn_readfirstlane((int)((pos >> (2 * bsh)) * 8u + q)));
    const uint32_t in = pos & ((1u << (2 * bsh)) - 1u), scene = fastdiv(b, k.div_bps), bb = b - scene * bps;
    const uint32_t by = fastdiv(bb, k.div_bw), bx = bb - by * bw;
    const uint32_t st = in >> 6, sty = st >> (bsh - 3), stx = st & ((1u << (bsh - 3)) - 1u);   // 8x8 sub-tile of the block
    const uint32_t y = (by << bsh) + (sty << 3) + ((in >> 3) & 7u), x = (bx << bsh) + (stx << 3) + (in & 7u);
    return scene * (uint32_t)k.hw + y * (uint32_t)k.width + x;
  }
  __device__ __forceinline__ uint32_t fetch() {
    if (!k.xcd_blocks) {
      uint32_t p = 0;
      if (lane == 0) p = atomicAdd(k.counter, 1u);
      return (uint32_t)__builtin_amdgcn_readfirstlane((int)p);
    }
    if (pos_next == pos_end && !dry) {
      dry = true;
      table_prefetch();
      for (uint32_t i = 0; i < 8; ++i) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(k.xcd_counter + q_cur * 16, batch);
        if (i == 0) table_pin();
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if ((base >> (2 * bsh)) * 8u + q_cur < n_blocks) { pos_next = base; pos_end = base + batch; dry = false; break; }
        q_cur = (q_cur + 1) & 7u;        // this queue is empty: steal from the next XCD's
      }
    }
    if (dry) return n_rays;
    return ray_at(q_cur, pos_next++);
  }
  // fetch() in two halves, for a caller that has something to do while the atomic is under way (skip_miss_run):
  // positions already claimed are handed out first and claimed() says whether there are any; claim_issue() starts the
  // atomic if the next fetch() would start with one and returns its raw per-lane result; claim_finish() takes the claim
  // over and is fetch().  The counter's offset goes through an opaque vector register: on a wave-uniform address the
  // atomic optimiser rewrites the add so that its result is read back on the spot.
  __device__ __forceinline__ bool claimed() const { return pos_next != pos_end; }
  __device__ __forceinline__ uint32_t take() { return ray_at(q_cur, pos_next++); }      // only if claimed()
  __device__ __forceinline__ uint32_t claim_issue() {
    uint32_t raw = 0, off = k.xcd_blocks ? q_cur * 16 : 0;
    asm volatile("" : "+v"(off));
    if (k.xcd_blocks && (claimed() || dry)) return raw;
    table_prefetch();
    if (lane == 0) raw = atomicAdd((k.xcd_blocks ? k.xcd_counter : k.counter) + off, k.xcd_blocks ? batch : 1u);
    table_pin();
    return raw;
  }
  __device__ __forceinline__ uint32_t claim_finish(uint32_t raw) {
    const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)raw);
    if (!k.xcd_blocks) return base;
    if (!claimed() && !dry) {
      if ((base >> (2 * bsh)) * 8u + q_cur < n_blocks) { pos_next = base; pos_end = base + batch; }
      else q_cur = (q_cur + 1) & 7u;     // this queue is empty: fetch() goes stealing, from the next XCD's on
    }
    return fetch();
  }
  // position of the single queue -> ray id.  Tile order: consecutive positions walk 8x8 pixel tiles, so the few thousand
  // rays in flight at any time cover a compact image region (a compact part of the three planes) instead of a band of
  // scanlines - better L2/Infinity-Cache reuse of the gather stream.  (A ray id of the per-XCD queues passes through.)
  __device__ __forceinline__ uint32_t ray_of(uint32_t pos) const {
    if (k.xcd_blocks || !k.tile_order) return pos;
    const uint32_t scene = pos / (uint32_t)k.hw, p = pos - scene * (uint32_t)k.hw;
    const uint32_t tile = p >> 6, in = p & 63u;
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    return scene * (uint32_t)k.hw + ((ty << 3) + (in >> 3)) * (uint32_t)k.width + (tx << 3) + (in & 7u);
  }
};

// Variants of the persistent render kernels (one template argument; they exclude each other):
//   kRenderPlain  rgb / depth / mask only - the inference kernel
//   kRenderTaps   + the optional stage taps or the training stash
//   kRenderProf   + per-phase cycle counters (S <= 64)
//   kRenderTerm   ray termination in the FINE pass (nfi_render_args.termination_eps): the coarse pass, hence the pdf and
//                 every sample index, is untouched; fine samples that lie behind the first coarse sample in front of
//                 which the coarse transmittance has fallen below eps are not evaluated (sigma = 0; they stay in the
//                 merge with their depth) and the surviving ones are compacted to the low lanes (wave ballot +
//                 popcount) so that whole 16-point tiles drop out
//   kRenderExtra  + the composited per-sample attributes of run.py:312-338 / lib/nerf_utils.py:147-159: `semantics`
//                 (softmax probabilities, parked per sample in a per-wave LDS table [A][pitch] by the field epilogue and
//                 composited with the merged weights brought back to source order) and `coords` (the query point
//                 o + d t of every merged sample)
//   kRenderNormals  kRenderExtra + the composited `normals` map (SDF only; lib/nerf_utils.py:149-151, 159): every sample's
//                 normalize(d sdf / d x) from the analytic derivative of the decoder (field_wave<..., NRM>), composited
//                 with the merged weights in source order like the semantics
constexpr int kRenderPlain = 0, kRenderTaps = 1, kRenderProf = 2, kRenderTerm = 3, kRenderExtra = 4, kRenderNormals = 5;
constexpr int kSemPitch = 2 * 64 + 4;                 // pitch = 4 (mod 64) dwords: conflict-free stores from the MFMA layout
// the 128 + 128 kernel parks the probabilities as unorm16 (tile_epilogue<SEMP < 0>): 41.6 KB of fp32 tables left room for ONE
// workgroup per CU next to the 47 KB of slabs and operands; 21 KB let two in (cfg5 + semantics 0.59 -> see DESIGN 4.2a).
// Pitch in 16-bit entries: 4 rows = 528 dwords = 16 (mod 64), the four row groups' stores fall into different banks
constexpr int kSemPitchWide = 2 * 128 + 8;
// dynamic LDS of the kRenderExtra / kRenderNormals kernels: [normal operands: kNrmLdsFloats, kRenderNormals only]
// [semantics tables: 4 waves x A x pitch floats, when asked for]
extern __shared__ __attribute__((aligned(16))) float nfi_dyn_lds[];

typedef __attribute__((address_space(3))) float lds_float;

// sum_e w_e (o + d t_e) over the merged samples (coords = x_in of the sampler, generator.py:643; run.py:337 puts it in the
// semantics slot of render_volume_density)
template <int NS, class Slab>
__device__ __forceinline__ void composite_coords(const Slab& slab, const float (&w)[NS], int n, int lane, float ox, float oy,
                                                 float oz, float dx, float dy, float dz, float* out3) {
  float cx = 0.0f, cy = 0.0f, cz = 0.0f;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int e = j * 64 + lane;
    if (e < n) {
      const float t = slab.srt[0][e];
      cx += w[j] * (ox + dx * t); cy += w[j] * (oy + dy * t); cz += w[j] * (oz + dz * t);
    }
  }
  cx = wave_sum(cx); cy = wave_sum(cy); cz = wave_sum(cz);
  if (lane == 0) { out3[0] = cx; out3[1] = cy; out3[2] = cz; }
}

// ---- what the three persistent render kernels share around their per-ray pipelines ----

// decoder image -> LDS: the fp32 fragments, or (PREC == 1) the fp16 fragments overlaying the fp32 fragment area with the
// biases staying where they are; ends with the workgroup barrier
template <int PREC, int kImg>
__device__ __forceinline__ void stage_decoder_image(float* lds, const float* image) {
  if (PREC == 1) {
    for (int i = threadIdx.x; i < kB1F; i += blockDim.x) lds[i] = image[kW1H + i];
    for (int i = kB1F + threadIdx.x; i < kLdsImageFloats; i += blockDim.x) lds[i] = image[i];
  } else {
    for (int i = threadIdx.x; i < kImg; i += blockDim.x) lds[i] = image[i];
  }
  __syncthreads();
}

// a wave moves on to another scene: the scene's texel buffer descriptor, and its attention rows into the wave's vf
template <int TEX>
__device__ __forceinline__ void enter_scene(FieldParams& P, const RenderKernelParams& k, float* vf, int scene, int lane) {
  const size_t tb = TEX == 0 ? 128 : 64;
  const char* tex_scene = reinterpret_cast<const char*>(k.texels) + (size_t)scene * 3 * k.res * k.res * tb;
  P.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(tex_scene), 0, (int)P.scene_bytes, 0x00020000);
  wave_lds_fence();
  {
    int c = lane & 3, row = lane >> 2;
    float v = 0.0f;
    if (k.att && c < 3 && row >= 1 && row <= k.A) v = k.att[((size_t)scene * k.A + (row - 1)) * 3 + c];
    vf[lane] = v;
  }
  wave_lds_fence();
}

// a ray's five results (the caller picks the lane, and the place: see the work fetch of render_fwd_kernel)
// (K: RenderKernelParams, or RenderKernelArgs - the three pointers re-read from the argument segment)
template <class K>
__device__ __forceinline__ void store_pixel(const K& k, uint32_t ray, float r, float g, float b, float depth,
                                            float mask) {
  k.rgb[(size_t)ray * 3] = r; k.rgb[(size_t)ray * 3 + 1] = g; k.rgb[(size_t)ray * 3 + 2] = b;
  k.depth[ray] = depth; k.mask[ray] = mask;
}

// one sample's entry of the optional per-sample taps (coarse or fine; entry i of the ray-major arrays)
__device__ __forceinline__ void store_sample_tap(float* t_out, float* sigma_out, float* rgb_out, size_t i, float t, float sigma,
                                                 float r, float g, float b) {
  if (t_out) t_out[i] = t;
  if (sigma_out) sigma_out[i] = sigma;
  if (rgb_out) { float* q = rgb_out + i * 3; q[0] = r; q[1] = g; q[2] = b; }
}

// the composite weights and the depths in merged order: n entries per ray, element e = slot * 64 + lane
template <int NS, class Slab>
__device__ __forceinline__ void store_sorted_taps(const RenderKernelParams& k, const Slab& slab, const float (&w)[NS], uint32_t ray,
                                                  int n, int lane) {
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int e = j * 64 + lane;
    if (e < n) {
      if (k.weights) k.weights[(size_t)ray * n + e] = w[j];
      if (k.t_sorted) k.t_sorted[(size_t)ray * n + e] = slab.srt[0][e];
    }
  }
}

// kRenderExtra / kRenderNormals, a ray whose line stays outside the scene cube: its composited attribute maps
template <bool NRM>
__device__ __forceinline__ void zero_missed_maps(const RenderKernelParams& k, uint32_t ray, int lane, float bg) {
  if (k.coords && lane < 3) k.coords[(size_t)ray * 3 + lane] = 0.0f;
  if (k.semantics && lane < k.A) k.semantics[(size_t)ray * k.A + lane] = 0.0f;
  if (NRM && lane < 3) k.normals[(size_t)ray * 3 + lane] = bg;      // sum w n + (1 - mask) on a white background
}

// training stash, a ray whose line stays outside the scene cube: an all-zero row - its composite backward is exactly
// zero and its points (the ray origin) carry no gradient
__device__ __forceinline__ void zero_stash_row(const RenderKernelParams& k, uint32_t ray, int S, int lane) {
  for (int e = lane; e < S; e += 64) {
    const size_t zs = (size_t)ray * (size_t)k.tap_stride + e;
    k.t_coarse[zs] = 0.0f; k.sigma_coarse[zs] = 0.0f;
    float* q = k.rgb_coarse + zs * 3; q[0] = 0.0f; q[1] = 0.0f; q[2] = 0.0f;
    if (k.fine) {
      k.t_fine[zs] = 0.0f; k.sigma_fine[zs] = 0.0f;
      q = k.rgb_fine + zs * 3; q[0] = 0.0f; q[1] = 0.0f; q[2] = 0.0f;
    }
  }
}

// everything a ray gets whose line stays outside the (inflated) scene cube: every sample has sigma == 0
template <bool EXTRA, bool NRM, bool TAPS>
__device__ __forceinline__ void put_missed_ray(const RenderKernelParams& k, uint32_t ray, int S, int lane, float bg) {
  if (lane == 0) store_pixel(k, ray, bg, bg, bg, 0.0f, 0.0f);
  if constexpr (EXTRA) zero_missed_maps<NRM>(k, ray, lane, bg);
  if constexpr (TAPS) {
    if (k.stash) zero_stash_row(k, ray, S, lane);
  }
}

// The hit bytes of two rays through the scalar data path (the dwords that hold them, through a constant-address-space
// view: the array is written by an earlier kernel and never by this one): ONE wait, and on lgkmcnt - not behind every
// store the wave has in flight on the in-order vmcnt.  Both rays are wave-uniform.  Returns hit[ra] | hit[rb] << 8.
__device__ __forceinline__ uint32_t hit_bytes_scalar(const RenderKernelParams& k, uint32_t ra, uint32_t rb) {
  typedef __attribute__((address_space(4))) const uint32_t const_u32;
  // (readfirstlane: where the compiler takes the ray index for divergent, the loads would become vector loads)
  const uintptr_t pa = reinterpret_cast<uintptr_t>(k.hit) + (uint32_t)__builtin_amdgcn_readfirstlane((int)ra),
                  pb = reinterpret_cast<uintptr_t>(k.hit) + (uint32_t)__builtin_amdgcn_readfirstlane((int)rb);
  uint32_t wa = *reinterpret_cast<const_u32*>(pa & ~(uintptr_t)3), wb = *reinterpret_cast<const_u32*>(pb & ~(uintptr_t)3);
  asm volatile("" : "+s"(wa), "+s"(wb));       // both loads in front of the one wait: the compiler would sink the second
  return ((wa >> ((uint32_t)(pa & 3) * 8u)) & 0xffu) | (((wb >> ((uint32_t)(pb & 3) * 8u)) & 0xffu) << 8);
}

// A run of missed rays.  Misses come in runs (the corners and edges of the pixel blocks), in which all waves of an XCD
// turn over positions at once and nothing hides what a turn waits for - so a turn here is as little as a missed ray
// needs: its hit byte.  Called with `cur` known to miss and `nxt` the position behind it, as yet untouched.  The
// positions this wave has claimed (at most two at fetch_batch = 2) are tested behind ONE wait; if they all miss, the next
// claim's atomic goes out before their background values are stored - nothing else of this wave is in flight then - and
// the loop turns on the new pair.  The wave never holds more positions than render_fwd_kernel's pipeline does, and it
// takes them in the same order.  Returns with `cur` the first position that hits, its inputs being loaded by `load`
// (one exposed input latency per run), and `nxt` the position behind it - or with both >= n_rays: no work left.
template <bool EXTRA, bool NRM, bool TAPS, class Load>
__device__ __forceinline__ void skip_miss_run(RayQueue& queue, const RenderKernelParams& k, int S, int lane, float bg,
                                              uint32_t& cur, uint32_t& nxt, Load&& load) {
  put_missed_ray<EXTRA, NRM, TAPS>(k, queue.ray_of(cur), S, lane, bg);
  uint32_t a = nxt;
  while (a < queue.n_rays) {
    const bool two = queue.claimed();
    const uint32_t b = two ? queue.take() : a;
    const uint32_t ra = queue.ray_of(a), rb = queue.ray_of(b);
    const uint32_t hits = hit_bytes_scalar(k, ra, rb);
    uint32_t claim;
    bool ends = true;
    if (hits & 2u) {
      cur = a; load(ra);
      if (two) { nxt = b; return; }
      claim = queue.claim_issue();
    } else if (two && (hits & 0x200u)) {
      put_missed_ray<EXTRA, NRM, TAPS>(k, ra, S, lane, bg);
      cur = b; load(rb);
      claim = queue.claim_issue();
    } else {
      claim = queue.claim_issue();
      put_missed_ray<EXTRA, NRM, TAPS>(k, ra, S, lane, bg);
      if (two) put_missed_ray<EXTRA, NRM, TAPS>(k, rb, S, lane, bg);
      ends = false;
    }
    const uint32_t got = queue.claim_finish(claim);       // (the one place of this helper that fetch()'s code is at)
    if (ends) { nxt = got; return; }
    a = got;
  }
  cur = nxt = a;
}

// Persistent kernel, S <= 64 samples per pass: one wave per ray, rays handed out by a RayQueue (scene-major, so the chip
// works on one scene's 25 MB of texels at a time).  The ray index two steps ahead is being fetched and the next ray's
// inputs are loaded (RayInputs) while the current ray is marched.
// OCC = waves per SIMD the register budget is held to; MODE = one of the kRender... variants above.
template <int TEX, bool ATT, int OCC, int MODE, int PREC, bool VD = false>
__global__ __launch_bounds__(256, OCC) void render_fwd_kernel(RenderKernelParams k) {
  constexpr bool TAPS = MODE == kRenderTaps, PROF = MODE == kRenderProf, TERM = MODE == kRenderTerm;
  constexpr bool EXTRA = MODE == kRenderExtra || MODE == kRenderNormals, NRM = MODE == kRenderNormals;
  constexpr int SEMP = (EXTRA && ATT) ? kSemPitch : 0;
  constexpr int kImg = VD ? kVdImageFloats : kLdsImageFloats;
  __shared__ __attribute__((aligned(16))) float lds[kImg];
  __shared__ __attribute__((aligned(16))) float vfs[4][64];
  __shared__ WaveSlab slabs[4];
  // Decoder output tables (field_wave): the slab's rows are free during the field passes, but the 464 floats beside the
  // stage tile do not hold one - static LDS, 30 272 + 17 408 B: three workgroups per CU still fit in 160 KB.  The PLAIN
  // kernels with attention only: they are the ones timed with it (profiles/r13); every other form keeps the per-tile
  // epilogue - and the normal map's kernel (47 680 + 29 568 of semantics tables + 8 464 of normal operands = 85 712 B) and
  // the view-direction decoder's map kernels (59 136 + 29 568 B) would lose their second workgroup per CU with a table.
  constexpr bool OTAB = MODE == kRenderPlain && ATT && !VD;
  __shared__ __attribute__((aligned(16))) float otabs[4][OTAB ? kOutTabFloats<ATT> : 4];
  if constexpr (NRM) stage_normal_operands(nfi_dyn_lds, k.image, VD ? kVdW1F : kW1F, VD ? kVdW2 : kW2F);
  ClockProbe clock;
  clock.start(k);
  stage_decoder_image<PREC, kImg>(lds, k.image);
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  WaveSlab& slab = slabs[wave];
  float* vf = vfs[wave];
  float* otab = otabs[wave];
  const int S = k.S;
  const bool valid = lane < S;
  const float fill_near = ordered_key_inv(~k.reduce[0]), fill_far = ordered_key_inv(k.reduce[1]);
  const float bg = k.white ? 1.0f : 0.0f;
  const uint32_t n_rays = (uint32_t)k.n_scenes * (uint32_t)k.hw;

  FieldParams P = make_field_params(k.texels, k.res, TEX, k.A, k.use_sdf, k.beta, k.alpha, lds, kImg, k.layout);
  P.vf = vf;
  P.w1t = nfi_dyn_lds; P.w2r0 = nfi_dyn_lds + kW1TFloats;       // (kRenderNormals only)
  int cur_scene = -1;

  // kRenderExtra: this wave's semantics table [A][kSemPitch]: column = sample (coarse [0,64), fine [64,128)).  Zeroed once:
  // a tile the field skips (all 16 points outside the cube) leaves an earlier ray's probabilities behind, and those meet
  // weights that are exactly 0 - finite stale values are harmless, uninitialised LDS would not be.
  float* semT = nullptr;
  if constexpr (SEMP > 0) {
    if (k.semantics) {
      semT = nfi_dyn_lds + (NRM ? kNrmLdsFloats : 0) + wave * (k.A * kSemPitch);
      for (int i = lane; i < k.A * kSemPitch; i += 64) ((lds_float*)semT)[i] = 0.0f;
      wave_lds_fence();
    }
  }

  // (the seven pointers, S, `fine` and the stride from the argument segment - see kernel_args_here.  together: all through
  //  one empty asm, so that the scalar loads go out in front of ONE wait - the ray loop's load, once per marched ray.  Not
  //  for the loads of skip_miss_run, one per run of misses: in its three branches the asm's outputs meet values that do not
  //  exist, which the compiler fills in with v_readfirstlane of nothing)
  auto load_inputs = [&](uint32_t ray, RayInputs& in, auto together) {
    RenderKernelArgs& a = *kernel_args_here();
    const uint8_t* hit = a.hit;
    const float *ro = a.ro, *rd = a.rd, *near_raw = a.near_raw, *far_raw = a.far_raw, *noise_c = a.noise_c, *noise_f = a.noise_f;
    int64_t noise_f_stride = a.noise_f_stride;
    int n_samples = a.S, fine = a.fine;
    if constexpr (decltype(together)::value)
      asm volatile("" : "+s"(hit), "+s"(ro), "+s"(rd), "+s"(near_raw), "+s"(far_raw), "+s"(noise_c), "+s"(noise_f),
                        "+s"(noise_f_stride), "+s"(n_samples), "+s"(fine));
    const size_t r3 = (size_t)ray * 3;
    const bool has = lane < n_samples;
    in.hit = hit[ray];
    in.ox = ro[r3]; in.oy = ro[r3 + 1]; in.oz = ro[r3 + 2];
    in.dx = rd[r3]; in.dy = rd[r3 + 1]; in.dz = rd[r3 + 2];
    in.near = near_raw[ray]; in.far = far_raw[ray];
    in.noise = (noise_c && has) ? noise_c[(size_t)ray * n_samples + lane] : 0.0f;
    in.u = (fine && has) ? noise_f[(size_t)ray * noise_f_stride + lane] : 0.0f;
  };

  // ray indices: cur (being marched), nxt (inputs being loaded), and one more in flight
  RayQueue queue(k, lane);
  auto fetch = [&]() -> uint32_t { return queue.fetch(); };
  uint32_t cur = fetch(), nxt = fetch(), fly = 0;
  RayInputs in, pre;
  // PROF: per-wave cycle accumulators [0..3] field tiles (see field_wave), [4] ray set-up, [5] coarse field,
  // [6] resample, [7] fine field, [8] merge, [9] composite + store, [10] rays, [11] total
  unsigned long long pc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tk0 = PROF ? __builtin_readcyclecounter() : 0;
  if (cur < n_rays) load_inputs(queue.ray_of(cur), in, std::false_type());
  // A ray that misses the cube never enters the loop below: it and the missed ones behind it are dealt with here, before
  // the first ray and behind every marched one, and `in` is loaded afresh for the ray that ends the run.  (Behind the
  // loop's turn and not in front of it: a second way back to the loop's head cost 14-23 vector registers.  The hit byte
  // through a scalar register: this branch writes the queue's wave-uniform state, and under a condition that sits in a
  // vector register the compiler moves that state, the ray index and with it the texel descriptor to vector registers.)
  auto skip_run = [&]() {
    if (k.skip_missed && cur < n_rays && !((uint32_t)__builtin_amdgcn_readfirstlane((int)in.hit) & 2))
      skip_miss_run<EXTRA, NRM, TAPS>(queue, k, S, lane, bg, cur, nxt, [&](uint32_t r) { load_inputs(r, in, std::false_type()); });
  };
  skip_run();
  while (cur < n_rays) {
    if (nxt < n_rays) load_inputs(queue.ray_of(nxt), pre, std::true_type());
    const uint32_t ray = queue.ray_of(cur);
    const uint32_t hitb = in.hit;
    // the ray's five results: stored after the work fetch at the end of the iteration (see there)
    float out_r = bg, out_g = bg, out_b = bg, out_d = 0.0f, out_m = 0.0f;
    unsigned long long t0 = PROF ? __builtin_readcyclecounter() : 0;
    // (the divisor's words: a struct in the constant address space does not copy into fastdiv's by-value parameter)
    RenderKernelArgs& ka = *kernel_args_here();
    const int scene = (int)fastdiv(ray, FastDiv{ka.div_scene_rays.mul, ka.div_scene_rays.shift});
    if (scene != cur_scene) {
      cur_scene = scene;
      enter_scene<TEX>(P, k, vf, scene, lane);
    }
    const float ox = in.ox, oy = in.oy, oz = in.oz, dx = in.dx, dy = in.dy, dz = in.dz;
    float near = in.near, far = in.far;
    finish_planes((hitb & 1) != 0, fill_near, fill_far, near, far);
    const float dnorm = norm3(dx, dy, dz);
    const size_t rs = (size_t)ray * (size_t)k.tap_stride;      // row of this ray in the per-sample tap / stash arrays

    // ---- coarse pass ----
    float tc = 0.0f;
    if (valid) tc = stratified_depth(near, far, lane, S, in.noise, kernel_args_here()->noise_c != nullptr);
    MergeIn c;
    float ncx = 0.0f, ncy = 0.0f, ncz = 0.0f, nfx = 0.0f, nfy = 0.0f, nfz = 0.0f;     // NRM: the samples' unit normals
    unsigned long long t1 = PROF ? __builtin_readcyclecounter() : 0;
    {
      SampleOut q = field_wave<TEX, ATT, true, PREC, VD, SEMP, NRM, OTAB>(P, k.scene_range, lane, ox + dx * tc, oy + dy * tc, oz + dz * tc,
                                                                    valid, semT, nullptr, &slab.srt[0][0], otab, PROF ? pc : nullptr,
                                                                    k.xray, (int)ray);
      c.t = tc; c.sigma = q.sigma; c.r = q.r; c.g = q.g; c.b = q.b;
      if constexpr (NRM) { ncx = q.nx; ncy = q.ny; ncz = q.nz; }
    }
    int n = S;
    int rank_c = lane, rank_f = 0;
    unsigned long long t2 = PROF ? __builtin_readcyclecounter() : 0, t3 = t2, t4 = t2, t5 = t2;
    if (k.fine) {
      // ---- hierarchical resampling + fine pass ----
      ResampleTaps rt;
      float tf = resample_ray(slab, c.sigma, tc, scalar_here(S), dnorm, in.u, lane, TERM ? &rt : nullptr);
      MergeIn f;
      if (PROF) { asm volatile("" :: "v"(tf)); t3 = __builtin_readcyclecounter(); }
      if constexpr (TERM) {
        // depth of the first coarse sample in front of which the coarse transmittance is already below eps
        const uint64_t dm = __ballot(valid && rt.T < k.term_eps);
        float t_dead = INFINITY;
        if (dm) t_dead = bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(tc), (int)__builtin_ctzll(dm)));
        // compaction: live fine samples to the low lanes, dropped ones behind them (they keep their depth)
        const bool live = valid && tf <= t_dead;
        const uint64_t lm = __ballot(live);
        const int nl = __builtin_popcountll(lm);
        const int nb = __builtin_popcountll(lm & ((1ull << lane) - 1ull));
        const int pos = live ? nb : nl + (lane - nb);
        wave_lds_fence();
        slab.cdf[pos] = tf;
        wave_lds_fence();
        tf = slab.cdf[lane];
        wave_lds_fence();
        const bool vl = lane < nl;
        SampleOut q = field_wave<TEX, ATT, true, PREC, VD, 0, false, OTAB>(P, k.scene_range, lane, ox + dx * tf, oy + dy * tf,
                                                                           oz + dz * tf, vl, nullptr, nullptr, &slab.srt[0][0],
                                                                           otab, nullptr, k.xray, (int)ray);
        f.t = tf; f.sigma = vl ? q.sigma : 0.0f; f.r = vl ? q.r : 0.0f; f.g = vl ? q.g : 0.0f; f.b = vl ? q.b : 0.0f;
      } else {
        SampleOut q = field_wave<TEX, ATT, true, PREC, VD, SEMP, NRM, OTAB>(P, k.scene_range, lane, ox + dx * tf, oy + dy * tf, oz + dz * tf,
                                                                      valid, semT ? semT + 64 : nullptr, nullptr, &slab.srt[0][0],
                                                                      otab, PROF ? pc : nullptr, k.xray, (int)ray);
        f.t = tf; f.sigma = q.sigma; f.r = q.r; f.g = q.g; f.b = q.b;
        if constexpr (NRM) { nfx = q.nx; nfy = q.ny; nfz = q.nz; }
      }
      if constexpr (TAPS) {
        if (valid) store_sample_tap(k.t_fine, k.sigma_fine, k.rgb_fine, rs + lane, tf, f.sigma, f.r, f.g, f.b);
      }
      n = 2 * S;
      if (PROF) t4 = __builtin_readcyclecounter();
      merge_pair_scatter(slab, c, f, scalar_here(S), lane, rank_c, rank_f);
      if (PROF) t5 = __builtin_readcyclecounter();
    } else {
      if (valid) { slab.srt[0][lane] = c.t; slab.srt[1][lane] = c.sigma; slab.srt[2][lane] = c.r; slab.srt[3][lane] = c.g; slab.srt[4][lane] = c.b; }
      wave_lds_fence();
    }
    float w[2];
    CompositeOut o = composite_slab<2>(slab, scalar_here(n), dnorm, k.white, lane, w);
    out_r = o.r; out_g = o.g; out_b = o.b; out_d = o.depth; out_m = o.mask;
    if constexpr (EXTRA) {
      if (k.coords) composite_coords<2>(slab, w, n, lane, ox, oy, oz, dx, dy, dz, k.coords + (size_t)ray * 3);
      float wc = 0.0f, wf = 0.0f;
      if ((SEMP > 0 && semT) || NRM) {
        // the merged weights back in source order (lane = sample): the cdf row is free after the merge
        wave_lds_fence();
        slab.cdf[lane] = w[0]; slab.cdf[64 + lane] = w[1];
        wave_lds_fence();
        wc = valid ? slab.cdf[rank_c] : 0.0f;
        wf = (valid && k.fine) ? slab.cdf[rank_f] : 0.0f;
      }
      if constexpr (NRM) {
        // normal_map = sum_k w_k n_k (+ 1 - mask on a white background), lib/nerf_utils.py:149-151, 159
        const float bgn = k.white ? 1.0f - o.mask : 0.0f;
        const float mx = wave_sum(wc * ncx + wf * nfx) + bgn, my = wave_sum(wc * ncy + wf * nfy) + bgn,
                    mz = wave_sum(wc * ncz + wf * nfz) + bgn;
        if (lane == 0) { float* q = k.normals + (size_t)ray * 3; q[0] = mx; q[1] = my; q[2] = mz; }
      }
      if constexpr (SEMP > 0) {
        if (semT) {
          const lds_float* sl = (const lds_float*)semT;
          float mine = 0.0f;
          for (int a = 0; a < k.A; ++a) {
            const float sa = wave_sum(wc * sl[a * kSemPitch + lane] + wf * sl[a * kSemPitch + 64 + lane]);
            if (lane == a) mine = sa;
          }
          if (lane < k.A) k.semantics[(size_t)ray * k.A + lane] = mine;
        }
      }
    }
    if constexpr (TAPS) {
      if (lane == 0) {
        if (k.near_plane) k.near_plane[ray] = near;
        if (k.far_plane) k.far_plane[ray] = far;
      }
      if (valid) {
        store_sample_tap(k.t_coarse, k.sigma_coarse, k.rgb_coarse, rs + lane, tc, c.sigma, c.r, c.g, c.b);
        if (k.perm) {
          k.perm[(size_t)ray * n + rank_c] = lane;
          if (k.fine) k.perm[(size_t)ray * n + rank_f] = S + lane;
        }
      }
      store_sorted_taps<2>(k, slab, w, ray, n, lane);
    }
    wave_lds_fence();  // slab is reused by the next ray
    if (PROF) {
      unsigned long long t6 = __builtin_readcyclecounter();
      pc[4] += t1 - t0; pc[5] += t2 - t1; pc[6] += t3 - t2; pc[7] += t4 - t3; pc[8] += t5 - t4; pc[9] += t6 - t5; pc[10] += 1;
    }
    // The work fetch waits for its atomic's round trip - and, vmcnt being ONE in-order counter of loads and stores, for
    // every store the wave has in flight.  Here, after the ray's arithmetic and BEFORE its result stores, nothing of this
    // ray is in flight any more (the taps / extra maps of those variants excepted): the wait is the atomic's alone.
    fly = fetch();
    if (lane == 0) store_pixel(*kernel_args_here(), ray, out_r, out_g, out_b, out_d, out_m);
    in = pre;
    cur = nxt;
    nxt = fly;
    skip_run();
  }
  if (PROF && k.prof && lane == 0) {
    pc[11] = __builtin_readcyclecounter() - tk0;
    for (int i = 0; i < 12; ++i) atomicAdd(k.prof + i, pc[i]);
  }
  clock.stop(k);
}

#ifdef NFI_SINGLE_KERNEL
// register-budget work (tools/vgpr_liveness.py): compile ONLY the plain inference kernel of one texel storage type -
// hipcc -S --cuda-device-only -DNFI_SINGLE_KERNEL=<TEX> [-DNFI_SINGLE_MODE=<kRender...>] -DNFI_RENDER_OCC=<waves per SIMD> ... -
// seconds instead of minutes
#ifndef NFI_SINGLE_MODE
#define NFI_SINGLE_MODE 0     // kRenderPlain ... kRenderExtra
#endif
template __global__ void render_fwd_kernel<NFI_SINGLE_KERNEL, true, NFI_RENDER_OCC, NFI_SINGLE_MODE, 1>(RenderKernelParams);
#endif
#if !defined(NFI_SINGLE_KERNEL) || defined(NFI_SINGLE_WIDE)
// The same pipeline for 64 < S <= 128 samples per pass (BASELINE cfg5, ray_multiplier=2): every lane
// owns two coarse and two fine samples (element e = slot*64 + lane), the field is marched 64 points
// at a time, and the merge ranks all 2S keys against each other.
template <int TEX, bool ATT, int MODE, int PREC, bool VD = false, int OCC = NFI_RENDER_OCC>
__global__ __launch_bounds__(256, OCC) void render_fwd_wide_kernel(RenderKernelParams k) {
  constexpr bool TAPS = MODE == kRenderTaps, TERM = MODE == kRenderTerm;
  constexpr bool EXTRA = MODE == kRenderExtra || MODE == kRenderNormals, NRM = MODE == kRenderNormals;
  constexpr int SEMP = (EXTRA && ATT) ? -kSemPitchWide : 0;        // < 0: 16-bit table entries
  constexpr int kImg = VD ? kVdImageFloats : kLdsImageFloats;
  __shared__ __attribute__((aligned(16))) float lds[kImg];
  __shared__ __attribute__((aligned(16))) float vfs[4][64];
  __shared__ WaveSlabWide slabs[4];
  if constexpr (NRM) stage_normal_operands(nfi_dyn_lds, k.image, VD ? kVdW1F : kW1F, VD ? kVdW2 : kW2F);
  ClockProbe clock;
  clock.start(k);
  stage_decoder_image<PREC, kImg>(lds, k.image);
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  WaveSlabWide& slab = slabs[wave];
  float* vf = vfs[wave];
  const int S = k.S;
  const float fill_near = ordered_key_inv(~k.reduce[0]), fill_far = ordered_key_inv(k.reduce[1]);
  const float bg = k.white ? 1.0f : 0.0f;
  const uint32_t n_rays = (uint32_t)k.n_scenes * (uint32_t)k.hw;
  FieldParams P = make_field_params(k.texels, k.res, TEX, k.A, k.use_sdf, k.beta, k.alpha, lds, kImg, k.layout);
  P.vf = vf;
  P.w1t = nfi_dyn_lds; P.w2r0 = nfi_dyn_lds + kW1TFloats;       // (kRenderNormals only)
  int cur_scene = -1;
  // kRenderExtra: this wave's semantics table [A][kSemPitchWide], column = sample: coarse [0,128), fine [128,256)
  typedef __attribute__((address_space(3))) unsigned short lds_u16;
  float* semT = nullptr;
  if constexpr (SEMP != 0) {
    if (k.semantics) {
      semT = reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(nfi_dyn_lds + (NRM ? kNrmLdsFloats : 0)) +
                                      wave * (k.A * kSemPitchWide));
      for (int i = lane; i < k.A * kSemPitchWide / 2; i += 64) ((lds_float*)semT)[i] = 0.0f;
      wave_lds_fence();
    }
  }
  // column `c` of the table (16-bit entries), as the pointer field_wave hands to tile_epilogue
  auto sem_col = [&](int c) -> float* {
    return semT ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(semT) + c) : nullptr;
  };
  RayQueue queue(k, lane);
  uint32_t cur = queue.fetch(), nxt = 0;
  while (cur < n_rays) {
    nxt = queue.fetch();
    const uint32_t ray = queue.ray_of(cur);
    const uint32_t hitb = k.hit[ray];
    if (k.skip_missed && !(hitb & 2)) {
      if (lane == 0) store_pixel(k, ray, bg, bg, bg, 0.0f, 0.0f);
      if constexpr (EXTRA) zero_missed_maps<NRM>(k, ray, lane, bg);
      if constexpr (TAPS) {
        if (k.stash) zero_stash_row(k, ray, S, lane);
      }
    } else {
      const int scene = (int)fastdiv(ray, k.div_scene_rays);
      if (scene != cur_scene) {
        cur_scene = scene;
        enter_scene<TEX>(P, k, vf, scene, lane);
      }
      const size_t r3 = (size_t)ray * 3;
      const float ox = k.ro[r3], oy = k.ro[r3 + 1], oz = k.ro[r3 + 2];
      const float dx = k.rd[r3], dy = k.rd[r3 + 1], dz = k.rd[r3 + 2];
      float near = k.near_raw[ray], far = k.far_raw[ray];
      finish_planes((hitb & 1) != 0, fill_near, fill_far, near, far);
      const float dnorm = norm3(dx, dy, dz);
      const size_t rs = (size_t)ray * S;
      const size_t ts = (size_t)ray * (size_t)k.tap_stride;      // row of this ray in the per-sample tap / stash arrays
      float* stage = &slab.srt[0][0];

      // ---- coarse pass ----
      float tc[2], sc[2], rc[2], gc[2], bc[2];
      bool val[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int e = j * 64 + lane;
        val[j] = e < S;
        const float nz = (k.noise_c && val[j]) ? k.noise_c[rs + e] : 0.0f;
        tc[j] = val[j] ? stratified_depth(near, far, e, S, nz, k.noise_c != nullptr) : 0.0f;
      }
      float nrm[4][3];                  // NRM: unit normals of the coarse (slots 0, 1) and fine (2, 3) samples
#pragma unroll
      for (int j = 0; j < 4; ++j) nrm[j][0] = nrm[j][1] = nrm[j][2] = 0.0f;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // (the per-tile epilogue, here and in the fine pass: the sample-layout one has not been timed in this kernel)
        SampleOut q = field_wave<TEX, ATT, true, PREC, VD, SEMP, NRM, false>(P, k.scene_range, lane, ox + dx * tc[j], oy + dy * tc[j],
                                                                             oz + dz * tc[j], val[j], sem_col(j * 64), nullptr,
                                                                             stage, nullptr, nullptr, k.xray, (int)ray);
        sc[j] = q.sigma; rc[j] = q.r; gc[j] = q.g; bc[j] = q.b;
        if constexpr (NRM) { nrm[j][0] = q.nx; nrm[j][1] = q.ny; nrm[j][2] = q.nz; }
      }
      int n = S;
      float dep[4], sig[4], cr[4], cg[4], cb[4];
      int eidx[4], rank[4];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        dep[j] = tc[j]; sig[j] = sc[j]; cr[j] = rc[j]; cg[j] = gc[j]; cb[j] = bc[j];
        eidx[j] = val[j] ? j * 64 + lane : 0x7fffffff;
        dep[2 + j] = sig[2 + j] = cr[2 + j] = cg[2 + j] = cb[2 + j] = 0.0f;
        eidx[2 + j] = 0x7fffffff;
        rank[j] = j * 64 + lane; rank[2 + j] = 0;
      }
      if (k.fine) {
        // ---- hierarchical resampling + fine pass ----
        float u[2], tf[2], wtap[2], smtap[2], Tc[2];
        int ind[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) u[j] = val[j] ? k.noise_f[(size_t)ray * k.noise_f_stride + j * 64 + lane] : 0.0f;
        wave_lds_fence();
        resample_ray_wide<2>(slab, sc, tc, S, dnorm, u, lane, tf, wtap, smtap, ind, Tc);
        bool vfine[2] = {val[0], val[1]};
        if constexpr (TERM) {
          // first coarse sample in front of which the coarse transmittance is below eps; fine samples behind it are dropped
          const uint64_t dm0 = __ballot(val[0] && Tc[0] < k.term_eps);
          const uint64_t dm1 = __ballot(val[1] && Tc[1] < k.term_eps);
          float t_dead = INFINITY;
          if (dm0) t_dead = bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(tc[0]), (int)__builtin_ctzll(dm0)));
          else if (dm1) t_dead = bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(tc[1]), (int)__builtin_ctzll(dm1)));
          const bool l0 = val[0] && tf[0] <= t_dead, l1 = val[1] && tf[1] <= t_dead;
          const uint64_t lm0 = __ballot(l0), lm1 = __ballot(l1);
          const int n0 = __builtin_popcountll(lm0), nl = n0 + __builtin_popcountll(lm1);
          const uint64_t below = (1ull << lane) - 1ull;
          const int b0 = __builtin_popcountll(lm0 & below), b1 = __builtin_popcountll(lm1 & below);
          const int p0 = l0 ? b0 : nl + (lane - b0);
          const int p1 = l1 ? n0 + b1 : nl + (64 - n0) + (lane - b1);
          wave_lds_fence();
          slab.cdf[p0] = tf[0];
          slab.cdf[p1] = tf[1];
          wave_lds_fence();
          tf[0] = slab.cdf[lane];
          tf[1] = slab.cdf[64 + lane];
          wave_lds_fence();
          vfine[0] = lane < nl;
          vfine[1] = 64 + lane < nl;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          SampleOut q = field_wave<TEX, ATT, true, PREC, VD, SEMP, NRM, false>(P, k.scene_range, lane, ox + dx * tf[j], oy + dy * tf[j],
                                                                               oz + dz * tf[j], vfine[j], sem_col(128 + j * 64),
                                                                               nullptr, stage, nullptr, nullptr, k.xray, (int)ray);
          if (TERM && !vfine[j]) { q.sigma = 0.0f; q.r = 0.0f; q.g = 0.0f; q.b = 0.0f; }
          if constexpr (NRM) { nrm[2 + j][0] = q.nx; nrm[2 + j][1] = q.ny; nrm[2 + j][2] = q.nz; }
          dep[2 + j] = tf[j]; sig[2 + j] = q.sigma; cr[2 + j] = q.r; cg[2 + j] = q.g; cb[2 + j] = q.b;
          eidx[2 + j] = val[j] ? S + j * 64 + lane : 0x7fffffff;
          if constexpr (TAPS) {
            if (val[j]) store_sample_tap(k.t_fine, k.sigma_fine, k.rgb_fine, ts + j * 64 + lane, tf[j], q.sigma, q.r, q.g, q.b);
          }
        }
        n = 2 * S;
        wave_lds_fence();
        if (!merge_pair_scatter_wide(slab, dep, sig, cr, cg, cb, S, lane, rank))
          merge_scatter<4>(slab, dep, sig, cr, cg, cb, eidx, n, rank);
      } else {
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int e = j * 64 + lane;
          if (val[j]) { slab.srt[0][e] = tc[j]; slab.srt[1][e] = sc[j]; slab.srt[2][e] = rc[j]; slab.srt[3][e] = gc[j]; slab.srt[4][e] = bc[j]; }
        }
        wave_lds_fence();
      }
      float w[4];
      CompositeOut o = composite_slab<4>(slab, n, dnorm, k.white, lane, w);
      if (lane == 0) store_pixel(k, ray, o.r, o.g, o.b, o.depth, o.mask);
      if constexpr (EXTRA) {
        if (k.coords) composite_coords<4>(slab, w, n, lane, ox, oy, oz, dx, dy, dz, k.coords + (size_t)ray * 3);
        float ws[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if ((SEMP != 0 && semT) || NRM) {
          // the merged weights back in source order (the cdf row is free after the merge)
          wave_lds_fence();
#pragma unroll
          for (int j = 0; j < 4; ++j) slab.cdf[j * 64 + lane] = w[j];
          wave_lds_fence();
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            ws[j] = val[j] ? slab.cdf[rank[j]] : 0.0f;
            ws[2 + j] = (val[j] && k.fine) ? slab.cdf[rank[2 + j]] : 0.0f;
          }
        }
        if constexpr (NRM) {
          const float bgn = k.white ? 1.0f - o.mask : 0.0f;
          float m3[3];
#pragma unroll
          for (int c = 0; c < 3; ++c)
            m3[c] = wave_sum((ws[0] * nrm[0][c] + ws[1] * nrm[1][c]) + (ws[2] * nrm[2][c] + ws[3] * nrm[3][c])) + bgn;
          if (lane == 0) { float* q = k.normals + (size_t)ray * 3; q[0] = m3[0]; q[1] = m3[1]; q[2] = m3[2]; }
        }
        if constexpr (SEMP != 0) {
          if (semT) {
            const lds_u16* sl = (const lds_u16*)semT;
            float mine = 0.0f;
            for (int a = 0; a < k.A; ++a) {
              const lds_u16* row = sl + a * kSemPitchWide + lane;
              const float sa = wave_sum((ws[0] * (float)row[0] + ws[1] * (float)row[64]) + (ws[2] * (float)row[128] + ws[3] * (float)row[192]));
              if (lane == a) mine = sa * (1.0f / 65535.0f);
            }
            // The unorm16 roundings of a sample's A probabilities do not cancel: their sum is off by up to A / 2 steps, and
            // on a ray that one sample dominates so is the map's (2.1e-5 seen at A = 14, 1.07e-4 possible).  Scale the map so
            // that it sums to the mask, as the fp32 table's does: entry a moves by (its share of the mask) x that error.
            const float tot = wave_sum(mine);
            if (tot > 0.0f) mine *= o.mask / tot;
            if (lane < k.A) k.semantics[(size_t)ray * k.A + lane] = mine;
          }
        }
      }
      if constexpr (TAPS) {
        if (lane == 0) {
          if (k.near_plane) k.near_plane[ray] = near;
          if (k.far_plane) k.far_plane[ray] = far;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (val[j]) {
            store_sample_tap(k.t_coarse, k.sigma_coarse, k.rgb_coarse, ts + j * 64 + lane, tc[j], sc[j], rc[j], gc[j], bc[j]);
            if (k.perm) {
              k.perm[(size_t)ray * n + rank[j]] = j * 64 + lane;
              if (k.fine) k.perm[(size_t)ray * n + rank[2 + j]] = S + j * 64 + lane;
            }
          }
        }
        store_sorted_taps<4>(k, slab, w, ray, n, lane);
      }
      wave_lds_fence();  // slab is reused by the next ray
    }
    cur = nxt;
  }
  clock.stop(k);
}

#endif   // wide kernel
#ifdef NFI_SINGLE_WIDE
template __global__ void render_fwd_wide_kernel<NFI_SINGLE_KERNEL, true, NFI_SINGLE_MODE, 1, false, NFI_RENDER_OCC>(RenderKernelParams);
#endif
