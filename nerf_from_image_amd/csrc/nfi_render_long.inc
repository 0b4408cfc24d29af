// nfi_render_long.inc — render_fwd_long_kernel, the third persistent render kernel (included by nfi_kernels.hip; left
// out of the NFI_SINGLE_KERNEL compiles).  Expects nfi_render_kernels.inc (RenderKernelParams, the queue and the shared
// scaffolding), nfi_wave_slab.inc (composite_slab), nfi_rays.inc (finish_planes, stratified_depth).

// One pass of 128 < S <= 512 samples without hierarchical resampling (run.py:2271: the inversion of a model trained
// without --fine_sampling asks for depth_samples_per_ray * 4 = 512 samples in a single pass).  Same persistent
// one-wave-per-ray scheme; the per-sample results go to this wave's LDS rows (element e = slot*64 + lane, already in
// ascending depth order - render_volume_density does not sort) and are composited from there.  The stage taps and the
// training stash are run-time switches here (a handful of wave-uniform branches per 64 samples).
struct __attribute__((aligned(16))) WaveSlabLong {
  float srt[5][NFI_MAX_SAMPLES_SINGLE_PASS];   // depth, sigma, r, g, b
  float stage[16 * 36];                        // field_wave's feature-tile transpose
};

template <int TEX, bool ATT, int PREC, bool VD = false>
__global__ __launch_bounds__(256, NFI_RENDER_OCC) void render_fwd_long_kernel(RenderKernelParams k) {
  constexpr int kImg = VD ? kVdImageFloats : kLdsImageFloats;
  constexpr int NS = NFI_MAX_SAMPLES_SINGLE_PASS / 64;
  __shared__ __attribute__((aligned(16))) float lds[kImg];
  __shared__ __attribute__((aligned(16))) float vfs[4][64];
  __shared__ WaveSlabLong slabs[4];
  ClockProbe clock;
  clock.start(k);
  stage_decoder_image<PREC, kImg>(lds, k.image);
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  WaveSlabLong& slab = slabs[wave];
  float* vf = vfs[wave];
  const int S = k.S;
  const int slots = (S + 63) >> 6;
  const float fill_near = ordered_key_inv(~k.reduce[0]), fill_far = ordered_key_inv(k.reduce[1]);
  const float bg = k.white ? 1.0f : 0.0f;
  const uint32_t n_rays = (uint32_t)k.n_scenes * (uint32_t)k.hw;
  FieldParams P = make_field_params(k.texels, k.res, TEX, k.A, k.use_sdf, k.beta, k.alpha, lds, kImg, k.layout);
  P.vf = vf;
  int cur_scene = -1;
  RayQueue queue(k, lane);
  uint32_t cur = queue.fetch(), nxt = 0;
  while (cur < n_rays) {
    nxt = queue.fetch();
    const uint32_t ray = queue.ray_of(cur);
    const uint32_t hitb = k.hit[ray];
    const size_t ts = (size_t)ray * (size_t)k.tap_stride;
    if (k.skip_missed && !(hitb & 2)) {
      if (lane == 0) store_pixel(k, ray, bg, bg, bg, 0.0f, 0.0f);
      if (k.stash) zero_stash_row(k, ray, S, lane);
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
#pragma unroll 1
      for (int j = 0; j < slots; ++j) {
        const int e = j * 64 + lane;
        const bool val = e < S;
        const float nz = (k.noise_c && val) ? k.noise_c[rs + e] : 0.0f;
        const float t = val ? stratified_depth(near, far, e, S, nz, k.noise_c != nullptr) : 0.0f;
        // (the per-tile epilogue: 63.8 KB of per-sample rows, all live while the field is marched - 75.3 KB with the
        //  view-direction image - leave no room for an output table beside two workgroups per CU)
        SampleOut q = field_wave<TEX, ATT, true, PREC, VD, 0, false, false>(P, k.scene_range, lane, ox + dx * t, oy + dy * t,
                                                                            oz + dz * t, val, nullptr, nullptr, slab.stage,
                                                                            nullptr, nullptr, k.xray, (int)ray);
        if (val) {
          slab.srt[0][e] = t; slab.srt[1][e] = q.sigma; slab.srt[2][e] = q.r; slab.srt[3][e] = q.g; slab.srt[4][e] = q.b;
          store_sample_tap(k.t_coarse, k.sigma_coarse, k.rgb_coarse, ts + e, t, q.sigma, q.r, q.g, q.b);
        }
      }
      wave_lds_fence();
      float w[NS];
      CompositeOut o = composite_slab<NS>(slab, S, dnorm, k.white, lane, w);
      if (lane == 0) {
        store_pixel(k, ray, o.r, o.g, o.b, o.depth, o.mask);
        if (k.near_plane) k.near_plane[ray] = near;
        if (k.far_plane) k.far_plane[ray] = far;
      }
      if (k.weights || k.t_sorted) store_sorted_taps<NS>(k, slab, w, ray, S, lane);
      if (k.perm) {
        for (int e = lane; e < S; e += 64) k.perm[rs + e] = e;
      }
      wave_lds_fence();  // the rows are reused by the next ray
    }
    cur = nxt;
  }
  clock.stop(k);
}
