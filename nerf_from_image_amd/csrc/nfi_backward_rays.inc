// nfi_backward_rays.inc — backward kernels of the per-ray stages (included by nfi_kernels.hip).
//
// Autograd of the reference for these stages (SURVEY.md section 8 a18): rgb_map, mask and the
// extra (semantic) map have gradients w.r.t. sigma, rgb, extras and - through dists * ||rd|| -
// the ray direction; depth_map is built from detached tensors (lib/nerf_utils.py:145) and depth
// samples carry no gradient (run.py:197-200, 261).  Camera gradients flow through x = o + d*t.

// ------------------------------------------------------------------------------------------------
// compositing backward (lib/nerf_utils.py:123-161 + the merge of run.py:283-335)
//   w_i = a_i T_i, a_i = 1 - exp(-sigma_i delta_i), T_i = prod_{j<i} (1 - a_j + 1e-10)
//   g_a_i = g_w_i T_i - (sum_{k>i} g_w_k w_k) / (1 - a_i + 1e-10)
// ------------------------------------------------------------------------------------------------
template <int NS>
__global__ __launch_bounds__(256) void composite_bwd_kernel(nfi_composite_bwd_args a) {
  __shared__ WaveSlabT<64 * NS> slabs[4];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * 4 + wave;
  if (ray >= a.n_rays) return;
  auto& slab = slabs[wave];
  const int na = a.n_a, nb = a.n_b, n = na + nb;
  const size_t row_a = a.list_row_stride > 0 ? (size_t)a.list_row_stride : (size_t)na;     // entries per ray in list a / b arrays
  const size_t row_b = a.list_row_stride > 0 ? (size_t)a.list_row_stride : (size_t)nb;
  float dep[NS], sig[NS], cr[NS], cg[NS], cb[NS];
  int eidx[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    dep[j] = sig[j] = cr[j] = cg[j] = cb[j] = 0.0f;
    eidx[j] = e;
    if (e < na) {
      size_t i = (size_t)ray * row_a + e;
      dep[j] = a.depth_a[i]; sig[j] = a.sigma_a[i];
      cr[j] = a.rgb_a[i * 3]; cg[j] = a.rgb_a[i * 3 + 1]; cb[j] = a.rgb_a[i * 3 + 2];
    } else if (e < n) {
      size_t i = (size_t)ray * row_b + (e - na);
      dep[j] = a.depth_b[i]; sig[j] = a.sigma_b[i];
      cr[j] = a.rgb_b[i * 3]; cg[j] = a.rgb_b[i * 3 + 1]; cb[j] = a.rgb_b[i * 3 + 2];
    }
  }
  int rank[NS];
  bool merged = false;
  if constexpr (NS == 2) {
    if (na == 64 && nb == 64) {
      // 64 + 64 (the renderer's own configuration): slot 0 is list a, slot 1 list b, one sample per lane - the ranking of
      // the fused forward (list a ascending: only the 64 keys of b are counted against; the general count otherwise)
      const MergeIn c{dep[0], sig[0], cr[0], cg[0], cb[0]}, f{dep[1], sig[1], cr[1], cg[1], cb[1]};
      merge_pair_scatter(slab, c, f, 64, lane, rank[0], rank[1]);
      merged = true;
    }
  }
  if (merged) {
  } else if (nb > 0) {
    merge_scatter<NS>(slab, dep, sig, cr, cg, cb, eidx, n, rank);
  } else {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      int e = j * 64 + lane;
      rank[j] = e;
      if (e < n) { slab.srt[0][e] = dep[j]; slab.srt[1][e] = sig[j]; }
    }
    wave_lds_fence();
  }
  // upstream gradients (uniform per ray)
  const float gcr = a.g_rgb_map[ray * 3], gcg = a.g_rgb_map[ray * 3 + 1], gcb = a.g_rgb_map[ray * 3 + 2];
  float gm = a.g_mask ? a.g_mask[ray] : 0.0f;
  if (a.white_background) gm -= (gcr + gcg) + gcb;   // rgb_map += 1 - mask
  // g_w per source element, parked at its merged position
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    if (e < n) {
      float gw = (gcr * cr[j] + gcg * cg[j]) + gcb * cb[j] + gm;
      if (a.n_extra > 0 && a.g_extra_map) {
        const float* ex = (e < na) ? a.extra_a + ((size_t)ray * row_a + e) * a.n_extra
                                   : a.extra_b + ((size_t)ray * row_b + (e - na)) * a.n_extra;
        for (int c = 0; c < a.n_extra; ++c) gw += a.g_extra_map[ray * a.n_extra + c] * ex[c];
      }
      slab.cdf[rank[j]] = gw;
    }
  }
  wave_lds_fence();
  // forward recompute in merged order
  const float dx = a.ray_directions[ray * 3], dy = a.ray_directions[ray * 3 + 1], dz = a.ray_directions[ray * 3 + 2];
  const float dn = norm3(dx, dy, dz);
  float t[NS], s[NS], tn[NS], alpha[NS], om[NS], T[NS], dt[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    t[j] = (e < n) ? slab.srt[0][e] : 0.0f;
    s[j] = (e < n) ? slab.srt[1][e] : 0.0f;
  }
  next_elem<NS>(t, tn, lane);
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    dt[j] = (e < n - 1) ? (tn[j] - t[j]) : 0.0f;
    float al = 1.0f - expf(-s[j] * (dt[j] * dn));
    if (e >= n) al = 0.0f;
    alpha[j] = al;
    om[j] = (1.0f - al) + 1e-10f;
  }
  excl_cumprod<NS>(om, T, lane);
  float gwm[NS], prod[NS], incl[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    gwm[j] = (e < n) ? slab.cdf[e] : 0.0f;
    prod[j] = gwm[j] * (alpha[j] * T[j]);
  }
  incl_cumsum<NS>(prod, incl, lane);
  const float total = bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(incl[NS - 1]), 63));
  wave_lds_fence();
  float g_dn = 0.0f;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    if (e < n) {
      float suffix = total - incl[j];                 // sum_{k>e} g_w_k w_k
      float ga = gwm[j] * T[j] - suffix / om[j];
      float keep = 1.0f - alpha[j];                   // exp(-sigma delta)
      float gs = ga * (dt[j] * dn) * keep;
      float gdelta = ga * s[j] * keep;
      g_dn += gdelta * dt[j];
      slab.bins[e] = gs;                              // g_sigma in merged order
      slab.cdf[e] = alpha[j] * T[j];                  // w in merged order
    }
  }
  g_dn = wave_sum(g_dn);
  wave_lds_fence();
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    if (e < n) {
      const float gs = slab.bins[rank[j]], w = slab.cdf[rank[j]];
      if (e < na) {
        size_t i = (size_t)ray * row_a + e;
        a.g_sigma_a[i] = gs;
        a.g_rgb_a[i * 3] = w * gcr; a.g_rgb_a[i * 3 + 1] = w * gcg; a.g_rgb_a[i * 3 + 2] = w * gcb;
        if (a.g_extra_a) for (int c = 0; c < a.n_extra; ++c) a.g_extra_a[i * a.n_extra + c] = w * a.g_extra_map[ray * a.n_extra + c];
      } else {
        size_t i = (size_t)ray * row_b + (e - na);
        a.g_sigma_b[i] = gs;
        a.g_rgb_b[i * 3] = w * gcr; a.g_rgb_b[i * 3 + 1] = w * gcg; a.g_rgb_b[i * 3 + 2] = w * gcb;
        if (a.g_extra_b) for (int c = 0; c < a.n_extra; ++c) a.g_extra_b[i * a.n_extra + c] = w * a.g_extra_map[ray * a.n_extra + c];
      }
    }
  }
  if (lane == 0 && a.g_ray_directions) {
    const float sc = g_dn / dn;
    a.g_ray_directions[ray * 3] = sc * dx; a.g_ray_directions[ray * 3 + 1] = sc * dy; a.g_ray_directions[ray * 3 + 2] = sc * dz;
  }
}

extern "C" int nfi_composite_bwd(const nfi_composite_bwd_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->ray_directions && a->depth_a && a->sigma_a && a->rgb_a && a->g_rgb_map && a->g_sigma_a && a->g_rgb_a,
          "composite_bwd: null pointer");
  REQUIRE(a->n_rays > 0 && a->n_a > 0 && a->n_b >= 0 && a->n_a + a->n_b <= NFI_MAX_SAMPLES_SINGLE_PASS,
          "composite_bwd: need 1 <= n_a + n_b <= 512");
  REQUIRE(a->n_b == 0 || (a->n_a <= NFI_MAX_SAMPLES && a->n_b <= NFI_MAX_SAMPLES), "composite_bwd: merged lists hold at most 128 samples each");
  REQUIRE(a->n_b == 0 || (a->depth_b && a->sigma_b && a->rgb_b && a->g_sigma_b && a->g_rgb_b), "composite_bwd: list b missing");
  REQUIRE(a->n_extra == 0 || !a->g_extra_map || (a->extra_a && (a->n_b == 0 || a->extra_b)), "composite_bwd: extra attribute missing");
  REQUIRE(a->list_row_stride == 0 || a->list_row_stride >= std::max(a->n_a, a->n_b), "composite_bwd: list_row_stride shorter than a list");
  const dim3 grid((unsigned)((a->n_rays + 3) / 4));
  if (a->n_a + a->n_b <= 128) hipLaunchKernelGGL(composite_bwd_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  else if (a->n_a + a->n_b <= 256) hipLaunchKernelGGL(composite_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  else hipLaunchKernelGGL(composite_bwd_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  return check_launch("composite_bwd");
}

// ------------------------------------------------------------------------------------------------
// x = o + d t  backward:  g_o = sum_s g_x,  g_d = sum_s g_x t   (t carries no gradient)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void points_bwd_kernel(const float* __restrict__ g_points, const float* __restrict__ depth,
                                                         int64_t n_rays, int S, float* __restrict__ g_ro,
                                                         float* __restrict__ g_rd) {
  const int lane = lane_id();
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= n_rays) return;
  float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
  for (int e = lane; e < S; e += 64) {
    const size_t i = (size_t)ray * S + e;
    const float t = depth[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float g = g_points[i * 3 + c];
      o[c] += g;
      d[c] += g * t;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { o[c] = wave_sum(o[c]); d[c] = wave_sum(d[c]); }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (g_ro) g_ro[ray * 3 + c] = o[c];
      if (g_rd) g_rd[ray * 3 + c] = d[c];
    }
  }
}

extern "C" int nfi_points_bwd(const float* g_points, const float* depth, int64_t n_rays, int n_samples, float* g_ro,
                              float* g_rd, nfi_stream_t stream) {
  REQUIRE(g_points && depth && (g_ro || g_rd), "points_bwd: null pointer");
  REQUIRE(n_rays > 0 && n_samples > 0, "points_bwd: bad shape");
  hipLaunchKernelGGL(points_bwd_kernel, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g_points,
                     depth, n_rays, n_samples, g_ro, g_rd);
  return check_launch("points_bwd");
}

// ------------------------------------------------------------------------------------------------
// camera-ray backward (lib/nerf_utils.py:28-91 + F.normalize): g_ro, g_rd -> g_cam2world, g_focal
// ------------------------------------------------------------------------------------------------
// one pixel's terms of the 17 sums (16 entries of cam2world + focal), added to acc
__device__ __forceinline__ void raygen_bwd_pixel(const CameraParams& cam, int b, int pix, const float* __restrict__ g_ro,
                                                 const float* __restrict__ g_rd, double (&acc)[17]) {
  const int hw = cam.height * cam.width;
  const int row = pix / cam.width, col = pix - row * cam.width;
  const int64_t ray = (int64_t)b * hw + pix;
  const float* M = cam.cam2world + (size_t)b * 16;
  // forward recompute of the camera-space vectors (un-normalised)
  CameraParams c2 = cam;
  c2.normalize = 0;
  float o[3], raw[3];
  make_ray(c2, b, row, col, o, raw);
  float go[3] = {0.0f, 0.0f, 0.0f}, gd[3] = {0.0f, 0.0f, 0.0f};
  if (g_ro) { go[0] = g_ro[ray * 3]; go[1] = g_ro[ray * 3 + 1]; go[2] = g_ro[ray * 3 + 2]; }
  if (g_rd) { gd[0] = g_rd[ray * 3]; gd[1] = g_rd[ray * 3 + 1]; gd[2] = g_rd[ray * 3 + 2]; }
  float graw[3] = {gd[0], gd[1], gd[2]};
  if (cam.normalize) {
    const float nrm = fmaxf(norm3(raw[0], raw[1], raw[2]), 1e-12f);
    const float ux = raw[0] / nrm, uy = raw[1] / nrm, uz = raw[2] / nrm;
    const float dot = ux * gd[0] + uy * gd[1] + uz * gd[2];
    graw[0] = (gd[0] - ux * dot) / nrm; graw[1] = (gd[1] - uy * dot) / nrm; graw[2] = (gd[2] - uz * dot) / nrm;
  }
  float u = (float)col / (float)cam.width, v = (float)row / (float)cam.height;
  if (cam.focal) {
    if (cam.center) { u = (u - 0.5f * (2.0f * cam.center[b * 2] - 1.0f)) - 0.5f; v = (v - 0.5f * (2.0f * cam.center[b * 2 + 1] - 1.0f)) - 0.5f; }
    else { u -= 0.5f; v -= 0.5f; }
    if (cam.bbox) { const float* bb = cam.bbox + b * 4; u = (bb[2] * (u + 0.5f) + bb[0]) * 0.5f; v = -(bb[3] * (-v + 0.5f) + bb[1]) * 0.5f; }
    const float f = cam.focal[b];
    const float cd[3] = {u / f, -(v / f), -1.0f};
    float gcd[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int m = 0; m < 3; ++m) { acc[k * 4 + m] += graw[k] * cd[m]; gcd[m] += graw[k] * M[k * 4 + m]; }
      acc[k * 4 + 3] += go[k];
    }
    acc[16] += (gcd[0] * (-u) + gcd[1] * v) / (f * f);
  } else {
    u = (u - 0.5f) * 2.0f; v = (v - 0.5f) * 2.0f;
    if (cam.bbox) { const float* bb = cam.bbox + b * 4; u = bb[2] * (u / 2.0f + 0.5f) + bb[0]; v = -(bb[3] * (-v / 2.0f + 0.5f) + bb[1]); }
    const float co[3] = {u, -v, 0.0f};
    const float w = M[15];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      acc[k * 4 + 0] += go[k] * co[0];
      acc[k * 4 + 1] += go[k] * co[1];
      acc[k * 4 + 2] += go[k] * co[2] - graw[k] / w;    // cd = (0,0,-1), rd = (R cd)/w
      acc[k * 4 + 3] += go[k];
      acc[15] += -graw[k] * raw[k] / w;                 // raw = (R cd)/w
    }
  }
}

// the block's 17 sums (256 threads): lanes, then the four waves, in float64 and in a fixed order; thread t < 17 gets sum t
// rounded to fp32
__device__ __forceinline__ float raygen_bwd_block_sum(const double (&acc)[17], double (&red)[4][17]) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 17; ++i) {
    double s = acc[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[wave][i] = s;
  }
  __syncthreads();
  const int t = threadIdx.x < 17 ? threadIdx.x : 0;
  return (float)((red[0][t] + red[1][t]) + (red[2][t] + red[3][t]));
}

__global__ __launch_bounds__(256) void raygen_bwd_kernel(CameraParams cam, int n_scenes, const float* __restrict__ g_ro,
                                                         const float* __restrict__ g_rd, float* __restrict__ g_cam,
                                                         float* __restrict__ g_focal) {
  // the 17 sums run over every ray of the image and cancel heavily (terms of both signs, |sum| << sum |term|): the block
  // accumulates them in float64 (the per-ray terms are fp32 products, as the reference's) - a 14 us kernel either way
  __shared__ double red[4][17];
  const int hw = cam.height * cam.width;
  const int b = blockIdx.y;
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  double acc[17];
#pragma unroll
  for (int i = 0; i < 17; ++i) acc[i] = 0.0;   // 16 matrix entries + focal
  if (pix < hw) raygen_bwd_pixel(cam, b, pix, g_ro, g_rd, acc);
  const float s = raygen_bwd_block_sum(acc, red);
  if (threadIdx.x < 17) {
    if (threadIdx.x < 16) atomicAdd(&g_cam[b * 16 + threadIdx.x], s);
    else if (g_focal) atomicAdd(&g_focal[b], s);
  }
}

extern "C" int nfi_raygen_bwd(const nfi_raygen_args* a, const float* g_ray_origins, const float* g_ray_directions,
                              float* g_cam2world, float* g_focal, nfi_stream_t stream) {
  REQUIRE(a && a->cam2world && g_cam2world && (g_ray_origins || g_ray_directions), "raygen_bwd: null pointer");
  REQUIRE(a->n_scenes > 0 && a->height > 0 && a->width > 0, "raygen_bwd: bad shape");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(g_cam2world, 0, sizeof(float) * 16 * a->n_scenes, s) != hipSuccess) return fail(NFI_ERR_LAUNCH, "raygen_bwd: memset failed");
  if (g_focal && hipMemsetAsync(g_focal, 0, sizeof(float) * a->n_scenes, s) != hipSuccess) return fail(NFI_ERR_LAUNCH, "raygen_bwd: memset failed");
  CameraParams cam{a->cam2world, a->focal, a->bbox, a->focal ? a->center : nullptr, a->height, a->width, a->normalize, a->height, 0};
  const int hw = a->height * a->width;
  dim3 grid((unsigned)((hw + 255) / 256), (unsigned)a->n_scenes);
  hipLaunchKernelGGL(raygen_bwd_kernel, grid, dim3(256), 0, s, cam, a->n_scenes, g_ray_origins, g_ray_directions,
                     g_cam2world, g_focal);
  return check_launch("raygen_bwd");
}

// ordered variant: one block per image walks all pixels (thread t: pixels t, t + 256, ...), the 17 sums stay in float64
// over the whole image (lanes, then waves, in a fixed order), are rounded once and STORED: no atomic, no memset, the same
// bits on every launch - and closer to the exact sums than the per-block rounding above
__global__ __launch_bounds__(256) void raygen_bwd_ordered_kernel(CameraParams cam, const float* __restrict__ g_ro,
                                                                 const float* __restrict__ g_rd, float* __restrict__ g_cam,
                                                                 float* __restrict__ g_focal) {
  __shared__ double red[4][17];
  const int hw = cam.height * cam.width;
  const int b = blockIdx.x;
  double acc[17];
#pragma unroll
  for (int i = 0; i < 17; ++i) acc[i] = 0.0;
  for (int pix = threadIdx.x; pix < hw; pix += 256) raygen_bwd_pixel(cam, b, pix, g_ro, g_rd, acc);
  const float s = raygen_bwd_block_sum(acc, red);
  if (threadIdx.x < 17) {
    if (threadIdx.x < 16) g_cam[b * 16 + threadIdx.x] = s;
    else if (g_focal) g_focal[b] = s;
  }
}

extern "C" int nfi_raygen_bwd_ordered(const nfi_raygen_args* a, const float* g_ray_origins, const float* g_ray_directions,
                                      float* g_cam2world, float* g_focal, nfi_stream_t stream) {
  REQUIRE(a && a->cam2world && g_cam2world && (g_ray_origins || g_ray_directions), "raygen_bwd_ordered: null pointer");
  REQUIRE(a->n_scenes > 0 && a->height > 0 && a->width > 0, "raygen_bwd_ordered: bad shape");
  CameraParams cam{a->cam2world, a->focal, a->bbox, a->focal ? a->center : nullptr, a->height, a->width, a->normalize, a->height, 0};
  hipLaunchKernelGGL(raygen_bwd_ordered_kernel, dim3((unsigned)a->n_scenes), dim3(256), 0, (hipStream_t)stream, cam,
                     g_ray_origins, g_ray_directions, g_cam2world, g_focal);
  return check_launch("raygen_bwd_ordered");
}
