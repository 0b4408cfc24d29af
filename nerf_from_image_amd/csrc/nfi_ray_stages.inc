// nfi_ray_stages.inc — the per-ray stages as kernels of their own, one wave per ray: nfi_ray_weights, nfi_sample_pdf,
// nfi_resample, nfi_composite_fwd (included by nfi_kernels.hip).  The staged path of the renderer and the tests' handle
// on each stage of the fused one.  Expects nfi_wave_slab.inc (every stage is a thin kernel around its helpers),
// nfi_host.hpp and `using namespace nfi`.

// ------------------------------------------------------------------------------------------------
// stand-alone stage kernels (one wave per ray)
// ------------------------------------------------------------------------------------------------
template <int NS>
__global__ __launch_bounds__(256) void ray_weights_kernel(nfi_weights_args a) {
  const int lane = lane_id();
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= a.n_rays) return;
  const int S = a.n_samples;
  float sig[NS], t[NS], w[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    sig[j] = e < S ? a.sigma[ray * S + e] : 0.0f;
    t[j] = e < S ? a.depth[ray * S + e] : 0.0f;
  }
  float dn = norm3(a.ray_directions[ray * 3], a.ray_directions[ray * 3 + 1], a.ray_directions[ray * 3 + 2]);
  ray_weights<NS>(sig, t, S, dn, lane, w);
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    if (e < S) a.weights[ray * S + e] = w[j];
  }
}

extern "C" int nfi_ray_weights(const nfi_weights_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->sigma && a->ray_directions && a->depth && a->weights, "ray_weights: null pointer");
  REQUIRE(a->n_rays > 0 && a->n_samples > 0 && a->n_samples <= NFI_MAX_SAMPLES_SINGLE_PASS, "ray_weights: n_samples must be in [1,512]");
  const dim3 grid((unsigned)((a->n_rays + 3) / 4));
  if (a->n_samples <= 128) hipLaunchKernelGGL(ray_weights_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  else hipLaunchKernelGGL(ray_weights_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  return check_launch("ray_weights");
}

__global__ __launch_bounds__(256) void sample_pdf_kernel(nfi_sample_pdf_args a) {
  __shared__ WaveSlab slabs[4];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * 4 + wave;
  if (ray >= a.n_rays) return;
  WaveSlab& slab = slabs[wave];
  const int M = a.n_bins, K = a.n_samples;
  float bins[2], wts[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int e = j * 64 + lane;
    bins[j] = e < M ? a.bins[ray * M + e] : 0.0f;
    wts[j] = e < M - 1 ? a.weights[ray * (M - 1) + e] : 0.0f;
  }
  build_cdf<2>(slab, bins, wts, M, lane);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int e = j * 64 + lane;
    if (e < K) {
      float u = a.u[ray * a.u_row_stride + e];
      int ind;
      float z = invert_cdf<16>(slab, M, u, ind);
      a.samples[ray * K + e] = z;
      if (a.inds) a.inds[ray * K + e] = ind;
    }
    if (a.cdf && e < M) a.cdf[ray * M + e] = slab.cdf[e];
  }
}

extern "C" int nfi_sample_pdf(const nfi_sample_pdf_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->bins && a->weights && a->u && a->samples, "sample_pdf: null pointer");
  REQUIRE(a->n_rays > 0 && a->n_bins >= 2 && a->n_bins <= 128 && a->n_samples >= 1 && a->n_samples <= 128,
          "sample_pdf: need 2 <= bins <= 128 and 1 <= samples <= 128");
  hipLaunchKernelGGL(sample_pdf_kernel, dim3((unsigned)((a->n_rays + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *a);
  return check_launch("sample_pdf");
}

__global__ __launch_bounds__(256) void resample_kernel(nfi_resample_args a) {
  __shared__ WaveSlab slabs[4];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * 4 + wave;
  if (ray >= a.n_rays) return;
  WaveSlab& slab = slabs[wave];
  const int S = a.n_samples;
  float sigma = lane < S ? a.sigma[ray * S + lane] : 0.0f;
  float t = lane < S ? a.depth[ray * S + lane] : 0.0f;
  float u = lane < S ? a.u[ray * a.u_row_stride + lane] : 0.0f;
  float dn = norm3(a.ray_directions[ray * 3], a.ray_directions[ray * 3 + 1], a.ray_directions[ray * 3 + 2]);
  ResampleTaps taps;
  float z = resample_ray(slab, sigma, t, S, dn, u, lane, &taps);
  if (lane < S) {
    a.fine_depth[ray * S + lane] = z;
    if (a.weights) a.weights[ray * S + lane] = taps.w;
    if (a.smooth) a.smooth[ray * S + lane] = taps.smooth;
    if (a.inds) a.inds[ray * S + lane] = taps.ind;
  }
  if (a.cdf && lane < S - 1) a.cdf[ray * (S - 1) + lane] = slab.cdf[lane];
}

__global__ __launch_bounds__(256) void resample_wide_kernel(nfi_resample_args a) {
  __shared__ WaveSlab slabs[4];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * 4 + wave;
  if (ray >= a.n_rays) return;
  WaveSlab& slab = slabs[wave];
  const int S = a.n_samples;
  float sigma[2], t[2], u[2], z[2], w[2], sm[2];
  int ind[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int e = j * 64 + lane;
    sigma[j] = e < S ? a.sigma[ray * S + e] : 0.0f;
    t[j] = e < S ? a.depth[ray * S + e] : 0.0f;
    u[j] = e < S ? a.u[ray * a.u_row_stride + e] : 0.0f;
  }
  float dn = norm3(a.ray_directions[ray * 3], a.ray_directions[ray * 3 + 1], a.ray_directions[ray * 3 + 2]);
  float Tc[2];
  resample_ray_wide<2>(slab, sigma, t, S, dn, u, lane, z, w, sm, ind, Tc);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int e = j * 64 + lane;
    if (e < S) {
      a.fine_depth[ray * S + e] = z[j];
      if (a.weights) a.weights[ray * S + e] = w[j];
      if (a.smooth) a.smooth[ray * S + e] = sm[j];
      if (a.inds) a.inds[ray * S + e] = ind[j];
    }
    if (a.cdf && e < S - 1) a.cdf[ray * (S - 1) + e] = slab.cdf[e];
  }
}

extern "C" int nfi_resample(const nfi_resample_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->sigma && a->ray_directions && a->depth && a->u && a->fine_depth, "resample: null pointer");
  REQUIRE(a->n_rays > 0 && a->n_samples >= 4 && a->n_samples <= NFI_MAX_SAMPLES, "resample: n_samples must be in [4,128]");
  const dim3 grid((unsigned)((a->n_rays + 3) / 4));
  if (a->n_samples <= 64) hipLaunchKernelGGL(resample_kernel, grid, dim3(256), 0, (hipStream_t)stream, *a);
  else hipLaunchKernelGGL(resample_wide_kernel, grid, dim3(256), 0, (hipStream_t)stream, *a);
  return check_launch("resample");
}

template <int NS>
__global__ __launch_bounds__(256) void composite_kernel(nfi_composite_args a) {
  __shared__ WaveSlabT<64 * NS> slabs[4];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * 4 + wave;
  if (ray >= a.n_rays) return;
  auto& slab = slabs[wave];
  const int na = a.n_a, nb = a.n_b, n = na + nb;
  float dep[NS], sig[NS], cr[NS], cg[NS], cb[NS];
  int eidx[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    dep[j] = sig[j] = cr[j] = cg[j] = cb[j] = 0.0f;
    eidx[j] = e;
    if (e < na) {
      size_t i = (size_t)ray * na + e;
      dep[j] = a.depth_a[i]; sig[j] = a.sigma_a[i];
      cr[j] = a.rgb_a[i * 3]; cg[j] = a.rgb_a[i * 3 + 1]; cb[j] = a.rgb_a[i * 3 + 2];
    } else if (e < n) {
      size_t i = (size_t)ray * nb + (e - na);
      dep[j] = a.depth_b[i]; sig[j] = a.sigma_b[i];
      cr[j] = a.rgb_b[i * 3]; cg[j] = a.rgb_b[i * 3 + 1]; cb[j] = a.rgb_b[i * 3 + 2];
    }
  }
  int rank[NS];
  if (nb > 0) {
    merge_scatter<NS>(slab, dep, sig, cr, cg, cb, eidx, n, rank);
  } else {
    // list a is composited in the order given (render_volume_density does not sort)
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      int e = j * 64 + lane;
      rank[j] = e;
      if (e < n) { slab.srt[0][e] = dep[j]; slab.srt[1][e] = sig[j]; slab.srt[2][e] = cr[j]; slab.srt[3][e] = cg[j]; slab.srt[4][e] = cb[j]; }
    }
    wave_lds_fence();
  }
  float dn = norm3(a.ray_directions[ray * 3], a.ray_directions[ray * 3 + 1], a.ray_directions[ray * 3 + 2]);
  float w[NS];
  CompositeOut o = composite_slab<NS>(slab, n, dn, a.white_background, lane, w);
  if (lane == 0) {
    a.rgb_map[ray * 3] = o.r; a.rgb_map[ray * 3 + 1] = o.g; a.rgb_map[ray * 3 + 2] = o.b;
    a.depth_map[ray] = o.depth;
    a.mask[ray] = o.mask;
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    if (e < n) {
      if (a.weights) a.weights[(size_t)ray * n + e] = w[j];
      if (a.depth_sorted) a.depth_sorted[(size_t)ray * n + e] = slab.srt[0][e];
      if (a.perm) a.perm[(size_t)ray * n + rank[j]] = e;
    }
  }
  // extra attribute (semantics / normals / coords): weights are in merged order, attributes in input order
  if (a.n_extra > 0 && a.extra_map) {
    wave_lds_fence();
    // park the merged-order weights in the slab, then every lane accumulates its own elements
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      int e = j * 64 + lane;
      if (e < n) slab.cdf[e] = w[j];
    }
    wave_lds_fence();
    float we[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) { int e = j * 64 + lane; we[j] = e < n ? slab.cdf[rank[j]] : 0.0f; }
    for (int c = 0; c < a.n_extra; ++c) {
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        int e = j * 64 + lane;
        if (e < na) acc += we[j] * a.extra_a[((size_t)ray * na + e) * a.n_extra + c];
        else if (e < n) acc += we[j] * a.extra_b[((size_t)ray * nb + (e - na)) * a.n_extra + c];
      }
      acc = wave_sum(acc);
      if (lane == 0) a.extra_map[ray * a.n_extra + c] = acc;
    }
  }
}

extern "C" int nfi_composite_fwd(const nfi_composite_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->ray_directions && a->depth_a && a->sigma_a && a->rgb_a && a->rgb_map && a->depth_map && a->mask,
          "composite: null pointer");
  REQUIRE(a->n_rays > 0 && a->n_a > 0 && a->n_b >= 0 && a->n_a + a->n_b <= NFI_MAX_SAMPLES_SINGLE_PASS,
          "composite: need 1 <= n_a + n_b <= 512");
  REQUIRE(a->n_b == 0 || (a->n_a <= NFI_MAX_SAMPLES && a->n_b <= NFI_MAX_SAMPLES), "composite: merged lists hold at most 128 samples each");
  REQUIRE(a->n_b == 0 || (a->depth_b && a->sigma_b && a->rgb_b), "composite: list b missing");
  REQUIRE(a->n_extra == 0 || (a->extra_a && (a->n_b == 0 || a->extra_b)), "composite: extra attribute missing");
  const dim3 grid((unsigned)((a->n_rays + 3) / 4));
  if (a->n_a + a->n_b <= 128) hipLaunchKernelGGL(composite_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  else if (a->n_a + a->n_b <= 256) hipLaunchKernelGGL(composite_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  else hipLaunchKernelGGL(composite_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  return check_launch("composite_fwd");
}
