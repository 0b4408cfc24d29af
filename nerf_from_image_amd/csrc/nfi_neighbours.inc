// nfi_neighbours.inc — the inversion loop's neighbours of the renderer (included by nfi_modules.hip; SURVEY.md 8(f)4).
//
// (1) The 2-D augmentation warp of run.py:720-769 (augment_impl): per image a rotation / isotropic scale /
//     translation drawn on the host, F.affine_grid(align_corners=False) + F.grid_sample(bilinear, zeros padding,
//     align_corners=False), with the white-background adjustment (img - 1 ... + 1).  The inversion loss applies it
//     15 times to cat(prediction, target) per step (run.py:2216-2231), so its backward (w.r.t. the image) is on
//     the path too.  One launch builds the matrix from (rot, scale, translation) and warps all channels of a pixel.
// (2) PSNR and mask IoU of lib/metrics.py:30-45 / 79-94 (the monitors of the inversion loop, run.py:2077-2090,
//     2247): range check, clamp, per-image mean squared error -> -10 log10, clamp at 60 dB; thresholded masks ->
//     (intersection + 1e-6) / (union + 1e-6).  One launch, one block per image, no intermediate tensors.
// (3) SSIM of lib/metrics.py:48-76 (called beside them, run.py:2076-2088, 1275-1283): range check, clamp, the five 7 x 7
//     box sums formed separably in LDS per tile of window centres, one partial per block, an ordered finish.

struct WarpParams {
  const float* img; float* out;            // [N,C,H,W]
  const float* g_out; float* g_img;        // backward
  const float* rot; const float* scale; const float* trans;   // [N], [N] (or null = 1), [N,2]
  int N, C, H, W;
  int white;                               // 1: warp (img - 1), add 1 afterwards
};

// mat_scaled of augment_impl (run.py:745-752) for image n: rows (a0, a1, a2), (b0, b1, b2)
__device__ __forceinline__ void warp_matrix(const WarpParams& k, int n, float (&a)[3], float (&b)[3]) {
  const float r = k.rot[n], sc = k.scale ? k.scale[n] : 1.0f;
  const float c = cosf(r), s = sinf(r);
  const float tx = k.trans[2 * n], ty = -k.trans[2 * n + 1];
  a[0] = c * sc; a[1] = -s * sc; b[0] = s * sc; b[1] = c * sc;
  const float u0 = tx * sc, u1 = ty * sc;
  a[2] = c * u0 + (-s) * u1;               // sum_j mat[i][j] * mat_scaled[j][2]
  b[2] = s * u0 + c * u1;
}

// source position (unnormalised, align_corners=False) of output pixel (y, x)
__device__ __forceinline__ void warp_source(const WarpParams& k, const float (&a)[3], const float (&b)[3], int y, int x,
                                            int& x0, int& y0, float& fx, float& fy) {
  // affine_grid base coordinates: linspace(-1, 1, W) * (W - 1) / W  ==  (2 j + 1) / W - 1
  const float xs = (2.0f * (float)x + 1.0f) / (float)k.W - 1.0f;
  const float ys = (2.0f * (float)y + 1.0f) / (float)k.H - 1.0f;
  const float gx = (a[0] * xs + a[1] * ys) + a[2];
  const float gy = (b[0] * xs + b[1] * ys) + b[2];
  const float ix = ((gx + 1.0f) * (float)k.W - 1.0f) / 2.0f;
  const float iy = ((gy + 1.0f) * (float)k.H - 1.0f) / 2.0f;
  const float flx = floorf(ix), fly = floorf(iy);
  // keep the int conversion defined for far-away samples (they contribute zeros)
  x0 = (int)fminf(fmaxf(flx, -2.0f), (float)k.W);
  y0 = (int)fminf(fmaxf(fly, -2.0f), (float)k.H);
  fx = ix - flx; fy = iy - fly;
  if (flx < -2.0f || flx > (float)k.W) fx = 0.0f;
  if (fly < -2.0f || fly > (float)k.H) fy = 0.0f;
}

template <bool BWD>
__global__ __launch_bounds__(256) void affine_warp_kernel(WarpParams k) {
  __shared__ float mat[6];
  const int n = blockIdx.y;
  if (threadIdx.x == 0) {
    float a[3], b[3];
    warp_matrix(k, n, a, b);
    mat[0] = a[0]; mat[1] = a[1]; mat[2] = a[2]; mat[3] = b[0]; mat[4] = b[1]; mat[5] = b[2];
  }
  __syncthreads();
  const float a[3] = {mat[0], mat[1], mat[2]}, b[3] = {mat[3], mat[4], mat[5]};
  const int hw = k.H * k.W;
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= hw) return;
  const int y = pix / k.W, x = pix - y * k.W;
  int x0, y0;
  float fx, fy;
  warp_source(k, a, b, y, x, x0, y0, fx, fy);
  const bool vx0 = x0 >= 0 && x0 < k.W, vx1 = x0 + 1 >= 0 && x0 + 1 < k.W;
  const bool vy0 = y0 >= 0 && y0 < k.H, vy1 = y0 + 1 >= 0 && y0 + 1 < k.H;
  const float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
  const int o00 = y0 * k.W + x0;
  const float bgv = k.white ? 1.0f : 0.0f;
  for (int c = 0; c < k.C; ++c) {
    const size_t plane = ((size_t)n * k.C + c) * hw;
    if (!BWD) {
      const float* src = k.img + plane;
      float acc = 0.0f;
      if (vx0 && vy0) acc += w00 * (src[o00] - bgv);
      if (vx1 && vy0) acc += w10 * (src[o00 + 1] - bgv);
      if (vx0 && vy1) acc += w01 * (src[o00 + k.W] - bgv);
      if (vx1 && vy1) acc += w11 * (src[o00 + k.W + 1] - bgv);
      k.out[plane + pix] = acc + bgv;
    } else {
      const float g = k.g_out[plane + pix];
      float* dst = k.g_img + plane;
      if (g != 0.0f) {
        if (vx0 && vy0 && w00 != 0.0f) unsafeAtomicAdd(dst + o00, w00 * g);
        if (vx1 && vy0 && w10 != 0.0f) unsafeAtomicAdd(dst + o00 + 1, w10 * g);
        if (vx0 && vy1 && w01 != 0.0f) unsafeAtomicAdd(dst + o00 + k.W, w01 * g);
        if (vx1 && vy1 && w11 != 0.0f) unsafeAtomicAdd(dst + o00 + k.W + 1, w11 * g);
      }
    }
  }
}

// The adjoint as a gather (nfi_affine_warp_bwd_ordered): one thread per SOURCE pixel (n, sy, sx) is the only writer of
// g_img there.  It walks, row-major, the output pixels whose bilinear footprint can reach it - the inverse affine image
// of the source square [sx-1, sx+1] x [sy-1, sy+1], widened for fp32 rounding and clipped to the image - recomputes
// warp_source for each (so the weights, clamped far-away samples included, are the forward's bits) and adds w * g where
// one of the candidate's corners is this pixel.  The window only has to be a superset: membership is decided by the
// recomputed (x0, y0).  It is bounded by the image alone (a strong zoom-out sends many outputs to one source pixel; a
// singular or non-finite matrix gives the whole image).  No atomics, one store per element.
constexpr int kWarpGatherChannels = 8;     // accumulators per pass over the window (C = 6 or 8 in the inversion loss)

__global__ __launch_bounds__(256) void affine_warp_bwd_gather_kernel(WarpParams k) {
  __shared__ float mat[6];
  const int n = blockIdx.y;
  if (threadIdx.x == 0) {
    float a[3], b[3];
    warp_matrix(k, n, a, b);
    mat[0] = a[0]; mat[1] = a[1]; mat[2] = a[2]; mat[3] = b[0]; mat[4] = b[1]; mat[5] = b[2];
  }
  __syncthreads();
  const float a[3] = {mat[0], mat[1], mat[2]}, b[3] = {mat[3], mat[4], mat[5]};
  const int hw = k.H * k.W;
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= hw) return;
  const int sy = pix / k.W, sx = pix - sy * k.W;
  // inverse map, source position (ix, iy) -> output position (ox, oy), both in pixels
  const float det = a[0] * b[1] - a[1] * b[0];
  const float fW = (float)k.W, fH = (float)k.H;
  float min_x = INFINITY, max_x = -INFINITY, min_y = INFINITY, max_y = -INFINITY;
#pragma unroll
  for (int corner = 0; corner < 4; ++corner) {
    const float ix = (float)(sx + ((corner & 1) ? 1 : -1)), iy = (float)(sy + ((corner & 2) ? 1 : -1));
    const float gx = (2.0f * ix + 1.0f) / fW - 1.0f - a[2], gy = (2.0f * iy + 1.0f) / fH - 1.0f - b[2];
    const float xs = (b[1] * gx - a[1] * gy) / det, ys = (a[0] * gy - b[0] * gx) / det;
    const float ox = ((xs + 1.0f) * fW - 1.0f) * 0.5f, oy = ((ys + 1.0f) * fH - 1.0f) * 0.5f;
    // a NaN must widen the window, not be dropped by fminf / fmaxf
    min_x = (ox == ox) ? fminf(min_x, ox) : -INFINITY; max_x = (ox == ox) ? fmaxf(max_x, ox) : INFINITY;
    min_y = (oy == oy) ? fminf(min_y, oy) : -INFINITY; max_y = (oy == oy) ? fmaxf(max_y, oy) : INFINITY;
  }
  // rounding of the forward's (ix, iy) and of the inverse above: a few ulp of the largest intermediate, (|row| + 1) * size,
  // seen through the inverse map (1 / sqrt(det) output pixels per source pixel); floorf / ceilf below round outwards
  const float reach = fabsf(a[0]) + fabsf(a[1]) + fabsf(a[2]) + fabsf(b[0]) + fabsf(b[1]) + fabsf(b[2]) + 2.0f;
  const float margin = 0.01f + 1e-5f * reach * fmaxf(fW, fH) * rsqrtf(det);        // NaN / inf -> whole image below
  const int x_lo = (int)fminf(fmaxf(floorf(min_x - margin), 0.0f), fW), x_hi = (int)fmaxf(fminf(ceilf(max_x + margin), fW - 1.0f), -1.0f);
  const int y_lo = (int)fminf(fmaxf(floorf(min_y - margin), 0.0f), fH), y_hi = (int)fmaxf(fminf(ceilf(max_y + margin), fH - 1.0f), -1.0f);
  for (int c0 = 0; c0 < k.C; c0 += kWarpGatherChannels) {
    const int nc = min(kWarpGatherChannels, k.C - c0);
    const size_t plane0 = ((size_t)n * k.C + c0) * hw;
    float acc[kWarpGatherChannels];
#pragma unroll
    for (int c = 0; c < kWarpGatherChannels; ++c) acc[c] = 0.0f;
    for (int y = y_lo; y <= y_hi; ++y) {
      for (int x = x_lo; x <= x_hi; ++x) {
        int x0, y0;
        float fx, fy;
        warp_source(k, a, b, y, x, x0, y0, fx, fy);
        const bool at_x0 = x0 == sx, at_y0 = y0 == sy;
        if (!(at_x0 || x0 + 1 == sx) || !(at_y0 || y0 + 1 == sy)) continue;
        const float w = (at_x0 ? 1.0f - fx : fx) * (at_y0 ? 1.0f - fy : fy);     // the forward's w00 / w10 / w01 / w11
        const float* gp = k.g_out + plane0 + (size_t)y * k.W + x;
#pragma unroll
        for (int c = 0; c < kWarpGatherChannels; ++c)
          if (c < nc) acc[c] += w * gp[(size_t)c * hw];
      }
    }
#pragma unroll
    for (int c = 0; c < kWarpGatherChannels; ++c)
      if (c < nc) k.g_img[plane0 + (size_t)c * hw + pix] = acc[c];
  }
}

static int warp_common(const nfi_warp_args* a, WarpParams& k) {
  REQUIRE(a && a->rot && a->translation, "affine_warp: null pointer");
  REQUIRE(a->n_images > 0 && a->channels > 0 && a->height > 0 && a->width > 0, "affine_warp: bad shape");
  REQUIRE((int64_t)a->height * a->width < ((int64_t)1 << 30), "affine_warp: image too large");
  memset(&k, 0, sizeof(k));
  k.rot = a->rot; k.scale = a->scale; k.trans = a->translation;
  k.N = a->n_images; k.C = a->channels; k.H = a->height; k.W = a->width; k.white = a->white_background;
  return NFI_OK;
}

extern "C" int nfi_affine_warp_fwd(const nfi_warp_args* a, nfi_stream_t stream) {
  WarpParams k;
  int rc = warp_common(a, k);
  if (rc) return rc;
  REQUIRE(a->image && a->warped, "affine_warp_fwd: null image pointer");
  k.img = a->image; k.out = a->warped;
  dim3 grid((unsigned)((k.H * k.W + 255) / 256), (unsigned)k.N);
  hipLaunchKernelGGL(affine_warp_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, k);
  return check_launch("affine_warp_fwd");
}

extern "C" int nfi_affine_warp_bwd(const nfi_warp_args* a, nfi_stream_t stream) {
  WarpParams k;
  int rc = warp_common(a, k);
  if (rc) return rc;
  REQUIRE(a->g_warped && a->g_image, "affine_warp_bwd: null gradient pointer");
  k.g_out = a->g_warped; k.g_img = a->g_image;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(a->g_image, 0, sizeof(float) * (size_t)k.N * k.C * k.H * k.W, s) != hipSuccess)
    return fail(NFI_ERR_LAUNCH, "affine_warp_bwd: memset failed");
  dim3 grid((unsigned)((k.H * k.W + 255) / 256), (unsigned)k.N);
  hipLaunchKernelGGL(affine_warp_kernel<true>, grid, dim3(256), 0, s, k);
  return check_launch("affine_warp_bwd");
}

extern "C" int nfi_affine_warp_bwd_ordered(const nfi_warp_args* a, nfi_stream_t stream) {
  WarpParams k;
  int rc = warp_common(a, k);
  if (rc) return rc;
  REQUIRE(a->g_warped && a->g_image, "affine_warp_bwd_ordered: null gradient pointer");
  k.g_out = a->g_warped; k.g_img = a->g_image;
  dim3 grid((unsigned)((k.H * k.W + 255) / 256), (unsigned)k.N);
  hipLaunchKernelGGL(affine_warp_bwd_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, k);
  return check_launch("affine_warp_bwd_ordered");
}

// ------------------------------------------------------------------------------------------------
// image metrics: one block per image
// ------------------------------------------------------------------------------------------------
struct MetricParams {
  const float* pred; const float* target; int64_t per_image;          // psnr: any layout, per_image elements each
  const float* mask_pred; const float* mask_real; int64_t per_mask;   // iou
  float* psnr; float* iou; int* out_of_range;
};

__global__ __launch_bounds__(256) void image_metrics_kernel(MetricParams k) {
  __shared__ double red[4];
  const int img = blockIdx.x;
  int bad = 0;
  // lib/metrics.py range_check: values must lie in (-0.1, 1.1)
  auto in_range = [&](float v) { if (!(v < 1.1f) || !(v > -0.1f)) bad = 1; };
  if (k.psnr) {
    const float* p = k.pred + (size_t)img * k.per_image;
    const float* t = k.target + (size_t)img * k.per_image;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < k.per_image; i += blockDim.x) {
      const float a = p[i], b = t[i];
      in_range(a); in_range(b);
      const float d = fminf(fmaxf(a, 0.0f), 1.0f) - fminf(fmaxf(b, 0.0f), 1.0f);
      acc += (double)(d * d);
    }
    acc = block_sum_f64(acc, red);
    if (threadIdx.x == 0) {
      const float mse = (float)(acc / (double)k.per_image);
      const float v = -10.0f * log10f(mse);
      k.psnr[img] = fminf(v, 60.0f);        // clamp(max=60): NaN stays NaN
    }
  }
  if (k.iou) {
    const float* p = k.mask_pred + (size_t)img * k.per_mask;
    const float* t = k.mask_real + (size_t)img * k.per_mask;
    double inter = 0.0, uni = 0.0;
    for (int64_t i = threadIdx.x; i < k.per_mask; i += blockDim.x) {
      const float a = p[i], b = t[i];
      in_range(a); in_range(b);
      const bool pa = a > 0.5f, pb = b > 0.5f;
      inter += (pa && pb) ? 1.0 : 0.0;
      uni += (pa || pb) ? 1.0 : 0.0;
    }
    inter = block_sum_f64(inter, red);
    uni = block_sum_f64(uni, red);
    if (threadIdx.x == 0) k.iou[img] = ((float)inter + 1e-6f) / ((float)uni + 1e-6f);
  }
  if (k.out_of_range && bad) atomicOr(k.out_of_range, 1);
}

extern "C" int nfi_image_metrics(const nfi_metrics_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->n_images > 0, "image_metrics: bad shape");
  REQUIRE(a->psnr || a->iou, "image_metrics: nothing requested");
  REQUIRE(!a->psnr || (a->pred && a->target && a->elements_per_image > 0), "image_metrics: psnr inputs missing");
  REQUIRE(!a->iou || (a->mask_pred && a->mask_real && a->elements_per_mask > 0), "image_metrics: iou inputs missing");
  hipStream_t s = (hipStream_t)stream;
  if (a->out_of_range && hipMemsetAsync(a->out_of_range, 0, sizeof(int), s) != hipSuccess)
    return fail(NFI_ERR_LAUNCH, "image_metrics: memset failed");
  MetricParams k{a->pred, a->target, a->elements_per_image, a->mask_pred, a->mask_real, a->elements_per_mask,
                 a->psnr, a->iou, a->out_of_range};
  hipLaunchKernelGGL(image_metrics_kernel, dim3((unsigned)a->n_images), dim3(256), 0, s, k);
  return check_launch("image_metrics");
}

// ------------------------------------------------------------------------------------------------
// SSIM (lib/metrics.py:48-76): one block per (image, channel, tile of window centres), then one wave per image
// ------------------------------------------------------------------------------------------------
constexpr int kSsimWin = 7, kSsimHalo = kSsimWin - 1;
// A tile of 16 x 32 window centres: a half wave (the unit of LDS banking for 4-byte reads) walks one row of 32 consecutive
// words in both passes, so neither pass has a bank conflict; 20.8 KB of LDS per block leaves 7 blocks (28 waves) on a CU.
constexpr int kSsimTileH = 16, kSsimTileW = 32;
constexpr int kSsimInH = kSsimTileH + kSsimHalo, kSsimInW = kSsimTileW + kSsimHalo;        // 22 x 38 staged pixels
static_assert(kSsimTileW == 32 && kSsimTileH * kSsimTileW == 2 * 256, "ssim_tile_kernel: two window centres per thread, 32 per row");

struct SsimParams {
  const float* pred; const float* target;
  size_t pred_image, pred_channel, pred_row, pred_pixel;          // element strides of (image, channel, row, column)
  size_t target_image, target_channel, target_row, target_pixel;
  int H, W, tiles_x, tiles;                                        // tiles = tiles_x * tiles_y, per image and channel
  double* partial;                                                 // [B,3,tiles]
  float* map;                                                      // [B,3,H-6,W-6] or null
  float* ssim;                                                     // [B]
  int* out_of_range;
};

static void ssim_strides(int layout, int H, int W, size_t& image, size_t& channel, size_t& row, size_t& pixel) {
  image = (size_t)3 * H * W;
  if (layout == 0) { channel = (size_t)H * W; row = (size_t)W; pixel = 1; }
  else { channel = 1; row = (size_t)3 * W; pixel = 3; }
}

__global__ __launch_bounds__(256) void ssim_tile_kernel(SsimParams k) {
  __shared__ float sx[kSsimInH][kSsimInW], sy[kSsimInH][kSsimInW];
  __shared__ float rows[5][kSsimInH][kSsimTileW];                  // the five sums over 7 columns, per staged row
  __shared__ double red[4];
  const int tile = blockIdx.x % k.tiles, plane = blockIdx.x / k.tiles;        // plane = image * 3 + channel
  const int img = plane / 3, ch = plane - 3 * img;
  const int y0 = (tile / k.tiles_x) * kSsimTileH, x0 = (tile % k.tiles_x) * kSsimTileW;
  const float* X = k.pred + (size_t)img * k.pred_image + (size_t)ch * k.pred_channel;
  const float* Y = k.target + (size_t)img * k.target_image + (size_t)ch * k.target_channel;
  auto unit = [](float v) { return fminf(fmaxf(v, 0.0f), 1.0f); };
  // The sums are taken of (value - pivot), the pivot being the tile's own middle pixel: variances and the covariance do not
  // move with a shift, and on a flat background every term is exactly 0 where sum(x^2)/49 - mean^2 would cancel to noise of
  // the size of C2.  The pivot depends on the image and the tile alone, never on the batch.
  const int py = min(y0 + kSsimInH / 2, k.H - 1), px = min(x0 + kSsimInW / 2, k.W - 1);
  const float pivot_x = unit(X[(size_t)py * k.pred_row + (size_t)px * k.pred_pixel]);
  const float pivot_y = unit(Y[(size_t)py * k.target_row + (size_t)px * k.target_pixel]);
  int bad = 0;
  for (int i = threadIdx.x; i < kSsimInH * kSsimInW; i += 256) {
    const int r = i / kSsimInW, c = i - r * kSsimInW;
    const int gy = y0 + r, gx = x0 + c;
    float a = 0.0f, b = 0.0f;
    if (gy < k.H && gx < k.W) {
      const float xv = X[(size_t)gy * k.pred_row + (size_t)gx * k.pred_pixel];
      const float yv = Y[(size_t)gy * k.target_row + (size_t)gx * k.target_pixel];
      // lib/metrics.py range_check: values must lie in (-0.1, 1.1); a NaN fails both comparisons
      if (!(xv < 1.1f) || !(xv > -0.1f) || !(yv < 1.1f) || !(yv > -0.1f)) bad = 1;
      a = unit(xv) - pivot_x;
      b = unit(yv) - pivot_y;
    }
    sx[r][c] = a;
    sy[r][c] = b;
  }
  if (k.out_of_range && bad) atomicOr(k.out_of_range, 1);
  __syncthreads();
  for (int i = threadIdx.x; i < kSsimInH * kSsimTileW; i += 256) {
    const int r = i >> 5, c = i & 31;
    float s_x = 0.0f, s_y = 0.0f, s_xx = 0.0f, s_yy = 0.0f, s_xy = 0.0f;
#pragma unroll
    for (int j = 0; j < kSsimWin; ++j) {
      const float a = sx[r][c + j], b = sy[r][c + j];
      s_x += a; s_y += b; s_xx += a * a; s_yy += b * b; s_xy += a * b;
    }
    rows[0][r][c] = s_x; rows[1][r][c] = s_y; rows[2][r][c] = s_xx; rows[3][r][c] = s_yy; rows[4][r][c] = s_xy;
  }
  __syncthreads();
  // each thread: the window centres (oy, ox) and (oy + 1, ox), which share six of their seven rows
  const int ox = threadIdx.x & 31, oy = 2 * (threadIdx.x >> 5);
  float lo[5], hi[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    float mid = rows[q][oy + 1][ox];
#pragma unroll
    for (int j = 2; j < kSsimWin; ++j) mid += rows[q][oy + j][ox];
    lo[q] = rows[q][oy][ox] + mid;
    hi[q] = mid + rows[q][oy + kSsimWin][ox];
  }
  const int out_h = k.H - kSsimHalo, out_w = k.W - kSsimHalo;
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float* s = t ? hi : lo;
    const int gy = y0 + oy + t, gx = x0 + ox;
    if (gy < out_h && gx < out_w) {
      const float n = (float)(kSsimWin * kSsimWin), c1 = 1e-4f, c2 = 9e-4f;      // (0.01 R)^2, (0.03 R)^2 at data_range R = 1
      const float mx = s[0] / n, my = s[1] / n;
      const float ux = pivot_x + mx, uy = pivot_y + my;
      const float vx = (s[2] - s[0] * mx) / (n - 1.0f), vy = (s[3] - s[1] * my) / (n - 1.0f), vxy = (s[4] - s[0] * my) / (n - 1.0f);
      const float v = ((2.0f * ux * uy + c1) * (2.0f * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
      if (k.map) k.map[((size_t)plane * out_h + gy) * out_w + gx] = v;
      acc += (double)v;
    }
  }
  acc = block_sum_f64(acc, red);
  if (threadIdx.x == 0) k.partial[blockIdx.x] = acc;
}

// One wave per image adds that image's partials, channel by channel: lane l takes tiles l, l + 64, ... in that order, then
// the lanes are combined by the same butterfly every time.
__global__ __launch_bounds__(64) void ssim_finish_kernel(SsimParams k) {
  const int img = blockIdx.x;
  const double count = (double)(k.H - kSsimHalo) * (double)(k.W - kSsimHalo);
  double value = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    const double* p = k.partial + ((size_t)img * 3 + ch) * k.tiles;
    double v = 0.0;
    for (int i = threadIdx.x; i < k.tiles; i += 64) v += p[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    value += v / count;
  }
  if (threadIdx.x == 0) k.ssim[img] = (float)(value / 3.0);
}

// tiles per (image, channel), or 0 for a shape nfi_image_ssim refuses
static int64_t ssim_tiles(const nfi_ssim_args* a, int* tiles_x) {
  if (!a || a->n_images < 1 || a->height < kSsimWin || a->width < kSsimWin) return 0;
  const int64_t tx = (a->width - kSsimHalo + kSsimTileW - 1) / kSsimTileW, ty = (a->height - kSsimHalo + kSsimTileH - 1) / kSsimTileH;
  if (tx * ty * 3 * a->n_images >= ((int64_t)1 << 31)) return 0;
  if (tiles_x) *tiles_x = (int)tx;
  return tx * ty;
}

extern "C" size_t nfi_image_ssim_workspace_bytes(const nfi_ssim_args* a) {
  return (size_t)ssim_tiles(a, nullptr) * 3 * (a ? (size_t)a->n_images : 0) * sizeof(double);
}

extern "C" int nfi_image_ssim(const nfi_ssim_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->pred && a->target && a->ssim, "image_ssim: null pointer");
  REQUIRE(a->n_images >= 1, "image_ssim: n_images must be at least 1");
  REQUIRE(a->height >= kSsimWin && a->width >= kSsimWin, "image_ssim: height and width must hold one 7 x 7 window");
  REQUIRE((a->pred_layout == 0 || a->pred_layout == 1) && (a->target_layout == 0 || a->target_layout == 1),
          "image_ssim: layout must be 0 ([B,3,H,W]) or 1 ([B,H,W,3])");
  SsimParams k;
  memset(&k, 0, sizeof(k));
  k.tiles = (int)ssim_tiles(a, &k.tiles_x);
  REQUIRE(k.tiles > 0, "image_ssim: more than 2^31 tiles");
  REQUIRE(a->workspace, "image_ssim: workspace missing");
  REQUIRE(a->workspace_bytes >= nfi_image_ssim_workspace_bytes(a), "image_ssim: workspace too small");
  REQUIRE(((uintptr_t)a->workspace & 7) == 0, "image_ssim: workspace must be 8-byte aligned");
  k.pred = a->pred; k.target = a->target; k.H = a->height; k.W = a->width;
  ssim_strides(a->pred_layout, k.H, k.W, k.pred_image, k.pred_channel, k.pred_row, k.pred_pixel);
  ssim_strides(a->target_layout, k.H, k.W, k.target_image, k.target_channel, k.target_row, k.target_pixel);
  k.partial = (double*)a->workspace; k.map = a->ssim_map; k.ssim = a->ssim; k.out_of_range = a->out_of_range;
  hipStream_t s = (hipStream_t)stream;
  if (a->out_of_range && hipMemsetAsync(a->out_of_range, 0, sizeof(int), s) != hipSuccess)
    return fail(NFI_ERR_LAUNCH, "image_ssim: memset failed");
  hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(k.tiles * 3 * a->n_images)), dim3(256), 0, s, k);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)a->n_images), dim3(64), 0, s, k);
  return check_launch("image_ssim");
}
