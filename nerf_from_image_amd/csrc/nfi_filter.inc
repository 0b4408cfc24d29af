// nfi_filter.inc — zero-padded, same-size separable correlation of an image batch: the progressive discriminator blur,
// lib/ops.py:29-55 (filt2d with a 1-D kernel, blur).  Included by nfi_modules.hip.
//
// One launch does both passes.  A block owns one tile of kFilterTileH x kFilterTileW output pixels of one (image, channel)
// plane: it stages the tile and its halo of `radius` pixels (input - background, 0 outside the image) in LDS, filters the
// rows into a second LDS array, then filters the columns of that array and writes output + background.
//
// The tile, 32 x 32 at 256 threads.  With r = 30 a band of T rows filters T + 60 rows in the row pass, so a pixel costs
// ((T + 60) / T + 1) x 61 multiply-adds: 3.9 x 61 at T = 32, 2.9 x 61 at T = 64, 6.8 x 61 at T = 16.  A tile of 64 rows would
// save a quarter of that, but the batch this is for - one replica's discriminator batch, 4 images of 4 channels at 128 x 128
// - is 256 tiles of 32 x 32, one per CU of the MI355X, and only 128 of 64 x 32: half the CUs idle and each busy one with
// 1.5 x the work.  One plane per block would be 16 blocks.  LDS: (32 + 60) x 93 + (32 + 60) x 33 + 2 x 61 floats = 46.9 KB,
// three blocks (12 waves) on the CU's 160 KB.
// Banks (64 x 4 B; a half wave of 32 lanes is served together): in the row pass a thread slides along 4 adjacent columns,
// 8 threads cover a row of the tile and 4 rows make a half wave; at the odd pitches 93 and 33 the 4 rows start 1, 2 and 3
// banks (mod 4) apart, so the 32 addresses 4 c + pitch * row fall into 32 different banks, for the reads and the writes.  In
// the column pass a half wave reads and writes 32 consecutive words.
// Per 4 multiply-adds a thread reads one sample and one tap (a broadcast) from LDS.
//
// Sums: one accumulator per output, taps applied in index order with fmaf in both passes - rows first, then columns.  No
// atomics, no workspace: the output repeats bit for bit.

namespace nfi_filter {

constexpr int kFilterMaxRadius = 30;
constexpr int kFilterTileH = 32, kFilterTileW = 32, kFilterThreads = 256;
constexpr int kFilterInH = kFilterTileH + 2 * kFilterMaxRadius, kFilterInW = kFilterTileW + 2 * kFilterMaxRadius;      // 92 x 92
constexpr int kFilterInPitch = kFilterInW + 1, kFilterMidPitch = kFilterTileW + 1;                                      // 93, 33
static_assert(kFilterTileW % 4 == 0 && kFilterTileH % 4 == 0, "separable_filter_kernel: 4 adjacent outputs per thread in either pass");
static_assert(kFilterTileW * (kFilterTileH / 4) == kFilterThreads, "separable_filter_kernel: the column pass is one step of the block");
static_assert(kFilterInPitch % 2 == 1 && kFilterMidPitch % 2 == 1, "separable_filter_kernel: odd pitches keep the row pass off shared banks");

struct FilterParams {
  const float* image; float* out;
  size_t image_stride, channel_stride, row_stride, pixel_stride;          // of the input, in elements
  int C, H, W, tiles_x, tiles;                                              // tiles = tiles_x * tiles_y, per plane
  int radius, flip;
  const float* taps;                                                        // [2 radius + 1] or null: from sigma
  float sigma, background;
};

__global__ __launch_bounds__(kFilterThreads) void separable_filter_kernel(FilterParams k) {
  __shared__ float in[kFilterInH][kFilterInPitch];
  __shared__ float mid[kFilterInH][kFilterMidPitch];
  __shared__ float taps[2 * kFilterMaxRadius + 1], raw[2 * kFilterMaxRadius + 1];
  const int r = k.radius, n_taps = 2 * r + 1;
  const int tile = blockIdx.x % k.tiles, plane = blockIdx.x / k.tiles;      // plane = image * C + channel
  const int img = plane / k.C, ch = plane - img * k.C;
  const int y0 = (tile / k.tiles_x) * kFilterTileH, x0 = (tile % k.tiles_x) * kFilterTileW;
  const int out_h = min(kFilterTileH, k.H - y0), out_w = min(kFilterTileW, k.W - x0);        // >= 1: the tile starts inside
  const int col_groups = (out_w + 3) >> 2;                                  // groups of 4 columns the row pass forms
  const int in_h = out_h + 2 * r, in_w = 4 * col_groups + 2 * r;            // <= 92 x 92

  // taps: given ones as they are; else f[j] = exp2(-((j - r) / sigma)^2), added in the order j = 0 .. 2r, divided by the sum
  if (k.taps) {
    if ((int)threadIdx.x < n_taps) taps[k.flip ? n_taps - 1 - (int)threadIdx.x : (int)threadIdx.x] = k.taps[threadIdx.x];
  } else {                                                                  // (k.taps is the same for every thread)
    if ((int)threadIdx.x < n_taps) {
      const float x = (float)((int)threadIdx.x - r) / k.sigma;
      raw[threadIdx.x] = exp2f(-(x * x));
    }
    __syncthreads();
    if ((int)threadIdx.x < n_taps) {                                        // every thread adds all of them, in the same order
      float s = 0.0f;
      for (int j = 0; j < n_taps; ++j) s += raw[j];
      taps[k.flip ? n_taps - 1 - (int)threadIdx.x : (int)threadIdx.x] = raw[threadIdx.x] / s;
    }
  }

  // stage input - background; 0 outside the image, which is the reference's zero padding after its shift
  const float* src = k.image + (size_t)img * k.image_stride + (size_t)ch * k.channel_stride;
  for (int i = threadIdx.x; i < in_h * in_w; i += kFilterThreads) {
    const int row = i / in_w, col = i - row * in_w;
    const int gy = y0 - r + row, gx = x0 - r + col;
    float v = 0.0f;
    if (gy >= 0 && gy < k.H && gx >= 0 && gx < k.W) v = src[(size_t)gy * k.row_stride + (size_t)gx * k.pixel_stride] - k.background;
    in[row][col] = v;
  }
  __syncthreads();

  // rows: mid[row][x] = sum_j taps[j] in[row][x + j], 4 adjacent x per thread, the window sliding by one sample per tap
  for (int i = threadIdx.x; i < in_h * col_groups; i += kFilterThreads) {
    const int row = i / col_groups, c0 = 4 * (i - row * col_groups);
    const float* p = &in[row][c0];
    float w0 = p[0], w1 = p[1], w2 = p[2];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int j = 0; j < n_taps; ++j) {
      const float w3 = p[j + 3], t = taps[j];
      a0 = fmaf(t, w0, a0); a1 = fmaf(t, w1, a1); a2 = fmaf(t, w2, a2); a3 = fmaf(t, w3, a3);
      w0 = w1; w1 = w2; w2 = w3;
    }
    float* q = &mid[row][c0];
    q[0] = a0; q[1] = a1; q[2] = a2; q[3] = a3;
  }
  __syncthreads();

  // columns: out[y][x] = sum_j taps[j] mid[y + j][x], 4 adjacent y per thread.  Rows of mid past in_h hold nothing this
  // block wrote; they reach only accumulators of rows >= out_h, which are not stored (every index stays inside the array).
  const int ox = threadIdx.x % kFilterTileW, oy = 4 * (threadIdx.x / kFilterTileW);
  if (ox < out_w && oy < out_h) {
    float w0 = mid[oy][ox], w1 = mid[oy + 1][ox], w2 = mid[oy + 2][ox];
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < n_taps; ++j) {
      const float w3 = mid[oy + j + 3][ox], t = taps[j];
      a[0] = fmaf(t, w0, a[0]); a[1] = fmaf(t, w1, a[1]); a[2] = fmaf(t, w2, a[2]); a[3] = fmaf(t, w3, a[3]);
      w0 = w1; w1 = w2; w2 = w3;
    }
    float* dst = k.out + ((size_t)plane * k.H + (size_t)(y0 + oy)) * k.W + (size_t)(x0 + ox);
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (oy + d < out_h) dst[(size_t)d * k.W] = a[d] + k.background;
  }
}

// tiles per plane, or 0 where the grid would not fit: n_images * channels * tiles must stay below 2^31
static int64_t filter_tiles(const nfi_filter_args* a, int* tiles_x) {
  const int64_t tx = ((int64_t)a->width + kFilterTileW - 1) / kFilterTileW, ty = ((int64_t)a->height + kFilterTileH - 1) / kFilterTileH;
  if (tx * ty >= ((int64_t)1 << 31) || tx * ty * a->n_images * a->channels >= ((int64_t)1 << 31)) return 0;
  *tiles_x = (int)tx;
  return tx * ty;
}

}  // namespace nfi_filter

extern "C" int nfi_separable_filter(const nfi_filter_args* a, nfi_stream_t stream) {
  using namespace nfi_filter;
  REQUIRE(a, "separable_filter: null argument struct");
  REQUIRE(a->image && a->out, "separable_filter: null image / out");
  REQUIRE(a->n_images >= 1 && a->channels >= 1, "separable_filter: n_images and channels must be at least 1");
  REQUIRE(a->height >= 1 && a->width >= 1, "separable_filter: height and width must be at least 1");
  REQUIRE(a->layout == NFI_FILTER_BCHW || a->layout == NFI_FILTER_BHWC, "separable_filter: layout must be 0 ([B,C,H,W]) or 1 ([B,H,W,C])");
  REQUIRE(a->radius >= 1 && a->radius <= kFilterMaxRadius, "separable_filter: radius must be in [1,30]");
  REQUIRE(a->taps || a->sigma > 0.0f, "separable_filter: sigma must be positive when taps is null");
  FilterParams k;
  memset(&k, 0, sizeof(k));
  k.tiles = (int)filter_tiles(a, &k.tiles_x);
  REQUIRE(k.tiles > 0, "separable_filter: grid too large: n_images * channels * ceil(height / 32) * ceil(width / 32) must be below 2^31");
  k.image = a->image; k.out = a->out; k.C = a->channels; k.H = a->height; k.W = a->width;
  const size_t C = (size_t)a->channels, H = (size_t)a->height, W = (size_t)a->width;
  k.image_stride = C * H * W;
  if (a->layout == NFI_FILTER_BCHW) { k.channel_stride = H * W; k.row_stride = W; k.pixel_stride = 1; }
  else { k.channel_stride = 1; k.row_stride = C * W; k.pixel_stride = C; }
  k.radius = a->radius; k.flip = a->flip != 0; k.taps = a->taps; k.sigma = a->sigma; k.background = a->background;
  const unsigned blocks = (unsigned)((int64_t)k.tiles * a->n_images * a->channels);
  hipLaunchKernelGGL(separable_filter_kernel, dim3(blocks), dim3(kFilterThreads), 0, (hipStream_t)stream, k);
  return check_launch("separable_filter");
}
