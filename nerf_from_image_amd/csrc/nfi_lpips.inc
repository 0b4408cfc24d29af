// nfi_lpips.inc — the distance head of LPIPS, everything lib/metrics.py:104-110, 130-133 does AFTER the VGG convolutions, one
// layer per call: unit-normalise both feature maps over the channels, subtract, square, weigh the channels (the lin layer's
// 1x1 convolution to one channel) and take the spatial mean.  Included by nfi_modules.hip.
//
//   rx[b,p] = sqrt(sum_c x[b,c,p]^2)     xh = x / (rx + eps)        (eps is added to the norm, not put under the root)
//   ry, yh likewise; with y_normalized:  yh = y as given            (lib/metrics.py:126-128, cached features)
//   out[b]  = (1 / (H W)) sum_p sum_c w[c] (xh[b,c,p] - yh[b,c,p])^2
//
// Tiling.  A block of 256 threads owns one image and kLpipsTile = 64 consecutive flattened pixels: lane l of every wave is
// pixel p0 + l (hw is the contiguous axis, so a wave's load or store of one channel is 256 contiguous bytes), and wave v takes
// the channels v, v + 4, v + 8, ...  The per-pixel channel sums of the four waves meet in LDS (4 x 64 doubles per quantity,
// read back in wave order by every thread).  For C = 64 and C = 128 (CPL = 16, 32 channels per lane) a lane's x and y stay in
// registers between the sweeps and every feature is read ONCE; any other C >= 1 takes the CPL = 0 body, which reads the tile
// again in each sweep (twice forward, three times backward; the tile, at most C x 512 B, comes back from L2).
//
// Arithmetic.  The difference xh - yh is formed per element and then squared - never the expanded sum w x^2/rx^2 - 2 w x y/(rx ry)
// + w y^2/ry^2, which cancels where prediction and target agree: identical inputs give exactly 0.0f, and exactly zero
// gradients.  (The unit is built with -ffp-contract=off: x * ix - y * iy is two products and one subtraction, no fused step
// that would leave a rounding residue between two equal products.)  Channel sums, the difference and the products are float64;
// the kernel is bound by bytes.
//
// Forward: lpips_head_tile_kernel writes ONE float64 partial per block to the workspace; lpips_head_finish_kernel, one wave per
// image, adds an image's partials in index order and stores out[b] (or adds to it in float32: accumulate).  No float atomics,
// no memset, no allocation: the same bits on every launch, and an image's value does not depend on the batch around it.
//
// Backward: lpips_head_bwd_kernel, ONE launch on the same tiling, recomputes the norms (the forward stashes nothing).  With
// g = g_out[b] / (H W), q[c] = 2 w[c] (xh[c] - yh[c]):
//   g_x[b,k,p] = g (q[k] / (rx + eps) - x[k] (sum_c q[c] x[c]) / ((rx + eps)^2 rx))
//   g_y: the same with x <-> y and q -> -q;  with y_normalized: g_y = -g q[k]
// Every element is written exactly once, no atomics: bit-reproducible by construction.
// DEVIATION (DESIGN.md section 9): at a pixel whose whole channel vector is zero (rx == 0) the second term is taken as 0 - x[k]
// is 0 there - so the gradient is the finite g q[k] / eps; the reference's autograd returns NaN (0/0 in sqrt's backward).
//
// All element offsets are 64-bit: the first VGG tap of the inversion batch is 537 MB per side.

namespace nfi_lpips {

constexpr int kLpipsTile = 64, kLpipsThreads = 256, kLpipsWaves = kLpipsThreads / 64;
// Registers: four waves per SIMD asked for (at most 128 VGPRs).  The kernels use 61 / 87 (forward) and 64 / 94 (backward) at
// CPL = 16 / 32 and no scratch - with next_sweep() and settle() below; without either the compiler needs twice that.
constexpr int kLpipsWavesPerSimd = 4;
static_assert(kLpipsTile == 64, "lpips_head kernels: one pixel per lane");

struct LpipsParams {
  const float* x; const float* y; const float* w;
  int C, y_normalized, accumulate;
  int64_t hw, tiles;                                  // pixels per image, blocks per image
  double eps;
  float* out; double* partial;                        // forward
  const float* g_out; float* g_x; float* g_y;         // backward
};

// the wave's index in its block as a scalar: the channel index, the row addresses and the weights derived from it are then
// wave-uniform (row addresses in scalar registers, one shared 32-bit lane offset) - the compiler cannot tell from threadIdx.x >> 6
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// f(j, c) for each channel c of this wave, j counting them: c = 4 j + wave
template <int CPL, class F>
__device__ __forceinline__ void each_channel(int C, int wave, F&& f) {
  if constexpr (CPL > 0) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) f(j, kLpipsWaves * j + wave);
  } else {
    for (int c = wave, j = 0; c < C; c += kLpipsWaves, ++j) f(j, c);
  }
}

// A sum that only a branch below uses: without this the compiler sinks the whole accumulation into that branch and keeps every
// term's operands alive until there (128 more VGPRs at CPL = 32, or scratch under the occupancy bound)
__device__ __forceinline__ void settle(double& v) { asm volatile("" : "+v"(v)); }

// red[wave][lane] -> the four waves' values of this lane's pixel, added in wave order (every thread gets the same total)
__device__ __forceinline__ double across_waves(double v, double (*red)[kLpipsTile], int wave, int lane) {
  red[wave][lane] = v;
  __syncthreads();
  return ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// One block's view of its tile: the lane's pixel, its channels (in registers for CPL > 0), the norms.
template <int CPL>
struct LpipsTileView {
  const float* X; const float* Y;                     // at (image, channel 0, the tile's first pixel): the same in every lane
  size_t hw;
  unsigned lane;                                      // the lane's pixel within the tile
  bool valid;                                         // ... lies inside the image
  float xr[CPL > 0 ? CPL : 1], yr[CPL > 0 ? CPL : 1];

  // element (c, lane) of a tensor whose tile starts at `base`: a wave-uniform row address plus a 32-bit lane offset, so the
  // 2 x CPL loads and stores of a sweep share one address register (per-channel 64-bit addresses cost 128 VGPRs at CPL = 32)
  template <class T>
  __device__ __forceinline__ T* at(T* base, int c) const { return base + (size_t)c * hw + lane; }

  __device__ __forceinline__ void open(const LpipsParams& k, int64_t img, int64_t tile) {
    hw = (size_t)k.hw;
    lane = threadIdx.x & 63;
    const int wave = wave_index();
    valid = tile * kLpipsTile + lane < k.hw;
    const size_t first = (size_t)img * (size_t)k.C * hw + (size_t)tile * kLpipsTile;
    X = k.x + first; Y = k.y + first;
    if constexpr (CPL > 0)
      each_channel<CPL>(k.C, wave, [&](int j, int c) {
        xr[j] = valid ? *at(X, c) : 0.0f;
        yr[j] = valid ? *at(Y, c) : 0.0f;
      });
  }
  // Between two sweeps: the resident values pass through an empty asm, so the compiler must convert them to float64 again in
  // the next sweep.  Without it, it keeps the converted values alive - two registers for one - across the barrier and spills
  // under the occupancy bound (116 B of scratch forward, 556 B backward at CPL = 32).
  __device__ __forceinline__ void next_sweep() {
    if constexpr (CPL > 0) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) asm volatile("" : "+v"(xr[j]), "+v"(yr[j]));
    }
  }
  __device__ __forceinline__ double xv(int j, int c) const { return CPL > 0 ? (double)xr[j] : (valid ? (double)*at(X, c) : 0.0); }
  __device__ __forceinline__ double yv(int j, int c) const { return CPL > 0 ? (double)yr[j] : (valid ? (double)*at(Y, c) : 0.0); }
};

template <int CPL>
__global__ __launch_bounds__(kLpipsThreads, kLpipsWavesPerSimd) void lpips_head_tile_kernel(LpipsParams k) {
  __shared__ double red[2][kLpipsWaves][kLpipsTile];
  __shared__ double fin[4];
  const int lane = threadIdx.x & 63, wave = wave_index();
  const int64_t img = blockIdx.x / k.tiles, tile = blockIdx.x - img * k.tiles;
  LpipsTileView<CPL> t;
  t.open(k, img, tile);
  double sx = 0.0, sy = 0.0;
  each_channel<CPL>(k.C, wave, [&](int j, int c) {
    const double a = t.xv(j, c), b = t.yv(j, c);
    sx += a * a; sy += b * b;
  });
  settle(sy);
  sx = across_waves(sx, red[0], wave, lane);
  const double ix = 1.0 / (sqrt(sx) + k.eps);
  double iy = 1.0;
  if (!k.y_normalized) iy = 1.0 / (sqrt(across_waves(sy, red[1], wave, lane)) + k.eps);
  double acc = 0.0;
  t.next_sweep();
  each_channel<CPL>(k.C, wave, [&](int j, int c) {
    const double xh = t.xv(j, c) * ix, yh = t.yv(j, c) * iy;
    const double d = xh - yh;
    acc += (double)k.w[c] * (d * d);
  });
  acc = block_sum_f64(t.valid ? acc : 0.0, fin);
  if (threadIdx.x == 0) k.partial[blockIdx.x] = acc;
}

// One wave per image adds that image's partials: lane l takes tiles l, l + 64, ... in that order, then the lanes are combined
// by the same butterfly every time.
__global__ __launch_bounds__(64) void lpips_head_finish_kernel(LpipsParams k) {
  const double* p = k.partial + (size_t)blockIdx.x * (size_t)k.tiles;
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < k.tiles; i += 64) v += p[i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if (threadIdx.x == 0) {
    const float value = (float)(v / (double)k.hw);
    k.out[blockIdx.x] = k.accumulate ? k.out[blockIdx.x] + value : value;
  }
}

template <int CPL>
__global__ __launch_bounds__(kLpipsThreads, kLpipsWavesPerSimd) void lpips_head_bwd_kernel(LpipsParams k) {
  __shared__ double red[4][kLpipsWaves][kLpipsTile];
  const int lane = threadIdx.x & 63, wave = wave_index();
  const int64_t img = blockIdx.x / k.tiles, tile = blockIdx.x - img * k.tiles;
  LpipsTileView<CPL> t;
  t.open(k, img, tile);
  double sx = 0.0, sy = 0.0;
  each_channel<CPL>(k.C, wave, [&](int j, int c) {
    const double a = t.xv(j, c), b = t.yv(j, c);
    sx += a * a; sy += b * b;
  });
  settle(sy);
  const double rx = sqrt(across_waves(sx, red[0], wave, lane));
  const double ix = 1.0 / (rx + k.eps);
  double ry = 0.0, iy = 1.0;
  if (!k.y_normalized) { ry = sqrt(across_waves(sy, red[1], wave, lane)); iy = 1.0 / (ry + k.eps); }
  // q . x and q . y over the channels
  double qx = 0.0, qy = 0.0;
  t.next_sweep();
  each_channel<CPL>(k.C, wave, [&](int j, int c) {
    const double a = t.xv(j, c), b = t.yv(j, c);
    const double xh = a * ix, yh = b * iy;
    const double q = 2.0 * (double)k.w[c] * (xh - yh);
    qx += q * a; qy += q * b;
  });
  settle(qy);
  qx = across_waves(qx, red[2], wave, lane);
  const double kx = rx > 0.0 ? qx * ix * ix / rx : 0.0;            // rx == 0: every x[k] is 0, the term is taken as 0
  double ky = 0.0;
  if (!k.y_normalized && k.g_y) { qy = across_waves(qy, red[3], wave, lane); ky = ry > 0.0 ? qy * iy * iy / ry : 0.0; }
  if (!t.valid) return;                                            // (after the last barrier)
  const double g = (double)k.g_out[img] / (double)k.hw;
  const size_t first = (size_t)(t.X - k.x);
  float* GX = k.g_x ? k.g_x + first : nullptr;
  float* GY = k.g_y ? k.g_y + first : nullptr;
  t.next_sweep();
  each_channel<CPL>(k.C, wave, [&](int j, int c) {
    const double a = t.xv(j, c), b = t.yv(j, c);
    const double xh = a * ix, yh = b * iy;
    const double q = 2.0 * (double)k.w[c] * (xh - yh);
    // (+ 0.0f: a zero gradient is +0.0f whatever the signs of g and q)
    if (GX) *t.at(GX, c) = (float)(g * (q * ix - a * kx)) + 0.0f;
    if (GY) *t.at(GY, c) = (float)(k.y_normalized ? -(g * q) : -(g * (q * iy - b * ky))) + 0.0f;
  });
}

// blocks per image, or 0 for a shape the entries refuse (a dimension under 1, a grid of 2^31 blocks or more)
static int64_t lpips_tiles(const nfi_lpips_head_args* a) {
  if (!a || a->n_images < 1 || a->channels < 1 || a->height < 1 || a->width < 1) return 0;
  const int64_t hw = (int64_t)a->height * a->width, tiles = (hw + kLpipsTile - 1) / kLpipsTile;
  if (tiles * a->n_images >= ((int64_t)1 << 31)) return 0;
  return tiles;
}

static bool lpips_overlap(const float* a, const float* b, size_t n) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b, bytes = n * sizeof(float);
  return p < q + bytes && q < p + bytes;
}

// what both entries check, and the parameters both launches share
static int lpips_common(const nfi_lpips_head_args* a, LpipsParams& k) {
  REQUIRE(a, "lpips_head: null argument struct");
  REQUIRE(a->x && a->y && a->weight, "lpips_head: null x / y / weight");
  REQUIRE(a->n_images >= 1 && a->channels >= 1 && a->height >= 1 && a->width >= 1,
          "lpips_head: n_images, channels, height and width must be at least 1");
  REQUIRE(a->eps >= 0.0f, "lpips_head: eps must not be negative (or NaN)");
  memset(&k, 0, sizeof(k));
  k.tiles = lpips_tiles(a);
  REQUIRE(k.tiles > 0, "lpips_head: grid too large: n_images * ceil(height * width / 64) must be below 2^31");
  k.x = a->x; k.y = a->y; k.w = a->weight; k.C = a->channels; k.y_normalized = a->y_normalized != 0;
  k.hw = (int64_t)a->height * a->width; k.eps = (double)a->eps;
  return NFI_OK;
}

template <template <int> class Launch>
static void lpips_dispatch(const LpipsParams& k, unsigned blocks, hipStream_t s) {
  if (k.C == 16 * kLpipsWaves) Launch<16>::go(k, blocks, s);
  else if (k.C == 32 * kLpipsWaves) Launch<32>::go(k, blocks, s);
  else Launch<0>::go(k, blocks, s);
}
template <int CPL> struct LpipsFwd {
  static void go(const LpipsParams& k, unsigned blocks, hipStream_t s) { hipLaunchKernelGGL(lpips_head_tile_kernel<CPL>, dim3(blocks), dim3(kLpipsThreads), 0, s, k); }
};
template <int CPL> struct LpipsBwd {
  static void go(const LpipsParams& k, unsigned blocks, hipStream_t s) { hipLaunchKernelGGL(lpips_head_bwd_kernel<CPL>, dim3(blocks), dim3(kLpipsThreads), 0, s, k); }
};

}  // namespace nfi_lpips

extern "C" size_t nfi_lpips_head_workspace_bytes(const nfi_lpips_head_args* a) {
  return (size_t)nfi_lpips::lpips_tiles(a) * (a ? (size_t)a->n_images : 0) * sizeof(double);
}

extern "C" int nfi_lpips_head_fwd(const nfi_lpips_head_args* a, nfi_stream_t stream) {
  using namespace nfi_lpips;
  LpipsParams k;
  int rc = lpips_common(a, k);
  if (rc) return rc;
  REQUIRE(a->out, "lpips_head_fwd: null out");
  REQUIRE(a->workspace, "lpips_head_fwd: workspace missing");
  REQUIRE(a->workspace_bytes >= nfi_lpips_head_workspace_bytes(a), "lpips_head_fwd: workspace too small");
  REQUIRE(((uintptr_t)a->workspace & 7) == 0, "lpips_head_fwd: workspace must be 8-byte aligned");
  k.out = a->out; k.accumulate = a->accumulate != 0; k.partial = (double*)a->workspace;
  hipStream_t s = (hipStream_t)stream;
  lpips_dispatch<LpipsFwd>(k, (unsigned)(k.tiles * a->n_images), s);
  hipLaunchKernelGGL(lpips_head_finish_kernel, dim3((unsigned)a->n_images), dim3(64), 0, s, k);
  return check_launch("lpips_head_fwd");
}

extern "C" int nfi_lpips_head_bwd(const nfi_lpips_head_args* a, nfi_stream_t stream) {
  using namespace nfi_lpips;
  LpipsParams k;
  int rc = lpips_common(a, k);
  if (rc) return rc;
  REQUIRE(a->g_out, "lpips_head_bwd: null g_out");
  REQUIRE(a->g_x || a->g_y, "lpips_head_bwd: g_x and g_y are both null");
  const size_t n = (size_t)a->n_images * (size_t)a->channels * (size_t)k.hw;
  for (const float* g : {(const float*)a->g_x, (const float*)a->g_y})
    REQUIRE(!g || (!lpips_overlap(g, a->x, n) && !lpips_overlap(g, a->y, n)), "lpips_head_bwd: a gradient overlaps x or y");
  REQUIRE(!a->g_x || !a->g_y || !lpips_overlap(a->g_x, a->g_y, n), "lpips_head_bwd: g_x overlaps g_y");
  k.g_out = a->g_out; k.g_x = a->g_x; k.g_y = a->g_y;
  lpips_dispatch<LpipsBwd>(k, (unsigned)(k.tiles * a->n_images), (hipStream_t)stream);
  return check_launch("lpips_head_bwd");
}
