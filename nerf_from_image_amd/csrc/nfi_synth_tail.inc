// nfi_synth_tail.inc — everything SynthesisLayer.forward does AFTER its convolution, models/stylegan.py:101-105 (the 4x4
// resample filter of an `up` layer, filter2d with gain 4), 139-140 (addcmul(noise, x, dcoefs)), 351-355 (+ bias, * act_gain,
// leaky_relu), as one launch forward and at most two (+ one for the noise gradient) backward.  Included by nfi_modules.hip.
//
//   f   = up ? sum_{a,b} (4 taps[a][b]) y[i + a - 1, j + b - 1]  (0 outside y, which is [R+1, R+1])  :  y
//   out = lrelu(((noise + f * dcoefs[b,c]) + bias[c]) * act_gain)
//
// The filter's 16 products are added in float64 and rounded to float32 once.  Every operation after it is rounded on its
// own, in the order written (the unit is built with -ffp-contract=off): a layer without `up` gives the bits of the same
// float32 expression evaluated one operation at a time.
//
// Up layers.  A block owns one tile of 64 x 64 outputs of one (image, channel) plane and stages the tile's 67 x 67 inputs
// in LDS (pitch 68 floats: rows start 16-byte aligned), so y is read once - 1.10 x with the halo - and out is written once.
// A thread owns 4 adjacent columns and a band of rows: per output row it reads 8 floats (two 16-byte LDS reads) into a
// sliding window of 4 rows, does 4 x 16 float64 fma in tap order a, b, and stores one float4 (R % 4 == 0, every real layer) - a
// wave writes four full 256-byte row segments per store instruction.  The bands shrink with the plane (rows per thread =
// ceil(tile rows / 16)), so a 16 x 16 plane still runs 64 threads.  LDS 18.2 KB per block; HBM bytes per output: 4 read
// (4.4 with the halo), 4 written, against five or more round trips of the PyTorch chain.
//
// Backward of an up layer, on the tiles of the (R+1) x (R+1) grid of g_y: the block stages gs = g_out * (out > 0 ? 1 :
// slope) with a halo of 2 above / left and 1 below / right (and y, for g_dcoefs, with the forward's halo), forms
// g_y = act_gain dcoefs sum_{a,b} (4 taps[3-a][3-b]) gs[p + a - 2, q + b - 2] - the adjoint, in float64, rounded once - through an
// LDS tile so that the rows of the odd-pitched g_y are written as contiguous dwords, and adds its share of sum(gs) and
// sum(gs * f) in float64 (f unrounded); the gain is applied to the block's sums.
// The per-block sums go to the workspace as float64 pairs; a second launch adds them per (image, channel) and per channel
// in index order.  g_noise, when asked for, is a launch of its own: a block owns 64 (small planes: 16) adjacent pixels, its
// thread groups every 4th (16th) plane, float64 sums joined in group order.  No atomics anywhere: the same bits on every launch.
//
// Layers without `up` are flat: a block owns 4096 consecutive elements of one plane, float4 where R*R % 4 == 0.

namespace nfi_synth_tail {

constexpr int kTailTile = 64, kTailThreads = 256;
constexpr int kTailRows = kTailTile + 3, kTailPitch = kTailTile + 4;      // 67 rows of 68 floats
constexpr int kTailChunk = 4096;                                         // elements of a flat block: 4 float4 per thread
constexpr int kTailMaxRes = 16384;                                       // R * R and (R + 1)^2 stay inside an int
static_assert(kTailPitch % 4 == 0, "synth tail: LDS rows must start 16-byte aligned");
static_assert(kTailThreads == 16 * (kTailTile / 4), "synth tail: 16 column groups x 16 row bands");
static_assert(kTailChunk == 4 * 4 * kTailThreads, "synth tail: a flat block is 4 float4 per thread");

struct TailParams {
  const float* y; const float* dcoefs; const float* bias; const float* taps; const float* noise;
  float* out;                                                             // written by fwd, read by bwd
  const float* g_out; float* g_y; float* g_dcoefs; float* g_bias; float* g_noise;
  double* partials;                                                       // [B*C][tiles][2]: sum(gu * f), sum(gu)
  int B, C, R, N, tiles_x, tiles;                                         // N: side of y; tiles per plane of this launch
  int noise_shared, activate, vec;
  float gain, slope;
};

__device__ __forceinline__ float tail_epilogue(float f, float d, bool has_noise, float nz, float bs, const TailParams& k) {
  float t = f * d;
  if (has_noise) t = nz + t;
  t = t + bs;
  t = t * k.gain;
  if (k.activate) t = t > 0.0f ? t : t * k.slope;
  return t;
}
// gu = gs * act_gain with gs = g_out * (out > 0 ? 1 : slope).  The sums add gs in float64 and apply the gain once, at the end
__device__ __forceinline__ float tail_gs(float g, float o, const TailParams& k) {
  return (k.activate && !(o > 0.0f)) ? g * k.slope : g;
}
__device__ __forceinline__ double tail_gs_f64(float g, float o, const TailParams& k) {
  return (k.activate && !(o > 0.0f)) ? (double)g * (double)k.slope : (double)g;
}

// the thread's share of a tile: 4 columns from 4 * cg, rows [r0, r1)
struct TailShare { int cg, r0, r1; };
__device__ __forceinline__ TailShare tail_share(int th, int tw) {
  TailShare s;
  s.cg = threadIdx.x & 15;
  const int band = threadIdx.x >> 4, rpt = (th + 15) >> 4;
  s.r0 = band * rpt;
  s.r1 = 4 * s.cg < tw ? min(s.r0 + rpt, th) : s.r0;
  return s;
}
__device__ __forceinline__ void tail_load_row(float (&w)[8], const float (*lds)[kTailPitch], int row, int cg) {
  const float4 q0 = *reinterpret_cast<const float4*>(&lds[row][4 * cg]), q1 = *reinterpret_cast<const float4*>(&lds[row][4 * cg + 4]);
  w[0] = q0.x; w[1] = q0.y; w[2] = q0.z; w[3] = q0.w; w[4] = q1.x; w[5] = q1.y; w[6] = q1.z; w[7] = q1.w;
}
__device__ __forceinline__ void tail_slide(float (&w)[4][8]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int x = 0; x < 8; ++x) w[a][x] = w[a + 1][x];
}
// acc[x] = sum_{a,b} K[a][b] w[a][x + b]: float64 fma in the order a, b, rounded to float32 once - the filtered value is
// the correctly rounded one whatever the taps (v_fma_f64 runs at the rate of the unpacked v_fma_f32 here, and the
// kernels are bound by memory)
__device__ __forceinline__ void tail_window(double (&acc)[4], const double (&K)[4][4], const float (&w)[4][8]) {
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) s = fma(K[a][b], (double)w[a][x + b], s);
    acc[x] = s;
  }
}
// block sum of two doubles in a fixed order: shuffles inside a wave, then the four waves in index order.  Thread 0 has it.
__device__ __forceinline__ void tail_block_sum(double& u, double& v, double (*red)[4]) {
#pragma unroll
  for (int off = 32; off; off >>= 1) { u += __shfl_down(u, off); v += __shfl_down(v, off); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = u; red[1][threadIdx.x >> 6] = v; }
  __syncthreads();
  u = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  v = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

__global__ __launch_bounds__(kTailThreads) void tail_up_fwd_kernel(TailParams k) {
  __shared__ __attribute__((aligned(16))) float in[kTailRows][kTailPitch];
  const int tile = blockIdx.x % k.tiles, plane = blockIdx.x / k.tiles;      // plane = image * C + channel
  const int img = plane / k.C, ch = plane - img * k.C;
  const int y0 = (tile / k.tiles_x) * kTailTile, x0 = (tile % k.tiles_x) * kTailTile;
  const int R = k.R, N = k.N;
  const int th = min(kTailTile, R - y0), tw = min(kTailTile, R - x0);       // >= 1: the tile starts inside
  const int in_w = 4 * ((tw + 3) >> 2) + 4;                                 // the columns the threads read, <= 68
  double K[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) K[a][b] = (double)(4.0f * k.taps[4 * a + b]);

  const float* src = k.y + (size_t)plane * N * N;
  for (int i = threadIdx.x; i < (th + 3) * in_w; i += kTailThreads) {       // in[r][c] = y[y0 - 1 + r, x0 - 1 + c], 0 outside
    const int row = i / in_w, col = i - row * in_w;
    const int gy = y0 - 1 + row, gx = x0 - 1 + col;
    in[row][col] = (gy >= 0 && gy < N && gx >= 0 && gx < N) ? src[(size_t)gy * N + gx] : 0.0f;
  }
  __syncthreads();

  const TailShare s = tail_share(th, tw);
  if (s.r0 >= s.r1) return;
  const float d = k.dcoefs[plane], bs = k.bias[ch];
  const bool has_noise = k.noise != nullptr;
  const float* nz = has_noise ? k.noise + (k.noise_shared ? (size_t)0 : (size_t)img * R * R) : nullptr;
  float* dst = k.out + (size_t)plane * R * R;
  const int gx = x0 + 4 * s.cg;
  float w[4][8];
#pragma unroll
  for (int a = 1; a < 4; ++a) tail_load_row(w[a], in, s.r0 + a - 1, s.cg);
  for (int r = s.r0; r < s.r1; ++r) {
    tail_slide(w);
    tail_load_row(w[3], in, r + 3, s.cg);
    double acc64[4];
    tail_window(acc64, K, w);
    const float acc[4] = {(float)acc64[0], (float)acc64[1], (float)acc64[2], (float)acc64[3]};
    const size_t at = (size_t)(y0 + r) * R + gx;
    if (k.vec) {                                                            // R % 4 == 0: the 4 columns are all inside
      float4 n4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (has_noise) n4 = *reinterpret_cast<const float4*>(nz + at);
      float4 o;
      o.x = tail_epilogue(acc[0], d, has_noise, n4.x, bs, k); o.y = tail_epilogue(acc[1], d, has_noise, n4.y, bs, k);
      o.z = tail_epilogue(acc[2], d, has_noise, n4.z, bs, k); o.w = tail_epilogue(acc[3], d, has_noise, n4.w, bs, k);
      *reinterpret_cast<float4*>(dst + at) = o;
    } else {
#pragma unroll
      for (int x = 0; x < 4; ++x)
        if (gx + x < R) dst[at + x] = tail_epilogue(acc[x], d, has_noise, has_noise ? nz[at + x] : 0.0f, bs, k);
    }
  }
}

// the tiles here are those of g_y: (R+1) x (R+1), N = R + 1
__global__ __launch_bounds__(kTailThreads) void tail_up_bwd_kernel(TailParams k) {
  __shared__ __attribute__((aligned(16))) float gu[kTailRows][kTailPitch];
  __shared__ __attribute__((aligned(16))) float yy[kTailRows][kTailPitch];
  __shared__ float ob[kTailTile][kTailTile + 1];
  __shared__ double red[2][4];
  const int tile = blockIdx.x % k.tiles, plane = blockIdx.x / k.tiles;
  const int y0 = (tile / k.tiles_x) * kTailTile, x0 = (tile % k.tiles_x) * kTailTile;
  const int R = k.R, N = k.N;
  const int th = min(kTailTile, N - y0), tw = min(kTailTile, N - x0);
  const int in_w = 4 * ((tw + 3) >> 2) + 4;
  const bool want_sums = k.partials != nullptr, want_f = k.g_dcoefs != nullptr, want_gy = k.g_y != nullptr;
  double K[4][4], Kf[4][4];                                                 // Kf: the adjoint's taps
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) { K[a][b] = (double)(4.0f * k.taps[4 * a + b]); Kf[a][b] = (double)(4.0f * k.taps[4 * (3 - a) + (3 - b)]); }

  const float* g_src = k.g_out + (size_t)plane * R * R;
  const float* o_src = k.out + (size_t)plane * R * R;
  const float* y_src = k.y + (size_t)plane * N * N;
  for (int i = threadIdx.x; i < (th + 3) * in_w; i += kTailThreads) {
    const int row = i / in_w, col = i - row * in_w;
    const int gi = y0 - 2 + row, gj = x0 - 2 + col;                         // gu[r][c] = gu(y0 - 2 + r, x0 - 2 + c), 0 outside
    float v = 0.0f;
    if (gi >= 0 && gi < R && gj >= 0 && gj < R) {
      const size_t at = (size_t)gi * R + gj;
      v = tail_gs(g_src[at], k.activate ? o_src[at] : 0.0f, k);
    }
    gu[row][col] = v;
    if (want_f) {                                                           // yy[r][c] = y[y0 - 1 + r, x0 - 1 + c], as in the forward
      const int gy = y0 - 1 + row, gx = x0 - 1 + col;
      yy[row][col] = (gy >= 0 && gy < N && gx >= 0 && gx < N) ? y_src[(size_t)gy * N + gx] : 0.0f;
    }
  }
  __syncthreads();

  const TailShare s = tail_share(th, tw);
  const double gain_d = (double)k.gain * (double)k.dcoefs[plane];            // g_y = act_gain dcoefs adjoint(gs), rounded once
  double sum_f = 0.0, sum_g = 0.0;
  if (s.r0 < s.r1) {
    float wg[4][8], wy[4][8];
#pragma unroll
    for (int a = 1; a < 4; ++a) {
      tail_load_row(wg[a], gu, s.r0 + a - 1, s.cg);
      if (want_f) tail_load_row(wy[a], yy, s.r0 + a - 1, s.cg);
    }
    for (int r = s.r0; r < s.r1; ++r) {
      tail_slide(wg);
      tail_load_row(wg[3], gu, r + 3, s.cg);
      if (want_gy) {
        double acc[4];
        tail_window(acc, Kf, wg);
#pragma unroll
        for (int x = 0; x < 4; ++x) ob[r][4 * s.cg + x] = (float)(gain_d * acc[x]);
      }
      double f[4] = {0.0, 0.0, 0.0, 0.0};
      if (want_f) {
        tail_slide(wy);
        tail_load_row(wy[3], yy, r + 3, s.cg);
        tail_window(f, K, wy);
      }
      if (want_sums && y0 + r < R) {                                        // the output (y0 + r, x0 + 4 cg + x): gs sits at window row 2, column x + 2
#pragma unroll
        for (int x = 0; x < 4; ++x)
          if (x0 + 4 * s.cg + x < R) { sum_g += (double)wg[2][x + 2]; sum_f = fma((double)wg[2][x + 2], f[x], sum_f); }
      }
    }
  }
  __syncthreads();
  if (want_gy) {
    float* dst = k.g_y + (size_t)plane * N * N;
    for (int i = threadIdx.x; i < th * tw; i += kTailThreads) {
      const int row = i / tw, col = i - row * tw;
      dst[(size_t)(y0 + row) * N + (x0 + col)] = ob[row][col];
    }
  }
  if (want_sums) {
    tail_block_sum(sum_f, sum_g, red);
    if (threadIdx.x == 0) {
      double* p = k.partials + ((size_t)plane * k.tiles + tile) * 2;
      p[0] = sum_f * (double)k.gain; p[1] = sum_g * (double)k.gain;
    }
  }
}

__global__ __launch_bounds__(kTailThreads) void tail_flat_fwd_kernel(TailParams k) {
  const int chunk = blockIdx.x % k.tiles, plane = blockIdx.x / k.tiles;
  const int img = plane / k.C, ch = plane - img * k.C;
  const int RR = k.R * k.R;
  const float d = k.dcoefs[plane], bs = k.bias[ch];
  const bool has_noise = k.noise != nullptr;
  const float* nz = has_noise ? k.noise + (k.noise_shared ? (size_t)0 : (size_t)img * RR) : nullptr;
  const float* src = k.y + (size_t)plane * RR;
  float* dst = k.out + (size_t)plane * RR;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int at = chunk * kTailChunk + q * (4 * kTailThreads) + 4 * (int)threadIdx.x;
    if (at >= RR) break;
    if (k.vec) {                                                            // RR % 4 == 0: at + 3 < RR
      const float4 v = *reinterpret_cast<const float4*>(src + at);
      float4 n4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (has_noise) n4 = *reinterpret_cast<const float4*>(nz + at);
      float4 o;
      o.x = tail_epilogue(v.x, d, has_noise, n4.x, bs, k); o.y = tail_epilogue(v.y, d, has_noise, n4.y, bs, k);
      o.z = tail_epilogue(v.z, d, has_noise, n4.z, bs, k); o.w = tail_epilogue(v.w, d, has_noise, n4.w, bs, k);
      *reinterpret_cast<float4*>(dst + at) = o;
    } else {
      for (int x = 0; x < 4 && at + x < RR; ++x)
        dst[at + x] = tail_epilogue(src[at + x], d, has_noise, has_noise ? nz[at + x] : 0.0f, bs, k);
    }
  }
}

__global__ __launch_bounds__(kTailThreads) void tail_flat_bwd_kernel(TailParams k) {
  __shared__ double red[2][4];
  const int chunk = blockIdx.x % k.tiles, plane = blockIdx.x / k.tiles;
  const int RR = k.R * k.R;
  const float d = k.dcoefs[plane];
  const bool want_sums = k.partials != nullptr, want_f = k.g_dcoefs != nullptr, want_gy = k.g_y != nullptr;
  const float* g_src = k.g_out + (size_t)plane * RR;
  const float* o_src = k.out + (size_t)plane * RR;
  const float* y_src = k.y + (size_t)plane * RR;
  float* dst = k.g_y ? k.g_y + (size_t)plane * RR : nullptr;
  double sum_f = 0.0, sum_g = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int at = chunk * kTailChunk + q * (4 * kTailThreads) + 4 * (int)threadIdx.x;
    if (at >= RR) break;
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f}, o[4] = {0.0f, 0.0f, 0.0f, 0.0f}, f[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int n = min(4, RR - at);
    if (k.vec) {
      const float4 g4 = *reinterpret_cast<const float4*>(g_src + at);
      g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
      if (k.activate) { const float4 o4 = *reinterpret_cast<const float4*>(o_src + at); o[0] = o4.x; o[1] = o4.y; o[2] = o4.z; o[3] = o4.w; }
      if (want_f) { const float4 y4 = *reinterpret_cast<const float4*>(y_src + at); f[0] = y4.x; f[1] = y4.y; f[2] = y4.z; f[3] = y4.w; }
      if (want_gy)                                                          // ((g * slope) * act_gain) * dcoefs, each rounded: autograd's own order
        *reinterpret_cast<float4*>(dst + at) = make_float4(tail_gs(g[0], o[0], k) * k.gain * d, tail_gs(g[1], o[1], k) * k.gain * d,
                                                           tail_gs(g[2], o[2], k) * k.gain * d, tail_gs(g[3], o[3], k) * k.gain * d);
    } else {
      for (int x = 0; x < n; ++x) {
        g[x] = g_src[at + x];
        if (k.activate) o[x] = o_src[at + x];
        if (want_f) f[x] = y_src[at + x];
        if (want_gy) dst[at + x] = tail_gs(g[x], o[x], k) * k.gain * d;
      }
    }
    for (int x = 0; x < n; ++x) { const double gs = tail_gs_f64(g[x], o[x], k); sum_g += gs; sum_f = fma(gs, (double)f[x], sum_f); }
  }
  if (want_sums) {
    tail_block_sum(sum_f, sum_g, red);
    if (threadIdx.x == 0) {
      double* p = k.partials + ((size_t)plane * k.tiles + chunk) * 2;
      p[0] = sum_f * (double)k.gain; p[1] = sum_g * (double)k.gain;
    }
  }
}

// one thread per (image, channel): g_dcoefs over the plane's tiles, and - the threads of image 0 - g_bias over every image
__global__ void tail_sums_kernel(TailParams k) {
  const int plane = blockIdx.x * blockDim.x + threadIdx.x;
  if (plane >= k.B * k.C) return;
  if (k.g_dcoefs) {
    double s = 0.0;
    for (int t = 0; t < k.tiles; ++t) s += k.partials[((size_t)plane * k.tiles + t) * 2];
    k.g_dcoefs[plane] = (float)s;
  }
  if (k.g_bias && plane < k.C) {
    double s = 0.0;
    for (int b = 0; b < k.B; ++b)
      for (int t = 0; t < k.tiles; ++t) s += k.partials[(((size_t)b * k.C + plane) * k.tiles + t) * 2 + 1];
    k.g_bias[plane] = (float)s;
  }
}

// g_noise[img or none, pixel] = sum over the planes of gu.  grid (ceil(R R / PIX), B or 1); a block owns PIX adjacent pixels,
// its 256 / PIX thread groups add planes group, group + 256 / PIX, ... in float64, joined in group order.  PIX = 64 (a wave
// reads 256-byte segments) where that alone fills the GPU, 16 (64-byte segments, 4 x the blocks, a quarter of the planes per
// thread) for the small planes, where 64 would leave most CUs idle behind a long serial loop.
template <int PIX>
__global__ __launch_bounds__(kTailThreads) void tail_noise_bwd_kernel(TailParams k) {
  constexpr int kGroups = kTailThreads / PIX;
  __shared__ double red[kGroups][PIX];
  const int RR = k.R * k.R;
  const int lane = threadIdx.x % PIX, group = threadIdx.x / PIX;
  const int pix = blockIdx.x * PIX + lane;
  const int first = k.noise_shared ? 0 : (int)blockIdx.y * k.C, count = k.noise_shared ? k.B * k.C : k.C;
  double s = 0.0;
  if (pix < RR) {
#pragma unroll 4
    for (int p = group; p < count; p += kGroups) {
      const size_t at = (size_t)(first + p) * RR + pix;
      s += tail_gs_f64(k.g_out[at], k.activate ? k.out[at] : 0.0f, k);
    }
  }
  red[group][lane] = s;
  __syncthreads();
  if (group == 0 && pix < RR) {
    double t = red[0][lane];
#pragma unroll
    for (int q = 1; q < kGroups; ++q) t += red[q][lane];
    k.g_noise[(k.noise_shared ? (size_t)0 : (size_t)blockIdx.y * RR) + pix] = (float)(t * (double)k.gain);
  }
}

static bool tail_aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if ((uintptr_t)p & 15) return false;
  return true;
}

// blocks per plane of the forward (bwd = 0) or the backward launch, or 0 where the shape is refused
static int64_t tail_tiles(const nfi_synth_tail_args* a, int bwd, int* tiles_x) {
  if (!a || a->batch < 1 || a->channels < 1 || a->resolution < 1 || a->resolution > kTailMaxRes) return 0;
  int64_t tx = 1, t;
  if (a->up) {
    tx = ((int64_t)a->resolution + (bwd ? 1 : 0) + kTailTile - 1) / kTailTile;
    t = tx * tx;
  } else {
    t = ((int64_t)a->resolution * a->resolution + kTailChunk - 1) / kTailChunk;
  }
  if (t * a->batch * a->channels >= ((int64_t)1 << 31)) return 0;
  if (tiles_x) *tiles_x = (int)tx;
  return t;
}

static int tail_common(const nfi_synth_tail_args* a, int bwd, TailParams& k) {
  REQUIRE(a, "synth_tail: null argument struct");
  REQUIRE(a->y, "synth_tail: null y");
  REQUIRE(a->dcoefs, "synth_tail: null dcoefs");
  REQUIRE(a->bias, "synth_tail: null bias");
  REQUIRE(a->out, "synth_tail: null out");
  REQUIRE(!a->up || a->taps, "synth_tail: null taps (an up layer needs the 16 filter taps)");
  REQUIRE(a->batch >= 1 && a->channels >= 1 && a->resolution >= 1, "synth_tail: batch, channels and resolution must be at least 1");
  REQUIRE(a->resolution <= kTailMaxRes, "synth_tail: resolution must be at most 16384");
  REQUIRE(a->in_size == a->resolution + (a->up ? 1 : 0), "synth_tail: in_size must be resolution + 1 with up, resolution without");
  REQUIRE(a->act_gain > 0.0f, "synth_tail: act_gain must be positive (the backward takes the sign of the pre-activation from out)");
  REQUIRE(a->slope >= 0.0f, "synth_tail: slope must not be negative");
  memset(&k, 0, sizeof(k));
  k.tiles = (int)tail_tiles(a, bwd, &k.tiles_x);
  REQUIRE(k.tiles > 0, "synth_tail: element count too large: batch * channels * blocks per plane must be below 2^31");
  k.y = a->y; k.dcoefs = a->dcoefs; k.bias = a->bias; k.taps = a->taps; k.noise = a->noise; k.out = a->out;
  k.B = a->batch; k.C = a->channels; k.R = a->resolution; k.N = a->in_size;
  k.noise_shared = a->noise_shared != 0; k.activate = a->activate != 0; k.gain = a->act_gain; k.slope = a->slope;
  return NFI_OK;
}

}  // namespace nfi_synth_tail

extern "C" size_t nfi_synth_tail_bwd_workspace_bytes(const nfi_synth_tail_args* a) {
  return (size_t)nfi_synth_tail::tail_tiles(a, 1, nullptr) * (a ? (size_t)a->batch * (size_t)a->channels : 0) * 2 * sizeof(double);
}

extern "C" int nfi_synth_tail_fwd(const nfi_synth_tail_args* a, nfi_stream_t stream) {
  using namespace nfi_synth_tail;
  TailParams k;
  if (int rc = tail_common(a, 0, k)) return rc;
  const unsigned blocks = (unsigned)((int64_t)k.tiles * k.B * k.C);
  if (a->up) {
    k.vec = k.R % 4 == 0 && tail_aligned16({k.out, k.noise});
    hipLaunchKernelGGL(tail_up_fwd_kernel, dim3(blocks), dim3(kTailThreads), 0, (hipStream_t)stream, k);
  } else {
    k.vec = (k.R * k.R) % 4 == 0 && tail_aligned16({k.y, k.out, k.noise});
    hipLaunchKernelGGL(tail_flat_fwd_kernel, dim3(blocks), dim3(kTailThreads), 0, (hipStream_t)stream, k);
  }
  return check_launch("synth_tail_fwd");
}

extern "C" int nfi_synth_tail_bwd(const nfi_synth_tail_args* a, nfi_stream_t stream) {
  using namespace nfi_synth_tail;
  TailParams k;
  if (int rc = tail_common(a, 1, k)) return rc;
  REQUIRE(a->g_out, "synth_tail_bwd: null g_out");
  REQUIRE(a->g_y || a->g_dcoefs || a->g_bias || a->g_noise, "synth_tail_bwd: no gradient asked for (g_y, g_dcoefs, g_bias, g_noise all null)");
  REQUIRE(!a->g_noise || a->noise_shared || a->batch <= 65535, "synth_tail_bwd: batch must be at most 65535 with a per-image g_noise");
  k.g_out = a->g_out; k.g_y = a->g_y; k.g_dcoefs = a->g_dcoefs; k.g_bias = a->g_bias; k.g_noise = a->g_noise;
  const bool sums = a->g_dcoefs || a->g_bias;
  if (sums) {
    REQUIRE(a->workspace && ((uintptr_t)a->workspace & 7) == 0, "synth_tail_bwd: workspace missing or not 8-byte aligned");
    REQUIRE(a->workspace_bytes >= nfi_synth_tail_bwd_workspace_bytes(a), "synth_tail_bwd: workspace too small");
    k.partials = (double*)a->workspace;
  }
  const int planes = k.B * k.C;
  if (a->g_y || sums) {
    const unsigned blocks = (unsigned)((int64_t)k.tiles * planes);
    if (a->up) {
      hipLaunchKernelGGL(tail_up_bwd_kernel, dim3(blocks), dim3(kTailThreads), 0, (hipStream_t)stream, k);
    } else {
      k.vec = (k.R * k.R) % 4 == 0 && tail_aligned16({k.y, k.out, k.g_out, k.g_y});
      hipLaunchKernelGGL(tail_flat_bwd_kernel, dim3(blocks), dim3(kTailThreads), 0, (hipStream_t)stream, k);
    }
    if (int rc = check_launch("synth_tail_bwd")) return rc;
  }
  if (sums) {
    hipLaunchKernelGGL(tail_sums_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k);
    if (int rc = check_launch("synth_tail_bwd (sums)")) return rc;
  }
  if (a->g_noise) {
    const unsigned images = k.noise_shared ? 1u : (unsigned)k.B;
    const int64_t wide = (int64_t)((k.R * k.R + 63) / 64) * images;         // blocks with 64 pixels each
    if (wide >= 512) {                                                     // two blocks per CU and more
      hipLaunchKernelGGL(tail_noise_bwd_kernel<64>, dim3((unsigned)((k.R * k.R + 63) / 64), images), dim3(kTailThreads), 0, (hipStream_t)stream, k);
    } else {
      hipLaunchKernelGGL(tail_noise_bwd_kernel<16>, dim3((unsigned)((k.R * k.R + 15) / 16), images), dim3(kTailThreads), 0, (hipStream_t)stream, k);
    }
    if (int rc = check_launch("synth_tail_bwd (noise)")) return rc;
  }
  return NFI_OK;
}
