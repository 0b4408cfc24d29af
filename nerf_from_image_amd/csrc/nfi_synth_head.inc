// nfi_synth_head.inc — everything SynthesisLayer.forward / OutputLayer.forward do BEFORE their convolution,
// models/stylegan.py:173-177 (the affine: EqualizedLinear), 127-130 (the demodulation coefficients) and 132 (x * styles),
// with what autograd records for those lines.  Included by nfi_modules.hip.
//
//   styles[b,i] = (sum_d latent[b,d] A[i,d] weight_gain + bias[i] bias_gain) style_gain
//   dcoefs[b,o] = rsqrt(sum_i styles[b,i]^2 Q[o,i] + 1e-8),   Q[o,i] = sum_k W[o,i,k]^2
//   out[b,c,:]  = x[b,c,:] styles[b,c]
//
// The reference forms W[None] * styles[:, None, :, None, None], a [B,O,I,3,3] tensor, squares it and sums it; the factored
// form reads W once for the whole batch and forms nothing of that size.  Every sum here is added in float64 in a fixed
// order and rounded to float32 once (v_fma_f64 runs at the rate of the unpacked v_fma_f32 on gfx950 and these kernels wait
// for memory or for their launch): no atomics, the same bits on every launch, and a result within one rounding of the exact
// one of the float32 inputs.  dcoefs and the gradients are formed from the ROUNDED styles / dcoefs, as a caller sees them.
//
// Forward, two launches (one without demodulate):
//   head_styles_kernel   a wave owns a row of A, lanes run along d (256-byte segments), the batch in groups of 8 images;
//   head_dcoefs_kernel   a block owns a row o of W, its threads the channels i: q = sum_k W[o,i,k]^2, then 8 images' sums
//                        s^2 q per thread, joined by shuffles and across the four waves in index order.
// Backward of the head, at most four launches:
//   head_bwd_rows_kernel   (only with g_dcoefs) the one pass over W: a thread owns a channel i and 8 rows o, and writes
//                          its share of t[b,i] = sum_o g_dcoefs d^3 Q[o,i] to the workspace; g_weight, when asked for, is
//                          written in the same pass (-W sum_b g_dcoefs d^3 s^2);
//   head_bwd_gs_kernel     g_s[b,i] = (g_styles - s t) style_gain, the shares added in index order, kept in the workspace as float64;
//                          a block owns 16 rows of A and, with g_latent, writes their share of sum_i g_s A[i,d] for 8 images;
//   head_bwd_latent_kernel g_latent: a thread per (b, d) adds those shares in index order (a first form - 64 columns per block,
//                          8 blocks at D = 512, one load in flight per wave - took 63 us a layer);
//   head_bwd_affine_kernel g_affine_weight (a thread per element) and g_affine_bias.
// Modulation: flat, a block owns 4096 consecutive elements, float4 where the plane is a multiple of 4 and the pointers are
// 16-byte aligned (a float4 then lies inside one plane).  Its backward with g_styles owns planes instead: 16 lanes per plane
// up to 256 elements (R = 4 .. 16: 16 planes per block), a wave per plane up to 2048, a block of 1024 per plane above (R = 64 ..
// 256 have 512 .. 128 channels per image: as many blocks); g_x alone is the flat kernel on g_out.

namespace nfi_synth_head {

constexpr int kHeadThreads = 256;
constexpr int kHeadImages = 8;                     // images whose sums a thread keeps in registers
constexpr int kHeadRows = 8;                       // rows of W per block of the backward's pass over W
constexpr int kHeadUnroll = 8;                     // loads a lane of the styles kernel keeps in flight
constexpr int kHeadChunk = 16;                     // rows of A per block of the g_s kernel: its share of g_latent
constexpr int kModChunk = 4096;                    // elements of a flat block: 4 float4 per thread
constexpr int kModGroupMax = 256, kModWaveMax = 2048;    // largest plane of the 16-lane and of the wave geometry
constexpr int kModBlockThreads = 1024;
constexpr int64_t kHeadMaxCount = (int64_t)1 << 31;
static_assert(kHeadChunk * kHeadImages <= kHeadThreads, "synth head: a thread of the g_s kernel owns one (row, image)");
static_assert(kModChunk == 4 * 4 * kHeadThreads, "synth head: a flat block is 4 float4 per thread");

struct HeadParams {
  const float* latent; const float* A; const float* a_bias; const float* W;
  float* styles; float* dcoefs;
  const float* g_styles; const float* g_dcoefs;
  float* g_latent; float* g_A; float* g_a_bias; float* g_W;
  double* t_part;                                  // [o_chunks][B][I]
  double* g_s;                                     // [B][I]
  double* lat_part;                                // [i_chunks][B][D]
  int B, D, I, O, K, latent_stride, o_chunks, i_chunks;
  float weight_gain, bias_gain, style_gain;
};

__device__ __forceinline__ double head_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
  return v;
}

// grid ceil(I / 4): wave = row i of A
__global__ __launch_bounds__(kHeadThreads) void head_styles_kernel(HeadParams k) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * (kHeadThreads / 64) + (threadIdx.x >> 6);
  if (i >= k.I) return;                                                     // the whole wave
  const float* row = k.A + (size_t)i * k.D;
  const double shift = k.a_bias ? (double)k.a_bias[i] * (double)k.bias_gain : 0.0;
  for (int b0 = 0; b0 < k.B; b0 += kHeadImages) {
    const int nb = min(kHeadImages, k.B - b0);
    double acc[kHeadImages];
#pragma unroll
    for (int j = 0; j < kHeadImages; ++j) acc[j] = 0.0;
    for (int d0 = lane; d0 < k.D; d0 += 64 * kHeadUnroll) {                 // 8 loads of the row in flight, then 8 per image
      float a[kHeadUnroll];
#pragma unroll
      for (int u = 0; u < kHeadUnroll; ++u) a[u] = d0 + 64 * u < k.D ? row[d0 + 64 * u] : 0.0f;
#pragma unroll
      for (int j = 0; j < kHeadImages; ++j)
        if (j < nb) {
          const float* lat = k.latent + (size_t)(b0 + j) * k.latent_stride;
          float l[kHeadUnroll];
#pragma unroll
          for (int u = 0; u < kHeadUnroll; ++u) l[u] = d0 + 64 * u < k.D ? lat[d0 + 64 * u] : 0.0f;
#pragma unroll
          for (int u = 0; u < kHeadUnroll; ++u) acc[j] = fma((double)l[u], (double)a[u], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < kHeadImages; ++j) {
      const double v = head_wave_sum(acc[j]);
      if (lane == 0 && j < nb) k.styles[(size_t)(b0 + j) * k.I + i] = (float)((v * (double)k.weight_gain + shift) * (double)k.style_gain);
    }
  }
}

// q = sum_k w[k]^2 of one (o, i); KT: the compile-time K (0: k.K)
template <int KT>
__device__ __forceinline__ double head_q(const float* w, int K) {
  double q = 0.0;
  if (KT) {
#pragma unroll
    for (int t = 0; t < KT; ++t) q = fma((double)w[t], (double)w[t], q);
  } else {
    for (int t = 0; t < K; ++t) q = fma((double)w[t], (double)w[t], q);
  }
  return q;
}

// grid (O, ceil(B / 8)): block = row o of W, thread = channels i, i + 256, ...
template <int KT>
__global__ __launch_bounds__(kHeadThreads) void head_dcoefs_kernel(HeadParams k) {
  __shared__ double red[kHeadImages][kHeadThreads / 64];
  const int o = blockIdx.x, b0 = blockIdx.y * kHeadImages, nb = min(kHeadImages, k.B - b0);
  const int K = KT ? KT : k.K;
  const float* row = k.W + (size_t)o * k.I * K;
  double acc[kHeadImages];
#pragma unroll
  for (int j = 0; j < kHeadImages; ++j) acc[j] = 0.0;
  for (int i = threadIdx.x; i < k.I; i += kHeadThreads) {
    const double q = head_q<KT>(row + (size_t)i * K, K);
#pragma unroll
    for (int j = 0; j < kHeadImages; ++j)
      if (j < nb) {
        const double s = (double)k.styles[(size_t)(b0 + j) * k.I + i];
        acc[j] = fma(s * s, q, acc[j]);
      }
  }
#pragma unroll
  for (int j = 0; j < kHeadImages; ++j) {
    const double v = head_wave_sum(acc[j]);
    if ((threadIdx.x & 63) == 0) red[j][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < nb) {
    const int j = threadIdx.x;
    const double sum = ((red[j][0] + red[j][1]) + red[j][2]) + red[j][3];
    k.dcoefs[(size_t)(b0 + j) * k.O + o] = (float)(1.0 / sqrt(sum + 1e-8));
  }
}

// c[b,o] = g_dcoefs d^3
__device__ __forceinline__ double head_c(const HeadParams& k, int b, int o) {
  const double d = (double)k.dcoefs[(size_t)b * k.O + o];
  return (double)k.g_dcoefs[(size_t)b * k.O + o] * (d * d * d);
}

// grid (ceil(I / 256), o_chunks, ceil(B / 8)): thread = channel i, rows [8 y, 8 y + 8) of W
template <int KT>
__global__ __launch_bounds__(kHeadThreads) void head_bwd_rows_kernel(HeadParams k) {
  const int i = blockIdx.x * kHeadThreads + threadIdx.x;
  if (i >= k.I) return;                                                     // no barrier below
  const int K = KT ? KT : k.K;
  const int b0 = blockIdx.z * kHeadImages, nb = min(kHeadImages, k.B - b0);
  const int o0 = blockIdx.y * kHeadRows, o1 = min(o0 + kHeadRows, k.O);
  double acc[kHeadImages];
#pragma unroll
  for (int j = 0; j < kHeadImages; ++j) acc[j] = 0.0;
  for (int o = o0; o < o1; ++o) {
    const size_t at = ((size_t)o * k.I + i) * K;
    const double q = head_q<KT>(k.W + at, K);
#pragma unroll
    for (int j = 0; j < kHeadImages; ++j)
      if (j < nb) acc[j] = fma(head_c(k, b0 + j, o), q, acc[j]);
    if (k.g_W && blockIdx.z == 0) {                                         // over the WHOLE batch, in image order
      double coef = 0.0;
      for (int b = 0; b < k.B; ++b) {
        const double s = (double)k.styles[(size_t)b * k.I + i];
        coef = fma(head_c(k, b, o), s * s, coef);
      }
      if (KT) {
#pragma unroll
        for (int t = 0; t < KT; ++t) k.g_W[at + t] = (float)(-(double)k.W[at + t] * coef);
      } else {
        for (int t = 0; t < K; ++t) k.g_W[at + t] = (float)(-(double)k.W[at + t] * coef);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kHeadImages; ++j)
    if (j < nb) k.t_part[((size_t)blockIdx.y * k.B + (b0 + j)) * k.I + i] = acc[j];
}

// grid (ceil(I / 16), ceil(B / 8)): the block owns 16 rows of A and 8 images.  Thread (row, image) adds the shares of t in
// index order and writes g_s; then, with g_latent, thread = column d adds the 16 rows' g_s A[i,d] per image: the block's
// share of g_latent, to the workspace
__global__ __launch_bounds__(kHeadThreads) void head_bwd_gs_kernel(HeadParams k) {
  __shared__ double gs[kHeadImages][kHeadChunk];
  const int i0 = blockIdx.x * kHeadChunk, b0 = blockIdx.y * kHeadImages, nb = min(kHeadImages, k.B - b0);
  if (threadIdx.x < kHeadChunk * kHeadImages) {
    const int il = threadIdx.x % kHeadChunk, j = threadIdx.x / kHeadChunk;
    double v = 0.0;
    if (i0 + il < k.I && j < nb) {
      const size_t e = (size_t)(b0 + j) * k.I + (i0 + il);
      double t = 0.0;
      if (k.g_dcoefs) {
#pragma unroll 8
        for (int c = 0; c < k.o_chunks; ++c) t += k.t_part[(size_t)c * k.B * k.I + e];
      }
      const double g = k.g_styles ? (double)k.g_styles[e] : 0.0;
      v = k.g_dcoefs ? (g - (double)k.styles[e] * t) * (double)k.style_gain : g * (double)k.style_gain;
      k.g_s[e] = v;
    }
    gs[j][il] = v;                                                          // 0 beyond I or the batch
  }
  if (!k.g_latent) return;                                                  // the whole block
  __syncthreads();
  const int rows = min(kHeadChunk, k.I - i0);
  for (int d = threadIdx.x; d < k.D; d += kHeadThreads) {
    float a[kHeadChunk];
#pragma unroll
    for (int r = 0; r < kHeadChunk; ++r) a[r] = r < rows ? k.A[(size_t)(i0 + r) * k.D + d] : 0.0f;
#pragma unroll
    for (int j = 0; j < kHeadImages; ++j)
      if (j < nb) {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < kHeadChunk; ++r) acc = fma(gs[j][r], (double)a[r], acc);
        k.lat_part[((size_t)blockIdx.x * k.B + (b0 + j)) * k.D + d] = acc;
      }
  }
}

// grid ceil(B D / 256): thread = (b, d), the shares of the g_s kernel's blocks added in index order
__global__ __launch_bounds__(kHeadThreads) void head_bwd_latent_kernel(HeadParams k) {
  const int64_t e = (int64_t)blockIdx.x * kHeadThreads + threadIdx.x;
  if (e >= (int64_t)k.B * k.D) return;
  double s = 0.0;
#pragma unroll 8
  for (int c = 0; c < k.i_chunks; ++c) s += k.lat_part[(size_t)c * k.B * k.D + e];
  k.g_latent[e] = (float)(s * (double)k.weight_gain);
}

// grid ceil(I D / 256) with g_A (thread = element (i, d); the threads of column 0 write g_a_bias too), ceil(I / 256) without
__global__ __launch_bounds__(kHeadThreads) void head_bwd_affine_kernel(HeadParams k) {
  const int64_t e = (int64_t)blockIdx.x * kHeadThreads + threadIdx.x;
  const int64_t count = k.g_A ? (int64_t)k.I * k.D : (int64_t)k.I;
  if (e >= count) return;
  const int i = k.g_A ? (int)(e / k.D) : (int)e, d = k.g_A ? (int)(e - (int64_t)i * k.D) : 0;
  double acc = 0.0, sum = 0.0;
  for (int b = 0; b < k.B; ++b) {
    const double g = k.g_s[(size_t)b * k.I + i];
    sum += g;
    if (k.g_A) acc = fma(g, (double)k.latent[(size_t)b * k.latent_stride + d], acc);
  }
  if (k.g_A) k.g_A[e] = (float)(acc * (double)k.weight_gain);
  if (k.g_a_bias && d == 0) k.g_a_bias[i] = (float)(sum * (double)k.bias_gain);
}

struct ModParams {
  const float* x; const float* styles; const float* g_out; float* g_x; float* g_styles;
  int planes, n, vec, lanes;
};

// out = in * styles[plane]; grid ceil(total / 4096), total = planes * n < 2^31.  The four 16-byte loads are issued before the
// first store; a block that lies inside one plane (every block from 4096 elements a plane on, where 4096 divides it) reads
// one style for all its threads
__global__ __launch_bounds__(kHeadThreads) void modulate_flat_kernel(const float* __restrict__ in, const float* __restrict__ styles,
                                                                     float* __restrict__ out, unsigned n, unsigned total, int vec) {
  const unsigned first = blockIdx.x * (unsigned)kModChunk;                  // < 2^31
  if (vec) {                                                                // n % 4 == 0: a float4 lies inside the tensor and inside one plane
    const unsigned p0 = first / n;
    const bool one_plane = first - p0 * n + (unsigned)kModChunk <= n;
    const float s0 = styles[p0];
    float4 v[4];
    unsigned at[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      at[q] = first + q * (4u * kHeadThreads) + 4u * threadIdx.x;           // < 2^31 + 4096
      if (at[q] < total) v[q] = *reinterpret_cast<const float4*>(in + at[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (at[q] < total) {
        const float s = one_plane ? s0 : styles[at[q] / n];
        *reinterpret_cast<float4*>(out + at[q]) = make_float4(v[q].x * s, v[q].y * s, v[q].z * s, v[q].w * s);
      }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned at = first + q * (4u * kHeadThreads) + 4u * threadIdx.x;
      for (unsigned x = 0; x < 4 && at + x < total; ++x) out[at + x] = in[at + x] * styles[(at + x) / n];
    }
  }
}

// this thread's share of one plane: elements first, first + step, ... (vec: float4 at 4 first, ...); g_x written, g * x added
__device__ __forceinline__ double modulate_bwd_share(const ModParams& k, int plane, int first, int step) {
  const size_t base = (size_t)plane * k.n;
  const float s = k.styles[plane];
  double acc = 0.0;
  if (k.vec) {
    for (int e = 4 * first; e < k.n; e += 4 * step) {
      const float4 g = *reinterpret_cast<const float4*>(k.g_out + base + e);
      if (k.g_x) *reinterpret_cast<float4*>(k.g_x + base + e) = make_float4(g.x * s, g.y * s, g.z * s, g.w * s);
      if (k.g_styles) {
        const float4 v = *reinterpret_cast<const float4*>(k.x + base + e);
        acc = fma((double)g.x, (double)v.x, acc); acc = fma((double)g.y, (double)v.y, acc);
        acc = fma((double)g.z, (double)v.z, acc); acc = fma((double)g.w, (double)v.w, acc);
      }
    }
  } else {
    for (int e = first; e < k.n; e += step) {
      const float g = k.g_out[base + e];
      if (k.g_x) k.g_x[base + e] = g * s;
      if (k.g_styles) acc = fma((double)g, (double)k.x[base + e], acc);
    }
  }
  return acc;
}

// `lanes` (16 or 64) adjacent lanes own a plane; grid ceil(planes / (256 / lanes))
__global__ __launch_bounds__(kHeadThreads) void modulate_bwd_group_kernel(ModParams k) {
  const int G = k.lanes, lane = threadIdx.x % G;
  const int64_t plane = (int64_t)blockIdx.x * (kHeadThreads / G) + threadIdx.x / G;
  const bool inside = plane < k.planes;
  double acc = inside ? modulate_bwd_share(k, (int)plane, lane, G) : 0.0;
  if (k.g_styles) {                                                         // every lane of the wave takes part
    for (int off = G >> 1; off; off >>= 1) acc += __shfl_down(acc, off, G);
    if (inside && lane == 0) k.g_styles[plane] = (float)acc;
  }
}

// a block of 1024 owns a plane; grid planes
__global__ __launch_bounds__(kModBlockThreads) void modulate_bwd_block_kernel(ModParams k) {
  __shared__ double red[kModBlockThreads / 64];
  const int plane = blockIdx.x;
  const double acc = head_wave_sum(modulate_bwd_share(k, plane, threadIdx.x, kModBlockThreads));
  if (!k.g_styles) return;                                                  // the whole block
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kModBlockThreads / 64; ++w) s += red[w];
    k.g_styles[plane] = (float)s;
  }
}

static bool head_aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if ((uintptr_t)p & 15) return false;
  return true;
}

static bool head_counts_fit(const nfi_synth_head_args* a) {
  const int64_t B = a->batch, D = a->latent_dim, I = a->in_channels, O = a->out_channels, K = a->taps;
  const int64_t stride = a->latent_stride > D ? a->latent_stride : D;
  return B * stride < kHeadMaxCount && B * I < kHeadMaxCount && B * O < kHeadMaxCount && I * D < kHeadMaxCount && O * I < kHeadMaxCount &&
         O * I * K < kHeadMaxCount && (B + kHeadImages - 1) / kHeadImages <= 65535 && (O + kHeadRows - 1) / kHeadRows <= 65535;
}

static bool head_shape_ok(const nfi_synth_head_args* a) {
  return a && a->batch >= 1 && a->latent_dim >= 1 && a->in_channels >= 1 && a->out_channels >= 1 && a->taps >= 1 && head_counts_fit(a);
}

static int head_common(const nfi_synth_head_args* a, HeadParams& k) {
  REQUIRE(a, "synth_head: null argument struct");
  REQUIRE(a->latent, "synth_head: null latent");
  REQUIRE(a->affine_weight, "synth_head: null affine_weight");
  REQUIRE(a->styles, "synth_head: null styles");
  REQUIRE(a->batch >= 1 && a->latent_dim >= 1 && a->in_channels >= 1 && a->out_channels >= 1 && a->taps >= 1,
          "synth_head: batch, latent_dim, in_channels, out_channels and taps must be at least 1");
  REQUIRE(a->latent_stride >= a->latent_dim, "synth_head: latent_stride must be at least latent_dim");
  REQUIRE(!a->demodulate || a->weight, "synth_head: demodulate without weight");
  REQUIRE(!a->demodulate || a->dcoefs, "synth_head: demodulate without dcoefs");
  REQUIRE(a->weight_gain == a->weight_gain, "synth_head: weight_gain is NaN");
  REQUIRE(a->bias_gain == a->bias_gain, "synth_head: bias_gain is NaN");
  REQUIRE(a->style_gain == a->style_gain, "synth_head: style_gain is NaN");
  REQUIRE(head_counts_fit(a), "synth_head: element count too large: batch * latent_stride, batch * in_channels, batch * out_channels, "
                              "in_channels * latent_dim and out_channels * in_channels * taps must be below 2^31");
  memset(&k, 0, sizeof(k));
  k.latent = a->latent; k.A = a->affine_weight; k.a_bias = a->affine_bias; k.W = a->weight; k.styles = a->styles; k.dcoefs = a->dcoefs;
  k.B = a->batch; k.D = a->latent_dim; k.I = a->in_channels; k.O = a->out_channels; k.K = a->taps; k.latent_stride = a->latent_stride;
  k.o_chunks = (a->out_channels + kHeadRows - 1) / kHeadRows;
  k.i_chunks = (a->in_channels + kHeadChunk - 1) / kHeadChunk;
  k.weight_gain = a->weight_gain; k.bias_gain = a->bias_gain; k.style_gain = a->style_gain;
  return NFI_OK;
}

static int modulate_common(const nfi_synth_modulate_args* a) {
  REQUIRE(a, "synth_modulate: null argument struct");
  REQUIRE(a->styles, "synth_modulate: null styles");
  REQUIRE(a->batch >= 1 && a->channels >= 1 && a->plane >= 1, "synth_modulate: batch, channels and plane must be at least 1");
  REQUIRE((int64_t)a->batch * a->channels * a->plane < kHeadMaxCount, "synth_modulate: element count too large: batch * channels * plane must be below 2^31");
  return NFI_OK;
}

}  // namespace nfi_synth_head

extern "C" size_t nfi_synth_head_bwd_workspace_bytes(const nfi_synth_head_args* a) {
  using namespace nfi_synth_head;
  if (!head_shape_ok(a)) return 0;
  const size_t o_chunks = a->demodulate ? (size_t)((a->out_channels + kHeadRows - 1) / kHeadRows) : 0;
  const size_t i_chunks = (size_t)((a->in_channels + kHeadChunk - 1) / kHeadChunk);
  return ((o_chunks + 1) * (size_t)a->batch * (size_t)a->in_channels + i_chunks * (size_t)a->batch * (size_t)a->latent_dim) * sizeof(double);
}

extern "C" int nfi_synth_head_fwd(const nfi_synth_head_args* a, nfi_stream_t stream) {
  using namespace nfi_synth_head;
  HeadParams k;
  if (int rc = head_common(a, k)) return rc;
  hipLaunchKernelGGL(head_styles_kernel, dim3((unsigned)((k.I + 3) / 4)), dim3(kHeadThreads), 0, (hipStream_t)stream, k);
  if (int rc = check_launch("synth_head_fwd (styles)")) return rc;
  if (a->demodulate) {
    const dim3 grid((unsigned)k.O, (unsigned)((k.B + kHeadImages - 1) / kHeadImages));
    if (k.K == 9) hipLaunchKernelGGL(head_dcoefs_kernel<9>, grid, dim3(kHeadThreads), 0, (hipStream_t)stream, k);
    else if (k.K == 1) hipLaunchKernelGGL(head_dcoefs_kernel<1>, grid, dim3(kHeadThreads), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(head_dcoefs_kernel<0>, grid, dim3(kHeadThreads), 0, (hipStream_t)stream, k);
    if (int rc = check_launch("synth_head_fwd (dcoefs)")) return rc;
  }
  return NFI_OK;
}

extern "C" int nfi_synth_head_bwd(const nfi_synth_head_args* a, nfi_stream_t stream) {
  using namespace nfi_synth_head;
  HeadParams k;
  if (int rc = head_common(a, k)) return rc;
  REQUIRE(a->g_styles || a->g_dcoefs, "synth_head_bwd: no upstream gradient (g_styles and g_dcoefs both null)");
  REQUIRE(a->g_latent || a->g_affine_weight || a->g_affine_bias || a->g_weight,
          "synth_head_bwd: no gradient asked for (g_latent, g_affine_weight, g_affine_bias, g_weight all null)");
  REQUIRE(!a->g_dcoefs || (a->demodulate && a->dcoefs && a->weight), "synth_head_bwd: g_dcoefs without dcoefs (demodulate, dcoefs and weight)");
  REQUIRE(!a->g_weight || a->g_dcoefs, "synth_head_bwd: g_weight without g_dcoefs (it is the demodulation's share only)");
  const size_t need = nfi_synth_head_bwd_workspace_bytes(a);
  REQUIRE(a->workspace && ((uintptr_t)a->workspace & 7) == 0, "synth_head_bwd: workspace missing or not 8-byte aligned");
  REQUIRE(a->workspace_bytes >= need, "synth_head_bwd: workspace too small");
  k.g_styles = a->g_styles; k.g_dcoefs = a->g_dcoefs;
  k.g_latent = a->g_latent; k.g_A = a->g_affine_weight; k.g_a_bias = a->g_affine_bias; k.g_W = a->g_weight;
  const size_t rows = (size_t)k.B * k.I;
  k.g_s = (double*)a->workspace;
  k.lat_part = k.g_s + rows;                                                // i_chunks * B * D
  k.t_part = k.lat_part + (size_t)k.i_chunks * k.B * k.D;                   // o_chunks * B * I: there with demodulate, the only case that reads it
  const unsigned b_chunks = (unsigned)((k.B + kHeadImages - 1) / kHeadImages);
  if (a->g_dcoefs) {
    const dim3 grid((unsigned)((k.I + kHeadThreads - 1) / kHeadThreads), (unsigned)k.o_chunks, b_chunks);
    if (k.K == 9) hipLaunchKernelGGL(head_bwd_rows_kernel<9>, grid, dim3(kHeadThreads), 0, (hipStream_t)stream, k);
    else if (k.K == 1) hipLaunchKernelGGL(head_bwd_rows_kernel<1>, grid, dim3(kHeadThreads), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(head_bwd_rows_kernel<0>, grid, dim3(kHeadThreads), 0, (hipStream_t)stream, k);
    if (int rc = check_launch("synth_head_bwd (rows)")) return rc;
  }
  if (a->g_latent || a->g_affine_weight || a->g_affine_bias) {
    hipLaunchKernelGGL(head_bwd_gs_kernel, dim3((unsigned)k.i_chunks, b_chunks), dim3(kHeadThreads), 0, (hipStream_t)stream, k);
    if (int rc = check_launch("synth_head_bwd (g_s)")) return rc;
  }
  if (a->g_latent) {
    hipLaunchKernelGGL(head_bwd_latent_kernel, dim3((unsigned)(((int64_t)k.B * k.D + kHeadThreads - 1) / kHeadThreads)), dim3(kHeadThreads), 0,
                       (hipStream_t)stream, k);
    if (int rc = check_launch("synth_head_bwd (latent)")) return rc;
  }
  if (a->g_affine_weight || a->g_affine_bias) {
    const int64_t count = a->g_affine_weight ? (int64_t)k.I * k.D : (int64_t)k.I;
    hipLaunchKernelGGL(head_bwd_affine_kernel, dim3((unsigned)((count + kHeadThreads - 1) / kHeadThreads)), dim3(kHeadThreads), 0, (hipStream_t)stream, k);
    if (int rc = check_launch("synth_head_bwd (affine)")) return rc;
  }
  return NFI_OK;
}

extern "C" int nfi_synth_modulate_fwd(const nfi_synth_modulate_args* a, nfi_stream_t stream) {
  using namespace nfi_synth_head;
  if (int rc = modulate_common(a)) return rc;
  REQUIRE(a->x, "synth_modulate_fwd: null x");
  REQUIRE(a->out, "synth_modulate_fwd: null out");
  const unsigned n = (unsigned)a->plane, total = (unsigned)((int64_t)a->batch * a->channels * a->plane);
  const int vec = n % 4 == 0 && head_aligned16({a->x, a->out});
  hipLaunchKernelGGL(modulate_flat_kernel, dim3((total + kModChunk - 1) / kModChunk), dim3(kHeadThreads), 0, (hipStream_t)stream, a->x, a->styles,
                     a->out, n, total, vec);
  return check_launch("synth_modulate_fwd");
}

extern "C" int nfi_synth_modulate_bwd(const nfi_synth_modulate_args* a, nfi_stream_t stream) {
  using namespace nfi_synth_head;
  if (int rc = modulate_common(a)) return rc;
  REQUIRE(a->g_out, "synth_modulate_bwd: null g_out");
  REQUIRE(a->g_x || a->g_styles, "synth_modulate_bwd: no gradient asked for (g_x and g_styles both null)");
  REQUIRE(!a->g_styles || a->x, "synth_modulate_bwd: g_styles without x");
  const unsigned n = (unsigned)a->plane, total = (unsigned)((int64_t)a->batch * a->channels * a->plane);
  if (!a->g_styles) {                                                       // g_x alone is the forward on g_out
    const int vec = n % 4 == 0 && head_aligned16({a->g_out, a->g_x});
    hipLaunchKernelGGL(modulate_flat_kernel, dim3((total + kModChunk - 1) / kModChunk), dim3(kHeadThreads), 0, (hipStream_t)stream, a->g_out,
                       a->styles, a->g_x, n, total, vec);
    return check_launch("synth_modulate_bwd");
  }
  ModParams k;
  k.x = a->x; k.styles = a->styles; k.g_out = a->g_out; k.g_x = a->g_x; k.g_styles = a->g_styles;
  k.planes = a->batch * a->channels; k.n = a->plane;
  k.vec = n % 4 == 0 && head_aligned16({a->x, a->g_out, a->g_x});
  if (k.n <= kModWaveMax) {
    k.lanes = k.n <= kModGroupMax ? 16 : 64;
    const int per_block = kHeadThreads / k.lanes;
    hipLaunchKernelGGL(modulate_bwd_group_kernel, dim3((unsigned)(((int64_t)k.planes + per_block - 1) / per_block)), dim3(kHeadThreads), 0, (hipStream_t)stream, k);
  } else {
    k.lanes = kModBlockThreads;
    hipLaunchKernelGGL(modulate_bwd_block_kernel, dim3((unsigned)k.planes), dim3(kModBlockThreads), 0, (hipStream_t)stream, k);
  }
  return check_launch("synth_modulate_bwd");
}
