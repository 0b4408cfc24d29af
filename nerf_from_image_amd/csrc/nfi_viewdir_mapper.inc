// nfi_viewdir_mapper.inc — the per-ray trunk of ViewDirectionMapper (models/generator.py:194-241) as one kernel forward and
// one kernel backward (included by nfi_modules.hip).
//
//   x = lrelu(fc0 v);  x = (lrelu(norm2 fc2 lrelu(norm1 fc1 x)) + x) c;  x = (lrelu(norm4 fc4 lrelu(norm3 fc3 x)) + x) c;
//   feature = fc6 lrelu(fc5 x)          c = sqrt(2)/2, lrelu slope 0.2, LayerNorm(64) with biased variance and eps 1e-5,
//   EqualizedLinear gains 1/sqrt(in) on the weights (models/stylegan.py:170-177), fc1..fc4 without bias.
//
// One THREAD per ray, one wave per block, plain fp32 FMAs.  A ray's 64 activations live in registers; every weight row is
// read at a wave-uniform address (scalar loads, the 23 k parameter floats stay in the scalar / L2 caches), so a layer is
// 64 rows x 64 FMAs with the row index rolled and the column index unrolled.  The one dynamic index a layer needs (the
// output row) goes through an LDS column the thread owns: lds[row * 65 + thread].  Nothing per layer reaches HBM.
//
// Backward: the forward is recomputed per ray (kept: fc0's output, the four normalised vectors, fc5's output: 384 floats a
// ray - as compiled the kernel takes all 512 registers of a lane, one wave per SIMD, and spills ~100 of them to scratch),
// then per layer
//   - the input gradient W^T g: the thread's own g read back from its LDS row, weight rows at uniform addresses;
//   - the weight gradient sum_rays g (x) x: the 64 rays of the block put g as rows [ray][j] and x as columns [k][ray] into
//     LDS; thread t owns column k = t of the 64 x 64 (fc6: 32 x 64) gradient and walks the rays, then adds its column to the
//     caller's buffer with one line-coalesced fp32 atomic per row; biases and norm affines are column sums of such rows.
//     (Not the field backward's one flush per resident block: the accumulators of a block are 23 392 floats, 366 registers
//     a lane on top of a kernel that spills already, or 91 KB of LDS.  Atomic traffic therefore grows with N: N / 64 adds
//     per address; measured against the PyTorch modules in profiles/r11.)
// Rays beyond n take part with a zero upstream gradient.  Without parameter-gradient pointers (a frozen generator: only
// g_viewdir is wanted) the weight-gradient stages and every atomic are skipped.

constexpr int kVmRays = 64;          // rays per block = threads per block (one wave)
constexpr int kVmCol = 65;           // LDS pitch of [feature][ray] columns: conflict-free both ways
constexpr int kVmRow = 68;           // LDS pitch of [ray][feature] rows: 16-byte aligned rows for wave-uniform float4 reads
constexpr float kVmSlope = 0.2f, kVmJoin = 0.70710678118654752440f, kVmEps = 1e-5f;

struct VmParams {
  int64_t n;
  const float* viewdir;
  const float *w0, *b0, *w[4], *nw[4], *nb[4], *w5, *b5, *w6, *b6;
  float* feature;
  const float* g_feature;
  float *g_w0, *g_b0, *g_w[4], *g_nw[4], *g_nb[4], *g_w5, *g_b5, *g_w6, *g_b6, *g_viewdir;
};

__device__ __forceinline__ float vm_lrelu(float x) { return x > 0.0f ? x : x * kVmSlope; }

// y = gain * W x (+ b), W [ROWS,64] row-major; col = the thread's LDS column (pitch kVmCol)
template <int ROWS>
__device__ __forceinline__ void vm_linear(const float* __restrict__ W, const float* __restrict__ b, float gain, const float (&x)[64],
                                          float* col, float (&y)[ROWS]) {
#pragma nounroll
  for (int j = 0; j < ROWS; ++j) {
    const float* __restrict__ wr = W + j * 64;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
    for (int k = 0; k < 64; k += 4) {
      a0 = fmaf(wr[k], x[k], a0);
      a1 = fmaf(wr[k + 1], x[k + 1], a1);
      a2 = fmaf(wr[k + 2], x[k + 2], a2);
      a3 = fmaf(wr[k + 3], x[k + 3], a3);
    }
    float s = ((a0 + a1) + (a2 + a3)) * gain;
    if (b) s += b[j];
    col[j * kVmCol] = s;
  }
#pragma unroll
  for (int j = 0; j < ROWS; ++j) y[j] = col[j * kVmCol];
}

// fc0: [64,3] with gain 1/sqrt(3) on the weight (rounded as the reference rounds it), bias, activation
__device__ __forceinline__ void vm_fc0(const float* __restrict__ W, const float* __restrict__ b, const float (&v)[3], float* col,
                                       float (&y)[64]) {
  const float gain = 0.57735026918962576451f;
#pragma nounroll
  for (int j = 0; j < 64; ++j) {
    float s = (W[3 * j] * gain) * v[0];
    s = fmaf(W[3 * j + 1] * gain, v[1], s);
    s = fmaf(W[3 * j + 2] * gain, v[2], s);
    col[j * kVmCol] = vm_lrelu(s + b[j]);
  }
#pragma unroll
  for (int j = 0; j < 64; ++j) y[j] = col[j * kVmCol];
}

// y -> (y - mean) * rstd in place; returns rstd
__device__ __forceinline__ float vm_normalise(float (&y)[64]) {
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
  for (int k = 0; k < 64; k += 4) { s0 += y[k]; s1 += y[k + 1]; s2 += y[k + 2]; s3 += y[k + 3]; }
  const float mean = ((s0 + s1) + (s2 + s3)) * (1.0f / 64.0f);
  s0 = s1 = s2 = s3 = 0.0f;
#pragma unroll
  for (int k = 0; k < 64; k += 4) {
    y[k] -= mean; y[k + 1] -= mean; y[k + 2] -= mean; y[k + 3] -= mean;
    s0 = fmaf(y[k], y[k], s0); s1 = fmaf(y[k + 1], y[k + 1], s1); s2 = fmaf(y[k + 2], y[k + 2], s2); s3 = fmaf(y[k + 3], y[k + 3], s3);
  }
  const float rstd = 1.0f / sqrtf(((s0 + s1) + (s2 + s3)) * (1.0f / 64.0f) + kVmEps);
#pragma unroll
  for (int k = 0; k < 64; ++k) y[k] *= rstd;
  return rstd;
}

// lrelu(xh * w + b)
__device__ __forceinline__ void vm_affine_act(const float (&xh)[64], const float* __restrict__ w, const float* __restrict__ b,
                                              float (&a)[64]) {
#pragma unroll
  for (int k = 0; k < 64; ++k) a[k] = vm_lrelu(fmaf(xh[k], w[k], b[k]));
}

__global__ __launch_bounds__(kVmRays) void viewdir_mapper_fwd_kernel(VmParams p) {
  __shared__ float lds[64 * kVmCol];
  const int64_t ray = (int64_t)blockIdx.x * kVmRays + threadIdx.x;
  if (ray >= p.n) return;          // (no barrier below: a thread only ever touches its own LDS column)
  float* col = lds + threadIdx.x;
  const float v[3] = {p.viewdir[3 * ray], p.viewdir[3 * ray + 1], p.viewdir[3 * ray + 2]};
  float x[64], y[64];
  vm_fc0(p.w0, p.b0, v, col, x);
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    vm_linear<64>(p.w[2 * blk], nullptr, 0.125f, x, col, y);
    vm_normalise(y);
    vm_affine_act(y, p.nw[2 * blk], p.nb[2 * blk], y);
    float z[64];
    vm_linear<64>(p.w[2 * blk + 1], nullptr, 0.125f, y, col, z);
    vm_normalise(z);
    vm_affine_act(z, p.nw[2 * blk + 1], p.nb[2 * blk + 1], z);
#pragma unroll
    for (int k = 0; k < 64; ++k) x[k] = (z[k] + x[k]) * kVmJoin;
  }
  vm_linear<64>(p.w5, p.b5, 0.125f, x, col, y);
#pragma unroll
  for (int k = 0; k < 64; ++k) y[k] = vm_lrelu(y[k]);
  float o[32];
  vm_linear<32>(p.w6, p.b6, 0.125f, y, col, o);
  float4* dst = reinterpret_cast<float4*>(p.feature + 32 * ray);
#pragma unroll
  for (int j = 0; j < 32; j += 4) dst[j >> 2] = make_float4(o[j], o[j + 1], o[j + 2], o[j + 3]);
}

// ---- backward helpers.  rows: [ray][kVmRow], cols: [feature][kVmCol]; every helper starts with a barrier (the readers
// of the previous contents are done) and leaves the thread's own row of `rows` readable. ----

// the block's rays put g into `rows`; returns sum over rays of g[t] for thread t (t < ROWS, else 0)
template <int ROWS>
__device__ __forceinline__ float vm_put_rows(const float (&g)[ROWS], float* rows) {
  const int t = threadIdx.x;
  __syncthreads();
  float4* mine = reinterpret_cast<float4*>(rows + t * kVmRow);
#pragma unroll
  for (int j = 0; j < ROWS; j += 4) mine[j >> 2] = make_float4(g[j], g[j + 1], g[j + 2], g[j + 3]);
  __syncthreads();
  float s = 0.0f;
  if (t < ROWS)
    for (int r = 0; r < kVmRays; ++r) s += rows[r * kVmRow + t];
  return s;
}

// g_w[j,t] += scale * sum_rays g[ray][j] x[ray][t] for the g already in `rows` (vm_put_rows) and this x
template <int ROWS>
__device__ __forceinline__ void vm_weight_grad(const float (&x)[64], const float* rows, float* cols, float scale, float* g_w) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 64; ++k) cols[k * kVmCol + t] = x[k];
  __syncthreads();
  float acc[ROWS];
#pragma unroll
  for (int j = 0; j < ROWS; ++j) acc[j] = 0.0f;
#pragma nounroll
  for (int r = 0; r < kVmRays; ++r) {
    const float xr = cols[t * kVmCol + r];
    const float4* g4 = reinterpret_cast<const float4*>(rows + r * kVmRow);
#pragma unroll
    for (int j = 0; j < ROWS; j += 4) {
      const float4 g = g4[j >> 2];
      acc[j] = fmaf(g.x, xr, acc[j]);
      acc[j + 1] = fmaf(g.y, xr, acc[j + 1]);
      acc[j + 2] = fmaf(g.z, xr, acc[j + 2]);
      acc[j + 3] = fmaf(g.w, xr, acc[j + 3]);
    }
  }
#pragma unroll
  for (int j = 0; j < ROWS; ++j) unsafeAtomicAdd(&g_w[j * 64 + t], acc[j] * scale);
  __syncthreads();       // cols may be rewritten
}

// gx = gain * W^T g, g = the thread's own row of `rows`
template <int ROWS>
__device__ __forceinline__ void vm_input_grad(const float* __restrict__ W, float gain, const float* rows, float (&gx)[64]) {
  const float* mine = rows + threadIdx.x * kVmRow;
#pragma unroll
  for (int k = 0; k < 64; ++k) gx[k] = 0.0f;
#pragma nounroll
  for (int j = 0; j < ROWS; ++j) {
    const float gj = mine[j];
    const float* __restrict__ wr = W + j * 64;
#pragma unroll
    for (int k = 0; k < 64; ++k) gx[k] = fmaf(wr[k], gj, gx[k]);
  }
#pragma unroll
  for (int k = 0; k < 64; ++k) gx[k] *= gain;
}

// backward of a = lrelu(xh * w + b), xh = normalise(y): g (w.r.t. a) -> g (w.r.t. y) in place; the affine gradients are
// added to g_nw / g_nb
__device__ __forceinline__ void vm_norm_bwd(float (&g)[64], const float (&xh)[64], float rstd, const float* __restrict__ w,
                                            const float* __restrict__ b, float* rows, float* g_nw, float* g_nb, bool wp) {
  const int t = threadIdx.x;
  float tmp[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    g[k] = fmaf(xh[k], w[k], b[k]) > 0.0f ? g[k] : g[k] * kVmSlope;       // w.r.t. the affine output
    tmp[k] = g[k] * xh[k];
  }
  if (wp) {
    const float sw = vm_put_rows<64>(tmp, rows);
    const float sb = vm_put_rows<64>(g, rows);
    unsafeAtomicAdd(&g_nw[t], sw);
    unsafeAtomicAdd(&g_nb[t], sb);
  }
  float m0 = 0.0f, m1 = 0.0f;
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    g[k] *= w[k];                                                          // w.r.t. xh
    m0 += g[k];
    m1 = fmaf(g[k], xh[k], m1);
  }
  m0 *= 1.0f / 64.0f;
  m1 *= 1.0f / 64.0f;
#pragma unroll
  for (int k = 0; k < 64; ++k) g[k] = ((g[k] - m0) - xh[k] * m1) * rstd;
}

__global__ __launch_bounds__(kVmRays) void viewdir_mapper_bwd_kernel(VmParams p) {
  __shared__ float cols[64 * kVmCol];
  __shared__ __attribute__((aligned(16))) float rows[kVmRays * kVmRow];
  __shared__ float vdir[kVmRays * 3];
  const int t = threadIdx.x;
  const int64_t ray = (int64_t)blockIdx.x * kVmRays + t;
  const bool live = ray < p.n;
  const bool wp = p.g_w0 != nullptr;          // parameter gradients wanted (all 18 or none: checked by the host entry)
  const int64_t src = live ? ray : p.n - 1;
  float* col = cols + t;
  const float v[3] = {p.viewdir[3 * src], p.viewdir[3 * src + 1], p.viewdir[3 * src + 2]};
  vdir[3 * t] = v[0]; vdir[3 * t + 1] = v[1]; vdir[3 * t + 2] = v[2];

  // ---- forward, recomputed ----
  float a0[64], xh[4][64], rstd[4], a5[64];
  {
    float x[64], y[64];
    vm_fc0(p.w0, p.b0, v, col, a0);
#pragma unroll
    for (int k = 0; k < 64; ++k) x[k] = a0[k];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      vm_linear<64>(p.w[2 * blk], nullptr, 0.125f, x, col, xh[2 * blk]);
      rstd[2 * blk] = vm_normalise(xh[2 * blk]);
      vm_affine_act(xh[2 * blk], p.nw[2 * blk], p.nb[2 * blk], y);
      vm_linear<64>(p.w[2 * blk + 1], nullptr, 0.125f, y, col, xh[2 * blk + 1]);
      rstd[2 * blk + 1] = vm_normalise(xh[2 * blk + 1]);
      vm_affine_act(xh[2 * blk + 1], p.nw[2 * blk + 1], p.nb[2 * blk + 1], y);
#pragma unroll
      for (int k = 0; k < 64; ++k) x[k] = (y[k] + x[k]) * kVmJoin;
    }
    vm_linear<64>(p.w5, p.b5, 0.125f, x, col, a5);
#pragma unroll
    for (int k = 0; k < 64; ++k) a5[k] = vm_lrelu(a5[k]);
  }

  // ---- fc6 ----
  float g[64], gx[64], x[64];
  {
    float go[32];
    const float4* up = reinterpret_cast<const float4*>(p.g_feature + 32 * src);
#pragma unroll
    for (int j = 0; j < 32; j += 4) {
      const float4 u = live ? up[j >> 2] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      go[j] = u.x; go[j + 1] = u.y; go[j + 2] = u.z; go[j + 3] = u.w;
    }
    const float sb = vm_put_rows<32>(go, rows);
    if (wp) {
      if (t < 32) unsafeAtomicAdd(&p.g_b6[t], sb);
      vm_weight_grad<32>(a5, rows, cols, 0.125f, p.g_w6);
    }
    vm_input_grad<32>(p.w6, 0.125f, rows, g);
  }
  // ---- fc5: input x = the second join's output ----
#pragma unroll
  for (int k = 0; k < 64; ++k) g[k] = a5[k] > 0.0f ? g[k] : g[k] * kVmSlope;
  {
    float y[64];
    vm_affine_act(xh[1], p.nw[1], p.nb[1], y);
#pragma unroll
    for (int k = 0; k < 64; ++k) x[k] = (y[k] + a0[k]) * kVmJoin;           // first join
    vm_affine_act(xh[3], p.nw[3], p.nb[3], y);
#pragma unroll
    for (int k = 0; k < 64; ++k) y[k] = (y[k] + x[k]) * kVmJoin;            // second join
    const float sb = vm_put_rows<64>(g, rows);
    if (wp) {
      unsafeAtomicAdd(&p.g_b5[t], sb);
      vm_weight_grad<64>(y, rows, cols, 0.125f, p.g_w5);
    }
  }
  vm_input_grad<64>(p.w5, 0.125f, rows, gx);
  // ---- the two residual blocks, last first.  gx: gradient w.r.t. the block's output; x: the FIRST join's output ----
#pragma unroll
  for (int blk = 1; blk >= 0; --blk) {
    float gs[64];                    // the shortcut's share
#pragma unroll
    for (int k = 0; k < 64; ++k) { gs[k] = gx[k] * kVmJoin; g[k] = gs[k]; }
    // second layer of the block: input = lrelu(affine(xh[2 blk]))
    vm_norm_bwd(g, xh[2 * blk + 1], rstd[2 * blk + 1], p.nw[2 * blk + 1], p.nb[2 * blk + 1], rows, p.g_nw[2 * blk + 1], p.g_nb[2 * blk + 1], wp);
    {
      float y[64];
      vm_affine_act(xh[2 * blk], p.nw[2 * blk], p.nb[2 * blk], y);
      vm_put_rows<64>(g, rows);
      if (wp) vm_weight_grad<64>(y, rows, cols, 0.125f, p.g_w[2 * blk + 1]);
    }
    vm_input_grad<64>(p.w[2 * blk + 1], 0.125f, rows, g);
    // first layer of the block: input = the block's input (blk 1: the first join's output x; blk 0: a0)
    vm_norm_bwd(g, xh[2 * blk], rstd[2 * blk], p.nw[2 * blk], p.nb[2 * blk], rows, p.g_nw[2 * blk], p.g_nb[2 * blk], wp);
    vm_put_rows<64>(g, rows);
    if (wp && blk == 1) vm_weight_grad<64>(x, rows, cols, 0.125f, p.g_w[2]);
    if (wp && blk == 0) vm_weight_grad<64>(a0, rows, cols, 0.125f, p.g_w[0]);
    vm_input_grad<64>(p.w[2 * blk], 0.125f, rows, gx);
#pragma unroll
    for (int k = 0; k < 64; ++k) gx[k] += gs[k];
  }
  // ---- fc0 ----
#pragma unroll
  for (int k = 0; k < 64; ++k) g[k] = a0[k] > 0.0f ? gx[k] : gx[k] * kVmSlope;
  const float gain0 = 0.57735026918962576451f;
  if (wp) {
    const float sb0 = vm_put_rows<64>(g, rows);
    unsafeAtomicAdd(&p.g_b0[t], sb0);
    float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f;       // row t of g_fc0_w
    for (int r = 0; r < kVmRays; ++r) {
      const float gr = rows[r * kVmRow + t];
      w0 = fmaf(gr, vdir[3 * r], w0); w1 = fmaf(gr, vdir[3 * r + 1], w1); w2 = fmaf(gr, vdir[3 * r + 2], w2);
    }
    unsafeAtomicAdd(&p.g_w0[3 * t], w0 * gain0);
    unsafeAtomicAdd(&p.g_w0[3 * t + 1], w1 * gain0);
    unsafeAtomicAdd(&p.g_w0[3 * t + 2], w2 * gain0);
  }
  if (p.g_viewdir && live) {
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      d0 = fmaf(p.w0[3 * j] * gain0, g[j], d0); d1 = fmaf(p.w0[3 * j + 1] * gain0, g[j], d1); d2 = fmaf(p.w0[3 * j + 2] * gain0, g[j], d2);
    }
    p.g_viewdir[3 * ray] = d0; p.g_viewdir[3 * ray + 1] = d1; p.g_viewdir[3 * ray + 2] = d2;
  }
}

static int viewdir_mapper_common(const nfi_viewdir_mapper_args* a, VmParams& k, const char* null_msg) {
  REQUIRE(a && a->viewdir && a->fc0_w && a->fc0_b && a->fc1_w && a->norm1_w && a->norm1_b && a->fc2_w && a->norm2_w && a->norm2_b &&
              a->fc3_w && a->norm3_w && a->norm3_b && a->fc4_w && a->norm4_w && a->norm4_b && a->fc5_w && a->fc5_b && a->fc6_w && a->fc6_b,
          null_msg);
  REQUIRE(a->n_rays > 0 && a->n_rays <= ((int64_t)1 << 36), "viewdir_mapper: n_rays must be in [1, 2^36]");
  memset(&k, 0, sizeof(k));
  k.n = a->n_rays; k.viewdir = a->viewdir;
  k.w0 = a->fc0_w; k.b0 = a->fc0_b;
  k.w[0] = a->fc1_w; k.w[1] = a->fc2_w; k.w[2] = a->fc3_w; k.w[3] = a->fc4_w;
  k.nw[0] = a->norm1_w; k.nw[1] = a->norm2_w; k.nw[2] = a->norm3_w; k.nw[3] = a->norm4_w;
  k.nb[0] = a->norm1_b; k.nb[1] = a->norm2_b; k.nb[2] = a->norm3_b; k.nb[3] = a->norm4_b;
  k.w5 = a->fc5_w; k.b5 = a->fc5_b; k.w6 = a->fc6_w; k.b6 = a->fc6_b;
  return NFI_OK;
}

extern "C" int nfi_viewdir_mapper_fwd(const nfi_viewdir_mapper_args* a, nfi_stream_t stream) {
  VmParams k;
  int rc = viewdir_mapper_common(a, k, "viewdir_mapper_fwd: null pointer");
  if (rc) return rc;
  REQUIRE(a->feature, "viewdir_mapper_fwd: null output pointer");
  k.feature = a->feature;
  const dim3 grid((unsigned)((a->n_rays + kVmRays - 1) / kVmRays));
  hipLaunchKernelGGL(viewdir_mapper_fwd_kernel, grid, dim3(kVmRays), 0, (hipStream_t)stream, k);
  return check_launch("viewdir_mapper_fwd");
}

extern "C" int nfi_viewdir_mapper_bwd(const nfi_viewdir_mapper_args* a, nfi_stream_t stream) {
  VmParams k;
  int rc = viewdir_mapper_common(a, k, "viewdir_mapper_bwd: null pointer");
  if (rc) return rc;
  REQUIRE(a->g_feature, "viewdir_mapper_bwd: null upstream gradient");
  float* const gp[18] = {a->g_fc0_w, a->g_fc0_b, a->g_fc1_w, a->g_norm1_w, a->g_norm1_b, a->g_fc2_w, a->g_norm2_w, a->g_norm2_b, a->g_fc3_w,
                         a->g_norm3_w, a->g_norm3_b, a->g_fc4_w, a->g_norm4_w, a->g_norm4_b, a->g_fc5_w, a->g_fc5_b, a->g_fc6_w, a->g_fc6_b};
  int given = 0;
  for (float* q : gp) given += q != nullptr;
  REQUIRE(given == 18 || given == 0, "viewdir_mapper_bwd: null parameter-gradient pointer (all 18 or none)");
  REQUIRE(given == 18 || a->g_viewdir, "viewdir_mapper_bwd: null output pointers: nothing to compute");
  k.g_feature = a->g_feature;
  k.g_w0 = a->g_fc0_w; k.g_b0 = a->g_fc0_b;
  k.g_w[0] = a->g_fc1_w; k.g_w[1] = a->g_fc2_w; k.g_w[2] = a->g_fc3_w; k.g_w[3] = a->g_fc4_w;
  k.g_nw[0] = a->g_norm1_w; k.g_nw[1] = a->g_norm2_w; k.g_nw[2] = a->g_norm3_w; k.g_nw[3] = a->g_norm4_w;
  k.g_nb[0] = a->g_norm1_b; k.g_nb[1] = a->g_norm2_b; k.g_nb[2] = a->g_norm3_b; k.g_nb[3] = a->g_norm4_b;
  k.g_w5 = a->g_fc5_w; k.g_b5 = a->g_fc5_b; k.g_w6 = a->g_fc6_w; k.g_b6 = a->g_fc6_b;
  k.g_viewdir = a->g_viewdir;
  const dim3 grid((unsigned)((a->n_rays + kVmRays - 1) / kVmRays));
  hipLaunchKernelGGL(viewdir_mapper_bwd_kernel, grid, dim3(kVmRays), 0, (hipStream_t)stream, k);
  return check_launch("viewdir_mapper_bwd");
}
