// nfi_regulariser.inc — the distance field and its spatial gradient as ONE differentiable operator
// (included by nfi_modules.hip).
//
// Reference: the regulariser branch of Generator.forward (models/generator.py:505-585).  The eikonal term needs
// x_grad = d(sdf)/d(x_in) WITH a graph (torch.autograd.grad(..., create_graph=True), 534-540), which is why the
// reference re-implements grid_sample with double-differentiation support (lib/ops.py:58-120).  Here the gradient
// is an explicit second OUTPUT of the operator,
//
//      (x, planes, W1, b1, w2[0], b2[0])  ->  d = sdf(x)  [B,P],   g = d sdf / d x  [B,P,3]
//
// so its backward kernel below IS the double backward.  With f = mean of the three bilinear plane samples,
// J = df/dx (piecewise constant in the texels' differences), h = W1' f + b1, s = softplus(h), sg = sigmoid(h):
//      d = w2'.s + b2,          g = J^T v,  v = W1'^T (sg * w2')
// and for upstream gradients (dd, dg), with q = J dg and a = W1' q:
//      dh  = (w2' * a) * sg (1 - sg) + dd * w2' * sg
//      dW1' += dh f^T + (sg * w2') q^T          db1 += dh          dw2' += sg * a + dd * s       db2 += dd
//      df  = W1'^T dh   (scattered with the bilinear weights)      dJ = v dg^T   (scattered with the weights' x-derivatives)
// The workload is small (31^3 points per scene, generator.py:509) and scattered over the whole planes.  Both kernels
// work on 16-point tiles with the decoder on the 16-bit matrix pipe (split-fp16 operands, as the field kernels); the
// weight gradients are accumulated per wave over all its chunks (one flush), and the plane gradients are scattered one
// point per atomic instruction (full lines) - 12 line updates per point, which is what bounds the backward: 4 x 31^3
// points = 1.43 M line updates = 170 us of the atomic units' time (tools/probes/atomic_scatter.hip).
// Points are expected strictly inside the cube (they are stratified samples of it, lib/ops.py:20-26); like
// lib/ops.grid_sample2d no coordinate clamp is applied beyond keeping the texel indices in range.

struct SdfGradParams {
  const float* points; int64_t P; int n_scenes;
  const float* texels; int res; float scene_range;
  const float* w1; const float* b1; const float* w2; const float* b2;     // raw parameters (row 0 of w2 / b2 is used)
  float* d; float* g;                                                        // forward outputs
  const float* gd; const float* gg;                                          // backward: upstream gradients
  float* g_texels; float* g_w1; float* g_b1; float* g_w2; float* g_b2;
  int layout;                  // texel layout (nfi_device.hpp): strides below, in floats
  // ordered backward only (nfi_sdf_gradient_bwd_ordered): regions of its workspace
  float* ord_df; float* ord_v;         // [scene][point][32]: a point's df row (W1'^T dh) and v row (W1'^T (sg w2'))
  uint8_t* ord_flag;                   // [scene][point]: 1 = the rows are written and count
  float* ord_slots;                    // [wave slot][kRgSlotFloats]: a wave's weight-gradient sums
  const uint64_t* ord_keys;            // [scene * 3 + plane][point]: (cell << 32 | point), sorted by cell for the gather
  __device__ __forceinline__ size_t pix_f() const { return layout ? 3 * kC : kC; }
  __device__ __forceinline__ size_t plane_f() const { return layout ? (size_t)kC : (size_t)res * res * kC; }
};

// texel index + fraction along one axis, as lib/ops.grid_sample2d computes them
__device__ __forceinline__ void reg_coord(float p, float scene_range, int res, int& i0, float& fr) {
  const float u = ((p / scene_range + 1.0f) / 2.0f) * (float)(res - 1);
  float fl = floorf(u);
  fl = fminf(fmaxf(fl, 0.0f), (float)(res - 2));
  i0 = (int)fl;
  fr = u - fl;
}

// ---- MFMA form of the operator (16 points per tile, 4 lanes per point in the gather; see the backward's header) ----
constexpr int kRgW1H = 0, kRgW1T = 2048, kRgB1 = 4096, kRgW2 = 4160, kRgStage = 4224;     // floats
constexpr int kRgWaveFloats = 3840;                                                        // 15 360 B per wave
constexpr int kRgFT = 0, kRgQT = 2304;                                                     // bytes: fp32 [16][36] tiles (R0)
constexpr int kRgF16Hi = 0, kRgF16Lo = 1536, kRgQ16Hi = 3072, kRgQ16Lo = 4608;            // bytes: fp16 [16][48] tiles (R0)
constexpr int kRgR1 = 6144;
constexpr int kRgDH16Hi = kRgR1, kRgDH16Lo = kRgR1 + 2304, kRgSW16Hi = kRgR1 + 4608, kRgSW16Lo = kRgR1 + 6912;   // fp16 [16][72]
constexpr int kRgDFRows = kRgR1, kRgVRows = kRgR1 + 2304;                                  // fp32 [16][36] (after the MFMAs)
constexpr int kRgLdsFloats = kRgStage + 4 * kRgWaveFloats;

// W1' (gain applied) as fp16 hi / lo A fragments: [nt][hi|lo][lane] of H = W1' F (K = channels in the MFMA layout's slot
// order) and [n2][kk][hi|lo][lane] of X = W1'^T Y (K = hidden units in the accumulator layout's order); b1, w2' plain.
__device__ __forceinline__ void reg_stage_fragments(float* dyn, const SdfGradParams& k) {
  const float gain1 = 0.17677669529663687f, gain2 = 0.125f;
  for (int idx = threadIdx.x; idx < 512; idx += blockDim.x) {
    const int l = idx & 63, lg = l >> 4, lj = l & 15;
    float x[8];
    f16x8 hi, lo;
    if (idx < 256) {
      const int nt = idx >> 6;
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = k.w1[(16 * nt + lj) * 32 + (i < 4 ? 4 * lg + i : 16 + 4 * lg + i - 4)] * gain1;
      split_f16x8(x, hi, lo);
      reinterpret_cast<u32x4*>(dyn + kRgW1H)[(nt * 2 + 0) * 64 + l] = __builtin_bit_cast(u32x4, hi);
      reinterpret_cast<u32x4*>(dyn + kRgW1H)[(nt * 2 + 1) * 64 + l] = __builtin_bit_cast(u32x4, lo);
    } else {
      const int n2 = (idx >> 7) & 1, kk = (idx >> 6) & 1;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        x[i] = k.w1[(i < 4 ? 32 * kk + 4 * lg + i : 32 * kk + 16 + 4 * lg + i - 4) * 32 + 16 * n2 + lj] * gain1;
      split_f16x8(x, hi, lo);
      reinterpret_cast<u32x4*>(dyn + kRgW1T)[((n2 * 2 + kk) * 2 + 0) * 64 + l] = __builtin_bit_cast(u32x4, hi);
      reinterpret_cast<u32x4*>(dyn + kRgW1T)[((n2 * 2 + kk) * 2 + 1) * 64 + l] = __builtin_bit_cast(u32x4, lo);
    }
  }
  if (threadIdx.x < 64) { dyn[kRgB1 + threadIdx.x] = k.b1[threadIdx.x]; dyn[kRgW2 + threadIdx.x] = k.w2[threadIdx.x] * gain2; }
  __syncthreads();
}

constexpr int kRgFwdWaveFloats = 2 * 16 * 36;            // F_T, then the V rows
constexpr int kRgFwdLdsFloats = kRgStage + 4 * kRgFwdWaveFloats;

__global__ __launch_bounds__(256, 2) void sdf_gradient_fwd_kernel(SdfGradParams k) {
  __shared__ __attribute__((aligned(16))) float dyn[kRgFwdLdsFloats];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4, lp = lane >> 2, lq = lane & 3;
  reg_stage_fragments(dyn, k);
  const u32x4* w1h = reinterpret_cast<const u32x4*>(dyn + kRgW1H);
  const u32x4* w1t = reinterpret_cast<const u32x4*>(dyn + kRgW1T);
  float* ft = dyn + kRgStage + wave * kRgFwdWaveFloats;
  float* vr = ft + 16 * 36;
  const int scene = blockIdx.y;
  const float* tex_scene = k.texels + (size_t)scene * 3 * k.res * k.res * kC;
  const float scale = (float)(k.res - 1) / (2.0f * k.scene_range);
  const float third = 1.0f / 3.0f;
  const size_t pix_f = k.pix_f(), plane_f = k.plane_f(), row_f = (size_t)k.res * pix_f;
  const float b2 = k.b2[0];
  const int64_t n_chunks = (k.P + 63) / 64;
  for (int64_t chunk = (int64_t)blockIdx.x * 4 + wave; chunk < n_chunks; chunk += (int64_t)gridDim.x * 4) {
    const int64_t p = chunk * 64 + lane;
    const bool valid = p < k.P;
    const size_t gi = (size_t)scene * k.P + (valid ? p : 0);
    int i0[3];
    float fr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) reg_coord(k.points[gi * 3 + a], k.scene_range, k.res, i0[a], fr[a]);
    const int xi = (int)((uint32_t)i0[0] | ((uint32_t)i0[1] << 10) | ((uint32_t)i0[2] << 20));
    const uint64_t live = __ballot(valid);
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
      if (((live >> (16 * t)) & 0xFFFFull) == 0) continue;
      const int srcL = 16 * t + lp;
      const uint32_t cxi = (uint32_t)__shfl(xi, srcL, 64);
      const float cfr[3] = {__shfl(fr[0], srcL, 64), __shfl(fr[1], srcL, 64), __shfl(fr[2], srcL, 64)};
      // gather: f and J = df/dx (texel units) of this lane's 8 channels
      float f[8], J[8][3];
#pragma unroll
      for (int s = 0; s < 8; ++s) { f[s] = 0.0f; J[s][0] = J[s][1] = J[s][2] = 0.0f; }
      {
        const int c0[3] = {(int)(cxi & 1023u), (int)((cxi >> 10) & 1023u), (int)((cxi >> 20) & 1023u)};
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          const int aa = (pl == 2) ? 1 : 0, ab = (pl == 0) ? 1 : 2;
          const float fa = cfr[aa], fb = cfr[ab];
          const float* t00 = tex_scene + (size_t)pl * plane_f + ((size_t)c0[ab] * k.res + c0[aa]) * pix_f + 4 * lq;
          const f32x4 x00[2] = {*reinterpret_cast<const f32x4*>(t00), *reinterpret_cast<const f32x4*>(t00 + 16)};
          const f32x4 x10[2] = {*reinterpret_cast<const f32x4*>(t00 + pix_f), *reinterpret_cast<const f32x4*>(t00 + pix_f + 16)};
          const f32x4 x01[2] = {*reinterpret_cast<const f32x4*>(t00 + row_f), *reinterpret_cast<const f32x4*>(t00 + row_f + 16)};
          const f32x4 x11[2] = {*reinterpret_cast<const f32x4*>(t00 + row_f + pix_f), *reinterpret_cast<const f32x4*>(t00 + row_f + pix_f + 16)};
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            const float v00 = x00[s >> 2][s & 3], v10 = x10[s >> 2][s & 3], v01 = x01[s >> 2][s & 3], v11 = x11[s >> 2][s & 3];
            f[s] += third * ((1.0f - fa) * (1.0f - fb) * v00 + fa * (1.0f - fb) * v10 + (1.0f - fa) * fb * v01 + fa * fb * v11);
            J[s][aa] += third * ((1.0f - fb) * (v10 - v00) + fb * (v11 - v01));
            J[s][ab] += third * ((1.0f - fa) * (v01 - v00) + fa * (v11 - v10));
          }
        }
      }
      // load layout -> MFMA layout
      float feat[8];
      wave_lds_fence();
      *reinterpret_cast<f32x4*>(ft + lp * 36 + 4 * lq) = f32x4{f[0], f[1], f[2], f[3]};
      *reinterpret_cast<f32x4*>(ft + lp * 36 + 16 + 4 * lq) = f32x4{f[4], f[5], f[6], f[7]};
      wave_lds_fence();
      {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(ft + j * 36 + 4 * g), a1 = *reinterpret_cast<const f32x4*>(ft + j * 36 + 16 + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) { feat[i] = a0[i]; feat[4 + i] = a1[i]; }
      }
      f16x8 fh, fl;
      split_f16x8(feat, fh, fl);
      // H = W1' F + b1 ; s = softplus, sg = sigmoid ; d = w2'.s + b2 ; sw = sg w2'
      f32x4 swv[4];
      float dpart = 0.0f, am_sw = 0.0f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const f16x8 wh = __builtin_bit_cast(f16x8, w1h[(nt * 2 + 0) * 64 + lane]);
        const f16x8 wl = __builtin_bit_cast(f16x8, w1h[(nt * 2 + 1) * 64 + lane]);
        f32x4 hacc = *reinterpret_cast<const f32x4*>(dyn + kRgB1 + 16 * nt + 4 * g);
        hacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, fh, hacc, 0, 0, 0);
        hacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, fl, hacc, 0, 0, 0);
        hacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, fh, hacc, 0, 0, 0);
        const f32x4 w2v = *reinterpret_cast<const f32x4*>(dyn + kRgW2 + 16 * nt + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float h = hacc[r];
          const float e = __builtin_amdgcn_exp2f(h * 1.4426950408889634f);
          const float tt = 1.0f + e;
          const float s = (h > 20.0f) ? h : __builtin_amdgcn_logf(tt) * 0.6931471805599453f;
          const float sg = 1.0f - __builtin_amdgcn_rcpf(tt);
          dpart = fmaf(w2v[r], s, dpart);
          swv[nt][r] = sg * w2v[r];
          am_sw = fmaxf(am_sw, fabsf(swv[nt][r]));
        }
      }
      const float dval = sum_xor32(sum_xor16(dpart)) + b2;        // over the four hidden groups of point j
      am_sw = max_xor32(max_xor16(am_sw));
      // V = W1'^T SW
      f32x4 v0 = {0, 0, 0, 0}, v1 = {0, 0, 0, 0};
      float ssc, s_inv;
      pow2_normaliser(am_sw, ssc, s_inv);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const float xs[8] = {swv[2 * kk][0] * ssc, swv[2 * kk][1] * ssc, swv[2 * kk][2] * ssc, swv[2 * kk][3] * ssc,
                             swv[2 * kk + 1][0] * ssc, swv[2 * kk + 1][1] * ssc, swv[2 * kk + 1][2] * ssc, swv[2 * kk + 1][3] * ssc};
        f16x8 sh, sl;
        split_f16x8(xs, sh, sl);
        const f16x8 ah = __builtin_bit_cast(f16x8, w1t[((0 * 2 + kk) * 2 + 0) * 64 + lane]);
        const f16x8 al = __builtin_bit_cast(f16x8, w1t[((0 * 2 + kk) * 2 + 1) * 64 + lane]);
        const f16x8 bh = __builtin_bit_cast(f16x8, w1t[((1 * 2 + kk) * 2 + 0) * 64 + lane]);
        const f16x8 bl = __builtin_bit_cast(f16x8, w1t[((1 * 2 + kk) * 2 + 1) * 64 + lane]);
        v0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, sh, v0, 0, 0, 0);
        v1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, sh, v1, 0, 0, 0);
        v0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, sl, v0, 0, 0, 0);
        v1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, sl, v1, 0, 0, 0);
        v0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, sh, v0, 0, 0, 0);
        v1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl, sh, v1, 0, 0, 0);
      }
      // MFMA layout -> load layout ; g = J^T v (8 channels per lane, 4 lanes per point)
      *reinterpret_cast<f32x4*>(vr + j * 36 + 4 * g) = v0 * s_inv;
      *reinterpret_cast<f32x4*>(vr + j * 36 + 16 + 4 * g) = v1 * s_inv;
      wave_lds_fence();
      {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(vr + lp * 36 + 4 * lq), a1 = *reinterpret_cast<const f32x4*>(vr + lp * 36 + 16 + 4 * lq);
        float gacc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const float vv = s < 4 ? a0[s & 3] : a1[s & 3];
          gacc[0] = fmaf(J[s][0], vv, gacc[0]); gacc[1] = fmaf(J[s][1], vv, gacc[1]); gacc[2] = fmaf(J[s][2], vv, gacc[2]);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          gacc[a] += dpp_f32<kDppQuadXor1>(0.0f, gacc[a]);
          gacc[a] += dpp_f32<kDppQuadXor2>(0.0f, gacc[a]);
        }
        const int64_t pL = chunk * 64 + srcL;
        if (lq == 0 && pL < k.P) {
          float* go = k.g + ((size_t)scene * k.P + pL) * 3;
          go[0] = gacc[0] * scale; go[1] = gacc[1] * scale; go[2] = gacc[2] * scale;
        }
      }
      const int64_t pM = chunk * 64 + 16 * t + j;
      if (g == 0 && pM < k.P) k.d[(size_t)scene * k.P + pM] = dval;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Backward (= the double backward of the reference's graph) on the matrix cores, 16 points per tile like the field
// kernels: gather f and its Jacobian J in the load layout (4 lanes per point, 8 channels each), q = J u; f, q go to the
// MFMA layout through LDS; H = W1' F and A = W1' Q, V = W1'^T SW and DF = W1'^T DH on v_mfma_f32_16x16x32_f16 with
// split-fp16 operands (gradient-side operands normalised per point, nfi_device.hpp); dW1' += DH F^T + SW Q^T with the
// point index on K through fp16 point-major tiles and ds_read_b64_tr_b16 (nfi_backward_field.inc); bias-type sums
// (db1, dw2') stay one partial per lane until the flush; the plane gradients are scattered one point per atomic
// instruction (64 consecutive floats = 2 full lines).  Round 1-3: one lane = one point with the MLP as scalar loops over
// LDS-broadcast weights, 256 VGPRs, one wave per SIMD: 358 us for 4 x 31^3 points.
// ------------------------------------------------------------------------------------------------
#ifndef NFI_REG_OCC
#define NFI_REG_OCC 1                      // workgroups per CU of the regulariser backward (2: 256 VGPRs with 96 B of scratch)
#endif

// a wave's slot of the ordered variant (floats): g_w1 [64][32], g_b1 [64], g_w2 row 0 [64], g_b2 [1], padded to 16
constexpr int kRgSlotW1 = 0, kRgSlotB1 = 2048, kRgSlotW2 = 2112, kRgSlotB2 = 2176, kRgSlotFloats = 2192;

// ORDERED (nfi_sdf_gradient_bwd_ordered, the scheme of nfi_backward_field.inc's ordered mode): no atomic at all - the
// plane-gradient loop is replaced by a coalesced store of the tile's df and v rows (and a live flag per point) for
// sdf_ord_gather_kernel, and the flush writes the wave's sums into its own slot for sdf_slot_finish_kernel.
template <bool ORDERED>
__global__ __launch_bounds__(256, NFI_REG_OCC) void sdf_gradient_bwd_kernel(SdfGradParams k) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  typedef unsigned long long u64;
  typedef u64 u64x2 __attribute__((ext_vector_type(2)));
  const float gain1 = 0.17677669529663687f, gain2 = 0.125f;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4, lp = lane >> 2, lq = lane & 3;
  reg_stage_fragments(dyn, k);
  const u32x4* w1h = reinterpret_cast<const u32x4*>(dyn + kRgW1H);
  const u32x4* w1t = reinterpret_cast<const u32x4*>(dyn + kRgW1T);
  char* wb = reinterpret_cast<char*>(dyn + kRgStage + wave * kRgWaveFloats);
  const int scene = blockIdx.y;
  const float* tex_scene = k.texels + (size_t)scene * 3 * k.res * k.res * kC;
  float* gtex_scene = k.g_texels + (size_t)scene * 3 * k.res * k.res * kC;
  const float scale = (float)(k.res - 1) / (2.0f * k.scene_range);
  const float third = 1.0f / 3.0f;
  const size_t pix_f = k.pix_f(), plane_f = k.plane_f(), row_f = (size_t)k.res * pix_f;
  // accumulators: dW1' [hidden tile][channel tile] (rows 4g + r, column j) in units of 1 / (sticky scale es); db1 / dw2'
  // one partial per lane (hidden unit 16 nt + 4 g + r, summed over this lane's point column at the flush)
  f32x4 dW1[4][2], db1a[4], dw2a[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    dW1[nt][0] = f32x4{0, 0, 0, 0}; dW1[nt][1] = f32x4{0, 0, 0, 0};
    db1a[nt] = f32x4{0, 0, 0, 0}; dw2a[nt] = f32x4{0, 0, 0, 0};
  }
  float db2 = 0.0f;
  int es = 0, et_max = 0;
  const int64_t n_chunks = (k.P + 63) / 64;
  for (int64_t chunk = (int64_t)blockIdx.x * 4 + wave; chunk < n_chunks; chunk += (int64_t)gridDim.x * 4) {
    const int64_t p = chunk * 64 + lane;
    const bool valid = p < k.P;
    const size_t gi = (size_t)scene * k.P + (valid ? p : 0);
    int i0[3];
    float fr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) reg_coord(k.points[gi * 3 + a], k.scene_range, k.res, i0[a], fr[a]);
    const float dd = (valid && k.gd) ? k.gd[gi] : 0.0f;
    float u[3] = {0.0f, 0.0f, 0.0f};
    if (valid && k.gg) { u[0] = k.gg[gi * 3] * scale; u[1] = k.gg[gi * 3 + 1] * scale; u[2] = k.gg[gi * 3 + 2] * scale; }
    db2 += dd;
    if constexpr (ORDERED) { if (valid) k.ord_flag[gi] = 1; }        // (every point below P is live: none is skipped)
    const int xi = (int)((uint32_t)i0[0] | ((uint32_t)i0[1] << 10) | ((uint32_t)i0[2] << 20));
    const uint64_t live = __ballot(valid);
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
      if (((live >> (16 * t)) & 0xFFFFull) == 0) continue;
      const int srcL = 16 * t + lp, srcM = 16 * t + j;
      const uint32_t cxi = (uint32_t)__shfl(xi, srcL, 64);
      const float cfr[3] = {__shfl(fr[0], srcL, 64), __shfl(fr[1], srcL, 64), __shfl(fr[2], srcL, 64)};
      const float cu[3] = {__shfl(u[0], srcL, 64), __shfl(u[1], srcL, 64), __shfl(u[2], srcL, 64)};
      const bool vM = ((live >> srcM) & 1ull) != 0;
      const float ddM = __shfl(dd, srcM, 64);
      // ---------------- gather: f and q = J u (J = df/dx in texel units) for this lane's 8 channels, one plane at a time ----------------
      float f[8], q[8];
      {
#pragma unroll
        for (int s = 0; s < 8; ++s) { f[s] = 0.0f; q[s] = 0.0f; }
        const int c0[3] = {(int)(cxi & 1023u), (int)((cxi >> 10) & 1023u), (int)((cxi >> 20) & 1023u)};
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          const int aa = (pl == 2) ? 1 : 0, ab = (pl == 0) ? 1 : 2;
          const float fa = cfr[aa], fb = cfr[ab], ua = cu[aa], ub = cu[ab];
          const float* t00 = tex_scene + (size_t)pl * plane_f + ((size_t)c0[ab] * k.res + c0[aa]) * pix_f + 4 * lq;
          const f32x4 x00[2] = {*reinterpret_cast<const f32x4*>(t00), *reinterpret_cast<const f32x4*>(t00 + 16)};
          const f32x4 x10[2] = {*reinterpret_cast<const f32x4*>(t00 + pix_f), *reinterpret_cast<const f32x4*>(t00 + pix_f + 16)};
          const f32x4 x01[2] = {*reinterpret_cast<const f32x4*>(t00 + row_f), *reinterpret_cast<const f32x4*>(t00 + row_f + 16)};
          const f32x4 x11[2] = {*reinterpret_cast<const f32x4*>(t00 + row_f + pix_f), *reinterpret_cast<const f32x4*>(t00 + row_f + pix_f + 16)};
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            const float v00 = x00[s >> 2][s & 3], v10 = x10[s >> 2][s & 3], v01 = x01[s >> 2][s & 3], v11 = x11[s >> 2][s & 3];
            f[s] += third * ((1.0f - fa) * (1.0f - fb) * v00 + fa * (1.0f - fb) * v10 + (1.0f - fa) * fb * v01 + fa * fb * v11);
            const float ja = (1.0f - fb) * (v10 - v00) + fb * (v11 - v01);         // d / d(first axis of the plane)
            const float jb = (1.0f - fa) * (v01 - v00) + fa * (v11 - v10);         // d / d(second axis)
            q[s] += third * (ja * ua + jb * ub);
          }
          __builtin_amdgcn_sched_barrier(0);         // keep the three planes' loads from being hoisted together (registers)
        }
      }
      // ---------------- load layout -> MFMA layout (lane (g, j): point j, channels 4g..4g+3 and 16+4g..16+4g+3) ----------------
      float feat[8], qm[8];
      {
        float* ft = reinterpret_cast<float*>(wb + kRgFT);
        float* qt = reinterpret_cast<float*>(wb + kRgQT);
        wave_lds_fence();
        *reinterpret_cast<f32x4*>(ft + lp * 36 + 4 * lq) = f32x4{f[0], f[1], f[2], f[3]};
        *reinterpret_cast<f32x4*>(ft + lp * 36 + 16 + 4 * lq) = f32x4{f[4], f[5], f[6], f[7]};
        *reinterpret_cast<f32x4*>(qt + lp * 36 + 4 * lq) = f32x4{q[0], q[1], q[2], q[3]};
        *reinterpret_cast<f32x4*>(qt + lp * 36 + 16 + 4 * lq) = f32x4{q[4], q[5], q[6], q[7]};
        wave_lds_fence();
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(ft + j * 36 + 4 * g), a1 = *reinterpret_cast<const f32x4*>(ft + j * 36 + 16 + 4 * g);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(qt + j * 36 + 4 * g), b1 = *reinterpret_cast<const f32x4*>(qt + j * 36 + 16 + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) { feat[i] = a0[i]; feat[4 + i] = a1[i]; qm[i] = b0[i]; qm[4 + i] = b1[i]; }
        wave_lds_fence();
      }
      f16x8 fh, fl, qh, ql;
      float q_inv, am_q = 0.0f;
      split_f16x8(feat, fh, fl);
      {
#pragma unroll
        for (int i = 0; i < 8; ++i) am_q = fmaxf(am_q, fabsf(qm[i]));
        am_q = max_xor32(max_xor16(am_q));                      // over the 32 channels of point j
        float qs;
        pow2_normaliser(am_q, qs, q_inv);
        const float x8[8] = {qm[0] * qs, qm[1] * qs, qm[2] * qs, qm[3] * qs, qm[4] * qs, qm[5] * qs, qm[6] * qs, qm[7] * qs};
        split_f16x8(x8, qh, ql);
      }
      {
        // F16 tiles (B operand of dW1' += DH F^T) over the fp32 tiles just read
        const u64x2 h2 = __builtin_bit_cast(u64x2, fh), l2 = __builtin_bit_cast(u64x2, fl);
        char* t16 = wb + j * 96 + 8 * g;
        *reinterpret_cast<u64*>(t16 + kRgF16Hi) = h2[0]; *reinterpret_cast<u64*>(t16 + kRgF16Hi + 32) = h2[1];
        *reinterpret_cast<u64*>(t16 + kRgF16Lo) = l2[0]; *reinterpret_cast<u64*>(t16 + kRgF16Lo + 32) = l2[1];
      }
      // ---------------- H = W1' F + b1, A = W1' Q ; s, sg ; sw = sg w2', dh ----------------
      f32x4 dhv[4], swv[4];
      float am_dh = 0.0f, am_sw = 0.0f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const f16x8 wh = __builtin_bit_cast(f16x8, w1h[(nt * 2 + 0) * 64 + lane]);
        const f16x8 wl = __builtin_bit_cast(f16x8, w1h[(nt * 2 + 1) * 64 + lane]);
        f32x4 hacc = *reinterpret_cast<const f32x4*>(dyn + kRgB1 + 16 * nt + 4 * g);
        f32x4 aacc = {0.0f, 0.0f, 0.0f, 0.0f};
        hacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, fh, hacc, 0, 0, 0);
        aacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, qh, aacc, 0, 0, 0);
        hacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, fl, hacc, 0, 0, 0);
        aacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, ql, aacc, 0, 0, 0);
        hacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, fh, hacc, 0, 0, 0);
        aacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, qh, aacc, 0, 0, 0);
        const f32x4 w2v = *reinterpret_cast<const f32x4*>(dyn + kRgW2 + 16 * nt + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float h = hacc[r], a = aacc[r] * q_inv;
          const float e = __builtin_amdgcn_exp2f(h * 1.4426950408889634f);
          const float tt = 1.0f + e;
          const float rc = __builtin_amdgcn_rcpf(tt);
          const float s = (h > 20.0f) ? h : __builtin_amdgcn_logf(tt) * 0.6931471805599453f;
          const float sg = 1.0f - rc;
          const float sw = sg * w2v[r];
          const float dh = vM ? ((w2v[r] * a) * (sg * rc) + ddM * sw) : 0.0f;
          dhv[nt][r] = dh;
          swv[nt][r] = vM ? sw : 0.0f;
          db1a[nt][r] += dh;
          dw2a[nt][r] += vM ? (sg * a + ddM * s) : 0.0f;
          am_dh = fmaxf(am_dh, fabsf(dh));
          am_sw = fmaxf(am_sw, fabsf(swv[nt][r]));
        }
      }
      am_dh = max_xor32(max_xor16(am_dh));                       // over the 64 hidden units of point j
      am_sw = max_xor32(max_xor16(am_sw));
      // one sticky scale for both terms of dW1' (dh and q carry the two upstream gradients' scales)
      {
        const float fac = sticky_scale(fmaxf(am_dh, am_q), es, et_max);
        if (fac != 1.0f) {
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) { dW1[nt][0] *= fac; dW1[nt][1] *= fac; }
        }
      }
      // ---------------- V = W1'^T SW, DF = W1'^T DH ; the fp16 tiles of dh (scaled), sw (natural), q (scaled) ----------------
      float d_inv, s_inv;
      f32x4 v0 = {0, 0, 0, 0}, v1 = {0, 0, 0, 0}, df0 = {0, 0, 0, 0}, df1 = {0, 0, 0, 0};
      {
        float dsc, ssc;
        pow2_normaliser(am_dh, dsc, d_inv);
        pow2_normaliser(am_sw, ssc, s_inv);
        const uint32_t r_dh = ratio_f16x2(es, d_inv), r_sw = ratio_f16x2(127, s_inv), r_q = ratio_f16x2(es, q_inv);
        const f16x8 rr_dh = __builtin_bit_cast(f16x8, u32x4{r_dh, r_dh, r_dh, r_dh});
        const f16x8 rr_sw = __builtin_bit_cast(f16x8, u32x4{r_sw, r_sw, r_sw, r_sw});
        const f16x8 rr_q = __builtin_bit_cast(f16x8, u32x4{r_q, r_q, r_q, r_q});
        {
          const u64x2 h2 = __builtin_bit_cast(u64x2, qh * rr_q), l2 = __builtin_bit_cast(u64x2, ql * rr_q);
          char* t16 = wb + j * 96 + 8 * g;
          *reinterpret_cast<u64*>(t16 + kRgQ16Hi) = h2[0]; *reinterpret_cast<u64*>(t16 + kRgQ16Hi + 32) = h2[1];
          *reinterpret_cast<u64*>(t16 + kRgQ16Lo) = l2[0]; *reinterpret_cast<u64*>(t16 + kRgQ16Lo + 32) = l2[1];
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const float xs[8] = {swv[2 * kk][0] * ssc, swv[2 * kk][1] * ssc, swv[2 * kk][2] * ssc, swv[2 * kk][3] * ssc,
                               swv[2 * kk + 1][0] * ssc, swv[2 * kk + 1][1] * ssc, swv[2 * kk + 1][2] * ssc, swv[2 * kk + 1][3] * ssc};
          const float xd[8] = {dhv[2 * kk][0] * dsc, dhv[2 * kk][1] * dsc, dhv[2 * kk][2] * dsc, dhv[2 * kk][3] * dsc,
                               dhv[2 * kk + 1][0] * dsc, dhv[2 * kk + 1][1] * dsc, dhv[2 * kk + 1][2] * dsc, dhv[2 * kk + 1][3] * dsc};
          f16x8 sh, sl, dh_h, dh_l;
          split_f16x8(xs, sh, sl);
          split_f16x8(xd, dh_h, dh_l);
          {
            // hidden units {32 kk + 4 g + r, 32 kk + 16 + 4 g + r} of point j
            char* t16 = wb + j * 144 + 2 * (32 * kk + 4 * g);
            const u64x2 a2 = __builtin_bit_cast(u64x2, dh_h * rr_dh), b2 = __builtin_bit_cast(u64x2, dh_l * rr_dh);
            const u64x2 c2 = __builtin_bit_cast(u64x2, sh * rr_sw), d2 = __builtin_bit_cast(u64x2, sl * rr_sw);
            *reinterpret_cast<u64*>(t16 + kRgDH16Hi) = a2[0]; *reinterpret_cast<u64*>(t16 + kRgDH16Hi + 32) = a2[1];
            *reinterpret_cast<u64*>(t16 + kRgDH16Lo) = b2[0]; *reinterpret_cast<u64*>(t16 + kRgDH16Lo + 32) = b2[1];
            *reinterpret_cast<u64*>(t16 + kRgSW16Hi) = c2[0]; *reinterpret_cast<u64*>(t16 + kRgSW16Hi + 32) = c2[1];
            *reinterpret_cast<u64*>(t16 + kRgSW16Lo) = d2[0]; *reinterpret_cast<u64*>(t16 + kRgSW16Lo + 32) = d2[1];
          }
          const f16x8 ah = __builtin_bit_cast(f16x8, w1t[((0 * 2 + kk) * 2 + 0) * 64 + lane]);
          const f16x8 al = __builtin_bit_cast(f16x8, w1t[((0 * 2 + kk) * 2 + 1) * 64 + lane]);
          const f16x8 bh = __builtin_bit_cast(f16x8, w1t[((1 * 2 + kk) * 2 + 0) * 64 + lane]);
          const f16x8 bl = __builtin_bit_cast(f16x8, w1t[((1 * 2 + kk) * 2 + 1) * 64 + lane]);
          v0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, sh, v0, 0, 0, 0);
          v1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, sh, v1, 0, 0, 0);
          df0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, dh_h, df0, 0, 0, 0);
          df1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, dh_h, df1, 0, 0, 0);
          v0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, sl, v0, 0, 0, 0);
          v1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, sl, v1, 0, 0, 0);
          df0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, dh_l, df0, 0, 0, 0);
          df1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, dh_l, df1, 0, 0, 0);
          v0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, sh, v0, 0, 0, 0);
          v1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl, sh, v1, 0, 0, 0);
          df0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, dh_h, df0, 0, 0, 0);
          df1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl, dh_h, df1, 0, 0, 0);
        }
      }
      // ---------------- dW1'[hid][ch] += sum_pt dh[hid][pt] f[ch][pt] + sw[hid][pt] q[ch][pt]  (K = the 16 points, hi | lo) ----------------
      wave_lds_fence();
      {
        const int rowb = 8 * (g & 1) + (j >> 2), colb = 8 * (j & 3), a_lo = g >> 1;
        const char* pb = wb + rowb * 96 + colb;
        f16x8 bfh[2], bfl[2], bqh[2], bql[2];
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2) {
          bfh[n2] = lds_read_tr16x2(pb + kRgF16Hi + 32 * n2, 4 * 96);
          bfl[n2] = lds_read_tr16x2(pb + kRgF16Lo + 32 * n2, 4 * 96);
          bqh[n2] = lds_read_tr16x2(pb + kRgQ16Hi + 32 * n2, 4 * 96);
          bql[n2] = lds_read_tr16x2(pb + kRgQ16Lo + 32 * n2, 4 * 96);
        }
        const char* pa = wb + rowb * 144 + colb;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const f16x8 a_dh = lds_read_tr16x2(pa + (a_lo ? kRgDH16Lo : kRgDH16Hi) + 32 * nt, 4 * 144);
          const f16x8 a_sw = lds_read_tr16x2(pa + (a_lo ? kRgSW16Lo : kRgSW16Hi) + 32 * nt, 4 * 144);
#pragma unroll
          for (int n2 = 0; n2 < 2; ++n2) {
            dW1[nt][n2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_dh, bfh[n2], dW1[nt][n2], 0, 0, 0);
            dW1[nt][n2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_dh, bfl[n2], dW1[nt][n2], 0, 0, 0);
            dW1[nt][n2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_sw, bqh[n2], dW1[nt][n2], 0, 0, 0);
            dW1[nt][n2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_sw, bql[n2], dW1[nt][n2], 0, 0, 0);
          }
        }
      }
      // ---------------- plane gradients: bilinear weights carry df, their derivatives carry dJ = v u^T ----------------
      // The per-point vectors go through LDS into channel-per-lane form so that one atomic instruction covers the two
      // x-adjacent corner texels of ONE point (64 consecutive floats = 2 full lines; the atomic units retire per line).
      wave_lds_fence();
      {
        float* dfr = reinterpret_cast<float*>(wb + kRgDFRows);
        float* vr = reinterpret_cast<float*>(wb + kRgVRows);
        *reinterpret_cast<f32x4*>(dfr + j * 36 + 4 * g) = df0 * d_inv;
        *reinterpret_cast<f32x4*>(dfr + j * 36 + 16 + 4 * g) = df1 * d_inv;
        *reinterpret_cast<f32x4*>(vr + j * 36 + 4 * g) = v0 * s_inv;
        *reinterpret_cast<f32x4*>(vr + j * 36 + 16 + 4 * g) = v1 * s_inv;
        wave_lds_fence();
        const int lc = lane & 31, lh = lane >> 5;
        if constexpr (ORDERED) {
          // two points per instruction, lane = channel: 2 x 128 B per point and row set
#pragma unroll 1
          for (int pt = lh; pt < 16; pt += 2) {
            const int src = 16 * t + pt;
            if (!((live >> src) & 1ull)) continue;
            const size_t row = ((size_t)scene * k.P + (size_t)(chunk * 64 + src)) * kC + lc;
            k.ord_df[row] = dfr[pt * 36 + lc];
            k.ord_v[row] = vr[pt * 36 + lc];
          }
        } else {
#pragma unroll 1
        for (int pt = 0; pt < 16; ++pt) {
          const int src = 16 * t + pt;
          if (!((live >> src) & 1ull)) continue;
          const float gv = dfr[pt * 36 + lc], vv = vr[pt * 36 + lc];
          const uint32_t pxi = (uint32_t)__builtin_amdgcn_readlane(xi, src);
          const int pi[3] = {(int)(pxi & 1023u), (int)((pxi >> 10) & 1023u), (int)((pxi >> 20) & 1023u)};
          float pf[3], pu[3];
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            pf[a] = bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(fr[a]), src));
            pu[a] = bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(u[a]), src));
          }
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
            const int aa = (pl == 2) ? 1 : 0, ab = (pl == 0) ? 1 : 2;
            const float fa = pf[aa], fb = pf[ab], ua = pu[aa], ub = pu[ab];
            float* base = gtex_scene + (size_t)pl * plane_f + ((size_t)pi[ab] * k.res + pi[aa] + lh) * pix_f + lc;
            // d f / d t = bilinear weight;  d J_a / d t = -(1-fb), +(1-fb), -fb, +fb;  d J_b / d t = -(1-fa), -fa, +(1-fa), +fa
            const float wx = lh ? fa : 1.0f - fa, sx = lh ? 1.0f : -1.0f;          // this half's x corner
            const float w_y0 = wx * (1.0f - fb), w_y1 = wx * fb;
            const float j_y0 = sx * (1.0f - fb) * ua - wx * ub, j_y1 = sx * fb * ua + wx * ub;
            unsafeAtomicAdd(base, third * (w_y0 * gv + j_y0 * vv));
            unsafeAtomicAdd(base + row_f, third * (w_y1 * gv + j_y1 * vv));
          }
        }
        }
      }
      wave_lds_fence();
    }
  }
  // ---------------- flush ----------------
  const float un = (es == 0) ? 1.0f : bits2f((uint32_t)(254 - es) << 23);
  if constexpr (ORDERED) {
    // plain stores into this wave's slot, every element of it (a wave without a chunk writes zeros): nothing to pre-zero
    float* slot = k.ord_slots + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * kRgSlotFloats;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        slot[kRgSlotW1 + (16 * nt + 4 * g + r) * 32 + j] = dW1[nt][0][r] * (gain1 * un);
        slot[kRgSlotW1 + (16 * nt + 4 * g + r) * 32 + 16 + j] = dW1[nt][1][r] * (gain1 * un);
        const float b = row_allreduce_sum(db1a[nt][r]), w = row_allreduce_sum(dw2a[nt][r]);
        if (j == 0) {
          slot[kRgSlotB1 + 16 * nt + 4 * g + r] = b;
          slot[kRgSlotW2 + 16 * nt + 4 * g + r] = w * gain2;
        }
      }
    db2 = wave_sum(db2);
    if (lane < 16) slot[kRgSlotB2 + lane] = lane == 0 ? db2 : 0.0f;
  } else {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        atomicAdd(&k.g_w1[(16 * nt + 4 * g + r) * 32 + j], dW1[nt][0][r] * (gain1 * un));
        atomicAdd(&k.g_w1[(16 * nt + 4 * g + r) * 32 + 16 + j], dW1[nt][1][r] * (gain1 * un));
        const float b = row_allreduce_sum(db1a[nt][r]), w = row_allreduce_sum(dw2a[nt][r]);     // over the 16 point columns
        if (j == 0) {
          atomicAdd(&k.g_b1[16 * nt + 4 * g + r], b);
          atomicAdd(&k.g_w2[16 * nt + 4 * g + r], w * gain2);
        }
      }
    db2 = wave_sum(db2);
    if (lane == 0) atomicAdd(&k.g_b2[0], db2);
  }
}

// ------------------------------------------------------------------------------------------------
// The ordered backward's other kernels.  Keys: one (cell << 32 | point) per point and plane, the cell from reg_coord - the
// backward kernel's own arithmetic, so key and kernel agree on the cell of a point that sits on a texel node.  The sort is
// the field backward's (ord_sort_by_cell).  Gather: one half-wave per texel and plane sums what the atomic loop above
// would have added to that texel, in a fixed order, and adds it to g_texels: one writer per texel.
// ------------------------------------------------------------------------------------------------
// grid (ceil(P / 256), scenes): thread = point
__global__ __launch_bounds__(256) void sdf_ord_keys_kernel(SdfGradParams k, uint64_t* keys) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= k.P) return;
  const int scene = blockIdx.y;
  const float* pt = k.points + ((size_t)scene * k.P + p) * 3;
  int i0[3];
  float fr;
#pragma unroll
  for (int a = 0; a < 3; ++a) reg_coord(pt[a], k.scene_range, k.res, i0[a], fr);
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    const int ia = i0[(pl == 2) ? 1 : 0], ib = i0[(pl == 0) ? 1 : 2];
    keys[(size_t)(scene * 3 + pl) * k.P + p] = ((uint64_t)(uint32_t)(ib * k.res + ia) << 32) | (uint64_t)p;
  }
}

// grid (ceil(scenes * 3 * res^2 / 8)), 256 threads: one half-wave per texel and plane, lane = channel.  The up to four cells
// that touch the texel in ascending cell order (lanes 0..7 find the cells' runs: one binary search each, side by side), a
// run in ascending point order in blocks of 32 entries: lane e works out entry e's corner weight w and Jacobian coefficient
// j with the atomic loop's expressions, every lane then adds third * (w * df[c] + j * v[c]) entry by entry; the blocks'
// sums are added in index order.
__global__ __launch_bounds__(256) void sdf_ord_gather_kernel(SdfGradParams k) {
  const int l32 = threadIdx.x & 31;
  const int64_t h = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int rr = k.res * k.res;
  if (h >= (int64_t)k.n_scenes * 3 * rr) return;
  const int seg = (int)(h / rr), tex = (int)(h - (int64_t)seg * rr);
  const int scene = seg / 3, pl = seg - scene * 3;
  const int b = tex / k.res, a = tex - b * k.res;
  const int aa = (pl == 2) ? 1 : 0, ab = (pl == 0) ? 1 : 2;
  const uint64_t* keys = k.ord_keys + (size_t)seg * k.P;
  const size_t first = (size_t)scene * k.P;
  const float scale = (float)(k.res - 1) / (2.0f * k.scene_range);
  const float third = 1.0f / 3.0f;
  // lane 2c: where cell c's run begins, lane 2c + 1: where it ends (a cell outside the plane: an empty run)
  int bound = 0;
  if (l32 < 8) {
    const int c = l32 >> 1, ia = a - 1 + (c & 1), ib = b - 1 + (c >> 1);
    if (ia >= 0 && ib >= 0 && ia <= k.res - 2 && ib <= k.res - 2) {
      const uint64_t v = (uint64_t)((uint32_t)(ib * k.res + ia) + (uint32_t)(l32 & 1)) << 32;
      bound = (int)ord_lower_bound(keys, k.P, v);       // P <= 2^25
    }
  }
  float total = 0.0f;
  bool any = false;
#pragma unroll 1
  for (int c = 0; c < 4; ++c) {                       // cells (a-1,b-1), (a,b-1), (a-1,b), (a,b): ascending cell index
    const int lo = __shfl(bound, 2 * c, 32), hi = __shfl(bound, 2 * c + 1, 32);
    const bool right = !(c & 1), upper = !(c >> 1);   // which corner of the cell this texel is
#pragma unroll 1
    for (int base = lo; base < hi; base += 32) {
      const int i = base + l32;
      uint32_t pt = 0u;
      float w = 0.0f, jc = 0.0f;
      bool live = false;
      if (i < hi) {
        pt = (uint32_t)keys[i];
        live = (int64_t)pt < k.P && k.ord_flag[first + pt] != 0;
        if (live) {
          const float* x = k.points + (first + pt) * 3;
          int i0;
          float fa, fb, ua = 0.0f, ub = 0.0f;
          reg_coord(x[aa], k.scene_range, k.res, i0, fa);
          reg_coord(x[ab], k.scene_range, k.res, i0, fb);
          if (k.gg) { ua = k.gg[(first + pt) * 3 + aa] * scale; ub = k.gg[(first + pt) * 3 + ab] * scale; }
          const float wx = right ? fa : 1.0f - fa, sx = right ? 1.0f : -1.0f;
          if (upper) { w = wx * fb; jc = sx * fb * ua + wx * ub; }
          else { w = wx * (1.0f - fb); jc = sx * (1.0f - fb) * ua - wx * ub; }
        }
      }
      const int n = min(32, hi - base);
      float part = 0.0f;
#pragma unroll 4
      for (int e = 0; e < n; ++e) {
        if (!__shfl((int)live, e, 32)) continue;
        const float we = __shfl(w, e, 32), je = __shfl(jc, e, 32);
        const size_t row = (first + (uint32_t)__shfl((int)pt, e, 32)) * kC + l32;
        part += third * (we * k.ord_df[row] + je * k.ord_v[row]);
        any = true;
      }
      total += part;
    }
  }
  if (!any) return;
  float* dst = k.g_texels + (size_t)scene * 3 * rr * kC + (size_t)pl * k.plane_f() + (size_t)tex * k.pix_f() + l32;
  *dst += total;
}

// grid (kRgSlotFloats / 16), 256 threads = 16 slot offsets x 16 parts: ordered_slot_sum over all slots, part 0 adds the sum
// to the caller's buffer
__global__ __launch_bounds__(256) void sdf_slot_finish_kernel(SdfGradParams k, int n_slots) {
  __shared__ float partial[16][16];
  const int e = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int o = blockIdx.x * 16 + e;
  const float t = ordered_slot_sum(k.ord_slots, kRgSlotFloats, o, 0, n_slots, partial);
  if (part != 0) return;
  if (o < kRgSlotB1) k.g_w1[o] += t;
  else if (o < kRgSlotW2) k.g_b1[o - kRgSlotB1] += t;
  else if (o < kRgSlotB2) k.g_w2[o - kRgSlotW2] += t;
  else if (o == kRgSlotB2) k.g_b2[0] += t;
}

static int sdf_gradient_common(const nfi_sdf_gradient_args* a, SdfGradParams& k) {
  REQUIRE(a && a->points && a->texels && a->w1 && a->b1 && a->w2 && a->b2, "sdf_gradient: null pointer");
  REQUIRE(a->n_scenes > 0 && a->points_per_scene > 0, "sdf_gradient: bad shape");
  REQUIRE(a->plane_res >= 2 && a->plane_res <= 1024, "sdf_gradient: plane_res must be in [2,1024]");
  memset(&k, 0, sizeof(k));
  k.points = a->points; k.P = a->points_per_scene; k.n_scenes = a->n_scenes;
  k.texels = a->texels; k.res = a->plane_res; k.scene_range = a->scene_range;
  k.w1 = a->w1; k.b1 = a->b1; k.w2 = a->w2; k.b2 = a->b2;
  REQUIRE(a->texel_layout == NFI_TEXELS_PLANAR || a->texel_layout == NFI_TEXELS_INTERLEAVED, "sdf_gradient: bad texel layout");
  k.layout = a->texel_layout;
  return NFI_OK;
}

extern "C" int nfi_sdf_gradient_fwd(const nfi_sdf_gradient_args* a, nfi_stream_t stream) {
  SdfGradParams k;
  int rc = sdf_gradient_common(a, k);
  if (rc) return rc;
  REQUIRE(a->sdf && a->gradient, "sdf_gradient_fwd: output pointer missing");
  k.d = a->sdf; k.g = a->gradient;
  int64_t blocks = (a->points_per_scene + 255) / 256;        // one 64-point chunk per wave and turn
  const int64_t cap = std::max<int64_t>(16, 1024 / a->n_scenes);
  if (blocks > cap) blocks = cap;
  dim3 grid((unsigned)blocks, (unsigned)a->n_scenes);
  hipLaunchKernelGGL(sdf_gradient_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, k);
  return check_launch("sdf_gradient_fwd");
}

// blocks per scene of the backward's grid: one 64-point chunk per wave and turn; a resident set of blocks (1 per CU: 256+
// registers): every wave flushes 2 177 sums at its end.  A function of (P, n_scenes) alone, which is what fixes the ordered
// variant's slot order.
static int64_t sdf_gradient_bwd_blocks(const nfi_sdf_gradient_args* a) {
  const int64_t blocks = (a->points_per_scene + 255) / 256;
  return std::min(blocks, std::max<int64_t>(16, 256 * NFI_REG_OCC / a->n_scenes));
}

// the backward's arguments and grid, for both entries
static int sdf_gradient_bwd_common(const nfi_sdf_gradient_args* a, SdfGradParams& k, dim3& grid, const char* no_upstream) {
  int rc = sdf_gradient_common(a, k);
  if (rc) return rc;
  REQUIRE(a->g_sdf || a->g_gradient, no_upstream);
  REQUIRE(a->g_texels && a->g_w1 && a->g_b1 && a->g_w2 && a->g_b2, "sdf_gradient_bwd: output pointer missing");
  k.gd = a->g_sdf; k.gg = a->g_gradient;
  k.g_texels = a->g_texels; k.g_w1 = a->g_w1; k.g_b1 = a->g_b1; k.g_w2 = a->g_w2; k.g_b2 = a->g_b2;
  grid = dim3((unsigned)sdf_gradient_bwd_blocks(a), (unsigned)a->n_scenes);
  return NFI_OK;
}

template <bool ORDERED>
static int launch_sdf_gradient_bwd(dim3 grid, hipStream_t s, const SdfGradParams& k) {
  const size_t shmem = (size_t)kRgLdsFloats * sizeof(float);
  const int rc = ensure_dynamic_lds<&sdf_gradient_bwd_kernel<ORDERED>>(shmem, "sdf_gradient_bwd");
  if (rc) return rc;
  hipLaunchKernelGGL(sdf_gradient_bwd_kernel<ORDERED>, grid, dim3(256), shmem, s, k);
  return NFI_OK;
}

extern "C" int nfi_sdf_gradient_bwd(const nfi_sdf_gradient_args* a, nfi_stream_t stream) {
  SdfGradParams k;
  dim3 grid;
  int rc = sdf_gradient_bwd_common(a, k, grid, "sdf_gradient_bwd: no upstream gradient");
  if (rc) return rc;
  rc = launch_sdf_gradient_bwd<false>(grid, (hipStream_t)stream, k);
  if (rc) return rc;
  return check_launch("sdf_gradient_bwd");
}

// The workspace of one nfi_sdf_gradient_bwd_ordered call: byte offsets of its regions and the total
struct SdfOrdCarve { size_t df, v, flag, keys[2], hist, slots, total; int n_slots; };

static SdfOrdCarve sdf_ord_carve(const nfi_sdf_gradient_args* a) {
  SdfOrdCarve c;
  memset(&c, 0, sizeof(c));
  const size_t n_pts = (size_t)a->n_scenes * (size_t)a->points_per_scene;
  c.n_slots = (int)(sdf_gradient_bwd_blocks(a) * a->n_scenes * 4);
  size_t at = 0;
  c.df = at; at += align256(n_pts * kC * sizeof(float));
  c.v = at; at += align256(n_pts * kC * sizeof(float));
  c.flag = at; at += align256(n_pts);
  c.keys[0] = at; at += align256(3 * n_pts * sizeof(uint64_t));
  c.keys[1] = at; at += align256(3 * n_pts * sizeof(uint64_t));
  c.hist = at; at += align256(ord_sort_plan(a->points_per_scene, a->n_scenes * 3, a->plane_res).hist_bytes);
  c.slots = at; at += align256((size_t)c.n_slots * kRgSlotFloats * sizeof(float));
  c.total = at;
  return c;
}

static bool sdf_ord_shape_ok(const nfi_sdf_gradient_args* a) {
  return a && a->n_scenes > 0 && a->points_per_scene > 0 && a->points_per_scene <= (int64_t)1 << 25 && a->plane_res >= 2 &&
         a->plane_res <= 1024;
}

extern "C" size_t nfi_sdf_gradient_bwd_ordered_workspace_bytes(const nfi_sdf_gradient_args* a) {
  return sdf_ord_shape_ok(a) ? sdf_ord_carve(a).total : 0;
}

extern "C" int nfi_sdf_gradient_bwd_ordered(const nfi_sdf_gradient_args* a, void* workspace, size_t workspace_bytes,
                                            nfi_stream_t stream) {
  SdfGradParams k;
  dim3 grid;
  int rc = sdf_gradient_bwd_common(a, k, grid, "sdf_gradient_bwd_ordered: no upstream gradient");
  if (rc) return rc;
  REQUIRE(a->points_per_scene <= (int64_t)1 << 25, "sdf_gradient_bwd_ordered: at most 2^25 points per scene (split the call)");
  REQUIRE(workspace, "sdf_gradient_bwd_ordered: workspace missing");
  const SdfOrdCarve ws = sdf_ord_carve(a);
  REQUIRE(workspace_bytes >= ws.total, "sdf_gradient_bwd_ordered: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* const w = reinterpret_cast<char*>(workspace);
  // nothing here is read before this call has written it (rows and flags of every point, every slot, keys, counts)
  k.ord_df = reinterpret_cast<float*>(w + ws.df); k.ord_v = reinterpret_cast<float*>(w + ws.v);
  k.ord_flag = reinterpret_cast<uint8_t*>(w + ws.flag);
  k.ord_slots = reinterpret_cast<float*>(w + ws.slots);
  rc = launch_sdf_gradient_bwd<true>(grid, s, k);
  if (rc) return rc;
  hipLaunchKernelGGL(sdf_slot_finish_kernel, dim3(kRgSlotFloats / 16), dim3(256), 0, s, k, ws.n_slots);
  uint64_t* keys = reinterpret_cast<uint64_t*>(w + ws.keys[0]);
  hipLaunchKernelGGL(sdf_ord_keys_kernel, dim3((unsigned)((a->points_per_scene + 255) / 256), (unsigned)a->n_scenes), dim3(256), 0, s,
                     k, keys);
  k.ord_keys = ord_sort_by_cell(keys, reinterpret_cast<uint64_t*>(w + ws.keys[1]), reinterpret_cast<uint32_t*>(w + ws.hist),
                                a->points_per_scene, a->n_scenes * 3, a->plane_res, s);
  const int64_t half_waves = (int64_t)a->n_scenes * 3 * a->plane_res * a->plane_res;
  hipLaunchKernelGGL(sdf_ord_gather_kernel, dim3((unsigned)((half_waves + 7) / 8)), dim3(256), 0, s, k);
  return check_launch("sdf_gradient_bwd_ordered");
}
