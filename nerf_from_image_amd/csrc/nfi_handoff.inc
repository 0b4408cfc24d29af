// nfi_handoff.inc — the plane producer's last step written straight into texel layout (included by nfi_modules.hip;
// SURVEY.md 8(f)3).
//
// Reference: the tail of the last StyleGAN2 synthesis block (models/stylegan.py:383-435, SynthesisBlock.forward):
//      img = upsample2d(img_prev)                    conv_transpose2d with the 4x4 bilinear filter * 4, stride 2, pad 1
//      y   = torgb(x, w)                             1x1 modulated conv WITHOUT demodulation + bias (OutputLayer, 351-372)
//      img = img + y                                 -> [B,96,R,R] NCHW, viewed as planes [B,3,32,R,R] (generator.py:475-477)
// followed, in round 1, by nfi_planes_to_texels (NCHW -> channel-last: 25 MB per scene read + written again).  Here the
// three steps are one kernel whose result IS the texel image, in the interleaved layout [B,R,R,3,32] = a channels-last
// [B,96,R,R] tensor, so the reference's own code keeps working on it (same shape, other strides) and the field kernels
// gather from it in place.
//
//   out[b,p,o] = sum_k W[o,k] * s[b,k] * x[b,k,p] + bias[o] + up(prev)[b,o,p]          p = pixel, o < 96, k < Cin
//
// This IS a dense contraction (96 x Cin per pixel: 1.6 GFLOP per 256x256 scene at Cin = 128), so it runs on MFMA:
// v_mfma_f32_16x16x4_f32 (exact fp32 - the reference runs an fp32 convolution here), D rows = output channels, columns
// = pixels; a wave owns 64 consecutive pixels as four column tiles n' = {p0 + 4j + n'} - strided, so that ONE
// 16-byte load per lane along the pixel axis of the NCHW activations feeds all four tiles (rows of 256 contiguous
// bytes per channel), and one 16-byte store per lane writes 4 consecutive channels of a texel.  The weights sit in
// LDS as lane-ordered A fragments; the per-sample styles scale the B operand (one multiply per loaded value).
// Both streams (x in, texels out) are touched exactly once: the kernel is HBM-bound by construction
// (B*R*R*(4 Cin + 384 + 96) bytes), with the MFMA time (768 instructions per 64 pixels) of the same order.
//
// Backward (training / inversion differentiate through the producer):
//   torgb_bwd_data_kernel    t = W^T g (MFMA, same tiling);  g_x = s * t (NCHW, 16-byte stores);  g_s = sum_p x * t
//   torgb_bwd_weight_kernel  g_W = sum_{b,p} g (s x)^T (MFMA with the pixels along K), g_bias = sum g
//   upsample_bwd_kernel      g_prev = the adjoint of the stride-2 bilinear up-filter (a 4x4 gather per coarse pixel)
// The two MFMA kernels sum g_s, g_W and g_bias with float atomics (LDS and global).  nfi_torgb_texels_bwd_ordered runs
// ordered COPIES of the two (why copies: at the ordered data kernel): every partial sum goes to a workspace slot of its own -
// one per (scene, block, wave) for g_s, one per block for g_W / g_bias, the block's four waves combined in wave order - and
// two finish kernels add the slots in index order.  g_x and g_prev have one writer per element either way.

struct TorgbParams {
  const float* x; const float* styles; const float* weight; const float* bias; const float* prev;
  float* out;
  int B, Cin, R;
  const float* g_out; float* g_x; float* g_styles; float* g_weight; float* g_bias; float* g_prev;
};

constexpr int kTorgbOut = 96;          // 3 planes x 32 channels
constexpr int kTorgbMaxCin = 256;      // largest in_channels accepted (sizes the dynamic-LDS limit once)
constexpr int kTorgbTilesPerWave = 4;  // 64-pixel tiles a wave walks per block visit
constexpr int kTorgbBlockPixels = 64 * 4 * kTorgbTilesPerWave;   // of a block of the forward and the data kernels

// 1-D taps of the up-filter for output index Y: rows (m_lo weight .., m_hi ..) of the coarse image, zero outside
__device__ __forceinline__ void up_taps(int Y, int half, int& m_a, int& m_b, float& w_a, float& w_b) {
  const int m = Y >> 1;
  m_a = m; w_a = 0.75f;
  m_b = (Y & 1) ? m + 1 : m - 1; w_b = 0.25f;
  if (m_b < 0 || m_b >= half) { m_b = m; w_b = 0.0f; }
}

__global__ __launch_bounds__(256, 2) void torgb_texels_fwd_kernel(TorgbParams k) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const int Cin = k.Cin, S4 = Cin >> 4;                  // groups of 16 input channels
  float* ldsA = dyn;                                     // [6][S4][64 lanes][4 u]   A fragments of W
  float* ldsS = dyn + kTorgbOut * Cin;                   // [S4][4 kk][4 u]          styles of this sample, fragment order
  float* ldsB = ldsS + Cin;                              // [96] bias
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < kTorgbOut * Cin; i += blockDim.x) {
    const int u = i & 3, lane = (i >> 2) & 63, rest = i >> 8;
    const int s4 = rest % S4, t = rest / S4;
    const int o = 16 * t + (lane & 15), kk = 16 * s4 + 4 * u + (lane >> 4);
    ldsA[i] = k.weight[o * Cin + kk];
  }
  for (int i = threadIdx.x; i < Cin; i += blockDim.x) {
    const int u = i & 3, kk = (i >> 2) & 3, s4 = i >> 4;
    ldsS[i] = k.styles[(size_t)b * Cin + 16 * s4 + 4 * u + kk];
  }
  for (int i = threadIdx.x; i < kTorgbOut; i += blockDim.x) ldsB[i] = k.bias[i];
  __syncthreads();
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int R = k.R, P = R * R, half = R >> 1;
  const f32x4* A4 = reinterpret_cast<const f32x4*>(ldsA);
  const f32x4* S4v = reinterpret_cast<const f32x4*>(ldsS);
  const float* xb = k.x + (size_t)b * Cin * P;
  for (int w = 0; w < kTorgbTilesPerWave; ++w) {
    const int pix0 = ((blockIdx.x * 4 + wave) * kTorgbTilesPerWave + w) * 64;
    if (pix0 >= P) break;
    f32x4 acc[6][4];
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[t][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // B operand of k-step (s4, u): lane (kk = g, j) holds x[16 s4 + 4u + kk][pix0 + 4j + n'], n' = the float4's lanes
    auto load_x = [&](int s4, f32x4 (&xv)[4]) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        xv[u] = *reinterpret_cast<const f32x4*>(xb + (size_t)(16 * s4 + 4 * u + g) * P + pix0 + 4 * j);
    };
    f32x4 cur[4], nxt[4];
    load_x(0, cur);
    for (int s4 = 0; s4 < S4; ++s4) {
      if (s4 + 1 < S4) load_x(s4 + 1, nxt);
      const f32x4 st = S4v[s4 * 4 + g];
#pragma unroll
      for (int u = 0; u < 4; ++u) cur[u] = cur[u] * st[u];
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        const f32x4 a = A4[(t * S4 + s4) * 64 + lane];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], cur[u][n], acc[t][n], 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
    }
    // ---- epilogue: + bias + upsampled previous image, 16-byte stores of 4 consecutive channels ----
    const int p4 = pix0 + 4 * j;                     // this lane's 4 pixels share a row (R % 4 == 0)
    const int Y = p4 / R, X0 = p4 - Y * R, c = X0 >> 1;
    int ma = 0, mb = 0;
    float wa = 0.0f, wb = 0.0f;
    up_taps(Y, half, ma, mb, wa, wb);
    // columns c-1 .. c+2 of the coarse rows; pixel n' uses (c, c-1), (c, c+1), (c+1, c), (c+1, c+2)
    const bool lo_ok = c - 1 >= 0, hi_ok = c + 2 < half;
    float* ob = k.out + ((size_t)b * P + p4) * kTorgbOut;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      const f32x4 bias = *reinterpret_cast<const f32x4*>(ldsB + 16 * t + 4 * g);
      f32x4 res[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) res[n] = f32x4{acc[t][n][0], acc[t][n][1], acc[t][n][2], acc[t][n][3]} + bias;
      if (k.prev) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float* pc = k.prev + ((size_t)b * kTorgbOut + 16 * t + 4 * g + r) * half * half;
          const float* ra = pc + (size_t)ma * half + c;
          const float* rb = pc + (size_t)mb * half + c;
          const float a_m1 = lo_ok ? ra[-1] : 0.0f, a_0 = ra[0], a_1 = ra[1], a_2 = hi_ok ? ra[2] : 0.0f;
          const float b_m1 = lo_ok ? rb[-1] : 0.0f, b_0 = rb[0], b_1 = rb[1], b_2 = hi_ok ? rb[2] : 0.0f;
          const float v_m1 = wa * a_m1 + wb * b_m1, v_0 = wa * a_0 + wb * b_0, v_1 = wa * a_1 + wb * b_1,
                      v_2 = wa * a_2 + wb * b_2;
          res[0][r] += 0.75f * v_0 + 0.25f * v_m1;
          res[1][r] += 0.75f * v_0 + 0.25f * v_1;
          res[2][r] += 0.75f * v_1 + 0.25f * v_0;
          res[3][r] += 0.75f * v_1 + 0.25f * v_2;
        }
      }
#pragma unroll
      for (int n = 0; n < 4; ++n) *reinterpret_cast<f32x4*>(ob + (size_t)n * kTorgbOut + 16 * t + 4 * g) = res[n];
    }
  }
}

// t = W^T g on MFMA; g_x = s * t; g_s += sum_p x * t
__global__ __launch_bounds__(256, 2) void torgb_bwd_data_kernel(TorgbParams k) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const int Cin = k.Cin, TK = Cin >> 4;                  // 16-row tiles of input channels
  float* ldsA = dyn;                                     // [TK][6 s6][64 lanes][4 u]: W[16 s6 + 4 kk + u][16 tk + i]
  float* ldsS = dyn + kTorgbOut * Cin;                   // [Cin] styles of this sample
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < kTorgbOut * Cin; i += blockDim.x) {
    const int u = i & 3, lane = (i >> 2) & 63, rest = i >> 8;
    const int s6 = rest % 6, tk = rest / 6;
    ldsA[i] = k.weight[(16 * s6 + 4 * (lane >> 4) + u) * Cin + 16 * tk + (lane & 15)];
  }
  for (int i = threadIdx.x; i < Cin; i += blockDim.x) ldsS[i] = k.styles[(size_t)b * Cin + i];
  __syncthreads();
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int R = k.R, P = R * R;
  const f32x4* A4 = reinterpret_cast<const f32x4*>(ldsA);
  const float* xb = k.x + (size_t)b * Cin * P;
  float* gxb = k.g_x + (size_t)b * Cin * P;
  float gs[8][4];                                        // per-lane partial of g_s[16 tk + 4g + r] (TK <= 8 per pass)
  for (int tk0 = 0; tk0 < TK; tk0 += 8) {
    const int ntk = min(8, TK - tk0);
#pragma unroll
    for (int a = 0; a < 8; ++a) gs[a][0] = gs[a][1] = gs[a][2] = gs[a][3] = 0.0f;
    for (int w = 0; w < kTorgbTilesPerWave; ++w) {
      const int pix0 = ((blockIdx.x * 4 + wave) * kTorgbTilesPerWave + w) * 64;
      if (pix0 >= P) break;
      f32x4 acc[8][4];
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[a][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      const float* gb = k.g_out + ((size_t)b * P + pix0 + 4 * j) * kTorgbOut + 4 * g;
#pragma unroll 1
      for (int s6 = 0; s6 < 6; ++s6) {
        // B operand: lane (kk = g, j), tile n': g[pix0 + 4j + n'][16 s6 + 4 kk + u]
        f32x4 gv[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) gv[n] = *reinterpret_cast<const f32x4*>(gb + (size_t)n * kTorgbOut + 16 * s6);
#pragma unroll
        for (int a = 0; a < 8; ++a) {
          if (a < ntk) {
            const f32x4 wv = A4[((tk0 + a) * 6 + s6) * 64 + lane];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int n = 0; n < 4; ++n)
                acc[a][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u], gv[n][u], acc[a][n], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        if (a < ntk) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int kc = 16 * (tk0 + a) + 4 * g + r;
            const size_t off = (size_t)kc * P + pix0 + 4 * j;
            const f32x4 t4 = {acc[a][0][r], acc[a][1][r], acc[a][2][r], acc[a][3][r]};
            const f32x4 x4 = *reinterpret_cast<const f32x4*>(xb + off);
            *reinterpret_cast<f32x4*>(gxb + off) = t4 * ldsS[kc];
            gs[a][r] += (x4[0] * t4[0] + x4[1] * t4[1]) + (x4[2] * t4[2] + x4[3] * t4[3]);
          }
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      if (a < ntk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = row_allreduce_sum(gs[a][r]);
          if (j == 0 && v != 0.0f) atomicAdd(&k.g_styles[(size_t)b * Cin + 16 * (tk0 + a) + 4 * g + r], v);
        }
      }
    }
  }
}

// torgb_bwd_data_kernel with g_s left to a finish kernel: the same statements (g_x is that kernel's, bit for bit), but each
// wave STORES its row-reduced sums to slots[scene][block][wave][Cin] - zeros from a wave without pixels.  Still a copy: one
// inlined body with a stateless flush functor kept every resource, and cost both default kernels 1 % (profiles/r20).
__global__ __launch_bounds__(256, 2) void torgb_bwd_data_ordered_kernel(TorgbParams k, float* slots) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const int Cin = k.Cin, TK = Cin >> 4;                  // 16-row tiles of input channels
  float* ldsA = dyn;                                     // [TK][6 s6][64 lanes][4 u]: W[16 s6 + 4 kk + u][16 tk + i]
  float* ldsS = dyn + kTorgbOut * Cin;                   // [Cin] styles of this sample
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < kTorgbOut * Cin; i += blockDim.x) {
    const int u = i & 3, lane = (i >> 2) & 63, rest = i >> 8;
    const int s6 = rest % 6, tk = rest / 6;
    ldsA[i] = k.weight[(16 * s6 + 4 * (lane >> 4) + u) * Cin + 16 * tk + (lane & 15)];
  }
  for (int i = threadIdx.x; i < Cin; i += blockDim.x) ldsS[i] = k.styles[(size_t)b * Cin + i];
  __syncthreads();
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int R = k.R, P = R * R;
  const f32x4* A4 = reinterpret_cast<const f32x4*>(ldsA);
  const float* xb = k.x + (size_t)b * Cin * P;
  float* gxb = k.g_x + (size_t)b * Cin * P;
  float gs[8][4];                                        // per-lane partial of g_s[16 tk + 4g + r] (TK <= 8 per pass)
  float* slot = slots + (((size_t)b * gridDim.x + blockIdx.x) * 4 + wave) * Cin;
  for (int tk0 = 0; tk0 < TK; tk0 += 8) {
    const int ntk = min(8, TK - tk0);
#pragma unroll
    for (int a = 0; a < 8; ++a) gs[a][0] = gs[a][1] = gs[a][2] = gs[a][3] = 0.0f;
    for (int w = 0; w < kTorgbTilesPerWave; ++w) {
      const int pix0 = ((blockIdx.x * 4 + wave) * kTorgbTilesPerWave + w) * 64;
      if (pix0 >= P) break;
      f32x4 acc[8][4];
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[a][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      const float* gb = k.g_out + ((size_t)b * P + pix0 + 4 * j) * kTorgbOut + 4 * g;
#pragma unroll 1
      for (int s6 = 0; s6 < 6; ++s6) {
        // B operand: lane (kk = g, j), tile n': g[pix0 + 4j + n'][16 s6 + 4 kk + u]
        f32x4 gv[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) gv[n] = *reinterpret_cast<const f32x4*>(gb + (size_t)n * kTorgbOut + 16 * s6);
#pragma unroll
        for (int a = 0; a < 8; ++a) {
          if (a < ntk) {
            const f32x4 wv = A4[((tk0 + a) * 6 + s6) * 64 + lane];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int n = 0; n < 4; ++n)
                acc[a][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u], gv[n][u], acc[a][n], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        if (a < ntk) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int kc = 16 * (tk0 + a) + 4 * g + r;
            const size_t off = (size_t)kc * P + pix0 + 4 * j;
            const f32x4 t4 = {acc[a][0][r], acc[a][1][r], acc[a][2][r], acc[a][3][r]};
            const f32x4 x4 = *reinterpret_cast<const f32x4*>(xb + off);
            *reinterpret_cast<f32x4*>(gxb + off) = t4 * ldsS[kc];
            gs[a][r] += (x4[0] * t4[0] + x4[1] * t4[1]) + (x4[2] * t4[2] + x4[3] * t4[3]);
          }
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      if (a < ntk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = row_allreduce_sum(gs[a][r]);
          if (j == 0) slot[16 * (tk0 + a) + 4 * g + r] = v;
        }
      }
    }
  }
}

// g_styles[b][kc] = the sum of its n_slots = blocks x 4 wave slots, in (block, wave) order
__global__ __launch_bounds__(256) void torgb_bwd_styles_finish_kernel(TorgbParams k, const float* slots, int n_slots) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k.B * k.Cin) return;
  const int b = i / k.Cin, kc = i - b * k.Cin;
  const float* p = slots + (size_t)b * n_slots * k.Cin + kc;
  float v = 0.0f;
  for (int s = 0; s < n_slots; ++s) v += p[(size_t)s * k.Cin];
  k.g_styles[i] = v;
}

// g_W[o][k] = sum_{b,p} g[b,p,o] * s[b,k] * x[b,k,p]  (pixels along the MFMA K axis), g_bias[o] = sum g.
// blockIdx.y picks a group of 4 input-channel tiles (64 channels): 96 x 64 accumulators per wave.
__global__ __launch_bounds__(256, 2) void torgb_bwd_weight_kernel(TorgbParams k, int groups_per_image) {
  __shared__ float red[kTorgbOut * 64];
  const int Cin = k.Cin, R = k.R, P = R * R;
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int tkg = blockIdx.y;                             // input channels [64 tkg, 64 tkg + 64)
  const int ntk = min(4, (Cin >> 4) - 4 * tkg);
  f32x4 acc[6][4];
  float bsum[6];
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    bsum[t] = 0.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[t][a] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const int64_t n_groups = (int64_t)k.B * groups_per_image;              // groups of 16 pixels
  for (int64_t grp = (int64_t)blockIdx.x * 4 + wave; grp < n_groups; grp += (int64_t)gridDim.x * 4) {
    const int b = (int)(grp / groups_per_image);
    const int pix0 = (int)(grp - (int64_t)b * groups_per_image) * 16;
    // B operand of k-step u: lane (kk = g, j): s * x[b][16 tk + j][pix0 + 4 kk + u]
    f32x4 xs[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a < ntk) {
        const int kc = 16 * (4 * tkg + a) + j;
        xs[a] = *reinterpret_cast<const f32x4*>(k.x + ((size_t)b * Cin + kc) * P + pix0 + 4 * g) * k.styles[(size_t)b * Cin + kc];
      } else {
        xs[a] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
    // A operand of k-step u: lane (kk = g, i = j): g[b][pix0 + 4 kk + u][16 t + i]
    const float* gp = k.g_out + ((size_t)b * P + pix0 + 4 * g) * kTorgbOut + j;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float av[6];
#pragma unroll
      for (int t = 0; t < 6; ++t) { av[t] = gp[(size_t)u * kTorgbOut + 16 * t]; bsum[t] += av[t]; }
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int a = 0; a < 4; ++a)
          acc[t][a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], xs[a][u], acc[t][a], 0, 0, 0);
    }
  }
  // block reduction through LDS, then one set of atomics per block: D lane (g, j): g_W[16 t + 4g + r][16 (4 tkg + a) + j]
  for (int i = threadIdx.x; i < kTorgbOut * 64; i += blockDim.x) red[i] = 0.0f;
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 6; ++t)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(&red[(16 * t + 4 * g + r) * 64 + 16 * a + j], acc[t][a][r]);
  __syncthreads();
  for (int i = threadIdx.x; i < kTorgbOut * 64; i += blockDim.x) {
    const int o = i >> 6, kc = 64 * tkg + (i & 63);
    if (kc < Cin && red[i] != 0.0f) atomicAdd(&k.g_weight[o * Cin + kc], red[i]);
  }
  if (tkg == 0) {
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      const float v = sum_xor32(sum_xor16(bsum[t]));       // over the four pixel groups kk
      if (g == 0 && v != 0.0f) atomicAdd(&k.g_bias[16 * t + j], v);
    }
  }
}

// torgb_bwd_weight_kernel without atomics: a copy of its grid-stride accumulation (shared, the default kernel was 1 % slower:
// profiles/r20), then the four waves add into red one after the other (wave order, a barrier between them), their bias sums
// meet in red_bias[wave][96], and the block stores part_w[tkg][block][96 x 64] / part_b[block][96] for the finish kernel.
__global__ __launch_bounds__(256, 2) void torgb_bwd_weight_ordered_kernel(TorgbParams k, int groups_per_image, float* part_w,
                                                                          float* part_b) {
  __shared__ float red[kTorgbOut * 64];                    // 24 KB + 1.5 KB: two blocks per CU, as the kernel above
  __shared__ float red_bias[4 * kTorgbOut];
  const int Cin = k.Cin, R = k.R, P = R * R;
  const int lane = lane_id(), wave = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int tkg = blockIdx.y;                             // input channels [64 tkg, 64 tkg + 64)
  const int ntk = min(4, (Cin >> 4) - 4 * tkg);
  f32x4 acc[6][4];
  float bsum[6];
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    bsum[t] = 0.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[t][a] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const int64_t n_groups = (int64_t)k.B * groups_per_image;              // groups of 16 pixels
  for (int64_t grp = (int64_t)blockIdx.x * 4 + wave; grp < n_groups; grp += (int64_t)gridDim.x * 4) {
    const int b = (int)(grp / groups_per_image);
    const int pix0 = (int)(grp - (int64_t)b * groups_per_image) * 16;
    // B operand of k-step u: lane (kk = g, j): s * x[b][16 tk + j][pix0 + 4 kk + u]
    f32x4 xs[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a < ntk) {
        const int kc = 16 * (4 * tkg + a) + j;
        xs[a] = *reinterpret_cast<const f32x4*>(k.x + ((size_t)b * Cin + kc) * P + pix0 + 4 * g) * k.styles[(size_t)b * Cin + kc];
      } else {
        xs[a] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
    // A operand of k-step u: lane (kk = g, i = j): g[b][pix0 + 4 kk + u][16 t + i]
    const float* gp = k.g_out + ((size_t)b * P + pix0 + 4 * g) * kTorgbOut + j;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float av[6];
#pragma unroll
      for (int t = 0; t < 6; ++t) { av[t] = gp[(size_t)u * kTorgbOut + 16 * t]; bsum[t] += av[t]; }
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int a = 0; a < 4; ++a)
          acc[t][a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], xs[a][u], acc[t][a], 0, 0, 0);
    }
  }
#pragma unroll 1
  for (int turn = 0; turn < 4; ++turn) {
    if (wave == turn) {
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* e = &red[(16 * t + 4 * g + r) * 64 + 16 * a + j];    // one lane of the wave per element
            *e = turn == 0 ? acc[t][a][r] : *e + acc[t][a][r];
          }
    }
    __syncthreads();
  }
  float* pw = part_w + ((size_t)tkg * gridDim.x + blockIdx.x) * (kTorgbOut * 64);
  for (int i = threadIdx.x; i < kTorgbOut * 64; i += blockDim.x) pw[i] = red[i];
  if (tkg == 0) {
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      const float v = sum_xor32(sum_xor16(bsum[t]));     // over the four pixel groups kk
      if (g == 0) red_bias[wave * kTorgbOut + 16 * t + j] = v;
    }
    __syncthreads();
    if (threadIdx.x < kTorgbOut) {
      const float* rb = red_bias + threadIdx.x;
      part_b[(size_t)blockIdx.x * kTorgbOut + threadIdx.x] = ((rb[0] + rb[kTorgbOut]) + rb[2 * kTorgbOut]) + rb[3 * kTorgbOut];
    }
  }
}

// g_weight[o][kc] / g_bias[o] = the sum of the n_blocks block partials, in block order
__global__ __launch_bounds__(256) void torgb_bwd_weight_finish_kernel(TorgbParams k, const float* part_w, const float* part_b,
                                                                      int n_blocks) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < kTorgbOut * k.Cin) {
    const int o = i / k.Cin, kc = i - o * k.Cin;
    const float* p = part_w + (size_t)(kc >> 6) * n_blocks * (kTorgbOut * 64) + o * 64 + (kc & 63);
    float v = 0.0f;
    for (int s = 0; s < n_blocks; ++s) v += p[(size_t)s * (kTorgbOut * 64)];
    k.g_weight[i] = v;
  } else if (i < kTorgbOut * k.Cin + kTorgbOut) {
    const int o = i - kTorgbOut * k.Cin;
    float v = 0.0f;
    for (int s = 0; s < n_blocks; ++s) v += part_b[(size_t)s * kTorgbOut + o];
    k.g_bias[o] = v;
  }
}

// adjoint of the stride-2 up-filter: g_prev[b,o,m,n] = sum_{dy,dx} u[dy] u[dx] g[b, 2m-1+dy, 2n-1+dx, o]
__global__ __launch_bounds__(256) void upsample_bwd_kernel(TorgbParams k) {
  const int R = k.R, half = R >> 1;
  const int64_t total = (int64_t)k.B * half * half * 24;            // 24 chunks of 4 channels per coarse pixel
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int q = (int)(idx % 24);
  const int64_t cp = idx / 24;
  const int n = (int)(cp % half), m = (int)((cp / half) % half), b = (int)(cp / ((int64_t)half * half));
  const float u4[4] = {0.25f, 0.75f, 0.75f, 0.25f};
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int dy = 0; dy < 4; ++dy) {
    const int Y = 2 * m - 1 + dy;
    if (Y < 0 || Y >= R) continue;
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) {
      const int X = 2 * n - 1 + dx;
      if (X < 0 || X >= R) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(k.g_out + (((size_t)b * R + Y) * R + X) * kTorgbOut + 4 * q);
      acc += v * (u4[dy] * u4[dx]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) k.g_prev[(((size_t)b * kTorgbOut + 4 * q + r) * half + m) * half + n] = acc[r];
}

// the shape rule of every entry (torgb_common refuses with one message per line, the workspace query answers 0)
static bool torgb_channels_ok(const nfi_torgb_args* a) {
  return a->n_scenes > 0 && a->in_channels >= 16 && a->in_channels <= kTorgbMaxCin && a->in_channels % 16 == 0;
}
static bool torgb_resolution_ok(const nfi_torgb_args* a) {
  return a->resolution >= 8 && a->resolution <= 1024 && a->resolution % 8 == 0;
}

static int torgb_common(const nfi_torgb_args* a, TorgbParams& k) {
  REQUIRE(a && a->x && a->styles && a->weight, "torgb_texels: null pointer");
  REQUIRE(torgb_channels_ok(a), "torgb_texels: in_channels must be a multiple of 16 in [16,256]");
  REQUIRE(torgb_resolution_ok(a), "torgb_texels: resolution must be a multiple of 8 in [8,1024]");
  memset(&k, 0, sizeof(k));
  k.x = a->x; k.styles = a->styles; k.weight = a->weight; k.bias = a->bias; k.prev = a->previous_image;
  k.B = a->n_scenes; k.Cin = a->in_channels; k.R = a->resolution;
  return NFI_OK;
}

extern "C" int nfi_torgb_texels_fwd(const nfi_torgb_args* a, nfi_stream_t stream) {
  TorgbParams k;
  int rc = torgb_common(a, k);
  if (rc) return rc;
  REQUIRE(a->bias && a->texels, "torgb_texels_fwd: null pointer");
  k.out = a->texels;
  const int P = k.R * k.R;
  dim3 grid((unsigned)((P + kTorgbBlockPixels - 1) / kTorgbBlockPixels), (unsigned)k.B);
  const size_t shmem = ((size_t)kTorgbOut * k.Cin + k.Cin + kTorgbOut) * sizeof(float);
  rc = ensure_dynamic_lds<&torgb_texels_fwd_kernel>(((size_t)kTorgbOut * kTorgbMaxCin + kTorgbMaxCin + kTorgbOut) * sizeof(float), "torgb_texels_fwd");
  if (rc) return rc;
  hipLaunchKernelGGL(torgb_texels_fwd_kernel, grid, dim3(256), shmem, (hipStream_t)stream, k);
  return check_launch("torgb_texels_fwd");
}

// the backward's arguments, for both entries (`entry`: the name in front of the messages)
static int torgb_bwd_common(const nfi_torgb_args* a, TorgbParams& k, const char* entry) {
  const int rc = torgb_common(a, k);
  if (rc) return rc;
  const char* bad = !(a->g_texels && a->g_x && a->g_styles) ? "g_texels / g_x / g_styles missing"
                    : a->g_previous_image && !a->previous_image ? "g_previous_image without previous_image" : nullptr;
  if (bad) {
    snprintf(nfi_err_buf, sizeof(nfi_err_buf), "%s: %s", entry, bad);
    return NFI_ERR_INVALID_ARGUMENT;
  }
  k.g_out = a->g_texels; k.g_x = a->g_x; k.g_styles = a->g_styles; k.g_weight = a->g_weight; k.g_bias = a->g_bias;
  k.g_prev = a->g_previous_image;
  return NFI_OK;
}

// The backward's grids, a function of the shape alone (which is what fixes the ordered entry's slot order): blocks per
// scene of the data kernels and their dynamic LDS, blocks and 64-channel groups of the weight kernels
struct TorgbBwdGrids { int data_blocks, weight_blocks, weight_groups; size_t data_lds; };
constexpr size_t kTorgbBwdMaxLds = ((size_t)kTorgbOut * kTorgbMaxCin + kTorgbMaxCin) * sizeof(float);

static TorgbBwdGrids torgb_bwd_grids(const nfi_torgb_args* a) {
  const int64_t P = (int64_t)a->resolution * a->resolution;
  TorgbBwdGrids g;
  g.data_blocks = (int)((P + kTorgbBlockPixels - 1) / kTorgbBlockPixels);
  g.weight_blocks = (int)std::min<int64_t>(((int64_t)a->n_scenes * (P / 16) + 3) / 4, 256);
  g.weight_groups = (a->in_channels + 63) / 64;
  g.data_lds = ((size_t)kTorgbOut * a->in_channels + a->in_channels) * sizeof(float);
  return g;
}

static void launch_upsample_bwd(const TorgbParams& k, hipStream_t s) {
  if (!k.g_prev) return;
  const int half = k.R / 2;
  const int64_t total = (int64_t)k.B * half * half * 24;
  hipLaunchKernelGGL(upsample_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, k);
}

extern "C" int nfi_torgb_texels_bwd(const nfi_torgb_args* a, nfi_stream_t stream) {
  TorgbParams k;
  int rc = torgb_bwd_common(a, k, "torgb_texels_bwd");
  if (rc) return rc;
  REQUIRE(!k.g_weight || k.g_bias, "torgb_texels_bwd: g_bias missing");      // before the first memset and launch
  const TorgbBwdGrids g = torgb_bwd_grids(a);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(k.g_styles, 0, sizeof(float) * (size_t)k.B * k.Cin, s) != hipSuccess) return fail(NFI_ERR_LAUNCH, "torgb_texels_bwd: memset failed");
  rc = ensure_dynamic_lds<&torgb_bwd_data_kernel>(kTorgbBwdMaxLds, "torgb_texels_bwd");
  if (rc) return rc;
  hipLaunchKernelGGL(torgb_bwd_data_kernel, dim3((unsigned)g.data_blocks, (unsigned)k.B), dim3(256), g.data_lds, s, k);
  if (k.g_weight) {
    if (hipMemsetAsync(k.g_weight, 0, sizeof(float) * (size_t)kTorgbOut * k.Cin, s) != hipSuccess ||
        hipMemsetAsync(k.g_bias, 0, sizeof(float) * kTorgbOut, s) != hipSuccess)
      return fail(NFI_ERR_LAUNCH, "torgb_texels_bwd: memset failed");
    hipLaunchKernelGGL(torgb_bwd_weight_kernel, dim3((unsigned)g.weight_blocks, (unsigned)g.weight_groups), dim3(256), 0, s, k,
                       k.R * k.R / 16);
  }
  launch_upsample_bwd(k, s);
  return check_launch("torgb_texels_bwd");
}

// The workspace of one nfi_torgb_texels_bwd_ordered call: byte offsets of its regions and the total
struct TorgbOrdCarve { size_t slots, part_w, part_b, total; };

static TorgbOrdCarve torgb_ord_carve(const nfi_torgb_args* a, const TorgbBwdGrids& g) {
  TorgbOrdCarve c;
  size_t at = 0;
  c.slots = at; at += align256((size_t)a->n_scenes * g.data_blocks * 4 * a->in_channels * sizeof(float));
  c.part_w = at; at += align256((size_t)g.weight_groups * g.weight_blocks * kTorgbOut * 64 * sizeof(float));
  c.part_b = at; at += align256((size_t)g.weight_blocks * kTorgbOut * sizeof(float));
  c.total = at;
  return c;
}

extern "C" size_t nfi_torgb_texels_bwd_ordered_workspace_bytes(const nfi_torgb_args* a) {
  return a && torgb_channels_ok(a) && torgb_resolution_ok(a) ? torgb_ord_carve(a, torgb_bwd_grids(a)).total : 0;
}

extern "C" int nfi_torgb_texels_bwd_ordered(const nfi_torgb_args* a, void* workspace, size_t workspace_bytes, nfi_stream_t stream) {
  TorgbParams k;
  int rc = torgb_bwd_common(a, k, "torgb_texels_bwd_ordered");
  if (rc) return rc;
  REQUIRE(!k.g_weight || k.g_bias, "torgb_texels_bwd_ordered: g_bias missing");
  REQUIRE(workspace, "torgb_texels_bwd_ordered: workspace missing");
  const TorgbBwdGrids g = torgb_bwd_grids(a);
  const TorgbOrdCarve ws = torgb_ord_carve(a, g);
  REQUIRE(workspace_bytes >= ws.total, "torgb_texels_bwd_ordered: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  // nothing here is read before this call has written it: every wave stores its slot, every block its partial
  auto region = [&](size_t at) { return reinterpret_cast<float*>(static_cast<char*>(workspace) + at); };
  float *slots = region(ws.slots), *part_w = region(ws.part_w), *part_b = region(ws.part_b);
  rc = ensure_dynamic_lds<&torgb_bwd_data_ordered_kernel>(kTorgbBwdMaxLds, "torgb_texels_bwd_ordered");
  if (rc) return rc;
  hipLaunchKernelGGL(torgb_bwd_data_ordered_kernel, dim3((unsigned)g.data_blocks, (unsigned)k.B), dim3(256), g.data_lds, s, k, slots);
  hipLaunchKernelGGL(torgb_bwd_styles_finish_kernel, dim3((unsigned)((k.B * k.Cin + 255) / 256)), dim3(256), 0, s, k, slots,
                     g.data_blocks * 4);
  if (k.g_weight) {
    hipLaunchKernelGGL(torgb_bwd_weight_ordered_kernel, dim3((unsigned)g.weight_blocks, (unsigned)g.weight_groups), dim3(256), 0, s,
                       k, k.R * k.R / 16, part_w, part_b);
    hipLaunchKernelGGL(torgb_bwd_weight_finish_kernel, dim3((unsigned)((kTorgbOut * k.Cin + kTorgbOut + 255) / 256)), dim3(256), 0, s, k,
                       part_w, part_b, g.weight_blocks);
  }
  launch_upsample_bwd(k, s);
  return check_launch("torgb_texels_bwd_ordered");
}
