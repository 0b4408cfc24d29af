// nfi_layout.inc — the storage layouts the kernels read: feature planes <-> texels (nfi_planes_to_texels,
// nfi_texels_to_planes) and the packers of the decoder image (nfi_decoder_pack, nfi_decoder_pack_viewdir), kernels and
// entry points (included by nfi_kernels.hip).  Expects nfi_host.hpp and `using namespace nfi`; nothing of the other topics.

// ------------------------------------------------------------------------------------------------
// planes [B,3,32,R,R] <-> texels [B,3,R,R,32]
// ------------------------------------------------------------------------------------------------
// 256 pixels x 32 channels per block through LDS.  Loads: 16 bytes per lane along the pixels (a wave reads 1 KB of one
// channel row per instruction).  tile[c][p + 8 (c >> 3)] with a row pitch of 288 floats: the 16-byte LDS writes stay
// aligned and contiguous, and the transposing reads - lane (p, q) gathers channels 8q .. 8q + 7 of pixel p - hit bank
// (p + 8 q) mod 32: conflict free.  Stores: every lane 32 contiguous bytes of its texel (4 lanes = one 128-B texel).
constexpr int kP2tPixels = 256, kP2tPitch = 288;
template <int TEX>
__global__ __launch_bounds__(256) void planes_to_texels_kernel(const float* __restrict__ planes, void* __restrict__ texels,
                                                               int hw) {
  __shared__ __attribute__((aligned(16))) float tile[kC][kP2tPitch];
  const int img = blockIdx.y;                 // b*3 + plane
  const int px0 = blockIdx.x * kP2tPixels;
  const float* src = planes + (size_t)img * kC * hw;
  {
    const int c4 = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    if ((hw & 3) == 0 && px0 + kP2tPixels <= hw) {
      f32x4 v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f32x4*>(src + (size_t)(r0 + 4 * i) * hw + px0 + 4 * c4);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int c = r0 + 4 * i;
        *reinterpret_cast<f32x4*>(&tile[c][4 * c4 + 8 * (c >> 3)]) = v[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int c = r0 + 4 * i;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int px = px0 + 4 * c4 + e;
          tile[c][4 * c4 + e + 8 * (c >> 3)] = (px < hw) ? src[(size_t)c * hw + px] : 0.0f;
        }
      }
    }
  }
  __syncthreads();
  const int q = threadIdx.x & 3;              // channel octet
#pragma unroll
  for (int it = 0; it < kP2tPixels / 64; ++it) {
    const int p = it * 64 + (threadIdx.x >> 2);
    if (px0 + p >= hw) continue;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tile[q * 8 + k][p + 8 * q];
    if (TEX == 0) {
      float4* dst = reinterpret_cast<float4*>(reinterpret_cast<float*>(texels) + ((size_t)img * hw + px0 + p) * kC + q * 8);
      dst[0] = make_float4(v[0], v[1], v[2], v[3]);
      dst[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else if (TEX == 2) {
      typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
      uint32_t w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        f16x2 h = {(_Float16)v[2 * k], (_Float16)v[2 * k + 1]};   // round-to-nearest-even fp32 -> fp16
        w[k] = __builtin_bit_cast(uint32_t, h);
      }
      uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(texels) + ((size_t)img * hw + px0 + p) * kC + q * 8);
      dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      uint32_t w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        // round-to-nearest-even fp32 -> bf16
        uint32_t a = f2bits(v[2 * k]), b = f2bits(v[2 * k + 1]);
        a = (a + 0x7FFFu + ((a >> 16) & 1u)) >> 16;
        b = (b + 0x7FFFu + ((b >> 16) & 1u)) >> 16;
        w[k] = a | (b << 16);
      }
      uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(texels) + ((size_t)img * hw + px0 + p) * kC + q * 8);
      dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

__global__ __launch_bounds__(256) void texels_to_planes_kernel(const float* __restrict__ texels, float* __restrict__ planes,
                                                               int hw) {
  __shared__ float tile[kC][65];
  const int img = blockIdx.y;
  const int px0 = blockIdx.x * 64;
  const int p = threadIdx.x >> 2, q = threadIdx.x & 3;
  if (px0 + p < hw) {
    const float4* src = reinterpret_cast<const float4*>(texels + ((size_t)img * hw + px0 + p) * kC + q * 8);
    float4 a = src[0], b = src[1];
    tile[q * 8 + 0][p] = a.x; tile[q * 8 + 1][p] = a.y; tile[q * 8 + 2][p] = a.z; tile[q * 8 + 3][p] = a.w;
    tile[q * 8 + 4][p] = b.x; tile[q * 8 + 5][p] = b.y; tile[q * 8 + 6][p] = b.z; tile[q * 8 + 7][p] = b.w;
  }
  __syncthreads();
  float* dst = planes + (size_t)img * kC * hw;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
  for (int c = ty; c < kC; c += 4) {
    int px = px0 + tx;
    if (px < hw) dst[(size_t)c * hw + px] = tile[c][tx];
  }
}

extern "C" int nfi_planes_to_texels(const float* planes, void* texels, int n_scenes, int plane_res, int texel_dtype,
                                    nfi_stream_t stream) {
  REQUIRE(planes && texels, "planes_to_texels: null pointer");
  REQUIRE(n_scenes > 0 && plane_res >= 2 && plane_res <= 1024, "planes_to_texels: plane_res must be in [2,1024]");
  REQUIRE(texel_dtype >= NFI_TEXEL_F32 && texel_dtype <= NFI_TEXEL_F16, "planes_to_texels: bad texel dtype");
  int hw = plane_res * plane_res;
  dim3 grid((hw + kP2tPixels - 1) / kP2tPixels, n_scenes * 3);
  if (texel_dtype == NFI_TEXEL_F32)
    hipLaunchKernelGGL(planes_to_texels_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, planes, texels, hw);
  else if (texel_dtype == NFI_TEXEL_BF16)
    hipLaunchKernelGGL(planes_to_texels_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, planes, texels, hw);
  else
    hipLaunchKernelGGL(planes_to_texels_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, planes, texels, hw);
  return check_launch("planes_to_texels");
}

extern "C" int nfi_texels_to_planes(const float* texels, float* planes, int n_scenes, int plane_res, nfi_stream_t stream) {
  REQUIRE(planes && texels, "texels_to_planes: null pointer");
  REQUIRE(n_scenes > 0 && plane_res >= 2 && plane_res <= 1024, "texels_to_planes: plane_res must be in [2,1024]");
  int hw = plane_res * plane_res;
  dim3 grid((hw + 63) / 64, n_scenes * 3);
  hipLaunchKernelGGL(texels_to_planes_kernel, grid, dim3(256), 0, (hipStream_t)stream, texels, planes, hw);
  return check_launch("texels_to_planes");
}

// ------------------------------------------------------------------------------------------------
// decoder operand image
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int feat_channel(int tex, int s, int g) {
  // which plane channel sits in feature register s of channel group g (see load_texel8)
  return tex == 0 ? ((s < 4) ? 4 * g + s : 16 + 4 * g + (s - 4)) : 8 * g + s;
}

__global__ __launch_bounds__(256) void decoder_pack_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2,
                                                           int n_out, int tex, float* __restrict__ image) {
  const float gain1 = 0.17677669529663687f;  // 1/sqrt(32)  (models/stylegan.py:171)
  const float gain2 = 0.125f;                // 1/sqrt(64)
  // one element per thread over ceil(kImageFloats / 256) workgroups (one workgroup walking the image took 11 us: 25
  // dependent round trips to the weights)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kImageFloats; i += gridDim.x * blockDim.x) {
    float v = 0.0f;
    if (i < kW2F) {
      int k = i - kW1F;
      int nt = k & 3, lane = (k >> 2) & 63, s = k >> 8;
      int row = 16 * nt + (lane & 15);
      int ch = feat_channel(tex, s, lane >> 4);
      // gain, the /3 of the three-plane mean (generator.py:328) and log2(e) for the base-2 softplus
      v = (w1[row * kC + ch] * gain1) * (kLog2e / 3.0f);
    } else if (i < kB1F) {
      int k = i - kW2F;
      int r = k & 3, lane = (k >> 2) & 63, nt = k >> 8;
      int row = lane & 15;
      int hid = 16 * nt + 4 * (lane >> 4) + r;
      if (row < n_out) {
        float w = w2[row * kHidden + hid] * gain2;
        // softplus was computed in base 2 (missing factor ln2).  Row 0 (distance / density) stays in
        // natural units; feature rows are wanted times log2(e) for the base-2 softmax/sigmoid, and
        // ln2*log2e == 1.
        v = (row == 0) ? w * kLn2 : w;
      }
    } else if (i < kB2F) {
      int k = i - kB1F;
      int r = k & 3, nt = (k >> 2) & 3, g = k >> 4;
      v = b1[16 * nt + 4 * g + r] * kLog2e;
    } else if (i < kW1H) {
      int k = i - kB2F;
      int row = k;  // 4g + r
      if (row < n_out) v = (row == 0) ? b2[0] : b2[row] * kLog2e;
    } else {
      // fp16 hi/lo operand images: one dword = two consecutive k-elements of one lane
      float w2v[2];
      int hl;
      if (i < kW2H) {
        int k = i - kW1H;
        int d = k & 3, lane = (k >> 2) & 63;
        hl = (k >> 8) & 1;
        int nt = k >> 9;
        int row = 16 * nt + (lane & 15);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          int ch = feat_channel(tex, 2 * d + h, lane >> 4);
          w2v[h] = (w1[row * kC + ch] * gain1) * (kLog2e / 3.0f);
        }
      } else {
        int k = i - kW2H;
        int d = k & 3, lane = (k >> 2) & 63;
        hl = (k >> 8) & 1;
        int kk = k >> 9;
        int row = lane & 15;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          int e = 2 * d + h;
          int hid = 16 * (2 * kk + (e >> 2)) + 4 * (lane >> 4) + (e & 3);
          float w = 0.0f;
          if (row < n_out) { w = w2[row * kHidden + hid] * gain2; if (row == 0) w *= kLn2; }
          w2v[h] = w;
        }
      }
      auto hi = __builtin_amdgcn_cvt_pkrtz(w2v[0], w2v[1]);
      auto lo = __builtin_amdgcn_cvt_pkrtz(w2v[0] - (float)hi[0], w2v[1] - (float)hi[1]);
      v = bits2f(hl == 0 ? __builtin_bit_cast(uint32_t, hi) : __builtin_bit_cast(uint32_t, lo));
    }
    image[i] = v;
  }
}

extern "C" size_t nfi_decoder_image_floats(void) { return (size_t)kImageFloats; }

extern "C" int nfi_decoder_pack(const float* w1, const float* b1, const float* w2, const float* b2, int n_attention,
                                int texel_dtype, float* image, nfi_stream_t stream) {
  REQUIRE(w1 && b1 && w2 && b2 && image, "decoder_pack: null pointer");
  REQUIRE(n_attention >= 0 && n_attention <= NFI_MAX_ATTENTION, "decoder_pack: attention_values must be in [0,14]");
  REQUIRE(texel_dtype >= NFI_TEXEL_F32 && texel_dtype <= NFI_TEXEL_F16, "decoder_pack: bad texel dtype");
  int n_out = n_attention > 0 ? 1 + n_attention : 4;
  hipLaunchKernelGGL(decoder_pack_kernel, dim3((kImageFloats + 255) / 256), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, b2,
                     n_out, texel_dtype, image);
  return check_launch("decoder_pack");
}

__global__ __launch_bounds__(256) void decoder_pack_vd_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                              const float* __restrict__ w2, const float* __restrict__ b2,
                                                              const float* __restrict__ w3, const float* __restrict__ b3,
                                                              int n3, int tex, float* __restrict__ image) {
  const float gain1 = 0.17677669529663687f;  // 1/sqrt(32)
  const float gain2 = 0.125f;                // 1/sqrt(64)
  const float gain3 = 0.17677669529663687f;  // 1/sqrt(32)
  for (int i = threadIdx.x; i < kVdImageFloats; i += blockDim.x) {
    float v = 0.0f;
    if (i < kVdB1F) {
      int k = i - kVdW1F;
      int nt = k & 3, lane = (k >> 2) & 63, s = k >> 8;
      int row = 16 * nt + (lane & 15);
      int ch = feat_channel(tex, s, lane >> 4);
      v = (w1[row * kC + ch] * gain1) * (kLog2e / 3.0f);
    } else if (i < kVdW2) {
      int k = i - kVdB1F;
      int r = k & 3, nt = (k >> 2) & 3, g = k >> 4;
      v = b1[16 * nt + 4 * g + r] * kLog2e;
    } else if (i < kVdB2) {
      int k = i - kVdW2;
      int r = k & 3, lane = (k >> 2) & 63, nt = (k >> 8) & 3, t = k >> 10;
      int row = 16 * t + (lane & 15);
      int hid = 16 * nt + 4 * (lane >> 4) + r;
      if (row < 33) v = (w2[row * kHidden + hid] * gain2) * kLn2;   // every row stays in natural units
    } else if (i < kVdW3) {
      int row = i - kVdB2;                                           // 16t + 4g + r
      if (row < 33) v = b2[row];
    } else if (i < kVdB3) {
      int k = i - kVdW3;
      int r = k & 3, lane = (k >> 2) & 63, t = k >> 8;
      int out = lane & 15;
      int kk = 16 * t + 4 * (lane >> 4) + r;                          // second-layer row feeding this K slot
      if (out == 0) v = (kk == 0) ? 1.0f : 0.0f;                      // the distance passes through
      else if (out <= n3 && kk >= 1 && kk <= 32) v = (w3[(out - 1) * 32 + (kk - 1)] * gain3) * kLog2e;
    } else {
      int out = i - kVdB3;
      if (out >= 1 && out <= n3) v = b3[out - 1] * kLog2e;
    }
    image[i] = v;
  }
}

extern "C" size_t nfi_decoder_image_floats_viewdir(void) { return (size_t)kVdImageFloats; }

extern "C" int nfi_decoder_pack_viewdir(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                                        const float* b3, int n_attention, int texel_dtype, float* image,
                                        nfi_stream_t stream) {
  REQUIRE(w1 && b1 && w2 && b2 && w3 && b3 && image, "decoder_pack_viewdir: null pointer");
  REQUIRE(n_attention >= 0 && n_attention <= NFI_MAX_ATTENTION, "decoder_pack_viewdir: attention_values must be in [0,14]");
  REQUIRE(texel_dtype >= NFI_TEXEL_F32 && texel_dtype <= NFI_TEXEL_F16, "decoder_pack_viewdir: bad texel dtype");
  static_assert(NFI_RAY_FEATURE_PITCH == kRayFeatPad, "ray feature pitch");
  int n3 = n_attention > 0 ? n_attention : 3;
  hipLaunchKernelGGL(decoder_pack_vd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, b2, w3, b3, n3,
                     texel_dtype, image);
  return check_launch("decoder_pack_viewdir");
}
