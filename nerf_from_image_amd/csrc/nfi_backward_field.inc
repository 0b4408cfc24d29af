// nfi_backward_field.inc — backward of the triplane field query (included by nfi_backward_field.hip).
//
// Reference: autograd through the sampler closure (models/generator.py:587-681): grid_sample
// backward (atomic scatter-add into the planes + coordinate gradients), the decoder MLP, the
// Laplace-CDF density and the attention colour head.  Here: one kernel, forward recomputed per
// 16-point tile (nothing but the points and the upstream gradients is read from HBM), every
// contraction on the matrix pipe (split-fp16 or fp32 operands: the two decoder back ends below):
//
//   gs^T [64x16] = W2^T [64x16] g_o^T [16x16]      (operands in accumulator layout)
//   gf^T [32x16] = W1^T [32x64] gh^T  [64x16]
//   dW2  [16x64] += g_o [16xpts] s^T  [ptsx64]     (points along K: operands staged in LDS)
//   dW1  [64x32] += gh  [64xpts] f^T  [ptsx32]
//
// Weight/bias/attention/beta/alpha gradients accumulate in registers over all tiles a wave
// processes and are flushed once per block with atomics.  The per-point feature gradient gf (32 floats) either goes
// straight into the gradient image with fp32 atomics (small queries) or to a workspace row, from which
// the binned scatter (bin_count / bin_scan / bin_fill / bin_reduce kernels below) merges the points of a texel cell
// before they reach the atomic units.  The coordinate gradients J^T gf stay here: their second gather hits lines this
// wave has just loaded - a separate gather pass was measured at 1.0 ms per 4.2 M points against 0.25 ms in place.
// The upstream gradients are loaded per tile in the MFMA layout (staging a chunk's worth through lane permutes or LDS
// was measured: no gain).  scatter_mode 2 ("ordered mode" below) replaces every one of these float atomics by a sum in a
// fixed order: rows gathered per texel from sorted keys, one workspace slot per wave for the parameter gradients.

constexpr int kBwdW2T = 0;                       // fp16 hi/lo: [4 m-tiles][2][64 lanes][4 dwords] (K slots 4..7 are zero)
constexpr int kBwdW1T = kBwdW2T + 4 * 2 * 64 * 4;    // fp16 hi/lo: [2 m-tiles][2 k-chunks][2][64 lanes][4 dwords]
constexpr int kBwdImageFloats = kBwdW1T + 2 * 2 * 2 * 64 * 4;   // 4096
constexpr int kBwdFwdFloats = kFieldLdsFloats;   //                    // fp32 forward operands + attention values staged by the backward kernel

__global__ __launch_bounds__(256) void decoder_pack_bwd_kernel(const float* __restrict__ w1, const float* __restrict__ w2,
                                                               int n_out, float* __restrict__ image) {
  // split-fp16 (hi + lo) A fragments of the two backward contractions over rows / hidden units (dwords = half pairs):
  //   W2T [4 m-tiles (hidden)][hi,lo][64 lanes][4 dwords]   v_mfma_f32_16x16x32_f16 with half of its K slots empty:
  //        A[i = hid 16mt+i][k-slot 8kb+e = output row 4kb+e for e < 4, zero for e >= 4]  (the four rows a lane group
  //        holds in accumulator layout).  [The K = 16 instruction v_mfma_f32_16x16x16_f16 fits the shape exactly, but with
  //        it the results of the LAST pass - points 12..15 of a tile - were occasionally read before they were written
  //        (timing-dependent wrong gradients for those points on MI355X / ROCm 7.2); the K = 32 form is the one the
  //        forward kernels use and has never shown that.]
  //   W1T [2 m-tiles (channels)][2 k-chunks][hi,lo][64 lanes][4 dwords]   v_mfma_f32_16x16x32_f16:
  //        A[i = ch 16mt2+i][k-slot 8kb+e = hidden 16(2kk + e/4) + 4kb + e%4]   (the accumulator layout of gh is its B operand)
  const float gain1 = 0.17677669529663687f, gain2 = 0.125f;
  for (int i = threadIdx.x; i < kBwdImageFloats; i += blockDim.x) {
    float v[2];
    int hl;
    if (i < kBwdW1T) {
      const int d = i & 3, lane = (i >> 2) & 63;
      hl = (i >> 8) & 1;
      const int mt = i >> 9;
      const int hid = 16 * mt + (lane & 15);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int e = 2 * d + h, row = 4 * (lane >> 4) + e;
        v[h] = (e < 4 && row < n_out) ? w2[row * kHidden + hid] * gain2 : 0.0f;
      }
    } else {
      const int k = i - kBwdW1T;
      const int d = k & 3, lane = (k >> 2) & 63;
      hl = (k >> 8) & 1;
      const int kk = (k >> 9) & 1, mt2 = k >> 10;
      const int ch = 16 * mt2 + (lane & 15);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int e = 2 * d + h;
        const int hid = 16 * (2 * kk + (e >> 2)) + 4 * (lane >> 4) + (e & 3);
        v[h] = w1[hid * kC + ch] * gain1;
      }
    }
    auto hi = __builtin_amdgcn_cvt_pkrtz(v[0], v[1]);
    auto lo = __builtin_amdgcn_cvt_pkrtz(v[0] - (float)hi[0], v[1] - (float)hi[1]);
    image[i] = bits2f(hl == 0 ? __builtin_bit_cast(uint32_t, hi) : __builtin_bit_cast(uint32_t, lo));
  }
}

// view-direction decoder: W3T [3 m-tiles (48 second-layer rows)][64 lanes][4 k-steps over the 16 outputs],
// W2T [4 m-tiles (hidden)][3 k-tiles][64 lanes][4], W1T as above
constexpr int kVbW3T = 0;
constexpr int kVbW2T = kVbW3T + 3 * 64 * 4;              // 768
constexpr int kVbW1T = kVbW2T + 4 * 3 * 64 * 4;          // 3840
constexpr int kVbImageFloats = kVbW1T + 2 * 4 * 64 * 4;  // 5888

__global__ __launch_bounds__(256) void decoder_pack_bwd_vd_kernel(const float* __restrict__ w1, const float* __restrict__ w2,
                                                                  const float* __restrict__ w3, int n3,
                                                                  float* __restrict__ image) {
  const float gain1 = 0.17677669529663687f, gain2 = 0.125f, gain3 = 0.17677669529663687f;
  for (int i = threadIdx.x; i < kVbImageFloats; i += blockDim.x) {
    float v = 0.0f;
    if (i < kVbW2T) {
      // A[i = second-layer row kk = 16t + (lane&15)][k = output 4(lane>>4) + r]
      int r = i & 3, lane = (i >> 2) & 63, t = i >> 8;
      int kk = 16 * t + (lane & 15), out = 4 * (lane >> 4) + r;
      if (out == 0) v = (kk == 0) ? 1.0f : 0.0f;
      else if (out <= n3 && kk >= 1 && kk <= 32) v = w3[(out - 1) * 32 + (kk - 1)] * gain3;
    } else if (i < kVbW1T) {
      // A[i = hidden 16mt + (lane&15)][k = second-layer row 16t + 4(lane>>4) + r]
      int k = i - kVbW2T;
      int r = k & 3, lane = (k >> 2) & 63, t = (k >> 8) % 3, mt = k / 768;
      int hid = 16 * mt + (lane & 15), row = 16 * t + 4 * (lane >> 4) + r;
      if (row < 33) v = w2[row * kHidden + hid] * gain2;
    } else {
      int k = i - kVbW1T;
      int r = k & 3, lane = (k >> 2) & 63, nt = (k >> 8) & 3, mt2 = k >> 10;
      int hid = 16 * nt + 4 * (lane >> 4) + r, ch = 16 * mt2 + (lane & 15);
      v = w1[hid * kC + ch] * gain1;
    }
    image[i] = v;
  }
}

struct FieldBwdParams {
  const float* points; int64_t P;
  const float* texels; int res;
  const float* image; const float* image_bwd; int A; const float* att;
  int use_sdf; const float* beta; const float* alpha; float scene_range;
  const float* g_sigma; const float* g_rgb; const float* g_sdf; const float* g_sem;
  float* g_texels; float* g_points;
  float* g_w1; float* g_b1; float* g_w2; float* g_b2; float* g_att; float* g_beta; float* g_alpha;
  int points_only; int normalize_points;
  const float* xray; int spr; float* g_xray; float* g_w3; float* g_b3;
  float* gf_out;                     // per-point feature gradient [B,P,32] (binned scatter and / or coordinate gradients)
  uint8_t* bin_flag;                 // binned scatter: [B,P] 1 = the point's gradient row is not all zero (null: atomic mode)
  int layout;                        // texel layout of texels AND g_texels (nfi_device.hpp)
  // ray-order hint (0 tiles: none): the points are [rays][cpr * 64] with the rays in row-major order of an image `tw` rays
  // wide; the kernel then walks them in tside x tside-pixel tiles, every XCD (= blockIdx.x % 8) one tile at a time
  int n_tiles, tiles_x, tside, tw, cpr;
  FastDiv div_cpr, div_tside, div_tiles_x;      // the tile walk's three divisions (wave-uniform operands: scalar-ALU work)
  // ordered mode (scatter_mode 2): the parameter-gradient pointers above are slot 0 of per-wave slots in the workspace,
  // slot_stride floats apart (0: the caller's buffers, shared by every wave; a slot holds its wave's scene's rows of g_att only)
  uint32_t slot_stride;
};

// ================================================================================================
// field_query_bwd_kernel = one shell (chunk walk, point set-up, gather, epilogue backward, row hand-off, scatter,
// coordinate gradients: the named steps below) around one of two decoder back ends (PlainDecoderBwd, ViewdirDecoderBwd:
// accumulators, per-wave LDS layout, forward recompute, backward to the feature gradient, flush).
// ================================================================================================

// A tile's 16 points are held in two lane layouts: L (load: lane = 4 lp + lq - point lp, channel chunk lq) and
// M (MFMA accumulator: lane = 16 g + j - point j, rows 4 g .. 4 g + 3)
struct BwdLane { int lane, j, g, lp, lq; };

// per-scene bases (uniform: scalar registers) and 32-bit point offsets instead of 64-bit address arithmetic per access
// (round 5: - 3 % with the softplus median below; points_per_scene <= 2^30 - and <= 2^25 where the 128-byte rows exist -
// keep every element offset under 2^32: checked by the launcher)
struct BwdScene {
  int scene;
  const float *pts, *gsig, *grgb, *gsdf;
  float* gfout;
  uint8_t* flag;
  float* gtex;
  size_t g_pix, g_plane, g_row;      // gradient image strides in floats (fp32 whatever the texel storage; same layout as the texels)
};

__device__ __forceinline__ BwdScene enter_bwd_scene(const FieldBwdParams& k, int scene) {
  BwdScene S;
  S.scene = scene;
  S.gtex = k.g_texels + (size_t)scene * 3 * k.res * k.res * kC;
  S.g_pix = k.layout ? 3 * kC : kC; S.g_plane = k.layout ? (size_t)kC : (size_t)k.res * k.res * kC; S.g_row = (size_t)k.res * S.g_pix;
  S.pts = k.points + (size_t)scene * k.P * 3;
  S.gsig = k.g_sigma + (size_t)scene * k.P;
  S.grgb = k.g_rgb + (size_t)scene * k.P * 3;
  S.gsdf = k.g_sdf ? k.g_sdf + (size_t)scene * k.P : nullptr;
  S.gfout = k.gf_out ? k.gf_out + (size_t)scene * k.P * kC : nullptr;
  S.flag = k.bin_flag ? k.bin_flag + (size_t)scene * k.P : nullptr;
  return S;
}

// ---- step: next chunk ----
// Order of the chunks (64 consecutive points).  Plain: grid-stride.  With the ray-order hint: the rays of one image
// tile (a thin column of the volume: its footprint in the three planes is a few hundred KB) are taken by the waves of
// ONE XCD, tile after tile, so that the texels a tile gathers stay in that XCD's 4 MB of L2 instead of every XCD
// streaming the whole slice of the volume that two image rows cut (52 % L2 hits, 5.5 GB fetched per 8.4 M points).
// next() RETURNS the chunk (-1: none left): with `bool next(int64_t& chunk)` and the variable in front of the loop the
// chunk became loop-carried and every one of the 16 kernels spilled (profiles/r10/README.md).
struct ChunkWalk {
  int64_t n_chunks, lin;
  bool tiled;
  int chunks_per_tile, waves_per_xcd, tile, cc;
  __device__ __forceinline__ ChunkWalk(const FieldBwdParams& k, int wave)
      : n_chunks((k.P + 63) / 64), lin((int64_t)blockIdx.x * 4 + wave), tiled(k.n_tiles > 0),
        chunks_per_tile(k.tside * k.tside * k.cpr), waves_per_xcd((int)(gridDim.x >> 3) * 4), tile((int)(blockIdx.x & 7)),
        cc((int)(blockIdx.x >> 3) * 4 + wave) {}
  __device__ __forceinline__ int64_t next(const FieldBwdParams& k) {
    int64_t chunk;
    if (!tiled) {
      if (lin >= n_chunks) return -1;
      chunk = lin;
      lin += (int64_t)gridDim.x * 4;
    } else {
      while (cc >= chunks_per_tile && tile < k.n_tiles) { cc -= chunks_per_tile; tile += 8; }
      if (tile >= k.n_tiles) return -1;
      const int rt = (int)fastdiv((uint32_t)cc, k.div_cpr), half = cc - rt * k.cpr;
      const int ty = (int)fastdiv((uint32_t)rt, k.div_tside), tx = rt - ty * k.tside;
      const int tile_y = (int)fastdiv((uint32_t)tile, k.div_tiles_x), tile_x = tile - tile_y * k.tiles_x;
      chunk = ((int64_t)(tile_y * k.tside + ty) * k.tw + tile_x * k.tside + tx) * k.cpr + half;
      cc += waves_per_xcd;
    }
    return chunk;
  }
};

// ---- step: point set-up and flags (lane = point of the chunk) ----
struct ChunkPoints {
  int64_t chunk;
  bool valid;
  uint32_t gi;                       // offset inside the scene (scene bases above)
  float fx, fy, fz;
  int xi;                            // x0 | y0 << 10 | z0 << 20
  int flags;                         // 1 outside the cube, 2 valid, 4 / 8 / 16 coordinate x / y / z inside (0, R-1)
  uint64_t live;
};

__device__ __forceinline__ ChunkPoints chunk_points(const FieldBwdParams& k, const FieldParams& P, const BwdScene& S, int64_t chunk,
                                                    int lane) {
  ChunkPoints C;
  C.chunk = chunk;
  const int64_t p = chunk * 64 + lane;
  const bool valid = p < k.P;
  const uint32_t gi = valid ? (uint32_t)p : 0u;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (valid) { px = S.pts[gi * 3u]; py = S.pts[gi * 3u + 1u]; pz = S.pts[gi * 3u + 2u]; }
  const float qx = px / k.scene_range, qy = py / k.scene_range, qz = pz / k.scene_range;
  const bool out = (fabsf(qx) > 1.0f) || (fabsf(qy) > 1.0f) || (fabsf(qz) > 1.0f);
  int x0, y0, z0;
  float fx, fy, fz;
  plane_coord(qx, P.res_m1, P.res, x0, fx);
  plane_coord(qy, P.res_m1, P.res, y0, fy);
  plane_coord(qz, P.res_m1, P.res, z0, fz);
  // border clamp: zero coordinate gradient where the unnormalised coordinate is outside (0, R-1)
  auto inside = [&](float q) { float u = ((q + 1.0f) / 2.0f) * P.res_m1; return (u > 0.0f && u < P.res_m1) ? 1 : 0; };
  C.flags = (out ? 1 : 0) | (valid ? 2 : 0) | (inside(qx) << 2) | (inside(qy) << 3) | (inside(qz) << 4);
  if (!valid) { x0 = y0 = z0 = 0; fx = fy = fz = 0.0f; }
  C.xi = (int)((uint32_t)x0 | ((uint32_t)y0 << 10) | ((uint32_t)z0 << 20));
  C.valid = valid; C.gi = gi; C.fx = fx; C.fy = fy; C.fz = fz;
  // a point contributes only if it is valid and inside the cube (sigma and its gradient are masked
  // by (1-outside); rgb of an outside point still has a gradient path to the colour head, exactly
  // like the reference, so only INVALID points are dropped from the work mask)
  C.live = __ballot(valid);
  return C;
}

// ---- step: the upstream-gradient peek ----
// does anything flow into the chunk's points?  ONE coalesced look at the upstream gradients per chunk (lane = point)
// instead of a dependent, four-fold redundant load in front of every tile's gather (field backward 1.785 -> 1.768 ms
// per 8.4 M points, profiles/r5/bwd_ab_moments_peek_prio.log)
__device__ __forceinline__ uint64_t upstream_peek(const FieldBwdParams& k, const BwdScene& S, const ChunkPoints& C) {
  bool nz = false;
  if (C.valid) {
    const uint32_t gi = C.gi;
    nz = __builtin_nontemporal_load(S.gsig + gi) != 0.0f || __builtin_nontemporal_load(S.grgb + gi * 3u) != 0.0f ||
         __builtin_nontemporal_load(S.grgb + gi * 3u + 1u) != 0.0f || __builtin_nontemporal_load(S.grgb + gi * 3u + 2u) != 0.0f ||
         (S.gsdf && __builtin_nontemporal_load(S.gsdf + gi) != 0.0f);
  }
  return k.g_sem ? ~0ull : __ballot(nz);
}

// one 16-point tile of a chunk: this lane's point in both layouts
struct BwdTile {
  int t, srcL;
  float cfx, cfy, cfz;
  uint32_t cxi;
  int flL, flM;
  int64_t ptM;                       // this lane's point in MFMA layout
};

__device__ __forceinline__ BwdTile tile_lanes(const ChunkPoints& C, int t, const BwdLane& L) {
  BwdTile T;
  const int srcL = 16 * t + L.lp, srcM = 16 * t + L.j;
  T.t = t; T.srcL = srcL;
  T.cfx = __shfl(C.fx, srcL, 64); T.cfy = __shfl(C.fy, srcL, 64); T.cfz = __shfl(C.fz, srcL, 64);
  T.cxi = (uint32_t)__shfl(C.xi, srcL, 64);
  T.flL = __shfl(C.flags, srcL, 64); T.flM = __shfl(C.flags, srcM, 64);
  T.ptM = C.chunk * 64 + srcM;
  return T;
}

// nothing flows into the tile (rays the renderer skipped, samples of zero weight, padding): every gradient of the tile is
// exactly zero - no gather, no MLP, no rows for the scatter
template <bool COORD>
__device__ __forceinline__ void zero_tile_outputs(const FieldBwdParams& k, const BwdScene& S, const ChunkPoints& C, const BwdTile& T,
                                                  const BwdLane& L) {
  if (k.bin_flag && L.g == 0 && T.ptM < k.P) k.bin_flag[(size_t)S.scene * k.P + T.ptM] = 0;
  if (COORD && k.g_points && L.lq == 0 && (T.flL & 2)) {
    float* gp = k.g_points + ((size_t)S.scene * k.P + C.chunk * 64 + T.srcL) * 3;
    gp[0] = 0.0f; gp[1] = 0.0f; gp[2] = 0.0f;
  }
}

// column of feature slot group q / g in the [point][channel] LDS tiles: fp32 texels: a lane owns channels
// {4q..4q+3, 16+4q..16+4q+3}; 16-bit texels: {8q..8q+7} (load_texel8): the first four slots at kColA * q, the other four
// kColB further
template <int TEX> struct FeatCols { static constexpr int kColA = TEX == 0 ? 4 : 8, kColB = TEX == 0 ? 16 : 4; };

// ---- step: gather plus L -> M transposition (through the fp32 tile F_T [16][36] at `ft`) ----
template <int TEX>
__device__ __forceinline__ void gather_features(const FieldParams& P, const BwdTile& T, const BwdLane& L, float* ft, float (&feat)[8]) {
  constexpr int kColA = FeatCols<TEX>::kColA, kColB = FeatCols<TEX>::kColB;
  float featL[8];
  {
    TileTex<TEX> tex;
    tile_issue<TEX>(P, L.lq, T.cxi, tex);
    tile_bilinear<TEX>(tex, T.cfx, T.cfy, T.cfz, featL);        // sum of the three planes (the /3 lives in W1F)
  }
  f32x4* wr = reinterpret_cast<f32x4*>(ft + L.lp * 36 + L.lq * kColA);
  wr[0] = f32x4{featL[0], featL[1], featL[2], featL[3]};
  wr[kColB / 4] = f32x4{featL[4], featL[5], featL[6], featL[7]};
  wave_lds_fence();
  const f32x4* rd = reinterpret_cast<const f32x4*>(ft + L.j * 36 + L.g * kColA);
  const f32x4 lo = rd[0], hi = rd[kColB / 4];
  feat[0] = lo.x; feat[1] = lo.y; feat[2] = lo.z; feat[3] = lo.w;
  feat[4] = hi.x; feat[5] = hi.y; feat[6] = hi.z; feat[7] = hi.w;
}

// hidden pre-activations -> softplus in base 2 (= softplus / ln2), accumulator layout
__device__ __forceinline__ void softplus2_tile(f32x4 (&sp)[4]) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float h = sp[nt][r];
      float s2 = __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(h));
      sp[nt][r] = __builtin_amdgcn_fmed3f(s2, h, 128.0f);     // == (h > thr ? h : s2) wherever the two differ in fp32 (tile_mlp)
    }
}

// ---- step: epilogue backward: upstream gradients -> g_o (rows 4g+r of point j) ----
// SDF / density into row 0; softmax over the colour table (ATT; the table's gradient dV on the matrix pipe, through the
// scratch rows at `rows`) or sigmoid into the colour rows.  dVacc is a 16 x 16 MFMA accumulator whose columns 0..2 are
// dV[row][c] = sum_pt p[row] g_rgb[c] (column 3 belongs to the decoder back end).
template <bool ATT>
__device__ __forceinline__ f32x4 epilogue_bwd(const FieldBwdParams& k, const FieldParams& P, const BwdScene& S, const BwdTile& T,
                                              const BwdLane& L, const f32x4& o, float alpha_v, float* rows, f32x4& dVacc,
                                              float& d_beta, float& d_alpha) {
  const int j = L.j, g = L.g, A = k.A;
  const bool pv = (T.flM & 2) != 0;
  const float keep = (T.flM & 1) ? 0.0f : 1.0f;          // 1 - outside
  const uint32_t ptU = (uint32_t)T.ptM;
  const float gsig = pv ? S.gsig[ptU] : 0.0f;
  float grgb[3] = {0.0f, 0.0f, 0.0f};
  if (pv) { grgb[0] = S.grgb[ptU * 3u]; grgb[1] = S.grgb[ptU * 3u + 1u]; grgb[2] = S.grgb[ptU * 3u + 2u]; }
  f32x4 go = {0.0f, 0.0f, 0.0f, 0.0f};
  const float sdf = bcast_row0(o.x);
  float g_d = (pv && S.gsdf) ? S.gsdf[ptU] : 0.0f;
  if (k.use_sdf) {
    // sigma = (1/alpha) * cdf(-d) * keep,  cdf(x) = 0.5 + 0.5 sign(x) (1 - exp(-|x|/beta))
    const float ad = fabsf(sdf);
    const float e = __builtin_amdgcn_exp2f(ad * P.neg_log2e_over_beta);
    const float sgn = (sdf < 0.0f) ? 1.0f : ((sdf > 0.0f) ? -1.0f : 0.0f);   // sign(-d)
    const float cdf = 0.5f + 0.5f * sgn * (1.0f - e);
    g_d += (sdf != 0.0f) ? gsig * (-(P.inv_alpha * keep) * (0.5f / P.beta) * e) : 0.0f;   // torch.sign(0) == 0
    if (g == 0) {
      d_beta += gsig * (P.inv_alpha * keep) * (-0.5f * sgn * ad * e / (P.beta * P.beta));
      d_alpha += gsig * (-(P.inv_alpha * cdf * keep) / alpha_v);
    }
  } else {
    const float dd = sdf - 1.0f;
    g_d += gsig * keep * (1.0f / (1.0f + __expf(-dd)));
  }
  if constexpr (ATT) {
    const size_t giM = (size_t)S.scene * k.P + (pv ? T.ptM : 0);
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) { int row = 4 * g + r; m = (row >= 1 && row <= A) ? fmaxf(m, o[r]) : m; }
    m = max_xor32(max_xor16(m));
    const f32x4* vf = reinterpret_cast<const f32x4*>(P.vf) + g * 4;
    float pe[4], gp[4], se = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int row = 4 * g + r;
      bool rv = (row >= 1) && (row <= A);
      pe[r] = rv ? __builtin_amdgcn_exp2f(o[r] - m) : 0.0f;
      se += pe[r];
      f32x4 v = vf[r];
      gp[r] = (grgb[0] * v.x + grgb[1] * v.y) + grgb[2] * v.z;
      if (rv && pv && k.g_sem) gp[r] += k.g_sem[giM * A + (row - 1)];
    }
    se = sum_xor32(sum_xor16(se));
    const float inv = 1.0f / se;
    float dot = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { pe[r] *= inv; dot += pe[r] * gp[r]; }
    dot = sum_xor32(sum_xor16(dot));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      go[r] = pe[r] * (gp[r] - dot);                      // d/d(feature), natural units
    }
    if (!k.points_only) {
      // dV[row][c] += sum_pt p[row][pt] g_rgb[c][pt] on the matrix pipe: P_T [pt][row] and the tile's g_rgb [pt][4]
      // go through the (free at this point) scratch rows
      wave_lds_fence();
      *reinterpret_cast<f32x4*>(rows + j * 20 + 4 * g) = f32x4{pe[0], pe[1], pe[2], pe[3]};
      if (g == 0) *reinterpret_cast<f32x4*>(rows + 320 + j * 4) = f32x4{grgb[0], grgb[1], grgb[2], 0.0f};
      wave_lds_fence();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int pt = 4 * ks + g;
        const float a_p = rows[pt * 20 + j];
        const float b_g = rows[320 + pt * 4 + (j & 3)];
        dVacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a_p, (j < 4) ? b_g : 0.0f, dVacc, 0, 0, 0);
      }
      wave_lds_fence();
    }
  } else {
    // rgb = 2.004 sigmoid(f) - 1.002 ; rows 1..3 live in group 0
    if (g == 0) {
      const float f3[3] = {o.y, o.z, o.w};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float sgm = 1.0f / (1.0f + __builtin_amdgcn_exp2f(-f3[c]));
        go[1 + c] = grgb[c] * 2.004f * sgm * (1.0f - sgm);
      }
    }
  }
  if (g == 0) go[0] = g_d;
  return go;
}

// what a decoder back end hands the shell for one tile: gf^T = W1^T gh^T (rows = channels, accumulator layout == feature
// layout M), in units of gf_inv (a power of two; 1 with fp32 MFMAs)
struct FeatureGrad { f32x4 gf0, gf1; float gf_inv; };

// ---- step: M -> L rows through LDS, pre-divided by 3 (mean of the three planes) ----
__device__ __forceinline__ void rows_to_load_layout(float* rows, const FeatureGrad& gf, const BwdLane& L) {
  wave_lds_fence();
  {
    const float third = (1.0f / 3.0f) * gf.gf_inv;
    f32x4* wr = reinterpret_cast<f32x4*>(rows + L.j * 36 + 4 * L.g);
    wr[0] = gf.gf0 * third;
    wr[4] = gf.gf1 * third;
  }
  wave_lds_fence();
}

// ---- step: gf_out rows plus flags ----
// hand the tile's feature-gradient rows to the follow-up kernels: the 16 rows are 2 KB of consecutive workspace,
// written as two 16-byte stores per lane (8 lanes = one row); the binned scatter also gets a flag per point: rows
// that are exactly zero (outside the cube, zero upstream) drop out
__device__ __forceinline__ void store_gf_rows(const FieldBwdParams& k, const BwdScene& S, const ChunkPoints& C, int t, const float* rows,
                                              int lane) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int pt = 8 * h + (lane >> 3), c4 = lane & 7;
    const int64_t pidx = C.chunk * 64 + 16 * t + pt;
    const f32x4 gv = *reinterpret_cast<const f32x4*>(rows + pt * 36 + 4 * c4);
    const uint64_t nzb = __ballot(gv.x != 0.0f || gv.y != 0.0f || gv.z != 0.0f || gv.w != 0.0f);
    if (pidx < k.P) {
      const uint32_t pu = (uint32_t)pidx;
      *reinterpret_cast<f32x4*>(S.gfout + (pu * (uint32_t)kC + 4u * (uint32_t)c4)) = gv;
      if (S.flag && c4 == 0) S.flag[pu] = ((nzb >> (lane & 56)) & 0xFFull) ? 1 : 0;
    }
  }
}

// ---- step: per-point atomic scatter of the plane gradient: one instruction = the two x-adjacent corners of one point ----
// (64 consecutive floats = 2 full 128-B lines per wave instruction; the atomic units retire per
//  line touched, so this is 8x cheaper than scattering in the quad load layout - tools/probes/atomic_scatter.hip)
__device__ __forceinline__ void scatter_tile_atomics(const FieldParams& P, const BwdScene& S, const ChunkPoints& C, int t, const float* rows,
                                                     int lane) {
  const int lc = lane & 31, lh = lane >> 5;
#pragma unroll 1
  for (int pt = 0; pt < 16; ++pt) {
    const int src = 16 * t + pt;
    const int fl = __builtin_amdgcn_readlane(C.flags, src);
    if (!(fl & 2)) continue;
    const float gv = rows[pt * 36 + lc];
    if (__ballot(gv != 0.0f) == 0) continue;
    const uint32_t pxi = (uint32_t)__builtin_amdgcn_readlane(C.xi, src);
    const float pfx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, C.fx), src));
    const float pfy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, C.fy), src));
    const float pfz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, C.fz), src));
    const uint32_t px0 = pxi & 1023u, py0 = (pxi >> 10) & 1023u, pz0 = (pxi >> 20) & 1023u;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      const uint32_t a0 = (pl == 2) ? py0 : px0, b0 = (pl == 0) ? py0 : pz0;
      const float fa = (pl == 2) ? pfy : pfx, fb = (pl == 0) ? pfy : pfz;
      const float wa = lh ? fa : 1.0f - fa;
      float* base = S.gtex + (size_t)pl * S.g_plane + ((size_t)b0 * P.res + a0 + lh) * S.g_pix + lc;
      const float v0 = (wa * (1.0f - fb)) * gv, v1 = (wa * fb) * gv;
      if (v0 != 0.0f) unsafeAtomicAdd(base, v0);
      if (v1 != 0.0f) unsafeAtomicAdd(base + S.g_row, v1);
    }
  }
}

// ---- step: coordinate gradients in the load layout: d/d(unnormalised u_x, u_y, u_z) ----
struct CoordGrad { float x, y, z; };

template <int TEX>
__device__ __forceinline__ CoordGrad coord_gradients(const FieldParams& P, const BwdTile& T, const BwdLane& L, const float* rows) {
  constexpr int kColA = FeatCols<TEX>::kColA, kColB = FeatCols<TEX>::kColB;
  const int lq = L.lq;
  const uint32_t cxi = T.cxi;
  const float cfx = T.cfx, cfy = T.cfy, cfz = T.cfz;
  const bool ptv = (T.flL & 2) != 0;
  float gcoord[3] = {0.0f, 0.0f, 0.0f};
  float gfL[8];
  {
    const f32x4* rd = reinterpret_cast<const f32x4*>(rows + L.lp * 36 + lq * kColA);
    const f32x4 lo = rd[0], hi = rd[kColB / 4];
    gfL[0] = lo.x; gfL[1] = lo.y; gfL[2] = lo.z; gfL[3] = lo.w;
    gfL[4] = hi.x; gfL[5] = hi.y; gfL[6] = hi.z; gfL[7] = hi.w;
  }
  bool any = false;
#pragma unroll
  for (int s = 0; s < 8; ++s) any = any || (gfL[s] != 0.0f);
  if (__ballot(any && ptv)) {
    // second gather, ONE PLANE AT A TIME: the lines are L1/L2-hot (this wave loaded them for the forward
    // recompute), and 32 texel registers instead of 96 keep the kernel's register peak - which is here, with all
    // the weight-gradient accumulators live - under the 256 of two waves per SIMD without spilling
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      const uint32_t x0 = cxi & 1023u, y0 = (cxi >> 10) & 1023u, z0 = (cxi >> 20) & 1023u;
      const uint32_t a0 = (pl == 2) ? y0 : x0, b0 = (pl == 0) ? y0 : z0;
      const uint32_t voff = (uint32_t)pl * P.plane_bytes + __umul24(b0 * (uint32_t)P.res + a0, P.pix_bytes) + (uint32_t)lq * 16u;
      float tv[4][8];
      load_texel8<TEX>(P, voff, 0, 0, tv[0]);
      load_texel8<TEX>(P, voff, P.pix_bytes, 0, tv[1]);
      load_texel8<TEX>(P, voff, P.row_bytes, 0, tv[2]);
      load_texel8<TEX>(P, voff, P.row_pix_bytes, 0, tv[3]);
      const float fa = (pl == 2) ? cfy : cfx, fb = (pl == 0) ? cfy : cfz;
      const float ga = 1.0f - fa, gb = 1.0f - fb;
      float dcorner[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float acc = 0.0f;
#pragma unroll
        for (int s = 0; s < 8; ++s) acc = fmaf(gfL[s], tv[c][s], acc);
        // sum over the 4 lanes (channel chunks) of the point: one DPP quad
        acc += dpp_f32<kDppQuadXor1>(0.0f, acc);
        acc += dpp_f32<kDppQuadXor2>(0.0f, acc);
        dcorner[c] = acc;
      }
      const float g_fa = gb * (dcorner[1] - dcorner[0]) + fb * (dcorner[3] - dcorner[2]);
      const float g_fb = ga * (dcorner[2] - dcorner[0]) + fa * (dcorner[3] - dcorner[1]);
      // plane 0: (x,y)  plane 1: (x,z)  plane 2: (y,z)
      gcoord[(pl == 2) ? 1 : 0] += g_fa;
      gcoord[(pl == 0) ? 1 : 2] += g_fb;
      __builtin_amdgcn_sched_barrier(0);       // keep the planes' loads from being hoisted together again
    }
  }
  return CoordGrad{gcoord[0], gcoord[1], gcoord[2]};
}

// ---- step: g_points store (one lane per point; border clamp, scale to scene units, optional F.normalize) ----
__device__ __forceinline__ void store_g_points(const FieldBwdParams& k, const FieldParams& P, const BwdScene& S, const ChunkPoints& C,
                                               const BwdTile& T, const CoordGrad& gc) {
  const int flL = T.flL;
  const int64_t ptL = C.chunk * 64 + T.srcL;
  const float sc = (P.res_m1 * 0.5f) / k.scene_range;
  float* gp = k.g_points + ((size_t)S.scene * k.P + ptL) * 3;
  float gx = ((flL >> 2) & 1) ? gc.x * sc : 0.0f;
  float gy = ((flL >> 3) & 1) ? gc.y * sc : 0.0f;
  float gz = ((flL >> 4) & 1) ? gc.z * sc : 0.0f;
  if (k.normalize_points) {
    const float nrm = fmaxf(norm3(gx, gy, gz), 1e-12f);     // F.normalize(x_grad, dim=-1)
    gx /= nrm; gy /= nrm; gz /= nrm;
  }
  gp[0] = gx; gp[1] = gy; gp[2] = gz;
}

// What the two decoder back ends hold and do alike: the first layer's weight gradient, the sums that come out of staged LDS
// tiles instead of 32 cross-lane reductions per tile (db1p of lane l = hidden unit l: the column sum of GH_T; dVacc: a
// 16 x 16 MFMA accumulator whose columns 0..2 are the epilogue's dV and whose column 3 is the LAST layer's bias gradient
// sum_pt g_o[row] - the weight-gradient MFMAs' A operand against an indicator column), and the block's LDS.
struct DecoderBwdCommon {
  f32x4 dW1[4][2];
  float db1p;
  f32x4 dVacc;
  float* lds;                        // forward operand image + attention values
  float* ldb;                        // backward operand image
  float* st;                         // this wave's staging

  __device__ __forceinline__ DecoderBwdCommon(float* lds_, float* ldb_, float* st_)
      : db1p(0.0f), dVacc{0.0f, 0.0f, 0.0f, 0.0f}, lds(lds_), ldb(ldb_), st(st_) {
#pragma unroll
    for (int a = 0; a < 4; ++a) { dW1[a][0] = f32x4{0, 0, 0, 0}; dW1[a][1] = f32x4{0, 0, 0, 0}; }
  }
  __device__ __forceinline__ void stage_forward_image(const FieldBwdParams& k, int scene, int fwd_img) {
    stage_field_lds(lds, k.image, k.att ? k.att + (size_t)scene * k.A * 3 : nullptr, k.A, fwd_img);
  }
  __device__ __forceinline__ void stage_backward_image(const FieldBwdParams& k, int bwd_img) {
    for (int i = threadIdx.x; i < bwd_img; i += blockDim.x) ldb[i] = k.image_bwd[i];
    __syncthreads();
  }
};

// ================================================================================================
// The plain decoder's back end: every contraction on the 16-bit matrix pipe with split-fp16 (hi + lo) operands.
//
// Weight gradients: dW[m][n] = sum_pt A[m][pt] B[n][pt] has the POINT index on K.  The f32-input MFMA that did this (48
// per tile) runs at the fp32 vector rate on gfx950 and blocks the VALU while it does (tools/probes/mfma_valu_overlap.hip):
// 1.5 k of the 7.6 k cycles of a tile.  Now: every operand as fp16 hi + lo in point-major LDS tiles [pt][unit], read back
// through ds_read_b64_tr_b16 (a 16-lane group's 16 x 8-byte rows come back transposed: lane c gets, as element i, element
// c & 3 of the row addressed by lane 4 i + (c >> 2) - tools/probes/tr_read.hip), with the two halves of the K = 32 slots of
// v_mfma_f32_16x16x32_f16 holding the SAME 16 points: A' = [A_hi | A_lo] against [B_hi ; B_hi] and [B_lo ; B_lo] gives
// (A_hi + A_lo)(B_hi + B_lo) in two MFMAs per 16 x 16 output tile (16 cycles each instead of 4 x 32).
// Gradient operands have no natural scale, and a weight gradient is a sum over points of very different magnitude: the
// A side is scaled by a power of two S per accumulator set (sticky: it changes - and the accumulators are rescaled,
// exactly - only when a tile's largest entry times S leaves [2^-2, 2^14)), so that every entry is resolved to 2^-22 of
// its TILE's largest entry whatever the loss scale; the accumulators are in units of 1/S until the flush.
// ================================================================================================
struct PlainDecoderBwd : DecoderBwdCommon {
  // operand images in LDS (floats): forward image + attention values, its staged part, the backward image
  static constexpr int kFwd = kBwdFwdFloats, kFwdImg = kLdsImageFloats, kBwdImg = kBwdImageFloats;
  static constexpr int kWorkgroupsPerCU = 2;
  // ---- per-wave LDS: kWaveFloats floats, two regions ----
  //   R0 [0, 768 floats): F_T fp32 [16][36] of the load -> MFMA layout change, then, over it, the fp16 feature tiles
  //   R1 [768, 3072 floats), one phase at a time: the epilogue's colour-table scratch (1 536 B) with the fp16 g_o tiles
  //      behind it and the fp16 activation tiles from 4 608 B on (written by the forward recompute, read by phase A);
  //      then the fp16 gh tiles and GH_T fp32 [16][68] (phase B); then the feature-gradient rows [16][36] of the hand-off
  static constexpr int kWaveFloats = 3072;
  static constexpr int kF = 0, kRows = 768;                                        // floats
  static constexpr int kPitchF = 96, kPitchH = 144, kPitchO = 32;                  // bytes: row pitch of the [pt][32] / [pt][64] / [pt][16] fp16 tiles
  static constexpr int kF16Hi = 0, kF16Lo = 16 * kPitchF;                          // bytes, R0: 3 072 B
  static constexpr int kGH16Hi = kRows * 4, kGH16Lo = kGH16Hi + 16 * kPitchH;      // bytes, phase B
  static constexpr int kGHT = (kGH16Lo + 16 * kPitchH) / 4;                        // floats, phase B: GH_T fp32 [16][68]
  static constexpr int kGO16Hi = kRows * 4 + 1536, kGO16Lo = kGO16Hi + 16 * kPitchO;   // bytes, phase A
  static constexpr int kS16Hi = kRows * 4 + 4608, kS16Lo = kS16Hi + 16 * kPitchH;      // bytes, phase A
  static_assert(kF16Lo + 16 * kPitchF <= kRows * 4 && kF + 16 * 36 <= kRows, "plain decoder backward: R0 of the per-wave LDS");
  static_assert(kGO16Lo + 16 * kPitchO <= kS16Hi && (320 + 64) * 4 <= 1536, "plain decoder backward: phase A tiles overlap");
  static_assert(kGHT + 16 * 68 <= kWaveFloats && kS16Lo + 16 * kPitchH <= kWaveFloats * 4, "plain decoder backward: per-wave LDS");

  // ---- accumulators over all tiles of the wave (natural units; gains and base-2 factors applied at the flush) ----
  f32x4 dW2[4];
  // biased exponents of the sticky power-of-two scales of dW2 / column 3 of dVacc and of dW1 (0: not set yet), and of the
  // largest tile maximum each set has seen
  int es_go, es_gh, et_max_go, et_max_gh;

  struct Fwd { f32x4 sp[4]; f32x4 o; };    // softplus in base 2 (accumulator layout) and the output rows

  __device__ __forceinline__ PlainDecoderBwd(float* lds_, float* ldb_, float* st_)
      : DecoderBwdCommon(lds_, ldb_, st_), es_go(0), es_gh(0), et_max_go(0), et_max_gh(0) {
#pragma unroll
    for (int a = 0; a < 4; ++a) dW2[a] = f32x4{0, 0, 0, 0};
  }

  // the block's operand images of the scene (all threads; ends with a barrier)
  __device__ __forceinline__ void enter_scene(const FieldBwdParams& k, int scene) {
    stage_forward_image(k, scene, kFwdImg);
    // the forward recompute runs on the split-fp16 fragments (they overlay the fp32 ones, biases stay)
    __syncthreads();
    for (int i = threadIdx.x; i < kB1F; i += blockDim.x) lds[i] = k.image[kW1H + i];
    stage_backward_image(k, kBwdImg);
  }

  // forward recompute: feature tile (M layout) -> sp, o; leaves the fp16 feature and activation tiles for phases B and A
  // (the tile's point data is the other back end's need: it looks up the ray of every point)
  template <int TEX>
  __device__ __forceinline__ Fwd forward(const FieldBwdParams& k, const BwdTile&, const BwdLane& L, const float (&feat)[8]) {
    constexpr int kColA = FeatCols<TEX>::kColA, kColB = FeatCols<TEX>::kColB;
    typedef unsigned long long u64;
    typedef u64 u64x2 __attribute__((ext_vector_type(2)));
    const int lane = L.lane, j = L.j, g = L.g;
    const f32x4* ldsv = reinterpret_cast<const f32x4*>(lds);
    const u32x4* ldsu = reinterpret_cast<const u32x4*>(lds);
    Fwd f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) f.sp[nt] = ldsv[(kB1F >> 2) + g * 4 + nt];
    // split-fp16 operands (hi + lo, 22 significand bits), fp32 accumulation - as the renderer's tile_mlp<PREC = 1>:
    // the f32-input MFMA runs at the fp32 VECTOR rate and two waves share the SIMD's matrix pipe, which made the
    // 144 fp32 MFMAs of a tile half of this kernel's time
    f16x8 fh, fl;
    split_f16x8(feat, fh, fl);
    if (!k.points_only) {
      // the feature tile in fp16 hi / lo, point-major, over the fp32 tile it was just read from (R0): B operand of dW1
      wave_lds_fence();
      char* f16 = reinterpret_cast<char*>(st) + j * kPitchF + 2 * kColA * g;
      const u64x2 h2 = __builtin_bit_cast(u64x2, fh), l2 = __builtin_bit_cast(u64x2, fl);
      *reinterpret_cast<u64*>(f16 + kF16Hi) = h2[0]; *reinterpret_cast<u64*>(f16 + kF16Hi + 2 * kColB) = h2[1];
      *reinterpret_cast<u64*>(f16 + kF16Lo) = l2[0]; *reinterpret_cast<u64*>(f16 + kF16Lo + 2 * kColB) = l2[1];
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const f16x8 wh = __builtin_bit_cast(f16x8, ldsu[(kW1H_lds >> 2) + (nt * 2 + 0) * 64 + lane]);
      const f16x8 wl = __builtin_bit_cast(f16x8, ldsu[(kW1H_lds >> 2) + (nt * 2 + 1) * 64 + lane]);
      f.sp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, fh, f.sp[nt], 0, 0, 0);
      f.sp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, fl, f.sp[nt], 0, 0, 0);
      f.sp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, fh, f.sp[nt], 0, 0, 0);
    }
    softplus2_tile(f.sp);
    f.o = ldsv[(kB2F >> 2) + g];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const f16x8 wh = __builtin_bit_cast(f16x8, ldsu[(kW2H_lds >> 2) + (kk * 2 + 0) * 64 + lane]);
      const f16x8 wl = __builtin_bit_cast(f16x8, ldsu[(kW2H_lds >> 2) + (kk * 2 + 1) * 64 + lane]);
      const float x8[8] = {f.sp[2 * kk][0], f.sp[2 * kk][1], f.sp[2 * kk][2], f.sp[2 * kk][3],
                           f.sp[2 * kk + 1][0], f.sp[2 * kk + 1][1], f.sp[2 * kk + 1][2], f.sp[2 * kk + 1][3]};
      f16x8 sh, sl;
      split_f16x8(x8, sh, sl);
      if (!k.points_only) {
        // the activations' fp16 halves are the B operand of dW2 (phase A): hidden units {32 kk + 4 g + r, 32 kk + 16 + 4 g + r}
        if (kk == 0) wave_lds_fence();
        const u64x2 h2 = __builtin_bit_cast(u64x2, sh), l2 = __builtin_bit_cast(u64x2, sl);
        char* s16 = reinterpret_cast<char*>(st) + j * kPitchH + 2 * (32 * kk + 4 * g);
        *reinterpret_cast<u64*>(s16 + kS16Hi) = h2[0]; *reinterpret_cast<u64*>(s16 + kS16Hi + 32) = h2[1];
        *reinterpret_cast<u64*>(s16 + kS16Lo) = l2[0]; *reinterpret_cast<u64*>(s16 + kS16Lo + 32) = l2[1];
      }
      f.o = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, sh, f.o, 0, 0, 0);
      f.o = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, sl, f.o, 0, 0, 0);
      f.o = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, sh, f.o, 0, 0, 0);
    }
    return f;
  }

  // backward: g_o -> gh = (W2^T g_o^T) * sigmoid(h) -> gf^T = W1^T gh^T, with dW2 / the bias column (phase A) and dW1 / db1
  // (phase B) accumulated on the way
  __device__ __forceinline__ FeatureGrad backward(const FieldBwdParams& k, const BwdLane& L, const f32x4& go, const Fwd& f) {
    typedef unsigned long long u64;
    typedef u64 u64x2 __attribute__((ext_vector_type(2)));
    const int lane = L.lane, j = L.j, g = L.g;
    // lane (g, j) addresses row 8 (g & 1) + (j >> 2) [+ 4 for the second read], columns 4 (j & 3) .. + 3 of a tile and
    // receives points 8 (g & 1) .. + 7 of column j; lanes g >= 2 (K slots 16 .. 31) take the A side from the lo tile
    const int rowb = 8 * (g & 1) + (j >> 2), colb = 8 * (j & 3), a_lo = g >> 1;
    const char* wb = reinterpret_cast<const char*>(st);
    // ---------------- gs^T = W2^T g_o^T ; gh = gs * sigmoid(h) ----------------
    // The split-fp16 operands resolve 2^-24 absolute (split_f16x8), and an upstream gradient has no natural scale
    // (a mean-squared-error loss over 10^4 pixels hands down 1e-6): every point's column is scaled by a power of
    // two into [1, 2) before the split and the fp32 accumulator is scaled back - exact, and the result then carries
    // fp32-like precision relative to the column's largest entry whatever the loss scale.
    f16x8 go_h, go_l;
    float go_inv = 1.0f, am_go = 0.0f;
    {
      float am = fmaxf(fmaxf(fabsf(go[0]), fabsf(go[1])), fmaxf(fabsf(go[2]), fabsf(go[3])));
      am = max_xor32(max_xor16(am));                       // over the 16 rows of point j
      am_go = am;
      float sc;
      pow2_normaliser(am, sc, go_inv);
      const float x8[8] = {go[0] * sc, go[1] * sc, go[2] * sc, go[3] * sc, 0.0f, 0.0f, 0.0f, 0.0f};
      split_f16x8(x8, go_h, go_l);
    }
    if (!k.points_only) {
      // ---------------- phase A: dW2[row][hid] += sum_pt g_o[row][pt] s[hid][pt] ; column 3 of dVacc += sum_pt g_o[row][pt] ----------------
      {
        const float fac = sticky_scale(am_go, es_go, et_max_go);
        if (fac != 1.0f) {
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) dW2[nt] *= fac;
          dVacc *= (j == 3) ? fac : 1.0f;
        }
      }
      {
        typedef _Float16 f16x4v __attribute__((ext_vector_type(4)));
        const uint32_t r_go = ratio_f16x2(es_go, go_inv);
        const f16x4v rr = __builtin_bit_cast(f16x4v, (__attribute__((ext_vector_type(2))) uint32_t){r_go, r_go});
        const f16x4v gh4 = __builtin_shufflevector(go_h, go_h, 0, 1, 2, 3) * rr, gl4 = __builtin_shufflevector(go_l, go_l, 0, 1, 2, 3) * rr;
        char* t16 = reinterpret_cast<char*>(st) + j * kPitchO + 8 * g;                 // rows 4 g + r of point j
        *reinterpret_cast<u64*>(t16 + kGO16Hi) = __builtin_bit_cast(u64, gh4);
        *reinterpret_cast<u64*>(t16 + kGO16Lo) = __builtin_bit_cast(u64, gl4);
      }
      wave_lds_fence();
      {
        const f16x8 a = lds_read_tr16x2(wb + (a_lo ? kGO16Lo : kGO16Hi) + rowb * kPitchO + colb, 4 * kPitchO);
        const _Float16 one = (j == 3) ? (_Float16)1.0f : (_Float16)0.0f;
        const f16x8 ind = {one, one, one, one, one, one, one, one};
        dVacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, ind, dVacc, 0, 0, 0);       // (g_o hi + g_o lo) . 1
        const char* ps = wb + rowb * kPitchH + colb;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const f16x8 bh = lds_read_tr16x2(ps + kS16Hi + 32 * nt, 4 * kPitchH);
          const f16x8 bl = lds_read_tr16x2(ps + kS16Lo + 32 * nt, 4 * kPitchH);
          dW2[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bh, dW2[nt], 0, 0, 0);
          dW2[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bl, dW2[nt], 0, 0, 0);
        }
      }
    }
    f32x4 gh[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      // K = the 16 output rows, in the low half of the K = 32 slots (see decoder_pack_bwd_kernel)
      const u32x4* wq = reinterpret_cast<const u32x4*>(ldb + kBwdW2T);
      const f16x8 wh = __builtin_bit_cast(f16x8, wq[(mt * 2 + 0) * 64 + lane]);
      const f16x8 wl = __builtin_bit_cast(f16x8, wq[(mt * 2 + 1) * 64 + lane]);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, go_h, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, go_l, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, go_h, acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sig = 1.0f - __builtin_amdgcn_exp2f(-f.sp[mt][r]);   // sigmoid(h) = 1 - exp(-softplus(h))
        gh[mt][r] = (acc[r] * go_inv) * sig;
      }
    }

    // ---------------- gf^T = W1^T gh^T  (rows = channels, accumulator layout == feature layout M) ----------------
    FeatureGrad out{{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}, 1.0f};
    const u32x4* ldbu = reinterpret_cast<const u32x4*>(ldb + kBwdW1T);
    float am = 0.0f, sc;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) am = fmaxf(am, fabsf(gh[mt][r]));
    am = max_xor32(max_xor16(am));                       // over the 64 hidden units of point j
    pow2_normaliser(am, sc, out.gf_inv);
    uint32_t r_gh = 0u;
    if (!k.points_only) {
      // phase B staging (R1 is free: the colour-table MFMAs are done): GH_T fp32 for the bias column sums, and below
      // the tile-scaled fp16 halves of gh as the A operand of dW1
      const float fac = sticky_scale(am, es_gh, et_max_gh);
      if (fac != 1.0f) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) { dW1[nt][0] *= fac; dW1[nt][1] *= fac; }
      }
      r_gh = ratio_f16x2(es_gh, out.gf_inv);
      wave_lds_fence();
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) *reinterpret_cast<f32x4*>(st + kGHT + j * 68 + 16 * nt + 4 * g) = gh[nt];
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const float x8[8] = {gh[2 * kk][0] * sc, gh[2 * kk][1] * sc, gh[2 * kk][2] * sc, gh[2 * kk][3] * sc,
                           gh[2 * kk + 1][0] * sc, gh[2 * kk + 1][1] * sc, gh[2 * kk + 1][2] * sc, gh[2 * kk + 1][3] * sc};
      f16x8 xh, xl;
      split_f16x8(x8, xh, xl);
      if (!k.points_only) {
        // hidden units {32 kk + 4 g + r, 32 kk + 16 + 4 g + r} of point j
        const f16x8 rr = __builtin_bit_cast(f16x8, u32x4{r_gh, r_gh, r_gh, r_gh});
        const u64x2 h2 = __builtin_bit_cast(u64x2, xh * rr), l2 = __builtin_bit_cast(u64x2, xl * rr);
        char* t16 = reinterpret_cast<char*>(st) + j * kPitchH + 2 * (32 * kk + 4 * g);
        *reinterpret_cast<u64*>(t16 + kGH16Hi) = h2[0]; *reinterpret_cast<u64*>(t16 + kGH16Hi + 32) = h2[1];
        *reinterpret_cast<u64*>(t16 + kGH16Lo) = l2[0]; *reinterpret_cast<u64*>(t16 + kGH16Lo + 32) = l2[1];
      }
      const f16x8 ah = __builtin_bit_cast(f16x8, ldbu[((0 * 2 + kk) * 2 + 0) * 64 + lane]);
      const f16x8 al = __builtin_bit_cast(f16x8, ldbu[((0 * 2 + kk) * 2 + 1) * 64 + lane]);
      const f16x8 bh = __builtin_bit_cast(f16x8, ldbu[((1 * 2 + kk) * 2 + 0) * 64 + lane]);
      const f16x8 bl = __builtin_bit_cast(f16x8, ldbu[((1 * 2 + kk) * 2 + 1) * 64 + lane]);
      out.gf0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, xh, out.gf0, 0, 0, 0);
      out.gf1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, xh, out.gf1, 0, 0, 0);
      out.gf0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, xl, out.gf0, 0, 0, 0);
      out.gf1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, xl, out.gf1, 0, 0, 0);
      out.gf0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, xh, out.gf0, 0, 0, 0);
      out.gf1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl, xh, out.gf1, 0, 0, 0);
    }
    if (!k.points_only) {
      // ---------------- phase B: db1 += column sums of GH_T ; dW1[hid][ch] += sum_pt gh[hid][pt] f[ch][pt] ----------------
      wave_lds_fence();
      {
        float cs = 0.0f;
#pragma unroll
        for (int pt = 0; pt < 16; ++pt) cs += st[kGHT + pt * 68 + lane];
        db1p += cs;
      }
      {
        const char* pf = wb + rowb * kPitchF + colb;
        f16x8 bfh[2], bfl[2];
#pragma unroll
        for (int n2 = 0; n2 < 2; ++n2) {
          bfh[n2] = lds_read_tr16x2(pf + kF16Hi + 32 * n2, 4 * kPitchF);
          bfl[n2] = lds_read_tr16x2(pf + kF16Lo + 32 * n2, 4 * kPitchF);
        }
        const char* pa = wb + (a_lo ? kGH16Lo : kGH16Hi) + rowb * kPitchH + colb;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const f16x8 a = lds_read_tr16x2(pa + 32 * nt, 4 * kPitchH);
#pragma unroll
          for (int n2 = 0; n2 < 2; ++n2) {
            dW1[nt][n2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bfh[n2], dW1[nt][n2], 0, 0, 0);
            dW1[nt][n2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bfl[n2], dW1[nt][n2], 0, 0, 0);
          }
        }
      }
    }
    return out;
  }

  // flush: g_w1, g_w2, g_b1, g_b2 (the accumulators are in units of 1 / their sticky scale)
  // (slot: this wave's offset in floats into the per-wave slots of the ordered mode; 0 otherwise)
  __device__ __forceinline__ void flush(const FieldBwdParams& k, const BwdLane& L, uint32_t slot) {
    const int lane = L.lane, j = L.j, g = L.g;
    const int n_out = k.A > 0 ? 1 + k.A : 4;
    const float g1 = 0.17677669529663687f, g2 = 0.125f;
    const float un_gh = (es_gh == 0) ? 1.0f : bits2f((uint32_t)(254 - es_gh) << 23);
    const float un_go = (es_go == 0) ? 1.0f : bits2f((uint32_t)(254 - es_go) << 23);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // dW1[hid = 16nt+4g+r][ch = 16*n2 + j] ; feat was the SUM of three planes -> /3
        atomicAdd(&k.g_w1[slot + (16 * nt + 4 * g + r) * kC + j], dW1[nt][0][r] * (g1 / 3.0f) * un_gh);
        atomicAdd(&k.g_w1[slot + (16 * nt + 4 * g + r) * kC + 16 + j], dW1[nt][1][r] * (g1 / 3.0f) * un_gh);
        // dW2[row = 4g+r][hid = 16nt + j] ; s = sp2 * ln2
        const int row = 4 * g + r;
        if (row < n_out) atomicAdd(&k.g_w2[slot + row * kHidden + 16 * nt + j], dW2[nt][r] * (g2 * kLn2) * un_go);
      }
    }
    atomicAdd(&k.g_b1[slot + lane], db1p);                                   // one hidden unit per lane (see db1p above)
    if (j == 3) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;                                    // column 3 of dVacc: the bias gradient of the row
        if (row < n_out) atomicAdd(&k.g_b2[slot + row], dVacc[r] * un_go);
      }
    }
  }
};

// ================================================================================================
// The view-direction decoder's back end: three layers (hidden 64 -> 33 second-layer rows + the per-ray feature ->
// leaky_relu -> the mapper's `output` Linear(32, n3)), every contraction on v_mfma_f32_16x16x4_f32:
//
//   gy^T [48x16] = W3'^T [48x16] g_o^T [16x16]     12 MFMA   (operands in accumulator layout)
//   gs^T [64x16] = W2^T  [64x48] g_o2^T [48x16]    48 MFMA
//   gf^T [32x16] = W1^T  [32x64] gh^T  [64x16]     32 MFMA
//   dW3 / dW2 / dW1 / bias columns: points along K, operands staged in LDS as fp32 tiles [pt][unit]
// ================================================================================================
struct ViewdirDecoderBwd : DecoderBwdCommon {
  static constexpr int kFwd = kVdFieldLdsFloats, kFwdImg = kVdImageFloats, kBwdImg = kVbImageFloats;
  static constexpr int kWorkgroupsPerCU = 1;         // 512 VGPRs per lane: the accumulators of three layers
  // ---- per-wave LDS (floats): F_T [16][36], GO_T [16][20], S_T [16][68], GH_T [16][68], Y_T [16][52] (third-layer
  // input), GO2_T [16][52] (second-layer output gradient).  S_T is free outside the staging block: the epilogue's
  // colour-table scratch and the feature-gradient rows [16][36] of the hand-off live there (kRows) ----
  static constexpr int kF = 0, kGO = kF + 16 * 36, kS = kGO + 16 * 20, kGH = kS + 16 * 68, kY = kGH + 16 * 68, kGO2 = kY + 16 * 52;
  static constexpr int kWaveFloats = kGO2 + 16 * 52;
  static constexpr int kRows = kS;
  static_assert(kF + 16 * 36 <= kGO && kRows + 16 * 36 <= kGH && kRows + 320 + 16 * 4 <= kGH,
                "view-direction decoder backward: the feature tile, the gradient rows and the colour-table scratch in their tiles");

  // ---- accumulators (natural units; gains applied at the flush) ----
  f32x4 dW2[3][4];                   // three 16-row tiles of the second layer's output
  f32x4 dW3[3], db2v[3];             // third-layer weights, second-layer bias
  const float* xray_scene;           // the scene's per-ray features and their gradient (null: not wanted)
  float* gxray_scene;

  // softplus in base 2, the output rows, the second layer's pre-activations (48 rows) and the third layer's input
  struct Fwd { f32x4 sp[4]; f32x4 o; f32x4 o2[3], yv[3]; int ray_j; };

  __device__ __forceinline__ ViewdirDecoderBwd(float* lds_, float* ldb_, float* st_)
      : DecoderBwdCommon(lds_, ldb_, st_), xray_scene(nullptr), gxray_scene(nullptr) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int t2 = 0; t2 < 3; ++t2) dW2[t2][a] = f32x4{0, 0, 0, 0};
      if (a < 3) { dW3[a] = f32x4{0, 0, 0, 0}; db2v[a] = f32x4{0, 0, 0, 0}; }
    }
  }

  // the block's operand images of the scene (all threads; ends with a barrier) and the scene's ray features
  __device__ __forceinline__ void enter_scene(const FieldBwdParams& k, int scene) {
    stage_forward_image(k, scene, kFwdImg);
    stage_backward_image(k, kBwdImg);
    xray_scene = k.xray + (size_t)scene * (size_t)(k.P / k.spr) * kRayFeatPad;
    gxray_scene = k.g_xray ? k.g_xray + (size_t)scene * (size_t)(k.P / k.spr) * kRayFeatPad : nullptr;
  }

  template <int TEX>
  __device__ __forceinline__ Fwd forward(const FieldBwdParams& k, const BwdTile& T, const BwdLane& L, const float (&feat)[8]) {
    const int lane = L.lane, g = L.g;
    const f32x4* ldsv = reinterpret_cast<const f32x4*>(lds);
    Fwd f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) f.sp[nt] = ldsv[(kVdB1F >> 2) + g * 4 + nt];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      f32x4 w = ldsv[(kVdW1F >> 2) + s * 64 + lane];
      f.sp[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, feat[s], f.sp[0], 0, 0, 0);
      f.sp[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, feat[s], f.sp[1], 0, 0, 0);
      f.sp[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, feat[s], f.sp[2], 0, 0, 0);
      f.sp[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, feat[s], f.sp[3], 0, 0, 0);
    }
    softplus2_tile(f.sp);
    f.ray_j = (T.flM & 2) ? (int)(T.ptM / k.spr) : 0;
#pragma unroll
    for (int t2 = 0; t2 < 3; ++t2) f.o2[t2] = ldsv[(kVdB2 >> 2) + t2 * 4 + g];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int t2 = 0; t2 < 3; ++t2) {
        const f32x4 w = ldsv[(kVdW2 >> 2) + (t2 * 4 + nt) * 64 + lane];
        f.o2[t2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, f.sp[nt][0], f.o2[t2], 0, 0, 0);
        f.o2[t2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, f.sp[nt][1], f.o2[t2], 0, 0, 0);
        f.o2[t2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, f.sp[nt][2], f.o2[t2], 0, 0, 0);
        f.o2[t2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, f.sp[nt][3], f.o2[t2], 0, 0, 0);
      }
    f32x4 oa = ldsv[(kVdB3 >> 2) + g], ob = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t2 = 0; t2 < 3; ++t2) {
      const f32x4 xr = *reinterpret_cast<const f32x4*>(xray_scene + (size_t)f.ray_j * kRayFeatPad + 16 * t2 + 4 * g);
      const f32x4 w = ldsv[(kVdW3 >> 2) + t2 * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = f.o2[t2][r] + xr[r];
        f.yv[t2][r] = (v > 0.0f) ? v : v * 0.2f;
        f.o2[t2][r] = v;                                  // keep the pre-activation for leaky_relu'
      }
      if (t2 == 0 && g == 0) f.yv[0][0] = f.o2[0][0];          // distance row passes through (padded xr[0] == 0)
      oa = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, f.yv[t2][0], oa, 0, 0, 0);
      ob = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, f.yv[t2][1], ob, 0, 0, 0);
      oa = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, f.yv[t2][2], oa, 0, 0, 0);
      ob = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, f.yv[t2][3], ob, 0, 0, 0);
    }
    f.o = oa + ob;
    return f;
  }

  __device__ __forceinline__ FeatureGrad backward(const FieldBwdParams& k, const BwdLane& L, const f32x4& go, const Fwd& f) {
    const int lane = L.lane, j = L.j, g = L.g;
    const f32x4* ldbv = reinterpret_cast<const f32x4*>(ldb);
    // ---------------- gy^T = W3'^T g_o^T ; g_o2 = gy * leaky_relu'(x_ray + f) ----------------
    f32x4 go2[3];
#pragma unroll
    for (int t2 = 0; t2 < 3; ++t2) {
      const f32x4 w = ldbv[(kVbW3T >> 2) + t2 * 64 + lane];
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, go[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, go[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, go[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, go[3], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) go2[t2][r] = acc[r] * ((f.o2[t2][r] > 0.0f) ? 1.0f : 0.2f);
      if (t2 == 0 && g == 0) go2[0][0] = acc[0];                     // distance row: identity
      db2v[t2] += go2[t2];
    }
    // gradient of the per-ray feature: sum over the samples of the ray
    if (gxray_scene) {
      const int ray_j = f.ray_j;
      const int r0 = __builtin_amdgcn_readfirstlane(ray_j);
      const bool uniform = __all(ray_j == r0);
#pragma unroll
      for (int t2 = 0; t2 < 3; ++t2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kk = 16 * t2 + 4 * g + r;
          float v = go2[t2][r];
          if (uniform) v = row_allreduce_sum(v);
          if (kk >= 1 && kk <= 32 && v != 0.0f && (!uniform || j == 0))
            unsafeAtomicAdd(gxray_scene + (size_t)ray_j * kRayFeatPad + kk, v);
        }
    }
    // ---------------- gs^T = W2^T g_o2^T ; gh = gs * sigmoid(h) ----------------
    f32x4 gh[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int t2 = 0; t2 < 3; ++t2) {
        const f32x4 w = ldbv[(kVbW2T >> 2) + (mt * 3 + t2) * 64 + lane];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, go2[t2][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, go2[t2][1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, go2[t2][2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, go2[t2][3], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sig = 1.0f - __builtin_amdgcn_exp2f(-f.sp[mt][r]);   // sigmoid(h) = 1 - exp(-softplus(h))
        gh[mt][r] = acc[r] * sig;
      }
    }

    if (!k.points_only) {
      // ---------------- stage transposed operands: GO_T [pt][row], S_T [pt][hid], GH_T [pt][hid], Y_T, GO2_T ----------------
      wave_lds_fence();
      *reinterpret_cast<f32x4*>(st + kGO + j * 20 + 4 * g) = go;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        *reinterpret_cast<f32x4*>(st + kS + j * 68 + 16 * nt + 4 * g) = f.sp[nt];
        *reinterpret_cast<f32x4*>(st + kGH + j * 68 + 16 * nt + 4 * g) = gh[nt];
      }
#pragma unroll
      for (int t2 = 0; t2 < 3; ++t2) {
        *reinterpret_cast<f32x4*>(st + kY + j * 52 + 16 * t2 + 4 * g) = f.yv[t2];
        *reinterpret_cast<f32x4*>(st + kGO2 + j * 52 + 16 * t2 + 4 * g) = go2[t2];
      }
      wave_lds_fence();
      {
        // db1[hid = lane] += sum_pt gh[hid][pt]: the column sum of GH_T
        float cs = 0.0f;
#pragma unroll
        for (int pt = 0; pt < 16; ++pt) cs += st[kGH + pt * 68 + lane];
        db1p += cs;
      }
      // dW3[row][kk] += sum_pt g_o[row][pt] y[kk][pt] ; dW2[kk][hid] += sum_pt g_o2[kk][pt] s[hid][pt] ;
      // dW1[hid][ch] += sum_pt gh[hid][pt] f[ch][pt]
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int pt = 4 * ks + g;
        const float a_go = st[kGO + pt * 20 + j];
        dVacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a_go, (j == 3) ? 1.0f : 0.0f, dVacc, 0, 0, 0);   // column 3: sum_pt g_o[row]
        const float b_f0 = st[kF + pt * 36 + j], b_f1 = st[kF + pt * 36 + 16 + j];
#pragma unroll
        for (int t2 = 0; t2 < 3; ++t2)
          dW3[t2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_go, st[kY + pt * 52 + 16 * t2 + j], dW3[t2], 0, 0, 0);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const float b_s = st[kS + pt * 68 + 16 * nt + j];
#pragma unroll
          for (int t2 = 0; t2 < 3; ++t2)
            dW2[t2][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(st[kGO2 + pt * 52 + 16 * t2 + j], b_s, dW2[t2][nt], 0, 0, 0);
          const float a_gh = st[kGH + pt * 68 + 16 * nt + j];
          dW1[nt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_gh, b_f0, dW1[nt][0], 0, 0, 0);
          dW1[nt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_gh, b_f1, dW1[nt][1], 0, 0, 0);
        }
      }
    }

    // ---------------- gf^T = W1^T gh^T  (rows = channels, accumulator layout == feature layout M) ----------------
    FeatureGrad out{{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}, 1.0f};
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const f32x4 wa = ldbv[(kVbW1T >> 2) + (0 * 4 + nt) * 64 + lane];
      const f32x4 wb = ldbv[(kVbW1T >> 2) + (1 * 4 + nt) * 64 + lane];
      out.gf0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa.x, gh[nt][0], out.gf0, 0, 0, 0);
      out.gf1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wb.x, gh[nt][0], out.gf1, 0, 0, 0);
      out.gf0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa.y, gh[nt][1], out.gf0, 0, 0, 0);
      out.gf1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wb.y, gh[nt][1], out.gf1, 0, 0, 0);
      out.gf0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa.z, gh[nt][2], out.gf0, 0, 0, 0);
      out.gf1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wb.z, gh[nt][2], out.gf1, 0, 0, 0);
      out.gf0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa.w, gh[nt][3], out.gf0, 0, 0, 0);
      out.gf1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wb.w, gh[nt][3], out.gf1, 0, 0, 0);
    }
    return out;
  }

  // flush: g_w1, g_w2 (33 rows), g_b1, g_b2 (33 rows), g_w3, g_b3 (no ordered mode for this decoder: no slots)
  __device__ __forceinline__ void flush(const FieldBwdParams& k, const BwdLane& L, uint32_t) {
    const int lane = L.lane, j = L.j, g = L.g;
    const int n3 = k.A > 0 ? k.A : 3;
    const float g1 = 0.17677669529663687f, g2 = 0.125f;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // dW1[hid = 16nt+4g+r][ch = 16*n2 + j] ; feat was the SUM of three planes -> /3
        atomicAdd(&k.g_w1[(16 * nt + 4 * g + r) * kC + j], dW1[nt][0][r] * (g1 / 3.0f));
        atomicAdd(&k.g_w1[(16 * nt + 4 * g + r) * kC + 16 + j], dW1[nt][1][r] * (g1 / 3.0f));
        // dW2[row = 16 t2 + 4g+r][hid = 16nt + j] ; s = sp2 * ln2
        const int row = 4 * g + r;
#pragma unroll
        for (int t2 = 0; t2 < 3; ++t2)
          if (16 * t2 + row < 33) atomicAdd(&k.g_w2[(16 * t2 + row) * kHidden + 16 * nt + j], dW2[t2][nt][r] * (g2 * kLn2));
      }
    }
    atomicAdd(&k.g_b1[lane], db1p);                                   // one hidden unit per lane (see db1p above)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * g + r;
      // column 3 of dVacc: the bias gradient of the last layer = the mapper's `output` Linear(32, n3)
      if (j == 3 && row >= 1 && row <= n3) atomicAdd(&k.g_b3[row - 1], dVacc[r]);
      // dW3 = the weight gradient of the mapper's `output` layer
#pragma unroll
      for (int t2 = 0; t2 < 3; ++t2) {
        const int kk = 16 * t2 + j;
        if (row >= 1 && row <= n3 && kk >= 1 && kk <= 32) atomicAdd(&k.g_w3[(row - 1) * 32 + (kk - 1)], dW3[t2][r] * g1);
        float b2v = row_allreduce_sum(db2v[t2][r]);
        if (j == 0 && 16 * t2 + row < 33) atomicAdd(&k.g_b2[16 * t2 + row], b2v);
      }
    }
  }
};

// VD selects the back end: here and nowhere else
template <bool VD> using FieldDecoderBwd = std::conditional_t<VD, ViewdirDecoderBwd, PlainDecoderBwd>;

// TEX: texel storage of the planes (0 fp32, 1 bf16, 2 fp16).  With 16-bit storage the forward recompute gathers the
// rounded texels and the gradient image stays fp32: it is the gradient w.r.t. the rounded planes, handed to the
// producer unchanged (straight-through rounding), which is what a bf16 / fp16 plane tensor gives under autograd.
template <bool ATT, bool COORD, bool VD = false, int TEX = 0>
__global__ __launch_bounds__(256, FieldDecoderBwd<VD>::kWorkgroupsPerCU) void field_query_bwd_kernel(FieldBwdParams k) {
  using Dec = FieldDecoderBwd<VD>;
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  float* lds = dyn;                                   // forward operand image + attention values
  float* ldb = dyn + Dec::kFwd;                       // backward operand image
  const int scene = blockIdx.y;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const BwdLane L{lane, lane & 15, lane >> 4, lane >> 2, lane & 3};
  float* st = ldb + Dec::kBwdImg + wave * Dec::kWaveFloats;
  Dec dec(lds, ldb, st);
  dec.enter_scene(k, scene);
  float* rows = st + Dec::kRows;                      // scratch rows of the epilogue / the feature-gradient rows
  const char* tex_scene = reinterpret_cast<const char*>(k.texels) + (size_t)scene * 3 * k.res * k.res * (TEX == 0 ? 128 : 64);
  FieldParams P = make_field_params(tex_scene, k.res, TEX, k.A, k.use_sdf, k.beta, k.alpha, lds, Dec::kFwdImg, k.layout);
  const BwdScene S = enter_bwd_scene(k, scene);
  const float alpha_v = k.use_sdf ? k.alpha[0] : 1.0f;
  float d_beta = 0.0f, d_alpha = 0.0f;
  // ordered mode: every wave adds into its own zeroed slot (exact), param_finish_kernel sums the slots in index order
  // (worked out here, as ONE scalar: at the flush it would keep the block's coordinates alive through the whole walk)
  uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * k.slot_stride));
  uint32_t att_at = k.slot_stride ? slot : (uint32_t)(scene * k.A * 3);      // this wave's rows of g_att
  asm volatile("" : "+s"(slot), "+s"(att_at));     // (pinned here: sunk to the flush they cost five scalar registers, not two)

  ChunkWalk walk(k, wave);
  while (true) {
    const int64_t chunk = walk.next(k);
    if (chunk < 0) break;
    const ChunkPoints C = chunk_points(k, P, S, chunk, lane);
    const uint64_t nzmask = upstream_peek(k, S, C);
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
      if (((C.live >> (16 * t)) & 0xFFFFull) == 0) continue;
      const BwdTile T = tile_lanes(C, t, L);
      // does anything flow into this tile?  (the chunk-level peek; the values are loaded again where they are used - held
      // across the forward recompute they cost the registers this kernel does not have)
      if (((nzmask >> (16 * t)) & 0xFFFFull) == 0) {
        zero_tile_outputs<COORD>(k, S, C, T, L);
        continue;
      }
      float feat[8];
      gather_features<TEX>(P, T, L, st + Dec::kF, feat);
      const typename Dec::Fwd f = dec.template forward<TEX>(k, T, L, feat);
      const f32x4 go = epilogue_bwd<ATT>(k, P, S, T, L, f.o, alpha_v, rows, dec.dVacc, d_beta, d_alpha);
      const FeatureGrad gf = dec.backward(k, L, go, f);
      rows_to_load_layout(rows, gf, L);
      if (k.gf_out) store_gf_rows(k, S, C, t, rows, lane);
      if (!k.points_only && !k.bin_flag) scatter_tile_atomics(P, S, C, t, rows, lane);
      if constexpr (COORD) {
        const CoordGrad gc = coord_gradients<TEX>(P, T, L, rows);
        if (k.g_points && L.lq == 0 && (T.flL & 2)) store_g_points(k, P, S, C, T, gc);
      }
      wave_lds_fence();
    }
  }

  // ---------------- flush the per-wave accumulators ----------------
  if (k.points_only) return;
  dec.flush(k, L, slot);
  if constexpr (ATT) {
    // columns j < 3 of dVacc hold dV[row][c = j]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * L.g + r;
      if (L.j < 3 && row >= 1 && row <= k.A) atomicAdd(&k.g_att[att_at + (row - 1) * 3 + L.j], dec.dVacc[r]);
    }
  }
  if (k.use_sdf) {
    d_beta = wave_sum(d_beta); d_alpha = wave_sum(d_alpha);
    if (lane == 0) { atomicAdd(k.g_beta + slot, d_beta); atomicAdd(k.g_alpha + slot, d_alpha); }
  }
}

// ------------------------------------------------------------------------------------------------
// binned plane-gradient scatter (scatter_mode 1): a two-level counting sort of the points by texel cell per plane -
// by PLANE TILE (16 x 16 texels; 32 x 32 above 512^2 planes) through global memory, by cell inside the tile in LDS -
// followed by a register reduction over the sorted entries (one set of line-coalesced atomics per cell run).
//   count : thread = point; bucket histogram privatised in LDS (<= 3072 buckets per scene), one global add per
//           non-empty bucket and block;
//   scan  : one block per scene: bucket offsets + the list of work items (a bucket in chunks of <= kBinChunk entries);
//   fill  : same block structure as count: LDS ranks + one returning global add per non-empty bucket and block reserve
//           the slots; an entry = {point, cell in the tile | cell in the plane, fa, fb} (16 B, written once, read once, coalesced);
//   reduce: one workgroup per work item (see bin_reduce_kernel).
// Round 2, first version: counting sort by texel CELL in global memory (3 returning global atomics per point for the
// ranks): 0.59 + 0.10 + 0.10 ms for histogram + scan + fill per 4.2 M points, the coarse buckets need no global
// atomic per point: 0.03 + 0.01 + 0.05 ms (HISTORY.md, backward).
// ------------------------------------------------------------------------------------------------
constexpr int kBinChunk = 4096;            // entries per work item (the longer the chunk, the longer the cell runs)
constexpr int kBinThreads = 512;           // threads of the reduce workgroup
#ifndef NFI_BIN_DEPTH
#define NFI_BIN_DEPTH 16
#endif
// Point GROUPS (round 4): the reduce reads every point's 128-B gradient row once per plane - three times - and the rows of
// one training step (1.07 GB for 8.4 M points) are far beyond the L2s and the 256 MB Infinity Cache, so all three reads
// come from HBM (3.6 GB per step at 80 % of the achievable HBM rate, profiles/r3/pmc_bin_reduce.json).  A scene's points
// (ray order: image row bands) are therefore cut into `groups` contiguous ranges whose rows fit the Infinity Cache
// (<= kBinGroupRowBytes), the group becomes the most significant part of the bucket id, and the work items are handed out
// IN ORDER (scene, group, plane, tile) by an atomic cursor: a group's three planes are reduced back to back, the second and
// third read of a row find it in the Infinity Cache (tools/probes/mall_probe.py: 1.3-1.6x the HBM rate for a 64 MB
// re-read).  Price: a texel cell whose points span several groups is flushed once per group.
// Measured on the training step's 8.4 M points (268 MB of rows per scene; tools/probes/scatter_variants.py at commit
// "point groups", profiles/r4/scatter_point_groups.log; field backward + scatter, ms): no groups 2.648, <= 160 MB (2 groups)
// 2.648, <= 80 MB (4 groups, 16-texel tiles) 2.595, <= 40 MB (8) 2.696, <= 20 MB (16) 3.019; 8-texel tiles for the grouped
// buckets 2.693 / 2.918: the in-order hand-out is worth more (2.73-2.84 before it) than the cache window itself.
constexpr size_t kBinGroupRowBytes = (size_t)80 << 20;
constexpr int kBinDepth = NFI_BIN_DEPTH;   // gathered rows in flight per half-wave of the reduce (the walk is latency bound)
constexpr int kBinMaxBuckets = 3072;       // 3 planes x 32 x 32 tiles

struct BinParams {
  const float* points; int64_t P; int n_scenes; int res; float scene_range;
  int groups; int64_t group_pts;   // point groups per scene (see above) and points per group (a multiple of 1024)
  int bpg;                         // buckets per group = 3 * tps^2 (<= kBinMaxBuckets)
  int* next_item;                  // the reduce's work cursor
  const uint8_t* flag;       // [B,P] from the backward kernel: the point's gradient row is non-zero
  const float* gf;           // [B,P,32] feature-gradient rows
  int* count; int* cursor;   // [B][n_buckets]: entries per bucket / next free slot (scan: = bucket offset)
  int4* entries;             // [B][3P] sorted by bucket
  int4* items; int* n_items; // work items {scene, bucket, first entry, entries}
  float* g_texels;
  int layout;
  int tile; int tps; int n_buckets;   // tile side (8 / 16 / 32), tiles per plane side, groups * 3 * tps^2 buckets per scene
};

struct BinEntry { int bucket[3]; int cell[3]; float fa[3], fb[3]; };

__device__ __forceinline__ void bin_entry(const BinParams& k, int64_t i, BinEntry& e) {
  const float px = k.points[i * 3], py = k.points[i * 3 + 1], pz = k.points[i * 3 + 2];
  int c0[3];
  float f[3];
  const float rm1 = (float)(k.res - 1);
  plane_coord(px / k.scene_range, rm1, k.res, c0[0], f[0]);
  plane_coord(py / k.scene_range, rm1, k.res, c0[1], f[1]);
  plane_coord(pz / k.scene_range, rm1, k.res, c0[2], f[2]);
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    const int ax_a = (pl == 2) ? 1 : 0, ax_b = (pl == 0) ? 1 : 2;      // plane 0: (x,y)  1: (x,z)  2: (y,z)
    const int ia = c0[ax_a], ib = c0[ax_b];
    const int ta = ia / k.tile, tb = ib / k.tile;
    e.bucket[pl] = (pl * k.tps + tb) * k.tps + ta;
    // cell word: texel cell inside the tile (sort key of the reduce) | cell index in the plane (address of the flush)
    e.cell[pl] = (((ib - tb * k.tile) * k.tile + (ia - ta * k.tile)) << 20) | (ib * k.res + ia);
    e.fa[pl] = f[ax_a]; e.fb[pl] = f[ax_b];
  }
}

// grid (ceil(P / 1024), scenes): bucket counts of 1024 consecutive points, privatised in LDS
__global__ __launch_bounds__(256) void bin_count_kernel(BinParams k) {
  __shared__ int hist[kBinMaxBuckets];
  const int scene = blockIdx.y;
  for (int b = threadIdx.x; b < k.bpg; b += 256) hist[b] = 0;
  __syncthreads();
  // the block's 1024 points lie in ONE group (group_pts is a multiple of 1024): the histogram holds that group's buckets
  const size_t gbase = (size_t)scene * k.n_buckets + (size_t)(((int64_t)blockIdx.x * 1024) / k.group_pts) * k.bpg;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t p = (int64_t)blockIdx.x * 1024 + q * 256 + threadIdx.x;
    if (p < k.P && k.flag[(int64_t)scene * k.P + p]) {
      BinEntry e;
      bin_entry(k, (int64_t)scene * k.P + p, e);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) atomicAdd(&hist[e.bucket[pl]], 1);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < k.bpg; b += 256)
    if (hist[b]) atomicAdd(&k.count[gbase + b], hist[b]);
}

// one block per scene: exclusive scan of the bucket counts (-> cursor) and the work-item list
__global__ __launch_bounds__(256) void bin_scan_kernel(BinParams k) {
  __shared__ int part[256];
  __shared__ int part_it[256];
  const int scene = blockIdx.x, nb = k.n_buckets;
  const int per = (nb + 255) / 256;
  const int lo = min((int)threadIdx.x * per, nb), hi = min(lo + per, nb);
  const int* cnt = k.count + (size_t)scene * nb;
  int sum = 0, n_it = 0;
  for (int c = lo; c < hi; ++c) { sum += cnt[c]; n_it += (cnt[c] + kBinChunk - 1) / kBinChunk; }
  part[threadIdx.x] = sum;
  part_it[threadIdx.x] = n_it;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = (threadIdx.x >= off) ? part[threadIdx.x - off] : 0;
    const int w = (threadIdx.x >= off) ? part_it[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    part_it[threadIdx.x] += w;
    __syncthreads();
  }
  int run = part[threadIdx.x] - sum;
  // item order = bucket order = (scene, group, plane, tile): a group's three planes are reduced in one time window, so the
  // second and third read of a point's gradient row find it in the Infinity Cache; the items of the scenes in front of
  // this one are counted from their bucket counts (a few thousand integers)
  __shared__ int before[256];
  int mine = 0;
  for (int c = threadIdx.x; c < scene * nb; c += 256) mine += (k.count[c] + kBinChunk - 1) / kBinChunk;
  before[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) before[threadIdx.x] += before[threadIdx.x + off];
    __syncthreads();
  }
  int at = before[0] + part_it[threadIdx.x] - n_it;
  if (scene == (int)gridDim.x - 1 && threadIdx.x == 255) *k.n_items = before[0] + part_it[255];
  int* cur = k.cursor + (size_t)scene * nb;
  for (int c = lo; c < hi; ++c) {
    cur[c] = run;
    for (int o = 0; o < cnt[c]; o += kBinChunk) k.items[at++] = int4{scene, c, run + o, min(kBinChunk, cnt[c] - o)};
    run += cnt[c];
  }
}

// same blocks as the count: rank inside the block (LDS), slots reserved per bucket and block, entries written
__global__ __launch_bounds__(256) void bin_fill_kernel(BinParams k) {
  __shared__ int hist[kBinMaxBuckets];
  const int scene = blockIdx.y;
  for (int b = threadIdx.x; b < k.bpg; b += 256) hist[b] = 0;
  __syncthreads();
  const size_t gbase = (size_t)scene * k.n_buckets + (size_t)(((int64_t)blockIdx.x * 1024) / k.group_pts) * k.bpg;
  BinEntry e[4];
  int rk[4][3];
  bool on[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t p = (int64_t)blockIdx.x * 1024 + q * 256 + threadIdx.x;
    on[q] = p < k.P && k.flag[(int64_t)scene * k.P + p];
    if (on[q]) {
      bin_entry(k, (int64_t)scene * k.P + p, e[q]);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) rk[q][pl] = atomicAdd(&hist[e[q].bucket[pl]], 1);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < k.bpg; b += 256)
    if (hist[b]) hist[b] = atomicAdd(&k.cursor[gbase + b], hist[b]);     // count -> first slot
  __syncthreads();
  int4* ent = k.entries + (size_t)scene * 3 * (size_t)k.P;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (!on[q]) continue;
    const int p = (int)((int64_t)blockIdx.x * 1024 + q * 256 + threadIdx.x);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      const int64_t slot = (int64_t)hist[e[q].bucket[pl]] + rk[q][pl];
      if (slot >= 0 && slot < 3 * k.P)            // (always true when count and fill agree)
        ent[slot] = int4{p, e[q].cell[pl], __builtin_bit_cast(int, e[q].fa[pl]), __builtin_bit_cast(int, e[q].fb[pl])};
    }
  }
}

// One workgroup per work item (<= kBinChunk entries of one bucket):
//   (1) counting sort of the chunk by texel cell INSIDE LDS (one LDS integer atomic per entry);
//   (2) every half-wave (lane = channel) walks an eighth of the sorted entries - each entry is ONE broadcast LDS read,
//       one 128-B row of feature gradient (kBinDepth rows in flight) and ten VALU operations on the four corner sums
//       of the current cell, held in registers - and issues four line-coalesced global atomics when the cell changes.
// Measured in the training step (12.6 M entries per launch): 0.70 ms for the reduction over the globally sorted
// entries of the first version, 0.87 ms for the first form of this kernel (issue bound: 160 issue cycles per entry,
// v_readlane broadcasts and an integer division per flush), see HISTORY.md for the current figure.
// (An LDS copy of the tile with ds_add_f32 per entry was tried first: LDS float atomics retire about one lane per
//  cycle and CU on gfx950 - 5.2 ms.)
__global__ __launch_bounds__(kBinThreads) void bin_reduce_kernel(BinParams k) {
  __shared__ int4 sorted[kBinChunk];            // 64 KB: two workgroups of 8 waves per CU
  __shared__ int cell_at[32 * 32];
  __shared__ int wave_tot[kBinThreads / 64];
  const int n_items = *k.n_items;
  const int cells = k.tile * k.tile;
  const int lane = lane_id(), lc = lane & 31, hw = (int)(threadIdx.x >> 5), wave = (int)(threadIdx.x >> 6);
  const int r2 = k.res * k.res;
  const uint32_t g_pix = k.layout ? 3 * kC : kC, g_row = (uint32_t)k.res * g_pix;
  __shared__ int next_it;
  for (;;) {
    if (threadIdx.x == 0) next_it = atomicAdd(k.next_item, 1);      // in order: see "point groups" above
    __syncthreads();
    const int it = next_it;
    if (it >= n_items) break;
    const int4 item = k.items[it];
    const int scene = item.x, bucket = item.y, first = item.z, n = item.w;
    const int4* ent = k.entries + (size_t)scene * 3 * (size_t)k.P + first;
    // ---- (1) counting sort by cell ----
    for (int c = threadIdx.x; c < cells; c += kBinThreads) cell_at[c] = 0;
    __syncthreads();
    int4 e[kBinChunk / kBinThreads];
    int rk[kBinChunk / kBinThreads];
#pragma unroll
    for (int q = 0; q < kBinChunk / kBinThreads; ++q)                   // all loads first (unconditional: they stay in flight together)
      e[q] = ent[min(q * kBinThreads + (int)threadIdx.x, n - 1)];
#pragma unroll
    for (int q = 0; q < kBinChunk / kBinThreads; ++q) {
      const int i = q * kBinThreads + (int)threadIdx.x;
      if (i < n) rk[q] = atomicAdd(&cell_at[e[q].y >> 20], 1);
    }
    __syncthreads();
    {
      // exclusive scan of the cell counts: <= 2 cells per thread, wave scan, wave totals
      const int per = (cells + kBinThreads - 1) / kBinThreads;
      const int lo = threadIdx.x * per, hi = min(lo + per, cells);
      int sum = 0;
      for (int c = lo; c < hi; ++c) sum += cell_at[c];
      int incl = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
      }
      if (lane == 63) wave_tot[wave] = incl;
      __syncthreads();
      int run = incl - sum;
      for (int w = 0; w < wave; ++w) run += wave_tot[w];
      for (int c = lo; c < hi; ++c) { const int m = cell_at[c]; cell_at[c] = run; run += m; }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kBinChunk / kBinThreads; ++q) {
      const int i = q * kBinThreads + (int)threadIdx.x;
      if (i < n) sorted[cell_at[e[q].y >> 20] + rk[q]] = e[q];
    }
    __syncthreads();
    // ---- (2) walk ----
    const int pl = (bucket % k.bpg) / (k.tps * k.tps);
    float* gtex = k.g_texels + (size_t)scene * 3 * r2 * kC + (size_t)pl * (k.layout ? (size_t)kC : (size_t)r2 * kC) + lc;
    // a point's row: wave-uniform base + a 32-bit byte offset (points_per_scene <= 2^25, checked by the launcher)
    const char* gf_scene = reinterpret_cast<const char*>(k.gf + (size_t)scene * (size_t)k.P * kC);
    const uint32_t lane_b = (uint32_t)lc * 4u;
    constexpr int kHalves = kBinThreads / 32;
    const int seg = (n + kHalves - 1) / kHalves;              // entries per half-wave
    const int s0 = min(hw * seg, n), s1 = min(s0 + seg, n);
    int cur = -1;
    float a00 = 0.0f, a10 = 0.0f, a01 = 0.0f, a11 = 0.0f;
    auto flush = [&]() {
      float* dst = gtex + (size_t)__umul24((uint32_t)cur, g_pix);
      unsafeAtomicAdd(dst, a00);
      unsafeAtomicAdd(dst + g_pix, a10);
      unsafeAtomicAdd(dst + g_row, a01);
      unsafeAtomicAdd(dst + g_row + g_pix, a11);
    };
    auto step = [&](const int4& e, float gv) {
      const int cj = e.y & 0xFFFFF;
      if (cj != cur) {
        if (cur >= 0) {
          // the left corner pair always goes out; when the next cell is the right-hand neighbour in the same texel row
          // its left corners are this cell's right corners - they are carried instead of written (halves the atomics on
          // densely populated rows)
          float* dst = gtex + (size_t)__umul24((uint32_t)cur, g_pix);
          unsafeAtomicAdd(dst, a00);
          unsafeAtomicAdd(dst + g_row, a01);
          if (cj != cur + 1) {
            unsafeAtomicAdd(dst + g_pix, a10);
            unsafeAtomicAdd(dst + g_row + g_pix, a11);
            a10 = a11 = 0.0f;
          }
          a00 = a10; a01 = a11;
        }
        cur = cj;
        a10 = a11 = 0.0f;
      }
      const float wa = __builtin_bit_cast(float, e.z), wb = __builtin_bit_cast(float, e.w);
      const float ga = 1.0f - wa, gb = 1.0f - wb;
      a00 = fmaf(ga * gb, gv, a00); a10 = fmaf(wa * gb, gv, a10);
      a01 = fmaf(ga * wb, gv, a01); a11 = fmaf(wa * wb, gv, a11);
    };
#pragma unroll 1
    for (int j = 0; j < seg; j += kBinDepth) {                 // seg is uniform: both halves of a wave run the same trip count
      int4 en[kBinDepth];
      float g[kBinDepth];
      const int base = s0 + j, left = s1 - base;               // entries base .. base + left - 1 are this half-wave's
      if (__all(left >= kBinDepth)) {
        // full group (all but the last turn of a segment): every LDS read (one broadcast address per half-wave, constant
        // offsets) is issued before the first row load, every row load before the first use - nothing conditional
        const int4* src = sorted + base;
#pragma unroll
        for (int q = 0; q < kBinDepth; ++q) en[q] = src[q];
#pragma unroll
        for (int q = 0; q < kBinDepth; ++q)
          g[q] = *reinterpret_cast<const float*>(gf_scene + (((uint32_t)en[q].x << 7) + lane_b));
#pragma unroll
        for (int q = 0; q < kBinDepth; ++q) step(en[q], g[q]);
      } else {
        const int last = max(s1 - 1, s0);                       // (an empty segment reads its neighbour's first entry: a valid point)
#pragma unroll
        for (int q = 0; q < kBinDepth; ++q) en[q] = sorted[min(min(base + q, last), n - 1)];
#pragma unroll
        for (int q = 0; q < kBinDepth; ++q)
          g[q] = *reinterpret_cast<const float*>(gf_scene + (((uint32_t)en[q].x << 7) + lane_b));
#pragma unroll
        for (int q = 0; q < kBinDepth; ++q)
          if (q < left) step(en[q], g[q]);
      }
    }
    if (cur >= 0) flush();
    __syncthreads();                                            // sorted[] / cell_at[] are reused by the next item
  }
}

// ------------------------------------------------------------------------------------------------
// ordered mode (scatter_mode 2): every gradient bit-identical from launch to launch.  No float atomic meets another
// and no sum depends on which wave came first:
//   g_texels : the backward kernel writes the rows and flags of the binned scatter; ord_keys makes one 64-bit key
//              (cell ib * res + ia << 32 | point) per point and plane - unique, in point order - and a STABLE radix sort
//              by cell (8-bit digits: hist / scan / scatter per pass, integer atomics only) turns each (scene, plane)
//              segment into runs of a cell in ascending point order; ord_gather: one half-wave per texel and plane,
//              lane = channel, walks the up to four cells that touch the texel in ascending cell order, a cell's run in
//              point order in blocks of 32 entries (weights recomputed with bin_entry's arithmetic, one fma chain per
//              block, the blocks' sums added in index order), then one load-add-store: each texel has one writer;
//   decoder, attention, beta, alpha: a zeroed slot per wave (FieldBwdParams::slot_stride), summed by param_finish_kernel
//              in slot order (16 contiguous parts per element, combined in part order).
// The statement holds for a fixed grid: the slot a chunk's sums land in follows the static chunk walk.
// ------------------------------------------------------------------------------------------------
constexpr int kOrdTile = 2048;             // keys per sort block: one wave, 32 steps of 64 (the order inside a block is the step order)
constexpr int kOrdDigits = 256;
// a wave's slot (floats): g_w1 [64][32], g_b1 [64], g_w2 [<= 16][64], g_b2 [<= 16], the scene's g_att [<= 15][3], beta, alpha;
// every region starts at a multiple of 16 (param_finish_kernel's blocks take 16 consecutive offsets)
constexpr int kSlotW1 = 0, kSlotB1 = kSlotW1 + kHidden * kC, kSlotW2 = kSlotB1 + kHidden, kSlotB2 = kSlotW2 + 16 * kHidden;
constexpr int kSlotAtt = kSlotB2 + 16, kSlotBeta = kSlotAtt + 48, kSlotAlpha = kSlotBeta + 1, kSlotFloats = kSlotBeta + 16;
static_assert(kSlotB1 % 16 == 0 && kSlotW2 % 16 == 0 && kSlotB2 % 16 == 0 && kSlotAtt % 16 == 0 && kSlotBeta % 16 == 0,
              "ordered mode: slot regions in units of 16 floats");

struct OrdParams {
  const float* points; int64_t P; int n_scenes; int res; float scene_range;
  const uint8_t* flag; const float* gf;
  uint64_t* keys_in; uint64_t* keys_out;       // [scenes * 3][P]: a pass reads one and writes the other
  uint32_t* hist; int nblk;                    // [scenes * 3][256 digits][nblk sort blocks]
  int shift;                                   // the pass's digit: key bits [32 + shift, 32 + shift + 8)
  float* g_texels; int layout;
};

// grid (ceil(P / 256), scenes): thread = point
__global__ __launch_bounds__(256) void ord_keys_kernel(OrdParams k) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= k.P) return;
  const int scene = blockIdx.y;
  const float* pt = k.points + ((size_t)scene * k.P + p) * 3;
  int c0[3];
  float f[3];
  const float rm1 = (float)(k.res - 1);
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    plane_coord(pt[ax] / k.scene_range, rm1, k.res, c0[ax], f[ax]);
    c0[ax] = min(max(c0[ax], 0), max(k.res - 2, 0));
  }
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
    const int ia = c0[(pl == 2) ? 1 : 0], ib = c0[(pl == 0) ? 1 : 2];      // plane 0: (x,y)  1: (x,z)  2: (y,z), as bin_entry
    k.keys_in[(size_t)(scene * 3 + pl) * k.P + p] = ((uint64_t)(uint32_t)(ib * k.res + ia) << 32) | (uint64_t)p;
  }
}

// grid (nblk, scenes * 3), 64 threads: digit counts of the block's kOrdTile keys
__global__ __launch_bounds__(64) void ord_hist_kernel(OrdParams k) {
  __shared__ uint32_t h[kOrdDigits];
  const int lane = threadIdx.x, seg = blockIdx.y;
  for (int d = lane; d < kOrdDigits; d += 64) h[d] = 0;
  __syncthreads();
  const uint64_t* keys = k.keys_in + (size_t)seg * k.P;
  for (int step = 0; step < kOrdTile / 64; ++step) {
    const int64_t i = (int64_t)blockIdx.x * kOrdTile + step * 64 + lane;
    if (i < k.P) atomicAdd(&h[(uint32_t)(keys[i] >> (32 + k.shift)) & 255u], 1u);
  }
  __syncthreads();
  for (int d = lane; d < kOrdDigits; d += 64) k.hist[((size_t)seg * kOrdDigits + d) * k.nblk + blockIdx.x] = h[d];
}

// grid (scenes * 3), 256 threads: exclusive scan of the segment's counts in (digit, block) order; thread = digit
__global__ __launch_bounds__(256) void ord_scan_kernel(OrdParams k) {
  __shared__ uint32_t tot[kOrdDigits];
  uint32_t* row = k.hist + ((size_t)blockIdx.x * kOrdDigits + threadIdx.x) * k.nblk;
  uint32_t sum = 0;
  for (int b = 0; b < k.nblk; ++b) sum += row[b];
  tot[threadIdx.x] = sum;
  __syncthreads();
  uint32_t at = 0;
  for (int d = 0; d < (int)threadIdx.x; ++d) at += tot[d];
  for (int b = 0; b < k.nblk; ++b) { const uint32_t c = row[b]; row[b] = at; at += c; }
}

// grid (nblk, scenes * 3), 64 threads: stable scatter - the block's keys in index order, 64 at a time; inside a step a key
// goes behind the keys of the same digit in lower lanes
__global__ __launch_bounds__(64) void ord_scatter_kernel(OrdParams k) {
  __shared__ uint32_t off[kOrdDigits];
  const int lane = threadIdx.x, seg = blockIdx.y;
  for (int d = lane; d < kOrdDigits; d += 64) off[d] = k.hist[((size_t)seg * kOrdDigits + d) * k.nblk + blockIdx.x];
  __syncthreads();
  const uint64_t* keys = k.keys_in + (size_t)seg * k.P;
  uint64_t* dst = k.keys_out + (size_t)seg * k.P;
  for (int step = 0; step < kOrdTile / 64; ++step) {
    const int64_t i = (int64_t)blockIdx.x * kOrdTile + step * 64 + lane;
    const bool valid = i < k.P;
    const uint64_t key = valid ? keys[i] : 0ull;
    const uint32_t d = (uint32_t)(key >> (32 + k.shift)) & 255u;
    uint64_t same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bal = __ballot(valid && bit);
      same &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull)), cnt = (uint32_t)__popcll(same);
    const uint32_t base = valid ? off[d] : 0u;
    __syncthreads();
    if (valid && rank + 1 == cnt) off[d] = base + cnt;       // the digit's last lane of the step
    __syncthreads();
    if (valid && (int64_t)base + rank < k.P) dst[base + rank] = key;
  }
}

// The sort as the two translation units call it (declared in nfi_host.hpp; the regulariser's ordered backward is the other
// user): `segments` runs of P keys each, sorted by cell with `passes` stable 8-bit passes - as many as the cell index
// res * res - 1 has digits.  keys / spare: [segments][P]; hist: plan.hist_bytes.  Returns the array that holds the result.
OrdSortPlan ord_sort_plan(int64_t P, int segments, int res) {
  OrdSortPlan plan;
  plan.blocks = (int)((P + kOrdTile - 1) / kOrdTile);
  int bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) < (uint64_t)res * res) ++bits;
  plan.passes = (bits + 7) / 8;
  plan.hist_bytes = (size_t)segments * kOrdDigits * plan.blocks * sizeof(uint32_t);
  return plan;
}

uint64_t* ord_sort_by_cell(uint64_t* keys, uint64_t* spare, uint32_t* hist, int64_t P, int segments, int res, hipStream_t s) {
  const OrdSortPlan plan = ord_sort_plan(P, segments, res);
  OrdParams op;
  memset(&op, 0, sizeof(op));
  op.P = P; op.keys_in = keys; op.keys_out = spare; op.hist = hist; op.nblk = plan.blocks;
  const dim3 sgrid((unsigned)plan.blocks, (unsigned)segments);
  for (int pass = 0; pass < plan.passes; ++pass) {
    op.shift = 8 * pass;
    hipLaunchKernelGGL(ord_hist_kernel, sgrid, dim3(64), 0, s, op);
    hipLaunchKernelGGL(ord_scan_kernel, dim3((unsigned)segments), dim3(256), 0, s, op);
    hipLaunchKernelGGL(ord_scatter_kernel, sgrid, dim3(64), 0, s, op);
    std::swap(op.keys_in, op.keys_out);
  }
  return op.keys_in;
}

// grid (ceil(scenes * 3 * res^2 / 8)), 256 threads: one half-wave per texel and plane, lane = channel (keys_in: the sorted keys)
__global__ __launch_bounds__(256) void ord_gather_kernel(OrdParams k) {
  const int l32 = threadIdx.x & 31;
  const int64_t h = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int rr = k.res * k.res;
  if (h >= (int64_t)k.n_scenes * 3 * rr) return;
  const int seg = (int)(h / rr), tex = (int)(h - (int64_t)seg * rr);
  const int scene = seg / 3, pl = seg - scene * 3;
  const int b = tex / k.res, a = tex - b * k.res;
  const int ax_a = (pl == 2) ? 1 : 0, ax_b = (pl == 0) ? 1 : 2;
  const uint64_t* keys = k.keys_in + (size_t)seg * k.P;
  const float* pts = k.points + (size_t)scene * k.P * 3;
  const uint8_t* flag = k.flag + (size_t)scene * k.P;
  const float* gf = k.gf + (size_t)scene * k.P * kC;
  const float rm1 = (float)(k.res - 1);
  float total = 0.0f;
  bool any = false;
#pragma unroll 1
  for (int c = 0; c < 4; ++c) {                       // cells (a-1,b-1), (a,b-1), (a-1,b), (a,b): ascending cell index
    const int ia = a - 1 + (c & 1), ib = b - 1 + (c >> 1);
    if (ia < 0 || ib < 0 || ia > k.res - 2 || ib > k.res - 2) continue;
    const bool right = !(c & 1), upper = !(c >> 1);   // which corner of the cell this texel is
    const uint32_t cell = (uint32_t)(ib * k.res + ia);
    const int64_t lo = ord_lower_bound(keys, k.P, (uint64_t)cell << 32);
    const int64_t hi = ord_lower_bound(keys, k.P, (uint64_t)(cell + 1u) << 32);
#pragma unroll 1
    for (int64_t base = lo; base < hi; base += 32) {
      const int64_t i = base + l32;
      uint32_t pt = 0u;
      float w = 0.0f;
      if (i < hi) {
        pt = (uint32_t)keys[i];
        if ((int64_t)pt < k.P && flag[pt]) {
          int i0;
          float fa, fb;
          plane_coord(pts[(size_t)pt * 3 + ax_a] / k.scene_range, rm1, k.res, i0, fa);
          plane_coord(pts[(size_t)pt * 3 + ax_b] / k.scene_range, rm1, k.res, i0, fb);
          w = (right ? fa : 1.0f - fa) * (upper ? fb : 1.0f - fb);
        }
      }
      const int n = (int)min((int64_t)32, hi - base);
      float part = 0.0f;
#pragma unroll 4
      for (int e = 0; e < n; ++e) {
        const float we = __shfl(w, e, 32);
        const uint32_t pe = (uint32_t)__shfl((int)pt, e, 32);
        if (we != 0.0f) { part = fmaf(we, gf[(size_t)pe * kC + l32], part); any = true; }
      }
      total += part;
    }
  }
  if (!any) return;
  const size_t g_pix = k.layout ? 3 * kC : kC, g_plane = k.layout ? (size_t)kC : (size_t)rr * kC;
  float* dst = k.g_texels + (size_t)scene * 3 * rr * kC + (size_t)pl * g_plane + (size_t)tex * g_pix + l32;
  *dst += total;
}

struct FinishParams {
  const float* slots; int slots_per_scene, n_scenes, A, n_out, use_sdf;
  float *g_w1, *g_b1, *g_w2, *g_b2, *g_att, *g_beta, *g_alpha;
};

// grid (kSlotFloats / 16), 256 threads = 16 slot offsets x 16 parts: ordered_slot_sum over all slots (the attention
// values: over each scene's), part 0 adds the sum to the caller's buffer
__global__ __launch_bounds__(256) void param_finish_kernel(FinishParams k) {
  __shared__ float partial[16][16];
  const int e = threadIdx.x & 15, part = threadIdx.x >> 4;
  const int o = blockIdx.x * 16 + e;
  if (o >= kSlotAtt && o < kSlotBeta) {               // (block-uniform: the regions are multiples of 16)
    for (int sc = 0; sc < k.n_scenes; ++sc) {
      const float t = ordered_slot_sum(k.slots, kSlotFloats, o, sc * k.slots_per_scene, k.slots_per_scene, partial);
      if (part == 0 && o - kSlotAtt < k.A * 3) k.g_att[(size_t)sc * k.A * 3 + (o - kSlotAtt)] += t;
    }
    return;
  }
  const float t = ordered_slot_sum(k.slots, kSlotFloats, o, 0, k.n_scenes * k.slots_per_scene, partial);
  if (part != 0) return;
  if (o < kSlotB1) k.g_w1[o] += t;
  else if (o < kSlotW2) k.g_b1[o - kSlotB1] += t;
  else if (o < kSlotB2) { if (o - kSlotW2 < k.n_out * kHidden) k.g_w2[o - kSlotW2] += t; }
  else if (o < kSlotAtt) { if (o - kSlotB2 < k.n_out) k.g_b2[o - kSlotB2] += t; }
  else if (k.use_sdf && o == kSlotBeta) k.g_beta[0] += t;
  else if (k.use_sdf && o == kSlotAlpha) k.g_alpha[0] += t;
}

// point groups per scene: the smallest power of two that brings a group's gradient rows under kBinGroupRowBytes (1 when
// the scene's rows already are, or when the points do not divide into groups of whole 1024-point blocks)
static inline int bin_groups(int64_t P) {
  int g = 1;
  while (g < 16 && (size_t)P * kC * sizeof(float) > kBinGroupRowBytes * (size_t)g) g *= 2;
  return (g > 1 && P % ((int64_t)g * 1024) == 0) ? g : 1;
}
// 8 x 8-texel tiles for planes up to 256^2 (buckets that fit one LDS chunk: complete cell runs), 16 x 16 when the scene is
// cut into four or more groups (the buckets of a group are a quarter as full: about the same entries per work item)
static inline int bin_tile_side(int res, int groups) { return res <= 256 ? (groups >= 4 ? 16 : 8) : (res <= 512 ? 16 : 32); }
static inline size_t bin_max_items(int n_scenes, int64_t P, int res) {
  const int g = bin_groups(P), t = bin_tile_side(res, g), tps = (res + t - 1) / t;
  return (size_t)n_scenes * ((size_t)(3 * P / kBinChunk) + (size_t)g * 3 * tps * tps);
}

// The workspace of one nfi_field_query_bwd call: byte offsets of its regions and the total.  Behind the backward operand
// image come, for the binned scatter only, the feature-gradient rows, the sorted entries, the bucket counters
// (count[nb], n_items + the reduce's cursor padded to 64 B, cursor[nb]), the work items and the per-point flags.
// The ordered mode keeps the rows and the flags and adds the two key arrays of the radix sort, its digit counts and the
// parameter-gradient slots (one per wave of the largest grid the call can get).
struct FieldBwdCarve {
  bool binned, ordered;
  int groups, tile, tps;             // binned scatter: point groups per scene, tile side, tiles per plane side
  size_t nb, max_items;              // buckets over all scenes, upper bound of the work items
  size_t gf, entries, counts, items, flag, total;
  int sort_blocks;                   // ordered: sort blocks per (scene, plane) segment (ord_sort_plan)
  size_t keys[2], hist, slots, slot_bytes;
};

// blocks per scene of the backward kernel's grid, before the ray-order hint rounds it down to the 8 XCDs:
// one resident set of blocks (2 per CU, 1 for the view-direction variant): every wave ends with ~3 k atomics on
// the same weight-gradient addresses as every other wave, so more waves than the chip holds only add flush traffic
// (points_only has no flush and balances better with more, smaller blocks)
static int64_t field_bwd_blocks(const nfi_field_bwd_args* a) {
  const int64_t chunks = (a->points_per_scene + 63) / 64;
  int64_t blocks = (chunks + 3) / 4;
  int64_t cap = (a->points_only ? 1024 : (a->ray_features ? 256 : 512)) / a->n_scenes;
  if (cap < 16) cap = 16;
  return blocks > cap ? cap : blocks;
}

static FieldBwdCarve field_bwd_carve(const nfi_field_bwd_args* a) {
  FieldBwdCarve c;
  memset(&c, 0, sizeof(c));
  c.binned = a->scatter_mode == 1 && !a->points_only;
  c.ordered = a->scatter_mode == 2 && !a->points_only && !a->ray_features && a->n_scenes > 0 && a->points_per_scene > 0 &&
              a->plane_res >= 2;
  size_t at = align256((a->ray_features ? kVbImageFloats : kBwdImageFloats) * sizeof(float));      // operand image at 0
  if (c.binned) {
    const size_t n_pts = (size_t)a->n_scenes * (size_t)a->points_per_scene;
    c.groups = bin_groups(a->points_per_scene);
    c.tile = bin_tile_side(a->plane_res, c.groups);
    c.tps = (a->plane_res + c.tile - 1) / c.tile;
    c.nb = (size_t)a->n_scenes * c.groups * 3 * c.tps * c.tps;
    c.max_items = bin_max_items(a->n_scenes, a->points_per_scene, a->plane_res);
    c.gf = at; at += align256(n_pts * kC * sizeof(float));
    c.entries = at; at += align256(3 * n_pts * sizeof(int4));
    c.counts = at; at += align256(2 * c.nb * sizeof(int) + 64);
    c.items = at; at += align256(c.max_items * sizeof(int4));
    c.flag = at; at += align256(n_pts);
  }
  if (c.ordered) {
    const size_t n_pts = (size_t)a->n_scenes * (size_t)a->points_per_scene;
    const OrdSortPlan plan = ord_sort_plan(a->points_per_scene, a->n_scenes * 3, a->plane_res);
    c.sort_blocks = plan.blocks;
    c.gf = at; at += align256(n_pts * kC * sizeof(float));
    c.flag = at; at += align256(n_pts);
    c.keys[0] = at; at += align256(3 * n_pts * sizeof(uint64_t));
    c.keys[1] = at; at += align256(3 * n_pts * sizeof(uint64_t));
    c.hist = at; at += align256(plan.hist_bytes);
    c.slot_bytes = (size_t)a->n_scenes * (size_t)field_bwd_blocks(a) * 4 * kSlotFloats * sizeof(float);
    c.slots = at; at += align256(c.slot_bytes);
  }
  c.total = at;
  return c;
}

extern "C" size_t nfi_field_bwd_workspace_bytes(const nfi_field_bwd_args* a) { return a ? field_bwd_carve(a).total : 0; }

extern "C" size_t nfi_decoder_bwd_image_floats(void) { return (size_t)kBwdImageFloats; }
extern "C" size_t nfi_decoder_bwd_image_floats_viewdir(void) { return (size_t)kVbImageFloats; }

template <bool ATT, bool COORD, bool VD, int TEX>
static int launch_field_bwd(dim3 grid, hipStream_t s, const FieldBwdParams& k) {
  constexpr auto kernel = &field_query_bwd_kernel<ATT, COORD, VD, TEX>;
  using Dec = FieldDecoderBwd<VD>;
  // the two operand images and four waves' staging: it depends on the decoder only
  constexpr size_t shmem = (size_t)(Dec::kFwd + Dec::kBwdImg + 4 * Dec::kWaveFloats) * sizeof(float);
  const int rc = ensure_dynamic_lds<kernel>(shmem, "field_query_bwd");
  if (rc) return rc;
  hipLaunchKernelGGL(kernel, grid, dim3(256), shmem, s, k);
  return NFI_OK;
}

// The argument rules of nfi_field_query_bwd (pointers against null, integers against limits: nothing is dereferenced)
static int field_bwd_check_call(const nfi_field_bwd_args* a) {
  REQUIRE(a && a->points && a->texels && a->decoder_image && a->w1 && a->w2 && a->workspace && a->g_sigma && a->g_rgb,
          "field_query_bwd: null pointer");
  REQUIRE(a->points_only ? a->g_points != nullptr : (a->g_texels && a->g_w1 && a->g_b1 && a->g_w2 && a->g_b2),
          "field_query_bwd: output pointer missing");
  REQUIRE(a->n_scenes > 0 && a->points_per_scene > 0, "field_query_bwd: bad shape");
  REQUIRE(a->texel_dtype >= NFI_TEXEL_F32 && a->texel_dtype <= NFI_TEXEL_F16, "field_query_bwd: bad texel dtype");
  REQUIRE(a->texel_dtype == NFI_TEXEL_F32 || !a->ray_features, "field_query_bwd: the view-direction decoder needs fp32 texels");
  int rc = check_field_common(a->texels, a->plane_res, a->texel_dtype, a->decoder_image, a->n_attention,
                              a->attention_values, a->use_sdf, a->beta, a->alpha, a->texel_layout);
  if (rc) return rc;
  REQUIRE(a->points_only || a->n_attention == 0 || a->g_attention_values, "field_query_bwd: g_attention_values missing");
  REQUIRE(a->points_only || !a->use_sdf || (a->g_beta && a->g_alpha), "field_query_bwd: g_beta / g_alpha missing");
  const bool vd = a->ray_features != nullptr;
  REQUIRE(a->scatter_mode >= 0 && a->scatter_mode <= 2, "field_query_bwd: scatter_mode must be 0, 1 or 2");
  REQUIRE(a->scatter_mode != 2 || !vd,
          "field_query_bwd: scatter_mode 2 (ordered) does not cover the view-direction decoder (its g_ray_features are atomics)");
  REQUIRE(a->scatter_mode != 2 || !a->points_only, "field_query_bwd: scatter_mode 2 (ordered) with points_only has nothing to order");
  REQUIRE(a->workspace_bytes >= nfi_field_bwd_workspace_bytes(a), "field_query_bwd: workspace too small");
  REQUIRE(a->points_per_scene <= (int64_t)1 << 30, "field_query_bwd: at most 2^30 points per scene");
  REQUIRE(a->scatter_mode == 0 || a->points_only || a->points_per_scene <= (int64_t)1 << 25,
          "field_query_bwd: the binned and the ordered scatter take at most 2^25 points per scene (use scatter_mode 0 or split the query)");
  REQUIRE(!vd || (a->w3 && a->samples_per_ray > 0 && a->points_per_scene % a->samples_per_ray == 0),
          "field_query_bwd: view-direction decoder needs w3 and points_per_scene % samples_per_ray == 0");
  REQUIRE(!vd || a->points_only || (a->g_w3 && a->g_b3), "field_query_bwd: g_w3 / g_b3 missing");
  return NFI_OK;
}

// which field_query_bwd_kernel instantiation a (validated) call gets: its launcher and its canonical name
struct FieldBwdLaunch { int (*launch)(dim3, hipStream_t, const FieldBwdParams&); const char* name; };
static constexpr char kFieldBwdFamily[] = "field_query_bwd_kernel";
template <bool ATT, bool COORD, bool VD, int TEX>
static FieldBwdLaunch field_bwd_launch() { return {&launch_field_bwd<ATT, COORD, VD, TEX>, KernelName<kFieldBwdFamily, ATT, COORD, VD, TEX>::value.s}; }

static FieldBwdLaunch select_field_bwd_kernel(const nfi_field_bwd_args* a) {
  const bool vd = a->ray_features != nullptr, coord = a->g_points != nullptr;
  return dispatch_texel_att(a->texel_dtype, a->n_attention > 0, [&](auto tex, auto att_c) -> FieldBwdLaunch {
    constexpr int TEX = decltype(tex)::value;
    constexpr bool ATT = decltype(att_c)::value;
    if constexpr (TEX == 0) {     // the view-direction decoder: fp32 texels (checked)
      if (vd) return coord ? field_bwd_launch<ATT, true, true, 0>() : field_bwd_launch<ATT, false, true, 0>();
    }
    return coord ? field_bwd_launch<ATT, true, false, TEX>() : field_bwd_launch<ATT, false, false, TEX>();
  });
}

extern "C" const char* nfi_field_bwd_kernel_name(const nfi_field_bwd_args* a) {
  if (field_bwd_check_call(a)) return nullptr;
  return select_field_bwd_kernel(a).name;
}

extern "C" int nfi_field_query_bwd(const nfi_field_bwd_args* a, nfi_stream_t stream) {
  int rc = field_bwd_check_call(a);
  if (rc) return rc;
  const bool vd = a->ray_features != nullptr;
  hipStream_t s = (hipStream_t)stream;
  const int n_out = a->n_attention > 0 ? 1 + a->n_attention : 4;
  const FieldBwdCarve ws = field_bwd_carve(a);
  char* const w = reinterpret_cast<char*>(a->workspace);
  float* image_bwd = reinterpret_cast<float*>(w);
  if (vd)
    hipLaunchKernelGGL(decoder_pack_bwd_vd_kernel, dim3(1), dim3(256), 0, s, a->w1, a->w2, a->w3,
                       a->n_attention > 0 ? a->n_attention : 3, image_bwd);
  else
    hipLaunchKernelGGL(decoder_pack_bwd_kernel, dim3(1), dim3(256), 0, s, a->w1, a->w2, n_out, image_bwd);
  FieldBwdParams k{};                // (no ray-order hint, atomic scatter: zeros / null)
  k.points = a->points; k.P = a->points_per_scene;
  k.texels = reinterpret_cast<const float*>(a->texels); k.res = a->plane_res; k.layout = a->texel_layout;
  k.image = a->decoder_image; k.image_bwd = image_bwd; k.A = a->n_attention; k.att = a->attention_values;
  k.use_sdf = a->use_sdf; k.beta = a->beta; k.alpha = a->alpha; k.scene_range = a->scene_range;
  k.g_sigma = a->g_sigma; k.g_rgb = a->g_rgb; k.g_sdf = a->g_sdf; k.g_sem = a->g_semantics;
  k.g_texels = a->g_texels; k.g_points = a->g_points;
  k.g_w1 = a->g_w1; k.g_b1 = a->g_b1; k.g_w2 = a->g_w2; k.g_b2 = a->g_b2;
  k.g_att = a->g_attention_values; k.g_beta = a->g_beta; k.g_alpha = a->g_alpha;
  k.points_only = a->points_only; k.normalize_points = a->normalize_g_points;
  k.xray = a->ray_features; k.spr = a->samples_per_ray; k.g_xray = a->g_ray_features; k.g_w3 = a->g_w3; k.g_b3 = a->g_b3;
  BinParams bp;
  memset(&bp, 0, sizeof(bp));
  if (ws.binned) {
    int* count = reinterpret_cast<int*>(w + ws.counts);      // count[nb], n_items (+ pad to 64 B), cursor[nb]
    int* n_items = count + ws.nb;
    // count[] and n_items are zeroed; cursor[], items[] and entries[] are written by the scan / fill, flag[] by the kernel
    if (hipMemsetAsync(count, 0, (ws.nb + 16) * sizeof(int), s) != hipSuccess)
      return fail(NFI_ERR_LAUNCH, "field_query_bwd: memset failed");
    k.gf_out = reinterpret_cast<float*>(w + ws.gf);
    k.bin_flag = reinterpret_cast<uint8_t*>(w + ws.flag);
    bp.points = a->points; bp.P = a->points_per_scene; bp.n_scenes = a->n_scenes; bp.res = a->plane_res;
    bp.scene_range = a->scene_range; bp.flag = k.bin_flag; bp.gf = k.gf_out; bp.count = count; bp.cursor = n_items + 16;
    bp.entries = reinterpret_cast<int4*>(w + ws.entries); bp.items = reinterpret_cast<int4*>(w + ws.items); bp.n_items = n_items;
    bp.g_texels = a->g_texels; bp.layout = a->texel_layout;
    bp.tile = ws.tile; bp.tps = ws.tps; bp.bpg = 3 * ws.tps * ws.tps; bp.n_buckets = ws.groups * bp.bpg;
    bp.groups = ws.groups; bp.group_pts = a->points_per_scene / ws.groups; bp.next_item = n_items + 1;
  }
  OrdParams op;
  memset(&op, 0, sizeof(op));
  if (ws.ordered) {
    // every wave's slot is zeroed; keys, counts, rows and flags are written before they are read
    float* slots = reinterpret_cast<float*>(w + ws.slots);
    if (hipMemsetAsync(slots, 0, ws.slot_bytes, s) != hipSuccess) return fail(NFI_ERR_LAUNCH, "field_query_bwd: memset failed");
    k.gf_out = reinterpret_cast<float*>(w + ws.gf);
    k.bin_flag = reinterpret_cast<uint8_t*>(w + ws.flag);
    k.g_w1 = slots + kSlotW1; k.g_b1 = slots + kSlotB1; k.g_w2 = slots + kSlotW2; k.g_b2 = slots + kSlotB2;
    k.g_att = slots + kSlotAtt; k.g_beta = slots + kSlotBeta; k.g_alpha = slots + kSlotAlpha;
    k.slot_stride = kSlotFloats;
    op.points = a->points; op.P = a->points_per_scene; op.n_scenes = a->n_scenes; op.res = a->plane_res;
    op.scene_range = a->scene_range; op.flag = k.bin_flag; op.gf = k.gf_out;
    op.hist = reinterpret_cast<uint32_t*>(w + ws.hist); op.nblk = ws.sort_blocks;
    op.g_texels = a->g_texels; op.layout = a->texel_layout;
  }
  int64_t blocks = field_bwd_blocks(a);
  if (a->rays_per_row > 0 && a->samples_per_ray > 0 && a->samples_per_ray % 64 == 0 &&
      a->points_per_scene % a->samples_per_ray == 0 && (a->points_per_scene / a->samples_per_ray) % a->rays_per_row == 0) {
    // ray-order hint: usable when the image divides into 16- or 8-pixel tiles and the grid into the 8 XCDs
    const int64_t rows = a->points_per_scene / a->samples_per_ray / a->rays_per_row;
    const int ts = (a->rays_per_row % 16 == 0 && rows % 16 == 0) ? 16 : ((a->rays_per_row % 8 == 0 && rows % 8 == 0) ? 8 : 0);
    if (ts && blocks >= 8 && rows * a->rays_per_row < ((int64_t)1 << 30)) {
      blocks &= ~(int64_t)7;
      k.tside = ts; k.tw = a->rays_per_row; k.cpr = a->samples_per_ray / 64;
      k.tiles_x = a->rays_per_row / ts; k.n_tiles = k.tiles_x * (int)(rows / ts);
      k.div_cpr = make_fastdiv((uint32_t)k.cpr); k.div_tside = make_fastdiv((uint32_t)ts); k.div_tiles_x = make_fastdiv((uint32_t)k.tiles_x);
    }
  }
  dim3 grid((unsigned)blocks, (unsigned)a->n_scenes);
  rc = select_field_bwd_kernel(a).launch(grid, s, k);
  if (rc) return rc;
  if (ws.binned) {
    const dim3 pgrid((unsigned)((a->points_per_scene + 1023) / 1024), (unsigned)a->n_scenes);
    hipLaunchKernelGGL(bin_count_kernel, pgrid, dim3(256), 0, s, bp);
    hipLaunchKernelGGL(bin_scan_kernel, dim3((unsigned)a->n_scenes), dim3(256), 0, s, bp);
    hipLaunchKernelGGL(bin_fill_kernel, pgrid, dim3(256), 0, s, bp);
    // persistent: the resident set of workgroups (2 per CU) takes the work items in order from the cursor
    hipLaunchKernelGGL(bin_reduce_kernel, dim3((unsigned)std::min<size_t>(ws.max_items, 256 * 2)), dim3(kBinThreads), 0, s, bp);
  }
  if (ws.ordered) {
    const FinishParams fp{reinterpret_cast<const float*>(w + ws.slots), (int)blocks * 4, a->n_scenes, a->n_attention, n_out, a->use_sdf,
                          a->g_w1, a->g_b1, a->g_w2, a->g_b2, a->g_attention_values, a->g_beta, a->g_alpha};
    hipLaunchKernelGGL(param_finish_kernel, dim3(kSlotFloats / 16), dim3(256), 0, s, fp);
    op.keys_in = reinterpret_cast<uint64_t*>(w + ws.keys[0]); op.keys_out = reinterpret_cast<uint64_t*>(w + ws.keys[1]);
    hipLaunchKernelGGL(ord_keys_kernel, dim3((unsigned)((a->points_per_scene + 255) / 256), (unsigned)a->n_scenes), dim3(256), 0, s, op);
    op.keys_in = ord_sort_by_cell(op.keys_in, op.keys_out, op.hist, a->points_per_scene, a->n_scenes * 3, a->plane_res, s);
    const int64_t half_waves = (int64_t)a->n_scenes * 3 * a->plane_res * a->plane_res;
    hipLaunchKernelGGL(ord_gather_kernel, dim3((unsigned)((half_waves + 7) / 8)), dim3(256), 0, s, op);
  }
  return check_launch("field_query_bwd");
}
