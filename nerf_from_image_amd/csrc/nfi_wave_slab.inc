// nfi_wave_slab.inc — what one wave does with one ray's samples, as device functions on a per-wave LDS slab: the CDF and
// its inverse, smoothing, importance resampling, the merge of the coarse and fine lists, compositing (included by
// nfi_kernels.hip).  No kernel and no entry point here.  Three users, all included after this file: the stand-alone stage
// kernels (nfi_ray_stages.inc), their backward (nfi_backward_rays.inc) and the persistent render kernels
// (nfi_render_kernels.inc, nfi_render_long.inc).  Expects nfi_device.hpp (the wave primitives) and `using namespace nfi`.

// ------------------------------------------------------------------------------------------------
// per-wave LDS slab used by the sampling / compositing stages
// ------------------------------------------------------------------------------------------------
template <int N>
struct __attribute__((aligned(16))) WaveSlabT {
  static constexpr int kN = N;
  float cdf[N];
  float bins[N];
  uint32_t key[N];
  float srt[5][N];   // depth, sigma, r, g, b in merged order
  float piv[N / 8];  // every eighth cdf entry (cdf[8p + 7], +inf past the end): build_cdf / invert_cdf
};
using WaveSlab = WaveSlabT<128>;       // up to 64 + 64 samples per ray
using WaveSlabWide = WaveSlabT<256>;   // up to 128 + 128

// ---- inverse CDF on a ray held one element per (slot, lane) -----------------------------------
// bins[e] e<M, weights[e] e<M-1 (already padded with 0 past M-1).  Writes cdf/bins to the slab and
// returns, for each of this lane's u values, the sample and the searchsorted index.
template <int SPL, class Slab>
__device__ __forceinline__ void build_cdf(Slab& slab, const float (&bins)[SPL], const float (&wts)[SPL], int M,
                                          int lane) {
  float q[SPL];
  float tot = 0.0f;
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    int e = j * 64 + lane;
    q[j] = (e < M - 1) ? (wts[j] + 1e-5f) : 0.0f;
    tot += q[j];
  }
  tot = wave_sum(tot);
  float pdf[SPL], inc[SPL];
#pragma unroll
  for (int j = 0; j < SPL; ++j) pdf[j] = (j * 64 + lane < M - 1) ? q[j] / tot : 0.0f;
  incl_cumsum<SPL>(pdf, inc, lane);
  // cdf[0] = 0, cdf[e+1] = inclusive sum through e
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    int e = j * 64 + lane;
    if (e < M - 1) slab.cdf[e + 1] = inc[j];
    if (e < M) slab.bins[e] = bins[j];
    // pivot table for the two-level search of invert_cdf: entry p = cdf[8p + 7] (+inf past the end)
    if (((e + 1) & 7) == 7) slab.piv[(e + 1) >> 3] = (e + 1 < M) ? inc[j] : INFINITY;
  }
  if (lane == 0) slab.cdf[0] = 0.0f;
  wave_lds_fence();
}

// NP: pivots to look at = ceil(largest M / 8) of the caller (a multiple of 4; build_cdf<SPL> writes 8 SPL of them)
template <int NP, class Slab>
__device__ __forceinline__ float invert_cdf(const Slab& slab, int M, float u, int& ind) {
  // searchsorted(cdf, u, right=True) = #{cdf <= u} over the ascending cdf, as an 8-way two-level search: the pivots
  // (every eighth entry: two or four 16-byte broadcast reads) give the block, the block's eight entries the position -
  // two dependent LDS round trips instead of the seven or eight of a binary search
  {
    const f32x4* pv = reinterpret_cast<const f32x4*>(slab.piv);
    int b = 0;
#pragma unroll
    for (int i = 0; i < NP / 4; ++i) {
      const f32x4 p = pv[i];
      b += (p.x <= u ? 1 : 0) + (p.y <= u ? 1 : 0) + (p.z <= u ? 1 : 0) + (p.w <= u ? 1 : 0);
    }
    const f32x4* cv = reinterpret_cast<const f32x4*>(slab.cdf + 8 * b);
    const f32x4 c0 = cv[0], c1 = cv[1];
    const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) cnt += (8 * b + e < M && c[e] <= u) ? 1 : 0;
    ind = 8 * b + cnt;
  }
  int lo = ind - 1 < 0 ? 0 : ind - 1;
  int hi = ind > M - 1 ? M - 1 : ind;
  float c_lo = slab.cdf[lo], c_hi = slab.cdf[hi];
  float b_lo = slab.bins[lo], b_hi = slab.bins[hi];
  float den = c_hi - c_lo;
  den = (den < 1e-5f) ? 1.0f : den;
  float fr = (u - c_lo) / den;
  return b_lo + fr * (b_hi - b_lo);
}

// EG3D smoothing of S weights held one per lane (run.py:264-272); lanes >= S return garbage
__device__ __forceinline__ float smooth_weights(float w, int S, int lane) {
  float wp = lane_prev(w, -INFINITY);
  float wn = lane_next(w, -INFINITY);
  if (lane >= S - 1) wn = -INFINITY;
  float m0 = fmaxf(wp, w);   // max(w[k-1], w[k])
  float m1 = fmaxf(w, wn);   // max(w[k], w[k+1])
  return (m0 + m1) / 2.0f + 0.01f;
}

// hierarchical resampling for S <= 64: coarse weights -> smooth -> pdf over smooth[1..S-2] on the
// S-1 bin mid-points -> S fine depths.  Returns the fine depth for this lane's u.
struct ResampleTaps { float w, smooth, T; int ind; };
__device__ __forceinline__ float resample_ray(WaveSlab& slab, float sigma, float t, int S, float dnorm, float u, int lane,
                                              ResampleTaps* taps) {
  float sg[1] = {lane < S ? sigma : 0.0f}, tt[1] = {t}, w[1], T[1];
  ray_weights<1>(sg, tt, S, dnorm, lane, w, T);
  float sm = smooth_weights(w[0], S, lane);
  float tn = lane_next(t, 0.0f);
  float mid[1] = {0.5f * (tn + t)};                       // bins e = 0..S-2
  float wts[1] = {lane_next(sm, 0.0f)};                    // weights e = 0..S-3  <- smooth[e+1]
  build_cdf<1>(slab, mid, wts, S - 1, lane);
  int ind;
  float z = invert_cdf<8>(slab, S - 1, u, ind);
  if (taps) { taps->w = w[0]; taps->smooth = sm; taps->ind = ind; taps->T = T[0]; }
  return z;
}

// The same for 64 < S <= 128 (two elements per lane, element e = slot*64 + lane).
template <int SP>
__device__ __forceinline__ void smooth_weights_wide(const float (&w)[SP], int S, int lane, float (&sm)[SP]) {
#pragma unroll
  for (int j = 0; j < SP; ++j) {
    const float prev_edge = j > 0 ? bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(w[j > 0 ? j - 1 : 0]), 63)) : -INFINITY;
    const float next_edge = j + 1 < SP ? bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(w[j + 1 < SP ? j + 1 : j]), 0)) : -INFINITY;
    const float wp = lane_prev(w[j], prev_edge);
    float wn = lane_next(w[j], next_edge);
    if (j * 64 + lane >= S - 1) wn = -INFINITY;
    const float m0 = fmaxf(wp, w[j]), m1 = fmaxf(w[j], wn);
    sm[j] = (m0 + m1) / 2.0f + 0.01f;
  }
}

template <int SP, class Slab>
__device__ __forceinline__ void resample_ray_wide(Slab& slab, const float (&sigma)[SP], const float (&t)[SP], int S, float dnorm,
                                                  const float (&u)[SP], int lane, float (&z)[SP], float (&w)[SP],
                                                  float (&sm)[SP], int (&ind)[SP], float (&T)[SP]) {
  float sg[SP];
#pragma unroll
  for (int j = 0; j < SP; ++j) sg[j] = (j * 64 + lane < S) ? sigma[j] : 0.0f;
  ray_weights<SP>(sg, t, S, dnorm, lane, w, T);
  smooth_weights_wide<SP>(w, S, lane, sm);
  float tn[SP], mid[SP], wts[SP];
  next_elem<SP>(t, tn, lane);
  next_elem<SP>(sm, wts, lane);                               // weights e = 0..S-3  <- smooth[e+1]
#pragma unroll
  for (int j = 0; j < SP; ++j) mid[j] = 0.5f * (tn[j] + t[j]);  // bins e = 0..S-2
  build_cdf<SP>(slab, mid, wts, S - 1, lane);
#pragma unroll
  for (int j = 0; j < SP; ++j) z[j] = invert_cdf<8 * SP>(slab, S - 1, u[j], ind[j]);
}

// ---- merge + composite ---------------------------------------------------------------------------
// Every lane owns up to 2 input samples (element e = slot*64+lane of cat(a,b)); computes the
// stable ascending rank of each key among the n keys, scatters (depth, sigma, rgb) to the slab in
// merged order.  rank_out: merged position of each of this lane's elements.
template <int NS, class Slab>
__device__ __forceinline__ void merge_scatter(Slab& slab, const float (&dep)[NS], const float (&sig)[NS],
                                              const float (&cr)[NS], const float (&cg)[NS], const float (&cb)[NS],
                                              const int (&eidx)[NS], int n, int (&rank_out)[NS]) {
  // eidx[j]: index of this lane's j-th element in cat(a, b) (>= n: no element)
  uint32_t key[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    key[j] = ordered_key(dep[j]);
    if (eidx[j] < n) slab.key[eidx[j]] = key[j];
  }
  wave_lds_fence();
  int rank[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) rank[j] = 0;
  const uint4* kv = reinterpret_cast<const uint4*>(slab.key);
  const int n4 = (n + 3) >> 2;
  for (int i = 0; i < n4; ++i) {
    uint4 q = kv[i];
    uint32_t qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int idx = 4 * i + c;
      bool in = idx < n;
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        bool before = (qq[c] < key[j]) || (qq[c] == key[j] && idx < eidx[j]);
        rank[j] += (in && before) ? 1 : 0;
      }
    }
  }
  wave_lds_fence();
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    rank_out[j] = rank[j];
    if (eidx[j] < n) {
      int r = rank[j];
      slab.srt[0][r] = dep[j]; slab.srt[1][r] = sig[j];
      slab.srt[2][r] = cr[j]; slab.srt[3][r] = cg[j]; slab.srt[4][r] = cb[j];
    }
  }
  wave_lds_fence();
}

// Merge for the fused renderer, lane = sample index k < S: the coarse list is (checked to be)
// ascending, so only the S fine keys have to be ranked by counting:
//   rank(coarse k) = k + #{fine j : z_j <  t_k}
//   rank(fine  k)  = #{coarse j : t_j <= z_k} + #{fine j : z_j < z_k or (z_j == z_k and j < k)}
// i.e. the stable ascending order of cat(coarse, fine) (coarse first on ties), ~4x fewer compares
// than ranking all 2S keys against all 2S keys.  Falls back to the general count when the coarse
// depths are not ascending (possible only through 1-ulp rounding of the jittered depths).
struct MergeIn { float t, sigma, r, g, b; };
__device__ __forceinline__ void merge_pair_scatter(WaveSlab& slab, const MergeIn& c, const MergeIn& f, int S, int lane,
                                                   int& rank_c, int& rank_f) {
  const bool valid = lane < S;
  const uint32_t kc = valid ? ordered_key(c.t) : 0xFFFFFFFFu;
  const uint32_t kf = valid ? ordered_key(f.t) : 0xFFFFFFFFu;
  const uint32_t kc_next = f2bits(lane_next(bits2f(kc), bits2f(0xFFFFFFFFu)));
  const bool ascending = __all(lane >= S - 1 || kc <= kc_next);
  slab.key[lane] = kf;            // fine keys   [0,64)   (padding 0xFFFFFFFF ranks after everything)
  slab.key[64 + lane] = kc;       // coarse keys [64,128)
  uint32_t* kpiv = reinterpret_cast<uint32_t*>(slab.piv);          // every eighth coarse key (the pivot row is free after the resampling)
  if ((lane & 7) == 7) kpiv[lane >> 3] = kc;
  wave_lds_fence();
  const uint4* kv = reinterpret_cast<const uint4*>(slab.key);
  const int n4 = (S + 3) >> 2;
  int cnt_a = 0, cnt_b = 0, cnt_c = 0;
  if (ascending) {
    // #{fine < z_k} against all fine keys; the coarse side needs no second comparison per key: with the coarse keys
    // ascending, a fine key f is below coarse key k exactly when #{coarse <= f} <= k, so #{fine < t_k} is the running sum
    // over the histogram of the fine keys' upper bounds (one LDS add per lane + one wave scan instead of 64 compares)
    // (all 16 quads, whatever S: the padding keys 0xFFFFFFFF never count, and a fixed trip count lets the 16 LDS reads
    //  go out together instead of one LDS latency per turn)
    uint4 qv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) qv[i] = kv[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t qq[4] = {qv[i].x, qv[i].y, qv[i].z, qv[i].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) cnt_b += (qq[e] < kf) ? 1 : 0;
    }
    // #{coarse <= z_k} over the ascending coarse keys: 8-way two-level search (pivots, then the block's eight keys), two
    // dependent LDS round trips instead of a binary search's seven
    {
      const uint4* pv = reinterpret_cast<const uint4*>(kpiv);
      const uint4 p0 = pv[0], p1 = pv[1];
      const int b = (p0.x <= kf ? 1 : 0) + (p0.y <= kf ? 1 : 0) + (p0.z <= kf ? 1 : 0) + (p0.w <= kf ? 1 : 0) +
                    (p1.x <= kf ? 1 : 0) + (p1.y <= kf ? 1 : 0) + (p1.z <= kf ? 1 : 0) + (p1.w <= kf ? 1 : 0);
      const uint4* cv = reinterpret_cast<const uint4*>(slab.key + 64 + 8 * b);
      const uint4 c0 = cv[0], c1 = cv[1];
      const uint32_t c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      int cnt = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) cnt += (8 * b + e < 64 && c[e] <= kf) ? 1 : 0;
      cnt_c = 8 * b + cnt;
    }
    uint32_t* hist = reinterpret_cast<uint32_t*>(slab.bins);      // (free after the resampling) entries 0 .. S
    hist[lane] = 0u;
    if (lane == 0) hist[64] = 0u;
    wave_lds_fence();
    if (valid) atomicAdd(&hist[cnt_c], 1u);
    wave_lds_fence();
    cnt_a = (int)wave_incl_scan_add_f32((float)hist[lane]);
  } else {
    for (int i = 0; i < n4; ++i) {
      const uint4 q = kv[i];
      const uint32_t qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        cnt_a += (qq[e] < kc) ? 1 : 0;
        cnt_b += (qq[e] < kf) ? 1 : 0;
      }
    }
  }
  // fine depths are almost never equal.  Equal keys have equal counts of smaller keys and distinct keys distinct counts,
  // so a tie shows as two lanes claiming the same slot of a scratch row (the cdf row is free after the resampling):
  // one LDS write + read instead of a third comparison per key.  Only then the count is redone with the stable
  // tie-break of torch.sort (earlier index first)
  uint32_t* claim = reinterpret_cast<uint32_t*>(slab.cdf);
  if (valid) claim[cnt_b] = (uint32_t)lane;
  wave_lds_fence();
  const bool lost = valid && claim[cnt_b] != (uint32_t)lane;
  wave_lds_fence();
  if (__any(lost)) {
    cnt_b = 0;
    for (int i = 0; i < n4; ++i) {
      const uint4 q = kv[i];
      const uint32_t qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = 4 * i + e;
        cnt_b += ((qq[e] < kf) || (qq[e] == kf && idx < lane)) ? 1 : 0;
      }
    }
  }
  if (ascending) {
    rank_c = lane + cnt_a;
  } else {
    int cnt_d = 0;   // coarse j before coarse k
    for (int i = 0; i < n4; ++i) {
      const uint4 q = kv[16 + i];
      const uint32_t qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = 4 * i + e;
        cnt_c += (idx < S && qq[e] <= kf) ? 1 : 0;
        cnt_d += (idx < S && (qq[e] < kc || (qq[e] == kc && idx < lane))) ? 1 : 0;
      }
    }
    rank_c = cnt_d + cnt_a;
  }
  rank_f = cnt_c + cnt_b;
  wave_lds_fence();
  if (valid) {
    slab.srt[0][rank_c] = c.t; slab.srt[1][rank_c] = c.sigma; slab.srt[2][rank_c] = c.r; slab.srt[3][rank_c] = c.g; slab.srt[4][rank_c] = c.b;
    slab.srt[0][rank_f] = f.t; slab.srt[1][rank_f] = f.sigma; slab.srt[2][rank_f] = f.r; slab.srt[3][rank_f] = f.g; slab.srt[4][rank_f] = f.b;
  }
  wave_lds_fence();
}

// The same for two elements per lane and list (64 < S <= 128, element e = slot*64 + lane).  Returns false - nothing
// written - when the coarse depths are not ascending; the caller then uses the general merge_scatter.
template <class Slab>
__device__ __forceinline__ bool merge_pair_scatter_wide(Slab& slab, const float (&dep)[4], const float (&sig)[4],
                                                        const float (&cr)[4], const float (&cg)[4], const float (&cb)[4],
                                                        int S, int lane, int (&rank)[4]) {
  // dep[0..1] coarse slots, dep[2..3] fine slots
  uint32_t kc[2], kf[2];
  bool val[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    val[j] = j * 64 + lane < S;
    kc[j] = val[j] ? ordered_key(dep[j]) : 0xFFFFFFFFu;
    kf[j] = val[j] ? ordered_key(dep[2 + j]) : 0xFFFFFFFFu;
  }
  // ascending check of the coarse list across the two slots
  const uint32_t first1 = (uint32_t)__builtin_amdgcn_readlane((int)kc[1], 0);
  const uint32_t n0 = f2bits(lane_next(bits2f(kc[0]), bits2f(first1)));
  const uint32_t n1 = f2bits(lane_next(bits2f(kc[1]), bits2f(0xFFFFFFFFu)));
  const bool ok0 = (lane >= S - 1) || kc[0] <= n0, ok1 = (64 + lane >= S - 1) || kc[1] <= n1;
  if (!__all(ok0 && ok1)) return false;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    slab.key[j * 64 + lane] = kf[j];           // fine keys   [0,128)
    slab.key[128 + j * 64 + lane] = kc[j];     // coarse keys [128,256)
  }
  uint32_t* kpiv = reinterpret_cast<uint32_t*>(slab.piv);          // every eighth coarse key (16 pivots)
#pragma unroll
  for (int j = 0; j < 2; ++j) if ((lane & 7) == 7) kpiv[(j * 64 + lane) >> 3] = kc[j];
  wave_lds_fence();
  const uint4* kv = reinterpret_cast<const uint4*>(slab.key);
  const int n4 = (S + 3) >> 2;
  int cnt_a[2] = {0, 0}, cnt_b[2] = {0, 0}, cnt_c[2];
  // all 32 quads of the fine keys in two batches of 16 LDS reads (padding keys never count; see merge_pair_scatter)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint4 qv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) qv[i] = kv[16 * h + i];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t qq[4] = {qv[i].x, qv[i].y, qv[i].z, qv[i].w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          cnt_b[j] += (qq[e] < kf[j]) ? 1 : 0;
        }
    }
  }
  {
    // #{coarse <= z} over the ascending coarse keys: two-level 8-way search (merge_pair_scatter)
    const uint4* pv = reinterpret_cast<const uint4*>(kpiv);
    const uint4 pq[4] = {pv[0], pv[1], pv[2], pv[3]};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int b = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        b += (pq[i].x <= kf[j] ? 1 : 0) + (pq[i].y <= kf[j] ? 1 : 0) + (pq[i].z <= kf[j] ? 1 : 0) + (pq[i].w <= kf[j] ? 1 : 0);
      const uint4* cv = reinterpret_cast<const uint4*>(slab.key + 128 + 8 * b);
      const uint4 c0 = cv[0], c1 = cv[1];
      const uint32_t c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      int cnt = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) cnt += (8 * b + e < 128 && c[e] <= kf[j]) ? 1 : 0;
      cnt_c[j] = 8 * b + cnt;
    }
  }
  {
    // #{fine < t_e} for the ascending coarse keys = running sum over the histogram of the fine keys' upper bounds
    // (merge_pair_scatter): entries 0 .. S of the bins row, element e = slot * 64 + lane
    uint32_t* hist = reinterpret_cast<uint32_t*>(slab.bins);
    hist[lane] = 0u; hist[64 + lane] = 0u;
    if (lane == 0) hist[128] = 0u;
    wave_lds_fence();
#pragma unroll
    for (int j = 0; j < 2; ++j) if (val[j]) atomicAdd(&hist[cnt_c[j]], 1u);
    wave_lds_fence();
    const float s0 = wave_incl_scan_add_f32((float)hist[lane]);
    const float t0 = bits2f((uint32_t)__builtin_amdgcn_readlane((int)f2bits(s0), 63));
    const float s1 = t0 + wave_incl_scan_add_f32((float)hist[64 + lane]);
    cnt_a[0] = (int)s0; cnt_a[1] = (int)s1;
  }
  // ties among the fine keys = two elements claiming the same slot (see merge_pair_scatter)
  uint32_t* claim = reinterpret_cast<uint32_t*>(slab.cdf);
#pragma unroll
  for (int j = 0; j < 2; ++j) if (val[j]) claim[cnt_b[j]] = (uint32_t)(j * 64 + lane);
  wave_lds_fence();
  bool lost = false;
#pragma unroll
  for (int j = 0; j < 2; ++j) lost = lost || (val[j] && claim[cnt_b[j]] != (uint32_t)(j * 64 + lane));
  wave_lds_fence();
  if (__any(lost)) {
    cnt_b[0] = cnt_b[1] = 0;            // equal fine depths exist: stable tie-break (earlier index first)
    for (int i = 0; i < n4; ++i) {
      const uint4 q = kv[i];
      const uint32_t qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int idx = 4 * i + e;
          cnt_b[j] += ((qq[e] < kf[j]) || (qq[e] == kf[j] && idx < j * 64 + lane)) ? 1 : 0;
        }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    rank[j] = j * 64 + lane + cnt_a[j];
    rank[2 + j] = cnt_c[j] + cnt_b[j];
  }
  wave_lds_fence();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (val[j]) {
      const int rc = rank[j], rf = rank[2 + j];
      slab.srt[0][rc] = dep[j]; slab.srt[1][rc] = sig[j]; slab.srt[2][rc] = cr[j]; slab.srt[3][rc] = cg[j]; slab.srt[4][rc] = cb[j];
      slab.srt[0][rf] = dep[2 + j]; slab.srt[1][rf] = sig[2 + j]; slab.srt[2][rf] = cr[2 + j]; slab.srt[3][rf] = cg[2 + j]; slab.srt[4][rf] = cb[2 + j];
    }
  }
  wave_lds_fence();
  return true;
}

struct CompositeOut { float r, g, b, depth, mask; };

// composite the n samples sitting in merged order in the slab (lib/nerf_utils.py:123-161)
template <int NS, class Slab>
__device__ __forceinline__ CompositeOut composite_slab(const Slab& slab, int n, float dnorm, int white, int lane,
                                                       float (&w_out)[NS]) {
  float dep[NS], sig[NS], w[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    dep[j] = (e < n) ? slab.srt[0][e] : 0.0f;
    sig[j] = (e < n) ? slab.srt[1][e] : 0.0f;
  }
  ray_weights<NS>(sig, dep, n, dnorm, lane, w);
  float r = 0.0f, g = 0.0f, b = 0.0f, d = 0.0f, m = 0.0f;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    int e = j * 64 + lane;
    if (e < n) {
      r += w[j] * slab.srt[2][e]; g += w[j] * slab.srt[3][e]; b += w[j] * slab.srt[4][e];
      d += w[j] * dep[j]; m += w[j];
    }
    w_out[j] = w[j];
  }
  CompositeOut o;
  o.r = wave_sum(r); o.g = wave_sum(g); o.b = wave_sum(b); o.depth = wave_sum(d); o.mask = wave_sum(m);
  if (white) { float bg = 1.0f - o.mask; o.r += bg; o.g += bg; o.b += bg; }
  return o;
}
