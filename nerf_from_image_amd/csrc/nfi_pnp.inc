// nfi_pnp.inc — camera pose from a canonical-coordinate map (included by nfi_modules.hip).
//
// Reference: lib/pose_estimation.py:30-131 (compute_pose_pnp), called per inversion batch through
// run.py:1709-1740 (estimate_poses_batch) with a .cpu().numpy() round trip and OpenCV's solvePnPGeneric
// (SQPNP, EPNP fallback, then an iterative refinement) per image and focal-length proposal.  OpenCV is not part of
// this image, so what is restated here is the PROBLEM the reference hands to it, not OpenCV's code:
//
//     given N >= 4 foreground pixels with screen positions (x, y) = (col / W - 0.5, row / H - 0.5), their canonical
//     object coordinates P and intrinsics diag(f, f, 1):  find [R | t] minimising the reprojection error
//     sum || f (R P + t)_xy / (R P + t)_z - (x, y) ||^2, report sqrt(sum / 2N) (OpenCV's RMSE), keep the focal
//     proposal with the smallest error among the solutions with t_z > 0.
//
// PARITY UNPINNED: no golden vectors can be produced here (cv2 absent); tests validate by pose recovery on exact and
// noisy synthetic correspondences and against an independent float64 solver (tests/test_pose_estimation.py).
//
// One workgroup per (image, focal proposal), everything in float64:
//   1. Hartley-normalised DLT: the 12x12 normal matrix of the projective constraints is assembled from 40 moment sums
//      (one pass over the pixels), its smallest eigenvector (cyclic Jacobi, one thread) is the projection matrix
//      M ~ lambda [R | t]; R by polar decomposition (Newton iteration), t = M[:,3] / lambda;
//   2. Levenberg-Marquardt on the reprojection error over the 6 pose parameters (left-multiplied rotation increment):
//      per iteration one pass over the pixels for J^T J (21 sums), J^T r (6) and the error, a 6x6 solve by one thread.
//   3. where the linear start does not exist (4 or 5 pixels: the reference solves those too, pose_estimation.py:58), is
//      degenerate (coplanar points: the second-smallest eigenvalue is as small as the smallest) or ends behind the camera
//      (OpenCV falls back to EPNP there): Levenberg-Marquardt from the 24 axis-aligned rotations, the translation from the
//      weak-perspective depth (image spread against object spread) and the centroids; the valid result with the smallest
//      error is kept.  The common case (>= 6 pixels in general position) still runs ONE refinement.
// A second launch selects the best proposal per image and writes flip @ [R | t] like pose_estimation.py:119-127.

constexpr int kPnpThreads = 256;
constexpr int kPnpCand = 16;     // doubles per candidate: R[9], t[3], rmse, valid, n, focal

struct PnpParams {
  int B, H, W, nf, iters;
  const float* coords; const float* mask; float thr;
  const float* focals;
  double* cand;
};

template <int K>
__device__ __forceinline__ void pnp_block_sum(double (&v)[K], double* red) {
  // red: [4 waves][K] doubles of LDS.  Afterwards every thread holds the block totals.
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double x = v[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const uint64_t b = __builtin_bit_cast(uint64_t, x);
      const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)b, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(b >> 32), d, 64);
      x += __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
    }
    if (lane == 0) red[wave * K + k] = x;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
  __syncthreads();
}

// symmetric index of (i, j), i <= j, in a packed upper triangle of an n x n matrix
__device__ __forceinline__ int pnp_tri(int i, int j, int n) { return i * n - i * (i - 1) / 2 + (j - i); }

// eigenvector of the smallest eigenvalue; gap[0] = smallest, gap[1] = second smallest, gap[2] = largest eigenvalue
__device__ void pnp_jacobi_smallest(double* a /*[12][12]*/, double* vecs /*[12][12]*/, double* out /*[12]*/, double* gap) {
  const int n = 12;
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) vecs[i * n + j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < n; ++p) for (int q = p + 1; q < n; ++q) off += a[p * n + q] * a[p * n + q];
    if (off < 1e-30) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[p * n + q];
        if (fabs(apq) < 1e-300) continue;
        const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {
          const double akp = a[k * n + p], akq = a[k * n + q];
          a[k * n + p] = c * akp - s * akq; a[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = a[p * n + k], aqk = a[q * n + k];
          a[p * n + k] = c * apk - s * aqk; a[q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = vecs[k * n + p], vkq = vecs[k * n + q];
          vecs[k * n + p] = c * vkp - s * vkq; vecs[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  int best = 0;
  for (int i = 1; i < n; ++i) if (a[i * n + i] < a[best * n + best]) best = i;
  for (int k = 0; k < n; ++k) out[k] = vecs[k * n + best];
  double second = 1e300, largest = 0.0;
  for (int i = 0; i < n; ++i) {
    if (i != best && a[i * n + i] < second) second = a[i * n + i];
    if (a[i * n + i] > largest) largest = a[i * n + i];
  }
  gap[0] = a[best * n + best]; gap[1] = second; gap[2] = largest;
}

// the 24 rotations that map coordinate axes onto coordinate axes (idx in [0, 24)): row r has its +-1 in column perm[r]
__device__ void pnp_cube_rotation(int idx, double* R) {
  const int perms[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {1, 0, 2}, {2, 1, 0}};
  const int p = idx >> 2, sg = idx & 3;
  const double parity = p < 3 ? 1.0 : -1.0;
  const double s0 = (sg & 1) ? -1.0 : 1.0, s1 = (sg & 2) ? -1.0 : 1.0, s2 = parity * s0 * s1;
  for (int i = 0; i < 9; ++i) R[i] = 0.0;
  R[0 * 3 + perms[p][0]] = s0; R[1 * 3 + perms[p][1]] = s1; R[2 * 3 + perms[p][2]] = s2;
}

__device__ __forceinline__ double pnp_det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__device__ __forceinline__ void pnp_inv3_t(const double* m, double* o) {   // o = inverse(m)^T = cofactor(m) / det
  const double d = pnp_det3(m);
  o[0] = (m[4] * m[8] - m[5] * m[7]) / d; o[1] = (m[5] * m[6] - m[3] * m[8]) / d; o[2] = (m[3] * m[7] - m[4] * m[6]) / d;
  o[3] = (m[2] * m[7] - m[1] * m[8]) / d; o[4] = (m[0] * m[8] - m[2] * m[6]) / d; o[5] = (m[1] * m[6] - m[0] * m[7]) / d;
  o[6] = (m[1] * m[5] - m[2] * m[4]) / d; o[7] = (m[2] * m[3] - m[0] * m[5]) / d; o[8] = (m[0] * m[4] - m[1] * m[3]) / d;
}

// solves (H + mu diag(H)) d = -g for the 6 pose parameters (Gaussian elimination with partial pivoting)
__device__ bool pnp_solve6(const double* H, const double* g, double mu, double* d) {
  double a[6][7];
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) a[i][j] = H[i <= j ? pnp_tri(i, j, 6) : pnp_tri(j, i, 6)];
    a[i][i] += mu * (a[i][i] + 1e-12);
    a[i][6] = -g[i];
  }
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    for (int r = c + 1; r < 6; ++r) if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
    if (fabs(a[piv][c]) < 1e-300) return false;
    if (piv != c) for (int k = 0; k < 7; ++k) { const double tmp = a[c][k]; a[c][k] = a[piv][k]; a[piv][k] = tmp; }
    for (int r = c + 1; r < 6; ++r) {
      const double f = a[r][c] / a[c][c];
      for (int k = c; k < 7; ++k) a[r][k] -= f * a[c][k];
    }
  }
  for (int r = 5; r >= 0; --r) {
    double s = a[r][6];
    for (int k = r + 1; k < 6; ++k) s -= a[r][k] * d[k];
    d[r] = s / a[r][r];
  }
  return true;
}

// R' = exp([w]x) R  (Rodrigues), t' = t + dt
__device__ void pnp_apply_step(const double* R, const double* t, const double* d, double* Rn, double* tn) {
  const double wx = d[0], wy = d[1], wz = d[2];
  const double th = sqrt(wx * wx + wy * wy + wz * wz);
  double E[9];
  if (th < 1e-12) {
    E[0] = 1; E[1] = -wz; E[2] = wy; E[3] = wz; E[4] = 1; E[5] = -wx; E[6] = -wy; E[7] = wx; E[8] = 1;
  } else {
    const double kx = wx / th, ky = wy / th, kz = wz / th, c = cos(th), s = sin(th), v = 1.0 - c;
    E[0] = c + kx * kx * v;      E[1] = kx * ky * v - kz * s; E[2] = kx * kz * v + ky * s;
    E[3] = ky * kx * v + kz * s; E[4] = c + ky * ky * v;      E[5] = ky * kz * v - kx * s;
    E[6] = kz * kx * v - ky * s; E[7] = kz * ky * v + kx * s; E[8] = c + kz * kz * v;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = E[i * 3] * R[j] + E[i * 3 + 1] * R[3 + j] + E[i * 3 + 2] * R[6 + j];
  for (int i = 0; i < 3; ++i) tn[i] = t[i] + d[3 + i];
}

__global__ __launch_bounds__(kPnpThreads) void pnp_solve_kernel(PnpParams k) {
  __shared__ double red[4 * 40];
  __shared__ double mat[144], vecs[144], pose[12], trial[12], Hcur[21], gcur[6], scal[8], best[13];
  const int b = blockIdx.y, fi = blockIdx.x;
  const int hw = k.H * k.W;
  const double f = (double)k.focals[fi];
  const float* C = k.coords + (size_t)b * hw * 3;
  const float* Mk = k.mask + (size_t)b * hw;
  double* out = k.cand + ((size_t)b * k.nf + fi) * kPnpCand;
  auto screen = [&](int i, double& x, double& y) {
    const int row = i / k.W, col = i - row * k.W;
    x = (double)col / (double)k.W - 0.5; y = (double)row / (double)k.H - 0.5;
  };
  // ---- pass 0: count and centroids ----
  double s0[6] = {0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < hw; i += kPnpThreads) {
    if (!(Mk[i] > k.thr)) continue;
    double x, y; screen(i, x, y);
    s0[0] += 1.0; s0[1] += C[i * 3]; s0[2] += C[i * 3 + 1]; s0[3] += C[i * 3 + 2]; s0[4] += x / f; s0[5] += y / f;
  }
  pnp_block_sum<6>(s0, red);
  const double n = s0[0];
  if (n < 4.0) {            // pose_estimation.py:58: fewer than 4 points are not solved
    if (threadIdx.x == 0) { for (int i = 0; i < kPnpCand; ++i) out[i] = 0.0; out[14] = n; out[15] = f; }
    return;
  }
  const double c3[3] = {s0[1] / n, s0[2] / n, s0[3] / n}, c2[2] = {s0[4] / n, s0[5] / n};
  // ---- pass 1: mean distances (Hartley normalisation) ----
  double s1[2] = {0, 0};
  for (int i = threadIdx.x; i < hw; i += kPnpThreads) {
    if (!(Mk[i] > k.thr)) continue;
    double x, y; screen(i, x, y);
    const double dx = C[i * 3] - c3[0], dy = C[i * 3 + 1] - c3[1], dz = C[i * 3 + 2] - c3[2];
    const double du = x / f - c2[0], dv = y / f - c2[1];
    s1[0] += sqrt(dx * dx + dy * dy + dz * dz); s1[1] += sqrt(du * du + dv * dv);
  }
  pnp_block_sum<2>(s1, red);
  const double sc3 = sqrt(3.0) / fmax(s1[0] / n, 1e-300), sc2 = sqrt(2.0) / fmax(s1[1] / n, 1e-300);
  if (threadIdx.x == 0) { scal[3] = 0.0; best[12] = -1.0; }      // scal[3]: a linear start exists
  if (n >= 6.0) {
  // ---- pass 2: moments  S = sum p p^T, Su = sum u p p^T, Sv = sum v p p^T, Sq = sum (u^2+v^2) p p^T  (p = (X,Y,Z,1)) ----
  double mo[40];
#pragma unroll
  for (int i = 0; i < 40; ++i) mo[i] = 0.0;
  for (int i = threadIdx.x; i < hw; i += kPnpThreads) {
    if (!(Mk[i] > k.thr)) continue;
    double x, y; screen(i, x, y);
    const double p[4] = {sc3 * (C[i * 3] - c3[0]), sc3 * (C[i * 3 + 1] - c3[1]), sc3 * (C[i * 3 + 2] - c3[2]), 1.0};
    const double u = sc2 * (x / f - c2[0]), v = sc2 * (y / f - c2[1]), q = u * u + v * v;
    int idx = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = r; c < 4; ++c) {
        const double pp = p[r] * p[c];
        mo[idx] += pp; mo[10 + idx] += u * pp; mo[20 + idx] += v * pp; mo[30 + idx] += q * pp;
        ++idx;
      }
  }
  pnp_block_sum<40>(mo, red);
  if (threadIdx.x == 0) {
    // A^T A for rows [p, 0, -u p], [0, p, -v p]
    auto S = [&](int blk, int r, int c) { return mo[blk * 10 + (r <= c ? pnp_tri(r, c, 4) : pnp_tri(c, r, 4))]; };
    for (int i = 0; i < 144; ++i) mat[i] = 0.0;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) {
        mat[r * 12 + c] = S(0, r, c); mat[(4 + r) * 12 + 4 + c] = S(0, r, c);
        mat[r * 12 + 8 + c] = -S(1, r, c); mat[(8 + r) * 12 + c] = -S(1, r, c);
        mat[(4 + r) * 12 + 8 + c] = -S(2, r, c); mat[(8 + r) * 12 + 4 + c] = -S(2, r, c);
        mat[(8 + r) * 12 + 8 + c] = S(3, r, c);
      }
    double m[12], gap[3];
    pnp_jacobi_smallest(mat, vecs, m, gap);
    // coplanar (or otherwise degenerate) points: the null space of the constraints has more than one dimension and the
    // eigenvector is an arbitrary member of it - no linear start then
    scal[3] = gap[1] > 1e-8 * gap[2] ? 1.0 : 0.0;
    // de-normalise: M = T2^-1 Mn T3,  T2^-1 = [[1/sc2, 0, c2x], [0, 1/sc2, c2y], [0, 0, 1]],  T3 = [[sc3 I, -sc3 c3], [0, 1]]
    double M[12];
    for (int c = 0; c < 4; ++c) {
      M[c] = m[c] / sc2 + c2[0] * m[8 + c]; M[4 + c] = m[4 + c] / sc2 + c2[1] * m[8 + c]; M[8 + c] = m[8 + c];
    }
    for (int r = 0; r < 3; ++r) {
      const double a0 = M[r * 4], a1 = M[r * 4 + 1], a2 = M[r * 4 + 2], a3 = M[r * 4 + 3];
      M[r * 4] = sc3 * a0; M[r * 4 + 1] = sc3 * a1; M[r * 4 + 2] = sc3 * a2;
      M[r * 4 + 3] = a3 - sc3 * (a0 * c3[0] + a1 * c3[1] + a2 * c3[2]);
    }
    double R[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]};
    double det = pnp_det3(R);
    const double sgn = det < 0.0 ? -1.0 : 1.0;
    const double lam = cbrt(fabs(det)) + 1e-300;
    for (int i = 0; i < 9; ++i) R[i] = sgn * R[i] / lam;
    for (int it = 0; it < 20; ++it) {       // polar decomposition: R <- (R + R^-T) / 2
      double Ri[9];
      pnp_inv3_t(R, Ri);
      for (int i = 0; i < 9; ++i) R[i] = 0.5 * (R[i] + Ri[i]);
    }
    for (int i = 0; i < 9; ++i) pose[i] = R[i];
    for (int i = 0; i < 3; ++i) pose[9 + i] = sgn * M[i * 4 + 3] / lam;
    for (int i = 0; i < 12; ++i) trial[i] = pose[i];
    for (int i = 0; i < 12; ++i) if (!(trial[i] == trial[i]) || fabs(trial[i]) > 1e30) scal[3] = 0.0;
  }
  }   // n >= 6
  __syncthreads();
  // ---- starts: 0 = the linear one, 1..24 = the axis-aligned rotations (only where the linear one does not do) ----
  for (int start = 0; start <= 24; ++start) {
    if (threadIdx.x == 0) {
      double go = 1.0;
      if (start == 0) go = scal[3] > 0.5 ? 1.0 : 0.0;
      else if (start == 1 && best[12] >= 0.0) go = 2.0;            // the linear start led to a valid pose: done
      else {
        double R0[9];
        pnp_cube_rotation(start - 1, R0);
        const double d0 = sc2 / sc3;                                // weak perspective: image spread = object spread / depth
        for (int i = 0; i < 9; ++i) trial[i] = R0[i];
        for (int r = 0; r < 3; ++r)
          trial[9 + r] = d0 * (r == 0 ? c2[0] : (r == 1 ? c2[1] : 1.0)) - (R0[r * 3] * c3[0] + R0[r * 3 + 1] * c3[1] + R0[r * 3 + 2] * c3[2]);
      }
      scal[0] = 1e-3;      // LM damping
      scal[1] = -1.0;      // error of `pose` (unknown yet)
      scal[2] = go;
    }
    __syncthreads();
    const double go = scal[2];
    __syncthreads();                                                // (thread 0 rewrites scal[] at the top of the next start)
    if (go > 1.5) break;
    if (go < 0.5) continue;
  // ---- Levenberg-Marquardt on the reprojection error ----
  for (int it = 0; it <= (start == 0 ? k.iters : (k.iters > 60 ? k.iters : 60)); ++it) {     // (an axis-aligned start can be 60 degrees off)
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = trial[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = trial[9 + i];
    double acc[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0.0;
    for (int i = threadIdx.x; i < hw; i += kPnpThreads) {
      if (!(Mk[i] > k.thr)) continue;
      double x, y; screen(i, x, y);
      const double X = C[i * 3], Y = C[i * 3 + 1], Z = C[i * 3 + 2];
      const double qx = R[0] * X + R[1] * Y + R[2] * Z, qy = R[3] * X + R[4] * Y + R[5] * Z, qz = R[6] * X + R[7] * Y + R[8] * Z;
      const double px = qx + t[0], py = qy + t[1], pz = qz + t[2];
      if (!(pz > 1e-9)) { acc[27] += 2.0; continue; }          // behind the camera: a constant penalty, no gradient
      const double iz = 1.0 / pz, rx = f * px * iz - x, ry = f * py * iz - y;
      // d(proj)/dP = f/pz [[1, 0, -px/pz], [0, 1, -py/pz]];  P = exp([w]x) q + t, q = R X:  dP/dw = -[q]x,  dP/dt = I
      const double a = f * iz, bx = -f * px * iz * iz, by = -f * py * iz * iz;
      const double Jx[6] = {bx * qy, a * qz - bx * qx, -a * qy, a, 0.0, bx};
      const double Jy[6] = {-a * qz + by * qy, -by * qx, a * qx, 0.0, a, by};
      int idx = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = r; c < 6; ++c) acc[idx++] += Jx[r] * Jx[c] + Jy[r] * Jy[c];
        acc[21 + r] += Jx[r] * rx + Jy[r] * ry;
      }
      acc[27] += rx * rx + ry * ry;
    }
    pnp_block_sum<28>(acc, red);
    if (threadIdx.x == 0) {
      const double err = acc[27];
      bool accepted = false;
      if (scal[1] < 0.0 || err < scal[1]) {
        for (int i = 0; i < 12; ++i) pose[i] = trial[i];
        for (int i = 0; i < 21; ++i) Hcur[i] = acc[i];
        for (int i = 0; i < 6; ++i) gcur[i] = acc[21 + i];
        if (scal[1] >= 0.0) scal[0] = fmax(scal[0] / 3.0, 1e-15);
        scal[1] = err;
        accepted = true;
      } else {
        scal[0] = fmin(scal[0] * 4.0, 1e12);
      }
      (void)accepted;
      double d[6];
      if (pnp_solve6(Hcur, gcur, scal[0], d)) pnp_apply_step(pose, pose + 9, d, trial, trial + 9);
      else for (int i = 0; i < 12; ++i) trial[i] = pose[i];
    }
    __syncthreads();
  }
    if (threadIdx.x == 0) {
      const double rmse = sqrt(scal[1] / (2.0 * n));
      const bool ok = pose[11] > 0.0 && rmse == rmse && rmse < 1e30;
      if (ok && (best[12] < 0.0 || rmse < best[12])) {
        for (int i = 0; i < 12; ++i) best[i] = pose[i];
        best[12] = rmse;
      }
    }
    __syncthreads();
  }   // starts
  if (threadIdx.x == 0) {
    const bool ok = best[12] >= 0.0;
    for (int i = 0; i < 12; ++i) out[i] = ok ? best[i] : 0.0;
    out[12] = ok ? best[12] : 0.0; out[13] = ok ? 1.0 : 0.0; out[14] = n; out[15] = f;
  }
}

__global__ void pnp_select_kernel(PnpParams k, float* world2cam, float* focal, float* error) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= k.B) return;
  int best = -1;
  double best_err = 1e300;
  for (int fi = 0; fi < k.nf; ++fi) {
    const double* c = k.cand + ((size_t)b * k.nf + fi) * kPnpCand;
    if (c[13] > 0.5 && c[12] < best_err) { best_err = c[12]; best = fi; }
  }
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, -10};
  double fo = 1.0, err = 10.0;              // pose_estimation.py:110-117: a dummy pose looking away from the object
  if (best >= 0) {
    const double* c = k.cand + ((size_t)b * k.nf + best) * kPnpCand;
    for (int i = 0; i < 9; ++i) R[i] = c[i];
    for (int i = 0; i < 3; ++i) t[i] = c[9 + i];
    fo = c[15]; err = c[12];
  }
  float* o = world2cam + (size_t)b * 16;
  // flip @ [R | t]: rows 1 and 2 negated (pose_estimation.py:121-127)
  for (int r = 0; r < 3; ++r) {
    const float s = r == 0 ? 1.0f : -1.0f;
    for (int c = 0; c < 3; ++c) o[r * 4 + c] = s * (float)R[r * 3 + c];
    o[r * 4 + 3] = s * (float)t[r];
  }
  o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
  focal[b] = (float)fo;
  error[b] = (float)err;
}

extern "C" size_t nfi_pnp_workspace_bytes(int n_images, int n_focal) {
  return (size_t)n_images * (size_t)n_focal * kPnpCand * sizeof(double);
}

extern "C" int nfi_pose_pnp(const nfi_pnp_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->coords && a->mask && a->focal_proposals && a->world2cam && a->focal && a->error && a->workspace,
          "pose_pnp: null pointer");
  REQUIRE(a->n_images > 0 && a->height > 0 && a->width > 0 && a->n_focal > 0 && a->n_focal <= 64,
          "pose_pnp: need images, a pixel grid and 1..64 focal proposals");
  REQUIRE(a->refine_iterations >= 0 && a->refine_iterations <= 200, "pose_pnp: refine_iterations must be in [0,200]");
  REQUIRE(a->workspace_bytes >= nfi_pnp_workspace_bytes(a->n_images, a->n_focal), "pose_pnp: workspace too small");
  REQUIRE((reinterpret_cast<uintptr_t>(a->workspace) & 7) == 0, "pose_pnp: workspace must be 8-byte aligned");
  PnpParams k{a->n_images, a->height, a->width, a->n_focal, a->refine_iterations, a->coords, a->mask, a->mask_threshold,
              a->focal_proposals, reinterpret_cast<double*>(a->workspace)};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pnp_solve_kernel, dim3((unsigned)a->n_focal, (unsigned)a->n_images), dim3(kPnpThreads), 0, s, k);
  hipLaunchKernelGGL(pnp_select_kernel, dim3((unsigned)((a->n_images + 63) / 64)), dim3(64), 0, s, k, a->world2cam, a->focal,
                     a->error);
  return check_launch("pose_pnp");
}
