// nfi_pose.inc — the pose algebra of the inversion loop, lib/pose_utils.py (included by nfi_modules.hip).
//
// Thread = image in every kernel; 64-thread blocks, a grid that covers n_images, a tail guard.  The work per image is a
// few hundred flops, so what a call costs is its launch: each entry is ONE launch where the reference runs a chain of
// tensor expressions on [B,4] / [B,4,4] operands (and, for matrix_to_pose and perturb_poses, host round trips).
// Arithmetic: fp32 in, float64 inside, one rounding out.  No atomics, no shared state: launches repeat bit for bit.

namespace nfi_pose {

constexpr int kThreads = 64;
constexpr double kNormEps = 1e-12;          // F.normalize's eps
constexpr double kDegrees = 180.0 / 3.14159265358979323846;

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 mul(double k, V3 a) { return {k * a.x, k * a.y, k * a.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 unit(int i) { return {i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, i == 2 ? 1.0 : 0.0}; }

// q / max(|q|, eps); returns the factor and whether the norm (not the eps) set it
__device__ __forceinline__ double normalize4(double q[4], bool* by_norm) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  *by_norm = n > kNormEps;
  const double inv = 1.0 / (*by_norm ? n : kNormEps);
  for (int i = 0; i < 4; ++i) q[i] *= inv;
  return inv;
}

// quaternion_rotate_vector on the rows of the identity (lib/pose_utils.py:30-45): R[i] = e_i + 2 (w u x e_i + u x (u x e_i))
__device__ __forceinline__ void rotation_rows(const double q[4], V3 R[3]) {
  const V3 u{q[1], q[2], q[3]};
  for (int i = 0; i < 3; ++i) {
    const V3 uv = cross(u, unit(i));
    R[i] = add(unit(i), mul(2.0, add(mul(q[0], uv), cross(u, uv))));
  }
}

// What both directions of pose_to_matrix share: the (normalised) quaternion, R, t3 and the scalars behind them.
struct PoseState {
  double q[4], inv_norm; bool by_norm;
  V3 R[3], t3;
  double s, e;          // e = exp(z0) (perspective)
};
__device__ __forceinline__ PoseState pose_state(const nfi_pose_args& a, int b) {
  PoseState p;
  for (int i = 0; i < 4; ++i) p.q[i] = a.q[(size_t)b * 4 + i];
  p.inv_norm = 1.0; p.by_norm = false;
  if (a.normalize_q) p.inv_norm = normalize4(p.q, &p.by_norm);
  rotation_rows(p.q, p.R);
  p.s = a.s[b];
  const double tx = a.t2[(size_t)b * 2], ty = a.t2[(size_t)b * 2 + 1];
  if (a.z0) {
    p.e = exp((double)a.z0[b]);
    p.t3 = {tx / p.s, ty / p.s, (1.0 + p.e) / p.s};
  } else {
    p.e = 0.0;
    p.t3 = {tx, ty, 10.0};
  }
  return p;
}

__global__ void __launch_bounds__(kThreads) pose_to_matrix_fwd_kernel(nfi_pose_args a) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= a.n_images) return;
  const PoseState p = pose_state(a, b);
  const double flip = a.camera_flipped ? -1.0 : 1.0;
  const double k = a.z0 ? 1.0 : 1.0 / p.s;          // the orthographic branch divides the whole matrix by s
  float* m = a.cam2world + (size_t)b * 16;
  for (int i = 0; i < 3; ++i) {
    m[i * 4 + 0] = (float)(p.R[i].x * k);
    m[i * 4 + 1] = (float)(flip * p.R[i].y * k);
    m[i * 4 + 2] = (float)(flip * p.R[i].z * k);
    m[i * 4 + 3] = (float)(flip * dot(p.t3, p.R[i]) * k);
  }
  m[12] = 0.0f; m[13] = 0.0f; m[14] = 0.0f; m[15] = (float)k;
  if (a.focal) a.focal[b] = (float)((1.0 + p.e) * 0.5);
}

__global__ void __launch_bounds__(kThreads) pose_to_matrix_bwd_kernel(nfi_pose_args a) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= a.n_images) return;
  const PoseState p = pose_state(a, b);
  const double flip = a.camera_flipped ? -1.0 : 1.0;
  const double k = a.z0 ? 1.0 : 1.0 / p.s;
  const float* g = a.g_cam2world + (size_t)b * 16;
  // cam2world[i] = k (R[i].x, flip R[i].y, flip R[i].z, flip t3 . R[i]); [3,3] = k
  V3 gR[3], g_t3{0.0, 0.0, 0.0};
  double g_k = g[15];                               // d cam2world[3,3] / d k = 1
  for (int i = 0; i < 3; ++i) {
    const double gx = g[i * 4], gy = flip * g[i * 4 + 1], gz = flip * g[i * 4 + 2], gt = flip * g[i * 4 + 3];
    g_k += gx * p.R[i].x + gy * p.R[i].y + gz * p.R[i].z + gt * dot(p.t3, p.R[i]);
    gR[i] = mul(k, add(V3{gx, gy, gz}, mul(gt, p.t3)));
    g_t3 = add(g_t3, mul(k * gt, p.R[i]));
  }
  double g_s, g_tx, g_ty, g_z0 = 0.0;
  if (a.z0) {                                       // t3 = (t2 / s, (1 + e) / s), focal = (1 + e) / 2
    const double g_f = g_t3.z / p.s + (a.g_focal ? 0.5 * (double)a.g_focal[b] : 0.0);
    g_tx = g_t3.x / p.s; g_ty = g_t3.y / p.s;
    g_s = -dot(g_t3, p.t3) / p.s;
    g_z0 = g_f * p.e;
  } else {                                          // t3 = (t2, 10), k = 1 / s
    g_tx = g_t3.x; g_ty = g_t3.y;
    g_s = -g_k * k * k;
  }
  if (a.g_t2) { a.g_t2[(size_t)b * 2] = (float)g_tx; a.g_t2[(size_t)b * 2 + 1] = (float)g_ty; }
  if (a.g_s) a.g_s[b] = (float)g_s;
  if (a.g_z0) a.g_z0[b] = (float)g_z0;
  if (!a.g_q) return;
  // R[i] = e_i + 2 (w uv + u x uv), uv = u x e_i;  for c = a x b: g_a = b x g_c, g_b = g_c x a
  const V3 u{p.q[1], p.q[2], p.q[3]};
  double g_w = 0.0;
  V3 g_u{0.0, 0.0, 0.0};
  for (int i = 0; i < 3; ++i) {
    const V3 uv = cross(u, unit(i)), g_uuv = mul(2.0, gR[i]);
    g_w += 2.0 * dot(gR[i], uv);
    const V3 g_uv = add(mul(2.0 * p.q[0], gR[i]), cross(g_uuv, u));
    g_u = add(g_u, add(cross(uv, g_uuv), cross(unit(i), g_uv)));
  }
  double gq[4] = {g_w, g_u.x, g_u.y, g_u.z};
  if (a.normalize_q) {                              // qn = q inv: through the norm, or through the constant 1 / eps
    const double along = p.by_norm ? gq[0] * p.q[0] + gq[1] * p.q[1] + gq[2] * p.q[2] + gq[3] * p.q[3] : 0.0;
    for (int i = 0; i < 4; ++i) gq[i] = p.inv_norm * (gq[i] - p.q[i] * along);
  }
  for (int i = 0; i < 4; ++i) a.g_q[(size_t)b * 4 + i] = (float)gq[i];
}

// matrix_to_quaternion, lib/pose_utils.py:73-95, of W = [[M, .], [0, 1]] (the fourth diagonal entry is 1)
__device__ __forceinline__ void quaternion_of(const double M[3][3], double q[4]) {
  double t = M[0][0] + M[1][1] + M[2][2] + 1.0;
  if (t > 1.0) {
    q[0] = t;
    q[3] = M[1][0] - M[0][1];
    q[2] = M[0][2] - M[2][0];
    q[1] = M[2][1] - M[1][2];
  } else {
    int i = 0, j = 1, k = 2;
    if (M[1][1] > M[0][0]) { i = 1; j = 2; k = 0; }
    if (M[2][2] > M[i][i]) { i = 2; j = 0; k = 1; }
    t = M[i][i] - (M[j][j] + M[k][k]) + 1.0;
    q[1 + i] = t;
    q[1 + j] = M[i][j] + M[j][i];
    q[1 + k] = M[k][i] + M[i][k];
    q[0] = M[k][j] - M[j][k];
  }
  const double scale = 0.5 / sqrt(t);
  for (int c = 0; c < 4; ++c) q[c] *= scale;
}

__global__ void __launch_bounds__(kThreads) matrix_to_pose_kernel(nfi_matrix_to_pose_args a) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= a.n_images) return;
  const float* m = a.cam2world + (size_t)b * 16;
  const double flip = a.camera_flipped ? -1.0 : 1.0;
  const double w = m[15];
  // invert_space, lib/pose_utils.py:20-27: W[:3,:3] = (A / w)^T, W[:3,3] = -(A / w)^T t
  double W[3][3];
  V3 t3{0.0, 0.0, 0.0};
  for (int i = 0; i < 3; ++i) {
    const double row[3] = {m[i * 4] / w, flip * m[i * 4 + 1] / w, flip * m[i * 4 + 2] / w};
    const double t = flip * m[i * 4 + 3];
    for (int j = 0; j < 3; ++j) W[j][i] = row[j];
    t3 = add(t3, mul(t, V3{row[0], row[1], row[2]}));          // t3 = -W[:3,3]
  }
  double s, z0 = 0.0, z0_cond = 0.0;
  if (a.focal) {
    const double f = a.focal[b];
    z0 = log(2.0 * f - 1.0);
    z0_cond = log(f);
    s = 2.0 * f / t3.z;
  } else {
    s = 1.0 / w;
  }
  const double tx = t3.x * s, ty = t3.y * s;
  if (a.z0) a.z0[b] = (float)z0;
  if (a.t2) { a.t2[(size_t)b * 2] = (float)tx; a.t2[(size_t)b * 2 + 1] = (float)ty; }
  if (a.s) a.s[b] = (float)s;
  if (a.q) {
    double q[4];
    quaternion_of(W, q);
    for (int c = 0; c < 4; ++c) a.q[(size_t)b * 4 + c] = (float)q[c];
  }
  if (a.cond) {
    float* c = a.cond + (size_t)b * 13;
    c[0] = (float)z0_cond; c[1] = (float)tx; c[2] = (float)ty; c[3] = (float)s;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) c[4 + i * 3 + j] = (float)W[i][j];
  }
}

// trace(P Q^T) of the 3 x 3 blocks = the sum of their elementwise products; dim 4: each block over its element [3,3]
__device__ __forceinline__ double angle_degrees(const float* p, const float* q, int dim) {
  double tr = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) tr += (double)p[i * dim + j] * (double)q[i * dim + j];
  if (dim == 4) tr /= (double)p[15] * (double)q[15];
  const double c = fmin(fmax((tr - 1.0) * 0.5, -1.0), 1.0);
  return acos(c) * kDegrees;
}

__global__ void __launch_bounds__(kThreads) rotation_distance_kernel(nfi_rotation_distance_args a) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= a.n_images) return;
  const size_t at = (size_t)b * a.dim * a.dim;
  a.degrees[b] = (float)angle_degrees(a.p + at, a.q + at, a.dim);
}

// Thread i walks every pose j in ascending order (all lanes read the same pose: one broadcast load each) and keeps the
// first j with the strictly smallest |distance - target|.
__global__ void __launch_bounds__(kThreads) pose_nearest_kernel(nfi_pose_nearest_args a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n_images) return;
  const float* mine = a.cam2world + (size_t)i * 16;
  const double target = a.target[i];
  int best = 0;
  double best_gap = fabs(angle_degrees(mine, a.cam2world, 4) - target);
  for (int j = 1; j < a.n_images; ++j) {
    const double gap = fabs(angle_degrees(mine, a.cam2world + (size_t)j * 16, 4) - target);
    if (gap < best_gap) { best_gap = gap; best = j; }
  }
  a.index[i] = best;
}

__global__ void __launch_bounds__(kThreads) pose_project_kernel(nfi_pose_project_args a) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= a.n_images) return;
  double q[4];
  bool by_norm;
  for (int i = 0; i < 4; ++i) q[i] = a.q[(size_t)b * 4 + i];
  normalize4(q, &by_norm);
  for (int i = 0; i < 4; ++i) a.q[(size_t)b * 4 + i] = (float)q[i];
  a.s[b] = fabsf(a.s[b]);
  if (a.z0) a.z0[b] = fminf(fmaxf(a.z0[b], -4.0f), 4.0f);
}

static inline dim3 grid_for(int n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

}  // namespace nfi_pose

extern "C" int nfi_pose_to_matrix_fwd(const nfi_pose_args* a, nfi_stream_t stream) {
  REQUIRE(a, "pose_to_matrix_fwd: null argument struct");
  REQUIRE(a->n_images > 0, "pose_to_matrix_fwd: n_images must be at least 1");
  REQUIRE(a->q && a->t2 && a->s && a->cam2world, "pose_to_matrix_fwd: null q / t2 / s / cam2world");
  REQUIRE(a->z0 || !a->focal, "pose_to_matrix_fwd: focal without z0 (the orthographic branch has no focal length)");
  hipLaunchKernelGGL(nfi_pose::pose_to_matrix_fwd_kernel, nfi_pose::grid_for(a->n_images), dim3(nfi_pose::kThreads), 0,
                     (hipStream_t)stream, *a);
  return check_launch("pose_to_matrix_fwd");
}

extern "C" int nfi_pose_to_matrix_bwd(const nfi_pose_args* a, nfi_stream_t stream) {
  REQUIRE(a, "pose_to_matrix_bwd: null argument struct");
  REQUIRE(a->n_images > 0, "pose_to_matrix_bwd: n_images must be at least 1");
  REQUIRE(a->q && a->t2 && a->s && a->g_cam2world, "pose_to_matrix_bwd: null q / t2 / s / g_cam2world");
  REQUIRE(a->z0 || !(a->g_focal || a->g_z0), "pose_to_matrix_bwd: g_focal / g_z0 without z0 (orthographic branch)");
  REQUIRE(a->g_q || a->g_t2 || a->g_s || a->g_z0, "pose_to_matrix_bwd: no gradient to write");
  hipLaunchKernelGGL(nfi_pose::pose_to_matrix_bwd_kernel, nfi_pose::grid_for(a->n_images), dim3(nfi_pose::kThreads), 0,
                     (hipStream_t)stream, *a);
  return check_launch("pose_to_matrix_bwd");
}

extern "C" int nfi_matrix_to_pose(const nfi_matrix_to_pose_args* a, nfi_stream_t stream) {
  REQUIRE(a, "matrix_to_pose: null argument struct");
  REQUIRE(a->n_images > 0, "matrix_to_pose: n_images must be at least 1");
  REQUIRE(a->cam2world, "matrix_to_pose: null cam2world");
  REQUIRE(a->focal || !a->z0, "matrix_to_pose: z0 without focal (the orthographic branch has no z0)");
  REQUIRE(a->z0 || a->t2 || a->s || a->q || a->cond, "matrix_to_pose: no output to write");
  hipLaunchKernelGGL(nfi_pose::matrix_to_pose_kernel, nfi_pose::grid_for(a->n_images), dim3(nfi_pose::kThreads), 0,
                     (hipStream_t)stream, *a);
  return check_launch("matrix_to_pose");
}

extern "C" int nfi_rotation_distance(const nfi_rotation_distance_args* a, nfi_stream_t stream) {
  REQUIRE(a, "rotation_distance: null argument struct");
  REQUIRE(a->n_images > 0, "rotation_distance: n_images must be at least 1");
  REQUIRE(a->dim == 3 || a->dim == 4, "rotation_distance: dim must be 3 or 4");
  REQUIRE(a->p && a->q && a->degrees, "rotation_distance: null p / q / degrees");
  hipLaunchKernelGGL(nfi_pose::rotation_distance_kernel, nfi_pose::grid_for(a->n_images), dim3(nfi_pose::kThreads), 0,
                     (hipStream_t)stream, *a);
  return check_launch("rotation_distance");
}

extern "C" int nfi_pose_nearest_by_angle(const nfi_pose_nearest_args* a, nfi_stream_t stream) {
  REQUIRE(a, "pose_nearest_by_angle: null argument struct");
  REQUIRE(a->n_images > 0, "pose_nearest_by_angle: n_images must be at least 1");
  REQUIRE(a->cam2world && a->target && a->index, "pose_nearest_by_angle: null cam2world / target / index");
  hipLaunchKernelGGL(nfi_pose::pose_nearest_kernel, nfi_pose::grid_for(a->n_images), dim3(nfi_pose::kThreads), 0,
                     (hipStream_t)stream, *a);
  return check_launch("pose_nearest_by_angle");
}

extern "C" int nfi_pose_project(const nfi_pose_project_args* a, nfi_stream_t stream) {
  REQUIRE(a, "pose_project: null argument struct");
  REQUIRE(a->n_images > 0, "pose_project: n_images must be at least 1");
  REQUIRE(a->q && a->s, "pose_project: null q / s");
  hipLaunchKernelGGL(nfi_pose::pose_project_kernel, nfi_pose::grid_for(a->n_images), dim3(nfi_pose::kThreads), 0,
                     (hipStream_t)stream, *a);
  return check_launch("pose_project");
}
