// nfi_rays.inc — ray set-up: ray generation with the scene cube's near / far planes and their batch-wide reduction
// (nfi_raygen, nfi_near_far), stratified depths and query points (nfi_points_on_rays, nfi_stratified_points)
// (included by nfi_kernels.hip).  Expects nfi_host.hpp and `using namespace nfi`.  The render uses what is defined here:
// raygen_kernel, RayPartial / kRayBlocks and block_reduce_keys in its set-up (nfi_render_host.inc), finish_planes and
// stratified_depth per ray in its kernels.

// ------------------------------------------------------------------------------------------------
// rays + scene-cube planes
// ------------------------------------------------------------------------------------------------
// reduce[0] = ~key(min near | hit) (so that zero-initialised memory + atomicMax works),
// reduce[1] = key(max far | hit), reduce[2] = hit count.
// Per-thread accumulators (a thread may have seen several rays): kmin/kmax keys as above, cnt = its hit count.
// block_reduce_keys leaves the block's totals in thread 0's arguments.  From there
//   raygen_kernel (the render's ray set-up) stores them as its block's RayPartial, and the one-block raygen_finish_kernel
//     behind it reduces the partials into reduce[] with plain stores: no cell has to be clear beforehand, no atomic;
//   slab_kernel (nfi_near_far) sends them to the three cells with atomics.  They all go to the same three addresses, and
//     same-address device atomics serialise at ~12 ns on this chip, so it runs a grid-stride loop over at most kSlabBlocks
//     blocks.
// kRayBlocks bounds raygen_kernel's grid, hence the partials (one thread per ray up to 262 144 rays, a grid-stride loop
// beyond).
constexpr int kSlabBlocks = 256;
constexpr int kRayBlocks = 1024;
struct RayPartial { uint32_t kmin, kmax, cnt, pad; };
__device__ __forceinline__ void block_reduce_keys(uint32_t& kmin, uint32_t& kmax, uint32_t& cnt) {
  __shared__ uint32_t s_min[4], s_max[4], s_cnt[4];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    uint32_t a = (uint32_t)__shfl_xor((int)kmin, d, 64), b = (uint32_t)__shfl_xor((int)kmax, d, 64);
    kmin = a > kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
    cnt += (uint32_t)__shfl_xor((int)cnt, d, 64);
  }
  int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_min[wave] = kmin; s_max[wave] = kmax; s_cnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    int nw = blockDim.x >> 6;
    for (int w = 1; w < nw; ++w) {
      kmin = s_min[w] > kmin ? s_min[w] : kmin;
      kmax = s_max[w] > kmax ? s_max[w] : kmax;
      cnt += s_cnt[w];
    }
  }
}

struct RaygenOut {
  float* ro; float* rd;          // [N,3] or null
  float* near_raw; float* far_raw; uint8_t* hit;  // [N] or null (null near_raw -> no slab test)
  RayPartial* partial;           // [gridDim.x] (with near_raw)
  float scene_range;
};

__global__ __launch_bounds__(256) void raygen_kernel(CameraParams cam, int n_scenes, RaygenOut out) {
  const int hw = cam.rows * cam.width;
  const int64_t n = (int64_t)n_scenes * hw;
  uint32_t kmin = 0u, kmax = 0u, cnt = 0u;
  for (int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ray < n; ray += (int64_t)gridDim.x * blockDim.x) {
    int b = (int)(ray / hw);
    int pix = (int)(ray - (int64_t)b * hw);
    int row = pix / cam.width, col = pix - row * cam.width;
    float o[3], d[3];
    make_ray(cam, b, cam.row0 + row, col, o, d);
    if (out.ro) { out.ro[ray * 3 + 0] = o[0]; out.ro[ray * 3 + 1] = o[1]; out.ro[ray * 3 + 2] = o[2]; }
    if (out.rd) { out.rd[ray * 3 + 0] = d[0]; out.rd[ray * 3 + 1] = d[1]; out.rd[ray * 3 + 2] = d[2]; }
    if (out.near_raw) {
      float near = 0.0f, far = 0.0f;
      const bool hit = slab_test(o, d, out.scene_range, near, far);
      // second, inflated test: lets the fused renderer skip rays that provably never enter the cube
      float n2, f2;
      bool hit_wide = slab_test(o, d, out.scene_range * 1.0001f, n2, f2);
      out.near_raw[ray] = near;
      out.far_raw[ray] = far;
      out.hit[ray] = (uint8_t)((hit ? 1 : 0) | (hit_wide ? 2 : 0));
      if (hit) {
        const uint32_t a = ~ordered_key(near), c = ordered_key(far);   // maximise the complement of the near key
        kmin = a > kmin ? a : kmin;
        kmax = c > kmax ? c : kmax;
        ++cnt;
      }
    }
  }
  if (out.near_raw) {
    block_reduce_keys(kmin, kmax, cnt);
    if (threadIdx.x == 0) out.partial[blockIdx.x] = RayPartial{kmin, kmax, cnt, 0u};
  }
}

__global__ __launch_bounds__(256) void slab_kernel(const float* __restrict__ ro, const float* __restrict__ rd, int64_t n,
                                                   float scene_range, float* __restrict__ near_raw,
                                                   float* __restrict__ far_raw, uint8_t* __restrict__ hit_out,
                                                   uint32_t* reduce) {
  uint32_t kmin = 0u, kmax = 0u, cnt = 0u;
  for (int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ray < n; ray += (int64_t)gridDim.x * blockDim.x) {
    float o[3] = {ro[ray * 3], ro[ray * 3 + 1], ro[ray * 3 + 2]};
    float d[3] = {rd[ray * 3], rd[ray * 3 + 1], rd[ray * 3 + 2]};
    float near = 0.0f, far = 0.0f;
    const bool hit = slab_test(o, d, scene_range, near, far);
    float n2, f2;
    bool hit_wide = slab_test(o, d, scene_range * 1.0001f, n2, f2);
    near_raw[ray] = near;
    far_raw[ray] = far;
    hit_out[ray] = (uint8_t)((hit ? 1 : 0) | (hit_wide ? 2 : 0));
    if (hit) {
      const uint32_t a = ~ordered_key(near), c = ordered_key(far);
      kmin = a > kmin ? a : kmin;
      kmax = c > kmax ? c : kmax;
      ++cnt;
    }
  }
  block_reduce_keys(kmin, kmax, cnt);
  if (threadIdx.x == 0 && cnt) {
    atomicMax(&reduce[0], kmin);
    atomicMax(&reduce[1], kmax);
    atomicAdd(&reduce[2], cnt);
  }
}

__global__ __launch_bounds__(256) void finish_planes_kernel(const float* __restrict__ near_raw,
                                                            const float* __restrict__ far_raw,
                                                            const uint8_t* __restrict__ hit, const uint32_t* __restrict__ reduce,
                                                            int64_t n, float* __restrict__ near_plane,
                                                            float* __restrict__ far_plane) {
  const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ray >= n) return;
  float fill_near = ordered_key_inv(~reduce[0]), fill_far = ordered_key_inv(reduce[1]);
  float a = near_raw[ray], b = far_raw[ray];
  finish_planes((hit[ray] & 1) != 0, fill_near, fill_far, a, b);
  near_plane[ray] = a;
  far_plane[ray] = b;
}

extern "C" int nfi_raygen(const nfi_raygen_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->cam2world && a->ray_origins && a->ray_directions, "raygen: null pointer");
  REQUIRE(a->n_scenes > 0 && a->height > 0 && a->width > 0, "raygen: bad shape");
  CameraParams cam{a->cam2world, a->focal, a->bbox, a->focal ? a->center : nullptr, a->height, a->width, a->normalize, a->height, 0};
  RaygenOut out{a->ray_origins, a->ray_directions, nullptr, nullptr, nullptr, nullptr, 0.0f};
  int64_t n = (int64_t)a->n_scenes * a->height * a->width;
  hipLaunchKernelGGL(raygen_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, kRayBlocks)), dim3(256), 0, (hipStream_t)stream, cam,
                     a->n_scenes, out);
  return check_launch("raygen");
}

extern "C" int nfi_near_far(const nfi_near_far_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->ray_origins && a->ray_directions && a->near_raw && a->far_raw && a->hit && a->reduce,
          "near_far: null pointer");
  REQUIRE(a->n_rays > 0, "near_far: no rays");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(a->reduce, 0, 16, s) != hipSuccess) return fail(NFI_ERR_LAUNCH, "near_far: memset failed");
  unsigned blocks = (unsigned)((a->n_rays + 255) / 256);
  hipLaunchKernelGGL(slab_kernel, dim3(std::min<unsigned>(blocks, kSlabBlocks)), dim3(256), 0, s, a->ray_origins, a->ray_directions, a->n_rays,
                     a->scene_range, a->near_raw, a->far_raw, a->hit, a->reduce);
  if (a->near_plane && a->far_plane)
    hipLaunchKernelGGL(finish_planes_kernel, dim3(blocks), dim3(256), 0, s, a->near_raw, a->far_raw, a->hit, a->reduce,
                       a->n_rays, a->near_plane, a->far_plane);
  return check_launch("near_far");
}

// ------------------------------------------------------------------------------------------------
// stratified depths + query points (lib/nerf_utils.py:94-120)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float stratified_depth(float near, float far, int k, int S, float noise, bool jitter) {
  float t = aten_lerp(near, far, (float)k / (float)S);
  if (jitter) t = t + noise * ((far - near) / (float)S);
  return t;
}

__global__ __launch_bounds__(256) void stratified_kernel(nfi_stratified_args a) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = a.n_rays * a.n_samples;
  if (idx >= total) return;
  const int64_t ray = idx / a.n_samples;
  const int k = (int)(idx - ray * a.n_samples);
  float near = a.near_plane[ray], far = a.far_plane[ray];
  float t = stratified_depth(near, far, k, a.n_samples, a.noise ? a.noise[idx] : 0.0f, a.noise != nullptr);
  a.depth[idx] = t;
  if (a.points) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.points[idx * 3 + c] = a.ray_origins[ray * 3 + c] + a.ray_directions[ray * 3 + c] * t;
  }
}

__global__ __launch_bounds__(256) void points_on_rays_kernel(const float* __restrict__ ro, const float* __restrict__ rd,
                                                             const float* __restrict__ depth, int64_t total, int S,
                                                             float* __restrict__ points) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int64_t ray = idx / S;
  const float t = depth[idx];
#pragma unroll
  for (int c = 0; c < 3; ++c) points[idx * 3 + c] = ro[ray * 3 + c] + rd[ray * 3 + c] * t;
}

extern "C" int nfi_points_on_rays(const float* ray_origins, const float* ray_directions, const float* depth,
                                  int64_t n_rays, int n_samples, float* points, nfi_stream_t stream) {
  REQUIRE(ray_origins && ray_directions && depth && points, "points_on_rays: null pointer");
  REQUIRE(n_rays > 0 && n_samples > 0, "points_on_rays: bad shape");
  int64_t total = n_rays * n_samples;
  hipLaunchKernelGGL(points_on_rays_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ray_origins, ray_directions, depth, total, n_samples, points);
  return check_launch("points_on_rays");
}

extern "C" int nfi_stratified_points(const nfi_stratified_args* a, nfi_stream_t stream) {
  REQUIRE(a && a->ray_origins && a->ray_directions && a->near_plane && a->far_plane && a->depth, "stratified: null pointer");
  REQUIRE(a->n_rays > 0 && a->n_samples > 0, "stratified: bad shape");
  int64_t total = a->n_rays * a->n_samples;
  hipLaunchKernelGGL(stratified_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
  return check_launch("stratified_points");
}
