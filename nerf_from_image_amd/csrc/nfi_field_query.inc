// nfi_field_query.inc — the field query forward as a kernel of its own (nfi_field_query_fwd, nfi_field_kernel_name) and
// the bounding-box overlay on its densities (nfi_bbox_overlay) (included by nfi_kernels.hip).  Expects nfi_host.hpp
// (stage_field_lds, make_field_params, dispatch_texel_att, KernelName) and `using namespace nfi`; the field march itself
// is nfi_device.hpp's.  Its backward is the other translation unit, nfi_backward_field.hip.

// ------------------------------------------------------------------------------------------------
// field query (sampler closure)
// ------------------------------------------------------------------------------------------------
struct FieldKernelParams {
  const float* points; int64_t P;
  const void* texels; int res; int tex;
  const float* image; int A; const float* att;
  int use_sdf; const float* beta; const float* alpha; float scene_range;
  float* sigma; float* rgb; float* sdf; float* sem; uint8_t* outside;
  const float* xray; int spr;
  int layout;
};

// PREC: 0 = exact fp32 MFMA (the sampler closure's default: bitwise an fmaf chain), 1 = split-fp16 operands as in the
// fused renderer (render()'s differentiable path: the same decoder arithmetic in both of its paths, and what the
// backward kernel recomputes)
static_assert(kOutLastRow == NFI_MAX_ATTENTION, "sample_epilogue reads rows 1 .. NFI_MAX_ATTENTION of the output table");
template <int TEX, bool ATT, bool VD = false, int PREC = 0>
__global__ __launch_bounds__(256) void field_query_kernel(FieldKernelParams k) {
  constexpr int kImg = VD ? kVdImageFloats : kLdsImageFloats;
  __shared__ __attribute__((aligned(16))) float lds[kImg + 64];
  __shared__ __attribute__((aligned(16))) float stages[4][16 * 36];
  const int scene = blockIdx.y;
  stage_field_lds(lds, k.image, k.att ? k.att + (size_t)scene * k.A * 3 : nullptr, k.A, kImg);
  if (PREC == 1) {
    // fp16 fragments overlay the fp32 fragment area; biases stay where they are
    __syncthreads();
    for (int i = threadIdx.x; i < kB1F; i += blockDim.x) lds[i] = k.image[kW1H + i];
  }
  __syncthreads();
  const size_t tb = TEX == 0 ? 128 : 64;
  const char* tex_scene = reinterpret_cast<const char*>(k.texels) + (size_t)scene * 3 * k.res * k.res * tb;
  FieldParams P = make_field_params(tex_scene, k.res, TEX, k.A, k.use_sdf, k.beta, k.alpha, lds, kImg, k.layout);
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t n_chunks = (k.P + 63) / 64;
  const float* xray_scene = VD ? k.xray + (size_t)scene * (size_t)(k.P / k.spr) * kRayFeatPad : nullptr;
  for (int64_t chunk = (int64_t)blockIdx.x * 4 + wave; chunk < n_chunks; chunk += (int64_t)gridDim.x * 4) {
    int64_t p = chunk * 64 + lane;
    bool valid = p < k.P;
    size_t gi = (size_t)scene * k.P + (valid ? p : 0);
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (valid) { px = k.points[gi * 3]; py = k.points[gi * 3 + 1]; pz = k.points[gi * 3 + 2]; }
    bool out;
    float* sem = k.sem ? k.sem + ((size_t)scene * k.P + chunk * 64) * k.A : nullptr;
    // (the per-tile epilogue: the sample-layout one of the plain render kernels has not been timed here)
    SampleOut so = field_wave<TEX, ATT, false, PREC, VD, 0, false, false>(P, k.scene_range, lane, px, py, pz, valid, sem, &out,
                                                                          stages[wave], nullptr, nullptr, xray_scene,
                                                                          VD && valid ? (int)(p / k.spr) : 0);
    if (valid) {
      k.sigma[gi] = so.sigma;
      k.rgb[gi * 3] = so.r; k.rgb[gi * 3 + 1] = so.g; k.rgb[gi * 3 + 2] = so.b;
      if (k.sdf) k.sdf[gi] = so.sdf;
      if (k.outside) k.outside[gi] = out ? 1 : 0;
    }
  }
}

// The argument rules of nfi_field_query_fwd (pointers against null, integers against limits: nothing is dereferenced)
static int field_check_call(const nfi_field_args* a) {
  REQUIRE(a && a->points && a->sigma && a->rgb, "field_query: null pointer");
  REQUIRE(a->n_scenes > 0 && a->points_per_scene > 0, "field_query: bad shape");
  int rc = check_field_common(a->texels, a->plane_res, a->texel_dtype, a->decoder_image, a->n_attention,
                              a->attention_values, a->use_sdf, a->beta, a->alpha, a->texel_layout);
  if (rc) return rc;
  REQUIRE(!a->semantics || a->n_attention > 0, "field_query: semantics need attention_values > 0");
  REQUIRE(!a->ray_features || (a->samples_per_ray > 0 && a->points_per_scene % a->samples_per_ray == 0),
          "field_query: with ray_features, points_per_scene must be a multiple of samples_per_ray");
  REQUIRE(a->mlp_precision == 0 || (a->mlp_precision == 1 && !a->ray_features),
          "field_query: mlp_precision must be 0 (exact fp32) or 1 (split fp16; not with the view-direction decoder)");
  return NFI_OK;
}

// which field_query_kernel instantiation a (validated) call gets, and its canonical name
using FieldKernel = void (*)(FieldKernelParams);
struct FieldLaunch { FieldKernel kernel; const char* name; };
static constexpr char kFieldFamily[] = "field_query_kernel";
template <int TEX, bool ATT, bool VD = false, int PREC = 0>
static FieldLaunch field_launch() { return {&field_query_kernel<TEX, ATT, VD, PREC>, KernelName<kFieldFamily, TEX, ATT, VD, PREC>::value.s}; }

static FieldLaunch select_field_kernel(const nfi_field_args* a) {
  return dispatch_texel_att(a->texel_dtype, a->n_attention > 0, [&](auto tex, auto att_c) -> FieldLaunch {
    constexpr int TEX = decltype(tex)::value;
    constexpr bool ATT = decltype(att_c)::value;
    if (a->ray_features) return field_launch<TEX, ATT, true>();
    if (a->mlp_precision == 1) return field_launch<TEX, ATT, false, 1>();
    return field_launch<TEX, ATT>();
  });
}

extern "C" const char* nfi_field_kernel_name(const nfi_field_args* a) {
  if (field_check_call(a)) return nullptr;
  return select_field_kernel(a).name;
}

extern "C" int nfi_field_query_fwd(const nfi_field_args* a, nfi_stream_t stream) {
  int rc = field_check_call(a);
  if (rc) return rc;
  // (semantics rows are stored per valid point only: field_wave guards them with the lane's valid flag)
  FieldKernelParams k{a->points, a->points_per_scene, a->texels, a->plane_res, a->texel_dtype, a->decoder_image,
                      a->n_attention, a->attention_values, a->use_sdf, a->beta, a->alpha, a->scene_range,
                      a->sigma, a->rgb, a->sdf, a->semantics, a->outside, a->ray_features, a->samples_per_ray, a->texel_layout};
  int64_t chunks = (a->points_per_scene + 63) / 64;
  int64_t blocks = (chunks + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  dim3 grid((unsigned)blocks, (unsigned)a->n_scenes);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(select_field_kernel(a).kernel, grid, dim3(256), 0, s, k);
  return check_launch("field_query_fwd");
}

__global__ __launch_bounds__(256) void bbox_overlay_kernel(const float* __restrict__ points, int64_t n, float scene_range,
                                                           float thr, const float* __restrict__ sigma_in,
                                                           float* __restrict__ sigma_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
  const bool outside = (fabsf(x / scene_range) > 1.0f) || (fabsf(y / scene_range) > 1.0f) || (fabsf(z / scene_range) > 1.0f);
  const bool ix = fabsf(x) < thr, iy = fabsf(y) < thr, iz = fabsf(z) < thr;
  // generator.py:650-658: product of (1 - both-inside) over the axis pairs xy, xz, yz (the last one twice)
  float m = 1.0f;
  m *= 1.0f - ((ix && iy) ? 1.0f : 0.0f);
  m *= 1.0f - ((ix && iz) ? 1.0f : 0.0f);
  m *= 1.0f - ((iy && iz) ? 1.0f : 0.0f);
  m *= 1.0f - ((iy && iz) ? 1.0f : 0.0f);
  m *= 1.0f - (outside ? 1.0f : 0.0f);
  sigma_out[i] = sigma_in[i] + 100.0f * m;
}

extern "C" int nfi_bbox_overlay(const float* points, int64_t n_points, float scene_range, float threshold,
                                const float* sigma_in, float* sigma_out, nfi_stream_t stream) {
  REQUIRE(points && sigma_in && sigma_out && n_points > 0, "bbox_overlay: null pointer / empty");
  hipLaunchKernelGGL(bbox_overlay_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     points, n_points, scene_range, threshold, sigma_in, sigma_out);
  return check_launch("bbox_overlay");
}
