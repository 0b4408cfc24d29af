// Host-side plumbing shared by the translation units of libnfi_hip.so (nfi_kernels.hip, nfi_backward_field.hip, nfi_modules.hip):
// error buffer behind nfi_last_error(), argument checks, and the device helpers that stage the decoder image in LDS.
#pragma once
#include "nfi_device.hpp"
#include "../../include/nfi_hip.h"

#include <atomic>
#include <cstdio>
#include <initializer_list>
#include <type_traits>

extern thread_local char nfi_err_buf[256];          // defined in nfi_kernels.hip

static inline int fail(int code, const char* msg) {
  snprintf(nfi_err_buf, sizeof(nfi_err_buf), "%s", msg);
  return code;
}
static inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(nfi_err_buf, sizeof(nfi_err_buf), "%s: %s", what, hipGetErrorString(e));
    return NFI_ERR_LAUNCH;
  }
  return NFI_OK;
}

// Raises Kernel's dynamic-LDS limit to `bytes` - the LARGEST size any launch of that kernel uses, a constant - once per
// device.  The attribute is process-global per kernel and device; because the value never changes, host threads
// launching concurrently (one per GPU under nn.DataParallel) cannot lower it under each other (two that race both
// write the same value), and a failure is reported instead of surfacing as a failed launch later.
// One flag per kernel - the function's own static - with one bit per device.
template <auto Kernel>
static int ensure_dynamic_lds(size_t bytes, const char* what) {
  static std::atomic<unsigned long long> done{0};
  int dev = 0;
  const char* failed = hipGetDevice(&dev) != hipSuccess ? "hipGetDevice" : nullptr;
  const unsigned long long bit = 1ull << (dev & 63);
  if (!failed && !(done.load(std::memory_order_acquire) & bit)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess)
      done.fetch_or(bit, std::memory_order_release);
    else
      failed = "hipFuncSetAttribute(MaxDynamicSharedMemorySize)";
  }
  if (!failed) return NFI_OK;
  snprintf(nfi_err_buf, sizeof(nfi_err_buf), "%s: %s failed", what, failed);
  return NFI_ERR_LAUNCH;
}

#define REQUIRE(cond, msg) \
  do {                     \
    if (!(cond)) return fail(NFI_ERR_INVALID_ARGUMENT, msg); \
  } while (0)

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }      // where a workspace region may start
static inline int texel_bytes(int dtype) { return dtype == NFI_TEXEL_F32 ? 128 : 64; }

// The run-time -> compile-time step of the kernel dispatchers: calls f(std::integral_constant<int, TEX>, std::bool_constant<ATT>)
// with the kernels' TEX argument of `texel_dtype` (0 fp32, 1 bf16, 2 fp16; the type was checked by check_field_common)
// and ATT = the decoder has attention values.  f is a generic lambda; all six calls must return the same type.
template <class F>
static auto dispatch_texel_att(int texel_dtype, bool att, F&& f) {
  auto with_tex = [&](auto tex) { return att ? f(tex, std::true_type{}) : f(tex, std::false_type{}); };
  if (texel_dtype == NFI_TEXEL_F32) return with_tex(std::integral_constant<int, 0>{});
  if (texel_dtype == NFI_TEXEL_BF16) return with_tex(std::integral_constant<int, 1>{});
  return with_tex(std::integral_constant<int, 2>{});
}

// The canonical name of a kernel instantiation - the template's name with every argument as an integer, in order, e.g.
// "render_fwd_kernel<0,1,2,0,1,0>" - built at compile time from the arguments the dispatchers instantiate the kernel
// with (what nfi_render_kernel_name / nfi_field_kernel_name / nfi_field_bwd_kernel_name return: static storage).
struct KernelNameText { char s[64]; };
constexpr KernelNameText make_kernel_name(const char* family, std::initializer_list<int> args) {
  KernelNameText t{};
  int n = 0;
  for (const char* p = family; *p; ++p) t.s[n++] = *p;
  t.s[n++] = '<';
  bool first = true;
  for (int v : args) {           // template arguments of the kernels: never negative
    if (!first) t.s[n++] = ',';
    first = false;
    char digits[12] = {};
    int m = 0;
    do { digits[m++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (m) t.s[n++] = digits[--m];
  }
  t.s[n++] = '>';
  t.s[n] = 0;
  return t;
}
// Family: a constexpr char array of static storage (the template's name)
template <const char* Family, int... Args>
struct KernelName { static constexpr KernelNameText value = make_kernel_name(Family, {Args...}); };

static inline int check_field_common(const void* texels, int plane_res, int texel_dtype, const float* image, int A,
                              const float* att, int use_sdf, const float* beta, const float* alpha, int layout = 0) {
  REQUIRE(layout == NFI_TEXELS_PLANAR || layout == NFI_TEXELS_INTERLEAVED, "field: bad texel layout");
  REQUIRE(texels && image, "field: null texels / decoder image");
  REQUIRE(plane_res >= 2 && plane_res <= 1024, "field: plane_res must be in [2,1024]");
  REQUIRE(texel_dtype >= NFI_TEXEL_F32 && texel_dtype <= NFI_TEXEL_F16, "field: bad texel dtype");
  REQUIRE(A >= 0 && A <= NFI_MAX_ATTENTION, "field: attention_values must be in [0,14]");
  REQUIRE(A == 0 || att, "field: attention_values tensor missing");
  REQUIRE(!use_sdf || (beta && alpha), "field: use_sdf needs beta and alpha");
  return NFI_OK;
}

// The ordered modes' sort (defined in nfi_backward_field.inc, also called by nfi_regulariser.inc): a stable 8-bit radix sort
// of 64-bit keys (cell << 32 | point) by cell, `segments` runs of P keys each.  Enqueues on `s`, allocates nothing.
struct OrdSortPlan { int blocks, passes; size_t hist_bytes; };      // sort blocks per segment, passes, bytes of `hist`
OrdSortPlan ord_sort_plan(int64_t P, int segments, int res);
uint64_t* ord_sort_by_cell(uint64_t* keys, uint64_t* spare, uint32_t* hist, int64_t P, int segments, int res, hipStream_t s);

namespace nfi {

// stage the decoder image (+ this scene's attention values in accumulator layout) into LDS
__device__ __forceinline__ void stage_field_lds(float* lds, const float* image, const float* att_scene, int A,
                                                int n_image = kLdsImageFloats) {
  for (int i = threadIdx.x; i < n_image; i += blockDim.x) lds[i] = image[i];
  for (int i = threadIdx.x; i < 64; i += blockDim.x) {
    int c = i & 3, row = i >> 2;  // row = 4g + r; value for feature row-1
    float v = 0.0f;
    if (att_scene && c < 3 && row >= 1 && row <= A) v = att_scene[(row - 1) * 3 + c];
    lds[n_image + i] = v;
  }
}

__device__ __forceinline__ FieldParams make_field_params(const void* texels_scene, int res, int tex, int A, int use_sdf,
                                                         const float* beta, const float* alpha, const float* lds,
                                                         int n_image = kLdsImageFloats, int layout = 0) {
  FieldParams P;
  uint32_t tb = tex == 0 ? 128u : 64u;
  P.scene_bytes = 3u * (uint32_t)res * (uint32_t)res * tb;
  P.pix_bytes = layout ? 3u * tb : tb;
  P.plane_bytes = layout ? tb : (uint32_t)res * (uint32_t)res * tb;
  P.row_bytes = (uint32_t)res * P.pix_bytes;
  P.row_pix_bytes = P.row_bytes + P.pix_bytes;
  P.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(texels_scene), 0, (int)P.scene_bytes, 0x00020000);
  P.res = res;
  P.res_m1 = (float)(res - 1);
  P.n_attention = A;
  P.use_sdf = use_sdf;
  P.inv_alpha = use_sdf ? 1.0f / alpha[0] : 1.0f;
  P.beta = use_sdf ? beta[0] : 1.0f;
  P.neg_log2e_over_beta = -kLog2e / P.beta;
  P.lds = lds;
  P.vf = lds + n_image;
  return P;
}

}  // namespace nfi
