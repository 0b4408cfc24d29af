/*
 * nfi_hip.h — C ABI of libnfi_hip.so, the MI355X (gfx950) implementation of the
 * nerf-from-image volumetric-rendering hot path.
 *
 * The reference (google-research/nerf-from-image) has no FFI: the boundary of this
 * path is a set of Python callables.  Each entry point below names the reference
 * callable it replaces (file:line relative to the reference checkout); the Python
 * binding in nerf_from_image_amd/ calls these through ctypes and re-creates the
 * reference's call surface on top (lib/nerf_utils.py functions, the Generator
 * `sampler` closure, run.py::render).  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a CALLER-OWNED DEVICE pointer (HIP, same device as the
 *     stream) unless the field says "host"; nothing is allocated, nothing is
 *     synchronised, every launch goes to the caller's stream;
 *   - all entry points are re-entrant (no global mutable state): the reference
 *     calls this path concurrently from one thread per GPU (nn.DataParallel,
 *     run.py:636-640);
 *   - return value: 0 on success, a negative nfi_status otherwise;
 *     nfi_last_error() returns a thread-local message for the last failure;
 *   - tensors are dense row-major fp32 unless stated; "N" is the number of rays
 *     B*H*W, "S" the samples per ray and pass.
 */
#ifndef NFI_HIP_H
#define NFI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nfi_stream_t; /* hipStream_t */

typedef enum nfi_status {
  NFI_OK = 0,
  NFI_ERR_INVALID_ARGUMENT = -1,
  NFI_ERR_UNSUPPORTED = -2,
  NFI_ERR_WORKSPACE_TOO_SMALL = -3,
  NFI_ERR_LAUNCH = -4
} nfi_status;

enum { NFI_PLANE_CHANNELS = 32, NFI_HIDDEN = 64, NFI_MAX_ATTENTION = 14, NFI_MAX_SAMPLES = 128 };
/* NFI_MAX_SAMPLES: samples per ray and PASS of the two-pass (coarse + fine) pipeline and of the fused kernel.  A single
 * pass without fine sampling (run.py:512-514: 128 samples; the inversion loop asks for ray_multiplier = 4, run.py:2271)
 * can hold up to NFI_MAX_SAMPLES_SINGLE_PASS samples in nfi_ray_weights / nfi_composite_fwd / nfi_composite_bwd. */
enum { NFI_MAX_SAMPLES_SINGLE_PASS = 512 };

/* texel storage type of the channel-last plane image */
enum { NFI_TEXEL_F32 = 0, NFI_TEXEL_BF16 = 1, NFI_TEXEL_F16 = 2 };
/* texel layout (`texel_layout` fields; 0 = default).  A texel = the 32 channels of one plane at one (y,x):
 *   PLANAR       [B,3,R,R,32]   written by nfi_planes_to_texels from the reference's NCHW planes;
 *   INTERLEAVED  [B,R,R,3,32]   = a channels-last (NHWC) [B,96,R,R] image, i.e. what a producer that emits
 *                               torch.channels_last - or nfi_torgb_texels_fwd - leaves in memory: read in place,
 *                               no hand-off kernel; gradient images use the layout of their texels. */
enum { NFI_TEXELS_PLANAR = 0, NFI_TEXELS_INTERLEAVED = 1 };
/* Pointers.  The ABI sees addresses, not strides: every array is DENSE in the shape its comment gives, on the device of
 * the stream, and as long as that shape says - none of which an entry can check.  Alignment: `texels` and `g_texels`
 * (every entry that has them: the field query, the fused render, the distance-gradient operator, their backwards) are
 * gathered and scattered as 16-byte vectors and must be 16-byte aligned, as must the arguments named under "Alignment"
 * at an entry; for every other float array, 16-byte alignment is the only one the kernels are tested with (a row of a
 * fresh allocation).  nerf_from_image_amd/ops.py guarantees all of this for its callers: it refuses a tensor of the
 * wrong type, device or length and copies one that is not dense or whose first byte is not on a multiple of 16. */

const char* nfi_last_error(void);
int nfi_version(void);

/* ------------------------------------------------------------------------------------------
 * Triplane hand-off: NCHW planes from the synthesis network -> channel-last texels.
 * Replaces the implicit layout the reference gathers from (models/generator.py:475-477,
 * 501-503: planes.view(B,3,32,R,R); F.grid_sample reads NCHW).  A texel (32 channels) becomes
 * one 128-byte line (fp32) / 64-byte line (bf16).
 *   planes  [B,3,32,R,R] fp32      texels  [B,3,R,R,32] fp32|bf16
 *   Alignment: planes and texels (both entries) are accessed as 16-byte vectors and must be 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int nfi_planes_to_texels(const float* planes, void* texels, int n_scenes, int plane_res,
                         int texel_dtype, nfi_stream_t stream);
/* adjoint of the above (fp32 only): texel-layout gradient -> NCHW gradient */
int nfi_texels_to_planes(const float* texels, float* planes, int n_scenes, int plane_res,
                         nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Decoder operand image.  Replaces the per-call weight scaling of EqualizedLinear
 * (models/stylegan.py:173-180: W * 1/sqrt(in), b * 1) for TriplanarDecoder.net
 * (models/generator.py:295-299): folds the gains, the /3 of the plane mean
 * (generator.py:328) and the exp2/log2 change of base into a lane-ordered MFMA operand image.
 *   w1 [64,32]  b1 [64]  w2 [n_out,64]  b2 [n_out]   (raw parameters, n_out = 1+A, or 4 if A==0)
 *   image: nfi_decoder_image_floats() floats
 * ------------------------------------------------------------------------------------------ */
size_t nfi_decoder_image_floats(void);
int nfi_decoder_pack(const float* w1, const float* b1, const float* w2, const float* b2,
                     int n_attention, int texel_dtype, float* image, nfi_stream_t stream);

/* View-direction variant (--use_viewdir; ViewDirectionMapper, models/generator.py:189-253; decoder output
 * widened to 32 features, 376-377; closure applied per sample, 243-251 / 662-663):
 *   w2 [33,64] b2 [33] (row 0 = distance, rows 1..32 = features);  w3 [n3,32] b3 [n3] = the mapper's
 *   `output` EqualizedLinear (raw parameters), n3 = A, or 3 if A == 0.
 * The per-ray output of ViewDirectionMapper.fc6 is handed to the field / render entry points as
 * ray_features [rays, NFI_RAY_FEATURE_PITCH] = [0, x_0 .. x_31, 0 x 15] (padded by the caller). */
enum { NFI_RAY_FEATURE_PITCH = 48 };
size_t nfi_decoder_image_floats_viewdir(void);
int nfi_decoder_pack_viewdir(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                             const float* b3, int n_attention, int texel_dtype, float* image, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Camera rays + scene-box intersection.
 * Replaces nerf_utils.get_ray_bundle (lib/nerf_utils.py:28-91), F.normalize (run.py:196)
 * and nerf_utils.compute_near_far_planes (lib/nerf_utils.py:225-273).
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_raygen_args {
  int n_scenes, height, width;
  const float* cam2world;   /* [B,4,4] */
  const float* focal;       /* [B] or NULL -> orthographic model (nerf_utils.py:66-89) */
  const float* bbox;        /* [B,2,2] or NULL */
  const float* center;      /* [B,2] or NULL (perspective only) */
  int normalize;            /* 1: ray directions L2-normalised (run.py:196) */
  float* ray_origins;       /* [N,3] out */
  float* ray_directions;    /* [N,3] out */
} nfi_raygen_args;
int nfi_raygen(const nfi_raygen_args* a, nfi_stream_t stream);

typedef struct nfi_near_far_args {
  int64_t n_rays;
  const float* ray_origins;    /* [N,3] */
  const float* ray_directions; /* [N,3] */
  float scene_range;
  float* near_raw;  /* [N] out: slab entry distance before the miss-fill / clamps */
  float* far_raw;   /* [N] out */
  uint8_t* hit;     /* [N] out: 1 if the ray's line meets the cube */
  uint32_t* reduce; /* [4] out: order-preserving keys of min(near|hit), max(far|hit), hit count, 0 */
  /* optional: finished planes (miss-fill with the batch-wide min/max, clamp >= 0.1,
   * far-near >= 1e-3; nerf_utils.py:258-268).  NULL to skip. */
  float* near_plane; /* [N] out or NULL */
  float* far_plane;  /* [N] out or NULL */
} nfi_near_far_args;
int nfi_near_far(const nfi_near_far_args* a, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Stratified depths + query points.  Replaces nerf_utils.compute_query_points_from_rays
 * (lib/nerf_utils.py:94-120).  noise: the reference's torch.rand_like draw, or NULL.
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_stratified_args {
  int64_t n_rays;
  int n_samples;
  const float* ray_origins;    /* [N,3] */
  const float* ray_directions; /* [N,3] */
  const float* near_plane;     /* [N] */
  const float* far_plane;      /* [N] */
  const float* noise;          /* [N,S] in [0,1) or NULL */
  float* depth;                /* [N,S] out */
  float* points;               /* [N,S,3] out */
} nfi_stratified_args;
int nfi_stratified_points(const nfi_stratified_args* a, nfi_stream_t stream);
/* x = o + d*t for given depths (the fine query points, run.py:286-288).
 * ray_origins/ray_directions [N,3], depth [N,S] -> points [N,S,3] */
int nfi_points_on_rays(const float* ray_origins, const float* ray_directions, const float* depth,
                       int64_t n_rays, int n_samples, float* points, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Field query: the `sampler` closure of Generator.forward (models/generator.py:587-681) with
 * TriplanarDecoder.forward (301-331), laplace_cdf (30-33) and the colour head (661-679).
 *   points [B,P,3] world coordinates -> sigma [B,P], rgb [B,P,3], optional sdf [B,P]
 *   (raw decoder output 0), semantics [B,P,A] (softmax probabilities), outside [B,P] (u8).
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_field_args {
  int n_scenes;
  int64_t points_per_scene;
  const float* points;           /* [B,P,3] */
  const void* texels;            /* [B,3,R,R,32] */
  int plane_res;
  int texel_dtype;
  const float* decoder_image;    /* from nfi_decoder_pack (same texel_dtype, same n_attention) */
  int n_attention;               /* A; 0 -> rgb = wide sigmoid of 3 features */
  const float* attention_values; /* [B,A,3] (A>0) */
  int use_sdf;                   /* 1: sigma = laplace_cdf(-d,beta)/alpha; 0: softplus(d-1) */
  const float* beta;             /* device scalar (use_sdf) */
  const float* alpha;            /* device scalar (use_sdf) */
  float scene_range;
  float* sigma;                  /* [B,P] out */
  float* rgb;                    /* [B,P,3] out */
  float* sdf;                    /* [B,P] out or NULL */
  float* semantics;              /* [B,P,A] out or NULL */
  uint8_t* outside;              /* [B,P] out or NULL */
  /* view-direction decoder: NULL, or [B, P/samples_per_ray, NFI_RAY_FEATURE_PITCH]; decoder_image must then
   * come from nfi_decoder_pack_viewdir and point p belongs to ray p / samples_per_ray (x_in [B,H,W,S,3]) */
  const float* ray_features;
  int samples_per_ray;
  int texel_layout;              /* NFI_TEXELS_PLANAR (0) / NFI_TEXELS_INTERLEAVED */
  int mlp_precision;             /* 0: exact fp32 MFMA (default); 1: split-fp16 operands with fp32 accumulation, the fused
                                  * renderer's decoder arithmetic (sigma within 3e-5 relative of mode 0) */
} nfi_field_args;
int nfi_field_query_fwd(const nfi_field_args* a, nfi_stream_t stream);
/* Which kernel nfi_field_query_fwd launches for *a: the canonical name of the instantiation - the template's name with
 * every argument as an integer, "field_query_kernel<TEX,ATT,VD,PREC>" - in static storage, or NULL (nfi_last_error()
 * says why) for a call the argument rules refuse.  Host only: the same rules and the same selection code as the launch,
 * no HIP call, no pointer of *a is dereferenced (usable without a GPU, with placeholder pointers). */
const char* nfi_field_kernel_name(const nfi_field_args* a);

/* 'bbox' visualisation overlay of the sampler closure (models/generator.py:645-659, only with 'coords' in the
 * sampler request and 'bbox' in the model request): sigma_out = sigma_in + 100 for points inside the scene cube
 * that lie within 5e-2 of at least one face pair on every axis pair (the wire frame of the cube).
 *   points [n,3], sigma_in / sigma_out [n] (may alias); threshold = (float)(scene_range - 5e-2) from the caller. */
int nfi_bbox_overlay(const float* points, int64_t n_points, float scene_range, float threshold, const float* sigma_in,
                     float* sigma_out, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-ray weights.  Replaces nerf_utils.render_volume_density_weights_only
 * (lib/nerf_utils.py:164-180, cumprod_exclusive 20-25).
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_weights_args {
  int64_t n_rays;
  int n_samples;               /* <= NFI_MAX_SAMPLES_SINGLE_PASS */
  const float* sigma;          /* [N,S] */
  const float* ray_directions; /* [N,3] */
  const float* depth;          /* [N,S] */
  float* weights;              /* [N,S] out */
} nfi_weights_args;
int nfi_ray_weights(const nfi_weights_args* a, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Inverse-CDF sampling.  Replaces nerf_utils.sample_pdf (lib/nerf_utils.py:183-222).
 *   bins [N,M], weights [N,M-1], u [N,K] (row stride u_row_stride floats; 0 broadcasts one
 *   row, which is how the deterministic linspace(0,1,K) of the reference is passed)
 *   -> samples [N,K]; optional inds int64 [N,K] (searchsorted(cdf,u,right=True)), cdf [N,M].
 *   M <= 128, K <= 128.
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_sample_pdf_args {
  int64_t n_rays;
  int n_bins;      /* M */
  int n_samples;   /* K */
  const float* bins;
  const float* weights;
  const float* u;
  int64_t u_row_stride;
  float* samples;
  int64_t* inds;   /* or NULL */
  float* cdf;      /* or NULL */
} nfi_sample_pdf_args;
int nfi_sample_pdf(const nfi_sample_pdf_args* a, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Hierarchical resampling as run.py does it between the two field queries: coarse weights
 * (run.py:262) -> EG3D smoothing (264-272) -> sample_pdf on the bin mid-points (274-281).
 *   sigma,depth [N,S]; u as above with K = S  ->  fine depths [N,S] (unsorted, like the reference)
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_resample_args {
  int64_t n_rays;
  int n_samples;               /* S <= 64 */
  const float* sigma;
  const float* ray_directions;
  const float* depth;
  const float* u;
  int64_t u_row_stride;
  float* fine_depth;           /* [N,S] out */
  float* weights;              /* [N,S] out or NULL (coarse weights) */
  float* smooth;               /* [N,S] out or NULL */
  float* cdf;                  /* [N,S-1] out or NULL */
  int64_t* inds;               /* [N,S] out or NULL */
} nfi_resample_args;
int nfi_resample(const nfi_resample_args* a, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Alpha compositing.  Replaces nerf_utils.render_volume_density (lib/nerf_utils.py:123-161)
 * and, when depth_b != NULL, the sort/merge of run.py:283-335 in front of it: the two depth
 * lists are merged ascending (stable: list a first on ties) and attributes follow.
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_composite_args {
  int64_t n_rays;
  int n_a;                      /* samples in list a (n_b == 0: <= 512; merged lists: <= 128 each) */
  int n_b;                      /* 0: plain compositing of list a, assumed in ray order */
  const float* ray_directions;  /* [N,3] */
  const float* depth_a; const float* sigma_a; const float* rgb_a;  /* [N,n_a], [N,n_a], [N,n_a,3] */
  const float* depth_b; const float* sigma_b; const float* rgb_b;  /* [N,n_b] ... or NULL */
  int n_extra;                  /* channels of an extra attribute (semantics / normals / coords), 0 = none */
  const float* extra_a;         /* [N,n_a,n_extra] */
  const float* extra_b;         /* [N,n_b,n_extra] */
  int white_background;
  float* rgb_map;    /* [N,3] out */
  float* depth_map;  /* [N] out */
  float* mask;       /* [N] out */
  float* extra_map;  /* [N,n_extra] out or NULL */
  float* weights;    /* [N,n_a+n_b] out or NULL (in merged order) */
  float* depth_sorted; /* [N,n_a+n_b] out or NULL */
  int64_t* perm;     /* [N,n_a+n_b] out or NULL: merged position -> index into cat(a,b) */
} nfi_composite_args;
int nfi_composite_fwd(const nfi_composite_args* a, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the per-ray stages (the reference gets these from autograd).
 * Gradients flow to sigma, rgb, extras and (through dists*||rd||) the ray directions; depth samples
 * and depth_map carry none (lib/nerf_utils.py:145, run.py:197-200, 261).
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_composite_bwd_args {
  int64_t n_rays;
  int n_a; int n_b;             /* as nfi_composite_args */
  const float* ray_directions;
  const float* depth_a; const float* sigma_a; const float* rgb_a;
  const float* depth_b; const float* sigma_b; const float* rgb_b;
  int n_extra; const float* extra_a; const float* extra_b;
  int white_background;
  const float* g_rgb_map;    /* [N,3] upstream gradient */
  const float* g_mask;       /* [N] or NULL */
  const float* g_extra_map;  /* [N,n_extra] or NULL */
  float* g_sigma_a; float* g_rgb_a;   /* [N,n_a], [N,n_a,3] out */
  float* g_sigma_b; float* g_rgb_b;   /* [N,n_b], [N,n_b,3] out (n_b > 0) */
  float* g_extra_a; float* g_extra_b; /* out or NULL */
  float* g_ray_directions;            /* [N,3] out or NULL */
  /* 0: lists a and b are dense ([N,n_a], [N,n_b]).  > 0: every per-sample array (inputs and gradients) has this many
   * entries per ray, e.g. n_a + n_b with depth_b = depth_a + n_a for the stash layout of nfi_render_fwd */
  int list_row_stride;
} nfi_composite_bwd_args;
int nfi_composite_bwd(const nfi_composite_bwd_args* a, nfi_stream_t stream);
/* x = o + d*t: g_points [N,S,3], depth [N,S] -> g_ray_origins [N,3], g_ray_directions [N,3] (either may be NULL) */
int nfi_points_bwd(const float* g_points, const float* depth, int64_t n_rays, int n_samples,
                   float* g_ray_origins, float* g_ray_directions, nfi_stream_t stream);
/* nfi_raygen backward: g_ray_origins / g_ray_directions [N,3] (either may be NULL) ->
 * g_cam2world [B,4,4] (zeroed inside), g_focal [B] or NULL.  a->ray_origins/ray_directions are ignored. */
int nfi_raygen_bwd(const nfi_raygen_args* a, const float* g_ray_origins, const float* g_ray_directions,
                   float* g_cam2world, float* g_focal, nfi_stream_t stream);
/* The same gradients, bit-identical from launch to launch: one block per image keeps the 17 sums in float64 over the whole
 * image, rounds once and stores (no atomic, no memset, no workspace; g_cam2world / g_focal are WRITTEN). */
int nfi_raygen_bwd_ordered(const nfi_raygen_args* a, const float* g_ray_origins, const float* g_ray_directions,
                           float* g_cam2world, float* g_focal, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Field query backward: autograd of the sampler closure (models/generator.py:587-681), i.e.
 * grid_sample backward (scatter-add into the planes + coordinate gradients), the decoder MLP, the
 * Laplace-CDF density and the colour head, with the forward recomputed per tile.
 *   upstream: g_sigma [B,P], g_rgb [B,P,3], optional g_sdf [B,P], g_semantics [B,P,A]
 *   results : g_texels [B,3,R,R,32] (ACCUMULATED: caller zeroes it; convert with nfi_texels_to_planes),
 *             g_w1 [64,32], g_b1 [64], g_w2 [n_out,64], g_b2 [n_out], g_attention_values [B,A,3],
 *             g_beta [1], g_alpha [1] (all ACCUMULATED into caller-zeroed buffers, raw-parameter
 *             gradients with the equalized-lr gains applied), g_points [B,P,3] or NULL (written).
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_field_bwd_args {
  int n_scenes;
  int64_t points_per_scene;          /* <= 2^30 (<= 2^25 with scatter_mode 1 or 2): the kernels address a scene's points by 32-bit offsets */
  const float* points;
  const void* texels; int plane_res; int texel_dtype;   /* any storage type; g_texels is fp32 (view-direction decoder: fp32 texels only) */
  const float* decoder_image;                            /* forward operand image */
  const float* w1; const float* w2;                      /* raw decoder weights (backward operands) */
  int n_attention; const float* attention_values;
  int use_sdf; const float* beta; const float* alpha;
  float scene_range;
  const float* g_sigma; const float* g_rgb; const float* g_sdf; const float* g_semantics;
  float* g_texels; float* g_points;
  float* g_w1; float* g_b1; float* g_w2; float* g_b2;
  float* g_attention_values; float* g_beta; float* g_alpha;
  void* workspace; size_t workspace_bytes;               /* >= nfi_decoder_bwd_image_floats()*4 bytes */
  /* points_only = 1: only g_points is produced (no plane scatter, no parameter gradients; all
   * other g_* outputs may be NULL).  normalize_g_points = 1: each g_points row is L2-normalised
   * (eps 1e-12).  Together with g_sdf == 1 this yields the analytic surface normals
   * normalize(d sdf / d x) of models/generator.py:599-623 without autograd. */
  int points_only; int normalize_g_points;
  /* view-direction decoder (decoder_image from nfi_decoder_pack_viewdir; w2 is [33,64], g_w2 [33,64], g_b2 [33]):
   * ray_features [B, P/samples_per_ray, NFI_RAY_FEATURE_PITCH], w3 raw [n3,32]; gradients g_ray_features (same
   * padded shape, zero-initialised by the caller, columns 1..32 accumulate), g_w3 [n3,32], g_b3 [n3]. */
  const float* ray_features; int samples_per_ray; const float* w3;
  float* g_ray_features; float* g_w3; float* g_b3;
  /* plane-gradient scatter.  0: fp32 atomics straight from the backward kernel (384 atomic dwords per point).
   * 1: binned - the kernel writes the per-point feature gradient (128 B) to the workspace, the points are counting-
   * sorted by texel cell per plane (by 16x16-texel tile through global memory, by cell inside LDS), and the sorted
   * entries are reduced in registers with one set of line-coalesced atomics per run of a cell; needs
   * nfi_field_bwd_workspace_bytes(a) of workspace (177 B per point).  Same result up to fp32 summation order.
   * 2: ordered - EVERY output of the call is bit-identical from launch to launch for identical arguments on the same
   * device and build, with the same rays_per_row (the grid, and with it the order of the parameter sums, follows the
   * arguments).  g_texels: the rows of mode 1, one 64-bit key (cell, point) per point and plane, a stable radix sort by
   * cell, and one half-wave per texel that adds the points of its up to four cells in ascending (cell, point) order and
   * is the texel's only writer; the decoder, attention, beta and alpha gradients: one zeroed workspace slot per wave,
   * summed in slot order by a finish kernel.  No float atomic meets another.  Same ACCUMULATED contract, same 2^25 limit;
   * all scratch from nfi_field_bwd_workspace_bytes(a) of workspace (177 B per point + 13 KB per wave of the grid), no
   * allocation, no synchronisation.  Plain decoder only: an error with ray_features (the view-direction decoder's
   * g_ray_features are atomics over up to 8 chunks per ray) and with points_only (nothing to order).  Slower than mode 1:
   * see DESIGN.md section 6.  Any other value is an error. */
  int scatter_mode;
  int texel_layout;              /* of texels AND g_texels */
  /* Order hint (0: none): the points are [rays][samples_per_ray] with the rays in row-major order of an image
   * rays_per_row wide (what nfi_render_fwd's training stash holds).  The kernel then walks the rays in 16 x 16- (or 8 x 8-)
   * pixel tiles, one tile at a time per XCD, for L2 locality of the texel gather; results do not depend on it beyond the
   * summation order of the parameter gradients.  Ignored unless samples_per_ray is a multiple of 64 and the image
   * divides into whole tiles. */
  int rays_per_row;
} nfi_field_bwd_args;
size_t nfi_field_bwd_workspace_bytes(const nfi_field_bwd_args* a);  /* for the scatter_mode / decoder of *a */
size_t nfi_decoder_bwd_image_floats(void);          /* workspace floats, plain decoder */
size_t nfi_decoder_bwd_image_floats_viewdir(void);  /* workspace floats, view-direction decoder */
int nfi_field_query_bwd(const nfi_field_bwd_args* a, nfi_stream_t stream);
/* as nfi_field_kernel_name, for nfi_field_query_bwd: "field_query_bwd_kernel<ATT,COORD,VD,TEX>" */
const char* nfi_field_bwd_kernel_name(const nfi_field_bwd_args* a);

/* ------------------------------------------------------------------------------------------
 * Distance field + its spatial gradient as one differentiable operator: the regulariser branch of
 * Generator.forward (models/generator.py:505-585).  The reference gets d(sdf)/d(x) from
 * torch.autograd.grad(..., create_graph=True) through a double-differentiable grid_sample
 * (lib/ops.py:58-120); here the gradient is a second OUTPUT, so nfi_sdf_gradient_bwd is that double backward.
 *   points [B,P,3] (inside the cube: stratified samples, lib/ops.py:20-26), texels fp32 [B,3,R,R,32],
 *   raw decoder parameters w1 [64,32] b1 [64] w2 [n_out,64] b2 [n_out] (row 0 = distance head)
 *   fwd: sdf [B,P], gradient [B,P,3] = d sdf / d points
 *   bwd: upstream g_sdf [B,P] / g_gradient [B,P,3] (either may be NULL) -> g_texels [B,3,R,R,32], g_w1 [64,32],
 *        g_b1 [64], g_w2 [64] (row 0), g_b2 [1]; all ACCUMULATED into (zero-initialise them).
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_sdf_gradient_args {
  int n_scenes;
  int64_t points_per_scene;
  const float* points;
  const float* texels; int plane_res;
  float scene_range;
  const float* w1; const float* b1; const float* w2; const float* b2;
  float* sdf; float* gradient;                       /* forward outputs */
  const float* g_sdf; const float* g_gradient;       /* backward inputs */
  float* g_texels; float* g_w1; float* g_b1; float* g_w2; float* g_b2;
  int texel_layout;              /* of texels AND g_texels */
} nfi_sdf_gradient_args;
int nfi_sdf_gradient_fwd(const nfi_sdf_gradient_args* a, nfi_stream_t stream);
int nfi_sdf_gradient_bwd(const nfi_sdf_gradient_args* a, nfi_stream_t stream);
/* nfi_sdf_gradient_bwd with every output bit-identical from launch to launch (same arguments, device and build): the
 * same per-contribution arithmetic, summed in a fixed order instead of by float atomics.  The reference's double backward
 * (lib/ops.py:58-120 under models/generator.py:534-540) sums with index_put / scatter atomics and makes no such promise;
 * this is the regulariser's share of nfi_field_bwd_args.scatter_mode = 2.  Same arguments, NULL-upstream rules and
 * ACCUMULATE contract as nfi_sdf_gradient_bwd (rows 1.. of g_w2 / g_b2 untouched).  No allocation, no synchronisation:
 * all scratch is `workspace` (device memory, 256-byte aligned), which need not be zeroed and holds, per point, two
 * gradient rows (2 x 128 B), a flag (1 B) and two sort keys per plane (2 x 3 x 8 B), plus the sort's digit counts and, per
 * wave of the backward's grid, one slot of 2 192 floats (8 768 B).  Refused: a NULL or too-small workspace, both upstream
 * gradients NULL, points_per_scene above 2^25 (the limit of nfi_field_query_bwd's ordered mode: 32-bit point indices in
 * the keys).  nfi_sdf_gradient_bwd_ordered_workspace_bytes returns 0 for a shape the call would refuse. */
size_t nfi_sdf_gradient_bwd_ordered_workspace_bytes(const nfi_sdf_gradient_args* a);
int nfi_sdf_gradient_bwd_ordered(const nfi_sdf_gradient_args* a, void* workspace, size_t workspace_bytes, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused forward render: run.py::render (176-350) from cameras + texels to pixels in one
 * persistent launch (plus the ray set-up launch), no per-sample HBM round trips.
 * ------------------------------------------------------------------------------------------ */
/* bits of nfi_render_args.tuning that the library reads (described at the field; every other bit is ignored) */
enum { NFI_TUNING_SCANLINE_ORDER = 4, NFI_TUNING_EXACT_FP32_MLP = 8, NFI_TUNING_SINGLE_WORK_COUNTER = 16,
       NFI_TUNING_XCD_BLOCKS_IN_ORDER = 32 };
typedef struct nfi_render_args {
  int n_scenes, height, width;   /* n_scenes: the number of images (= scenes x views_per_scene) */
  int n_samples;                 /* S per pass, <= NFI_MAX_SAMPLES; without fine_sampling a single pass of up to
                                  * NFI_MAX_SAMPLES_SINGLE_PASS (run.py:2271), with stage taps / stash / viewdir but
                                  * without the extra maps, the cycle profile and termination_eps */
  int fine_sampling;             /* args.fine_sampling (run.py:259) */
  int white_background;          /* dataset_config['white_background'] (run.py:348) */
  float scene_range;             /* dataset_config['scene_range'] (run.py:200) */
  /* Views per scene, V (0 and 1 both mean one view).  The images of a call are ordered scene-major: image i has camera i,
   * noise rows i and output / tap / stash rows i, and reads the texels and attention rows of scene i / V.  n_scenes stays
   * the number of IMAGES and must be a multiple of V; `texels` and `attention_values` then hold n_scenes / V scenes.
   * Everything per ray is unchanged, and the batch-wide miss-fill of lib/nerf_utils.py:258-259 is taken over all n_scenes
   * images - the result is bit for bit that of a one-view call with every scene's texels and attention rows repeated V
   * times.  nfi_render_setup does not read the field. */
  int views_per_scene;
  /* camera (as nfi_raygen_args) */
  const float* cam2world; const float* focal; const float* bbox; const float* center;
  /* field (as nfi_field_args) */
  const void* texels; int plane_res; int texel_dtype;              /* texels of n_scenes / views_per_scene scenes */
  const float* decoder_image; int n_attention; const float* attention_values;   /* [n_scenes / views_per_scene, A] */
  int use_sdf; const float* beta; const float* alpha;
  /* the reference's two random draws (nerf_utils.py:115, 202); NULL = deterministic */
  const float* noise_coarse;     /* [N,S] or NULL */
  const float* noise_fine;       /* u: [N,S] with row stride below, never NULL when fine_sampling */
  int64_t noise_fine_row_stride;
  /* outputs */
  float* rgb;        /* [N,3] */
  float* depth;      /* [N] */
  float* mask;       /* [N] */
  float* semantics;  /* [N,A] or NULL: composited softmax probabilities, sum_k w_k softmax(features_k) over the merged
                      * samples (compute_semantics: run.py:231-233, 312-335; lib/nerf_utils.py:153-156); n_attention > 0 */
  /* optional stage taps (any may be NULL) */
  float* ray_origins; float* ray_directions; float* near_plane; float* far_plane; uint8_t* hit;
  float* t_coarse; float* sigma_coarse; float* rgb_coarse;   /* [N,S], [N,S], [N,S,3] */
  float* t_fine; float* sigma_fine; float* rgb_fine;
  float* t_sorted; float* weights; int32_t* perm;            /* [N,2S] */
  /* workspace: nfi_render_workspace_bytes(n_scenes*height*width) bytes, 4-byte aligned, contents arbitrary (the ray set-up
   * writes every cell it or the render kernel reads).  Layout: a 576-byte header (the three reduction cells of the ray
   * set-up first), ray_origins and ray_directions [N,3], near and far [N], hit [N] bytes padded to 64, and behind those the
   * set-up's per-block partial reductions (internal, 16 384 bytes) and, at byte 576 + 32 N + pad64(N) + 16 384, the block
   * table of the per-XCD queues: N / 64 uint32, queue slot -> pixel block (a hint for balance: every aligned group of 16
   * slots is a permutation of itself, the render is the same for any such permutation). */
  void* workspace; size_t workspace_bytes;
  /* 1: rays whose line misses the scene cube inflated by 1e-4 skip both passes (exact:
   * every sample of such a ray is outside the cube, sigma==0).  0: evaluate every ray. */
  int skip_missed_rays;
  /* optional hipEvent_t pair recorded on the stream immediately before / after the render kernel
   * (excludes the ray set-up launch): live per-launch kernel timing for bench.py.  NULL = off. */
  void* event_start; void* event_stop;
  /* tuning knob, 0 = default, an OR of NFI_TUNING_*.  bit 2 (SCANLINE_ORDER): hand rays out in scanline order instead
   * of 8x8 pixel tiles (results identical).  bit 3 (EXACT_FP32_MLP): evaluate the decoder MLP with exact-fp32 MFMA instead of the
   * split-fp16 (hi+lo, 22 significand bits) MFMA; both meet the 1e-4 parity budget (fp32 texels only: with 16-bit texel
   * storage the texels, not the MLP operands, set the precision - the call is refused).  bit 4 (SINGLE_WORK_COUNTER): ONE device-wide work
   * counter instead of the per-XCD queues over square pixel blocks (results identical; the per-XCD queues take the
   * largest of 32 / 16 / 8 pixels that divides both image sides, two positions per atomic, and fall back to the single
   * counter when not even 8 does).  bit 5 (XCD_BLOCKS_IN_ORDER): pixel block b sits in slot b of the per-XCD queues,
   * instead of where the set-up's block table puts it - of every 16 consecutive blocks the heaviest and the lightest by
   * rays that hit the scene cube go to one XCD, the second of each to the next, ... (results identical; for A/B runs). */
  int tuning;
  /* optional uint64[12] device array: per-phase shader-cycle sums over all waves (profiling build of
   * the kernel; NULL = off): field tile {unused (0), gather issue+wait+interp, mlp, count}, ray set-up, coarse field,
   * resample, fine field, merge, composite, rays marched, wave lifetime; fp32 texels only */
  void* profile_cycles;
  /* view-direction decoder: NULL, or [N, NFI_RAY_FEATURE_PITCH] (decoder_image from nfi_decoder_pack_viewdir;
   * the MLP then runs in exact fp32) */
  const float* ray_features;
  /* Ray termination in the FINE pass (0 = off; BASELINE cfg5: "wavefront early-termination + sample compaction").  eps in
   * (0,1): the coarse pass - hence the resampling pdf, every sample index and every depth - is untouched; fine samples
   * that lie behind the first coarse sample in front of which the COARSE transmittance prod(1 - alpha_j + 1e-10) has
   * fallen below eps are not evaluated (sigma = 0; they stay in the merge with their depth), and the surviving fine
   * samples are compacted to the low lanes by wave ballot + popcount so that whole 16-point field tiles drop out.
   * What is dropped carries at most the merged transmittance at that depth (about eps) of compositing weight:
   * |d rgb|, |d mask| <= ~eps; tests hold eps = 1e-5 to the 1e-4 parity budget at full size.  Not available together
   * with stage taps, extra maps, the cycle profile, the view-direction decoder or the exact-fp32 MLP. */
  float termination_eps;
  int texel_layout;              /* NFI_TEXELS_PLANAR (0) / NFI_TEXELS_INTERLEAVED */
  /* optional uint64[2] device array (NULL = off): shader cycles (s_memtime) and 100 MHz reference ticks
   * (s_memrealtime) between the start and the end of workgroup 0 / wave 0 of the render kernel, i.e. the shader clock
   * DURING this launch = cycles / ticks x 1e8 Hz (bench.py prices the kernel's issue rate against it) */
  void* clock_probe;
  /* pixel-row window: this call renders rows [row_offset, row_offset + height) of an image that is full_height rows
   * tall (full_height 0 = height: the whole image).  Rays, samples and pixels are bit-identical to the same rows of the
   * full render (the pixel coordinate of get_ray_bundle, lib/nerf_utils.py:36-39, is (row_offset + row) / full_height)
   * - with ONE exception: the batch-wide miss-fill of lib/nerf_utils.py:258-259 (min near / max far over the hit rays,
   * the first two cells of the workspace after nfi_render_setup) is taken over the WINDOW's rays, so rays that are
   * marched although they miss the exact cube (inside the 1e-4 inflated one, or any missed ray with skip_missed_rays =
   * 0) get the window's fill, not the image's.  A caller that shards one image max-reduces those two cells (and sums
   * the third, the hit count) over the windows between nfi_render_setup and nfi_render_fwd(rays_ready = 1):
   * parallel.allreduce_ray_setup.  Outputs, noise and taps are sized for the window.  One image sharded over the ranks of a node: SURVEY.md 8(e),
   * run.py:598-605 (res_multiplier renders). */
  int row_offset; int full_height;
  /* training stash (all three or none): the per-sample state the backward needs, ray-major with the coarse samples in
   * [0,S) and the fine samples in [S,2S) of every row - stash_t [N,2S], stash_sigma [N,2S], stash_rgb [N,2S,3], in
   * SOURCE order (not merged); without fine_sampling the rows hold the S samples of the single pass ([N,S], [N,S],
   * [N,S,3]).  nfi_composite_bwd (list_row_stride = 2S, or one list of S) and nfi_field_query_bwd over the points of
   * every ray then replace autograd of run.py:193-348.  Unlike the debug
   * taps the stash keeps the missed-ray skip: rays that are skipped get an all-zero row.  Mutually exclusive with the
   * t_coarse ... rgb_fine taps. */
  float* stash_t; float* stash_sigma; float* stash_rgb;
  /* 1: the workspace already holds the ray set-up of these cameras / this image window (nfi_render_setup with the same
   * camera, shape, scene_range and workspace arguments, ordered before this call): nfi_render_fwd then launches the render
   * kernel only.  Lets a caller run the set-up of the NEXT batch on another stream while this one renders. */
  int rays_ready;
  /* [N,3] or NULL: composited query points, sum_k w_k (o + d t_k) over the merged samples - the sampler's 'coords'
   * output (models/generator.py:643) in the semantics slot of render_volume_density (compute_coords: run.py:234-235,
   * 337-338; the encoder-training loop asks for it every iteration, run.py:1639-1646).  Like `semantics` it comes out of
   * the SAME render launch (rgb / depth / mask bit-identical to a call without it); neither is available together with
   * stage taps, the cycle profile or the exact-fp32 MLP; with the view-direction decoder (ray_features) both exist for fp32
   * texels.  (The 128 + 128 kernel parks the probabilities of `semantics` as unorm16 between the passes: |error| <= 7.7e-6
   * per sample under a convex combination; the composited map is then scaled to sum to the mask, as the fp32 table's
   * does - the roundings of a sample's A probabilities do not cancel.) */
  float* coords;
  /* [N,3] or NULL: the composited normal map, sum_k w_k normalize(d sdf / d x)_k over the merged samples, + (1 - mask)
   * on a white background (compute_normals: run.py:228-230, 241-245, 296-300; lib/nerf_utils.py:149-151, 159; the
   * sampler's 'normals' output, models/generator.py:599-618, here the analytic derivative of the decoder's distance
   * instead of autograd).  use_sdf only; any texel storage; same launch, same restrictions as `coords` (with the
   * view-direction decoder: fp32 texels - the distance is row 0 of its second layer). */
  float* normals;
} nfi_render_args;
size_t nfi_render_workspace_bytes(int64_t n_rays);
int nfi_render_fwd(const nfi_render_args* a, nfi_stream_t stream);
/* as nfi_field_kernel_name, for the render kernel of nfi_render_fwd (its argument rules except the workspace size, the
 * row window and rays_ready, which do not bear on the selection): "render_fwd_kernel<TEX,ATT,OCC,MODE,PREC,VD>" for
 * n_samples <= 64, "render_fwd_wide_kernel<TEX,ATT,MODE,PREC,VD,OCC>" up to 128, "render_fwd_long_kernel<TEX,ATT,PREC,VD>"
 * for a single pass beyond that */
const char* nfi_render_kernel_name(const nfi_render_args* a);
/* The ray set-up of nfi_render_fwd alone (get_ray_bundle + normalize + the scene-cube test of
 * lib/nerf_utils.py:28-91, 237-268 into the workspace, the batch-wide miss-fill reduction and the work counters cleared).
 * Reads only the camera / shape / scene_range / workspace fields (and ray_origins / ray_directions / hit if given). */
int nfi_render_setup(const nfi_render_args* a, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Camera pose from a canonical-coordinate map: replaces the .cpu().numpy() + OpenCV solvePnPGeneric round trip of
 * lib/pose_estimation.py:30-131 (compute_pose_pnp) that run.py:1709-1740 (estimate_poses_batch) makes for every
 * inversion batch.  Per image and focal proposal: Hartley-normalised DLT start, polar decomposition, Levenberg-Marquardt
 * on the reprojection error; per image the proposal with the smallest RMS reprojection error (OpenCV's definition,
 * sqrt(sum |r|^2 / 2N)) among the solutions with t_z > 0; images without a solution (or with fewer than 4 foreground
 * pixels, as in the reference) get the reference's dummy pose (t = (0,0,-10), focal 1, error 10).  4 or 5 pixels,
 * coplanar points and linear starts that end behind the camera: refinement from the 24 axis-aligned rotations instead.
 * PARITY UNPINNED: OpenCV is not available offline, no golden vectors exist (see csrc/nfi_pnp.inc).
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_pnp_args {
  int n_images; int height; int width;
  const float* coords;          /* [B,H,W,3] canonical object coordinates per pixel */
  const float* mask;            /* [B,H,W]: a pixel is foreground where mask > mask_threshold (run.py:1710: 0.9) */
  float mask_threshold;
  int n_focal; const float* focal_proposals;   /* [n_focal] device array (pose_estimation.py:134-143) */
  int refine_iterations;        /* Levenberg-Marquardt passes (0: linear start only = refine=False) */
  void* workspace; size_t workspace_bytes;     /* nfi_pnp_workspace_bytes(n_images, n_focal), 8-byte aligned */
  float* world2cam;             /* [B,4,4] out: flip @ [R|t], flip = diag(1,-1,-1,1) (pose_estimation.py:119-127) */
  float* focal;                 /* [B] out: the chosen proposal */
  float* error;                 /* [B] out: its RMS reprojection error */
} nfi_pnp_args;
size_t nfi_pnp_workspace_bytes(int n_images, int n_focal);
int nfi_pose_pnp(const nfi_pnp_args* a, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Pose algebra of the inversion loop: lib/pose_utils.py between the optimiser's parameters (z0, t2, s, quaternion) and
 * the cam2world matrix the render takes.  One thread per image, any n_images >= 1; no workspace, no atomics, no
 * allocation, no synchronisation: every result is the same bits on every launch.  Each thread reads its fp32 inputs,
 * works in float64 and rounds once on the way out, so a result is within one rounding of the exact value of the
 * reference's formula (the reference's own fp32 chain is a few roundings off it).  Tensors are dense.
 * Every entry refuses, with -1 and a message before any launch: a null argument struct, n_images < 1, a null required
 * pointer, and what its own comment lists.
 *
 * pose_to_matrix, lib/pose_utils.py:30-70.  q [B,4] = (w, x, y, z); R = quaternion_to_matrix of q, whose ROW i is e_i
 * rotated (lib/pose_utils.py:41-45), a polynomial in q that is evaluated as such for a non-unit q too.
 *   normalize_q != 0: q is first replaced by q / max(|q|, 1e-12), F.normalize(q, dim=-1) of run.py:2257-2262.
 *   z0 given (perspective): f = 1 + exp(z0), t3 = (t2 / s, f / s); cam2world = [[R, R t3], [0, 1]], focal = f / 2.
 *   z0 NULL (orthographic): t3 = (t2, 10); cam2world = [[R, R t3], [0, 1]] / s; focal must be NULL.
 *   camera_flipped != 0: columns 1..3 of the top three rows change sign (lib/pose_utils.py:59-60, 68-69).
 * The forward writes cam2world [B,4,4] and focal [B] (NULL allowed in the perspective branch too).  The backward reads
 * g_cam2world [B,4,4] and g_focal [B] (NULL: zero) and writes those of g_q [B,4], g_t2 [B,2], g_s [B], g_z0 [B] that
 * are not NULL, through the normalisation when normalize_q is set (where |q| < 1e-12 the clamp passes no gradient to
 * the norm, as in F.normalize).  Refused: focal / g_focal / g_z0 given together with a null z0; a backward with no
 * gradient to write. */
typedef struct nfi_pose_args {
  int n_images, camera_flipped, normalize_q;
  const float* q; const float* t2; const float* s; const float* z0;
  float* cam2world; float* focal;                                  /* forward outputs */
  const float* g_cam2world; const float* g_focal;                  /* backward inputs */
  float* g_q; float* g_t2; float* g_s; float* g_z0;                /* backward outputs, each optional */
} nfi_pose_args;
int nfi_pose_to_matrix_fwd(const nfi_pose_args* a, nfi_stream_t stream);
int nfi_pose_to_matrix_bwd(const nfi_pose_args* a, nfi_stream_t stream);

/* matrix_to_pose, lib/pose_utils.py:98-121, with matrix_to_quaternion (73-95) inside the kernel instead of a copy to
 * the host and a numpy loop, and matrix_to_conditioning_vector (124-145).  From cam2world [B,4,4] (columns 1..3 of the
 * top rows change sign first when camera_flipped) W = invert_space of it, t3 = -W[:3,3];
 *   focal given: z0 = log(2 focal - 1), s = 2 focal / t3.z;   focal NULL: s = 1 / cam2world[3,3], z0 must be NULL;
 *   t2 = t3.xy * s;  q [B,4] = matrix_to_quaternion of W: the reference's four branches, chosen on float64 values.
 *   cond [B,13] = (log(focal) unshifted, or 0 without focal; t2; s; the nine entries of W[:3,:3] row by row).
 * Every output is optional, at least one must be given.  Refused: z0 without focal. */
typedef struct nfi_matrix_to_pose_args {
  int n_images, camera_flipped;
  const float* cam2world; const float* focal;
  float* z0; float* t2; float* s; float* q; float* cond;
} nfi_matrix_to_pose_args;
int nfi_matrix_to_pose(const nfi_matrix_to_pose_args* a, nfi_stream_t stream);

/* rotation_matrix_distance, lib/pose_utils.py:148-156: degrees [B] = acos(clamp((trace(P Q^T) - 1) / 2, -1, 1)) * 180 /
 * pi of p, q [B,dim,dim]; dim = 4: the top-left 3 x 3 of each, divided by its element [3,3].  Refused: dim not 3 or 4. */
typedef struct nfi_rotation_distance_args {
  int n_images, dim;
  const float* p; const float* q;
  float* degrees;
} nfi_rotation_distance_args;
int nfi_rotation_distance(const nfi_rotation_distance_args* a, nfi_stream_t stream);

/* The selection inside perturb_poses, lib/pose_utils.py:159-170: index[i] = the j that minimises
 * |distance(cam2world[i], cam2world[j]) - target[i]| (the 4 x 4 distance above; on an exact tie the lowest j), for
 * cam2world [N,4,4] and target [N] in degrees: one launch in place of N rounds of a dozen launches and two reads each.
 * The N x N distances exist only in registers. */
typedef struct nfi_pose_nearest_args {
  int n_images;
  const float* cam2world; const float* target;
  int32_t* index;
} nfi_pose_nearest_args;
int nfi_pose_nearest_by_angle(const nfi_pose_nearest_args* a, nfi_stream_t stream);

/* The fix-ups after an optimiser step, run.py:2307-2310, in place: q [B,4] <- q / max(|q|, 1e-12), s [B] <- |s|,
 * z0 [B] <- clamp(z0, -4, 4) (z0 NULL: orthographic, skipped). */
typedef struct nfi_pose_project_args {
  int n_images;
  float* q; float* s; float* z0;
} nfi_pose_project_args;
int nfi_pose_project(const nfi_pose_project_args* a, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Plane-producer hand-off: the tail of the LAST StyleGAN2 synthesis block
 * (models/stylegan.py:383-435: img = upsample2d(img_prev); y = torgb(x, w); img += y) fused into one kernel that
 * writes the result as texels in the INTERLEAVED layout [B,R,R,3,32] (= a channels-last [B,96,R,R] tensor), so
 * that neither nfi_planes_to_texels nor nfi_texels_to_planes is needed.
 *   x [B,Cin,R,R] NCHW activations of conv1; styles [B,Cin] = torgb.affine(w) * torgb.weight_gain (stylegan.py:365);
 *   weight [96,Cin] = torgb.weight (1x1, no demodulation); bias [96]; previous_image [B,96,R/2,R/2] or NULL.
 *   fwd: texels [B,R,R,96].
 *   bwd: g_texels [B,R,R,96] -> g_x [B,Cin,R,R], g_styles [B,Cin], optional g_weight [96,Cin] + g_bias [96] (both
 *        or neither), optional g_previous_image [B,96,R/2,R/2]; all written (zeroed inside where accumulated).
 * Cin: multiple of 16, <= 256; R: multiple of 8.
 *   Alignment: x, texels and g_texels are accessed as 16-byte vectors and must be 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_torgb_args {
  int n_scenes, in_channels, resolution;
  const float* x; const float* styles; const float* weight; const float* bias; const float* previous_image;
  float* texels;                                         /* forward output */
  const float* g_texels;                                 /* backward input */
  float* g_x; float* g_styles; float* g_weight; float* g_bias; float* g_previous_image;
} nfi_torgb_args;
int nfi_torgb_texels_fwd(const nfi_torgb_args* a, nfi_stream_t stream);
int nfi_torgb_texels_bwd(const nfi_torgb_args* a, nfi_stream_t stream);
/* nfi_torgb_texels_bwd with every output bit-identical from launch to launch for identical arguments on the same device
 * and build: the same per-element arithmetic, summed in a fixed order instead of by float atomics (the reference's
 * backward of models/stylegan.py:424-443 - conv2d / conv_transpose2d gradients and the add - makes no such promise unless
 * MIOpen is held to its deterministic solvers).  Same arguments, shapes and WRITE semantics as nfi_torgb_texels_bwd;
 * g_x and g_previous_image carry the bits of that call (they have one writer per element there too).  g_styles: each wave
 * of the data kernel stores its sums to a slot (scene, block, wave) and a finish kernel adds the slots in index order;
 * g_weight / g_bias: the four waves of a block are combined in wave order, each block of the shape-determined grid
 * (min(ceil(B R^2 / 64), 256) x ceil(Cin / 64)) stores one partial and a finish kernel adds them in block order.  No
 * allocation, no synchronisation: all scratch is `workspace` (device memory, 4-byte aligned), which need not be zeroed
 * and holds 4 Cin floats per data block (1 024 pixels) and scene, and 96 x 64 (+ 96) floats per weight block.  Refused: a
 * NULL or too-small workspace, and what nfi_torgb_texels_bwd refuses.  nfi_torgb_texels_bwd_ordered_workspace_bytes
 * reads n_scenes, in_channels and resolution alone and returns 0 for a shape the call would refuse. */
size_t nfi_torgb_texels_bwd_ordered_workspace_bytes(const nfi_torgb_args* a);
int nfi_torgb_texels_bwd_ordered(const nfi_torgb_args* a, void* workspace, size_t workspace_bytes, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Neighbours of the renderer in the inversion loop.
 *
 * 2-D augmentation warp: the image part of augment_impl (run.py:720-769): mat = [[cos r, -sin r, tx], [sin r, cos r,
 * -ty]], scaled by `scale`, translation column re-projected (run.py:745-752), F.affine_grid(align_corners=False) +
 * F.grid_sample(bilinear, padding zeros, align_corners=False); white_background: (img - 1) is warped and 1 added
 * back (run.py:755-764).  The inversion loss warps cat(prediction, target) 15 times per step (run.py:2216-2231).
 *   image / warped [N,C,H,W]; rot [N], scale [N] or NULL (= 1), translation [N,2] (the host's random draws).
 *   bwd: g_warped [N,C,H,W] -> g_image [N,C,H,W] (zeroed inside; the adjoint of the forward w.r.t. the image).
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_warp_args {
  int n_images, channels, height, width;
  const float* image; float* warped;            /* forward */
  const float* g_warped; float* g_image;        /* backward */
  const float* rot; const float* scale; const float* translation;
  int white_background;
} nfi_warp_args;
int nfi_affine_warp_fwd(const nfi_warp_args* a, nfi_stream_t stream);
int nfi_affine_warp_bwd(const nfi_warp_args* a, nfi_stream_t stream);
/* nfi_affine_warp_bwd with g_image bit-identical from launch to launch for identical arguments on the same device and
 * build.  The reference's backward of run.py:745-766 is grid_sample's scatter of atomics, as nfi_affine_warp_bwd's is;
 * here the adjoint is a gather: one thread per SOURCE pixel visits, in row-major order, the output pixels whose bilinear
 * footprint can reach it (the inverse affine image of its 2 x 2 neighbourhood, widened for fp32 rounding, clipped to the
 * image - never by a constant: a zoom-out of `scale` sends about 4 / scale^2 outputs to one pixel), recomputes the
 * forward's sample position and weights for each, adds the ones that touch it and stores once.  Same arguments, shapes and
 * WRITE semantics as nfi_affine_warp_bwd (white_background is accepted and does not enter the adjoint); no workspace,
 * no allocation, no synchronisation. */
int nfi_affine_warp_bwd_ordered(const nfi_warp_args* a, nfi_stream_t stream);

/* Image metrics of the inversion / evaluation loops: lib/metrics.py psnr (30-45) and iou (79-94), per image.
 *   pred / target: n_images x elements_per_image values in [0,1] (any layout, identical for both) -> psnr [n_images]
 *   = min(60, -10 log10(mean((clamp(pred) - clamp(target))^2)));
 *   mask_pred / mask_real: n_images x elements_per_mask -> iou [n_images] = (|a & b| + 1e-6) / (|a | b| + 1e-6) of
 *   the masks thresholded at 0.5.  out_of_range (int, optional): set to 1 if any input violates the reference's
 *   range_check (-0.1 < v < 1.1; lib/metrics.py:22-27), 0 otherwise.  Either metric may be skipped (NULL output). */
typedef struct nfi_metrics_args {
  int n_images;
  const float* pred; const float* target; int64_t elements_per_image;
  const float* mask_pred; const float* mask_real; int64_t elements_per_mask;
  float* psnr; float* iou; int* out_of_range;
} nfi_metrics_args;
int nfi_image_metrics(const nfi_metrics_args* a, nfi_stream_t stream);

/* SSIM of the same loops: lib/metrics.py:48-76 ssim, per image - skimage.metrics.structural_similarity(channel_axis=0,
 * data_range=1.) with its other arguments at their defaults, on inputs clamped to [0,1].  Per channel, with u(.) the 7 x 7
 * box mean, v. = (49/48) (u(..) - u(.) u(.)), C1 = 1e-4, C2 = 9e-4:
 *   S = ((2 ux uy + C1) (2 vxy + C2)) / ((ux^2 + uy^2 + C1) (vx + vy + C2)),
 * averaged over the window centres at least 3 pixels from every edge ((H-6) x (W-6) values: no padding rule enters), then
 * over the three channels.  fp32 per window (the sums are taken about a per-tile pivot, so flat regions do not cancel),
 * float64 from the tile sums on.  One block per (image, channel, tile of 16 x 32 centres) writes one partial sum; a second
 * kernel adds them in index order: no float atomics, the same bits on every launch, and an image's value does not depend
 * on the batch around it.  No allocation, no synchronisation.
 *   n_images, height, width: B >= 1, H >= 7, W >= 7 (lib/metrics.py:48-76: scikit-image raises below one window).
 *   pred / target: B x 3 x H x W values, each dense in its own layout (lib/metrics.py:48-76 asserts [B,3,H,W]):
 *   pred_layout / target_layout 0 = [B,3,H,W], 1 = [B,H,W,3] (what run.py's permute(0,3,1,2) of a render is in memory).
 *   ssim [B] (required); ssim_map [B,3,H-6,W-6] or NULL: S per window centre, the cropped map of lib/metrics.py:48-76's
 *   call with full=True.  out_of_range (int, optional): 1 if any input violates the range_check lib/metrics.py:48-76
 *   runs on both inputs (-0.1 < v < 1.1, so a NaN is flagged), 0 otherwise.
 *   workspace: device memory, 8-byte aligned, need not be zeroed; nfi_image_ssim_workspace_bytes reads n_images, height
 *   and width alone (one double per block) and returns 0 for a shape the call refuses.
 * Refused before any launch (-1, nfi_last_error()): a null argument / pred / target / ssim, n_images < 1, a side under
 * 7, a layout other than 0 or 1, a missing, too small or misaligned workspace. */
typedef struct nfi_ssim_args {
  int n_images, height, width;
  const float* pred; int pred_layout;
  const float* target; int target_layout;
  float* ssim;
  float* ssim_map;
  int* out_of_range;
  void* workspace; size_t workspace_bytes;
} nfi_ssim_args;
size_t nfi_image_ssim_workspace_bytes(const nfi_ssim_args* a);
int nfi_image_ssim(const nfi_ssim_args* a, nfi_stream_t stream);

/* Separable image filter, the progressive discriminator blur: lib/ops.py:29-55 (filt2d with a 1-D kernel, and blur, which
 * run.py:998 and run.py:1090-1093 call for the first blur_warmup_iters iterations).  With f the 2 radius + 1 taps:
 *   out[y,x] = background + sum_{a,b} f[a] f[b] (image[y + a - radius, x + b - radius] - background),
 * samples outside the image contributing 0 - lib/ops.py:29-55's conv2d with padding radius on image - 1 (white background)
 * or on image itself, a cross-correlation, same size out as in.  ONE launch: a block per (image, channel, tile of 32 x 32
 * pixels) stages its tile and halo in LDS, filters the rows, then the columns.  Exact fp32: one accumulator per output, the
 * taps applied in index order with fmaf, rows first.  No atomics, no workspace, no allocation, no synchronisation: the same
 * bits on every launch.
 *   n_images, channels, height, width: B, C, H, W, each >= 1 (images smaller than the radius included).
 *   image: B x C x H x W values, dense in `layout`: NFI_FILTER_BCHW = [B,C,H,W], NFI_FILTER_BHWC = [B,H,W,C] (what run.py's
 *   target_img.permute(0,3,1,2) is in memory).  out: dense [B,C,H,W], always; must not overlap image.
 *   radius: 1 .. 30 (lib/ops.py:29-55's blur has sigma <= 10, hence at most 61 taps).
 *   taps: float[2 radius + 1] on the device, used as given (filt2d), or NULL: every block computes lib/ops.py:29-55's own,
 *   f[j] = exp2(-((j - radius) / sigma)^2) - base 2 - added in the order j = 0 .. 2 radius and divided by that sum.
 *   background: subtracted from every sample as it is read and added to every output (1 = white, 0 = none).
 *   flip: nonzero applies the taps reversed - the adjoint of the same call, i.e. its backward with background 0.
 * Refused before any launch (-1, nfi_last_error()): a null argument / image / out; n_images, channels, height or width
 * under 1; a layout other than the two; radius outside 1 .. 30; null taps with sigma <= 0 (or NaN); a grid over the launch
 * limit: n_images * channels * ceil(height / 32) * ceil(width / 32) must be below 2^31. */
enum { NFI_FILTER_BCHW = 0, NFI_FILTER_BHWC = 1 };
typedef struct nfi_filter_args {
  int n_images, channels, height, width;
  int layout;
  const float* image;
  float* out;
  int radius;
  const float* taps;
  float sigma, background;
  int flip;
} nfi_filter_args;
int nfi_separable_filter(const nfi_filter_args* a, nfi_stream_t stream);

/* The distance head of LPIPS, one layer per call: lib/metrics.py:104-110, 130-133 - what LPIPSLoss does to each of the five
 * feature maps AFTER the VGG convolutions (which stay with the library that runs them).  With p over the H W pixels:
 *   rx[b,p] = sqrt(sum_c x[b,c,p]^2),  xh = x / (rx + eps)      (normalize_tensor: eps added to the norm, not under the root)
 *   ry, yh likewise; y_normalized != 0: yh = y as given         (cached features, lib/metrics.py:126-128)
 *   out[b]  = (1 / (H W)) sum_p sum_c weight[c] (xh[b,c,p] - yh[b,c,p])^2
 * The difference is formed per element and then squared, in float64 like the channel sums: identical x and y give exactly
 * 0.0f and exactly zero gradients.  A block owns one image and 64 consecutive pixels; channels 64 and 128 are read once
 * (kept in registers between the sweeps), any other count >= 1 is read again per sweep.
 *   fwd: every block writes one float64 partial to the workspace; a second kernel adds an image's partials in index order
 *     and stores out[b], or adds to it in float32 with accumulate != 0 (chaining the layers as lib/metrics.py:130-133's sum
 *     does).  No float atomics, no memset, no allocation: the same bits on every launch, whatever the batch around an image.
 *   bwd: ONE launch; the norms are recomputed, the forward stashes nothing.  g = g_out[b] / (H W), q[c] = 2 weight[c] (xh - yh):
 *       g_x[b,k,p] = g (q[k] / (rx + eps) - x[k] (sum_c q[c] x[c]) / ((rx + eps)^2 rx))
 *       g_y: the same with x <-> y and q -> -q;  y_normalized: g_y = -g q[k]
 *     Either of g_x / g_y may be NULL (skipped).  Every element is written exactly once, no atomics.  Where a pixel's whole
 *     channel vector is zero the second term is taken as 0: the gradient is the finite g q[k] / eps there, where the
 *     reference's autograd gives NaN (a stated deviation).
 *   x, y: dense [B,C,H,W]; weight [C], the lin layer's weight[0,:,0,0]; eps >= 0 (1e-10 in the reference); out, g_out [B];
 *   g_x, g_y dense [B,C,H,W].  All element offsets are 64-bit.  The forward-only fields (out, accumulate, the workspace) are
 *   ignored by bwd and the g_* fields by fwd.
 *   workspace: device memory, 8-byte aligned, need not be zeroed; nfi_lpips_head_workspace_bytes reads n_images, channels,
 *   height and width alone (one double per block) and returns 0 for a shape the calls refuse.
 * Refused before any launch (-1, nfi_last_error()): a null argument / x / y / weight; out null (fwd); g_out null or both
 * gradients null (bwd); a gradient overlapping x, y or the other gradient; a dimension under 1; eps negative or NaN; a
 * missing, too small or misaligned workspace (fwd); a grid over the launch limit: n_images * ceil(height * width / 64) must
 * be below 2^31. */
typedef struct nfi_lpips_head_args {
  int n_images, channels, height, width;
  const float* x; const float* y; int y_normalized;
  const float* weight; float eps;
  float* out; int accumulate;                    /* forward */
  const float* g_out; float* g_x; float* g_y;    /* backward */
  void* workspace; size_t workspace_bytes;       /* forward only */
} nfi_lpips_head_args;
size_t nfi_lpips_head_workspace_bytes(const nfi_lpips_head_args* a);
int nfi_lpips_head_fwd(const nfi_lpips_head_args* a, nfi_stream_t stream);
int nfi_lpips_head_bwd(const nfi_lpips_head_args* a, nfi_stream_t stream);

/* The tail of a synthesis layer: everything SynthesisLayer.forward (models/stylegan.py:325-356) does AFTER its convolution -
 * filter2d(x, f, gain=4) of an `up` layer (stylegan.py:58-69, 101-105), addcmul(noise, x, dcoefs) (139-140), + bias (351),
 * * act_gain (352-353), leaky_relu (354-355).  All tensors dense float32, NCHW.  With R = resolution:
 *   f   = up ? sum_{a,b in 0..3} (4 taps[a][b]) y[i + a - 1, j + b - 1]   (0 outside y, which is [B,C,R+1,R+1])
 *            : y                                                          (y is [B,C,R,R])
 *   out = lrelu_slope(((noise + f * dcoefs[b,c]) + bias[c]) * act_gain)   [B,C,R,R]; no lrelu with activate == 0
 * Every operation after the filter is rounded on its own, in that order; the filter adds its 16 products in float64, in the
 * order a, b, and rounds once.  taps: the layer's resample_filter buffer, 16 floats ON THE DEVICE, any values (read by the kernels, never
 * copied to the host; not read without up).  noise: NULL, or [B,1,R,R] (noise_shared == 0), or [R,R] for the whole batch
 * (noise_shared != 0).
 *   fwd (stylegan.py:101-105, 139-140, 351-355): ONE launch; y is read once (an up layer stages 64 x 64 tiles with their halo
 *     in LDS) and out written once.
 *   bwd (what autograd records for those lines): out is the forward's result, read for the sign of the pre-activation (hence
 *     act_gain > 0, slope >= 0).  gu = g_out * (out > 0 ? 1 : slope) * act_gain;
 *       g_y      = dcoefs[b,c] * (the adjoint filter of gu, on the R+1 grid)   - or dcoefs * gu without up
 *       g_dcoefs [B,C] = sum_ij gu f   (f recomputed from y),  g_bias [C] = sum_b,ij gu,
 *       g_noise  = sum_c gu [B,1,R,R], or sum_b,c gu [R,R] with noise_shared.
 *     Each may be NULL (skipped), not all four.  One launch for g_y and the per-block float64 sums, one that adds those in
 *     index order into g_dcoefs / g_bias (only when either is asked for), one for g_noise (only when asked for).  No float
 *     atomics: the same bits on every launch.  No gradient for the taps, no second order.
 *   workspace (bwd, only with g_dcoefs or g_bias): device memory, 8-byte aligned, need not be zeroed;
 *   nfi_synth_tail_bwd_workspace_bytes reads batch, channels, resolution and up and returns 0 for a shape the calls refuse.
 * Refused before any launch (-1, nfi_last_error() names the argument): a null argument struct / y / dcoefs / bias / out, null
 * taps with up, null g_out or no gradient pointer (bwd); batch, channels or resolution under 1, resolution over 16384;
 * in_size other than resolution + 1 with up and resolution without; act_gain <= 0 or NaN; slope < 0 or NaN; an element
 * count the index arithmetic cannot hold: batch * channels * blocks per plane (ceil(side / 64)^2 with up, ceil(R R / 4096)
 * without) must be below 2^31; a missing, misaligned or too small workspace (bwd). */
typedef struct nfi_synth_tail_args {
  int batch, channels, resolution;               /* B, C, R */
  int in_size;                                   /* side of y */
  int up, activate;
  float act_gain, slope;
  const float* y; const float* dcoefs; const float* bias; const float* taps;
  const float* noise; int noise_shared;
  float* out;                                    /* written by fwd, read by bwd */
  const float* g_out; float* g_y; float* g_dcoefs; float* g_bias; float* g_noise;    /* backward */
  void* workspace; size_t workspace_bytes;       /* backward */
} nfi_synth_tail_args;
size_t nfi_synth_tail_bwd_workspace_bytes(const nfi_synth_tail_args* a);
int nfi_synth_tail_fwd(const nfi_synth_tail_args* a, nfi_stream_t stream);
int nfi_synth_tail_bwd(const nfi_synth_tail_args* a, nfi_stream_t stream);

/* The head of a synthesis layer: everything SynthesisLayer.forward (models/stylegan.py:325-356) and OutputLayer.forward
 * (372-380) do BEFORE their convolution - the affine, EqualizedLinear.forward (stylegan.py:173-177), the demodulation
 * coefficients of conv_modulated2d (127-130) and the modulation of the input (132) - and what autograd records for those
 * lines.  All tensors float32; B = batch, D = latent_dim, I = in_channels, O = out_channels, K = taps (kh * kw).
 *   styles[b,i] = (sum_d latent[b,d] affine_weight[i,d] weight_gain + affine_bias[i] bias_gain) style_gain          [B,I]
 *   dcoefs[b,o] = rsqrt(sum_i styles[b,i]^2 Q[o,i] + 1e-8),  Q[o,i] = sum_k weight[o,i,k]^2      [B,O], with demodulate
 * style_gain: 1 for a synthesis layer, OutputLayer.weight_gain for toRGB (373).  The reference's [B,O,I,kh,kw] product
 * weight[None] * styles[:, None, :, None, None] (127-128) is never formed: Q is computed from weight inside the kernel, and
 * weight is read once per call for up to 8 images (once per 8 beyond that).  Every sum is added in float64 in a fixed order and
 * rounded to float32 once: no atomics, the same bits on every launch.  dcoefs and the gradients use the rounded styles / dcoefs.
 *   latent: rows of D floats, latent_stride floats apart (>= D: a layer's ws.unbind(1)[k] is read in place); affine_weight
 *   dense [I,D]; affine_bias [I] or NULL; weight dense [O,I,K] (may be NULL without demodulate; O and K are then only checked).
 *   fwd (stylegan.py:173-177, 127-130, 373): writes styles and, with demodulate, dcoefs.  TWO launches, one without demodulate.
 *   bwd: upstream g_styles [B,I] (the modulation's, and toRGB's) and g_dcoefs [B,O] (the tail's), either may be NULL, not both;
 *     styles and dcoefs are the forward's results.  With c[b,o] = g_dcoefs d^3 (0 without g_dcoefs):
 *       g_s[b,i]             = (g_styles[b,i] - styles[b,i] sum_o c[b,o] Q[o,i]) style_gain        (internal, float64)
 *       g_latent[b,d]        = weight_gain sum_i g_s[b,i] affine_weight[i,d]                        dense [B,D]
 *       g_affine_weight[i,d] = weight_gain sum_b g_s[b,i] latent[b,d]                               [I,D]
 *       g_affine_bias[i]     = bias_gain sum_b g_s[b,i]                                             [I]
 *       g_weight[o,i,k]      = -weight[o,i,k] sum_b c[b,o] styles[b,i]^2                            [O,I,K]
 *     g_weight is the demodulation's share only (the convolution's stays with the caller).  Each may be NULL (skipped), not
 *     all four.  At most FOUR launches: one pass over weight (only with g_dcoefs; it writes g_weight too, so weight is read
 *     once with or without it), g_s, g_latent, g_affine_weight with g_affine_bias.  No second order.
 *   workspace (bwd): device memory, 8-byte aligned, need not be zeroed; nfi_synth_head_bwd_workspace_bytes reads batch,
 *   latent_dim, latent_stride, in_channels, out_channels, taps and demodulate and returns 0 for a shape the calls refuse.
 * Refused before any launch (-1, nfi_last_error() names the argument): a null argument struct / latent / affine_weight /
 * styles; batch, latent_dim, in_channels, out_channels or taps under 1; latent_stride under latent_dim; demodulate without
 * weight or without dcoefs; a NaN weight_gain, bias_gain or style_gain; (bwd) no upstream gradient, no gradient pointer,
 * g_dcoefs without dcoefs (or without demodulate / weight), g_weight without g_dcoefs, a missing, misaligned or too small
 * workspace; an element count the index arithmetic cannot hold: batch * latent_stride, batch * in_channels, batch *
 * out_channels, in_channels * latent_dim and out_channels * in_channels * taps must be below 2^31, batch at most 8 * 65535 and
 * out_channels at most 8 * 65535. */
typedef struct nfi_synth_head_args {
  int batch, latent_dim, in_channels, out_channels, taps;      /* B, D, I, O, K */
  int latent_stride;                             /* floats between the rows of latent */
  int demodulate;
  float weight_gain, bias_gain, style_gain;
  const float* latent; const float* affine_weight; const float* affine_bias; const float* weight;
  float* styles; float* dcoefs;                  /* written by fwd, read by bwd */
  const float* g_styles; const float* g_dcoefs;  /* backward: upstream */
  float* g_latent; float* g_affine_weight; float* g_affine_bias; float* g_weight;    /* backward */
  void* workspace; size_t workspace_bytes;       /* backward */
} nfi_synth_head_args;
size_t nfi_synth_head_bwd_workspace_bytes(const nfi_synth_head_args* a);
int nfi_synth_head_fwd(const nfi_synth_head_args* a, nfi_stream_t stream);
int nfi_synth_head_bwd(const nfi_synth_head_args* a, nfi_stream_t stream);

/* The modulation of a layer's input, x * styles.reshape(bs, -1, 1, 1) (stylegan.py:132): x dense [B,C,n] (n = plane = H * W),
 * styles [B,C].
 *   fwd: out[b,c,:] = x[b,c,:] styles[b,c].  ONE launch, flat over the tensor.
 *   bwd: g_x = g_out styles;  g_styles[b,c] = sum_n g_out x, added in float64 in a fixed order (no atomics: the same bits on
 *     every launch).  Either may be NULL (skipped), not both; x is read only for g_styles.  ONE launch: g_x alone is the flat
 *     kernel; with g_styles 16 lanes own a plane up to 256 elements, a wave up to 2048, a block of 1024 threads above.
 *   16-byte accesses where plane % 4 == 0 and x / out / g_out / g_x are 16-byte aligned; a scalar path otherwise.
 * Refused before any launch (-1, nfi_last_error() names the argument): a null argument struct / styles; null x or out (fwd);
 * null g_out, g_x and g_styles both null, g_styles without x (bwd); batch, channels or plane under 1; an element count the
 * index arithmetic cannot hold: batch * channels * plane must be below 2^31. */
typedef struct nfi_synth_modulate_args {
  int batch, channels, plane;                    /* B, C, n */
  const float* x; const float* styles;
  float* out;                                    /* forward */
  const float* g_out; float* g_x; float* g_styles;    /* backward */
} nfi_synth_modulate_args;
int nfi_synth_modulate_fwd(const nfi_synth_modulate_args* a, nfi_stream_t stream);
int nfi_synth_modulate_bwd(const nfi_synth_modulate_args* a, nfi_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * View-direction mapper, the per-ray trunk.  Replaces ViewDirectionMapper.__init__'s layers as forward runs them
 * (models/generator.py:194-241: fc0 .. fc6, norm1 .. norm4, two residual joins scaled by sqrt(2)/2, LeakyReLU(0.2);
 * EqualizedLinear gains 1/sqrt(in), models/stylegan.py:170-177) by ONE launch forward and ONE launch backward, with no
 * per-layer tensor in memory; the closure the class returns (243-251) is part of the field / render kernels (ray_features).
 * Exact fp32 (plain FMAs).  All parameters are the modules' RAW tensors:
 *   fc0_w [64,3] fc0_b [64];  fc1_w .. fc4_w [64,64] (no bias);  norm1_w/_b .. norm4_w/_b [64] (nn.LayerNorm(64), biased
 *   variance, eps 1e-5);  fc5_w [64,64] fc5_b [64];  fc6_w [32,64] fc6_b [32].
 *   fwd: viewdir [N,3] -> feature [N,32] (fc6's output; N is any positive count).  Deterministic: no atomics.
 *   bwd: upstream g_feature [N,32] -> the 18 parameter gradients, shaped like the parameters, raw-parameter gradients
 *        with the gains applied, all ACCUMULATED into caller-initialised buffers as nfi_sdf_gradient_bwd does (zero them
 *        for a plain gradient; a second call into the same buffers adds its gradient to the first's; fp32 atomics, so
 *        the summation order over rays is not fixed), and g_viewdir [N,3] or NULL = not wanted (WRITTEN, every row).
 *        The 18 parameter-gradient pointers are given all or none: with none (a frozen generator, only g_viewdir
 *        wanted) the weight-gradient stages and every atomic are skipped; g_viewdir must then be given.
 *        The forward is recomputed per ray; no workspace, nothing is stashed by the forward.
 *   Alignment: feature and g_feature are accessed as 16-byte vectors and must be 16-byte aligned (rows of 128 B).
 *   Forward-only fields (feature) are ignored by bwd and the g_* fields by fwd.
 * ------------------------------------------------------------------------------------------ */
typedef struct nfi_viewdir_mapper_args {
  int64_t n_rays;
  const float* viewdir;
  const float *fc0_w, *fc0_b;
  const float *fc1_w, *norm1_w, *norm1_b;
  const float *fc2_w, *norm2_w, *norm2_b;
  const float *fc3_w, *norm3_w, *norm3_b;
  const float *fc4_w, *norm4_w, *norm4_b;
  const float *fc5_w, *fc5_b, *fc6_w, *fc6_b;
  float* feature;                /* forward output */
  const float* g_feature;        /* backward input */
  float *g_fc0_w, *g_fc0_b;
  float *g_fc1_w, *g_norm1_w, *g_norm1_b;
  float *g_fc2_w, *g_norm2_w, *g_norm2_b;
  float *g_fc3_w, *g_norm3_w, *g_norm3_b;
  float *g_fc4_w, *g_norm4_w, *g_norm4_b;
  float *g_fc5_w, *g_fc5_b, *g_fc6_w, *g_fc6_b;
  float* g_viewdir;              /* [N,3] out or NULL */
} nfi_viewdir_mapper_args;
int nfi_viewdir_mapper_fwd(const nfi_viewdir_mapper_args* a, nfi_stream_t stream);
int nfi_viewdir_mapper_bwd(const nfi_viewdir_mapper_args* a, nfi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFI_HIP_H */
