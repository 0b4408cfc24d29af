// nfi_kernels.hip — the core translation unit of libnfi_hip.so (gfx950 / MI355X only): the fused render, the staged ray
// kernels and the field query, forward.  See include/nfi_hip.h for the contract and nfi_device.hpp for the building blocks.
// This file is the list of topics; the code is in the .inc files, in the order the compiler has to see it.
// (The other units: nfi_backward_field.hip - the field backward, built without SLP vectorisation - and nfi_modules.hip -
// every kernel family around the renderer, regulariser ... synthesis tail.)
#include "nfi_device.hpp"
#include "../../include/nfi_hip.h"
#include "nfi_host.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <type_traits>

using namespace nfi;

// error plumbing, argument checks and the LDS staging helpers shared with the other units: nfi_host.hpp
thread_local char nfi_err_buf[256] = "";
extern "C" const char* nfi_last_error(void) { return nfi_err_buf; }
extern "C" int nfi_version(void) { return 107; }

#include "nfi_layout.inc"           // planes <-> texels, the decoder image packers
#include "nfi_rays.inc"             // ray generation, near / far planes, stratified query points
#include "nfi_field_query.inc"      // field query forward, bounding-box overlay
#include "nfi_wave_slab.inc"        // per-wave LDS slab: inverse CDF, resampling, merge, composite (device helpers only)
#include "nfi_ray_stages.inc"       // the stand-alone stage kernels on those helpers
#include "nfi_backward_rays.inc"    // and their backward

// Register-budget work compiles ONE render kernel (tools/vgpr_liveness.py, the ISA tests), in seconds instead of minutes:
//   hipcc -S --cuda-device-only -DNFI_SINGLE_KERNEL=<TEX> [-DNFI_SINGLE_MODE=<kRender...>] -DNFI_RENDER_OCC=<waves per SIMD>
// instantiates the plain 64-sample inference kernel of one texel storage type, + -DNFI_SINGLE_WIDE the 128-sample one
// (both inside nfi_render_kernels.inc, next to their kernels), and leaves out the long kernel and the host side:
#include "nfi_render_kernels.inc"   // parameters, work queues, the 64- and the 128-sample persistent kernels
#ifndef NFI_SINGLE_KERNEL
#include "nfi_render_long.inc"      // the single-pass kernel for up to 512 samples
#include "nfi_render_host.inc"      // workspace, set-up, checks, select_render_kernel, nfi_render_fwd
#endif  // NFI_SINGLE_KERNEL
