// The kernel families around the renderer - regulariser, neighbour / metric kernels, hand-off, PnP, pose algebra, blur,
// LPIPS head, view-direction mapper, synthesis-layer tail and head - as their own translation unit.
//
// None of them uses anything of nfi_kernels.hip, and nothing there uses them: with a code object of their own, adding or
// editing a family leaves the benchmarked render, stage and field kernels where they are in theirs.  Built with the
// library's plain flags (__graft_entry__.UNITS).  Each family's first comment says what it holds; all they share beyond
// nfi_host.hpp / nfi_device.hpp is ord_sort_by_cell (nfi_regulariser.inc; defined in nfi_backward_field.inc).
#include "nfi_host.hpp"

#include <algorithm>
#include <cstring>

using namespace nfi;

#include "nfi_regulariser.inc"
#include "nfi_neighbours.inc"
#include "nfi_handoff.inc"
#include "nfi_pnp.inc"
#include "nfi_pose.inc"
#include "nfi_filter.inc"
#include "nfi_lpips.inc"
#include "nfi_viewdir_mapper.inc"
#include "nfi_synth_tail.inc"
#include "nfi_synth_head.inc"
