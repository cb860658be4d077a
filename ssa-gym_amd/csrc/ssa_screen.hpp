// ssa_screen.hpp -- the visibility screen of a synthetic orbit catalogue (include/ssa_hip.h: ssa_catalogue_screen_f64 and
// ssa_catalogue_screen_network_f64).
//
// catalogue._accepted (orbit_gen.py's acceptance rule) operation for operation, with the observer generalised to a network of
// S sites: a sample is visible when ANY site sees it above its own mask.
//
// Mapping: one wavefront per candidate, lane l runs samples l, l + 64, ... -- the per-sample work (12 Newton
// steps of Kepler's equation, the c2t rotation, the altitude and S elevations) is independent across samples, so a draw-loop batch
// of 4 096 candidates is 4 096 wavefronts (4 per SIMD) instead of 64.  Visibility and the altitude test become 64-bit ballots per
// chunk of 64 samples; the longest invisible run and the first-window test are folded from those masks, identically in every lane.
//
// One body, two kernels: ssa_screen_body.hpp is compiled twice.  With SSA_SCREEN_NETWORK 0 it is
// catalogue_screen_kernel, the ground-mask screen of 8e, exactly as it stood; with 1 it is catalogue_screen_network_kernel, which judges
// every sensor by the rule the fused kernels apply to it -- a moving sensor by los_clear on its own site row, a sunlit_only sensor
// by sunlit_cylinder (and, on the ground, its dark bit).  The flag is the preprocessor's and not a template's because the old kernel's
// instruction stream is to stay what it was: merely calling the unchanged body as an inlined function reorders its epilogue.
#pragma once

#define SSA_SCREEN_WAVES 4          // wavefronts (= candidates) per workgroup

namespace screen {
constexpr double WGS84_A = 6378137.0;                 // catalogue.WGS84_A / WGS84_F
constexpr double WGS84_F = 0.0033528106647474805;
constexpr int SITE_WORDS = 13;                        // enu[9] (row-major, as host.enu_matrix), obs_itrs[3], el_min [rad]
constexpr int SITE_ROW = 16;                          // doubles per (sample, sensor) of site_rows: enu[9], obs_itrs[3], 4 unread
constexpr int SUN_ROW = 4;                            // doubles per sample of sun: sx, sy, sz, the int64 word of dark bits
}

#define SSA_SCREEN_NETWORK 0
#include "ssa_screen_body.hpp"
#undef SSA_SCREEN_NETWORK
#define SSA_SCREEN_NETWORK 1
#include "ssa_screen_body.hpp"
#undef SSA_SCREEN_NETWORK
