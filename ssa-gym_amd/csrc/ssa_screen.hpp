// ssa_screen.hpp -- the visibility screen of a synthetic orbit catalogue (include/ssa_hip.h: ssa_catalogue_screen_f64).
//
// catalogue._accepted (orbit_gen.py's acceptance rule) operation for operation, with the observer generalised to a network of
// S sites: a sample is visible when ANY site sees it above its own mask.
//
// Mapping: one wavefront per candidate, lane l runs samples l, l + 64, ... -- the per-sample work (12 Newton
// steps of Kepler's equation, the c2t rotation, the altitude and S elevations) is independent across samples, so a draw-loop batch
// of 4 096 candidates is 4 096 wavefronts (4 per SIMD) instead of 64.  Visibility and the altitude test become 64-bit ballots per
// chunk of 64 samples; the longest invisible run and the first-window test are folded from those masks, identically in every lane.
#pragma once

#define SSA_SCREEN_WAVES 4          // wavefronts (= candidates) per workgroup

namespace screen {
constexpr double WGS84_A = 6378137.0;                 // catalogue.WGS84_A / WGS84_F
constexpr double WGS84_F = 0.0033528106647474805;
constexpr int SITE_WORDS = 13;                        // enu[9] (row-major, as host.enu_matrix), obs_itrs[3], el_min [rad]
}

__global__ void __launch_bounds__(64 * SSA_SCREEN_WAVES) catalogue_screen_kernel(const ssa_screen_params p)
{
    const int64_t c = (int64_t)blockIdx.x * SSA_SCREEN_WAVES + threadIdx.x / 64;
    if (c >= p.n) return;                              // a whole wavefront leaves together
    const int lane = threadIdx.x & 63;
    const double* el = p.elements + c * 6;
    const double a = el[0], e = el[1], inc = el[2], raan = el[3], argp = el[4], nu = el[5];

    // perifocal unit vectors in GCRS, the anomaly at t = 0, mean motion and semi-minor axis (as _accepted)
    const double cO = cos(raan), sO = sin(raan), ci = cos(inc), si = sin(inc), cw = cos(argp), sw = sin(argp);
    const double P0 = cO * cw - sO * ci * sw, P1 = sO * cw + cO * ci * sw, P2 = si * sw;
    const double Q0 = -cO * sw - sO * ci * cw, Q1 = -sO * sw + cO * ci * cw, Q2 = si * cw;
    const double E0 = 2.0 * atan2(sqrt(1.0 - e) * sin(nu / 2.0), sqrt(1.0 + e) * cos(nu / 2.0));
    const double M0 = E0 - e * sin(E0);
    const double nmot = sqrt(ssa::MU / (a * a * a));
    const double b = a * sqrt(1.0 - e * e);

    const int T = p.n_time;
    int run = 0, worst = 0;
    bool alt_ok = true, first_vis = false, always = true;
    for (int base = 0; base < T; base += 64) {
        const int i = base + lane;
        bool alt_bad = false, vis = false;
        if (i < T) {
            const double t = p.step * i;
            const double M = M0 + nmot * t;
            double E = M + e * sin(M);
            for (int it = 0; it < 12; ++it)            // fixed count, no early exit: numpy's loop
                E = E - (E - e * sin(E) - M) / (1.0 - e * cos(E));
            const double ra = a * (cos(E) - e), rb = b * sin(E);
            const double r0 = ra * P0 + rb * Q0, r1 = ra * P1 + rb * Q1, r2 = ra * P2 + rb * Q2;
            const double* Mt = p.trans + (int64_t)i * 9;   // x = trans[i] . r  (numpy: r @ M_t[i].T)
            const double x0 = Mt[0] * r0 + Mt[1] * r1 + Mt[2] * r2;
            const double x1 = Mt[3] * r0 + Mt[4] * r1 + Mt[5] * r2;
            const double x2 = Mt[6] * r0 + Mt[7] * r1 + Mt[8] * r2;
            const double rn = sqrt(x0 * x0 + x1 * x1 + x2 * x2);
            const double sl = sin(asin(x2 / rn));
            alt_bad = !(rn - screen::WGS84_A * (1.0 - screen::WGS84_F * (sl * sl)) > p.min_alt);   // NaN fails, as in numpy
            for (int s = 0; s < p.n_site; ++s) {
                const double* q = p.sites + s * screen::SITE_WORDS;
                const double d0 = x0 - q[9], d1 = x1 - q[10], d2 = x2 - q[11];
                const double up = d0 * q[2] + d1 * q[5] + d2 * q[8];          // d @ enu[:, 2]
                vis |= asin(up / sqrt(d0 * d0 + d1 * d1 + d2 * d2)) >= q[12];
            }
        }
        const unsigned long long vmask = __ballot(vis), amask = __ballot(alt_bad);
        const int cnt = min(64, T - base);
        const unsigned long long full = cnt == 64 ? ~0ull : (1ull << cnt) - 1;
        alt_ok = alt_ok && amask == 0;
        always = always && vmask == full;
        if (base < p.first) {
            const int w = min(cnt, p.first - base);
            first_vis = first_vis || (vmask & (w == 64 ? ~0ull : (1ull << w) - 1)) != 0;
        }
        for (int k = 0; k < cnt; ++k) {               // runs of invisible samples, carried across chunks (wave-uniform)
            run = (vmask >> k) & 1 ? 0 : run + 1;
            worst = max(worst, run);
        }
    }
    if (lane == 0) {
        p.accept[c] = alt_ok && (always || (first_vis && worst < p.max_gap)) ? 1 : 0;
        if (p.worst_gap) p.worst_gap[c] = worst;
        if (p.flags) p.flags[c] = (alt_ok ? 1 : 0) | (first_vis ? 2 : 0) | (always ? 4 : 0);
    }
}
