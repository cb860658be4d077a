// ssa_screen_body.hpp -- the body of the two catalogue screen kernels; ssa_screen.hpp includes it once per value of SSA_SCREEN_NETWORK.
//   SSA_SCREEN_NETWORK 0: catalogue_screen_kernel, the ground-mask screen -- what is left after preprocessing is that
//                         kernel's source as it was before the network instance existed, token for token
//   SSA_SCREEN_NETWORK 1: catalogue_screen_network_kernel, every sensor judged by its own rule
#if SSA_SCREEN_NETWORK
__global__ void __launch_bounds__(64 * SSA_SCREEN_WAVES) catalogue_screen_network_kernel(const ssa_screen_network_params net)
{
    const ssa_screen_params& p = net.base;
#else
__global__ void __launch_bounds__(64 * SSA_SCREEN_WAVES) catalogue_screen_kernel(const ssa_screen_params p)
{
#endif
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
#if SSA_SCREEN_NETWORK
    unsigned seen = 0;                                 // bit s: this lane saw the candidate from sensor s at one of its samples
#endif
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
#if SSA_SCREEN_NETWORK
            // the sunlit verdict belongs to the sample, not to a sensor: once, from the lane's own Sun row, and only if some sensor asks
            bool lit = false;
            long long dark = 0;
            if (net.sunlit_only != 0) {
                const double* srow = net.sun + (int64_t)i * screen::SUN_ROW;
                const double r[3] = {r0, r1, r2};
                lit = ssa::sunlit_cylinder(r, srow, net.shadow_radius);
                dark = ((const long long*)srow)[3];
            }
#endif
            for (int s = 0; s < p.n_site; ++s) {       // (network: s and both sensor words are wave-uniform -- scalar branches)
#if SSA_SCREEN_NETWORK
                if ((net.site_moving >> s) & 1) {        // a moving sensor: its own row's obs_itrs, the limb sphere, no night
                    const double* row = net.site_rows + ((int64_t)i * p.n_site + s) * screen::SITE_ROW + 9;
                    const double o[3] = {row[0], row[1], row[2]};
                    const double d[3] = {x0 - o[0], x1 - o[1], x2 - o[2]};
                    bool v = ssa::los_clear(d, o, net.limb_radius);
                    if ((net.sunlit_only >> s) & 1) v = v && lit;
                    vis |= v;
                    seen |= (v ? 1u : 0u) << s;
                    continue;
                }
#endif
                const double* q = p.sites + s * screen::SITE_WORDS;
                const double d0 = x0 - q[9], d1 = x1 - q[10], d2 = x2 - q[11];
                const double up = d0 * q[2] + d1 * q[5] + d2 * q[8];          // d @ enu[:, 2]
#if SSA_SCREEN_NETWORK
                bool v = asin(up / sqrt(d0 * d0 + d1 * d1 + d2 * d2)) >= q[12];
                if ((net.sunlit_only >> s) & 1) v = v && lit && ((dark >> s) & 1);       // a telescope: a dark site and a sunlit object
                vis |= v;
                seen |= (v ? 1u : 0u) << s;
#else
                vis |= asin(up / sqrt(d0 * d0 + d1 * d1 + d2 * d2)) >= q[12];
#endif
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
#if SSA_SCREEN_NETWORK
    unsigned seen_any = 0;                             // (a ballot per sensor: every lane takes part)
    if (net.seen_by)
        for (int s = 0; s < p.n_site; ++s) seen_any |= (__ballot((seen >> s) & 1) != 0 ? 1u : 0u) << s;
#endif
    if (lane == 0) {
        p.accept[c] = alt_ok && (always || (first_vis && worst < p.max_gap)) ? 1 : 0;
        if (p.worst_gap) p.worst_gap[c] = worst;
        if (p.flags) p.flags[c] = (alt_ok ? 1 : 0) | (first_vis ? 2 : 0) | (always ? 4 : 0);
#if SSA_SCREEN_NETWORK
        if (net.seen_by) net.seen_by[c] = (uint8_t)seen_any;
#endif
    }
}
