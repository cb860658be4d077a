// ssa_access.hpp -- the pass table of a sensor network (include/ssa_hip.h: ssa_access_sensors_f64).
//
// The visibility test of every fused kernel is judged on the TRUE state, and the truth chain x_true[i + 1] = propagate(x_true[i], dt)
// depends on no action, no noise draw and no filter: the verdict of every (step, sensor, object) cell of the rest of an episode is
// known when the episode starts.  This kernel walks that chain once and keeps every verdict, one bit per cell, packed along TIME.
//
// Mapping: one lane per object, the truth in registers across the T steps; every env starts on a wavefront boundary (block = one
// wavefront, grid = selected envs x ceil(m / 64)), so that the env, its time word and with it the rows of `trans`, the Sun table and the
// site table are wave-uniform -- their addresses are formed from scalars and the rows come by scalar loads from the constant address
// space (nothing of the launch writes those tables).  Per step: one propagation, then the sensors in turn -- the loop over them is
// unrolled over SSA_MAX_SENSORS with a wave-uniform guard, so that the per-sensor words and summaries below are registers (an array
// indexed by a loop counter would live in scratch).  A sensor's verdict is shifted into its current 64-bit word; the word is stored when
// it fills and once more at the end, by a plain 8-byte store at the row the CALLER numbers the object by (obj_ids).  No LDS, no
// atomics, no workspace.
//
// The verdict is the fused kernels' own (process_wave, lane 13): hx_aer_enu's elevation against the sensor's mask; for a moving sensor
// observer_to_object + los_clear on the row's obs_itrs words behind the barrier hx_moving_site documents; sunlit_cylinder and the row's
// dark bit where the sensor asks; time_row for the row.  The propagation is the stand-alone operators' (propagate_kernel,
// propagate_hybrid_kernel, propagate_j2_kernel): the device functions the step kernels run on a healthy state, with the operators'
// complete semantics for a state outside the series solver's domain.
#pragma once

namespace ssa {

struct AccessK {
    ssa_step_params p;
    ssa_sensor_params s;
    ssa_access_params a;
    double dt;
    J2Params j2;
    int32_t waves_per_env;
};

// x -> the truth one step later, as the stand-alone propagate operator of PROP computes it
template <int PROP>
SSA_DEV void access_propagate(const double* x, const AccessK& k, double* o)
{
    if constexpr (PROP == SSA_PROP_J2_RK4) {
        propagate_j2_rk4(x, k.dt, k.j2, o);
    } else if constexpr (PROP == SSA_PROP_HYBRID) {
        bool fast = kepler_hybrid_fast(x, k.dt, o);
        if (__any(!fast)) {       // propagate_hybrid_kernel's tiers: strong-hyperbolic inline, the rest out of line
            if (!fast) fast = kepler_conic_lean<0, true>(x, k.dt, o);
        }
        if (__any(!fast)) {
            if (!fast) {
                Vec6 si;
#pragma unroll
                for (int c = 0; c < 6; ++c) si.v[c] = x[c];
                Vec6 oo = kepler_beyond_series_tagged<0>(si, k.dt);
#pragma unroll
                for (int c = 0; c < 6; ++c) o[c] = oo.v[c];
            }
        }
    } else kepler_step<PROP>(x, k.dt, o);
}

// the running pass summary of one (sensor, object) row: first step seen, length of that first pass, steps seen, passes
struct AccessRow {
    unsigned long long word;
    int first, length, count, passes;
};

template <int PROP>
__global__ void __launch_bounds__(64) access_sensors_kernel(const AccessK k)
{
    // (everything up to `lane` is wave-uniform: the block is one wavefront)
    const int sel = (int)(blockIdx.x / (unsigned)k.waves_per_env);
    const int wv = (int)(blockIdx.x - (unsigned)sel * (unsigned)k.waves_per_env);
    int e = sel;
    if (k.a.n_sel > 0) e = ((ConstPtr<int32_t>)k.a.env_sel)[sel];
    if ((unsigned)e >= (unsigned)k.p.n_env) return;      // (a selection word outside the launch: the whole wavefront leaves, nothing is written)
    const int lane = threadIdx.x;
    const int64_t m = k.p.n_obj;
    const int64_t i = (int64_t)wv * 64 + lane;
    const bool ok = i < m;
    const int64_t ii = ok ? i : 0;      // padding lanes run the env's object 0 and store nothing: the solvers' __all() loops need a convergent wave
    const int S = k.s.n_sensor;
    const int T = k.a.n_steps;
    const int W = (T + 63) >> 6;
    int left = T;
    if (k.a.n_left) left = min(T, max(0, ((ConstPtr<int32_t>)k.a.n_left)[e]));
    const int t0 = __builtin_amdgcn_readfirstlane(env_time_of(k.p, e)) + k.p.time_offset;
    const unsigned moving = (unsigned)k.p.site_moving, sunlit = (unsigned)k.s.sunlit_only;

    double x[6];
    {
        const double* src = k.p.x_true_in + ((int64_t)e * m + ii) * 6;
#pragma unroll
        for (int c = 0; c < 6; ++c) x[c] = src[c];
    }
    // the row of this lane's object in the caller's numbering; a lane whose row would lie outside the env stores nothing
    int64_t id = i;
    if (k.p.obj_ids) id = k.p.obj_ids[(int64_t)e * m + ii];
    const bool live = ok && (uint64_t)id < (uint64_t)m;
    const int64_t row0 = ((int64_t)e * S * m + id);      // row (e, 0, id); sensor s: + s * m

    AccessRow r[SSA_MAX_SENSORS];
#pragma unroll
    for (int s = 0; s < SSA_MAX_SENSORS; ++s) r[s] = AccessRow{0ull, -1, 0, 0, 0};
    unsigned prev = 0;      // bit s: sensor s saw the object at the step before

    for (int h = 0; h < left; ++h) {
        double o[6];
        access_propagate<PROP>(x, k, o);
#pragma unroll
        for (int c = 0; c < 6; ++c) x[c] = o[c];
        const int trow = __builtin_amdgcn_readfirstlane(time_row(t0 + h, k.p.n_time));
        double Mm[9];
        {
            const ConstPtr<double> Mrow = (ConstPtr<double>)k.p.trans + (int64_t)trow * 9;
#pragma unroll
            for (int c = 0; c < 9; ++c) Mm[c] = Mrow[c];
        }
        bool lit = false;
        long long dark = 0;
        if (sunlit != 0) {      // (wave-uniform: the Sun row is not read unless some sensor asks)
            const ConstPtr<double> srow = (ConstPtr<double>)__builtin_assume_aligned(k.s.sun, 32) + (int64_t)trow * 4;
            const double sun[3] = {srow[0], srow[1], srow[2]};
            dark = __double_as_longlong(srow[3]);
            lit = sunlit_cylinder(x, sun, k.s.shadow_radius);
        }
        const int bit = h & 63;
#pragma unroll
        for (int s = 0; s < SSA_MAX_SENSORS; ++s) {
            if (s < S) {      // (wave-uniform)
                bool v;
                if ((moving >> s) & 1) {      // a moving sensor: its own row's obs_itrs, the limb sphere, no horizon, no night
                    const ConstPtr<double> site =
                        (ConstPtr<double>)__builtin_assume_aligned(k.p.site_rows, 128) + ((int64_t)trow * S + s) * 16 + 9;
                    const double obs[3] = {site[0], site[1], site[2]};
                    double d[3];
                    observer_to_object(x, Mm, obs, d);
                    SSA_OPAQUE(d[0]);
                    SSA_OPAQUE(d[1]);
                    SSA_OPAQUE(d[2]);
                    v = los_clear(d, obs, k.p.limb_radius);
                    if ((sunlit >> s) & 1) v = v && lit;
                } else {
                    double aer[3], enu_vec[3];
                    hx_aer_enu(x, Mm, k.s.enu[s], k.s.obs_itrs[s], aer, enu_vec);
                    v = aer[1] >= k.s.obs_limit[s];      // (a NaN elevation is below every mask)
                    if ((sunlit >> s) & 1) v = v && lit && ((dark >> s) & 1);
                }
                const int vb = v ? 1 : 0;
                r[s].word |= (unsigned long long)vb << bit;
                r[s].count += vb;
                r[s].passes += vb & (int)(~(prev >> s) & 1u);
                if (v && r[s].first < 0) r[s].first = h;
                r[s].length += (v && r[s].passes == 1) ? 1 : 0;
                prev = (prev & ~(1u << s)) | ((unsigned)vb << s);
            }
        }
        if (bit == 63) {      // the words are full: one store per sensor, then they start again
#pragma unroll
            for (int s = 0; s < SSA_MAX_SENSORS; ++s) {
                if (s < S) {
                    if (live) k.a.bits[(row0 + (int64_t)s * m) * W + (h >> 6)] = r[s].word;
                    r[s].word = 0ull;
                }
            }
        }
    }
    if (!live) return;
    // the word the loop left unfinished, and zeros for every word behind the steps counted
    const int done = left >> 6;      // words the loop stored
#pragma unroll
    for (int s = 0; s < SSA_MAX_SENSORS; ++s) {
        if (s < S) {
            uint64_t* dst = k.a.bits + (row0 + (int64_t)s * m) * W;
            for (int w = done; w < W; ++w) dst[w] = (w == done) ? r[s].word : 0ull;
            if (k.a.pass) {
                int32_t* ps = k.a.pass + (row0 + (int64_t)s * m) * 4;
                ps[0] = r[s].first;
                ps[1] = r[s].length;
                ps[2] = r[s].count;
                ps[3] = r[s].passes;
            }
        }
    }
}

}  // namespace ssa
