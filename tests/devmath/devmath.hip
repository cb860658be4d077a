// The per-lane device math of the product (ssa-gym_amd/csrc/ssa_math.hpp, ssa_conics.hpp) as GPU kernels: one kernel per hm_*
// entry point of tests/hostmath/hostmath.cpp, compiled with the library's own hipcc flags (ssa-gym_amd/_build.py HIPCC_FLAGS).
// Test-only: tests/test_device_math_gpu.py runs the host pins on the device, and the bit-identity tests lay items out in chosen
// orders.  Every kernel processes ONE item per lane in 64-lane blocks, in array order -- the caller chooses a lane's wavefront
// neighbours by ordering the input -- and its padding lanes compute on item 0, as propagate_kernel's do.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../ssa-gym_amd/csrc/ssa_math.hpp"
#include "../../ssa-gym_amd/csrc/ssa_conics.hpp"

namespace ssa {   // (the out-of-line wrappers of ssa_kernels.hip)
__device__ __noinline__ Vec6 kepler_general_v(Vec6 x, double tof)
{
    Vec6 o;
    kepler_general_impl(x.v, tof, o.v, nullptr);
    return o;
}
__device__ __noinline__ Vec8 kepler_general_diag_v(Vec6 x, double tof, Vec6* out)
{
    Vec8 d;
    Vec6 o;
    kepler_general_impl(x.v, tof, o.v, d.v);
    *out = o;
    return d;
}
}  // namespace ssa

namespace {
constexpr int BLOCK = 64;

__device__ inline int64_t item(int64_t n, bool& ok)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    ok = i < n;
    return ok ? i : 0;      // padding lanes recompute item 0 (the wave stays convergent for the votes)
}
__device__ inline void load6(const double* x, int64_t i, double* v)
{
#pragma unroll
    for (int c = 0; c < 6; ++c) v[c] = x[i * 6 + c];
}
__device__ inline void store6(double* y, int64_t i, const double* v)
{
#pragma unroll
    for (int c = 0; c < 6; ++c) y[i * 6 + c] = v[c];
}

// prop 1: SSA_PROP_FG (kepler_fg_fast), prop 0: SSA_PROP_ELEMENTS strong-elliptic path (kepler_elements_fast); ok = handled
template <int PROP>
__global__ void k_propagate(const double* x, int64_t n, double dt, double* out, int32_t* okf)
{
    bool ok;
    const int64_t i = item(n, ok);
    double s[6], o[6];
    load6(x, i, s);
    const bool h = PROP == 1 ? ssa::kepler_fg_fast<0>(s, dt, o) : ssa::kepler_elements_fast(s, dt, o);
    if (ok) { store6(out, i, o); okf[i] = h; }
}
// SSA_PROP_J2_RK4 (propagate_j2_rk4): nsub RK4 sub-steps under (j2, r_eq); ok = its return value
__global__ void k_propagate_j2(const double* x, int64_t n, double dt, ssa::J2Params q, double* out, int32_t* okf)
{
    bool ok;
    const int64_t i = item(n, ok);
    double s[6], o[6];
    load6(x, i, s);
    const bool h = ssa::propagate_j2_rk4(s, dt, q, o);
    if (ok) { store6(out, i, o); okf[i] = h; }
}
__global__ void k_uv_fast(const double* x, int64_t n, double dt, double* out, int32_t* handled)
{
    bool ok;
    const int64_t i = item(n, ok);
    double s[6], o[6];
    load6(x, i, s);
    bool h;
    ssa::kepler_uv_fast(s, dt, o, h);
    if (ok) { store6(out, i, o); handled[i] = h; }
}
__global__ void k_uv_general(const double* x, int64_t n, double dt, double* out, int32_t* okf)
{
    bool ok;
    const int64_t i = item(n, ok);
    double s[6], o[6];
    load6(x, i, s);
    const bool h = ssa::kepler_uv_general(s, dt, o);
    if (ok) { store6(out, i, o); okf[i] = h; }
}
__global__ void k_general_libm(const double* x, int64_t n, double dt, double* out, int32_t* okf)
{
    bool ok;
    const int64_t i = item(n, ok);
    double s[6], o[6];
    load6(x, i, s);
    ssa::kepler_general_impl(s, dt, o, nullptr);
    if (ok) { store6(out, i, o); okf[i] = 1; }
}
__global__ void k_general_fast(const double* x, int64_t n, double dt, double* out, int32_t* okf)
{
    bool ok;
    const int64_t i = item(n, ok);
    ssa::Vec6 s;
    load6(x, i, s.v);
    const ssa::Vec6 o = ssa::kepler_general_fast_impl<0>(s, dt);
    if (ok) { store6(out, i, o.v); okf[i] = 1; }
}
__global__ void k_conic_lean(const double* x, int64_t n, double dt, double* out, int32_t* okf)
{
    bool ok;
    const int64_t i = item(n, ok);
    double s[6], o[6];
    load6(x, i, s);
#pragma unroll
    for (int c = 0; c < 6; ++c) o[c] = __builtin_nan("");
    const bool h = ssa::kepler_conic_lean<0, false>(s, dt, o);
    if (ok) { store6(out, i, o); okf[i] = h; }
}
// the band functions alone: nu(t0 + tof) from (nu, ecc, q), fast and libm
__global__ void k_band(const double* nu, const double* ecc, const double* q, int64_t n, double tof, double* fast, double* libm)
{
    bool ok;
    const int64_t i = item(n, ok);
    const double f = ssa::genf::nu_from_delta_t_band(ssa::genf::delta_t_from_nu_band(nu[i], ecc[i], q[i]) + tof, ecc[i], q[i]);
    const double l = ssa::gen::nu_from_delta_t(ssa::gen::delta_t_from_nu(nu[i], ecc[i], ssa::MU, q[i]) + tof, ecc[i], ssa::MU, q[i]);
    if (ok) { fast[i] = f; libm[i] = l; }
}
__global__ void k_log_pos(const double* x, int64_t n, double* r)
{
    bool ok;
    const int64_t i = item(n, ok);
    const double v = ssa::genf::log_pos(x[i]);
    if (ok) r[i] = v;
}
__global__ void k_sincos_fast(const double* x, int64_t n, double* s, double* c)
{
    bool ok;
    const int64_t i = item(n, ok);
    double sv, cv;
    ssa::sincos_fast(x[i], sv, cv);
    if (ok) { s[i] = sv; c[i] = cv; }
}
__global__ void k_atan2_fast(const double* y, const double* x, int64_t n, double* r)
{
    bool ok;
    const int64_t i = item(n, ok);
    const double v = ssa::atan2_fast(y[i], x[i]);
    if (ok) r[i] = v;
}
__global__ void k_exp_fast(const double* x, int64_t n, double* r)
{
    bool ok;
    const int64_t i = item(n, ok);
    const double v = ssa::exp_fast(x[i]);
    if (ok) r[i] = v;
}
__global__ void k_recip(const double* x, int64_t n, double* r, double* rs)
{
    bool ok;
    const int64_t i = item(n, ok);
    const double a = ssa::rcp_nr(x[i]), b = ssa::rsqrt_nr(x[i]);
    if (ok) { r[i] = a; rs[i] = b; }
}

inline dim3 grid(int64_t n) { return dim3((unsigned)((n + BLOCK - 1) / BLOCK)); }
inline int status() { return (int)hipGetLastError(); }
}  // namespace

// launchers: device pointers, n, stream; 0 = launched (a HIP error code otherwise); n <= 0 launches nothing
#define DM_LAUNCH(kern, ...)                                                                                       \
    do {                                                                                                           \
        if (n <= 0) return 0;                                                                                      \
        hipLaunchKernelGGL(kern, grid(n), dim3(BLOCK), 0, (hipStream_t)stream, __VA_ARGS__);                       \
        return status();                                                                                           \
    } while (0)

extern "C" {
int dm_propagate(const double* x, int64_t n, double dt, int32_t prop, double* out, int32_t* ok, void* stream)
{
    if (prop == 1) DM_LAUNCH(k_propagate<1>, x, n, dt, out, ok);
    if (prop == 0) DM_LAUNCH(k_propagate<0>, x, n, dt, out, ok);
    return -1;
}
int dm_propagate_j2(const double* x, int64_t n, double dt, double j2, double r_eq, int32_t nsub, double* out, int32_t* ok, void* stream)
{
    if (nsub < 1) return -1;
    const ssa::J2Params q = {j2, r_eq, nsub};
    DM_LAUNCH(k_propagate_j2, x, n, dt, q, out, ok);
}
int dm_uv_fast(const double* x, int64_t n, double dt, double* out, int32_t* handled, void* stream) { DM_LAUNCH(k_uv_fast, x, n, dt, out, handled); }
int dm_uv_general(const double* x, int64_t n, double dt, double* out, int32_t* ok, void* stream) { DM_LAUNCH(k_uv_general, x, n, dt, out, ok); }
int dm_general_libm(const double* x, int64_t n, double dt, double* out, int32_t* ok, void* stream) { DM_LAUNCH(k_general_libm, x, n, dt, out, ok); }
int dm_general_fast(const double* x, int64_t n, double dt, double* out, int32_t* ok, void* stream) { DM_LAUNCH(k_general_fast, x, n, dt, out, ok); }
int dm_conic_lean(const double* x, int64_t n, double dt, double* out, int32_t* ok, void* stream) { DM_LAUNCH(k_conic_lean, x, n, dt, out, ok); }
int dm_band(const double* nu, const double* ecc, const double* q, int64_t n, double tof, double* fast, double* libm, void* stream)
{
    DM_LAUNCH(k_band, nu, ecc, q, n, tof, fast, libm);
}
int dm_log_pos(const double* x, int64_t n, double* r, void* stream) { DM_LAUNCH(k_log_pos, x, n, r); }
int dm_sincos_fast(const double* x, int64_t n, double* s, double* c, void* stream) { DM_LAUNCH(k_sincos_fast, x, n, s, c); }
int dm_atan2_fast(const double* y, const double* x, int64_t n, double* r, void* stream) { DM_LAUNCH(k_atan2_fast, y, x, n, r); }
int dm_exp_fast(const double* x, int64_t n, double* r, void* stream) { DM_LAUNCH(k_exp_fast, x, n, r); }
int dm_recip(const double* x, int64_t n, double* r, double* rs, void* stream) { DM_LAUNCH(k_recip, x, n, r, rs); }
}
