// ssa_kernels.hip -- gfx950 kernels + C ABI (include/ssa_hip.h) for the ssa-gym hot path.
//
// Mapping (DESIGN.md "Kernel"): one 16-lane DPP row of a wavefront owns one object:
//   lane 0      sigma_0 = x
//   lanes 1-6   x + U[k]        lanes 7-12  x - U[k]       (U = robust_cholesky((n+lambda) P), rows)
//   lane 13     the TRUE state of the same object (x_true[i-1] -> x_true[i])
//   lanes 14-15 idle
// so one wavefront advances 4 objects and every Kepler solve of the step (13 m sigma points
// + m true states) runs in its own lane.  State / covariance tiles are staged through LDS
// with block-contiguous (fully coalesced) global loads and stores; the 13-point mean is a
// DPP row reduction; the covariance outer products run from LDS.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/ssa_hip.h"
#include "ssa_math.hpp"
#include "ssa_conics.hpp"
#include "ssa_screen.hpp"

namespace ssa {

__device__ __noinline__ Vec6 kepler_general_v(Vec6 x, double tof)
{
    Vec6 o;
    kepler_general_impl(x.v, tof, o.v, nullptr);
    return o;
}
// the step kernels' own instance (inherits their register budget; spills inside it are confined to the rare call)
template <int TAG>
__device__ __noinline__ Vec6 kepler_general_tagged(Vec6 x, double tof)
{
    Vec6 o;
    kepler_general_impl(x.v, tof, o.v, nullptr);
    return o;
}
// the step kernels' own instance (inherits their register budget, see kepler_general_tagged)
template <int TAG>
__device__ __noinline__ Vec6 kepler_general_fast_tagged(Vec6 x, double tof) { return kepler_general_fast_impl<TAG>(x, tof); }
// What the series solver declined, out of line: every conic of the general orientation in the lean form, bands inline (ssa_conics.hpp);
// what THAT declines -- rv2coe's special branches, non-finite input: practically never inside a step -- goes on to the complete
// restatement from here (a nested call: the kernels see ONE call site, as they always did).
template <int TAG>
__device__ __noinline__ Vec6 kepler_beyond_series_tagged(Vec6 x, double tof)
{
    Vec6 o;
    const bool ok = kepler_conic_lean<TAG, false>(x.v, tof, o.v);
    if (__any(!ok)) {
        if (!ok) o = kepler_general_fast_tagged<TAG>(x, tof);
    }
    return o;
}
// the hybrid's lane-level choice: true = the series solver's result stands (strong-elliptic state inside its domain)
SSA_DEV bool kepler_hybrid_fast(const double* s, double tof, double* o)
{
    const double rr = dot3(s, s), vv = dot3(s + 3, s + 3), rv = dot3(s, s + 3);
    const double c1 = vv - MU * rsqrt_nr(rr);
    const double ex = c1 * s[0] - rv * s[3], ey = c1 * s[1] - rv * s[4], ez = c1 * s[2] - rv * s[5];
    const double e2 = (ex * ex + ey * ey + ez * ez) * (1.0 / (MU * MU));
    bool handled;
    const bool ok = kepler_uv_fast(s, tof, o, handled);
    return ok && (e2 < (1.0 - 1e-2) * (1.0 - 1e-2));          // (farnocchia.py:871: ecc < 1 - delta)
}

__device__ __noinline__ Vec8 kepler_general_diag_v(Vec6 x, double tof, Vec6* out)
{
    Vec8 d;
    Vec6 o;
    kepler_general_impl(x.v, tof, o.v, d.v);
    *out = o;
    return d;
}

// ------------------------------------------------------------------------------------------
// fused env step: ONE launch per step over every object.  The common path (plain Cholesky,
// strong-elliptic Kepler) and robust_cholesky's jitter ladder are inline; the other conic branches
// are out-of-line calls taken only by the lanes that need them.  The per-env UKF update runs in the
// row that owns the selected object, hidden among the other waves of the launch.
struct StepK {
    ssa_consts c;
    ssa_step_params p;
};

constexpr int OBJ_PER_WAVE = 4;
constexpr double X_FAILED_POS = 1e20, X_FAILED_VEL = 1e12;  // ssa_tasker_simple_2.py:157-158

// LDS working set of one wavefront (4 objects): 7 600 bytes -- it must stay <= 7 680: with 7 984 only 18 wavefronts fit a CU
// (the allocation granule is larger than 512 bytes) and the 20 000-object step needs a second round (+2 us, measured).
// D holds the centred propagated sigma points d_i = sigma_i' - sigma_0' (i = 1..12) of the four objects as rows of 8
// doubles [d_i[0..5], 1.0, 0.0]: the layout the matrix unit reads its operands from (below); the object blocks start at
// {0, 100, 208, 308} doubles so that the 32 lanes of one ds_read_b64 half hit 32 different 8-byte bank slots.
struct alignas(16) Tiles {
    // The first 1 984 bytes are laid out for the tile's LDS-DMA loads (tile_dma_issue): a global_load_lds_dwordx4 writes
    // LDS at (wave-uniform base) + lane x 16, so one of them with base &P[0] fills P[0..128) from all 64 lanes, and three masked
    // ones with base &P[128] put lanes 0-7 on the tail of P, lanes 32-43 on X (byte 1024 + 32 x 16 = 1536) and lanes 48-59 on T
    // (byte 1024 + 48 x 16 = 1792).  The small members live in the gaps.
    double P[OBJ_PER_WAVE * 36];       // @0     P_in, later P_out
    double Q[36];                      // @1152  process noise (read per covariance entry with a lane-dependent index)
    double Z[8];                       // @1440  six zeros: the "factor row" of the lanes that add nothing (sigma_0, truth, idle)
    int St[OBJ_PER_WAVE];              // @1504
    int Oid[OBJ_PER_WAVE];             // @1520  the caller's index of each row's object (ssa_step_params.obj_ids; else unused)
    double X[OBJ_PER_WAVE * 6];        // @1536  x_in, then sigma_0', then x_out
    double pad1[8];                    // @1728  [0..4): the update's row of the Sun table (ssa_sensor_params.sun), for the sensors that need it
    double T[OBJ_PER_WAVE * 6];        // @1792  x_true_in, later x_true_out
    double UA[OBJ_PER_WAVE * 36];      // Cholesky factor rows [4][36] (the transform's moment sums stay in registers)
    double D[408];                     // centred propagated sigma points (see above); scratch of the update
    double M[OBJ_PER_WAVE * 12];       // s = Wi sum d_i | m' = mean - sigma_0'
    double Obs[OBJ_PER_WAVE * 12];     // until the update has run: its prefetched inputs (GCRS->ITRS matrix [9] | measurement noise [3]) per object
    double Met[OBJ_PER_WAVE * 4];
};
static_assert(offsetof(Tiles, P) == 0 && offsetof(Tiles, X) == 1536 && offsetof(Tiles, T) == 1792, "LDS-DMA image of the tile (tile_dma_issue)");
SSA_DEV int dbase(int g) { return g * 96 + (g & 1) * 4 + (g >> 1) * 16; }   // 0, 100, 208, 308
static_assert(sizeof(Tiles) <= 7680, "Tiles must fit 20 wavefronts per CU (see above)");

// Wave-contiguous tile I/O: the 4 objects of a wavefront are consecutive, so P / x / x_true / obs are
// single contiguous spans (1152 / 192 / 192 / 384 B) moved as 16-byte lanes -- whole cache lines per
// instruction instead of four 288-byte pieces.  `cnt` = valid objects in the tile (1..4).
// The tile's inputs travel global -> registers -> LDS in two halves, so that a wavefront that advances
// several tiles can have the NEXT tile's loads in flight while it works on the current one:
//   tile_issue : 16-byte wave-contiguous loads into 8 VGPRs.  `main` = P entries [2 lane, 2 lane + 2);
//                `aux` by lane: 0-7 the tail of P | 32-43 x_filter | 48-59 x_true | 60-63 status (bits)
//   tile_commit: registers -> LDS tiles (rows beyond `cnt` are zero / marked failed)
struct TileRegs { double2 main, aux; int st; bool dma; };   // (the status word travels in its own register: packing it into `aux` put a wait for
                                                 // EVERY outstanding load right behind the tile's loads)
// one 16-byte lane of a tile load (plain: marking the inputs streaming was measured slower, 45.4 k vs 46.5 k)
SSA_DEV double2 load16(const double* src) { return *reinterpret_cast<const double2*>(src); }
SSA_DEV void tile_issue_from(TileRegs& r, const double* P_in, const double* x_in, const double* x_true_in, const int32_t* status,
                            int lane, int64_t base, int cnt)
{
    const double2 zero = make_double2(0.0, 0.0);
    r.main = zero;
    r.aux = zero;
    r.st = SSA_ST_PREDICT_NAN;
    r.dma = false;
    if (cnt <= 0) return;
    const double* Pin = P_in + base * 36;
    if (lane < cnt * 18) r.main = load16(Pin + 2 * lane);
    // the rest of the tile -- lanes [0, 8): the tail of P, [32, 44): x, [48, 60): x_true -- is ONE 16-byte load per lane whose
    // source is selected by lane range (a tree of nested lane-range branches cost 80 scalar instructions and their branch
    // latencies in front of the loads); a ragged tile (cnt < 4) shortens every range through `lim`
    const bool sX = lane >= 32, sT = lane >= 48;
    const int i = lane - (sT ? 48 : sX ? 32 : 0);
    const int lim = sX ? cnt * 3 : cnt * 18 - 64;
    const double* src = sT ? x_true_in + base * 6 : sX ? x_in + base * 6 : Pin + 128;
    if (i < lim) r.aux = load16(src + 2 * i);
    if (lane >= 60 && lane - 60 < cnt) r.st = status[base + (lane - 60)];
}
SSA_DEV void tile_issue(TileRegs& r, const ssa_step_params& p, int lane, int64_t base, int cnt)
{
    tile_issue_from(r, p.P_in, p.x_in, p.x_true_in, p.status, lane, base, cnt);
}
SSA_DEV void tile_commit(Tiles& t, const TileRegs& r, int lane)
{
    reinterpret_cast<double2*>(t.P)[lane] = r.main;
    const bool sX = lane >= 32, sT = lane >= 48;
    const int i = lane - (sT ? 48 : sX ? 32 : 0);
    double* dst = sT ? t.T : sX ? t.X : t.P + 128;
    if (i < (sX ? 12 : 8)) reinterpret_cast<double2*>(dst)[i] = r.aux;
    if (lane >= 60) t.St[lane - 60] = r.st;
}
// The one-tile kernels' load: the tile travels global -> LDS directly (LDS-DMA, no VGPR staging, no ds_write pass, the source
// addresses in scalar-base + lane-offset form: four instructions and a handful of scalar ones where the register path spends
// ~80 vector instructions on lane-range selects, 64-bit address arithmetic and the commit).  A ragged last tile (cnt < 4) takes
// the register path, which zero-fills what it does not load.  Completion: s_waitcnt vmcnt(0) (tile_dma_wait) -- the compiler
// does not know these loads write LDS.
// the objects of a launch (a sensor network: one env)
SSA_DEV int64_t tile_total(const ssa_step_params& p, bool one_env) { return one_env ? p.n_obj : (int64_t)p.n_env * p.n_obj; }
typedef const __attribute__((address_space(1))) void* GlobalVoidPtr;
typedef __attribute__((address_space(3))) void* LdsVoidPtr;
SSA_DEV void glds16(const double* src, double* lds_base)
{
    __builtin_amdgcn_global_load_lds((GlobalVoidPtr)src, (LdsVoidPtr)lds_base, 16, 0, 0);
}
// `whole` comes from the kernel's preloaded arguments alone, so the DMA loads leave before any scalar load has returned; the object total --
// a scalar load from the argument segment -- is read by the ragged tile only.
SSA_DEV void tile_dma_issue(Tiles& t, TileRegs& r, const double* P_in, const double* x_in, const double* x_true_in, const int32_t* status,
                            int lane, int64_t base, bool whole, const ssa_step_params& p, bool one_env)
{
    r.dma = whole;
    if (!whole) {
        tile_issue_from(r, P_in, x_in, x_true_in, status, lane, base, (int)(tile_total(p, one_env) - base));
        return;
    }
    r.st = SSA_ST_PREDICT_NAN;
    const double* Pin = P_in + base * 36;
    glds16(Pin + 2 * lane, t.P);                                                           // P[0 .. 128)
    if (lane < 8) glds16(Pin + 128 + 2 * lane, t.P + 128);                                 // P[128 .. 144)
    if (lane >= 32 && lane < 44) glds16(x_in + base * 6 - 64 + 2 * lane, t.P + 128);       // -> X: entries 2 (lane - 32) ..
    if (lane >= 48 && lane < 60) glds16(x_true_in + base * 6 - 96 + 2 * lane, t.P + 128);  // -> T: entries 2 (lane - 48) ..
    if (lane >= 60) r.st = status[base + (lane - 60)];
}
SSA_DEV void tile_dma_wait(Tiles& t, const TileRegs& r, int lane)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane >= 60) t.St[lane - 60] = r.st;
}
typedef double v2d __attribute__((ext_vector_type(2)));
// one 16-byte lane of a tile store.  NT (non-temporal): for launches of up to 20 480 objects and for rollouts the
// outputs are marked streaming, which leaves less dirty data for the end-of-kernel L2 write-back (-0.55 us per launch
// at 20 000 objects).  Not for the multi-tile step kernel: at 160 000 objects the next step re-reads 61 MB of these
// outputs from the Infinity Cache, and streaming them past it cost 19 %.
template <bool NT>
SSA_DEV void store16(double* dst, const double* src)
{
    if (NT) __builtin_nontemporal_store(*reinterpret_cast<const v2d*>(src), reinterpret_cast<v2d*>(dst));
    else *reinterpret_cast<v2d*>(dst) = *reinterpret_cast<const v2d*>(src);
}
// first row of the env a tile belongs to (a storage layout with several envs: whole tiles per env, so the tile has ONE env)
SSA_DEV int64_t env_row0(const ssa_step_params& p, int64_t base)
{
    return p.n_env > 1 ? (int64_t)((uint32_t)base / (uint32_t)p.n_obj) * p.n_obj : 0;
}
// PLAIN (step_plain_kernel, see ActPlain): one env and no obs_mirror, known when the kernel was compiled -- and the ragged last tile only:
// the plain form's whole tile has a store stage of its own (plain_tile_out)
template <bool NT, bool PLAIN = false>
SSA_DEV void store_tile(const Tiles& t, const ssa_step_params& p, int lane, int64_t base, int cnt)
{
#define SSA_SKIP(b) 0   // (no store is skipped; without the ragged tile's `skip` below the multi-tile step kernel allocates its registers differently)
    if (!PLAIN && cnt == OBJ_PER_WAVE) {
        // A whole tile (wave-uniform; every tile of a launch but a ragged last one).  Every group of lanes stores from
        // (uniform pointer) + lane x 16 bytes on both sides -- the global address in scalar-base + lane-offset form, the LDS address
        // one shared register plus an immediate -- instead of selecting 64-bit destination and source pointers per lane range
        // (that was 58 vector + 60 scalar instructions per wavefront).  The observation rows [x, diag P] (results.py:61) are read
        // from the state / covariance tiles by the lanes that store them: no staging copy.
        if (!SSA_SKIP(1)) {
            store16<NT>(p.P_out + base * 36 + 2 * lane, t.P + 2 * lane);
            if (lane < 8) store16<NT>(p.P_out + base * 36 + 128 + 2 * lane, t.P + 128 + 2 * lane);
        }
        if (!SSA_SKIP(4)) {
            if ((unsigned)(lane - 8) < 12u) store16<NT>(p.x_out + base * 6 - 16 + 2 * lane, t.X - 16 + 2 * lane);
            if ((unsigned)(lane - 20) < 12u) store16<NT>(p.x_true_out + base * 6 - 40 + 2 * lane, t.T - 40 + 2 * lane);
        }
        if (!SSA_SKIP(2) && lane >= 32 && lane < 56) {   // obs: 24 lanes x 16 bytes; lane i = entries [2 i, 2 i + 2) of the tile's 48
            const int i = lane - 32;
            const int jj = (i * 43) >> 8;                // i / 6: the object
            const int r = 2 * i - 12 * jj;               // 0, 2, 4: x | 6, 8, 10: diag P
            double* dst = p.obs + base * 12 - 64 + 2 * lane;
            v2d pair;
            if (r < 6) pair = *reinterpret_cast<const v2d*>(t.X + jj * 6 + r);
            else {
                const double* d = t.P + jj * 36 + 7 * (r - 6);
                pair = v2d{d[0], d[7]};
            }
            if (NT) __builtin_nontemporal_store(pair, reinterpret_cast<v2d*>(dst));
            else *reinterpret_cast<v2d*>(dst) = pair;
            if (p.obs_mirror) {   // (e.g. host-mapped memory; with obj_ids: row by row at the caller's index of the object)
                // (in observation entries; several envs: the table holds indices within the env, whose rows start at env_row0)
                const int64_t at = p.obj_ids ? (env_row0(p, base) + t.Oid[jj]) * 12 + r : base * 12 - 64 + 2 * lane;
                if (p.launch_mask & SSA_LAUNCH_MIRROR_F32)      // the host-facing copy in single precision: half the bytes over PCIe
                    *reinterpret_cast<float2*>(reinterpret_cast<float*>(p.obs_mirror) + at) = make_float2((float)pair.x, (float)pair.y);
                else *reinterpret_cast<v2d*>(p.obs_mirror + at) = pair;
            }
        }
        if (!SSA_SKIP(16) && lane >= 56 && lane < 60) p.status[base - 56 + lane] = t.St[lane - 56];
        if (!SSA_SKIP(8) && lane < 16) {   // metrics [E][4][m]: four 32-byte runs per tile
            const int kk = lane >> 2, jj = lane & 3;
            const int64_t obj = base + jj;
            if (p.n_env == 1) {   // (scalar row stride, one 64-bit multiply-add per lane)
                p.metrics[(int64_t)kk * p.n_obj + obj] = t.Met[jj * 4 + kk];
            } else {
                const int64_t e = (int64_t)((uint32_t)obj / (uint32_t)p.n_obj), j = obj - e * p.n_obj;
                p.metrics[(e * 4 + kk) * p.n_obj + j] = t.Met[jj * 4 + kk];
            }
        }
        return;
    }
    // ragged last tile: the general form (the observation rows were staged in t.Obs by observe_rows)
    if (!SSA_SKIP(1) && lane < cnt * 18) store16<NT>(p.P_out + base * 36 + 2 * lane, t.P + 2 * lane);
    {   // lanes [0, 12): x | [16, 28): x_true | [32, 40): the tail of P | [40, 64): obs -- one 16-byte store per lane, destination and
        // LDS source selected by lane range (see tile_issue_from)
        const bool sT = lane >= 16, sP = lane >= 32, sO = lane >= 40;
        const int i = lane - (sO ? 40 : sP ? 32 : sT ? 16 : 0);
        const int lim = sO ? cnt * 6 : sP ? cnt * 18 - 64 : cnt * 3;
        double* dst = sO ? p.obs + base * 12 : sP ? p.P_out + base * 36 + 128 : sT ? p.x_true_out + base * 6 : p.x_out + base * 6;
        const double* src = sO ? t.Obs : sP ? t.P + 128 : sT ? t.T : t.X;
        const bool skip = sO ? SSA_SKIP(2) : sP ? SSA_SKIP(1) : SSA_SKIP(4);
        if (!skip && i < lim) store16<NT>(dst + 2 * i, src + 2 * i);
        if (!PLAIN && sO && p.obs_mirror && i < lim) {
            const int jj = (i * 43) >> 8;     // i / 6: the object (rows beyond cnt are masked by `lim`)
            const int64_t at = p.obj_ids ? (env_row0(p, base) + t.Oid[jj]) * 12 + (2 * i - 12 * jj) : base * 12 + 2 * i;
            if (p.launch_mask & SSA_LAUNCH_MIRROR_F32)
                *reinterpret_cast<float2*>(reinterpret_cast<float*>(p.obs_mirror) + at) = make_float2((float)src[2 * i], (float)src[2 * i + 1]);
            else store16<false>(p.obs_mirror + at, src + 2 * i);
        }
    }
    if (!SSA_SKIP(16) && lane >= 12 && lane < 16) {
        const int i = lane - 12;
        if (i < cnt) p.status[base + i] = t.St[i];
    }
    if (!SSA_SKIP(8) && lane < 16) {   // metrics [E][4][m]: four 32-byte runs per tile
        const int kk = lane >> 2, jj = lane & 3;
        if (jj < cnt) {
            const int64_t obj = base + jj;
            if (PLAIN || p.n_env == 1) {   // (scalar row stride, one 64-bit multiply-add per lane)
                p.metrics[(int64_t)kk * p.n_obj + obj] = t.Met[jj * 4 + kk];
            } else {
                const int64_t e = (int64_t)((uint32_t)obj / (uint32_t)p.n_obj), j = obj - e * p.n_obj;
                p.metrics[(e * 4 + kk) * p.n_obj + j] = t.Met[jj * 4 + kk];
            }
        }
    }
}

// O1/O2 for the row's object from the tiles (results.py:61, :37)
// metric l (< 4) of row g's object: |x - x_true| over the position / the velocity block, then sigma_pos, sigma_vel.  Written once:
// observe_rows stages it in t.Met, the plain whole-tile store stage (plain_tile_out) stores it from the register -- the same
// expressions in the same order (under -ffp-contract=fast a reworded sum may contract differently)
SSA_DEV double metric_value(const Tiles& t, int g, int l)
{
    const int off = (l & 1) * 3;  // 0: position block, 1: velocity block
    double v;
    if (l < 2) {
        double a0 = t.X[g * 6 + off] - t.T[g * 6 + off];
        double a1 = t.X[g * 6 + off + 1] - t.T[g * 6 + off + 1];
        double a2 = t.X[g * 6 + off + 2] - t.T[g * 6 + off + 2];
        v = sqrt_fast(a0 * a0 + a1 * a1 + a2 * a2);
    } else {   // (a negative sum -- indefinite covariance -- gives NaN, as numpy's sqrt)
        v = sqrt_fast(t.P[g * 36 + 7 * off] + t.P[g * 36 + 7 * (off + 1)] + t.P[g * 36 + 7 * (off + 2)]);
    }
    return v;
}
SSA_DEV void observe_rows(Tiles& t, int g, int l, bool stage_obs)
{
    // (a whole tile's observation rows leave straight from the state / covariance tiles: store_tile)
    if (stage_obs && l < 12) t.Obs[g * 12 + l] = (l < 6) ? t.X[g * 6 + l] : t.P[g * 36 + 7 * (l - 6)];
    if (l < 4) t.Met[g * 4 + l] = metric_value(t, g, l);
}

// U3 on the matrix unit.  With D^(g) the 12 x 8 matrix of object g's rows [d_i, 1, 0], the transform needs
//   A^(g) = D^T D :  A[a][b] = sum_i d_i[a] d_i[b]  (a, b < 6)   and   A[a][6] = sum_i d_i[a]
// -- 21 row reductions over the 16 lanes plus 6 more for the mean if done with DPP butterflies.  v_mfma_f64_4x4x4_4b_f64
// multiplies four independent 4x4x4 blocks per instruction; its block index is lane bits 3:2, its k (operands) / i
// (result) index lane bits 5:4, its i / j index lane bits 1:0 (measured: profiles/r02_mfma_probe.txt): block b = object b, three
// k-chunks of four sigma points, 4x4 tiles (0,0), (0,1), (1,1) of the symmetric 8x8 result = 9 instructions of 16 cycles
// on the otherwise idle matrix pipe, operands by six conflict-free ds_read_b64.  Lane (hi, mid, lo) ends up with
// A^(mid)[hi][lo], A^(mid)[hi][4 + lo], A^(mid)[4 + hi][4 + lo] and KEEPS them in registers: covariance_finish() below turns
// them into the entries of P in the same lanes.  Only the column of sums A[a][6] goes to LDS (t.M[mid][a]: the mean needs it).
struct Moments { double c00, c01, c11; };
template <bool SUMS_ONLY = false>   // SUMS_ONLY: the column of sums alone (SSA_FLAG_REFERENCE_COV forms its own second moments): block (0,0) is skipped
SSA_DEV Moments moment_sums_mfma(Tiles& t, int lane)
{
    const int hi = lane >> 4, mid = (lane >> 2) & 3, lo = lane & 3;
    const double* src = &t.D[dbase(mid) + hi * 8 + lo];
    double a0[3], a1[3];
#pragma unroll
    for (int kc = 0; kc < 3; ++kc) {
        a0[kc] = src[kc * 32];
        a1[kc] = src[kc * 32 + 4];
    }
    Moments mo = {0.0, 0.0, 0.0};
#pragma unroll
    for (int kc = 0; kc < 3; ++kc) {
        if (!SUMS_ONLY) mo.c00 = __builtin_amdgcn_mfma_f64_4x4x4f64(a0[kc], a0[kc], mo.c00, 0, 0, 0);
        mo.c01 = __builtin_amdgcn_mfma_f64_4x4x4f64(a0[kc], a1[kc], mo.c01, 0, 0, 0);
        mo.c11 = __builtin_amdgcn_mfma_f64_4x4x4f64(a1[kc], a1[kc], mo.c11, 0, 0, 0);
    }
    if (lo == 2) {                                   // column 6 of the blocks (0,1) and (1,1): the sums over the sigma points
        t.M[mid * 12 + hi] = mo.c01;
        if (hi < 2) t.M[mid * 12 + 4 + hi] = mo.c11;
    }
    return mo;
}

// U3 (second half): P = sum Wc_i y_i y_i^T + Q with y_i = sigma_i' - x, expanded around sigma_0':
//   P = Wi A - m' s^T - s m'^T + sum(Wc) m' m'^T + Q       (A in the registers moment_sums_mfma left; s, m' in t.M)
// in the matrix unit's result layout: lane (hi, mid, lo) finishes object mid's entries (hi, lo), (hi, 4 + lo), (4 + hi, 4 + lo)
// -- all 64 lanes, no index arithmetic beyond the lane's bit fields, no second LDS copy of A (the earlier version ran the
// 21 upper-triangle entries over the object's 16 lanes in two passes, half of its instructions index arithmetic).  A is
// bit-symmetric (same products, same order) but the expression below is not under a <-> b, so only lanes with a <= b
// write, to both [a][b] and [b][a]: P leaves exactly symmetric.
SSA_DEV double covariance_entry(const ssa_consts& C, double acc, double sa_, double ma, double sb_, double mb, double q)
{
    return C.Wi * acc - ma * sb_ - sa_ * mb + C.sum_wc * ma * mb + q;
}
SSA_DEV void covariance_finish(Tiles& t, const ssa_consts& C, int lane, const Moments& mo)
{
    const int hi = lane >> 4, mid = (lane >> 2) & 3, lo = lane & 3;
    const int hi1 = hi & 1, lo1 = lo & 1;            // (rows / columns 4, 5: the lanes beyond them compute on valid addresses and do not write)
    const double* M = &t.M[mid * 12];
    double* P = &t.P[mid * 36];
    const double s_a = M[hi], m_a = M[6 + hi], s_b = M[lo], m_b = M[6 + lo];
    const double s_a4 = M[4 + hi1], m_a4 = M[10 + hi1], s_b4 = M[4 + lo1], m_b4 = M[10 + lo1];
    const double p00 = covariance_entry(C, mo.c00, s_a, m_a, s_b, m_b, t.Q[hi * 6 + lo]);
    const double p01 = covariance_entry(C, mo.c01, s_a, m_a, s_b4, m_b4, t.Q[hi * 6 + 4 + lo1]);
    const double p11 = covariance_entry(C, mo.c11, s_a4, m_a4, s_b4, m_b4, t.Q[(4 + hi1) * 6 + 4 + lo1]);
    if (hi <= lo) {
        P[hi * 6 + lo] = p00;
        P[lo * 6 + hi] = p00;
    }
    if (lo < 2) {
        P[hi * 6 + 4 + lo] = p01;
        P[(4 + lo) * 6 + hi] = p01;
        if (hi <= lo) {                              // (hi, lo) in {(0,0), (0,1), (1,1)}
            P[(4 + hi) * 6 + 4 + lo] = p11;
            P[(4 + lo) * 6 + 4 + hi] = p11;
        }
    }
}

// O3 accumulator.  NaN ranks above everything (np.max / np.argmax semantics), ties keep the lowest index.
struct StatAcc {
    double mx, sm;       // max delta_pos (NaN excluded), max sigma_pos (valid when !sm_nan)
    long long arg;       // index of sm (or of the first NaN sigma_pos)
    unsigned c4, c7, nf;
    int mx_nan, sm_nan;
};
SSA_DEV void stat_merge(StatAcc& a, const StatAcc& b)
{
    a.mx = fmax(a.mx, b.mx);
    a.mx_nan |= b.mx_nan;
    a.c4 += b.c4; a.c7 += b.c7; a.nf += b.nf;
    bool take_b;
    if (a.sm_nan || b.sm_nan) take_b = b.sm_nan && (!a.sm_nan || b.arg < a.arg);
    else take_b = (b.sm > a.sm) || (b.sm == a.sm && b.arg < a.arg);
    if (take_b) { a.sm = b.sm; a.arg = b.arg; a.sm_nan = b.sm_nan; }
}
SSA_DEV StatAcc stat_shfl_down(const StatAcc& a, int off)
{
    StatAcc b;
    b.mx = __shfl_down(a.mx, off, 64);
    b.sm = __shfl_down(a.sm, off, 64);
    b.arg = __shfl_down(a.arg, off, 64);
    b.c4 = __shfl_down(a.c4, off, 64);
    b.c7 = __shfl_down(a.c7, off, 64);
    b.nf = __shfl_down(a.nf, off, 64);
    b.mx_nan = __shfl_down(a.mx_nan, off, 64);
    b.sm_nan = __shfl_down(a.sm_nan, off, 64);
    return b;
}
SSA_DEV StatAcc stat_identity()
{
    StatAcc a;
    a.mx = -1.0; a.sm = -1.0; a.arg = 0x7fffffffffffffffLL; a.c4 = a.c7 = a.nf = 0; a.mx_nan = a.sm_nan = 0;
    return a;
}
SSA_DEV StatAcc stat_wave_reduce(StatAcc a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        StatAcc b = stat_shfl_down(a, off);
        stat_merge(a, b);
    }
    return a;
}

// ------------------------------------------------------------------------------------------
// Intra-wave LDS hand-off.  The step kernel's workgroup IS one wavefront, all lanes run in
// lockstep and the LDS queue is in order, so "every lane's earlier LDS writes are visible to every
// lane's later LDS reads" only needs the compiler not to move accesses across this point and the
// outstanding DS operations to have completed.  (Usable inside row-divergent branches, unlike a
// workgroup barrier.)
SSA_DEV void wave_lds_sync()
{
    // wavefront-scope fence: no instruction on gfx9 (the DS unit executes one wavefront's operations in
    // issue order, so a lane's read issued after another lane's write observes it); it only pins the
    // compiler's ordering of the LDS accesses around this point
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// U3, covariance in the REFERENCE's own arithmetic (SSA_FLAG_REFERENCE_COV): filterpy's unscented_transform evaluates
//   P = sum_i (sigma_i' - x) (Wc_i (sigma_i' - x))^T + Q,      i = 0 .. 12,  Wc_0 ~ -2e8 at alpha = 1e-4
// -- a sum of thirteen outer products whose first term cancels the other twelve.  For a filter whose prior has diverged
// (|sigma_0' - x| ~ 1e9 m late in a predict-only episode) that cancellation leaves rounding noise of 1e10 m^2 in P: the
// covariance turns indefinite, robust_cholesky (dynamics.py:402-417) exhausts its ladder at the next predict and the
// reference marks the filter FAILED (ssa_tasker_simple_2.py:271-285, 369-382): 2-3 % of the filters of a 480-step
// episode.  covariance_finish() above evaluates the same matrix expanded around sigma_0' without that cancellation and
// such filters survive; this form reproduces the reference's failure behaviour (tests/test_episode_failures.py).
// The thirteen rows y_i = sigma_i' - x go to LDS (factor tile + D, contiguous and free by now), the matrix unit forms the
// three 4x4 tiles of sum_i y_i (Wc_i y_i)^T, i = 0 .. 11, in three k-chunks and three vector fmas add point 12; the weight enters
// with the right operand, as in the reference.  (What the form costs -- every wavefront of a SIMD runs this stage at the same time, so
// its instructions add up: a vector instruction ~8 ns of a 20 000-object step, a 4x4x4 matrix instruction ~33 ns; 13.0 us per healthy
// step against 11.9 with covariance_finish.)
SSA_DEV int ybase(int g) { return g * 104 + (g & 1) * 28 + (g >> 1) * 32; }   // 0, 132, 240, 372: bank slots as dbase()
// (xb_l: lanes 0 .. 5 of a row hold component l of the row's prior mean -- the value they have just written to t.X.  The other lanes take
// it from there by DPP row broadcasts: the detour through t.X was three dependent LDS round trips in front of the y rows' own)
SSA_DEV void covariance_reference(Tiles& t, const ssa_consts& C, int lane, const double (&o)[6], double xb_l)
{
    static_assert(372 + 16 * 8 <= OBJ_PER_WAVE * 36 + 408, "y rows fit the factor tile + D");
    typedef double v2d_t __attribute__((ext_vector_type(2)));
    double* const Y = t.UA;
    {
        const int g = lane >> 4, l = lane & 15;
        const double x0 = row_bcast<0>(xb_l), x1 = row_bcast<1>(xb_l), x2 = row_bcast<2>(xb_l), x3 = row_bcast<3>(xb_l),
                     x4 = row_bcast<4>(xb_l), x5 = row_bcast<5>(xb_l);
        if (l <= 12) {
            v2d_t* dst = reinterpret_cast<v2d_t*>(&Y[ybase(g) + l * 8]);
            dst[0] = v2d_t{o[0] - x0, o[1] - x1};
            dst[1] = v2d_t{o[2] - x2, o[3] - x3};
            dst[2] = v2d_t{o[4] - x4, o[5] - x5};
            dst[3] = v2d_t{0.0, 0.0};
        }
    }
    wave_lds_sync();
    const int hi = lane >> 4, mid = (lane >> 2) & 3, lo = lane & 3;
    const double* src = &Y[ybase(mid) + hi * 8 + lo];
    Moments mo = {0.0, 0.0, 0.0};
    constexpr int NKC = 3;
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
        double a0 = src[kc * 32], a1 = src[kc * 32 + 4];
        if (kc == 3 && hi != 0) { a0 = 0.0; a1 = 0.0; }           // rows 13 .. 15 do not exist
        const double w = (kc == 0 && hi == 0) ? C.Wc0 : C.Wi;
        const double b0 = w * a0, b1 = w * a1;
        mo.c00 = __builtin_amdgcn_mfma_f64_4x4x4f64(a0, b0, mo.c00, 0, 0, 0);
        mo.c01 = __builtin_amdgcn_mfma_f64_4x4x4f64(a0, b1, mo.c01, 0, 0, 0);
        mo.c11 = __builtin_amdgcn_mfma_f64_4x4x4f64(a1, b1, mo.c11, 0, 0, 0);
    }
    {   // point 12, the last term of the sum, by three vector fmas: the fourth k-chunk held it alone (three matrix instructions that
        // multiplied three rows of zeros) -- entry (i, j) += y12[i] (Wi y12[j]), the product rounded as the matrix unit's operand was;
        // whole 20 000-object episodes bit-identical to the four-chunk form, 0.2 us per step less with
        // the broadcasts above
        const double* y12 = &Y[ybase(mid) + 12 * 8];
        const double ai = y12[hi], ai4 = y12[4 + hi], bj = C.Wi * y12[lo], bj4 = C.Wi * y12[4 + lo];
        mo.c00 = fma(ai, bj, mo.c00);
        mo.c01 = fma(ai, bj4, mo.c01);
        mo.c11 = fma(ai4, bj4, mo.c11);
    }
    const int hi1 = hi & 1, lo1 = lo & 1;
    double* P = &t.P[mid * 36];
    const double p00 = mo.c00 + t.Q[hi * 6 + lo];
    const double p01 = mo.c01 + t.Q[hi * 6 + 4 + lo1];
    const double p11 = mo.c11 + t.Q[(4 + hi1) * 6 + 4 + lo1];
    // scipy's cholesky reads the upper triangle only; the entries a <= b are mirrored (as covariance_finish)
    if (hi <= lo) {
        P[hi * 6 + lo] = p00;
        P[lo * 6 + hi] = p00;
    }
    if (lo < 2) {
        P[hi * 6 + 4 + lo] = p01;
        P[(4 + lo) * 6 + hi] = p01;
        if (hi <= lo) {
            P[(4 + hi) * 6 + 4 + lo] = p11;
            P[(4 + lo) * 6 + 4 + hi] = p11;
        }
    }
}

// U3 with SSA_FLAG_REFERENCE_COV in the plain family (step_plain_kernel): ONE tile feeds both matrix passes.  The two tiles above -- the rows
// [sigma_i' - sigma_0', 1, 0] of t.D and the rows [sigma_i' - x, 0, 0] of Y -- are the same thirteen propagated points minus a vector every
// lane can fetch, each written once (behind six row broadcasts, and Y behind a fence of its own) and read once.  Here lanes 0 .. 12 of a row
// write their point as it left the propagator, rows of 8 doubles [sigma_i'[0..5], -, -] in the factor tile + D (contiguous and free by
// then), and each pass subtracts in the matrix unit's operand layout: the same IEEE subtraction on the same operands as the row layout's,
// so the same bits -- d_i = sigma_i' - sigma_0' with one rounding, y_i = sigma_i' - x with one rounding (forming y_i from d_i would take two,
// and fail other filters than the reference does).  The two pad words of a row are never written and no lane reads one as a value that is
// used: the lanes lo >= 2 read them as components "6, 7", which reach rows / columns >= 6 of the 8 x 8 result only -- a NaN there touches
// nothing that is stored.
SSA_DEV int sbase(int g) { return g * 104 + (g & 1) * 28 + (g >> 1) * 32; }   // 0, 132, 240, 372: bank slots as dbase() / ybase()
static_assert(372 + 13 * 8 <= OBJ_PER_WAVE * 36 + 408, "the rows of sigma points fit the factor tile + D");
SSA_DEV void sigma_rows_write(Tiles& t, int g, int l, const double (&o)[6])
{
    typedef double v2d_t __attribute__((ext_vector_type(2)));
    if (l <= 12) {
        v2d_t* dst = reinterpret_cast<v2d_t*>(&t.UA[sbase(g) + l * 8]);
        dst[0] = v2d_t{o[0], o[1]};
        dst[1] = v2d_t{o[2], o[3]};
        dst[2] = v2d_t{o[4], o[5]};
    }
    if (l == 0 || l == 13) {   // sigma_0' (until the mean replaces it) | x_true[i]
        v2d_t* dst = reinterpret_cast<v2d_t*>(l == 0 ? &t.X[g * 6] : &t.T[g * 6]);
        dst[0] = v2d_t{o[0], o[1]};
        dst[1] = v2d_t{o[2], o[3]};
        dst[2] = v2d_t{o[4], o[5]};
    }
}
// the first pass, moment_sums_mfma<true> from the rows above: t.M[mid][a] = sum_{i = 1 .. 12} (sigma_i'[a] - sigma_0'[a]).  The column of
// ones is a register constant of the right operand (1.0 in the lanes lo == 2): the products d x 1.0 and the zeros added to them are exact,
// and the sums leave column 2 of both blocks as they left column 6 of the 8 x 8 result.
SSA_DEV void moment_sums_rows(Tiles& t, int lane)
{
    const int hi = lane >> 4, mid = (lane >> 2) & 3, lo = lane & 3;
    const double* src = &t.UA[sbase(mid) + hi * 8 + lo];
    const double* s0 = &t.UA[sbase(mid) + lo];       // sigma_0'
    const double z0 = s0[0], z1 = s0[4];
    double a0[3], a1[3];
#pragma unroll
    for (int kc = 0; kc < 3; ++kc) {                 // rows 4 kc + hi + 1
        a0[kc] = src[8 + kc * 32];
        a1[kc] = src[8 + kc * 32 + 4];
    }
    const double one = (lo == 2) ? 1.0 : 0.0;
    double c01 = 0.0, c11 = 0.0;
#pragma unroll
    for (int kc = 0; kc < 3; ++kc) {
        const double d0 = a0[kc] - z0, d1 = a1[kc] - z1;
        c01 = __builtin_amdgcn_mfma_f64_4x4x4f64(d0, one, c01, 0, 0, 0);
        c11 = __builtin_amdgcn_mfma_f64_4x4x4f64(d1, one, c11, 0, 0, 0);
    }
    if (lo == 2) {
        t.M[mid * 12 + hi] = c01;
        if (hi < 2) t.M[mid * 12 + 4 + hi] = c11;
    }
}
// the second pass, covariance_reference from the same rows: behind the mean (t.X holds x), y = sigma_i' - x formed in the operand layout, rows
// 4 kc + hi; the weights on the right operand, the three k-chunks and the three vector fmas of point 12 as they are above -- the accumulation
// order i = 0 .. 12 is unchanged.  No row broadcasts, no second tile and no fence of its own: the rows are as old as the first pass, the mean sits behind the caller's.
SSA_DEV void covariance_reference_rows(Tiles& t, const ssa_consts& C, int lane)
{
    const int hi = lane >> 4, mid = (lane >> 2) & 3, lo = lane & 3;
    const double* src = &t.UA[sbase(mid) + hi * 8 + lo];
    const double* r12 = &t.UA[sbase(mid) + 12 * 8];
    const double* xb = &t.X[mid * 6];                // (components "6, 7" of the lanes lo / hi >= 2: the next object's words or pad1, unused)
    // every read of the tile and of the mean, then one wait
    double a0[3], a1[3];
#pragma unroll
    for (int kc = 0; kc < 3; ++kc) {
        a0[kc] = src[kc * 32];
        a1[kc] = src[kc * 32 + 4];
    }
    const double x_lo = xb[lo], x_lo4 = xb[4 + lo], x_hi = xb[hi], x_hi4 = xb[4 + hi];
    const double s_lo = r12[lo], s_lo4 = r12[4 + lo], s_hi = r12[hi], s_hi4 = r12[4 + hi];
    Moments mo = {0.0, 0.0, 0.0};
#pragma unroll
    for (int kc = 0; kc < 3; ++kc) {
        const double y0 = a0[kc] - x_lo, y1 = a1[kc] - x_lo4;
        const double w = (kc == 0 && hi == 0) ? C.Wc0 : C.Wi;
        const double b0 = w * y0, b1 = w * y1;
        mo.c00 = __builtin_amdgcn_mfma_f64_4x4x4f64(y0, b0, mo.c00, 0, 0, 0);
        mo.c01 = __builtin_amdgcn_mfma_f64_4x4x4f64(y0, b1, mo.c01, 0, 0, 0);
        mo.c11 = __builtin_amdgcn_mfma_f64_4x4x4f64(y1, b1, mo.c11, 0, 0, 0);
    }
    {   // point 12 (see covariance_reference)
        const double ai = s_hi - x_hi, ai4 = s_hi4 - x_hi4, bj = C.Wi * (s_lo - x_lo), bj4 = C.Wi * (s_lo4 - x_lo4);
        mo.c00 = fma(ai, bj, mo.c00);
        mo.c01 = fma(ai, bj4, mo.c01);
        mo.c11 = fma(ai4, bj4, mo.c11);
    }
    const int hi1 = hi & 1, lo1 = lo & 1;
    double* P = &t.P[mid * 36];
    const double p00 = mo.c00 + t.Q[hi * 6 + lo];
    const double p01 = mo.c01 + t.Q[hi * 6 + 4 + lo1];
    const double p11 = mo.c11 + t.Q[(4 + hi1) * 6 + 4 + lo1];
    if (hi <= lo) {
        P[hi * 6 + lo] = p00;
        P[lo * 6 + hi] = p00;
    }
    if (lo < 2) {
        P[hi * 6 + 4 + lo] = p01;
        P[(4 + lo) * 6 + hi] = p01;
        if (hi <= lo) {
            P[(4 + hi) * 6 + 4 + lo] = p11;
            P[(4 + lo) * 6 + 4 + hi] = p11;
        }
    }
}

// U2 (common case): upper Cholesky of scale*P for the row's object, lane-distributed: lane c owns column c of the factor in
// registers; step j (LAPACK dpotf2('U') order) needs column j's finished entries U[i][j], i < j, and the pivot -- all held
// by lane j -- in every lane, which is one v_mov_b64_dpp row_newbcast:j each (21 per factorisation, no LDS round trip, no
// wait; the earlier version went through LDS and paid a write -> read hand-off per pivot).  Lane j forms the pivot from its
// own column with the same operations as before (same bits).  The factor rows land in t.U at the end (the sigma points
// need ROWS of U: lane l reads row (l-1)%6, a transposition of the register layout).
// Returns false (row-uniform) when a pivot is <= 0 / NaN or P holds a non-finite entry -> the ladder.
template <int J>
SSA_DEV void chol_step(const double (&a)[6], double (&uc)[6], int lc, bool& ok)
{
    double v = a[J];                          // A[J][lc] (meaningful for lc >= J; lane J: the diagonal)
#pragma unroll
    for (int i = 0; i < J; ++i) {
        const double uij = row_bcast<J>(uc[i]);   // U[i][J]
        v = fma(-uij, uc[i], v);                  // lane J: ajj -= U[i][J]^2 ; lane c > J: A[J][c] -= U[i][J] U[i][c]
    }
    const double y = row_bcast<J>(rsqrt_nr(v));   // 1 / sqrt(pivot) of lane J; NaN / inf when the pivot is <= 0 or NaN
    // a bad pivot poisons everything downstream (row J becomes inf / NaN, every later pivot in its column picks up -inf or NaN),
    // so the positivity test of the LAST pivot covers all six
    if (J == 5) ok = ok && (y > 0.0) && (y <= 1.79769313486231570e308);
    uc[J] = (lc >= J) ? v * y : 0.0;              // lane J: ajj / sqrt(ajj) = the diagonal entry
}
// ---- The factorisation in the plain family (step_plain_kernel; FUSED, set by process_wave<.., ActPlain> alone).  The same operations on the
// same operands in the same order per entry -- the same bits -- with three things taken off the vector unit:
//  * the row broadcast of U[i][J] and the fused multiply-add that consumes it are ONE instruction, v_fmac_f64_dpp with the negated DPP source
//    (the compiler does not form it: the negation selects the three-address fma before its DPP combiner runs).  The loop runs RIGHT-looking
//    for it: as soon as row I of the factor exists, A[J][c] -= U[I][J] U[I][c] for every J > I, each accumulator still taking its terms in
//    the order I = 0 .. J - 1.  The six pivot broadcasts feed a v_mul_f64, which has no DPP form, and stay moves.
//  * no select per step: the lanes lc < J keep what the arithmetic leaves there.  No later step reads it (row_bcast<J'>(uc[i]) reads lane
//    J' > i, the last pivot's test reads lane 5); the factor tile's lower triangle is zeroed where the rows are stored (chol_store_rows_zeroed).
//  * the verdicts are wavefront masks in scalar registers from the compares on (chol_row_regs_fused).
// Wait states.  The hazard recogniser does not look inside an asm statement; a DPP instruction must not read a VGPR that a vector
// instruction wrote less than 2 wait states before it, and the compiler applies the rule to every VGPR operand, the accumulator included.
//  (a) uc[I], the DPP source, may be the instruction in front of the statement (v * y): the statement opens with s_nop 1, which is the
//      2 wait states for it and for anything else the compiler placed there (the first statement's accumulators, scale * pv).
//  (b) inside a statement every instruction has an accumulator of its own and none writes uc[I].
//  (c) the accumulators a statement writes are next read by a DPP instruction in the NEXT statement, which needs y of the next pivot: the
//      refined reciprocal square root of one of them, eight vector instructions at the least, lies in between by data dependence.
#define SSA_FMAC_BCAST(J) "v_fmac_f64_dpp %[v" #J "], -%[u], %[u] row_newbcast:" #J " row_mask:0xf bank_mask:0xf\n\t"
template <int I>
SSA_DEV void chol_row_update(double u, double (&v)[6])   // v[J] = fma(-row_bcast<J>(u), u, v[J]), J = I + 1 .. 5; u = uc[I]
{
    static_assert(I >= 0 && I < 5, "rows 0 .. 4 of the factor");
    if constexpr (I == 0)
        asm volatile("s_nop 1\n\t" SSA_FMAC_BCAST(1) SSA_FMAC_BCAST(2) SSA_FMAC_BCAST(3) SSA_FMAC_BCAST(4) SSA_FMAC_BCAST(5)
                     : [v1] "+v"(v[1]), [v2] "+v"(v[2]), [v3] "+v"(v[3]), [v4] "+v"(v[4]), [v5] "+v"(v[5]) : [u] "v"(u));
    else if constexpr (I == 1)
        asm volatile("s_nop 1\n\t" SSA_FMAC_BCAST(2) SSA_FMAC_BCAST(3) SSA_FMAC_BCAST(4) SSA_FMAC_BCAST(5)
                     : [v2] "+v"(v[2]), [v3] "+v"(v[3]), [v4] "+v"(v[4]), [v5] "+v"(v[5]) : [u] "v"(u));
    else if constexpr (I == 2)
        asm volatile("s_nop 1\n\t" SSA_FMAC_BCAST(3) SSA_FMAC_BCAST(4) SSA_FMAC_BCAST(5)
                     : [v3] "+v"(v[3]), [v4] "+v"(v[4]), [v5] "+v"(v[5]) : [u] "v"(u));
    else if constexpr (I == 3)
        asm volatile("s_nop 1\n\t" SSA_FMAC_BCAST(4) SSA_FMAC_BCAST(5) : [v4] "+v"(v[4]), [v5] "+v"(v[5]) : [u] "v"(u));
    else
        asm volatile("s_nop 1\n\t" SSA_FMAC_BCAST(5) : [v5] "+v"(v[5]) : [u] "v"(u));
}
#undef SSA_FMAC_BCAST
// step J of the FUSED form: v[J] arrives finished (chol_row_update<0 .. J - 1>); row J of the factor, then its terms into the rows below
template <int J>
SSA_DEV void chol_step_fused(double (&v)[6], double (&uc)[6], unsigned long long& bad)
{
    const double y = row_bcast<J>(rsqrt_nr(v[J]));   // as chol_step: NaN / inf when the pivot is <= 0 or NaN, and it poisons what follows
    if constexpr (J == 5)   // (y is row-uniform: so are the bits; one ballot per compare, see chol_row_regs_fused)
        bad |= __builtin_amdgcn_ballot_w64(!(y > 0.0)) | __builtin_amdgcn_ballot_w64(!(y <= 1.79769313486231570e308));
    uc[J] = v[J] * y;                                // (lanes lc < J: not an entry of the factor, see above)
    if constexpr (J < 5) chol_row_update<J>(uc[J], v);
}
// One entry of the matrix a rung factorises, in the REFERENCE's two roundings: sigma_points() hands robust_cholesky the product
// (n + lambda) P already rounded, and the ladder adds its jitter to that (dynamics.py:410: cholesky(a + e)).  Written out with an
// optimisation barrier between the two: under -ffp-contract=fast the compiler fused scale * p + jit into one fma at some call sites and -- where it could
// share scale * p with a neighbouring factorisation of the same matrix -- not at others.  One rounding more or less in a diagonal entry
// is nothing, except for the matrices the ladder exists for: (n + lambda) P of a diverged filter has condition 1e20, the factor's last
// rows move by 1e-8 relative with that bit, and two builds of the same source parted over an episode (round 3's "two-pass" ladder
// picked the SAME rungs as the sequential one -- ssa_ladder_probe_f64, tests/golden/ladder_illconditioned_tile.npz -- and still left
// different filters: its second factorisation was the unfused instance).  Now every instance is the reference's arithmetic.
SSA_DEV double scaled_entry(double scale, double pv, double jit)
{
    double sp = scale * pv;
    SSA_OPAQUE(sp);              // (two roundings: the product is a value of its own before the jitter is added)
    return sp + jit;
}
// factorises the matrix at Pg (row-major 6x6 in LDS) in the calling row `grow`; the factor's column lc stays in uc[]
template <bool PLAIN>   // PLAIN: the jitter-free first attempt (no diagonal select / add on the common path)
SSA_DEV bool chol_row_regs(const double* Pg, double scale, double jit, int grow, int l, double (&uc)[6])
{
    const int lc = l < 6 ? l : 5;   // lanes 6..15 shadow column 5 (their stores are masked)
    // column lc of the UPPER triangle of scale*P + jit*I (scipy.linalg.cholesky reads the upper triangle only); the six
    // owning lanes see all 36 entries between them: scipy's check_finite
    double a[6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double pv = Pg[j * 6 + lc];
        ok = ok && (fabs(pv) <= 1.79769313486231570e308);
        a[j] = (PLAIN || lc != j) ? scale * pv : scaled_entry(scale, pv, jit);
    }
    ok = ((__ballot(!ok) >> (grow * 16)) & 0xFFFFull) == 0;
    chol_step<0>(a, uc, lc, ok);
    chol_step<1>(a, uc, lc, ok);
    chol_step<2>(a, uc, lc, ok);
    chol_step<3>(a, uc, lc, ok);
    chol_step<4>(a, uc, lc, ok);
    chol_step<5>(a, uc, lc, ok);
    return ok;
}
SSA_DEV void chol_store_rows(double* Ug, const double (&uc)[6], int l)
{
    if (l < 6) {
#pragma unroll
        for (int j = 0; j < 6; ++j) Ug[j * 6 + l] = uc[j];
    }
}
// the lanes of every row whose bit is set in `m16`, as a condition: the wavefront mask is a scalar constant, no lane compares its index
SSA_DEV bool row_lanes(unsigned long long m16) { return __builtin_amdgcn_inverse_ballot_w64(m16 * 0x0001000100010001ull); }
// chol_row_regs in the FUSED form (chol_step_fused).  Returns the wavefront's FAILED lanes, whole rows of them, as a scalar mask: what
// __ballot(!ok) is of chol_row_regs' answer.  scipy's check_finite: lanes 0 .. 5 of a row see its 36 entries between them; their six bits
// of the compares' ballot decide the row (lanes 6 .. 15 repeat lane 5).  Per 16-bit field: bit 15 of (bits + 0x7fff) is "some bit is set"
// -- the sum stays inside the field -- and h | (h - (h >> 15)) fills the field from it.
template <bool PLAIN>
SSA_DEV unsigned long long chol_row_regs_fused(const double* Pg, double scale, double jit, int l, double (&uc)[6])
{
    const int lc = l < 6 ? l : 5;
    double a[6];
    unsigned long long nf = 0ull;   // (one ballot per compare, joined as scalars: the ballot of a joined condition goes through a select and a compare)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double pv = Pg[j * 6 + lc];
        nf |= __builtin_amdgcn_ballot_w64(!(fabs(pv) <= 1.79769313486231570e308));
        a[j] = (PLAIN || lc != j) ? scale * pv : scaled_entry(scale, pv, jit);
    }
    nf &= 0x003F003F003F003Full;
    const unsigned long long h = (nf + 0x7FFF7FFF7FFF7FFFull) & 0x8000800080008000ull;
    unsigned long long bad = h | (h - (h >> 15));
    chol_step_fused<0>(a, uc, bad);
    chol_step_fused<1>(a, uc, bad);
    chol_step_fused<2>(a, uc, bad);
    chol_step_fused<3>(a, uc, bad);
    chol_step_fused<4>(a, uc, bad);
    chol_step_fused<5>(a, uc, bad);
    return bad;
}
// chol_store_rows for the FUSED form, whose lanes l < j hold no zeros in uc[j]: the six rows as they are, then +0.0 over the fifteen
// entries (j, c < j) of the strictly lower triangle, by lanes of the same address &Ug[l] through two more two-address writes -- entry
// 6 j + c is l + 6 / l + 18 for l in {0, 6, 7, 12, 13, 14}, l + 26 / l + 33 for l in {0, 1}: all fifteen, each inside the block, none on
// or above the diagonal.  A wavefront's LDS writes land in issue order, so the zeros replace what the first three writes left there.
// (Every step: the transform and the update use the factor tile as scratch.)
SSA_DEV void chol_store_rows_zeroed(double* Ug, const double (&uc)[6], int l)
{
    double* col = Ug + l;
    if (row_lanes(0x003Full)) {
#pragma unroll
        for (int j = 0; j < 6; ++j) col[j * 6] = uc[j];
    }
    wave_lds_sync();   // (the order ACROSS lanes: to the compiler col[6] of one lane and col[12] of another are unrelated)
    double z = 0.0;
    SSA_OPAQUE(z);     // (one register pair for both writes)
    if (row_lanes(0x70C1ull)) {
        col[6] = z;
        col[18] = z;
    }
    if (row_lanes(0x0003ull)) {
        col[26] = z;
        col[33] = z;
    }
}

// robust_cholesky (dynamics.py:402-417) for the four objects of the wavefront: plain attempt, then a + 10^i I for
// i = -6..9 (first success wins); returns the calling row's -1, 0..15, or 16 (LinAlgError).
// The plain attempt runs row-parallel (each row its own object); the rows that fail then try all sixteen rungs at once, one
// lane per rung (robust_chol_row_lds below).
__constant__ double JITTER[16] = {1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, 10.0, 100.0, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9};
// Does scale * P + jit * I factorise?  ONE lane decides, alone, in its own registers: the ladder's unit of work when every lane
// of a row tries its own rung (robust_chol_row_lds below).  Operation by operation the arithmetic of chol_row_regs<false> --
// the same matrix entries (scaled_entry), the same fused multiply-adds in the same order, the same refined reciprocal square
// root -- so a rung succeeds here exactly when it succeeds there (with round 3's fused diagonal the one-pass ladder reproduced the
// round-3 library bit for bit over 20 000-object episodes of all three propagators: profiles/r04_ab_ladder_against_round3.txt).
// Only the verdict leaves: an entry U[i][c] is dead once step c has used it, so at most nine entries are live at a time
// (a lane that kept its whole factor, 42 registers, made the closed-loop kernels spill); the winning rung's factor is then
// formed once more by the row (chol_row_regs<false>), which is where it is needed in the row-distributed layout anyway.
// The matrix is read from LDS where it is used (the lanes of a row read the same address: a broadcast).
SSA_DEV bool chol_lane_ok(const double* Pg, double scale, double jit)
{
    double U[21];
    double y = 0.0;
#pragma unroll
    for (int J = 0; J < 6; ++J) {
        double vp = scaled_entry(scale, Pg[J * 6 + J], jit);
#pragma unroll
        for (int i = 0; i < J; ++i) vp = fma(-U[tri(i, J)], U[tri(i, J)], vp);
        y = rsqrt_nr(vp);               // NaN / inf when the pivot is <= 0 or NaN: poisons everything behind it (see chol_step)
#pragma unroll
        for (int c = J + 1; c < 6; ++c) {
            double v = scale * Pg[J * 6 + c];
#pragma unroll
            for (int i = 0; i < J; ++i) v = fma(-U[tri(i, J)], U[tri(i, c)], v);
            U[tri(J, c)] = v * y;
        }
    }
    return (y > 0.0) && (y <= 1.79769313486231570e308);
}
template <bool FUSED = false>   // FUSED: the plain family's factorisation (chol_step_fused), the first attempt and the winning rung's both
SSA_DEV int robust_chol_row_lds(Tiles& t, double scale, int g, int l)
{
    double uc[6];
    int rung = 16;
    unsigned long long bad;
    if constexpr (FUSED) {
        bad = chol_row_regs_fused<true>(&t.P[g * 36], scale, 0.0, l, uc);
        if (!__builtin_amdgcn_inverse_ballot_w64(bad)) {
            chol_store_rows_zeroed(&t.UA[g * 36], uc, l);
            rung = -1;
        }
    } else {
        const bool ok = chol_row_regs<true>(&t.P[g * 36], scale, 0.0, g, l, uc);
        if (ok) {
            chol_store_rows(&t.UA[g * 36], uc, l);
            rung = -1;
        }
        bad = __ballot(!ok);
    }
    wave_lds_sync();
    if (bad == 0ull) return rung;                  // the common case, wave-uniform
    __builtin_amdgcn_s_setprio(3);                 // a straggler in the making: issue priority for the rest of its life
    // The ladder in ONE pass, every failed row at once: lane l of a row decides, whole and alone (chol_lane_ok), whether its
    // row's matrix factorises with rung l's jitter, so the sixteen rungs of up to four objects are tried side by side; the
    // FIRST rung that succeeds -- the reference's sequential answer, dynamics.py:406-414, also where success is not monotone
    // in the jitter: every rung is actually tried -- is the lowest set bit of the row's ballot, and the row forms that rung's
    // factor.  Two factorisations' latency whatever the rung and however many of the four objects need the ladder (before:
    // the rows took turns, four rungs per pass: a wavefront with four diverged objects at rungs 12-15 ran sixteen passes back
    // to back and held the end of a late-episode launch, profiles/r03_wave_timeline_hybrid_step400.txt).
    const bool mine = ((bad >> (g * 16)) & 1ull) != 0ull;   // row-uniform
    if (mine) {
        const double* Pg = &t.P[g * 36];
        const double jit = JITTER[l];
        bool finite = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int idx = l + 16 * r;
            if (idx < 36) finite = finite && (fabs(Pg[idx]) <= 1.79769313486231570e308);
        }
        finite = ((__ballot(!finite) >> (g * 16)) & 0xFFFFull) == 0ull;      // scipy's check_finite: the whole matrix
        const bool okr = chol_lane_ok(Pg, scale, jit) && finite;
        const unsigned won = (unsigned)((__ballot(okr) >> (g * 16)) & 0xFFFFull);
        if (won != 0u) {
            rung = __ffs((int)won) - 1;
            const double jw = __shfl(jit, g * 16 + rung, 64);            // the winning rung's jitter, from the lane that tried it
            if constexpr (FUSED) {                                       // (succeeds: the same arithmetic said so)
                chol_row_regs_fused<false>(Pg, scale, jw, l, uc);
                chol_store_rows_zeroed(&t.UA[g * 36], uc, l);
            } else {
                chol_row_regs<false>(Pg, scale, jw, g, l, uc);
                chol_store_rows(&t.UA[g * 36], uc, l);
            }
        }
    }
    wave_lds_sync();
    return rung;
}

// the action of env e: the word in memory, or the value in the parameter block (SSA_LAUNCH_INLINE_ACTION, one env)
// (word e of an array in the parameter block, by a chain of selects over constant indices: a register-indexed read would make
// the kernels that keep a modified copy of the block -- rollout, closed loop -- spill the whole array to scratch)
SSA_DEV int inline_word(const int32_t (&w)[SSA_INLINE_ENVS], int e)
{
    int v = w[0];
#pragma unroll
    for (int i = 1; i < SSA_INLINE_ENVS; ++i) v = (e == i) ? w[i] : v;
    return v;
}
// INL = false: the instance never sees SSA_LAUNCH_INLINE_ENVS (rollout and closed-loop kernels, whose per-step copy of the block
// stays in scalar registers only while nothing indexes into it)
// SEG = true: `p` IS the parameter block of a one-tile kernel, in its argument segment (process_wave<.., 0>).  The word then has ONE source
// address -- device memory or the word's copy in the segment, which are the same address space to a load -- selected from launch_mask, and one
// load: with one env a scalar load from the constant address space (wave-uniform; no wavefront of a step launch writes these words, and the
// scalar cache starts every kernel empty, so what an earlier launch wrote is seen), with several a per-lane global load.  Written as
// `mask ? p.action0 : p.actions[e]` the compiler forms the same select of two addresses, but of generic ones, and loads through the FLAT
// segment: a vector-memory AND an LDS-queue wait behind the tile's loads.
template <class T> using ConstPtr = const __attribute__((address_space(4))) T*;
typedef const __attribute__((address_space(1))) int32_t* GlobalWords;
typedef int v4i __attribute__((ext_vector_type(4)));
SSA_DEV ConstPtr<ssa_step_params> tile_kernel_params();   // (the one-tile kernels' block in the segment: defined behind TileArgs)
template <bool TIME>
SSA_DEV ConstPtr<int32_t> segment_word_src(uint32_t m, const int32_t* mem)   // env 0's word: formed from scalars alone
{
    const ConstPtr<ssa_step_params> seg = tile_kernel_params();
    if (TIME) return (m & SSA_LAUNCH_INLINE_ENVS) ? seg->inline_time : (ConstPtr<int32_t>)mem;
    return (m & SSA_LAUNCH_INLINE_ENVS) ? seg->inline_action : (m & SSA_LAUNCH_INLINE_ACTION) ? &seg->action0 : (ConstPtr<int32_t>)mem;
}
// (several envs: env e's word, per lane.  It is waited for HERE, inside the caller's branch: at the join with the one-env path the compiler
// would otherwise have to assume a vector load outstanding on either path, and put the one-env path's first use behind the tile's loads)
SSA_DEV int segment_lane_word(ConstPtr<int32_t> src, int e)
{
    int w = ((GlobalWords)src)[e];
    asm volatile("" : "+v"(w));
    return w;
}
template <bool TIME>
SSA_DEV int segment_env_word(const ssa_step_params& p, int e)
{
    const ConstPtr<int32_t> src = segment_word_src<TIME>(p.launch_mask, TIME ? p.env_time : p.actions);
    if (p.n_env > 1) return segment_lane_word(src, e);
    return *src;
}
template <bool INL = true, bool SEG = false>
SSA_DEV int env_action(const ssa_step_params& p, int e)
{
    if (SEG) return segment_env_word<false>(p, e);
    if (INL && (p.launch_mask & SSA_LAUNCH_INLINE_ENVS)) return inline_word(p.inline_action, e);
    return (p.launch_mask & SSA_LAUNCH_INLINE_ACTION) ? p.action0 : p.actions[e];
}
// ... and its time index (before time_offset): the word in memory, or the parameter block's (SSA_LAUNCH_INLINE_ENVS)
template <bool INL = true, bool SEG = false>
SSA_DEV int env_time_of(const ssa_step_params& p, int e)
{
    if (SEG) return segment_env_word<true>(p, e);
    return (INL && (p.launch_mask & SSA_LAUNCH_INLINE_ENVS)) ? inline_word(p.inline_time, e) : p.env_time[e];
}
// tix % n_time, the division (a ~25-instruction sequence on the vector unit) only when the index has actually wrapped
SSA_DEV int time_row(int tix, int n_time)
{
    if (n_time <= 0) return 0;
    return ((unsigned)tix < (unsigned)n_time) ? tix : tix % n_time;
}
// hx of a MOVING sensor s of a network (ssa_step_params.site_moving): hx_aer_enu with the sensor's 12 site words taken from row
// (time row, s) of ssa_step_params.site_rows instead of the sites' block.  A network's tile belongs to one env, so the time row is the
// wavefront's (the first active lane's), the row's address is formed from scalars and its 128 bytes come by scalar loads from the constant
// address space -- nothing of the launch writes the table -- into scalar registers, where the block's site words live on the other path.
// Issued here, behind the predict, whose lanes never wait for it.  lim: the mask every real elevation clears (a moving sensor has no
// horizon).  Returns whether the sphere of limb_radius blocks the line of sight from the sensor to the lane's state x.
SSA_DEV bool hx_moving_site(const ssa_step_params& p, int n_sensor, int s, int tix, const double* x, const double* M, double* z, double* R,
                            double& lim)
{
    const int row = __builtin_amdgcn_readfirstlane(time_row(tix, p.n_time));
    const ConstPtr<double> src = (ConstPtr<double>)__builtin_assume_aligned(p.site_rows, 128) + ((int64_t)row * n_sensor + s) * 16;
    double site[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) site[i] = src[i];
    hx_aer_enu(x, M, site, site + 9, z, R);
    // the vector hx_aer_enu has just formed, behind a barrier: the rule's own products (d.d among them) must not be merged with those of
    // hx_aer_enu's range -- under -ffp-contract=fast a shared d0 * d0 changes which product of the sum is fused, and the range then differs
    // in its last bit from the one the ground path computes from the same words (tests/test_orbiting_gpu.py pins the equality).
    // Every lane of the row evaluates the rule on its own state; only the truth lane's verdict (lane 13) reaches the broadcast that
    // decides visibility -- the sigma lanes' is formed and dropped, which is cheaper than a lane test around a dozen instructions
    double d[3];
    observer_to_object(x, M, site + 9, d);
    SSA_OPAQUE(d[0]);
    SSA_OPAQUE(d[1]);
    SSA_OPAQUE(d[2]);
    lim = -__builtin_inf();
    return !los_clear(d, site + 9, p.limb_radius);
}

// O4 for one object (ssa_tasker_simple_2.py:834-840): [hx(x_filter[:3]), trace(P)], NaN/inf -> 0.001
SSA_DEV void aer_obs_row(const double* x, const double* P, const ssa_step_params& p, const ssa_consts& C, int e, int64_t obj)
{
    if (p.aer_cols == 1) {   // trace P only
        const double tr1 = P[0] + P[7] + P[14] + P[21] + P[28] + P[35];
        p.aer_out[obj] = (fabs(tr1) <= 1.79769313486231570e308) ? tr1 : 0.001;
        return;
    }
    const int tix = env_time_of(p, e) + p.time_offset;
    const double* M = p.trans + (int64_t)((p.n_time > 0) ? tix % p.n_time : 0) * 9;
    double Mm[9], xx[3] = {x[0], x[1], x[2]}, z[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Mm[i] = M[i];
    hx_aer(xx, Mm, C.enu, C.obs_itrs, z);
    const double tr = P[0] + P[7] + P[14] + P[21] + P[28] + P[35];
    const double v[4] = {z[0], z[1], z[2], tr};
#pragma unroll
    for (int c = 0; c < 4; ++c) p.aer_out[obj * 4 + c] = (fabs(v[c]) <= 1.79769313486231570e308) ? v[c] : 0.001;
}

// The same block in the step kernel's epilogue, from the tiles, on lanes 0..3 of the object's row: lane c produces component
// c.  Azimuth (lane 0) and elevation (lane 1) are both ONE atan2 -- az = atan2(n, e), el = atan2(u, hypot(e, n)) -- so the
// two lanes walk the same instruction stream once (hx_aer evaluates them one after the other), lane 2 keeps the range,
// lane 3 trace(P); one 8-byte store per lane, 32 contiguous bytes per object.
SSA_DEV void aer_obs_tile_at(const Tiles& t, const ssa_step_params& p, const ssa_consts& C, int g, int l, int64_t obj, int tix)
{
    const double* M = p.trans + (int64_t)time_row(tix, p.n_time) * 9;
    const double* x = &t.X[g * 6];
    const double* P = &t.P[g * 36];
    double d[3], R[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = M[i * 3] * x[0] + M[i * 3 + 1] * x[1] + M[i * 3 + 2] * x[2] - C.obs_itrs[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) R[j] = C.enu[j] * d[0] + C.enu[3 + j] * d[1] + C.enu[6 + j] * d[2];
    const double h2 = R[0] * R[0] + R[1] * R[1];
    const double rt = sqrt_fast((l == 1) ? h2 : d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);   // lane 1: hypot(e, n); others: the range
    double a = atan2_fast((l == 1) ? R[2] : R[1], (l == 1) ? rt : R[0]);
    if (l == 0 && a < 0.0) a += TWO_PI;
    const double tr = P[0] + P[7] + P[14] + P[21] + P[28] + P[35];
    const double v = (l < 2) ? a : (l == 2) ? rt : tr;
    const double w = (fabs(v) <= 1.79769313486231570e308) ? v : 0.001;
    if (p.launch_mask & SSA_LAUNCH_MIRROR_F32) reinterpret_cast<float*>(p.aer_out)[obj * 4 + l] = (float)w;
    else p.aer_out[obj * 4 + l] = w;
}
template <bool INL, bool SEG>
SSA_DEV void aer_obs_tile(const Tiles& t, const ssa_step_params& p, const ssa_consts& C, int g, int l, int e, int64_t obj)
{
    if (p.aer_cols == 1) {   // trace P only: lane 0 of the row
        if (l == 0) {
            const double* P = &t.P[g * 36];
            const double tr = P[0] + P[7] + P[14] + P[21] + P[28] + P[35];
            const double w = (fabs(tr) <= 1.79769313486231570e308) ? tr : 0.001;
            if (p.launch_mask & SSA_LAUNCH_MIRROR_F32) reinterpret_cast<float*>(p.aer_out)[obj] = (float)w;
            else p.aer_out[obj] = w;
        }
        return;
    }
    // one env: the time index is wave-uniform, so the GCRS->ITRS matrix arrives by scalar loads (nine per-lane loads otherwise)
    if (p.n_env > 1) aer_obs_tile_at(t, p, C, g, l, obj, env_time_of<INL, SEG>(p, e) + p.time_offset);
    else aer_obs_tile_at(t, p, C, g, l, obj, env_time_of<INL, SEG>(p, 0) + p.time_offset);
}


// SSA_LAUNCH_FOLD_INSIDE: the statistics of the step are folded by the LAST wavefront of the launch to finish its atomics instead
// of by a fold kernel behind it (a caller that needs them on the host right after the step -- the gym env -- saves a dependent
// launch, ~4 us on the GPU and 2 us of enqueueing).  Word 3 of every shard counts the tiles that have added to it, word 4 of shard 0
// the shards that are complete; a wavefront bumps them only after its own atomics are acknowledged, so whoever completes the last
// shard reads finished sums (agent-scope loads), writes `stats` and clears shards and counters for the next step.
// (one lane, after its atomics into shard `tile & 127` of env e are acknowledged) counts the tile; true = it completed env e.
// Tiles that add to env e: t_lo = first object / 4 ... t_hi = last object / 4 (a tile that straddles two envs counts in both).
SSA_DEV bool stat_tile_counted(const ssa_step_params& p, int64_t e, int tile)
{
    const int64_t first = e * p.n_obj;
    const int t_lo = (int)(first / OBJ_PER_WAVE), t_hi = (int)((first + p.n_obj - 1) / OBJ_PER_WAVE);
    const int shard = tile & (SSA_STAT_SHARDS - 1);
    // tiles of [t_lo, t_hi] congruent to `shard` modulo 128 (arithmetic shifts: floor division of the negative operands too)
    const unsigned expect = (unsigned)(((t_hi - shard) >> 7) - ((t_lo - 1 - shard) >> 7));
    unsigned long long* env0 = (unsigned long long*)p.stat_shards + e * SSA_STAT_SHARDS * SSA_STAT_SHARD_WORDS;
    unsigned long long* sh = env0 + (int64_t)shard * SSA_STAT_SHARD_WORDS;
    const unsigned old = (unsigned)__hip_atomic_fetch_add(sh + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old != expect - 1u) return false;
    __hip_atomic_store(sh + 3, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int nt = t_hi - t_lo + 1;
    const unsigned used = (unsigned)(nt < SSA_STAT_SHARDS ? nt : SSA_STAT_SHARDS);
    const unsigned old2 = (unsigned)__hip_atomic_fetch_add(env0 + 4, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old2 != used - 1u) return false;
    __hip_atomic_store(env0 + 4, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}
// ---- arg-max of sigma_pos on the one-launch paths (the 'shaped' reward needs np.argmax(sigma_pos[i - 1]),
// ssa_tasker_simple_2.py:346).  Every wavefront leaves (key, index) of its tile's first maximum in the tile's slot of `spos_tiles`
// -- no atomics -- and whoever folds the statistics shards reduces the slots with np.argmax's semantics: the first maximum, and a
// NaN ranks above everything (the first NaN wins).  key = the double's bits (sigma_pos >= 0: non-negative doubles order like
// unsigned integers, NaN -- canonicalised -- above infinity); index = the object's index in its env.
constexpr unsigned long long SPOS_NAN_KEY = 0x7ff8000000000000ull;
SSA_DEV unsigned long long spos_key(double v)
{
    return (v != v) ? SPOS_NAN_KEY : ((unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull);
}
SSA_DEV double spos_of_key(unsigned long long k) { return __longlong_as_double((long long)k); }
// first maximum of the tile's `cnt` objects (lane-local: any lane may call it; reads t.Met)
// (ids: the rows' indices as the CALLER numbers them -- ssa_step_params.obj_ids, a layout that stores the objects in another order: the
// first maximum is then the one with the lowest such index, whatever row it sits in)
SSA_DEV void spos_tile_best(const Tiles& t, int cnt, int64_t j0, unsigned long long& key, unsigned long long& idx, bool ids = false)
{
    key = spos_key(t.Met[2]);
    idx = ids ? (unsigned long long)t.Oid[0] : (unsigned long long)j0;
#pragma unroll
    for (int g = 1; g < OBJ_PER_WAVE; ++g) {
        const unsigned long long k = spos_key(t.Met[g * 4 + 2]);
        const unsigned long long ig = ids ? (unsigned long long)t.Oid[g] : (unsigned long long)(j0 + g);
        if (g < cnt && (k > key || (ids && k == key && ig < idx))) { key = k; idx = ig; }
    }
}
// 64-bit wave folds by DPP rotations + readlanes (see the closed loop, which introduced them)
template <int CTRL>
SSA_DEV unsigned long long dpp_u64(unsigned long long v)
{
    return (unsigned long long)__builtin_amdgcn_update_dpp((long long)v, (long long)v, CTRL, 0xF, 0xF, true);
}
SSA_DEV unsigned long long lane_u64(unsigned long long v, int l)
{
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (unsigned)__builtin_amdgcn_readlane((int)v, l);
}
struct OpMax { SSA_DEV unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a > b ? a : b; } };
struct OpMin { SSA_DEV unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a < b ? a : b; } };
struct OpAdd { SSA_DEV unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; } };
template <class OP>
SSA_DEV unsigned long long wave_fold_u64(unsigned long long v, OP op)
{
    v = op(v, dpp_u64<0x128>(v));   // row_ror:8
    v = op(v, dpp_u64<0x124>(v));   // row_ror:4
    v = op(v, dpp_u64<0x122>(v));   // row_ror:2
    v = op(v, dpp_u64<0x121>(v));   // row_ror:1
    return op(op(lane_u64(v, 0), lane_u64(v, 16)), op(lane_u64(v, 32), lane_u64(v, 48)));
}
// reduces the slots of env e's tiles (tiles [t_lo, t_hi]: whole tiles of ONE env -- the launcher refuses spos_tiles for envs whose
// object count is not a multiple of four unless there is only one env) into stats.  COHERENT: agent-scope loads (the slots were
// written by other wavefronts of the SAME launch: SSA_LAUNCH_FOLD_INSIDE); otherwise a kernel boundary lies in between.
template <bool COHERENT>
SSA_DEV void fold_spos_tiles(const unsigned long long* __restrict__ slots, int t_lo, int t_hi, double* __restrict__ stats, int lane)
{
    unsigned long long key = 0ull, idx = ~0ull;
    bool any = false;
    for (int tb = t_lo + lane; tb <= t_hi; tb += 64) {
        unsigned long long k, i;
        if (COHERENT) {
            k = __hip_atomic_load(slots + 2 * (int64_t)tb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            i = __hip_atomic_load(slots + 2 * (int64_t)tb + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(slots + 2 * (int64_t)tb);
            k = v.x; i = v.y;
        }
        if (!any || k > key || (k == key && i < idx)) { key = k; idx = i; any = true; }      // (ties: the lower index -- the earlier tile, unless a layout renumbers)
    }
    const unsigned long long top = wave_fold_u64(any ? key : 0ull, OpMax());
    const unsigned long long who = wave_fold_u64((any && key == top) ? idx : ~0ull, OpMin());
    if (lane == 0) {
        stats[SSA_STAT_ARGMAX_SPOS] = (double)(long long)who;
        stats[SSA_STAT_MAX_SPOS] = spos_of_key(top);
    }
}
// tiles of env e (whole tiles; one env: all of them)
SSA_DEV void env_tile_range(int64_t n_obj, int e, int& t_lo, int& t_hi)
{
    const int64_t first = (int64_t)e * n_obj;
    t_lo = (int)(first / OBJ_PER_WAVE);
    t_hi = (int)((first + n_obj - 1) / OBJ_PER_WAVE);
}
SSA_DEV void fold_stat_shards_inside(unsigned long long* __restrict__ shards, double* __restrict__ stats, int lane)
{
    unsigned long long* sh = shards + (int64_t)lane * SSA_STAT_SHARD_WORDS;
    unsigned long long* sh2 = sh + 64 * SSA_STAT_SHARD_WORDS;
    unsigned long long mx = __hip_atomic_load(sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long cn = __hip_atomic_load(sh + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long nf = __hip_atomic_load(sh + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long mb = __hip_atomic_load(sh2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long cb = __hip_atomic_load(sh2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long nb = __hip_atomic_load(sh2 + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        __hip_atomic_store(sh + q, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(sh2 + q, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    mx = mb > mx ? mb : mx;
    cn += cb;
    nf += nb;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long m2 = __shfl_down(mx, off, 64), c2 = __shfl_down(cn, off, 64), n2 = __shfl_down(nf, off, 64);
        mx = m2 > mx ? m2 : mx;
        cn += c2;
        nf += n2;
    }
    if (lane == 0) {
        stats[SSA_STAT_MAX_DPOS] = __longlong_as_double((long long)mx);
        stats[SSA_STAT_CNT_LT_1E4] = (double)(cn & 0xffffffffull);
        stats[SSA_STAT_CNT_LT_1E7] = (double)(cn >> 32);
        stats[SSA_STAT_ARGMAX_SPOS] = -1.0;
        stats[SSA_STAT_N_FAILED] = (double)nf;
        stats[SSA_STAT_MAX_SPOS] = __builtin_nan("");
        stats[6] = 0.0; stats[7] = 0.0;
    }
}

// SSA_LAUNCH_STATS_FROM_METRICS: service wavefront w of nserv (<= SSA_STAT_SHARDS) reduces its slice of the delta_pos row the previous
// step stored -- every load issued before the first use, 64 objects per instruction -- into ONE partial: max as ordered bits and the
// packed trinary counts, exactly the words the step kernel's atomics would have summed.  The partial goes to words 0 / 1 of shard line w
// (plain agent-scope stores: the line is this wavefront's own), then one returning atomic takes a ticket on word 4 of shard 0; whoever
// draws the last ticket folds the lines -- the partials and the failure counts the step's own wavefronts added to word 2 -- as the
// last tile of SSA_LAUNCH_FOLD_INSIDE does, and leaves lines and ticket word zero.
constexpr int STAT_SERVICE_WAVES = 32, STAT_SERVICE_ILP = 10;   // (20 000 objects: 625 per wavefront, one pass of ten loads per lane)
static_assert(STAT_SERVICE_WAVES <= SSA_STAT_SHARDS, "one shard line per service wavefront");
SSA_DEV void stats_service_wave(const double* __restrict__ dpos, unsigned long long* __restrict__ shards, double* __restrict__ stats,
                                const unsigned long long* __restrict__ spos, int64_t n_obj, int w, int nserv, int lane)
{
    const uint32_t n = (uint32_t)n_obj;                       // (n_env * n_obj < 2^31: the launcher)
    const uint32_t per = (n + (uint32_t)nserv - 1u) / (uint32_t)nserv;
    const uint32_t lo = (uint32_t)w * per < n ? (uint32_t)w * per : n;
    const uint32_t hi = n - lo < per ? n : lo + per;
    unsigned long long mx = 0ull, cn = 0ull;
    for (uint32_t b = lo; b < hi; b += 64u * STAT_SERVICE_ILP) {
        double v[STAT_SERVICE_ILP];
#pragma unroll
        for (int q = 0; q < STAT_SERVICE_ILP; ++q) {
            const uint32_t i = b + (uint32_t)(q * 64 + lane);
            v[q] = i < hi ? dpos[i] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < STAT_SERVICE_ILP; ++q) {
            const uint32_t i = b + (uint32_t)(q * 64 + lane);
            if (i < hi) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(v[q]) & 0x7fffffffffffffffull;
                mx = bits > mx ? bits : mx;
                cn += (unsigned long long)(v[q] < 1e4) + ((unsigned long long)(v[q] < 1e7) << 32);
            }
        }
    }
    mx = wave_fold_u64(mx, OpMax());
    cn = wave_fold_u64(cn, OpAdd());
    bool last = false;
    if (lane == 0) {
        unsigned long long* sh = shards + (int64_t)w * SSA_STAT_SHARD_WORDS;
        __hip_atomic_store(sh, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(sh + 1, cn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the partial is in before its ticket is drawn
        const unsigned old = (unsigned)__hip_atomic_fetch_add(shards + 4, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == (unsigned)nserv - 1u) {
            __hip_atomic_store(shards + 4, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = true;
        }
    }
    if (__any(last)) {
        fold_stat_shards_inside(shards, stats, lane);
        if (spos) {     // (the slots were written by the previous launch: a kernel boundary lies in between)
            int t_lo, t_hi;
            env_tile_range(n_obj, 0, t_lo, t_hi);
            fold_spos_tiles<false>(spos, t_lo, t_hi, stats, lane);
        }
    }
}

// ActBase: what an action source is unless it says otherwise -- the action is in memory (get() = -1: nothing to wait for, nothing to do
// while waiting or in mid-step), no kind of process_wave's applies, and there are no sensor sites.  Each source below states only what
// sets it apart: its kind as the flags process_wave reads, and sites().
struct ActBase {
    static constexpr bool late = false;           // the action is decided on the device while the step runs (ActLate)
    static constexpr bool all = false;            // the lookahead: every row updated hypothetically, nothing committed
    static constexpr bool sensors = false;        // a sensor network: one update per sensor, each with its own site
    static constexpr bool look_sensors = false;   // the lookahead of a sensor network: `all`, one pass per sensor
    static constexpr bool forecast = false;       // ... as step h of a forecast: `look_sensors` on a resident tile
    static constexpr bool envs = false;           // `sensors` in each of several envs: a row of actions per env (ActSensorEnvs)
    static constexpr bool look_envs = false;      // `look_sensors` in each of several envs (ActLookSensorEnvs)
    static constexpr bool plain = false;          // the plain one-env launch form, decided by the launcher (ActPlain)
    static constexpr bool dryrun = false;         // `sensors` + `envs` as a dry run: P+ committed to the tile, x kept, records only (ActDryRunEnvs)
    SSA_DEV int get() { return -1; }
    SSA_DEV void before_wait(Tiles&, int, int) {}
    SSA_DEV void mid_step(Tiles&, int) {}
    SSA_DEV const ssa_sensor_params* sites() const { return nullptr; }
};
// One wavefront advances up to 4 consecutive objects (one per 16-lane row) by one env step, complete semantics:
// the robust_cholesky ladder is inline, conic branches beyond the strong-elliptic one are out-of-line calls taken
// only by the lanes that need them.
// TILE: 0 = the tile is loaded here; 1 = it was prefetched (commit now, request the next one after the
// Kepler stage); 2 = the tiles already hold the state (a rollout's later steps)
// Where a wavefront learns its env's action.  ActEarly: the action word is in memory when the step starts (per-step launches,
// rollouts).  ActLate (closed_loop_kernel, one env): the action of step k is decided ON THE DEVICE from the state step k - 1
// left, while the predicts of step k are already running -- a wavefront asks for it only where the update needs it, behind
// its predict, and every row prefetches the update's inputs for its OWN object in case it turns out to be the selected one.
struct ActEarly : ActBase {};
// ActPlain (step_plain_kernel): ActEarly for the launch form the launcher has already recognised (step_plain_form) -- one env, the action
// and time words in memory, statistics from the metrics rows with a deferred fold, an update in every step, no resampling, az-el-range
// measurements, no aer_out / obs_mirror / spos_tiles / stat_shards_clear.  What process_wave decides per wavefront from the argument
// segment for every other form is a constant here; the arithmetic is the same, instruction for instruction.
struct ActPlain : ActBase {
    static constexpr bool plain = true;
};
struct ActLate;
struct LoopK;
SSA_DEV void closed_loop_prescore(ActLate& a, Tiles& t, int lane, int cnt);   // (defined with the closed-loop kernel)
SSA_DEV void closed_loop_store(const LoopK* lk, Tiles& t, int lane, int kk, int64_t base, int cnt);
constexpr unsigned CL_ABORT_GEN = 0xFFFFFFFFu;            // decision number that means "give up" (a wavefront timed out)
constexpr unsigned long long CL_TIMEOUT_TICKS = 200000000ull;   // default bound of a wait: 2 s of the 100 MHz wall clock (ssa_closed_loop_params.wait_ticks)
struct ActLate : ActBase {
    static constexpr bool late = true;
    unsigned long long* flag;        // this wavefront's group flag: (decision number << 32) | action
    unsigned long long* all_flags;   // [nflags] flags, 16 words apart (abort broadcast)
    int* err;                        // device word set to 1 on a timeout (may be host-mapped)
    int nflags;
    unsigned long long timeout;      // bound of every wait, 100 MHz ticks
    unsigned want;                   // decision needed: the step's index (>= 1); 0 = `first`
    int first;                       // action of the launch's first step (decided by the caller)
    int last;                        // the action get() returned most recently
    bool aborted;
    int agent;                       // SSA_AGENT_*
    const ssa_consts* C;             // (kernarg copy)
    const double* M;                 // GCRS -> ITRS matrix of the current step
    int* vis;                        // [OBJ_PER_WAVE] in LDS: visibility of the tile's objects at the current step
    // work that does not depend on the decision, done where a wavefront would otherwise only wait for it: the visibility of its
    // objects' NEW true states (the agents' mask, agents.py:36-42) -- off the path decision -> update -> score -> decision
    SSA_DEV void before_wait(Tiles& t, int lane, int cnt) { closed_loop_prescore(*this, t, lane, cnt); }
    // The outputs of step k leave for HBM inside step k + 1, behind its Cholesky stage (the tile is intact until then): right
    // after the decision every wavefront is released at once, and 18 MB of tile stores issued at that moment delayed the
    // acknowledgements of the parts the NEXT decision waits for (late announcers: +3 us);
    // here they overlap the Kepler stage instead.
    const LoopK* lk;                 // the kernel's argument block
    int pend;                        // step whose tile is still to be stored (-1: none)
    int64_t base;
    int cnt;
    SSA_DEV void mid_step(Tiles& t, int lane)
    {
        if (pend < 0) return;
        closed_loop_store(lk, t, lane, pend, base, cnt);
        pend = -1;
    }
    SSA_DEV void abort_all()
    {
        const int lane = threadIdx.x;
        for (int i = lane; i < nflags; i += 64)
            __hip_atomic_store(all_flags + (int64_t)i * 16, (unsigned long long)CL_ABORT_GEN << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0 && err) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // the decision `want`: polls the group flag (agent-scope loads: coherent across the XCDs' L2s) with a bounded wait -- every
    // wavefront reaches an exit whatever the others do
    SSA_DEV int get()
    {
        if (want == 0u) { last = first; return first; }
        const unsigned long long t0 = wall_clock64();
        unsigned lo, hi;
        for (;;) {
            const unsigned long long v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lo = __builtin_amdgcn_readfirstlane((unsigned)v);
            hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
            if (hi >= want) break;
            if (wall_clock64() - t0 > timeout) {
                abort_all();
                hi = CL_ABORT_GEN;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        if (hi == CL_ABORT_GEN) {
            aborted = true;
            return -2;
        }
        last = (int)lo;
        return (int)lo;
    }
};
// ActAll (lookahead_kernel, ssa_lookahead_f64): EVERY row is "selected" -- the update's covariance of every object as if the action
// had chosen it (P+ = P- - K S K^T does not depend on the measured value), nothing committed.  The update block then runs Phase 1 in
// all four rows at once and Phase 2 in four turns; the outputs go to `o` at the caller's rows, the measurement noise is never read,
// and no history slot, status word, failure record, update record or statistics word is written.
struct ActAll : ActBase {
    static constexpr bool all = true;
    const ssa_lookahead_out* o;
};
// ActSensors (step_sensors_kernel, ssa_env_step_sensors_f64; one env): up to SSA_MAX_SENSORS sites each select one object.  A row is
// selected if any sensor's action is its caller index; it then carries the lowest such sensor's index, and the update block reads that
// sensor's site, elevation mask, R, noise table and record slot instead of ssa_consts' / ssa_step_params'.  `s` points at the kernel's
// argument block: the actions and the geometry are wave-uniform (scalar) loads.
struct ActSensors : ActBase {
    static constexpr bool sensors = true;
    const ssa_sensor_params* s;
    SSA_DEV const ssa_sensor_params* sites() const { return s; }
    // the sensors' actions (all of them: indexable; one of them) and the records' base, through the pointer process_wave holds the sites by
    SSA_DEV const int32_t* actions(const ssa_sensor_params* sp) const { return sp->action; }
    SSA_DEV int action(const ssa_sensor_params* sp, int k) const { return sp->action[k]; }
    SSA_DEV double* records(const ssa_sensor_params* sp) const { return sp->upd; }
};
// ActSchedule (rollout_sensors_kernel, ssa_env_rollout_sensors_f64; one env): ActSensors for the steps of a rollout, where the sensors'
// actions and the records' destination change with every step while the sites do not.  `s` points at the kernel's argument block as
// ActSensors' does (its action words and record pointer are not read); `row` is the step's row of the schedule in device memory --
// SSA_MAX_SENSORS words, 32-byte aligned, read-only for the launch: one wave-uniform scalar load of eight words whatever S is; `upd` is
// the step's record slot, null for a step that does not end up owning it.
struct ActSchedule : ActBase {
    static constexpr bool sensors = true;
    const ssa_sensor_params* s;
    const int32_t* row;
    double* upd;
    SSA_DEV const ssa_sensor_params* sites() const { return s; }
    typedef int row_t __attribute__((ext_vector_type(SSA_MAX_SENSORS)));
    typedef const __attribute__((address_space(4))) int32_t* WordPtr;   // (constant for the launch: the scalar cache may serve it)
    SSA_DEV row_t actions(const ssa_sensor_params*) const
    {
        typedef const __attribute__((address_space(4))) row_t* RowPtr;
        return *(RowPtr)__builtin_assume_aligned(row, sizeof(row_t));
    }
    SSA_DEV int action(const ssa_sensor_params*, int k) const { return ((WordPtr)row)[k]; }   // (k not known at compile time: one word)
    SSA_DEV double* records(const ssa_sensor_params*) const { return upd; }
};
// ActSensorEnvs (vector_sensors_kernel, ssa_env_step_sensors_envs_f64): ActSensors in each of E envs.  The sites are shared; an env has
// its own row of SSA_MAX_SENSORS action words, its own block of S update records, its own time word and its own noise tables.  Several
// envs come in whole tiles (n_obj % 4 == 0: the launcher), so a tile's env is wave-uniform -- enter() forms it once per tile, as a scalar --
// and the env's row is what a schedule's row is to ActSchedule: one scalar load of eight words through the constant address space, from
// device memory (`actions`, 32-byte aligned) or, with SSA_LAUNCH_INLINE_ENVS, from the kernel's own argument block (`inline_action`).
// Three things of process_wave's `sensors` path take the env's value, each behind `envs`: the time word, the row that clears the idle
// sensors' records (the env's first) with the records' base, and the caller's index of a row (its index within the env).
SSA_DEV ConstPtr<int32_t> vector_sensors_inline_rows();   // (inline_action in the argument segment: defined behind VecSensK)
struct ActSensorEnvs : ActBase {
    static constexpr bool sensors = true, envs = true;
    const ssa_sensor_params* s;
    const ssa_sensor_envs_params* v;   // (in the kernel's argument block, as `s`)
    int env;                           // the tile's env
    ConstPtr<int32_t> row;             // ... its action words
    double* upd;                       // ... its records, or null
    SSA_DEV const ssa_sensor_params* sites() const { return s; }
    SSA_DEV void enter(uint32_t mask, int n_env, int64_t n_obj, int64_t base)
    {
        env = (n_env > 1) ? __builtin_amdgcn_readfirstlane((int)((uint32_t)base / (uint32_t)n_obj)) : 0;
        const ConstPtr<int32_t> rows = (mask & SSA_LAUNCH_INLINE_ENVS) ? vector_sensors_inline_rows() : (ConstPtr<int32_t>)v->actions;
        row = rows + (int64_t)env * SSA_MAX_SENSORS;
        upd = v->upd ? v->upd + (int64_t)env * s->n_sensor * SSA_UPD_STRIDE : nullptr;
    }
    typedef int row_t __attribute__((ext_vector_type(SSA_MAX_SENSORS)));
    SSA_DEV row_t actions(const ssa_sensor_params*) const { return *(ConstPtr<row_t>)__builtin_assume_aligned(row, sizeof(row_t)); }
    SSA_DEV int action(const ssa_sensor_params*, int k) const { return row[k]; }
    SSA_DEV double* records(const ssa_sensor_params*) const { return upd; }
};
// ActScheduleEnvs (rollout_sensor_envs_kernel, ssa_env_rollout_sensors_envs_f64): ActSchedule in each of E envs, as ActSensorEnvs is
// ActSensors in each of them -- step kk of a schedule on a resident tile whose env is a scalar.  enter() forms the tile's env once per
// tile and step; row (kk, env) of the schedule is one scalar load of eight words through the constant address space, and the records
// of (kk, env) are a block of their own: every step owns its block, so every step writes it.  What `sensors` and `envs` put into
// process_wave holds for it unchanged; the time word comes from memory (a resident tile's steps do not see SSA_LAUNCH_INLINE_ENVS).
struct ActScheduleEnvs : ActBase {
    static constexpr bool sensors = true, envs = true;
    const ssa_sensor_params* s;
    const ssa_rollout_sensors_envs_params* v;   // (in the kernel's argument block, as `s`)
    int kk;                            // the step
    int env;                           // the tile's env
    ConstPtr<int32_t> row;             // ... its action words at step kk
    double* upd;                       // ... its records of step kk, or null
    SSA_DEV const ssa_sensor_params* sites() const { return s; }
    SSA_DEV void enter(uint32_t, int n_env, int64_t n_obj, int64_t base)
    {
        env = (n_env > 1) ? __builtin_amdgcn_readfirstlane((int)((uint32_t)base / (uint32_t)n_obj)) : 0;
        const int64_t ke = (int64_t)kk * n_env + env;
        row = (ConstPtr<int32_t>)v->actions + ke * SSA_MAX_SENSORS;
        upd = v->upd_out ? v->upd_out + ke * s->n_sensor * SSA_UPD_STRIDE : nullptr;
    }
    typedef int row_t __attribute__((ext_vector_type(SSA_MAX_SENSORS)));
    SSA_DEV row_t actions(const ssa_sensor_params*) const { return *(ConstPtr<row_t>)__builtin_assume_aligned(row, sizeof(row_t)); }
    SSA_DEV int action(const ssa_sensor_params*, int k) const { return row[k]; }
    SSA_DEV double* records(const ssa_sensor_params*) const { return upd; }
};
// ActDryRunEnvs (dryrun_sensors_kernel, ssa_dryrun_sensors_envs_f64): ActScheduleEnvs as a dry run -- step kk of a candidate schedule on
// a resident tile whose (pseudo-)env is a scalar, read-only like the forecast's.  The `sensors` / `envs` paths of process_wave hold for it
// (the row's sensor, its site, visibility, S, the inverse, K); behind `dryrun` the update commits P+ = P- - K S K^T alone (the `all`
// path's arithmetic, through the row's consumed staging matrix, so that P- is still there for the scores), x stays the predict's, the
// noise is not fetched, a failed row follows the forecast's rule (no ring to re-read), and the one output is the slot's record.
// records() is null: nothing of the sensor step's update record is written.  An action >= n_obj_caller is idle whatever n_obj is (a
// gathered block's n_obj is not the catalogue's size): the row's words are filtered as they are read.
struct ActDryRunEnvs : ActBase {
    static constexpr bool sensors = true, envs = true, dryrun = true;
    const ssa_sensor_params* s;
    const ssa_dryrun_sensors_params* v;   // (in the kernel's argument block, as `s`)
    int kk;                            // the step
    int env;                           // the tile's env
    ConstPtr<int32_t> row;             // ... its action words at step kk
    double* out;                       // ... its records of step kk
    int lim;                           // n_obj_caller
    SSA_DEV const ssa_sensor_params* sites() const { return s; }
    SSA_DEV void enter(uint32_t, int n_env, int64_t n_obj, int64_t base)
    {
        env = (n_env > 1) ? __builtin_amdgcn_readfirstlane((int)((uint32_t)base / (uint32_t)n_obj)) : 0;
        const int64_t ke = (int64_t)kk * n_env + env;
        row = (ConstPtr<int32_t>)v->actions + ke * SSA_MAX_SENSORS;
        out = v->out + ke * s->n_sensor * SSA_DRY_STRIDE;
        lim = v->n_obj_caller;
    }
    typedef int row_t __attribute__((ext_vector_type(SSA_MAX_SENSORS)));
    SSA_DEV row_t actions(const ssa_sensor_params*) const
    {
        row_t r = *(ConstPtr<row_t>)__builtin_assume_aligned(row, sizeof(row_t));
#pragma unroll
        for (int k = 0; k < SSA_MAX_SENSORS; ++k) r[k] = r[k] < lim ? r[k] : -1;
        return r;
    }
    SSA_DEV int action(const ssa_sensor_params*, int k) const { return row[k] < lim ? row[k] : -1; }
    SSA_DEV double* records(const ssa_sensor_params*) const { return nullptr; }
    SSA_DEV double* record(int sid) const { return out + (int64_t)sid * SSA_DRY_STRIDE; }
};
// the sensor that updates the object the caller calls `jid`: the lowest-numbered one whose action it is, -1 for none
template <class ACT>
SSA_DEV int sensor_index(const ACT& a, const ssa_sensor_params* s, int64_t jid)
{
    int sid = -1;
    const auto act = a.actions(s);
#pragma unroll
    for (int k = SSA_MAX_SENSORS - 1; k >= 0; --k)
        if (k < s->n_sensor && act[k] >= 0 && (int64_t)act[k] == jid) sid = k;
    return sid;
}
// ActLookSensors (lookahead_sensors_kernel, ssa_lookahead_sensors_f64; one env): ActAll for every sensor of a network.  The predict
// runs once; the update block and the outputs then run once per sensor (a pass), from that sensor's site with its elevation mask and R
// -- wave-uniform: scalar loads of the argument block, no waterfall.  Sensor s's outputs go to row s * n_obj + the caller's index; the
// prior (x_prior / P_prior) is written by the first pass only.
struct ActLookSensors : ActBase {
    static constexpr bool all = true, look_sensors = true;
    const ssa_lookahead_out* o;
    const ssa_sensor_params* s;
    SSA_DEV const ssa_sensor_params* sites() const { return s; }
};
// ActForecastSensors (forecast_sensors_kernel, ssa_forecast_sensors_f64; one env): ActLookSensors for step h of a forecast, whose tile
// stays in LDS from step to step with every sensor idle.  Three things differ from the one-step lookahead, each behind `forecast`
// in process_wave: the outputs go to slab h of the blocks `o` names (slab()); the status the tile carries to step h + 1 is the
// predict's (a singular S of a hypothetical update shows in that step's outputs only); and a row that failed INSIDE the horizon is
// handed on as the failure sentinels -- there is no ring slot to re-read, and the input slot holds its healthy state.
struct ActForecastSensors : ActBase {
    static constexpr bool all = true, look_sensors = true, forecast = true;
    const ssa_lookahead_out* o;
    const ssa_sensor_params* s;
    int h;
    SSA_DEV const ssa_sensor_params* sites() const { return s; }
    // the output block of step h: [H][S * m] rows per sensor output, [H][m] rows of the prior
    SSA_DEV void slab(ssa_lookahead_out& os, int64_t m, int S) const
    {
        const int64_t rs = (int64_t)h * S * m, rp = (int64_t)h * m;
        os.score += rs * SSA_LOOK_NSCORE;
        os.status += rs;
        os.visible += rs;
        if (os.P_post) os.P_post += rs * 36;
        if (os.x_prior) os.x_prior += rp * 6;
        if (os.P_prior) os.P_prior += rp * 36;
    }
};
// ActLookSensorEnvs (lookahead_sensor_envs_kernel, ssa_lookahead_sensors_envs_f64): ActLookSensors in each of E envs, as ActSensorEnvs
// is ActSensors in each of them.  The sites are shared; several envs come in whole tiles (n_obj % 4 == 0: the launcher), so a tile's env
// is wave-uniform -- enter() forms it once per tile, as a scalar -- and its time word is a scalar load indexed by it.  Two things of
// process_wave's `look_sensors` path take the env's value, each behind `look_envs`: the time word, and in every pass the env's slab of
// the blocks `o` names (slab()) with the caller's index of a row (its index within the env).
struct ActLookSensorEnvs : ActBase {
    static constexpr bool all = true, look_sensors = true, look_envs = true;
    const ssa_lookahead_out* o;
    const ssa_sensor_params* s;
    int env;                           // the tile's env
    SSA_DEV const ssa_sensor_params* sites() const { return s; }
    SSA_DEV void enter(int n_env, int64_t n_obj, int64_t base)
    {
        env = (n_env > 1) ? __builtin_amdgcn_readfirstlane((int)((uint32_t)base / (uint32_t)n_obj)) : 0;
    }
    // the env's output block: [E][S * m] rows per sensor output, [E][m] rows of the prior
    SSA_DEV void slab(ssa_lookahead_out& os, int64_t m, int S) const
    {
        const int64_t rs = (int64_t)env * S * m, rp = (int64_t)env * m;
        os.score += rs * SSA_LOOK_NSCORE;
        os.status += rs;
        os.visible += rs;
        if (os.P_post) os.P_post += rs * 36;
        if (os.x_prior) os.x_prior += rp * 6;
        if (os.P_prior) os.P_prior += rp * 36;
    }
};
// ActForecastSensorEnvs (forecast_sensor_envs_kernel, ssa_forecast_sensors_envs_f64): ActForecastSensors in each of E envs -- both of
// the above at once: step h of a forecast on a resident tile whose env is a scalar.  What `forecast` and `look_envs` each put into
// process_wave holds for it unchanged (the status carried to h + 1, the pass-through against the sentinels by the storage row's own
// status word, the row's index within its env); what the two would do twice is done once: slab() offsets every block to step h, then
// env e -- rows ((h E + e) S + s) m + j per sensor output, (h E + e) m + j of the prior, so that slab h of the scores is one
// contiguous [E][S][m][3] block, what ssa_assign_sensors_envs_f64 takes.  The env's time word is a scalar load indexed by the env, from
// device memory or -- SSA_LAUNCH_INLINE_ENVS -- from the kernel's own argument block (time_word()).
SSA_DEV ConstPtr<int32_t> forecast_envs_inline_time();   // (inline_time in the argument segment: defined behind VecForeSensK)
struct ActForecastSensorEnvs : ActBase {
    static constexpr bool all = true, look_sensors = true, forecast = true, look_envs = true;
    const ssa_lookahead_out* o;
    const ssa_sensor_params* s;
    int h;
    int n_env;                         // E of the launch (the slab's stride)
    int env;                           // the tile's env
    SSA_DEV const ssa_sensor_params* sites() const { return s; }
    SSA_DEV void enter(int n_env_, int64_t n_obj, int64_t base)
    {
        env = (n_env_ > 1) ? __builtin_amdgcn_readfirstlane((int)((uint32_t)base / (uint32_t)n_obj)) : 0;
    }
    SSA_DEV int time_word(uint32_t mask, const int32_t* mem) const
    {
        const ConstPtr<int32_t> src = (mask & SSA_LAUNCH_INLINE_ENVS) ? forecast_envs_inline_time() : (ConstPtr<int32_t>)mem;
        return src[env];
    }
    // the output block of step h and env e: [H][E][S * m] rows per sensor output, [H][E][m] rows of the prior
    SSA_DEV void slab(ssa_lookahead_out& os, int64_t m, int S) const
    {
        const int64_t he = (int64_t)h * n_env + env;
        const int64_t rs = he * S * m, rp = he * m;
        os.score += rs * SSA_LOOK_NSCORE;
        os.status += rs;
        os.visible += rs;
        if (os.P_post) os.P_post += rs * 36;
        if (os.x_prior) os.x_prior += rp * 6;
        if (os.P_prior) os.P_prior += rp * 36;
    }
};
// a pointer into the argument segment that the optimiser cannot see through: the (scalar) loads from it stay inside ActLookSensors'
// passes instead of being hoisted in front of them, where their results would hold scalar registers across every pass
template <class T> SSA_DEV const T* kernarg_opaque(const T* q)
{
    typedef const __attribute__((address_space(4))) T* KP;
    KP k = (KP)q;
    asm volatile("" : "+s"(k));
    return (const T*)k;
}
SSA_DEV double logdet_chol(const double (&A)[21]);   // (defined with the agents' scores)
// where entry idx of P+ lies in a row's staging matrix ([13][9]): PPL 0 (ActAll) -- the first 36 slots; PPL 1 (ActLookSensors) -- the
// right halves (the residual columns) of its first 12 rows, so that the left halves survive the pass
template <int PPL> SSA_DEV int pp_at(int idx) { return PPL == 0 ? idx : (idx / 3) * 9 + 6 + idx % 3; }
// the lookahead's outputs of row g (lane l of it) at the caller's row `orow`.  P- / x- are the tile after the predict and the
// failure sentinels (what a step leaves for an object it does not update); P+ (row g's turn of Phase 2, left in t.UA[g * 117 ...] as
// pp_at<PPL> places it) where the update ran, the sentinel where S was singular, P- otherwise.  The scores: one lane per object, log-dets
// by logdet_chol.
template <int PPL = 0>
SSA_DEV void lookahead_store(const Tiles& t, const ssa_lookahead_out& o, int g, int l, int64_t orow, int st, bool vis, bool taken)
{
    const double* Pm = &t.P[g * 36];
    const double* Pp = &t.UA[g * 117];
    const bool lin = st == SSA_ST_UPDATE_LINALG;
    for (int idx = l; idx < 36; idx += 16) {
        const int a = idx / 6, b = idx - 6 * a;
        const double pm = Pm[idx];
        const double pp = taken ? Pp[pp_at<PPL>(idx)] : (lin ? ((a == b) ? (a < 3 ? X_FAILED_POS : X_FAILED_VEL) : 0.0) : pm);
        if (o.P_prior) o.P_prior[orow * 36 + idx] = pm;
        if (o.P_post) o.P_post[orow * 36 + idx] = pp;
    }
    if (o.x_prior && l < 6) o.x_prior[orow * 6 + l] = t.X[g * 6 + l];
    // the two log-dets in two lanes of the row (lane 0: P-, lane 1: P+): one factorisation's registers at a time
    double ld = 0.0;
    if (taken && l < 2) {   // (status OK and visible: exactly the rows whose update ran)
        const double* src = (l == 0) ? Pm : Pp;
        double A[21];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) A[tri(r, c)] = (PPL == 0 || l == 0) ? src[r * 6 + c] : src[pp_at<PPL>(r * 6 + c)];
        ld = logdet_chol(A);
    }
    const double ld_post = __shfl_down(ld, 1, 64);
    if (l == 0) {
        const double nan = __builtin_nan("");
        double sc[SSA_LOOK_NSCORE] = {nan, nan, nan};
        if (taken) {
            double trm = 0.0, trp = 0.0, pos_m = 0.0, pos_p = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                trm += Pm[7 * r];
                trp += Pp[pp_at<PPL>(7 * r)];
                if (r == 2) { pos_m = trm; pos_p = trp; }
            }
            sc[SSA_LOOK_TRACE_GAIN] = trm - trp;
            sc[SSA_LOOK_POS_TRACE_GAIN] = pos_m - pos_p;
            sc[SSA_LOOK_INFO_GAIN] = 0.5 * (ld - ld_post);
        }
#pragma unroll
        for (int k = 0; k < SSA_LOOK_NSCORE; ++k) o.score[orow * SSA_LOOK_NSCORE + k] = sc[k];
        o.status[orow] = st;
        o.visible[orow] = vis ? 1 : 0;
    }
}

// the dry run's record of a tasked row g (lane l of it): the slot's action, visibility, outcome and status, and the lookahead's three
// scores from P- (the tile) and P+ (the first 36 slots of the row's staging matrix, pp_at<0>) -- lookahead_store's arithmetic, line by line
SSA_DEV void dryrun_store(const Tiles& t, double* rec, int g, int l, double action, int st, bool vis, bool taken)
{
    const double* Pm = &t.P[g * 36];
    const double* Pp = &t.UA[g * 117];
    double ld = 0.0;
    if (taken && l < 2) {
        const double* src = (l == 0) ? Pm : Pp;
        double A[21];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) A[tri(r, c)] = src[r * 6 + c];
        ld = logdet_chol(A);
    }
    const double ld_post = __shfl_down(ld, 1, 64);
    if (l == 0) {
        const double nan = __builtin_nan("");
        double sc[SSA_LOOK_NSCORE] = {nan, nan, nan};
        if (taken) {
            double trm = 0.0, trp = 0.0, pos_m = 0.0, pos_p = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                trm += Pm[7 * r];
                trp += Pp[7 * r];
                if (r == 2) { pos_m = trm; pos_p = trp; }
            }
            sc[SSA_LOOK_TRACE_GAIN] = trm - trp;
            sc[SSA_LOOK_POS_TRACE_GAIN] = pos_m - pos_p;
            sc[SSA_LOOK_INFO_GAIN] = 0.5 * (ld - ld_post);
        }
        rec[SSA_DRY_ACTION] = action;
        rec[SSA_DRY_VISIBLE] = vis ? 1.0 : 0.0;
        rec[SSA_DRY_TAKEN] = taken ? 1.0 : 0.0;
        rec[SSA_DRY_STATUS] = (double)st;
#pragma unroll
        for (int k = 0; k < SSA_LOOK_NSCORE; ++k) rec[SSA_DRY_SCORE + k] = sc[k];
        rec[SSA_DRY_SPARE] = 0.0;
    }
}

// ---- The store stage of a WHOLE tile in the plain form (step_plain_kernel, ActPlain): what store_tile's whole-tile block writes, word for
// word, scheduled for a wavefront whose life is bound by dependent round trips.
//   plain_dst_fetch: what the compiler does not keep from the head -- the destinations status, obs, metrics and the metrics' row stride
//     n_obj -- in ONE batch of scalar loads from the argument segment, issued in front of the metrics' arithmetic and waited for once,
//     behind it.  As asm statements: a plain load of an argument word is sunk to its use, which puts a scalar round trip in front of each
//     store group.  The pointers are typed as global ones -- through an asm statement an untyped pointer is generic and its stores go
//     through the FLAT segment.  The caller issues the batch on the path that waits for it ONLY: the compiler takes an asm statement's
//     results for written when it has run, and would hand their registers out again while the loads are still in flight.
//   plain_tile_out: the metrics and the status word leave from the lanes that computed them (no t.Met / t.St round trip).  Then every lane
//     issues ALL its LDS reads -- P main (16 B), one 16-byte piece by lane range (the tail of P | x | x_true), the observation pair --
//     before the first store, and the stores follow behind counted waits (the DS unit returns a wavefront's reads in issue order).
//     Every store is (scalar base) + (unsigned 32-bit lane offset): one shared offset register, lane x 16, for P / x / x_true, whose bases
//     are moved back by the group's first lane on the scalar unit.  The observation rows [x, diag P] of object g leave from lanes 8..13
//     of row g (no division: the row IS the object), entries [2 k, 2 k + 2) from lane 8 + k.  n_obj: one tile per wavefront bounds it by
//     80 x the CU count (tile_grid), far below 2^24, so lane x n_obj is a 24-bit multiply and every byte offset fits 32 bits.
typedef __attribute__((address_space(1))) char* GlobalBytes;
struct PlainDst {
    __attribute__((address_space(1))) int32_t* status;
    __attribute__((address_space(1))) double *obs, *metrics;
    uint32_t n_obj;   // (the low word: see above)
};
SSA_DEV void plain_dst_fetch(PlainDst& d)
{
    const ConstPtr<ssa_step_params> kp = tile_kernel_params();
    asm volatile("s_load_dwordx2 %0, %4, %5\n\ts_load_dwordx2 %1, %4, %6\n\ts_load_dwordx2 %2, %4, %7\n\ts_load_dword %3, %4, %8"
                 : "=&s"(d.status), "=&s"(d.obs), "=&s"(d.metrics), "=&s"(d.n_obj)
                 : "s"(kp), "i"(offsetof(ssa_step_params, status)), "i"(offsetof(ssa_step_params, obs)), "i"(offsetof(ssa_step_params, metrics)),
                   "i"(offsetof(ssa_step_params, n_obj)));
}
// a store base the compiler cannot see into: it would peel the constant part off again and add it behind a per-lane 64-bit sum
SSA_DEV GlobalBytes opaque_base(GlobalBytes b)
{
    asm volatile("" : "+s"(b));
    return b;
}
template <bool NT>
SSA_DEV void store16_at(GlobalBytes sbase, uint32_t off, v2d v)
{
    // (the offset is made the masked region's own value: shared between regions its zero-extension is hoisted out of them, and the
    // store, which then sees a 64-bit register pair, adds the base per lane)
    asm volatile("" : "+v"(off));
    __attribute__((address_space(1))) v2d* dst = (__attribute__((address_space(1))) v2d*)(sbase + (uint64_t)off);
    if (NT) __builtin_nontemporal_store(v, dst);
    else *dst = v;
}
template <bool NT>
SSA_DEV void plain_tile_out(Tiles& t, const ssa_step_params& p, PlainDst d, int lane, int64_t base, double met, int st_new)
{
    const uint32_t g = (uint32_t)lane >> 4, l = (uint32_t)lane & 15u;
    // the destinations have arrived (the one wait for the scalar batch, in front of the stage's first LDS read)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(d.status), "+s"(d.obs), "+s"(d.metrics), "+s"(d.n_obj)::"memory");
    if (l < 4u) *(__attribute__((address_space(1))) double*)((GlobalBytes)(d.metrics + base) + (uint64_t)((__umul24(l, d.n_obj) + g) << 3)) = met;
    if (l == 0u) *(__attribute__((address_space(1))) int32_t*)((GlobalBytes)(d.status + base) + (uint64_t)(g << 2)) = st_new;
    // the batch: four reads per lane, every address inside the tiles whatever the lane (a lane outside a group reads words it does not store)
    const uint32_t t0 = (uint32_t)(uintptr_t)(LdsVoidPtr)&t;
    const uint32_t off16 = (uint32_t)lane << 4;
    const uint32_t a_main = t0 + (uint32_t)offsetof(Tiles, P) + off16;
    const uint32_t a_aux = a_main + (lane < 8 ? 1024u : lane < 20 ? (uint32_t)offsetof(Tiles, X) - 8u * 16u : (uint32_t)offsetof(Tiles, T) - 20u * 16u);
    // lanes 8..13 of a row, k = l - 8: its object's observation entries [2 k, 2 k + 2) -- x[2 k], x[2 k + 1] (k < 3) | P[2 k - 6][2 k - 6] and the
    // next diagonal entry: g x (row bytes) + l x (step) + (origin - 8 steps), the three constants selected by the half (24-bit multiply-adds)
    const uint32_t k = l - 8u;
    const bool ox = l < 11u;
    const uint32_t a_o0 = t0 + __umul24(g, ox ? 48u : 288u) + __umul24(l, ox ? 16u : 112u) +
                          (ox ? (uint32_t)offsetof(Tiles, X) - 8u * 16u : (uint32_t)offsetof(Tiles, P) - 11u * 112u);
    const uint32_t a_o1 = a_o0 + (ox ? 8u : 56u);
    v2d m, a;
    double o0, o1;
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b64 %2, %6\n\tds_read_b64 %3, %7"
                 : "=&v"(m), "=&v"(a), "=&v"(o0), "=&v"(o1)
                 : "v"(a_main), "v"(a_aux), "v"(a_o0), "v"(a_o1)
                 : "memory");
    const GlobalBytes Pb = (GlobalBytes)((__attribute__((address_space(1))) double*)p.P_out + base * 36);
    const GlobalBytes Pt = opaque_base(Pb + 1024);
    const GlobalBytes xb = opaque_base((GlobalBytes)((__attribute__((address_space(1))) double*)p.x_out + base * 6) - 8 * 16);
    const GlobalBytes tb = opaque_base((GlobalBytes)((__attribute__((address_space(1))) double*)p.x_true_out + base * 6) - 20 * 16);
    asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(m)::"memory");
    store16_at<NT>(Pb, off16, m);
    asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(a)::"memory");
    if (lane < 8) store16_at<NT>(Pt, off16, a);
    if ((unsigned)(lane - 8) < 12u) store16_at<NT>(xb, off16, a);
    if ((unsigned)(lane - 20) < 12u) store16_at<NT>(tb, off16, a);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(o0), "+v"(o1)::"memory");
    if (k < 6u) store16_at<NT>((GlobalBytes)(d.obs + base * 12), __umul24(g, 96u) + (k << 4), v2d{o0, o1});
}

template <int PROP, int TILE, class ACT>
SSA_DEV void process_wave(Tiles& t, const ssa_consts& C, const ssa_step_params& p, int lane, int64_t obj_in, bool valid,
                          int64_t base, int cnt, TileRegs& pf, int64_t next_base, int next_cnt, int tile, ACT& asrc)
{
    constexpr bool INL = (TILE != 2) && !ACT::late;   // (the per-step launches: SSA_LAUNCH_INLINE_ENVS may be set)
    constexpr bool SEG = (TILE == 0);                 // (`p` is the kernel's own argument block: env_action)
    // SSA_LAUNCH_FOLD_INSIDE exists in the one-tile instance only: counting a tile means waiting for its atomics' acknowledgement
    // and for a returning atomic -- once, at the end of a one-tile wavefront's life, but ~1.5 us per tile in the grid-stride
    // instance (8 x 20 000 objects: 100.7 us per step instead of 89.0); the launcher sends those launches a fold kernel instead.
    // (Round 4 tried counting once per WAVEFRONT, at the end of its life -- lane i counts the walk's i-th tile, one round trip:
    // profiles/r04_vec_env_breakdown.txt.  Correct, and slower than the 4.3 us fold kernel it replaces: the wavefronts of
    // a grid-stride launch end together, and the 128 shard-complete increments per env land on ONE word one after the other -- the vector
    // env's step 123.9 -> 130.4 us although its host side got 4 us shorter.)
    constexpr bool FOLD_OK = (TILE == 0);
    // SSA_LAUNCH_STATS_FROM_METRICS: the one-tile step kernel only (the launcher refuses it everywhere else)
    constexpr bool FROM_METRICS = (TILE == 0) && !ACT::late && !ACT::all && !ACT::sensors && !ACT::look_sensors;
    constexpr bool ALL = ACT::all;   // the lookahead: every row updated hypothetically, nothing committed (ActAll)
    constexpr bool SENS = ACT::sensors;   // a sensor network: one update per sensor, each with its own site (ActSensors)
    constexpr bool LSENS = ACT::look_sensors;   // the lookahead of a sensor network: ALL, one pass per sensor (ActLookSensors)
    constexpr bool FCAST = ACT::forecast;      // ... as step h of a forecast: LSENS on a resident tile (ActForecastSensors)
    constexpr bool ENVS = ACT::envs;           // SENS in each of several envs, whole tiles per env (ActSensorEnvs)
    constexpr bool LENVS = ACT::look_envs;     // LSENS in each of several envs, whole tiles per env (ActLookSensorEnvs)
    constexpr bool PLAIN = ACT::plain;         // the launcher's plain form (ActPlain): the decisions below marked PLAIN are constants
    constexpr bool DRY = ACT::dryrun;          // SENS + ENVS as a dry run on a resident tile: P+ alone committed, records only (ActDryRunEnvs)
    static_assert(!DRY || (SENS && ENVS && TILE == 2), "ActDryRunEnvs: a resident tile's sensor step in several envs");
    static_assert(!PLAIN || (!ACT::late && !ALL && !SENS && !LSENS), "ActPlain: a step kernel's form");   // (and launched as the one-tile instance only)
#define SSA_NENV (PLAIN ? 1 : p.n_env)   /* (at the place of use: every other instance reads the word where it did) */
    // (ActLookSensors, multi-tile instance: the next tile's loads leave once, behind the last pass -- except with SSA_PROP_ELEMENTS, whose
    // out-of-line call then spills 8 more VGPRs: there they are issued as in every other kernel, after the propagator and again at the end
    // of each pass's update)
    constexpr bool ISSUE_LAST = LSENS && PROP != 0;
    // (ActLookSensors: the sites' and the outputs' pointers through kernarg_opaque in every pass -- but in that same SSA_PROP_ELEMENTS
    // instance, which re-derives its argument block per tile anyway and spills across the tile loop with it)
    constexpr bool PASS_ARGS = LSENS && !(TILE == 1 && PROP == 0);
    int g = lane >> 4, l = lane & 15;
    int64_t obj = obj_in;
    // (TILE 0: the kernel issued the tile's loads from its preloaded pointer arguments, whole tile or not decided from them too, before
    // any scalar load.)  Everything else the head needs from memory is requested HERE, behind them and in front of the one wait for the
    // tile: the process noise (a per-lane load from the argument segment, committed to LDS behind that wait -- placed there it was a
    // dependent vector-memory round trip of its own), then the scalar loads of the action / time words and of the tile's obj_ids.
    double q_in = 0.0;
    if (TILE == 0 && lane < 36) q_in = C.Q[lane];
    // ... and ONE round trip to the argument segment for every scalar the head decides by: held through an empty asm statement as
    // in/out operands, so that the selects and loads below start from registers (the value used is the statement's result, which the
    // compiler cannot get by loading the word again) -- left to itself the compiler loads launch_mask, branches on it, loads the pointer
    // the branch picked, then the word: four scalar round trips in a row.
    struct { uint32_t mask; const int32_t *actions, *env_time, *obj_ids; int n_env, time_offset, update_interval; } hw =
        {PLAIN ? (SSA_LAUNCH_DEFER_FOLD | SSA_LAUNCH_STATS_FROM_METRICS) : p.launch_mask, p.actions, p.env_time, p.obj_ids, SSA_NENV,
         p.time_offset, PLAIN ? 1 : C.update_interval};
    if constexpr (PLAIN) {   // (the mask, the env count and the interval are not fetched: known)
        asm volatile("" : "+s"(hw.actions), "+s"(hw.env_time), "+s"(hw.obj_ids), "+s"(hw.time_offset)
                     : "s"(p.P_out), "s"(p.x_out), "s"(p.x_true_out), "s"(p.obs), "s"(p.metrics), "s"(p.stat_shards), "s"(p.upd), "s"(p.n_obj));
    } else if (TILE == 0 && !ALL) {
        // the epilogue's output pointers are fetched NOW as well: their scalar loads (kernarg segment) overlap the tile's HBM round
        // trip instead of each adding a scalar-memory round trip to the store path of a latency-bound wavefront.  (As inputs only: the
        // compiler is free to drop them again, and does so with p.obs and p.metrics -- the store stage loads those a second time.)
        asm volatile("" : "+s"(hw.mask), "+s"(hw.actions), "+s"(hw.env_time), "+s"(hw.obj_ids), "+s"(hw.n_env), "+s"(hw.time_offset),
                          "+s"(hw.update_interval)
                     : "s"(p.P_out), "s"(p.x_out), "s"(p.x_true_out), "s"(p.obs), "s"(p.metrics), "s"(p.stat_shards), "s"(p.upd), "s"(p.aer_out),
                       "s"(p.n_obj));
    } else if (TILE == 0) {
        asm volatile("" : "+s"(hw.mask), "+s"(hw.env_time), "+s"(hw.obj_ids), "+s"(hw.n_env), "+s"(hw.time_offset), "+s"(hw.update_interval));
    }

    if constexpr (ENVS) asrc.enter(hw.mask, hw.n_env, p.n_obj, base);   // (the tile's env, a scalar: its action row, records and time word)
    // env of the object: no division for the single-env case, a 32-bit one otherwise (n_env * n_obj < 2^31)
    int e = (valid && hw.n_env > 1) ? (int)((uint32_t)obj / (uint32_t)p.n_obj) : 0;
    if constexpr (ENVS) e = asrc.env;   // (whole tiles per env: no division per lane)
    if constexpr (LENVS) {              // (the same for a network's lookahead: the tile's env, a scalar)
        asrc.enter(hw.n_env, p.n_obj, base);
        e = asrc.env;
    }
    const int64_t j = valid ? obj - (int64_t)e * p.n_obj : 0;
    // the action / time index of this object's env, fetched early (used after the transform)
    // (one env: wave-uniform loads -- scalar ones from the constant address space in the one-tile instances, see env_action; the
    // grid-stride instance's still compile to loads through the FLAT segment --; per-lane loads with their 64-bit address arithmetic only
    // for vectorised envs)
    int act, tix;
    int id0 = 0, id1 = 0, id2 = 0, id3 = 0;   // (the one-tile instances: the tile's obj_ids)
    if (ACT::late) {   // (one env; the action arrives behind the predict)
        act = -1;
        tix = valid ? p.env_time[0] + p.time_offset : 0;
    } else if (SEG) {   // (the one-tile instances: no action for the lookahead, where every row is selected, nor for a sensor network)
        // env 0's words and the tile's obj_ids: three scalar loads, issued together and waited for once (the asm statement needs all of them)
        const ConstPtr<int32_t> t_src = segment_word_src<true>(hw.mask, hw.env_time), a_src = segment_word_src<false>(hw.mask, hw.actions);
        int t0 = *t_src, a0 = -1;
        if constexpr (ENVS) t0 = t_src[asrc.env];   // (the tile's env: still a scalar load)
        if constexpr (LENVS) t0 = t_src[asrc.env];
        if (!ALL && !SENS) a0 = *a_src;
        if (hw.obj_ids) {
            const v4i w = *(ConstPtr<v4i>)(hw.obj_ids + base);
            id0 = w.x; id1 = w.y; id2 = w.z; id3 = w.w;
        }
        asm volatile("" : "+s"(t0), "+s"(a0), "+s"(id0), "+s"(id1), "+s"(id2), "+s"(id3));
        if (!ENVS && !LENVS && hw.n_env > 1) {
            t0 = segment_lane_word(t_src, e);
            if (!ALL && !SENS) a0 = segment_lane_word(a_src, e);
        }
        act = valid ? a0 : -1;
        tix = valid ? t0 + hw.time_offset : 0;
    } else if (ALL) {   // (no action: every row is selected)
        act = -1;
        if constexpr (FCAST && LENVS) tix = valid ? asrc.time_word(hw.mask, hw.env_time) + p.time_offset : 0;   // (the tile's env: a scalar load)
        else tix = valid ? env_time_of<INL>(p, e) + p.time_offset : 0;
    } else if (SENS) {   // (one env; the sensors' actions are matched below, against the row's caller index)
        act = -1;
        if constexpr (ENVS) tix = valid ? env_time_of<INL>(p, asrc.env) + p.time_offset : 0;
        else tix = valid ? env_time_of<INL>(p, 0) + p.time_offset : 0;
    } else if (p.n_env > 1) {
        act = valid ? env_action<INL>(p, e) : -1;
        tix = valid ? env_time_of<INL>(p, e) + p.time_offset : 0;
    } else {
        const int a0 = env_action<INL>(p, 0), t0 = env_time_of<INL>(p, 0);
        act = valid ? a0 : -1;
        tix = valid ? t0 + p.time_offset : 0;
    }
    // ---- the one update of this env (ssa_tasker_simple_2.py:292-315) runs in the row that owns the selected object.  Its
    // wavefront is the longest-living one of the launch, so its inputs (this step's GCRS->ITRS matrix, the measurement noise)
    // leave HBM now and wait in LDS, instead of costing two memory round trips when the update starts
    const bool interval_ok = (hw.update_interval <= 1) || (tix % hw.update_interval == 0);
    // ssa_step_params.obj_ids (the per-step kernels; per env, indices within the env): the objects are stored in another order than the caller numbers them; the
    // action, the failure records, the arg-max of sigma_pos and the host-facing observation rows speak the CALLER's indices
    int64_t jid = j;
    if (hw.obj_ids) {
        // (the tile's four indices by ONE wave-uniform 16-byte load; the update's input prefetch below hangs on `my_update`; the table is
        // padded to whole tiles.  The one-tile instances read it through the constant address space, which makes it a scalar load next to
        // the action word's: as a plain load the compiler cannot tell that no store of the kernel reaches the table, and issues a vector
        // load that queues behind the tile's.  The rollout / closed-loop instances run behind launches' worth of their own stores: plain.)
        int4 ids;
        if (TILE == 0) ids = make_int4(id0, id1, id2, id3);   // (loaded with the action / time words above)
        else ids = *reinterpret_cast<const int4*>(hw.obj_ids + base);
        const int mine = (g == 0) ? ids.x : (g == 1) ? ids.y : (g == 2) ? ids.z : ids.w;
        jid = valid ? (int64_t)mine : 0;
        if (l == 0) t.Oid[g] = mine;
    }
    int sid = -1;   // (ActSensors: the sensor that updates this row's object, -1 for none)
    if constexpr (SENS) {
        sid = valid ? sensor_index(asrc, asrc.sites(), jid) : -1;
        act = (sid >= 0) ? (int)jid : -1;
    }
    bool my_update = ALL ? (valid && interval_ok) : SENS ? (sid >= 0 && interval_ok)
                                                         : (!ACT::late && valid && act >= 0 && (int64_t)act == jid && interval_ok);
    // (ActLate: every row prefetches for its own object)
    const bool may_update = ACT::late ? (valid && interval_ok) : my_update;
    // ... and it issues ahead of its SIMD's other wavefronts from here on: at equal priority its predict runs at a fifth of the
    // SIMD and the update then starts when everybody else is finishing (the kernel's tail)
    if (!ACT::late && !ALL && __any(my_update)) __builtin_amdgcn_s_setprio(3);
    int tmod = 0;                                           // row of `trans` / `z_noise` (episodes wrap)
    double upd_in = 0.0;
    if (may_update && l < ((ALL || DRY) ? 9 : 12)) {   // (ActAll, a dry run: the matrix only -- the noise slots stay zero, z_noise is never read)
        tmod = time_row(tix, p.n_time);
        const int64_t aobj = ACT::late ? jid : (int64_t)act;   // (the measurement noise is indexed as the caller numbers the objects)
        const double* src = (l < 9) ? p.trans + (int64_t)tmod * 9 + l
                                    : p.z_noise + (int64_t)e * p.zn_stride_env + (int64_t)tmod * p.zn_stride_time + aobj * p.zn_stride_obj + (l - 9);
        if constexpr (SENS) {
            if (l >= 9) src += (int64_t)sid * asrc.sites()->zn_stride_sensor;   // (the sensor's own noise table)
        }
        upd_in = *src;
    }
    // a sensor that sees sunlit objects only (ssa_sensor_params.sunlit_only; the row's sensor, or any of the lookahead's passes): the
    // 32-byte row of the Sun table at the SAME time row travels with the update's inputs, one word in each of the row's idle lanes 12..15
    // -- a network's tile belongs to one env, so the row is the wavefront's and every selected row brings the same four words
    // ... and the word of the moving sensors (ssa_step_params.site_moving), fetched here once and held in a scalar register, so that no
    // pass of a lookahead waits for it behind the predict
    [[maybe_unused]] int32_t moving_bits = 0;
    if constexpr (SENS || LSENS) {
        moving_bits = p.site_moving;
        asm volatile("" : "+s"(moving_bits));
    }
    if constexpr (SENS || LSENS) {
        const int32_t sun_bits = asrc.sites()->sunlit_only;
        if (sun_bits != 0) {   // (wave-uniform: with no bit set nothing is loaded)
            if (may_update && l >= 12 && (LSENS || ((sun_bits >> sid) & 1))) {
                tmod = time_row(tix, p.n_time);
                upd_in = asrc.sites()->sun[(int64_t)tmod * 4 + (l - 12)];   // (lane 15: the dark word's bits, moved as they are)
            }
        }
    }

    if (TILE == 0 && pf.dma) tile_dma_wait(t, pf, lane);   // (the one-tile kernels: the tile came by LDS-DMA)
    else if (TILE != 2) tile_commit(t, pf, lane);        // TILE 1: requested one tile ago (or by the kernel prologue)
    if (lane < 8) t.Z[lane] = 0.0;
    if (TILE == 0) {
        if (lane < 36) t.Q[lane] = q_in;                 // (requested at the top)
    } else if (TILE != 2 && lane < 36) t.Q[lane] = C.Q[lane];   // (a rollout's later steps find it in place)
    wave_lds_sync();

    const int st_in = t.St[g];
    const bool active = valid && st_in == SSA_ST_OK;

    // ---- U1/U2: sigma points
    const int rung = robust_chol_row_lds<PLAIN>(t, C.scale, g, l);   // (PLAIN: the fused form, chol_step_fused)
    asrc.mid_step(t, lane);   // (closed loop: the PREVIOUS step's tile leaves for HBM now, its last reader of t.Obs)
    if (may_update && l < 12) t.Obs[g * 12 + l] = upd_in;
    if constexpr (SENS || LSENS) {   // (the Sun row, where it was fetched: into the gap behind t.X, which nothing else writes)
        const int32_t sun_bits = asrc.sites()->sunlit_only;
        if (sun_bits != 0 && may_update && l >= 12 && (LSENS || ((sun_bits >> sid) & 1))) t.pad1[l - 12] = upd_in;
    }
    wave_lds_sync();
    const bool chol_fail = (rung == 16);
    const bool is_sigma = (l <= 12);
    const bool is_pm = (l >= 1 && l <= 12);
    double s[6];
    {
        const int krow = (l >= 7) ? l - 7 : l - 1;          // factor row of lanes 1..12
        const double sgn = (l >= 7) ? -1.0 : 1.0;
        const bool use_filter = active && !chol_fail && l != 13;
        // inactive rows (failed / out-of-range objects) and lane 13 propagate the true state; sigma_0 and the idle lanes
        // add the zero row: the operands are chosen by ADDRESS (three 16-byte LDS reads each), not by value
        const double* base = use_filter ? &t.X[g * 6] : &t.T[g * 6];
        const double* urow = (use_filter && is_pm) ? &t.UA[g * 36 + krow * 6] : &t.Z[0];
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] = fma(sgn, urow[c], base[c]);
    }
    // ---- P1-P5: one Kepler solve per lane; strong-elliptic fast path inline, every other conic
    // branch through the out-of-line complete restatement
    double o[6];
    {
        bool kep_ok;
        if (PROP == 2) {
            const J2Params jq = {C.j2, C.r_eq, C.rk4_substeps};
            kep_ok = propagate_j2_rk4(s, C.dt, jq, o);
        } else {
            if (PROP == 3) kep_ok = kepler_hybrid_fast(s, C.dt, o);
            else kep_ok = kepler_step_fast<PROP == 2 ? 1 : PROP, 1>(s, C.dt, o);
        }
        if (PROP == 3) {
            if (__any(!kep_ok)) {   // sigma points outside the strong-elliptic regime: the reference's branches (whole-wave branch)
                // (no issue priority for the inline tier: late in an episode three wavefronts in four take it, and boosting the many
                // only starves the few -- they became the launch's tail, 8-11 us in their Cholesky stage; the rare out-of-line call keeps it)
                // second tier, inline: the conic branches for the general orientation (the strong-hyperbolic one -- where a diverged filter
                // lives -- without a call); third tier, out of line: the complete restatement for rv2coe's special branches and NaN input
                bool served = kep_ok;
                if (!ACT::late) {     // (the closed-loop instance keeps the call alone: with the tier inline it spilled until round 4's band change and is
                                      // 6 % slower since -- 56.8 k against 60.2 k env-steps/s; the callee takes the lean form too)
                    if (!kep_ok) served = kepler_conic_lean<1, true>(s, C.dt, o);
                }
                if (__any(!served)) {
                    __builtin_amdgcn_s_setprio(3);
                    if (!served) {
                        Vec6 si;
#pragma unroll
                        for (int c = 0; c < 6; ++c) si.v[c] = s[c];
                        Vec6 oo = kepler_beyond_series_tagged<1>(si, C.dt);
#pragma unroll
                        for (int c = 0; c < 6; ++c) o[c] = oo.v[c];
                    }
                }
            }
        } else if (PROP != 0) {
            // SSA_PROP_FG / J2: the solvers cover every conic; they decline only NaN / degenerate input or a
            // non-converging iteration, which IS a NaN result (farnocchia.py:353) -> 'predict returned nan'
            if (__any(!kep_ok)) {   // (whole-wave branch: twelve selects on the common path otherwise)
                asm volatile("");   // (keeps the optimiser from flattening the branch back into those selects)
                if (!kep_ok) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) o[c] = __builtin_nan("");
                }
            }
        } else if (__any(!kep_ok)) {
            // SSA_PROP_ELEMENTS outside the strong-elliptic regime (or NaN input): the complete restatement of
            // farnocchia(), out of line, for the lanes that need it (whole-wave branch: skipped otherwise)
            // (the reference's formulas branch by branch with this file's fast primitives, as SSA_PROP_HYBRID: the strong-hyperbolic
            // branch inline, the rest through the out-of-line restatement)
            bool served = kep_ok;
            if (!ACT::late) {     // (the closed-loop instance of this variant keeps the call alone: with the tier inline it spilled)
                if (!kep_ok) served = kepler_conic_lean<2, true>(s, C.dt, o);
            }
            if (__any(!served)) {
                if (!served) {
                    Vec6 si;
#pragma unroll
                    for (int c = 0; c < 6; ++c) si.v[c] = s[c];
                    Vec6 oo = kepler_beyond_series_tagged<2>(si, C.dt);
#pragma unroll
                    for (int c = 0; c < 6; ++c) o[c] = oo.v[c];
                }
            }
        }
    }
    wave_lds_sync();   // every lane has consumed t.X / t.T / t.U
    // The propagator is the register-pressure peak of the kernel.  Re-derive the lane coordinates behind it, so that the
    // lane-derived LDS addresses of the stages that follow are formed there instead of being carried across it (the
    // alternative the allocator picks for the RK4 instance is a spill).
    asm volatile("" : "+v"(lane));
    g = lane >> 4;
    l = lane & 15;
    // ... and so are the object index and its env (the multi-tile instance spilled these and the action word across the
    // propagator: 24 bytes per lane and tile = 61 MB of scratch writes per 160 000-object step); the action word is read
    // again where the rare paths below need it (a scalar load here would sit in front of every LDS wait that follows)
    obj = base + g;
    e = (valid && SSA_NENV > 1) ? (int)((uint32_t)obj / (uint32_t)p.n_obj) : 0;
    if constexpr (ENVS) e = asrc.env;
    if constexpr (FCAST && LENVS) e = asrc.env;   // (a forecast in several envs: no division per lane anywhere)
    // the next tile's inputs: in flight during the transform / covariance / observation / store of this one
    if (TILE == 1 && !ISSUE_LAST) tile_issue(pf, p, lane, next_base, next_cnt);

    // ---- U3: unscented transform, centred form of x = dot(Wm, sigmas_f):
    //   x = sigma_0' + m',   m' = (sum(Wm) - 1) sigma_0' + Wi sum_{i>=1} (sigma_i' - sigma_0')
    // (the reference's sum evaluated without the 1e8-fold cancellation of Wm0 ~ -2e8)
    // (the plain family with SSA_FLAG_REFERENCE_COV: one tile of the points themselves feeds both matrix passes, see sigma_rows_write)
    const bool rows_form = PLAIN && (C.flags & SSA_FLAG_REFERENCE_COV);   // (wave-uniform; false at compile time outside the plain family)
    if (rows_form) {
        sigma_rows_write(t, g, l, o);
    } else {
        typedef double v2d_t __attribute__((ext_vector_type(2)));
        double d[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) d[c] = o[c] - row_bcast<0>(o[c]);
        if (is_pm) {          // row [d_i, 1, 0] of the operand matrix
            v2d_t* dst = reinterpret_cast<v2d_t*>(&t.D[dbase(g) + (l - 1) * 8]);
            dst[0] = v2d_t{d[0], d[1]};
            dst[1] = v2d_t{d[2], d[3]};
            dst[2] = v2d_t{d[4], d[5]};
            dst[3] = v2d_t{1.0, 0.0};
        } else if (l == 0 || l == 13) {   // sigma_0' (until the mean replaces it) | x_true[i]
            v2d_t* dst = reinterpret_cast<v2d_t*>(l == 0 ? &t.X[g * 6] : &t.T[g * 6]);
            dst[0] = v2d_t{o[0], o[1]};
            dst[1] = v2d_t{o[2], o[3]};
            dst[2] = v2d_t{o[4], o[5]};
        }
    }
    wave_lds_sync();
    Moments mo = {0.0, 0.0, 0.0};
    if (rows_form) moment_sums_rows(t, lane);
    else if (!PLAIN && (C.flags & SSA_FLAG_REFERENCE_COV)) mo = moment_sums_mfma<true>(t, lane);   // (wave-uniform branch: the sums alone, six matrix instructions)
    else mo = moment_sums_mfma(t, lane);
    wave_lds_sync();
    double xb_l = 0.0;   // lanes 0..5: component l of the prior mean
    if (l < 6) {
        const double s0 = t.X[g * 6 + l];
        const double ssum = C.Wi * t.M[g * 12 + l];
        const double mp = C.sum_wm_m1 * s0 + ssum;
        xb_l = s0 + mp;
        t.M[g * 12 + l] = ssum;
        t.M[g * 12 + 6 + l] = mp;
        t.X[g * 6 + l] = xb_l;
    }
    const bool nan_x = ((__ballot(l < 6 && xb_l != xb_l) >> (g * 16)) & 0xFFFFull) != 0;
    wave_lds_sync();
    if (rows_form) covariance_reference_rows(t, C, lane);
    else if (!PLAIN && (C.flags & SSA_FLAG_REFERENCE_COV)) covariance_reference(t, C, lane, o, xb_l);   // (wave-uniform branch)
    else covariance_finish(t, C, lane, mo);
    wave_lds_sync();

    int st_new = st_in;
    if (active) {
        if (chol_fail) st_new = SSA_ST_PREDICT_LINALG;
        else if (nan_x) st_new = SSA_ST_PREDICT_NAN;
    }
    // SSA_FLAG_RESAMPLE (the predict() of filterpy's development branch): sigma_points(x_prior, P_prior) is drawn at the
    // end of predict() for EVERY filter, so an exhausted robust_cholesky ladder fails the filter in THIS step's predict
    // (not one step later); the update then uses those points (t.U holds the factor rows)
    if (!PLAIN && (C.flags & SSA_FLAG_RESAMPLE)) {
        const int rg = robust_chol_row_lds(t, C.scale, g, l);
        wave_lds_sync();
        if (active && st_new == SSA_ST_OK && rg == 16) st_new = SSA_ST_PREDICT_LINALG;
    }
    const int st_pred = st_new;   // (ActAll: the tile keeps the predict's outcome; a singular S shows in the outputs only)

    // ---- U5: the one update of this env (ssa_tasker_simple_2.py:292-315) for the selected object.
    // Phase 1 (row-local, lanes of the selected object's row): measurement of the sigma points, predicted measurement,
    // residuals; the rows [sigma - x | rz] go to the row's staging matrix.  Phase 2 (whole wavefront, below): the two
    // weighted moment matrices on the matrix unit (the weights enter with the right operand), inverse, gain, state and
    // covariance over all 64 lanes.
    if (ACT::late) {   // the closed loop's decision for this step: needed from here on, and normally made long ago
        asrc.before_wait(t, lane, cnt);
        act = asrc.get();
        my_update = valid && act >= 0 && (int64_t)act == (p.obj_ids ? (int64_t)t.Oid[g] : obj) && interval_ok;   // (one env: the object index IS the index in the env)
        if (__any(my_update)) __builtin_amdgcn_s_setprio(3);
    }
    // ActLookSensors: the passes start here, one per sensor.  What the predict left stays in place for every pass: the tile's x- / P-
    // (t.X / t.P), the truth (t.T), the step's matrix (t.Obs) and, from the first pass on, the sigma points handed to update() (the
    // left halves of the staging matrices).  Each pass rewrites the residual columns, P+ among them, and starts again from the
    // predict's status.
    int look_s = 0;
look_pass:
    if constexpr (LSENS) st_new = st_pred;
    bool look_vis = false, look_taken = false;   // (ActAll: the row's visibility and whether its update ran, for the outputs)
    // (ActSensors: the row's sensor matched again here rather than carried across the propagator)
    const ssa_sensor_params* SP = PASS_ARGS ? kernarg_opaque(asrc.sites()) : asrc.sites();
    if constexpr (ENVS) sid = valid ? sensor_index(asrc, SP, p.obj_ids ? (int64_t)t.Oid[g] : obj - (int64_t)asrc.env * p.n_obj) : -1;
    else if constexpr (SENS) sid = valid ? sensor_index(asrc, SP, p.obj_ids ? (int64_t)t.Oid[g] : obj) : -1;
    if (__any(my_update)) {   // whole-wave branch: a wavefront without a selected object skips the block, its variables included
    bool upd_go = false, taken = false, visible = false, attempted = false;
    double z[3] = {0.0, 0.0, 0.0}, y_row[3] = {0.0, 0.0, 0.0};   // (y_row: lane 13 of the row keeps the innovation)
    double* rec = nullptr;
    // staging matrix of the row's update: [13][9], row i = [sigma_i - x | rz_i].  The four rows' matrices (468 doubles) lie in the
    // transform's scratch, free by now: the factor tile and the head of t.D (contiguous members of Tiles)
    double* const STG = &t.UA[g * 117];
    double* const W = &t.D[330];        // small matrices: W[0..9) S | W[9..27) Pxz | W[36..54) K | W[54..57) y
    static_assert(offsetof(Tiles, D) == offsetof(Tiles, UA) + sizeof(double) * OBJ_PER_WAVE * 36, "UA and D contiguous");
    static_assert(4 * 117 <= OBJ_PER_WAVE * 36 + 330 && 330 + 57 <= 408, "update staging fits");
    if (my_update) {
        if constexpr (SENS) rec = asrc.records(SP) ? asrc.records(SP) + (int64_t)sid * SSA_UPD_STRIDE : nullptr;
        else rec = (!ALL && p.upd) ? p.upd + (int64_t)e * SSA_UPD_STRIDE : nullptr;
        // a filter that has failed (earlier, or in this step's predict) is skipped entirely (:293): no z_true, no record
        attempted = (st_new == SSA_ST_OK);
        if (attempted) {
            const double* M = &t.Obs[g * 12];
            // sigma points handed to update(): the propagated ones or, with
            // SSA_FLAG_RESAMPLE, the set drawn from the prior at the end of predict (factor rows in t.U)
            double sf[6], xb[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                sf[c] = o[c];
                xb[c] = t.X[g * 6 + c];   // the prior mean
            }
            if (!PLAIN && (C.flags & SSA_FLAG_RESAMPLE) && (!LSENS || look_s == 0)) {
                const int krow = is_pm ? (l - 1) % 6 : 0;
                const double sgn = (l >= 1 && l <= 6) ? 1.0 : ((l >= 7 && l <= 12) ? -1.0 : 0.0);
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    if (l != 13) sf[c] = xb[c] + sgn * t.UA[g * 36 + krow * 6 + c];
            }
            // (the left half of the staging row leaves now -- harmless if the object turns out not to be visible -- so that the
            // prior mean does not have to live across the measurement function)
            if constexpr (LSENS) {
                // ActLookSensors: the left half holds the sigma point itself (Phase 2 subtracts the prior mean as it reads it), and
                // keeps it for the later passes, which take their points from there -- and the truth from t.T -- instead of registers
                if (look_s == 0) {
                    if (l <= 12) {
#pragma unroll
                        for (int c = 0; c < 6; ++c) STG[l * 9 + c] = sf[c];
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 6; ++c) sf[c] = (l <= 12) ? STG[l * 9 + c] : t.T[g * 6 + c];
                }
            } else if (l <= 12) {
#pragma unroll
                for (int c = 0; c < 6; ++c) STG[l * 9 + c] = sf[c] - xb[c];
            }
            // H1/H2: measurement of every sigma point (lanes 0-12) and of the true state (lane 13)
            double enu_vec[3];
            double el_mine;
            double lim = 0.0;   // (ActSensors: the elevation mask of the row's sensor)
            bool blocked = false;   // (a moving sensor: the Earth stands between it and the lane's state)
            {
                double Mm[9], aer[3];
#pragma unroll
                for (int i = 0; i < 9; ++i) Mm[i] = M[i];
                if constexpr (SENS) {
                    // the rows of one sensor at a time (a waterfall over the sensors present), its site in scalar registers
                    for (;;) {
                        const int su = __builtin_amdgcn_readfirstlane(sid);
                        if (sid == su) {
                            if ((moving_bits >> su) & 1) blocked = hx_moving_site(p, SP->n_sensor, su, tix, sf, Mm, aer, enu_vec, lim);
                            else {
                                hx_aer_enu(sf, Mm, SP->enu[su], SP->obs_itrs[su], aer, enu_vec);
                                lim = SP->obs_limit[su];
                            }
                            break;
                        }
                    }
                } else if constexpr (LSENS) {   // (the pass's sensor: one site for the whole wavefront)
                    if ((moving_bits >> look_s) & 1) blocked = hx_moving_site(p, SP->n_sensor, look_s, tix, sf, Mm, aer, enu_vec, lim);
                    else {
                        hx_aer_enu(sf, Mm, SP->enu[look_s], SP->obs_itrs[look_s], aer, enu_vec);
                        lim = SP->obs_limit[look_s];
                    }
                } else hx_aer_enu(sf, Mm, C.enu, C.obs_itrs, aer, enu_vec);
                el_mine = aer[1];
                if (PLAIN || C.obs_type == SSA_OBS_AER) { z[0] = aer[0]; z[1] = aer[1]; z[2] = aer[2]; }
                else { z[0] = sf[0]; z[1] = sf[1]; z[2] = sf[2]; }
            }
            if constexpr (SENS || LSENS) {
                // a sensor that sees sunlit objects only, from a dark site: lane 13 holds the propagated truth in sf and tests it against
                // the Sun row the head left in LDS; an object that fails has no elevation (a NaN is below every mask), so that it is an
                // invisible object in every respect and the broadcast below stays the one there was
                // (a moving sensor has no night: the row's dark bit is not read for it, the object's own illumination still is -- and an
                // object behind the Earth's limb has no elevation either, against the mask of -infinity hx_moving_site left in lim)
                const int sun_s = SENS ? sid : look_s;
                if ((SP->sunlit_only >> sun_s) & 1) {
                    const double* sun = &t.pad1[0];
                    const bool dark = (((__double_as_longlong(sun[3]) >> sun_s) | (long long)(moving_bits >> sun_s)) & 1) != 0;
                    if (!(dark && sunlit_cylinder(sf, sun, SP->shadow_radius))) el_mine = __builtin_nan("");
                }
                if (blocked) el_mine = __builtin_nan("");
                visible = row_bcast<13>(el_mine) >= lim;   // (as seen from the row's sensor)
            } else visible = row_bcast<13>(el_mine) >= C.obs_limit;  // object_visible(): elevation of the TRUE state (:418-425)
            if (rec && l == 13) {
#pragma unroll
                for (int c = 0; c < 3; ++c) rec[SSA_UPD_Z_TRUE + c] = z[c];
            }
            if (visible) {
                // H3/H5: predicted measurement
                double zp[3];
                const double wl = (l == 0) ? C.Wc0 : (is_pm ? C.Wi : 0.0);
                if (PLAIN || C.obs_type == SSA_OBS_AER) {
                    double um[3];   // mean_z_uvw (dynamics.py:343): aer2uvw of a sigma point is its local vector enu_vec
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double u0 = row_bcast<0>(enu_vec[c]);
                        double du = is_pm ? (enu_vec[c] - u0) : 0.0;
                        um[c] = u0 + (C.sum_wm_m1 * u0 + C.Wi * row_allsum(du));
                    }
                    uvw2aer(um, zp);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        double u0 = row_bcast<0>(z[c]);
                        double du = is_pm ? (z[c] - u0) : 0.0;
                        zp[c] = u0 + (C.sum_wm_m1 * u0 + C.Wi * row_allsum(du));
                    }
                }
                // H4: residuals; lane 13 forms the innovation of the noisy measurement
                double rz[3];
                {
                    double zin[3];
                    if (l == 13) {
                        const double* zn = &t.Obs[g * 12 + 9];
#pragma unroll
                        for (int c = 0; c < 3; ++c) zin[c] = z[c] + zn[c];
                    } else {
#pragma unroll
                        for (int c = 0; c < 3; ++c) zin[c] = z[c];
                    }
                    if (PLAIN || C.obs_type == SSA_OBS_AER) residual_z_aer_wrapped(zin, zp, rz);
                    else {
#pragma unroll
                        for (int c = 0; c < 3; ++c) rz[c] = zin[c] - zp[c];
                    }
                }
                // an angles-only sensor (ssa_sensor_params.angles_only; the row's sensor, or the pass's): no range residual -- an
                // assignment, so nothing of the range noise word survives.  With S in block form below, column 2 of Pxz and of K are
                // exact zeros and x+ / P+ are the update of dim_z = 2
                if constexpr (SENS) {
                    if ((SP->angles_only >> sid) & 1) rz[2] = 0.0;
                } else if constexpr (LSENS) {
                    if ((SP->angles_only >> look_s) & 1) rz[2] = 0.0;
                }
                upd_go = true;
                if (l <= 12) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) STG[l * 9 + 6 + c] = rz[c];
                }
                if (l == 13) {   // the innovation
#pragma unroll
                    for (int c = 0; c < 3; ++c) y_row[c] = rz[c];
                }
            }
        }
    }
    // ---- Phase 2: whole wavefront, one selected object at a time
    {
        unsigned long long pend = __ballot(upd_go);
        while (pend) {   // (several selected objects in one wavefront -- vectorised envs of fewer than four objects -- take turns)
            const int gu = (__ffsll((long long)pend) - 1) >> 4;
            pend &= ~(0xFFFFull << (gu * 16));
            const double* Rm = C.R;   // (ActSensors: R of row gu's sensor, a wave-uniform index)
            if constexpr (SENS) Rm = SP->R[__builtin_amdgcn_readlane(sid, gu * 16)];
            if constexpr (LSENS) Rm = SP->R[look_s];
            // (row gu's sensor measures az and el only: wave-uniform, the turn's own)
            [[maybe_unused]] const bool ang = SENS    ? ((SP->angles_only >> __builtin_amdgcn_readlane(sid, gu * 16)) & 1) != 0
                                              : LSENS ? ((SP->angles_only >> look_s) & 1) != 0 : false;
            if (g == gu && l == 13) {
#pragma unroll
                for (int c = 0; c < 3; ++c) W[54 + c] = y_row[c];
            }
            wave_lds_sync();
            // G = [sigma - x | rz]^T (Wc rz)  (9 x 3): rows 0..5 = Pxz, rows 6..8 = S - R.  One v_mfma_f64_4x4x4 per chunk of four
            // sigma points; its blocks (lane bits 3:2) take the row tiles 0-3, 4-7 and 8 of the left operand;
            // k = lane bits 5:4, i / j = lane bits 1:0 (see moment_sums_mfma)
            {
                const int kk = lane >> 4, blk = (lane >> 2) & 3, ij = lane & 3;
                const double* SG = &t.UA[gu * 117];
                const int acol = (blk < 2) ? 4 * blk + ij : 8;     // (block 2: row 8 in every lane, rows 9..11 of G are not used; block 3 idles on it)
                double acc = 0.0;
#pragma unroll
                for (int cch = 0; cch < 4; ++cch) {
                    const int k = (cch < 3) ? 4 * cch + kk : 12;   // sigma point; the last chunk holds point 12 and three empty slots
                    const double* row = &SG[k * 9];
                    double av = row[acol];
                    if constexpr (LSENS) {   // (sigma - x: the left half holds the sigma point)
                        if (acol < 6) av = av - t.X[gu * 6 + acol];
                    }
                    double bv = row[6 + (ij < 3 ? ij : 2)] * ((cch == 0 && kk == 0) ? C.Wc0 : C.Wi);
                    if (cch == 3 && kk != 0) { av = 0.0; bv = 0.0; }
                    acc = __builtin_amdgcn_mfma_f64_4x4x4f64(av, bv, acc, 0, 0, 0);
                }
                // result lane (i = lane bits 5:4, blk, j = lane bits 1:0) holds G[4 blk + i][j]
                const int ri = 4 * blk + kk;
                if (ij < 3 && ri < 6) W[9 + ri * 3 + ij] = acc;
                if (ij < 3 && ri >= 6 && ri < 9 && ri - 6 <= ij) {   // S symmetric by construction: the upper triangle, mirrored
                    const int a = ri - 6;
                    W[a * 3 + ij] = acc + Rm[a * 3 + ij];
                    W[ij * 3 + a] = acc + Rm[ij * 3 + a];
                    if constexpr (SENS || LSENS) {
                        // (an angles-only sensor: R's 2 x 2 block alone; row and column 2 of S are exact 0 and 1, whatever R holds there)
                        if (ang && ij == 2) W[a * 3 + 2] = W[6 + a] = (a == 2) ? 1.0 : 0.0;
                    }
                }
            }
            wave_lds_sync();
            bool inv_ok;
            double SI[9];
            {
                double S[9];
#pragma unroll
                for (int c = 0; c < 9; ++c) S[c] = W[c];
                inv_ok = inv3(S, SI);          // (every lane: the inverse stays in registers)
            }
            bool nan_u = false;
            if (inv_ok) {
                // K = Pxz inv(S): 18 entries, one per lane
                if (lane < 18) {
                    const int a = lane / 3, b = lane - 3 * a;
                    W[36 + lane] = W[9 + a * 3] * SI[b] + W[9 + a * 3 + 1] * SI[3 + b] + W[9 + a * 3 + 2] * SI[6 + b];
                }
                wave_lds_sync();
                if constexpr (ALL || DRY) {   // P+ = P- - K S K^T into the row's consumed staging matrix; x and the tile's P stay as they are
                                              // (a dry run commits P+ to the tile behind its record, below)
                    if (lane < 36) {
                        const int a = lane / 6, b = lane - 6 * a;
                        double corr = 0.0;
#pragma unroll
                        for (int u = 0; u < 3; ++u) {
                            const double sk = W[u * 3] * W[36 + b * 3] + W[u * 3 + 1] * W[36 + b * 3 + 1] + W[u * 3 + 2] * W[36 + b * 3 + 2];  // (S K^T)[u][b]
                            corr = fma(W[36 + a * 3 + u], sk, corr);
                        }
                        t.UA[gu * 117 + (LSENS ? pp_at<1>(lane) : lane)] = t.P[gu * 36 + lane] - corr;
                    }
                } else {
                // x += K y  (lanes 0..5); P -= K S K^T (36 entries, one per lane)
                double xn = 0.0;
                if (lane < 6) xn = t.X[gu * 6 + lane] + (W[36 + lane * 3] * W[54] + W[36 + lane * 3 + 1] * W[55] + W[36 + lane * 3 + 2] * W[56]);
                nan_u = __ballot(lane < 6 && xn != xn) != 0;
                if (lane < 36) {
                    const int a = lane / 6, b = lane - 6 * a;
                    double corr = 0.0;
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        const double sk = W[u * 3] * W[36 + b * 3] + W[u * 3 + 1] * W[36 + b * 3 + 1] + W[u * 3 + 2] * W[36 + b * 3 + 2];  // (S K^T)[u][b]
                        corr = fma(W[36 + a * 3 + u], sk, corr);
                    }
                    t.P[gu * 36 + lane] = t.P[gu * 36 + lane] - corr;
                }
                if (lane < 6) t.X[gu * 6 + lane] = xn;
                }
            }
            if (g == gu) {
                if (!inv_ok) st_new = SSA_ST_UPDATE_LINALG;
                else {
                    taken = true;
                    if (nan_u) st_new = SSA_ST_UPDATE_NAN;
                    if (rec) {
                        if (l < 3) rec[SSA_UPD_Y + l] = W[54 + l];
                        if (l < 9) rec[SSA_UPD_S + l] = W[l];
                        if (is_sigma) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) rec[SSA_UPD_SIGMAS_H + l * 3 + c] = z[c];
                        }
                    }
                }
            }
            wave_lds_sync();   // (the next selected object reuses W)
        }
    }
    if (my_update && rec && l == 0) {
        rec[SSA_UPD_OBS_TAKEN] = taken ? 1.0 : 0.0;
        rec[SSA_UPD_VISIBLE] = visible ? 1.0 : 0.0;
        if constexpr (ENVS) rec[SSA_UPD_ACTION] = attempted ? (double)(p.obj_ids ? (int64_t)t.Oid[g] : obj - (int64_t)asrc.env * p.n_obj) : -1.0;
        else if constexpr (SENS) rec[SSA_UPD_ACTION] = attempted ? (double)(p.obj_ids ? (int64_t)t.Oid[g] : obj) : -1.0;   // (the sensor's action IS this object)
        else rec[SSA_UPD_ACTION] = attempted ? (double)(ACT::late ? act : PLAIN ? *(ConstPtr<int32_t>)p.actions : env_action<INL, SEG>(p, e)) : -1.0;   // (my_update: the env's action IS this object)
    }
    if constexpr (ALL) {
        look_vis = visible;
        look_taken = taken;
    }
    if constexpr (DRY) {   // the slot's record from P- (the tile) and P+ (the staging matrix); then P+ is the tile's
        if (my_update)
            dryrun_store(t, asrc.record(sid), g, l, attempted ? (double)(p.obj_ids ? (int64_t)t.Oid[g] : obj - (int64_t)asrc.env * p.n_obj) : -1.0,
                         st_new, visible, taken);
        wave_lds_sync();
        if (taken) {
            for (int idx = l; idx < 36; idx += 16) t.P[g * 36 + idx] = t.UA[g * 117 + idx];
        }
    }
    // The update is the register-pressure peak behind the propagator and only ONE wavefront of a launch runs it: whatever is
    // live across it would be spilled by EVERY wavefront.  So the values that are cheap to get again are got again behind
    // it: the lane coordinates, the object / env, and the next tile's loads (issued a second time).
    asm volatile("" : "+v"(lane));
    g = lane >> 4;
    l = lane & 15;
    obj = base + g;
    e = (valid && SSA_NENV > 1) ? (int)((uint32_t)obj / (uint32_t)p.n_obj) : 0;
    if constexpr (ENVS) e = asrc.env;
    if constexpr (FCAST && LENVS) e = asrc.env;   // (a forecast in several envs: no division per lane anywhere)
    if (TILE == 1 && !ISSUE_LAST) tile_issue(pf, p, lane, next_base, next_cnt);
    }   // wavefronts holding a selected object
    // envs whose action selects nobody still get a cleared record (written by object 0's row)
    if (!ALL && valid && p.upd && obj == (int64_t)e * p.n_obj && l == 0) {   // (object 0 of an env: one lane per env)
      const int a_env = ACT::late ? act : PLAIN ? *(ConstPtr<int32_t>)p.actions : env_action<INL, SEG>(p, e);
      if (!(a_env >= 0 && interval_ok && (int64_t)a_env < p.n_obj)) {
        double* rec = p.upd + (int64_t)e * SSA_UPD_STRIDE;
        rec[SSA_UPD_OBS_TAKEN] = 0.0;
        rec[SSA_UPD_VISIBLE] = 0.0;
        rec[SSA_UPD_ACTION] = -1.0;
      }
    }
    if constexpr (DRY) {    // (ActDryRunEnvs: the slots that update nobody, once per env by its first row -- the cleared record)
        if (valid && obj == (int64_t)asrc.env * p.n_obj && l == 0) {
            for (int k = 0; k < SP->n_sensor; ++k) {
                const int a = asrc.action(SP, k);   // (>= n_obj_caller: read as -1)
                bool owns = a >= 0 && interval_ok;
                for (int q = 0; q < k; ++q)
                    if (asrc.action(SP, q) == a) owns = false;
                if (!owns) {
                    double* rec = asrc.record(k);
                    const double nan = __builtin_nan("");
                    rec[SSA_DRY_ACTION] = -1.0;
                    rec[SSA_DRY_VISIBLE] = 0.0;
                    rec[SSA_DRY_TAKEN] = 0.0;
                    rec[SSA_DRY_STATUS] = 0.0;
#pragma unroll
                    for (int q = 0; q < SSA_LOOK_NSCORE; ++q) rec[SSA_DRY_SCORE + q] = nan;
                    rec[SSA_DRY_SPARE] = 0.0;
                }
            }
        }
    } else if constexpr (ENVS) {   // (ActSensorEnvs: the block below once per env -- by the first row of the tile's env, into that env's records.  Written
                            // out a second time: the one-env kernels' instructions do not survive any rewording of their own block)
        if (asrc.records(SP) && valid && obj == (int64_t)asrc.env * p.n_obj && l == 0) {
            for (int k = 0; k < SP->n_sensor; ++k) {
                const int a = asrc.action(SP, k);
                bool owns = a >= 0 && (int64_t)a < p.n_obj && interval_ok;
                for (int q = 0; q < k; ++q)
                    if (asrc.action(SP, q) == a) owns = false;
                if (!owns) {
                    double* rec = asrc.records(SP) + (int64_t)k * SSA_UPD_STRIDE;
                    rec[SSA_UPD_OBS_TAKEN] = 0.0;
                    rec[SSA_UPD_VISIBLE] = 0.0;
                    rec[SSA_UPD_ACTION] = -1.0;
                }
            }
        }
    } else if constexpr (SENS) {   // sensors that update nobody -- idle, out of range, a lower sensor's object, a step the interval skips: a cleared record
        if (asrc.records(SP) && valid && obj == 0 && l == 0) {
            for (int k = 0; k < SP->n_sensor; ++k) {
                const int a = asrc.action(SP, k);
                bool owns = a >= 0 && (int64_t)a < p.n_obj && interval_ok;
                for (int q = 0; q < k; ++q)
                    if (asrc.action(SP, q) == a) owns = false;
                if (!owns) {
                    double* rec = asrc.records(SP) + (int64_t)k * SSA_UPD_STRIDE;
                    rec[SSA_UPD_OBS_TAKEN] = 0.0;
                    rec[SSA_UPD_VISIBLE] = 0.0;
                    rec[SSA_UPD_ACTION] = -1.0;
                }
            }
        }
    }

    // ---- F1: failed filters carry the sentinels (ssa_tasker_simple_2.py:157-158, 369-382)
    wave_lds_sync();
    if (valid && (ALL ? st_pred : st_new) != SSA_ST_OK && st_in == SSA_ST_OK) {   // (ActAll: the predict's failures only)
        for (int idx = l; idx < 36; idx += 16) {
            int a = idx / 6, b = idx - a * 6;
            t.P[g * 36 + idx] = (a == b) ? (a < 3 ? X_FAILED_POS : X_FAILED_VEL) : 0.0;
        }
        if (l < 6) t.X[g * 6 + l] = (l < 3) ? X_FAILED_POS : X_FAILED_VEL;
        if (!ALL && !DRY && p.fail_log && l == 0) {
            // filter_error()'s record (:369-382): who, why, when, and error_failed() of the state the filter failed FROM (:376-378) -- the
            // step's inputs, still in HBM (a rare, row-divergent branch: three loads per failing filter)
            if (ACT::late) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the closed loop stores the previous step's tile inside this one)
            const double* xt = p.x_true_in + obj * 6;
            const double* xf = p.x_in + obj * 6;
            const double* Pd = p.P_in + obj * 36;
            const double a0 = xf[0] - xt[0], a1 = xf[1] - xt[1], a2 = xf[2] - xt[2];
            const double b0 = xf[3] - xt[3], b1 = xf[4] - xt[4], b2 = xf[5] - xt[5];
            const unsigned at = atomicAdd(p.fail_count, 1u);
            if ((int)at < p.fail_cap) {
                double* rec = p.fail_log + (int64_t)at * SSA_FAIL_STRIDE;
                rec[SSA_FAIL_ENV] = (double)e;
                rec[SSA_FAIL_OBJ] = p.obj_ids ? (double)t.Oid[g] : (double)(obj - (int64_t)e * p.n_obj);
                rec[SSA_FAIL_STATUS] = (double)st_new;
                rec[SSA_FAIL_TIME] = (double)((ACT::late ? p.env_time[0] : PLAIN ? *(ConstPtr<int32_t>)p.env_time : env_time_of<INL, SEG>(p, e)) + p.time_offset);
                rec[SSA_FAIL_ERR + 0] = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
                rec[SSA_FAIL_ERR + 1] = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
                rec[SSA_FAIL_ERR + 2] = sqrt(Pd[0] + Pd[7] + Pd[14]);
                rec[SSA_FAIL_ERR + 3] = sqrt(Pd[21] + Pd[28] + Pd[35]);
            }
        }
    }
    if constexpr (FCAST || DRY) {
        // a forecast (a dry run) has no ring: a row that had failed when the launch started passes through from the input slot, as below; one that
        // failed at an earlier step of the horizon carries the sentinels F1 gave it then (its input slot holds the healthy state)
        if (valid && st_in != SSA_ST_OK) {
            const bool at_entry = p.status[obj] != SSA_ST_OK;   // (the caller's word: never written by this launch)
            for (int idx = l; idx < 36; idx += 16) {
                const int a = idx / 6, b = idx - a * 6;
                t.P[g * 36 + idx] = at_entry ? p.P_in[obj * 36 + idx] : ((a == b) ? (a < 3 ? X_FAILED_POS : X_FAILED_VEL) : 0.0);
            }
            if (l < 6) t.X[g * 6 + l] = at_entry ? p.x_in[obj * 6 + l] : ((l < 3) ? X_FAILED_POS : X_FAILED_VEL);
        }
        if (l == 0) t.St[g] = DRY ? st_new : st_pred;   // (a forecast: the predict's outcome alone travels to the next step; a dry run: the step's)
    } else {
    if (valid && st_in != SSA_ST_OK) {  // already failed: the filter state passes through unchanged (:272)
        if (ACT::late) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (its previous state left for HBM earlier in THIS step)
        for (int idx = l; idx < 36; idx += 16) t.P[g * 36 + idx] = p.P_in[obj * 36 + idx];
        if (l < 6) t.X[g * 6 + l] = p.x_in[obj * 6 + l];
    }
    if (!(PLAIN && cnt == OBJ_PER_WAVE) && l == 0) t.St[g] = st_new;   // (the plain form's whole tile stores the register: plain_tile_out)
    }
    wave_lds_sync();
    if constexpr (LSENS) {   // sensor look_s's outputs (one env), then the next sensor's pass
        const bool last = look_s + 1 >= SP->n_sensor;
        if (TILE == 1 && ISSUE_LAST && last) tile_issue(pf, p, lane, next_base, next_cnt);
        ssa_lookahead_out os = PASS_ARGS ? *kernarg_opaque(asrc.o) : *asrc.o;
        if constexpr (FCAST) asrc.slab(os, p.n_obj, SP->n_sensor);   // (a forecast: this step's slab of every block)
        if constexpr (LENVS && !FCAST) asrc.slab(os, p.n_obj, SP->n_sensor);   // (several envs: the env's slab of every block; a forecast
                                                                               // in several envs: the one slab() above is step h's AND the env's)
        if (look_s > 0) os.x_prior = os.P_prior = nullptr;   // (no sensor axis: the first pass wrote them)
        if constexpr (LENVS) {
            if (valid) lookahead_store<1>(t, os, g, l, (int64_t)look_s * p.n_obj + (p.obj_ids ? (int64_t)t.Oid[g] : obj - (int64_t)asrc.env * p.n_obj),
                                          st_new, look_vis, look_taken);
        } else {
        if (valid) lookahead_store<1>(t, os, g, l, (int64_t)look_s * p.n_obj + (p.obj_ids ? (int64_t)t.Oid[g] : obj), st_new, look_vis, look_taken);
        }
        if (!last) {
            ++look_s;
            wave_lds_sync();   // (this pass's reads of P+ precede the next pass's staging)
            goto look_pass;
        }
        return;
    } else if constexpr (ALL) {   // the lookahead's outputs; nothing of the step's epilogue (observation, metrics, statistics, tile store)
        if (valid) lookahead_store(t, *asrc.o, g, l, (int64_t)e * p.n_obj + (p.obj_ids ? (int64_t)t.Oid[g] : obj - (int64_t)e * p.n_obj),
                                   st_new, look_vis, look_taken);
        return;
    } else if constexpr (DRY) {   // the records are out; nothing of the step's epilogue, and the tile stays where it is
        return;
    }
    // (the plain form's whole tile -- wave-uniform --: the metrics from registers and a store stage of its own, see plain_tile_out)
    const bool plain_whole = PLAIN && cnt == OBJ_PER_WAVE;
    if constexpr (PLAIN) {
        if (plain_whole) {
            PlainDst dst;
            plain_dst_fetch(dst);
            double met = 0.0;
            if (l < 4) met = metric_value(t, g, l);
            plain_tile_out<TILE != 1>(t, p, dst, lane, base, met, st_new);
        }
    }
    if (!plain_whole) observe_rows(t, g, l, cnt != OBJ_PER_WAVE);
    // O4 in the epilogue (atomics-statistics path): the (az, el, range, trace P) block of the NEW state -- the 'aer'
    // observation mode and the multi-GPU all-gather payload -- from the tiles, so that no second pass over x / P (the
    // former post kernel: 6.7 MB re-read per 20 000 objects plus a launch) is needed
    if (!PLAIN && p.aer_out && p.stat_shards) {
        if (l < 4 && valid) aer_obs_tile<INL, SEG>(t, p, C, g, l, e, p.obj_ids ? (int64_t)e * p.n_obj + t.Oid[g] : obj);
    }
    wave_lds_sync();
    if (!ACT::late) {   // (closed_loop_kernel stores the tile itself, AFTER it has announced its part of the decision)
        if (!PLAIN && p.spos_tiles && p.stat_shards && lane == 0) {   // the tile's first maximum of sigma_pos (np.argmax for the 'shaped' reward): one slot, no atomics
            unsigned long long key, idx;
            spos_tile_best(t, cnt, obj - (int64_t)e * p.n_obj, key, idx, p.obj_ids != nullptr);
            unsigned long long* slot = (unsigned long long*)p.spos_tiles + 2 * (int64_t)tile;
            __hip_atomic_store(slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (agent scope: SSA_LAUNCH_FOLD_INSIDE reads them in this launch)
            __hip_atomic_store(slot + 1, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!plain_whole) store_tile<TILE != 1, PLAIN>(t, p, lane, base, cnt);
        // O3 by sharded atomics: max delta_pos (as ordered bits: non-negative doubles and NaN order like unsigned
        // integers, so NaN wins exactly as in np.max), trinary counts (packed in one word), failures
        const bool one_env = SSA_NENV == 1 || ((uint32_t)base / (uint32_t)p.n_obj == (uint32_t)(base + cnt - 1) / (uint32_t)p.n_obj);
        if (FROM_METRICS && (PLAIN || (p.launch_mask & SSA_LAUNCH_STATS_FROM_METRICS))) {
            // (one env, stat_shards given: the launcher.)  Max delta_pos and the counts are reduced from the metrics rows just stored by the
            // service wavefronts of the NEXT launch (stats_service_wave); only the failed filters are counted here -- the status words
            // are updated in place -- and only by a tile that has one: the row's status is still in a register, no LDS read, no wait
            const unsigned long long failed = __ballot(valid && st_new != 0) & 0x0001000100010001ull;
            if (failed && lane == 63) {
                unsigned long long* sh = (unsigned long long*)p.stat_shards + (int64_t)(tile & (SSA_STAT_SHARDS - 1)) * SSA_STAT_SHARD_WORDS;
                atomicAdd(sh + 2, (unsigned long long)__popcll(failed));
            }
        } else if (p.stat_shards && one_env) {
            // common case, the tile lies in one env.  Every lane of a row reads its row's delta_pos, so the COUNTS are ballots:
            // one bit per row (lanes 0, 16, 32, 48) of the comparison's mask, counted by the scalar unit -- no packing into
            // words, no cross-row adds.  The maximum crosses rows by two DPP steps (row_bcast:15 into rows 1 and 3, row_bcast:31
            // into rows 2 and 3) and ends in row 3.
            const double dp = t.Met[g * 4 + 0];
            const bool rv = g < cnt;
            const unsigned long long rowbit = 0x0001000100010001ull;
            const unsigned c4 = (unsigned)__popcll(__ballot(rv && dp < 1e4) & rowbit);
            const unsigned c7 = (unsigned)__popcll(__ballot(rv && dp < 1e7) & rowbit);
            const unsigned nfl = (unsigned)__popcll(__ballot(rv && t.St[g] != 0) & rowbit);
            unsigned long long mx = rv ? ((unsigned long long)__double_as_longlong(dp) & 0x7fffffffffffffffull) : 0ull;
#define SSA_XROW(CTRL, ROWMASK)                                                                                          \
            {                                                                                                            \
                const unsigned long long m2 = ((unsigned long long)(unsigned)__builtin_amdgcn_update_dpp(0, (int)(mx >> 32), CTRL, ROWMASK, 0xF, false) << 32) | \
                                              (unsigned)__builtin_amdgcn_update_dpp(0, (int)(mx & 0xffffffffull), CTRL, ROWMASK, 0xF, false);                 \
                mx = m2 > mx ? m2 : mx;                                                                                  \
            }
            SSA_XROW(0x142, 0xA)   // row_bcast:15
            SSA_XROW(0x143, 0xC)   // row_bcast:31
#undef SSA_XROW
            bool i_fold = false;
            if (lane == 63) {
                const int64_t e_tile = (p.n_env > 1) ? (int64_t)((uint32_t)base / (uint32_t)p.n_obj) : 0;
                unsigned long long* sh = (unsigned long long*)p.stat_shards + ((e_tile * SSA_STAT_SHARDS) + (tile & (SSA_STAT_SHARDS - 1))) * SSA_STAT_SHARD_WORDS;
                atomicMax(sh, mx);
                atomicAdd(sh + 1, (unsigned long long)c4 | ((unsigned long long)c7 << 32));
                if (nfl) atomicAdd(sh + 2, (unsigned long long)nfl);
                if (FOLD_OK && (p.launch_mask & SSA_LAUNCH_FOLD_INSIDE)) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // this tile's sums are in before it is counted
                    i_fold = stat_tile_counted(p, e_tile, tile);
                }
            }
            if (FOLD_OK && (p.launch_mask & SSA_LAUNCH_FOLD_INSIDE) && __any(i_fold)) {    // the env's last tile: every shard of it is complete
                const int64_t e_tile = (p.n_env > 1) ? (int64_t)((uint32_t)base / (uint32_t)p.n_obj) : 0;
                fold_stat_shards_inside((unsigned long long*)p.stat_shards + e_tile * SSA_STAT_SHARDS * SSA_STAT_SHARD_WORDS,
                                        p.stats + e_tile * SSA_STAT_STRIDE, lane);
                if (p.spos_tiles) {
                    int t_lo, t_hi;
                    env_tile_range(p.n_obj, (int)e_tile, t_lo, t_hi);
                    fold_spos_tiles<true>((const unsigned long long*)p.spos_tiles, t_lo, t_hi, p.stats + e_tile * SSA_STAT_STRIDE, lane);
                }
            }
        } else if (p.stat_shards) {   // a tile that straddles envs: one group of atomics per env (lane 0)
          unsigned fold_envs = 0u;    // bit i: env e_first + i was completed by this tile (a tile spans at most four envs)
          const int64_t e_first = (p.n_env > 1) ? (int64_t)((uint32_t)base / (uint32_t)p.n_obj) : 0;
          if (lane == 0) {
            int64_t e_cur = -1;
            unsigned long long mx = 0ull, cnts = 0ull, nf = 0ull;
            int64_t j_run = base - e_first * p.n_obj, e_run = e_first;   // (env, index) of row gg, advanced without dividing
            for (int gg = 0; gg <= cnt; ++gg) {
                while (j_run >= p.n_obj) { j_run -= p.n_obj; ++e_run; }
                const int64_t eg = (gg < cnt) ? e_run : -2;
                ++j_run;
                if (eg != e_cur) {
                    if (e_cur >= 0) {
                        unsigned long long* sh = (unsigned long long*)p.stat_shards + ((e_cur * SSA_STAT_SHARDS) + (tile & (SSA_STAT_SHARDS - 1))) * SSA_STAT_SHARD_WORDS;
                        atomicMax(sh, mx);
                        atomicAdd(sh + 1, cnts);
                        if (nf) atomicAdd(sh + 2, nf);
                        if (FOLD_OK && (p.launch_mask & SSA_LAUNCH_FOLD_INSIDE)) {
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                            if (stat_tile_counted(p, e_cur, tile)) fold_envs |= 1u << (unsigned)(e_cur - e_first);
                        }
                    }
                    e_cur = eg; mx = 0ull; cnts = 0ull; nf = 0ull;
                }
                if (gg < cnt) {
                    const double dp = t.Met[gg * 4 + 0];
                    unsigned long long bits = (unsigned long long)__double_as_longlong(dp) & 0x7fffffffffffffffull;
                    mx = bits > mx ? bits : mx;
                    cnts += (unsigned long long)(dp < 1e4) + ((unsigned long long)(dp < 1e7) << 32);
                    nf += t.St[gg] != 0;
                }
            }
          }
          if (FOLD_OK && (p.launch_mask & SSA_LAUNCH_FOLD_INSIDE)) {
              fold_envs = (unsigned)__builtin_amdgcn_readfirstlane((int)fold_envs);   // (lane 0's word)
              for (int i = 0; i < OBJ_PER_WAVE; ++i)
                  if (fold_envs & (1u << i))
                      fold_stat_shards_inside((unsigned long long*)p.stat_shards + (e_first + i) * SSA_STAT_SHARDS * SSA_STAT_SHARD_WORDS,
                                              p.stats + (e_first + i) * SSA_STAT_STRIDE, lane);      // (straddling tiles: no spos_tiles, see step_launch)
          }
        }
        // raw-shard consumers (stat_shards_clear): the first tile's wavefront zeroes the shard set the NEXT step accumulates
        // into -- at the very end, so that no wavefront waits for this pointer's kernarg line before its tile loads
        if (!PLAIN && tile == 0) {
            if (p.stat_shards_clear) {
                unsigned long long* z = (unsigned long long*)p.stat_shards_clear;
                for (int i = lane; i < p.n_env * SSA_STAT_SHARDS * 4; i += 64) z[(i >> 2) * SSA_STAT_SHARD_WORDS + (i & 3)] = 0ull;   // (the used words)
            }
        }
    }
#undef SSA_NENV
}

// folds the SSA_STAT_SHARDS accumulators of the atomics path of env e into stats and clears them (one wavefront)
SSA_DEV void fold_stat_shards(unsigned long long* __restrict__ shards, double* __restrict__ stats, int e, int lane,
                              const unsigned long long* __restrict__ spos = nullptr, int64_t n_obj = 0)
{
    static_assert(SSA_STAT_SHARDS == 128, "two shards per lane");
    unsigned long long* sh = shards + ((int64_t)e * SSA_STAT_SHARDS + lane) * SSA_STAT_SHARD_WORDS;
    unsigned long long* sh2 = sh + 64 * SSA_STAT_SHARD_WORDS;
    unsigned long long mx = sh[0], cn = sh[1], nf = sh[2];
    const unsigned long long mb = sh2[0], cb = sh2[1], nb = sh2[2];
    sh[0] = 0ull; sh[1] = 0ull; sh[2] = 0ull;
    sh2[0] = 0ull; sh2[1] = 0ull; sh2[2] = 0ull;
    mx = mb > mx ? mb : mx;
    cn += cb;
    nf += nb;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long m2 = __shfl_down(mx, off, 64), c2 = __shfl_down(cn, off, 64), n2 = __shfl_down(nf, off, 64);
        mx = m2 > mx ? m2 : mx;
        cn += c2;
        nf += n2;
    }
    if (lane == 0 && stats) {
        double* o = stats + (int64_t)e * SSA_STAT_STRIDE;
        o[SSA_STAT_MAX_DPOS] = __longlong_as_double((long long)mx);
        o[SSA_STAT_CNT_LT_1E4] = (double)(cn & 0xffffffffull);
        o[SSA_STAT_CNT_LT_1E7] = (double)(cn >> 32);
        o[SSA_STAT_ARGMAX_SPOS] = -1.0;
        o[SSA_STAT_N_FAILED] = (double)nf;
        o[SSA_STAT_MAX_SPOS] = __builtin_nan("");
        o[6] = 0.0; o[7] = 0.0;
    }
    if (spos && stats) {     // np.argmax / np.max of sigma_pos from the tiles' slots (a kernel boundary behind their writers)
        int t_lo, t_hi;
        env_tile_range(n_obj, e, t_lo, t_hi);
        fold_spos_tiles<false>(spos, t_lo, t_hi, stats + (int64_t)e * SSA_STAT_STRIDE, lane);
    }
}
__global__ void __launch_bounds__(64) reward_fold_kernel(unsigned long long* __restrict__ shards, double* __restrict__ stats,
                                                         const unsigned long long* __restrict__ spos, int64_t n_obj)
{
    fold_stat_shards(shards, stats, blockIdx.x, threadIdx.x, spos, n_obj);
}

// the service wavefronts on their own (ssa_stats_fold_metrics_f64: the last step of a sequence), one per block
__global__ void __launch_bounds__(64) reward_service_kernel(const double* __restrict__ dpos, unsigned long long* __restrict__ shards,
                                                            double* __restrict__ stats, const unsigned long long* __restrict__ spos, int64_t n_obj)
{
    stats_service_wave(dpos, shards, stats, spos, n_obj, blockIdx.x, gridDim.x, threadIdx.x);
}

// Workgroup -> tile, XCD-aware.  Workgroups are handed to the eight XCDs round-robin (block b runs on XCD b % 8) and every XCD
// has its own L2.  With tile = b, neighbouring tiles -- which share the 128-byte lines of x / x_true (192 B per tile), the
// metrics (32-byte runs) and the status words -- always sat on different XCDs: both fetched the shared input lines and both
// wrote their part of the shared output lines back (PMC at 160 000 objects: reads 1.26x, writes 1.66x the algorithmic
// bytes).  Here the blocks of one XCD take a CONTIGUOUS run of tiles: XCD x owns tiles [x q + min(x, r), ...) with
// q = n / 8, r = n % 8.
SSA_DEV int xcd_tile(int b, int n)
{
    const int x = b & 7, i = b >> 3, q = n >> 3, r = n & 7;
    return x * q + (x < r ? x : r) + i;
}

// The issue priority of a wavefront for its next turn (a tile of a grid-stride step, a step of a resident tile), rotated by its slot on
// its SIMD (HW_ID bits 3:0).  The SIMD arbiter serves the oldest wavefront first: left alone, the 5 co-resident wavefronts finish their
// K steps one after the other and the SIMD runs the tail of the launch with 4, 3, 2, 1 of them (latency-bound).  Rotating the issue
// priority per turn keeps them level, so all stay resident and the stages of different wavefronts interleave until the end.
// (s_setprio takes an immediate: hence the switch.)
SSA_DEV void rotate_issue_priority(unsigned wave_slot, unsigned turn)
{
    switch ((wave_slot + turn) & 3u) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}

// The tile walk of the four tile kernels: step_fast_kernel (ActEarly), step_sensors_kernel (ActSensors), lookahead_kernel (ActAll)
// and lookahead_sensors_kernel (ActLookSensors).  MULTI = false is the one-tile-per-wavefront instance (every launch up to
// 20 480 objects): no loop, no staging registers.  MULTI = true is the grid-stride walk: wavefront w advances tiles w, w + G,
// w + 2G, ... (G = nwork, chosen by the launcher so that every wavefront is resident at once and all get the same number of
// tiles) with the next tile's loads issued while the current one is being worked on.
//
// Each kernel carries one argument block K behind six scalar arguments.  TileArgs<K> is its kernarg segment as a struct: kernel
// arguments are laid out in declaration order at their natural alignment, exactly as the members of this mirror are
// (tests/test_abi_and_host.py parses the shipped code object's metadata and checks the offset of the by-value block against it).
// The leading arguments -- the two tile counts and the pointers k.p.{P_in, x_in, x_true_in, status} repeated -- are plain
// scalars: they are PRELOADED into SGPRs at wavefront launch (-amdgpu-kernarg-preload-count, _build.py), so the tile's loads --
// the first link of every wavefront's dependency chain -- leave without waiting for a scalar-memory round trip to the segment.
// That holds only while NOTHING in front of the loads reads the block: the one-tile instance therefore gets the count of WHOLE tiles
// in `ntiles` (TileGrid::arg) and decides "LDS-DMA or the ragged tile's register path" from it -- decided from n_env x n_obj, as
// it was, the loads stood behind a scalar load of both and its wait.  The grid-stride instance keeps the tile count there.
template <class K> struct TileArgs {
    int ntiles, nwork;
    const double *pre_P_in, *pre_x_in, *pre_x_true_in;
    const int32_t* pre_status;
    K k;
};
template <class K> using KernargPtr = ConstPtr<K>;
// every tile kernel's block starts with the step's, at the same place behind the preloaded arguments
static_assert(offsetof(TileArgs<StepK>, k) == 40 && offsetof(StepK, p) == sizeof(ssa_consts), "the step's parameter block in the argument segment");
SSA_DEV ConstPtr<ssa_step_params> tile_kernel_params()
{
    return (ConstPtr<ssa_step_params>)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TileArgs<StepK>, k) + offsetof(StepK, p));
}
// The argument blocks: the step's own (StepK); the lookahead's outputs, at the caller's rows, behind it (LookK); a sensor
// network's sites behind the step's (SensK) or the lookahead's (LookSensK) block.
struct LookK {
    StepK k;
    ssa_lookahead_out o;
};
struct SensK {
    StepK k;
    ssa_sensor_params s;
};
struct LookSensK {
    LookK k;
    ssa_sensor_params s;
};
struct VecLookSensK {   // (LookSensK's layout under a name of its own: the type selects ActLookSensorEnvs)
    LookK k;
    ssa_sensor_params s;
};
struct PlainK {   // (StepK's layout under a name of its own: the type selects ActPlain)
    StepK k;
};
struct VecSensK {   // ... and, behind SensK's, the envs' action rows and records (ssa_env_step_sensors_envs_f64)
    StepK k;
    ssa_sensor_params s;
    ssa_sensor_envs_params v;
};
// what a block hands process_wave: the step's constants and parameters, and the ACT policy (its pointers into the block)
SSA_DEV const StepK& step_of(const StepK& k) { return k; }
SSA_DEV const StepK& step_of(const LookK& k) { return k.k; }
SSA_DEV const StepK& step_of(const PlainK& k) { return k.k; }
SSA_DEV const StepK& step_of(const SensK& k) { return k.k; }
SSA_DEV const StepK& step_of(const LookSensK& k) { return k.k.k; }
SSA_DEV const StepK& step_of(const VecLookSensK& k) { return k.k.k; }
SSA_DEV ConstPtr<int32_t> vector_sensors_inline_rows()   // (by the segment's address, as tile_kernel_params: rows indexed by the tile's env)
{
    return (ConstPtr<int32_t>)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TileArgs<VecSensK>, k) + offsetof(VecSensK, v) +
                               offsetof(ssa_sensor_envs_params, inline_action));
}
SSA_DEV const StepK& step_of(const VecSensK& k) { return k.k; }
SSA_DEV ActEarly act_of(const StepK&) { return ActEarly(); }   // (the leading {} below: ActBase, which has no members)
SSA_DEV ActPlain act_of(const PlainK&) { return ActPlain(); }
SSA_DEV ActAll act_of(const LookK& k) { return ActAll{{}, &k.o}; }
SSA_DEV ActSensors act_of(const SensK& k) { return ActSensors{{}, &k.s}; }
SSA_DEV ActLookSensors act_of(const LookSensK& k) { return ActLookSensors{{}, &k.k.o, &k.s}; }
SSA_DEV ActLookSensorEnvs act_of(const VecLookSensK& k) { return ActLookSensorEnvs{{}, &k.k.o, &k.s, 0}; }   // (process_wave enters the tile's env)
SSA_DEV ActSensorEnvs act_of(const VecSensK& k) { return ActSensorEnvs{{}, &k.s, &k.v, 0, nullptr, nullptr}; }   // (process_wave enters the tile's env)
// WALK: what sets the four kernels apart
enum : unsigned {
    WALK_STEP = 1,          // a step: the deferred fold of the previous step's statistics in the extra wavefronts (unit >= nwork, one
                            // per env) and the issue priority rotated per tile (rotate_issue_priority)
    WALK_ONE_ENV = 2,       // a sensor network: one env, n_obj objects
    WALK_ACT_SEGMENT = 4,   // the one-tile instance takes the ACT's pointers by the argument segment's address, not the argument's:
                            // kernarg_opaque (process_wave) needs a pointer into the segment
    WALK_BASE_PER_TILE = 8, // the grid-stride loop carries the segment's base and adds the block's offset per tile (step_fast_kernel),
                            // not the block's address formed once in front of the loop
    WALK_PLAIN = 16         // the launcher's plain form (ActPlain; one-tile instance only): one env, statistics from the metrics rows
};
// One tile kernel: NAME<PROP, MULTI>(ntiles (MULTI; else the whole tiles), nwork, pre_P_in, pre_x_in, pre_x_true_in, pre_status, const K k_arg).
// The walk is written out once, here, but expands into the body of each kernel rather than living in a device function they call:
// process_wave has to be inlined straight into the kernel.  Behind a device function its body is optimised once more, on its own
// and without the kernel's launch bounds, before it reaches the kernel -- which reorders the step kernel's instructions (and
// promotes one of its private arrays that the kernel itself leaves to the code generator).
// In the grid-stride loop the body must compile like a one-tile kernel: the argument block and the lane id are re-derived per
// tile (the empty asm statements), so that the ~100 argument scalars and the lane-derived LDS addresses are produced on demand
// instead of being carried around the loop in registers.  The block lies behind the preloaded scalar arguments (TileArgs).
// wave_lds_sync() between tiles: the tile's LDS reads (its stores) precede the next tile's commit.
#define SSA_TILE_KERNEL(NAME, K, WALK)                                                                                                        \
    template <int PROP, bool MULTI>                                                                                                           \
    __global__ void __launch_bounds__(64, SSA_STEP_WAVES) NAME(int ntiles, int nwork, const double* pre_P_in, const double* pre_x_in,         \
                                                               const double* pre_x_true_in, const int32_t* pre_status, const K k_arg)         \
    {                                                                                                                                         \
        __shared__ Tiles t;                                                                                                                   \
        int lane = threadIdx.x;                                                                                                               \
        const int unit = (int)blockIdx.x;                                                                                                     \
        if (((WALK) & WALK_STEP) && unit >= nwork) {                                                                                          \
            const ssa_step_params& p = step_of(k_arg).p;                                                                                      \
            if (!MULTI && !((WALK) & WALK_ONE_ENV) && (((WALK) & WALK_PLAIN) || (p.launch_mask & SSA_LAUNCH_STATS_FROM_METRICS)))             \
                stats_service_wave(p.metrics_prev, (unsigned long long*)p.stat_shards_prev, p.stats_prev,                                     \
                                   (const unsigned long long*)p.spos_tiles_prev, p.n_obj, unit - nwork, (int)gridDim.x - nwork, lane);        \
            else                                                                                                                              \
                fold_stat_shards((unsigned long long*)p.stat_shards_prev, p.stats_prev, unit - nwork, lane,                                   \
                                 (const unsigned long long*)p.spos_tiles_prev, p.n_obj);                                                      \
            return;                                                                                                                           \
        }                                                                                                                                     \
        const int64_t total = ((WALK) & WALK_ONE_ENV) ? step_of(k_arg).p.n_obj : (int64_t)step_of(k_arg).p.n_env * step_of(k_arg).p.n_obj;    \
        TileRegs pf;                                                                                                                          \
        int tile = xcd_tile(unit, nwork);                                                                                                     \
        if (!MULTI) {                                                                                                                         \
            const int64_t base = (int64_t)tile * OBJ_PER_WAVE;                                                                                \
            const bool whole = tile < ntiles;   /* (this instance: the count of WHOLE tiles, TileGrid::arg)   */                               \
            /* (the object total -- scalar loads and a wait -- is formed where it is used: by the ragged tile, and behind the loads) */       \
            tile_dma_issue(t, pf, pre_P_in, pre_x_in, pre_x_true_in, pre_status, lane, base, whole, step_of(k_arg).p,                         \
                           ((WALK) & (WALK_ONE_ENV | WALK_PLAIN)) != 0);                                                                      \
            int cnt = OBJ_PER_WAVE;                                                                                                           \
            asm volatile("" : "+s"(cnt));                                                                                                     \
            if (!whole) cnt = (int)(tile_total(step_of(k_arg).p, ((WALK) & (WALK_ONE_ENV | WALK_PLAIN)) != 0) - base);                        \
            const K& ka = ((WALK) & WALK_ACT_SEGMENT)                                                                                         \
                              ? *(const K*)(KernargPtr<K>)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TileArgs<K>, k))    \
                              : k_arg;                                                                                                        \
            auto act = act_of(ka);                                                                                                            \
            process_wave<PROP, 0>(t, step_of(k_arg).c, step_of(k_arg).p, lane, base + (lane >> 4), (lane >> 4) < cnt, base, cnt, pf, 0, 0,    \
                                  tile, act);                                                                                                 \
            return;                                                                                                                           \
        }                                                                                                                                     \
        {                                                                                                                                     \
            const int64_t b0 = (int64_t)tile * OBJ_PER_WAVE;                                                                                  \
            tile_issue(pf, step_of(k_arg).p, lane, b0, tile < ntiles ? (int)((total - b0) < OBJ_PER_WAVE ? (total - b0) : OBJ_PER_WAVE) : 0); \
        }                                                                                                                                     \
        constexpr size_t pre_off = ((WALK) & WALK_BASE_PER_TILE) ? 0 : offsetof(TileArgs<K>, k);                                              \
        KernargPtr<K> kp = (KernargPtr<K>)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + pre_off);                                    \
        unsigned wave_slot, turn = 0;                                                                                                         \
        if ((WALK) & WALK_STEP) asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 0, 4)" : "=s"(wave_slot));                                 \
        for (; tile < ntiles; tile += nwork) {                                                                                                \
            if ((WALK) & WALK_STEP) rotate_issue_priority(wave_slot, turn++);                                                                 \
            asm volatile("" : "+s"(kp));                                                                                                      \
            asm volatile("" : "+v"(lane));                                                                                                    \
            const K& k = *(const K*)((const char*)kp + (offsetof(TileArgs<K>, k) - pre_off));                                                 \
            const int64_t base = (int64_t)tile * OBJ_PER_WAVE;                                                                                \
            const int cnt = (int)((total - base) < OBJ_PER_WAVE ? (total - base) : OBJ_PER_WAVE);                                             \
            const int nt = tile + nwork;                                                                                                      \
            const int64_t nbase = (int64_t)nt * OBJ_PER_WAVE;                                                                                 \
            const int ncnt = nt < ntiles ? (int)((total - nbase) < OBJ_PER_WAVE ? (total - nbase) : OBJ_PER_WAVE) : 0;                        \
            auto act = act_of(k);                                                                                                             \
            process_wave<PROP, 1>(t, step_of(k).c, step_of(k).p, lane, base + (lane >> 4), (lane >> 4) < cnt, base, cnt, pf, nbase, ncnt,     \
                                  tile, act);                                                                                                 \
            wave_lds_sync();                                                                                                                  \
        }                                                                                                                                     \
    }

// The kernels' names are what the profiles, the host tests and bench.py's roofline find them by.
SSA_TILE_KERNEL(step_fast_kernel, StepK, WALK_STEP | WALK_BASE_PER_TILE)                   // a step (ssa_env_step_f64)
SSA_TILE_KERNEL(step_plain_kernel, PlainK, WALK_STEP | WALK_PLAIN)                         // ... in the plain one-env form (step_plain_form)
SSA_TILE_KERNEL(lookahead_kernel, LookK, 0)                                                // the lookahead (ssa_lookahead_f64)
SSA_TILE_KERNEL(lookahead_sensors_kernel, LookSensK, WALK_ONE_ENV | WALK_ACT_SEGMENT)      // a sensor network's lookahead
SSA_TILE_KERNEL(step_sensors_kernel, SensK, WALK_STEP | WALK_ONE_ENV)                      // a sensor network's step
SSA_TILE_KERNEL(vector_sensors_kernel, VecSensK, WALK_STEP)                                // ... in each of several envs
SSA_TILE_KERNEL(lookahead_sensor_envs_kernel, VecLookSensK, WALK_ACT_SEGMENT)           // a network's lookahead in each of several envs
#undef SSA_TILE_KERNEL

// Rollout: K consecutive env steps of the same objects in ONE launch.  An object's trajectory depends on no other
// object (the single update per step touches only the selected one; the statistics are reductions), so a wavefront
// loads its tile once and advances it K steps with state, covariance, truth and status resident in LDS, writing every
// step's outputs to that step's ring slot exactly as K single-step launches would; per-step statistics go to per-step
// shard sets, folded by rollout_fold_kernel.  Needs the actions of all K steps up front (open-loop schedules).
struct RollK {   // ONE kernel argument, so that the per-step re-derivation below can address both halves
    StepK k;
    ssa_rollout_params r;
};
// ... and a sensor network's: its sites and its schedule behind the rollout's block (ssa_env_rollout_sensors_f64)
struct RollSensK {
    RollK k;
    ssa_sensor_params s;
    ssa_rollout_sensors_params rs;
};
// What sets the resident-tile kernels apart, chosen by the argument-block type (as step_of / act_of for the tile kernels): the step's
// block (step_of), what the launch fixes -- its steps, its objects, a ring's strides (roll_plan) --, the block the tile is first loaded
// from (roll_source), and the block and the ACT of step kk (roll_act).
SSA_DEV const RollK& roll_of(const RollK& a) { return a; }
SSA_DEV const RollK& roll_of(const RollSensK& a) { return a.k; }
SSA_DEV const StepK& step_of(const RollK& a) { return a.k; }
SSA_DEV const StepK& step_of(const RollSensK& a) { return a.k.k; }
// the envs of the launch: a sensor network's is one (nothing per env is formed or carried, as WALK_ONE_ENV in the tile kernels)
SSA_DEV int roll_envs(const RollK& a) { return a.k.p.n_env; }
SSA_DEV int roll_envs(const RollSensK&) { return 1; }
// A rollout's plan: the ring of E envs -- slots, steps, objects and the strides of a slot -- formed once, in front of the walk's loops.
struct Ring {
    int E, H, K_steps;
    int64_t total, sx, sP, so_, sm, su;
};
SSA_DEV Ring ring_of(const RollK& a, int E)
{
    const int H = a.r.history, K_steps = a.r.n_steps;
    const int64_t total = (int64_t)E * a.k.p.n_obj;
    return Ring{E, H, K_steps, total, total * 6, total * 36, total * 12, (int64_t)E * 4 * a.k.p.n_obj, (int64_t)E * SSA_UPD_STRIDE};
}
SSA_DEV Ring roll_plan(const RollK& a) { return ring_of(a, roll_envs(a)); }
SSA_DEV Ring roll_plan(const RollSensK& a) { return ring_of(a.k, roll_envs(a)); }
// the tile's state comes from the ring's input slot ...
SSA_DEV ssa_step_params roll_source(const RollK& a, const Ring& g)
{
    const int si0 = (a.r.slot_out + g.H - 1) % g.H;
    ssa_step_params p0 = a.k.p;
    p0.x_true_in = a.r.x_true_ring + si0 * g.sx;
    p0.x_in = a.r.x_ring + si0 * g.sx;
    p0.P_in = a.r.P_ring + si0 * g.sP;
    return p0;
}
SSA_DEV ssa_step_params roll_source(const RollSensK& a, const Ring& g) { return roll_source(a.k, g); }
// the ACT policy of a rollout's step kk, which writes ring slot `so` (owns: it is the step that finally owns the slot) -- after pk's own fields
SSA_DEV ActEarly ring_act(const RollK&, ssa_step_params&, int, int, bool) { return ActEarly(); }
SSA_DEV ActSchedule ring_act(const RollSensK& a, ssa_step_params& pk, int kk, int so, bool owns)
{
    pk.upd = nullptr;       // (the env's action word and record are not read, as in the network's step)
    pk.actions = nullptr;
    return ActSchedule{{}, &a.s, a.rs.actions + (int64_t)kk * SSA_MAX_SENSORS,
                       (a.rs.upd_ring && owns) ? a.rs.upd_ring + (int64_t)so * a.s.n_sensor * SSA_UPD_STRIDE : nullptr};
}
// ... and step kk reads slot si and writes slot so: the block (pk) and the ACT policy of step kk; `ka` is the block as re-derived for
// this step.  One body for both rollouts, and the plan's scalars in locals of its own: the slot's derivation and ring_act's arguments
// have to meet in ONE function with plain values to work on -- halves in functions of their own, or values read through `g` where they
// are used, are optimised apart before they reach the kernel, which then compiles to other instructions.
template <class K>
SSA_DEV auto roll_act(const Ring& g, const K& ka, ssa_step_params& pk, int kk, int ntiles)
{
    const int E = g.E, H = g.H, K_steps = g.K_steps;
    const int64_t sx = g.sx, sP = g.sP, so_ = g.so_, sm = g.sm, su = g.su;
    const StepK& k = roll_of(ka).k;
    const ssa_rollout_params& r = roll_of(ka).r;
    const int so = (r.slot_out + kk) % H, si = (so + H - 1) % H;
    pk = k.p;
    pk.time_offset = k.p.time_offset + kk;
    pk.x_true_in = r.x_true_ring + si * sx;  pk.x_true_out = r.x_true_ring + so * sx;
    pk.x_in = r.x_ring + si * sx;            pk.x_out = r.x_ring + so * sx;
    pk.P_in = r.P_ring + si * sP;            pk.P_out = r.P_ring + so * sP;
    pk.obs = r.obs_ring + so * so_;
    pk.metrics = r.metrics_ring + so * sm;
    // per-ENV outputs are written by whichever wavefront owns the selected object, and wavefronts advance at their own pace: only the
    // step that finally owns a ring slot may write it (per-object outputs have one writer, in order)
    pk.upd = (r.upd_ring && kk >= K_steps - H) ? r.upd_ring + so * su : nullptr;
    pk.actions = r.actions + (int64_t)kk * E;
    pk.stat_shards = r.stat_shards + (int64_t)kk * E * SSA_STAT_SHARDS * SSA_STAT_SHARD_WORDS;
    pk.spos_tiles = r.spos_tiles ? r.spos_tiles + (int64_t)kk * ntiles * 2 : nullptr;
    pk.aer_out = nullptr;
    return ring_act(ka, pk, kk, so, kk >= K_steps - H);
}
// One resident-tile kernel: NAME<PROP>(const K a, ntiles, nwork).  A wavefront loads its tile once and advances it plan.K_steps steps
// in LDS.  Written once and expanded into each kernel's body, as the tile kernels' walk is (SSA_TILE_KERNEL): process_wave has to be
// inlined straight into the kernel.
#define SSA_RESIDENT_KERNEL(NAME, K)                                                                                                          \
    template <int PROP>                                                                                                                       \
    __global__ void __launch_bounds__(64, SSA_STEP_WAVES) NAME(const K a, int ntiles, int nwork)                                              \
    {                                                                                                                                         \
        __shared__ Tiles t;                                                                                                                   \
        int lane = threadIdx.x;                                                                                                               \
        const auto plan = roll_plan(a);                                                                                                       \
        const int K_steps = plan.K_steps;                                                                                                     \
        const int64_t total = plan.total;                                                                                                     \
        TileRegs pf;                                                                                                                          \
        typedef const __attribute__((address_space(4))) K* RollArgPtr;                                                                        \
        RollArgPtr kp = (RollArgPtr)__builtin_amdgcn_kernarg_segment_ptr();                                                                   \
        for (int tile = xcd_tile((int)blockIdx.x, nwork); tile < ntiles; tile += nwork) {                                                     \
            const int64_t base = (int64_t)tile * OBJ_PER_WAVE;                                                                                \
            const int cnt = (int)((total - base) < OBJ_PER_WAVE ? (total - base) : OBJ_PER_WAVE);                                             \
            {                                                                                                                                 \
                const ssa_step_params p0 = roll_source(a, plan);                                                                              \
                wave_lds_sync();   /* the previous tile's last stores have read the tiles */                                                  \
                tile_issue(pf, p0, lane, base, cnt);                                                                                          \
                tile_commit(t, pf, lane);                                                                                                     \
                if (lane < 36) t.Q[lane] = step_of(a).c.Q[lane];   /* process_wave<.., 2> expects the process noise in place */               \
            }                                                                                                                                 \
            unsigned wave_slot;   /* the wavefront's slot on its SIMD (HW_ID bits 3:0) */                                                     \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 0, 4)" : "=s"(wave_slot));                                                     \
            for (int kk = 0; kk < K_steps; ++kk) {                                                                                            \
                rotate_issue_priority(wave_slot, (unsigned)kk);                                                                               \
                asm volatile("" : "+s"(kp));      /* per step, as per tile in the tile kernels: nothing carried around the loop */            \
                asm volatile("" : "+v"(lane));                                                                                                \
                const K& ka = *(const K*)kp;                                                                                                  \
                ssa_step_params pk;                                                                                                           \
                auto act = roll_act(plan, ka, pk, kk, ntiles);                                                                                \
                process_wave<PROP, 2>(t, step_of(ka).c, pk, lane, base + (lane >> 4), (lane >> 4) < cnt, base, cnt, pf, 0, 0, tile, act);     \
                wave_lds_sync();                                                                                                              \
            }                                                                                                                                 \
        }                                                                                                                                     \
    }
SSA_RESIDENT_KERNEL(rollout_kernel, RollK)                  // an env's schedule (ssa_env_rollout_f64)
SSA_RESIDENT_KERNEL(rollout_sensors_kernel, RollSensK)      // a sensor network's (ssa_env_rollout_sensors_f64)

// Forecast: the lookahead of a sensor network at each of H consecutive steps, every sensor idle in between, in ONE launch
// (ssa_forecast_sensors_f64).  The third resident-tile kernel: a wavefront loads its tile once and runs H predicts on it with state,
// covariance, truth and status resident in LDS -- what the passes of ActLookSensors leave in t.X / t.P IS what an idle step would have
// stored -- and writes nothing but slab h of the outputs.  No ring, no statistics, no records: the caller's state is only read -- the
// tile comes from the caller's block, and step h's block differs from it in the time alone.
struct ForeSensK {   // ONE kernel argument (see RollK)
    StepK k;
    ssa_sensor_params s;
    ssa_forecast_params f;
};
SSA_DEV const StepK& step_of(const ForeSensK& a) { return a.k; }
struct ForePlan {   // (no ring: the steps and the objects)
    int K_steps;
    int64_t total;
};
SSA_DEV ForePlan roll_plan(const ForeSensK& a) { return ForePlan{a.f.n_steps, a.k.p.n_obj}; }
SSA_DEV ssa_step_params roll_source(const ForeSensK& a, ForePlan) { return a.k.p; }
SSA_DEV ActForecastSensors roll_act(ForePlan, const ForeSensK& ka, ssa_step_params& pk, int h, int)
{
    pk = ka.k.p;
    pk.time_offset = ka.k.p.time_offset + h;
    return ActForecastSensors{{}, &ka.f.out, &ka.s, h};   // (pointers into the segment: kernarg_opaque in process_wave)
}
SSA_RESIDENT_KERNEL(forecast_sensors_kernel, ForeSensK)
// ... in each of several envs (ssa_forecast_sensors_envs_f64): the fourth resident-tile kernel.  The tiles walk all E * m rows of the
// caller's block -- whole tiles per env with several envs (the launcher), so a tile's env is a scalar --, step h's block differs from the
// caller's in the time alone, and the outputs carry the leading [H][E] axes (ActForecastSensorEnvs::slab).
struct VecForeSensK {   // (ForeSensK's layout under a name of its own: the type selects ActForecastSensorEnvs)
    StepK k;
    ssa_sensor_params s;
    ssa_forecast_params f;
};
SSA_DEV ConstPtr<int32_t> forecast_envs_inline_time()   // (by the segment's address: the block is the kernel's first argument)
{
    return (ConstPtr<int32_t>)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(VecForeSensK, k) + offsetof(StepK, p) +
                               offsetof(ssa_step_params, inline_time));
}
SSA_DEV const StepK& step_of(const VecForeSensK& a) { return a.k; }
SSA_DEV ForePlan roll_plan(const VecForeSensK& a) { return ForePlan{a.f.n_steps, (int64_t)a.k.p.n_env * a.k.p.n_obj}; }
SSA_DEV ssa_step_params roll_source(const VecForeSensK& a, ForePlan) { return a.k.p; }
SSA_DEV ActForecastSensorEnvs roll_act(ForePlan, const VecForeSensK& ka, ssa_step_params& pk, int h, int)
{
    pk = ka.k.p;
    pk.time_offset = ka.k.p.time_offset + h;
    return ActForecastSensorEnvs{{}, &ka.f.out, &ka.s, h, ka.k.p.n_env, 0};   // (process_wave enters the tile's env)
}
SSA_RESIDENT_KERNEL(forecast_sensor_envs_kernel, VecForeSensK)
// A sensor network's schedule in each of several envs (ssa_env_rollout_sensors_envs_f64): the fifth resident-tile kernel, and the
// second combination of two existing halves -- the ring and the per-step block of the rollouts (roll_act's template as it stands)
// with the tile's env as a scalar (ActScheduleEnvs).  The tiles walk all E * m rows of the ring, whole tiles per env with several
// envs (the launcher); the block's type selects the overloads.
struct VecRollSensK {
    RollK k;
    ssa_sensor_params s;
    ssa_rollout_sensors_envs_params v;
};
SSA_DEV const RollK& roll_of(const VecRollSensK& a) { return a.k; }
SSA_DEV const StepK& step_of(const VecRollSensK& a) { return a.k.k; }
SSA_DEV Ring roll_plan(const VecRollSensK& a) { return ring_of(a.k, a.k.k.p.n_env); }
SSA_DEV ssa_step_params roll_source(const VecRollSensK& a, const Ring& g) { return roll_source(a.k, g); }
SSA_DEV ActScheduleEnvs ring_act(const VecRollSensK& a, ssa_step_params& pk, int kk, int, bool)
{
    pk.upd = nullptr;       // (the envs' action words and records are not read, as in the network's step)
    pk.actions = nullptr;
    return ActScheduleEnvs{{}, &a.s, &a.v, kk, 0, nullptr, nullptr};   // (process_wave enters the tile's env)
}
SSA_RESIDENT_KERNEL(rollout_sensor_envs_kernel, VecRollSensK)
// The dry run of B candidate schedules (ssa_dryrun_sensors_envs_f64): the sixth resident-tile kernel -- the forecast's read-only plan
// and source (the caller's block; step k's differs from it in the time alone) with the schedule's action source as a dry run
// (ActDryRunEnvs).  The tiles walk all E * n_obj rows, whole tiles per pseudo-env with several of them (the launcher).
struct DryRunK {
    StepK k;
    ssa_sensor_params s;
    ssa_dryrun_sensors_params d;
};
SSA_DEV const StepK& step_of(const DryRunK& a) { return a.k; }
SSA_DEV ForePlan roll_plan(const DryRunK& a) { return ForePlan{a.d.n_steps, (int64_t)a.k.p.n_env * a.k.p.n_obj}; }
SSA_DEV ssa_step_params roll_source(const DryRunK& a, ForePlan) { return a.k.p; }
SSA_DEV ActDryRunEnvs roll_act(ForePlan, const DryRunK& ka, ssa_step_params& pk, int kk, int)
{
    pk = ka.k.p;
    pk.time_offset = ka.k.p.time_offset + kk;
    return ActDryRunEnvs{{}, &ka.s, &ka.d, kk, 0, nullptr, nullptr, 0};   // (process_wave enters the tile's env)
}
SSA_RESIDENT_KERNEL(dryrun_sensors_kernel, DryRunK)
#undef SSA_RESIDENT_KERNEL
// The totals of a dry run's records (ssa_dryrun_totals_f64): one thread per (candidate, score column) adds the taken slots' scores in
// slot order, k outer and s inner -- one defined fp64 sum, whatever the launch's shape.
__global__ void __launch_bounds__(64) dryrun_totals_kernel(const double* __restrict__ rec, int n_env, int n_steps, int n_sensor,
                                                           double* __restrict__ total)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= (int64_t)n_env * SSA_LOOK_NSCORE) return;
    const int b = (int)(i / SSA_LOOK_NSCORE), c = (int)(i - (int64_t)b * SSA_LOOK_NSCORE);
    double t = 0.0;
    for (int k = 0; k < n_steps; ++k)
        for (int s = 0; s < n_sensor; ++s) {
            const double* r = rec + (((int64_t)k * n_env + b) * n_sensor + s) * SSA_DRY_STRIDE;
            if (r[SSA_DRY_TAKEN] != 0.0) t += r[SSA_DRY_SCORE + c];
        }
    total[i] = t;
}
// The gathered block of a vector dry run (ssa_dryrun_gather_f64): output row q of the E * B * W takes the 48 doubles and the status
// word of one source row.  A row is 24 pieces of 16 bytes (3 of x_true, 3 of x, 18 of P: the row strides of 48 and 288 bytes keep
// every piece aligned) and one word: half a wavefront per row, one lane per piece -- lanes 0 .. 23 a piece each, lane 24 the status
// word, lane 25 of a candidate's first row its time word, the rest idle -- so a wavefront holds two whole rows and a block eight.
// Every lane of a row forms the same source row from the same two or three words (the id, the candidate's first id, the table's
// entry): broadcast loads.  The indices are brought into range before they address anything.
#define SSA_GATHER_ROWS 8     // rows per block of 256 lanes
__global__ void __launch_bounds__(32 * SSA_GATHER_ROWS) dryrun_gather_kernel(const ssa_dryrun_gather_params g)
{
    const int lane = threadIdx.x & 31;
    const int64_t q = (int64_t)blockIdx.x * SSA_GATHER_ROWS + (threadIdx.x >> 5);
    const int64_t W = g.n_rows, m = g.n_obj;
    if (q >= (int64_t)g.n_env * g.n_cand * W || lane > 25) return;
    // (the launcher keeps every row count below 2^31: 32-bit divisions)
    const int64_t cand = (uint32_t)q / (uint32_t)g.n_rows;
    const int64_t e = (uint32_t)cand / (uint32_t)g.n_cand;
    if (lane == 25) {
        if (q == cand * W) g.time_out[cand] = g.env_time[e];
        return;
    }
    int64_t j = g.ids[q];
    if (j < 0 || j >= m) {      // padding: the candidate's first object, object 0 for an all-idle candidate
        j = g.ids[cand * W];
        j = j < 0 ? 0 : j >= m ? m - 1 : j;
    }
    int64_t r = e * m + j;
    if (g.slot_of) {
        r = g.slot_of[r];
        r = r < 0 ? 0 : r >= g.n_env * m ? g.n_env * m - 1 : r;
    }
    if (lane == 24) {
        g.status_out[q] = g.status_in[r];
        return;
    }
    const double* src;
    double* dst;
    if (lane < 3) {
        src = g.x_true_in + r * 6 + 2 * lane;
        dst = g.x_true_out + q * 6 + 2 * lane;
    } else if (lane < 6) {
        src = g.x_in + r * 6 + 2 * (lane - 3);
        dst = g.x_out + q * 6 + 2 * (lane - 3);
    } else {
        src = g.P_in + r * 36 + 2 * (lane - 6);
        dst = g.P_out + q * 36 + 2 * (lane - 6);
    }
    *reinterpret_cast<double2*>(dst) = *reinterpret_cast<const double2*>(src);
}
// grid (n_steps, n_env): folds step k's shard set into the statistics slot of step k -- when that slot still
// belongs to step k at the end of the rollout (the last `history` steps) -- and clears it
__global__ void __launch_bounds__(64) rollout_fold_kernel(unsigned long long* __restrict__ shards, double* __restrict__ stats_ring,
                                                          int n_env, int n_steps, int slot_out, int history,
                                                          const unsigned long long* __restrict__ spos, int64_t n_obj, int64_t ntiles)
{
    const int kk = blockIdx.x, e = blockIdx.y;
    const int so = (slot_out + kk) % history;
    double* dst = (kk >= n_steps - history) ? stats_ring + (int64_t)so * n_env * SSA_STAT_STRIDE : nullptr;
    fold_stat_shards(shards + (int64_t)kk * n_env * SSA_STAT_SHARDS * SSA_STAT_SHARD_WORDS, dst, e, threadIdx.x,
                     spos ? spos + (int64_t)kk * ntiles * 2 : nullptr, n_obj);
}
// ... and for ssa_env_rollout_sensors_envs_f64, same grid: step k's shard set folded into stats_out[k] -- every step's statistics,
// whatever the history -- and copied into the statistics ring's slot where step k still owns it at the end (lane 0 wrote every word of
// the block: it copies what it wrote)
__global__ void __launch_bounds__(64) rollout_fold_steps_kernel(unsigned long long* __restrict__ shards, double* stats_out, double* stats_ring,
                                                                int n_env, int n_steps, int slot_out, int history,
                                                                const unsigned long long* __restrict__ spos, int64_t n_obj, int64_t ntiles)
{
    const int kk = blockIdx.x, e = blockIdx.y;
    double* dst = stats_out + (int64_t)kk * n_env * SSA_STAT_STRIDE;
    fold_stat_shards(shards + (int64_t)kk * n_env * SSA_STAT_SHARDS * SSA_STAT_SHARD_WORDS, dst, e, threadIdx.x,
                     spos ? spos + (int64_t)kk * ntiles * 2 : nullptr, n_obj);
    if (threadIdx.x == 0 && kk >= n_steps - history) {
        const unsigned long long* w = reinterpret_cast<const unsigned long long*>(dst + (int64_t)e * SSA_STAT_STRIDE);
        unsigned long long* ring = reinterpret_cast<unsigned long long*>(stats_ring + ((int64_t)((slot_out + kk) % history) * n_env + e) * SSA_STAT_STRIDE);
#pragma unroll
        for (int q = 0; q < SSA_STAT_STRIDE; ++q) ring[q] = w[q];
    }
}

// Post kernel, grid (nparts, n_env) x 256 threads, launched when a payload or the exact statistics are wanted:
// (1) the (az, el, range, trace P) observation block O4 of this block's slice (aer_out); (2) the statistics: the
// fold of the step kernel's shards in the first wavefront, or -- without stat_shards -- this block's slice of the
// exact reduction (arg-max sigma_pos included), one StatAcc per block for reward_final_kernel.
constexpr int POST_T = 256, POST_ILP = 4;
template <int PROP>
__global__ void __launch_bounds__(POST_T) step_post_kernel(const StepK k, StatAcc* __restrict__ parts, int nparts)
{
    __shared__ StatAcc part[POST_T / 64];
    const ssa_consts& C = k.c;
    const ssa_step_params& p = k.p;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int e = blockIdx.y;
    const int64_t m = p.n_obj;
    StatAcc acc = stat_identity();
    if (p.aer_out) {
        for (int64_t i = (int64_t)blockIdx.x * POST_T + tid; i < m; i += (int64_t)nparts * POST_T) {
            const int64_t obj = (int64_t)e * m + i;
            aer_obs_row(p.x_out + obj * 6, p.P_out + obj * 36, p, C, e, obj);
        }
    }
    if (p.stats) {
        const double* dpos = p.metrics + ((int64_t)e * 4 + 0) * m;
        const double* spos = p.metrics + ((int64_t)e * 4 + 2) * m;
        const int32_t* st = p.status + (int64_t)e * m;
        for (int64_t b0 = (int64_t)blockIdx.x * POST_T * POST_ILP; b0 < m; b0 += (int64_t)nparts * POST_T * POST_ILP) {
            double dp[POST_ILP], sp[POST_ILP];
            int sv[POST_ILP];
#pragma unroll
            for (int q = 0; q < POST_ILP; ++q) {
                int64_t i = b0 + (int64_t)q * POST_T + tid;
                bool in = i < m;
                dp[q] = in ? dpos[i] : 0.0;
                sp[q] = in ? spos[i] : -2.0;
                sv[q] = in ? st[i] : 0;
            }
#pragma unroll
            for (int q = 0; q < POST_ILP; ++q) {
                int64_t i = b0 + (int64_t)q * POST_T + tid;
                if (i < m) {
                    if (dp[q] != dp[q]) acc.mx_nan = 1; else acc.mx = fmax(acc.mx, dp[q]);
                    acc.c4 += dp[q] < 1e4;
                    acc.c7 += dp[q] < 1e7;
                    acc.nf += sv[q] != 0;
                    bool better = acc.sm_nan ? false : ((sp[q] != sp[q]) ? true : (sp[q] > acc.sm || (sp[q] == acc.sm && i < acc.arg)));
                    if (better) { acc.sm = sp[q]; acc.arg = i; acc.sm_nan = (sp[q] != sp[q]); }
                }
            }
        }
        acc = stat_wave_reduce(acc);
        if (lane == 0) part[w] = acc;
        __syncthreads();
        if (tid == 0) {
            StatAcc r = part[0];
            for (int q = 1; q < POST_T / 64; ++q) stat_merge(r, part[q]);
            parts[(int64_t)e * nparts + blockIdx.x] = r;
        }
    }
}


// ------------------------------------------------------------------------------------------
// O3: per-env reward statistics
// Two small launches: `reward_partial_kernel` spreads the 20-byte-per-object read over many CUs
// (a single CU only pulls ~24 GB/s, MI355X_MICROARCH.md) and leaves one StatAcc per block;
// `reward_final_kernel` folds those.  The kernel boundary orders the two, no device-scope fence.
constexpr int STAT_T = 256, STAT_ILP = 4, STAT_MAX_PARTS = 1024;

__global__ void __launch_bounds__(STAT_T) reward_partial_kernel(const double* __restrict__ metrics,
                                                                const int32_t* __restrict__ status,
                                                                StatAcc* __restrict__ parts, int64_t m, int nparts)
{
    const int e = blockIdx.y, t = threadIdx.x;
    const double* dpos = metrics + ((int64_t)e * 4 + 0) * m;
    const double* spos = metrics + ((int64_t)e * 4 + 2) * m;
    const int32_t* st = status + (int64_t)e * m;
    StatAcc a = stat_identity();
    for (int64_t base = (int64_t)blockIdx.x * STAT_T * STAT_ILP; base < m; base += (int64_t)nparts * STAT_T * STAT_ILP) {
        double dp[STAT_ILP], sp[STAT_ILP];
        int sv[STAT_ILP];
#pragma unroll
        for (int k = 0; k < STAT_ILP; ++k) {
            int64_t i = base + (int64_t)k * STAT_T + t;
            bool in = i < m;
            dp[k] = in ? dpos[i] : 0.0;
            sp[k] = in ? spos[i] : -2.0;
            sv[k] = in ? st[i] : 0;
        }
#pragma unroll
        for (int k = 0; k < STAT_ILP; ++k) {
            int64_t i = base + (int64_t)k * STAT_T + t;
            if (i < m) {
                if (dp[k] != dp[k]) a.mx_nan = 1; else a.mx = fmax(a.mx, dp[k]);
                a.c4 += dp[k] < 1e4;
                a.c7 += dp[k] < 1e7;
                a.nf += sv[k] != 0;
                bool better = a.sm_nan ? false : ((sp[k] != sp[k]) ? true : (sp[k] > a.sm));
                if (better) { a.sm = sp[k]; a.arg = i; a.sm_nan = (sp[k] != sp[k]); }
            }
        }
    }
    a = stat_wave_reduce(a);
    __shared__ StatAcc part[STAT_T / 64];
    if ((t & 63) == 0) part[t >> 6] = a;
    __syncthreads();
    if (t == 0) {
        StatAcc r = part[0];
        for (int w = 1; w < STAT_T / 64; ++w) stat_merge(r, part[w]);
        parts[(int64_t)e * nparts + blockIdx.x] = r;
    }
}
__global__ void __launch_bounds__(64) reward_final_kernel(const StatAcc* __restrict__ parts, double* __restrict__ stats, int nparts)
{
    const int e = blockIdx.x, t = threadIdx.x;
    StatAcc a = stat_identity();
    for (int i = t; i < nparts; i += 64) stat_merge(a, parts[(int64_t)e * nparts + i]);
    a = stat_wave_reduce(a);
    if (t == 0 && stats) {
        double* o = stats + (int64_t)e * SSA_STAT_STRIDE;
        o[SSA_STAT_MAX_DPOS] = a.mx_nan ? __builtin_nan("") : a.mx;
        o[SSA_STAT_CNT_LT_1E4] = (double)a.c4;
        o[SSA_STAT_CNT_LT_1E7] = (double)a.c7;
        o[SSA_STAT_ARGMAX_SPOS] = (double)a.arg;
        o[SSA_STAT_N_FAILED] = (double)a.nf;
        o[SSA_STAT_MAX_SPOS] = a.sm_nan ? __builtin_nan("") : a.sm;
        o[6] = 0.0; o[7] = 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// single-operator kernels (one lane per item)
template <int PROP>
__global__ void propagate_kernel(const double* __restrict__ xin, double* __restrict__ xout, int64_t n, double dt)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = i < n;
    int64_t ii = ok ? i : 0;  // keep the wave convergent for the __all() in the Newton loops
    double x[6], o[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) x[c] = xin[ii * 6 + c];
    kepler_step<PROP>(x, dt, o);
    if (ok) {
#pragma unroll
        for (int c = 0; c < 6; ++c) xout[i * 6 + c] = o[c];
    }
}
__global__ void propagate_hybrid_kernel(const double* __restrict__ xin, double* __restrict__ xout, int64_t n, double dt)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = i < n;
    int64_t ii = ok ? i : 0;  // keep the wave convergent for the __all() in the solver loops
    double x[6], o[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) x[c] = xin[ii * 6 + c];
    bool fast = kepler_hybrid_fast(x, dt, o);
    if (__any(!fast)) {       // the step kernels' tiers: strong-hyperbolic inline, the rest out of line
        if (!fast) fast = kepler_conic_lean<0, true>(x, dt, o);
    }
    if (__any(!fast)) {
        if (!fast) {
            Vec6 si;
#pragma unroll
            for (int c = 0; c < 6; ++c) si.v[c] = x[c];
            Vec6 oo = kepler_beyond_series_tagged<0>(si, dt);
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = oo.v[c];
        }
    }
    if (ok) {
#pragma unroll
        for (int c = 0; c < 6; ++c) xout[i * 6 + c] = o[c];
    }
}
__global__ void propagate_j2_kernel(const double* __restrict__ xin, double* __restrict__ xout, int64_t n, double dt, J2Params q)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x[6], o[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) x[c] = xin[i * 6 + c];
    propagate_j2_rk4(x, dt, q, o);
#pragma unroll
    for (int c = 0; c < 6; ++c) xout[i * 6 + c] = o[c];
}
__global__ void elements_kernel(const double* __restrict__ xin, double* __restrict__ coe, int64_t n, double dt)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = i < n;
    int64_t ii = ok ? i : 0;
    double x[6], o[6], dg[8];
#pragma unroll
    for (int c = 0; c < 6; ++c) x[c] = xin[ii * 6 + c];
    kepler_elements(x, dt, o, dg);
    if (ok) {
#pragma unroll
        for (int c = 0; c < 8; ++c) coe[i * 8 + c] = dg[c];
    }
}
__global__ void cholesky_kernel(const double* __restrict__ A, double* __restrict__ U, int32_t* __restrict__ rung, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a[21], u[21];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) a[tri(r, c)] = A[i * 36 + r * 6 + c];
    // scipy.linalg.cholesky checks the WHOLE matrix for non-finite entries
    bool finite = true;
    for (int t = 0; t < 36; ++t) finite = finite && (fabs(A[i * 36 + t]) <= 1.79769313486231570e308);
    int rg = finite ? robust_chol6(a, u) : 16;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) U[i * 36 + r * 6 + c] = (c >= r && rg != 16) ? u[tri(r, c)] : 0.0;
    rung[i] = rg;
}
// U2 as the fused step kernels run it: one wavefront per four matrices, the row-distributed ladder itself (robust_chol_row_lds) plus,
// for the record, WHICH rungs factorise in that arithmetic (chol_lane_ok per lane = per rung; bit 16 = the plain attempt).
__global__ void __launch_bounds__(64) ladder_probe_kernel(const double* __restrict__ A, double scale, int32_t* __restrict__ rung_out,
                                                          int32_t* __restrict__ mask_out, double* __restrict__ U, int64_t n)
{
    __shared__ Tiles t;
    const int lane = threadIdx.x, g = lane >> 4, l = lane & 15;
    const int64_t base = (int64_t)blockIdx.x * OBJ_PER_WAVE;
    const int cnt = (int)((n - base) < OBJ_PER_WAVE ? (n - base) : OBJ_PER_WAVE);
    for (int i = lane; i < OBJ_PER_WAVE * 36; i += 64) {
        const int gg = i / 36;
        t.P[i] = (gg < cnt) ? A[base * 36 + i] : ((i % 36) % 7 == 0 ? 1.0 : 0.0);     // (rows beyond n: the identity)
        t.UA[i] = 0.0;
    }
    wave_lds_sync();
    const int rung = robust_chol_row_lds(t, scale, g, l);
    wave_lds_sync();
    const double* Pg = &t.P[g * 36];
    bool finite = true;
    for (int i = 0; i < 36; ++i) finite = finite && (fabs(Pg[i]) <= 1.79769313486231570e308);
    const bool okl = finite && chol_lane_ok(Pg, scale, JITTER[l]);
    const bool ok0 = finite && chol_lane_ok(Pg, scale, 0.0);
    const unsigned m16 = (unsigned)((__ballot(okl) >> (g * 16)) & 0xFFFFull);
    if (g < cnt) {
        if (l == 0) {
            rung_out[base + g] = rung;
            mask_out[base + g] = (int32_t)(m16 | (ok0 ? 0x10000u : 0u));
        }
        if (U) for (int i = l; i < 36; i += 16) U[(base + g) * 36 + i] = (rung != 16) ? t.UA[g * 36 + i] : 0.0;
    }
}
__global__ void sigma_points_kernel(const double* __restrict__ x, const double* __restrict__ P, double scale,
                                    double* __restrict__ sig, int32_t* __restrict__ fail, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a[21], u[21];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) a[tri(r, c)] = scale * P[i * 36 + r * 6 + c];
    int rg = robust_chol6(a, u);
    fail[i] = rg == 16 ? SSA_ST_PREDICT_LINALG : SSA_ST_OK;
    double xx[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        xx[c] = x[i * 6 + c];
        sig[i * 78 + c] = xx[c];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double uv = (c >= r && rg != 16) ? u[tri(r, c)] : 0.0;
            sig[i * 78 + (r + 1) * 6 + c] = xx[c] + uv;
            sig[i * 78 + (r + 7) * 6 + c] = xx[c] - uv;
        }
}
struct GeoK {
    double enu[9];
    double obs[3];
    double obs_limit;
    double Wi, sum_wm_m1;
};
__global__ void hx_kernel(const double* __restrict__ x, int64_t stride, const double* __restrict__ M, GeoK g,
                          double* __restrict__ z, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double Mm[9], xx[3], zz[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) Mm[c] = M[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) xx[c] = x[i * stride + c];
    hx_aer(xx, Mm, g.enu, g.obs, zz);
#pragma unroll
    for (int c = 0; c < 3; ++c) z[i * 3 + c] = zz[c];
}
__global__ void mean_z_kernel(const double* __restrict__ sig, GeoK g, double* __restrict__ zp, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double u0[3], acc[3] = {0.0, 0.0, 0.0}, a[3], um[3], out[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = sig[i * 39 + c];
    aer2uvw(a, u0);
    for (int s = 1; s < 13; ++s) {
        double u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = sig[i * 39 + s * 3 + c];
        aer2uvw(a, u);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += u[c] - u0[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) um[c] = u0[c] + (g.sum_wm_m1 * u0[c] + g.Wi * acc[c]);
    uvw2aer(um, out);
#pragma unroll
    for (int c = 0; c < 3; ++c) zp[i * 3 + c] = out[c];
}
__global__ void residual_kernel(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ c, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double aa[3] = {a[i * 3], a[i * 3 + 1], a[i * 3 + 2]}, bb[3] = {b[i * 3], b[i * 3 + 1], b[i * 3 + 2]}, cc[3];
    residual_z_aer(aa, bb, cc);
    c[i * 3] = cc[0]; c[i * 3 + 1] = cc[1]; c[i * 3 + 2] = cc[2];
}
// (tix: optional device word; with it M is the TABLE and the matrix is row (tix[0] + tix_off) % n_time -- for callers inside a captured
// graph, whose time index lives on the device)
SSA_DEV const double* matrix_at(const double* M, const int32_t* tix, int32_t tix_off, int32_t n_time)
{
    if (!tix) return M;
    const int t = tix[0] + tix_off;
    return M + (int64_t)((n_time > 0) ? ((t % n_time) + n_time) % n_time : 0) * 9;
}
__global__ void visible_kernel(const double* __restrict__ x, const double* __restrict__ M0, GeoK g,
                               uint8_t* __restrict__ mask, double* __restrict__ el, int64_t n, const int32_t* __restrict__ tix, int32_t tix_off, int32_t n_time)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* M = matrix_at(M0, tix, tix_off, n_time);
    double Mm[9], xx[3], zz[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) Mm[c] = M[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) xx[c] = x[i * 6 + c];
    hx_aer(xx, Mm, g.enu, g.obs, zz);
    mask[i] = zz[1] >= g.obs_limit ? 1 : 0;
    if (el) el[i] = zz[1];
}
// the sunlit rule of the sensor kernels (sunlit_cylinder) for n true states against ONE row of a Sun table: a lane per object
__global__ void sunlit_kernel(const double* __restrict__ x, const double* __restrict__ sun_row, double shadow_radius,
                              uint8_t* __restrict__ mask, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double r[3] = {x[i * 6], x[i * 6 + 1], x[i * 6 + 2]}, s[3] = {sun_row[0], sun_row[1], sun_row[2]};
    mask[i] = sunlit_cylinder(r, s, shadow_radius) ? 1 : 0;
}
// the line-of-sight rule of a moving sensor (los_clear, on the vector hx_aer_enu forms) for n true states against ONE trans row and ONE
// site row: a lane per object
__global__ void los_kernel(const double* __restrict__ x, const double* __restrict__ trans_row, const double* __restrict__ site_row,
                           double limb_radius, uint8_t* __restrict__ mask, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double M[9], o[3], d[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = trans_row[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = site_row[9 + k];
    const double r[3] = {x[i * 6], x[i * 6 + 1], x[i * 6 + 2]};
    observer_to_object(r, M, o, d);
    mask[i] = los_clear(d, o, limb_radius) ? 1 : 0;
}
__global__ void observe_kernel(const double* __restrict__ xt, const double* __restrict__ x, const double* __restrict__ P,
                               double* __restrict__ obs, double* __restrict__ met, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double xx[6], dg[6], tt[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        xx[c] = x[i * 6 + c];
        tt[c] = xt[i * 6 + c];
        dg[c] = P[i * 36 + 7 * c];
        obs[i * 12 + c] = xx[c];
        obs[i * 12 + 6 + c] = dg[c];
    }
    double a0 = xx[0] - tt[0], a1 = xx[1] - tt[1], a2 = xx[2] - tt[2];
    double b0 = xx[3] - tt[3], b1 = xx[4] - tt[4], b2 = xx[5] - tt[5];
    met[i] = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
    met[n + i] = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    met[2 * n + i] = sqrt(dg[0] + dg[1] + dg[2]);
    met[3 * n + i] = sqrt(dg[3] + dg[4] + dg[5]);
}
__global__ void aer_obs_kernel(const double* __restrict__ x, const double* __restrict__ P, const double* __restrict__ M,
                               GeoK g, double* __restrict__ out, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double Mm[9], xx[3], zz[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) Mm[c] = M[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) xx[c] = x[i * 6 + c];
    hx_aer(xx, Mm, g.enu, g.obs, zz);
    double tr = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) tr += P[i * 36 + 7 * c];
    double v[4] = {zz[0], zz[1], zz[2], tr};
#pragma unroll
    for (int c = 0; c < 4; ++c) out[i * 4 + c] = (fabs(v[c]) <= 1.79769313486231570e308) ? v[c] : 0.001;
}

// agents.py score arrays + visibility (one lane per object).  sc[0..3] = trace P | log(det P_cur / det P_prev) | |dpos| | |dvel|;
// WANT selects what is evaluated (bit k = row k, bit 4 = visibility) -- the two log-determinants are the expensive part.
// log det through the (plain) Cholesky factor: det > 0 for the covariances the filter keeps; anything else gives NaN, which
// the arg-max skips
SSA_DEV double logdet_chol(const double (&A)[21])
{
    double U[21];
    double ld = __builtin_nan("");
    if (chol6_upper(A, 0.0, U)) {
        // det P = (prod U_ii)^2: ONE logarithm of the product (as the reference: np.log(np.linalg.det(P)), agents.py:24) instead of
        // six of the factors -- the diagonal of the factor is sqrt-sized (1e-3 .. 1e6), its product far from over- / underflow
        double pr = U[tri(0, 0)];
#pragma unroll
        for (int c = 1; c < 6; ++c) pr *= U[tri(c, c)];
        ld = 2.0 * log(pr);
    }
    return ld;
}
// the scores from values in registers: xt / x = true and estimated state, A = upper triangle of P_cur, ld_prev = logdet_chol of
// P_prev (NaN when there is none); *ld_cur (optional) receives logdet_chol(P_cur) -- the closed-loop kernel hands it on as the
// next step's ld_prev instead of factorising the same matrix twice.  M = GCRS -> ITRS matrix of the step.
template <int WANT>
SSA_DEV bool agent_score_core(const double (&xt)[6], const double (&x)[6], const double (&A)[21], double ld_prev,
                              const double* __restrict__ M, const GeoK& g, double* sc, double* ld_cur)
{
    if (WANT & 1) {
        double tr = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) tr += A[tri(c, c)];
        sc[0] = tr;
    }
    if (WANT & 2) {
        const double ld_c = logdet_chol(A);
        if (ld_cur) *ld_cur = ld_c;
        sc[1] = ld_c - ld_prev;
    }
    if (WANT & 12) {
        double d[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) d[c] = x[c] - xt[c];
        sc[2] = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        sc[3] = sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
    }
    bool vis = true;
    if (WANT & 16) {
        double Mm[9], xx[3] = {xt[0], xt[1], xt[2]}, zz[3];
#pragma unroll
        for (int c = 0; c < 9; ++c) Mm[c] = M[c];
        hx_aer(xx, Mm, g.enu, g.obs, zz);
        vis = zz[1] >= g.obs_limit;
    }
    return vis;
}
template <int WANT>
SSA_DEV bool agent_score_rows(const double* __restrict__ xt, const double* __restrict__ x, const double* __restrict__ Pc,
                              const double* __restrict__ Pp, const double* __restrict__ M, const GeoK& g, int64_t i, double* sc)
{
    double A[21] = {0.0}, xtv[6] = {0.0}, xv[6] = {0.0};
    if (WANT & 3) {
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) A[tri(r, c)] = Pc[i * 36 + r * 6 + c];
    }
    double ld_p = __builtin_nan("");
    if ((WANT & 2) && Pp) {
        double B[21];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) B[tri(r, c)] = Pp[i * 36 + r * 6 + c];
        ld_p = logdet_chol(B);
    }
    if (WANT & 12) {
#pragma unroll
        for (int c = 0; c < 6; ++c) xv[c] = x[i * 6 + c];
    }
    if (WANT & 28) {
#pragma unroll
        for (int c = 0; c < 6; ++c) xtv[c] = xt[i * 6 + c];
    }
    return agent_score_core<WANT>(xtv, xv, A, ld_p, M, g, sc, nullptr);
}
__global__ void agent_scores_kernel(const double* __restrict__ xt, const double* __restrict__ x, const double* __restrict__ Pc,
                                    const double* __restrict__ Pp, const double* __restrict__ M0, GeoK g,
                                    double* __restrict__ scores, uint8_t* __restrict__ mask, int64_t n, const int32_t* __restrict__ tix,
                                    int32_t tix_off, int32_t n_time)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* M = mask ? matrix_at(M0, tix, tix_off, n_time) : M0;
    double sc[4];
    bool vis;
    if (mask) vis = agent_score_rows<31>(xt, x, Pc, Pp, M, g, i, sc);
    else vis = agent_score_rows<15>(xt, x, Pc, Pp, M, g, i, sc);
    scores[i] = sc[0];
    scores[n + i] = sc[1];
    scores[2 * n + i] = sc[2];
    scores[3 * n + i] = sc[3];
    if (mask) mask[i] = vis ? 1 : 0;
}

// ---- closed loop on the device: the reference's heuristic agents (agents.py:7-81) choose the next action
// from the state the step just wrote; here that choice never leaves the GPU.  agent_partial_kernel scores one object per
// lane and reduces each block to its first maximum; agent_final_kernel folds the blocks of an env and writes the action
// word the NEXT ssa_env_step_f64 reads (a fallback action when nothing is visible: the reference samples at random).
struct AgentPart { double best; long long arg; };
SSA_DEV void agent_merge(double& b, long long& a, double b2, long long a2)
{
    const bool take = a2 >= 0 && (a < 0 || b2 > b || (b2 == b && a2 < a));
    if (take) { b = b2; a = a2; }
}
constexpr int AGENT_T = 256;
template <int KIND>
__global__ void __launch_bounds__(AGENT_T) agent_partial_kernel(const double* __restrict__ xt, const double* __restrict__ x,
                                                                const double* __restrict__ Pc, const double* __restrict__ Pp,
                                                                const double* __restrict__ trans, const int32_t* __restrict__ env_time,
                                                                int32_t time_offset, int32_t n_time, GeoK g,
                                                                AgentPart* __restrict__ parts, int64_t n, const int32_t* __restrict__ ids)
{
    // (ids: a storage layout's table -- ssa_step_params.obj_ids -- or NULL: the candidate is named as the CALLER numbers it, and the first
    // maximum is the one with the lowest such index)
    const int e = blockIdx.y, t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * AGENT_T + t;
    double best = 0.0;
    long long arg = -1;
    if (i < n) {
        const int64_t obj = (int64_t)e * n + i;
        const int tix = env_time[e] + time_offset;
        const double* M = trans + (int64_t)((n_time > 0) ? tix % n_time : 0) * 9;
        double sc[4];
        constexpr int ROW = (KIND == SSA_AGENT_SHANNON) ? 1 : (KIND == SSA_AGENT_POS_ERROR) ? 2 : (KIND == SSA_AGENT_VEL_ERROR) ? 3 : 0;
        constexpr int WANT = (ROW == 0 ? 1 : ROW == 1 ? 2 : 12) | (KIND == SSA_AGENT_NAIVE_GREEDY ? 0 : 16);
        const bool vis = agent_score_rows<WANT>(xt, x, Pc, Pp, M, g, obj, sc);
        const double v = sc[ROW];
        if (vis && v == v) { best = v; arg = ids ? (long long)ids[i] : (long long)i; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double b2 = __shfl_down(best, off, 64);
        const long long a2 = __shfl_down(arg, off, 64);
        agent_merge(best, arg, b2, a2);
    }
    __shared__ AgentPart part[AGENT_T / 64];
    if ((t & 63) == 0) { part[t >> 6].best = best; part[t >> 6].arg = arg; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < AGENT_T / 64; ++w) agent_merge(best, arg, part[w].best, part[w].arg);
        AgentPart r;
        r.best = best; r.arg = arg;
        parts[(int64_t)e * gridDim.x + blockIdx.x] = r;
    }
}
__global__ void __launch_bounds__(64) agent_final_kernel(const AgentPart* __restrict__ parts, int nparts,
                                                         const int32_t* __restrict__ fallback, int32_t* __restrict__ action_out,
                                                         int64_t* __restrict__ pick_out)
{
    const int e = blockIdx.x, t = threadIdx.x;
    double best = 0.0;
    long long arg = -1;
    for (int i = t; i < nparts; i += 64) agent_merge(best, arg, parts[(int64_t)e * nparts + i].best, parts[(int64_t)e * nparts + i].arg);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double b2 = __shfl_down(best, off, 64);
        const long long a2 = __shfl_down(arg, off, 64);
        agent_merge(best, arg, b2, a2);
    }
    if (t == 0) {
        action_out[e] = (arg >= 0) ? (int32_t)arg : (fallback ? fallback[e] : -1);
        if (pick_out) { pick_out[2 * e] = arg; pick_out[2 * e + 1] = __double_as_longlong(best); }
    }
}

// ------------------------------------------------------------------------------------------
// Closed loop in ONE launch (the reference's `a = agent(obs, env); obs, r, done, _ = env.step(a)` of
// run_environment.py:26-29 for its greedy agents, agents.py:7-81).  As in rollout_kernel a wavefront keeps its four objects'
// state in LDS across the K steps and writes every step's outputs to that step's ring slot; in addition the NEXT step's
// action is decided inside the launch:
//   * after step k every compute wavefront scores its objects (agent_score_core: the arithmetic of ssa_agent_select_f64, so
//     the choices are identical to the multi-launch loop's), merges them with its share of the step's reward statistics into
//     one 32-byte part, stores it and bumps its GROUP's arrival counter (64 wavefronts per group) -- and goes on with step
//     k + 1's predicts, which do not depend on the action;
//   * one SERVICE wavefront per group (extra workgroups of the same launch, no objects of their own) polls that counter, folds
//     the group's 64 parts and bumps the launch's counter; one more service wavefront polls that one, folds the groups, writes
//     the action (or the caller's fallback when nothing qualifies) and the step's statistics, and publishes (decision number,
//     action) in every group's flag word;
//   * a compute wavefront reads its group's flag only where the update needs it (ActLate), so the decision's latency hides
//     behind the predict.
// (First version: the last wavefront to arrive did the folding.  The wavefront that runs the update arrives last, lost three
// more microseconds folding while the others were already in their next predict, so it was the last to arrive at the NEXT
// step too -- every step waited for one wavefront's predict + update + folds in series: 14.4 us per step against 10.2 without
// the wait, profiles/r03_closed_loop_timeline.txt.  Folders without objects cannot fall behind.)
// No compute wavefront can be two steps ahead (the update of step k + 1 needs every part of step k), hence two sets of parts,
// indexed by the step's parity, suffice; the counters only ever grow.  All words that cross wavefronts are agent-scope atomics
// (coherent across the XCDs' L2s); a store is ordered before the atomic that announces it by waiting for its
// acknowledgement (s_waitcnt vmcnt(0)).  Every wait is bounded: a wavefront that times out publishes the abort generation in
// every flag and all wavefronts leave -- the grid drains whatever happens.  Needs every wavefront resident at once (one tile
// per compute wavefront + the service wavefronts): the launcher checks that against the occupancy the runtime reports and
// refuses otherwise.
// (skey, sarg: the part's first maximum of sigma_pos -- ordered key and object index -- for np.argmax(sigma_pos), the 'shaped' reward;
// exchanged only with SSA_LOOP_ARGMAX_SPOS (`wide`): two more words per part)
struct ClPart { double best; long long arg; unsigned long long mx, cnt, skey, sarg; };   // cnt: [< 1e4] | [< 1e7] << 21 | [failed] << 42
constexpr int CL_PART_WORDS = 8;      // words between parts (64 bytes: six used)
SSA_DEV void cl_merge(ClPart& a, const ClPart& b)
{
    agent_merge(a.best, a.arg, b.best, b.arg);
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    a.cnt += b.cnt;
    if (b.skey > a.skey || (b.skey == a.skey && b.sarg < a.sarg)) { a.skey = b.skey; a.sarg = b.sarg; }
}
SSA_DEV ClPart cl_identity()
{
    ClPart r;
    r.best = 0.0; r.arg = -1; r.mx = 0ull; r.cnt = 0ull; r.skey = 0ull; r.sarg = ~0ull;
    return r;
}
SSA_DEV ClPart cl_load(const unsigned long long* w, bool wide)
{
    ClPart r;
    r.best = __longlong_as_double((long long)__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    r.arg = (long long)__hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    r.mx = __hip_atomic_load(w + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    r.cnt = __hip_atomic_load(w + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    r.skey = 0ull; r.sarg = ~0ull;
    if (wide) {
        r.skey = __hip_atomic_load(w + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r.sarg = __hip_atomic_load(w + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return r;
}
SSA_DEV void cl_store(unsigned long long* w, const ClPart& v, bool wide)
{
    __hip_atomic_store(w, (unsigned long long)__double_as_longlong(v.best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 1, (unsigned long long)v.arg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 2, v.mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 3, v.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wide) {
        __hip_atomic_store(w + 4, v.skey, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(w + 5, v.sarg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// Fold over the 64 lanes, result wave-uniform.  Four DPP rotations leave every row's fold in all of its lanes, four readlanes
// combine the rows (the ds_bpermute shuffle tree this replaces took ~1.5 us per fold: 48 dependent LDS-crossbar round trips).
// The agent's "first maximum" (highest score, lowest index among equals, agent_merge) becomes two folds of integers: the
// score as an order-preserving 64-bit key (0 = no candidate), then the lowest index among the lanes that hold the maximum.
SSA_DEV unsigned long long score_key(double v)   // order-preserving; > 0 for every non-NaN double (-0 ranks as +0)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
SSA_DEV double score_of_key(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
SSA_DEV ClPart cl_wave_reduce(const ClPart& a, bool wide)
{
    const unsigned long long key = a.arg >= 0 ? score_key(a.best) : 0ull;
    const unsigned long long top = wave_fold_u64(key, OpMax());
    const unsigned long long cand = (a.arg >= 0 && key == top) ? (unsigned long long)a.arg : ~0ull;
    const unsigned long long who = wave_fold_u64(cand, OpMin());
    ClPart r;
    r.arg = top ? (long long)who : -1;
    r.best = top ? score_of_key(top) : 0.0;
    r.mx = wave_fold_u64(a.mx, OpMax());
    r.cnt = wave_fold_u64(a.cnt, OpAdd());
    r.skey = 0ull; r.sarg = ~0ull;
    if (wide) {
        r.skey = wave_fold_u64(a.skey, OpMax());
        r.sarg = wave_fold_u64((a.skey == r.skey) ? a.sarg : ~0ull, OpMin());
    }
    return r;
}
// own stores acknowledged (visible at agent scope) before what follows
SSA_DEV void cl_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// workspace layout in 8-byte words (ng = groups of 64 compute wavefronts); everything before `parts` must be zero at launch
struct ClLayout {
    int64_t flags, gcount, fcount, parts, gparts, cparts, total;
    int ng;
};
static __host__ __device__ inline ClLayout cl_layout(int nwork)
{
    ClLayout L;
    L.ng = (nwork + 63) / 64;
    L.flags = 0;                                   // [ng] x 16 words: one 128-byte line per group
    L.gcount = (int64_t)L.ng * 16;                 // [ng] x 16: arrivals so far (all steps)
    L.fcount = L.gcount + (int64_t)L.ng * 16;      // x 16: folded groups so far (all steps)
    L.parts = L.fcount + 16;                       // [2][nwork] x CL_PART_WORDS
    L.gparts = L.parts + (int64_t)2 * CL_PART_WORDS * nwork;       // [2][ng] x CL_PART_WORDS
    L.cparts = L.gparts + (int64_t)2 * CL_PART_WORDS * L.ng;       // [2] x CL_PART_WORDS: the part of the wavefront that ran the update (straight to the decision)
    L.total = L.cparts + 2 * CL_PART_WORDS;
    return L;
}

SSA_DEV void closed_loop_prescore(ActLate& a, Tiles& t, int lane, int cnt)
{
    if (a.agent == SSA_AGENT_NAIVE_GREEDY) return;       // (no visibility mask: agents.py:7)
    const int g = lane >> 4, l = lane & 15;
    if (l == 0 && g < cnt) {
        GeoK geo;
        for (int i = 0; i < 9; ++i) geo.enu[i] = a.C->enu[i];
        for (int i = 0; i < 3; ++i) geo.obs[i] = a.C->obs_itrs[i];
        geo.obs_limit = a.C->obs_limit; geo.Wi = a.C->Wi; geo.sum_wm_m1 = a.C->sum_wm_m1;
        double xt[6], x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, A[21] = {0.0}, sc[4];
#pragma unroll
        for (int c = 0; c < 6; ++c) xt[c] = t.T[g * 6 + c];
        a.vis[g] = agent_score_core<16>(xt, x, A, 0.0, a.M, geo, sc, nullptr) ? 1 : 0;
    }
}

// The wavefront that runs the update of a step announces its part last (the update is three microseconds the others do not
// have): it hands it to the deciding wavefront DIRECTLY instead of through its group's fold -- one exchange level less on the
// path decision -> update -> decision.  Who that is follows from the action alone, so everybody agrees on it: the tile of the
// selected object, or tile 0 when the action selects nobody.
// (slot_of: with a storage layout -- ssa_step_params.obj_ids -- the position of the object the caller calls `act`; NULL: the identity)
SSA_DEV int closer_tile(int act, int64_t total, const int32_t* __restrict__ slot_of = nullptr)
{
    if (!(act >= 0 && (int64_t)act < total)) return 0;
    return (slot_of ? slot_of[act] : act) >> 2;
}
SSA_DEV int block_of_tile(int tile, int n)   // inverse of xcd_tile()
{
    const int q = n >> 3, r = n & 7;
    int x = 0;
#pragma unroll
    for (int c = 1; c < 8; ++c)
        if (tile >= c * q + (c < r ? c : r)) x = c;
    return (tile - (x * q + (x < r ? x : r))) * 8 + x;
}
// bounded wait of a service wavefront: until *counter >= target (returns true), or the launch was abandoned / the wait timed
// out (false; on a timeout the abort generation has been published)
SSA_DEV bool cl_service_wait(const unsigned long long* counter, unsigned long long target, ActLate& ab)
{
    // polling at the LOWEST issue priority: the service wavefronts share their SIMDs with compute wavefronts, and a top-priority
    // polling loop took a third of those SIMDs' issue slots (the compute wavefronts next to them finished microseconds late and
    // everybody waited for them); top priority only for the fold that follows
    __builtin_amdgcn_s_setprio(0);
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        const unsigned long long v = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane_u64(v, 0) >= target) {
            __builtin_amdgcn_s_setprio(3);
            return true;
        }
        const unsigned long long f = __hip_atomic_load(ab.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)(lane_u64(f, 0) >> 32) == CL_ABORT_GEN) return false;
        if (wall_clock64() - t0 > ab.timeout) {
            ab.abort_all();
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

struct LoopK {   // ONE kernel argument (see RollK)
    StepK k;
    ssa_closed_loop_params c;
};
SSA_DEV void closed_loop_store(const LoopK* lk, Tiles& t, int lane, int kk, int64_t base, int cnt)
{
    const ssa_closed_loop_params& r = lk->c;
    const int64_t total = lk->k.p.n_obj;
    const int so = (r.slot_out + kk) % r.history;
    ssa_step_params q = lk->k.p;
    q.x_true_out = r.x_true_ring + so * total * 6;
    q.x_out = r.x_ring + so * total * 6;
    q.P_out = r.P_ring + so * total * 36;
    q.obs = r.obs_ring + so * total * 12;
    q.metrics = r.metrics_ring + so * 4 * total;
    store_tile<true>(t, q, lane, base, cnt);
}
template <int PROP>
__global__ void __launch_bounds__(64, SSA_STEP_WAVES) closed_loop_kernel(const LoopK a, int ntiles, int nwork)
{
    const StepK& k_arg = a.k;
    __shared__ Tiles t;
    __shared__ double ld_prev[OBJ_PER_WAVE];   // agent_shannon: log det of each object's covariance one step ago
    __shared__ ClPart rowpart[OBJ_PER_WAVE];
    __shared__ int vis_row[OBJ_PER_WAVE];
    int lane = threadIdx.x;
    const int64_t total = k_arg.p.n_obj;       // (one env)
    const int H = a.c.history, K = a.c.n_steps;
    const int w = (int)blockIdx.x;
    const ClLayout L = cl_layout(nwork);
    unsigned long long* const ws = (unsigned long long*)a.c.workspace;
    ActLate asrc;
    asrc.all_flags = ws + L.flags;
    asrc.err = a.c.error;
    asrc.nflags = L.ng;
    asrc.timeout = a.c.wait_ticks > 0 ? (unsigned long long)a.c.wait_ticks : CL_TIMEOUT_TICKS;
    asrc.aborted = false;
    asrc.last = -1;
    asrc.agent = a.c.agent;
    asrc.vis = vis_row;
    const bool wide = (a.c.flags & SSA_LOOP_ARGMAX_SPOS) != 0u;      // np.argmax(sigma_pos) travels with the parts

    // ---------------- service wavefronts: w in [nwork, nwork + ng) fold one group each, w == nwork + ng decides
    if (w >= nwork) {
        __builtin_amdgcn_s_setprio(3);
        const int G = w - nwork;
        if (G < L.ng) {
            const int gsize = (nwork - G * 64) < 64 ? (nwork - G * 64) : 64;
            asrc.flag = ws + L.flags + (int64_t)G * 16;
            asrc.first = a.c.actions[0];
            unsigned long long target = 0ull;   // arrivals of this group so far, all steps
            for (int kk = 0; kk < K; ++kk) {
                asrc.want = (unsigned)kk;       // this step's action says whose part bypasses the groups
                __builtin_amdgcn_s_setprio(0);
                const int act = asrc.get();
                if (asrc.aborted) return;
                const int cw = block_of_tile(closer_tile(act, total, a.c.slot_of), nwork);
                target += (unsigned long long)(gsize - ((cw >> 6) == G ? 1 : 0));
                if (!cl_service_wait(ws + L.gcount + (int64_t)G * 16, target, asrc)) return;
                const int q = kk & 1;
                ClPart me = cl_identity();
                if (lane < gsize && G * 64 + lane != cw) me = cl_load(ws + L.parts + ((int64_t)q * nwork + (int64_t)G * 64 + lane) * CL_PART_WORDS, wide);
                const ClPart red = cl_wave_reduce(me, wide);
                if (lane == 0) {
                    cl_store(ws + L.gparts + ((int64_t)q * L.ng + G) * CL_PART_WORDS, red, wide);
                    cl_stores_done();
                    __hip_atomic_fetch_add(ws + L.fcount, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            return;
        }
        asrc.flag = ws + L.flags;
        for (int kk = 0; kk < K; ++kk) {
            if (!cl_service_wait(ws + L.fcount, (unsigned long long)(kk + 1) * (unsigned long long)(L.ng + 1), asrc)) return;
            const int q = kk & 1;
            ClPart f = cl_identity();
            if (lane == 63) f = cl_load(ws + L.cparts + (int64_t)q * CL_PART_WORDS, wide);    // the update's wavefront
            for (int i0 = 0; i0 < L.ng; i0 += 128) {     // (two loads in flight per lane: 128 groups = 32 768 objects per round)
                ClPart b0 = cl_identity(), b1 = cl_identity();
                if (i0 + lane < L.ng) b0 = cl_load(ws + L.gparts + ((int64_t)q * L.ng + i0 + lane) * CL_PART_WORDS, wide);
                if (i0 + lane + 64 < L.ng) b1 = cl_load(ws + L.gparts + ((int64_t)q * L.ng + i0 + lane + 64) * CL_PART_WORDS, wide);
                cl_merge(f, b0);
                cl_merge(f, b1);
            }
            f = cl_wave_reduce(f, wide);
            const ssa_closed_loop_params& r = a.c;
            const int action = (f.arg >= 0) ? (int)f.arg : (r.fallback ? r.fallback[kk + 1] : -1);   // (wave-uniform)
            const unsigned long long word = ((unsigned long long)(unsigned)(kk + 1) << 32) | (unsigned long long)(unsigned)action;
            if (!(r.flags & SSA_LOOP_DEBUG_WITHHOLD))      // (diagnostic: the decision is never published -> every wait runs into its bound)
                for (int i = lane; i < L.ng; i += 64)
                    __hip_atomic_store(ws + L.flags + (int64_t)i * 16, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lane == 0) {   // (for the host: nobody in the launch reads these)
                r.actions[kk + 1] = action;
                if (r.picks) { r.picks[2 * (int64_t)(kk + 1)] = f.arg; r.picks[2 * (int64_t)(kk + 1) + 1] = __double_as_longlong(f.best); }
                double* o = r.stats_out + (int64_t)kk * SSA_STAT_STRIDE;
                o[SSA_STAT_MAX_DPOS] = __longlong_as_double((long long)f.mx);
                o[SSA_STAT_CNT_LT_1E4] = (double)(f.cnt & 0x1fffffull);
                o[SSA_STAT_CNT_LT_1E7] = (double)((f.cnt >> 21) & 0x1fffffull);
                o[SSA_STAT_ARGMAX_SPOS] = wide ? (double)(long long)f.sarg : -1.0;
                o[SSA_STAT_N_FAILED] = (double)(f.cnt >> 42);
                o[SSA_STAT_MAX_SPOS] = wide ? spos_of_key(f.skey) : __builtin_nan("");
                o[6] = 0.0; o[7] = 0.0;
            }
        }
        return;
    }

    // ---------------- compute wavefronts
    const int64_t sx = total * 6, sP = total * 36, so_ = total * 12, sm = 4 * k_arg.p.n_obj;
    const int tile = xcd_tile(w, nwork);
    const int64_t base = (int64_t)tile * OBJ_PER_WAVE;
    const int cnt = (int)((total - base) < OBJ_PER_WAVE ? (total - base) : OBJ_PER_WAVE);
    const int G = w >> 6;
    asrc.flag = ws + L.flags + (int64_t)G * 16;
    asrc.first = a.c.actions[0];
    asrc.pend = -1;
    asrc.base = base;
    asrc.cnt = cnt;
    TileRegs pf;
    typedef const __attribute__((address_space(4))) LoopK* LoopArgPtr;
    LoopArgPtr kp = (LoopArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    GeoK geo;
    {   // the tile's state from the input slot
        const int si0 = (a.c.slot_out + H - 1) % H;
        ssa_step_params p0 = k_arg.p;
        p0.x_true_in = a.c.x_true_ring + si0 * sx;
        p0.x_in = a.c.x_ring + si0 * sx;
        p0.P_in = a.c.P_ring + si0 * sP;
        tile_issue(pf, p0, lane, base, cnt);
        tile_commit(t, pf, lane);
        if (lane < 36) t.Q[lane] = k_arg.c.Q[lane];
        wave_lds_sync();
        if (a.c.agent == SSA_AGENT_SHANNON && (lane & 15) == 0) {   // log det of the covariances the launch starts from
            const int g = lane >> 4;
            double A[21];
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) A[tri(r, c)] = t.P[g * 36 + r * 6 + c];
            ld_prev[g] = logdet_chol(A);
        }
        wave_lds_sync();
    }
    unsigned wave_slot;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 0, 4)" : "=s"(wave_slot));
    bool boost = false;   // this wavefront ran the previous step's update: it is behind the others
    for (int kk = 0; kk < K; ++kk) {
        // issue priority rotated per step (rotate_issue_priority) -- except for the wavefront that ran the update: it lost
        // microseconds the others spent on the next predict, and if it stays behind it is the last to announce its part of
        // the NEXT step too, with every wavefront waiting for it.  It catches up at top priority.
        if (boost) __builtin_amdgcn_s_setprio(3);
        else rotate_issue_priority(wave_slot, (unsigned)kk);
        asm volatile("" : "+s"(kp));
        asm volatile("" : "+v"(lane));
        const StepK& k = ((const LoopK*)kp)->k;
        const ssa_closed_loop_params& r = ((const LoopK*)kp)->c;
        const int so = (r.slot_out + kk) % H, si = (so + H - 1) % H;
        ssa_step_params pk = k.p;
        pk.time_offset = k.p.time_offset + kk;
        pk.x_true_in = r.x_true_ring + si * sx;  pk.x_true_out = r.x_true_ring + so * sx;
        pk.x_in = r.x_ring + si * sx;            pk.x_out = r.x_ring + so * sx;
        pk.P_in = r.P_ring + si * sP;            pk.P_out = r.P_ring + so * sP;
        pk.obs = r.obs_ring + so * so_;
        pk.metrics = r.metrics_ring + so * sm;
        pk.upd = r.upd_out ? r.upd_out + (int64_t)kk * SSA_UPD_STRIDE : nullptr;
        pk.actions = r.actions + kk;
        pk.stat_shards = nullptr;      // the statistics travel with the decision (ClPart)
        pk.stats = nullptr;
        pk.aer_out = nullptr;
        pk.stat_shards_clear = nullptr;
        asrc.want = (unsigned)kk;
        asrc.C = &k.c;
        asrc.lk = (const LoopK*)kp;
        asrc.M = k.p.trans + (int64_t)time_row(k.p.env_time[0] + pk.time_offset, k.p.n_time) * 9;
        process_wave<PROP, 2>(t, k.c, pk, lane, base + (lane >> 4), (lane >> 4) < cnt, base, cnt, pf, 0, 0, tile, asrc);
        wave_lds_sync();
        if (asrc.aborted) return;
        boost = tile == closer_tile(asrc.last, total, r.slot_of);           // the update ran here (or would have)
        // ---- this wavefront's part: the agent's score of its objects (lane 0 of each row) and the step's statistics
        {
            const int g = lane >> 4, l = lane & 15;
            if (l == 0) {
                ClPart me = cl_identity();
                if (g < cnt) {
                    double xt[6], x[6], A[21], sc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int c = 0; c < 6; ++c) { xt[c] = t.T[g * 6 + c]; x[c] = t.X[g * 6 + c]; }
#pragma unroll
                    for (int rr = 0; rr < 6; ++rr)
#pragma unroll
                        for (int c = rr; c < 6; ++c) A[tri(rr, c)] = t.P[g * 36 + rr * 6 + c];
                    // (the visibility of the new true state was evaluated where the wavefront waited for this step's action)
                    const bool vis = (r.agent == SSA_AGENT_NAIVE_GREEDY) || vis_row[g] != 0;
                    double v = 0.0;
                    switch (r.agent) {
                        case SSA_AGENT_NAIVE_GREEDY:
                        case SSA_AGENT_VISIBLE_GREEDY: agent_score_core<1>(xt, x, A, 0.0, nullptr, geo, sc, nullptr); v = sc[0]; break;
                        case SSA_AGENT_SHANNON: {
                            double ld_c;
                            agent_score_core<2>(xt, x, A, ld_prev[g], nullptr, geo, sc, &ld_c);
                            ld_prev[g] = ld_c;
                            v = sc[1];
                            break;
                        }
                        case SSA_AGENT_POS_ERROR: agent_score_core<12>(xt, x, A, 0.0, nullptr, geo, sc, nullptr); v = sc[2]; break;
                        default: agent_score_core<12>(xt, x, A, 0.0, nullptr, geo, sc, nullptr); v = sc[3]; break;
                    }
                    const long long gid = k.p.obj_ids ? (long long)t.Oid[g] : (long long)(base + g);
                    if (vis && v == v) { me.best = v; me.arg = gid; }
                    const double dp = t.Met[g * 4 + 0];
                    me.mx = (unsigned long long)__double_as_longlong(dp) & 0x7fffffffffffffffull;   // (ordered bits; NaN on top: np.max)
                    me.cnt = (unsigned long long)(dp < 1e4) | ((unsigned long long)(dp < 1e7) << 21) | ((unsigned long long)(t.St[g] != 0) << 42);
                    if (wide) { me.skey = spos_key(t.Met[g * 4 + 2]); me.sarg = (unsigned long long)gid; }
                }
                rowpart[g] = me;
            }
        }
        wave_lds_sync();
        if (lane == 0) {
            ClPart me = rowpart[0];
            cl_merge(me, rowpart[1]);
            cl_merge(me, rowpart[2]);
            cl_merge(me, rowpart[3]);
            const bool closer = tile == closer_tile(asrc.last, total, r.slot_of);
            cl_store(closer ? ws + L.cparts + (int64_t)(kk & 1) * CL_PART_WORDS : ws + L.parts + ((int64_t)(kk & 1) * nwork + w) * CL_PART_WORDS, me, wide);
            cl_stores_done();
            __hip_atomic_fetch_add(closer ? ws + L.fcount : ws + L.gcount + (int64_t)G * 16, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (nobody waits for it here)
        }
        asrc.pend = kk;      // the step's outputs leave inside the next step (ActLate::mid_step)
    }
    if (asrc.pend >= 0) closed_loop_store((const LoopK*)kp, t, lane, asrc.pend, base, cnt);
}

// first maximum of score over mask: ONE workgroup of 16 wavefronts (a policy's arg-max head sits between two step launches: a second launch
// for a cross-workgroup fold would cost more than it saves at 20 000 entries).  16 loads in flight per thread (20 000 entries = two rounds),
// the fold by wavefront shuffles + one LDS exchange of the 16 wavefront results: 3-4 us where the first version (8 loads per round, a
// 10-level __syncthreads tree over 1 024 LDS slots) took 11.8 (profiles/r04_run_policy_timeline.txt).
__global__ void __launch_bounds__(1024) masked_argmax_kernel(const double* __restrict__ score, const uint8_t* __restrict__ mask,
                                                             int64_t n, int64_t* __restrict__ out)
{
    const int t = threadIdx.x;
    double best = 0.0;
    long long arg = -1;
    constexpr int Q = 16;
    for (int64_t b0 = 0; b0 < n; b0 += 1024 * Q) {
        double v[Q];
        bool ok[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int64_t i = b0 + (int64_t)q * 1024 + t;
            const bool in = i < n;
            v[q] = in ? score[i] : 0.0;
            ok[q] = in && (mask ? mask[i] != 0 : true);
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {    // (ascending indices per thread: `>` keeps the first maximum)
            const int64_t i = b0 + (int64_t)q * 1024 + t;
            if (ok[q] && v[q] == v[q] && (arg < 0 || v[q] > best)) { best = v[q]; arg = i; }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double b2 = __shfl_down(best, off, 64);
        const long long a2 = __shfl_down(arg, off, 64);
        agent_merge(best, arg, b2, a2);
    }
    __shared__ AgentPart part[16];
    if ((t & 63) == 0) { part[t >> 6].best = best; part[t >> 6].arg = arg; }
    __syncthreads();
    if (t < 64) {
        best = (t < 16) ? part[t].best : 0.0;
        arg = (t < 16) ? part[t].arg : -1;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            const double b2 = __shfl_down(best, off, 64);
            const long long a2 = __shfl_down(arg, off, 64);
            agent_merge(best, arg, b2, a2);
        }
        if (t == 0) {
            out[0] = arg;
            out[1] = __double_as_longlong(best);
        }
    }
}

// The same over many workgroups, for callers that own a small workspace (a policy's arg-max head inside a replayed graph): ONE workgroup
// reads 20 000 entries at the ~40 GB/s a single CU gets (8.6 us, profiles/r04_run_policy_timeline.txt); here every workgroup of 256 lanes
// folds 2 048 entries, stores its part (agent-scope stores), takes a ticket, and the LAST one to arrive folds the parts.  ws: [ticket | pad to
// 64 bytes | parts]; the ticket wraps back to 0 with the last arrival (atomicInc), so the workspace needs zeroing ONCE.  One call at a time
// per workspace (calls in one stream are).
constexpr int AMAX_T = 256, AMAX_Q = 8;
__global__ void __launch_bounds__(AMAX_T) masked_argmax_blocks_kernel(const double* __restrict__ score, const uint8_t* __restrict__ mask,
                                                                      int64_t n, int64_t* __restrict__ out, unsigned long long* __restrict__ ws)
{
    const int t = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * (AMAX_T * AMAX_Q);
    double best = 0.0;
    long long arg = -1;
    {
        double v[AMAX_Q];
        bool ok[AMAX_Q];
#pragma unroll
        for (int q = 0; q < AMAX_Q; ++q) {
            const int64_t i = b0 + q * AMAX_T + t;
            const bool in = i < n;
            v[q] = in ? score[i] : 0.0;
            ok[q] = in && (mask ? mask[i] != 0 : true);
        }
#pragma unroll
        for (int q = 0; q < AMAX_Q; ++q) {
            const int64_t i = b0 + q * AMAX_T + t;
            if (ok[q] && v[q] == v[q] && (arg < 0 || v[q] > best)) { best = v[q]; arg = i; }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double b2 = __shfl_down(best, off, 64);
        const long long a2 = __shfl_down(arg, off, 64);
        agent_merge(best, arg, b2, a2);
    }
    __shared__ AgentPart part[AMAX_T / 64];
    __shared__ int last;
    if ((t & 63) == 0) { part[t >> 6].best = best; part[t >> 6].arg = arg; }
    __syncthreads();
    unsigned long long* parts = ws + 8;
    if (t == 0) {
        for (int w = 1; w < AMAX_T / 64; ++w) agent_merge(best, arg, part[w].best, part[w].arg);
        __hip_atomic_store(parts + 2 * blockIdx.x, (unsigned long long)__double_as_longlong(best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(parts + 2 * blockIdx.x + 1, (unsigned long long)arg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        last = atomicInc(reinterpret_cast<unsigned int*>(ws), gridDim.x - 1) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last || t >= 64) return;
    __threadfence();
    best = 0.0; arg = -1;
    for (int i = t; i < (int)gridDim.x; i += 64) {     // (ascending block index per lane; ties go to the lower object index in agent_merge)
        const double b2 = __longlong_as_double((long long)__hip_atomic_load(parts + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const long long a2 = (long long)__hip_atomic_load(parts + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        agent_merge(best, arg, b2, a2);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double b2 = __shfl_down(best, off, 64);
        const long long a2 = __shfl_down(arg, off, 64);
        agent_merge(best, arg, b2, a2);
    }
    if (t == 0) {
        out[0] = arg;
        out[1] = __double_as_longlong(best);
    }
}

// ---- the tasking assignment of a sensor network (include/ssa_hip.h: ssa_assign_sensors_f64): the global greedy assignment of
// agents._assign_lookahead_sensors over one column of the [S][m][3] scores of ssa_lookahead_sensors_f64 -- S masked arg-max launches, S
// read-backs and the host's mask edits between them -- in ONE launch that writes the action row the next launch reads.
// What makes one pass enough: before sensor s gets its turn at most S - 1 objects have left, so its best remaining object is among its S
// best under the order (value descending, index ascending: agent_merge's).
//   phase 1: a workgroup takes ASG_CH objects; wavefront w does sensors w, w + 4: ASG_Q scores per lane in registers, S rounds of "the
//            first candidate after the previous pick" by wavefront shuffles, the S picks stored as one row of the workspace.  Then the
//            publish of cdna_hip_programming.md (Guideline 16): every wavefront waits for its stores, the barrier, ONE agent-scope release,
//            the ticket (it wraps to 0 with the last arrival: the workspace needs zeroing once).
//   phase 2: the last workgroup to arrive acquires at agent scope, merges the chunks' rows into the S x S table (the same S rounds over
//            nb * S candidates per sensor, loaded once into registers), and ONE wavefront -- lane 8 s + r holds sensor s's r-th candidate -- runs the S greedy rounds
//            over (value descending, s * m + j ascending), applies the fallback rule in ascending s and stores the eight action words.
// ws: [ticket | pad to 64 bytes | nb chunks x S sensors x S (value, index) pairs]; one call at a time per workspace.
constexpr int ASG_T = 256, ASG_CH = 512, ASG_Q = ASG_CH / 64, ASG_HOLD = 8;
struct AsgCand { double v; long long j; };      // (j < 0: none)
SSA_DEV void asg_wave_first(double& v, long long& j)     // the first of the wavefront's candidates, in every lane (distinct j: the merge commutes)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double v2 = __shfl_xor(v, off, 64);
        const long long j2 = __shfl_xor(j, off, 64);
        agent_merge(v, j, v2, j2);
    }
}
SSA_DEV bool asg_after(double v, long long j, double pv, long long pj)      // does (v, j) come strictly after the pick (pv, pj)?
{
    return j >= 0 && (v < pv || (v == pv && j > pj));
}
// ---- the OPTIMAL assignment of a sensor network (include/ssa_hip.h: ssa_match_sensors_f64): one object per sensor, distinct objects,
// first as many sensors tasked as possible, then the largest sum of scores -- over the same S x S table as the greedy rule above
// (assign_sensors_body<true>: the candidates are the finite scores of magnitude <= 2^1020, so that no sum of eight overflows).  The table
// suffices: if an optimal assignment gives sensor s an object outside its S best, at most S - 1 of those S are held by other sensors, one
// is free and at least as good, and the swap keeps the number of tasked sensors.
// The deciding part is a dynamic programme over sensor subsets, run by the whole workgroup that holds the table, one lane per subset:
//   columns: the distinct objects of the table (<= 64) in ascending object index, ranked by one wavefront; w[c][s]: sensor s's score of
//            column c's object, -inf where the object is not in its list;
//   dp[mask]: the best sum that tasks exactly the sensors of `mask` with the columns so far, -inf where there is none (-inf + w stays
//            -inf and wins no comparison: no branch on the sentinels).  Per column, from the previous column's values,
//            new[mask] = max(old[mask], max over s in mask of old[mask ^ 1 << s] + w[c][s]), choice[c][mask] = that s, or 8 for "kept";
//            two buffers, one barrier per column.  The only rounding of the decision is in these sums of at most S scores.
//   ties:    a mask keeps its value unless a sum is strictly greater; among sensors with equal sums the lowest s; the final mask is the
//            one of largest popcount, then largest sum, then lowest mask value.  A pure function of the table's bits.
//   then lane 0 walks `choice` back from the last column, and the first wavefront applies the fallback rule and stores, as for the
//   greedy rule.
// LDS: tab 1 040 + dp 4 096 + w 4 096 + choice 16 384 + the columns' objects and their count 272 + the eight results 128 = 26 016 bytes.
constexpr int ASG_NTAB = SSA_MAX_SENSORS * SSA_MAX_SENSORS;
constexpr int MSN_COLS = ASG_NTAB, MSN_MASKS = 1 << SSA_MAX_SENSORS, MSN_KEPT = SSA_MAX_SENSORS;
static_assert(MSN_MASKS == ASG_T && SSA_MAX_SENSORS == 8, "one lane per sensor subset; lane 8 s + r is sensor s's r-th candidate");
SSA_DEV void msn_better(int& pc, double& bv, int& bm, int p2, double v2, int m2)      // (a total order: the merge commutes)
{
    const bool take = p2 > pc || (p2 == pc && (v2 > bv || (v2 == bv && m2 < bm)));
    if (take) { pc = p2; bv = v2; bm = m2; }
}
SSA_DEV void asg_decide_optimal(const AsgCand* tab, int& act, double& pick_v)
{
    __shared__ double dp[2][MSN_MASKS];
    __shared__ double w[MSN_COLS][SSA_MAX_SENSORS];
    __shared__ unsigned char choice[MSN_COLS][MSN_MASKS];
    __shared__ int colj[MSN_COLS + 4];          // (column c's object; the number of columns in entry MSN_COLS; a multiple of 16 bytes)
    __shared__ AsgCand res[SSA_MAX_SENSORS];    // sensor s's object (j < 0: none) and its score
    const int t = threadIdx.x, lane = t & 63;
    const double NONE = -__builtin_huge_val();
    (&w[0][0])[t] = NONE;
    (&w[0][0])[t + MSN_MASKS] = NONE;
    dp[0][t] = (t == 0) ? 0.0 : NONE;
    if (t < SSA_MAX_SENSORS) { res[t].v = 0.0; res[t].j = -1; }
    __syncthreads();
    if (t < 64) {
        const double cv = tab[lane].v;
        const int cj = (int)tab[lane].j;        // (an object index below 2^31, or -1)
        unsigned long long firsts = 0;          // bit k: lane k is the lowest lane that names its object
        int rank = 0;                           // the distinct objects below this lane's
#pragma unroll 1
        for (int k = 0; k < MSN_COLS; ++k) {    // (a scalar loop: unrolled, its 64 broadcasts at once run the kernel out of SGPRs)
            const int jk = __builtin_amdgcn_readlane(cj, k);
            const bool fk = jk >= 0 && __ffsll((unsigned long long)__ballot(cj == jk)) - 1 == k;
            firsts |= (unsigned long long)fk << k;
            rank += (int)(fk && jk < cj);
        }
        if (cj >= 0) w[rank][lane >> 3] = cv;
        if ((firsts >> lane) & 1) colj[rank] = cj;
        if (lane == 0) colj[MSN_COLS] = __popcll(firsts);
    }
    __syncthreads();
    const int C = colj[MSN_COLS];
    int cur = 0;
    for (int c = 0; c < C; ++c) {
        double best = dp[cur][t];
        int ch = MSN_KEPT;
#pragma unroll
        for (int s = 0; s < SSA_MAX_SENSORS; ++s) {
            const double cand = ((t >> s) & 1) ? dp[cur][t ^ (1 << s)] + w[c][s] : NONE;
            if (cand > best) { best = cand; ch = s; }
        }
        dp[cur ^ 1][t] = best;
        choice[c][t] = (unsigned char)ch;
        cur ^= 1;
        __syncthreads();
    }
    if (t < 64) {
        int pc = -1, bm = 0;
        double bv = 0.0;
#pragma unroll
        for (int q = 0; q < MSN_MASKS / 64; ++q) {
            const int mk = lane + 64 * q;
            const double v = dp[cur][mk];
            if (v != NONE) msn_better(pc, bv, bm, __popc((unsigned)mk), v, mk);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int p2 = __shfl_xor(pc, off, 64), m2 = __shfl_xor(bm, off, 64);
            const double v2 = __shfl_xor(bv, off, 64);
            msn_better(pc, bv, bm, p2, v2, m2);
        }
        if (lane == 0) {
            int mk = bm;                        // (the empty mask is always reachable: pc >= 0)
            for (int c = C - 1; c >= 0; --c) {
                const int ch = choice[c][mk];
                if (ch == MSN_KEPT) continue;
                res[ch].v = w[c][ch];
                res[ch].j = colj[c];
                mk ^= 1 << ch;
            }
        }
    }
    __syncthreads();
    act = (lane < SSA_MAX_SENSORS) ? (int)res[lane & (SSA_MAX_SENSORS - 1)].j : -1;
    pick_v = res[lane & (SSA_MAX_SENSORS - 1)].v;
}
// (one body for one env -- assign_sensors_kernel -- and for E of them -- assign_sensors_envs_kernel, which hands it each env's
// scores, rows and part of the workspace: the grid's x axis walks the chunks, the hand-over is among the gridDim.x workgroups of an env.
// OPTIMAL: the body of match_sensors_kernel / match_sensors_envs_kernel -- the candidates are the finite scores of magnitude <= 2^1020
// instead of the scores that are not NaN, and asg_decide_optimal decides over the table instead of the S greedy rounds; phases 1 and 2,
// the hand-over, the fallback rule and the stores are these lines for both.)
template <bool OPTIMAL>
SSA_DEV void assign_sensors_body(const double* __restrict__ score, int64_t m, int S, int col, const int32_t* __restrict__ fallback,
                                 int32_t* __restrict__ action_out, int64_t* __restrict__ pick_out, unsigned long long* ws)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    AsgCand* parts = reinterpret_cast<AsgCand*>(ws + 8);
    const int64_t j0 = (int64_t)blockIdx.x * ASG_CH;
    for (int s = wave; s < S; s += ASG_T / 64) {
        double v[ASG_Q];
        unsigned ok = 0;        // bit q: object j0 + 64 q + lane is a candidate (in range, not NaN)
#pragma unroll
        for (int q = 0; q < ASG_Q; ++q) {
            const int64_t jj = j0 + q * 64 + lane;
            v[q] = (jj < m) ? score[((int64_t)s * m + jj) * SSA_LOOK_NSCORE + col] : 0.0;
            ok |= (unsigned)(jj < m && (OPTIMAL ? fabs(v[q]) <= 0x1p1020 : v[q] == v[q])) << q;
        }
        double pv = 0.0, kv = 0.0;
        long long pj = -1, kj = -1;
        for (int r = 0; r < S; ++r) {
            double bv = 0.0;
            long long bj = -1;
            if (r == 0 || pj >= 0) {      // (an empty round: every later one is empty)
#pragma unroll
                for (int q = 0; q < ASG_Q; ++q) {      // (ascending indices per lane)
                    const long long jq = j0 + q * 64 + lane;
                    if (((ok >> q) & 1) && (r == 0 || asg_after(v[q], jq, pv, pj))) agent_merge(bv, bj, v[q], jq);
                }
                asg_wave_first(bv, bj);
            }
            if (lane == r) { kv = bv; kj = bj; }
            pv = bv; pj = bj;
        }
        if (lane < S) {
            AsgCand c;
            c.v = kv; c.j = kj;
            parts[((int64_t)blockIdx.x * S + s) * S + lane] = c;
        }
    }
    constexpr int NTAB = ASG_NTAB;
    __shared__ AsgCand tab[NTAB + 1];       // (the one LDS object: the table, and the last-arrival flag in the j of its extra entry)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const bool won = atomicInc(reinterpret_cast<unsigned int*>(ws), gridDim.x - 1) == gridDim.x - 1;
        if (won) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        tab[NTAB].j = won;
    }
    if (t < NTAB) { tab[t].v = 0.0; tab[t].j = -1; }
    __syncthreads();
    if (!tab[NTAB].j) return;
    // lane 8 b + k reads rank k of chunks b, b + 8, ...: no division by S, 32-bit indices (nb * S * S < 2^28).  The first ASG_HOLD of
    // them -- 8 ASG_HOLD chunks, 32 768 objects -- stay in registers over the S rounds; only what lies beyond is re-read from L2.
    const int nb = (int)gridDim.x, rk = lane & 7, b0 = lane >> 3;
    for (int s = wave; s < S; s += ASG_T / 64) {
        AsgCand held[ASG_HOLD];
#pragma unroll
        for (int q = 0; q < ASG_HOLD; ++q) {
            const int b = b0 + 8 * q;
            held[q].v = 0.0; held[q].j = -1;
            if (rk < S && b < nb) held[q] = parts[(b * S + s) * S + rk];
        }
        double pv = 0.0, kv = 0.0;
        long long pj = -1, kj = -1;
        for (int r = 0; r < S; ++r) {
            double bv = 0.0;
            long long bj = -1;
            if (r == 0 || pj >= 0) {
#pragma unroll
                for (int q = 0; q < ASG_HOLD; ++q)
                    if (r == 0 ? held[q].j >= 0 : asg_after(held[q].v, held[q].j, pv, pj)) agent_merge(bv, bj, held[q].v, held[q].j);
                if (rk < S)
                    for (int b = b0 + 8 * ASG_HOLD; b < nb; b += 8) {
                        const AsgCand a = parts[(b * S + s) * S + rk];
                        if (r == 0 ? a.j >= 0 : asg_after(a.v, a.j, pv, pj)) agent_merge(bv, bj, a.v, a.j);
                    }
                asg_wave_first(bv, bj);
            }
            if (lane == r) { kv = bv; kj = bj; }
            pv = bv; pj = bj;
        }
        if (lane < S) { tab[s * SSA_MAX_SENSORS + lane].v = kv; tab[s * SSA_MAX_SENSORS + lane].j = kj; }
    }
    __syncthreads();
    int act = -1;                  // lane s < S: sensor s's object
    double pick_v = 0.0;
    if constexpr (OPTIMAL) {
        asg_decide_optimal(tab, act, pick_v);
        if (t >= 64) return;
    } else {
        if (t >= 64) return;
        const int cs = lane >> 3;
        const double cv = tab[lane].v;
        long long cj = tab[lane].j;
        for (int r = 0; r < S; ++r) {
            double bv = cv;
            long long bf = (cj >= 0) ? (long long)cs * m + cj : -1;      // (ties: the lowest s * m + j, the masked arg-max's first maximum)
            const long long mine = bf;
            asg_wave_first(bv, bf);
            if (bf < 0) break;
            const int ws_s = (__ffsll((unsigned long long)__ballot(mine == bf)) - 1) >> 3;
            const long long wj = bf - (long long)ws_s * m;
            if (lane == ws_s) { act = (int)wj; pick_v = bv; }
            if (cs == ws_s || cj == wj) cj = -1;       // the sensor and the object leave the pool
        }
    }
    const int assigned = act;
    const int fb = (fallback && lane < S) ? fallback[lane] : -1;
    for (int s = 0; s < S; ++s) {       // a sensor left without an object: the caller's draw, unless out of range or held by anybody
        const int a_s = __shfl(act, s, 64), f_s = __shfl(fb, s, 64);
        if (a_s >= 0 || f_s < 0 || (int64_t)f_s >= m) continue;
        const bool held = __any(lane < S && act == f_s);
        if (!held && lane == s) act = f_s;
    }
    if (lane < SSA_MAX_SENSORS) {
        action_out[lane] = (lane < S) ? act : -1;
        if (pick_out) {
            pick_out[2 * lane] = (lane < S) ? (int64_t)assigned : -1;
            pick_out[2 * lane + 1] = __double_as_longlong(pick_v);
        }
    }
}
__global__ void __launch_bounds__(ASG_T) assign_sensors_kernel(const double* __restrict__ score, int64_t m, int S, int col,
                                                               const int32_t* __restrict__ fallback, int32_t* __restrict__ action_out,
                                                               int64_t* __restrict__ pick_out, unsigned long long* ws)
{
    assign_sensors_body<false>(score, m, S, col, fallback, action_out, pick_out, ws);
}
// ... of every env of a vector launch (ssa_assign_sensors_envs_f64): grid (chunks, envs).  Env e = blockIdx.y has its [S][m][3] slab of
// the scores, its rows of `fallback`, `action_out` and `pick_out`, and its own ticket and candidate area, `ws_words` words apart
// (64-byte aligned); the last workgroup to arrive FOR ITS ENV merges and assigns that env.
__global__ void __launch_bounds__(ASG_T) assign_sensors_envs_kernel(const double* __restrict__ score, int64_t m, int S, int col,
                                                                    const int32_t* __restrict__ fallback, int32_t* __restrict__ action_out,
                                                                    int64_t* __restrict__ pick_out, unsigned long long* ws, int64_t ws_words)
{
    const int64_t e = blockIdx.y;
    assign_sensors_body<false>(score + e * S * m * SSA_LOOK_NSCORE, m, S, col, fallback ? fallback + e * SSA_MAX_SENSORS : nullptr,
                        action_out + e * SSA_MAX_SENSORS, pick_out ? pick_out + e * SSA_MAX_SENSORS * 2 : nullptr, ws + e * ws_words);
}
// the optimal rule's kernels: the arguments, grids and workspaces of the two above
__global__ void __launch_bounds__(ASG_T) match_sensors_kernel(const double* __restrict__ score, int64_t m, int S, int col,
                                                              const int32_t* __restrict__ fallback, int32_t* __restrict__ action_out,
                                                              int64_t* __restrict__ pick_out, unsigned long long* ws)
{
    assign_sensors_body<true>(score, m, S, col, fallback, action_out, pick_out, ws);
}
// ... of every env of a vector launch (ssa_match_sensors_envs_f64): the grid and the workspace of assign_sensors_envs_kernel
__global__ void __launch_bounds__(ASG_T) match_sensors_envs_kernel(const double* __restrict__ score, int64_t m, int S, int col,
                                                                   const int32_t* __restrict__ fallback, int32_t* __restrict__ action_out,
                                                                   int64_t* __restrict__ pick_out, unsigned long long* ws, int64_t ws_words)
{
    const int64_t e = blockIdx.y;
    assign_sensors_body<true>(score + e * S * m * SSA_LOOK_NSCORE, m, S, col, fallback ? fallback + e * SSA_MAX_SENSORS : nullptr,
                       action_out + e * SSA_MAX_SENSORS, pick_out ? pick_out + e * SSA_MAX_SENSORS * 2 : nullptr, ws + e * ws_words);
}

// ---- the horizon-wide OPTIMAL tasking plan of a sensor network (include/ssa_hip.h: ssa_plan_sensors_f64): one
// assignment problem over the N = H' S slots (h, s) of a forecast [H'][E][S][m][3], an object planned at most once per env -- first as
// many slots filled as possible, then the largest sum of scores -- in ONE launch, grid (chunks, envs), PLN_T threads.
//   phase 1: a workgroup takes PLN_CH objects of one env; wavefront w does slots w, w + 16, ...: the slot's N best candidates of the chunk
//            in the total order (score descending, object ascending) as ONE entry per lane, sorted across the wavefront.  A group of 64
//            scores is sorted by a bitonic network over lane exchanges; the lane-wise better of the list and the reversed group is the
//            top 64 as a bitonic sequence, six more exchange stages sort it.  A group none of whose candidates beats the list's N-th
//            entry is skipped (a ballot).  An entry is (key, object): key = the score's bits mapped so that unsigned order is value
//            order (-0.0 read as +0.0), 0 = none.  The lists go to the workspace; the publish and the ticket are assign_sensors_body's.
//   phase 2: the last workgroup to arrive FOR ITS ENV merges the chunks' lists per slot the same way (chunk lists are sorted: no sort,
//            the six merge stages only; a chunk whose best does not beat the list's N-th is skipped) into the N x N table in LDS.
//   decide : scores -> int64 multiples of 2^(e - 52), 2^e the smallest power of two above the table's largest magnitude (exact for every
//            table whose entries are multiples of that unit: dyadic tables are).  Columns: the table's distinct objects (<= N^2), numbered
//            through an LDS hash table (which object gets which number never enters a decision), plus one private idle column per slot.
//            Costs: pairs (idle, -q) ordered lexicographically and added componentwise -- an ordered group, so the shortest-augmenting-
//            path solver (Jonker-Volgenant) runs on them unchanged and the count needs no large constant.  ONE wavefront inserts the
//            slots in ascending order; the search is Dijkstra's over the SLOTS (a slot's <= N + 1 finite entries are relaxed one lane each;
//            a matched column leads to exactly one slot, so the relaxations of one scan never collide), with the duals u (a register per
//            slot), v (LDS, per column) keeping every reduced cost >= 0.
//   ties   : slots are inserted in ascending h S + s; the unscanned slot of least distance is scanned next, the lowest slot among
//            equals; a free column replaces the best one found so far only if strictly nearer, within one scan the entry of lowest
//            rank in the slot's list, its idle column last; a slot's distance and predecessor change only for a strictly smaller
//            distance; the search stops as soon as no unscanned slot is strictly nearer than the best free column.
// ws per env: [ticket | pad to 64 bytes | nb chunks x N slots x N entries of 16 bytes]; one call at a time per workspace.
// LDS: q 32 768 + objects 16 384 + column numbers 8 192 + the hash table, later the columns' duals 49 152 + the columns' slots 4 096
//      + one scan's relaxations 1 280 + the result 256 + scan totals 64 + the largest magnitude, the flag 16 = 112 208 bytes.
constexpr int PLN_T = 1024, PLN_W = PLN_T / 64, PLN_CH = 512, PLN_G = PLN_CH / 64, PLN_N = SSA_MAX_PLAN_SLOTS, PLN_PF = 8;
constexpr int PLN_HASH = 2 * PLN_N * PLN_N, PLN_NONE = 0x7fffffff, PLN_IDLE = PLN_N, PLN_INF = 1 << 20;
static_assert(PLN_N == 64 && PLN_HASH == 8 * PLN_T, "a slot's list is one entry per lane; eight hash slots per thread");
struct alignas(16) PlnEnt { unsigned long long key; int j; int pad; };
struct PlnLds {
    long long q[PLN_N][PLN_N];                  // slot i's k-th entry: first its key, then its quantised score
    int obj[PLN_N][PLN_N];                      // ... its object (-1: none)
    unsigned short col[PLN_N][PLN_N];           // ... its column: first its hash slot, then its number
    unsigned long long pool[3 * PLN_HASH / 4];  // the hash keys (int [PLN_HASH]) and numbers (short [PLN_HASH]); then vq (int64 [N^2]), vc (int [N^2])
    signed char rowof[PLN_N * PLN_N];           // the slot a column is matched to (-1: free)
    long long rlq[PLN_N];                       // one scan's relaxation of slot i: the distance (rlc, rlq) through entry rlk, valid if rls == the scan's stamp
    int rlc[PLN_N], rlk[PLN_N], rls[PLN_N];
    int res[PLN_N];                             // slot i's object
    int wtot[PLN_W];
    unsigned long long amax;                    // the bits of the table's largest magnitude
    int won, pad;
};
static_assert(sizeof(PlnLds) == 112208, "the LDS sum of the comment above");
SSA_DEV unsigned long long pln_key(double v)    // finite v: unsigned order of the keys = value order, -0.0 = +0.0; never 0
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
SSA_DEV double pln_val(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
SSA_DEV bool pln_before(unsigned long long k, int j, unsigned long long k2, int j2) { return k > k2 || (k == k2 && j < j2); }
// one exchange stage: lanes l and l ^ d compare; the lane with keep_first keeps the entry that comes first
// lane l ^ d's value, d a power of two below 64, all 64 lanes active: DPP inside a row of 16 (quad permutes for 1 and 2, half-row mirror
// then quad reversal for 4 -- l ^ 7 ^ 3 --, a rotation by 8 for 8) and gfx950's row and half swaps for 16 and 32: no LDS-crossbar traffic,
// which sixteen wavefronts sorting at once would otherwise queue for
SSA_DEV int pln_x32(int v, int d, int lane)
{
    typedef unsigned pair_t __attribute__((ext_vector_type(2)));
    switch (d) {
        case 1: return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
        case 2: return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
        case 4: return __builtin_amdgcn_update_dpp(0, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true), 0x1B, 0xF, 0xF, true);
        case 8: return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, true);
        case 16: {
            const pair_t r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
            return (int)((lane & 16) ? r[0] : r[1]);
        }
        default: {
            const pair_t r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
            return (int)((lane & 32) ? r[0] : r[1]);
        }
    }
}
SSA_DEV unsigned long long pln_x64(unsigned long long v, int d, int lane)
{
    const unsigned lo = (unsigned)pln_x32((int)(unsigned)v, d, lane), hi = (unsigned)pln_x32((int)(unsigned)(v >> 32), d, lane);
    return ((unsigned long long)hi << 32) | lo;
}
SSA_DEV void pln_cx(unsigned long long& k, int& j, int d, bool keep_first, int lane)
{
    const unsigned long long k2 = pln_x64(k, d, lane);
    const int j2 = pln_x32(j, d, lane);
    if (pln_before(k, j, k2, j2) != keep_first) { k = k2; j = j2; }
}
SSA_DEV void pln_sort(unsigned long long& k, int& j, int lane)       // 64 entries, the first in lane 0
{
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
        for (int d = size >> 1; d > 0; d >>= 1) pln_cx(k, j, d, ((lane & d) == 0) == ((lane & size) == 0), lane);
}
SSA_DEV void pln_merge(unsigned long long& lk, int& lj, unsigned long long ck, int cj, int lane)      // both sorted; the first 64 of the union
{
    const unsigned long long rk = __shfl(ck, 63 - lane, 64);
    const int rj = __shfl(cj, 63 - lane, 64);
    if (pln_before(rk, rj, lk, lj)) { lk = rk; lj = rj; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) pln_cx(lk, lj, d, (lane & d) == 0, lane);
}
SSA_DEV bool pln_less(int c, long long q, int c2, long long q2) { return c < c2 || (c == c2 && q < q2); }
SSA_DEV void pln_wave_min(int& c, long long& q, int& id, int lane)      // the least (c, q, id) of the wavefront, in every lane (distinct id: the merge commutes)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int c2 = pln_x32(c, off, lane), id2 = pln_x32(id, off, lane);
        const long long q2 = (long long)pln_x64((unsigned long long)q, off, lane);
        if (pln_less(c2, q2, c, q) || (c2 == c && q2 == q && id2 < id)) { c = c2; q = q2; id = id2; }
    }
}
SSA_DEV void pln_wave_sync()        // LDS written by one lane, read by another lane of the SAME wavefront
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// the deciding part: ONE wavefront over the table in LDS; lane i is slot i (its dual, its matched entry) and, within a scan, entry k = lane
SSA_DEV void pln_decide(PlnLds& L, int N, int lane)
{
    long long* vq = reinterpret_cast<long long*>(L.pool);
    int* vc = reinterpret_cast<int*>(L.pool + PLN_N * PLN_N);
    int uc = 0, mk = -1, vidc = 0;              // slot `lane`: its dual, its matched entry (PLN_IDLE: its idle column), its idle column's dual
    long long uq = 0, vidq = 0;
    int stamp = 1;
    for (int i0 = 0; i0 < N; ++i0) {
        {   // u[i0] = its least cost less the column's dual: every reduced cost of the new slot >= 0 (its idle column's dual is still 0)
            const int cn = (lane < N) ? (int)L.col[i0][lane] : 0xffff;
            int c = PLN_INF, id = lane;
            long long q = 0;
            if (cn != 0xffff) { c = -vc[cn]; q = -L.q[i0][lane] - vq[cn]; }
            pln_wave_min(c, q, id, lane);
            if (!pln_less(c, q, 1, 0)) { c = 1; q = 0; }
            if (lane == i0) { uc = c; uq = q; }
        }
        int Dc = (lane == i0) ? 0 : PLN_INF, pred = -1, predk = -1;
        long long Dq = 0;
        bool vis = false;
        int bc = PLN_INF, brow = -1, bk = -1;
        long long bq = 0;
        for (int scan = 0; scan < N; ++scan) {      // (every scan takes a new slot: N at most)
            int mc = vis ? PLN_INF : Dc, mi = lane;
            long long mq = vis ? 0 : Dq;
            pln_wave_min(mc, mq, mi, lane);
            if (mc >= PLN_INF || !pln_less(mc, mq, bc, bq)) break;
            if (lane == mi) vis = true;
            const int uic = __shfl(uc, mi, 64), mkm = __shfl(mk, mi, 64), vic = __shfl(vidc, mi, 64);
            const long long uiq = __shfl(uq, mi, 64), viq = __shfl(vidq, mi, 64);
            const int cn = (lane < N) ? (int)L.col[mi][lane] : 0xffff;
            int sc = PLN_INF, sk = lane;
            long long sq = 0;
            if (cn != 0xffff) {
                const int nc = mc - uic - vc[cn];
                const long long nq = mq - L.q[mi][lane] - uiq - vq[cn];
                const int owner = L.rowof[cn];
                if (owner < 0) { sc = nc; sq = nq; }
                else if (owner != mi) { L.rlc[owner] = nc; L.rlq[owner] = nq; L.rlk[owner] = lane; L.rls[owner] = stamp; }
            }
            pln_wave_sync();
            if (!vis && L.rls[lane] == stamp && pln_less(L.rlc[lane], L.rlq[lane], Dc, Dq)) {
                Dc = L.rlc[lane]; Dq = L.rlq[lane]; pred = mi; predk = L.rlk[lane];
            }
            pln_wave_min(sc, sq, sk, lane);
            if (mkm != PLN_IDLE) {      // its idle column is free: the last of the scan's candidates
                const int ic = mc + 1 - uic - vic;
                const long long iq = mq - uiq - viq;
                if (pln_less(ic, iq, sc, sq)) { sc = ic; sq = iq; sk = PLN_IDLE; }
            }
            if (pln_less(sc, sq, bc, bq)) { bc = sc; bq = sq; brow = mi; bk = sk; }
            ++stamp;
        }
        // the duals: every scanned slot rises by what it was nearer than the free column, its matched column falls by as much
        if (vis) {
            const int dc = bc - Dc;
            const long long dq = bq - Dq;
            uc += dc; uq += dq;
            if (mk == PLN_IDLE) { vidc -= dc; vidq -= dq; }
            else if (mk >= 0) { const int cn = L.col[lane][mk]; vc[cn] -= dc; vq[cn] -= dq; }
        }
        // the augmenting path, back from the free column to the new slot
        for (int r = brow, k = bk, hop = 0; hop < N; ++hop) {      // (a path visits a slot once: N hops at most)
            const int pr = __shfl(pred, r, 64), pk = __shfl(predk, r, 64);
            if (lane == r) {
                mk = k;
                if (k != PLN_IDLE) L.rowof[L.col[r][k]] = (signed char)r;
            }
            if (r == i0) break;
            r = pr; k = pk;
        }
        pln_wave_sync();
    }
    L.res[lane] = (lane < N && mk >= 0 && mk != PLN_IDLE) ? L.obj[lane][mk] : -1;
    pln_wave_sync();
}
__global__ void __launch_bounds__(PLN_T) plan_sensors_kernel(const double* __restrict__ score, int64_t m, int S, int H, int col,
                                                             int32_t* __restrict__ plan_out, int64_t* __restrict__ pick_out,
                                                             unsigned long long* ws_all, int64_t ws_words)
{
    __shared__ PlnLds L;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, N = H * S;
    const int64_t e = blockIdx.y, E = gridDim.y;
    unsigned long long* ws = ws_all + e * ws_words;
    PlnEnt* parts = reinterpret_cast<PlnEnt*>(ws + 8);
    const int64_t j0 = (int64_t)blockIdx.x * PLN_CH;
    for (int i = wave; i < N; i += PLN_W) {
        const int h = i / S, s = i - h * S;
        const double* base = score + (((int64_t)h * E + e) * S + s) * m * SSA_LOOK_NSCORE + col;
        double v[PLN_G];
#pragma unroll
        for (int g = 0; g < PLN_G; ++g) {
            const int64_t jj = j0 + g * 64 + lane;
            v[g] = (jj < m) ? base[jj * SSA_LOOK_NSCORE] : __builtin_nan("");
        }
        unsigned long long lk = 0;
        int lj = PLN_NONE;
#pragma unroll
        for (int g = 0; g < PLN_G; ++g) {
            const bool ok = fabs(v[g]) <= 0x1p1020;       // (NaN, +-inf, out of range: false)
            unsigned long long ck = ok ? pln_key(v[g]) : 0ull;
            int cj = ok ? (int)(j0 + g * 64 + lane) : PLN_NONE;
            const unsigned long long wk = __shfl(lk, N - 1, 64);
            const int wj = __shfl(lj, N - 1, 64);
            if (!__any(ok && pln_before(ck, cj, wk, wj))) continue;
            pln_sort(ck, cj, lane);
            pln_merge(lk, lj, ck, cj, lane);
        }
        if (lane < N) {
            PlnEnt c;
            c.key = lk; c.j = lj; c.pad = 0;
            parts[((int64_t)blockIdx.x * N + i) * N + lane] = c;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const bool won = atomicInc(reinterpret_cast<unsigned int*>(ws), gridDim.x - 1) == gridDim.x - 1;
        if (won) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        L.won = won;
        L.amax = 0;
    }
    __syncthreads();
    if (!L.won) return;
    const int nb = (int)gridDim.x;
    for (int i = wave; i < N; i += PLN_W) {
        unsigned long long lk = 0;
        int lj = PLN_NONE;
        for (int b0 = 0; b0 < nb; b0 += PLN_PF) {
            PlnEnt c[PLN_PF];
#pragma unroll
            for (int p = 0; p < PLN_PF; ++p) {
                c[p].key = 0; c[p].j = PLN_NONE;
                if (lane < N && b0 + p < nb) c[p] = parts[((int64_t)(b0 + p) * N + i) * N + lane];
            }
#pragma unroll
            for (int p = 0; p < PLN_PF; ++p) {
                const unsigned long long fk = __shfl(c[p].key, 0, 64), wk = __shfl(lk, N - 1, 64);
                const int fj = __shfl(c[p].j, 0, 64), wj = __shfl(lj, N - 1, 64);
                if (!pln_before(fk, fj, wk, wj)) continue;
                pln_merge(lk, lj, c[p].key, c[p].j, lane);
            }
        }
        const bool has = lane < N && lj != PLN_NONE;
        L.q[i][lane] = (long long)lk;
        L.obj[i][lane] = has ? lj : -1;
        unsigned long long a = has ? (unsigned long long)__double_as_longlong(fabs(pln_val(lk))) : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long a2 = __shfl_xor(a, off, 64);
            a = a2 > a ? a2 : a;
        }
        if (lane == 0) atomicMax(&L.amax, a);
    }
    int* hkey = reinterpret_cast<int*>(L.pool);
    unsigned short* hid = reinterpret_cast<unsigned short*>(L.pool + PLN_HASH / 2);
#pragma unroll
    for (int p = 0; p < PLN_HASH / PLN_T; ++p) hkey[t + PLN_T * p] = -1;
    __syncthreads();
    int ex;
    (void)frexp(__longlong_as_double((long long)L.amax), &ex);      // amax < 2^ex, the smallest such power of two
    for (int idx = t; idx < N * PLN_N; idx += PLN_T) {
        const int i = idx >> 6, k = idx & 63, o = L.obj[i][k];
        if (o < 0) { L.col[i][k] = 0xffff; continue; }
        L.q[i][k] = (long long)rint(ldexp(pln_val((unsigned long long)L.q[i][k]), 52 - ex));      // |q| <= 2^52
        unsigned slot = ((unsigned)o * 2654435761u) >> 19;
        for (;;) {
            const int old = atomicCAS(&hkey[slot], -1, o);
            if (old == -1 || old == o) break;
            slot = (slot + 1) & (PLN_HASH - 1);
        }
        L.col[i][k] = (unsigned short)slot;
    }
    __syncthreads();
    {   // number the occupied hash slots 0, 1, ...: eight slots per thread, a scan over the workgroup
        int cnt = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p) cnt += hkey[8 * t + p] != -1;
        int inc = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(inc, off, 64);
            if (lane >= off) inc += up;
        }
        if (lane == 63) L.wtot[wave] = inc;
        __syncthreads();
        int at = inc - cnt;
        for (int w = 0; w < wave; ++w) at += L.wtot[w];
#pragma unroll
        for (int p = 0; p < 8; ++p)
            if (hkey[8 * t + p] != -1) hid[8 * t + p] = (unsigned short)at++;
    }
    __syncthreads();
    for (int idx = t; idx < N * PLN_N; idx += PLN_T) {
        const int i = idx >> 6, k = idx & 63;
        if (L.col[i][k] != 0xffff) L.col[i][k] = hid[L.col[i][k]];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 3 * PLN_HASH / 4 / PLN_T; ++p) L.pool[t + PLN_T * p] = 0;      // the columns' duals
    reinterpret_cast<int*>(L.rowof)[t] = -1;
    if (t < PLN_N) L.rls[t] = 0;
    __syncthreads();
    if (t >= 64) return;
    pln_decide(L, N, lane);
    // the rows of this env: [H][E][SSA_MAX_SENSORS], -1 beyond S and in unfilled slots; the picks' scores are read where they were read first
    for (int idx = lane; idx < H * SSA_MAX_SENSORS; idx += 64) {
        const int h = idx >> 3, s = idx & 7;
        const int o = (s < S) ? L.res[h * S + s] : -1;
        const int64_t row = ((int64_t)h * E + e) * SSA_MAX_SENSORS + s;
        plan_out[row] = o;
        if (pick_out) {
            pick_out[2 * row] = o;
            pick_out[2 * row + 1] = (o >= 0) ? __double_as_longlong(score[((((int64_t)h * E + e) * S + s) * m + o) * SSA_LOOK_NSCORE + col]) : 0;
        }
    }
}

// ---- diagnostic reductions of SURVEY 8f-4 (ssa_tasker_simple_2.py:436-446, 750-775): NEES = d^T inv(P) d with
// d = x_true - x_filter, NIS = y^T inv(S) y.  One lane per (step, object): Gaussian elimination with partial pivoting on
// the augmented system [P | d] (the arithmetic class of numpy.linalg.inv's LU), then the dot product.
__global__ void nees_kernel(const double* __restrict__ xt, const double* __restrict__ x, const double* __restrict__ P,
                            double* __restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double A[6][7], d[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        d[r] = xt[i * 6 + r] - x[i * 6 + r];
#pragma unroll
        for (int c = 0; c < 6; ++c) A[r][c] = P[i * 36 + r * 6 + c];
        A[r][6] = d[r];
    }
    bool singular = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        // pivot: the largest |A[r][k]|, r >= k, swapped into row k with compile-time indices (registers, no scratch)
#pragma unroll
        for (int r = k + 1; r < 6; ++r) {
            const bool sw = fabs(A[r][k]) > fabs(A[k][k]);
#pragma unroll
            for (int c = k; c < 7; ++c) {
                const double a = A[k][c], b = A[r][c];
                A[k][c] = sw ? b : a;
                A[r][c] = sw ? a : b;
            }
        }
        singular = singular || (A[k][k] == 0.0);
        const double inv = 1.0 / A[k][k];
#pragma unroll
        for (int r = k + 1; r < 6; ++r) {
            const double f = A[r][k] * inv;
#pragma unroll
            for (int c = k + 1; c < 7; ++c) A[r][c] = fma(-f, A[k][c], A[r][c]);
        }
    }
    double z[6];
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double acc = A[r][6];
#pragma unroll
        for (int c = r + 1; c < 6; ++c) acc = fma(-A[r][c], z[c], acc);
        z[r] = acc / A[r][r];
    }
    double q = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) q = fma(d[r], z[r], q);
    out[i] = singular ? __builtin_nan("") : q;   // numpy raises LinAlgError('Singular matrix') there
}
__global__ void nis_kernel(const double* __restrict__ y, const double* __restrict__ S, double* __restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s[9], si[9], yy[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) s[c] = S[i * 9 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) yy[c] = y[i * 3 + c];
    if (!inv3(s, si)) { out[i] = __builtin_nan(""); return; }
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) q += yy[a] * (si[a * 3] * yy[0] + si[a * 3 + 1] * yy[1] + si[a * 3 + 2] * yy[2]);
    out[i] = q;
}

// fitness_test()'s chi-square containment (ssa_tasker_simple_2.py:750-775): how many of v[0..n) lie strictly inside (lo, hi) -- the
// two-sided 95 % critical points of chi2(df) the caller passes in -- next to the number of non-NaN entries (the reference drops
// NaN NIS values before taking the mean, :757, and keeps them in the NEES mean, :771).  counts[0] = inside, counts[1] = non-NaN.
__global__ void __launch_bounds__(64) chi2_zero_kernel(unsigned long long* __restrict__ counts)
{
    if (threadIdx.x < 2) counts[threadIdx.x] = 0ull;
}
__global__ void __launch_bounds__(256) chi2_contained_kernel(const double* __restrict__ v, int64_t n, double lo, double hi,
                                                             unsigned long long* __restrict__ counts)
{
    unsigned inside = 0, valid = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double x = v[i];
        inside += (x > lo) && (x < hi);
        valid += (x == x);
    }
    // per wavefront: two ballots per 64 values would need a loop of its own; a shuffle tree of two 32-bit counters is 12 steps
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        inside += __shfl_down(inside, off, 64);
        valid += __shfl_down(valid, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (inside) atomicAdd(counts, (unsigned long long)inside);
        if (valid) atomicAdd(counts + 1, (unsigned long long)valid);
    }
}

static GeoK make_geo(const ssa_consts* c)
{
    GeoK g;
    for (int i = 0; i < 9; ++i) g.enu[i] = c->enu[i];
    for (int i = 0; i < 3; ++i) g.obs[i] = c->obs_itrs[i];
    g.obs_limit = c->obs_limit;
    g.Wi = c->Wi;
    g.sum_wm_m1 = c->sum_wm_m1;
    return g;
}
static inline int launch_status()
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return SSA_OK;
    fprintf(stderr, "libssa_hip: kernel launch failed: %s (%s)\n", hipGetErrorName(e), hipGetErrorString(e));   // fail loudly
    return SSA_E_LAUNCH;
}
static inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }


// ---- all-gather by direct peer stores (SURVEY 8e "Collective"): every rank writes its payload of one step straight into the slot it owns
// in every peer's receive buffer (pointers mapped once over hipIpc, host side: ssa-gym_amd/peer.py) and then raises a per-source flag word
// next to it; a consumer waits for the flags of the step it wants.  Nothing here is a collective: no communicator, no rendezvous inside the
// launch, plain kernels a hipGraph captures at any world size.  The step number a launch stands for is seq_base[0] + seq_off (seq_base in
// device memory: a replayed graph advances it on the device, as the time index of the step launches).
//   ordering: every lane's stores, a system-scope fence, the workgroup barrier, then ONE release store of the flag (system scope): a peer
//   that reads the flag >= seq with an acquire load sees the whole payload.  Flags only grow (a 64-bit step counter).
//   a push is PEER_SPLIT workgroups per peer (one workgroup moves 160 KB at a single CU's ~40 GB/s: 4 us); each fences at system scope and
//   takes a ticket, the last one raises the flag.  prev_flags (optional): the rank's OWN flag words of the previous step's buffer -- the
//   workgroups that write to peer r first wait (bounded) until r's payload of step seq - 1 has arrived here, by which time r's readers of the
//   slot about to be overwritten (step seq - 3) have passed in r's stream order: the reuse rule of the rotating buffers inside the push itself,
//   one dispatch per step instead of two.
constexpr int PEER_SPLIT = 8;
__global__ void __launch_bounds__(256) peer_push_kernel(const double* __restrict__ src, int64_t n_words, double* const* __restrict__ dst,
                                                        unsigned long long* const* __restrict__ flag,
                                                        const unsigned long long* __restrict__ seq_base, unsigned long long seq_off,
                                                        const unsigned long long* __restrict__ prev_flags, long long timeout_ticks,
                                                        int32_t* __restrict__ error, unsigned int* __restrict__ tickets)
{
    const int r = blockIdx.x, sl = blockIdx.y, t = threadIdx.x;
    const unsigned long long seq = seq_base[0] + seq_off;
    if (prev_flags && seq >= 2ull) {
        if (t == 0) {
            const long long t0 = (long long)wall_clock64();
            while (__hip_atomic_load(&prev_flags[r], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < seq - 1ull) {
                if ((long long)wall_clock64() - t0 > timeout_ticks) {
                    if (error) atomicMax(error, 1 + r);
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
            }
        }
        __syncthreads();
    }
    double* __restrict__ d = dst[r];
    int64_t chunk = (n_words + gridDim.y - 1) / gridDim.y;
    chunk += chunk & 1;                                          // (even: the slices keep the 16-byte alignment of the whole)
    const int64_t lo = (int64_t)sl * chunk, hi = (lo + chunk < n_words) ? lo + chunk : n_words;
    if (lo < hi) {
        const bool wide = ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
        if (wide) {
            const double2* __restrict__ s2 = reinterpret_cast<const double2*>(src + lo);
            double2* __restrict__ d2 = reinterpret_cast<double2*>(d + lo);
            const int64_t n2 = (hi - lo) >> 1;
            for (int64_t i = t; i < n2; i += blockDim.x) d2[i] = s2[i];
            if (((hi - lo) & 1) && t == 0) d[hi - 1] = src[hi - 1];
        } else {
            for (int64_t i = lo + t; i < hi; i += blockDim.x) d[i] = src[i];
        }
    }
    __threadfence_system();
    __syncthreads();
    if (t == 0 && atomicInc(&tickets[r], gridDim.y - 1) == gridDim.y - 1) {     // (the ticket wraps back to 0 with the last arrival)
        __threadfence_system();
        __hip_atomic_store(flag[r], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// one wavefront: lane r waits for source r's flag to reach the step; `error` (optional) is set to 1 + r of a source that did not arrive
// within timeout_ticks of the 100 MHz wall clock -- the wait ALWAYS ends (a peer that died must not hang the queue).
__global__ void __launch_bounds__(64) peer_wait_kernel(const unsigned long long* __restrict__ flags, int32_t n_src,
                                                       const unsigned long long* __restrict__ seq_base, unsigned long long seq_off,
                                                       long long timeout_ticks, int32_t* __restrict__ error)
{
    const unsigned long long want = seq_base[0] + seq_off;
    const long long t0 = (long long)wall_clock64();
    for (int r = threadIdx.x; r < n_src; r += 64) {
        while (__hip_atomic_load(&flags[r], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < want) {
            if ((long long)wall_clock64() - t0 > timeout_ticks) {
                if (error) atomicMax(error, 1 + r);
                break;
            }
            __builtin_amdgcn_s_sleep(8);
        }
    }
}

}  // namespace ssa

#include "ssa_access.hpp"   // the pass table of a sensor network (needs time_row, env_time_of and the propagators above)

// ============================================================================= C ABI
using namespace ssa;

// f(std::integral_constant<int, P>()) for the propagator `prop` (checked by consts_ok): the kernels' PROP template argument
template <class F> static void with_prop(int prop, F&& f)
{
    if (prop == SSA_PROP_FG) f(std::integral_constant<int, SSA_PROP_FG>());
    else if (prop == SSA_PROP_ELEMENTS) f(std::integral_constant<int, SSA_PROP_ELEMENTS>());
    else if (prop == SSA_PROP_HYBRID) f(std::integral_constant<int, SSA_PROP_HYBRID>());
    else f(std::integral_constant<int, SSA_PROP_J2_RK4>());
}
// ... and the tile kernels' MULTI: f(P, std::bool_constant<multi>())
template <class F> static void with_prop(int prop, bool multi, F&& f)
{
    with_prop(prop, [&](auto P) {
        if (multi) f(P, std::true_type());
        else f(P, std::false_type());
    });
}

extern "C" {

int ssa_abi_version(void) { return SSA_ABI_VERSION; }
const char* ssa_build_info(void) { return "libssa_hip gfx950 fp64 (" __DATE__ " " __TIME__ ")"; }

static int device_cu_count()
{
    static int cached = 0;   // per process: one GPU per process (the launcher model of this library)
    if (cached <= 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached = n;
    }
    return cached;
}
static int post_parts(int64_t n_obj, int32_t n_env)
{
    (void)n_env;
    int64_t want = (n_obj + POST_T - 1) / POST_T;   // one payload row per thread (the statistics slice strides)
    if (want < 1) want = 1;
    if (want > 256) want = 256;
    return (int)want;
}
// the checks of ssa_consts every fused launch shares: observation model, propagator, RK4 substeps
// (the propagator's half alone: what an entry that forms no measurement judges -- ssa_access_sensors_f64)
static bool propagator_ok(const ssa_consts* c)
{
    if (c->propagator != SSA_PROP_FG && c->propagator != SSA_PROP_ELEMENTS && c->propagator != SSA_PROP_J2_RK4 && c->propagator != SSA_PROP_HYBRID) return false;
    return c->propagator != SSA_PROP_J2_RK4 || (c->rk4_substeps >= 1 && c->rk4_substeps <= 4096);
}
static bool consts_ok(const ssa_consts* c)
{
    if (c->obs_type != SSA_OBS_AER && c->obs_type != SSA_OBS_XYZ) return false;
    return propagator_ok(c);
}
// the tile kernels' grid: tiles per wavefront T = ceil(tiles / resident wavefront slots); G = ceil(tiles / T) wavefronts.  T = 1:
// the one-tile instance, else the grid-stride walk.
// `arg`, the tile kernels' first argument: the grid-stride walk's tile count; the one-tile instance's count of WHOLE tiles (a tile below it
// takes the LDS-DMA path, decided from a preloaded argument: SSA_TILE_KERNEL)
struct TileGrid {
    int64_t ntiles, per_wave;
    int nwork, arg;
};
static TileGrid tile_grid(int64_t total)
{
    TileGrid g;
    g.ntiles = (total + OBJ_PER_WAVE - 1) / OBJ_PER_WAVE;
    const int64_t slots = (int64_t)device_cu_count() * 4 * SSA_STEP_WAVES;
    g.per_wave = (g.ntiles + slots - 1) / slots;
    g.nwork = (int)((g.ntiles + g.per_wave - 1) / g.per_wave);
    g.arg = g.per_wave != 1 ? (int)g.ntiles : (int)(total / OBJ_PER_WAVE);
    return g;
}
// ---- the argument rules the entries share, each written once.  An entry calls them in ITS order: the order decides the code of a block
// that breaks two rules, and it differs between siblings (tests/test_refusal_order_host.py pins it).
// several envs without whole tiles per env (a tile's env is wave-uniform); a * b * c rows below 2^31 (they are addressed with 32 bits); a
// row of SSA_MAX_SENSORS action words, there and aligned to its 32 bytes; no more envs by value than SSA_LAUNCH_INLINE_ENVS carries
static bool ragged_envs(int64_t n_obj, int32_t n_env) { return n_env > 1 && (n_obj % OBJ_PER_WAVE) != 0; }
static bool ragged_envs(const ssa_step_params* p) { return ragged_envs(p->n_obj, p->n_env); }
static bool rows_fit(int64_t a, int64_t b, int64_t c = 1) { return a * b * c < ((int64_t)1 << 31); }
static bool row_aligned(const int32_t* row) { return row && ((uintptr_t)row % (SSA_MAX_SENSORS * sizeof(int32_t))) == 0; }
static bool inline_envs_fit(const ssa_step_params* p) { return !(p->launch_mask & SSA_LAUNCH_INLINE_ENVS) || p->n_env <= SSA_INLINE_ENVS; }
// a network's sites: 1..SSA_MAX_SENSORS of them, no NaN elevation mask; SSA_OK or the refusal.  `between`: a refusal of the caller's
// that ranks behind the count and before the masks
static int sites_ok(const ssa_sensor_params* sp, int between = SSA_OK)
{
    if (sp->n_sensor < 1 || sp->n_sensor > SSA_MAX_SENSORS) return SSA_E_INVALID;
    if (between != SSA_OK) return between;
    for (int k = 0; k < sp->n_sensor; ++k)
        if (!(sp->obs_limit[k] == sp->obs_limit[k])) return SSA_E_INVALID;
    return SSA_OK;
}
// ... of the one-env entries: several envs are the *_envs entries'
static int sensors_ok(const ssa_sensor_params* sp, const ssa_step_params* p) { return sites_ok(sp, p->n_env != 1 ? SSA_E_UNSUPPORTED : SSA_OK); }
// ... and of the sensors' own noise tables, where the measurement noise is read
static bool noise_stride_ok(const ssa_sensor_params* sp)
{
    return sp->zn_stride_sensor >= 0 && (sp->n_sensor <= 1 || sp->zn_stride_sensor != 0);
}
// ... and of the sensors' measurement kinds (ssa_sensor_params.angles_only): no bit at or above n_sensor, and none at all unless the
// observation is az-el-range.  Every entry applies it behind all its other rules, so that no older refusal changes its rank
static bool kinds_ok(const ssa_consts* c, const ssa_sensor_params* sp)
{
    const uint32_t bits = (uint32_t)sp->angles_only;
    return bits == 0 || ((bits >> sp->n_sensor) == 0 && c->obs_type == SSA_OBS_AER);
}
// ... and of the sensors that see sunlit objects only (ssa_sensor_params.sunlit_only): no bit at or above n_sensor, and with any bit set
// a Sun table (32-byte rows) and a shadow radius that is a number >= 0.  Whatever obs_type is.  Applied with kinds_ok, behind all else
static bool illumination_ok(const ssa_sensor_params* sp)
{
    const uint32_t bits = (uint32_t)sp->sunlit_only;
    return bits == 0 || ((bits >> sp->n_sensor) == 0 && sp->sun && ((uintptr_t)sp->sun & 31) == 0 && sp->shadow_radius >= 0.0);
}
// ... and of the moving sensors (ssa_step_params.site_moving): no bit at or above n_sensor, not bit 0 (sensor 0 is the primary observer
// of ssa_consts), and with any bit set a table of 128-byte rows, a limb radius that is a number >= 0 and the az-el-range observation
static bool moving_ok(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp)
{
    const uint32_t bits = (uint32_t)p->site_moving;
    return bits == 0 || ((bits >> sp->n_sensor) == 0 && !(bits & 1u) && p->site_rows && ((uintptr_t)p->site_rows & 127) == 0 &&
                         p->limb_radius >= 0.0 && c->obs_type == SSA_OBS_AER);
}
// ... which an entry without a network cannot honour: its kernels read the one observer of ssa_consts.  Behind all its other rules
static int no_moving_sites(const ssa_step_params* p) { return p->site_moving != 0 ? SSA_E_UNSUPPORTED : SSA_OK; }
static bool sensor_tail_ok(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp)
{
    return kinds_ok(c, sp) && illumination_ok(sp) && moving_ok(c, p, sp);
}
// a network's sites as the kernels take them that read neither its action words nor its record destination
static ssa_sensor_params idle_sites(const ssa_sensor_params* sp)
{
    ssa_sensor_params s = *sp;
    s.upd = nullptr;
    for (int q = 0; q < SSA_MAX_SENSORS; ++q) s.action[q] = -1;
    return s;
}

// the argument rules of a step launch, in the order step_launch has always applied them; SSA_OK leaves the launch's grid in `g`
static int step_args(const ssa_consts* c, const ssa_step_params* p, bool sens, TileGrid& g)
{
    if (!c || !p || p->n_obj <= 0 || p->n_env <= 0) return SSA_E_INVALID;
    if (!p->x_true_in || !p->x_true_out || !p->x_in || !p->x_out || !p->P_in || !p->P_out || !p->status ||
        !p->obs || !p->metrics || !p->trans || !p->env_time || !p->z_noise || !p->stat_ws)
        return SSA_E_INVALID;
    if (sens) {   // (the actions are the sensors'; the env's action word and record are not read)
    } else if (p->launch_mask & SSA_LAUNCH_INLINE_ENVS) {
        if (!inline_envs_fit(p) || (p->launch_mask & SSA_LAUNCH_INLINE_ACTION)) return SSA_E_INVALID;
    } else if (p->launch_mask & SSA_LAUNCH_INLINE_ACTION) {
        if (p->n_env != 1) return SSA_E_INVALID;
    } else if (!p->actions) return SSA_E_INVALID;
    if ((p->launch_mask & SSA_LAUNCH_FOLD_INSIDE) &&
        (!p->stat_shards || !p->stats || (p->launch_mask & SSA_LAUNCH_DEFER_FOLD))) return SSA_E_INVALID;
    if (p->spos_tiles && !p->stat_shards) return SSA_E_INVALID;
    if (p->fail_log && (!p->fail_count || p->fail_cap <= 0)) return SSA_E_INVALID;
    if ((p->launch_mask & SSA_LAUNCH_MIRROR_F32) && !p->stat_shards) return SSA_E_UNSUPPORTED;   // (the post kernel writes aer_out in double)
    // (the statistics of the one-launch paths: the post kernel's arg-max would speak storage positions; several envs: one table row per env,
    // indices within the env, whole tiles per env)
    if (p->obj_ids && (!p->stat_shards || ragged_envs(p))) return SSA_E_UNSUPPORTED;
    if ((p->spos_tiles || p->spos_tiles_prev) && ragged_envs(p)) return SSA_E_UNSUPPORTED;
    if (!consts_ok(c)) return SSA_E_INVALID;
    if (p->aer_cols != 0 && p->aer_cols != 1 && p->aer_cols != 4) return SSA_E_INVALID;
    if (!rows_fit(p->n_env, p->n_obj)) return SSA_E_INVALID;
    g = tile_grid((int64_t)p->n_env * p->n_obj);
    const bool fast_stats = p->stat_shards != nullptr;   // statistics by the common-path kernel's atomics
    const bool defer = fast_stats && (p->launch_mask & SSA_LAUNCH_DEFER_FOLD);
    if (defer && p->stat_shards_prev && (!p->stats_prev || p->stat_shards_prev == p->stat_shards)) return SSA_E_INVALID;
    if (p->launch_mask & SSA_LAUNCH_STATS_FROM_METRICS) {   // (the one-tile step kernel of one env, deferred fold: see the bit)
        if (!defer || sens || p->n_env != 1 || g.per_wave != 1 || (p->launch_mask & SSA_LAUNCH_FOLD_INSIDE) || p->stat_shards_clear)
            return SSA_E_UNSUPPORTED;
        if (p->stat_shards_prev && !p->metrics_prev) return SSA_E_INVALID;
    }
    return SSA_OK;
}
// The plain launch form: what step_plain_kernel (ActPlain) was compiled for.  Every condition is one that process_wave<.., ActPlain> holds
// as a constant; a block that breaks any of them -- or carries SSA_LAUNCH_GENERIC -- gets step_fast_kernel.  (launch_mask bits 1 / 2 / 4:
// the diagnostic selection of single launches; SSA_LAUNCH_STATS_FROM_METRICS has passed step_args: one env, one tile per wavefront, a
// deferred fold, no SSA_LAUNCH_FOLD_INSIDE, no stat_shards_clear -- restated here so that the predicate stands on its own.)
static bool step_plain_form(const ssa_consts* c, const ssa_step_params* p, bool sens, const TileGrid& g)
{
    const uint32_t need = SSA_LAUNCH_DEFER_FOLD | SSA_LAUNCH_STATS_FROM_METRICS;
    const uint32_t none = SSA_LAUNCH_INLINE_ACTION | SSA_LAUNCH_INLINE_ENVS | SSA_LAUNCH_FOLD_INSIDE | SSA_LAUNCH_MIRROR_F32 | SSA_LAUNCH_GENERIC | 7u;
    return !sens && p->n_env == 1 && g.per_wave == 1 && (p->launch_mask & need) == need && !(p->launch_mask & none) && p->actions &&
           !p->aer_out && !p->obs_mirror && !p->spos_tiles && !p->spos_tiles_prev && !p->stat_shards_clear && c->update_interval <= 1 &&
           !(c->flags & SSA_FLAG_RESAMPLE) && c->obs_type == SSA_OBS_AER;
}

// sens: a sensor network's step (ssa_env_step_sensors_f64; checked by the caller) -- step_sensors_kernel instead of step_fast_kernel
// envs: ... in each of n_env envs (ssa_env_step_sensors_envs_f64; checked by the caller) -- vector_sensors_kernel
static int step_launch(const ssa_consts* c, const ssa_step_params* p, void* stream, hipEvent_t ev0, hipEvent_t ev1,
                       const ssa_sensor_params* sens = nullptr, const ssa_sensor_envs_params* envs = nullptr)
{
    TileGrid g;
    const int rc = step_args(c, p, sens != nullptr, g);
    if (rc != SSA_OK) return rc;
    if (sens && !sensor_tail_ok(c, p, sens)) return SSA_E_INVALID;
    if (!sens && no_moving_sites(p) != SSA_OK) return no_moving_sites(p);
    StepK k;
    k.c = *c;
    k.p = *p;
    const bool fast_stats = p->stat_shards != nullptr;   // statistics by the common-path kernel's atomics
    const bool defer = fast_stats && (p->launch_mask & SSA_LAUNCH_DEFER_FOLD);
    const bool from_metrics = (p->launch_mask & SSA_LAUNCH_STATS_FROM_METRICS) != 0;
    const int nfold = (defer && p->stat_shards_prev) ? (from_metrics ? STAT_SERVICE_WAVES : p->n_env) : 0;
    dim3 grid((unsigned)(g.nwork + nfold)), block(64);
    const int nparts = post_parts(p->n_obj, p->n_env);
    StatAcc* parts = (StatAcc*)p->stat_ws;
    hipStream_t s = (hipStream_t)stream;
    const unsigned mask = (p->launch_mask & 7u) ? (p->launch_mask & 7u) : 7u;   // diagnostic: time one launch alone
    const int prop = c->propagator;
    if ((mask & 1u) && envs) {
        VecSensK kv;
        kv.k = k;
        kv.k.p.upd = nullptr;
        kv.k.p.actions = nullptr;
        kv.s = idle_sites(sens);
        kv.v = *envs;
        with_prop(prop, g.per_wave != 1, [&](auto P, auto M) {
            hipExtLaunchKernelGGL((vector_sensors_kernel<P, M>), grid, block, 0, s, ev0, ev1, 0, g.arg, g.nwork, p->P_in, p->x_in, p->x_true_in, p->status, kv);
        });
    } else if ((mask & 1u) && sens) {
        SensK ks;
        ks.k = k;
        ks.k.p.upd = nullptr;
        ks.k.p.actions = nullptr;
        ks.k.p.launch_mask &= ~SSA_LAUNCH_INLINE_ACTION;
        ks.s = *sens;
        with_prop(prop, g.per_wave != 1, [&](auto P, auto M) {
            hipExtLaunchKernelGGL((step_sensors_kernel<P, M>), grid, block, 0, s, ev0, ev1, 0, g.arg, g.nwork, p->P_in, p->x_in, p->x_true_in, p->status, ks);
        });
    } else if ((mask & 1u) && step_plain_form(c, p, false, g)) {   // (the plain form: the instance compiled for it)
        PlainK kp;
        kp.k = k;
        with_prop(prop, [&](auto P) {
            hipExtLaunchKernelGGL((step_plain_kernel<P, false>), grid, block, 0, s, ev0, ev1, 0, g.arg, g.nwork, p->P_in, p->x_in, p->x_true_in, p->status, kp);
        });
    } else if (mask & 1u) {   // (ev0, ev1: dispatch timestamps of this kernel for ssa_env_step_profiled_f64, else null)
        with_prop(prop, g.per_wave != 1, [&](auto P, auto M) {
            hipExtLaunchKernelGGL((step_fast_kernel<P, M>), grid, block, 0, s, ev0, ev1, 0, g.arg, g.nwork, p->P_in, p->x_in, p->x_true_in, p->status, k);
        });
    }
    if (fast_stats) {   // (the aer_out payload, if any, was the step kernel's epilogue) a one-wave fold finishes the step
                        // (2 launches), unless deferred (1 launch)
        if ((p->launch_mask & SSA_LAUNCH_FOLD_INSIDE) && g.per_wave == 1) return launch_status();   // (folded by the step kernel's last wavefronts)
        if ((mask & 6u) && !defer && p->stats)   // (stats NULL: the caller consumes the raw shard words, see stat_shards_clear)
            hipLaunchKernelGGL(reward_fold_kernel, dim3(p->n_env), dim3(64), 0, s, (unsigned long long*)p->stat_shards, p->stats,
                               (const unsigned long long*)p->spos_tiles, p->n_obj);
        return launch_status();
    }
    if (mask & 2u)
        with_prop(prop, [&](auto P) { hipLaunchKernelGGL(step_post_kernel<P>, dim3(nparts, p->n_env), dim3(POST_T), 0, s, k, parts, nparts); });
    // folds the per-block statistics
    if ((mask & 4u) && p->stats)
        hipLaunchKernelGGL(reward_final_kernel, dim3(p->n_env), dim3(64), 0, s, (const StatAcc*)parts, p->stats, nparts);
    return launch_status();
}
int32_t ssa_stats_from_metrics_waves(int64_t n_obj, int32_t n_env)
{
    if (n_obj <= 0 || n_env != 1) return 0;
    return tile_grid(n_obj).per_wave == 1 ? STAT_SERVICE_WAVES : 0;
}
int ssa_stats_fold_metrics_f64(const double* metrics, uint64_t* stat_shards, const uint64_t* spos_tiles, double* stats, int64_t n_obj,
                               void* stream)
{
    if (!metrics || !stat_shards || !stats || n_obj <= 0 || n_obj >= ((int64_t)1 << 31)) return SSA_E_INVALID;
    hipLaunchKernelGGL(reward_service_kernel, dim3(STAT_SERVICE_WAVES), dim3(64), 0, (hipStream_t)stream, metrics,
                       (unsigned long long*)stat_shards, stats, (const unsigned long long*)spos_tiles, n_obj);
    return launch_status();
}
int ssa_env_step_f64(const ssa_consts* c, const ssa_step_params* p, void* stream)
{
    return step_launch(c, p, stream, nullptr, nullptr);
}
int ssa_env_step_instance(const ssa_consts* c, const ssa_step_params* p)
{
    TileGrid g;
    const int rc = step_args(c, p, false, g);
    if (rc != SSA_OK) return rc;
    if (no_moving_sites(p) != SSA_OK) return no_moving_sites(p);
    return step_plain_form(c, p, false, g) ? 1 : 0;
}
int ssa_env_step_sensors_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp, void* stream)
{
    if (!c || !p || !sp) return SSA_E_INVALID;
    const int rc = sensors_ok(sp, p);
    if (rc != SSA_OK) return rc;
    if (!noise_stride_ok(sp)) return SSA_E_INVALID;
    return step_launch(c, p, stream, nullptr, nullptr, sp);
}
int ssa_env_step_sensors_envs_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp,
                                  const ssa_sensor_envs_params* envs, void* stream)
{
    if (!c || !p || !sp || !envs) return SSA_E_INVALID;
    if (sites_ok(sp) != SSA_OK || !noise_stride_ok(sp)) return SSA_E_INVALID;
    if ((p->launch_mask & SSA_LAUNCH_INLINE_ACTION) || !inline_envs_fit(p)) return SSA_E_INVALID;
    if (!(p->launch_mask & SSA_LAUNCH_INLINE_ENVS) && !row_aligned(envs->actions)) return SSA_E_INVALID;   // (by value: not read)
    if (ragged_envs(p) || (p->launch_mask & SSA_LAUNCH_STATS_FROM_METRICS)) return SSA_E_UNSUPPORTED;
    return step_launch(c, p, stream, nullptr, nullptr, sp, envs);
}
// dispatch-timestamp event pairs, created on first use (a ring, so that back-to-back launches can be timed
// without draining the queue after each of them)
static hipEvent_t g_prof_ev[SSA_PROFILE_SLOTS][2];
static bool g_prof_made[SSA_PROFILE_SLOTS];
int ssa_env_step_profiled_f64(const ssa_consts* c, const ssa_step_params* p, void* stream, int32_t slot)
{
    if (slot < 0 || slot >= SSA_PROFILE_SLOTS) return SSA_E_INVALID;
    if (!g_prof_made[slot]) {
        if (hipEventCreate(&g_prof_ev[slot][0]) != hipSuccess || hipEventCreate(&g_prof_ev[slot][1]) != hipSuccess) return SSA_E_LAUNCH;
        g_prof_made[slot] = true;
    }
    return step_launch(c, p, stream, g_prof_ev[slot][0], g_prof_ev[slot][1]);
}
int ssa_env_step_profile_ms(int32_t slot, float* kernel_ms)
{
    if (slot < 0 || slot >= SSA_PROFILE_SLOTS || !kernel_ms || !g_prof_made[slot]) return SSA_E_INVALID;
    if (hipEventSynchronize(g_prof_ev[slot][1]) != hipSuccess ||
        hipEventElapsedTime(kernel_ms, g_prof_ev[slot][0], g_prof_ev[slot][1]) != hipSuccess) return SSA_E_LAUNCH;
    return SSA_OK;
}
// the checks and the argument block shared by ssa_lookahead_f64 and ssa_lookahead_sensors_f64; SSA_OK or the refusal
static int lookahead_args(const ssa_consts* c, const ssa_step_params* p, const ssa_lookahead_out* o, LookK& k)
{
    if (!c || !p || !o || p->n_obj <= 0 || p->n_env <= 0) return SSA_E_INVALID;
    if (!p->x_true_in || !p->x_in || !p->P_in || !p->status || !p->trans || !p->env_time) return SSA_E_INVALID;
    if (!o->score || !o->status || !o->visible) return SSA_E_INVALID;
    if (!inline_envs_fit(p)) return SSA_E_INVALID;
    if (p->obj_ids && ragged_envs(p)) return SSA_E_UNSUPPORTED;   // (as the step)
    if (!consts_ok(c) || !rows_fit(p->n_env, p->n_obj)) return SSA_E_INVALID;
    k.k.c = *c;
    k.k.p = *p;
    k.o = *o;
    // the inputs only: every output of the step -- and the action / measurement noise -- is withheld from the kernel
    ssa_step_params& q = k.k.p;
    q.x_true_out = nullptr; q.x_out = nullptr; q.P_out = nullptr; q.obs = nullptr; q.metrics = nullptr; q.upd = nullptr;
    q.actions = nullptr; q.z_noise = nullptr; q.stats = nullptr; q.work = nullptr; q.stat_ws = nullptr;
    q.stat_shards = nullptr; q.stat_shards_prev = nullptr; q.stats_prev = nullptr; q.aer_out = nullptr; q.stat_shards_clear = nullptr;
    q.metrics_prev = nullptr;
    q.obs_mirror = nullptr; q.spos_tiles = nullptr; q.spos_tiles_prev = nullptr; q.fail_log = nullptr; q.fail_count = nullptr;
    q.fail_cap = 0;
    q.launch_mask = p->launch_mask & SSA_LAUNCH_INLINE_ENVS;
    return SSA_OK;
}
int ssa_lookahead_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_lookahead_out* o, void* stream)
{
    LookK k;
    const int rc = lookahead_args(c, p, o, k);
    if (rc != SSA_OK) return rc;
    if (no_moving_sites(p) != SSA_OK) return no_moving_sites(p);
    const TileGrid g = tile_grid((int64_t)p->n_env * p->n_obj);
    dim3 grid((unsigned)g.nwork), block(64);
    hipStream_t s = (hipStream_t)stream;
    with_prop(c->propagator, g.per_wave != 1, [&](auto P, auto M) {
        hipLaunchKernelGGL((lookahead_kernel<P, M>), grid, block, 0, s, g.arg, g.nwork, p->P_in, p->x_in, p->x_true_in, p->status, k);
    });
    return launch_status();
}
// ... and by a network's lookahead and forecast entries on top of it: the network's checks, and its sites in `sites`
// (envs: the *_envs entries -- several envs, whole tiles each)
static int lookahead_sensors_args(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp, const ssa_lookahead_out* o,
                                  bool envs, LookK& k, ssa_sensor_params& sites)
{
    if (!c || !p || !sp || !o) return SSA_E_INVALID;
    int rc = envs ? sites_ok(sp) : sensors_ok(sp, p);
    if (rc != SSA_OK) return rc;
    rc = lookahead_args(c, p, o, k);
    if (rc != SSA_OK) return rc;
    if (!rows_fit(p->n_env, sp->n_sensor, p->n_obj)) return SSA_E_INVALID;
    if (ragged_envs(p)) return SSA_E_UNSUPPORTED;
    sites = idle_sites(sp);
    return SSA_OK;
}
int ssa_lookahead_sensors_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp, const ssa_lookahead_out* o,
                              void* stream)
{
    LookSensK k;
    const int rc = lookahead_sensors_args(c, p, sp, o, false, k.k, k.s);
    if (rc != SSA_OK) return rc;
    if (!sensor_tail_ok(c, p, sp)) return SSA_E_INVALID;
    const TileGrid g = tile_grid(p->n_obj);
    dim3 grid((unsigned)g.nwork), block(64);
    hipStream_t s = (hipStream_t)stream;
    with_prop(c->propagator, g.per_wave != 1, [&](auto P, auto M) {
        hipLaunchKernelGGL((lookahead_sensors_kernel<P, M>), grid, block, 0, s, g.arg, g.nwork, p->P_in, p->x_in, p->x_true_in, p->status, k);
    });
    return launch_status();
}
int ssa_lookahead_sensors_envs_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp, const ssa_lookahead_out* o,
                                   void* stream)
{
    VecLookSensK k;
    const int rc = lookahead_sensors_args(c, p, sp, o, true, k.k, k.s);
    if (rc != SSA_OK) return rc;
    if (!sensor_tail_ok(c, p, sp)) return SSA_E_INVALID;
    const TileGrid g = tile_grid((int64_t)p->n_env * p->n_obj);
    dim3 grid((unsigned)g.nwork), block(64);
    hipStream_t s = (hipStream_t)stream;
    with_prop(c->propagator, g.per_wave != 1, [&](auto P, auto M) {
        hipLaunchKernelGGL((lookahead_sensor_envs_kernel<P, M>), grid, block, 0, s, g.arg, g.nwork, p->P_in, p->x_in, p->x_true_in, p->status, k);
    });
    return launch_status();
}
int ssa_forecast_sensors_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp, const ssa_forecast_params* f,
                             void* stream)
{
    if (!f) return SSA_E_INVALID;
    LookK lk;
    ForeSensK k;
    const int rc = lookahead_sensors_args(c, p, sp, &f->out, false, lk, k.s);
    if (rc != SSA_OK) return rc;
    if (f->n_steps < 1 || !sensor_tail_ok(c, p, sp)) return SSA_E_INVALID;
    k.k = lk.k;
    k.k.p.launch_mask = 0;   // (the time word is read from env_time: a resident tile's steps do not see SSA_LAUNCH_INLINE_ENVS)
    k.f = *f;
    const TileGrid g = tile_grid(p->n_obj);
    hipStream_t s = (hipStream_t)stream;
    with_prop(c->propagator, [&](auto P) { hipLaunchKernelGGL(forecast_sensors_kernel<P>, dim3(g.nwork), dim3(64), 0, s, k, (int)g.ntiles, g.nwork); });
    return launch_status();
}
int ssa_forecast_sensors_envs_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp, const ssa_forecast_params* f,
                                  void* stream)
{
    if (!f) return SSA_E_INVALID;
    LookK lk;
    VecForeSensK k;
    const int rc = lookahead_sensors_args(c, p, sp, &f->out, true, lk, k.s);
    if (rc != SSA_OK) return rc;
    if (f->n_steps < 1 || !sensor_tail_ok(c, p, sp)) return SSA_E_INVALID;
    k.k = lk.k;   // (launch_mask: SSA_LAUNCH_INLINE_ENVS alone survives lookahead_args, and the kernel reads inline_time by it)
    k.f = *f;
    const TileGrid g = tile_grid((int64_t)p->n_env * p->n_obj);
    hipStream_t s = (hipStream_t)stream;
    with_prop(c->propagator, [&](auto P) { hipLaunchKernelGGL(forecast_sensor_envs_kernel<P>, dim3(g.nwork), dim3(64), 0, s, k, (int)g.ntiles, g.nwork); });
    return launch_status();
}
int ssa_dryrun_sensors_envs_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp, const ssa_dryrun_sensors_params* d,
                                void* stream)
{
    if (!d) return SSA_E_INVALID;
    // (the forecast's rules with d->out as every required output)
    const ssa_lookahead_out o = {d->out, (int32_t*)d->out, (uint8_t*)d->out, nullptr, nullptr, nullptr};
    LookK lk;
    DryRunK k;
    const int rc = lookahead_sensors_args(c, p, sp, &o, true, lk, k.s);
    if (rc != SSA_OK) return rc;
    if (d->n_steps < 1 || d->n_obj_caller < 1 || !row_aligned(d->actions)) return SSA_E_INVALID;
    if (!rows_fit(p->n_env, sp->n_sensor, d->n_steps) || !sensor_tail_ok(c, p, sp)) return SSA_E_INVALID;
    k.k = lk.k;
    k.k.p.launch_mask = 0;   // (the time words are read from env_time: a resident tile's steps do not see SSA_LAUNCH_INLINE_ENVS)
    k.d = *d;
    const TileGrid g = tile_grid((int64_t)p->n_env * p->n_obj);
    hipStream_t s = (hipStream_t)stream;
    with_prop(c->propagator, [&](auto P) { hipLaunchKernelGGL(dryrun_sensors_kernel<P>, dim3(g.nwork), dim3(64), 0, s, k, (int)g.ntiles, g.nwork); });
    return launch_status();
}
int ssa_dryrun_totals_f64(const double* records, int32_t n_env, int32_t n_steps, int32_t n_sensor, double* total, void* stream)
{
    if (!records || !total || n_env < 1 || n_steps < 1 || n_sensor < 1 || n_sensor > SSA_MAX_SENSORS) return SSA_E_INVALID;
    if (!rows_fit(n_env, n_sensor, n_steps)) return SSA_E_INVALID;
    hipLaunchKernelGGL(dryrun_totals_kernel, dim3((unsigned)nblk((int64_t)n_env * SSA_LOOK_NSCORE, 64)), dim3(64), 0, (hipStream_t)stream, records,
                       (int)n_env, (int)n_steps, (int)n_sensor, total);
    return launch_status();
}
int ssa_dryrun_gather_f64(const ssa_dryrun_gather_params* g, void* stream)
{
    if (!g || g->n_obj < 1 || g->n_env < 1 || g->n_cand < 1 || g->n_rows < 1 || g->n_rows % 4 || g->reserved) return SSA_E_INVALID;
    if (!g->ids || !g->env_time || !g->x_true_in || !g->x_in || !g->P_in || !g->status_in || !g->x_true_out || !g->x_out || !g->P_out ||
        !g->status_out || !g->time_out)
        return SSA_E_INVALID;
    // (n_obj and E * B first: every product below stays inside 64 bits)
    if (g->n_obj >= ((int64_t)1 << 31) || !rows_fit(g->n_env, g->n_obj) || !rows_fit(g->n_env, g->n_cand) ||
        !rows_fit((int64_t)g->n_env * g->n_cand, g->n_rows))
        return SSA_E_INVALID;
    for (const double* ptr : {g->x_true_in, g->x_in, g->P_in, (const double*)g->x_true_out, (const double*)g->x_out, (const double*)g->P_out})
        if ((uintptr_t)ptr % 16) return SSA_E_INVALID;
    const int64_t rows = (int64_t)g->n_env * g->n_cand * g->n_rows;
    hipLaunchKernelGGL(dryrun_gather_kernel, dim3(nblk(rows, SSA_GATHER_ROWS)), dim3(32 * SSA_GATHER_ROWS), 0, (hipStream_t)stream, *g);
    return launch_status();
}
// the checks and the argument block shared by ssa_env_rollout_f64 and ssa_env_rollout_sensors_f64 (sens: r->actions is not read); SSA_OK or
// the refusal
// (ids_per_env: the kernel honours obj_ids per env -- whole tiles per env, the caller's check)
static int rollout_args(const ssa_consts* c, const ssa_step_params* p, const ssa_rollout_params* r, bool sens, RollK& rk, bool ids_per_env = false)
{
    if (!c || !p || !r || p->n_obj <= 0 || p->n_env <= 0 || r->n_steps < 1 || r->history < 2) return SSA_E_INVALID;
    if (r->slot_out < 0 || r->slot_out >= r->history) return SSA_E_INVALID;
    if (!r->x_true_ring || !r->x_ring || !r->P_ring || !r->obs_ring || !r->metrics_ring || !r->stats_ring || (!sens && !r->actions) ||
        !r->stat_shards)
        return SSA_E_INVALID;
    if (!p->status || !p->trans || !p->env_time || !p->z_noise) return SSA_E_INVALID;
    if (!consts_ok(c)) return SSA_E_INVALID;
    if (!rows_fit(p->n_env, p->n_obj)) return SSA_E_INVALID;
    if (r->spos_tiles && ragged_envs(p)) return SSA_E_UNSUPPORTED;
    rk.k.c = *c;
    rk.k.p = *p;
    rk.k.p.aer_out = nullptr;
    rk.k.p.spos_tiles = nullptr;
    rk.k.p.spos_tiles_prev = nullptr;
    if (p->obj_ids && p->n_env != 1 && !ids_per_env) return SSA_E_UNSUPPORTED;
    rk.r = *r;
    return SSA_OK;
}
// the fold of a rollout's per-step statistics, behind its kernel
static int rollout_fold(const ssa_step_params* p, const ssa_rollout_params* r, int64_t ntiles, hipStream_t s)
{
    hipLaunchKernelGGL(rollout_fold_kernel, dim3(r->n_steps, p->n_env), dim3(64), 0, s, (unsigned long long*)r->stat_shards, r->stats_ring,
                       p->n_env, r->n_steps, r->slot_out, r->history, (const unsigned long long*)r->spos_tiles, p->n_obj, ntiles);
    return launch_status();
}
int ssa_env_rollout_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_rollout_params* r, void* stream)
{
    RollK rk;
    const int rc = rollout_args(c, p, r, false, rk);
    if (rc != SSA_OK) return rc;
    if (no_moving_sites(p) != SSA_OK) return no_moving_sites(p);
    const TileGrid g = tile_grid((int64_t)p->n_env * p->n_obj);
    hipStream_t s = (hipStream_t)stream;
    with_prop(c->propagator, [&](auto P) { hipLaunchKernelGGL(rollout_kernel<P>, dim3(g.nwork), dim3(64), 0, s, rk, (int)g.ntiles, g.nwork); });
    return rollout_fold(p, r, g.ntiles, s);
}
// ... and by a network's two rollout entries on top of it: the network's checks, the schedule's rows (`actions`) in place of the env's
// action words and record ring, and its sites in `sites` (envs: ssa_env_rollout_sensors_envs_f64 -- several envs, whole tiles each)
static int rollout_sensors_args(const ssa_consts* c, const ssa_step_params* p, const ssa_rollout_params* r, const ssa_sensor_params* sp,
                                const int32_t* actions, bool envs, RollK& rk, ssa_sensor_params& sites)
{
    if (!c || !p || !r || !sp) return SSA_E_INVALID;
    int rc = rollout_args(c, p, r, true, rk, envs);
    if (rc != SSA_OK) return rc;
    rc = envs ? sites_ok(sp) : sensors_ok(sp, p);
    if (rc != SSA_OK) return rc;
    if (!noise_stride_ok(sp)) return SSA_E_INVALID;
    if (envs && (p->launch_mask & SSA_LAUNCH_INLINE_ENVS)) return SSA_E_INVALID;   // (a resident tile's steps read the time words from memory)
    if (ragged_envs(p)) return SSA_E_UNSUPPORTED;
    if (!row_aligned(actions)) return SSA_E_INVALID;
    rk.r.actions = nullptr;
    rk.r.upd_ring = nullptr;
    sites = idle_sites(sp);
    return SSA_OK;
}
int ssa_env_rollout_sensors_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_rollout_params* r, const ssa_sensor_params* sp,
                                const ssa_rollout_sensors_params* rs, void* stream)
{
    if (!rs) return SSA_E_INVALID;
    RollSensK rk;
    const int rc = rollout_sensors_args(c, p, r, sp, rs->actions, false, rk.k, rk.s);
    if (rc != SSA_OK) return rc;
    if (!sensor_tail_ok(c, p, sp)) return SSA_E_INVALID;
    rk.rs = *rs;
    const TileGrid g = tile_grid(p->n_obj);
    hipStream_t s = (hipStream_t)stream;
    with_prop(c->propagator, [&](auto P) { hipLaunchKernelGGL(rollout_sensors_kernel<P>, dim3(g.nwork), dim3(64), 0, s, rk, (int)g.ntiles, g.nwork); });
    return rollout_fold(p, r, g.ntiles, s);
}
int ssa_env_rollout_sensors_envs_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_rollout_params* r, const ssa_sensor_params* sp,
                                     const ssa_rollout_sensors_envs_params* re, void* stream)
{
    if (!re) return SSA_E_INVALID;
    VecRollSensK rk;
    const int rc = rollout_sensors_args(c, p, r, sp, re->actions, true, rk.k, rk.s);
    if (rc != SSA_OK) return rc;
    if (!re->stats_out || !sensor_tail_ok(c, p, sp)) return SSA_E_INVALID;
    rk.v = *re;
    const TileGrid g = tile_grid((int64_t)p->n_env * p->n_obj);
    hipStream_t s = (hipStream_t)stream;
    with_prop(c->propagator, [&](auto P) { hipLaunchKernelGGL(rollout_sensor_envs_kernel<P>, dim3(g.nwork), dim3(64), 0, s, rk, (int)g.ntiles, g.nwork); });
    hipLaunchKernelGGL(rollout_fold_steps_kernel, dim3(r->n_steps, p->n_env), dim3(64), 0, s, (unsigned long long*)r->stat_shards, re->stats_out,
                       r->stats_ring, p->n_env, r->n_steps, r->slot_out, r->history, (const unsigned long long*)r->spos_tiles, p->n_obj, g.ntiles);
    return launch_status();
}
int64_t ssa_closed_loop_workspace_bytes(int64_t n_obj, int32_t n_env)
{
    if (n_obj <= 0 || n_env != 1) return 0;
    const int64_t ntiles = (n_obj + OBJ_PER_WAVE - 1) / OBJ_PER_WAVE;
    if (ntiles >= ((int64_t)1 << 30)) return 0;
    return cl_layout((int)ntiles).total * 8;
}
// wavefronts of closed_loop_kernel<prop> the device holds at once (the runtime's occupancy figure x compute units)
static int64_t closed_loop_capacity(int prop)
{
    static int64_t cached[4] = {0, 0, 0, 0};
    if (cached[prop] <= 0) {
        int per_cu = 0;
        hipError_t e;
        with_prop(prop, [&](auto P) { e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, closed_loop_kernel<P>, 64, 0); });
        if (e != hipSuccess || per_cu <= 0) return 0;
        cached[prop] = (int64_t)per_cu * device_cu_count();
    }
    return cached[prop];
}
int ssa_env_closed_loop_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_closed_loop_params* r, void* stream)
{
    if (!c || !p || !r || p->n_obj <= 0 || r->n_steps < 1 || r->history < 2) return SSA_E_INVALID;
    if (r->slot_out < 0 || r->slot_out >= r->history) return SSA_E_INVALID;
    if (!r->x_true_ring || !r->x_ring || !r->P_ring || !r->obs_ring || !r->metrics_ring || !r->stats_out || !r->actions || !r->workspace)
        return SSA_E_INVALID;
    if (!p->status || !p->trans || !p->env_time || !p->z_noise) return SSA_E_INVALID;
    if (r->agent < SSA_AGENT_NAIVE_GREEDY || r->agent > SSA_AGENT_VEL_ERROR) return SSA_E_INVALID;
    if (!consts_ok(c)) return SSA_E_INVALID;
    if (p->n_env != 1) return SSA_E_UNSUPPORTED;
    if ((p->obj_ids != nullptr) != (r->slot_of != nullptr)) return SSA_E_INVALID;     // (a storage layout comes with its inverse table)
    const int64_t ntiles = (p->n_obj + OBJ_PER_WAVE - 1) / OBJ_PER_WAVE;
    const int64_t cap = closed_loop_capacity(c->propagator);
    const ClLayout L = cl_layout((int)ntiles);
    if (ntiles + L.ng + 1 > cap) return SSA_E_UNSUPPORTED;   // every wavefront (compute + service) must be resident: the decision is a grid-wide exchange
    if (r->workspace_bytes < L.total * 8) return SSA_E_INVALID;
    if (r->wait_ticks < 0 || (r->flags & ~(SSA_LOOP_ARGMAX_SPOS | SSA_LOOP_DEBUG_WITHHOLD))) return SSA_E_INVALID;
    if (no_moving_sites(p) != SSA_OK) return no_moving_sites(p);
    LoopK lk;
    lk.k.c = *c;
    lk.k.p = *p;
    lk.k.p.aer_out = nullptr;
    lk.k.p.spos_tiles = nullptr;
    lk.k.p.spos_tiles_prev = nullptr;
    lk.c = *r;
    hipStream_t s = (hipStream_t)stream;
    // counters, flags: zero (a memset node: capturable)
    if (hipMemsetAsync(r->workspace, 0, (size_t)L.parts * 8, s) != hipSuccess) return SSA_E_LAUNCH;
    int nwork = (int)ntiles;
    const dim3 grid((unsigned)(nwork + L.ng + 1));
    // A COOPERATIVE launch: the decision is a grid-wide exchange, so every wavefront must be resident at once -- with a cooperative
    // launch that is the runtime's guarantee (it refuses a grid the device cannot hold next to what else is running), not only this
    // function's occupancy estimate above.
    void* args[3] = {(void*)&lk, (void*)&nwork, (void*)&nwork};
    const void* fn = nullptr;
    with_prop(c->propagator, [&](auto P) { fn = (const void*)closed_loop_kernel<P>; });
    const hipError_t ce = hipLaunchCooperativeKernel(fn, grid, dim3(64), args, 0, s);
    if (ce == hipErrorCooperativeLaunchTooLarge) {
        (void)hipGetLastError();
        return SSA_E_UNSUPPORTED;          // (the device cannot hold the grid right now: the caller takes the per-step launches)
    }
    if (ce != hipSuccess) {
        fprintf(stderr, "libssa_hip: cooperative launch of the closed loop failed: %s (%s)\n", hipGetErrorName(ce), hipGetErrorString(ce));
        (void)hipGetLastError();
        return SSA_E_LAUNCH;
    }
    return launch_status();
}
int ssa_stats_fold_f64(uint64_t* stat_shards, double* stats, int32_t n_env, void* stream)
{
    if (!stat_shards || !stats || n_env <= 0) return SSA_E_INVALID;
    hipLaunchKernelGGL(reward_fold_kernel, dim3(n_env), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)stat_shards, stats,
                       (const unsigned long long*)nullptr, (int64_t)0);
    return launch_status();
}
int ssa_stats_fold_spos_f64(uint64_t* stat_shards, const uint64_t* spos_tiles, double* stats, int64_t n_obj, int32_t n_env, void* stream)
{
    if (!stat_shards || !stats || n_env <= 0 || n_obj <= 0) return SSA_E_INVALID;
    if (spos_tiles && ragged_envs(n_obj, n_env)) return SSA_E_UNSUPPORTED;
    hipLaunchKernelGGL(reward_fold_kernel, dim3(n_env), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)stat_shards, stats,
                       (const unsigned long long*)spos_tiles, n_obj);
    return launch_status();
}
int64_t ssa_env_step_work_bytes(int64_t n_obj, int32_t n_env)
{
    (void)n_obj; (void)n_env;
    return 16;   // `work` is not used any more (the exception queue is gone); a token size keeps old callers valid
}

int ssa_reward_stats_f64(const double* metrics, const int32_t* status, double* stats, void* workspace, int64_t n_obj,
                         int32_t n_env, void* stream)
{
    if (!metrics || !status || !stats || !workspace || n_obj <= 0 || n_env <= 0) return SSA_E_INVALID;
    int64_t want = (n_obj + (int64_t)STAT_T * STAT_ILP - 1) / ((int64_t)STAT_T * STAT_ILP);
    int nparts = (int)(want < 1 ? 1 : (want > STAT_MAX_PARTS / 4 ? STAT_MAX_PARTS / 4 : want));
    StatAcc* parts = (StatAcc*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(reward_partial_kernel, dim3(nparts, n_env), dim3(STAT_T), 0, s, metrics, status, parts, n_obj, nparts);
    hipLaunchKernelGGL(reward_final_kernel, dim3(n_env), dim3(64), 0, s, (const StatAcc*)parts, stats, nparts);
    return launch_status();
}
int64_t ssa_reward_stats_workspace_bytes(int32_t n_env)
{
    return (int64_t)(n_env < 1 ? 1 : n_env) * 256 * (int64_t)sizeof(StatAcc) + 64;
}

int ssa_propagate_f64(const double* x_in, double* x_out, int64_t n, double dt, int32_t propagator, void* stream)
{
    if (n == 0) return SSA_OK;
    if (!x_in || !x_out || n < 0) return SSA_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (propagator == SSA_PROP_FG) hipLaunchKernelGGL(propagate_kernel<1>, dim3(nblk(n, 64)), dim3(64), 0, s, x_in, x_out, n, dt);
    else if (propagator == SSA_PROP_ELEMENTS) hipLaunchKernelGGL(propagate_kernel<0>, dim3(nblk(n, 64)), dim3(64), 0, s, x_in, x_out, n, dt);
    else if (propagator == SSA_PROP_HYBRID) hipLaunchKernelGGL(propagate_hybrid_kernel, dim3(nblk(n, 64)), dim3(64), 0, s, x_in, x_out, n, dt);
    else return SSA_E_INVALID;
    return launch_status();
}

int ssa_propagate_j2_f64(const double* x_in, double* x_out, int64_t n, double dt, double j2, double r_eq, int32_t substeps,
                         void* stream)
{
    if (n == 0) return SSA_OK;
    if (!x_in || !x_out || n < 0 || substeps < 1 || substeps > 4096) return SSA_E_INVALID;
    J2Params q = {j2, r_eq, substeps};
    hipLaunchKernelGGL(propagate_j2_kernel, dim3(nblk(n, 64)), dim3(64), 0, (hipStream_t)stream, x_in, x_out, n, dt, q);
    return launch_status();
}

int ssa_kepler_elements_f64(const double* x_in, double* coe, int64_t n, double dt, void* stream)
{
    if (!x_in || !coe || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(elements_kernel, dim3(nblk(n, 64)), dim3(64), 0, (hipStream_t)stream, x_in, coe, n, dt);
    return launch_status();
}

int ssa_robust_cholesky6_f64(const double* A, double* U, int32_t* rung, int64_t n, void* stream)
{
    if (!A || !U || !rung || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(cholesky_kernel, dim3(nblk(n, 64)), dim3(64), 0, (hipStream_t)stream, A, U, rung, n);
    return launch_status();
}

int ssa_ladder_probe_f64(const double* A, double scale, int32_t* rung, int32_t* mask, double* U, int64_t n, void* stream)
{
    if (!A || !rung || !mask || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(ladder_probe_kernel, dim3(nblk(n, OBJ_PER_WAVE)), dim3(64), 0, (hipStream_t)stream, A, scale, rung, mask, U, n);
    return launch_status();
}

int ssa_sigma_points_f64(const double* x, const double* P, double scale, double* sig, int32_t* fail, int64_t n, void* stream)
{
    if (!x || !P || !sig || !fail || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(sigma_points_kernel, dim3(nblk(n, 64)), dim3(64), 0, (hipStream_t)stream, x, P, scale, sig, fail, n);
    return launch_status();
}

int ssa_hx_aer_f64(const double* x, int64_t x_stride, const double* M, const ssa_consts* c, double* z, int64_t n, void* stream)
{
    if (!x || !M || !c || !z || n < 0 || x_stride < 3) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(hx_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, x, x_stride, M, make_geo(c), z, n);
    return launch_status();
}

int ssa_mean_z_uvw_f64(const double* sigmas, const ssa_consts* c, double* zp, int64_t n, void* stream)
{
    if (!sigmas || !c || !zp || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(mean_z_kernel, dim3(nblk(n, 64)), dim3(64), 0, (hipStream_t)stream, sigmas, make_geo(c), zp, n);
    return launch_status();
}

int ssa_residual_z_aer_f64(const double* a, const double* b, double* c, int64_t n, void* stream)
{
    if (!a || !b || !c || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(residual_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, a, b, c, n);
    return launch_status();
}

int ssa_sunlit_mask_f64(const double* x_true, const double* sun_row, double shadow_radius, uint8_t* mask, int64_t n, void* stream)
{
    if (!x_true || !sun_row || !mask || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(sunlit_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, x_true, sun_row, shadow_radius, mask, n);
    return launch_status();
}

int ssa_los_mask_f64(const double* x_true, const double* trans_row, const double* site_row, double limb_radius, uint8_t* mask, int64_t n,
                     void* stream)
{
    if (!x_true || !trans_row || !site_row || !mask || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(los_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, x_true, trans_row, site_row, limb_radius, mask, n);
    return launch_status();
}

int ssa_visible_mask_f64(const double* x_true, const double* M, const ssa_consts* c, uint8_t* mask, double* el, int64_t n,
                         void* stream)
{
    if (!x_true || !M || !c || !mask || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(visible_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, x_true, M, make_geo(c), mask, el, n,
                       (const int32_t*)nullptr, 0, 0);
    return launch_status();
}
int ssa_visible_mask_at_f64(const double* x_true, const double* trans, const int32_t* env_time, int32_t time_offset, int32_t n_time,
                            const ssa_consts* c, uint8_t* mask, double* el, int64_t n, void* stream)
{
    if (!x_true || !trans || !env_time || n_time <= 0 || !c || !mask || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(visible_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, x_true, trans, make_geo(c), mask, el, n,
                       env_time, time_offset, n_time);
    return launch_status();
}

// the refusals of the ground-mask screen, stated once for both screen entries (the pointers matter only where something would launch)
static int screen_refused(const ssa_screen_params* p)
{
    if (!p || p->n < 0 || p->n_time < 1 || p->n_site < 1 || p->n_site > SSA_MAX_SENSORS || p->first < 0) return SSA_E_INVALID;
    if (p->n > 0 && (!p->elements || !p->trans || !p->sites || !p->accept)) return SSA_E_INVALID;
    return SSA_OK;
}

int ssa_catalogue_screen_f64(const ssa_screen_params* p, void* stream)
{
    if (screen_refused(p) != SSA_OK) return SSA_E_INVALID;
    if (p->n == 0) return SSA_OK;
    hipLaunchKernelGGL(catalogue_screen_kernel, dim3(nblk(p->n, SSA_SCREEN_WAVES)), dim3(64 * SSA_SCREEN_WAVES), 0, (hipStream_t)stream, *p);
    return launch_status();
}

int ssa_catalogue_screen_network_f64(const ssa_screen_network_params* q, void* stream)
{
    if (!q || screen_refused(&q->base) != SSA_OK || q->reserved != 0) return SSA_E_INVALID;
    const uint32_t beyond = ~0u << q->base.n_site;      // (n_site is 1 .. 8 here)
    if (q->site_moving != 0) {
        if ((uint32_t)q->site_moving & beyond) return SSA_E_INVALID;
        if (!q->site_rows || ((uintptr_t)q->site_rows & 127) != 0) return SSA_E_INVALID;
        if (!(q->limb_radius >= 0.0)) return SSA_E_INVALID;
    }
    if (q->sunlit_only != 0) {
        if ((uint32_t)q->sunlit_only & beyond) return SSA_E_INVALID;
        if (!q->sun || ((uintptr_t)q->sun & 31) != 0) return SSA_E_INVALID;
        if (!(q->shadow_radius >= 0.0)) return SSA_E_INVALID;
    }
    if (q->base.n == 0) return SSA_OK;
    hipLaunchKernelGGL(catalogue_screen_network_kernel, dim3(nblk(q->base.n, SSA_SCREEN_WAVES)), dim3(64 * SSA_SCREEN_WAVES), 0,
                       (hipStream_t)stream, *q);
    return launch_status();
}

// the pass table of a sensor network (ssa_access.hpp).  The rules in the header's order; the shared ones through the functions every
// sensor entry calls -- the sensor tail on a copy whose measurement kinds are cleared: this entry forms no measurement and does not judge them
int ssa_access_sensors_f64(const ssa_consts* c, const ssa_step_params* p, const ssa_sensor_params* sp, const ssa_access_params* a, void* stream)
{
    if (!c || !p || !sp || !a) return SSA_E_INVALID;
    if (p->n_obj <= 0 || p->n_env <= 0) return SSA_E_INVALID;
    if (!p->x_true_in || !p->trans || !p->env_time) return SSA_E_INVALID;
    if (!inline_envs_fit(p) || !propagator_ok(c)) return SSA_E_INVALID;
    if (sites_ok(sp) != SSA_OK) return SSA_E_INVALID;
    if (a->n_steps < 1 || !a->bits || ((uintptr_t)a->bits & 7) != 0) return SSA_E_INVALID;
    if (a->n_sel < 0 || (a->n_sel > 0 && !a->env_sel) || a->n_sel > p->n_env) return SSA_E_INVALID;
    const int64_t W = ((int64_t)a->n_steps + 63) / 64;
    const int64_t rows = (int64_t)p->n_env * sp->n_sensor;      // (every product below is taken only once its factors are below 2^31)
    if (p->n_obj >= ((int64_t)1 << 31) || !rows_fit(rows, 1) || !rows_fit(rows, p->n_obj) || !rows_fit(rows * p->n_obj, W)) return SSA_E_INVALID;
    ssa_sensor_params tail = *sp;
    tail.angles_only = 0;
    if (!sensor_tail_ok(c, p, &tail)) return SSA_E_INVALID;
    AccessK k;
    k.p = *p;
    k.p.launch_mask = p->launch_mask & SSA_LAUNCH_INLINE_ENVS;
    k.s = idle_sites(sp);
    k.a = *a;
    k.dt = c->dt;
    k.j2 = J2Params{c->j2, c->r_eq, c->rk4_substeps};
    k.waves_per_env = (int32_t)((p->n_obj + 63) / 64);
    const int64_t nsel = a->n_sel > 0 ? a->n_sel : p->n_env;      // (nsel <= n_env: the grid is below n_env * n_obj < 2^31 wavefronts)
    hipStream_t s = (hipStream_t)stream;
    with_prop(c->propagator, [&](auto P) { hipLaunchKernelGGL(access_sensors_kernel<P>, dim3((unsigned)(nsel * k.waves_per_env)), dim3(64), 0, s, k); });
    return launch_status();
}

int ssa_observe_f64(const double* x_true, const double* x, const double* P, double* obs, double* metrics, int64_t n, void* stream)
{
    if (!x_true || !x || !P || !obs || !metrics || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(observe_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, x_true, x, P, obs, metrics, n);
    return launch_status();
}

int ssa_aer_obs_f64(const double* x, const double* P, const double* M, const ssa_consts* c, double* out, int64_t n, void* stream)
{
    if (!x || !P || !M || !c || !out || n < 0) return SSA_E_INVALID;
    if (n == 0) return SSA_OK;
    hipLaunchKernelGGL(aer_obs_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, x, P, M, make_geo(c), out, n);
    return launch_status();
}

int ssa_agent_scores_f64(const double* x_true, const double* x_cur, const double* P_cur, const double* P_prev, const double* M,
                         const ssa_consts* c, double* scores, uint8_t* mask, int64_t n, void* stream)
{
    if (n == 0) return SSA_OK;
    if (!x_true || !x_cur || !P_cur || !scores || !c || n < 0 || (mask && !M)) return SSA_E_INVALID;
    hipLaunchKernelGGL(agent_scores_kernel, dim3(nblk(n, 64)), dim3(64), 0, (hipStream_t)stream, x_true, x_cur, P_cur, P_prev, M,
                       make_geo(c), scores, mask, n, (const int32_t*)nullptr, 0, 0);
    return launch_status();
}
int ssa_agent_scores_at_f64(const double* x_true, const double* x_cur, const double* P_cur, const double* P_prev, const double* trans,
                            const int32_t* env_time, int32_t time_offset, int32_t n_time, const ssa_consts* c, double* scores, uint8_t* mask,
                            int64_t n, void* stream)
{
    if (n == 0) return SSA_OK;
    if (!x_true || !x_cur || !P_cur || !scores || !c || n < 0 || !trans || !env_time || n_time <= 0 || !mask) return SSA_E_INVALID;
    hipLaunchKernelGGL(agent_scores_kernel, dim3(nblk(n, 64)), dim3(64), 0, (hipStream_t)stream, x_true, x_cur, P_cur, P_prev, trans,
                       make_geo(c), scores, mask, n, env_time, time_offset, n_time);
    return launch_status();
}

int ssa_nees_f64(const double* x_true, const double* x, const double* P, double* nees, int64_t n, void* stream)
{
    if (n == 0) return SSA_OK;
    if (!x_true || !x || !P || !nees || n < 0) return SSA_E_INVALID;
    hipLaunchKernelGGL(nees_kernel, dim3(nblk(n, 64)), dim3(64), 0, (hipStream_t)stream, x_true, x, P, nees, n);
    return launch_status();
}
int ssa_nis_f64(const double* y, const double* S, double* nis, int64_t n, void* stream)
{
    if (n == 0) return SSA_OK;
    if (!y || !S || !nis || n < 0) return SSA_E_INVALID;
    hipLaunchKernelGGL(nis_kernel, dim3(nblk(n, 64)), dim3(64), 0, (hipStream_t)stream, y, S, nis, n);
    return launch_status();
}

int ssa_chi2_contained_f64(const double* v, int64_t n, double lo, double hi, int64_t* counts, void* stream)
{
    if (!counts || n < 0 || (n > 0 && !v)) return SSA_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(chi2_zero_kernel, dim3(1), dim3(64), 0, s, (unsigned long long*)counts);
    if (n > 0) {
        int64_t nb = (n + 256 * 8 - 1) / (256 * 8);
        if (nb > 2048) nb = 2048;
        hipLaunchKernelGGL(chi2_contained_kernel, dim3((unsigned)nb), dim3(256), 0, s, v, n, lo, hi, (unsigned long long*)counts);
    }
    return launch_status();
}

int64_t ssa_agent_select_workspace_bytes(int64_t n_obj, int32_t n_env)
{
    if (n_obj <= 0 || n_env <= 0) return 0;
    return (int64_t)n_env * ((n_obj + AGENT_T - 1) / AGENT_T) * (int64_t)sizeof(AgentPart);
}
int ssa_agent_select_f64(const ssa_consts* c, int32_t kind, const double* x_true, const double* x_cur, const double* P_cur,
                         const double* P_prev, const double* trans, const int32_t* env_time, int32_t time_offset, int32_t n_time,
                         const int32_t* fallback, void* workspace, int32_t* action_out, int64_t* pick_out, int64_t n_obj,
                         int32_t n_env, void* stream)
{
    return ssa_agent_select_ids_f64(c, kind, x_true, x_cur, P_cur, P_prev, trans, env_time, time_offset, n_time, fallback, workspace, action_out,
                                    pick_out, n_obj, n_env, nullptr, stream);
}
int ssa_agent_select_ids_f64(const ssa_consts* c, int32_t kind, const double* x_true, const double* x_cur, const double* P_cur,
                             const double* P_prev, const double* trans, const int32_t* env_time, int32_t time_offset, int32_t n_time,
                             const int32_t* fallback, void* workspace, int32_t* action_out, int64_t* pick_out, int64_t n_obj,
                             int32_t n_env, const int32_t* obj_ids, void* stream)
{
    if (!c || !x_true || !x_cur || !P_cur || !trans || !env_time || !workspace || !action_out || n_obj <= 0 || n_env <= 0)
        return SSA_E_INVALID;
    if (obj_ids && n_env != 1) return SSA_E_UNSUPPORTED;
    const int nparts = (int)((n_obj + AGENT_T - 1) / AGENT_T);
    const dim3 grid(nparts, n_env), block(AGENT_T);
    hipStream_t s = (hipStream_t)stream;
    AgentPart* parts = (AgentPart*)workspace;
    const GeoK g = make_geo(c);
#define SSA_AGENT_LAUNCH(K) hipLaunchKernelGGL(agent_partial_kernel<K>, grid, block, 0, s, x_true, x_cur, P_cur, P_prev, trans, env_time, \
                                               time_offset, n_time, g, parts, n_obj, obj_ids)
    switch (kind) {
        case SSA_AGENT_NAIVE_GREEDY: SSA_AGENT_LAUNCH(SSA_AGENT_NAIVE_GREEDY); break;
        case SSA_AGENT_VISIBLE_GREEDY: SSA_AGENT_LAUNCH(SSA_AGENT_VISIBLE_GREEDY); break;
        case SSA_AGENT_SHANNON: SSA_AGENT_LAUNCH(SSA_AGENT_SHANNON); break;
        case SSA_AGENT_POS_ERROR: SSA_AGENT_LAUNCH(SSA_AGENT_POS_ERROR); break;
        case SSA_AGENT_VEL_ERROR: SSA_AGENT_LAUNCH(SSA_AGENT_VEL_ERROR); break;
        default: return SSA_E_INVALID;
    }
#undef SSA_AGENT_LAUNCH
    hipLaunchKernelGGL(agent_final_kernel, dim3(n_env), dim3(64), 0, s, (const AgentPart*)parts, nparts, fallback, action_out, pick_out);
    return launch_status();
}

int ssa_masked_argmax_f64(const double* score, const uint8_t* mask, int64_t n, int64_t* out, void* stream)
{
    if (!out || n < 0 || (n > 0 && !score)) return SSA_E_INVALID;
    hipLaunchKernelGGL(masked_argmax_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, score, mask, n, out);
    return launch_status();
}

int64_t ssa_masked_argmax_workspace_bytes(int64_t n)
{
    if (n < 0) return SSA_E_INVALID;
    return 64 + 16 * ((n + AMAX_T * AMAX_Q - 1) / (AMAX_T * AMAX_Q) + 1);
}
int ssa_masked_argmax_ws_f64(const double* score, const uint8_t* mask, int64_t n, int64_t* out, void* workspace, int64_t workspace_bytes,
                             void* stream)
{
    if (!out || n < 0 || (n > 0 && !score)) return SSA_E_INVALID;
    const int64_t nb = (n + AMAX_T * AMAX_Q - 1) / (AMAX_T * AMAX_Q);
    if (nb <= 1 || !workspace)      // (one workgroup's worth, or no workspace: the single-workgroup kernel)
        return ssa_masked_argmax_f64(score, mask, n, out, stream);
    if (workspace_bytes < ssa_masked_argmax_workspace_bytes(n) || nb > 0x7fffffff) return SSA_E_INVALID;
    hipLaunchKernelGGL(masked_argmax_blocks_kernel, dim3((unsigned)nb), dim3(AMAX_T), 0, (hipStream_t)stream, score, mask, n, out,
                       (unsigned long long*)workspace);
    return launch_status();
}

int64_t ssa_assign_sensors_workspace_bytes(int64_t n_obj, int32_t n_sensor)
{
    if (n_obj < 1 || n_obj > 0x7fffffff || n_sensor < 1 || n_sensor > SSA_MAX_SENSORS) return SSA_E_INVALID;
    return 64 + ((n_obj + ASG_CH - 1) / ASG_CH) * n_sensor * n_sensor * (int64_t)sizeof(AsgCand);
}
// the argument rules of the four assignment entries (greedy and optimal, one env and E of them), in the order they have always been
// checked: the workspace size of THIS call, or SSA_E_INVALID.  align: what the workspace's address must be a multiple of.
static int64_t assign_sensors_args(const double* score, int32_t column, const int32_t* action_out, int64_t need, const void* workspace,
                                   int64_t workspace_bytes, uintptr_t align)
{
    if (!score || !row_aligned(action_out) || column < 0 || column >= SSA_LOOK_NSCORE) return SSA_E_INVALID;
    if (need < 0 || !workspace || ((uintptr_t)workspace & (align - 1)) || workspace_bytes < need) return SSA_E_INVALID;
    return need;
}
static bool assign_envs_fit(int64_t n_obj, int32_t n_sensor, int32_t n_env) { return rows_fit(n_env, n_sensor, n_obj) && n_env <= 65535; }
int ssa_assign_sensors_f64(const double* score, int64_t n_obj, int32_t n_sensor, int32_t column, const int32_t* fallback,
                           int32_t* action_out, int64_t* pick_out, void* workspace, int64_t workspace_bytes, void* stream)
{
    // (the size query refuses n_obj and n_sensor out of range)
    if (assign_sensors_args(score, column, action_out, ssa_assign_sensors_workspace_bytes(n_obj, n_sensor), workspace, workspace_bytes, 16) < 0)
        return SSA_E_INVALID;
    hipLaunchKernelGGL(assign_sensors_kernel, dim3(nblk(n_obj, ASG_CH)), dim3(ASG_T), 0, (hipStream_t)stream, score, n_obj, (int)n_sensor,
                       (int)column, fallback, action_out, pick_out, (unsigned long long*)workspace);
    return launch_status();
}
int ssa_match_sensors_f64(const double* score, int64_t n_obj, int32_t n_sensor, int32_t column, const int32_t* fallback,
                          int32_t* action_out, int64_t* pick_out, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (assign_sensors_args(score, column, action_out, ssa_assign_sensors_workspace_bytes(n_obj, n_sensor), workspace, workspace_bytes, 16) < 0)
        return SSA_E_INVALID;
    hipLaunchKernelGGL(match_sensors_kernel, dim3(nblk(n_obj, ASG_CH)), dim3(ASG_T), 0, (hipStream_t)stream, score, n_obj, (int)n_sensor,
                       (int)column, fallback, action_out, pick_out, (unsigned long long*)workspace);
    return launch_status();
}
// every env's part of the workspace: the one-env workspace rounded up to 64 bytes
int64_t ssa_assign_sensors_envs_workspace_bytes(int64_t n_obj, int32_t n_sensor, int32_t n_env)
{
    const int64_t one = ssa_assign_sensors_workspace_bytes(n_obj, n_sensor);
    if (one < 0 || n_env < 1) return SSA_E_INVALID;
    return n_env * ((one + 63) / 64 * 64);
}
int ssa_assign_sensors_envs_f64(const double* score, int64_t n_obj, int32_t n_sensor, int32_t n_env, int32_t column, const int32_t* fallback,
                                int32_t* action_out, int64_t* pick_out, void* workspace, int64_t workspace_bytes, void* stream)
{
    // (the size query refuses n_obj, n_sensor and n_env out of range)
    const int64_t need = assign_sensors_args(score, column, action_out, ssa_assign_sensors_envs_workspace_bytes(n_obj, n_sensor, n_env),
                                             workspace, workspace_bytes, 64);
    if (need < 0 || !assign_envs_fit(n_obj, n_sensor, n_env)) return SSA_E_INVALID;
    hipLaunchKernelGGL(assign_sensors_envs_kernel, dim3(nblk(n_obj, ASG_CH), (unsigned)n_env), dim3(ASG_T), 0, (hipStream_t)stream, score,
                       n_obj, (int)n_sensor, (int)column, fallback, action_out, pick_out, (unsigned long long*)workspace, need / n_env / 8);
    return launch_status();
}
int ssa_match_sensors_envs_f64(const double* score, int64_t n_obj, int32_t n_sensor, int32_t n_env, int32_t column, const int32_t* fallback,
                               int32_t* action_out, int64_t* pick_out, void* workspace, int64_t workspace_bytes, void* stream)
{
    const int64_t need = assign_sensors_args(score, column, action_out, ssa_assign_sensors_envs_workspace_bytes(n_obj, n_sensor, n_env),
                                             workspace, workspace_bytes, 64);
    if (need < 0 || !assign_envs_fit(n_obj, n_sensor, n_env)) return SSA_E_INVALID;
    hipLaunchKernelGGL(match_sensors_envs_kernel, dim3(nblk(n_obj, ASG_CH), (unsigned)n_env), dim3(ASG_T), 0, (hipStream_t)stream, score,
                       n_obj, (int)n_sensor, (int)column, fallback, action_out, pick_out, (unsigned long long*)workspace, need / n_env / 8);
    return launch_status();
}

// ---- the horizon-wide optimal plan (plan_sensors_kernel): the argument rules in the header's order; the workspace size, or SSA_E_INVALID
static int64_t plan_sensors_need(int64_t n_obj, int32_t n_sensor, int32_t n_step, int32_t n_env, int32_t column)
{
    if (n_sensor < 1 || n_sensor > SSA_MAX_SENSORS || n_step < 1 || (int64_t)n_step * n_sensor > SSA_MAX_PLAN_SLOTS) return SSA_E_INVALID;
    if (n_env < 1 || n_env > 65535 || column < 0 || column >= SSA_LOOK_NSCORE || n_obj < 1) return SSA_E_INVALID;
    const int64_t N = (int64_t)n_step * n_sensor;
    if (n_obj > 0x7fffffffll / (N * n_env)) return SSA_E_INVALID;       // (n_step n_env n_sensor n_obj >= 2^31)
    return n_env * (64 + (int64_t)nblk(n_obj, PLN_CH) * N * N * (int64_t)sizeof(PlnEnt));
}
int64_t ssa_plan_sensors_workspace_bytes(int64_t n_obj, int32_t n_sensor, int32_t n_step, int32_t n_env)
{
    return plan_sensors_need(n_obj, n_sensor, n_step, n_env, 0);
}
int ssa_plan_sensors_f64(const double* score, int64_t n_obj, int32_t n_sensor, int32_t n_step, int32_t n_env, int32_t column,
                         int32_t* plan_out, int64_t* pick_out, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (!score || !row_aligned(plan_out)) return SSA_E_INVALID;
    const int64_t need = plan_sensors_need(n_obj, n_sensor, n_step, n_env, column);
    if (need < 0 || !workspace || ((uintptr_t)workspace & 63) || workspace_bytes < need) return SSA_E_INVALID;
    hipLaunchKernelGGL(plan_sensors_kernel, dim3(nblk(n_obj, PLN_CH), (unsigned)n_env), dim3(PLN_T), 0, (hipStream_t)stream, score, n_obj,
                       (int)n_sensor, (int)n_step, (int)column, plan_out, pick_out, (unsigned long long*)workspace, need / n_env / 8);
    return launch_status();
}

// ---- all-gather by direct peer stores (include/ssa_hip.h): no collective, plain kernels
int ssa_peer_push_f64(const double* src, int64_t n_words, double* const* dst, uint64_t* const* flag, int32_t n_peer,
                      const uint64_t* seq_base, uint64_t seq_off, const uint64_t* prev_flags, int64_t timeout_ticks, int32_t* error,
                      uint32_t* tickets, void* stream)
{
    if (n_peer < 0 || n_words < 0 || !seq_base || (n_peer > 0 && (!dst || !flag || !tickets || (n_words > 0 && !src)))) return SSA_E_INVALID;
    if (n_peer == 0) return SSA_OK;
    hipLaunchKernelGGL(peer_push_kernel, dim3(n_peer, PEER_SPLIT), dim3(256), 0, (hipStream_t)stream, src, n_words, dst,
                       (unsigned long long* const*)flag, (const unsigned long long*)seq_base, (unsigned long long)seq_off,
                       (const unsigned long long*)prev_flags, (long long)(timeout_ticks > 0 ? timeout_ticks : 200000000ll), error, tickets);
    return launch_status();
}
int ssa_peer_wait(const uint64_t* flags, int32_t n_src, const uint64_t* seq_base, uint64_t seq_off, int64_t timeout_ticks, int32_t* error,
                  void* stream)
{
    if (n_src < 0 || !seq_base || (n_src > 0 && !flags)) return SSA_E_INVALID;
    if (n_src == 0) return SSA_OK;
    hipLaunchKernelGGL(peer_wait_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const unsigned long long*)flags, n_src,
                       (const unsigned long long*)seq_base, (unsigned long long)seq_off,
                       (long long)(timeout_ticks > 0 ? timeout_ticks : 200000000ll), error);
    return launch_status();
}

}  // extern "C"
