/*
 * ssa_hip.h -- C ABI of libssa_hip.so: the MI355X (gfx950) implementation of
 * ssa-gym's per-step hot path (propagate -> UKF predict -> one UKF update ->
 * observation / error metrics / reward statistics).
 *
 * The reference (AshHarvey/ssa-gym) is pure Python and has no FFI of its own;
 * the boundary it exposes is the gym.Env class plus the operator callables in
 * its env_config dict (envs/__init__.py:23-28).  This library sits directly
 * below that class: every entry point replaces the per-object Python loop or
 * numba/filterpy/LAPACK call cited next to it (file:line under the reference
 * root).  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (hipMalloc / torch.Tensor.data_ptr())
 *     unless the parameter name ends in _host;
 *   - arrays are float64, C-contiguous, array-of-structures exactly as the
 *     reference's numpy arrays: states [n][6] (m, m/s, GCRS), covariances
 *     [n][6][6], observations [n][12], measurements [n][3];
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     launches are asynchronous, nothing synchronises;
 *   - every function returns 0 on success or a negative SSA_E_* code; no
 *     exceptions, no allocation, no host<->device copies -> all entry points
 *     are hipGraph-capturable.
 */
#ifndef SSA_HIP_H
#define SSA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSA_ABI_VERSION 23
#define SSA_INLINE_ENVS 8

/* error codes */
#define SSA_OK 0
#define SSA_E_INVALID (-1) /* bad size / null pointer / unknown flag */
#define SSA_E_LAUNCH (-2)  /* hipGetLastError() != hipSuccess after launch */
#define SSA_E_UNSUPPORTED (-3) /* valid arguments, but this entry point does not cover the configuration (the caller takes the
                                  general one: e.g. ssa_env_closed_loop_f64 with more objects than wavefronts resident at once) */

/* per-object filter status (int32), persists across steps.
 * ssa_tasker_simple_2.py:271-285, 300-313, 369-382 (filter_error): a failed filter is
 * overwritten with the sentinels x_failed / P_failed (:157-158) and skipped afterwards. */
#define SSA_ST_OK 0
#define SSA_ST_PREDICT_NAN 1    /* ', predict returned nan. ' */
#define SSA_ST_PREDICT_LINALG 2 /* robust_cholesky ladder exhausted -> LinAlgError */
#define SSA_ST_UPDATE_NAN 3     /* ', update returned nan. ' */
#define SSA_ST_UPDATE_LINALG 4  /* inv(S) singular -> LinAlgError */

/* observation model of the update (env_config['obs_type'], ssa_tasker_simple_2.py:98-107) */
#define SSA_OBS_AER 0 /* hx_aer_erfa + mean_z_uvw + residual_z_aer (dynamics.py:219,343,260) */
#define SSA_OBS_XYZ 1 /* hx_xyz + mean_xyz + residual_xyz/np.subtract (dynamics.py:207,276,271) */

/* two-body propagator variant; both evaluate envs/farnocchia.py:1010 farnocchia() */
#define SSA_PROP_ELEMENTS 0 /* rv2coe -> delta_t_from_nu -> nu_from_delta_t -> coe2rv, operation by operation; with
                               SSA_FLAG_REFERENCE_COV the BEHAVIOUR-FAITHFUL variant (the reference's episode-level filter failures) */
#define SSA_PROP_FG 1       /* every conic branch of farnocchia() through ONE equation: Kepler's equation in universal variables
                               (Stumpff series + Halley steps; closed-form Stumpff functions + Laguerre-Conway iterations for
                               long steps), state by the Lagrange coefficients f, g.  More accurate than the reference's chain on
                               diverged (hyperbolic) states, which is why its filters do not fail where the reference's do */
#define SSA_PROP_J2_RK4 2   /* EXTENSION without reference counterpart: two-body + J2 zonal
                               acceleration, classical RK4 with ssa_consts.rk4_substeps sub-steps per dt */

#define SSA_PROP_HYBRID 3   /* the behaviour-faithful variant at speed: the universal-variable series solver of SSA_PROP_FG on
                               strong-elliptic states (ecc < 1 - 1e-2, farnocchia.py:871: there the reference's chain agrees with it
                               to 1e-14); the reference's own STRONG-HYPERBOLIC chain (ecc > 1 + 1e-2, farnocchia.py:909-912,
                               1001-1004: F from the elements, F -> nu -> F, the hyperbolic Newton solve, F -> nu) -- operation by
                               operation, NaN by NaN -- on the states where its filters go wrong: a diverged filter's sigma points, which
                               that chain propagates metres to kilometres off; and (round 4) the universal-variable solver again on
                               the bands in between (|ecc - 1| <= 1e-2, elliptic orbits beyond the series' range), where the reference
                               is accurate to its Newton tolerance and the two agree to ~1e-12.  rv2coe's special orientations
                               (circular, equatorial) take the complete restatement.  With SSA_FLAG_REFERENCE_COV the same
                               episode-level failure statistics as SSA_PROP_ELEMENTS and the oracle (tests/test_episode_failures.py:
                               pooled counts, failed-set overlap, first-failure-step distributions over five workloads) */

/* flags of ssa_step_params.flags */
#define SSA_FLAG_RESAMPLE 1u /* predict() ends by redrawing the sigma points from the prior, for every filter (the
                                predict() of filterpy's development branch); default off = the propagated points are
                                kept for update() (believed to be what the released filterpy 1.4.5 does).  Which
                                of the two the reference's unpinned `filterpy` requirement resolved to cannot be checked
                                offline (the package is absent): the default is PARITY-UNPINNED, both are tested. */

#define SSA_FLAG_REFERENCE_COV 2u /* the prior covariance in the reference's own arithmetic: P = sum_i (sigma_i' - x)(Wc_i (sigma_i'
                                - x))^T + Q over all 13 points (filterpy's unscented_transform, call ssa_tasker_simple_2.py:275), whose
                                Wc_0 ~ -2e8 term cancels the other twelve.  For filters that have diverged late in a predict-mostly
                                episode that cancellation makes P indefinite and the NEXT predict fails with LinAlgError -- the
                                reference loses 2-3 % of its filters per 480-step episode this way (:271-285, 369-382).  Default
                                off: the same matrix expanded around sigma_0' (no cancellation, those filters survive).  On = the
                                BEHAVIOUR-FAITHFUL form; the env selects it together with SSA_PROP_ELEMENTS. */

/* layout of the per-env update record written by ssa_env_step_f64 (doubles) */
#define SSA_UPD_STRIDE 64
#define SSA_UPD_OBS_TAKEN 0 /* 1.0 if filters[a].update() ran (obs_taken[i], :305) */
#define SSA_UPD_Z_TRUE 1    /* [3] hx(x_true[i][a])                      (:298) */
#define SSA_UPD_Y 4         /* [3] innovation                            (:302) */
#define SSA_UPD_S 7         /* [3][3] innovation covariance              (:303) */
#define SSA_UPD_SIGMAS_H 16 /* [13][3] measurement sigma points          (:304) */
#define SSA_UPD_VISIBLE 55  /* 1.0 if object_visible([a])                (:299) */
#define SSA_UPD_ACTION 56   /* the action this record belongs to (as double), -1 = no update attempted */

/* layout of the per-env reward statistics written by ssa_reward_stats_f64 (doubles) */
#define SSA_STAT_SHARDS 128 /* accumulator shards per env of the atomics-based statistics path */
#define SSA_STAT_SHARD_WORDS 16 /* uint64 words between shards: every shard owns a 128-byte line (words 0..2 used); with 64 shards
                                  packed four words apart, 5000 wavefronts x 2 atomics met on 16 lines: +2 us per 20 000-object step */
#define SSA_STAT_STRIDE 8
#define SSA_STAT_MAX_DPOS 0   /* np.max(delta_pos[i])  (NaN-propagating)        (:325-343) */
#define SSA_STAT_CNT_LT_1E4 1 /* count(delta_pos < 1e4)  } results.py:432        */
#define SSA_STAT_CNT_LT_1E7 2 /* count(delta_pos < 1e7)  } reward_proportional_trinary_true */
#define SSA_STAT_ARGMAX_SPOS 3 /* np.argmax(sigma_pos[i]) (first max; 'shaped' uses it next step, :346) */
#define SSA_STAT_N_FAILED 4   /* number of objects with status != 0 */
#define SSA_STAT_MAX_SPOS 5   /* np.max(sigma_pos[i]) */

/* Constants of one environment family; built on the host, passed by value. */
typedef struct ssa_consts {
    double Q[36];       /* process noise, Q_discrete_white_noise (ssa_tasker_simple_2.py:110) */
    double R[9];        /* measurement noise (:128-131) */
    double Wm0, Wc0, Wi; /* Merwe weights: Wm[0], Wc[0], Wm[i]=Wc[i] (i>=1) (filterpy, :211-214) */
    double sum_wm_m1;   /* sum(Wm) - 1 evaluated exactly from the double weights */
    double sum_wc;      /* sum(Wc) evaluated exactly from the double weights */
    double scale;       /* n + lambda */
    double dt;          /* time_step [s] */
    double obs_limit;   /* elevation mask [rad] (:86) */
    double enu[9];      /* ecef2aer's trans_uvw_ecef matrix for the observer (transformations.py:341-343) */
    double obs_itrs[3]; /* lla2ecef(observer) (transformations.py:217) */
    int32_t obs_type;   /* SSA_OBS_* */
    int32_t propagator; /* SSA_PROP_* */
    uint32_t flags;     /* SSA_FLAG_* */
    int32_t update_interval; /* env_config['update_interval'] (:292) */
    double j2, r_eq;    /* SSA_PROP_J2_RK4: zonal coefficient and equatorial radius [m] (j2 = 0 -> two-body) */
    int32_t rk4_substeps; /* SSA_PROP_J2_RK4: RK4 steps per dt (>= 1) */
    int32_t reserved0;
} ssa_consts;

/* One env step for n_env independent environments of n_obj objects each
 * (object g = e * n_obj + j).  Replaces SSA_Tasker_Env.step() lines 265-322. */
typedef struct ssa_step_params {
    int64_t n_obj; /* m */
    int32_t n_env; /* E (1 for the plain gym env) */
    int32_t time_offset; /* added to env_time[e] (lets a captured / looped launch advance time) */
    const double *x_true_in; double *x_true_out; /* [E*m][6]  x_true[i-1] -> x_true[i]   (:265-266) */
    const double *x_in;      double *x_out;      /* [E*m][6]  filters[j].x               (:275,286) */
    const double *P_in;      double *P_out;      /* [E*m][6][6] filters[j].P             (:275,287) */
    int32_t *status;                             /* [E*m] in/out, SSA_ST_*               (:272,293) */
    double *obs;     /* [E*m][12]  observations(x, P)                     (results.py:61)  */
    double *metrics; /* [E][4][m]  delta_pos | delta_vel | sigma_pos | sigma_vel (results.py:37) */
    double *upd;     /* [E][SSA_UPD_STRIDE] update record, may be NULL */
    const double *trans;       /* [n_time][3][3] GCRS->ITRS matrices (trans_matrix, :137) */
    const int32_t *env_time;   /* [E] time index i of this step per env (after the increment of :259) */
    const int32_t *actions;    /* [E] object chosen per env, < 0 = no update */
    const double *z_noise;     /* measurement noise [3] of (env e, time i, object a) at
                                  z_noise + e*zn_stride_env + i*zn_stride_time + a*zn_stride_obj   (:219-221);
                                  the reference layout z_noise[n][m][3] has strides (0, 3m, 3) */
    int64_t zn_stride_env, zn_stride_time, zn_stride_obj;
    int32_t n_time;            /* rows in `trans` / time rows of `z_noise` (index = i % n_time) */
    uint32_t launch_mask;      /* 0 = everything; diagnostic: 1 common-path kernel, 2 post kernel, 4 final;
                                  SSA_LAUNCH_DEFER_FOLD (8): see stat_shards_prev */
    double *stats;             /* [E][SSA_STAT_STRIDE] reward statistics of this step (O3), may be NULL */
    int32_t *work;             /* unused since ABI 12 (the exception queue is gone); may be NULL */
    void *stat_ws;             /* ssa_reward_stats_workspace_bytes(): per-block statistics partials */
    uint64_t *stat_shards;     /* [E][SSA_STAT_SHARDS][SSA_STAT_SHARD_WORDS] zero-initialised device words, or NULL.  When given the
                                  step kernel accumulates max delta_pos / trinary counts / failures itself with sharded
                                  atomics (and writes aer_out, if asked, in its epilogue); a one-wave fold kernel writes
                                  `stats` and clears the words: two launches per step instead of three.  arg-max
                                  sigma_pos (only the 'shaped' reward needs it) is then computed only when spos_tiles is
                                  given; without: stats[SSA_STAT_ARGMAX_SPOS] = -1, stats[SSA_STAT_MAX_SPOS] = NaN. */
    uint64_t *stat_shards_prev;/* deferred fold (with SSA_LAUNCH_DEFER_FOLD in launch_mask): the shard set the PREVIOUS step
                                  accumulated into, or NULL.  The step kernel then carries n_env extra wavefronts that fold
                                  it into stats_prev and clear it while the objects of THIS step are being advanced, and
                                  this step's own statistics stay in stat_shards (no fold launch: ONE launch per step) until
                                  the next step passes them here or ssa_stats_fold_f64() folds them.  Alternate two sets. */
    double *stats_prev;        /* [E][SSA_STAT_STRIDE] destination of that fold */
    double *aer_out;           /* [E*m][4] aer_obs() of the NEW state (O4: az, el, range, trace P; NaN/inf -> 0.001;
                                  ssa_tasker_simple_2.py:834-840), may be NULL.  With stat_shards it is written by the step
                                  kernel's epilogue from the on-chip tiles (no extra launch, no second pass over x / P);
                                  without, by the post kernel: the 'aer' observation / the sharded all-gather payload. */
    uint64_t *stat_shards_clear; /* [E][SSA_STAT_SHARDS][SSA_STAT_SHARD_WORDS] or NULL: a shard set this launch ZEROES (nothing reads or adds to it
                                  during the launch).  Lets a consumer that takes the statistics as RAW shards -- the sharded
                                  multi-GPU step sends its rank's shard words in the all-gather payload and every rank
                                  folds all ranks' words itself -- rotate payload buffers without a fold / clear
                                  launch: step k accumulates into buffer k % N and clears buffer (k + 1) % N (N = 2 when the
                                  all-gather runs in the step's stream, 3 when it overlaps the next step on another one). */
    int32_t aer_cols;          /* columns of aer_out per object: 0 or 4 = (az, el, range, trace P); 1 = trace P only, [E*m] --
                                  the "per-object covariance-trace observation" of the sharded 160 000-object configuration:
                                  a quarter of the all-gather payload and no inverse trigonometry in the epilogue */
    int32_t action0;           /* with SSA_LAUNCH_INLINE_ACTION in launch_mask (one env): the env's action BY VALUE -- `actions` is then not
                                  read and may be NULL.  For callers whose action is born on the host every step (a gym env): a word
                                  in host-mapped memory would be fetched over PCIe by every wavefront of the launch (5 000 reads at
                                  20 000 objects: the step took 28 us instead of 16), a host-to-device copy costs a copy-engine pass */
    double *obs_mirror;        /* [E*m][12] or NULL: a SECOND destination of the observation rows (O1), written by the same lanes as
                                  `obs`.  Meant for host-mapped pinned memory: the 'flatten' observation of a gym-style caller then
                                  reaches the host from inside the kernel, overlapped with the other wavefronts' arithmetic, instead
                                  of through a copy-engine pass after it (1.92 MB at 20 000 objects: 44 us) */
    int32_t inline_time[SSA_INLINE_ENVS];   /* with SSA_LAUNCH_INLINE_ENVS (n_env <= SSA_INLINE_ENVS): env e's time index and action BY VALUE; */
    int32_t inline_action[SSA_INLINE_ENVS]; /* `env_time` / `actions` are then not read (env_time must still be non-NULL).  A vector env whose
                                  actions are born on the host every step saves the host-to-device copy in front of the launch */
    uint64_t *spos_tiles;      /* [ceil(E*m / 4)][2] device words or NULL (with stat_shards): arg-max of sigma_pos ON THE ONE-LAUNCH PATHS -- what the
                                  'shaped' reward reads, np.argmax(sigma_pos[i - 1]) (ssa_tasker_simple_2.py:339-352).  Every wavefront of the step
                                  kernel leaves (ordered bits of its tile's largest sigma_pos, index in the env of the first object that holds it) in
                                  its tile's slot -- no atomics -- and whoever folds the statistics shards (the fold kernel, the deferred fold's
                                  wavefront in the next launch, the last wavefront with SSA_LAUNCH_FOLD_INSIDE) reduces the slots with np.argmax's
                                  semantics (first maximum; the first NaN wins): stats[SSA_STAT_ARGMAX_SPOS] and stats[SSA_STAT_MAX_SPOS] are then
                                  exact on these paths too.  Needs whole tiles per env: n_env == 1 or n_obj % 4 == 0 (SSA_E_UNSUPPORTED otherwise:
                                  take the three-launch path, stat_shards = NULL).  Contents need no initialisation. */
    uint64_t *spos_tiles_prev; /* with SSA_LAUNCH_DEFER_FOLD: the slots the PREVIOUS step wrote (folded with stat_shards_prev), or NULL */
    double *fail_log;          /* [fail_cap][SSA_FAIL_STRIDE] or NULL: the filter_error() bookkeeping (ssa_tasker_simple_2.py:369-382) written BY THE KERNEL.
                                  A filter that fails in this step appends one record -- env, object, SSA_ST_* code, the step's time index and
                                  error_failed() of the state it failed from (:376-378: |x - x_true| and sqrt(sum diag P) of position and velocity, taken
                                  from the step's inputs) -- at index atomicAdd(fail_count, 1).  Meant for host-mapped pinned memory: the host reads the new
                                  records (their number = the rise of stats[SSA_STAT_N_FAILED]) right after the step's synchronisation, with no
                                  further copy -- the reference loses 2-3 % of its filters per episode, a few per step late in an episode, and a
                                  status read-back plus gathers per step doubled the cost of a gym-style step (round 4) */
    uint32_t *fail_count;      /* device word: records appended so far (the caller zeroes it when it resets its episode); NULL with fail_log NULL */
    int32_t fail_cap;          /* capacity of fail_log in records (a record beyond it is counted but not written) */
    int32_t reserved1;
    const int32_t *obj_ids;    /* [4 ceil(m / 4)] device words or NULL (one env: ssa_env_step_f64 with stat_shards, ssa_env_rollout_f64,
                                  ssa_env_closed_loop_f64 together with ssa_closed_loop_params.slot_of; SEVERAL envs, ssa_env_step_f64 only:
                                  [n_env][m] words, m % 4 == 0, every env its own permutation of 0 .. m - 1 -- indices within the env, as the
                                  actions are; obs_mirror / aer_out row e m + obj_ids[e][i]).  A LAYOUT: the caller stores its objects in another order than it numbers them --
                                  position i of every array of this struct holds the object the caller calls obj_ids[i] (round 4: objects of one orbit
                                  regime share wavefronts; late in an episode the diverged filters are the LEO objects, and packed they cost the launch
                                  10 % less: DESIGN.md section 6).  The kernel then speaks the CALLER's indices wherever an index leaves it or enters it:
                                  `actions` / action0 select obj_ids[i] == action, z_noise is indexed by the action as before, fail_log records and
                                  stats[SSA_STAT_ARGMAX_SPOS] carry obj_ids values (np.argmax's first maximum = the lowest such index), and the
                                  HOST-FACING copies of the observation -- obs_mirror rows, aer_out rows -- are written at row obj_ids[i].  x / P / x_true /
                                  status / obs / metrics stay in storage order.  An object's arithmetic does not depend on its position. */
    const double *metrics_prev;/* with SSA_LAUNCH_STATS_FROM_METRICS and stat_shards_prev: the `metrics` block [4][m] the PREVIOUS step wrote (it must
                                  still hold that step's rows: the service wavefronts of this launch reduce its delta_pos row) */
    /* ---- moving (space-based) sensors of a network, appended under ABI version 23: a zero tail is the behaviour before.
     * A sensor s >= 1 of an ssa_sensor_params network with bit s of `site_moving` set is not a point on the Earth's surface: wherever a
     * kernel would read ssa_sensor_params.enu[s] / obs_itrs[s] it reads row (t, s) of `site_rows` instead, t being the time row whose
     * `trans` matrix the same update reads (step, every pass of a lookahead, step h of a forecast, a rollout's or dry run's step, each
     * env's own time word in the *_envs entries).  The measurement arithmetic is unchanged: d = M x - obs, then the enu product.
     * Visibility of such a sensor: ssa_sensor_params.obs_limit[s] is NOT read.  With o = the row's obs_itrs, d = M r - o for the object's
     * true position r at the update, p = -(o.d), dd = d.d, oo = o.o:
     *     clear   = (p <= 0) || (p >= dd) || (oo dd - p p >= R_b R_b dd)      the segment sensor -> object stays outside the sphere R_b
     *     visible = clear && (no sunlit_only bit || object sunlit)            the Sun row's dark bit is NOT read for a moving sensor
     * A NaN anywhere gives not visible; an object that fails is an invisible object in every respect (record, status, OBS_TAKEN, a
     * lookahead score of NaN).  Measurement kinds, R, noise tables, failure handling, flags and propagators are untouched.
     * With site_moving == 0 neither `site_rows` nor `limb_radius` is read.
     * Refused before any launch, behind every other refusal of an entry -- SSA_E_INVALID by the entries that take an
     * ssa_sensor_params: a site_moving bit at or above n_sensor, or bit 0 (sensor 0 is the primary observer of ssa_consts); any bit set
     * while `site_rows` is NULL or not 128-byte aligned; any bit set while !(limb_radius >= 0); any bit set while obs_type is not
     * SSA_OBS_AER -- SSA_E_UNSUPPORTED by the entries that take no ssa_sensor_params -- ssa_env_step_f64 and its profiled
     * form, ssa_env_step_instance, ssa_env_rollout_f64, ssa_env_closed_loop_f64, ssa_lookahead_f64 --: any bit set. */
    const double *site_rows;   /* [n_time][n_sensor][16] doubles on the device, base 128-byte aligned.  Row (t, s): enu[9] in the layout of
                                  ssa_sensor_params.enu[s], obs_itrs[3], then 4 words that are 0.  Row t is the row whose `trans` the
                                  same update reads.  Entries of sensors without a bit in site_moving are never read. */
    double   limb_radius;      /* R_b [m]: the radius a moving sensor's line of sight must clear */
    int32_t  site_moving;      /* bit s: sensor s takes enu / obs_itrs from site_rows and is screened by line of sight */
    int32_t  reserved3;        /* 0 */
} ssa_step_params;
#define SSA_FAIL_STRIDE 8
#define SSA_FAIL_ENV 0
#define SSA_FAIL_OBJ 1      /* index within the env */
#define SSA_FAIL_STATUS 2
#define SSA_FAIL_TIME 3     /* the step's time index i (env_time + time_offset) */
#define SSA_FAIL_ERR 4      /* [4] delta_pos, delta_vel, sigma_pos, sigma_vel of the state the filter failed from */

/* ---------------------------------------------------------------- fused hot path
 * One env step for every object of every env, every propagator:
 * the step kernel advances 4 objects per wavefront with complete semantics (robust_cholesky's jitter ladder inline,
 * conic branches beyond the strong-elliptic one as out-of-line calls), the update and -- with stat_shards -- the
 * reward statistics included.  Launches per step:
 *   stat_shards given : step kernel (aer_out, if asked, in its epilogue) + a one-wave fold; nothing more with
 *       SSA_LAUNCH_DEFER_FOLD (the next step's launch folds): 2 / 1;
 *   stat_shards NULL  : step kernel + post kernel (exact statistics per block, arg-max sigma_pos included, and the
 *       payload) + a one-wave fold of those: 3 launches. */
int ssa_env_step_f64(const ssa_consts *c_host, const ssa_step_params *p_host, void *stream);
/* Same step, with the dominant launch (the common-path kernel) bracketed by the event pair `slot`
 * (0 <= slot < SSA_PROFILE_SLOTS) bound to that dispatch: ssa_env_step_profile_ms() then returns the kernel's
 * duration from its own begin/end timestamps -- what rocprofv3 --kernel-trace reports -- without the queue having
 * been drained between launches.  Measurement aid of bench.py's roofline line (an event pair recorded around the
 * call would add the queue latency of the records, ~10 us). */
#define SSA_PROFILE_SLOTS 1024
#define SSA_LAUNCH_DEFER_FOLD 8u
#define SSA_LAUNCH_INLINE_ACTION 16u /* the env's action is ssa_step_params.action0 (n_env == 1) */
#define SSA_LAUNCH_FOLD_INSIDE 32u   /* with stat_shards + stats, no deferral: the statistics of env e are folded by the LAST wavefront of the
                                        step kernel that adds to them (it counts the tiles behind the shards' sums, words 3 / 4 of the env's
                                        shard lines) instead of by a fold kernel launched behind the step: ONE launch per step with the
                                        statistics available when it completes -- for callers that read them on the host after every step.
                                        Launches with more than one tile per wavefront (> 20 480 objects in all) get the fold kernel behind
                                        the step instead: counting a tile costs such a wavefront a memory round trip per tile */
#define SSA_LAUNCH_MIRROR_F32 128u    /* EXTENSION (round 4; the reference's observations are float64): the HOST-FACING copies of the observation -- obs_mirror
                                         rows and, on the one-launch statistics path, aer_out rows -- are written in SINGLE precision (obs_mirror / aer_out
                                         then point at float arrays of the same shape): half the bytes over PCIe for consumers that cast to float32
                                         anyway (every RL framework does).  `obs` (the device-resident rows) stays double. */
#define SSA_LAUNCH_INLINE_ENVS 64u   /* time indices and actions of all envs are ssa_step_params.inline_time / inline_action (n_env <= 8);
                                        time_offset is still added */
#define SSA_LAUNCH_STATS_FROM_METRICS 256u /* with SSA_LAUNCH_DEFER_FOLD (one env, one tile per wavefront, no sensor network, no
                                        SSA_LAUNCH_FOLD_INSIDE, no stat_shards_clear; SSA_E_UNSUPPORTED otherwise): the step kernel's wavefronts
                                        leave the statistics block out of their epilogue -- only the number of failed filters of a tile that has
                                        one is added to word 2 of its shard (status is updated in place: it cannot be re-read a launch later).
                                        Max delta_pos and the trinary counts of step k are reduced from the metrics rows step k stored, 64 objects
                                        per instruction, by the ssa_stats_from_metrics_waves() service wavefronts that ride in launch k + 1 (given
                                        stat_shards_prev, stats_prev, metrics_prev) in place of the single fold wavefront: each leaves one partial
                                        in words 0 / 1 of its own shard line of stat_shards_prev and takes a ticket (word 4 of shard 0); the last
                                        one folds the lines into stats_prev and clears them.  Same bits as the atomics path: max, counts and the
                                        first arg-max do not depend on the order.  Both launches of a hand-over carry the bit;
                                        ssa_stats_fold_metrics_f64() folds the last step. */
#define SSA_LAUNCH_GENERIC 512u  /* ABI 23, additive: keep this launch on the generic step kernel.  Without the bit ssa_env_step_f64 sends the
                                    PLAIN launch form to an instance of the one-tile step kernel compiled for exactly that form
                                    (step_plain_kernel: what the generic one decides per wavefront from its arguments is a constant there;
                                    same arithmetic, bit-identical results).  The plain form: no sensor network, n_env == 1, one tile per
                                    wavefront, SSA_LAUNCH_DEFER_FOLD | SSA_LAUNCH_STATS_FROM_METRICS and none of SSA_LAUNCH_INLINE_ACTION,
                                    SSA_LAUNCH_INLINE_ENVS, SSA_LAUNCH_FOLD_INSIDE, SSA_LAUNCH_MIRROR_F32 nor the diagnostic bits 1 / 2 / 4,
                                    `actions` given, aer_out / obs_mirror / spos_tiles / spos_tiles_prev / stat_shards_clear NULL,
                                    update_interval <= 1, no SSA_FLAG_RESAMPLE, SSA_OBS_AER.  For tests and A/B measurements. */
/* which instance ssa_env_step_f64 would launch for this block: 1 = the plain form's, 0 = the generic one, or the negative SSA_E_* code
 * with which ssa_env_step_f64 refuses the block.  Host only: nothing is launched, no pointer is followed. */
int ssa_env_step_instance(const ssa_consts *c_host, const ssa_step_params *p_host);
int ssa_env_step_profiled_f64(const ssa_consts *c_host, const ssa_step_params *p_host, void *stream, int32_t slot);
/* waits for slot's kernel and writes its duration in milliseconds */
int ssa_env_step_profile_ms(int32_t slot, float *kernel_ms);
/* ---------------------------------------------------------------- rollout: K steps in one launch
 * For open-loop action schedules (the reference's round-robin / random agents, agents.py, and filter-only runs): the
 * K calls ssa_env_step_f64 would make, with every step's outputs written to that step's slot of the history rings and
 * results bit-identical to them, but each wavefront keeps its objects' state in LDS across the steps (an object's
 * trajectory depends on no other object).  `first` is the parameter block of the FIRST step (n_obj, n_env, time_offset,
 * status, trans, env_time, z_noise and strides, n_time; its in/out/stats pointers are ignored).  Two launches: the rollout kernel and a fold of the per-step statistics. */
typedef struct ssa_rollout_params {
    int32_t n_steps;           /* K >= 1 */
    int32_t history;           /* H >= 2: depth of the rings below */
    int32_t slot_out;          /* step k (0-based) reads slot (slot_out + k - 1) mod H and writes slot (slot_out + k) mod H */
    int32_t reserved;
    double *x_true_ring;       /* [H][E*m][6]   slot 0 of each ring */
    double *x_ring;            /* [H][E*m][6] */
    double *P_ring;            /* [H][E*m][6][6] */
    double *obs_ring;          /* [H][E*m][12] */
    double *metrics_ring;      /* [H][E][4][m] */
    double *upd_ring;          /* [H][E][SSA_UPD_STRIDE] or NULL */
    double *stats_ring;        /* [H][E][SSA_STAT_STRIDE]; only the last H steps' statistics survive, as in any ring */
    const int32_t *actions;    /* [K][E] */
    uint64_t *stat_shards;     /* [K][E][SSA_STAT_SHARDS][SSA_STAT_SHARD_WORDS] zero-initialised; cleared again by the fold */
    uint64_t *spos_tiles;      /* [K][ceil(E*m / 4)][2] or NULL: per-step arg-max slots (ssa_step_params.spos_tiles): the statistics of every
                                  step then carry np.argmax(sigma_pos) -- the 'shaped' reward over a rollout */
} ssa_rollout_params;
int ssa_env_rollout_f64(const ssa_consts *c_host, const ssa_step_params *first, const ssa_rollout_params *r, void *stream);

/* folds a shard set into stats[n_env][SSA_STAT_STRIDE] and clears it: the last step of a deferred-fold sequence,
 * or whenever the host wants the statistics of the step just launched */
int ssa_stats_fold_f64(uint64_t *stat_shards, double *stats, int32_t n_env, void *stream);
/* the same with the arg-max slots of that step (ssa_step_params.spos_tiles; NULL = as ssa_stats_fold_f64) */
int ssa_stats_fold_spos_f64(uint64_t *stat_shards, const uint64_t *spos_tiles, double *stats, int64_t n_obj, int32_t n_env, void *stream);
/* SSA_LAUNCH_STATS_FROM_METRICS: the service wavefronts per launch for n_env envs of n_obj objects on this device, or 0 where the path
 * does not apply (several envs, more than one tile per wavefront) */
int32_t ssa_stats_from_metrics_waves(int64_t n_obj, int32_t n_env);
/* the stand-alone fold of a step launched with SSA_LAUNCH_STATS_FROM_METRICS (one env): `metrics` [4][m] and `stat_shards` of THAT step,
 * its arg-max slots or NULL; writes stats[SSA_STAT_STRIDE] and clears the shard set.  One launch. */
int ssa_stats_fold_metrics_f64(const double *metrics, uint64_t *stat_shards, const uint64_t *spos_tiles, double *stats, int64_t n_obj,
                               void *stream);
/* historical: size of the `work` buffer (now unused); returns a token size */
int64_t ssa_env_step_work_bytes(int64_t n_obj, int32_t n_env);

/* O3: per-env reductions over metrics[E][4][m] and status -> stats[E][SSA_STAT_STRIDE]
 * (ssa_tasker_simple_2.py:324-354, results.py:432). */
int ssa_reward_stats_f64(const double *metrics, const int32_t *status, double *stats, void *workspace,
                         int64_t n_obj, int32_t n_env, void *stream);
/* bytes of device workspace ssa_reward_stats_f64 needs for n_env environments */
int64_t ssa_reward_stats_workspace_bytes(int32_t n_env);

/* ----------------------------------------------------- single operators (rows of SURVEY 8a) */
/* P1-P5  fx_xyz_farnocchia(x, dt) for n states (farnocchia.py:1054). */
int ssa_propagate_f64(const double *x_in, double *x_out, int64_t n, double dt, int32_t propagator, void *stream);
/* the J2 + RK4 extension propagator on its own (SSA_PROP_J2_RK4) */
int ssa_propagate_j2_f64(const double *x_in, double *x_out, int64_t n, double dt, double j2, double r_eq,
                         int32_t substeps, void *stream);
/* P2-P4 diagnostics: coe[n][8] = p, ecc, inc, raan, argp, nu0, delta_t0, nu(dt)  (farnocchia.py:165,847,925). */
int ssa_kepler_elements_f64(const double *x_in, double *coe, int64_t n, double dt, void *stream);
/* U2  robust_cholesky(A) for n 6x6 matrices: U upper (zeros below), rung[n] = -1 (no jitter),
 * 0..15 (10^(rung-6) added), 16 = LinAlgError (dynamics.py:402). */
int ssa_robust_cholesky6_f64(const double *A, double *U, int32_t *rung, int64_t n, void *stream);
/* U2 as the FUSED step kernels run it (the row-distributed ladder of robust_chol_row_lds, four matrices per wavefront): rung[n] as above
 * from the kernel's one-pass ladder, mask[n] = bit i set when rung i (jitter 10^(i-6)) factorises in the kernel's arithmetic (bit 16: the
 * plain attempt) -- all sixteen rungs are actually tried, so rung[n] must be the lowest set bit of mask[n] whatever the pattern.  (On the
 * numerically rank-one (n + lambda) P of a diverged filter that round 3 took for a non-monotone case -- tests/golden/
 * ladder_illconditioned_tile.npz -- the mask is 0111...1, and so it is on 4 096 one-ulp perturbations: DESIGN.md section 6, Round 4.) */
int ssa_ladder_probe_f64(const double *A, double scale, int32_t *rung, int32_t *mask, double *U, int64_t n, void *stream);
/* U1  MerweScaledSigmaPoints.sigma_points(x, P): sig[n][13][6], fail[n] (0 / SSA_ST_PREDICT_LINALG). */
int ssa_sigma_points_f64(const double *x, const double *P, double scale, double *sig, int32_t *fail,
                         int64_t n, void *stream);
/* H1  hx_aer_erfa for n states sharing one matrix M[9] (device pointer) (dynamics.py:219). */
int ssa_hx_aer_f64(const double *x, int64_t x_stride, const double *M, const ssa_consts *c_host, double *z,
                   int64_t n, void *stream);
/* H3  mean_z_uvw(sigmas[n][13][3], Wm) with the Merwe weights of c_host (dynamics.py:343). */
int ssa_mean_z_uvw_f64(const double *sigmas, const ssa_consts *c_host, double *zp, int64_t n, void *stream);
/* H4  residual_z_aer(a[n][3], b[n][3]) (dynamics.py:260). */
int ssa_residual_z_aer_f64(const double *a, const double *b, double *c, int64_t n, void *stream);
/* V1  object_visibility(): mask[n] = elevation(x_true) >= obs_limit; el[n] optional (:418-434). */
int ssa_visible_mask_f64(const double *x_true, const double *M, const ssa_consts *c_host, uint8_t *mask,
                         double *el, int64_t n, void *stream);
/* EXTENSION, no reference counterpart: the sunlit rule of ssa_sensor_params, for the n true states x_true[n][6] against ONE 32-byte row
 * of a Sun table, sun_row = (sx, sy, sz, dark word; the word is not read): mask[n] = 1 where the object is outside the Earth's
 * cylindrical shadow of radius shadow_radius -- (p >= 0) || (d2 >= R R) with p = r.s, d2 = r.r - p p -- else 0; a NaN in r or s: 0.
 * The device function is the one the sensor kernels evaluate. */
int ssa_sunlit_mask_f64(const double *x_true, const double *sun_row, double shadow_radius, uint8_t *mask, int64_t n, void *stream);
/* EXTENSION, no reference counterpart: the line-of-sight rule of a moving sensor (ssa_step_params.site_moving), for the n true states
 * x_true[n][6] against ONE `trans` row (9 doubles) and ONE 128-byte site row (enu[9], obs_itrs[3], 4 words that are not read), all on the
 * device: mask[n] = 1 where the segment from the sensor to the object stays outside the sphere of radius limb_radius --
 * (p <= 0) || (p >= dd) || (oo dd - p p >= R_b R_b dd) with d = M r - o, p = -(o.d), dd = d.d, oo = o.o -- else 0; a NaN anywhere: 0.
 * The device function is the one the sensor kernels evaluate.  Refused (SSA_E_INVALID): a NULL pointer, n < 0. */
int ssa_los_mask_f64(const double *x_true, const double *trans_row, const double *site_row, double limb_radius, uint8_t *mask, int64_t n,
                     void *stream);
/* O1/O2  observations() + error() for n objects of one env (results.py:61,37); metrics[4][n]. */
int ssa_observe_f64(const double *x_true, const double *x, const double *P, double *obs, double *metrics,
                    int64_t n, void *stream);
/* O4  aer_obs(): out[n][4] = hx(x_filter), trace(P); NaN/inf -> 0.001 (ssa_tasker_simple_2.py:834). */
int ssa_aer_obs_f64(const double *x, const double *P, const double *M, const ssa_consts *c_host, double *out,
                    int64_t n, void *stream);

/* ------------------------------------------------ device-side agent primitives
 * Per-object scores the reference's heuristic agents compute in Python loops (agents.py:7-81):
 *   scores[0][j] = trace(P_cur[j])                        agent_naive_greedy / agent_visible_greedy
 *   scores[1][j] = log(det P_cur[j] / det P_prev[j])      agent_shannon        (NaN if either Cholesky fails, below)
 *   scores[2][j] = |x_cur[j][:3] - x_true[j][:3]|         agent_pos_error_greedy
 *   scores[3][j] = |x_cur[j][3:] - x_true[j][3:]|         agent_vel_error_greedy
 *   mask[j]      = elevation(x_true[j]) >= obs_limit      visible_objects()    (:410-425)
 * P_prev may be NULL (scores[1] = NaN).  scores[1] is 2 log(prod diag U) of the plain Cholesky factor U of each matrix's upper
 * triangle, and NaN whenever either factorisation fails -- not only when a determinant is <= 0: a matrix with two negative
 * eigenvalues has det > 0 and a finite reference score, and late in an episode the filter leaves covariances whose smallest
 * eigenvalue is negative at rounding level (at most 3e-16 of the largest, diagonal entries 1e18 .. 1e21; 1-3 objects per step of
 * tests/episode_workload.py's seed-7 episode from step 300 on).  The reference's score on those is set by rounding, not by the
 * filter, and the arg-max skips them (tests/test_agent_ops.py). */
int ssa_agent_scores_f64(const double *x_true, const double *x_cur, const double *P_cur, const double *P_prev,
                         const double *M, const ssa_consts *c_host, double *scores, uint8_t *mask, int64_t n,
                         void *stream);
/* The two primitives above for callers whose time index lives ON THE DEVICE (a policy evaluated inside a captured hipGraph: the graph
 * advances the index between replays): the GCRS->ITRS matrix is row (env_time[0] + time_offset) % n_time of the table `trans`, as in the step. */
int ssa_visible_mask_at_f64(const double *x_true, const double *trans, const int32_t *env_time, int32_t time_offset, int32_t n_time,
                            const ssa_consts *c_host, uint8_t *mask, double *el, int64_t n, void *stream);
int ssa_agent_scores_at_f64(const double *x_true, const double *x_cur, const double *P_cur, const double *P_prev, const double *trans,
                            const int32_t *env_time, int32_t time_offset, int32_t n_time, const ssa_consts *c_host, double *scores,
                            uint8_t *mask, int64_t n, void *stream);
/* np.argmax(score[mask]) mapped back to object indices: out[0] = index of the first maximum of `score`
 * over entries with mask != 0 (mask may be NULL = all), or -1 when no entry is selected / n == 0;
 * NaN entries are skipped (the reference's agents run under np.errstate and np.argmax would return a
 * NaN's index; skipping is the documented deviation).  out[1] = the maximum (as double bits). */
int ssa_masked_argmax_f64(const double *score, const uint8_t *mask, int64_t n, int64_t *out, void *stream);
/* The same fold spread over the chip, for callers that own a workspace -- the arg-max head of a device-side policy between two step
 * launches (SSA_Tasker_Env.run_policy, PolicyView.argmax): one workgroup reads 20 000 entries in 8.6 us (a single CU's share of the memory
 * system), ceil(n / 2048) workgroups and a last-arrival fold take about 3.  `workspace`: ssa_masked_argmax_workspace_bytes(n) bytes of
 * device memory, ZERO before the first call (the kernel leaves it zero-ticketed for the next), used by one call at a time (calls in one
 * stream are).  NULL workspace or n <= 2048: the single-workgroup kernel. */
int ssa_masked_argmax_ws_f64(const double *score, const uint8_t *mask, int64_t n, int64_t *out, void *workspace, int64_t workspace_bytes,
                             void *stream);
int64_t ssa_masked_argmax_workspace_bytes(int64_t n);

/* ------------------------------------------------ closed loop on the device
 * The agent's choice for the NEXT step, made on the GPU from the state the step just wrote and stored into the int32
 * action word(s) ssa_step_params.actions of that next step points at -- enqueue  step, select, step, select, ...  in one
 * stream and a greedy agent runs at kernel rate with no host round trip (the reference's loop is
 * `a = agent(obs, env); obs, r, done, _ = env.step(a)`, run_environment.py / compare_agents.py).
 *   kind                        score (first maximum wins, NaN scores skipped)              objects considered
 *   SSA_AGENT_NAIVE_GREEDY      trace(P_cur[j])                              agents.py:7    all
 *   SSA_AGENT_VISIBLE_GREEDY    trace(P_cur[j])                              agents.py:36   visible (elevation of x_true >= obs_limit)
 *   SSA_AGENT_SHANNON           log(det P_cur[j] / det P_prev[j])            agents.py:15   visible
 *   SSA_AGENT_POS_ERROR         |x_cur[j][:3] - x_true[j][:3]|               agents.py:66   visible
 *   SSA_AGENT_VEL_ERROR         |x_cur[j][3:] - x_true[j][3:]|               agents.py:75   visible
 * Per env e (objects e*n_obj .. +n_obj): action_out[e] = index of the first maximum, or fallback[e] when no object
 * qualifies (the reference calls action_space.sample() there; the caller supplies that draw), or -1 with fallback NULL.
 * The GCRS->ITRS matrix is row (env_time[e] + time_offset) % n_time of `trans`, as in the step.  pick_out (optional,
 * [E][2] int64): the arg-max (-1 = none) and the winning score's bit pattern.  workspace: ssa_agent_select_workspace_bytes().
 * P_prev may be NULL (no previous step yet): the Shannon score is then NaN for every object -> fallback, as agents.py at i = 0.
 * Two small launches (per-block first maxima over all CUs, then one wavefront per env). */
#define SSA_AGENT_NAIVE_GREEDY 0
#define SSA_AGENT_VISIBLE_GREEDY 1
#define SSA_AGENT_SHANNON 2
#define SSA_AGENT_POS_ERROR 3
#define SSA_AGENT_VEL_ERROR 4
int ssa_agent_select_f64(const ssa_consts *c_host, int32_t kind, const double *x_true, const double *x_cur,
                         const double *P_cur, const double *P_prev, const double *trans, const int32_t *env_time,
                         int32_t time_offset, int32_t n_time, const int32_t *fallback, void *workspace,
                         int32_t *action_out, int64_t *pick_out, int64_t n_obj, int32_t n_env, void *stream);
/* the same with a storage layout (ssa_step_params.obj_ids, one env): the state tensors are in storage order, the action word and the pick
 * name the object as the CALLER numbers it, and the first maximum is the candidate with the lowest such index.  obj_ids NULL: identical to
 * ssa_agent_select_f64. */
int ssa_agent_select_ids_f64(const ssa_consts *c_host, int32_t kind, const double *x_true, const double *x_cur,
                             const double *P_cur, const double *P_prev, const double *trans, const int32_t *env_time,
                             int32_t time_offset, int32_t n_time, const int32_t *fallback, void *workspace,
                             int32_t *action_out, int64_t *pick_out, int64_t n_obj, int32_t n_env, const int32_t *obj_ids, void *stream);
int64_t ssa_agent_select_workspace_bytes(int64_t n_obj, int32_t n_env);

/* ------------------------------------------------ consistency diagnostics
 * NEES  nees[k] = d^T inv(P[k]) d, d = x_true[k] - x[k]   for n (step, object) pairs  (anees(), ssa_tasker_simple_2.py:436-446;
 *       fitness_test() :764-768) -- LU with partial pivoting per lane, NaN where P is singular;
 * NIS   nis[k] = y[k]^T inv(S[k]) y[k]                     (fitness_test() :750-754). */
int ssa_nees_f64(const double *x_true, const double *x, const double *P, double *nees, int64_t n, void *stream);
int ssa_nis_f64(const double *y, const double *S, double *nis, int64_t n, void *stream);
/* chi-square containment of fitness_test() (ssa_tasker_simple_2.py:757-760 NIS, :770-771 NEES): counts[0] = number of v[k] with
 * lo < v[k] < hi (lo, hi = stats.chi2.ppf([alpha/2, 1 - alpha/2], df), computed by the caller), counts[1] = number of non-NaN
 * v[k] (the reference drops NaN NIS values before the mean and keeps NaN NEES values in it).  counts: device int64[2]. */
int ssa_chi2_contained_f64(const double *v, int64_t n, double lo, double hi, int64_t *counts, void *stream);

/* ---------------------------------------------------------------- closed loop: K steps AND their K decisions in one launch
 * The loop `a = agent(obs, env); obs, r, done, _ = env.step(a)` of the reference's drivers (run_environment.py:26-29,
 * compare_agents.py:41-42) for one of its greedy agents (agents.py:7-81, SSA_AGENT_*): what K x [ssa_env_step_f64 +
 * ssa_agent_select_f64] enqueue, with bit-identical states and identical actions, but as ONE persistent launch -- every
 * wavefront keeps its objects in LDS across the steps (as ssa_env_rollout_f64), and the wavefronts agree on the next action
 * among themselves through agent-scope atomics while the next step's predicts (which do not depend on it) already run.
 * One env; every wavefront must be resident at once -- one per four objects plus one service wavefront per 64 of those plus
 * one (they fold the wavefronts' scores into the decision): n_obj <= 20 160 on MI355X; SSA_E_UNSUPPORTED otherwise -- use the
 * per-step calls.  `first` as for ssa_env_rollout_f64.
 *   actions[0]   in : the action of the first step (e.g. from ssa_agent_select_f64 on the state the launch starts from)
 *   actions[k]   out: the agent's choice for step k (0-based), k = 1 .. K  (actions[K]: the decision after the last step)
 *   fallback[k]     : used for actions[k] when no object qualifies at that decision (the reference samples at random,
 *                     agents.py:40-42: the caller supplies the draws); NULL -> -1 (no update)
 *   stats_out[k]    : [SSA_STAT_STRIDE] reward statistics of step k (arg-max sigma_pos only with SSA_LOOP_ARGMAX_SPOS; else -1 / NaN)
 *   upd_out[k]      : [SSA_UPD_STRIDE] update record of step k, or NULL
 *   picks[k]        : optional [K+1][2] int64: arg-max (-1 = fallback used) and the winning score's bits of decision k >= 1
 *   error           : optional device-visible int32, set to 1 if a wavefront waited 2 s for a decision and the launch gave up
 *                     (every wait is bounded; outputs are then incomplete)
 * The rings hold the last `history` steps as after K per-step calls. */
typedef struct ssa_closed_loop_params {
    int32_t n_steps;           /* K >= 1 */
    int32_t history;           /* H >= 2 */
    int32_t slot_out;          /* step k reads slot (slot_out + k - 1) mod H, writes slot (slot_out + k) mod H */
    int32_t agent;             /* SSA_AGENT_* */
    double *x_true_ring, *x_ring, *P_ring, *obs_ring, *metrics_ring;   /* as ssa_rollout_params */
    double *upd_out;           /* [K][SSA_UPD_STRIDE] or NULL */
    double *stats_out;         /* [K][SSA_STAT_STRIDE] */
    int32_t *actions;          /* [K + 1] */
    const int32_t *fallback;   /* [K + 1] or NULL */
    int64_t *picks;            /* [K + 1][2] or NULL */
    int32_t *error;            /* or NULL */
    void *workspace;           /* ssa_closed_loop_workspace_bytes() bytes of device memory (contents irrelevant) */
    int64_t workspace_bytes;
    int64_t wait_ticks;        /* bound of every wait inside the launch, in ticks of the 100 MHz wall clock; 0 = the default (2 s).  A wavefront
                                  that waits longer for a decision publishes the abort generation, every wavefront leaves, `error` is set */
    uint32_t flags;            /* SSA_LOOP_* */
    uint32_t reserved;
    const int32_t *slot_of;    /* with ssa_step_params.obj_ids (a storage layout): [m] device words, slot_of[j] = the position at which the object the
                                  caller calls j is stored (the inverse of obj_ids) -- the wavefronts agree through it on whose tile holds the selected
                                  object; NULL without a layout.  Actions, picks, failure records and the arg-max of sigma_pos speak the caller's
                                  indices (first maximum = the lowest such index), as in the per-step launches */
} ssa_closed_loop_params;
#define SSA_LOOP_ARGMAX_SPOS 1u   /* stats_out[k][SSA_STAT_ARGMAX_SPOS / SSA_STAT_MAX_SPOS] = np.argmax / np.max of sigma_pos after step k (the
                                     'shaped' reward): two more words per wavefront in the exchange */
#define SSA_LOOP_DEBUG_WITHHOLD 2u /* DIAGNOSTIC: the deciding wavefront never publishes -- every wait runs into its bound.  For the test of the
                                     give-up path (tests/test_env_gpu.py): the grid must drain, `error` must be set, later launches must work */
int ssa_env_closed_loop_f64(const ssa_consts *c_host, const ssa_step_params *first, const ssa_closed_loop_params *r, void *stream);
int64_t ssa_closed_loop_workspace_bytes(int64_t n_obj, int32_t n_env);

/* ---------------------------------------------------------------- one-step tasking lookahead
 * From the state a step would start from (ssa_step_params inputs: slot i), for EVERY object j of every env what the step at i + 1
 * would produce for j if the env's action were j -- the prior, the covariance after the hypothetical update and the gains of the
 * classic sensor-tasking baselines -- in one launch of the step kernel's own predict / update code (nothing committed).  The UKF
 * update's covariance P+ = P- - K S K^T does not depend on the measured value, so no measurement noise is involved: z_noise is never
 * read, and nothing returned depends on it (no x+, no innovation).  Bit-identical to the step: x_prior / P_prior to what
 * ssa_env_step_f64 leaves for any object it does not update, P_post to P_out[j] of a step whose action is j, status / visible to that
 * step's status word and SSA_UPD_VISIBLE -- for every propagator, observation type, SSA_FLAG_RESAMPLE and SSA_FLAG_REFERENCE_COV.
 * Cost: every wavefront runs four updates where a step runs at most one per env. */
#define SSA_LOOK_NSCORE 3
#define SSA_LOOK_TRACE_GAIN 0     /* tr P- - tr P+ (agent_visible_greedy's trace, agents.py:36) */
#define SSA_LOOK_POS_TRACE_GAIN 1 /* the same over the 3x3 position block */
#define SSA_LOOK_INFO_GAIN 2      /* expected information gain 1/2 (ln det P- - ln det P+), both log-dets through the Cholesky factor */
typedef struct ssa_lookahead_out {
    double *score;     /* [E*m][SSA_LOOK_NSCORE], required.  NaN unless status == SSA_ST_OK and visible */
    int32_t *status;   /* [E*m], required: the SSA_ST_* code object j would carry after the step that updates it -- an earlier failure,
                          SSA_ST_PREDICT_NAN / SSA_ST_PREDICT_LINALG of this predict, SSA_ST_UPDATE_LINALG (singular S).  SSA_ST_UPDATE_NAN
                          is NOT foreseen: it comes from x+, which depends on the drawn measurement noise */
    uint8_t *visible;  /* [E*m], required: the update's visibility test (elevation of the true state at i + 1, ssa_tasker_simple_2.py:418-425);
                          0 where the update would not be attempted (a failed filter, a step the update_interval skips) */
    double *x_prior;   /* [E*m][6] or NULL */
    double *P_prior;   /* [E*m][36] or NULL */
    double *P_post;    /* [E*m][36] or NULL: P- where the update would not run, the failure sentinel where S is singular */
} ssa_lookahead_out;
/* Reads only the INPUT fields of ssa_step_params: n_obj, n_env, time_offset, x_true_in, x_in, P_in, status, trans, env_time, n_time,
 * obj_ids and -- the only launch_mask bit honoured -- SSA_LAUNCH_INLINE_ENVS with inline_time.  None of its output pointers is touched,
 * nor actions / z_noise: no history slot, status word, failure record, update record or statistics word is written.  Output row of an
 * object = e * n_obj + its index as the caller numbers it (obj_ids, as obs_mirror / aer_out): a storage layout never shows. */
int ssa_lookahead_f64(const ssa_consts *c_host, const ssa_step_params *p_host, const ssa_lookahead_out *out, void *stream);

/* ---------------------------------------------------------------- sensor networks: several ground sensors in one step
 * EXTENSION without reference counterpart (the reference has one observer).  One env step in which each of n_sensor ground sites
 * observes one object: sensor s updates object action[s] exactly as ssa_env_step_f64 updates the env's action, with ITS site's
 * geometry (enu, obs_itrs), elevation mask and measurement noise covariance R -- the visibility test of the true state as seen from
 * site s, z_true, the innovation, S, K and the failure handling.  Everything else -- the predict of every object, observations,
 * metrics, reward statistics, failure records (per object), obs_mirror / aer_out, obj_ids, spos_tiles, every launch_mask bit but
 * SSA_LAUNCH_INLINE_ACTION -- comes from ssa_step_params with unchanged meaning; its `actions` / action0 and `upd` are not read (set
 * the update records' destination here).  aer_out is hx of ssa_consts' observer (the primary sensor: the caller passes sensor 0's).
 *   action[s] < 0 or >= n_obj: sensor s is idle.  Two sensors on one object: the lowest-numbered one updates it; the others are idle.
 *   An idle sensor, every sensor of a step the update_interval skips, and a sensor whose object has failed get a record with
 *   SSA_UPD_ACTION = -1 (OBS_TAKEN = VISIBLE = 0 unless the update was attempted).
 *   Measurement noise of sensor s: z_noise + s*zn_stride_sensor + i*zn_stride_time + action[s]*zn_stride_obj (ssa_step_params strides).
 * n_env == 1 only (SSA_E_UNSUPPORTED otherwise; a network in each of several envs: ssa_env_step_sensors_envs_f64 below);
 * 1 <= n_sensor <= SSA_MAX_SENSORS.
 * Measurement kinds: bit s of `angles_only` set -- sensor s measures azimuth and elevation only (a telescope); clear -- azimuth,
 * elevation and range (the default).  For an angles-only sensor the update is the UKF update with dim_z = 2: hx, the predicted
 * measurement and the residual are the first two components of the az-el-range ones (the azimuth wrap unchanged), R is R[s][0..1][0..1],
 * K = Pxz inv(S) with a 2 x 2 S.  Visibility, failure handling (a singular 2 x 2 S: SSA_ST_UPDATE_LINALG; a NaN in x+:
 * SSA_ST_UPDATE_NAN), update_interval, SSA_FLAG_RESAMPLE, SSA_FLAG_REFERENCE_COV and every propagator hold unchanged.  For such a sensor
 * every entry point that takes this block
 *   reads R[s][0..1][0..1] only (the third row and column of R[s] may hold anything, NaN included), and
 *   reads the first two words of each noise triple only (the tables keep three words per (sensor, step, object), so that changing a
 *   sensor's kind changes no other sensor's draws).
 * Its update record holds SSA_UPD_Y[2] = 0 and SSA_UPD_S in block form: the 2 x 2 innovation covariance in [0..1][0..1], exact zeros in
 * the rest of row and column 2 and exactly 1.0 at [2][2] -- ssa_nis_f64 on the record then returns the 2-dof NIS as it stands.
 * SSA_UPD_Z_TRUE[2] and the third column of SSA_UPD_SIGMAS_H keep the range the geometry gives: recorded, not used by the update.
 * Refused before any launch (SSA_E_INVALID), behind every other refusal of an entry: a bit set at or above n_sensor; any bit set while
 * ssa_consts.obs_type is not SSA_OBS_AER.
 * Illumination: bit s of `sunlit_only` set -- sensor s (an optical one, or a laser ranger: the test does not depend on obs_type or on the
 * sensor's kind) sees an object only while the object is sunlit and the sensor's own site is dark.  `sun` is a table of n_time rows,
 * row t = time_row of the update, the row whose `trans` matrix the same update reads: the unit vector s from the geocentre to the Sun in
 * the frame of x_true (taken as unit length, never normalised, never computed here) and the word of the sites' dark bits.  With r the
 * object's TRUE position at the time of the update, p = r.s and d2 = r.r - p p, the object is sunlit iff (p >= 0) || (d2 >= R R), R =
 * shadow_radius: the Earth's cylindrical shadow -- a NaN anywhere gives not sunlit.  For such a sensor
 *   visible = elevation >= obs_limit[s]  &&  bit s of the row's dark word  &&  sunlit;
 * an object that fails it is an invisible object in every respect (record, status, OBS_TAKEN, lookahead score NaN).  It holds in every
 * entry point that takes this block: a forecast's step h, a dry run's slot, each env's own time word in the *_envs forms.
 * With sunlit_only == 0 neither `sun` nor `shadow_radius` is read.
 * Refused before any launch (SSA_E_INVALID), behind every other refusal of an entry: a sunlit_only bit at or above n_sensor; any bit set
 * while `sun` is NULL or not 32-byte aligned; any bit set while !(shadow_radius >= 0). */
#define SSA_MAX_SENSORS 8
typedef struct ssa_sensor_params {
    int32_t n_sensor;                      /* S */
    int32_t angles_only;                   /* bit s: sensor s measures az and el only (0: every sensor measures az, el and range) */
    int32_t action[SSA_MAX_SENSORS];       /* object sensor s observes, BY VALUE (< 0: idle) */
    double enu[SSA_MAX_SENSORS][9];        /* ecef2aer's trans_uvw_ecef matrix of site s (as ssa_consts.enu) */
    double obs_itrs[SSA_MAX_SENSORS][3];   /* lla2ecef(site s) */
    double obs_limit[SSA_MAX_SENSORS];     /* elevation mask of site s [rad] */
    double R[SSA_MAX_SENSORS][9];          /* measurement noise covariance of sensor s */
    int64_t zn_stride_sensor;              /* doubles between the noise tables of consecutive sensors */
    double *upd;                           /* [S][SSA_UPD_STRIDE] update record per sensor, or NULL */
    /* illumination (appended under ABI 23; a zero tail: no sensor tests it) */
    const double *sun;                     /* [n_time] rows of 32 bytes on the device, base 32-byte aligned: doubles sx, sy, sz, then ONE int64
                                              word, bit s set = site s is dark at this row.  Not read unless sunlit_only != 0 */
    double shadow_radius;                  /* R [m] of the Earth's cylindrical shadow.  Not read unless sunlit_only != 0 */
    int32_t sunlit_only;                   /* bit s: sensor s sees only sunlit objects, and only while its site is dark */
    int32_t reserved2;                     /* 0 */
} ssa_sensor_params;
int ssa_env_step_sensors_f64(const ssa_consts *c_host, const ssa_step_params *p_host, const ssa_sensor_params *s_host, void *stream);

/* ---------------------------------------------------------------- a sensor network in each of E envs, one launch
 * ssa_env_step_sensors_f64 for every env of a vector launch: the sites (`sites`: n_sensor, angles_only, enu, obs_itrs, obs_limit, R,
 * zn_stride_sensor -- its `action` and `upd` are not read) are shared by all envs; each env tasks them on its own objects.  Per env the
 * semantics are exactly ssa_env_step_sensors_f64's: an action < 0 or >= n_obj is an idle sensor; two sensors of ONE env on one object --
 * the lowest-numbered one updates it; the same object index in two envs is two objects, both updated; a failed filter or a step the
 * update_interval skips leaves a record with SSA_UPD_ACTION = -1.
 *   rows   : env e's sensors task actions[e*SSA_MAX_SENSORS + s] (SSA_MAX_SENSORS words per row whatever S is: one aligned 32-byte read
 *            per tile) or, with SSA_LAUNCH_INLINE_ENVS, inline_action[e][s] -- the time word is then ssa_step_params.inline_time[e],
 *            else env_time[e].
 *   records: sensor s of env e writes upd + (e*S + s)*SSA_UPD_STRIDE.
 *   noise  : z_noise + e*zn_stride_env + s*zn_stride_sensor + i*zn_stride_time + a*zn_stride_obj, a = the sensor's action.
 * Of ssa_step_params it reads what ssa_env_step_sensors_f64 reads, with the same meaning, and env_time[e] / inline_time[e] and
 * zn_stride_env.  Several envs need whole tiles per env (n_obj % 4 == 0).  n_env == 1 is accepted for any n_obj and gives exactly
 * what ssa_env_step_sensors_f64 gives for row 0.
 * Refused before any launch, SSA_E_INVALID: every refusal of ssa_env_step_sensors_f64 but its n_env one, a NULL `envs`, NULL or
 * misaligned `actions` without SSA_LAUNCH_INLINE_ENVS, SSA_LAUNCH_INLINE_ENVS with n_env > SSA_INLINE_ENVS, SSA_LAUNCH_INLINE_ACTION;
 * SSA_E_UNSUPPORTED: n_env > 1 with n_obj % 4 != 0, SSA_LAUNCH_STATS_FROM_METRICS. */
typedef struct ssa_sensor_envs_params {
    const int32_t *actions;   /* [E][SSA_MAX_SENSORS] device words, base 32-byte aligned; not read (may be NULL) with SSA_LAUNCH_INLINE_ENVS */
    double *upd;              /* [E][S][SSA_UPD_STRIDE] update records, or NULL */
    int32_t inline_action[SSA_INLINE_ENVS][SSA_MAX_SENSORS];   /* with SSA_LAUNCH_INLINE_ENVS (n_env <= SSA_INLINE_ENVS) */
} ssa_sensor_envs_params;
int ssa_env_step_sensors_envs_f64(const ssa_consts *c, const ssa_step_params *p, const ssa_sensor_params *sites,
                                  const ssa_sensor_envs_params *envs, void *stream);

/* ---------------------------------------------------------------- the lookahead of a sensor network
 * ssa_lookahead_f64 for every sensor of ssa_sensor_params, in one launch (one env).  For sensor s and object j the outputs are what
 * ssa_env_step_sensors_f64 would leave for j with action[s] = j and every other sensor idle -- by the sensor step's definition, what
 * ssa_lookahead_f64 reports for j with ssa_consts' site, elevation mask and R replaced by sensor s's -- bit for bit.  The predict runs
 * once; the hypothetical update runs once per sensor.  Output rows, with m = n_obj and the caller's object numbering:
 *   score [S*m][SSA_LOOK_NSCORE], status [S*m], visible [S*m], P_post [S*m][36] (or NULL): row s * m + j;
 *   x_prior [m][6], P_prior [m][36] (or NULL): row j -- the prediction does not depend on the site.
 * Reads the same ssa_step_params fields as ssa_lookahead_f64 and, of ssa_sensor_params, n_sensor, angles_only, enu, obs_itrs, obs_limit
 * and R (its action, zn_stride_sensor and upd are not read).  Nothing is written but `out`.
 * Refused before any launch: NULL blocks or required outputs, n_sensor outside 1 .. SSA_MAX_SENSORS, a NaN elevation mask
 * (SSA_E_INVALID); n_env != 1 (SSA_E_UNSUPPORTED); and every refusal of ssa_lookahead_f64. */
int ssa_lookahead_sensors_f64(const ssa_consts *c_host, const ssa_step_params *p_host, const ssa_sensor_params *s_host,
                              const ssa_lookahead_out *out, void *stream);
/* ... in each of E envs, one launch: ssa_lookahead_sensors_f64 for every env of a vector launch.  The sites are shared by all envs; env
 * e's time word is env_time[e] or, with SSA_LAUNCH_INLINE_ENVS (n_env <= SSA_INLINE_ENVS), inline_time[e], as ssa_lookahead_f64 reads
 * them.  Per env the semantics are exactly ssa_lookahead_sensors_f64's.  Output rows, with E = n_env, m = n_obj, S = n_sensor and each
 * env's own object numbering (obj_ids honoured per env):
 *   score [E*S*m][SSA_LOOK_NSCORE], status [E*S*m], visible [E*S*m], P_post [E*S*m][36] (or NULL): row (e*S + s)*m + j;
 *   x_prior [E*m][6], P_prior [E*m][36] (or NULL): row e*m + j
 * -- env e's slab of every block is byte for byte what ssa_lookahead_sensors_f64 writes for that env alone, and what
 * ssa_assign_sensors_envs_f64 / ssa_assign_sensors_f64 take.  Nothing is written but `out`.
 * Refused before any launch: every refusal of ssa_lookahead_sensors_f64 but its n_env one; n_env * n_sensor * n_obj >= 2^31
 * (SSA_E_INVALID); several envs with n_obj % 4 != 0 (SSA_E_UNSUPPORTED: whole tiles per env, the rule of
 * ssa_env_step_sensors_envs_f64).  n_env == 1 is accepted for any n_obj and gives exactly what ssa_lookahead_sensors_f64 gives. */
int ssa_lookahead_sensors_envs_f64(const ssa_consts *c, const ssa_step_params *p, const ssa_sensor_params *sites,
                                   const ssa_lookahead_out *out, void *stream);

/* ---------------------------------------------------------------- the rollout of a sensor network: a K-step tasking schedule in one launch
 * The K launches ssa_env_step_sensors_f64 would make for the rows 0 .. K-1 of `actions`, starting from history slot slot_out - 1, with
 * every output bit-identical to them: every surviving ring slot (x_true, x, P, obs, metrics), `status`, the failure log and count, the
 * statistics of the last min(K, H) steps (np.argmax of sigma_pos included when spos_tiles is given) and the per-sensor update records of
 * the last min(K, H) steps -- but each wavefront keeps its objects' state in LDS across the steps, as ssa_env_rollout_f64 does.
 *   actions: row k = the sensors' objects at step k, SSA_MAX_SENSORS words per row whatever S is (one aligned 32-byte read per step;
 *            the base 32-byte aligned).  Entries s >= n_sensor are ignored; < 0 or >= n_obj: sensor s is idle at that step; two sensors on
 *            one object: the lowest-numbered one updates it -- as ssa_sensor_params.action.
 *   upd_ring: the records of step k go to slot (slot_out + k) mod H, [S][SSA_UPD_STRIDE] per slot, written only by the step that finally
 *            owns the slot (k >= K - H); a sensor that updates nobody gets the cleared record, as in the step.
 * `first` and `r` are read as ssa_env_rollout_f64 reads them, obj_ids included (r->actions and r->upd_ring are not read); of `sites`:
 * n_sensor, enu, obs_itrs, obs_limit, R and zn_stride_sensor (its action and upd are not read).  Two launches: the rollout and the
 * fold of the per-step statistics.
 * Refused before any launch: every refusal of ssa_env_rollout_f64 (r->actions may be NULL); NULL blocks or NULL / misaligned actions,
 * n_sensor outside 1 .. SSA_MAX_SENSORS, a NaN elevation mask, zn_stride_sensor < 0 or == 0 with S >= 2 (SSA_E_INVALID);
 * n_env != 1 (SSA_E_UNSUPPORTED). */
typedef struct ssa_rollout_sensors_params {
    const int32_t *actions;   /* [K][SSA_MAX_SENSORS] device words */
    double *upd_ring;         /* [H][S][SSA_UPD_STRIDE] or NULL */
} ssa_rollout_sensors_params;
int ssa_env_rollout_sensors_f64(const ssa_consts *c_host, const ssa_step_params *first, const ssa_rollout_params *r,
                                const ssa_sensor_params *sites, const ssa_rollout_sensors_params *rs, void *stream);
/* ... in each of E envs, one launch: exactly the K launches ssa_env_step_sensors_envs_f64 would make for the rows actions[k], with every
 * output bit-identical to them: the ring slots (slot_out + k) mod H of x_true, x, P, obs and metrics (H = 2: the two slots alternate),
 * `status`, the failure log and count, the statistics and the update records of EVERY step (stats_out, upd_out -- whatever H is), and
 * the statistics ring's slots of the last min(K, H) steps as ssa_env_rollout_f64 leaves them -- with each wavefront's objects resident
 * in LDS across the steps.  The sites are shared by all envs; env e's time index at step k is env_time[e] + time_offset + k (the time
 * words come from memory: launch_mask is not honoured); the noise is per (env, sensor, time) as in ssa_env_step_sensors_envs_f64;
 * obj_ids is honoured per env.
 *   actions  : [K][E][SSA_MAX_SENSORS] device words, 32-byte aligned, read-only for the launch.  Row (k, e) = the objects of env e's
 *              sensors at step k in env e's own numbering; entries s >= n_sensor are ignored; < 0 or >= n_obj: idle; two sensors of one
 *              env on one object: the lowest-numbered one updates it.
 *   stats_out: [K][E][SSA_STAT_STRIDE], required: the statistics of every step (np.argmax of sigma_pos included when r->spos_tiles is given).
 *   upd_out  : [K][E][S][SSA_UPD_STRIDE] or NULL: every step's per-sensor update records (every step owns its block).
 * `first` and `r` are read as ssa_env_rollout_sensors_f64 reads them (r->actions and r->upd_ring are not read).  Two launches: the
 * rollout and the fold of the per-step statistics.
 * Refused before any launch: every refusal of ssa_env_rollout_sensors_f64 but its n_env one; SSA_LAUNCH_INLINE_ENVS in launch_mask,
 * n_env * n_obj >= 2^31, NULL or misaligned `actions`, NULL `stats_out` (SSA_E_INVALID); several envs with n_obj % 4 != 0
 * (SSA_E_UNSUPPORTED: whole tiles per env).  n_env == 1 is accepted for any n_obj and runs the same kernel. */
typedef struct ssa_rollout_sensors_envs_params {
    const int32_t *actions;   /* [K][E][SSA_MAX_SENSORS] device words */
    double *stats_out;        /* [K][E][SSA_STAT_STRIDE] */
    double *upd_out;          /* [K][E][S][SSA_UPD_STRIDE] or NULL */
} ssa_rollout_sensors_envs_params;
int ssa_env_rollout_sensors_envs_f64(const ssa_consts *c_host, const ssa_step_params *first, const ssa_rollout_params *r,
                                     const ssa_sensor_params *sites, const ssa_rollout_sensors_envs_params *re, void *stream);

/* ---------------------------------------------------------------- the tasking forecast of a sensor network: H lookaheads in one launch
 * From the state ssa_lookahead_sensors_f64 reads (ssa_step_params inputs: slot i, time index time_offset), for h = 0 .. H-1 what
 * ssa_lookahead_sensors_f64 would write if ssa_env_step_sensors_f64 had first been run h times with every sensor idle -- the pass
 * forecast (visible), the covariance growth (P_prior) and the gain of an observation by sensor s at step i + 1 + h (score, P_post), for
 * every sensor and object -- bit for bit, with the state of each wavefront's objects resident in LDS across the steps as in
 * ssa_env_rollout_sensors_f64.  Step h has time index time_offset + h; the NaN rules, status codes and update_interval handling are the
 * lookahead's, per step.  The status a row carries from step h to h + 1 is the predict's: SSA_ST_UPDATE_LINALG of a hypothetical
 * update shows in output (h, s, j) only.  A row that fails inside the horizon reports the failure sentinels from then on; a row that
 * had failed before the launch passes through from the input slot.
 * Outputs, ssa_lookahead_out with a leading step axis, m = n_obj, S = n_sensor, the caller's object numbering (obj_ids):
 *   score [H][S*m][SSA_LOOK_NSCORE], status [H][S*m], visible [H][S*m] (required), P_post [H][S*m][36] (or NULL): row (h*S + s)*m + j;
 *   x_prior [H][m][6], P_prior [H][m][36] (or NULL): row h*m + j.
 * Reads the ssa_step_params fields ssa_lookahead_sensors_f64 reads, except that launch_mask is not honoured (the time word is
 * env_time[0]), and the same fields of ssa_sensor_params.  Nothing of the caller's state is written: no ring slot, status word,
 * statistics shard, failure record, update record, observation or metrics row; the measurement noise is never read.  One launch.
 * Refused before any launch: every refusal of ssa_lookahead_sensors_f64 (with `f->out` as its outputs), a NULL `f`, n_steps < 1
 * (SSA_E_INVALID). */
typedef struct ssa_forecast_params {
    int32_t n_steps;         /* H >= 1 */
    int32_t reserved;
    ssa_lookahead_out out;   /* each block with the leading step axis above */
} ssa_forecast_params;
int ssa_forecast_sensors_f64(const ssa_consts *c_host, const ssa_step_params *p_host, const ssa_sensor_params *s_host,
                             const ssa_forecast_params *f, void *stream);
/* ... in each of E envs, one launch: ssa_forecast_sensors_f64 for every env of a vector launch, as ssa_lookahead_sensors_envs_f64 is
 * ssa_lookahead_sensors_f64 for every env.  The sites are shared by all envs; env e's time word is env_time[e] or, with
 * SSA_LAUNCH_INLINE_ENVS (n_env <= SSA_INLINE_ENVS), inline_time[e] -- the only launch_mask bit honoured --, and its step h has time
 * index (time word) + time_offset + h.  Per env the semantics are exactly ssa_forecast_sensors_f64's; obj_ids is honoured per env.
 * `f` is ssa_forecast_params unchanged, its blocks with the leading axes [H][E], E = n_env, m = n_obj, S = n_sensor:
 *   score [H][E][S*m][SSA_LOOK_NSCORE], status / visible [H][E][S*m] (required), P_post [H][E][S*m][36] (or NULL):
 *       row ((h*E + e)*S + s)*m + j;
 *   x_prior [H][E][m][6], P_prior [H][E][m][36] (or NULL): row (h*E + e)*m + j
 * (64-bit offsets) -- slab h of the scores is the contiguous [E][S][m][SSA_LOOK_NSCORE] block ssa_assign_sensors_envs_f64 takes, and
 * env e's part of slab h is byte for byte what ssa_forecast_sensors_f64 writes into slab h for that env alone.  The measurement noise
 * is never read; nothing is written but `f->out`.  One launch.
 * Refused before any launch: every refusal of ssa_forecast_sensors_f64 but its n_env one; n_env * n_sensor * n_obj >= 2^31
 * (SSA_E_INVALID); SSA_LAUNCH_INLINE_ENVS with n_env > SSA_INLINE_ENVS (SSA_E_INVALID); several envs with n_obj % 4 != 0
 * (SSA_E_UNSUPPORTED: whole tiles per env).  n_env == 1 is accepted for any n_obj, runs the same kernel and gives exactly what
 * ssa_forecast_sensors_f64 gives. */
int ssa_forecast_sensors_envs_f64(const ssa_consts *c, const ssa_step_params *p, const ssa_sensor_params *sites,
                                  const ssa_forecast_params *f, void *stream);

/* ---------------------------------------------------------------- the dry run of B candidate schedules, one launch
 * What a K-step tasking schedule would be worth if it were run: ssa_env_rollout_sensors_envs_f64 with every innovation equal to zero
 * and nothing written but the records below.  The covariance update does not depend on the measurement drawn (P+ = P- - K S K^T) and
 * under the filter's own model the expected posterior mean is the prior mean, so per pseudo-env e (a block of n_obj rows -- one
 * candidate schedule) and step k = 0 .. K-1:
 *   predict: every row exactly as an idle step predicts it, time index env_time[e] + time_offset + k;
 *   actions: row (k, e) of `actions`, read as ssa_env_rollout_sensors_envs_f64 reads it -- entries s >= n_sensor are ignored; < 0 or
 *            >= n_obj_caller: idle; two sensors on one object: the lowest-numbered one updates it; update_interval is honoured;
 *   update : a row whose caller's index (obj_ids, else its index in the env) is sensor s's action runs the sensor step's update from
 *            site s (visibility of the true state, S, its inverse, K), commits P+ = P- - K S K^T to the resident tile and leaves x as
 *            the predict left it.  P+ is the step's and the lookahead's, bit for bit.  The measurement noise is never read;
 *   status : the step's -- SSA_ST_UPDATE_LINALG (singular S) fails the filter from then on, the failure sentinels in the tile; a
 *            later slot on that object is not attempted.  SSA_ST_UPDATE_NAN cannot arise.  Without a ring a failed row follows the
 *            forecast: failed at entry -- it passes through from the input block; failed inside the horizon -- the sentinels.
 * Output: one record of SSA_DRY_STRIDE doubles per slot, out[((k*E + e)*S + s)*SSA_DRY_STRIDE + ...]:
 *   SSA_DRY_ACTION : the caller's index of the object if the update was attempted, else -1 (as SSA_UPD_ACTION)
 *   SSA_DRY_VISIBLE, SSA_DRY_TAKEN : 1 / 0
 *   SSA_DRY_STATUS : the SSA_ST_* the object carries after the step; 0 for a slot that updates nobody
 *   SSA_DRY_SCORE + SSA_LOOK_TRACE_GAIN / POS_TRACE_GAIN / INFO_GAIN: from this step's P- and P+ exactly as ssa_lookahead_sensors_f64
 *                    computes them; NaN unless taken
 *   SSA_DRY_SPARE  : 0
 * A slot that updates nobody -- idle, out of range, a lower sensor's object, a step the interval skips -- gets the cleared record
 * (ACTION -1, zeros, NaN scores), written by the env's first row; a tasked filter that has failed gets ACTION -1, zeros, its status
 * and NaN scores from its own row.  A valid action that no row of its env holds (obj_ids) leaves its record unwritten.  Nothing else
 * is written: no ring slot, status word, failure record, statistics word, observation row or update record; the tile is not stored.
 * Of ssa_step_params it reads the INPUT fields ssa_forecast_sensors_envs_f64 reads; obj_ids is per env, and an id of -1 marks a padding
 * row that matches no action and writes nothing; launch_mask is not honoured (the time words come from env_time).  Of `sites`:
 * n_sensor, enu, obs_itrs, obs_limit and R.  One launch.
 * Refused before any launch: every refusal of ssa_forecast_sensors_envs_f64 that applies (with d->out as its output), a NULL `d`,
 * n_steps < 1, NULL or misaligned `actions`, NULL `out`, n_obj_caller < 1, n_env * n_sensor * n_steps >= 2^31 (SSA_E_INVALID);
 * several envs with n_obj % 4 != 0 (SSA_E_UNSUPPORTED: whole tiles per env).  n_env == 1 is accepted for any n_obj: the full-catalogue
 * form on a ring slot. */
#define SSA_DRY_STRIDE 8
#define SSA_DRY_ACTION 0
#define SSA_DRY_VISIBLE 1
#define SSA_DRY_TAKEN 2
#define SSA_DRY_STATUS 3
#define SSA_DRY_SCORE 4
#define SSA_DRY_SPARE 7
typedef struct ssa_dryrun_sensors_params {
    int32_t n_steps;          /* K >= 1 */
    int32_t n_obj_caller;     /* actions >= this are idle: the catalogue's size, which a gathered block's n_obj is not */
    const int32_t *actions;   /* [K][E][SSA_MAX_SENSORS] device words, 32-byte aligned, read-only */
    double *out;              /* [K][E][S][SSA_DRY_STRIDE], required */
} ssa_dryrun_sensors_params;
int ssa_dryrun_sensors_envs_f64(const ssa_consts *c, const ssa_step_params *p, const ssa_sensor_params *sites,
                                const ssa_dryrun_sensors_params *d, void *stream);
/* ... and the totals of its records: total[e*SSA_LOOK_NSCORE + c] = the sum of SSA_DRY_SCORE + c over env e's slots with SSA_DRY_TAKEN
 * set, added in slot order (k outer, s inner) in fp64 -- one defined sum per candidate and column; 0 for a candidate that takes nothing.
 * records: [K][E][S][SSA_DRY_STRIDE] as ssa_dryrun_sensors_envs_f64 leaves them; total: [E][SSA_LOOK_NSCORE].  One launch.
 * Refused before any launch (SSA_E_INVALID): NULL records or total, a count < 1, n_sensor > SSA_MAX_SENSORS,
 * n_env * n_sensor * n_steps >= 2^31. */
int ssa_dryrun_totals_f64(const double *records, int32_t n_env, int32_t n_steps, int32_t n_sensor, double *total, void *stream);
/* ... and the gathered block in front of it, for B candidates in each of E envs: the E * B pseudo-envs of W rows that
 * ssa_dryrun_sensors_envs_f64 then takes (n_env = E * B, n_obj = W, obj_ids = ids, env_time = time_out), copied out of the envs' state
 * in ONE launch.  Output row q = (e * B + b) * W + w:
 *   j = ids[q]; an id < 0 or >= n_obj (padding, or anything else) is replaced by the candidate's first id, ids[(e * B + b) * W], taken
 *   as 0 when negative and as n_obj - 1 when >= n_obj -- a padding row carries the state of the candidate's first object, and of object 0
 *   in an all-idle candidate: a healthy row to predict;
 *   r = e * n_obj + j, the caller's global row; with a slot_of table r = slot_of[r], the storage row (an entry outside 0 .. E * n_obj - 1
 *   is brought to the nearest end: the launch reads inside the source blocks whatever ids and slot_of hold);
 *   rows r of x_true_in, x_in, P_in (6, 6 and 36 doubles) and word r of status_in are copied to row q of the outputs, bit for bit;
 *   time_out[e * B + b] = env_time[e].
 * Nothing else is written.  The outputs must not overlap the inputs or one another.
 * Refused before any launch (SSA_E_INVALID): a NULL block, any NULL pointer but slot_of, a count < 1, n_rows % 4 != 0, reserved != 0,
 * E * B * W >= 2^31 or E * n_obj >= 2^31, one of the six double pointers not 16-byte aligned (the rows move as 16-byte pieces). */
typedef struct ssa_dryrun_gather_params {
    int64_t n_obj;             /* m: rows per env in the source block */
    int32_t n_env, n_cand;     /* E >= 1, B >= 1 */
    int32_t n_rows, reserved;  /* W >= 4, W % 4 == 0;  reserved == 0 */
    const int32_t *ids;        /* [E*B][W]: the caller's object index, -1 = padding */
    const int32_t *slot_of;    /* [E*m] caller's global row -> storage row, or NULL */
    const int32_t *env_time;   /* [E] */
    const double *x_true_in, *x_in, *P_in;  const int32_t *status_in;   /* [E*m] rows of 6 / 6 / 36 doubles, 1 word */
    double *x_true_out, *x_out, *P_out;  int32_t *status_out;           /* [E*B*W] rows */
    int32_t *time_out;         /* [E*B] */
} ssa_dryrun_gather_params;
int ssa_dryrun_gather_f64(const ssa_dryrun_gather_params *g, void *stream);

/* ---------------------------------------------------------------- the tasking assignment of a sensor network, on the device
 * One object per sensor from one column of the scores ssa_lookahead_sensors_f64 leaves, in ONE launch and written where the next launch
 * reads it: the global greedy assignment of agents._assign_lookahead_sensors (S ssa_masked_argmax_f64 launches, S read-backs and the
 * host's mask edits between them).  Among all remaining (s, j) whose score[(s * n_obj + j) * SSA_LOOK_NSCORE + column] is not NaN the
 * largest value assigns object j to sensor s (compared by value: -0.0 == 0.0, +-inf are ordinary values; equal values: the lowest
 * s * n_obj + j, the first maximum of ssa_masked_argmax_f64); sensor s and object j leave the pool; repeated until n_sensor rounds are
 * done or nothing but NaN is left.
 * A sensor left without an object: with fallback == NULL it stays idle (-1).  Otherwise fallback holds SSA_MAX_SENSORS device words,
 * the caller's draws, and the sensors are taken in ascending s: sensor s takes fallback[s] if 0 <= fallback[s] < n_obj and no sensor
 * holds that object yet -- assigned (any s) or fallen back (a lower s) -- and stays idle otherwise.  No object is named twice.
 *   action_out: SSA_MAX_SENSORS device words, 32-byte aligned: one row of ssa_rollout_sensors_params.actions; entries s >= n_sensor = -1.
 *   pick_out  : [SSA_MAX_SENSORS][2] or NULL: per sensor the ASSIGNED object (-1: fallen back or idle; s >= n_sensor: -1) and the bit
 *               pattern of its winning score (0 without one) -- as the pick_out of ssa_agent_select_f64.
 *   workspace : ssa_assign_sensors_workspace_bytes(n_obj, n_sensor) bytes of device memory, 16-byte aligned, zeroed ONCE by the caller
 *               (the last workgroup to arrive leaves its ticket word at zero); one call at a time per workspace (calls in one stream are).
 * One launch: ceil(n_obj / 512) workgroups keep, per sensor, the S best candidates of their objects; the last one to arrive merges them
 * and assigns.  Refused before any launch (SSA_E_INVALID): NULL score or action_out, a misaligned action_out, n_sensor outside
 * 1 .. SSA_MAX_SENSORS, column outside 0 .. SSA_LOOK_NSCORE - 1, n_obj < 1 (or > INT32_MAX: an action is an int32 word), a workspace
 * that is NULL, misaligned or too small.  ssa_assign_sensors_workspace_bytes returns SSA_E_INVALID for n_obj / n_sensor out of range. */
int ssa_assign_sensors_f64(const double *score, int64_t n_obj, int32_t n_sensor, int32_t column, const int32_t *fallback,
                           int32_t *action_out, int64_t *pick_out, void *workspace, int64_t workspace_bytes, void *stream);
int64_t ssa_assign_sensors_workspace_bytes(int64_t n_obj, int32_t n_sensor);
/* ... of every env of a vector launch, one launch, written into the [E][SSA_MAX_SENSORS] action table ssa_env_step_sensors_envs_f64
 * reads (ssa_sensor_envs_params.actions).  Env e's row and picks are exactly what ssa_assign_sensors_f64 writes for env e's slab of
 * `score`, env e's fallback row and a workspace of its own: the same order, tie rule, NaN rule, fallback rule and -1 beyond S.  The same
 * object index may be assigned in two envs: they are two objects.
 *   score     : [E][S][m][SSA_LOOK_NSCORE], as ssa_lookahead_sensors_envs_f64 leaves it
 *   fallback  : NULL, or [E][SSA_MAX_SENSORS] device words
 *   action_out: [E][SSA_MAX_SENSORS] device words, the base 32-byte aligned
 *   pick_out  : NULL, or [E][SSA_MAX_SENSORS][2]
 *   workspace : ssa_assign_sensors_envs_workspace_bytes(n_obj, n_sensor, n_env) bytes of device memory, 64-byte aligned, zeroed ONCE by
 *               the caller: n_env parts, each the one-env workspace rounded up to 64 bytes, with a ticket word of its own that its
 *               env's last arrival leaves at zero; one call at a time per workspace.
 * One launch of ceil(n_obj / 512) x n_env workgroups; the last workgroup to arrive FOR ITS ENV merges and assigns that env.
 * Refused before any launch (SSA_E_INVALID): the refusals of ssa_assign_sensors_f64, n_env < 1 (or > 65535: the grid's second
 * dimension), n_env * n_sensor * n_obj >= 2^31, a workspace that is NULL, not 64-byte aligned or smaller than the query.
 * ssa_assign_sensors_envs_workspace_bytes returns SSA_E_INVALID for n_obj / n_sensor / n_env out of range. */
int ssa_assign_sensors_envs_f64(const double *score, int64_t n_obj, int32_t n_sensor, int32_t n_env, int32_t column,
                                const int32_t *fallback, int32_t *action_out, int64_t *pick_out,
                                void *workspace, int64_t workspace_bytes, void *stream);
int64_t ssa_assign_sensors_envs_workspace_bytes(int64_t n_obj, int32_t n_sensor, int32_t n_env);

/* ---------------------------------------------------------------- the OPTIMAL assignment of a sensor network, on the device
 * The arguments, the workspace (layout, size queries, alignment, zeroed once), the refusals and their order, action_out, pick_out and the
 * fallback rule of ssa_assign_sensors_f64 / ssa_assign_sensors_envs_f64 -- but the exact one-step optimum instead of the greedy rounds.
 * A pair (s, j) is a CANDIDATE iff its score[(s * n_obj + j) * SSA_LOOK_NSCORE + column] is finite and of magnitude <= 2^1020.  NaN is
 * "not a candidate", as for the greedy rule; UNLIKE the greedy rule, where +-inf are ordinary values, +-inf and anything above 2^1020
 * are not candidates either: a sum that contains them has no order (or overflows: the rule compares sums of up to eight scores).
 * Among all assignments of distinct objects to sensors over candidates the result has
 *   1. the largest number of tasked sensors (so a sensor whose only candidate scores below zero is still tasked), and
 *   2. among those, the largest sum of scores.  With the gains ssa_lookahead_sensors_f64 writes (>= 0) the two agree.
 * The only rounding in the decision is that of the sums of at most n_sensor scores it compares, each added up in ascending object
 * index: the result's sum is within 2 S (S - 1) 2^-53 max|score| of the optimum's, and IS the optimum where those sums are exact.
 * Ties (-0.0 == 0.0) are broken by one fixed rule -- objects are taken in ascending index, a sensor subset keeps the assignment it has
 * unless a sum is strictly greater, among sensors that give equal sums the lowest s; at the end the subset of most sensors, then of
 * largest sum, then the lowest read as a binary number (bit s: sensor s) -- so the row is a pure function of the input bits: the same from
 * every call and from both entries.  With n_sensor == 1 and finite scores it is the greedy row (first maximum, lowest j).
 * One workspace may serve greedy and optimal calls in any order without being zeroed again. */
int ssa_match_sensors_f64(const double *score, int64_t n_obj, int32_t n_sensor, int32_t column, const int32_t *fallback,
                          int32_t *action_out, int64_t *pick_out, void *workspace, int64_t workspace_bytes, void *stream);
int ssa_match_sensors_envs_f64(const double *score, int64_t n_obj, int32_t n_sensor, int32_t n_env, int32_t column,
                               const int32_t *fallback, int32_t *action_out, int64_t *pick_out,
                               void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- the horizon-wide OPTIMAL tasking plan of a sensor network, on the device
 * A whole forecast turned into a schedule in ONE launch: the plan as ONE assignment problem over all its (step, sensor) pairs, instead of
 * one assignment per step in time order with the earlier steps' objects masked out (additive: the ABI version stays).
 * A SLOT is a pair (h, s); there are N = n_step * n_sensor of them, 1 <= N <= SSA_MAX_PLAN_SLOTS.  A triple (h, s, j) is a CANDIDATE iff
 * its score[(((h * n_env + e) * n_sensor + s) * n_obj + j) * SSA_LOOK_NSCORE + column] is finite and of magnitude <= 2^1020 (the
 * candidate test of ssa_match_sensors_f64: NaN, +-inf and anything above 2^1020 are not candidates).  A PLAN gives each slot at most one
 * candidate object and gives no object to two slots of the same env, in any step (the forecast's gains are gains of a FIRST observation).
 * Among all plans the result has
 *   1. the most filled slots -- exact for every input: the count is decided on integers, no large constant is added to any double --, and
 *   2. among those, the largest sum of scores.
 * Arithmetic of 2.: the scores of the N best candidates of each slot (that table suffices: DESIGN.md section 8o) are rounded ONCE to
 * int64 multiples of the unit 2^(e - 52), 2^e the smallest power of two above the table's largest magnitude, and everything after that is
 * exact integer arithmetic.  So the sum IS the exact optimum whenever the table's scores are multiples of that unit -- guaranteed for
 * dyadic tables (multiples of 2^-10 of magnitude below 2^10) --, and for any other input the result's sum is within
 *     4 N 2^-53 max|candidate score|
 * of the optimum's (each of the <= N scores on either side moves by at most half a unit, and the unit is <= 4 * 2^-53 * the largest
 * magnitude).  -0.0 == 0.0.
 * Ties are broken by one fixed rule: the slots enter a shortest-augmenting-path solver in ascending h * n_sensor + s; a slot's candidates
 * are ranked by (score descending, object ascending); costs are pairs (idle slots, -sum) compared lexicographically; the unscanned slot
 * of least distance is scanned next, the lowest slot among equals; a free object (or the slot's own idleness, ranked last) replaces the
 * best end found so far only if strictly nearer, within one scan the lowest rank; a slot's distance and predecessor change only for a
 * strictly smaller distance; the search ends as soon as no unscanned slot is strictly nearer than the best end.  So the plan is a pure
 * function of the input bits: the same from every call, and the same for an env whether it is planned alone or as one of n_env.  With
 * N == 1 and finite scores it is the first maximum (lowest j), as for ssa_assign_sensors_f64.  There is no fallback argument: an
 * unfilled slot is -1.
 *   score     : [n_step][n_env][n_sensor][n_obj][SSA_LOOK_NSCORE]: exactly what ssa_forecast_sensors_envs_f64 leaves, and with
 *               n_env == 1 exactly what ssa_forecast_sensors_f64 leaves
 *   plan_out  : [n_step][n_env][SSA_MAX_SENSORS] device words, the base 32-byte aligned; -1 beyond n_sensor and in unfilled slots: the
 *               action table ssa_env_rollout_sensors_envs_f64 reads, and with n_env == 1 the one ssa_env_rollout_sensors_f64 reads
 *   pick_out  : NULL, or [n_step][n_env][SSA_MAX_SENSORS][2]: the object (-1: none) and the bit pattern of its score (0 without one)
 *   workspace : ssa_plan_sensors_workspace_bytes(n_obj, n_sensor, n_step, n_env) bytes of device memory, 64-byte aligned, zeroed ONCE by
 *               the caller (per env a ticket word that the env's last workgroup to arrive leaves at zero); one call at a time per workspace.
 * One launch of ceil(n_obj / 512) x n_env workgroups that reads the scores once.  Refused before any launch (SSA_E_INVALID), in this
 * order: NULL score or plan_out; a misaligned plan_out; n_sensor outside 1 .. SSA_MAX_SENSORS; n_step < 1; n_step * n_sensor >
 * SSA_MAX_PLAN_SLOTS; n_env outside 1 .. 65535; column outside 0 .. SSA_LOOK_NSCORE - 1; n_obj < 1; n_step * n_env * n_sensor * n_obj >=
 * 2^31; a workspace that is NULL, misaligned or too small.  The size query returns SSA_E_INVALID for the same ranges. */
#define SSA_MAX_PLAN_SLOTS 64
int ssa_plan_sensors_f64(const double *score, int64_t n_obj, int32_t n_sensor, int32_t n_step, int32_t n_env, int32_t column,
                         int32_t *plan_out, int64_t *pick_out, void *workspace, int64_t workspace_bytes, void *stream);
int64_t ssa_plan_sensors_workspace_bytes(int64_t n_obj, int32_t n_sensor, int32_t n_step, int32_t n_env);

/* ---------------------------------------------------------------- visibility screen of a synthetic orbit catalogue
 * catalogue._accepted (orbit_gen.py's acceptance rule) for n candidate element sets, the observer generalised to a network of
 * n_site ground sites.  Candidate c = elements[c] = (a, ecc, inc, raan, argp, nu) (m, -, rad) is propagated by Kepler's equation
 * (12 Newton steps from E = M + e sin M) to t = step * i for i < n_time and rotated to ITRS by trans[i].  Sample i passes the
 * altitude test if |x| - WGS84_A (1 - WGS84_F sin^2 lat) > min_alt, and is visible if asin(up_s / |x - obs_itrs_s|) >= el_min_s for
 * ANY site s (one site: exactly _accepted).  With worst = the longest run of consecutive invisible samples:
 *   accept[c] = every sample passes the altitude test && (every sample visible
 *               || (some sample in [0, first) visible && worst < max_gap))
 *   worst_gap[c] = worst (optional); flags[c] = bit 0 altitude ok, bit 1 visible in [0, first), bit 2 always visible (optional).
 * Refused before any launch (SSA_E_INVALID): n < 0, n_time < 1, n_site outside 1 .. SSA_MAX_SENSORS, first < 0, and with n > 0
 * NULL elements / trans / sites / accept.  n == 0 launches nothing. */
typedef struct ssa_screen_params {
    int64_t n;                 /* candidates */
    int32_t n_time;            /* samples per candidate (T) */
    int32_t n_site;            /* S */
    double step;               /* seconds between samples */
    double min_alt;            /* altitude floor [m] */
    int32_t first;             /* first-window length [samples] */
    int32_t max_gap;           /* a run of max_gap invisible samples rejects [samples] */
    const double *elements;    /* [n][6] */
    const double *trans;       /* [n_time][3][3] GCRS -> ITRS, row-major (trans_matrix_table) */
    const double *sites;       /* [n_site][13]: enu[9] (row-major, host.enu_matrix), obs_itrs[3] [m], el_min [rad] */
    uint8_t *accept;           /* [n] */
    int32_t *worst_gap;        /* [n] or NULL */
    uint8_t *flags;            /* [n] or NULL */
} ssa_screen_params;
int ssa_catalogue_screen_f64(const ssa_screen_params *p, void *stream);

/* EXTENSION (ABI 23, additive): the screen by a network's OWN visibility rule -- ssa_catalogue_screen_f64 with every sensor judged as
 * the fused kernels judge it (ssa_step_params.site_rows / site_moving, ssa_sensor_params.sun / sunlit_only).  Candidates, samples, the
 * altitude test and the fold of accept / worst_gap / flags from the per-sample verdicts are those of `base`, unchanged.  With r the
 * candidate's inertial position at sample i (before the rotation) and x = trans[i] r, sensor s sees sample i if
 *   no site_moving bit s:  asin(up_s / |x - obs_itrs_s|) >= el_min_s on base.sites[s]                (the ground mask, as above)
 *   site_moving bit s:     los_clear(x - o, o, limb_radius), o = the obs_itrs words of site_rows row (i, s): the segment from the sensor
 *                          to the object stays outside the sphere of radius limb_radius.  base.sites[s] is NOT read, nor the row's enu words
 *   sunlit_only bit s:     additionally the object outside the Earth's cylindrical shadow -- (p >= 0) || (d2 >= R R), p = r.sun_i,
 *                          d2 = r.r - p p, R = shadow_radius -- and, for a GROUND sensor, bit s of row i's dark word.  A moving sensor's
 *                          dark bit is NOT read
 * and a NaN anywhere gives "not visible".  A sample is visible if any sensor sees it.  seen_by[c] (optional): bit s set iff sensor s
 * sees candidate c at one sample or more.  Row i of site_rows and of sun belongs to sample i, the sample trans[i] belongs to.
 * Bit 0 of site_moving is ALLOWED here: the screen has no primary observer and no ssa_consts, so sensor 0 may be in orbit (a network
 * of one space-based sensor).  The step entries keep refusing it.
 * With site_moving == 0 neither site_rows nor limb_radius is read; with sunlit_only == 0 neither sun nor shadow_radius; with both 0
 * the three outputs are those of ssa_catalogue_screen_f64 on `base`.
 * Refused before any launch (SSA_E_INVALID), in this order: a NULL block; every refusal of ssa_catalogue_screen_f64 on `base`, in its
 * order; reserved != 0; a site_moving bit at or above n_site; any such bit with site_rows NULL or not 128-byte aligned; any such bit
 * with !(limb_radius >= 0); a sunlit_only bit at or above n_site; any such bit with sun NULL or not 32-byte aligned; any such bit with
 * !(shadow_radius >= 0).  n == 0 launches nothing. */
typedef struct ssa_screen_network_params {
    ssa_screen_params base;     /* every field with its present meaning */
    const double *site_rows;    /* [base.n_time][base.n_site][16]; layout and 128-byte base alignment of ssa_step_params.site_rows;
                                   row (i, s) belongs to sample i, the sample trans[i] belongs to; read only for sensors with a bit
                                   in site_moving */
    const double *sun;          /* [base.n_time] rows of 32 bytes; layout and 32-byte base alignment of ssa_sensor_params.sun
                                   (sx, sy, sz in the frame of the candidate's inertial position, then the int64 word of dark bits);
                                   read only if sunlit_only != 0 */
    double limb_radius, shadow_radius;
    int32_t site_moving, sunlit_only;   /* bit s, as in ssa_step_params / ssa_sensor_params */
    uint8_t *seen_by;           /* [n] or NULL: bit s set iff sensor s sees the candidate at one sample or more */
    int64_t reserved;           /* 0 */
} ssa_screen_network_params;
int ssa_catalogue_screen_network_f64(const ssa_screen_network_params *p, void *stream);

/* ---------------------------------------------------------------- the pass table of a sensor network: a whole episode in one launch
 * EXTENSION (ABI 23, additive; no reference counterpart).  The visibility test of every fused kernel is judged on the TRUE state, and
 * the truth chain x_true[i + 1] = propagate(x_true[i], dt) depends on no action, no noise draw and no filter: which sensor can see
 * which object at which step of the rest of an episode is known when the episode starts.  This entry produces all of it, under the
 * network's own rule, in one launch.
 * Inputs: of ssa_step_params the fields a lookahead reads -- x_true_in, trans, env_time, time_offset, n_time, n_obj, n_env, obj_ids,
 * site_rows, limb_radius, site_moving and, the only launch_mask bit honoured, SSA_LAUNCH_INLINE_ENVS with inline_time (as
 * ssa_lookahead_f64); of ssa_sensor_params n_sensor, enu, obs_itrs, obs_limit, sun, shadow_radius, sunlit_only; of ssa_consts dt,
 * propagator, j2, r_eq, rk4_substeps; T = n_steps.  For h = 0 .. T-1, env e, sensor s and object j:
 *   x_{h+1}  the truth after h + 1 CHAINED propagations by dt with the env's propagator -- the chain the step kernels run, not one
 *            propagation by (h + 1) dt.  Every SSA_PROP_* value, through the device functions of the stand-alone operators
 *            (ssa_propagate_f64 / ssa_propagate_j2_f64), which are the ones the step kernels run on a healthy state;
 *   row      time_row(env_time[e] + time_offset + h, n_time) (inline_time[e] with SSA_LAUNCH_INLINE_ENVS): the row of `trans`, of the
 *            Sun table and of site_rows alike;
 *   access(h, e, s, j), the fused kernels' verdict for sensor s on x_{h+1}:
 *            a ground sensor      elevation (hx_aer_erfa from enu[s] / obs_itrs[s]) >= obs_limit[s];
 *            a site_moving sensor the line of sight from row (row, s) of site_rows clear of the sphere limb_radius (obs_limit not read);
 *            a sunlit_only bit    additionally the object outside the Earth's cylindrical shadow, and for a ground sensor bit s of
 *                                 the row's dark word;
 *            a NaN anywhere       0.
 * The filter's status and ssa_consts.update_interval do NOT enter: a forecast's visible[h] == access[h] AND (the update would be
 * attempted -- the filter has not failed, the step is not one the update_interval skips).
 * Outputs, in the caller's object numbering (obj_ids honoured per env: a storage layout never shows), E = n_env, S = n_sensor,
 * m = n_obj, W = ceil(T / 64):
 *   bits   uint64 [E][S][m][W], required, 8-byte aligned: bit (h mod 64) of word (h div 64) of row (e, s, j) is access(h, e, s, j);
 *          bits at h >= T are 0.  Packed along TIME, per object: the mask of step k is (bits[..., k / 64] >> (k % 64)) & 1.
 *   pass   int32 [E][S][m][4] or NULL, over the steps counted: first (smallest h with the bit set, -1: none), length (consecutive set
 *          bits from `first`), count (set bits), passes (maximal runs of set bits).
 *   n_left const int32 [E] device words or NULL: env e counts only h < min(T, n_left[e]) (a value < 0 counts as 0); later bits are
 *          0.  NULL: T for every env.
 *   env_sel / n_sel: const int32 [n_sel] device words, or NULL with n_sel == 0 (= every env).  Only the named envs are computed and
 *          only their slabs of bits / pass are written; every other byte is left as it is (a vector env refreshes the envs that
 *          have just auto-reset).  A word outside 0 .. n_env - 1 names no env: nothing is computed or written for it.
 * Nothing else is written: no ring slot, status word, record, statistic or observation; z_noise, x_in, P_in and status are not read,
 * nor of ssa_sensor_params angles_only, R, action, zn_stride_sensor, upd.  Any n_env >= 1 and any n_obj (every env starts on a wavefront
 * boundary; no whole-tile rule).  One launch.
 * Refused before any launch, SSA_E_INVALID, in this order: a NULL block; n_obj < 1 or n_env < 1; NULL x_true_in, trans or env_time;
 * SSA_LAUNCH_INLINE_ENVS with n_env > SSA_INLINE_ENVS; an unknown propagator (SSA_PROP_J2_RK4: rk4_substeps outside 1 .. 4096);
 * n_sensor outside 1 .. SSA_MAX_SENSORS; a NaN elevation mask; n_steps < 1; NULL or misaligned bits; n_sel < 0; n_sel > 0 with a NULL
 * env_sel; n_sel > n_env; n_env * n_sensor * n_obj * W >= 2^31; and, behind all of these, the rules of the sensor tail for sunlit_only
 * (ssa_sensor_params) and site_moving (ssa_step_params) as every sensor entry applies them.  ssa_consts.obs_type is read by the
 * site_moving rule alone (a moving sensor needs SSA_OBS_AER, as everywhere) and is not judged otherwise. */
typedef struct ssa_access_params {
    int32_t n_steps;          /* T >= 1 */
    int32_t n_sel;            /* 0: every env; else the number of words of env_sel */
    uint64_t *bits;           /* [E][S][m][W] */
    int32_t *pass;            /* [E][S][m][4] (first, length, count, passes) or NULL */
    const int32_t *n_left;    /* [E] or NULL */
    const int32_t *env_sel;   /* [n_sel] or NULL */
} ssa_access_params;
#define SSA_PASS_FIRST 0
#define SSA_PASS_LENGTH 1
#define SSA_PASS_COUNT 2
#define SSA_PASS_PASSES 3
int ssa_access_sensors_f64(const ssa_consts *c, const ssa_step_params *p, const ssa_sensor_params *sites,
                           const ssa_access_params *a, void *stream);

/* ------------------------------------------------ all-gather by direct peer stores (SURVEY 8e "Collective")
 * The reference runs one env per process and has no exchange step; the sharded env of this library (one env's objects spread over the
 * GPUs of a node) reassembles every step's observation block + statistics words on every rank.  These two entry points do that without a
 * collective library: after the step kernel of step k a rank PUSHES its payload (n_words doubles at src) into the slot it owns in each of
 * n_peer receive buffers -- dst[r], device pointers the host obtained once by mapping every peer's buffer over hipIpc (its own buffer
 * included: dst of the own rank is a local pointer) -- and then stores the step number into flag[r] (release, system scope).  A consumer
 * WAITS until the n_src flag words of its own buffer have reached the step number.  The step number of a launch is seq_base[0] + seq_off:
 * seq_base lives in device memory so that a replayed hipGraph can advance it (as ssa_step_params.env_time does for the time index).
 * Plain kernels: capturable at any world size, no rendezvous inside the launch, no RCCL communicator.  The wait is bounded: a source that
 * has not arrived after timeout_ticks of the 100 MHz wall clock (0 = 2 s) sets error[0] = 1 + its index (if error != NULL) and the kernel
 * ends.  Flags only grow; the caller rotates >= 2 receive buffers (ssa-gym_amd/parallel.py: 3) and pushes step k to a peer only after that
 * peer's payload of step k - 1 has arrived (its readers of the slot being overwritten have then passed, in its stream order): pass the
 * rank's own flag words of the previous step's buffer as prev_flags and the push waits for exactly that, per peer, inside its launch
 * (bounded like ssa_peer_wait; NULL = the caller has waited).  tickets: n_peer zeroed 32-bit device words owned by this exchange (a push
 * is several workgroups per peer; the last one to finish raises the flag and leaves the ticket at zero). */
int ssa_peer_push_f64(const double *src, int64_t n_words, double *const *dst, uint64_t *const *flag, int32_t n_peer,
                      const uint64_t *seq_base, uint64_t seq_off, const uint64_t *prev_flags, int64_t timeout_ticks, int32_t *error,
                      uint32_t *tickets, void *stream);
int ssa_peer_wait(const uint64_t *flags, int32_t n_src, const uint64_t *seq_base, uint64_t seq_off, int64_t timeout_ticks, int32_t *error,
                  void *stream);

/* library identification */
int ssa_abi_version(void);
const char *ssa_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* SSA_HIP_H */
