"""step_plain_kernel: the one-tile step kernel compiled for the plain one-env launch form (ActPlain, ssa_kernels.hip), and the routing
that sends a launch to it.  Without a GPU: the family's budget against its generic twin from the shipped code object, and the routing
table through the host-only query ssa_env_step_instance() on bare parameter blocks (no pointer is followed, nothing is launched).

The plain form (include/ssa_hip.h, SSA_LAUNCH_GENERIC): no sensor network, one env, one tile per wavefront, SSA_LAUNCH_DEFER_FOLD |
SSA_LAUNCH_STATS_FROM_METRICS and no other launch bit, `actions` given, no aer_out / obs_mirror / spos_tiles / spos_tiles_prev /
stat_shards_clear, update_interval <= 1, no SSA_FLAG_RESAMPLE, SSA_OBS_AER, SSA_LAUNCH_GENERIC clear.  A sensor network goes through
entries of its own (ssa_env_step_sensors*_f64), which never reach the plain family: the query has no argument that could name one.
Four conditions cannot be broken alone without the launcher refusing the block -- SSA_LAUNCH_STATS_FROM_METRICS itself demands one env,
one tile per wavefront, a deferred fold, no SSA_LAUNCH_FOLD_INSIDE and no stat_shards_clear, and a missing `actions` is invalid
without an inline action: for those the query must answer the launcher's own code, and 0 for the nearest block the launcher accepts."""
import ctypes as C

import pytest

from support.codeobj import _kernels, assert_family_budget, family, twin
from support.gpu import pkg  # noqa: F401  (the module fixture)
from support.refusals import PTR, valid_blocks


def test_plain_family_fits_its_twins_budget(tmp_path):
    kern, ins_of = _kernels(tmp_path)
    assert_family_budget(kern, ins_of, "step_plain_kernel", "step_fast_kernel", 4, same_args=True)
    for name in family(kern, "step_plain_kernel"):
        ins, generic = ins_of[name], ins_of[twin(kern, name, "step_fast_kernel")]
        assert not [op for op in ins if op.startswith("flat_load")], name
        assert len(ins) < len(generic), (name, len(ins), len(generic))
        for other in ("step_fast_kernel", "rollout_kernel", "closed_loop_kernel"):      # (families the other host tests count by substring)
            assert other not in name


def bench_form():
    """the block of the benchmark's launches: one env, deferred fold, statistics from the metrics rows, a storage layout, the previous
    step's hand-over"""
    from ssa_gym_amd import _lib
    b = valid_blocks("ssa_env_step_f64")
    p = b["p"]
    p.launch_mask = _lib.LAUNCH_DEFER_FOLD | _lib.LAUNCH_STATS_FROM_METRICS
    p.stat_shards, p.stats, p.upd, p.obj_ids = PTR, PTR, PTR, PTR
    p.stat_shards_prev, p.stats_prev, p.metrics_prev = 2 * PTR, PTR, PTR
    p.fail_log, p.fail_count, p.fail_cap = PTR, PTR, 8
    return b


def ask(b):
    from ssa_gym_amd import _lib
    return _lib.load().ssa_env_step_instance(C.byref(b["c"]), C.byref(b["p"]))


def launch_code(b):
    """the launcher's answer -- for blocks it refuses only (a refusal comes before any launch)"""
    from ssa_gym_amd import _lib
    return _lib.load().ssa_env_step_f64(C.byref(b["c"]), C.byref(b["p"]), None)


def _set(which, **kw):
    def f(b):
        for k, v in kw.items():
            setattr(b[which], k, v)
    return f


def _mask(set_bits=0, clear_bits=0):
    def f(b):
        b["p"].launch_mask = (b["p"].launch_mask | set_bits) & ~clear_bits
    return f


def test_the_benchmarks_form_is_plain_and_what_stays_a_run_time_decision_keeps_it_so(pkg):
    from ssa_gym_amd import _lib
    assert ask(bench_form()) == 1
    for spoil in (_set("p", obj_ids=0), _set("p", upd=0), _set("p", fail_log=0, fail_count=0, fail_cap=0), _set("c", flags=_lib.FLAG_REFERENCE_COV),
                  _set("p", n_obj=66), _set("p", n_obj=20000), _set("c", update_interval=0), _set("c", update_interval=1),
                  _set("p", stat_shards_prev=0, stats_prev=0, metrics_prev=0)):
        b = bench_form()
        spoil(b)
        assert ask(b) == 1
    for prop in (_lib.PROP_ELEMENTS, _lib.PROP_FG, _lib.PROP_HYBRID):
        b = bench_form()
        b["c"].propagator = prop
        assert ask(b) == 1


def test_every_single_condition_flipped_takes_the_generic_instance(pkg):
    from ssa_gym_amd import _lib
    L = _lib
    both = L.LAUNCH_DEFER_FOLD | L.LAUNCH_STATS_FROM_METRICS
    flips = {
        "no statistics from the metrics rows": _mask(clear_bits=L.LAUNCH_STATS_FROM_METRICS),
        "inline action": _mask(set_bits=L.LAUNCH_INLINE_ACTION),
        "inline envs": _mask(set_bits=L.LAUNCH_INLINE_ENVS),
        "mirror f32": _mask(set_bits=L.LAUNCH_MIRROR_F32),
        "diagnostic bit 1": _mask(set_bits=1), "diagnostic bit 2": _mask(set_bits=2), "diagnostic bit 4": _mask(set_bits=4),
        "generic forced": _mask(set_bits=L.LAUNCH_GENERIC),
        "aer_out": _set("p", aer_out=PTR), "obs_mirror": _set("p", obs_mirror=PTR),
        "spos_tiles": _set("p", spos_tiles=PTR), "spos_tiles_prev": _set("p", spos_tiles_prev=PTR),
        "update_interval": _set("c", update_interval=2), "resample": _set("c", flags=L.FLAG_RESAMPLE),
        "resample with the reference covariance": _set("c", flags=L.FLAG_RESAMPLE | L.FLAG_REFERENCE_COV),
        "xyz measurements": _set("c", obs_type=L.OBS_XYZ),
    }
    for what, spoil in flips.items():
        b = bench_form()
        spoil(b)
        assert ask(b) == 0, what
    # conditions SSA_LAUNCH_STATS_FROM_METRICS (or the action rule) demands itself: broken alone the launcher refuses the block and the
    # query says so with the same code; the nearest block the launcher accepts is generic
    alone = {
        "two envs": (_set("p", n_env=2), _mask(clear_bits=L.LAUNCH_STATS_FROM_METRICS)),
        "several tiles per wavefront": (_set("p", n_obj=40000), _mask(clear_bits=L.LAUNCH_STATS_FROM_METRICS)),
        "no deferred fold": (_mask(clear_bits=L.LAUNCH_DEFER_FOLD), _mask(clear_bits=both)),
        "fold inside": (_mask(set_bits=L.LAUNCH_FOLD_INSIDE), _mask(set_bits=L.LAUNCH_FOLD_INSIDE, clear_bits=both)),
        "stat_shards_clear": (_set("p", stat_shards_clear=PTR), _mask(clear_bits=L.LAUNCH_STATS_FROM_METRICS)),
        "no action word": (_set("p", actions=0), _mask(set_bits=L.LAUNCH_INLINE_ACTION)),
    }
    for what, (spoil, mend) in alone.items():
        b = bench_form()
        spoil(b)
        rc = ask(b)
        assert rc < 0 and rc == launch_code(b), (what, rc)
        mend(b)
        assert ask(b) == 0, what


def test_a_refused_block_gets_the_launchers_code(pkg):
    from ssa_gym_amd import _lib
    L = _lib
    cases = [_set("p", n_obj=0), _set("p", n_env=0), _set("p", P_in=0), _set("p", stat_ws=0), _set("p", aer_cols=3), _set("c", obs_type=7),
             _set("c", propagator=9), _set("c", propagator=L.PROP_J2_RK4, rk4_substeps=0), _set("p", fail_cap=0),
             _set("p", stat_shards=0), _set("p", stats_prev=0), _set("p", stat_shards_prev=PTR), _set("p", metrics_prev=0),
             _set("p", n_obj=1 << 31), _set("p", stat_shards=0, launch_mask=L.LAUNCH_MIRROR_F32, obj_ids=0)]
    seen = set()
    for spoil in cases:
        b = bench_form()
        spoil(b)
        rc = ask(b)      # (first: only a block the query calls refused is handed to the launcher)
        assert rc in (L.E_INVALID, L.E_UNSUPPORTED) and launch_code(b) == rc, rc
        seen.add(rc)
    assert seen == {L.E_INVALID, L.E_UNSUPPORTED}
    lib = L.load()
    b = bench_form()
    assert lib.ssa_env_step_instance(None, C.byref(b["p"])) == L.E_INVALID and lib.ssa_env_step_instance(C.byref(b["c"]), None) == L.E_INVALID


def test_the_engines_switch_sets_the_bit(pkg):
    """HotPathEngine.force_generic is off by default and is what puts SSA_LAUNCH_GENERIC into launch_step's mask (source-level: an engine
    needs a GPU)"""
    import inspect
    from ssa_gym_amd import _lib, engine
    src = inspect.getsource(engine.HotPathEngine)
    assert "self.force_generic = False" in src and "if self.force_generic:\n            inline |= _lib.LAUNCH_GENERIC" in src
    assert _lib.LAUNCH_GENERIC == 512 and _lib.ABI_VERSION == 23
