"""CPU-only checks of the dry run of candidate schedules in every env of a vector env (include/ssa_hip.h: ssa_dryrun_gather_f64;
device.dryrun_gather_rows; HotPathEngine.launch_dryrun_sensors_envs; SSA_Tasker_VecEnv.evaluate_schedules; agents.refine_plan_sensors
on a vector env): the export, the parameter block's layout against the header, every refusal before any launch, the gather's row rule
on hand-made ids, the env's and the planner's guards without device state, the vector planner on a stubbed evaluator, and the new
kernel's resources in the shipped code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from support.codeobj import _kernels, family, header
from support.dryrun import StubEnv
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.vector_dryrun import ALIGNED16, ENTRY, PTR_FIELDS, StubVecEnv, gather_refused
from support.vector_forecast import bare_vec


def test_the_entry_is_exported_declared_and_bound(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint %s\s*\(" % ENTRY, hdr) and re.search(r"\}\s*ssa_dryrun_gather_params\s*;", hdr)
    assert ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    res, args = _lib.SIGNATURES[ENTRY]
    assert res is C.c_int and len(args) == 2 and args[0] is C.POINTER(_lib.ssa_dryrun_gather_params)
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)
    assert re.search(r"#define\s+SSA_ABI_VERSION\s+23\b", hdr)
    assert [f for f, _ in _lib.ssa_dryrun_gather_params._fields_][5:] == list(PTR_FIELDS)


def test_params_layout_matches_the_header(tmp_path):
    from ssa_gym_amd import _lib
    st = _lib.ssa_dryrun_gather_params
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(ssa_dryrun_gather_params));']
    want = [C.sizeof(st)]
    for f, _ in st._fields_:
        src.append('printf("%%zu\\n", offsetof(ssa_dryrun_gather_params, %s));' % f)
        want.append(getattr(st, f).offset)
    src.append('return 0;}')
    c = tmp_path / "gather.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "gather"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want
    assert want[0] == 24 + 8 * len(PTR_FIELDS)


def test_gather_refuses_bad_arguments_before_any_launch(lib):
    """every refusal the header lists, each from an otherwise complete block; nothing is launched (no device is touched: this runs
    without a GPU)"""
    from ssa_gym_amd import _lib
    fn = getattr(lib, ENTRY)
    assert fn(None, None) == _lib.E_INVALID
    for name in PTR_FIELDS:
        if name != "slot_of":
            assert gather_refused(fn, **{name: 0}) == _lib.E_INVALID, name
    for name in ("n_obj", "n_env", "n_cand", "n_rows"):
        for v in (0, -1, -4):
            assert gather_refused(fn, **{name: v}) == _lib.E_INVALID, (name, v)
    for W in (1, 2, 3, 5, 6, 7, 9, 4098):
        assert gather_refused(fn, n_rows=W) == _lib.E_INVALID, W
    for v in (1, -1, 1 << 20):
        assert gather_refused(fn, reserved=v) == _lib.E_INVALID, v
    # the rows are 32-bit counts: E * B * W and E * m below 2^31
    assert gather_refused(fn, n_env=1 << 10, n_cand=1 << 10, n_rows=1 << 11) == _lib.E_INVALID
    assert gather_refused(fn, n_env=(1 << 10) - 1, n_cand=1 << 10, n_rows=1 << 11, x_in=0) == _lib.E_INVALID   # (in range: refused for the NULL)
    assert gather_refused(fn, n_env=2, n_obj=1 << 30) == _lib.E_INVALID
    assert gather_refused(fn, n_env=1, n_obj=1 << 31) == _lib.E_INVALID
    assert gather_refused(fn, n_env=3, n_obj=1 << 62) == _lib.E_INVALID
    assert gather_refused(fn, n_env=1 << 30, n_cand=1 << 30, n_rows=1 << 30) == _lib.E_INVALID
    # the six double pointers move 16-byte pieces
    for name in ALIGNED16:
        for off in (8, 4, 24):
            assert gather_refused(fn, **{name: 0x10000 + off}) == _lib.E_INVALID, (name, off)


def test_row_rule_on_hand_made_ids():
    """device.dryrun_gather_rows: the statement of the kernel's contract"""
    from ssa_gym_amd import device
    m = 10
    # E = 1, B = 3, W = 4, no table: padding rows take the candidate's first object; an all-idle candidate object 0
    ids = np.array([[3, 7, -1, -1], [-1, -1, -1, -1], [2, 4, 6, 9]], dtype=np.int32)
    rows = device.dryrun_gather_rows(ids, 1, 3, m)
    assert rows.dtype == np.int64 and rows.tolist() == [3, 7, 3, 3, 0, 0, 0, 0, 2, 4, 6, 9]
    # an id >= m (and any other negative one) is a padding row; a first id >= m is clamped below m
    ids = np.array([[5, 10, 99, -7], [12, 1, -1, 10]], dtype=np.int32)
    assert device.dryrun_gather_rows(ids, 1, 2, m).tolist() == [5, 5, 5, 5, 9, 1, 9, 9]
    # two envs, B = 2: env e's rows start at e * m; each env through its own permutation of its rows
    ids = np.array([[0, 9, -1, -1], [4, -1, -1, -1], [0, 9, -1, -1], [-1, -1, -1, -1]], dtype=np.int32)
    assert device.dryrun_gather_rows(ids, 2, 2, m).tolist() == [0, 9, 0, 0, 4, 4, 4, 4, 10, 19, 10, 10, 10, 10, 10, 10]
    perm = [np.random.RandomState(e).permutation(m) for e in range(2)]
    slot_of = np.concatenate([perm[0], perm[1] + m]).astype(np.int32)
    got = device.dryrun_gather_rows(ids, 2, 2, m, slot_of=slot_of)
    want = [perm[0][j] for j in (0, 9, 0, 0, 4, 4, 4, 4)] + [m + perm[1][j] for j in (0, 9, 0, 0, 0, 0, 0, 0)]
    assert got.tolist() == want and not np.array_equal(perm[0], perm[1])
    assert device.dryrun_gather_rows(ids.reshape(-1), 2, 2, m, slot_of=slot_of).tolist() == want       # (flat ids: the same)
    # the ids dryrun_rows leaves, straight in
    cand = np.array([[[7, 3], [3, 7]], [[-1, -4], [10, 999]]])
    ids, _ = device.dryrun_rows(cand, m)
    assert device.dryrun_gather_rows(ids, 2, 1, m).tolist() == [3, 7, 3, 3, 10, 10, 10, 10]
    for bad in (dict(ids=ids.astype(float)), dict(n_env=0), dict(n_env=3), dict(n_obj=0), dict(slot_of=slot_of[:5])):
        kw = dict(dict(ids=ids, n_env=2, n_cand=1, n_obj=m), **bad)
        with pytest.raises(ValueError):
            device.dryrun_gather_rows(**kw)


def test_vector_env_and_planner_guards_without_device_state():
    from ssa_gym_amd import _lib, agents
    for S in (1, 3):
        vec = bare_vec(S)                          # E = 3, m = 8, n = 12
        for sched in (np.zeros((3, 2, S), dtype=np.int64), np.zeros((3, 4, 2, S), dtype=np.int64), np.zeros((5,), dtype=float)):
            with pytest.raises(_lib.SsaHipError, match="no device state"):      # (checked first, whatever the schedule)
                vec.evaluate_schedules(sched)
        with pytest.raises(_lib.SsaHipError, match="no device state"):
            agents.refine_plan_sensors(vec, np.zeros((3, 2, S), dtype=np.int64))
        # shape and dtype: refused before anything of the engine is read (an object() has nothing to read)
        vec._eng = object()
        for bad in (np.zeros((2, S), dtype=np.int64), np.zeros((2, 2, S), dtype=np.int64), np.zeros((3, 2, S + 1), dtype=np.int64),
                    np.zeros((3, 2, S), dtype=np.float64), np.zeros((3, 0, 2, S), dtype=np.int64), np.zeros((3, 1, 1, 2, S), dtype=np.int64),
                    np.zeros((3, 2, 0, S), dtype=np.int64)):
            with pytest.raises(ValueError):
                vec.evaluate_schedules(bad)
        vec.i[1] = vec.n - 1                       # (an env on its last index: K' < 1)
        with pytest.raises(ValueError, match="at least one step"):
            vec.evaluate_schedules(np.zeros((3, 2, S), dtype=np.int64))
        with pytest.raises(ValueError, match="at least one step"):
            agents.refine_plan_sensors(vec, np.zeros((3, 2, S), dtype=np.int64))
        vec.i[1] = 0
        for bad in (np.zeros((2, S), dtype=np.int64), np.zeros((2, 2, S), dtype=np.int64), np.zeros((3, 2, S + 1), dtype=np.int64)):
            with pytest.raises(ValueError, match="a plan"):
                agents.refine_plan_sensors(vec, bad)
        with pytest.raises(ValueError, match="kind"):
            agents.refine_plan_sensors(vec, np.zeros((3, 2, S), dtype=np.int64), kind="gain")
    eng_cls = __import__("ssa_gym_amd.engine", fromlist=["HotPathEngine"]).HotPathEngine
    eng = eng_cls.__new__(eng_cls)
    eng.E, eng.m = 3, 8
    sp = type("Sites", (), {"n_sensor": 2})()
    for bad in (np.zeros((2, 2, 2), dtype=np.int64), np.zeros((2, 1, 2, 2), dtype=np.int64), np.zeros((3, 1, 2, 3), dtype=np.int64),
                np.zeros((3, 1, 2, 2), dtype=float)):
        with pytest.raises(ValueError):            # (before anything else of the engine is read)
            eng.launch_dryrun_sensors_envs(0, 1, sp, bad)
    with pytest.raises(_lib.SsaHipError, match="one env"):                 # (the single-env launch still refuses several envs)
        eng.launch_dryrun_sensors(0, 1, None, np.zeros((1, 2, 2), dtype=np.int64))


def test_vector_refine_on_a_stub():
    """one forecast, one evaluation per round for all envs; candidate 0 is each env's incumbent; a redrawn slot never repeats an object
    of its row; env e's draws are RandomState(seed + e)'s in the single env's order -- its plan equals the single stub's with seed + e;
    the global numpy generator is not drawn from"""
    from ssa_gym_amd import _lib, agents
    E = 3
    plan = np.stack([np.array([[0, 1], [1, 0], [2, 3]]) + e for e in range(E)])
    state = np.random.get_state()[1].copy()
    vec = StubVecEnv(E)
    out, total = agents.refine_plan_sensors(vec, plan, kind='info', rounds=3, candidates=8, seed=4)
    assert np.array_equal(np.random.get_state()[1], state)
    assert vec.forecasts == 1 and len(vec.calls) == 3
    assert out.shape == (E, 3, 2) and out.dtype == np.int64 and total.shape == (E, 3) and total.dtype == np.float64
    inc = plan
    for cand in vec.calls:
        assert cand.shape == (E, 8, 3, 2) and np.array_equal(cand[:, 0], inc)
        nxt = []
        for e in range(E):
            assert all(len(set(r.tolist())) == 2 for c in cand[e] for r in c)
            assert all((c != inc[e]).sum() <= 1 for c in cand[e])
            nxt.append(cand[e][int(np.argmax(cand[e].reshape(8, -1).sum(axis=1)))])      # (the first of equal maxima)
        inc = np.stack(nxt)
    assert np.array_equal(out, inc)
    assert np.array_equal(total[:, _lib.LOOK_INFO_GAIN], out.reshape(E, -1).sum(axis=1)) and (out.reshape(E, -1).sum(axis=1) >= plan.reshape(E, -1).sum(axis=1)).all()
    again, total2 = agents.refine_plan_sensors(StubVecEnv(E), plan, rounds=3, candidates=8, seed=4)
    assert np.array_equal(again, out) and np.array_equal(total2, total)
    for e in range(E):
        one, tot = agents.refine_plan_sensors(StubEnv(), plan[e], rounds=3, candidates=8, seed=4 + e)
        assert np.array_equal(one, out[e]) and np.array_equal(tot, total[e]), e
    assert len({out[e].tobytes() for e in range(E)}) > 1
    # candidates = 1: the incumbents alone -- no forecast, no draw, one evaluation, the plans unchanged
    vec = StubVecEnv(E)
    same, tot = agents.refine_plan_sensors(vec, plan, rounds=3, candidates=1)
    assert np.array_equal(same, plan) and same is not plan and vec.forecasts == 0 and len(vec.calls) == 1
    assert np.array_equal(vec.calls[0][:, 0], plan) and np.array_equal(tot[:, 2], plan.reshape(E, -1).sum(axis=1))
    # K' is one horizon for all envs: the env nearest its end decides
    vec = StubVecEnv(E)
    vec.i[2] = vec.n - 3
    cut, _ = agents.refine_plan_sensors(vec, plan, rounds=1, candidates=4, seed=1)
    assert cut.shape == (E, 2, 2) and vec.calls[0].shape == (E, 4, 2, 2)
    # a NaN total never wins
    class NanFirst(StubVecEnv):
        def evaluate_schedules(self, actions):
            r = StubVecEnv.evaluate_schedules(self, actions)
            r["total"][:, 1:, :] = float("nan")
            return r
    kept, _ = agents.refine_plan_sensors(NanFirst(E), plan, rounds=2, candidates=6, seed=3)
    assert np.array_equal(kept, plan)


def test_the_gather_kernel_in_the_code_object(tmp_path):
    """exactly one dryrun_gather_kernel: no LDS, no scratch, no spills, no atomics, 16-byte loads and stores; and still exactly
    four dryrun_sensors_kernel instances"""
    kern, ins_of = _kernels(tmp_path)
    names = family(kern, "dryrun_gather_kernel")
    assert len(names) == 1, names
    k, ins = kern[names[0]], ins_of[names[0]]
    assert k["group_segment_fixed_size"] == 0 and k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert not [op for op in ins if op.startswith(("scratch_", "ds_", "buffer_atomic", "global_atomic", "flat_atomic"))]
    assert "global_load_dwordx4" in ins and "global_store_dwordx4" in ins
    assert len(family(kern, "dryrun_sensors_kernel")) == 4
