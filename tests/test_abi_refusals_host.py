"""What the controllers' entry points (mrca_render, mrca_orca_actions ... mrca_subgoals) answer to bad arguments, held to a
record: tests/golden/abi_refusals.json, written by tools/make_golden_refusals.py from the library as it stood BEFORE the
entry points were rewritten on one set of helpers.  Every case of abi_refusal_cases.cases() is replayed: the return code and the
whole text of mrca_last_error() must be the recorded ones -- so must the order of the checks, which the cases with two faults
pin.  No case gets as far as a launch (env is NULL, host addresses stand where device buffers would).

The params classes of the Python side (mrca/orca.py ... mrca/planner.py) are held to literal values checked on the same commit.
Already asserted as strictly elsewhere and not repeated: the noise model's comma string, "default" and "a parameter that is not
named is 0" (test_scan_noise_host.py), PlannerParams.for_grid's stride / inflate / lookahead (test_planner_host.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import abi_refusal_cases as AC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_refusals.json")
f32 = lambda v: float(np.float32(v))


def test_every_refusal_is_the_recorded_one(built_lib):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = AC.record(built_lib)
    assert sorted(got) == sorted(want), (sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5])
    assert len(got) == 1351
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, (len(wrong), list(wrong.items())[:10])
    # the record says what it is meant to: a good call fails on the env alone, a bad one is never MRCA_OK
    assert all(v[0] != 0 for k, v in want.items() if not k.endswith("|bytes"))
    assert all(want[f"{fn}|good"] == [-1, "env is NULL"] for fn in AC.CALLS if fn != "mrca_hybrid_commit")
    assert want["mrca_hybrid_commit|good"] == [-1, "mrca_hybrid_commit: actions_dev is NULL"]


def test_hybrid_commit_with_good_arguments_is_not_refused_before_its_launch(built_lib):
    """(recorded by hand: mrca_hybrid_commit takes no env, so a call that passes every check is launched -- on buffers of the
    device where there is one; without one it ends in the runtime's error, whose text is not ours)"""
    import torch
    if torch.cuda.is_available():
        t = torch.zeros(64, dtype=torch.float32, device="cuda")
        rc = AC.invoke(built_lib, "mrca_hybrid_commit", {k: t.data_ptr() for k in ("mask_dev", "mode_dev", "pid_dev", "policy_dev",
                                                                                   "actions_dev")})[0]
        torch.cuda.synchronize()
        assert rc == 0, built_lib.mrca_last_error()
    else:
        rc, msg = AC.invoke(built_lib, "mrca_hybrid_commit", {"actions_dev": AC.BUF})
        assert rc not in (0, -1) and "mrca_hybrid_commit:" not in msg, (rc, msg)


ORCA = dict(radius=0.35, neighbor_dist=6.0, time_horizon=2.0, time_horizon_obst=1.5, obst_dist=3.0, v_pref=1.0, max_speed=1.0,
            responsibility=0.5, k_omega=6.0, jitter=0.0, max_neighbors=10)
DWA = dict(radius=0.35, horizon=2.0, obst_dist=3.0, clear_cap=1.0, max_speed=1.0, max_omega=1.0, acc_v=10.0, acc_w=20.0, w_goal=1.0,
           w_heading=0.0, w_clear=0.2, w_speed=0.3, steps=10, nv=5, nw=21)
NOISE = dict(sigma_const=0.01, sigma_prop=0.01, dropout=0.005, quantum=0.0)
HYBRID = dict(risk_dist=0.6, stop_dist=0.3, safe_scale=0.75, corridor=1.0, look=6.0, front_cos=0.5, v_pid=1.0, k_omega=6.0, max_speed=1.0)
SAFE = dict(scan_scale=0.3, v_cap=0.75)
PLANNER = dict(stride=2, inflate=7, lookahead=15, max_rounds=0)


def mirrors():
    from mrca import _lib
    from mrca.dwa import DwaParams
    from mrca.hybrid import HybridParams, SafePolicyParams
    from mrca.noise import ScanNoiseParams
    from mrca.orca import OrcaParams
    from mrca.planner import PlannerParams
    # class, its struct, the defaults, its flag, a good list and what it gives, the names its error lists
    return [(OrcaParams, _lib.OrcaParamsStruct, ORCA, "--orca-param", ["radius=0.4", "max_neighbors=12"], dict(radius=0.4, max_neighbors=12)),
            (DwaParams, _lib.DwaParamsStruct, DWA, "--dwa-param", ["horizon=1.5", "nw=31", "steps=7"], dict(horizon=1.5, nw=31, steps=7)),
            (ScanNoiseParams, _lib.ScanNoiseParamsStruct, NOISE, "--lidar-noise", ["prop=0.25", "quantum=0.5"],
             dict(sigma_const=0.0, sigma_prop=0.25, dropout=0.0, quantum=0.5)),
            (HybridParams, _lib.HybridParamsStruct, HYBRID, "--hybrid-param", ["risk_dist=0.8", "look=3"], dict(risk_dist=0.8, look=3.0)),
            (SafePolicyParams, _lib.SafePolicyParamsStruct, SAFE, "--hybrid-safe-param", ["scan_scale=0.7"], dict(scan_scale=0.7)),
            (PlannerParams, _lib.PlannerParamsStruct, PLANNER, "--planner-param", ["stride=1", "lookahead=20"], dict(stride=1, lookahead=20))]


def test_the_python_mirrors_of_the_params(built_lib):
    import dataclasses
    for cls, st_cls, defaults, flag, items, given in mirrors():
        ints = [k for k, t in st_cls._fields_ if t is C.c_int32]
        names = [k for k, _t in st_cls._fields_]
        assert [f.name for f in dataclasses.fields(cls)] == names == list(defaults)
        want = {k: (v if k in ints else f32(v)) for k, v in defaults.items()}
        p = cls()
        assert dataclasses.asdict(p) == want, cls
        assert all(type(getattr(p, k)) is (int if k in ints else float) for k in names), cls
        # struct() round-trips, the library's defaults and other values
        st = p.struct()
        assert type(st) is st_cls and {k: getattr(st, k) for k in names} == want
        q = cls(**{k: (3 if k in ints else 0.625) for k in names})
        assert {k: getattr(q.struct(), k) for k in names} == {k: (3 if k in ints else 0.625) for k in names}
        assert dataclasses.asdict(cls(**{k: getattr(q.struct(), k) for k in names})) == dataclasses.asdict(q)
        # an integer field goes to the library as an int whatever it was given as
        for k in ints:
            r = cls(**{k: np.int64(3)})
            assert getattr(r, k) == 3 and type(getattr(r.struct(), k)) is int, (cls, k)
            assert not hasattr(r, "as_dict") or type(r.as_dict()[k]) is int
            assert type(getattr(r, k)) is int or cls.__name__ == "PlannerParams"     # (which converts in struct() and as_dict())
        # from_assignments: a good list, nothing, and the two mistakes
        got = cls.from_assignments(items)
        base = dict.fromkeys(names, 0.0) if flag == "--lidar-noise" else want
        assert dataclasses.asdict(got) == dict(base, **given), cls
        assert all(type(getattr(got, k)) is int for k in ints)
        assert dataclasses.asdict(cls.from_assignments([])) == dataclasses.asdict(cls.from_assignments(None)) == want
        listed = (["const", "prop"] if flag == "--lidar-noise" else []) + names
        for bad in ("nonsense=1", names[0], "=1"):
            with pytest.raises(ValueError) as e:
                cls.from_assignments(items + [bad])
            assert str(e.value) == f"{flag} {bad!r}: expected name=value with name in {listed}", cls
        with pytest.raises(ValueError):
            cls.from_assignments([f"{names[0]}=x"])


def test_noise_short_names_and_planner_base(built_lib):
    from mrca import scenario as S
    from mrca.noise import ScanNoiseParams
    from mrca.planner import PlannerParams
    assert ScanNoiseParams.from_assignments(["const=0.5", "sigma_prop=0.25"]).as_dict() == dict(sigma_const=0.5, sigma_prop=0.25,
                                                                                                  dropout=0.0, quantum=0.0)
    assert ScanNoiseParams.from_assignments("").as_dict() == ScanNoiseParams().as_dict() == {k: f32(v) for k, v in NOISE.items()}
    assert all(type(v) is float for v in ScanNoiseParams(dropout=1).as_dict().values())
    base = PlannerParams(stride=1, inflate=4, lookahead=9, max_rounds=50)
    assert PlannerParams.from_assignments(["lookahead=20"], base=base).as_dict() == dict(stride=1, inflate=4, lookahead=20, max_rounds=50)
    assert PlannerParams.from_assignments(None, base=base) == base
    assert PlannerParams.from_assignments(["lookahead=20"]).as_dict() == dict(PLANNER, lookahead=20)
    assert all(type(v) is int for v in PlannerParams(stride=np.int32(2)).as_dict().values())
    pg = PlannerParams.for_grid(S.doorway().grid, radius=0.5, lookahead_m=1.0, max_rounds=np.int64(77))
    assert pg.as_dict() == dict(stride=1, inflate=5, lookahead=10, max_rounds=77) and type(pg.max_rounds) is int
    assert PlannerParams.for_grid(S.stage2().grid).as_dict() == dict(stride=2, inflate=7, lookahead=15, max_rounds=0)
