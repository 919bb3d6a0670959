"""The refusals of the controllers' entry points (mrca_render ... mrca_subgoals) as a list of cases: what
tools/make_golden_refusals.py records into tests/golden/abi_refusals.json and tests/test_abi_refusals_host.py replays.

Every parameter and pointer check of these calls runs before `env` is looked at, so with env = NULL and host addresses where the
device buffers would stand no call gets as far as a launch: a case is a key and a function of the loaded library that returns
[return code, mrca_last_error()].  mrca_hybrid_commit takes no env; its cases keep actions_dev (its last check) NULL, so that a
call whose subject is accepted is still refused -- by that pointer.  The one call of it that passes every check is not in the
list: the test makes it by hand."""
import ctypes as C
import struct

import numpy as np

from mrca import _lib

F32 = np.float32
_buf = np.zeros(64 + 4, F32)
BUF = (_buf.ctypes.data + 15) & ~15           # a 16-byte aligned host address with 256 bytes behind it


def _around(b):
    return [float(np.nextafter(F32(b), F32(-np.inf))), float(b), float(np.nextafter(F32(b), F32(np.inf)))]


# every float field sees every bound any of the tables names (-1, 0, 1, 6) and its two neighbours
FLOATS = [float("nan"), float("inf"), float("-inf"), 7.0] + [v for b in (-1.0, 0.0, 1.0, 6.0) for v in _around(b)]
INT_MAX = {"max_neighbors": 48, "steps": 64, "nv": 16, "nw": 64, "stride": 8, "inflate": 64, "lookahead": 256,
           "max_rounds": 2 ** 31 - 1, "G": 4096, "n_robots": 2 ** 31 - 1, "num_views": 256, "width": 4096, "height": 4096}
STRUCTS = {"orca": _lib.OrcaParamsStruct, "dwa": _lib.DwaParamsStruct, "scan_noise": _lib.ScanNoiseParamsStruct,
           "hybrid": _lib.HybridParamsStruct, "safe_policy": _lib.SafePolicyParamsStruct, "planner": _lib.PlannerParamsStruct}

# a call's arguments in order: ("env",) | ("params", argument name, struct) | ("ptr", name, must it be given?) | ("int", name, a
# good value) | ("stream",).  "must it be given" only chooses the pairs of faults below; every pointer gets every fault.
ENV, STREAM, MASK = ("env",), ("stream",), ("ptr", "mask_dev", False)
_ORCA = [ENV, ("params", "params", "orca"), MASK, ("ptr", "actions_dev", True), ("ptr", "vel_dev", False), STREAM]
_PLAN = ("params", "params", "planner")
CALLS = {
    "mrca_orca_actions": _ORCA,
    "mrca_orca_actions_any": _ORCA,
    "mrca_dwa_actions": [ENV, ("params", "params", "dwa"), MASK, ("ptr", "actions_dev", True), ("ptr", "choice_dev", False),
                         ("ptr", "score_dev", False), STREAM],
    "mrca_scan_noise": [ENV, ("params", "params", "scan_noise"), MASK, STREAM],
    "mrca_hybrid_actions": [ENV, ("params", "params", "hybrid"), MASK, ("ptr", "policy_dev", True), ("ptr", "actions_dev", True),
                            ("ptr", "mode_dev", False), ("ptr", "clear_dev", False), STREAM],
    "mrca_hybrid_plan": [ENV, ("params", "hybrid_params", "hybrid"), ("params", "safe_params", "safe_policy"), MASK,
                         ("ptr", "mode_dev", True), ("ptr", "scale_dev", True), ("ptr", "pid_dev", True), ("ptr", "clear_dev", False),
                         STREAM],
    "mrca_hybrid_commit": [("int", "n_robots", 4), ("params", "safe_params", "safe_policy"), MASK, ("ptr", "mode_dev", True),
                           ("ptr", "pid_dev", True), ("ptr", "policy_dev", True), ("ptr", "actions_dev", True), STREAM],
    "mrca_planner_grid": [ENV, _PLAN, ("ptr", "pw_out", True), ("ptr", "ph_out", True)],
    "mrca_goal_fields": [ENV, _PLAN, ("ptr", "goals_dev", True), ("int", "G", 4), ("ptr", "field_dev", True),
                         ("ptr", "rounds_out", False), STREAM],
    "mrca_subgoals": [ENV, _PLAN, ("ptr", "field_dev", True), ("ptr", "goals_dev", True), ("int", "G", 4), ("ptr", "slot_dev", False),
                      MASK, ("ptr", "local_dev", True), ("ptr", "subgoal_dev", False), ("ptr", "dist_dev", False),
                      ("ptr", "status_dev", False), STREAM],
    "mrca_render": [ENV, ("views",), ("int", "num_views", 1), ("int", "width", 8), ("int", "height", 8), ("int", "layers", 7),
                    ("ptr", "ids_dev", True), ("ptr", "trail_dev", False), ("ptr", "rgb_dev", False), STREAM],
}
# what a call is given where a case says nothing else
KEPT_NULL = {"mrca_hybrid_commit": {"actions_dev": None}}


def defaults_of(lib, kind):
    st = STRUCTS[kind]()
    assert getattr(lib, f"mrca_{kind}_default_params")(C.byref(st)) == 0
    return st


def _views(entries):
    return (_lib.RenderView * len(entries))(*[_lib.RenderView(*e) for e in entries])


def invoke(lib, fn, over):
    """`fn` with its good arguments, except for `over`: {argument name: value} -- a pointer's address or None, an integer, a
    {field: value} on top of the library's defaults for a params struct, a list of (world, cx, cy, m_per_px) for the views."""
    over = dict(KEPT_NULL.get(fn, {}), **over)
    args, keep = [], []
    for a in CALLS[fn]:
        if a[0] in ("env", "stream"):
            args.append(None)
        elif a[0] == "params":
            st = None
            if a[1] in over:
                st = defaults_of(lib, a[2])
                for k, v in over[a[1]].items():
                    setattr(st, k, v)
                keep.append(st)
            args.append(None if st is None else C.byref(st))
        elif a[0] == "views":
            v = over.get("views", [(0, 0.0, 0.0, 0.1)] * max(1, min(257, over.get("num_views", 1))))
            keep.append(v if v is None else _views(v))
            args.append(keep[-1])
        elif a[0] == "ptr":
            p = over.get(a[1], BUF)
            if a[1] in ("pw_out", "ph_out", "rounds_out"):
                p = None if p is None else C.cast(C.c_void_p(p), C.POINTER(C.c_int32))
            args.append(p)
        else:
            args.append(over.get(a[1], a[2]))
    rc = getattr(lib, fn)(*args)
    return [rc, lib.mrca_last_error().decode()]


def _fkey(v):
    return f"{v!r}/{struct.pack('<f', v).hex()}"


def _ints(name):
    m = INT_MAX[name]
    return [-1, 0, 1, m] + ([m + 1] if m + 1 < 2 ** 31 else [])


def cases():
    """{key: function of the library -> [rc, message] or another JSON value}"""
    out = {}

    def add(fn, what, over):
        key = f"{fn}|{what}"
        assert key not in out, key
        out[key] = lambda lib, fn=fn, over=over: invoke(lib, fn, over)

    for kind, st in STRUCTS.items():
        name = f"mrca_{kind}_default_params"
        out[f"{name}|bytes"] = lambda lib, kind=kind: bytes(defaults_of(lib, kind)).hex()
        out[f"{name}|out=NULL"] = lambda lib, name=name: [getattr(lib, name)(None), lib.mrca_last_error().decode()]
    for fn, spec in CALLS.items():
        add(fn, "good", {})
        ptrs = [a[1] for a in spec if a[0] == "ptr"]
        needed = [a[1] for a in spec if a[0] == "ptr" and a[2]]
        first_bad = None            # the first parameter, refused
        for a in spec:
            if a[0] == "params":
                for k, t in STRUCTS[a[2]]._fields_:
                    for v in (FLOATS if t is C.c_float else _ints(k)):
                        add(fn, f"{a[1]}.{k}={_fkey(v) if t is C.c_float else v}", {a[1]: {k: v}})
                first_field = STRUCTS[a[2]]._fields_[0]
                first_bad = first_bad or {a[1]: {first_field[0]: float("nan") if first_field[1] is C.c_float else -1}}
                add(fn, f"{a[1]}=defaults", {a[1]: {}})
                if a[2] == "hybrid":        # the rule across two fields: stop_dist >= risk_dist, on either side of equal
                    for stop, risk in [(0.5, 0.5), (float(np.nextafter(F32(0.5), F32(0))), 0.5), (0.7, 0.6), (0.0, 0.0), (6.5, 6.5),
                                       (6.0, 6.0), (-1.0, -1.0), (5.0, 6.5)]:
                        add(fn, f"{a[1]}.stop_dist={stop!r},risk_dist={risk!r}", {a[1]: {"stop_dist": stop, "risk_dist": risk}})
            elif a[0] == "int" and a[1] != "layers":
                for v in _ints(a[1]):
                    add(fn, f"{a[1]}={v}", {a[1]: v})
                first_bad = first_bad or {a[1]: 0}
            elif a[0] == "ptr":
                add(fn, f"{a[1]}=NULL", {a[1]: None})
                for off in (1, 2, 4):
                    add(fn, f"{a[1]}+{off}", {a[1]: BUF + off})
        # pairs of faults: which of the two is reported pins the order of the checks
        if needed:
            add(fn, f"first parameter bad, {needed[-1]}=NULL", dict(first_bad, **{needed[-1]: None}))
            later = [p for p in ptrs[ptrs.index(needed[0]) + 1:] if p != "mask_dev"]
            for p in later:
                add(fn, f"{needed[0]}=NULL, {p}+1", {needed[0]: None, p: BUF + 1})
        if fn == "mrca_hybrid_plan":
            add(fn, "both params bad", {"hybrid_params": {"max_speed": 2.0}, "safe_params": {"scan_scale": float("nan")}})
            add(fn, "safe_params bad, mode_dev=NULL", {"safe_params": {"v_cap": 0.0}, "mode_dev": None})
        if fn == "mrca_hybrid_commit":
            add(fn, "n_robots=0, safe_params.v_cap=nan", {"n_robots": 0, "safe_params": {"v_cap": float("nan")}})
            add(fn, "n_robots=0, mode_dev=NULL", {"n_robots": 0, "mode_dev": None})
        if fn == "mrca_planner_grid":
            add(fn, "pw_out=NULL, ph_out=NULL", {"pw_out": None, "ph_out": None})
        if fn in ("mrca_goal_fields", "mrca_subgoals"):
            add(fn, "G=0, params.stride=0", {"G": 0, "params": {"stride": 0}})
            add(fn, "G=0, goals_dev=NULL, field_dev=NULL", {"G": 0, "goals_dev": None, "field_dev": None})
            add(fn, "goals_dev=NULL, field_dev=NULL", {"goals_dev": None, "field_dev": None})
    fn = "mrca_render"
    add(fn, "views=NULL", {"views": None})
    add(fn, "views=NULL, num_views=0", {"views": None, "num_views": 0})
    add(fn, "width=0, height=0", {"width": 0, "height": 0})
    add(fn, "width=4097, layers=16", {"width": 4097, "layers": 16})
    for v in (0, 1, 2, 4, 8, 15, 16, 31, 0x80000000, 0x80000007, 0xFFFFFFFF):
        add(fn, f"layers={v:#x}", {"layers": v})
    add(fn, "layers=0x10, ids_dev=NULL", {"layers": 16, "ids_dev": None})
    add(fn, "trail_dev+1, rgb_dev+2", {"trail_dev": BUF + 1, "rgb_dev": BUF + 2})
    add(fn, "ids_dev+2, view 0 m_per_px=0", {"ids_dev": BUF + 2, "views": [(0, 0.0, 0.0, 0.0)]})
    for k, field in enumerate(("cx", "cy", "m_per_px")):
        for v in [float("nan"), float("inf"), float("-inf"), -1.0, 7.0] + _around(0.0):
            view = [0, 0.0, 0.0, 0.1]
            view[1 + k] = v
            add(fn, f"view 0 {field}={_fkey(v)}", {"views": [tuple(view)]})
    for w in (-1, 0, 1, 2 ** 31 - 1):        # (the world index is judged behind the env)
        add(fn, f"view 0 world={w}", {"views": [(w, 0.0, 0.0, 0.1)]})
    add(fn, "view 1 of 2 m_per_px=nan", {"num_views": 2, "views": [(0, 0.0, 0.0, 0.1), (0, 0.0, 0.0, float("nan"))]})
    add(fn, "views 1 and 2 of 3 bad", {"num_views": 3, "views": [(0, 0.0, 0.0, 0.1), (0, float("inf"), 0.0, 0.1), (0, 0.0, 0.0, -1.0)]})
    add(fn, "view 255 of 256 cy=inf", {"num_views": 256, "views": [(0, 0.0, 0.0, 0.1)] * 255 + [(0, 0.0, float("inf"), 0.1)]})
    return out


def record(lib):
    return {k: f(lib) for k, f in cases().items()}
