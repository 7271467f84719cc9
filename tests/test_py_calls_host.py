"""``_lib``'s restatement of every public header of ``_lib.HEADERS`` pinned to the header, prototype by prototype,
structure by structure and enum by enum; and the contract of ``_lib.call``, the one way the package's wrappers enter the
library.  No device."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import scanlib_header as H
from pyracecarsimulator_amd import _lib
from pyracecarsimulator_amd import racecar as RC

PKG = os.path.dirname(os.path.abspath(_lib.__file__))
EDGE_ARGS = (16, -2.355, 0.29, 0.275, 0.2032, 0.3302)        # rl_car_edge_distances without its output


# ---------------------------------------------------------------- the tables against the headers
HEADERS = [H.Header(entry) for entry in _lib.HEADERS]
SCANLIB = HEADERS[0]
PROTOTYPES = {h.entry.file: h.prototypes() for h in HEADERS}


per_header = pytest.mark.parametrize("header", HEADERS, ids=[h.entry.file for h in HEADERS])


def test_the_registry_is_the_headers_of_include():
    assert sorted(e.file for e in _lib.HEADERS) == sorted(f for f in os.listdir(H.INCLUDE) if f.endswith(".h"))
    assert [len(e.symbols) for e in _lib.HEADERS] == [105, 4, 4, 9, 3, 7, 3]
    tables = [getattr(_lib, t) for t in ("SYMBOLS", "EXT_SYMBOLS", "SEAT_SYMBOLS", "POP_SYMBOLS", "LEAGUE_SYMBOLS",
                                         "LEAGUE_ENV_SYMBOLS", "TRACK_DRIVE_SYMBOLS")]
    assert all(e.symbols is t for e, t in zip(_lib.HEADERS, tables)) and len(_lib.HEADERS) == len(tables)
    assert _lib.HEADERS[0].file == "scanlib.h" and not _lib.HEADERS[0].handles
    # two headers that declare one name do not load
    twice = _lib.Header("scanlib_extra.h", {"rl_env_step": _lib.SYMBOLS["rl_env_step"]}, {}, ())
    with pytest.raises(ValueError, match="scanlib_extra.h declares rl_env_step again"):
        _lib._merge(_lib.HEADERS + (twice,))
    assert _lib._merge(_lib.HEADERS) == _lib._DECLARED and len(_lib._DECLARED) == 135
    with pytest.raises(KeyError):
        _lib.declared("rl_no_such_symbol")
    # what build() watches: every unit and kernel header of csrc, and every file of include/
    watched, csrc = {os.path.normpath(f) for f in _lib.build_sources()}, os.path.join(PKG, "csrc")
    assert {os.path.join(H.INCLUDE, f) for f in os.listdir(H.INCLUDE)} <= watched
    assert {os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))} <= watched


@per_header
def test_the_header_and_the_table_name_the_same_symbols(header):
    protos, table = PROTOTYPES[header.entry.file], header.entry.symbols
    assert set(protos) == set(table), set(protos) ^ set(table)
    assert set(re.findall(r"\b(rl_[a-z_0-9]+)\s*\(", header.text())) == set(table)


@pytest.mark.parametrize("name", [pytest.param((h, n), id=n) for h in HEADERS for n in sorted(h.entry.symbols)])
def test_prototype_matches_the_table(name):
    header, name = name
    res, args, names = PROTOTYPES[header.entry.file][name]
    bound_res, bound_args = header.entry.symbols[name]
    assert bound_res is res, (name, bound_res, res)
    assert len(bound_args) == len(args), (name, names)
    for i, (got, want) in enumerate(zip(bound_args, args)):
        assert got is want, "%s argument %d (%s): the table has %s, the header %s" % (name, i, names[i], got, want)


def test_int_valued_symbols_return_int_and_are_declared():
    protos = PROTOTYPES["scanlib.h"]
    assert _lib.INT_VALUED <= set(protos)
    assert all(protos[n][0] is C.c_int for n in _lib.INT_VALUED)
    # the header's rule, "every function returns RL_OK (0) or a negative rl_status", covers every other int function
    status = [n for n, (res, _, _) in protos.items() if res is C.c_int and n not in _lib.INT_VALUED]
    assert all(_lib.converters(n)[2] for n in status) and not any(_lib.converters(n)[2] for n in _lib.INT_VALUED)
    assert not _lib.converters("rl_version")[2] and not _lib.converters("rl_map_destroy")[2]


@per_header
def test_the_library_exports_the_table_and_the_call_layer_reads_it(header):
    L = _lib.lib()
    for name, (res, args) in header.entry.symbols.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        assert _lib.declared(name) is header.entry.symbols[name], name
        raw, convs, status = _lib.converters(name)
        assert status is (res is C.c_int and name not in _lib.INT_VALUED), name        # (rl_status: call checks it)
        assert len(convs) == len(args), name
    if header is not SCANLIB:
        # a feature header's int is always an rl_status, and its handle types are the registry's
        assert not set(header.entry.symbols) & _lib.INT_VALUED
        assert all(res is C.c_int or (res is None and name.endswith("_destroy"))
                   for name, (res, _) in header.entry.symbols.items())
        assert header.handles() == set(header.entry.handles) and not header.handles() & SCANLIB.handles()


@per_header
def test_a_newer_header_rebuilds_the_unit_that_includes_it(header):
    """make itself: with the header newer than everything (-W), a dry run of the library's rule compiles abi_car."""
    _lib.build()
    out = subprocess.run(["make", "-n", "-W", "../../include/" + header.entry.file, "../libscan_amd.so"],
                         cwd=os.path.join(PKG, "csrc"), check=True, capture_output=True, text=True).stdout
    assert re.search(r"-c -o \.obj/abi_car\.o abi_car\.hip", out), out


@pytest.mark.parametrize("name", [pytest.param((h, n), id=n) for h in HEADERS for n in sorted(h.entry.structs)])
def test_structure_matches_the_header(name):
    header, name = name
    declared = header.structs()[name]
    fields = [(f[0], f[1]) for f in header.entry.structs[name]._fields_]
    assert [n for n, _ in fields] == [n for n, _ in declared]
    for (n, got), (_, want) in zip(fields, declared):
        assert got is want, "%s.%s: the class has %s, the header %s" % (name, n, got, want)


@per_header
def test_every_structure_of_the_header_is_restated(header):
    assert set(header.structs()) == set(header.entry.structs)
    assert all(H.STRUCTS[name] is cls for name, cls in header.entry.structs.items())
    if header is SCANLIB:
        assert len(header.entry.structs) == 7
        assert dict(_lib.RaceEnvParams._fields_)["env"] is _lib.EnvParams
        assert dict(_lib.PfParams._fields_)["motion_std"] is C.c_double * 3
        assert [n for n, _ in _lib.TrackParams._fields_] == ["window", "goal_span", "reward_mode", "lookahead"]
        assert len(_lib.PlanOpts._fields_) == 28


def test_enums_match_the_header():
    E = SCANLIB.enums()
    assert set(E) == {"rl_status", "rl_kind", "rl_mcts_source", "rl_kernel_id", "rl_binning"}
    for enum in ("rl_status", "rl_kind", "rl_mcts_source"):
        for const, value in E[enum].items():
            assert getattr(_lib, const) == value, const
    # the package names no RL_ constant the header does not
    ours = {n for n in vars(_lib) if re.fullmatch(r"RL_[A-Z_0-9]+", n)}
    assert ours == set(E["rl_status"]) | set(E["rl_kind"]) | set(E["rl_mcts_source"])
    # the plan's dictionaries: the same values, and the C name (lower case, without its prefix) is the dictionary's
    # name or abbreviates it (RL_K_RM_STREAM_LIT is "rm_stream_literal")
    for enum, prefix, table in (("rl_kernel_id", "RL_K_", _lib.KERNEL_IDS), ("rl_binning", "RL_BIN_", _lib.BINNINGS)):
        assert sorted(E[enum].values()) == sorted(table)
        assert len(set(table.values())) == len(table)
        for const, value in E[enum].items():
            assert const.startswith(prefix) and table[value].startswith(const[len(prefix):].lower()), const
    assert all(_lib.BINNINGS[v] == c[7:].lower() for c, v in E["rl_binning"].items())


def test_the_parser_refuses_what_it_does_not_know():
    for decl in ("long", "unsigned int", "struct foo *", "float ***", "rl_plan_opts **", "char **"):
        with pytest.raises(H.HeaderError):
            H.ctype(decl, "x", SCANLIB.handles())
    assert H.ctype("const float *", "d_poses") is C.c_void_p and H.ctype("const float *", "poses") is _lib.f32p
    assert H.ctype("rl_map **", "out", {"rl_map"}) == C.POINTER(C.c_void_p) and H.ctype("void ", "") is None


# ---------------------------------------------------------------- the call layer
@pytest.fixture
def entered(monkeypatch):
    """Names of the symbols ``call`` entered the library at, in order."""
    class Names(list):
        pass
    names = Names()

    def watch(name):
        fn, convs, status = _lib.converters(name)
        monkeypatch.setitem(_lib._CALLS, name, (lambda *a: (names.append(name), fn(*a))[1], convs, status))
    names.watch = watch
    return names


@pytest.mark.parametrize("name, args, pos", [
    ("rl_car_is_crashed", (np.ones(16), 16, 1, np.ones(16), 0.1, C.c_int()), 0),                      # f64 for float *
    ("rl_car_is_crashed", (np.ones(16, np.float32), 16, 1, np.ones(16), 0.1, np.zeros(1, np.int64)), 5),   # i64 for int *
    ("rl_car_edge_distances", EDGE_ARGS + (np.empty(16, np.float32),), 6),                            # f32 for double *
    ("rl_car_edge_distances", EDGE_ARGS + (np.empty(32)[::2],), 6),                                   # not contiguous
    ("rl_car_edge_distances", EDGE_ARGS + ([0.0] * 16,), 6),                                          # not an array
    ("rl_car_edge_distances", EDGE_ARGS + (C.c_float(),), 6),                                         # the wrong scalar
    ("rl_plan_default_opts", (_lib.LaunchPlan(),), 0),                                                # the wrong struct
    ("rl_map_rows", (np.zeros(4, np.uint8),), 0),                                                     # array for void *
])
def test_a_wrong_argument_is_a_type_error_before_the_library_is_entered(entered, name, args, pos):
    entered.watch(name)
    with pytest.raises(TypeError, match=r"%s argument %d\b" % (name, pos)):
        _lib.call(name, *args)
    assert entered == []
    with pytest.raises(TypeError, match="takes %d arguments" % len(_lib.SYMBOLS[name][1])):
        _lib.call(name, *args, 0)


def test_converters_by_declared_type():
    conv = lambda name, i: _lib.converters(name)[1][i]
    u16 = conv("rl_method_read_lut", 3)
    with pytest.raises(TypeError, match="rl_method_read_lut argument 3"):
        u16(np.zeros(4, np.uint8))
    a = np.zeros(4, np.uint16)
    assert u16(a) == a.ctypes.data and u16(None) is None
    v = C.c_uint16(3)
    assert u16(v) == C.addressof(v)

    class Thing(_lib.Handle):
        pass
    t = Thing()
    t._h = C.c_void_p(0x1234)
    void = conv("rl_map_rows", 0)
    assert void(t) is t._h and void(t._h) is t._h and void(None) is None and void(0) is None
    assert void(0x1000) == 0x1000 and void(np.int64(0x1000)) == 0x1000
    t._h = None                                        # (nothing to destroy)
    for bad in (np.zeros(1, np.uint8), 1.5, "x"):
        with pytest.raises(TypeError):
            void(bad)
    assert conv("rl_method_set_option", 1)("timing") == b"timing"
    assert conv("rl_method_set_option", 2)(np.int64(3)) == 3 and conv("rl_method_set_option", 2)(True) == 1
    assert type(conv("rl_set_noise", 1)(np.float32(0.5))) is float
    # the pair of rl_policy_create: a sequence of float32 arrays, each checked, as an array of addresses
    Ws = [np.zeros((3, 2), np.float32), np.zeros((2, 1), np.float32)]
    got = conv("rl_policy_create", 3)(Ws)
    assert list(got) == [W.ctypes.data for W in Ws]
    with pytest.raises(TypeError, match="rl_policy_create argument 3"):
        conv("rl_policy_create", 3)([Ws[0], Ws[1].astype(np.float64)])


def test_none_reaches_the_library_as_null_and_a_negative_status_raises_its_message(entered):
    entered.watch("rl_car_edge_distances")
    with pytest.raises(_lib.ScanLibError) as e:
        _lib.call("rl_car_edge_distances", *EDGE_ARGS, None)
    assert entered == ["rl_car_edge_distances"] and e.value.code == _lib.RL_ERR_INVALID
    msg = _lib.call("rl_last_error")
    assert isinstance(msg, bytes) and msg and msg.decode() in str(e.value)
    with pytest.raises(_lib.ScanLibError):
        _lib.call("rl_plan_default_opts", None)


def test_out_parameters_structs_and_numpy_scalars():
    out = np.full(16, np.nan)
    assert _lib.call("rl_car_edge_distances", *EDGE_ARGS, out) is None and np.isfinite(out).all()
    again = np.empty(16)
    _lib.call("rl_car_edge_distances", np.int64(16), *(np.float64(v) for v in EDGE_ARGS[1:]), again)
    assert np.array_equal(out, again) and np.array_equal(out, RC.edge_distances(*EDGE_ARGS))
    # a ctypes scalar comes back filled, and so does a one-element array in its place
    rays = np.full((2, 16), 5.0, np.float32)
    first, arr = C.c_int(7), np.full(1, 7, np.int32)
    _lib.call("rl_car_is_crashed", rays, 16, 2, np.abs(out), 0.001, first)
    _lib.call("rl_car_is_crashed", rays, 16, 2, np.abs(out), 0.001, arr)
    assert first.value == arr[0] == -3 == RC.is_crashed(rays, 16, 2, np.abs(out), 0.001)
    rays[1, 4] = 0.0
    _lib.call("rl_car_is_crashed", rays, np.int32(16), np.int64(2), np.abs(out), np.float32(0.5), first)
    assert first.value == 1
    # structs go by reference, in and out; bools pass for int
    o = _lib.PlanOpts()
    assert _lib.call("rl_plan_default_opts", o) is None and o.wg_threads > 0
    pl = _lib.LaunchPlan()
    _lib.call("rl_plan_fan", _lib.RL_RM_GPU, 256, 512, 512, 300.0, 0, o, 64, 1081, np.bool_(False), True, pl)
    assert pl.as_dict() == _lib.plan_fan(_lib.RL_RM_GPU, 512, 512, 64, 1081, crash=True) and pl.crash == 1 and pl.name


def test_a_value_symbol_returns_its_value():
    L = _lib.lib()
    assert _lib.call("rl_version") == L.rl_version() and b"gfx950" in _lib.call("rl_version")
    assert _lib.call("rl_launch_contexts") == L.rl_launch_contexts() > 0
    assert _lib.call("rl_device_count") == L.rl_device_count() >= 0


def test_lib_and_raw_are_what_they_were():
    raw = _lib.raw("rl_calc_range_fan")                # (lib(): test_the_library_exports_the_table_and_the_call_layer_reads_it)
    assert raw is _lib.raw("rl_calc_range_fan") and raw.restype is C.c_int
    assert tuple(raw.argtypes) == (C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)


# ---------------------------------------------------------------- the wrappers are on the layer
def test_no_wrapper_marshals_by_hand():
    """Outside _lib.py the package builds no ctypes pointer and reaches no entry point of ``lib()``: handles are made
    empty (``C.c_void_p()``) and a replica's from the address the library returned (``_h=C.c_void_p(p)``)."""
    banned = {r"\.ctypes\.data_as\(": "data_as", r"\bbyref\(": "byref", r"\bPOINTER\(": "POINTER",
              r"lib\(\)\s*\.\s*rl_": "lib().rl_", r"(?<!_h=C\.)\bc_void_p\((?!\))": "c_void_p(pointer)",
              r"\bptr\s*=\s*lambda": "ptr lambda", r"\bf(32|64)p\b|\b[iu](8|16|32)p\b": "pointer type"}
    files = sorted(set(glob.glob(os.path.join(PKG, "*.py"))) - {os.path.join(PKG, "_lib.py")})
    assert len(files) >= 15
    found = []
    for path in files:
        for n, line in enumerate(open(path), 1):
            found += ["%s:%d %s" % (os.path.basename(path), n, what) for rx, what in banned.items() if re.search(rx, line)]
    assert not found, found


def test_the_shared_validators_keep_each_caller_s_contract():
    from pyracecarsimulator_amd import range_libc as R
    n = 8
    hits, steps = np.zeros(2 * n + 2, np.int32), np.zeros(n + 1, np.uint16)
    R._check_aux_outs(None, None, n, "P*num_rays")
    R._check_aux_outs(hits, steps, n, "P*num_rays")                       # the fan forms take a larger buffer
    R._check_aux_outs(hits[:2 * n], steps[:n], n, "P*A", exact=True)
    with pytest.raises(ValueError, match=r"hit_cells must be C-contiguous int32 \(P\*A, 2\)"):
        R._check_aux_outs(hits, None, n, "P*A", exact=True)               # ... the repeat-angle form the exact size
    with pytest.raises(ValueError, match=r"steps must be C-contiguous uint16 \(P\*A,\)"):
        R._check_aux_outs(None, steps, n, "P*A", exact=True)
    for bad_hits, bad_steps in ((hits[:2 * n - 1], None), (hits.astype(np.int64), None), (hits[::2], None),
                                (hits.tolist(), None), (None, steps[:n - 1]), (None, steps.astype(np.int16)),
                                (None, np.zeros(2 * n, np.uint16)[::2]), (None, steps.tolist())):
        with pytest.raises(ValueError, match=r"must be C-contiguous (int32 \(N\*num_rays, 2\)|uint16 \(N\*num_rays,\))"):
            R._check_aux_outs(bad_hits, bad_steps, n, "N*num_rays")
    poses, edge = R._prep_crash([[1, 2, 3]] * 4, [0.5] * 6, 6, group=2)
    assert poses.dtype == np.float32 and poses.shape == (4, 3) and edge.dtype == np.float64
    assert poses.flags.c_contiguous and edge.flags.c_contiguous
    with pytest.raises(ValueError, match="multiple of the group size"):
        R._prep_crash(np.zeros((5, 3)), np.zeros(6), 6, group=2)
    with pytest.raises(ValueError, match="edge_distances needs num_rays entries"):
        R._prep_crash(np.zeros((4, 3)), np.zeros(5), 6)
