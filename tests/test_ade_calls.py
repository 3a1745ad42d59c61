"""CPU suite of tests/ade_calls.py, the raw-call layer of the fluid + scalar GPU suites: the parameter lists it reads from
include/lbm_hip.h are pinned to the literal table below -- a header edit that reorders, adds or drops a parameter fails here,
not as a mis-placed pointer on the GPU -- and every entry's argument list is built in the prototype's order, checked with a
stub in the library's place that records what it receives."""
import ctypes as ct

import pytest

import ade_calls
import pylbm

PROTOTYPES = {
    "lbm_ade_collide": "fp gp f g_in g bc fluid scalar rho u conc s",
    "lbm_ade_stream_collide": "fn gn fo go g bc fluid scalar row_begin row_end rho u conc s",
    "lbm_ade_stream_collide_part": "fn gn fo go g bc fluid scalar part edge_rows rho u conc s",
    "lbm_ade_stream_collide_ex": "fn gn fo go g bc fluid scalar sbc row_begin row_end rho u conc s",
    "lbm_ade_stream_collide_part_ex": "fn gn fo go g bc fluid scalar sbc part edge_rows rho u conc s",
    "lbm_ade_collide_b": "fp gp f g_in g bc fluid scalar sbc buoy rho u conc s",
    "lbm_ade_stream_collide_b": "fn gn fo go g bc fluid scalar sbc buoy row_begin row_end rho u conc s",
    "lbm_ade_stream_collide_part_b": "fn gn fo go g bc fluid scalar sbc buoy part edge_rows rho u conc s",
    "lbm_ade_stream_collide_w": "fn gn fo go g bc fluid scalar sbc buoy iwalls row_begin row_end rho u conc s",
    "lbm_ade_stream_collide_part_w": "fn gn fo go g bc fluid scalar sbc buoy iwalls part edge_rows rho u conc s",
    "lbm_ade_collide_m": "fp gp f g_in g bc fluid scalar sbc rho u conc s",
    "lbm_ade_stream_collide_m": "fn gn fo go g bc fluid scalar sbc iwalls row_begin row_end rho u conc s",
    "lbm_ade_stream_collide_part_m": "fn gn fo go g bc fluid scalar sbc iwalls part edge_rows rho u conc s",
    "lbm_ade_collide_mb": "fp gp f g_in g bc fluid scalar sbc buoy rho u conc s",
    "lbm_ade_stream_collide_mb": "fn gn fo go g bc fluid scalar sbc buoy iwalls row_begin row_end rho u conc s",
    "lbm_ade_collide_o": "fp gp f g_in g bc fluid scalar sbc buoy open carry_out rho u conc s",
    "lbm_ade_stream_collide_o":
        "fn gn fo go g bc fluid scalar sbc buoy iwalls open carry_in carry_out row_begin row_end rho u conc s",
    "lbm_ade_stream_collide_part_o":
        "fn gn fo go g bc fluid scalar sbc buoy iwalls view carry_in carry_out part edge_rows rho u conc s",
    "lbm_ring_ade_collide": "rg fp gp f g_in bc fluid scalar main",
    "lbm_ring_ade_step": "rg fn gn fo go bc fluid scalar edge_rows main",
    "lbm_ring_ade_step_ex": "rg fn gn fo go bc fluid scalar sbc edge_rows main",
    "lbm_ring_ade_collide_b": "rg fp gp f g_in bc fluid scalar sbc buoy main",
    "lbm_ring_ade_step_b": "rg fn gn fo go bc fluid scalar sbc buoy edge_rows main",
    "lbm_ring_ade_step_w": "rg fn gn fo go bc fluid scalar sbc buoy iwalls edge_rows main",
    "lbm_ring_ade_collide_o": "rg fp gp f g_in bc fluid scalar sbc buoy view carry_out main",
    "lbm_ring_ade_step_o": "rg fn gn fo go bc fluid scalar sbc buoy iwalls view carry_in carry_out edge_rows main",
    "lbm_ring_ade_collide_m": "rg fp gp f g_in bc fluid scalar sbc main",
    "lbm_ring_ade_step_m": "rg fn gn fo go bc fluid scalar sbc iwalls edge_rows main",
}
ENTRIES = sorted(PROTOTYPES)


def test_the_parsed_prototypes_are_the_table():
    assert len(PROTOTYPES) == 28
    assert ade_calls.PROTOTYPES == {name: names.split() for name, names in PROTOTYPES.items()}
    assert set(PROTOTYPES) <= set(pylbm.declared_symbols())


class Table:
    def __init__(self, address):
        self.h = ct.c_void_p(address)


class StubLib:
    """in the library's place: every lbm_* call records its arguments and returns `status`"""

    def __init__(self, status=0):
        self.status, self.calls = status, []
        self.raw = self

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name, args))
            return self.status
        return record


def a_value(name, i):
    """a value for parameter `name` that its position i can be read back from"""
    if name in ade_calls.CONVERT and ade_calls.CONVERT[name] is ade_calls.ref:
        return (ct.c_int * 1)(1000 + i)
    if name in ("iwalls", "open", "view"):
        return Table(2000 + i)
    if name == "rg":
        return ct.c_void_p(3000 + i)
    if name in ("row_begin", "row_end", "part", "edge_rows", "s", "main"):
        return 4000 + i
    return 8 * (5000 + i)  # a device address: pylbm._ptr takes an int


def read_back(name, arg):
    if name in ade_calls.CONVERT and ade_calls.CONVERT[name] is ade_calls.ref:
        return arg._obj[0] - 1000
    if name in ("iwalls", "open", "view"):
        return arg.value - 2000
    if name == "rg":
        return arg.value - 3000
    if name in ("row_begin", "row_end", "part", "edge_rows"):
        return arg - 4000
    if name in ("s", "main"):
        return arg.value - 4000
    return ct.cast(arg, ct.c_void_p).value // 8 - 5000


@pytest.mark.parametrize("name", ENTRIES)
def test_every_argument_lands_at_its_parameters_index(name):
    names = PROTOTYPES[name].split()
    lib = StubLib()
    assert ade_calls.call_rc(lib, name, **{n: a_value(n, i) for i, n in enumerate(names)}) == 0
    (called, args), = lib.calls
    assert called == name and len(args) == len(names)
    assert [read_back(n, a) for n, a in zip(names, args)] == list(range(len(names)))


@pytest.mark.parametrize("name", ENTRIES)
def test_an_omitted_optional_parameter_is_null_and_the_shorthands_fill_their_parameters(name):
    names = PROTOTYPES[name].split()
    first = 1 if names[0] == "rg" else 0
    value = {n: a_value(n, i) for i, n in enumerate(names)}
    kw = {n: value[n] for n in names if n not in ade_calls.OPTIONAL and n not in names[first:first + 4] + ["fluid", "scalar"]}
    kw.update(dst=[value[n] for n in names[first:first + 2]], src=[value[n] for n in names[first + 2:first + 4]],
              prm=(value["fluid"], value["scalar"]))
    args = ade_calls.arguments(name, **kw)
    assert len(args) == len(names)
    for i, (n, a) in enumerate(zip(names, args)):
        if n in ade_calls.OPTIONAL:
            assert not a or not getattr(a, "value", 1), (n, a)  # NULL: None, a typed null pointer or stream 0
        else:
            assert read_back(n, a) == i, n
    if "rho" in names:
        m = [value[n] for n in ("rho", "u", "conc")]
        args = ade_calls.arguments(name, moments=m, **kw)
        assert [read_back(n, args[names.index(n)]) for n in ("rho", "u", "conc")] == [names.index(n) for n in ("rho", "u", "conc")]


@pytest.mark.parametrize("name", ENTRIES)
def test_an_argument_the_entry_does_not_take_is_a_type_error(name):
    names = PROTOTYPES[name].split()
    kw = {n: a_value(n, i) for i, n in enumerate(names)}
    for extra in ("sbc", "buoy", "iwalls", "open", "view", "carry_in", "carry_out", "g", "rho", "row_begin", "part", "nonsense"):
        if extra not in names:
            with pytest.raises(TypeError, match=f"{name} takes no {extra}"):
                ade_calls.arguments(name, **kw, **{extra: a_value(extra, 0)})
    required = next(n for n in names if n not in ade_calls.OPTIONAL)
    with pytest.raises(TypeError, match=f"{name} needs {required}"):
        ade_calls.arguments(name, **{n: v for n, v in kw.items() if n != required})


def test_the_checked_call_raises_the_librarys_error_and_the_rc_form_returns_the_status():
    """through pylbm.Lib's own checked call: only the loaded library is replaced"""
    stub = StubLib(status=-1)
    stub.lbm_last_error_string = lambda: b"lbm_ade_collide: refused for the test"
    lib = pylbm.Lib.__new__(pylbm.Lib)
    lib.raw = stub
    kw = {n: a_value(n, i) for i, n in enumerate(PROTOTYPES["lbm_ade_collide"].split())}
    assert ade_calls.call_rc(lib, "lbm_ade_collide", **kw) == -1
    with pytest.raises(pylbm.LbmError, match="lbm_ade_collide -> -1: lbm_ade_collide: refused for the test"):
        ade_calls.call(lib, "lbm_ade_collide", **kw)
    assert [c[0] for c in stub.calls] == ["lbm_ade_collide"] * 2


def test_the_suites_calls_pick_the_entry_of_their_suffix():
    lib = pylbm.Lib.__new__(pylbm.Lib)
    lib.raw = StubLib()
    g = pylbm.Geom(6, 8, 0)
    one = (ct.c_int * 1)(0)
    lat = (8, 16), (24, 32)
    for sfx in ("", "_ex", "_b", "_w", "_o", "_m"):
        ade_calls.step_into(lib, sfx, g, one, (one, one), *lat, rows=(2, 5))
        ade_calls.both_parts(lib, sfx, g, one, (one, one), *lat, 1)
    for sfx in ("", "_b", "_m", "_mb", "_o"):
        ade_calls.collide(lib, sfx, g, one, (one, one), *lat)
    called = [c[0] for c in lib.raw.calls]
    assert called[:6] == ["lbm_ade_stream_collide", "lbm_ade_stream_collide_part", "lbm_ade_stream_collide_part",
                          "lbm_ade_stream_collide_ex", "lbm_ade_stream_collide_part_ex", "lbm_ade_stream_collide_part_ex"]
    assert called[-5:] == ["lbm_ade_collide", "lbm_ade_collide_b", "lbm_ade_collide_m", "lbm_ade_collide_mb", "lbm_ade_collide_o"]
    step, frame, inner = (lib.raw.calls[i][1] for i in range(3))
    names = PROTOTYPES["lbm_ade_stream_collide"].split()
    assert (step[names.index("row_begin")], step[names.index("row_end")]) == (2, 5)
    names = PROTOTYPES["lbm_ade_stream_collide_part"].split()
    assert [a[names.index("part")] for a in (frame, inner)] == [pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER]
    assert frame[names.index("edge_rows")] == 1
    with pytest.raises(TypeError, match="lbm_ade_stream_collide_part takes no buoy"):
        ade_calls.part(lib, "", g, one, (one, one), *lat, pylbm.ADE_PART_FRAME, 1, buoy=one)
