"""The raw calls of the fluid + scalar suites, in one place: every lbm_ade_collide*, lbm_ade_stream_collide*,
lbm_ade_stream_collide_part* and lbm_ring_ade_* entry point is called through `call` (checked: LbmError) or `call_rc` (the
status, for the refusal tests), with keyword arguments named after the parameters of its prototype in include/lbm_hip.h.
The prototypes are read from the header once (PROTOTYPES); tests/test_ade_calls.py pins them to a literal table on the CPU,
so a reordered parameter fails there and not as a mis-placed pointer on the GPU.

An omitted (or None) optional parameter is passed as NULL; a keyword the entry does not take is a TypeError -- a test never
drops its buoyancy or its table by picking the wrong suffix.  Shorthands: dst = (fn, gn) / (fp, gp), src = (fo, go) /
(f, g_in), prm = (fluid, scalar), moments = (rho, u, conc).

On top of it the five calls the suites make, each with the suffix of the entry it goes through ("", "_ex", "_b", "_w",
"_o", "_m", "_mb"): full_step, step_into, part, both_parts, collide."""
import ctypes as ct
import re

import pylbm
from pylbm import _ptr

FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
OPTIONAL = {"sbc", "buoy", "iwalls", "open", "view", "carry_in", "carry_out", "rho", "u", "conc", "s", "main"}


def ref(x):
    """a pylbm structure -> its address, None -> NULL"""
    return ct.byref(x) if x is not None else None


def handle(table):
    """a table object (pylbm.AdeInteriorWalls, pylbm.AdeOpenBoundary) -> its handle, None -> NULL"""
    return table.h if table is not None else None


CONVERT = dict.fromkeys(("g", "bc", "fluid", "scalar", "sbc", "buoy"), ref)
CONVERT.update(dict.fromkeys(("iwalls", "open", "view"), handle))
CONVERT.update(dict.fromkeys(("row_begin", "row_end", "part", "edge_rows"), int))
CONVERT.update(dict.fromkeys(("s", "main"), pylbm._stream))
CONVERT["rg"] = lambda ring: ring


def prototypes(header=pylbm.HEADER):
    """{entry: its parameter names in order} of the entry points this module calls"""
    txt = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    found = re.findall(r"\bint\s+(lbm_(?:ring_)?ade_(?:collide|stream_collide|step)\w*)\s*\(([^)]*)\)\s*;", txt)
    return {name: [re.search(r"(\w+)\s*$", a).group(1) for a in args.split(",")] for name, args in found}


PROTOTYPES = prototypes()


def arguments(name, **kw):
    """the positional arguments of entry `name` from keywords named after its parameters"""
    names = PROTOTYPES[name]
    first = 1 if names[0] == "rg" else 0
    for short, group in (("dst", names[first:first + 2]), ("src", names[first + 2:first + 4]), ("prm", ["fluid", "scalar"]),
                         ("moments", ["rho", "u", "conc"])):
        values = kw.pop(short, None)
        if values is not None:
            assert len(values) == len(group) and not set(group) & set(kw), (name, short)
            kw.update(zip(group, values))
    kw = {k: v for k, v in kw.items() if v is not None}
    extra = sorted(set(kw) - set(names))
    if extra:
        raise TypeError(f"{name} takes no {', '.join(extra)}")
    missing = [n for n in names if n not in kw and n not in OPTIONAL]
    if missing:
        raise TypeError(f"{name} needs {', '.join(missing)}")
    return [CONVERT.get(n, _ptr)(kw.get(n)) for n in names]


def call(lib, name, **kw):
    """the checked call: a non-zero status raises pylbm.LbmError with the library's message"""
    return getattr(lib, name[len("lbm_"):])(*arguments(name, **kw))


def call_rc(lib, name, **kw):
    """the unchecked call -> its status; the message is lib.raw.lbm_last_error_string()"""
    return getattr(lib.raw, name)(*arguments(name, **kw))


# ---- the calls the suites make; sfx: the suffix of the entry -------------------------------------------------------------
def step_into(lib, sfx, g, bc, prm, dst, src, rows=None, **kw):
    """lbm_ade_stream_collide<sfx> over rows [rows[0], rows[1]) (default: all of them) into the lattices given"""
    r0, r1 = rows if rows is not None else (0, g.R)
    call(lib, "lbm_ade_stream_collide" + sfx, dst=dst, src=src, g=g, bc=bc, prm=prm, row_begin=r0, row_end=r1, **kw)


def full_step(lib, sfx, g, bc, prm, fo, go, **kw):
    """lbm_ade_stream_collide<sfx> on every row into fresh lattices -> (fn, gn)"""
    from ade_util import alloc
    fn, gn = alloc(g), alloc(g)
    step_into(lib, sfx, g, bc, prm, (fn, gn), (fo, go), **kw)
    return fn, gn


def part(lib, sfx, g, bc, prm, dst, src, which, E, **kw):
    """lbm_ade_stream_collide_part<sfx>: part `which` with E edge rows"""
    call(lib, "lbm_ade_stream_collide_part" + sfx, dst=dst, src=src, g=g, bc=bc, prm=prm, part=which, edge_rows=E, **kw)


def both_parts(lib, sfx, g, bc, prm, dst, src, E, **kw):
    """FRAME, then INNER"""
    for which in (FRAME, INNER):
        part(lib, sfx, g, bc, prm, dst, src, which, E, **kw)


def collide(lib, sfx, g, bc, prm, dst, src, **kw):
    """lbm_ade_collide<sfx>: the collide-only call"""
    call(lib, "lbm_ade_collide" + sfx, dst=dst, src=src, g=g, bc=bc, prm=prm, **kw)
