"""The raw calls of the buoyant slab and ring entries of the fluid + scalar step with the fluid by model --
lbm_ade_slab_stream_collide_mb, lbm_ring_ade_slab_collide_mb, lbm_ring_ade_slab_step_mb -- in the manner of
tests/ade_calls.py: keyword arguments named after the parameters of the prototype in include/lbm_hip.h, an omitted optional
parameter is NULL, a keyword the entry does not take is a TypeError.  The three prototypes are read from the header HERE
(their names are outside the family tests/ade_calls.py reads and tests/test_ade_calls.py pins);
tests/test_ade_kbc_buoyancy_slab_abi.py pins them to a literal table on the CPU."""
import re

import pylbm
from ade_calls import CONVERT, OPTIONAL
from pylbm import _ptr

FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
PART, RING_COLLIDE, RING_STEP = "lbm_ade_slab_stream_collide_mb", "lbm_ring_ade_slab_collide_mb", "lbm_ring_ade_slab_step_mb"


def prototypes(header=pylbm.HEADER):
    """{entry: its parameter names in order} of the three entries"""
    txt = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    found = re.findall(r"\bint\s+(lbm_(?:ring_)?ade_slab_\w+_mb)\s*\(([^)]*)\)\s*;", txt)
    return {name: [re.search(r"(\w+)\s*$", a).group(1) for a in args.split(",")] for name, args in found}


PROTOTYPES = prototypes()


def arguments(name, **kw):
    """the positional arguments of entry `name` from keywords named after its parameters; dst, src, prm, moments as in
    tests/ade_calls.py"""
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


def part(lib, g, bc, prm, dst, src, which, E, **kw):
    """lbm_ade_slab_stream_collide_mb: part `which` with E edge rows"""
    call(lib, PART, dst=dst, src=src, g=g, bc=bc, prm=prm, part=which, edge_rows=E, **kw)


def both_parts(lib, g, bc, prm, dst, src, E, **kw):
    """FRAME, then INNER"""
    for which in (FRAME, INNER):
        part(lib, g, bc, prm, dst, src, which, E, **kw)
