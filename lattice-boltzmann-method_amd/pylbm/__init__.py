"""ctypes binding of liblbm_hip.so (the C ABI in include/lbm_hip.h) for tests and bench.py.

The product's host side is C++ (lattice-boltzmann-method_amd/include/lbm/*.hpp, mirroring the
reference's headers); this module is the thin Python door onto the same C ABI.  There is no
CPU fallback: if the HIP library is missing, import fails loudly.
"""
import ctypes as ct
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
REPO = os.path.dirname(PKG_DIR)
LIB_PATH = os.environ.get("LBM_HIP_LIB", os.path.join(PKG_DIR, "lib", "liblbm_hip.so"))
HEADER = os.path.join(REPO, "include", "lbm_hip.h")

EDGE_PERIODIC, EDGE_HALO, EDGE_BOUNCE_BACK, EDGE_SPECULAR, EDGE_ABB_VELOCITY, EDGE_WRAP_NOSHIFT = range(6)
HALO_TWO_PHASE = -3  # lbm_halo_pack / _unpack depth code of the colour-gradient step (21 rows)
MODEL_BGK, MODEL_KBC = 0, 1
FORM_DEFAULT, FORM_REFERENCE_ORDER, FORM_REASSOCIATED = 0, 1, 2   # field `form` of the parameter structs (LBM_FORM_*)
RING_DEFAULT, RING_RCCL, RING_IPC = -1, 0, 1
CG_PART_FRAME, CG_PART_INNER = 1, 2   # lbm_cg_step_fused_part (LBM_CG_PART_*)
ADE_PART_FRAME, ADE_PART_INNER = 1, 2  # lbm_ade_stream_collide_part (LBM_ADE_PART_*)
ADE_SCALAR_NO_FLUX, ADE_SCALAR_FIXED = 0, 1  # lbm_ade_scalar_bc.mode (LBM_ADE_SCALAR_*)
# slot masks of the interior walls' axis-aligned facings (LBM_ADE_FACE_*): bit s-1 = slot s, fluid on the named side
ADE_FACE_ROW_POS, ADE_FACE_ROW_NEG, ADE_FACE_COL_POS, ADE_FACE_COL_NEG = 0x91, 0x64, 0x32, 0xC8

# f rules of the open boundaries (LBM_ADE_OPEN_*)
ADE_OPEN_BOUNCE_BACK, ADE_OPEN_SPECULAR_ROW, ADE_OPEN_SPECULAR_COL, ADE_OPEN_ABB, ADE_OPEN_ABB_EXTRAPOLATED = 1, 2, 3, 4, 5

# value slots of the diagnostics (LBM_DIAG_*): lbm_diag_rows / lbm_diag_fold / Solver.diag / AdeSolver.diag
DIAG_NQ = 17
(DIAG_SUM_RHO, DIAG_SUM_UR, DIAG_SUM_UC, DIAG_SUM_MR, DIAG_SUM_MC, DIAG_SUM_KE, DIAG_MAX_U2, DIAG_MIN_RHO, DIAG_MAX_RHO,
 DIAG_NONFINITE, DIAG_SUM_C, DIAG_SUM_CUR, DIAG_SUM_CUC, DIAG_MIN_C, DIAG_MAX_C, DIAG_SUM_C2, DIAG_SUM_DEV2) = range(DIAG_NQ)
DIAG_NAMES = ("SUM_RHO", "SUM_UR", "SUM_UC", "SUM_MR", "SUM_MC", "SUM_KE", "MAX_U2", "MIN_RHO", "MAX_RHO", "NONFINITE",
              "SUM_C", "SUM_CUR", "SUM_CUC", "MIN_C", "MAX_C", "SUM_C2", "SUM_DEV2")

# value slots of the wall exchange (LBM_WALLX_*): lbm_ade_wallx_rows / lbm_ade_wallx_fold / AdeSolver.wall_exchange
WALLX_NQ = 6
WALLX_FORCE_R, WALLX_FORCE_C, WALLX_MASS, WALLX_SCALAR, WALLX_SCALAR_FIXED, WALLX_NODES = range(WALLX_NQ)
WALLX_NAMES = ("FORCE_R", "FORCE_C", "MASS", "SCALAR", "SCALAR_FIXED", "NODES")

_dp = ct.POINTER(ct.c_double)


class Geom(ct.Structure):
    _fields_ = [("R", ct.c_int), ("C", ct.c_int), ("ghost", ct.c_int),
                ("plane_stride", ct.c_longlong), ("row_pitch", ct.c_int)]

    def __init__(self, R=0, C=0, ghost=0, plane_stride=0, row_pitch=0):
        super().__init__(R, C, ghost, plane_stride, row_pitch)


class Bc(ct.Structure):
    _fields_ = [("row_lo", ct.c_int), ("row_hi", ct.c_int), ("col_lo", ct.c_int),
                ("col_hi", ct.c_int), ("pressure_rows", ct.c_int), ("rho_inlet", ct.c_double),
                ("rho_outlet", ct.c_double), ("uw_r", ct.c_double), ("uw_c", ct.c_double)]

    def __init__(self, row_lo=0, row_hi=0, col_lo=0, col_hi=0, pressure_rows=0, rho_inlet=1.0,
                 rho_outlet=1.0, uw_r=0.0, uw_c=0.0):
        super().__init__(row_lo, row_hi, col_lo, col_hi, pressure_rows, rho_inlet, rho_outlet, uw_r, uw_c)

    @staticmethod
    def periodic():
        return Bc()


class BgkParams(ct.Structure):
    _fields_ = [("omega", ct.c_double), ("incompressible", ct.c_int), ("delta_form", ct.c_int),
                ("force_mode", ct.c_int), ("force_r", ct.c_double), ("force_c", ct.c_double),
                ("guo_a", ct.c_double), ("guo_b", ct.c_double), ("form", ct.c_int)]

    def __init__(self, omega=1.0, incompressible=0, delta_form=0, force=None, guo=(1.0 / 3.0, 1.0 / 9.0), form=FORM_DEFAULT):
        """force=(Fr, Fc): the body force of test/gravity_test.cpp (u += F, Guo-type source); form: FORM_*"""
        if force is None:
            super().__init__(omega, incompressible, delta_form, 0, 0.0, 0.0, 0.0, 0.0, form)
        else:
            super().__init__(omega, incompressible, 1, 1, force[0], force[1], guo[0], guo[1], form)


class KbcParams(ct.Structure):
    _fields_ = [("s2", ct.c_double), ("form", ct.c_int)]

    def __init__(self, s2=1.0, form=FORM_DEFAULT):
        super().__init__(s2, form)


class CgColour(ct.Structure):
    _fields_ = [("rho_0", ct.c_double), ("alpha", ct.c_double), ("nu", ct.c_double),
                ("beta", ct.c_double)]


class CgParams(ct.Structure):
    _fields_ = [("red", CgColour), ("blue", CgColour), ("sigma", ct.c_double),
                ("gravity_r", ct.c_double), ("gravity_c", ct.c_double), ("add_source", ct.c_int),
                ("delta", ct.c_double), ("form", ct.c_int)]


class AdeParams(ct.Structure):
    """lbm_ade_params: the transported scalar's relaxation rate, the velocity w added to the fluid's u in its
    equilibrium (the sedimentation driver's w_s on both components), and the form of both halves (FORM_*)"""
    _fields_ = [("omega_g", ct.c_double), ("w_r", ct.c_double), ("w_c", ct.c_double), ("form", ct.c_int)]

    def __init__(self, omega_g=1.0, w=(0.0, 0.0), form=FORM_DEFAULT):
        super().__init__(omega_g, w[0], w[1], form)


class AdeFluid(ct.Structure):
    """lbm_ade_fluid: the fluid of the fluid + scalar step by model -- AdeFluid(BgkParams(...)) or AdeFluid(KbcParams(...));
    what lbm_ade_collide_m, lbm_ade_stream_collide_m, their buoyant forms lbm_ade_collide_mb / lbm_ade_stream_collide_mb and
    lbm_ade_solver_create_m take"""
    _fields_ = [("model", ct.c_int), ("bgk", BgkParams), ("kbc", KbcParams)]

    def __init__(self, params=None, model=None):
        """model: MODEL_* to override what the type of params says (the ABI tests pass an unknown one)"""
        super().__init__()
        if isinstance(params, KbcParams):
            self.model, self.kbc = MODEL_KBC, params
        elif params is not None:
            self.model, self.bgk = MODEL_BGK, params
        if model is not None:
            self.model = model


class AdeScalarBC(ct.Structure):
    """lbm_ade_scalar_bc: the scalar's wall per edge (row_lo, row_hi, col_lo, col_hi), NO_FLUX or FIXED.  A FIXED edge
    takes fixed=(conc, profile) with profile None (the constant conc) or a device array of C_w along the edge (a float64
    torch tensor, C values on a row edge / R on a column edge, or a device address), read by every step, never copied."""
    EDGES = ("row_lo", "row_hi", "col_lo", "col_hi")
    _fields_ = [("mode", ct.c_int * 4), ("conc", ct.c_double * 4), ("profile", _dp * 4)]

    def __init__(self, **fixed):
        """AdeScalarBC(col_lo=1e-3, col_hi=(0.0, profile_tensor)): the named edges FIXED, the others NO_FLUX"""
        super().__init__()
        self._keep = []  # the profile tensors stay alive with the descriptor
        for name, v in fixed.items():
            e = self.EDGES.index(name)
            conc, prof = (v if isinstance(v, tuple) else (v, None))
            self.mode[e] = ADE_SCALAR_FIXED
            self.conc[e] = float(conc)
            self.profile[e] = _ptr(prof) if prof is not None else ct.cast(None, _dp)
            if prof is not None and not isinstance(prof, int):
                self._keep.append(prof)


class AdeBuoyancy(ct.Structure):
    """lbm_ade_buoyancy: the scalar pushes on the fluid (Boussinesq), per node F = beta * (C - c_ref), rows / columns.
    u_shift * F is added to u before both equilibria and guo = (a, b) are the source term's coefficients: the defaults
    (1, (1/3, 1/9)) are the reference's gravity_test.cpp, (0.5, (3, 9)) is Guo's scheme.  beta = (0, 0) is the passive step."""
    _fields_ = [("beta_r", ct.c_double), ("beta_c", ct.c_double), ("c_ref", ct.c_double), ("u_shift", ct.c_double),
                ("guo_a", ct.c_double), ("guo_b", ct.c_double)]

    def __init__(self, beta=(0.0, 0.0), c_ref=0.0, u_shift=1.0, guo=(1.0 / 3.0, 1.0 / 9.0)):
        super().__init__(beta[0], beta[1], c_ref, u_shift, guo[0], guo[1])


class Converge(ct.Structure):
    """lbm_converge: the stopping rule of run_until.  The watched value is the sum `quantity` (a DIAG_SUM_* index) over rows
    [row_begin, row_end) divided by their node count, formed at every iteration count t > 0 with t % interval == offset
    from the moments of iteration t - 1; the run stops when |value / old - 1| < tolerance.  The defaults are the
    reference drivers' (SUM_UR, 100, 1, 1e-12, 1.0); row_end=None: all rows of the solver."""
    _fields_ = [("quantity", ct.c_int), ("interval", ct.c_int), ("offset", ct.c_int), ("tolerance", ct.c_double),
                ("old_value", ct.c_double), ("row_begin", ct.c_int), ("row_end", ct.c_int)]

    def __init__(self, quantity=DIAG_SUM_UR, interval=100, offset=1, tolerance=1e-12, old_value=1.0, row_begin=0, row_end=None):
        super().__init__(quantity, interval, offset, tolerance, old_value, row_begin, -1 if row_end is None else row_end)


class LbmError(RuntimeError):
    pass


class AdeInteriorWalls:
    """Python face of lbm_ade_iwalls: wall nodes inside the block of the fluid + scalar step (the rectangle of
    test/rectangle_sedimentation_test.cpp:184-196, :220-232).  Build with add / add_box, then finalize() -- the upload --
    and hand it to AdeSolver(walls=...) / set_walls; it must outlive every solver and captured graph that uses it."""

    def __init__(self, lib, R, C):
        self.lib, self.R, self.C = lib, R, C
        self.h = ct.c_void_p()
        lib.ade_iwalls_create(ct.byref(self.h), int(R), int(C))

    def add(self, r0, c0, dr, dc, n, f_slots, g_slots, g_mode=ADE_SCALAR_NO_FLUX, conc=0.0):
        """the n nodes (r0 + i dr, c0 + i dc); negative r0 / c0 count from the end; slot masks: bit s-1 = slot s"""
        self.lib.ade_iwalls_add(self.h, int(r0), int(c0), int(dr), int(dc), int(n), ct.c_uint(f_slots), ct.c_uint(g_slots),
                                int(g_mode), ct.c_double(conc))
        return self

    def add_box(self, r0, r1, c0, c1, g_mode=ADE_SCALAR_NO_FLUX, conc=0.0):
        """the closed box of rows r0..r1 and columns c0..c1 (inclusive, 0 <= r0 <= r1, 0 <= c0 <= c1) as four
        outward-facing segments, f and g alike; a corner node carries the union of its two facings"""
        for args in ((r0, c0, 0, 1, c1 - c0 + 1, ADE_FACE_ROW_NEG), (r1, c0, 0, 1, c1 - c0 + 1, ADE_FACE_ROW_POS),
                     (r0, c0, 1, 0, r1 - r0 + 1, ADE_FACE_COL_NEG), (r0, c1, 1, 0, r1 - r0 + 1, ADE_FACE_COL_POS)):
            self.add(*args, args[-1], g_mode, conc)
        return self

    def count(self):
        return int(self.lib.raw.lbm_ade_iwalls_count(self.h))

    def nodes(self):
        """the merged table, sorted by (r, c): a list of dicts r, c, f_slots, g_slots, g_fixed_slots, conc"""
        out = []
        for i in range(self.count()):
            r, c, f, g, gf, conc = ct.c_int(), ct.c_int(), ct.c_uint(), ct.c_uint(), ct.c_uint(), ct.c_double()
            self.lib.ade_iwalls_node(self.h, i, *[ct.byref(x) for x in (r, c, f, g, gf, conc)])
            out.append(dict(r=r.value, c=c.value, f_slots=f.value, g_slots=g.value, g_fixed_slots=gf.value, conc=conc.value))
        return out

    def finalize(self):
        self.lib.ade_iwalls_finalize(self.h)
        return self

    def slab(self, row0, R):
        """the slab view (lbm_ade_iwalls_slab): a new, unfinalized AdeInteriorWalls for an R x C lattice holding this
        table's nodes of rows [row0, row0 + R) with r - row0; this table may be finalized or not and is not modified"""
        view = AdeInteriorWalls.__new__(AdeInteriorWalls)
        view.lib, view.R, view.C, view.h = self.lib, int(R), self.C, ct.c_void_p()
        self.lib.ade_iwalls_slab(ct.byref(view.h), self.h, int(row0), int(R))
        return view

    def close(self):
        if self.h:
            self.lib.ade_iwalls_destroy(self.h)
            self.h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AdeOpenBoundary:
    """Python face of lbm_ade_open: open boundaries of the fluid + scalar step on one block (inlet, outlet, specular lid and
    zero-gradient copies of test/rectangle_sedimentation_test.cpp).  Build with add_f / add_g / add_g_copy (or channel),
    then finalize() -- the upload -- and hand it to AdeSolver(open=...) / set_open; it must outlive every solver and
    captured graph that uses it."""

    def __init__(self, lib, R, C):
        self.lib, self.R, self.C = lib, R, C
        self.h = ct.c_void_p()
        lib.ade_open_create(ct.byref(self.h), int(R), int(C))

    def add_f(self, r0, c0, dr, dc, n, slots, rule, p=(0.0, 0.0), neighbour=(0, 0)):
        """an f rule (ADE_OPEN_*) on the slots of the mask; p: u_w of ABB, (a, b) of ABB_EXTRAPOLATED with its inward
        neighbour offset"""
        self.lib.ade_open_add_f(self.h, int(r0), int(c0), int(dr), int(dc), int(n), ct.c_uint(slots), int(rule),
                                ct.c_double(p[0]), ct.c_double(p[1]), int(neighbour[0]), int(neighbour[1]))
        return self

    def add_g(self, r0, c0, dr, dc, n, slots, g_mode=ADE_SCALAR_NO_FLUX, conc=0.0):
        self.lib.ade_open_add_g(self.h, int(r0), int(c0), int(dr), int(dc), int(n), ct.c_uint(slots), int(g_mode),
                                ct.c_double(conc))
        return self

    def add_g_copy(self, r0, c0, dr, dc, n, source):
        """the nodes of the segment read their post-collision g from node + source"""
        self.lib.ade_open_add_g_copy(self.h, int(r0), int(c0), int(dr), int(dc), int(n), int(source[0]), int(source[1]))
        return self

    def channel(self, u_in, conc_w=1e-3, conc_rows=50):
        """the sedimentation channel of the reference driver for this R x C (lbm_ade_open_add_channel)"""
        self.lib.ade_open_add_channel(self.h, ct.c_double(u_in), ct.c_double(conc_w), int(conc_rows))
        return self

    def count(self):
        return int(self.lib.raw.lbm_ade_open_count(self.h))

    def carry_len(self):
        return int(self.lib.raw.lbm_ade_open_carry_len(self.h))

    def node(self, i):
        """node i of the resolved table: dict r, c, f_rule [8], g_rule [8] (0 none, 1 + ADE_SCALAR_*), g_src [9] of (r, c)"""
        r, c = ct.c_int(), ct.c_int()
        fr, gr, sr, sc = (ct.c_int * 8)(), (ct.c_int * 8)(), (ct.c_int * 9)(), (ct.c_int * 9)()
        self.lib.ade_open_node(self.h, int(i), ct.byref(r), ct.byref(c), fr, gr, sr, sc)
        return dict(r=r.value, c=c.value, f_rule=list(fr), g_rule=list(gr), g_src=list(zip(sr, sc)),
                    unreachable=int(self.lib.raw.lbm_ade_open_unreachable(self.h, int(i))))

    def nodes(self):
        return [self.node(i) for i in range(self.count())]

    def finalize(self):
        self.lib.ade_open_finalize(self.h)
        return self

    def slab(self, row0, R):
        """the slab view (lbm_ade_open_slab): a new, unfinalized AdeOpenBoundary for an R x C lattice listing this table's
        nodes of rows [row0, row0 + R) at r - row0, its g sources slab-local with the row in [-1, R] (the ghost rows), its
        carry its own; this table may be finalized or not and is not modified.  A view takes no add_* call and goes to
        ade_stream_collide_part_o / ring_ade_collide_o / ring_ade_step_o only."""
        view = AdeOpenBoundary.__new__(AdeOpenBoundary)
        view.lib, view.R, view.C, view.h = self.lib, int(R), self.C, ct.c_void_p()
        self.lib.ade_open_slab(ct.byref(view.h), self.h, int(row0), int(R))
        return view

    def close(self):
        if self.h:
            self.lib.ade_open_destroy(self.h)
            self.h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def declared_symbols(header=HEADER):
    """Every function the C header declares (used by the ABI-completeness test)."""
    txt = open(header).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lbm_[a-z0-9_]+)\s*\(", txt)))


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise LbmError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C lattice-boltzmann-method_amd/csrc` (no CPU fallback exists)")
    lib = ct.CDLL(path)
    lib.lbm_last_error_string.restype = ct.c_char_p
    lib.lbm_default_plane_pad.restype = ct.c_longlong
    lib.lbm_solver_block_launches.restype = ct.c_longlong
    lib.lbm_slab_ibm_msg_doubles.restype = ct.c_longlong
    lib.lbm_cg_solver_pair_launches.restype = ct.c_longlong
    lib.lbm_slab_pressure_msg_doubles.restype = ct.c_longlong
    lib.lbm_ade_solver_launches.restype = ct.c_longlong
    lib.lbm_ade_open_carry_len.restype = ct.c_longlong
    lib.lbm_ade_part_launches.restype = ct.c_longlong
    # the slab and ring entries of the fluid by model (AdeFluid): lattices, descriptors by reference, handles, streams
    p, i = ct.c_void_p, ct.c_int
    lib.lbm_ade_stream_collide_part_m.argtypes = [p, p, p, p, p, p, p, p, p, p, i, i, p, p, p, p]
    lib.lbm_ring_ade_collide_m.argtypes = [p, p, p, p, p, p, p, p, p, p]
    lib.lbm_ring_ade_step_m.argtypes = [p, p, p, p, p, p, p, p, p, p, i, p]
    # and their buoyant forms: the descriptor of lbm_ade_buoyancy after sbc
    lib.lbm_ade_slab_stream_collide_mb.argtypes = [p, p, p, p, p, p, p, p, p, p, p, i, i, p, p, p, p]
    lib.lbm_ring_ade_slab_collide_mb.argtypes = [p, p, p, p, p, p, p, p, p, p, p]
    lib.lbm_ring_ade_slab_step_mb.argtypes = [p, p, p, p, p, p, p, p, p, p, p, i, p]
    # open boundaries and the wall exchange with the fluid by model: lbm_ade_collide_o / lbm_ade_stream_collide_o /
    # lbm_ade_solver_set_open / lbm_ade_wallx_rows / lbm_ade_solver_wall_exchange with an AdeFluid
    lib.lbm_ade_open_collide_m.argtypes = [p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p]
    lib.lbm_ade_open_stream_collide_m.argtypes = [p, p, p, p, p, p, p, p, p, p, p, p, p, p, i, i, p, p, p, p]
    lib.lbm_ade_solver_set_open_m.argtypes = [p, p]
    lib.lbm_ade_wallx_rows_m.argtypes = [p, i, i, p, p, p, p, p, p, p, p, p, p, i, i, p]
    lib.lbm_ade_solver_wall_exchange_m.argtypes = [p, p, i, i, p, p]
    for fn in (lib.lbm_ade_stream_collide_part_m, lib.lbm_ring_ade_collide_m, lib.lbm_ring_ade_step_m,
               lib.lbm_ade_slab_stream_collide_mb, lib.lbm_ring_ade_slab_collide_mb, lib.lbm_ring_ade_slab_step_mb,
               lib.lbm_ade_open_collide_m, lib.lbm_ade_open_stream_collide_m, lib.lbm_ade_solver_set_open_m,
               lib.lbm_ade_wallx_rows_m, lib.lbm_ade_solver_wall_exchange_m):
        fn.restype = ct.c_int
    return lib


class Lib:
    """Checked calls: any non-zero status raises LbmError with the library's message."""

    def __init__(self, path=LIB_PATH):
        self.raw = load_library(path)

    def __getattr__(self, name):
        fn = getattr(self.raw, "lbm_" + name)

        def call(*args):
            rc = fn(*args)
            if rc != 0:
                raise LbmError(f"lbm_{name} -> {rc}: {self.raw.lbm_last_error_string().decode()}")
            return rc

        return call

    def device_count(self):
        return self.raw.lbm_device_count()

    def default_plane_pad(self, R, C):
        return int(self.raw.lbm_default_plane_pad(R, C))

    def diag_fold_host(self, table, row_begin=0, row_end=None):
        """lbm_diag_fold_host: rows [row_begin, row_end) of a host row table [DIAG_NQ, rows] -> the DIAG_NQ values
        (diag_rows / diag_fold, the device calls, go through __getattr__ like every other entry point)"""
        table = np.ascontiguousarray(table, dtype=np.float64)
        assert table.ndim == 2 and table.shape[0] == DIAG_NQ, table.shape
        out = np.empty(DIAG_NQ)
        self.__getattr__("diag_fold_host")(_hptr(out), _hptr(table), table.shape[1], int(row_begin),
                                           int(table.shape[1] if row_end is None else row_end))
        return out

    def wallx_fold_host(self, table, row_begin=0, row_end=None):
        """lbm_ade_wallx_fold_host: rows [row_begin, row_end) of a host row table [WALLX_NQ, rows] -> the WALLX_NQ values"""
        table = np.ascontiguousarray(table, dtype=np.float64)
        assert table.ndim == 2 and table.shape[0] == WALLX_NQ, table.shape
        out = np.empty(WALLX_NQ)
        self.__getattr__("ade_wallx_fold_host")(_hptr(out), _hptr(table), table.shape[1], int(row_begin),
                                                int(table.shape[1] if row_end is None else row_end))
        return out

    def reset_tuning(self):
        for k in (b"variant", b"nt", b"grid_cap", b"block", b"rows", b"xcd_swizzle", b"tb_rows", b"tb_block", b"tb_order", b"sw_rows", b"sw_waves", b"solver_depth", b"cg_fused", b"cg_tile", b"cg_xcd", b"kbc_fast", b"kbc_depth", b"bgk_fast", b"cg_strip", b"cg_rows", b"cg_split", b"sw_split", b"solver_depth_walls", b"ibm_depth", b"ibm_gate", b"bgk_fast_delta", b"pressure_depth", b"halo_grid", b"cg_strip2", b"cg_rows2", b"sw_pair", b"sw_pf2", b"cg_strip_xcd", b"cg_merge", b"cg_frame_beside", b"ring_period", b"ibm_step_opt", b"ibm_step_split", b"ibm_step_chain", b"ibm_box", b"ibm_box_overlap", b"bg_priority", b"ibm_chain_kernel", b"ibm_chain_wgs", b"ibm_box_sole", b"sw_ldsring", b"ring_ipc_timeout_ms", b"cg_big", b"cg_big_xcd", b"ring_ipc_force_cached", b"ring_ipc_cached_ok", b"row_pad", b"cg_walk_rows", b"cg_walk_tile_xcd", b"sw_cols2"):
            self.set_tuning(k, -1)


def _ptr(t):
    """torch CUDA tensor (float64, contiguous) or int address -> double*"""
    if t is None:
        return ct.cast(None, _dp)
    if isinstance(t, int):
        return ct.cast(t, _dp)
    # strided lattice views (padded planes) are fine: the geometry carries the plane stride
    assert t.stride(-1) == 1 and str(t.dtype) == "torch.float64", (t.dtype, t.stride())
    return ct.cast(t.data_ptr(), _dp)


def _hptr(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_dp)


def _stream(s):
    return ct.c_void_p(0 if s is None else int(s))


def _diag(call, h, R, profile, row_begin, row_end, table):
    """shared by Solver.diag / AdeSolver.diag: the DIAG_NQ values of rows [row_begin, row_end), with the row table
    [DIAG_NQ, R] as a second result if table"""
    out = np.empty(DIAG_NQ)
    tab = np.empty((DIAG_NQ, R)) if table else None
    call(h, _ptr(profile), int(row_begin), int(R if row_end is None else row_end), _hptr(out),
         _hptr(tab) if table else None)
    return (out, tab) if table else out


def _run_until(call, h, R, converge, max_steps):
    """shared by Solver.run_until / AdeSolver.run_until: (steps_done, converged, last_value)"""
    cv = Converge(converge.quantity, converge.interval, converge.offset, converge.tolerance, converge.old_value,
                  converge.row_begin, R if converge.row_end < 0 else converge.row_end)
    steps, conv, last = ct.c_int(), ct.c_int(), ct.c_double()
    call(h, ct.byref(cv), int(max_steps), ct.byref(steps), ct.byref(conv), ct.byref(last))
    return steps.value, bool(conv.value), last.value


class Solver:
    """Python face of lbm_solver (single block).  numpy AoS in/out, reference layout."""

    def __init__(self, lib, model, R, C, params, bc=None, stream=None):
        self.lib, self.R, self.C = lib, R, C
        self.g = Geom(R, C, 0)
        self.bc = bc if bc is not None else Bc.periodic()
        self.params = params
        self.h = ct.c_void_p()
        lib.solver_create(ct.byref(self.h), model, ct.byref(self.g), ct.byref(self.bc),
                          ct.byref(params), _stream(stream))

    def close(self):
        if self.h:
            self.lib.solver_destroy(self.h)
            self.h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_f(self, f):
        f = np.ascontiguousarray(f, dtype=np.float64)
        assert f.shape == (self.R, self.C, 9)
        self.lib.solver_set_f_aos(self.h, _hptr(f))

    def set_moments(self, rho, u):
        """KBC: the first iteration collides on these held moments (ulbm_poiseuille.cpp:85-86)"""
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        assert rho.shape == (self.R, self.C) and u.shape == (self.R, self.C, 2)
        self.lib.solver_set_moments_aos(self.h, _hptr(rho), _hptr(u))

    def get_f(self):
        f = np.empty((self.R, self.C, 9))
        self.lib.solver_get_f_aos(self.h, _hptr(f))
        return f

    def step(self, n, record_moments=False):
        self.lib.solver_step(self.h, int(n), int(bool(record_moments)))

    def moments(self):
        rho = np.empty((self.R, self.C))
        u = np.empty((self.R, self.C, 2))
        self.lib.solver_get_moments_aos(self.h, _hptr(rho), _hptr(u))
        return rho, u

    def sync(self):
        self.lib.solver_sync(self.h)

    def diag(self, profile=None, row_begin=0, row_end=None, table=False):
        """the DIAG_NQ diagnostics of the moments of the last step(.., record_moments=True), reduced on the device;
        profile: a device array [C] (float64 torch tensor or address) for DIAG_SUM_DEV2; table=True: (values, row table)"""
        return _diag(self.lib.solver_diag, self.h, self.R, profile, row_begin, row_end, table)

    def run_until(self, converge, max_steps):
        """step until the rule of `converge` (Converge) fires or max_steps are done: (steps_done, converged, last_value)"""
        return _run_until(self.lib.solver_run_until, self.h, self.R, converge, max_steps)

    def checkpoint_save(self, path):
        self.lib.solver_checkpoint_save(self.h, str(path).encode())

    def checkpoint_load(self, path):
        self.lib.solver_checkpoint_load(self.h, str(path).encode())

    def attach_ibm(self, ibm, guo_a=1.0 / 3.0, guo_b=1.0 / 9.0):
        """defaults: the (1/3, 1/9) the cylinder driver uses (cylinder_test.cpp:66-67)"""
        self._ibm = ibm  # keep alive
        self.lib.solver_attach_ibm(self.h, ibm.h, ct.c_double(guo_a), ct.c_double(guo_b))

    def lattices(self):
        a, b, g = _dp(), _dp(), Geom()
        self.lib.solver_lattices(self.h, ct.byref(a), ct.byref(b), ct.byref(g))
        return ct.cast(a, ct.c_void_p).value, ct.cast(b, ct.c_void_p).value, g


class AdeSolver:
    """Python face of lbm_ade_solver: a fluid f and a transported scalar g on one block (the sediment loop of
    test/rectangle_sedimentation_test.cpp), numpy AoS in/out, reference layout.  fluid: BgkParams (the compressible BGK
    fluid, lbm_ade_solver_create), or KbcParams / AdeFluid (the entropic KBC fluid, lbm_ade_solver_create_m)."""

    def __init__(self, lib, R, C, fluid, scalar, bc=None, stream=None, scalar_bc=None, buoyancy=None, walls=None,
                 open=None):
        self.lib, self.R, self.C, self.fluid, self.scalar = lib, R, C, fluid, scalar
        self.g = Geom(R, C, 0)
        self.bc = bc if bc is not None else Bc.periodic()
        self.h = ct.c_void_p()
        if isinstance(fluid, (KbcParams, AdeFluid)):
            self.fluid_m = fluid if isinstance(fluid, AdeFluid) else AdeFluid(fluid)
            lib.ade_solver_create_m(ct.byref(self.h), ct.byref(self.g), ct.byref(self.bc), ct.byref(self.fluid_m),
                                    ct.byref(scalar), _stream(stream))
        else:
            lib.ade_solver_create(ct.byref(self.h), ct.byref(self.g), ct.byref(self.bc), ct.byref(fluid),
                                  ct.byref(scalar), _stream(stream))
        self.scalar_bc = self.buoyancy = self.walls = self.open = None
        try:
            if walls is not None:
                self.set_walls(walls)
            if open is not None:  # by model: a KBC fluid takes the table through set_open_m
                (self.set_open_m if isinstance(fluid, (KbcParams, AdeFluid)) else self.set_open)(open)
            if scalar_bc is not None:
                self.set_scalar_bc(scalar_bc)
            if buoyancy is not None:  # by model: a KBC fluid takes the forced collision of set_buoyancy_m
                (self.set_buoyancy_m if isinstance(fluid, (KbcParams, AdeFluid)) else self.set_buoyancy)(buoyancy)
        except LbmError:
            self.close()
            raise

    def set_scalar_bc(self, scalar_bc):
        """the scalar's walls from the next stream on (AdeScalarBC, or None: all NO_FLUX)"""
        self.lib.ade_solver_set_scalar_bc(self.h, ct.byref(scalar_bc) if scalar_bc is not None else None)
        self.scalar_bc = scalar_bc  # keeps its profile arrays alive

    def set_buoyancy(self, buoyancy):
        """the scalar's force on the fluid from the next step on (AdeBuoyancy, or None: the passive scalar)"""
        self.lib.ade_solver_set_buoyancy(self.h, ct.byref(buoyancy) if buoyancy is not None else None)
        self.buoyancy = buoyancy

    def set_buoyancy_m(self, buoyancy):
        """set_buoyancy for either fluid (lbm_ade_solver_set_buoyancy_m): with a KBC fluid the forced KBC collision --
        kbc::collide on the held moments (rho, u0 + u_shift F), guo not read; with a BGK fluid set_buoyancy itself"""
        self.lib.ade_solver_set_buoyancy_m(self.h, ct.byref(buoyancy) if buoyancy is not None else None)
        self.buoyancy = buoyancy

    def set_walls(self, walls):
        """the interior walls from the next stream on (a finalized AdeInteriorWalls, or None: none); borrowed, not copied"""
        self.lib.ade_solver_set_walls(self.h, walls.h if walls is not None else None)
        self.walls = walls  # keeps the table alive

    def set_open(self, table):
        """the open boundaries from the next step on (a finalized AdeOpenBoundary, or None: none); borrowed, not copied.
        A non-empty table is taken before the first step or before set_state only."""
        self.lib.ade_solver_set_open(self.h, table.h if table is not None else None)
        self.open = table  # keeps the table alive

    def set_open_m(self, table):
        """set_open for either fluid (lbm_ade_solver_set_open_m): with a KBC fluid the open pass with that fluid's
        collision, the forced one under set_buoyancy_m; with a BGK fluid set_open itself"""
        self.lib.ade_solver_set_open_m(self.h, table.h if table is not None else None)
        self.open = table  # keeps the table alive

    def close(self):
        if self.h:
            self.lib.ade_solver_destroy(self.h)
            self.h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, f, g):
        """f_adve, g_adve as [R, C, 9]"""
        f = np.ascontiguousarray(f, dtype=np.float64)
        g = np.ascontiguousarray(g, dtype=np.float64)
        assert f.shape == (self.R, self.C, 9) and g.shape == (self.R, self.C, 9)
        self.lib.ade_solver_set_state(self.h, _hptr(f), _hptr(g))

    def step(self, n):
        self.lib.ade_solver_step(self.h, int(n))

    def get_state(self):
        """dict f, g [R, C, 9], rho [R, C], u [R, C, 2], C [R, C]: what the reference loop holds"""
        R, C = self.R, self.C
        out = dict(f=np.empty((R, C, 9)), g=np.empty((R, C, 9)), rho=np.empty((R, C)), u=np.empty((R, C, 2)),
                   C=np.empty((R, C)))
        self.lib.ade_solver_get_state(self.h, *[_hptr(out[k]) for k in ("f", "g", "rho", "u", "C")])
        return out

    def sync(self):
        self.lib.ade_solver_sync(self.h)

    def diag(self, profile=None, row_begin=0, row_end=None, table=False):
        """the DIAG_NQ diagnostics of rho, u, C of the streamed state (what get_state returns), reduced on the device;
        profile: a device array [C] for DIAG_SUM_DEV2; table=True: (values, row table)"""
        return _diag(self.lib.ade_solver_diag, self.h, self.R, profile, row_begin, row_end, table)

    def run_until(self, converge, max_steps):
        """step until the rule of `converge` (Converge) fires or max_steps are done: (steps_done, converged, last_value)"""
        return _run_until(self.lib.ade_solver_run_until, self.h, self.R, converge, max_steps)

    def wall_exchange(self, region=None, row_begin=0, row_end=None, table=False):
        """the WALLX_NQ values of what the interior walls take in the stream get_state shows (force on them, fluid mass,
        scalar uptake), over rows [row_begin, row_end); region = (r0, r1, c0, c1): the nodes of that box only (clipped to
        the lattice); table=True: (values, row table [WALLX_NQ, R])"""
        out = np.empty(WALLX_NQ)
        tab = np.empty((WALLX_NQ, self.R)) if table else None
        box = (ct.c_int * 4)(*[int(v) for v in region]) if region is not None else None
        self.lib.ade_solver_wall_exchange(self.h, box, int(row_begin), int(self.R if row_end is None else row_end),
                                          _hptr(out), _hptr(tab) if table else None)
        return (out, tab) if table else out

    def wall_exchange_m(self, region=None, row_begin=0, row_end=None, table=False):
        """wall_exchange for either fluid (lbm_ade_solver_wall_exchange_m): with a KBC fluid the FIXED slots see that
        collision's u (the unshifted u0 under buoyancy); with a BGK fluid wall_exchange itself"""
        out = np.empty(WALLX_NQ)
        tab = np.empty((WALLX_NQ, self.R)) if table else None
        box = (ct.c_int * 4)(*[int(v) for v in region]) if region is not None else None
        self.lib.ade_solver_wall_exchange_m(self.h, box, int(row_begin), int(self.R if row_end is None else row_end),
                                            _hptr(out), _hptr(tab) if table else None)
        return (out, tab) if table else out

    def launches(self):
        return int(self.lib.raw.lbm_ade_solver_launches(self.h))

    def lattices(self):
        """device addresses (f_cur, g_cur, f_other, g_other) and the padded geometry"""
        p = [_dp() for _ in range(4)]
        g = Geom()
        self.lib.ade_solver_lattices(self.h, *[ct.byref(x) for x in p], ct.byref(g))
        return tuple(ct.cast(x, ct.c_void_p).value for x in p) + (g,)


def cg_params(red=(3.0, 0.7, 0.04, 0.7), blue=(1.0, 0.1, 0.04, -0.7), sigma=0.1, gravity=6.25e-6,
              delta=0.1, gravity_c=0.0, add_source=1, form=FORM_DEFAULT):
    """[red]/[blue] of mrtcg-rayleigh-taylor-gamma3.toml as (rho_0, alpha, nu, beta); sigma and
    gravity are this build's recorded choices for the keys the shipped TOML lacks."""
    return CgParams(CgColour(*red), CgColour(*blue), sigma, gravity, gravity_c, add_source, delta, form)


class CgSolver:
    """Python face of lbm_cg_solver: the two-phase driver loop, numpy AoS in/out."""

    def __init__(self, lib, R, C, params, bc=None, stream=None):
        self.lib, self.R, self.C, self.params = lib, R, C, params
        self.g = Geom(R, C, 0)
        self.h = ct.c_void_p()
        lib.cg_solver_create(ct.byref(self.h), ct.byref(self.g), ct.byref(bc) if bc is not None else None,
                             ct.byref(params), _stream(stream))

    def close(self):
        if self.h:
            self.lib.cg_solver_destroy(self.h)
            self.h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, f_r, f_b, rho_r, rho_b, u):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (f_r, f_b, rho_r, rho_b, u)]
        self.lib.cg_solver_set_state(self.h, *[_hptr(a) for a in arrs])

    def step(self, n):
        self.lib.cg_solver_step(self.h, int(n))

    def get_state(self):
        R, C = self.R, self.C
        out = dict(f_r=np.empty((R, C, 9)), f_b=np.empty((R, C, 9)), rho_r=np.empty((R, C)),
                   rho_b=np.empty((R, C)), u=np.empty((R, C, 2)), psi=np.empty((R, C)),
                   s_nu=np.empty((R, C)))
        self.lib.cg_solver_get_state(self.h, *[_hptr(out[k]) for k in
                                               ("f_r", "f_b", "rho_r", "rho_b", "u", "psi", "s_nu")])
        return out


class Ibm:
    """Python face of lbm_ibm (immersed boundary, stationary markers)."""

    def __init__(self, lib, x, y, X, Y, m_max=5, row_offset=0):
        self.lib = lib
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        self.h = ct.c_void_p()
        lib.ibm_create_slab(ct.byref(self.h), _hptr(x), _hptr(y), len(x), int(m_max), int(X), int(Y),
                            int(row_offset))

    def roi(self):
        v = [ct.c_int() for _ in range(4)]
        self.lib.ibm_roi(self.h, *[ct.byref(i) for i in v])
        return tuple(i.value for i in v)

    def surface_force(self, stream=None):
        out = np.zeros(2)
        self.lib.ibm_surface_force(self.h, _hptr(out), _stream(stream))
        return out

    def close(self):
        if self.h:
            self.lib.ibm_destroy(self.h)
            self.h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SlabIbm:
    """Python face of lbm_slab_ibm: one BGK row slab of a domain with an immersed boundary, advanced in
    blocks of `depth` steps (capi_slab_ibm.hip).  The transport between slabs is the caller's."""

    def __init__(self, lib, geom, slab_row0, rows_global, bc_global, prm, depth, x, y, m_max=5,
                 guo=(1.0 / 3.0, 1.0 / 9.0)):
        self.lib, self.geom = lib, geom
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        self.h = ct.c_void_p()
        lib.slab_ibm_create(ct.byref(self.h), ct.byref(geom), int(slab_row0), int(rows_global), ct.byref(bc_global),
                            ct.byref(prm), int(depth), _hptr(x), _hptr(y), len(x), int(m_max),
                            ct.c_double(guo[0]), ct.c_double(guo[1]))
        v = [ct.c_int() for _ in range(5)]
        lib.slab_ibm_info(self.h, *[ct.byref(i) for i in v])
        self.owner, self.straddle_prev, self.straddle_next, self.b0, self.b1 = (i.value for i in v)
        self.msg_doubles = int(lib.raw.lbm_slab_ibm_msg_doubles(self.h))

    def prime_counts(self, side):
        a, b = ct.c_longlong(), ct.c_longlong()
        self.lib.slab_ibm_prime_counts(self.h, int(side), ct.byref(a), ct.byref(b))
        return a.value, b.value

    def surface_force(self):
        out = np.zeros(2)
        self.lib.slab_ibm_surface_force(self.h, _hptr(out), None)
        return out

    def close(self):
        if self.h:
            self.lib.slab_ibm_destroy(self.h)
            self.h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
