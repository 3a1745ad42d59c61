"""The reference-order collision of a case of tests/exact_collide.py composed from the oracle's primitives: what
tests/test_exact_collide.py measures against the 80-bit yardstick and what the reference-order HIP kernels must equal
bitwise (tests/test_gpu_collision_accuracy.py).  Never calls the library under test."""
import numpy as np


def reference_order(orc, case, st):
    """(pop [n, 9 or 18], mom [n, 3 or 4]) of the oracle's reference-order collision of a case's states: calc_rho, calc_u,
    equilibrium, collision (the delta form as cylinder_test.cpp writes it), kbc_collide on the populations' own moments,
    the scalar composed as tests/ade_util.py collide does"""
    f = st["f"][None]                                   # the oracle's layout [R, C, 9] with R = 1
    rho = orc.calc_rho(f)
    u = orc.calc_u(f, rho)
    if case.cls.endswith("kbc"):
        fc = orc.kbc_collide(f, rho, u, case.fluid)[0]
    elif case.delta_form:
        fc = f + (-case.fluid * (f - orc.equilibrium(u, rho)))
    else:
        fc = orc.collision(f, orc.equilibrium(u, rho), case.fluid)
    pop, mom = [fc[0]], [rho[0][:, None], u[0]]
    if case.cls.startswith("ade"):
        g = st["g"][None]
        conc = orc.calc_rho(g)
        pop.append(orc.collision(g, orc.equilibrium(u + np.asarray(case.w), conc), case.omega_g)[0])
        mom.append(conc[0][:, None])
    return np.concatenate(pop, axis=1), np.concatenate(mom, axis=1)
