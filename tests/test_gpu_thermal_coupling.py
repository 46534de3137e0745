"""The fluid side of conjugate heat transfer on the device (reference DAOutputThermalCoupling.C, DAInputThermalCoupling.C; the calls of
DAFoamThermal, dafoam/mphys/mphys_dafoam.py:870-951).  thermalCouplingOutput: size, values and their determinism, the stateVar / volCoord /
patchVelocity / patchVar / field products and the errors, against the numpy restatement (tests/thermal_coupling_restatement.py).  The mixed T
patch field against the unmodified oracle; the thermalCoupling input: the fractions it sets and its products.  Tolerances: 1e-12 relative for values and 1e-10 relative for products, those of
tests/test_gpu_force_coupling.py; the volCoord and boundary-value criteria are the ones of that file too."""
import copy
import ctypes as C

import numpy as np
import pytest

import function_restatement_more as FM
import thermal_coupling_restatement as TC
from common import blocks, norm_states, options, relerr
from dafoam_amd import _capi
from dafoam_amd._capi import DASError
from dafoam_amd.meshgen import (BC_MIXED, BC_ZERO_GRADIENT, channel_case, rho_channel_case, scalar_transport_case, simple_T_channel_case,
                                turbo_channel_case, with_mixed_T)
from mixed_mesh import mixed
from oracle import jacobian as J
from oracle.foam_mesh import Geometry
from oracle.residual import residual
from test_gpu_functions_more import local_gradients, moved_case

pytestmark = pytest.mark.gpu

OUT = "thermalCouplingOutput"
CASES = ["simpleT", "rho", "turbo", "mixed"]
PATCHES = ["inlet", "bottom"]  # as the user lists them - not sorted; the two patches share a row of cells


def build_case(which):
    """6 x 5 x 4 channels with wall functions on the walls; the 148-cell pyramid / prism / polyhedron mesh as DARhoSimpleFoam."""
    if which == "mixed":
        return mixed("rho", wall_function=True)
    return {"simpleT": simple_T_channel_case, "rho": rho_channel_case, "turbo": turbo_channel_case}[which](6, 5, 4, wall_function=True, perturb=0.02)


def info(patches):
    return {"type": OUT, "patches": list(patches), "components": ["thermalCoupling"]}  # reference dafoam/mphys/mphys_dafoam.py:888


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=options(case, **extra), case=case)


def seeds_for(n, count=3):
    return np.random.default_rng(11).standard_normal((count, n))


# ---- 1: size, value, determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", TC.MODES)
@pytest.mark.parametrize("which", CASES)
def test_size_value_and_determinism(which, mode):
    case = build_case(which)
    g = Geometry(case.mesh)
    S = make(case, outputInfo={"q": info(PATCHES)}, wallDistanceMethod=mode).solver
    n = TC.size(case, PATCHES)
    nF = n // 2
    assert S.getOutputSize("q", OUT) == n and S.getOutputDistributed("q", OUT) == 1
    ref = TC.output(case, g, case.states, PATCHES, mode)
    a, b = np.zeros(n), np.ones(n)
    S.calcOutput("q", OUT, a)
    S.calcOutput("q", OUT, b)
    assert np.array_equal(a, b)
    assert np.array_equal(a[:nF], ref[:nF])  # T of the owner cells: copied
    err = np.abs(a[nF:] - ref[nF:]).max() / np.abs(ref[nF:]).max()
    print(f"{which} {mode}: {n} entries, kappa / d max abs err / max = {err:.2e}")
    assert ref[nF:].min() > 0 and err <= 1e-12
    other = TC.output(case, g, case.states, PATCHES, TC.MODES[1 - TC.MODES.index(mode)])
    if which != "mixed":  # perturbed hexahedra: the two distances differ, so the mode is seen
        assert np.abs(other[nF:] / ref[nF:] - 1.0).max() > 1e-6


# ---- 2: stateVar ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,mode", [("simpleT", "default"), ("rho", "daCustom"), ("turbo", "default"), ("mixed", "default")])
def test_state_product(which, mode):
    case = build_case(which)
    g = Geometry(case.mesh)
    D = make(case, outputInfo={"q": info(PATCHES)}, wallDistanceMethod=mode)
    W = case.states
    sc = J.state_scales(case, g, norm_states(case))
    n = TC.size(case, PATCHES)
    Sd = seeds_for(n)
    Sd[2, : n // 2] = 0.0  # the second half alone: T, p and nuTilda of the owner cell through mu_b, rho_b and nut_b
    grads = local_gradients(lambda Wp: Sd @ TC.output(case, g, Wp, PATCHES, mode), case, g, W, sc, sorted(PATCHES))
    for seeds, dFo in zip(Sd, grads):
        prod = np.zeros(W.size)
        D.solverAD.calcJacTVecProduct("states", "stateVar", W, "q", OUT, seeds, prod)
        err = np.abs(prod - dFo).max() / np.abs(dFo).max()
        print(f"{which} {mode}: d(seeds . q)/dW rel max err {err:.2e}")
        assert dFo.any() and err <= 1e-10


# ---- 3: volCoord --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,mode", [("simpleT", "default"), ("simpleT", "daCustom"), ("rho", "default"), ("mixed", "daCustom")])
def test_volcoord_product(which, mode):
    """The criterion of check_volcoord (tests/test_gpu_functions_more.py), with a tenth of its step: kappa / d goes like 1 / d, and on the
    small pyramids of the mixed mesh the truncation error (h / d)^2 of a central difference with that file's step reaches 1e-8 of the terms
    of product . dX, which cancel to a hundredth of their size in some directions.  (Measured: the difference approaches the product like
    h^2, down to 2e-12 relative at this step.)  The first half does not see the points; the seeds of the second half carry the product."""
    case = build_case(which)
    D = make(case, outputInfo={"q": info(PATCHES)}, inputInfo={"x": {"type": "volCoord"}}, wallDistanceMethod=mode)
    S = D.solverAD
    X0 = np.zeros(S.getNLocalPoints() * 3)
    S.getOFMeshPoints(X0)
    rng = np.random.default_rng(5)
    h = 1e-7 * np.abs(X0).max()
    n = TC.size(case, PATCHES)
    for seeds in seeds_for(n, 2):
        prod = np.zeros(X0.size)
        S.calcJacTVecProduct("x", "volCoord", X0, "q", OUT, seeds, prod)
        for _ in range(2):
            dX = rng.standard_normal(X0.size)
            vals = []
            for sgn in (1.0, -1.0):
                c = moved_case(case, X0 + sgn * h * dX)
                vals.append(seeds @ TC.output(c, Geometry(c.mesh), case.states, PATCHES, mode))
            fd = (vals[0] - vals[1]) / (2 * h)
            print(f"{which} {mode}: product {prod @ dX!r} central difference {fd!r}")
            assert fd != 0.0 and abs(prod @ dX - fd) <= 1e-6 * max(abs(fd), 1e-12 * np.abs(prod).max() * np.abs(dX).max())
    only_T = np.concatenate([np.ones(n // 2), np.zeros(n // 2)])
    prod = np.ones(X0.size)
    S.calcJacTVecProduct("x", "volCoord", X0, "q", OUT, only_T, prod)
    assert np.all(prod == 0.0)


def test_volcoord_fd_mode_is_rejected_by_name():
    case = build_case("simpleT")
    D = make(case, outputInfo={"q": info(PATCHES)}, inputInfo={"x": {"type": "volCoord"}}, amd={"volCoordMode": "fd"})
    X0 = case.mesh.points.ravel().copy()
    with pytest.raises(DASError, match="thermalCouplingOutput needs amd.volCoordMode dual"):
        D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "q", OUT, np.ones(TC.size(case, PATCHES)), np.zeros(X0.size))


# ---- 4: boundary-value and field inputs -----------------------------------------------------------------------------------------------------
def with_bc(bcs, patch, field, value):
    out = copy.deepcopy(bcs)
    out[patch][field] = (bcs[patch][field][0], value)
    return out


def test_patch_var_and_field_inputs():
    """The oracle's patch table holds real numbers, so no complex step reaches a patch value: central differences at 1e-6 relative, as in
    tests/test_gpu_force_coupling.py.  T of the owner cells reads no boundary value and would only add a constant of the size of 300 |seeds|
    to both sides of every difference, so the seeds of the first half are zero here.  On the compressible channel T_b and p_b set rho_b of the
    inlet and outlet faces and through it the turbulent part of alphaEff_b: those products are not zero.  A fixedValue inlet velocity reaches
    neither T_c nor alphaEff_b (nut_b of the inlet is nuTilda_b fv1; the wall function reads the wall's own velocity): exactly zero on both
    sides.  The output does not read betaFINuTilda: that product is exactly zero, as for the patch functions."""
    case = build_case("rho")
    patches = ["outlet", "inlet", "bottom"]
    g = Geometry(case.mesh)
    W = case.states
    D = make(case, outputInfo={"q": info(patches)},
             inputInfo={"TIn": {"type": "patchVar", "patches": ["inlet"], "varName": "T", "varType": "scalar"},
                        "pOut": {"type": "patchVar", "patches": ["outlet"], "varName": "p", "varType": "scalar"},
                        "UIn": {"type": "patchVar", "patches": ["inlet"], "varName": "U", "varType": "vector"},
                        "beta": {"type": "field", "fieldName": "betaFINuTilda", "fieldType": "scalar"}})
    S = D.solverAD
    n = TC.size(case, patches)
    inputs = [("TIn", "patchVar", np.array([310.0]), lambda bcs, x: with_bc(bcs, "inlet", "T", float(x[0])), (1e-2,), True),
              ("pOut", "patchVar", np.array([1.0e5]), lambda bcs, x: with_bc(bcs, "outlet", "p", float(x[0])), (10.0,), True),
              ("UIn", "patchVar", np.array([50.0, 0.4, -0.2]), lambda bcs, x: with_bc(bcs, "inlet", "U", tuple(x)), (1e-3, 1e-3, 1e-3), False)]
    bcs = case.bcs  # the patch table as the inputs set so far have left it
    for seeds in seeds_for(n, 2):
        seeds[: n // 2] = 0.0
        restated = lambda table: seeds @ TC.output(case, g, W, patches, "default", table)  # noqa: E731
        for name, typ, x0, bcs_of, steps, seen in inputs:
            prod = np.ones(x0.size)
            S.calcJacTVecProduct(name, typ, x0, "q", OUT, seeds, prod)
            F0 = restated(bcs_of(bcs, x0))
            out = np.zeros(n)
            S.calcOutput("q", OUT, out)  # the input stays set: the value follows it
            assert abs(seeds @ out - F0) <= 1e-11 * np.abs(seeds * out).sum(), name
            for k, h in enumerate(steps):
                e = np.eye(x0.size)[k]
                fd = (restated(bcs_of(bcs, x0 + h * e)) - restated(bcs_of(bcs, x0 - h * e))) / (2 * h)
                print(f"{name}[{k}]: product {prod[k]!r} central difference {fd!r}")
                if seen:
                    assert fd != 0.0 and abs(prod[k] - fd) <= 1e-6 * abs(fd), (name, k, prod[k], fd)
                else:
                    assert fd == 0.0 and prod[k] == 0.0, (name, k, prod[k], fd)
            bcs = bcs_of(bcs, x0)
        beta = np.ones(g.nC)
        S.calcJacTVecProduct("beta", "field", np.ones(g.nC), "q", OUT, seeds, beta)
        assert np.all(beta == 0.0)


def test_patch_velocity_input_is_accepted():
    """patchVelocity on the inlet of the DASimpleFoam channel: the input is applied and its product is exactly zero, as the restatement
    says (see test_patch_var_and_field_inputs)."""
    case = build_case("simpleT")
    g = Geometry(case.mesh)
    patches = ["inlet", "bottom"]
    D = make(case, outputInfo={"q": info(patches)},
             inputInfo={"patchV": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "y"}})
    seeds = seeds_for(TC.size(case, patches), 1)[0]
    x0 = np.array([10.0, 3.0])
    prod = np.ones(2)
    D.solverAD.calcJacTVecProduct("patchV", "patchVelocity", x0, "q", OUT, seeds, prod)
    vals = []
    for um in (10.0, 11.0):
        a = 3.0 * np.pi / 180.0
        vals.append(seeds @ TC.output(case, g, case.states, patches, "default", with_bc(case.bcs, "inlet", "U", (um * np.cos(a), um * np.sin(a), 0.0))))
    assert vals[0] == vals[1] and np.all(prod == 0.0)


# ---- 5: errors ------------------------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_problem():
    small = simple_T_channel_case(4, 4, 3)
    D = make(small, outputInfo={"q": info(PATCHES)})
    S = D.solverAD
    n = TC.size(small, PATCHES)
    W = small.states
    with pytest.raises(DASError, match="thermalCouplingOutput not defined: g"):
        S.getOutputSize("g", OUT)
    with pytest.raises(DASError, match="thermalCouplingOutput not defined: g"):
        S.calcJacTVecProduct("states", "stateVar", W, "g", OUT, np.ones(n), np.zeros(W.size))
    with pytest.raises(AssertionError, match="invalid seed array size"):
        S.calcJacTVecProduct("states", "stateVar", W, "q", OUT, np.ones(n - 2), np.zeros(W.size))
    with pytest.raises(AssertionError, match="invalid array size"):
        S.calcOutput("q", OUT, np.zeros(n + 2))
    with pytest.raises(DASError, match="patch wing is not in the mesh"):
        make(small, outputInfo={"q": info(["bottom", "wing"])})
    with pytest.raises(DASError, match="discipline aero only"):
        make(small, outputInfo={"q": info(PATCHES)}, discipline="thermal")
    with pytest.raises(DASError, match="wallDistanceMethod: meshWave not supported! Options are: default and daCustom."):
        make(small, outputInfo={"q": info(PATCHES)}, wallDistanceMethod="meshWave")
    for case in (channel_case(4, 4, 3), scalar_transport_case(4, 4, 3)):
        with pytest.raises(NotImplementedError, match="thermalCouplingOutput and the thermalCoupling input. is not built for solvers without a T field"):
            make(case, outputInfo={"q": info(["inlet"])})
    # a sharded solver: the owned-cell mask of dafoam_amd.distributed is set after the construction, so the output says so when it is used
    mask = np.ones(W.size, dtype=np.uint8)
    _capi.check(_capi.lib().das_set_owned_mask(S._h, mask.ctypes.data_as(C.POINTER(C.c_ubyte))))
    with pytest.raises(DASError, match="thermalCouplingOutput runs on an undecomposed solver"):
        S.calcOutput("q", OUT, np.zeros(n))


# ---- 6: the mixed T patch field against the unmodified oracle -----------------------------------------------------------------------------------
WALL = "bottom"
TB, TC_STAR = 320.0, 305.0


def wall_faces(case):
    return TC.selected_faces(case, [WALL])


def uniform_wall_state(case, rng):
    """The case with T of the owner cells of the wall set to one value, and per-face (refValue, valueFraction), the fractions spread over
    (0.1, 0.9), chosen so that f ref + (1 - f) T_c is TB on every face: the mixed wall then hands the equations what a fixedValue TB does."""
    N = case.mesh.n_cells
    c = copy.copy(case)
    c.states = case.states.copy()
    c.states[4 * N + case.mesh.owner[wall_faces(case)]] = TC_STAR
    f = 0.1 + 0.8 * rng.random(wall_faces(case).size)
    return c, (TB - (1.0 - f) * TC_STAR) / f, f


def device_residual(case):
    R = np.zeros(case.states.size)
    make(case).solver.getResiduals(R)
    return R


@pytest.mark.parametrize("which", ["simpleT", "rho", "turbo"])
def test_mixed_residual_is_the_oracle_residual_of_the_equivalent_patch(which):
    """Fraction 1 is fixedValue, fraction 0 is zeroGradient, and in between a wall whose faces all come to the boundary value TB is the
    fixedValue TB wall - each against the unmodified oracle, block by block at the 1e-12 of tests/test_gpu_parity.py."""
    base = build_case(which)
    g = Geometry(base.mesh)
    zero_gradient = copy.copy(base)
    zero_gradient.bcs = copy.deepcopy(base.bcs)
    zero_gradient.bcs[WALL]["T"] = (BC_ZERO_GRADIENT, 0.0)
    mid, ref, f = uniform_wall_state(base, np.random.default_rng(6))
    assert f.min() > 0.1 and f.max() < 0.9 and f.max() - f.min() > 0.5 and np.abs(ref - TB).max() > 1.0
    pairs = [("fraction 1", with_mixed_T(base, WALL, TB, 1.0), TC.as_fixed_value(base, [WALL], [TB])),
             ("fraction 0", with_mixed_T(base, WALL, 123.0, 0.0), zero_gradient),
             ("in between", with_mixed_T(mid, WALL, ref, f), TC.as_fixed_value(mid, [WALL], [TB]))]
    # the test can fail: the oracle's residuals of the fixedValue and the zeroGradient wall differ by far more than the bar
    Ra, Rb = residual(pairs[0][2], g, base.states), residual(pairs[1][2], g, base.states)
    sl = dict(blocks(base, g))["T"]
    assert relerr(Ra[sl], Rb[sl]) > 1e-6  # a million times the bar
    assert relerr(residual(pairs[2][2], g, mid.states)[sl], residual(TC.as_fixed_value(mid, [WALL], [TB + 1.0]), g, mid.states)[sl]) > 1e-6
    for label, dev, orc in pairs:
        R, Ro = device_residual(dev), residual(orc, g, dev.states)
        for nm, s_ in blocks(base, g):
            print(f"{which} {label} {nm}: rel err {relerr(R[s_], Ro[s_]):.2e}")
            assert relerr(R[s_], Ro[s_]) < 1e-12, (label, nm)


@pytest.mark.parametrize("which", ["simpleT", "rho"])
def test_mixed_jacobian_transpose_and_adjoint_solve(which):
    """With a mixed wall of non-trivial fractions: psi . (dR/dW (s o v)) = v . (s o dRdW^T psi) - the forward-mode product against the
    assembled transposed one - and a GMRES adjoint solve that converges."""
    mid, ref, f = uniform_wall_state(build_case(which), np.random.default_rng(6))
    ref = ref + np.random.default_rng(7).standard_normal(ref.size)  # the faces no longer agree on a boundary value
    case = with_mixed_T(mid, WALL, ref, f)
    D = make(case, adjEqnOption={"gmresRelTol": 1e-10, "printInfo": 0})
    S = D.solverAD
    W = case.states
    rng = np.random.default_rng(4)
    for _ in range(2):
        psi, v = rng.standard_normal(W.size), rng.standard_normal(W.size)
        JTpsi, Jv = np.zeros(W.size), np.zeros(W.size)
        S.calcJacTVecProduct("states", "stateVar", W, "residuals", "residual", psi, JTpsi)
        S.calcJacVecProduct(v, Jv)
        lhs, rhs = psi @ Jv, v @ JTpsi
        print(f"{which}: psi . (J v) = {lhs!r}, v . (J^T psi) = {rhs!r}, rel {abs(lhs - rhs) / abs(rhs):.2e}")
        assert rhs != 0.0 and abs(lhs - rhs) <= 1e-10 * abs(rhs)
    rhs = rng.standard_normal(W.size)
    psi, fail = D.solveAdjoint(rhs)
    assert fail == 0 and np.isfinite(psi).all()


# ---- 7: the thermalCoupling input ---------------------------------------------------------------------------------------------------------------
IN = "thermalCoupling"
HFX = {"type": "wallHeatFlux", "source": "patchToFace", "patches": ["bottom", "inlet"], "scale": 2.0, "byUnitArea": False}


def split(case, patches, a):
    """{patch: its part} of an array over the faces of the sorted patches."""
    sizes = {p.name: p.size for p in case.mesh.patches}
    out, at = {}, 0
    for nm in sorted(patches):
        out[nm] = a[at : at + sizes[nm]]
        at += sizes[nm]
    return out


def complex_step_gradient(fun, x):
    out = np.zeros(x.size)
    for k in range(x.size):
        xp = x.astype(np.complex128)
        xp[k] += 1e-30j * abs(x[k])
        out[k] = fun(xp).imag / (1e-30 * abs(x[k]))
    return out


@pytest.mark.parametrize("which,mode", [("simpleT", "daCustom"), ("rho", "default")])
def test_input_sets_the_fractions_and_its_products(which, mode):
    """The inlet and the wall, which share a row of corner cells, start as mixed patches of fraction 1 - fixedValue patches to the
    restatement.  Setting the input: refValue is the first half, valueFraction = nk / (myK + nk) at 1e-12, myK this side's kappa / d at the
    boundary values the patches had before the call (on the compressible solvers it reads T_b through rho_b, so every call that applies the
    input again moves it a little; the restatement follows call by call).  The products to the output, to a wallHeatFlux function and
    (DASimpleFoam: T is passive, the restated T rows are the whole dependence) to the residual against complex steps through the
    restatement, in which a mixed face is the fixedValue face of value f ref + (1 - f) T_c with f = nk / (myK + nk) and myK frozen -
    1e-10 relative.  Two solvers given the same calls return the same bits."""
    base = build_case(which)
    g = Geometry(base.mesh)
    W = base.states
    N = g.nC
    start = {"bottom": 320.0, "inlet": 300.0}
    dev = base
    for nm, v in start.items():
        dev = with_mixed_T(dev, nm, v, 1.0)
    fixed = TC.as_fixed_value(base, PATCHES)
    n = TC.size(base, PATCHES)
    nF = n // 2
    rng = np.random.default_rng(8)
    orc0 = TC.as_fixed_value(base, sorted(start), [start[nm] for nm in sorted(start)])
    myK0 = TC.output(orc0, g, W, PATCHES, mode)[nF:]
    x = np.concatenate([300.0 + 20.0 * rng.random(nF), myK0 * (0.2 + 3.0 * rng.random(nF))])
    seeds = seeds_for(n, 1)[0]
    psi = np.random.default_rng(3).standard_normal(W.size)

    def values(xx, myK):  # the boundary values of T the input xx leaves behind when this side's kappa / d was myK
        f = split(base, PATCHES, xx[nF:] / (myK + xx[nF:]))
        return TC.mixed_T_values(fixed, g, W, {nm: (r, f[nm]) for nm, r in split(base, PATCHES, xx[:nF]).items()})

    checks = [("q", OUT, seeds, lambda xx, myK: seeds @ TC.output(fixed, g, W, PATCHES, mode, None, values(xx, myK)), which == "rho"),
              ("HFX", "function", np.array([1.5]), lambda xx, myK: 1.5 * FM.wall_heat_flux(fixed, g, W, HFX, mode, values(xx, myK)), True)]
    if which == "simpleT":
        checks.append(("residuals", "residual", psi, lambda xx, myK: psi[4 * N : 5 * N] @ TC.simple_T_rows(fixed, g, W, values(xx, myK)), True))

    def calls(S):
        assert S.getInputSize("cht", IN) == n and S.getInputDistributed("cht", IN) == 1
        S.setSolverInput("cht", IN, n, x)
        got = [S.getPatchMixedT(nm) for nm in sorted(PATCHES)]
        out = [np.concatenate([a for a, _ in got]), np.concatenate([b for _, b in got])]
        for name, typ, sd, _, _ in checks:
            prod = np.ones(n)
            S.calcJacTVecProduct("cht", IN, x, name, typ, sd, prod)
            out.append(prod)
        R = np.zeros(W.size)
        S.getResiduals(R)
        return out + [R]

    opts = dict(inputInfo={"cht": {"type": IN, "patches": PATCHES, "components": ["solver"]}}, outputInfo={"q": info(PATCHES)}, function={"HFX": HFX},
                wallDistanceMethod=mode)
    first, second = calls(make(dev, **opts).solverAD), calls(make(dev, **opts).solverAD)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)  # no atomics: the same bits
    ref, frac = first[0], first[1]
    f0 = TC.fraction(orc0, g, W, PATCHES, x[nF:], mode)
    print(f"{which} {mode}: fractions {frac.min():.3f} .. {frac.max():.3f}, max rel err {np.abs(frac / f0 - 1).max():.2e}")
    assert np.array_equal(ref, x[:nF]) and np.abs(frac - f0).max() <= 1e-12 * np.abs(f0).max() and f0.max() - f0.min() > 0.3
    myK = myK0
    for (name, typ, sd, fun, seen), prod in zip(checks, first[2:]):
        myK = TC.output(fixed, g, W, PATCHES, mode, None, values(x, myK))[nF:].real  # the product applies the input again
        grad = complex_step_gradient(lambda xx: fun(xx, myK), x)
        if not seen:  # DASimpleFoam: neither T_c nor nu / Pr + nut_b / Prt reads a boundary value of T
            assert not grad.any() and not prod.any(), name
            continue
        err = np.abs(prod - grad).max() / np.abs(grad).max()
        print(f"{which} {mode} -> {typ}: rel max err {err:.2e}; |d/d ref| max {np.abs(grad[:nF]).max():.3e}, |d/d nk| max {np.abs(grad[nF:]).max():.3e}")
        assert grad[:nF].any() and grad[nF:].any() and err <= 1e-10, name
    assert (which == "rho") == bool(np.abs(myK / myK0 - 1.0).max() > 1e-9)  # only the compressible kappa / d reads T_b
    # the value follows the input: the device's T rows are the restated ones
    if which == "simpleT":
        assert relerr(first[-1][4 * N : 5 * N], TC.simple_T_rows(fixed, g, W, values(x, myK)).real) < 1e-12


def test_input_residual_product_on_the_compressible_channel():
    """Where T is no passive scalar the restatement has no rows to differentiate; the oracle's patch table takes one real number per patch.
    So the wall is brought to one boundary value as in the residual test above, through the input itself, and the product is contracted
    with the two directions of the input that raise that boundary value uniformly: d ref_f = 1 / f_f, and
    d nk_f = 1 / ((ref_f - T_c) d f_f / d nk_f).  Both must equal the central difference of psi . R of the oracle in the fixedValue of the
    wall - at the 1e-6 of the boundary-value products of tests/test_gpu_force_coupling.py."""
    base = build_case("rho")
    g = Geometry(base.mesh)
    mid, _, _ = uniform_wall_state(base, np.random.default_rng(6))
    W = mid.states
    dev = with_mixed_T(mid, WALL, TB, 1.0)
    D = make(dev, inputInfo={"cht": {"type": IN, "patches": [WALL], "components": ["solver"]}})
    S = D.solverAD
    nF = wall_faces(base).size
    myK = TC.output(TC.as_fixed_value(mid, [WALL], [TB]), g, W, [WALL])[nF:]
    nk = myK * (0.2 + 3.0 * np.random.default_rng(8).random(nF))
    f = nk / (myK + nk)
    ref = (TB - (1.0 - f) * TC_STAR) / f
    x = np.concatenate([ref, nk])
    psi = np.random.default_rng(3).standard_normal(W.size)
    prod = np.zeros(2 * nF)
    S.calcJacTVecProduct("cht", IN, x, "residuals", "residual", psi, prod)
    R = np.zeros(W.size)
    S.getResiduals(R)
    for nm, s_ in blocks(base, g):  # the input has produced the fixedValue TB wall
        assert relerr(R[s_], residual(TC.as_fixed_value(mid, [WALL], [TB]), g, W)[s_]) < 1e-12, nm
    h = 1e-3
    fd = psi @ (residual(TC.as_fixed_value(mid, [WALL], [TB + h]), g, W) - residual(TC.as_fixed_value(mid, [WALL], [TB - h]), g, W)) / (2 * h)
    by_ref = prod[:nF] @ (1.0 / f)
    by_nk = prod[nF:] @ (1.0 / ((ref - TC_STAR) * myK / (myK + nk) ** 2))
    print(f"psi . dR / d TB: central difference {fd!r}, through refValue {by_ref!r}, through nk {by_nk!r}")
    assert fd != 0.0 and abs(by_ref - fd) <= 1e-6 * abs(fd) and abs(by_nk - fd) <= 1e-6 * abs(fd)


def test_input_and_mixed_errors_name_the_problem():
    base = build_case("simpleT")
    mixed_wall = with_mixed_T(base, WALL, TB, 1.0)
    entry = {"type": IN, "patches": [WALL], "components": ["solver"]}
    with pytest.raises(DASError, match="patch inlet does not carry a mixed T patch field"):
        make(mixed_wall, inputInfo={"cht": dict(entry, patches=["inlet", WALL])})
    with pytest.raises(DASError, match="patch wing is not in the mesh"):
        make(mixed_wall, inputInfo={"cht": dict(entry, patches=["wing"])})
    with pytest.raises(DASError, match="discipline aero only"):
        make(mixed_wall, inputInfo={"cht": entry}, discipline="thermal")
    with pytest.raises(DASError, match="wallDistanceMethod: meshWave not supported! Options are: default and daCustom."):
        make(mixed_wall, inputInfo={"cht": entry}, wallDistanceMethod="meshWave")
    with pytest.raises(NotImplementedError, match="without a T field"):
        make(channel_case(4, 4, 3), inputInfo={"cht": entry})
    for field in ("U", "p", "nuTilda"):
        c = copy.copy(base)
        c.bcs = copy.deepcopy(base.bcs)
        c.bcs[WALL][field] = (BC_MIXED, (0.0, 0.0, 0.0) if field == "U" else 0.0)
        with pytest.raises(DASError, match=f"patch {WALL}: the mixed patch field is built for T only, not for {field}"):
            make(c)
    S = make(mixed_wall, inputInfo={"cht": entry}).solverAD
    n = 2 * wall_faces(base).size
    with pytest.raises(DASError, match="thermalCoupling input cht has not been set"):
        _capi.check(_capi.lib().das_calc_dthermal_coupling_product(S._h, b"cht", b"residuals", b"residual", _capi.dptr(np.zeros(base.states.size)),
                                                                   _capi.dptr(np.zeros(n)), n))
    with pytest.raises(DASError, match="inputInfo has no entry other"):
        S.getInputSize("other", IN)
    mask = np.ones(base.states.size, dtype=np.uint8)
    _capi.check(_capi.lib().das_set_owned_mask(S._h, mask.ctypes.data_as(C.POINTER(C.c_ubyte))))
    with pytest.raises(DASError, match="runs on an undecomposed solver"):
        S.setSolverInput("cht", IN, n, np.ones(n))
