"""forceCouplingOutput on the device (reference DAOutputForceCoupling.C; the calls of DAFoamForces, dafoam/mphys/mphys_dafoam.py:1004-1104):
size, values and their determinism, the stateVar / volCoord / patchVelocity / patchVar / field products, the adjoint of the coupling
functional and the errors, against the numpy restatement (tests/force_coupling_restatement.py).  Tolerances: those of
tests/test_gpu_functions_more.py and tests/test_gpu_zz_flowdir.py."""
import copy

import numpy as np
import pytest

import force_coupling_restatement as FC
from common import norm_states, options
from dafoam_amd._capi import DASError
from dafoam_amd.meshgen import channel_case, rho_channel_case, scalar_transport_case, turbo_channel_case
from mixed_mesh import mixed
from oracle import jacobian as J
from oracle.foam_mesh import Geometry
from test_gpu_functions_more import local_gradients, moved_case

pytestmark = pytest.mark.gpu

OUT = "forceCouplingOutput"
CASES = ["simple", "rho", "turbo", "mixed"]


def build_case(which):
    """(case, patches as the user lists them - not sorted -, pRef).  The channels: a wall and the inlet, which share an edge of points.  The
    mixed mesh: walls on all four sides; front and back carry triangles next to quadrilaterals."""
    if which == "mixed":
        return mixed("simple", side_walls=True), ["front", "bottom", "back"], 7.5
    if which == "simple":
        return channel_case(6, 5, 4, wall_function=True, perturb=0.02), ["inlet", "bottom"], 7.5
    return (rho_channel_case if which == "rho" else turbo_channel_case)(6, 5, 4, wall_function=True, perturb=0.02), ["inlet", "bottom"], 9.0e4


def info(patches, pRef):
    return {"type": OUT, "patches": list(patches), "components": ["forceCoupling"], "pRef": pRef}  # reference tests/runRegTests_AeroStruct.py:110-117


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=options(case, **extra), case=case)


def seeds_for(n, count=3):
    return np.random.default_rng(11).standard_normal((count, n))


# ---- 1: size, value, determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CASES)
def test_size_value_and_determinism(which):
    case, patches, pRef = build_case(which)
    g = Geometry(case.mesh)
    if which == "mixed":  # the / nPoints factor takes both values
        assert set(np.diff(case.mesh.face_ptr)[FC.selected_faces(case, patches)]) >= {3, 4}
    fns = {"F" + "xyz"[d]: {"type": "force", "source": "patchToFace", "patches": patches, "directionMode": "fixedDirection",
                            "direction": list(np.eye(3)[d]), "scale": 1.0} for d in range(3)}
    D = make(case, function=fns, outputInfo={"f0": info(patches, 0.0), "f": info(patches, pRef)})
    S = D.solver
    n = FC.size(case, patches)
    assert S.getOutputSize("f", OUT) == n and S.getOutputSize("f0", OUT) == n
    assert S.getOutputDistributed("f", OUT) == 1
    f0o, fo = FC.nodal_forces(case, g, case.states, patches, 0.0), FC.nodal_forces(case, g, case.states, patches, pRef)
    out = {}
    for name, ref in (("f0", f0o), ("f", fo)):
        a, b = np.zeros(n), np.ones(n)
        S.calcOutput(name, OUT, a)
        S.calcOutput(name, OUT, b)
        err = np.abs(a - ref).max() / np.abs(ref).max()
        print(f"{which} {name}: {n} entries, max abs err / max |f| = {err:.2e}")
        assert np.array_equal(a, b), name
        assert np.abs(ref).max() > 0 and err <= 1e-12, name
        out[name] = a
    # a non-zero pRef shifts the result by the restated shift
    shift = FC.distribute(case, g, -pRef * g.bSf, patches)
    errs = np.abs(out["f"] - out["f0"] - shift).max() / np.abs(f0o).max()
    print(f"{which}: pRef shift, max abs err / max |f(pRef = 0)| = {errs:.2e}")
    assert np.abs(shift).max() > 0 and errs <= 1e-12
    # per component, the nodal forces add up to the force objective on the same patches
    for d in range(3):
        F = S.calcFunction("F" + "xyz"[d])
        tot = out["f0"].reshape(-1, 3)[:, d].sum()
        print(f"{which} component {d}: sum of nodal forces {tot!r} force function {F!r} rel {abs(tot - F) / abs(F):.2e}")
        assert F != 0.0 and abs(tot - F) <= 1e-12 * abs(F)


# ---- 2: stateVar ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", CASES)
def test_state_product(which):
    case, patches, pRef = build_case(which)
    g = Geometry(case.mesh)
    D = make(case, outputInfo={"f": info(patches, pRef)})
    W = case.states
    sc = J.state_scales(case, g, norm_states(case))
    Sd = seeds_for(FC.size(case, patches))
    grads = local_gradients(lambda Wp: Sd @ FC.nodal_forces(case, g, Wp, patches, pRef), case, g, W, sc, sorted(patches))
    for seeds, dFo in zip(Sd, grads):
        prod = np.zeros(W.size)
        D.solverAD.calcJacTVecProduct("states", "stateVar", W, "f", OUT, seeds, prod)
        err = np.abs(prod - dFo).max() / np.abs(dFo).max()
        print(f"{which}: d(seeds . f)/dW rel max err {err:.2e}")
        assert dFo.any() and err <= 1e-10


# ---- 3: volCoord --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["simple", "rho", "mixed"])
def test_volcoord_product(which):
    """The criterion of check_volcoord (tests/test_gpu_functions_more.py), with a non-zero pRef: the pRef dSf term is part of it."""
    case, patches, pRef = build_case(which)
    D = make(case, outputInfo={"f": info(patches, pRef)}, inputInfo={"x": {"type": "volCoord"}})
    S = D.solverAD
    X0 = np.zeros(S.getNLocalPoints() * 3)
    S.getOFMeshPoints(X0)
    rng = np.random.default_rng(5)
    h = 1e-6 * np.abs(X0).max()
    for seeds in seeds_for(FC.size(case, patches), 2):
        prod = np.zeros(X0.size)
        S.calcJacTVecProduct("x", "volCoord", X0, "f", OUT, seeds, prod)
        for _ in range(2):
            dX = rng.standard_normal(X0.size)
            vals = []
            for sgn in (1.0, -1.0):
                c = moved_case(case, X0 + sgn * h * dX)
                vals.append(seeds @ FC.nodal_forces(c, Geometry(c.mesh), case.states, patches, pRef))
            fd = (vals[0] - vals[1]) / (2 * h)
            print(f"{which}: product {prod @ dX!r} central difference {fd!r}")
            assert fd != 0.0 and abs(prod @ dX - fd) <= 1e-6 * max(abs(fd), 1e-12 * np.abs(prod).max() * np.abs(dX).max())


def test_volcoord_fd_mode_is_rejected_by_name():
    case, patches, pRef = build_case("simple")
    D = make(case, outputInfo={"f": info(patches, pRef)}, inputInfo={"x": {"type": "volCoord"}}, amd={"volCoordMode": "fd"})
    X0 = case.mesh.points.ravel().copy()
    with pytest.raises(DASError, match="amd.volCoordMode dual"):
        D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "f", OUT, np.ones(FC.size(case, patches)), np.zeros(X0.size))


# ---- 4: boundary-value and field inputs -----------------------------------------------------------------------------------------------------
def with_bc(bcs, patch, field, value):
    out = copy.deepcopy(bcs)
    out[patch][field] = (bcs[patch][field][0], value)
    return out


def test_patch_velocity_patch_var_and_field_inputs():
    """The oracle's patch table holds real numbers, so no complex step reaches a patch value: central differences, the project's 1e-6
    (tests/test_gpu_zz_flowdir.py).  The forces do not read betaFINuTilda: that product is exactly zero, as for the patch functions."""
    case, _, pRef = build_case("simple")
    patches = ["outlet", "inlet", "bottom"]
    g = Geometry(case.mesh)
    W = case.states
    D = make(case, outputInfo={"f": info(patches, pRef)},
             inputInfo={"patchV": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "y"},
                        "pOut": {"type": "patchVar", "patches": ["outlet"], "varName": "p", "varType": "scalar"},
                        "UIn": {"type": "patchVar", "patches": ["inlet"], "varName": "U", "varType": "vector"},
                        "beta": {"type": "field", "fieldName": "betaFINuTilda", "fieldType": "scalar"}})
    S = D.solverAD
    n = FC.size(case, patches)

    def inlet(bcs, x):
        a = x[1] * np.pi / 180.0
        return with_bc(bcs, "inlet", "U", (x[0] * np.cos(a), x[0] * np.sin(a), bcs["inlet"]["U"][1][2]))  # the third component stays

    inputs = [("patchV", "patchVelocity", np.array([10.0, 3.0]), inlet, (1e-4, 1e-3)),
              ("pOut", "patchVar", np.array([2.0]), lambda bcs, x: with_bc(bcs, "outlet", "p", float(x[0])), (1e-3,)),
              ("UIn", "patchVar", np.array([10.0, 0.4, -0.2]), lambda bcs, x: with_bc(bcs, "inlet", "U", tuple(x)), (1e-4, 1e-4, 1e-4))]
    bcs = case.bcs  # the patch table as the inputs set so far have left it
    for seeds in seeds_for(n, 2):
        restated = lambda table: seeds @ FC.nodal_forces(case, g, W, patches, pRef, table)  # noqa: E731
        for name, typ, x0, bcs_of, steps in inputs:
            prod = np.zeros(x0.size)
            S.calcJacTVecProduct(name, typ, x0, "f", OUT, seeds, prod)
            F0 = restated(bcs_of(bcs, x0))
            out = np.zeros(n)
            S.calcOutput("f", OUT, out)  # the input stays set: the value follows it
            assert abs(seeds @ out - F0) <= 1e-11 * np.abs(seeds * out).sum(), name
            for k, h in enumerate(steps):
                e = np.eye(x0.size)[k]
                fd = (restated(bcs_of(bcs, x0 + h * e)) - restated(bcs_of(bcs, x0 - h * e))) / (2 * h)
                print(f"{name}[{k}]: product {prod[k]!r} central difference {fd!r}")
                assert fd != 0.0 and abs(prod[k] - fd) <= 1e-6 * max(abs(fd), 1e-3 * abs(F0)), (name, k, prod[k], fd)
            bcs = bcs_of(bcs, x0)
        beta = np.ones(g.nC)
        S.calcJacTVecProduct("beta", "field", np.ones(g.nC), "f", OUT, seeds, beta)
        assert np.all(beta == 0.0)


# ---- 5: the adjoint of the coupling functional ------------------------------------------------------------------------------------------------
def test_adjoint_of_the_coupling_functional_matches_the_forward_product():
    """psi solves dR/dW^T psi = d(seeds . f)/dW, as DAFoamForces' seeds reach the adjoint.  For any state direction v,
    psi . (dR/dW (s o v)) = (s o d(seeds . f)/dW) . v: the left side through the device's forward-mode residual product, the right side the
    stateVar product itself.  (A finite difference of the oracle primal - three Newton solves with complex-step Jacobians - is left to
    test_total_pressure_ratio_adjoint_total_end_to_end; it takes longer than a test of this file should.)"""
    case, patches, pRef = build_case("simple")
    D = make(case, outputInfo={"f": info(patches, pRef)}, adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0})
    S = D.solverAD
    W = case.states
    seeds = seeds_for(FC.size(case, patches), 1)[0]
    dFdW = np.zeros(W.size)
    S.calcJacTVecProduct("states", "stateVar", W, "f", OUT, seeds, dFdW)
    psi, fail = D.solveAdjoint(dFdW)
    assert fail == 0
    rng = np.random.default_rng(4)
    for _ in range(2):
        v = rng.standard_normal(W.size)
        Jv = np.zeros(W.size)
        S.calcJacVecProduct(v, Jv)
        lhs, rhs = psi @ Jv, dFdW @ v
        print(f"psi . (dR/dW s o v) = {lhs!r}, (s o dF/dW) . v = {rhs!r}")
        assert rhs != 0.0 and abs(lhs - rhs) <= 1e-5 * abs(rhs)


# ---- 6: errors ------------------------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_problem():
    patches, pRef = ["inlet", "bottom"], 7.5
    small = channel_case(4, 4, 3)
    D = make(small, outputInfo={"f": info(patches, pRef)})
    S = D.solverAD
    n = FC.size(small, patches)
    W = small.states
    with pytest.raises(DASError, match="forceCouplingOutput not defined: g"):
        S.getOutputSize("g", OUT)
    with pytest.raises(DASError, match="forceCouplingOutput not defined: g"):
        S.calcJacTVecProduct("states", "stateVar", W, "g", OUT, np.ones(n), np.zeros(W.size))
    with pytest.raises(AssertionError, match="invalid seed array size"):
        S.calcJacTVecProduct("states", "stateVar", W, "f", OUT, np.ones(n - 3), np.zeros(W.size))
    with pytest.raises(AssertionError, match="invalid array size"):
        S.calcOutput("f", OUT, np.zeros(n + 3))
    no_pref = {k: v for k, v in info(patches, pRef).items() if k != "pRef"}
    with pytest.raises(DASError, match="needs pRef"):
        make(small, outputInfo={"f": no_pref})
    with pytest.raises(DASError, match="patch wing is not in the mesh"):
        make(small, outputInfo={"f": info(["bottom", "wing"], pRef)})
    with pytest.raises(DASError, match="DAScalarTransportFoam has no p"):
        make(scalar_transport_case(4, 4, 3), outputInfo={"f": info(["inlet"], pRef)})
    with pytest.raises(NotImplementedError, match="thermalCouplingOutput"):
        make(small, outputInfo={"q": {"type": "thermalCouplingOutput", "patches": ["bottom"], "components": ["thermalCoupling"]}})
