"""meshQualityKS and residualNorm on the device: values, bit-repeatability, moved points, the KS reduction over many workgroups, the volCoord
products and the products from the other inputs, the refusals - against the numpy restatement (tests/mesh_quality_restatement.py) and the
oracle's residual.  On the commit before these functions the solver construction raises NotImplementedError, so every test here fails there."""
import copy
import ctypes as C

import numpy as np
import pytest

import mesh_quality_restatement as MQ
from common import blocks, norm_states, options
from dafoam_amd import _capi
from dafoam_amd._capi import DASError
from dafoam_amd.meshgen import BC_FIXED_VALUE, channel_case, periodic_channel_case, rho_channel_case
from mixed_mesh import MIXED
from oracle import jacobian as J
from oracle.foam_mesh import Geometry
from oracle.residual import residual

pytestmark = pytest.mark.gpu

# reference tests/runRegTests_AeroOpt.py (skewness, nonOrtho) and runUnitTests_DAFunction.py (the third metric), but for the names
MQ_FNS = {
    "skewness": {"type": "meshQualityKS", "source": "allCells", "coeffKS": 10.0, "metric": "faceSkewness", "scale": 1.0},
    "nonOrtho": {"type": "meshQualityKS", "source": "allCells", "coeffKS": 1.0, "metric": "nonOrthoAngle", "scale": 1.0},
    "ortho": {"type": "meshQualityKS", "source": "allCells", "coeffKS": 10.0, "metric": "faceOrthogonality", "scale": 1.0, "includeProcPatches": 1},
}
MQ_MORE = {
    "skewnessScaled": dict(MQ_FNS["skewness"], scale=2.0),
    "skewnessRef": dict(MQ_FNS["skewness"], calcRefVar=1, ref=[0.4]),
}
CASES = {"channel": channel_case(6, 5, 4), "mixed": MIXED}
# reference tests/runUnitTests_DAFunction.py: ResNorm (L2Norm) and ResNorm1 (L1Norm) pass TRes to a case without T
RES_WEIGHT = {"URes": 2.0, "pRes": 3.0, "nuTildaRes": 0.5, "phiRes": 1.5, "TRes": 0.25}
RN_FNS = {
    "ResNorm": {"type": "residualNorm", "source": "allCells", "resWeight": RES_WEIGHT, "resMode": "L2Norm", "scale": 1.0},
    "ResNorm1": {"type": "residualNorm", "source": "allCells", "resWeight": RES_WEIGHT, "resMode": "L1Norm", "scale": 1.0},
    "ResNormRef": {"type": "residualNorm", "source": "allCells", "resWeight": RES_WEIGHT, "calcRefVar": 1, "ref": [10.0], "scale": 3.0},
}


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=options(case, **extra), case=case)


def moved_case(case, X):
    c = copy.copy(case)
    c.mesh = copy.deepcopy(case.mesh)
    c.mesh.points = np.asarray(X, dtype=np.float64).reshape(-1, 3).copy()
    return c


def close(a, b, tol):
    return abs(a - b) <= tol * abs(b)


# ---- meshQualityKS: values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_mesh_quality_values_repeat_and_follow_the_points(name):
    case = CASES[name]
    fns = dict(MQ_FNS, **MQ_MORE)
    D = make(case, function=fns)
    for X in (None, MQ.jitter(case.mesh, 7)):
        if X is not None:
            D.setVolCoords(X.ravel())  # the value follows the moved points
        for fname, fd in fns.items():
            F1, F2 = D.solver.calcFunction(fname), D.solver.calcFunction(fname)
            Fo = MQ.mesh_quality_ks(case.mesh, fd, X)
            print(f"{name} {fname} moved={X is not None}: device {F1!r} restated {Fo!r} rel {abs(F1 - Fo) / abs(Fo):.2e}")
            assert F1 == F2, fname  # the same bits on every call
            assert close(F1, Fo, 1e-12), (fname, F1, Fo)
        assert D.solver.calcFunction("skewnessScaled") == D.solver.calcFunction("skewness")  # scale is read and not applied
        F0 = D.solver.calcFunction("skewness")
        assert close(D.solver.calcFunction("skewnessRef"), (F0 - 0.4) ** 2, 1e-12)


def test_mesh_quality_ks_over_many_workgroups():
    """20 x 20 x 8: 10 160 faces, 40 workgroups of partials, against the exactly rounded sum (math.fsum)"""
    case = channel_case(20, 20, 8)
    assert case.mesh.n_faces > 10000
    D = make(case, function=MQ_FNS)
    for fname, fd in MQ_FNS.items():
        F1, F2 = D.solver.calcFunction(fname), D.solver.calcFunction(fname)
        Fo = MQ.mesh_quality_ks(case.mesh, fd)
        print(f"{fname}: device {F1!r} fsum {Fo!r} rel {abs(F1 - Fo) / abs(Fo):.2e}")
        assert F1 == F2 and close(F1, Fo, 1e-13), (fname, F1, Fo)


# ---- meshQualityKS: products ----------------------------------------------------------------------------------------------------------------
def check_jitter(g):
    """what the tangent comparisons need, asserted from the restatement before anything is compared: positive volumes, no clamped internal
    face, no tie in the point maximum of fd, no |sv| = 0"""
    _, sv_over_d, gap = MQ.face_skewness(g, details=True)
    assert g.V.min() > 0 and not MQ.clamped(g)[: g.nIF].any()
    assert gap.min() >= 1e-6 and sv_over_d.min() >= 1e-5, (gap.min(), sv_over_d.min())


@pytest.mark.parametrize("seed", [7, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_mesh_quality_volcoord_product(name, seed):
    """The full product over all points, on the jittered mesh (set through setVolCoords: the solver is constructed on the original one),
    against the restatement's complex step on a seeded subset of 60 entries plus every coordinate of the points of the face with the
    largest metric, at 1e-10 of the largest entry."""
    case = CASES[name]
    X = MQ.jitter(case.mesh, seed)
    g = MQ.MeshGeometry(case.mesh, X)
    check_jitter(g)
    fns = dict(MQ_FNS, skewnessRef=MQ_MORE["skewnessRef"])
    D = make(case, function=fns, inputInfo={"x": {"type": "volCoord"}})
    D.setVolCoords(X.ravel())
    S = D.solverAD
    rng = np.random.default_rng(seed)
    for fname, fd in fns.items():
        prod = np.zeros(X.size)
        S.calcJacTVecProduct("x", "volCoord", X.ravel(), fname, "function", np.array([1.5]), prod)
        fmax = int(np.argmax(MQ.metric_values(g, fd["metric"])))
        pts = case.mesh.face_pts[case.mesh.face_ptr[fmax] : case.mesh.face_ptr[fmax + 1]]
        idx = np.unique(np.concatenate([rng.choice(X.size, 60, replace=False), (3 * np.asarray(pts)[:, None] + np.arange(3)).ravel()]))
        ref = np.zeros(idx.size)
        for k, j in enumerate(idx):
            Xc = X.ravel().astype(np.complex128)
            Xc[j] += 1e-30j
            ref[k] = 1.5 * MQ.mesh_quality_ks(case.mesh, fd, Xc).imag / 1e-30
        err = np.abs(prod[idx] - ref).max() / np.abs(ref).max()
        print(f"{name} seed {seed} {fname}: {idx.size} entries, largest of them {np.abs(ref).max():.3e} (of the product {np.abs(prod).max():.3e}), error {err:.2e}")
        assert np.abs(ref).max() > 0 and err <= 1e-10, fname


def test_mesh_quality_products_from_other_inputs_are_exact_zeros():
    case = CASES["channel"]
    info = {"pOut": {"type": "patchVar", "patches": ["outlet"], "varName": "p", "varType": "scalar"},
            "pv": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "y"},
            "beta": {"type": "field", "fieldName": "betaFINuTilda", "fieldType": "scalar"}}
    D = make(case, function=MQ_FNS, inputInfo=info)
    S = D.solverAD
    N = case.mesh.n_cells
    for fname in MQ_FNS:
        dF = np.ones(case.states.size)
        S.calcJacTVecProduct("states", "stateVar", case.states, fname, "function", np.array([1.5]), dF)
        assert np.all(dF == 0.0), fname
        out = np.ones(1)
        S.calcJacTVecProduct("pOut", "patchVar", np.array([0.3]), fname, "function", np.ones(1), out)
        assert np.all(out == 0.0), fname
        out = np.ones(2)
        S.calcJacTVecProduct("pv", "patchVelocity", np.array([10.0, 3.0]), fname, "function", np.ones(1), out)
        assert np.all(out == 0.0), fname
        prod = np.ones(N)
        S.calcJacTVecProduct("beta", "field", np.ones(N), fname, "function", np.ones(1), prod)
        assert np.all(prod == 0.0), fname


# ---- residualNorm ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["simple", "rho"])
def rn(request):
    """one solver per case with the three functions, and the oracle's pieces computed once: residual, rows, the complex-step dRdW^T"""
    case = (channel_case if request.param == "simple" else rho_channel_case)(6, 5, 4)
    g = Geometry(case.mesh)
    bl = blocks(case, g)
    info = {"x": {"type": "volCoord"}, "pv": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "y"}}
    D = make(case, function=RN_FNS, inputInfo=info)
    W = case.states
    sc = J.state_scales(case, g, norm_states(case))
    con = J.connectivity(case, g)
    col, _ = J.greedy_coloring(con)
    A = J.jacobian_colored(case, g, W, con, col, sc, mode="cs", lower_bound=0)  # rows: states, entry s_j dR_i/dW_j
    w, iphi = MQ.residual_rows(bl, RES_WEIGHT, g.nIF)
    # The seeds of L1Norm are |w| sign(R).  On the rows whose residual is rounding residue (phiRes of a symmetry plane: U_b . Sf with U_b the
    # tangential part of U) the sign is that of the residue, which no two implementations share - the restated seed RULE is applied to
    # the residual the library returns, once that is shown to be the oracle's (1e-12 of the largest).
    R = residual(case, g, W)
    Rdev = np.zeros(W.size)
    D.solver.getResiduals(Rdev)
    assert np.abs(Rdev - R).max() <= 1e-12 * np.abs(R).max()
    return dict(case=case, g=g, bl=bl, D=D, W=W, A=A, R=R, Rdev=Rdev, w=w, iphi=iphi)


def test_residual_norm_values(rn):
    for fname, fd in RN_FNS.items():
        F1, F2 = rn["D"].solver.calcFunction(fname), rn["D"].solver.calcFunction(fname)
        Fo = MQ.residual_norm_of(rn["R"], rn["w"], rn["iphi"], fd)
        print(f"{rn['case'].solver_name} {fname}: device {F1!r} restated {Fo!r} rel {abs(F1 - Fo) / abs(Fo):.2e}")
        assert F1 == F2 and close(F1, Fo, 1e-12), (fname, F1, Fo)
    if rn["case"].solver_name == "DARhoSimpleFoam":  # TRes counts where there is a T
        assert not close(MQ.residual_norm_of(rn["R"], *MQ.residual_rows(rn["bl"], dict(RES_WEIGHT, TRes=0.0), rn["g"].nIF), RN_FNS["ResNorm"]),
                         rn["D"].solver.calcFunction("ResNorm"), 1e-6)


def test_residual_norm_state_product(rn):
    """dRdW^T g with the restated seeds g = seed dF/dR, from the oracle's coloured complex step"""
    for fname, fd in RN_FNS.items():
        prod = np.zeros(rn["W"].size)
        rn["D"].solverAD.calcJacTVecProduct("states", "stateVar", rn["W"], fname, "function", np.array([1.5]), prod)
        ref = rn["A"] @ MQ.residual_norm_seeds(rn["Rdev"], rn["w"], rn["iphi"], fd, seed=1.5)
        err = np.abs(prod - ref).max() / np.abs(ref).max()
        print(f"{rn['case'].solver_name} {fname}: dFdW error relative to the largest {err:.2e}")
        assert err <= 1e-10, fname


def test_residual_norm_volcoord_product(rn):
    """equal to the volCoord -> residual product with the restated seeds (1e-12); its contraction with two seeded displacements against
    central differences of the restatement on moved meshes (1e-5).  The displacements keep the points of the symmetry planes (front / back,
    z = const) in their plane: the symmetry patch field has a kink in the plane normal at n = (0, 0, 1) (|n_k|), so along a direction that
    tilts the plane the one-sided derivatives of the residual differ, by 2e-4 of this product here, and no difference quotient is the derivative."""
    case, g, S = rn["case"], rn["g"], rn["D"].solverAD
    X0 = case.mesh.points.ravel().copy()
    rng = np.random.default_rng(11)
    h = 1e-6 * np.abs(X0).max()
    mesh = case.mesh
    sym = np.unique(np.concatenate([mesh.face_pts[mesh.face_ptr[f] : mesh.face_ptr[f + 1]] for p in mesh.patches if p.type == "symmetry"
                                    for f in range(p.start, p.start + p.size)]))
    for fname, fd in RN_FNS.items():
        prod, via = np.zeros(X0.size), np.zeros(X0.size)
        S.calcJacTVecProduct("x", "volCoord", X0, fname, "function", np.array([1.5]), prod)
        S.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", MQ.residual_norm_seeds(rn["Rdev"], rn["w"], rn["iphi"], fd, seed=1.5), via)
        err = np.abs(prod - via).max() / np.abs(via).max()
        print(f"{case.solver_name} {fname}: against the residual product with restated seeds {err:.2e}")
        assert err <= 1e-12, fname
        for _ in range(2):
            dX = rng.standard_normal(X0.size)
            dX.reshape(-1, 3)[sym, 2] = 0.0
            vals = []
            for sgn in (1.0, -1.0):
                c = moved_case(case, X0 + sgn * h * dX)
                vals.append(MQ.residual_norm(c, Geometry(c.mesh), rn["W"], fd, rn["bl"]))
            cd = 1.5 * (vals[0] - vals[1]) / (2 * h)
            print(f"{case.solver_name} {fname}: product . dX {prod @ dX!r} central difference {cd!r}")
            assert cd != 0.0 and abs(prod @ dX - cd) <= 1e-5 * abs(cd), fname


def test_residual_norm_patch_velocity_product():
    """d/d(UMag, AoA) of the inlet velocity on DASimpleFoam against central differences of the restatement (1e-6)"""
    case = channel_case(6, 5, 4)
    g = Geometry(case.mesh)
    bl = blocks(case, g)
    D = make(case, function=RN_FNS, inputInfo={"pv": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "y"}})
    x = np.array([10.0, 3.0])

    def restated(xv, fd):
        c = copy.copy(case)
        c.bcs = copy.deepcopy(case.bcs)
        a = np.deg2rad(xv[1])
        c.bcs["inlet"]["U"] = (BC_FIXED_VALUE, (xv[0] * np.cos(a), xv[0] * np.sin(a), 0.0))
        return MQ.residual_norm(c, g, case.states, fd, bl)

    for fname, fd in RN_FNS.items():
        out = np.zeros(2)
        D.solverAD.calcJacTVecProduct("pv", "patchVelocity", x, fname, "function", np.ones(1), out)
        for k in range(2):
            e = np.zeros(2)
            e[k] = 1e-4
            cd = (restated(x + e, fd) - restated(x - e, fd)) / 2e-4
            print(f"{fname}: d/dx[{k}] {out[k]!r} central difference {cd!r}")
            assert cd != 0.0 and abs(out[k] - cd) <= 1e-6 * abs(cd), (fname, k)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_problem():
    plain = channel_case(4, 4, 3)
    sk, rnf = MQ_FNS["skewness"], RN_FNS["ResNorm"]
    cases = [
        (plain, {"function": {"F": dict(sk, metric="aspectRatio")}}, "metric not valid! Options: faceOrthogonality, nonOrthoAngle, or faceSkewness"),
        (plain, {"function": {"F": {k: v for k, v in sk.items() if k != "coeffKS"}}}, "meshQualityKS needs coeffKS"),
        (plain, {"function": {"F": {k: v for k, v in sk.items() if k != "metric"}}}, "meshQualityKS needs metric"),
        (periodic_channel_case(4, 4, 3), {"function": {"F": sk}}, "cyclic patches"),
        (plain, {"function": {"F": dict(rnf, resMode="LInfNorm")}}, "resMode not supported"),
        (plain, {"function": {"F": dict(rnf, resWeight={k: v for k, v in RES_WEIGHT.items() if k != "pRes"})}}, "resWeight has no entry for pRes"),
        (rho_channel_case(4, 4, 3), {"function": {"F": dict(rnf, resWeight={k: v for k, v in RES_WEIGHT.items() if k != "TRes"})}},
         "resWeight has no entry for TRes"),
        (plain, {"function": {"F": {k: v for k, v in rnf.items() if k != "resWeight"}}}, "residualNorm needs the dictionary resWeight"),
    ]
    for case, extra, msg in cases:
        with pytest.raises(DASError, match=msg):
            make(case, **extra)
    with pytest.raises(NotImplementedError):
        make(plain, function={"F": {"type": "fieldMax", "varName": "p"}})
    # the difference mode of the volCoord product is refused by name; a zero L2Norm has no derivative
    zero = dict(rnf, resWeight={k: 0.0 for k in RES_WEIGHT})
    D = make(plain, function={"sk": sk, "zero": zero}, inputInfo={"x": {"type": "volCoord"}}, amd={"volCoordMode": "fd"})
    X0 = plain.mesh.points.ravel().copy()
    with pytest.raises(DASError, match="meshQualityKS function sk needs amd.volCoordMode dual"):
        D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "sk", "function", np.ones(1), np.zeros(X0.size))
    assert D.solver.calcFunction("zero") == 0.0
    with pytest.raises(DASError, match="residualNorm function zero: the L2Norm is zero"):
        D.solverAD.calcJacTVecProduct("states", "stateVar", plain.states, "zero", "function", np.ones(1), np.zeros(plain.states.size))
    # a sharded solver: the owned-cell mask is set after the construction, so the function says so when it is used
    mask = np.ones(plain.states.size, dtype=np.uint8)
    _capi.check(_capi.lib().das_set_owned_mask(D.solver._h, mask.ctypes.data_as(C.POINTER(C.c_ubyte))))
    for fname, ftype in (("sk", "meshQualityKS"), ("zero", "residualNorm")):
        with pytest.raises(DASError, match=f"{ftype} function {fname} runs on an undecomposed solver"):
            D.solver.calcFunction(fname)
