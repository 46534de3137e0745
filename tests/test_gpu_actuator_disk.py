"""The actuator disks of DASimpleFoam (the fvSource option, type actuatorDisk) and the fvSourcePar input on the device: the field and its
sums, the residual, the state Jacobians with the source in H, the parameter and the mesh products, updateOFMesh, the Newton primal and
adjoint total derivatives - against the numpy restatement (tests/actuator_disk_restatement.py) and its complex step.  Bars
(tests/README_heat_transfer.md): 1e-12 relative for values, 1e-10 for tangents and products, fields relative to their maximum; "bitwise"
is np.array_equal.  Notes and every measured number: tests/README_actuator_disk.md."""
import functools
import math

import numpy as np
import pytest

import actuator_disk_restatement as AD
from actuator_disk_cases import ALL_DISKS, DISK_A, DISK_B, DISK_C, MESHES, NAMES, NORM, disk_case, disks, geom, options
from dafoam_amd.meshgen import channel_case, simple_T_channel_case
from oracle import jacobian as J

pytestmark = pytest.mark.gpu

PAR_INPUTS = {"all_A": {"type": "fvSourcePar", "fvSourceName": "mid_A", "components": ["solver"]},
              "two_A": {"type": "fvSourcePar", "fvSourceName": "mid_A", "indices": [0, 7], "components": ["solver"]},
              "all_C": {"type": "fvSourcePar", "fvSourceName": "head_C", "components": ["solver"]},
              "x": {"type": "volCoord"}}
UNNORMALISED = {"normalizeResiduals": ["TRes"]}
TP = {"TP": {"type": "totalPressure", "source": "patchToFace", "patches": ["outlet"], "scale": 1.0}}


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=options(**extra), case=case)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def pars_of(name):
    e = ALL_DISKS[name]
    return np.array(list(e["center"]) + list(e["direction"]) + [e[k] for k in AD.PAR_NAMES[6:]], dtype=np.float64)


def blocks(g):
    N = g.nC
    return {"U": slice(0, 3 * N), "p": slice(3 * N, 4 * N), "nuTilda": slice(4 * N, 5 * N), "phi": slice(5 * N, None)}


def block_errors(R, ref, g):
    return {k: rel(R[sl], ref[sl]) for k, sl in blocks(g).items()}


@functools.lru_cache(maxsize=None)
def restated(mesh):
    """(case, geometry, disks, field, residual with the field) - computed once, shared, read-only"""
    case, g, S = disk_case(mesh), geom(mesh), disks(mesh)
    return case, g, S, np.real(S.field(g)), np.real(AD.residual(case, g, case.states, S))


# ---- the field ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_field_sums_and_repeatability(mesh):
    case, g, S, q, _ = restated(mesh)
    D = make(case, fvSource=dict(ALL_DISKS))
    a, b = D.solver.getFvSource(), D.solver.getFvSource()
    info = {n: D.solver.actuatorDiskInfo(n) for n in NAMES}
    print(mesh, "field", rel(a, q), {n: (info[n]["scale"], info[n]["thrustSourceSum"], info[n]["torqueSourceSum"]) for n in NAMES})
    assert a.shape == (g.nC, 3) and np.array_equal(a, b) and rel(a, q) <= 1e-12
    for n in NAMES:
        _, thrust, torque = S.entry(g, n)
        assert abs(info[n]["thrustSourceSum"] - thrust.real) <= 1e-13 * abs(thrust.real) and abs(info[n]["torqueSourceSum"] - torque.real) <= 1e-13 * abs(torque.real)
        assert abs(info[n]["scale"] - S.scale(g, n).real) <= 1e-13 * abs(S.scale(g, n).real)
    assert abs(info["head_C"]["thrustSourceSum"] - DISK_C["targetThrust"]) <= 1e-13 * DISK_C["targetThrust"]
    assert info["mid_A"]["scale"] == DISK_A["scale"] and info["tail_B"]["scale"] == DISK_B["scale"]
    if mesh == "box":  # 9 workgroups of partial sums: the two-stage sums against exactly rounded ones
        for n in NAMES:
            e = S.entries[n]
            with np.errstate(invalid="ignore"):  # the Hoekstra form outside B's set: not used
                _, fa, fc, _, _ = AD.disk_force(g.C, e["pars"].real, e["eps"], e["rotDir"], e["smooth"], scale=S.scale(g, n).real)
            keep = np.ones(g.nC, bool) if e["smooth"] else np.isin(np.arange(g.nC), e["cells"])
            thrust, torque = math.fsum((fa * g.V).real[keep]), math.fsum((fc * g.V).real[keep])
            assert abs(info[n]["thrustSourceSum"] - thrust) <= 1e-13 * abs(thrust) and abs(info[n]["torqueSourceSum"] - torque) <= 1e-13 * abs(torque)
        unit = math.fsum((AD.disk_force(g.C, S.entries["head_C"]["pars"].real, DISK_C["eps"], DISK_C["rotDir"], True, scale=1.0)[1] * g.V).real)
        assert abs(info["head_C"]["unitThrust"] - unit) <= 1e-13 * unit
    assert sorted(info["tail_B"]["cells"]) == sorted(S.entries["tail_B"]["cells"]) and info["mid_A"]["nCells"] == g.nC
    # the order of definition does not matter: the entries are walked by name
    D2 = make(case, fvSource={n: ALL_DISKS[n] for n in reversed(NAMES)})
    assert np.array_equal(D2.solver.getFvSource(), a)


def test_a_cell_centre_on_the_axis_is_refused_by_name():
    from dafoam_amd import _capi

    case = disk_case("flat")
    D = make(case)
    Cc = np.zeros(3 * case.mesh.n_cells)  # the library's own centres: the last bits decide
    _capi.check(_capi.lib().das_get_geometry(D.solver._h, None, None, _capi.dptr(Cc), None, None, None, None, None))
    with pytest.raises(_capi.DASError, match="fvSource.*axis"):
        make(case, fvSource={"on_axis": dict(DISK_A, center=[float(x) for x in Cc[3 * 77: 3 * 77 + 3]])})
    # a disk that was refused is not kept: the solver goes on without it
    L = _capi.lib()
    pars = np.array(list(Cc[3 * 77: 3 * 77 + 3]) + DISK_A["direction"] + [0.01, 0.08, 1.0, 0.7, 1.0, 0.5, 0.0])
    assert L.das_define_actuator_disk(D.solver._h, b"on_axis", b"cylinderAnnulusSmooth", _capi.dptr(pars), b"left", 0.02, 0) < 0
    assert "axis" in L.das_last_error().decode() and not D.solver.getFvSource().any()
    Ra, Rb = np.zeros(case.states.size), np.zeros(case.states.size)
    D.solver.getResiduals(Ra)
    make(case).solver.getResiduals(Rb)
    assert np.array_equal(Ra, Rb)
    # parameters that are refused when the field is computed are not kept, and a refused redefinition leaves the disk of that name alone
    D2 = make(case, fvSource={"a": DISK_A})
    f0, info0 = D2.solver.getFvSource(), D2.solver.actuatorDiskInfo("a")
    idx = np.arange(3, dtype=np.int32)
    assert L.das_set_actuator_disk_pars(D2.solver._h, b"a", idx.ctypes.data_as(_capi.c_int_p), 3, _capi.dptr(np.ascontiguousarray(Cc[3 * 77: 3 * 77 + 3]))) < 0
    assert "axis" in L.das_last_error().decode()
    assert np.array_equal(D2.solver.actuatorDiskInfo("a")["pars"], info0["pars"]) and np.array_equal(D2.solver.getFvSource(), f0)
    assert L.das_define_actuator_disk(D2.solver._h, b"a", b"cylinderAnnulusSmooth", _capi.dptr(pars), b"left", 0.02, 0) < 0
    assert np.array_equal(D2.solver.actuatorDiskInfo("a")["pars"], info0["pars"]) and np.array_equal(D2.solver.getFvSource(), f0)


def test_the_reference_docstring_example_constructs():
    """DAFvSourceActuatorDisk.C:58-89, the geometry scaled into the 1.0 x 0.2 x 0.1 channel, the keys as they stand there"""
    fv = {"disk1": {"type": "actuatorDisk", "source": "cylinderAnnulusToCell", "p1": [0.3, 0.1, 0.05], "p2": [0.5, 0.1, 0.05], "innerRadius": 0.01,
                    "outerRadius": 0.08, "rotDir": "left", "scale": 1.0, "POD": 0.7},
          "disk2": {"type": "actuatorDisk", "source": "cylinderAnnulusSmooth", "center": [0.6, 0.1, 0.05], "direction": [1.0, 0.0, 0.0], "innerRadius": 0.01,
                    "outerRadius": 0.08, "rotDir": "right", "scale": 0.1, "POD": 1.0, "eps": 0.02, "expM": 1.0, "expN": 0.5}}
    case, g = disk_case("bump"), geom("bump")
    D = make(case, fvSource=fv)
    assert rel(D.solver.getFvSource(), np.real(AD.Disks(g, fv).field(g))) <= 1e-12


# ---- the residual ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["flat", "bump", "mixed"])
def test_residual_with_disks_and_bitwise_without(mesh):
    case, g, S, q, Ro = restated(mesh)
    n = case.states.size
    D = make(case, fvSource=dict(ALL_DISKS))
    R, R2 = np.zeros(n), np.ones(n)
    D.solver.getResiduals(R)
    D.solver.calcResiduals(1, R2)
    errs = block_errors(R, Ro, g)
    print(mesh, "residual", errs)
    assert max(errs.values()) <= 1e-12
    RoPC = np.real(AD.residual(case, g, case.states, S, isPC=True, pc_blend=0.5))  # amd.pcUpwindBlend: 0.5 by default
    assert max(block_errors(R2, RoPC, g).values()) <= 1e-12
    Du = make(case, fvSource=dict(ALL_DISKS), **UNNORMALISED)
    Ru = np.zeros(n)
    Du.solver.getResiduals(Ru)
    errs = block_errors(Ru, np.real(AD.residual(case, g, case.states, S, normalize=("TRes",))), g)
    print(mesh, "not normalised", errs)
    assert max(errs.values()) <= 1e-12
    # no fvSource option, an empty one: the same bits
    Ra, Rb = np.zeros(n), np.zeros(n)
    make(case).solver.getResiduals(Ra)
    make(case, fvSource={}).solver.getResiduals(Rb)
    assert np.array_equal(Ra, Rb) and max(block_errors(Ra, np.real(AD.residual(case, g, case.states)), g).values()) <= 1e-12
    d = R - Ra
    sl = blocks(g)
    assert np.abs(d[sl["U"]]).max() > 1.0 and np.abs(d[sl["p"]]).max() > 1e-3 and np.abs(d[sl["phi"]]).max() > 1e-6


# ---- the state Jacobians see the source through H -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["bump", "mixed"])
def test_state_products_and_jacobian_entries_with_the_source_in_H(mesh):
    from dafoam_amd.pyDASolvers import Mat

    case, g, S, q, _ = restated(mesh)
    W = case.states
    n = W.size
    sc = J.state_scales(case, g, NORM)
    rng = np.random.default_rng(5)
    psi, v = rng.standard_normal(n), rng.standard_normal(n)
    D = make(case, fvSource=dict(ALL_DISKS), jacLowerBounds={"dRdW": 0.0, "dRdWPC": 0.0})
    D0 = make(case, jacLowerBounds={"dRdW": 0.0, "dRdWPC": 0.0})

    def column(j, srcs):  # s_j dR/dW_j
        Wc = W.astype(np.complex128)
        Wc[j] += 1e-30j * sc[j]
        return np.imag(AD.residual(case, g, Wc, srcs)) / 1e-30

    # forward: one complex step in the direction s o v
    fwd, fwd0 = np.zeros(n), np.zeros(n)
    D.solver.calcJacVecProduct(v, fwd)
    D0.solver.calcJacVecProduct(v, fwd0)
    ref = np.imag(AD.residual(case, g, W + 1e-30j * sc * v, S)) / 1e-30
    ref0 = np.imag(AD.residual(case, g, W + 1e-30j * sc * v)) / 1e-30
    errs = block_errors(fwd, ref, g)
    print(mesh, "dRdW v", errs, "the source's share", block_errors(ref0, ref, g))
    assert max(errs.values()) <= 1e-10
    # a kernel that drops the source from H, or a product without it, misses the bound by orders
    assert rel(fwd0, ref) > 1e-6 and rel(ref0[blocks(g)["p"]], ref[blocks(g)["p"]]) > 1e-6
    # transposed: the columns of the states of the cells where the source is largest (U, p, nuTilda) and of their faces (phi), and some more
    N = g.nC
    hot = np.argsort(-np.abs(q).max(1))[:3]
    faces = [int(np.nonzero(case.mesh.owner == c)[0][0]) for c in hot]
    cols = sorted(set([3 * c + k for c in hot for k in range(3)] + [3 * N + c for c in hot] + [4 * N + c for c in hot] + [5 * N + f for f in faces]
                      + list(rng.integers(0, n, 6))))
    prod, prod0 = np.zeros(n), np.zeros(n)
    D.solverAD.calcJacTVecProduct("states", "stateVar", W, "residuals", "residual", psi, prod)
    D0.solverAD.calcJacTVecProduct("states", "stateVar", W, "residuals", "residual", psi, prod0)
    D.solver.runColoring()
    M, Mp = Mat(), Mat()
    D.solver.calcdRdWT(0, M, mode=1)
    D.solver.calcdRdWT(1, Mp)  # the coloured finite differences of dRdWTPC see the field too
    A, Ap = M.to_scipy().tocsr(), Mp.to_scipy().tocsr()
    D0.solver.runColoring()
    Mp0 = Mat()
    D0.solver.calcdRdWT(1, Mp0)
    Ap0 = Mp0.to_scipy().tocsr()
    scale_p, scale_a = np.abs(prod).max(), np.abs(A.data).max()
    worst = dict(prod=0.0, entries=0.0, share=0.0, pc=0.0)
    for j in cols:
        cj, cj0 = column(j, S), column(j, None)
        worst["prod"] = max(worst["prod"], abs(prod[j] - psi @ cj) / scale_p)
        worst["entries"] = max(worst["entries"], np.abs(A[j].toarray().ravel() - cj).max() / scale_a)
        worst["share"] = max(worst["share"], np.abs(cj - cj0).max() / scale_a)
        worst["pc"] = max(worst["pc"], np.abs(Ap[j].toarray().ravel() - Ap0[j].toarray().ravel()).max() / scale_a)
    print(mesh, len(cols), "columns:", worst, "product moved by the source", rel(prod0, prod))
    assert worst["prod"] <= 1e-10 and worst["entries"] <= 1e-10
    assert worst["pc"] > 1e-6  # dRdWTPC (reduced stencil, blended upwind: no exact twin here) moves with the field as well
    assert worst["share"] > 1e-6 and rel(prod0, prod) > 1e-6


# ---- fvSourcePar ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("mesh", ["bump", "mixed"])
def test_fv_source_par_products(mesh, normalized):
    case, g, S, _, _ = restated(mesh)
    extra = {} if normalized else dict(UNNORMALISED)
    kw = {} if normalized else dict(normalize=("TRes",))
    D = make(case, fvSource=dict(ALL_DISKS), inputInfo=PAR_INPUTS, function=TP,
             outputInfo={"f": {"type": "forceCouplingOutput", "patches": ["bottom"], "pRef": 0.0, "components": ["forceCoupling"]}}, **extra)
    A = D.solverAD
    W = case.states
    psi = np.random.default_rng(7).standard_normal(W.size)

    def ref(name, idx, seeds):
        p0 = S.entries[name]["pars"]
        return np.array([np.imag(seeds @ AD.residual(case, g, W, S, pars={name: p0 + 1e-30j * np.eye(13)[i]}, **kw)) / 1e-30 for i in idx])

    pa, pab, p2 = np.zeros(13), np.ones(13), np.zeros(2)
    A.calcJacTVecProduct("all_A", "fvSourcePar", pars_of("mid_A"), "residuals", "residual", psi, pa)
    A.calcJacTVecProduct("all_A", "fvSourcePar", pars_of("mid_A"), "residuals", "residual", psi, pab)
    ra = ref("mid_A", range(13), psi)
    print(mesh, normalized, "A:", np.abs(pa - ra)[:12] / np.abs(ra)[:12])
    assert np.array_equal(pa, pab) and np.all(ra[:12] != 0) and np.all(np.abs(pa - ra)[:12] <= 1e-10 * np.abs(ra)[:12])
    assert pa[12] == 0.0 and ra[12] == 0.0  # targetThrust is not read without adjustThrust
    A.calcJacTVecProduct("two_A", "fvSourcePar", pars_of("mid_A")[[0, 7]], "residuals", "residual", psi, p2)
    assert np.array_equal(p2, pa[[0, 7]])
    pc = np.ones(13)
    A.calcJacTVecProduct("all_C", "fvSourcePar", pars_of("head_C"), "residuals", "residual", psi, pc)
    rc = ref("head_C", range(13), psi)
    live = [i for i in range(13) if i != 8]
    print(mesh, normalized, "C:", np.abs(pc - rc)[live] / np.abs(rc)[live])
    assert pc[8] == 0.0 and rc[8] == 0.0  # scale is not read with adjustThrust
    assert np.all(rc[live] != 0) and np.all(np.abs(pc - rc)[live] <= 1e-10 * np.abs(rc)[live])
    # seeds on the p and phi rows only: the path through rAU H that a tangent added to the U rows alone would miss
    sl = blocks(g)
    psi_pphi = np.zeros(W.size)
    psi_pphi[sl["p"]], psi_pphi[sl["phi"]] = psi[sl["p"]], psi[sl["phi"]]
    pp = np.zeros(13)
    A.calcJacTVecProduct("all_A", "fvSourcePar", pars_of("mid_A"), "residuals", "residual", psi_pphi, pp)
    rp = ref("mid_A", range(13), psi_pphi)
    print(mesh, normalized, "A, p and phi rows only:", pp[:12], np.abs(pp - rp)[:12] / np.abs(rp)[:12])
    assert np.all(pp[:12] != 0) and np.all(np.abs(pp - rp)[:12] <= 1e-10 * np.abs(rp)[:12])
    for name, typ, seeds in (("TP", "function", np.ones(1)), ("f", "forceCouplingOutput", np.ones(A.getOutputSize("f", "forceCouplingOutput")))):
        z = np.ones(13)
        A.calcJacTVecProduct("all_A", "fvSourcePar", pars_of("mid_A"), name, typ, seeds, z)
        assert np.all(z == 0.0)


def test_with_a_T_field_the_residual_the_products_and_exact_zeros_to_every_coupling_output():
    """DASimpleFoam with the optional T field (states [U | p | T | nuTilda | phi]) and A + B + C: the residual per block, fvSourcePar -> residual,
    and fvSourcePar -> function, forceCouplingOutput and thermalCouplingOutput, which read no source: exact zeros."""
    case = simple_T_channel_case(10, 8, 6)
    g = AD.FlowGeom(case.mesh)
    S = AD.Disks(g, ALL_DISKS)
    N, W = g.nC, case.states
    assert W.size == 6 * N + g.nF
    tb = {"U": slice(0, 3 * N), "p": slice(3 * N, 4 * N), "T": slice(4 * N, 5 * N), "nuTilda": slice(5 * N, 6 * N), "phi": slice(6 * N, None)}
    out = {"q": {"type": "thermalCouplingOutput", "patches": ["inlet", "bottom"], "components": ["thermalCoupling"]},
           "f": {"type": "forceCouplingOutput", "patches": ["bottom"], "pRef": 0.0, "components": ["forceCoupling"]}}
    D = make(case, fvSource=dict(ALL_DISKS), inputInfo=PAR_INPUTS, function=TP, outputInfo=out)
    R, R0 = np.zeros(W.size), np.zeros(W.size)
    D.solver.getResiduals(R)
    make(case).solver.getResiduals(R0)
    ref = np.real(AD.residual(case, g, W, S))
    errs = {k: rel(R[sl], ref[sl]) for k, sl in tb.items()}
    print("T field: residual", errs, "field", rel(D.solver.getFvSource(), np.real(S.field(g))))
    assert max(errs.values()) <= 1e-12 and rel(D.solver.getFvSource(), np.real(S.field(g))) <= 1e-12
    # the passive T equation and the SA equation read no source; the U, p and phi rows move
    assert np.array_equal(R[tb["T"]], R0[tb["T"]]) and np.array_equal(R[tb["nuTilda"]], R0[tb["nuTilda"]])
    assert np.abs(R - R0)[tb["U"]].max() > 1.0 and np.abs(R - R0)[tb["p"]].max() > 1e-3 and np.abs(R - R0)[tb["phi"]].max() > 1e-6
    A = D.solverAD
    psi = np.random.default_rng(7).standard_normal(W.size)
    for inp, name, dead in (("all_A", "mid_A", 12), ("all_C", "head_C", 8)):
        p0 = S.entries[name]["pars"]
        prod = np.ones(13)
        A.calcJacTVecProduct(inp, "fvSourcePar", pars_of(name), "residuals", "residual", psi, prod)
        r = np.array([np.imag(psi @ AD.residual(case, g, W, S, pars={name: p0 + 1e-30j * np.eye(13)[i]})) / 1e-30 for i in range(13)])
        live = [i for i in range(13) if i != dead]
        print("T field:", name, np.abs(prod - r)[live] / np.abs(r)[live])
        assert prod[dead] == 0.0 and r[dead] == 0.0 and np.all(r[live] != 0) and np.all(np.abs(prod - r)[live] <= 1e-10 * np.abs(r)[live])
        for oname, typ in (("TP", "function"), ("f", "forceCouplingOutput"), ("q", "thermalCouplingOutput")):
            n_out = 1 if typ == "function" else A.getOutputSize(oname, typ)
            assert n_out > 0
            z = np.ones(13)
            A.calcJacTVecProduct(inp, "fvSourcePar", pars_of(name), oname, typ, np.ones(n_out), z)
            assert np.all(z == 0.0), (name, typ)


def test_set_solver_input_moves_the_field_and_the_residual():
    case, g, S, q0, _ = restated("mixed")
    D = make(case, fvSource=dict(ALL_DISKS), inputInfo=PAR_INPUTS)
    new = pars_of("mid_A") * np.array([1.05, 0.9, 1.1, 1.0, 2.0, 0.5, 1.3, 0.9, 1.7, 1.2, 1.1, 0.8, 1.0])
    newC = pars_of("head_C") * np.array([1, 1, 1, 1, 1, 1, 1, 1, 3.0, 1, 1, 1, 2.0])
    D.set_solver_input({"all_A": new, "all_C": newC, "two_A": new[[0, 7]], "x": case.mesh.points.ravel()})
    qn = np.real(S.field(g, {"mid_A": new, "head_C": newC}))
    R = np.zeros(case.states.size)
    D.solver.getResiduals(R)
    f = D.solver.getFvSource()
    print("field", rel(f, qn), "moved by", rel(qn, q0))
    assert rel(f, qn) <= 1e-12 and rel(qn, q0) > 0.1
    assert max(block_errors(R, np.real(AD.residual(case, g, case.states, S, pars={"mid_A": new, "head_C": newC})), g).values()) <= 1e-12
    assert np.array_equal(D.solver.actuatorDiskInfo("mid_A")["pars"], new)
    assert abs(D.solver.actuatorDiskInfo("head_C")["thrustSourceSum"] - 2.0 * DISK_C["targetThrust"]) <= 1e-13
    D.solver.setSolverInput("two_A", "fvSourcePar", 2, pars_of("mid_A")[[0, 7]])
    assert np.array_equal(D.solver.actuatorDiskInfo("mid_A")["pars"][[0, 7]], pars_of("mid_A")[[0, 7]])


def test_update_of_mesh_moves_the_field_keeps_the_set_and_rescales():
    case, g, S, q0, _ = restated("mixed")
    D = make(case, fvSource=dict(ALL_DISKS))
    m = case.mesh
    rng = np.random.default_rng(4)
    X = m.points + 0.004 * rng.standard_normal(m.points.shape) * np.array([1.0, 0.2, 0.1])
    before = {n: D.solver.actuatorDiskInfo(n) for n in NAMES}
    D.solver.updateOFMesh(np.ascontiguousarray(X.ravel()))
    g2 = AD.FlowGeom(m, X)
    q2 = np.real(S.field(g2))  # the cell set of the first mesh, the metrics of the second
    after = {n: D.solver.actuatorDiskInfo(n) for n in NAMES}
    f = D.solver.getFvSource()
    print("moved field", rel(f, q2), "moved by", rel(q2, q0), "scale of C", before["head_C"]["scale"], "->", after["head_C"]["scale"])
    assert rel(f, q2) <= 1e-12 and rel(q2, q0) > 1e-3
    assert np.array_equal(before["tail_B"]["cells"], after["tail_B"]["cells"])
    assert before["head_C"]["scale"] != after["head_C"]["scale"] and abs(after["head_C"]["scale"] - S.scale(g2, "head_C").real) <= 1e-13 * after["head_C"]["scale"]
    assert abs(after["head_C"]["thrustSourceSum"] - DISK_C["targetThrust"]) <= 1e-13 * DISK_C["targetThrust"]
    R = np.zeros(case.states.size)
    D.solver.getResiduals(R)
    case2 = disk_case("mixed")
    # the wall distance of the case is data of the case: the residual at the new metrics with it
    assert max(block_errors(R, np.real(AD.residual(case2, g2, case.states, S)), g).values()) <= 1e-12


# ---- volCoord ---------------------------------------------------------------------------------------------------------------------------
def sample_points(case, g, S, off_symmetry=False):
    """an interior, a patch and a corner point, a point inside each disk (of the cell where it is strongest) and the far corner.
    off_symmetry: no point of a symmetry patch (tests/actuator_disk_cases.py says why) - that drops the corners, which lie on them"""
    m = case.mesh
    by = {p.name: p for p in m.patches}
    on = lambda names: set(int(q) for nm in names for f in range(by[nm].start, by[nm].start + by[nm].size) for q in m.face_pts[m.face_ptr[f]:m.face_ptr[f + 1]])
    if off_symmetry:
        sym = on([p.name for p in m.patches if p.type == "symmetry"])
        assert sym
        pts = {"patch": sorted(on(["bottom"]) - sym)[5], "top": sorted(on(["top"]) - sym)[-3]}
        boundary = on([p.name for p in m.patches])
        pts["interior"] = next(p for p in range(m.n_points // 2, m.n_points) if p not in boundary)
        for n in NAMES:
            cell = int(np.argmax(np.abs(np.real(S.entry(g, n)[0])).max(1)))
            pts["in_" + n] = next(int(q) for f in np.nonzero(m.owner == cell)[0] for q in m.face_pts[m.face_ptr[f]:m.face_ptr[f + 1]] if int(q) not in sym)
        return pts
    pts = {"corner": 0, "patch": int(m.face_pts[m.face_ptr[by["bottom"].start + 5]]), "far": int(np.argmax(m.points @ np.array([1.0, -1.0, -1.0])))}
    boundary = set(int(p) for f in range(m.n_internal_faces, m.n_faces) for p in m.face_pts[m.face_ptr[f]:m.face_ptr[f + 1]])
    pts["interior"] = next(p for p in range(m.n_points // 2, m.n_points) if p not in boundary)
    for n in NAMES:
        cell = int(np.argmax(np.abs(np.real(S.entry(g, n)[0])).max(1)))
        pts["in_" + n] = int(m.face_pts[m.face_ptr[int(np.nonzero(m.owner == cell)[0][0])]])
    return pts


def volcoord_reference(case, g, S, psi, idx, srcs=True, frozen=None, **kw):
    X0 = case.mesh.points.ravel()
    out = []
    for j in idx:
        X = X0.astype(np.complex128)
        X[j] += 1e-30j
        gg = AD.FlowGeom(case.mesh, X.reshape(-1, 3))
        out.append(np.imag(psi @ AD.residual(case, gg, case.states.astype(np.complex128), S if srcs else None, frozen=frozen, **kw)) / 1e-30)
    return np.array(out)


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("mesh", ["bump_walls", "mixed_walls", "bump"])
def test_vol_coord_product_with_disks(mesh, normalized):
    case, g, S, _, _ = restated(mesh)
    extra = {} if normalized else dict(UNNORMALISED)
    kw = {} if normalized else dict(normalize=("TRes",))
    psi = np.random.default_rng(9).standard_normal(case.states.size)
    X0 = case.mesh.points.ravel().copy()
    pts = sample_points(case, g, S, off_symmetry=mesh == "bump")  # bump: the issue's mesh, at points off its symmetry planes
    idx = [3 * p + k for p in pts.values() for k in range(3)]
    ref, ref0, ref_local = (volcoord_reference(case, g, S, psi, idx, **kw), volcoord_reference(case, g, S, psi, idx, srcs=False, **kw),
                            volcoord_reference(case, g, S, psi, idx, frozen=g, **kw))
    D = make(case, fvSource=dict(ALL_DISKS), inputInfo=PAR_INPUTS, **extra)
    prod, prod2 = np.zeros(X0.size), np.ones(X0.size)
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod)
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod2)
    scale = np.abs(prod).max()
    err = np.abs(prod[idx] - ref).reshape(-1, 3).max(1) / scale
    print(mesh, normalized, "volCoord:", dict(zip(pts, err)), "the disks' share:", dict(zip(pts, np.abs(ref - ref0).reshape(-1, 3).max(1) / scale)))
    assert np.array_equal(prod, prod2) and np.abs(prod[idx] - ref).max() <= 1e-10 * scale
    # what a point does to the rows it cannot reach - through the adjustThrust total of C - is in the reference and not in a pass with the
    # total frozen: a product without the rank-one term cannot meet the bar at the points inside C
    gap = np.abs(ref - ref_local).reshape(-1, 3).max(1) / scale
    print("  of which through the total of C:", dict(zip(pts, gap)))
    assert gap[list(pts).index("in_head_C")] > 1e-8
    # the field is what it was
    assert rel(D.solver.getFvSource(), np.real(S.field(g))) <= 1e-12


def test_vol_coord_product_in_difference_mode():
    """amd.volCoordMode fd against the complex step of the restatement, at the bar of the difference mode (tests/README_heat_source.md: 95 %
    of the entries within 1e-4 of the largest, all within 5e-2)."""
    case, g, S, _, _ = restated("bump_walls")
    psi = np.random.default_rng(9).standard_normal(case.states.size)
    X0 = case.mesh.points.ravel().copy()
    pts = sample_points(case, g, S)
    idx = [3 * p + k for p in pts.values() for k in range(3)]
    ref = volcoord_reference(case, g, S, psi, idx)
    D = make(case, fvSource=dict(ALL_DISKS), inputInfo=PAR_INPUTS, amd={"volCoordMode": "fd"})
    prod = np.zeros(X0.size)
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod)
    err = np.abs(prod[idx] - ref) / np.abs(prod).max()
    print("fd mode:", dict(zip(pts, err.reshape(-1, 3).max(1))))
    assert np.percentile(err, 95) <= 1e-4 and err.max() <= 5e-2
    assert rel(D.solver.getFvSource(), np.real(S.field(g))) <= 1e-12


# ---- the primal and the adjoint totals --------------------------------------------------------------------------------------------------
AB = {"a": DISK_A, "b": DISK_B}


@functools.lru_cache(maxsize=None)
def primal_case():
    """the channel of the Newton-Krylov primal test (tests/test_gpu_parity.py) at 8 x 6 x 5"""
    return channel_case(8, 6, 5, perturb=0.0)


def test_newton_primal_with_disks_converges_to_a_zero_of_the_restatement():
    from dafoam_amd._capi import DASError

    case = primal_case()
    g = AD.FlowGeom(case.mesh)
    S = AD.Disks(g, AB)
    D = make(case, fvSource=dict(AB))
    R0 = np.zeros(case.states.size)
    D.solver.getResiduals(R0)
    fail, info = D.solver.solvePrimal(maxSteps=80, relTol=1e-10)
    W = D.getStates()
    res = np.linalg.norm(np.real(AD.residual(case, g, W, S))) / np.linalg.norm(R0)
    res_without = np.linalg.norm(np.real(AD.residual(case, g, W))) / np.linalg.norm(R0)
    print("primal:", info["steps"], "steps,", info["res"] / info["res0"], "restatement with the disks", res, "without", res_without)
    assert fail == 0 and info["res"] <= 1e-10 * info["res0"]
    assert res <= 1e-9 and res_without > 1e-4
    with pytest.raises(DASError, match="das_simple_iteration.*fvSource"):
        D.solver.simpleIteration(1)


def sweep(value, p0, i, f0):
    """central difference in parameter i at the relative step where the two one-sided differences agree best; (fd, 10 x disagreement, step)"""
    best = None
    for h in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6):
        dp = np.zeros(p0.size)
        dp[i] = h * p0[i]
        up, dn = (value(p0 + dp) - f0) / dp[i], (f0 - value(p0 - dp)) / dp[i]
        print("   parameter", i, "step", h, "one-sided", up, dn)
        if best is None or abs(up - dn) < best[0]:
            best = (abs(up - dn), 0.5 * (up + dn), h)
    return best[1], 10.0 * best[0], best[2]


TOTALS = {"A-scale": ("mid_A", 8), "A-center_x": ("mid_A", 0), "A-outerRadius": ("mid_A", 7), "A-POD": ("mid_A", 9), "C-targetThrust": ("head_C", 12)}


@pytest.mark.parametrize("which", list(TOTALS))
def test_adjoint_total_derivative_of_the_total_pressure_in_a_disk_parameter(which):
    """dTP(outlet) / d(scale, center_x, outerRadius, POD) of A and d / d(targetThrust) of C: -psi^T dR/dp with psi from solveAdjoint at
    gmresRelTol 1e-12, against central differences of solvePrimal + calcFunction.  The step is the one at which the two one-sided
    differences agree best, the bound ten times their disagreement (the rule of tests/README_heat_source.md).  One parameter per case:
    each sweep is twelve primal solutions."""
    case = primal_case()
    disk, index = TOTALS[which]
    fv = {"d": ALL_DISKS[disk], "b": DISK_B}
    inputs = {"p": {"type": "fvSourcePar", "fvSourceName": "d", "indices": [index], "components": ["solver"]}}
    D = make(case, fvSource=fv, function=TP, inputInfo=inputs, adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0})
    p0 = pars_of(disk)[[index]]

    def value(p):
        D.solver.setSolverInput("p", "fvSourcePar", 1, np.ascontiguousarray(p))
        fail, info = D.solver.solvePrimal(maxSteps=80, relTol=0.0, absTol=tol)
        assert fail == 0, info
        return D.solver.calcFunction("TP")

    R0 = np.zeros(case.states.size)
    D.solver.getResiduals(R0)
    tol = 1e-12 * np.linalg.norm(R0)
    f0 = value(p0)
    fd, bound, step = sweep(value, p0, 0, f0)
    assert abs(value(p0) - f0) <= 1e-11 * abs(f0)
    W = D.getStates()
    rhs = np.zeros(W.size)
    D.solverAD.calcJacTVecProduct("states", "stateVar", W, "TP", "function", np.ones(1), rhs)
    psi, fail = D.solveAdjoint(rhs)
    prod = np.zeros(1)
    D.solverAD.calcJacTVecProduct("p", "fvSourcePar", p0, "residuals", "residual", psi, prod)
    total = -prod[0]
    print(which, "adjoint total", total, "central differences", fd, "relative step", step, "bound", bound, "difference", abs(total - fd))
    assert fail == 0 and fd != 0 and abs(total - fd) <= bound
